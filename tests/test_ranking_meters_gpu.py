"""The ranking meters and their entry points on MI355X (src/ranking.py over kernels.rank_table).

* AucTable on [B, V, K, C] logits, B = 97, n = 2 repeats, fed in two uneven batches and (K = 1) in both
  layouts, against sklearn's roc_auc_score on the fp64 softmax-mean of the same f32 logits, <= 1e-12:
  C = 2 with K in {1, 3}, C = 5 with positive_class = 3.  Condition on the data, asserted by the builder:
  per column, neighbouring fp64 scores differ by a relative 1e-4 at least, or belong to samples
  duplicated whole (7 of the 97) -- the f32 softmax (a few 1e-7) cannot reorder the former, the latter tie
  exactly, so the f32 ranks are the fp64 ranks and the AUC is the same exact rational.
* selective() on a decompose meter's per_sample() at S = 200 against tests/ranking_ref.py and against
  uncertainty.auroc, on the f32 scores the kernel ranks, <= 1e-12 (the bar of test_ranking_host.py).
* --auc_table, --auc_from (1 and 3 files) and --selective once each on --synthetic data: strict JSON, the
  keys as specified, the figures those of the Python call on the saved .npy files.
* RelianceCallback(auc=True) logs five finite columns; auc=False leaves columns() and the logs alone.
"""
import json
import os

import numpy as np
import pytest
import torch
from sklearn.metrics import roc_auc_score

import ranking_ref as R

pytestmark = pytest.mark.gpu
BAR = 1e-12
MIN_GAP = 1e-4
SYMBOL = "mmu_rank_table"
AUC_KEYS = ["full", "image", "text", "image_control", "text_control"]


@pytest.fixture(scope="module", autouse=True)
def deterministic_convs():
    """the tests compare separate runs, so MIOpen is pinned to its deterministic solvers (see
    test_uncertainty_gpu.py's fixture of the same name)"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def strict_load(path):
    def strict(c):
        raise AssertionError(f"not strict JSON: {c}")
    return json.loads(open(path).read(), parse_constant=strict)


def flat_aucs(block):
    return [block["full"], block["image"], block["text"]] + block["image_control"]["values"] + \
        block["text_control"]["values"]


def check_block_shape(block, n):
    assert list(block) == AUC_KEYS
    for k in ("image_control", "text_control"):
        assert list(block[k]) == ["mean", "std", "values"] and len(block[k]["values"]) == n


def prob64(z, positive_class):
    """fp64 mean_k softmax of the f32 logits [S, V, K, C] -> [S, V]"""
    return R.softmax64(z)[..., positive_class].mean(axis=2)


def separated(p, dup_of=None):
    """per column: neighbours in sorted order are >= MIN_GAP apart relatively, or whole duplicates"""
    order = np.argsort(p, axis=0, kind="stable")
    srt = np.take_along_axis(p, order, axis=0)
    ok = (srt[1:] - srt[:-1]) >= MIN_GAP * np.abs(srt[1:])
    if dup_of is not None:
        a, b = dup_of[order[1:]], dup_of[order[:-1]]
        ok |= (a == b) & (srt[1:] == srt[:-1])
    return bool(ok.all())


def make_logits(B, V, Kp, C, positive_class, seed, n_dup=7):
    """f32 logits [B, V, Kp, C], the last n_dup samples whole duplicates of the first n_dup, the rest
    well separated; labels with both classes among originals and duplicates"""
    rng = np.random.default_rng(seed)
    base = B - n_dup
    while True:
        z = (rng.standard_normal((base, V, Kp, C)) * 2.0).astype(np.float32)
        if separated(prob64(z, positive_class)):
            break
    z = np.concatenate([z, z[:n_dup]])
    dup_of = np.concatenate([np.arange(base), np.arange(n_dup)])
    assert separated(prob64(z, positive_class), dup_of) and not separated(prob64(z, positive_class))
    y = rng.integers(0, C, B)
    y[:2] = (positive_class, (positive_class + 1) % C)
    y[base:base + 2] = ((positive_class + 1) % C, positive_class)     # a duplicate pair with different labels
    return z, y


@pytest.mark.parametrize("C,Kp,pc", [(2, 1, 1), (2, 3, 1), (5, 3, 3)])
def test_auc_table_against_sklearn(dev, C, Kp, pc):
    from src.ranking import AucTable
    B, n = 97, 2
    V = 3 + 2 * n
    z, y = make_logits(B, V, Kp, C, pc, 100 + 10 * C + Kp)
    want = [roc_auc_score(y == pc, prob64(z, pc)[:, v]) for v in range(V)]
    zd, yd = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    tables = {"BVKC": AucTable(n, pc)}
    tables["BVKC"].update(zd[:40], yd[:40])
    tables["BVKC"].update(zd[40:], yd[40:])
    if Kp == 1:
        tables["BVC"] = AucTable(n, pc)
        tables["BVC"].update(zd[:13, :, 0], yd[:13])
        tables["BVC"].update(zd[13:, :, 0].contiguous(), yd[13:])
        tables["VBC"] = AucTable(n, pc)
        vbc = zd[:, :, 0].transpose(0, 1).contiguous()                  # [V, B, C], as robustness_logits leaves it
        tables["VBC"].update(vbc[:, :61], yd[:61], layout="VBC")
        tables["VBC"].update(vbc[:, 61:], yd[61:], layout="VBC")
    for name, t in tables.items():
        res = t.result()
        assert list(res) == ["n", "n_pos", "auc"] and (res["n"], res["n_pos"]) == (B, int((y == pc).sum()))
        check_block_shape(res["auc"], n)
        got = flat_aucs(res["auc"])
        worst = max(abs(a - b) for a, b in zip(got, want))
        print(f"\nC={C} K={Kp} positive={pc} {name}: worst |AUC - sklearn on fp64| = {worst:.3g} (bar {BAR:g})")
        assert worst <= BAR
        assert abs(res["auc"]["image_control"]["mean"] - np.mean(want[3:3 + n])) <= BAR
        assert abs(res["auc"]["text_control"]["std"] - np.std(want[3 + n:])) <= BAR
    # merge of the two halves' states is the whole; one class only is None
    a, b = AucTable(n, pc), AucTable(n, pc, dev)
    a.update(zd[:50], yd[:50])
    b.update(zd[50:], yd[50:])
    a.merge(b.state())
    assert a.result() == tables["BVKC"].result()
    only = AucTable(n, pc)
    only.update(zd, torch.full_like(yd, pc))
    assert flat_aucs(only.result()["auc"]) == [None] * V and only.result()["n_pos"] == B
    with pytest.raises(ValueError, match="variants"):
        AucTable(n + 1, pc).update(zd, yd)
    with pytest.raises(ValueError, match="positive_class"):
        AucTable(n, C).update(zd, yd)


def test_selective_on_a_decompose_meter(dev):
    from src.ranking import SELECTIVE_SCORES, aurc_from_ranks, selective, selective_of_meter
    from src.uncertainty import UncertaintyMeter, auroc
    S, Km, T, C = 200, 3, 2, 5
    g = torch.Generator().manual_seed(21)
    lo = (torch.randn(Km, T, S, C, generator=g) * 1.5).to(dev)
    y = torch.randint(0, C, (S,), generator=g).to(dev)
    meter = UncertaintyMeter(15, decompose=True)
    meter.update(lo, y)
    ps = meter.per_sample()
    wrong = ps["correct"] == 0
    assert 0 < wrong.sum() < S
    got = selective_of_meter(meter, dev)
    assert list(got) == list(SELECTIVE_SCORES) + ["n", "error_rate"]
    assert got["n"] == S and got["error_rate"] == float(wrong.mean())
    scores = {"total": ps["total"], "mi": ps["mi"], "one_minus_conf": 1.0 - ps["conf"],
              "vote_disagreement": ps["vote_disagreement"]}
    host = meter.result()["auroc"]
    for name in SELECTIVE_SCORES:
        s32 = scores[name].astype(np.float32)                    # what the kernel ranks
        rank, counts = R.rank_table_ref(s32.reshape(S, 1), wrong)
        d_host, d_ref = abs(got[name]["auroc"] - auroc(s32, wrong)), abs(got[name]["auroc"] - R.auroc_ref(s32, wrong))
        want = aurc_from_ranks(rank[0], wrong)
        print(f"\n{name}: auroc {got[name]['auroc']:.6f} (|d| host {d_host:.3g}, ref {d_ref:.3g}; the meter's own on "
              f"fp64 scores {host[name]:.6f}), aurc {got[name]['aurc']:.6f}, eaurc {got[name]['eaurc']:.6f}")
        assert list(got[name]) == ["auroc", "aurc", "eaurc"]
        assert d_host <= BAR and d_ref <= BAR
        assert got[name]["aurc"] == want["aurc"] and got[name]["eaurc"] == want["eaurc"]
        assert 0.0 <= got[name]["eaurc"] <= got[name]["aurc"] <= 1.0
        if np.unique(s32).size == S:
            assert abs(got[name]["aurc"] - R.aurc_sorted_ref(s32, wrong)) <= BAR
        if name in ("total", "vote_disagreement"):               # f32 columns: nothing is rounded on the way
            assert abs(got[name]["auroc"] - host[name]) <= BAR
    assert np.unique(scores["vote_disagreement"]).size < 10             # heavy ties were reached
    # a perfect score, its reverse, and a tie-free score against the sort definition
    shuffled = np.random.default_rng(6).permutation(S).astype(np.float32)
    more = selective({"oracle": wrong.astype(np.float64), "reversed": 1.0 - wrong, "shuffled": shuffled}, wrong, dev)
    assert more["oracle"]["auroc"] == 1.0 and abs(more["oracle"]["eaurc"]) <= BAR
    assert more["reversed"]["auroc"] == 0.0 and more["reversed"]["eaurc"] > 0.1
    assert abs(more["shuffled"]["aurc"] - R.aurc_sorted_ref(shuffled, wrong)) <= BAR
    assert abs(more["shuffled"]["auroc"] - auroc(shuffled, wrong)) <= BAR


# ------------------------------------------------------------------------------- entry points
def test_auc_table_and_auc_from_entry_points(dev, tmp_path, monkeypatch):
    import eval_mmbt_robustness as E
    from src.mmbt import MultimodalBertClf
    from src.ranking import AucTable, ensemble_auc
    from src.testing import _Vocab, small_args

    def build(args):
        return MultimodalBertClf(small_args(n_classes=args.n_classes, vocab=args.vocab,
                                            vocab_size=args.vocab.vocab_sz,
                                            num_image_embeds=args.num_image_embeds))
    monkeypatch.setattr(E, "MultimodalBertClf", build)
    torch.manual_seed(5)
    ck = build(type("A", (), dict(n_classes=101, vocab=_Vocab(), num_image_embeds=3)))
    path = str(tmp_path / "small_model.pt")
    torch.save({"model": ck.state_dict()}, path)
    del ck
    n, pc = 2, 50                                                        # two of the 8 synthetic labels are 50
    V = 3 + 2 * n
    common = ["--phase", "val", "--batch_size", "3", "--checkpoint_path", path, "--synthetic", "8",
              "--max_seq_len", "24", "--n_repeats", str(n), "--seed", "13"]
    old_dir, new_dir = str(tmp_path / "old"), str(tmp_path / "new")
    assert E.main(common + ["--save_path", old_dir, "--summary"]) is not None
    E.main(common + ["--save_path", new_dir, "--summary", "--auc_table", "--positive_class", str(pc)])
    assert sorted(os.listdir(new_dir)) == sorted(os.listdir(old_dir) + ["robustness_small_model_auc_val.json"])
    for f in os.listdir(old_dir):                                        # the other files do not change
        assert open(os.path.join(old_dir, f), "rb").read() == open(os.path.join(new_dir, f), "rb").read(), f
    only_dir = str(tmp_path / "only")
    ret = E.main(common + ["--save_path", only_dir, "--auc_table", "--positive_class", str(pc)])   # without --summary
    written = strict_load(os.path.join(new_dir, "robustness_small_model_auc_val.json"))
    assert ret == written == strict_load(os.path.join(only_dir, "robustness_small_model_auc_val.json"))
    assert list(written) == ["n", "n_pos", "auc", "n_repeats", "seed", "positive_class"]
    preds_path = os.path.join(new_dir, "robustness_small_model_predictions_val.npy")
    labels_path = os.path.join(new_dir, "robustness_small_model_labels_val.npy")
    preds, labels = np.load(preds_path), np.load(labels_path)
    assert (written["n"], written["n_pos"], written["n_repeats"], written["seed"], written["positive_class"]) == \
        (8, int((labels == pc).sum()), n, 13, pc) and written["n_pos"] == 2
    check_block_shape(written["auc"], n)
    by_hand = AucTable(n, pc)
    by_hand.update(torch.from_numpy(preds).to(dev), torch.from_numpy(labels).to(dev))
    assert by_hand.result()["auc"] == written["auc"]
    assert all(v is not None and 0.0 <= v <= 1.0 for v in flat_aucs(written["auc"]))
    print(f"\nAUC table of the small model: {json.dumps(written['auc'])}")

    # --auc_from: no model, no dataset
    monkeypatch.setattr(E, "MultimodalBertClf", lambda a: pytest.fail("a model was built"))
    monkeypatch.setattr(E, "load_data", lambda a: pytest.fail("a dataset was read"))
    one_dir = str(tmp_path / "one")
    one = E.main(["--save_path", one_dir, "--positive_class", str(pc), "--auc_from", labels_path, preds_path])
    assert os.listdir(one_dir) == ["robustness_small_model_predictions_val_auc_from.json"]
    assert one == strict_load(os.path.join(one_dir, os.listdir(one_dir)[0]))
    assert list(one) == ["n", "n_pos", "auc", "n_repeats", "positive_class", "files"]
    assert one["auc"] == written["auc"] and (one["n"], one["n_pos"], one["n_repeats"]) == (8, 2, n)
    rng = np.random.default_rng(4)
    stacks = [preds, np.stack([preds + rng.standard_normal(preds.shape).astype(np.float32) for _ in range(2)], axis=2),
              preds + 2 * rng.standard_normal(preds.shape).astype(np.float32)]
    paths = [preds_path]
    for i, s in enumerate(stacks[1:]):
        paths.append(str(tmp_path / f"epoch{i + 2}.npy"))
        np.save(paths[-1], s)
    assert stacks[1].shape == (8, V, 2, 101)                             # a [S, V, K, C] stack among them
    three_dir = str(tmp_path / "three")
    three = E.main(["--save_path", three_dir, "--positive_class", str(pc), "--auc_from", labels_path] + paths)
    assert three == strict_load(os.path.join(three_dir, os.listdir(three_dir)[0]))
    assert list(three) == list(one) + ["ensemble"] and {k: three[k] for k in one if k != "files"} == \
        {k: one[k] for k in one if k != "files"}
    assert three["files"] == [os.path.basename(p) for p in paths]
    ens = three["ensemble"]
    assert list(ens) == ["n_files", "full", "auc"] and ens["n_files"] == 3 and len(ens["full"]) == 3
    check_block_shape(ens["auc"], n)
    by_hand = ensemble_auc(stacks, labels, n, pc, dev)
    assert by_hand["full"] == ens["full"] and by_hand["ensemble"] == ens["auc"] and ens["full"][0] == one["auc"]["full"]
    # and the block is the AUC of the files' mean probability (fp64, where well separated)
    mean = np.mean([prob64(s if s.ndim == 4 else s[:, :, None], pc) for s in stacks], axis=0)
    if separated(mean):
        want = [roc_auc_score(labels == pc, mean[:, v]) for v in range(V)]
        assert max(abs(a - b) for a, b in zip(flat_aucs(ens["auc"]), want)) <= BAR
    with pytest.raises(SystemExit, match="at least one PRED"):
        E.main(["--save_path", one_dir, "--auc_from", labels_path])


def test_selective_entry_point(dev, tmp_path, monkeypatch):
    import eval_robustness as E
    from src import _native as N
    from src.ranking import SELECTIVE_SCORES, selective_of_meter
    from src.testing import small_args
    from src.uncertainty import UncertaintyMeter
    monkeypatch.setattr(E, "mmbt_model_args", lambda args, n_classes, vocab: small_args(
        n_classes=n_classes, vocab=vocab, vocab_size=vocab.vocab_sz, num_image_embeds=args.num_image_embeds))
    cks = [str(tmp_path / f"m{i}.pt") for i in range(2)]
    for p in cks:
        torch.save({"model": {}}, p)      # nothing to load over the seeded initialisation: member i is seed + i
    named = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: named.append(name) or real(name, *a))
    common = ["--mmbt", "--synthetic", "5", "--batch_size", "3", "--max_seq_len", "24", "--mc_samples", "2",
              "--checkpoint_paths"] + cks + ["--variants", "full", "img_only", "--decompose"]
    plain_dir, sel_dir = str(tmp_path / "plain"), str(tmp_path / "sel")
    plain = E.main(common + ["--save_path", plain_dir])
    assert SYMBOL not in named
    sel = E.main(common + ["--save_path", sel_dir, "--selective"])
    assert named.count(SYMBOL) == 2                                      # one launch per meter: full, img_only
    assert list(sel) == list(plain)[:6] + ["selective"] + list(plain)[6:]
    assert {k: sel[k] for k in plain if k != "variants"} == {k: plain[k] for k in plain if k != "variants"}
    assert sorted(os.listdir(sel_dir)) == sorted(os.listdir(plain_dir))
    for f in os.listdir(plain_dir):
        if f.endswith(".npy"):
            assert np.array_equal(np.load(os.path.join(plain_dir, f)), np.load(os.path.join(sel_dir, f))), f
    saved = strict_load(os.path.join(sel_dir, "uncertainty_val_metrics.json"))
    assert saved == sel
    for v in ("full", "img_only"):
        entry = dict(sel["variants"][v])
        s = entry.pop("selective")
        assert entry == plain["variants"][v]
        assert list(s) == list(SELECTIVE_SCORES) + ["n", "error_rate"] and s["n"] == 5
        for name in SELECTIVE_SCORES:
            assert list(s[name]) == ["auroc", "aurc", "eaurc"]
        # the figures are those of the Python call on the saved logits
        lo = np.load(os.path.join(sel_dir, "uncertainty_val_logits.npy" if v == "full" else
                                  "uncertainty_val_img_only_logits.npy"))
        y = np.load(os.path.join(sel_dir, "uncertainty_val_labels.npy"))
        meter = UncertaintyMeter(15, decompose=True)
        meter.update(torch.from_numpy(lo).to(dev), torch.from_numpy(y).to(dev), layout="SKTC")
        assert selective_of_meter(meter, dev) == s
    assert sel["selective"] == sel["variants"]["full"]["selective"]
    print(f"\nselective block of the two seeded members: {json.dumps(sel['selective'])}")
    with pytest.raises(SystemExit, match="--decompose"):
        E.main(["--mmbt", "--synthetic", "5", "--batch_size", "3", "--save_path", sel_dir, "--selective"])


# ------------------------------------------------------------------------------- callback
def test_reliance_callback_logs_the_auc_columns(dev):
    from oracle.weights import SMALL, make_state_dict
    from src.mmbt import MultimodalBertClf
    from src.ranking import AucTable
    from src.robustness import REL_COLUMNS, RelianceCallback, robustness_logits
    from src.testing import small_args, synthetic_batch
    torch.manual_seed(0)
    model = MultimodalBertClf(small_args())
    model.load_state_dict(make_state_dict(3, SMALL), strict=True)
    model = model.to(dev).eval()
    n, seed = 2, 5
    loader = []
    for i in range(2):
        x, y = synthetic_batch(3, 12, vocab=SMALL.vocab, lens=[12, 6, 9], seed=60 + i)
        loader.append((x, torch.tensor([1, 0, 1] if i == 0 else [0, 0, 1])))
    plain = RelianceCallback(model, loader, dev, n_repeats=n, seed=seed)
    off = RelianceCallback(model, loader, dev, n_repeats=n, seed=seed, auc=False)
    on = RelianceCallback(model, loader, dev, n_repeats=n, seed=seed, auc=True)
    base = ["val_rel_" + c for c in REL_COLUMNS]
    extra = ["val_rel_auc_" + k for k in AUC_KEYS]
    assert plain.columns() == off.columns() == base and on.columns() == base + extra
    logs = {}
    for name, cb in (("plain", plain), ("off", off), ("on", on)):
        logs[name] = {}
        cb.on_epoch_end(1, logs[name])
    assert list(logs["plain"]) == list(logs["off"]) == base and logs["plain"] == logs["off"]
    assert list(logs["on"]) == base + extra and {k: logs["on"][k] for k in base} == logs["plain"]
    vals = [logs["on"][k] for k in extra]
    print(f"\nval_rel_auc_*: {vals}")
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals)
    # the same pass spelled out
    torch.manual_seed(seed)
    table = AucTable(n)
    with torch.no_grad():
        for (txt, segment, mask, img), y in loader:
            lo = robustness_logits(model, txt.to(dev), segment.to(dev), mask.to(dev), img.to(dev), n)
            table.update(lo.float(), y.to(dev))
    auc = table.result()["auc"]
    assert on.last_auc["auc"] == auc and on.last_auc["n"] == 6
    assert vals == [auc["full"], auc["image"], auc["text"], auc["image_control"]["mean"], auc["text_control"]["mean"]]
    # a skipped epoch logs NaN in every column, the new ones included
    skipped = {}
    RelianceCallback(model, loader, dev, n_repeats=n, every=2, seed=seed, auc=True).on_epoch_end(1, skipped)
    assert list(skipped) == base + extra and all(np.isnan(v) for v in skipped.values())
