"""The ensemble's modality variants and the decomposition meter, end to end on MI355X (small model;
the set-up of test_uncertainty_gpu.py: small_args, oracle.weights.SMALL, a 4-sample batch of uneven
lengths, MIOpen pinned to its deterministic solvers).

* T = 1, no dropout, K = 2: for img_only, txt_only and both controls (torch.manual_seed(n) before each
  call), member k's logits from EnsembleMMBT.logits(variant=...) equal member k's own forward_* on the
  HIP path, within the tolerance test_uncertainty_gpu.py uses for "member vs its own forward"
  (rel 1e-2, abs 1e-3); variant=None is bitwise the call without the argument.
* mc_samples = 3, dropout 0.1: UncertaintyMeter(decompose=True) fed the [K, T, B, C] tensor in place
  gives per-sample statistics equal to the fp64 reference (test_uncertainty_decompose_gpu.py
  decompose_ref) on those HIP logits within that file's bar, its nll / ece / acc equal the default
  meter's on the permuted logits (1e-5 relative, 1e-5, exact: the tolerances of
  test_config3_full_members_k5_t30), and both mutual-information parts are positive for some sample.
* The default UncertaintyMeter never reaches the new symbol.
* eval_robustness.py --mmbt: the same files and metrics without the new flags, the "decomposition" and
  "variants" blocks and the per-variant logits files with them.
"""
import numpy as np
import pytest
import torch

from test_uncertainty_decompose_gpu import COLUMNS, decompose_ref, sweep

pytestmark = pytest.mark.gpu

VARIANTS = ("img_only", "txt_only", ("control", "image"), ("control", "text"))


@pytest.fixture(scope="module", autouse=True)
def deterministic_convs():
    """the tests compare separate calls, so MIOpen is pinned to its deterministic solvers (see
    test_uncertainty_gpu.py's fixture of the same name)"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def tol_check(got, ref, rel, abs_, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    assert err <= rel * scale + abs_, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def members(dev, K, **over):
    from oracle.weights import SMALL, make_state_dict
    from src.mmbt import MultimodalBertClf
    from src.testing import small_args
    over.setdefault("img_precision", "fp32")
    out = []
    for k in range(K):
        torch.manual_seed(k)
        m = MultimodalBertClf(small_args(**over))
        m.load_state_dict(make_state_dict(k, SMALL), strict=True)
        out.append(m.to(dev).eval())
    return out


@pytest.fixture(scope="module")
def batch(dev):
    from oracle.weights import SMALL
    from src.testing import synthetic_batch
    x, y = synthetic_batch(4, 24, lens=[24, 17, 9, 24], vocab=SMALL.vocab, seed=21)
    return tuple(t.to(dev) for t in x), y.to(dev)


@pytest.fixture(scope="module")
def ensemble(dev):
    from src.uncertainty import EnsembleMMBT
    ms = members(dev, 2)
    return ms, EnsembleMMBT(ms)


@pytest.fixture(scope="module")
def mc_logits(ensemble, batch):
    """[K = 2, T = 3, B = 4, C] with BERT dropout 0.1, one seeded call shared by the meter tests"""
    _, ens = ensemble
    torch.manual_seed(11)
    return ens.logits(*batch[0], mc_samples=3)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v if isinstance(v, str) else "_".join(v))
def test_member_equals_its_own_variant_forward(ensemble, batch, variant):
    ms, ens = ensemble
    xd, _ = batch
    torch.manual_seed(3)
    lo = ens.logits(*xd, mc_samples=1, variant=variant)
    assert lo.shape == (2, 1, 4, 101) and torch.isfinite(lo).all()
    for k, m in enumerate(ms):
        torch.manual_seed(3)
        with torch.no_grad():
            single = {"img_only": m.forward_img_only, "txt_only": m.forward_txt_only}[variant](*xd) \
                if isinstance(variant, str) else m.forward_control(*xd, variant[1])
        tol_check(lo[k, 0].cpu(), single.cpu(), 1e-2, 1e-3, f"member {k} {variant} vs its own forward")
    # the variant is not the full forward in disguise
    moved = (ens.logits(*xd, mc_samples=1) - lo).abs().amax().item()
    print(f"{variant}: max |full - variant| = {moved:.3e}")
    assert moved > 1e-3


def test_variant_none_is_the_call_without_it(ensemble, batch):
    _, ens = ensemble
    xd, _ = batch
    assert torch.equal(ens.logits(*xd, mc_samples=1), ens.logits(*xd, mc_samples=1, variant=None))
    torch.manual_seed(7)
    a = ens.logits(*xd, mc_samples=3)
    torch.manual_seed(7)
    b = ens.logits(*xd, mc_samples=3, variant=None)
    assert torch.equal(a, b)


def test_variants_run_with_mc_dropout(ensemble, batch):
    """T = 3 passes of a variant: finite, the passes differ, seed-reproducible, one control draw per call"""
    _, ens = ensemble
    xd, _ = batch
    for variant in ("img_only", ("control", "text")):
        torch.manual_seed(5)
        a = ens.logits(*xd, mc_samples=3, variant=variant)
        torch.manual_seed(5)
        b = ens.logits(*xd, mc_samples=3, variant=variant)
        assert a.shape == (2, 3, 4, 101) and torch.isfinite(a).all() and torch.equal(a, b)
        assert (a[:, 1:] - a[:, :1]).abs().amax().item() > 1e-3, "MC-dropout passes are identical"


def test_decompose_meter_on_the_ensemble_logits_in_place(mc_logits, batch):
    from src.uncertainty import UncertaintyMeter
    lo, y = mc_logits, batch[1]
    bar = sweep()["bar"]
    meter = UncertaintyMeter(15, decompose=True)
    p_bar = meter.update(lo, y).double().cpu().numpy()
    ref = decompose_ref(lo.permute(2, 0, 1, 3).cpu().numpy(), y.cpu().numpy(), np.float64)
    ps = meter.per_sample()
    for c in COLUMNS:
        err = np.abs(ps[c] - ref[c]).max()
        print(f"{c:18s} error {err:.3e} bar {bar[c]:.3e}")
        assert err <= bar[c], f"{c}: {err:.3e} > bar {bar[c]:.3e}"
    assert np.abs(p_bar - ref["p_bar"]).max() <= bar["p_bar"]
    assert np.abs(ps["mi"] - (ref["mi_members"] + ref["mi_passes"])).max() <= bar["mi_members"] + bar["mi_passes"]
    assert np.abs(np.concatenate(meter.member_nll) - ref["member_nll"]).max() <= bar["member_nll"]
    print(f"mi_passes {ps['mi_passes']} mi_members {ps['mi_members']}")
    assert ps["mi_passes"].max() > 0 and ps["mi_members"].max() > 0
    # the same logits in the other layout, in two updates: the per-sample statistics do not move
    two = UncertaintyMeter(15, decompose=True)
    skt = lo.permute(2, 0, 1, 3).contiguous()
    two.update(skt[:3], y[:3], layout="SKTC")
    two.update(skt[3:], y[3:], layout="SKTC")
    for c in COLUMNS:
        assert np.array_equal(two.per_sample()[c], ps[c]), c

    res = meter.result()
    plain = UncertaintyMeter(15)
    plain.update(lo.permute(2, 0, 1, 3).reshape(4, 6, -1), y)
    old = plain.result()
    assert set(old) == {"nll", "ece", "acc", "n"}
    assert abs(res["nll"] - old["nll"]) <= 1e-5 * abs(old["nll"]) + 1e-7
    assert abs(res["ece"] - old["ece"]) < 1e-5
    assert res["acc"] == old["acc"] and res["n"] == old["n"] == 4
    # the host-side summary
    for c in COLUMNS:
        if c not in ("nll", "correct"):
            assert res[c] == pytest.approx(ps[c].mean(), abs=1e-12)
    assert res["mi"] == pytest.approx(res["mi_members"] + res["mi_passes"], abs=1e-12)
    assert len(res["member_nll"]) == 2
    assert res["member_nll"] == pytest.approx(ref["member_nll"].mean(0), abs=bar["member_nll"])
    assert res["ensemble_gain"] == pytest.approx(np.mean(res["member_nll"]) - res["nll"], abs=1e-12)
    assert set(res["auroc"]) == {"total", "mi", "one_minus_conf", "vote_disagreement"}
    wrong = ref["correct"] == 0
    for v in res["auroc"].values():
        assert (v is None) == (wrong.all() or not wrong.any())
        assert v is None or 0.0 <= v <= 1.0


def test_default_meter_never_reaches_the_new_symbol(mc_logits, batch, monkeypatch):
    from src import kernels as K
    from src.uncertainty import UncertaintyMeter
    lo, y = mc_logits, batch[1]
    flat = lo.permute(2, 0, 1, 3).reshape(4, 6, -1)
    before = UncertaintyMeter()
    before.update(flat, y)

    def boom(*a, **k):
        raise AssertionError("UncertaintyMeter() called uncertainty_decompose")
    monkeypatch.setattr(K, "uncertainty_decompose", boom)
    after = UncertaintyMeter()
    p_bar = after.update(flat, y)
    assert after.result() == before.result() and set(after.result()) == {"nll", "ece", "acc", "n"}
    assert p_bar.shape == (4, 101)
    with pytest.raises(AssertionError, match="called uncertainty_decompose"):
        UncertaintyMeter(decompose=True).update(lo, y)


def test_entry_point_writes_the_decomposition_and_the_variants(dev, tmp_path, monkeypatch):
    """eval_robustness.py --mmbt on 3 synthetic samples (batches of 2 and 1) with a small model:
    without the new flags the three files and the metrics keys of before; with them the
    "decomposition" and "variants" blocks and one logits file per variant that is not the full forward"""
    import json
    import os
    import eval_robustness as E
    from src.testing import small_args
    monkeypatch.setattr(E, "mmbt_model_args", lambda args, n_classes, vocab: small_args(
        n_classes=n_classes, vocab=vocab, vocab_size=vocab.vocab_sz, num_image_embeds=args.num_image_embeds))
    common = ["--mmbt", "--synthetic", "3", "--batch_size", "2", "--max_seq_len", "24", "--mc_samples", "2"]
    old_dir, new_dir = str(tmp_path / "old"), str(tmp_path / "new")
    old = E.main(common + ["--save_path", old_dir])
    assert list(old) == ["nll", "ece", "acc", "n", "K", "T"]
    assert sorted(os.listdir(old_dir)) == ["uncertainty_val_labels.npy", "uncertainty_val_logits.npy",
                                           "uncertainty_val_metrics.json"]
    new = E.main(common + ["--save_path", new_dir, "--decompose", "--variants", "full", "img_only", "control_text"])
    assert new == json.load(open(os.path.join(new_dir, "uncertainty_val_metrics.json")))
    assert list(new)[:6] == list(old) and (new["n"], new["K"], new["T"]) == (3, 1, 2)
    assert list(new["variants"]) == ["full", "img_only", "control_text"]
    assert {k: new[k] for k in ("nll", "ece", "acc", "n")} == {k: new["variants"]["full"][k]
                                                                for k in ("nll", "ece", "acc", "n")}
    for block in [new["decomposition"]] + [{k: v for k, v in b.items() if k not in ("nll", "ece", "acc", "n")}
                                           for b in new["variants"].values()]:
        assert set(block) == {"total", "aleatoric", "mi_members", "mi_passes", "brier", "conf", "vote_disagreement",
                              "mi", "member_nll", "ensemble_gain", "auroc"}
        assert abs(block["mi_members"]) <= sweep()["bar"]["mi_members"]          # one member
        assert abs(block["ensemble_gain"]) < 1e-5
    assert np.load(os.path.join(new_dir, "uncertainty_val_logits.npy")).shape == (3, 1, 2, 101)
    for v in ("img_only", "control_text"):
        assert np.load(os.path.join(new_dir, f"uncertainty_val_{v}_logits.npy")).shape == (3, 1, 2, 101)
    assert len(os.listdir(new_dir)) == 5
