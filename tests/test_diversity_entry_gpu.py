"""Ensemble diversity through eval_robustness.py on MI355X.

* --diversity_from on a small saved stack (S = 7, K = 3, T = 2, C = 11): the JSON it writes against a
  DiversityMeter driven from tests/diversity_ref.py's fp64 rows -- every counted figure (disagreement,
  the contingency tables and what follows from them, the accuracies, how many tau are defined) equal,
  js within the bar of test_diversity_gpu.py, tau within 2^-24 (the kernel stores the f32 rounding of a
  value in [-1, 1]).  No model is built.
* One tiny-model run (the small args of src.testing, 2 members that differ by their seeds, T = 2, 3
  synthetic samples) with --variants full img_only, without and with --diversity: the flag adds the
  "diversity" and "variants_diversity" blocks and uncertainty_val_diversity.json and leaves the logits
  files, the labels and every other metric bitwise alone; the run without it never names the symbol.
"""
import json
import os

import numpy as np
import pytest
import torch

from diversity_ref import diversity_ref, make_logits

pytestmark = pytest.mark.gpu

SYMBOL = "mmu_ensemble_diversity"
COUNTED = ("n", "K", "top", "mute_true", "pairs", "disagree", "tau_n", "contingency", "double_fault", "q", "phi",
           "member_acc")


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


@pytest.mark.parametrize("keep_true", [False, True])
def test_diversity_from_a_saved_stack(dev, tmp_path, monkeypatch, keep_true):
    import eval_robustness as E
    from src.diversity import DiversityMeter
    from test_diversity_gpu import sweep
    bar = sweep()["bar"]
    z, y = make_logits(11, 3, 2, 7, 1, 77, 5)
    y[3] = 11                                                      # a label outside the classes mutes nothing
    np.save(tmp_path / "lo.npy", z)
    np.save(tmp_path / "y.npy", y)
    monkeypatch.setattr(E, "run_mmbt", lambda a: pytest.fail("a model run was started"))
    out = E.main(["--save_path", str(tmp_path / "out"), "--phase", "test", "--diversity_from",
                  str(tmp_path / "lo.npy"), str(tmp_path / "y.npy")] + (["--diversity_keep_true"] if keep_true else []))
    assert os.listdir(tmp_path / "out") == ["uncertainty_test_diversity.json"]
    got = strict_load(tmp_path / "out" / "uncertainty_test_diversity.json")
    assert got == out and list(got) == ["diversity"]
    r = diversity_ref(z, y, 5, not keep_true, np.float64)
    ref = DiversityMeter(5, not keep_true)
    ref.update_rows(np.stack([r["js"], r["disagree"], r["tau"]], axis=2), r["member_arg"], y)
    want, got = ref.result(), got["diversity"]
    assert list(got) == list(want)
    for k in COUNTED:
        assert got[k] == want[k], k
    assert got["tau_n"] == [7, 7, 7]
    for name, tol in (("js", bar), ("tau", 2.0 ** -24)):
        err = max(abs(a - b) for a, b in zip(got[name], want[name]))
        print(f"\n{name}: largest difference of a pair's mean {err:.3e}, bound {tol:.3e}")
        assert err <= tol
        assert abs(got["mean"][name] - want["mean"][name]) <= tol
        for i in range(3):
            for j in range(3):
                a, b = got["matrix"][name][i][j], want["matrix"][name][i][j]
                assert (a is None) == (b is None) and (a is None or abs(a - b) <= tol)
    for name in ("disagree", "double_fault", "q", "phi"):
        assert got["matrix"][name] == want["matrix"][name] and got["mean"][name] == want["mean"][name]


def test_entry_point_adds_the_blocks_and_leaves_the_rest(dev, tmp_path, monkeypatch):
    import eval_robustness as E
    from src import _native as N
    from src.testing import small_args
    monkeypatch.setattr(E, "mmbt_model_args", lambda args, n_classes, vocab: small_args(
        n_classes=n_classes, vocab=vocab, vocab_size=vocab.vocab_sz, num_image_embeds=args.num_image_embeds))
    cks = [str(tmp_path / f"m{i}.pt") for i in range(2)]
    for p in cks:
        torch.save({"model": {}}, p)      # nothing to load over the seeded initialisation: member i is seed + i
    named = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: named.append(name) or real(name, *a))
    common = ["--mmbt", "--synthetic", "3", "--batch_size", "2", "--max_seq_len", "24", "--mc_samples", "2",
              "--checkpoint_paths"] + cks + ["--variants", "full", "img_only"]
    plain_dir, div_dir = str(tmp_path / "plain"), str(tmp_path / "div")
    plain = E.main(common + ["--save_path", plain_dir])
    assert SYMBOL not in named and "mmu_uncertainty_decompose" in named
    div = E.main(common + ["--save_path", div_dir, "--diversity"])
    assert named.count(SYMBOL) == 2 * 2                              # 2 batches x (full, img_only)
    assert list(div) == list(plain) + ["diversity", "variants_diversity"]
    assert {k: div[k] for k in plain} == plain
    assert sorted(os.listdir(div_dir)) == sorted(os.listdir(plain_dir) + ["uncertainty_val_diversity.json"])
    for f in os.listdir(plain_dir):
        if f.endswith(".npy"):
            assert np.array_equal(np.load(os.path.join(plain_dir, f)), np.load(os.path.join(div_dir, f))), f
    saved = json.load(open(os.path.join(div_dir, "uncertainty_val_metrics.json")))
    assert saved == div and {k: saved[k] for k in plain} == json.load(
        open(os.path.join(plain_dir, "uncertainty_val_metrics.json")))
    blocks = strict_load(os.path.join(div_dir, "uncertainty_val_diversity.json"))
    assert blocks == {"diversity": div["diversity"], "variants_diversity": div["variants_diversity"]}
    assert list(div["variants_diversity"]) == ["full", "img_only"]
    assert div["variants_diversity"]["full"] == div["diversity"]
    for d in (div["diversity"], div["variants_diversity"]["img_only"]):
        assert (d["n"], d["K"], d["top"], d["mute_true"], d["pairs"]) == (3, 2, 5, True, [[0, 1]])
        assert 0.0 <= d["js"][0] <= np.log(2.0) + 1e-6 and d["disagree"][0] in (0.0, 1 / 3, 2 / 3, 1.0)
        assert d["tau_n"] == [3] and -1.0 <= d["tau"][0] <= 1.0 and sum(d["contingency"][0]) == 3
    # the figures are those of the meter on the saved logits
    lo = np.load(os.path.join(div_dir, "uncertainty_val_logits.npy"))
    y = np.load(os.path.join(div_dir, "uncertainty_val_labels.npy"))
    assert lo.shape[:3] == (3, 2, 2)
    r = diversity_ref(lo, y, 5, True, np.float64)
    assert div["diversity"]["member_acc"] == [float(v) for v in (r["member_arg"] == y[:, None]).mean(0)]
    assert abs(div["diversity"]["js"][0] - r["js"].mean()) <= 1e-5
    print(f"\ndiversity of the two seeded members: {json.dumps(div['diversity'])}")
    # --diversity_keep_true and --diversity_top reach the meter
    keep = E.main(common + ["--save_path", str(tmp_path / "keep"), "--diversity", "--diversity_keep_true",
                            "--diversity_top", "0"])
    assert (keep["diversity"]["top"], keep["diversity"]["mute_true"]) == (0, False)
