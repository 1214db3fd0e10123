"""Temperature scaling end to end on MI355X (small model; the set-up of test_uncertainty_variants_gpu.py:
small_args, oracle.weights.SMALL, a 4-sample batch of uneven lengths, MIOpen pinned to its deterministic
solvers).

* TemperatureScaler on two chunks of [K = 2, T = 3, B = 4, C] ensemble logits read in place, both modes:
  the fp64 mean NLL (tests/calibration_ref.py) at the tau it finds is no worse than at the tau
  fit_temperature finds with the fp64 numpy evaluator on the same logits, plus 2 x the nll bar of
  test_temperature_nll_gpu.py (each of the two searches ranks candidates by figures that far from fp64
  at most); the two ln tau are printed, not barred -- near the optimum the objective is flat to f32
  resolution.  nll_after <= nll_before.
* UncertaintyMeter(decompose=True, inv_temp=ones) is bitwise the meter without it.
* The default meters and an entry-point run with the flags off never reach the new symbols.
* eval_robustness.py --mmbt --calibrate shared on 3 synthetic samples: the calibration JSON, the
  same-split warning, --temperature with that file reproducing `after` bitwise, and the metrics of a run
  without the flags unchanged.
"""
import json
import os

import numpy as np
import pytest
import torch

from calibration_ref import mean_nll_evaluator
from test_temperature_nll_gpu import sweep as nll_sweep
from test_uncertainty_variants_gpu import members

pytestmark = pytest.mark.gpu

NEW_SYMBOLS = ("mmu_temperature_nll", "mmu_uncertainty_decompose_scaled")


@pytest.fixture(scope="module", autouse=True)
def deterministic_convs():
    """the tests compare separate calls, so MIOpen is pinned to its deterministic solvers (see
    test_uncertainty_gpu.py's fixture of the same name)"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


@pytest.fixture(scope="module")
def batch(dev):
    from oracle.weights import SMALL
    from src.testing import synthetic_batch
    x, y = synthetic_batch(4, 24, lens=[24, 17, 9, 24], vocab=SMALL.vocab, seed=21)
    return tuple(t.to(dev) for t in x), y.to(dev)


@pytest.fixture(scope="module")
def chunks(dev, batch):
    """two seeded [K = 2, T = 3, B = 4, C] calls of one ensemble with BERT dropout 0.1"""
    from src.uncertainty import EnsembleMMBT
    ens = EnsembleMMBT(members(dev, 2))
    out = []
    for seed in (11, 13):
        torch.manual_seed(seed)
        out.append(ens.logits(*batch[0], mc_samples=3))
    return out


@pytest.mark.parametrize("mode", ["shared", "per_member"])
def test_scaler_fits_on_the_logits_in_place(chunks, batch, mode):
    from src.calibration import TemperatureScaler, fit_temperature
    y = batch[1]
    bar = nll_sweep()["bar"]
    sc = TemperatureScaler(mode)
    for lo in chunks:
        sc.add(lo, y)
    assert sc.count == 8 and all(c[0].data_ptr() == lo.data_ptr() for c, lo in zip(sc.chunks, chunks))
    r = sc.fit()
    z = np.concatenate([lo.permute(2, 0, 1, 3).cpu().numpy() for lo in chunks])
    ev = mean_nll_evaluator(z, np.concatenate([y.cpu().numpy()] * 2))
    ref = fit_temperature(ev, 2, mode=mode)
    at_gpu, at_ref = ev(1.0 / np.array([r["tau"]]))[0], ev(1.0 / np.array([ref["tau"]]))[0]
    print(f"\n{mode}: ln tau on device {np.log(r['tau'])}, with the fp64 evaluator {np.log(ref['tau'])}; fp64 mean NLL "
          f"{at_gpu:.7f} vs {at_ref:.7f} (bar {bar:.3e}); device nll {r['nll_before']:.6f} -> {r['nll_after']:.6f}")
    assert at_gpu <= at_ref + 2 * bar
    assert r["nll_after"] <= r["nll_before"]
    assert abs(r["nll_before"] - ev(np.ones((1, 2)))[0]) <= bar and abs(r["nll_after"] - at_gpu) <= bar
    assert r["mode"] == mode and len(r["tau"]) == 2 and (r["passes"] == 4) == (mode == "shared")
    assert sc.fit() == r                                                  # and a second fit is the first
    inv = sc.inv_temp(y.device)
    assert inv.dtype == torch.float32 and inv.is_cuda and inv.shape == (2,)
    assert np.array_equal(inv.cpu().numpy(), (1.0 / np.array(r["tau"])).astype(np.float32))


def test_meter_with_unit_temperatures_is_the_meter_without(chunks, batch):
    from src.uncertainty import UncertaintyMeter
    y = batch[1]
    plain, unit = UncertaintyMeter(15, decompose=True), UncertaintyMeter(
        15, decompose=True, inv_temp=torch.ones(2, device=y.device))
    for lo in chunks:
        assert torch.equal(plain.update(lo, y), unit.update(lo, y))
    for c, v in plain.per_sample().items():
        assert np.array_equal(v, unit.per_sample()[c]), c
    assert np.array_equal(np.concatenate(plain.member_nll), np.concatenate(unit.member_nll))
    assert plain.result() == unit.result()
    # and a temperature moves it: 2 x tau flattens every sample's prediction
    warm = UncertaintyMeter(15, decompose=True, inv_temp=torch.full((2,), 0.5, device=y.device))
    for lo in chunks:
        warm.update(lo, y)
    assert (warm.per_sample()["conf"] < plain.per_sample()["conf"]).all()


def small_model(E, monkeypatch):
    from src.testing import small_args
    monkeypatch.setattr(E, "mmbt_model_args", lambda args, n_classes, vocab: small_args(
        n_classes=n_classes, vocab=vocab, vocab_size=vocab.vocab_sz, num_image_embeds=args.num_image_embeds))


COMMON = ["--mmbt", "--synthetic", "3", "--batch_size", "2", "--max_seq_len", "24", "--mc_samples", "2"]


def test_defaults_never_reach_the_new_symbols(chunks, batch, tmp_path, monkeypatch):
    import eval_robustness as E
    from src import _native as N
    from src import kernels as K
    from src.uncertainty import UncertaintyMeter
    small_model(E, monkeypatch)
    real = N.call

    def guarded_call(name, *a):
        if name in NEW_SYMBOLS:
            raise AssertionError(f"a default path called {name}")
        return real(name, *a)
    monkeypatch.setattr(N, "call", guarded_call)

    def boom(*a, **k):
        raise AssertionError("a default path called temperature_nll")
    monkeypatch.setattr(K, "temperature_nll", boom)
    lo, y = chunks[0], batch[1]
    UncertaintyMeter().update(lo.permute(2, 0, 1, 3).reshape(4, 6, -1), y)
    UncertaintyMeter(15, decompose=True).update(lo, y)
    res = E.main(COMMON + ["--save_path", str(tmp_path / "plain")])
    assert list(res) == ["nll", "ece", "acc", "n", "K", "T"]
    res = E.main(COMMON + ["--save_path", str(tmp_path / "dec"), "--decompose"])
    assert "calibrated" not in res and "variants_calibrated" not in res
    # the guard does guard
    with pytest.raises(AssertionError, match="mmu_uncertainty_decompose_scaled"):
        UncertaintyMeter(15, decompose=True, inv_temp=torch.ones(2, device=y.device)).update(lo, y)
    with pytest.raises(AssertionError, match="temperature_nll"):
        E.main(COMMON + ["--save_path", str(tmp_path / "cal"), "--calibrate", "shared"])


def test_entry_point_calibrates(dev, tmp_path, monkeypatch, capsys):
    import eval_robustness as E
    small_model(E, monkeypatch)
    bar = nll_sweep()["bar"]
    plain_dir, cal_dir, app_dir, var_dir = (str(tmp_path / d) for d in ("plain", "cal", "applied", "variants"))
    plain = E.main(COMMON + ["--save_path", plain_dir])
    assert "WARNING" not in capsys.readouterr().out
    cal = E.main(COMMON + ["--save_path", cal_dir, "--calibrate", "shared", "--calibrate_phase", "val", "--phase", "val"])
    out = capsys.readouterr().out
    assert out.count("WARNING: the temperature was fitted on the split it is evaluated on (val)") == 1
    assert sorted(os.listdir(cal_dir)) == ["uncertainty_val_calibration.json", "uncertainty_val_labels.npy",
                                           "uncertainty_val_logits.npy", "uncertainty_val_metrics.json"]
    cal_json = os.path.join(cal_dir, "uncertainty_val_calibration.json")

    def strict(c):
        raise AssertionError(f"not strict JSON: {c}")
    fit = json.loads(open(cal_json).read(), parse_constant=strict)
    assert set(fit) == {"mode", "tau", "nll_before", "nll_after", "passes", "rounds", "at_bound", "fit_phase",
                        "eval_phase", "same_split", "before", "after"}
    assert (fit["mode"], fit["fit_phase"], fit["eval_phase"], fit["same_split"]) == ("shared", "val", "val", True)
    assert len(fit["tau"]) == 1 and fit["passes"] == 4
    for d in (fit["before"], fit["after"]):
        assert list(d) == list(E.CALIBRATION_KEYS) and all(np.isfinite(v) for v in d.values())
    print(f"\ntau {fit['tau']}, before {fit['before']}, after {fit['after']}")
    assert fit["after"]["nll"] <= fit["before"]["nll"] + bar
    # fitted and evaluated on the same logits: the meters' nll are the fit's own figures
    assert abs(fit["before"]["nll"] - fit["nll_before"]) <= bar and abs(fit["after"]["nll"] - fit["nll_after"]) <= bar
    # the metrics of a run without the flags, plus one key; the same logits and labels
    assert cal == json.load(open(os.path.join(cal_dir, "uncertainty_val_metrics.json")))
    assert list(cal) == list(plain) + ["calibrated"] and cal["calibrated"] == fit["after"]
    assert {k: cal[k] for k in plain} == plain
    assert plain == json.load(open(os.path.join(plain_dir, "uncertainty_val_metrics.json")))
    for f in ("uncertainty_val_logits.npy", "uncertainty_val_labels.npy"):
        assert np.array_equal(np.load(os.path.join(plain_dir, f)), np.load(os.path.join(cal_dir, f)))
    assert abs(fit["before"]["nll"] - plain["nll"]) <= bar and fit["before"]["acc"] == plain["acc"]
    # --temperature with that file: `after` again, bit for bit
    app = E.main(COMMON + ["--save_path", app_dir, "--temperature", cal_json])
    assert "WARNING" in capsys.readouterr().out                           # the file says it was fitted on val
    again = json.load(open(os.path.join(app_dir, "uncertainty_val_calibration.json")))
    assert again["after"] == fit["after"] and again["before"] == fit["before"] and again["tau"] == fit["tau"]
    assert app == cal
    # both flags at once, and a fit for another ensemble size
    with pytest.raises(ValueError, match="give one of them"):
        E.main(COMMON + ["--save_path", app_dir, "--calibrate", "shared", "--temperature", cal_json])
    two = str(tmp_path / "two.json")
    json.dump(dict(fit, tau=[1.0, 2.0], at_bound=[False, False]), open(two, "w"))
    with pytest.raises(ValueError, match="holds 2 members, the ensemble 1"):
        E.main(COMMON + ["--save_path", app_dir, "--temperature", two])
    # --variants: every variant again under the full forward's temperature
    var = E.main(COMMON + ["--save_path", var_dir, "--temperature", cal_json, "--variants", "full", "img_only"])
    assert list(var["variants_calibrated"]) == list(var["variants"]) == ["full", "img_only"]
    assert var["calibrated"] == {k: var["variants_calibrated"]["full"][k] for k in E.CALIBRATION_KEYS}
    assert all(np.isfinite(v) for v in var["calibrated"].values())       # (other logits: the variant calls draw seeds)
    assert set(var["variants_calibrated"]["img_only"]) == set(var["variants"]["img_only"])
    assert var["variants_calibrated"]["img_only"] != var["variants"]["img_only"] or fit["tau"] == [1.0]
