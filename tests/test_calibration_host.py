"""src/calibration.py without a GPU: fit_temperature driven by an fp64 numpy evaluator of include/mmu.h's
definitions (tests/calibration_ref.py), the TemperatureScaler's JSON round trip, every refusal, and the
new eval_robustness.py flags.

The planted-temperature cases: labels are drawn from softmax(z0) and the logits served are tau0 z0, so
the expected NLL is smallest at tau = tau0.  With S = 4000 samples of C = 10 classes (z0 standard normal
x 2) the maximum-likelihood tau has a standard error of about 2 % (measured over seeds: |ln tau - ln tau0|
stayed below 0.04), well inside the 0.1 asked of it.
"""
import argparse
import json

import numpy as np
import pytest

from calibration_ref import mean_nll_evaluator, temperature_nll_ref
from src.calibration import TemperatureScaler, fit_temperature

LO, HI = 0.05, 20.0


def planted(taus, S=4000, C=10, T=1, seed=0):
    """members that all see z0, member k served as tau_k z0; labels drawn from softmax(z0)
    -> (z f32 [S, K, T, C], y [S])"""
    g = np.random.default_rng(seed)
    z0 = 2.0 * g.standard_normal((S, C))
    p = np.exp(z0 - z0.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    y = (p.cumsum(-1) < g.uniform(size=(S, 1))).sum(-1).clip(0, C - 1).astype(np.int64)
    z = np.stack([np.repeat((t * z0)[:, None, :], T, axis=1) for t in taus], axis=1)
    return z.astype(np.float32), y


@pytest.mark.parametrize("tau0", [0.5, 3.0])
def test_planted_shared_temperature_is_recovered(tau0):
    z, y = planted([tau0])
    r = fit_temperature(mean_nll_evaluator(z, y), 1)
    print(f"tau0 {tau0}: fitted {r['tau'][0]:.4f}, nll {r['nll_before']:.4f} -> {r['nll_after']:.4f}")
    assert abs(np.log(r["tau"][0]) - np.log(tau0)) <= 0.1
    assert r["mode"] == "shared" and r["passes"] == 4 and r["rounds"] == 0 and r["at_bound"] == [False]
    assert r["nll_after"] < r["nll_before"]
    ev = mean_nll_evaluator(z, y)
    assert r["nll_before"] == ev(np.ones((1, 1)))[0]
    assert r["nll_after"] == ev(1.0 / np.array([r["tau"]]))[0]


@pytest.mark.parametrize("mode", ["shared", "per_member"])
def test_ties_leave_tau_at_one(mode):
    """all-equal logits, and C = 1: every candidate has the same NLL, and the tie rule (smallest |ln tau|)
    keeps tau = 1 exactly"""
    y = np.array([0, 2, 1, 0], dtype=np.int64)
    for z in (np.zeros((4, 2, 3, 5), dtype=np.float32), np.full((4, 2, 3, 5), 7.5, dtype=np.float32)):
        r = fit_temperature(mean_nll_evaluator(z, y), 2, mode=mode)
        assert r["tau"] == [1.0, 1.0] and r["nll_before"] == r["nll_after"] and r["at_bound"] == [False, False]
    z1 = np.random.default_rng(0).standard_normal((4, 2, 3, 1)).astype(np.float32)
    r = fit_temperature(mean_nll_evaluator(z1, np.zeros(4, dtype=np.int64)), 2, mode=mode)
    assert r["tau"] == [1.0, 1.0] and r["nll_after"] == 0.0


def test_always_right_runs_to_the_lower_bound():
    """labels always the argmax: sharper is better without end, so the fit stops on the range's lower end"""
    z = np.random.default_rng(1).standard_normal((200, 1, 2, 5)).astype(np.float32)
    y = z.mean(2)[:, 0].argmax(-1).astype(np.int64)
    z[np.arange(200)[:, None], 0, np.arange(2)[None, :], y[:, None]] = z.max(-1)[:, 0] + 0.5    # every pass agrees
    r = fit_temperature(mean_nll_evaluator(z, y), 1)
    assert r["at_bound"] == [True] and r["tau"][0] == pytest.approx(LO, rel=1e-12)
    assert r["nll_after"] < r["nll_before"]
    r = fit_temperature(mean_nll_evaluator(z, y), 1, tau_range=(0.5, 4.0))
    assert r["at_bound"] == [True] and r["tau"][0] == pytest.approx(0.5, rel=1e-12)


PLANTED = (0.3, 3.0)


def test_per_member_beats_shared_and_finds_the_planted_temperatures():
    z, y = planted(PLANTED)
    ev = mean_nll_evaluator(z, y)
    sh = fit_temperature(ev, 2, mode="shared")
    pm = fit_temperature(ev, 2, mode="per_member")
    print(f"shared tau {sh['tau'][0]:.4f} nll {sh['nll_after']:.5f}; per-member tau {pm['tau']} "
          f"nll {pm['nll_after']:.5f} in {pm['rounds']} rounds, {pm['passes']} passes")
    assert pm["nll_after"] <= sh["nll_after"] <= sh["nll_before"]
    assert pm["nll_before"] == sh["nll_before"]
    assert sh["tau"][0] == sh["tau"][1] and 1 <= pm["rounds"] <= 8
    for k, t0 in enumerate(PLANTED):
        assert abs(np.log(pm["tau"][k]) - np.log(t0)) < abs(np.log(sh["tau"][k]) - np.log(t0)), (k, pm, sh)
    assert pm["nll_after"] == ev(1.0 / np.array([pm["tau"]]))[0]


@pytest.mark.parametrize("mode", ["shared", "per_member"])
def test_two_fits_are_identical(mode):
    z, y = planted((0.7, 2.0), S=300, T=2, seed=3)
    a = fit_temperature(mean_nll_evaluator(z, y), 2, mode=mode)
    b = fit_temperature(mean_nll_evaluator(z, y), 2, mode=mode)
    assert a == b


def test_even_grid_and_lopsided_range_still_report_nll_before():
    z, y = planted([2.0], S=300, seed=4)
    ev = mean_nll_evaluator(z, y)
    for kw in (dict(grid=16), dict(tau_range=(0.5, 20.0)), dict(grid=3, tol=1e-3)):
        r = fit_temperature(ev, 1, **kw)
        assert r["nll_before"] == ev(np.ones((1, 1)))[0] and r["nll_after"] <= r["nll_before"]
        assert abs(np.log(r["tau"][0]) - np.log(2.0)) <= 0.3


@pytest.mark.parametrize("tau0", [0.5, 3.0])
def test_three_point_grid_terminates_and_converges(tau0):
    """grid = 3: when the middle point wins, its neighbours are the bracket itself, which is then halved
    around it; when an end wins, the bracket moves one spacing that way.  The search ends at the tolerance
    and lands where the 33-point search does"""
    z, y = planted([tau0], S=1000, seed=6)
    ev = mean_nll_evaluator(z, y)
    fine = fit_temperature(ev, 1)
    r = fit_temperature(ev, 1, grid=3)
    print(f"tau0 {tau0}: grid 3 -> {r['tau'][0]:.5f} in {r['passes']} passes, grid 33 -> {fine['tau'][0]:.5f}")
    # ln(400) / 1e-4 < 2^16 halvings, and after each at most one move
    assert 4 < r["passes"] <= 34
    assert abs(np.log(r["tau"][0]) - np.log(fine["tau"][0])) <= 2e-4          # each within a tolerance of the minimum
    assert abs(r["nll_after"] - fine["nll_after"]) <= 1e-8 and r["nll_after"] <= r["nll_before"]
    assert r["at_bound"] == [False]


@pytest.mark.parametrize("grid", [3, 4, 33])
def test_an_unreachable_tolerance_still_terminates(grid):
    """tol below fp64's spacing around ln tau: the bracket collapses to one value and the search ends"""
    z, y = planted([2.0], S=200, seed=7)
    ev = mean_nll_evaluator(z, y)
    r = fit_temperature(ev, 1, grid=grid, tol=1e-300)
    print(f"grid {grid}: {r['passes']} passes")
    assert r["passes"] <= 130                     # 6 / 2^-52 is under 2^56 halvings-or-moves at grid 3
    assert abs(np.log(r["tau"][0]) - np.log(fit_temperature(ev, 1)["tau"][0])) <= 2e-4


def test_an_argmin_on_a_bracket_end_moves_the_bracket():
    """an even grid does not contain the last argmin, so the best point can sit on the new bracket's end;
    the bracket then extends one spacing past it (clamped at the range, not at the bracket)"""
    seen = []

    def ev(beta):                                  # a parabola in u = -ln beta with its minimum at 1.234
        u = -np.log(beta[:, 0])
        seen.append((u.min(), u.max()))
        return (u - 1.234) ** 2
    for grid in (3, 4, 6, 33):
        r = fit_temperature(ev, 1, grid=grid, tol=1e-6)
        assert abs(np.log(r["tau"][0]) - 1.234) <= 1e-6, grid
    assert all(lo >= np.log(LO) - 1e-12 and hi <= np.log(HI) + 1e-12 for lo, hi in seen)


def test_evaluator_never_sees_more_than_grid_candidates():
    z, y = planted((0.7, 2.0), S=100, seed=5)
    seen = []

    def ev(beta):
        assert beta.dtype == np.float64 and beta.ndim == 2 and beta.shape[1] == 2 and (beta > 0).all()
        seen.append(beta.shape[0])
        return mean_nll_evaluator(z, y)(beta)
    r = fit_temperature(ev, 2, mode="per_member", grid=9)
    assert max(seen) <= 9 and len(seen) == r["passes"]


def test_json_round_trip(tmp_path):
    z, y = planted((0.7, 2.0), S=300, T=2, seed=3)
    sc = TemperatureScaler("per_member", grid=17)
    with pytest.raises(ValueError, match="nothing fitted"):
        sc.save(str(tmp_path / "none.json"))
    with pytest.raises(ValueError, match="no logits"):
        sc.fit()
    sc.result = fit_temperature(mean_nll_evaluator(z, y), 2, mode="per_member", grid=17)
    path = str(tmp_path / "fit.json")
    sc.save(path)

    def strict(c):
        raise AssertionError(f"not strict JSON: {c}")
    on_disk = json.loads(open(path).read(), parse_constant=strict)
    assert on_disk == sc.result
    back = TemperatureScaler.load(path)
    assert back.result == sc.result and back.mode == "per_member"
    assert back.inv_temp().dtype.is_floating_point and back.inv_temp().tolist() == sc.inv_temp().tolist()
    assert back.inv_temp().numpy().dtype == np.float32
    assert np.array_equal(back.inv_temp().numpy(), (1.0 / np.array(sc.result["tau"])).astype(np.float32))
    # a file with more keys (the entry point's calibration JSON) loads too; one with fewer does not
    json.dump(dict(on_disk, fit_phase="val", before={}, after={}), open(path, "w"))
    more = TemperatureScaler.load(path)
    assert more.result == sc.result and more.extra == dict(fit_phase="val", before={}, after={}) and back.extra == {}
    json.dump({k: v for k, v in on_disk.items() if k != "tau"}, open(path, "w"))
    with pytest.raises(ValueError, match="lacks"):
        TemperatureScaler.load(path)
    json.dump(dict(on_disk, tau=[1.0, -2.0]), open(path, "w"))
    with pytest.raises(ValueError, match="no valid fit"):
        TemperatureScaler.load(path)


REFUSALS = [
    (dict(mode="vector"), "mode must be one of"),
    (dict(grid=2), "grid = 2 must be 3 .. 64"),
    (dict(grid=65), "grid = 65 must be 3 .. 64"),
    (dict(grid=7.5), "grid = 7.5 must be"),
    (dict(tau_range=(0.0, 20.0)), "must be positive with low < high"),
    (dict(tau_range=(-1.0, 20.0)), "must be positive with low < high"),
    (dict(tau_range=(20.0, 0.05)), "must be positive with low < high"),
    (dict(tau_range=(2.0, 2.0)), "must be positive with low < high"),
    (dict(tau_range=(0.05, float("inf"))), "must be positive with low < high"),
    (dict(tau_range=(2.0, 20.0)), "must contain tau = 1"),
    (dict(tau_range=(0.05, 0.5)), "must contain tau = 1"),
    (dict(tau_range=3.0), "must be a .low, high. pair"),
    (dict(K=0), "K = 0 must be a positive integer"),
    (dict(K=-3), "K = -3 must be a positive integer"),
    (dict(tol=0.0), "tol = 0.0 must be positive"),
    (dict(max_rounds=0), "max_rounds = 0 must be a positive integer"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_fit_refuses(i):
    over, msg = REFUSALS[i]

    def never(beta):
        raise AssertionError("a refused fit called its evaluator")
    kw = dict(K=2)
    kw.update(over)
    with pytest.raises(ValueError, match="fit_temperature: .*" + msg):
        fit_temperature(never, kw.pop("K"), **kw)


def test_scaler_and_meter_refuse():
    import torch
    from src.uncertainty import UncertaintyMeter
    with pytest.raises(ValueError, match="mode must be one of"):
        TemperatureScaler("matrix")
    sc = TemperatureScaler()
    assert sc.mode == "shared" and sc.count == 0
    with pytest.raises(ValueError, match="layout"):
        sc.add(torch.zeros(3, 6, 10), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="layout"):
        sc.add(torch.zeros(2, 3, 4, 10), torch.zeros(4, dtype=torch.int64), layout="BKTC")
    with pytest.raises(ValueError, match="float32"):
        sc.add(torch.zeros(2, 3, 4, 10, dtype=torch.float64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"y must be \[S\] = \[4\]"):
        sc.add(torch.zeros(2, 3, 4, 10), torch.zeros(3, dtype=torch.int64))
    lo = torch.zeros(2, 3, 4, 10)
    sc.add(lo, torch.zeros(4, dtype=torch.int64))
    assert sc.count == 4 and sc.chunks[0][0].data_ptr() == lo.data_ptr()          # kept, not copied
    with pytest.raises(ValueError, match="3 members, the earlier chunks had 2"):
        sc.add(torch.zeros(3, 3, 4, 10), torch.zeros(4, dtype=torch.int64))
    sc.add(torch.zeros(5, 2, 3, 10), torch.zeros(5, dtype=torch.int64), layout="SKTC")
    assert sc.count == 9
    with pytest.raises(ValueError, match="nothing fitted"):
        sc.inv_temp()
    with pytest.raises(ValueError, match="inv_temp needs decompose=True"):
        UncertaintyMeter(15, inv_temp=torch.ones(2))
    m = UncertaintyMeter()
    assert (m.n_bins, m.decompose, m.inv_temp) == (15, False, None)


def test_reference_floors_and_ignores_labels_out_of_range():
    z = np.random.default_rng(2).standard_normal((3, 2, 2, 4)).astype(np.float32)
    y = np.array([1, 4, -1], dtype=np.int64)
    beta = np.array([[1.0, 1.0], [0.0, 0.0], [0.5, 3.0]])
    r = temperature_nll_ref(z, y, beta, np.float64)
    assert np.array_equal(r[1:], np.full((2, 3), -np.log(1e-12)))
    assert r[0, 1] == pytest.approx(np.log(4), abs=1e-15)
    e = np.exp(z[0].astype(np.float64))
    assert r[0, 0] == pytest.approx(-np.log((e[..., 1] / e.sum(-1)).mean()), abs=1e-13)


def parse(argv):
    import eval_robustness as E
    p = argparse.ArgumentParser()
    E.get_args(p)
    return p.parse_args(["--save_path", "out"] + argv)


def test_flags_parse_and_default():
    import eval_robustness as E
    a = parse([])
    assert a.calibrate is None and a.temperature is None and a.calibrate_phase == "val"
    a = parse(["--mmbt", "--calibrate", "per_member", "--calibrate_phase", "train", "--phase", "test"])
    assert (a.calibrate, a.calibrate_phase, a.phase, a.temperature) == ("per_member", "train", "test", None)
    assert parse(["--calibrate", "shared"]).calibrate == "shared"
    assert parse(["--temperature", "fit.json"]).temperature == "fit.json"
    with pytest.raises(SystemExit):
        parse(["--calibrate", "vector"])
    E.check_calibration_flags(parse(["--calibrate", "shared"]))
    E.check_calibration_flags(parse(["--temperature", "fit.json"]))
    with pytest.raises(ValueError, match="give one of them"):
        E.check_calibration_flags(parse(["--calibrate", "shared", "--temperature", "fit.json"]))
    assert [f for f, _ in E.FLAGS][-3:] == ["--calibrate", "--calibrate_phase", "--temperature"]
    assert E.CALIBRATION_KEYS == ("nll", "ece", "brier", "acc", "total", "mi")
