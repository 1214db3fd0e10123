"""mmu_temperature_nll (csrc/calibration.hip) against fp64 on MI355X.

The reference is `calibration_ref.temperature_nll_ref`: the definition of include/mmu.h in numpy,
evaluated in fp64 on the same f32 logits and f32 inverse temperatures.  The tolerance is absolute:
4 x the largest error of the SAME function evaluated in float32 numpy against fp64 over the whole
sweep (`sweep()["floor"]`, computed on the CPU and never from the kernel) -- the margin
test_uncertainty_decompose_gpu.py and test_robustness_summary_gpu.py hold their kernels to.  Each test
prints the floor and the error it measured.

Sweep: C in {1, 2, 63, 64, 65, 101, 128, 129, 1024} x (K, T) in {(1,1), (3,1), (2,3), (5,30)} x
S in {1, 3, 5} x logit scale in {0, 1, 8, 80} x J in {1, 5, 64} x both layouts ([K, T, S, C] read in
place through its strides, contiguous [S, K, T, C]), one case with a padded pass stride, and one with
S = 257 (the cross-sample sum walks more than one stride per lane).  A case's table has 64 rows: 62
drawn log-uniform in [0.05, 20] per (j, k), a row of exact ones and a row of zeros; J = 5 launches
rows (0, 1, 2, ones, zeros) of it and J = 1 row 0, so one fp64 evaluation serves the three.  Labels:
make_logits' (the favourite class for even samples, a random class for odd ones), and the last sample
of every case has y = C: out of range, p_y = 0, nll = -ln 1e-12 exactly as f32.  Every tensor is a
view inside a tests/guarded.py buffer: inputs NaN-surrounded and unchanged afterwards, outputs
NaN-prefilled and fully written.
"""
import functools

import numpy as np
import pytest
import torch

from calibration_ref import temperature_nll_ref
from guarded import NAN, Guarded, check_written, out_buf
from test_uncertainty_decompose_gpu import make_logits

pytestmark = pytest.mark.gpu

f32, f64, i64 = torch.float32, torch.float64, torch.int64
CS = (1, 2, 63, 64, 65, 101, 128, 129, 1024)
KTS = ((1, 1), (3, 1), (2, 3), (5, 30))
SS = (1, 3, 5)
SCALES = (0, 1, 8, 80)
JS = (1, 5, 64)
LAYOUTS = ("KTSC", "SKTC")
BAR_FACTOR = 4.0
ROWS = {1: (0,), 5: (0, 1, 2, 62, 63), 64: tuple(range(64))}     # the rows of a case's table a J-launch takes
ONES, ZEROS = 62, 63
MANY = (101, 2, 3, 257, 1)                                        # the S = 257 case
NLL_FLOOR = np.float32(-np.log(np.float64(np.float32(1e-12))))    # -ln 1e-12 as f32
SUM_RTOL = 1e-12    # nll_sum against np.sum of the f64-cast column: an f64 reordering bound, not a measurement


def make_case(C, K, T, S, scale, seed):
    """(z f32 [S, K, T, C], y [S] with y[-1] = C, beta f32 [64, K])"""
    z, y = make_logits(C, K, T, S, scale, seed)
    y[-1] = C
    g = np.random.default_rng(seed + 50000)
    beta = np.exp(g.uniform(np.log(0.05), np.log(20.0), (64, K))).astype(np.float32)
    beta[ONES], beta[ZEROS] = 1.0, 0.0
    return z, y, beta


@functools.lru_cache(maxsize=None)
def sweep():
    """every case's logits, labels, table and fp64 result, computed once -> {"cases": {(C, K, T, S, scale):
    (z, y, beta, ref64 [S, 64])}, "floor": max |f32 - fp64| over the sweep, "bar": 4 x floor}"""
    keys = [(C, K, T, S, sc) for C in CS for (K, T) in KTS for S in SS for sc in SCALES] + [MANY]
    cases, floor = {}, 0.0
    for n, key in enumerate(keys):
        z, y, beta = make_case(*key, seed=3000 + n)
        r64, r32 = temperature_nll_ref(z, y, beta, np.float64), temperature_nll_ref(z, y, beta, np.float32)
        floor = max(floor, float(np.abs(r32.astype(np.float64) - r64).max()))
        cases[key] = (z, y, beta, r64)
    return {"cases": cases, "floor": floor, "bar": BAR_FACTOR * floor}


def launch(dev, z, y, beta, layout, ld=None, with_sum=True):
    """the kernel on z (numpy [S, K, T, C]) laid out as `layout` with class rows ld apart and the table
    beta [J, K], everything in guarded buffers -> (nll f32 [S, J], nll_sum f64 [J] or None, fails)"""
    from src import kernels as k
    S, K, T, C = z.shape
    J = beta.shape[0]
    ld = C if ld is None else ld
    shape = (K, T, S, ld) if layout == "KTSC" else (S, K, T, ld)
    gz = Guarded(dev, f32, NAN, int(np.prod(shape)))
    v = gz.view.view(*shape)[..., :C]
    v = v.permute(2, 0, 1, 3) if layout == "KTSC" else v
    v.copy_(torch.from_numpy(z))
    gz.set_canary()
    gy = Guarded(dev, i64, 85, S)
    gy.view.copy_(torch.from_numpy(y))
    gy.set_canary()
    gb = Guarded(dev, f32, NAN, J * K)
    gb.view.copy_(torch.from_numpy(np.ascontiguousarray(beta)).reshape(-1))
    gb.set_canary()
    outs = {"nll": out_buf(dev, f32, S, J)}
    if with_sum:
        outs["nll_sum"] = out_buf(dev, f64, J)
    k.temperature_nll(v, gy.view, gb.view.view(J, K), outs["nll"][1], outs["nll_sum"][1] if with_sum else None)
    torch.cuda.synchronize()
    fails, tag = [], f"C={C} K={K} T={T} S={S} J={J} {layout} ld={ld}"
    check_written({n: g for n, (g, _) in outs.items()}, fails, tag)
    if not (gz.unchanged() and gy.unchanged() and gb.unchanged()):
        fails.append(f"{tag}: an input was written")
    return outs["nll"][1].cpu().numpy(), outs["nll_sum"][1].cpu().numpy() if with_sum else None, fails


def compare(nll, nll_sum, r64, y, C, fails, tag, bar):
    """nll f32 [S, J] and its column sums vs the fp64 reference -> the largest error"""
    if not np.isfinite(nll).all():
        fails.append(f"{tag}: nll not finite")
    e = float(np.abs(nll.astype(np.float64) - r64).max())
    if e > bar:
        fails.append(f"{tag}: error {e:.3e} > bar {bar:.3e}")
    outside = (y < 0) | (y >= C)
    if not (nll[outside].view(np.int32) == NLL_FLOOR.view(np.int32)).all():
        fails.append(f"{tag}: an out-of-range label did not get -ln 1e-12 exactly")
    if nll_sum is not None:
        want = nll.astype(np.float64).sum(0)
        if (np.abs(nll_sum - want) > SUM_RTOL * np.abs(want)).any():
            fails.append(f"{tag}: nll_sum {nll_sum} != {want}")
    return e


@pytest.mark.parametrize("C", CS)
def test_sweep_against_fp64(dev, C):
    sw = sweep()
    worst, fails = 0.0, []
    for (K, T) in KTS:
        for S in SS:
            for scale in SCALES:
                z, y, beta, r64 = sw["cases"][(C, K, T, S, scale)]
                for J in JS:
                    rows = list(ROWS[J])
                    for layout in LAYOUTS:
                        nll, nll_sum, f = launch(dev, z, y, beta[rows], layout)
                        fails += f
                        worst = max(worst, compare(nll, nll_sum, r64[:, rows], y, C, fails,
                                                   f"C={C} K={K} T={T} S={S} scale={scale} J={J} {layout}", sw["bar"]))
    print(f"\nC = {C}: f32-numpy floor {sw['floor']:.3e}, bar {sw['bar']:.3e}, measured {worst:.3e}")
    assert not fails, "\n".join(fails[:20])


def test_padded_pass_stride(dev):
    """st > C: the class rows sit 101 + 7 apart and the padding holds NaN"""
    sw = sweep()
    z, y, beta, r64 = sw["cases"][(101, 2, 3, 3, 1)]
    worst, fails = 0.0, []
    for layout in LAYOUTS:
        nll, nll_sum, f = launch(dev, z, y, beta, layout, ld=108)
        fails += f
        worst = max(worst, compare(nll, nll_sum, r64, y, 101, fails, f"padded {layout}", sw["bar"]))
    print(f"\npadded pass stride: floor {sw['floor']:.3e}, bar {sw['bar']:.3e}, measured {worst:.3e}")
    assert not fails, "\n".join(fails)


def test_many_samples(dev):
    """S = 257: every lane of the cross-sample sum walks more than one stride (lane 0 five of them)"""
    sw = sweep()
    z, y, beta, r64 = sw["cases"][MANY]
    worst, fails = 0.0, []
    for J in JS:
        rows = list(ROWS[J])
        for layout in LAYOUTS:
            nll, nll_sum, f = launch(dev, z, y, beta[rows], layout)
            fails += f
            worst = max(worst, compare(nll, nll_sum, r64[:, rows], y, 101, fails, f"S=257 J={J} {layout}", sw["bar"]))
    print(f"\nS = 257: floor {sw['floor']:.3e}, bar {sw['bar']:.3e}, measured {worst:.3e}")
    assert not fails, "\n".join(fails)


def test_nll_sum_is_optional(dev):
    sw = sweep()
    z, y, beta, r64 = sw["cases"][(65, 3, 1, 3, 8)]
    nll, nll_sum, fails = launch(dev, z, y, beta[list(ROWS[5])], "KTSC", with_sum=False)
    assert nll_sum is None
    compare(nll, None, r64[:, list(ROWS[5])], y, 65, fails, "no nll_sum", sw["bar"])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", [(2, 3, 1, 3, 8), (101, 2, 3, 3, 1), (129, 5, 30, 5, 8), (1024, 5, 30, 3, 1)])
def test_beta_one_is_the_decomposition_nll(dev, case):
    """the row of exact ones against mmu_uncertainty_decompose's nll column on the same logits (in-range
    labels; the decomposition leaves labels outside [0, C) to its caller)"""
    from src import kernels as k
    sw = sweep()
    C, K, T, S, _ = case
    z, y, beta, _ = sw["cases"][case]
    y = np.where(y >= C, 0, y)
    nll, _, fails = launch(dev, z, y, beta[[ONES]], "KTSC")
    assert not fails, fails
    zd, yd = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    stats, p_bar = torch.empty(S, k.UNC_NSTAT, device=dev), torch.empty(S, C, device=dev)
    k.uncertainty_decompose(zd, yd, stats, p_bar)
    old = stats[:, k.UNC_COLUMNS.index("nll")].double().cpu().numpy()
    d = float(np.abs(nll[:, 0].astype(np.float64) - old).max())
    print(f"\n{case}: beta = 1 vs mmu_uncertainty_decompose nll {d:.3e} (bar {sw['bar']:.3e})")
    assert d <= sw["bar"]


def test_zero_inverse_temperature_is_ln_c(dev):
    """beta = 0: every row is uniform, so nll = ln C for every in-range label, whatever the logits"""
    sw = sweep()
    for C in (1, 65, 1024):
        z, y, beta, _ = sw["cases"][(C, 2, 3, 5, 80)]
        nll, _, fails = launch(dev, z, y, beta[[ZEROS]], "SKTC")
        assert not fails, fails
        assert np.abs(nll[:-1, 0].astype(np.float64) - np.log(C)).max() <= sw["bar"]


@pytest.mark.parametrize("case,layout", [((101, 2, 3, 3, 8), "KTSC"), ((1024, 5, 30, 3, 1), "SKTC"),
                                         ((63, 3, 1, 5, 80), "KTSC")])
def test_one_launch_equals_single_candidate_launches(dev, case, layout):
    """a candidate's figures do not depend on the other candidates of its launch: bitwise"""
    sw = sweep()
    z, y, beta, _ = sw["cases"][case]
    for J in (5, 64):
        rows = list(ROWS[J])
        nll, nll_sum, fails = launch(dev, z, y, beta[rows], layout)
        assert not fails, fails
        for n, r in enumerate(rows):
            one, one_sum, f = launch(dev, z, y, beta[[r]], layout)
            assert not f, f
            assert np.array_equal(one[:, 0].view(np.int32), nll[:, n].view(np.int32)), f"{case} J={J} row {r}"
            assert one_sum[0] == nll_sum[n]


@pytest.mark.parametrize("det", [False, True])
def test_bitwise_repeatable(dev, det):
    from src import kernels as k
    sw = sweep()
    for case, layout in (((1024, 5, 30, 5, 1), "KTSC"), ((101, 2, 3, 3, 8), "SKTC"), (MANY, "KTSC")):
        z, y, beta, _ = sw["cases"][case]
        with k.deterministic(det):
            a, asum, fa = launch(dev, z, y, beta, layout)
            b, bsum, fb = launch(dev, z, y, beta, layout)
        assert not fa and not fb
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(asum, bsum), \
            f"{case}: two launches differ (deterministic={det})"
        # and the mode itself changes nothing: one kernel serves both
        with k.deterministic(not det):
            c, csum, _ = launch(dev, z, y, beta, layout)
        assert np.array_equal(a.view(np.int32), c.view(np.int32)) and np.array_equal(asum, csum)
