"""mmu_uncertainty_decompose_scaled (csrc/uncertainty.hip, the SCALED instantiation) on MI355X.

* Against fp64: the table of include/mmu.h with z_kt replaced by beta_k z_kt, per-member beta mixed from
  {0.25, 1, 4}, over C in {1, 65, 101, 1024} x (K, T) in {(1,1), (2,3), (5,30)} x S = 3 x scale in {1, 8} x
  both layouts.  The reference is test_uncertainty_decompose_gpu.py's `decompose_ref` on the scaled
  logits: in fp64 on the exact products (an f32 x f32 product is exact in fp64), and the yardstick is the
  same function in float32 on the f32 products.  The bar is 4 x that floor per column, the floor taken
  over this file's beta-mix sweep alone.  One cell deviates: `mi_passes` in the K = T = 1 cases is held
  to the `mi_passes` bar of test_uncertainty_decompose_gpu.py's sweep instead.  There numpy's value is
  H[p] - H[p] of one array, exactly 0 at either precision, so those cases add nothing to the floor, while
  the kernel forms the member entropy and the row entropy by two formulas, each good to an ulp or two of
  ln C; that arithmetic is the unscaled symbol's, which must keep its bits, and the unscaled sweep's bar
  is what it is already held to.  Measured on MI355X: 1.55e-6 at C = 1024, K = T = 1, beta = 0.25, against
  1.05e-6 from the mix cases and 9.5e-6 from the unscaled sweep.  `correct` and the votes are exact:
  scaling a row by beta > 0 moves no argmax, and the data has no near-ties (asserted while the sweep is
  built).
* Bitwise: on every case of the original sweep at S = 3, inv_temp=None, inv_temp=ones and
  mmu_uncertainty_decompose give the same bits in every output.
"""
import functools

import numpy as np
import pytest
import torch

from guarded import NAN, Guarded, check_written, out_buf
from test_uncertainty_decompose_gpu import (BAR_FACTOR, COLUMNS, CS, EXTRA, KTS, LAYOUTS, SCALES, compare,
                                            decompose_ref, make_logits, report)
from test_uncertainty_decompose_gpu import launch as launch_unscaled
from test_uncertainty_decompose_gpu import sweep as unscaled_sweep

pytestmark = pytest.mark.gpu

f32, i64 = torch.float32, torch.int64
S_CS = (1, 65, 101, 1024)
S_KTS = ((1, 1), (2, 3), (5, 30))
S_SCALES = (1, 8)
S = 3
BETAS = (0.25, 1.0, 4.0)


def member_betas(K, n):
    """K values from BETAS, a different mix per case, never all equal when K > 1"""
    return np.array([BETAS[(n + 2 * k) % 3] for k in range(K)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def sweep():
    """{"cases": {(C, K, T, scale): (z, y, beta, ref64)}, "floor": {column: max |f32 - fp64|}, "bar": 4 x floor}"""
    cases, floor = {}, {c: 0.0 for c in COLUMNS + EXTRA}
    for n, (C, (K, T), scale) in enumerate((C, kt, sc) for C in S_CS for kt in S_KTS for sc in S_SCALES):
        z, y = make_logits(C, K, T, S, scale, 7000 + n)
        beta = member_betas(K, n)
        b = beta[None, :, None, None]
        r64 = decompose_ref(z.astype(np.float64) * b.astype(np.float64), y, np.float64)
        r32 = decompose_ref(z * b, y, np.float32)
        assert r64["row_gap"] >= 1e-3 and r64["mean_gap"] >= 1e-4, (C, K, T, scale, r64["row_gap"], r64["mean_gap"])
        for c in floor:
            floor[c] = max(floor[c], float(np.abs(r32[c].astype(np.float64) - r64[c]).max()))
        cases[(C, K, T, scale)] = (z, y, beta, r64)
    return {"cases": cases, "floor": floor, "bar": {c: BAR_FACTOR * v for c, v in floor.items()}}


def launch(dev, z, y, beta, layout, member=True):
    """test_uncertainty_decompose_gpu.launch with an inverse-temperature vector (numpy [K], or None)"""
    from src import kernels as k
    Sn, K, T, C = z.shape
    shape = (K, T, Sn, C) if layout == "KTSC" else (Sn, K, T, C)
    gz = Guarded(dev, f32, NAN, int(np.prod(shape)))
    v = gz.view.view(*shape)
    v = v.permute(2, 0, 1, 3) if layout == "KTSC" else v
    v.copy_(torch.from_numpy(z))
    gz.set_canary()
    gy = Guarded(dev, i64, 85, Sn)
    gy.view.copy_(torch.from_numpy(y))
    gy.set_canary()
    gb = None
    if beta is not None:
        gb = Guarded(dev, f32, NAN, K)
        gb.view.copy_(torch.from_numpy(beta))
        gb.set_canary()
    outs = {"stats": out_buf(dev, f32, Sn, k.UNC_NSTAT), "p_bar": out_buf(dev, f32, Sn, C)}
    if member:
        outs["member_nll"] = out_buf(dev, f32, Sn, K)
    k.uncertainty_decompose(v, gy.view, outs["stats"][1], outs["p_bar"][1], outs["member_nll"][1] if member else None,
                            inv_temp=None if gb is None else gb.view)
    torch.cuda.synchronize()
    fails, tag = [], f"C={C} K={K} T={T} S={Sn} {layout} beta={beta}"
    check_written({n: g for n, (g, _) in outs.items()}, fails, tag)
    if not (gz.unchanged() and gy.unchanged() and (gb is None or gb.unchanged())):
        fails.append(f"{tag}: an input was written")
    st = outs["stats"][1].cpu().numpy()
    got = {c: st[:, i] for i, c in enumerate(k.UNC_COLUMNS)}
    got["p_bar"] = outs["p_bar"][1].cpu().numpy()
    if member:
        got["member_nll"] = outs["member_nll"][1].cpu().numpy()
    return got, fails


@pytest.mark.parametrize("C", S_CS)
def test_scaled_table_against_fp64(dev, C):
    sw = sweep()
    # the one exception (module docstring): mi_passes where numpy's own value is identically 0
    single = dict(sw["bar"], mi_passes=unscaled_sweep()["bar"]["mi_passes"])
    errs, fails = {}, []
    for (K, T) in S_KTS:
        for scale in S_SCALES:
            z, y, beta, r64 = sw["cases"][(C, K, T, scale)]
            for layout in LAYOUTS:
                got, f = launch(dev, z, y, beta, layout)
                fails += f
                compare({c: v.astype(np.float64) for c, v in got.items()}, r64, K, T, errs, fails,
                        f"C={C} K={K} T={T} scale={scale} beta={beta} {layout}",
                        single if (K, T) == (1, 1) else sw["bar"])
    report(f"scaled, C = {C}", errs, sw)
    assert not fails, "\n".join(fails[:20])


def test_scaling_changes_the_table(dev):
    """the scaled symbol is not the unscaled one in disguise: beta = 4 sharpens, beta = 0.25 flattens"""
    z, y, _, _ = sweep()["cases"][(101, 2, 3, 1)]
    base, _ = launch(dev, z, y, None, "KTSC")
    sharp, _ = launch(dev, z, y, np.full(2, 4.0, dtype=np.float32), "KTSC")
    flat, _ = launch(dev, z, y, np.full(2, 0.25, dtype=np.float32), "KTSC")
    assert (sharp["conf"] > base["conf"]).all() and (flat["conf"] < base["conf"]).all()
    assert (sharp["aleatoric"] < base["aleatoric"]).all() and (flat["aleatoric"] > base["aleatoric"]).all()
    zero, _ = launch(dev, z, y, np.zeros(2, dtype=np.float32), "KTSC")                 # beta = 0: uniform rows
    assert np.abs(zero["total"].astype(np.float64) - np.log(101)).max() <= unscaled_sweep()["bar"]["total"]


@pytest.mark.parametrize("C", CS)
def test_none_and_ones_are_bitwise_the_unscaled_kernel(dev, C):
    """every case of the original sweep at S = 3, both layouts: three calls, one set of bits"""
    usw = unscaled_sweep()
    for (K, T) in KTS:
        for scale in SCALES:
            z, y, _, _ = usw["cases"][(C, K, T, 3, scale)]
            for layout in LAYOUTS:
                old, f0 = launch_unscaled(dev, z, y, layout)
                none, f1 = launch(dev, z, y, None, layout)
                one, f2 = launch(dev, z, y, np.ones(K, dtype=np.float32), layout)
                assert not (f0 or f1 or f2), f0 + f1 + f2
                for c in none:
                    tag = f"C={C} K={K} T={T} scale={scale} {layout} {c}"
                    assert np.array_equal(none[c].view(np.int32), one[c].view(np.int32)), tag + ": None != ones"
                    assert np.array_equal(old[c], none[c].astype(np.float64)), tag + ": None != unscaled"
