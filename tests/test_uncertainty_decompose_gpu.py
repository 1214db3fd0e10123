"""mmu_uncertainty_decompose (csrc/uncertainty.hip) against fp64 on MI355X.

The reference is `decompose_ref`: the table of include/mmu.h restated in numpy, evaluated in fp64 on
the same f32 logits.  The tolerance is absolute and per column: 4 x the error of the SAME function
evaluated in float32 numpy against fp64, taken over the whole sweep (`sweep()["floor"]`) -- a kernel
may sum in another order but has no business being further off than that.  Each test prints the
floor and the error it measured.

Sweep: C in {1, 2, 63, 64, 65, 101, 128, 129, 1024} x (K, T) in {(1,1), (3,1), (2,3), (5,30)} x
S in {1, 3, 5} x logit scale in {0, 1, 8, 80} (0: all-equal logits; 80: near-one-hot rows, the
0 ln 0 case) x both layouts ([K, T, S, C] read in place through its strides, contiguous
[S, K, T, C]), plus one case with a padded pass stride (st > C).  Every tensor is a view inside a
tests/guarded.py buffer: inputs NaN-surrounded and unchanged afterwards, outputs NaN-prefilled.

The data has no near-ties (`make_logits` lifts every row's top logit; `sweep()` asserts a top-two
gap >= 1e-3 in probability for every row and >= 1e-4 for the mean) except at scale 0, where every
row is an exact tie and the rule "lowest class" decides; so `correct` and the row votes must equal
the reference exactly.
"""
import functools

import numpy as np
import pytest
import torch

from guarded import NAN, Guarded, check_written, out_buf

pytestmark = pytest.mark.gpu

f32, i64 = torch.float32, torch.int64
CS = (1, 2, 63, 64, 65, 101, 128, 129, 1024)
KTS = ((1, 1), (3, 1), (2, 3), (5, 30))
SS = (1, 3, 5)
SCALES = (0, 1, 8, 80)
LAYOUTS = ("KTSC", "SKTC")
COLUMNS = ("total", "aleatoric", "mi_members", "mi_passes", "brier", "nll", "conf", "correct", "vote_disagreement")
EXTRA = ("p_bar", "member_nll")
BAR_FACTOR = 4.0


def xlogx(q):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(q > 0, q * np.log(q), q.dtype.type(0))


def decompose_ref(z, y, dt):
    """include/mmu.h's table at precision dt.  z f32 [S, K, T, C], y [S] -> {column: [S]}, "p_bar" [S, C],
    "member_nll" [S, K], and the integers behind two columns: "argmax" [S], "votes" [S] (largest count)"""
    S, K, T, C = z.shape
    z = z.astype(dt)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)                         # p_kt
    pk = p.mean(2, dtype=dt)                                  # mean over the passes
    pb = pk.mean(1, dtype=dt)                                 # mean over the members
    H = lambda q: -xlogx(q).sum(-1, dtype=dt)                 # noqa: E731
    total, hk, alea = H(pb), H(pk).mean(1, dtype=dt), H(p).mean((1, 2), dtype=dt)
    rows = np.arange(S)
    onehot = np.zeros((S, C), dtype=dt)
    onehot[rows, y] = 1
    floor = dt(1e-12)
    arg = pb.argmax(-1)
    rowarg = p.argmax(-1).reshape(S, K * T)
    votes = np.array([np.bincount(r, minlength=C).max() for r in rowarg])
    return {"total": total, "aleatoric": alea, "mi_members": total - hk, "mi_passes": hk - alea,
            "brier": ((pb - onehot) ** 2).sum(-1, dtype=dt), "nll": -np.log(np.maximum(pb[rows, y], floor)),
            "conf": pb.max(-1), "correct": (arg == y).astype(dt),
            "vote_disagreement": dt(1) - votes.astype(dt) / dt(K * T), "p_bar": pb,
            "member_nll": -np.log(np.maximum(pk[rows, :, y], floor)), "argmax": arg, "votes": votes,
            "row_gap": top_two_gap(p), "mean_gap": top_two_gap(pb)}


def top_two_gap(p):
    if p.shape[-1] == 1:
        return np.inf
    top = np.sort(p, axis=-1)[..., -2:]
    return float((top[..., 1] - top[..., 0]).min())


def make_logits(C, K, T, S, scale, seed):
    """f32 [S, K, T, C]: a per-sample pattern that the members and passes perturb.  Every row has a
    winner 3 (x scale) above its other logits, so no row is a near-tie: the sample's favourite class, or
    in fewer than half of the sample's K * T rows another class -- the favourite keeps a strict plurality
    of the votes, so the mean has no tie either, however one-hot the rows are.  Labels: the favourite
    for even samples, a random class for odd ones."""
    g = np.random.default_rng(seed)
    R = K * T
    z = (g.standard_normal((S, 1, 1, C)) + 0.7 * g.standard_normal((S, K, 1, C))
         + 0.5 * g.standard_normal((S, K, T, C))).reshape(S, R, C)
    fav = g.integers(0, C, S)
    for s in range(S):
        win = np.full(R, fav[s])
        if C > 1:
            dissent = g.choice(R, g.integers(0, (R - 1) // 2 + 1), replace=False)
            win[dissent] = (fav[s] + g.integers(1, C, dissent.size)) % C
        z[s, np.arange(R), win] = z[s].max(-1) + 3.0
    z = (z * scale).astype(np.float32).reshape(S, K, T, C)
    y = np.where(np.arange(S) % 2 == 0, fav, g.integers(0, C, S)).astype(np.int64)
    return z, y


@functools.lru_cache(maxsize=None)
def sweep():
    """every case's logits, labels, fp64 and f32 results, computed once -> {"cases": {(C, K, T, S, scale):
    (z, y, ref64, ref32)}, "floor": {column: max |f32 - fp64| over the sweep}, "bar": 4 x floor}"""
    cases, floor = {}, {c: 0.0 for c in COLUMNS + EXTRA}
    for n, (C, (K, T), S, scale) in enumerate((C, kt, S, sc) for C in CS for kt in KTS for S in SS for sc in SCALES):
        z, y = make_logits(C, K, T, S, scale, 1000 + n)
        r64, r32 = decompose_ref(z, y, np.float64), decompose_ref(z, y, np.float32)
        if scale:
            assert r64["row_gap"] >= 1e-3 and r64["mean_gap"] >= 1e-4, (C, K, T, S, scale, r64["row_gap"],
                                                                        r64["mean_gap"])
        for c in floor:
            floor[c] = max(floor[c], float(np.abs(r32[c].astype(np.float64) - r64[c]).max()))
        cases[(C, K, T, S, scale)] = (z, y, r64, r32)
    return {"cases": cases, "floor": floor, "bar": {c: BAR_FACTOR * v for c, v in floor.items()}}


def launch(dev, z, y, layout, ld=None, member=True):
    """the kernel on z (numpy [S, K, T, C]) laid out as `layout` with class rows ld apart, everything in
    guarded buffers -> ({column / "p_bar" / "member_nll": numpy}, fails)"""
    from src import kernels as k
    S, K, T, C = z.shape
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
    outs = {"stats": out_buf(dev, f32, S, k.UNC_NSTAT), "p_bar": out_buf(dev, f32, S, C)}
    if member:
        outs["member_nll"] = out_buf(dev, f32, S, K)
    k.uncertainty_decompose(v, gy.view, outs["stats"][1], outs["p_bar"][1], outs["member_nll"][1] if member else None)
    torch.cuda.synchronize()
    fails, tag = [], f"C={C} K={K} T={T} S={S} {layout} ld={ld}"
    check_written({n: g for n, (g, _) in outs.items()}, fails, tag)
    if not (gz.unchanged() and gy.unchanged()):
        fails.append(f"{tag}: an input was written")
    st = outs["stats"][1].double().cpu().numpy()
    got = {c: st[:, i] for i, c in enumerate(k.UNC_COLUMNS)}
    got["p_bar"] = outs["p_bar"][1].double().cpu().numpy()
    if member:
        got["member_nll"] = outs["member_nll"][1].double().cpu().numpy()
    return got, fails


def compare(got, r64, K, T, errs, fails, tag, bar):
    """got vs the fp64 reference: per-column error into errs, the exact properties into fails"""
    for c in got:
        if not np.isfinite(got[c]).all():
            fails.append(f"{tag} {c}: not finite")
        e = float(np.abs(got[c] - r64[c]).max())
        errs[c] = max(errs.get(c, 0.0), e)
        if e > bar[c]:
            fails.append(f"{tag} {c}: error {e:.3e} > bar {bar[c]:.3e}")
    if not np.array_equal(got["correct"], r64["correct"]):
        fails.append(f"{tag}: correct differs from the reference")
    if not np.array_equal(np.rint((1.0 - got["vote_disagreement"]) * (K * T)).astype(np.int64), r64["votes"]):
        fails.append(f"{tag}: the largest vote count differs from the reference")
    if np.abs(got["p_bar"].sum(-1) - 1.0).max() > 1e-5:
        fails.append(f"{tag}: p_bar rows do not sum to 1")
    for c in ("mi_members", "mi_passes"):
        if got[c].min() < -bar[c]:
            fails.append(f"{tag} {c}: {got[c].min():.3e} < -bar (Jensen)")


def report(what, errs, sw):
    print(f"\n{what}: column, f32-numpy floor, bar, measured")
    for c in errs:
        print(f"  {c:18s} {sw['floor'][c]:.3e} {sw['bar'][c]:.3e} {errs[c]:.3e}")


def test_the_columns_are_the_headers(dev):
    from src import kernels as k
    assert k.UNC_COLUMNS == COLUMNS and k.UNC_NSTAT == 9


@pytest.mark.parametrize("C", CS)
def test_sweep_against_fp64(dev, C):
    sw = sweep()
    errs, fails = {}, []
    for (K, T) in KTS:
        for S in SS:
            for scale in SCALES:
                z, y, r64, _ = sw["cases"][(C, K, T, S, scale)]
                for layout in LAYOUTS:
                    got, f = launch(dev, z, y, layout)
                    fails += f
                    compare(got, r64, K, T, errs, fails, f"C={C} K={K} T={T} S={S} scale={scale} {layout}", sw["bar"])
    report(f"C = {C}", errs, sw)
    assert not fails, "\n".join(fails[:20])


def test_padded_pass_stride(dev):
    """st > C: the class rows sit 101 + 7 apart and the padding holds NaN"""
    sw = sweep()
    errs, fails = {}, []
    for layout in LAYOUTS:
        z, y, r64, _ = sw["cases"][(101, 2, 3, 3, 1)]
        got, f = launch(dev, z, y, layout, ld=108)
        fails += f
        compare(got, r64, 2, 3, errs, fails, f"padded {layout}", sw["bar"])
    report("padded pass stride", errs, sw)
    assert not fails, "\n".join(fails)


def test_member_nll_is_optional(dev):
    sw = sweep()
    z, y, r64, _ = sw["cases"][(65, 3, 1, 3, 8)]
    got, fails = launch(dev, z, y, "KTSC", member=False)
    compare(got, r64, 3, 1, {}, fails, "no member_nll", sw["bar"])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", CS)
def test_equal_logits(dev, C):
    """scale 0: total = aleatoric = ln C, no mutual information, conf = 1 / C, class 0 wins every vote"""
    sw = sweep()
    bar = sw["bar"]
    for (K, T) in KTS:
        z, y, _, _ = sw["cases"][(C, K, T, 3, 0)]
        got, fails = launch(dev, z, y, "KTSC")
        assert not fails, fails
        assert np.abs(got["total"] - np.log(C)).max() <= bar["total"]
        assert np.abs(got["aleatoric"] - np.log(C)).max() <= bar["aleatoric"]
        assert np.abs(got["mi_members"]).max() <= bar["mi_members"]
        assert np.abs(got["mi_passes"]).max() <= bar["mi_passes"]
        assert np.abs(got["conf"] - 1.0 / C).max() <= bar["conf"]
        assert np.array_equal(got["correct"], (y == 0).astype(np.float64))      # argmax = class 0
        assert np.array_equal(got["vote_disagreement"], np.zeros(3))


@pytest.mark.parametrize("C", CS)
def test_single_member_single_pass(dev, C):
    """K = T = 1: nothing to disagree about, and the one member's NLL is the ensemble's"""
    sw = sweep()
    bar = sw["bar"]
    for scale in SCALES:
        z, y, _, _ = sw["cases"][(C, 1, 1, 5, scale)]
        got, fails = launch(dev, z, y, "SKTC")
        assert not fails, fails
        assert np.abs(got["mi_members"]).max() <= bar["mi_members"]
        assert np.abs(got["mi_passes"]).max() <= bar["mi_passes"]
        assert np.array_equal(got["member_nll"][:, 0], got["nll"])
        assert np.array_equal(got["vote_disagreement"], np.zeros(5))


@pytest.mark.parametrize("case", [(2, 3, 1, 1, 8), (101, 2, 3, 3, 1), (129, 5, 30, 5, 8), (1024, 5, 30, 3, 1)])
def test_agrees_with_mmu_uncertainty(dev, case):
    """p_bar / nll / conf / correct of the existing kernel on the same logits ([S, K * T, C] contiguous)"""
    from src import kernels as k
    sw = sweep()
    bar = sw["bar"]
    C, K, T, S, _ = case
    z, y, _, _ = sw["cases"][case]
    got, fails = launch(dev, z, y, "KTSC")
    assert not fails, fails
    zd, yd = torch.from_numpy(z).to(dev).reshape(S, K * T, C).contiguous(), torch.from_numpy(y).to(dev)
    pb = torch.empty(S, C, device=dev)
    nll, conf, cor = (torch.empty(S, device=dev) for _ in range(3))
    k.uncertainty(zd, yd, pb, nll, conf, cor)
    d = {"p_bar": np.abs(pb.double().cpu().numpy() - got["p_bar"]).max(),
         "nll": np.abs(nll.double().cpu().numpy() - got["nll"]).max(),
         "conf": np.abs(conf.double().cpu().numpy() - got["conf"]).max()}
    print(f"\n{case}: vs mmu_uncertainty " + " ".join(f"{c} {v:.3e} (bar {bar[c]:.3e})" for c, v in d.items()))
    assert np.array_equal(cor.double().cpu().numpy(), got["correct"])
    for c, v in d.items():
        assert v <= bar[c], f"{c}: {v:.3e} > bar {bar[c]:.3e}"


@pytest.mark.parametrize("det", [False, True])
def test_bitwise_repeatable(dev, det):
    from src import kernels as k
    sw = sweep()
    for case, layout in (((1024, 5, 30, 5, 1), "KTSC"), ((101, 2, 3, 3, 8), "SKTC"), ((63, 3, 1, 1, 80), "KTSC")):
        z, y, _, _ = sw["cases"][case]
        with k.deterministic(det):
            a, fa = launch(dev, z, y, layout)
            b, fb = launch(dev, z, y, layout)
        assert not fa and not fb
        for c in a:
            assert np.array_equal(a[c], b[c]), f"{case} {c}: two launches differ (deterministic={det})"
    # and the mode itself changes nothing: one kernel serves both
    with k.deterministic(not det):
        c2, _ = launch(dev, z, y, layout)
    for c in a:
        assert np.array_equal(a[c], c2[c])
