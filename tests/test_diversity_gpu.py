"""mmu_ensemble_diversity (csrc/diversity.hip) against fp64 on MI355X.

The reference is tests/diversity_ref.py `diversity_ref`: the definitions of include/mmu.h restated in
numpy, evaluated in fp64 on the same f32 logits.

Sweep (`sweep()`): C in {1, 2, 5, 6, 63, 64, 65, 101, 128, 129, 1024} (5 / 6 straddle top) x (K, T) in
{(2, 1), (3, 1), (2, 3), (5, 30), (16, 1)} ((5, 30): a wave takes several rows and pairs; K = 16 at
C = 1024 is the LDS limit, above 64 KiB) x S in {1, 3} x logit scale in {0, 1, 8, 80} x muting on and off
at top = 5, plus the untruncated call (top = 0) where every class of the data is well separated: the
podium recipe at C in {2, 5, 6} (all classes are podium classes there), and `make_ladder` data of its
own at C in {65, 129} (with the recipe's Gaussian logits 1024 unkept probabilities come arbitrarily
close, and no precision orders them reliably).  Both layouts ([K, T, S, C] read in place through its
strides, contiguous [S, K, T, C]), plus one case with a padded class stride (101 + 7).  Every tensor is
a view inside a tests/guarded.py buffer: inputs NaN-surrounded and unchanged afterwards, outputs
sentinel-prefilled (tau may be NaN by definition, so NaN cannot mark "unwritten") and fully written.

Bars.
* js: absolute, 4 x the error of float32 numpy against fp64 over the whole sweep (`sweep()["floor"]`):
  the rule and the factor of test_robustness_summary_gpu.py.  Each test prints floor, bar and what it
  measured.
* member_arg, disagree, counts at scales {0, 1, 8}: equal to the fp64 reference exactly.  The builder
  asserts for every such case that float32 numpy and fp64 agree on all three, and that every ordering
  they rest on (neighbouring kept values, the two largest probabilities, the last kept against the
  first dropped) has a relative gap of at least MIN_GAP = 1e-2 or is an exact tie -- the kernel's f32
  sums run in another order than numpy's, and a few 1e-7 cannot bridge that.
* tau: the f32 rounding of the fp64 quotient of the reference's counts, NaN exactly where it is NaN;
  and, at every scale, the f32 rounding of the quotient of the counts the kernel itself wrote.
* scale 80 is not held to exact counts: in f32 exp(-240 ...) underflows to 0 where fp64 keeps 1e-100, so
  ties legitimately differ.  There: counts within [0, n0], conc + disc <= n0, tau in [-1, 1] or NaN.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from diversity_ref import diversity_ref, make_ladder, make_logits, member_probs, min_kept_gap, tau_b
from guarded import NAN, Guarded

pytestmark = pytest.mark.gpu

f32, i32, i64 = torch.float32, torch.int32, torch.int64
CS = (1, 2, 5, 6, 63, 64, 65, 101, 128, 129, 1024)
KTS = ((2, 1), (3, 1), (2, 3), (5, 30), (16, 1))
SS = (1, 3)
SCALES = (0, 1, 8, 80)
EXACT_SCALES = (0, 1, 8)
LAYOUTS = ("KTSC", "SKTC")
TOP = 5
TOP0_PODIUM = tuple((C, K, T) for C in (2, 5, 6) for K, T in ((3, 1), (2, 3)))
TOP0_LADDER = ((65, 3, 1), (65, 5, 30), (129, 3, 1), (129, 2, 3))
BAR_FACTOR = 4.0
MIN_GAP = 1e-2
SENTINEL = -7777
LN2 = float(np.log(2.0))


def same_f32(a, b):
    return np.array_equal(np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32), equal_nan=True)


def _add(cases, floor, key, z, y, top, mute, scale, p64, p32):
    r64 = diversity_ref(z, y, top, mute, np.float64, p=p64)
    r32 = diversity_ref(z, y, top, mute, np.float32, p=p32, with_counts=scale in EXACT_SCALES)
    if scale in EXACT_SCALES:
        for c in ("member_arg", "disagree", "counts"):
            assert np.array_equal(r32[c], r64[c]), (key, c)
        gap = min_kept_gap(r64, top)
        assert gap >= MIN_GAP, (key, gap)
        floor["gap"] = min(floor["gap"], gap)
    floor["js"] = max(floor["js"], float(np.abs(r32["js"].astype(np.float64) - r64["js"]).max()))
    cases[key] = (z, y, r64)


@functools.lru_cache(maxsize=None)
def sweep():
    """every case's logits, labels and fp64 result, computed once -> {"cases": {(C, K, T, S, scale, top,
    mute): (z, y, ref64)}, "floor": max |f32 - fp64| of js over the sweep, "bar": 4 x floor, "gap": the
    smallest relative gap an exact case rests on}"""
    cases, floor = {}, {"js": 0.0, "gap": np.inf}
    grid = ((C, K, T, S, sc) for C in CS for K, T in KTS for S in SS for sc in SCALES)
    for i, (C, K, T, S, scale) in enumerate(grid):
        z, y = make_logits(C, K, T, S, scale, 7000 + i, TOP)
        p64, p32 = member_probs(z, np.float64), member_probs(z, np.float32)
        tops = (TOP, 0) if (C, K, T) in TOP0_PODIUM else (TOP,)
        for top in tops:
            for mute in (True, False):
                _add(cases, floor, (C, K, T, S, scale, top, mute), z, y, top, mute, scale, p64, p32)
    for i, (C, K, T) in enumerate(TOP0_LADDER):
        z, y = make_ladder(C, K, T, 3, 9000 + i)
        p64, p32 = member_probs(z, np.float64), member_probs(z, np.float32)
        for mute in (True, False):
            _add(cases, floor, (C, K, T, 3, "ladder", 0, mute), z, y, 0, mute, 1, p64, p32)
    return {"cases": cases, "floor": floor["js"], "bar": BAR_FACTOR * floor["js"], "gap": floor["gap"]}


def launch(dev, z, y, layout, top, mute, ld=None, with_counts=True, three_d=False):
    """the kernel on z (numpy [S, K, T, C]) laid out as `layout` with class rows ld apart, everything in
    guarded buffers -> ({"js" / "disagree" / "tau" [S, P], "counts" [S, P, 4], "member_arg" [S, K]}, fails)"""
    from src import kernels as k
    S, K, T, C = z.shape
    P = K * (K - 1) // 2
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
    outs = {"pair": Guarded(dev, f32, float(SENTINEL), S * P * k.DIV_NPAIR),
            "member_arg": Guarded(dev, i32, SENTINEL, S * K)}
    if with_counts:
        outs["counts"] = Guarded(dev, i32, SENTINEL, S * P * 4)
    if three_d:
        assert T == 1
        v = v[:, :, 0]
    k.ensemble_diversity(v, gy.view, outs["pair"].view.view(S, P, k.DIV_NPAIR),
                         outs["counts"].view.view(S, P, 4) if with_counts else None,
                         outs["member_arg"].view.view(S, K), top=top, mute_true=mute)
    torch.cuda.synchronize()
    fails, tag = [], f"C={C} K={K} T={T} S={S} {layout} ld={ld} top={top} mute={mute}"
    for name, g in outs.items():
        if not g.guards_intact():
            fails.append(f"{tag} {name}: a guard element was written")
        if bool((g.view == SENTINEL).any()):
            fails.append(f"{tag} {name}: an element was left unwritten")
    if not (gz.unchanged() and gy.unchanged()):
        fails.append(f"{tag}: an input was written")
    pair = outs["pair"].view.view(S, P, k.DIV_NPAIR).double().cpu().numpy()
    got = {c: pair[:, :, i] for i, c in enumerate(k.DIV_COLUMNS)}
    got["pair_bits"] = outs["pair"].view.view(torch.int32).cpu().numpy().copy()
    got["member_arg"] = outs["member_arg"].view.view(S, K).cpu().numpy().astype(np.int64)
    if with_counts:
        got["counts"] = outs["counts"].view.view(S, P, 4).cpu().numpy().astype(np.int64)
    return got, fails


def compare(got, r64, C, exact, errs, fails, tag, bar):
    """got vs the fp64 reference: the js error into errs, everything else into fails"""
    n0 = C * (C - 1) // 2
    if not np.isfinite(got["js"]).all():
        fails.append(f"{tag} js: not finite")
    e = float(np.abs(got["js"] - r64["js"]).max())
    errs["js"] = max(errs.get("js", 0.0), e)
    if e > bar:
        fails.append(f"{tag} js: error {e:.3e} > bar {bar:.3e}")
    if got["js"].min() < -bar or got["js"].max() > LN2 + bar:
        fails.append(f"{tag}: js outside [-bar, ln 2 + bar]")
    if not np.isin(got["disagree"], (0.0, 1.0)).all():
        fails.append(f"{tag} disagree: neither 0 nor 1")
    cn = got["counts"]
    own = np.array([[tau_b(cn[s, q], C) for q in range(cn.shape[1])] for s in range(cn.shape[0])])
    if not same_f32(got["tau"], own):
        fails.append(f"{tag} tau: not the f32 rounding of the quotient of the kernel's own counts")
    if cn.min() < 0 or cn.max() > n0 or (cn[..., 0] + cn[..., 1]).max() > n0:
        fails.append(f"{tag} counts: outside [0, n0 = {n0}]")
    t = got["tau"][np.isfinite(got["tau"])]
    if np.isinf(got["tau"]).any() or (t.size and (t.min() < -1.0 or t.max() > 1.0)):
        fails.append(f"{tag} tau: outside [-1, 1]")
    if exact:
        for c in ("member_arg", "disagree", "counts"):
            if not np.array_equal(got[c], r64[c]):
                fails.append(f"{tag} {c}: differs from the reference")
        if not same_f32(got["tau"], r64["tau"]):
            fails.append(f"{tag} tau: differs from the f32 rounding of the reference")


def report(what, errs, sw):
    print(f"\n{what}: js f32-numpy floor {sw['floor']:.3e}, bar {sw['bar']:.3e}, measured {errs.get('js', 0.0):.3e}; "
          f"smallest relative gap of an exact case {sw['gap']:.3f}")


def test_the_columns_are_the_headers(dev):
    from src import kernels as k
    assert k.DIV_COLUMNS == ("js", "disagree", "tau") and k.DIV_NPAIR == 3


@pytest.mark.parametrize("C", CS)
def test_sweep_against_fp64(dev, C):
    sw = sweep()
    errs, fails = {}, []
    for (c, K, T, S, scale, top, mute), (z, y, r64) in sw["cases"].items():
        if c != C:
            continue
        for layout in LAYOUTS:
            got, f = launch(dev, z, y, layout, top, mute)
            fails += f
            compare(got, r64, C, scale != 80, errs, fails,
                    f"C={C} K={K} T={T} S={S} scale={scale} top={top} mute={mute} {layout}", sw["bar"])
    report(f"C = {C}", errs, sw)
    assert not fails, "\n".join(fails[:20])


def test_padded_class_stride(dev):
    """class rows 101 + 7 apart, the padding holds NaN"""
    sw = sweep()
    errs, fails = {}, []
    for layout in LAYOUTS:
        for case in ((101, 3, 1, 3, 1, TOP, True), (101, 5, 30, 3, 8, TOP, False)):
            z, y, r64 = sw["cases"][case]
            got, f = launch(dev, z, y, layout, case[5], case[6], ld=108)
            fails += f
            compare(got, r64, 101, True, errs, fails, f"padded {case} {layout}", sw["bar"])
    report("padded class stride", errs, sw)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", CS)
def test_equal_logits(dev, C):
    """scale 0: every row an exact tie, so no divergence, no disagreement, every argmax 0 and every class
    kept; muting (the labels are in range) leaves one class below C - 1 equal ones, tau = 1 exactly for
    C >= 2 and NaN at C = 1; without muting x is constant and tau is NaN"""
    sw = sweep()
    for K, T in KTS:
        for mute in (True, False):
            z, y, _ = sw["cases"][(C, K, T, 3, 0, TOP, mute)]
            assert ((y >= 0) & (y < C)).all()
            got, fails = launch(dev, z, y, "KTSC", TOP, mute)
            assert not fails, fails
            assert np.abs(got["js"]).max() <= sw["bar"]
            assert not got["disagree"].any() and not got["member_arg"].any()
            if mute and C >= 2:
                assert np.array_equal(got["tau"], np.ones_like(got["tau"])), (C, K, T)
            else:
                assert np.isnan(got["tau"]).all(), (C, K, T, mute)


@pytest.mark.parametrize("case", [(1, 2, 3, 3, 1), (6, 3, 1, 3, 8), (65, 5, 30, 3, 1), (1024, 3, 1, 3, 8)])
def test_labels_outside_the_classes(dev, case):
    """y = -1 and y = C: nothing is muted for those samples, the guards stay intact, and the sample
    between them is as the reference has it"""
    sw = sweep()
    C = case[0]
    z, y, _ = sw["cases"][case + (TOP, True)]
    y = y.copy()
    y[0], y[2] = -1, C
    r64 = diversity_ref(z, y, TOP, True, np.float64)
    unmuted = diversity_ref(z, y, TOP, False, np.float64)
    for s in (0, 2):
        assert np.array_equal(r64["counts"][s], unmuted["counts"][s])
    for layout in LAYOUTS:
        got, fails = launch(dev, z, y, layout, TOP, True)
        compare(got, r64, C, True, {}, fails, f"{case} {layout}", sw["bar"])
        assert not fails, "\n".join(fails)


def test_counts_are_optional(dev):
    sw = sweep()
    for case in ((65, 5, 30, 3, 8, TOP, True), (1024, 16, 1, 3, 1, TOP, False), (6, 2, 3, 1, 1, 0, True)):
        z, y, _ = sw["cases"][case]
        a, fa = launch(dev, z, y, "KTSC", case[5], case[6])
        b, fb = launch(dev, z, y, "KTSC", case[5], case[6], with_counts=False)
        assert not fa and not fb, fa + fb
        assert "counts" not in b
        assert np.array_equal(a["pair_bits"], b["pair_bits"]) and np.array_equal(a["member_arg"], b["member_arg"])


@pytest.mark.parametrize("case", [(2, 2, 1, 3, 8), (101, 16, 1, 3, 1), (129, 3, 1, 1, 80), (1024, 3, 1, 3, 8)])
def test_three_d_stack_is_the_one_pass_call(dev, case):
    """T = 1: the [S, K, C] call equals the [S, K, 1, C] call bitwise, in both layouts"""
    z, y, _ = sweep()["cases"][case + (TOP, True)]
    for layout in LAYOUTS:
        a, fa = launch(dev, z, y, layout, TOP, True)
        b, fb = launch(dev, z, y, layout, TOP, True, three_d=True)
        assert not fa and not fb, fa + fb
        for c in ("pair_bits", "counts", "member_arg"):
            assert np.array_equal(a[c], b[c]), f"{case} {layout} {c}"


@pytest.mark.parametrize("det", [False, True])
def test_bitwise_repeatable(dev, det):
    from src import kernels as k
    sw = sweep()
    for case, layout in (((1024, 16, 1, 3, 1, TOP, True), "KTSC"), ((101, 5, 30, 3, 8, TOP, False), "SKTC"),
                         ((63, 2, 3, 1, 80, TOP, True), "KTSC")):
        z, y, _ = sw["cases"][case]
        with k.deterministic(det):
            a, fa = launch(dev, z, y, layout, case[5], case[6])
            b, fb = launch(dev, z, y, layout, case[5], case[6])
        assert not fa and not fb
        with k.deterministic(not det):   # and the mode itself changes nothing: one kernel serves both
            c2, _ = launch(dev, z, y, layout, case[5], case[6])
        for c in ("pair_bits", "counts", "member_arg"):
            assert np.array_equal(a[c], b[c]), f"{case} {c}: two launches differ (deterministic={det})"
            assert np.array_equal(a[c], c2[c]), f"{case} {c}: the modes differ"


@pytest.mark.parametrize("case", [(101, 5, 30, 3, 1), (1024, 3, 1, 3, 8), (64, 2, 3, 3, 80)])
def test_js_is_the_robustness_summary_js(dev, case):
    """js of a pair against mmu_robustness_summary's js of the same two distributions: member i's T rows as
    the heads of variant 0, member j's as variant 1 (variants 2 .. 4 repeat variant 0), within this
    file's bar plus that kernel's own (test_robustness_summary_gpu.py)"""
    from src import kernels as k
    from test_robustness_summary_gpu import sweep as rob_sweep
    sw = sweep()
    bar = sw["bar"] + rob_sweep()["bar"]["js"]
    z, y, _ = sw["cases"][case + (TOP, True)]
    S, K, T, C = z.shape
    got, fails = launch(dev, z, y, "SKTC", TOP, True)
    assert not fails, fails
    worst = 0.0
    for q, (i, j) in enumerate(itertools.combinations(range(K), 2)):
        stack = np.stack([z[:, i], z[:, j], z[:, i], z[:, i], z[:, i]], axis=1)          # [S, V = 5, T, C]
        lo = torch.from_numpy(np.ascontiguousarray(stack)).to(dev)
        stats = torch.empty(S, k.ROB_NSTAT, dtype=f32, device=dev)
        k.robustness_summary(lo, torch.from_numpy(y).to(dev), stats)
        rob = stats[:, k.ROB_COLUMNS.index("js_image")].double().cpu().numpy()
        worst = max(worst, float(np.abs(rob - got["js"][:, q]).max()))
    print(f"\n{case}: |js - robustness js| {worst:.3e}, bar {bar:.3e}")
    assert worst <= bar
