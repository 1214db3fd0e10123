"""mmu_robustness_summary (csrc/robustness.hip) against fp64 on MI355X.

The reference is `summary_ref`: the table of include/mmu.h restated in numpy, evaluated in fp64 on the
same f32 logits.  The tolerance is absolute and per column: 4 x the error of the SAME function
evaluated in float32 numpy against fp64, taken over the whole sweep (`sweep()["floor"]`), the rule and
the factor of test_uncertainty_decompose_gpu.py.  Each test prints the floor and the error it measured.

Sweep: C in {1, 2, 63, 64, 65, 101, 128, 129, 1024} x n in {1, 2, 3, 20} (V = 5, 7, 9, 43; V = 5 is
the smallest shape in which a wave takes a second variant, n = 1 makes both std columns exactly 0) x
K in {1, 2, 5} x S in {1, 3} x logit scale in {0, 1, 8, 80} x both layouts ([V, S, K, C] read in place
through its strides, contiguous [S, V, K, C]), plus one case with a padded class stride.  Every tensor
is a view inside a tests/guarded.py buffer: inputs NaN-surrounded and unchanged afterwards, outputs
NaN-prefilled and fully written.

Data (`make_logits`): a per-sample pattern plus per-variant and per-head noise; every (sample, variant)
has one winner class shared by its heads, lifted 3 (x scale) above every other logit of those rows, so
the top-two gap of the head-mean logits is 3 x scale (less the f32 rounding of the logits) and float32
and fp64 agree on every hit: hit_*, acc_*_control and the hit plane must equal the reference exactly.
At scale 0 every row is an exact tie and class 0 wins.
"""
import functools

import numpy as np
import pytest
import torch

from guarded import NAN, Guarded, check_written, out_buf

pytestmark = pytest.mark.gpu

f32, i64 = torch.float32, torch.int64
CS = (1, 2, 63, 64, 65, 101, 128, 129, 1024)
NS = (1, 2, 3, 20)
KS = (1, 2, 5)
SS = (1, 3)
SCALES = (0, 1, 8, 80)
LAYOUTS = ("VSKC", "SVKC")
COLUMNS = ("p_full", "dp_image", "dp_image_control", "sd_image_control", "dp_text", "dp_text_control",
           "sd_text_control", "js_image", "js_image_control", "js_text", "js_text_control", "hit_full", "hit_image",
           "hit_text", "acc_image_control", "acc_text_control")
PLANES = ("p_label", "js", "hit")
EXACT = ("hit_full", "hit_image", "hit_text", "acc_image_control", "acc_text_control", "hit")
BAR_FACTOR = 4.0
LN2 = float(np.log(2.0))


def same_f32(a, b):
    """equal once both are rounded to float32, the precision the kernel stores: a hit is 0 or 1, a control
    accuracy the correctly rounded quotient of an integer by n"""
    return np.array_equal(np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32))


def xlogx(q):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(q > 0, q * np.log(q), q.dtype.type(0))


def summary_ref(z, y, dt):
    """include/mmu.h's table at precision dt.  z f32 [S, V, K, C], y [S] (any integers) -> {column: [S]},
    the planes "p_label" / "js" / "hit" [S, V], and "gap": the smallest top-two gap of the head-mean logits"""
    S, V, K, C = z.shape
    n = (V - 3) // 2
    z = z.astype(dt)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = (e / e.sum(-1, keepdims=True)).mean(2, dtype=dt)                  # p_v [S, V, C]
    zm = z.mean(2, dtype=dt)                                              # head-mean logits
    inside = (y >= 0) & (y < C)
    yc = np.where(inside, y, 0)
    rows = np.arange(S)
    p_label = np.where(inside[:, None], p[rows, :, yc], dt(0))
    hit = ((zm.argmax(-1) == y[:, None]) & inside[:, None]).astype(dt)
    H = lambda q: -xlogx(q).sum(-1, dtype=dt)                             # noqa: E731
    m = (p + p[:, :1]) / dt(2)
    js = H(m) - (H(p) + H(p[:, :1])) / dt(2)
    dp = p_label - p_label[:, :1]
    img, txt = slice(3, 3 + n), slice(3 + n, 3 + 2 * n)
    if C > 1:
        top = np.sort(zm, axis=-1)[..., -2:]
        gap = float((top[..., 1] - top[..., 0]).min())
    else:
        gap = np.inf
    return {"p_full": p_label[:, 0],
            "dp_image": dp[:, 1], "dp_image_control": dp[:, img].mean(1, dtype=dt), "sd_image_control": dp[:, img].std(1),
            "dp_text": dp[:, 2], "dp_text_control": dp[:, txt].mean(1, dtype=dt), "sd_text_control": dp[:, txt].std(1),
            "js_image": js[:, 1], "js_image_control": js[:, img].mean(1, dtype=dt),
            "js_text": js[:, 2], "js_text_control": js[:, txt].mean(1, dtype=dt),
            "hit_full": hit[:, 0], "hit_image": hit[:, 1], "hit_text": hit[:, 2],
            "acc_image_control": hit[:, img].mean(1, dtype=dt), "acc_text_control": hit[:, txt].mean(1, dtype=dt),
            "p_label": p_label, "js": js, "hit": hit, "gap": gap}


def rows_and_hits(ref):
    """what RelianceMeter.update_rows takes, from a summary_ref result: fp64 [S, 16] rows, fp64 [V] hit sums"""
    return (np.stack([ref[c] for c in COLUMNS], axis=1).astype(np.float64),
            ref["hit"].astype(np.float64).sum(0))


def make_logits(C, n, K, S, scale, seed):
    """f32 [S, V, K, C] and labels [S]: see the module docstring"""
    g = np.random.default_rng(seed)
    V = 3 + 2 * n
    z = (g.standard_normal((S, 1, 1, C)) + 0.7 * g.standard_normal((S, V, 1, C))
         + 0.5 * g.standard_normal((S, V, K, C)))
    win = g.integers(0, C, (S, V))
    for s in range(S):
        for v in range(V):
            z[s, v, :, win[s, v]] = z[s, v].max() + 3.0
    z = (z * scale).astype(np.float32)
    y = np.where(np.arange(S) % 2 == 0, win[:, 0], g.integers(0, C, S)).astype(np.int64)
    return z, y


@functools.lru_cache(maxsize=None)
def sweep():
    """every case's logits, labels and fp64 result, computed once -> {"cases": {(C, n, K, S, scale):
    (z, y, ref64)}, "floor": {column: max |f32 - fp64| over the sweep}, "bar": 4 x floor}"""
    cases, floor = {}, {c: 0.0 for c in COLUMNS + PLANES}
    grid = ((C, n, K, S, sc) for C in CS for n in NS for K in KS for S in SS for sc in SCALES)
    for i, (C, n, K, S, scale) in enumerate(grid):
        z, y = make_logits(C, n, K, S, scale, 5000 + i)
        r64, r32 = summary_ref(z, y, np.float64), summary_ref(z, y, np.float32)
        # the lift is 3 x scale before the logits are rounded to f32 (two roundings of the largest logit)
        slack = 2 * np.finfo(np.float32).eps * float(np.abs(z).max())
        assert r64["gap"] >= 3.0 * scale - slack, (C, n, K, S, scale, r64["gap"])
        for c in EXACT:
            assert same_f32(r32[c], r64[c]), (C, n, K, S, scale, c)
        for c in floor:
            floor[c] = max(floor[c], float(np.abs(r32[c].astype(np.float64) - r64[c]).max()))
        cases[(C, n, K, S, scale)] = (z, y, r64)
    return {"cases": cases, "floor": floor, "bar": {c: BAR_FACTOR * v for c, v in floor.items()}}


def launch(dev, z, y, layout, ld=None, planes=True, three_d=False):
    """the kernel on z (numpy [S, V, K, C]) laid out as `layout` with class rows ld apart, everything in
    guarded buffers -> ({column / plane: numpy fp64}, fails)"""
    from src import kernels as k
    S, V, K, C = z.shape
    ld = C if ld is None else ld
    shape = (V, S, K, ld) if layout == "VSKC" else (S, V, K, ld)
    gz = Guarded(dev, f32, NAN, int(np.prod(shape)))
    v = gz.view.view(*shape)[..., :C]
    v = v.permute(1, 0, 2, 3) if layout == "VSKC" else v
    v.copy_(torch.from_numpy(z))
    gz.set_canary()
    gy = Guarded(dev, i64, 85, S)
    gy.view.copy_(torch.from_numpy(y))
    gy.set_canary()
    outs = {"stats": out_buf(dev, f32, S, k.ROB_NSTAT)}
    if planes:
        outs["per_variant"] = out_buf(dev, f32, S, 3, V)
    if three_d:
        assert K == 1
        v = v[:, :, 0]
    k.robustness_summary(v, gy.view, outs["stats"][1], outs["per_variant"][1] if planes else None)
    torch.cuda.synchronize()
    fails, tag = [], f"C={C} V={V} K={K} S={S} {layout} ld={ld}"
    check_written({name: g for name, (g, _) in outs.items()}, fails, tag)
    if not (gz.unchanged() and gy.unchanged()):
        fails.append(f"{tag}: an input was written")
    st = outs["stats"][1].double().cpu().numpy()
    got = {c: st[:, i] for i, c in enumerate(k.ROB_COLUMNS)}
    if planes:
        pv = outs["per_variant"][1].double().cpu().numpy()
        got.update({c: pv[:, i] for i, c in enumerate(PLANES)})
    return got, fails


def compare(got, r64, n, errs, fails, tag, bar):
    """got vs the fp64 reference: per-column error into errs, the exact properties into fails"""
    for c in got:
        if not np.isfinite(got[c]).all():
            fails.append(f"{tag} {c}: not finite")
        e = float(np.abs(got[c] - r64[c]).max())
        errs[c] = max(errs.get(c, 0.0), e)
        if e > bar[c]:
            fails.append(f"{tag} {c}: error {e:.3e} > bar {bar[c]:.3e}")
        if c in EXACT and not same_f32(got[c], r64[c]):
            fails.append(f"{tag} {c}: differs from the reference")
    if "js" in got:
        if got["js"].min() < -bar["js"] or got["js"].max() > LN2 + bar["js"]:
            fails.append(f"{tag}: js outside [-bar, ln 2 + bar]: {got['js'].min():.3e} .. {got['js'].max():.6f}")
        if np.abs(got["js"][:, 0]).max() > bar["js"]:
            fails.append(f"{tag}: js of the full variant from itself is {np.abs(got['js'][:, 0]).max():.3e}")
    if n == 1:
        for c in ("sd_image_control", "sd_text_control"):
            if not np.array_equal(got[c], np.zeros_like(got[c])):
                fails.append(f"{tag} {c}: not exactly 0 at n = 1")


def report(what, errs, sw):
    print(f"\n{what}: column, f32-numpy floor, bar, measured")
    for c in errs:
        print(f"  {c:18s} {sw['floor'][c]:.3e} {sw['bar'][c]:.3e} {errs[c]:.3e}")


def test_the_columns_are_the_headers(dev):
    from src import kernels as k
    assert k.ROB_COLUMNS == COLUMNS and k.ROB_NSTAT == 16


@pytest.mark.parametrize("C", CS)
def test_sweep_against_fp64(dev, C):
    sw = sweep()
    errs, fails = {}, []
    for n in NS:
        for K in KS:
            for S in SS:
                for scale in SCALES:
                    z, y, r64 = sw["cases"][(C, n, K, S, scale)]
                    for layout in LAYOUTS:
                        got, f = launch(dev, z, y, layout)
                        fails += f
                        compare(got, r64, n, errs, fails, f"C={C} n={n} K={K} S={S} scale={scale} {layout}",
                                sw["bar"])
    report(f"C = {C}", errs, sw)
    assert not fails, "\n".join(fails[:20])


def test_padded_class_stride(dev):
    """class rows 101 + 7 apart, the padding holds NaN"""
    sw = sweep()
    errs, fails = {}, []
    for layout in LAYOUTS:
        z, y, r64 = sw["cases"][(101, 2, 2, 3, 1)]
        got, f = launch(dev, z, y, layout, ld=108)
        fails += f
        compare(got, r64, 2, errs, fails, f"padded {layout}", sw["bar"])
    report("padded class stride", errs, sw)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", CS)
def test_equal_logits(dev, C):
    """scale 0: every row an exact tie, class 0 wins, no shift and no divergence, p_full = 1 / C"""
    sw = sweep()
    bar = sw["bar"]
    for n in NS:
        for K in KS:
            z, y, _ = sw["cases"][(C, n, K, 3, 0)]
            got, fails = launch(dev, z, y, "VSKC")
            assert not fails, fails
            assert np.abs(got["p_full"] - 1.0 / C).max() <= bar["p_full"]
            for c in COLUMNS:
                if c.startswith(("dp_", "js_", "sd_")):
                    assert np.abs(got[c]).max() <= bar[c], c
            assert np.abs(got["js"]).max() <= bar["js"]
            won = (y == 0).astype(np.float64)
            for c in ("hit_full", "hit_image", "hit_text", "acc_image_control", "acc_text_control"):
                assert np.array_equal(got[c], won), c
            assert np.array_equal(got["hit"], np.repeat(won[:, None], 3 + 2 * n, 1))


@pytest.mark.parametrize("case", [(2, 1, 1, 3, 8), (101, 20, 1, 3, 1), (129, 3, 1, 1, 80), (1024, 2, 1, 3, 8)])
def test_three_d_stack_is_the_one_head_call(dev, case):
    """K = 1: the [S, V, C] call equals the [S, V, 1, C] call bitwise, in both layouts"""
    z, y, _ = sweep()["cases"][case]
    for layout in LAYOUTS:
        a, fa = launch(dev, z, y, layout)
        b, fb = launch(dev, z, y, layout, three_d=True)
        assert not fa and not fb, fa + fb
        for c in a:
            assert np.array_equal(a[c], b[c]), f"{case} {layout} {c}"


@pytest.mark.parametrize("case", [(1, 1, 2, 3, 1), (65, 2, 5, 3, 8), (1024, 20, 2, 3, 1)])
def test_labels_outside_the_classes(dev, case):
    """y = -1 and y = C: p_label = 0 and hit = 0 for every variant, the guards intact, and the sample
    between them as the reference has it"""
    sw = sweep()
    C, n = case[0], case[1]
    z, y, _ = sw["cases"][case]
    y = y.copy()
    y[0], y[2] = -1, C
    r64 = summary_ref(z, y, np.float64)
    for layout in LAYOUTS:
        got, fails = launch(dev, z, y, layout)
        compare(got, r64, n, {}, fails, f"{case} {layout}", sw["bar"])
        assert not fails, "\n".join(fails)
        for s in (0, 2):
            assert np.array_equal(got["p_label"][s], np.zeros(3 + 2 * n))
            assert np.array_equal(got["hit"][s], np.zeros(3 + 2 * n))
            for c in COLUMNS:
                if not c.startswith("js_"):
                    assert got[c][s] == 0.0, (c, s)


def test_per_variant_is_optional(dev):
    sw = sweep()
    for case in ((65, 3, 2, 3, 8), (1024, 20, 5, 3, 1)):
        z, y, r64 = sw["cases"][case]
        a, fa = launch(dev, z, y, "VSKC")
        b, fb = launch(dev, z, y, "VSKC", planes=False)
        assert not fa and not fb, fa + fb
        assert set(b) == set(COLUMNS)
        for c in COLUMNS:
            assert np.array_equal(a[c], b[c]), c


@pytest.mark.parametrize("det", [False, True])
def test_bitwise_repeatable(dev, det):
    from src import kernels as k
    sw = sweep()
    for case, layout in (((1024, 20, 5, 3, 1), "VSKC"), ((101, 20, 1, 3, 8), "SVKC"), ((63, 1, 2, 1, 80), "VSKC")):
        z, y, _ = sw["cases"][case]
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
            assert np.array_equal(a[c], c2[c]), f"{case} {c}: the modes differ"
