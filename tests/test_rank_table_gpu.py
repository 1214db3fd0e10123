"""mmu_rank_table (csrc/ranking.hip) against the brute-force table on MI355X: rank and counts must EQUAL
tests/ranking_ref.py rank_table_ref exactly -- they are integers, there is no tolerance.

Sweep.  S in {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025}: the kernel's block rows and its LDS tile
are both 1024 samples (kernels.RANK_BLOCK_ROWS, RANK_TILE; asserted below), so 1023 / 1024 / 1025 are
those two +- 1, 1025 runs two blocks of two tiles each, and S mod 4 takes every value (the sweep reads four
candidates per step and pads the last group with NaN).  J in {1, 3, 47}.  Value recipes, one per column
of a 47-column table (column j has recipe j mod 7, its own seed): distinct Gaussians; integers 0 .. 3
(heavy ties); all equal; +-0 mixed with a few other values; +-inf present; distinct subnormals; about
10 % NaN.  The J = 47 call takes the whole table, J = 3 its column windows [0, 3), [3, 6), [6, 9) (every
recipe), J = 1 each of its first seven columns: columns are independent, so one reference per (S,
groups) serves them all.  Groups: all 0, all 1, mixed.  Layouts: contiguous [S, J]; a [J, S] table read
through its strides; a row stride padded by 5.  Every tensor is a view in a tests/guarded.py buffer:
inputs NaN- (85-) surrounded and unchanged afterwards, outputs sentinel-prefilled, fully written and
nothing around them touched.
"""
import functools

import numpy as np
import pytest
import torch

from guarded import NAN, Guarded
from ranking_ref import EQ, EQ0, EQ1, GT, LT0, LT1, N0, N1, rank_table_ref
from ranking_ref import NAN as C_NAN

pytestmark = pytest.mark.gpu

f32, i32, i64, u8 = torch.float32, torch.int32, torch.int64, torch.uint8
SS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
JMAX = 47
RECIPES = ("gauss", "ties", "equal", "zeros", "inf", "subnormal", "nan")
GROUPS = ("zeros", "ones", "mixed")
LAYOUTS = ("SJ", "JS", "padded")
SENTINEL = -7777
# (first column, J): the whole table, three windows of 3 that cover every recipe, the first seven columns alone
WINDOWS = ((0, 47), (0, 3), (3, 3), (6, 3)) + tuple((j, 1) for j in range(7))


def column(recipe, S, rng):
    if recipe == "gauss":
        while True:
            v = rng.standard_normal(S).astype(np.float32)
            if np.unique(v).size == S:
                return v
    if recipe == "ties":
        return rng.integers(0, 4, S).astype(np.float32)
    if recipe == "equal":
        return np.full(S, np.float32(rng.standard_normal()), dtype=np.float32)
    if recipe == "zeros":
        return rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.5, -2.0], dtype=np.float32), S)
    if recipe == "inf":
        v = rng.integers(-2, 3, S).astype(np.float32)
        v[rng.random(S) < 0.2] = np.inf
        v[rng.random(S) < 0.2] = -np.inf
        return v
    if recipe == "subnormal":   # distinct multiples of the smallest subnormal, both signs: flushed, they would all tie
        bits = rng.permutation(4 * S)[:S].astype(np.uint32) + 1
        v = bits.view(np.float32).copy()
        assert (np.abs(v) < np.finfo(np.float32).tiny).all() and (v != 0).all()
        v[rng.random(S) < 0.5] *= -1
        return v
    if recipe == "nan":
        v = rng.standard_normal(S).astype(np.float32)
        v[rng.random(S) < 0.1] = np.nan
        if S >= 2:
            v[rng.integers(S)] = np.nan
        return v
    raise AssertionError(recipe)


@functools.lru_cache(maxsize=None)
def table(S):
    rng = np.random.default_rng(4000 + S)
    x = np.stack([column(RECIPES[j % len(RECIPES)], S, rng) for j in range(JMAX)], axis=1)
    mixed = rng.random(S) < 0.4
    if S >= 2:
        mixed[:2] = (True, False)
    x.setflags(write=False)
    return x, {"zeros": np.zeros(S, bool), "ones": np.ones(S, bool), "mixed": mixed}


@functools.lru_cache(maxsize=None)
def reference(S, groups):
    """the 47-column reference of one (S, groups), computed once and left unchanged"""
    x, g = table(S)
    rank, counts = rank_table_ref(x, g[groups])
    rank.setflags(write=False)
    counts.setflags(write=False)
    return rank, counts


def launch(dev, x, group, layout, with_rank=True):
    """the kernel on x (numpy f32 [S, J]) laid out as `layout`, everything in guarded buffers ->
    (rank int32 [J, S, 4] or None, counts int64 [J, 5], fails)"""
    from src import kernels as k
    S, J = x.shape
    if layout == "JS":
        gx = Guarded(dev, f32, NAN, J * S)
        v = gx.view.view(J, S).t()
    else:
        ld = J + (5 if layout == "padded" else 0)
        gx = Guarded(dev, f32, NAN, S * ld)
        v = gx.view.view(S, ld)[:, :J]
    v.copy_(torch.from_numpy(np.array(x)))
    gx.set_canary()
    gg = Guarded(dev, u8, 85, S)
    gg.view.copy_(torch.from_numpy(group.astype(np.uint8) * 3))       # non-zero marks group 1, not only 1
    gg.set_canary()
    outs = {"counts": Guarded(dev, i64, SENTINEL, J * k.RANK_NCOUNT)}
    if with_rank:
        outs["rank"] = Guarded(dev, i32, SENTINEL, J * S * k.RANK_NRANK)
    rank, counts = k.rank_table(v, gg.view, rank=outs["rank"].view.view(J, S, k.RANK_NRANK) if with_rank else None,
                                counts=outs["counts"].view.view(J, k.RANK_NCOUNT))
    torch.cuda.synchronize()
    fails, tag = [], f"S={S} J={J} {layout} rank={with_rank}"
    for name, g in outs.items():
        if not g.guards_intact():
            fails.append(f"{tag} {name}: a guard element was written")
        if bool((g.view == SENTINEL).any()):
            fails.append(f"{tag} {name}: an element was left unwritten")
    if not (gx.unchanged() and gg.unchanged()):
        fails.append(f"{tag}: an input was written")
    assert (rank is None) == (not with_rank)
    return (rank.cpu().numpy() if with_rank else None), counts.cpu().numpy(), fails


def test_the_sweep_straddles_the_kernels_tiling(dev):
    from src import kernels as k
    assert k.RANK_BLOCK_ROWS == 1024 and k.RANK_TILE == 1024
    for edge in (k.RANK_BLOCK_ROWS, k.RANK_TILE):
        assert {edge - 1, edge, edge + 1} <= set(SS)
    assert {s % 4 for s in SS} == {0, 1, 2, 3}
    assert {RECIPES[(j0 + d) % 7] for j0, J in WINDOWS if J == 3 for d in range(3)} == set(RECIPES)
    x, _ = table(257)
    assert np.isnan(x[:, 6]).any() and np.isinf(x[:, 4]).any() and (np.signbit(x[:, 3]) & (x[:, 3] == 0)).any()


@pytest.mark.parametrize("S", SS)
def test_sweep_equals_the_brute_force_table(dev, S):
    x, groups = table(S)
    fails, n = [], 0
    for gname in GROUPS:
        rank_ref, counts_ref = reference(S, gname)
        for j0, J in WINDOWS:
            for layout in LAYOUTS:
                rank, counts, f = launch(dev, x[:, j0:j0 + J], groups[gname], layout)
                tag = f"S={S} J={J} (from column {j0}) groups={gname} {layout}"
                fails += f
                n += 1
                if not np.array_equal(rank, rank_ref[j0:j0 + J]):
                    bad = np.argwhere(rank != rank_ref[j0:j0 + J])[0]
                    fails.append(f"{tag}: rank differs, first at (column, sample, which) = {tuple(bad)}")
                if not np.array_equal(counts, counts_ref[j0:j0 + J]):
                    fails.append(f"{tag}: counts {counts.tolist()[:2]} != {counts_ref[j0:j0 + J].tolist()[:2]}")
    print(f"\nS = {S}: {n} launches compared")
    assert not fails, "\n".join(fails[:20])


def test_what_the_ieee_compares_imply(dev):
    """on the kernel's own output: -0 ties +0, +-inf rank as ordinary values, the subnormals are all
    distinct, a NaN sample has four zeros and is counted by nobody"""
    S = 257
    x, groups = table(S)
    rank, counts, fails = launch(dev, x[:, :7], groups["mixed"], "SJ")
    assert not fails, fails
    g = groups["mixed"]
    tot_lt, tot_eq = rank[:, :, LT0] + rank[:, :, LT1], rank[:, :, EQ0] + rank[:, :, EQ1]
    col = {r: j for j, r in enumerate(RECIPES)}
    assert sorted(tot_lt[col["gauss"]]) == list(range(S)) and (tot_eq[col["gauss"]] == 1).all()
    assert (tot_lt[col["equal"]] == 0).all() and (tot_eq[col["equal"]] == S).all()
    z = x[:, col["zeros"]]
    zero = z == 0
    assert np.signbit(z[zero]).any() and not np.signbit(z[zero]).all()
    assert (tot_eq[col["zeros"]][zero] == zero.sum()).all() and np.unique(tot_lt[col["zeros"]][zero]).size == 1
    v = x[:, col["inf"]]
    assert (tot_lt[col["inf"]][v == -np.inf] == 0).all() and (tot_eq[col["inf"]][v == np.inf] == (v == np.inf).sum()).all()
    assert (tot_lt[col["inf"]][v == np.inf] == (v < np.inf).sum()).all()
    assert sorted(tot_lt[col["subnormal"]]) == list(range(S)) and (tot_eq[col["subnormal"]] == 1).all()
    nan = np.isnan(x[:, col["nan"]])
    assert nan.any() and (rank[col["nan"]][nan] == 0).all()
    assert counts[col["nan"], C_NAN] == nan.sum() and tot_lt[col["nan"]].max() == S - nan.sum() - 1
    assert counts[col["nan"], N1] == (g & ~nan).sum() and counts[col["nan"], N0] == (~g & ~nan).sum()
    for j in range(6):
        assert counts[j, C_NAN] == 0 and counts[j, N1] == g.sum() and counts[j, N0] == S - g.sum()
        assert counts[j, GT] == rank[j, g, LT0].sum() and counts[j, EQ] == rank[j, g, EQ0].sum()


@pytest.mark.parametrize("S", [1, 65, 1025])
def test_rank_is_optional(dev, S):
    x, groups = table(S)
    for gname in GROUPS:
        for layout in LAYOUTS:
            _, a, fa = launch(dev, x, groups[gname], layout)
            rank, b, fb = launch(dev, x, groups[gname], layout, with_rank=False)
            assert not fa and not fb, fa + fb
            assert rank is None and np.array_equal(a, b) and np.array_equal(a, reference(S, gname)[1])


def test_the_wrapper_allocates_what_it_is_not_given(dev):
    from src import kernels as k
    x, groups = table(255)
    xd = torch.from_numpy(np.array(x[:, :9])).to(dev)
    g = torch.from_numpy(groups["mixed"]).to(dev)                       # a bool tensor
    rank, counts = k.rank_table(xd, g, rank=True)
    none, counts2 = k.rank_table(xd.t().contiguous().t(), g.to(u8))
    torch.cuda.synchronize()
    r, c = reference(255, "mixed")
    assert none is None and rank.dtype == i32 and counts.dtype == i64
    assert np.array_equal(rank.cpu().numpy(), r[:9]) and np.array_equal(counts.cpu().numpy(), c[:9])
    assert np.array_equal(counts2.cpu().numpy(), c[:9])


@pytest.mark.parametrize("det", [False, True])
def test_bitwise_repeatable(dev, det):
    from src import kernels as k
    for S, layout in ((1025, "SJ"), (257, "JS"), (64, "padded")):
        x, groups = table(S)
        with k.deterministic(det):
            ra, ca, fa = launch(dev, x, groups["mixed"], layout)
            rb, cb, fb = launch(dev, x, groups["mixed"], layout)
        assert not fa and not fb
        with k.deterministic(not det):   # and the mode itself changes nothing: one launch serves both
            rc, cc, _ = launch(dev, x, groups["mixed"], layout)
        assert np.array_equal(ra, rb) and np.array_equal(ca, cb), f"S={S}: two launches differ (deterministic={det})"
        assert np.array_equal(ra, rc) and np.array_equal(ca, cc), f"S={S}: the modes differ"
