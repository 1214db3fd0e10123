"""CPU: the launch plans of the GEMM and conv products (csrc/plan.h), asked of the library through
mmu_gemm_plan / mmu_conv_implicit_plan / mmu_conv_wgrad_plan over a grid of shapes, knobs and
workspaces, stay inside the bounds whose violation would be an out-of-bounds write on the GPU: the
K slices of a split product tile K in whole 64-deep steps, their slabs fit the workspace, the split
tail rows and their slabs fit the per-stream scratch, the column sums' partial rows fit theirs, and
the tiles cover the output with no empty tile row or column.  The queries run the functions the
launches run, so what holds here holds for what is launched.
"""
import ctypes
import os
import re

import pytest

from src import _native as Nat
from src import kernels as K
import gemm_harness as G

SCRATCH_FLOATS = 8 << 20        # each per-stream scratch slot of mmu_gemm: 32 MiB (csrc/capi.hip, tail_workspace)
ENV_KEYS = ("MMU_GEMM_WIDE", "MMU_GEMM_WIDE_MIN_TILES", "MMU_GEMM_TAIL", "MMU_GEMM_CS_PART")
GEMM_M = (1, 7, 64, 127, 128, 129, 255, 256, 257, 511, 513, 1024, 4104, 16416, 32768, 65536, 65537, 65665, 65792,
          131328, 131329, 131584, 262144)
GEMM_N = (128, 256, 384, 512, 640, 768, 1024, 1152, 2304, 3072, 4096)
GEMM_K = (64, 128, 512, 768, 1024, 1088, 3072, 4096, 16416, 32768, 131328)
GEMM_ENVS = ({}, G.WIDE_ENV, G.TAIL_ENV, {**G.WIDE_ENV, **G.TAIL_ENV}, G.ATOMICS_ENV)
GEMM_WS = (K.SPLITK_WS_FLOATS, 3 * 256 * 256)
# (kind, f32 C, bias, colsum): every kind, f32 where the kind allows, column sums for DGELU / ADD_RES
GEMM_EPIS = ((G.STORE, False, False, False), (G.STORE, True, False, False), (G.BIAS_GELU, False, True, False),
             (G.BIAS_DROP_RES, False, True, False), (G.BIAS_DROP_RES, True, True, False),
             (G.DGELU, False, False, False), (G.DGELU, False, False, True), (G.ADD_RES, False, False, False),
             (G.ADD_RES, False, False, True), (G.BIAS_DROP_QGELU, False, True, False))
# the table kinds run at batch 1 in one layout each (mmu_gemm refuses the others): (kind, A K-major, B K-major)
GEMM_TABLES = ((G.STORE_STATS, True, True), (G.STORE_BNB, True, False), (G.ADD_RES_BNB, True, False))
TILE = {0: (128, 128), 1: (256, 256), 2: (256, 384)}
SHAPE_RULES = ("must be a multiple of", "bad shape", "bad geometry", "map size out of range", "too large for 32-bit",
               "% 64 == 0", "% 256 == 0")


def gemm_grid():
    """-> (M, N, K, batch, lda, ldb, ak, bk, c_dtype, kind, bias, colsum, ws_floats), dense operands,
    skipping the layouts the shape rules refuse (an M-major A needs M % 128 == 0, a K-major operand
    K % 64 == 0)"""
    for M in GEMM_M:
        for N in GEMM_N:
            for Kd in GEMM_K:
                for ak, bk in G.LAYOUTS:
                    if (not ak and M % 128) or ((ak or bk) and Kd % 64):
                        continue
                    lda, ldb = (Kd if ak else M), (Kd if bk else N)
                    for batch in (1, 2):
                        for kind, f32_, bias, cs in GEMM_EPIS:
                            for ws in (GEMM_WS if kind == G.STORE and f32_ else GEMM_WS[:1]):
                                yield (M, N, Kd, batch, lda, ldb, int(ak), int(bk), int(f32_), kind, int(bias),
                                       int(cs), ws)
                for kind, ak, bk in GEMM_TABLES if Kd % 64 == 0 else ():
                    yield (M, N, Kd, 1, Kd, Kd if bk else N, int(ak), int(bk), 0, kind, 0, 1, GEMM_WS[0])


def tiles_k(K_, slices, chunk):
    return chunk % 64 == 0 and (slices - 1) * chunk < K_ <= slices * chunk


def gemm_violation(a, p):
    """the plan p (the query's int64 fields) of the call a -> None, or the bound it breaks"""
    M, N, Kd, batch, ws = a[0], a[1], a[2], a[3], a[12]
    tiling, tiles_m, tiles_n, _, splitk, kchunk, m_main, tail_rows, tail_split, tail_chunk, cs, cs_rows, cs_parts = p
    tm, tn = TILE[tiling]
    if not ((tiles_m - 1) * tm < M <= tiles_m * tm and (tiles_n - 1) * tn < N <= tiles_n * tn):
        return "tiles do not cover the output exactly"
    if splitk > 1:
        if not (tiles_k(Kd, splitk, kchunk) and splitk <= 64):
            return "split-K slices do not tile K"
        if splitk * batch * M * N > ws:
            return "split-K slabs exceed the workspace"
        if tail_rows:
            return "split-K and the split tail coincide"
    elif splitk != 1 or kchunk != Kd:
        return "an unsplit plan with kchunk != K"
    if tail_rows:
        if m_main % 256 or m_main <= 0 or m_main + tail_rows != M or tail_split < 2:
            return "bad tail rows"
        if not tiles_k(Kd, tail_split, tail_chunk):
            return "tail slices do not tile K"
        if tail_split * tail_rows * N > SCRATCH_FLOATS:
            return "tail slabs exceed the scratch"
    elif m_main != M:
        return "no tail rows but m_main != M"
    if cs == 2:
        if cs_rows not in (64, 128) or cs_parts < -(-m_main // cs_rows) + -(-tail_rows // 64):
            return "partial rows do not cover the rows"
        if cs_parts * N > SCRATCH_FLOATS:
            return "partial rows exceed the scratch"
    return None


def test_gemm_plans_stay_in_bounds(monkeypatch):
    fn = Nat.load().mmu_gemm_plan
    out = (ctypes.c_int64 * len(Nat.PLAN_FIELDS["mmu_gemm_plan"]))()
    seen = {"plans": 0, "wide": 0, "tail": 0, "splitk": 0, "cs1": 0, "cs2": 0, "cs3": 0}
    bad = []
    for env in GEMM_ENVS:
        for key in ENV_KEYS:
            monkeypatch.delenv(key, raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        for a in gemm_grid():
            assert fn(*a, out) == 0, (a, Nat.last_error())
            p = tuple(out)
            why = gemm_violation(a, p)
            if why:
                bad.append((why, env, a, p))
            seen["plans"] += 1
            seen["wide"] += p[0] == 2
            seen["tail"] += p[7] > 0
            seen["splitk"] += p[4] > 1
            seen[f"cs{p[10]}"] = seen.get(f"cs{p[10]}", 0) + 1
    print(seen)
    assert not bad, f"{len(bad)} plans out of bounds, e.g. {bad[:3]}"
    assert all(seen.values()), f"a path of the plan has no case on the grid: {seen}"


CONV_N = (1, 2, 3, 8, 32, 256)
CONV_MAPS = ((1, 1), (1, 3), (3, 3), (7, 7), (7, 13), (8, 8), (14, 14), (16, 16), (28, 28), (56, 56))
CONV_CH = (64, 128, 256, 512, 1024, 2048)
CONV_WS = (K.SPLITK_WS_FLOATS, 1 << 20)


def conv_grid(wgrad):
    for n in CONV_N + ((700,) if wgrad else ()):
        for H, W in CONV_MAPS:
            for C in CONV_CH:
                for N in CONV_CH:
                    for ks in (1, 3):
                        for s in (1, 2, 3, 4):
                            for ws in CONV_WS:
                                yield (n, H, W, C, N, ks, s, ws)


def conv_violation(wgrad, a, p):
    n, H, W, C, N, ks, s, ws = a
    if wgrad:
        Kd, _, _, tiles_m, tiles_n, _, splitk, kchunk = p
        rows, cols = N, ks * ks * C                      # dW [Cout][T Cin]
        covered = (tiles_m - 1) * 256 < rows <= tiles_m * 256 and tiles_n * 256 == cols
    else:
        small, rows, Kd, _, _, tiles_m, tiles_n, splitk, kchunk = p
        cols, t = N, 128 if small else 256               # Y [pixels][N]
        covered = (tiles_m - 1) * t < rows <= tiles_m * t and (tiles_n - 1) * t < cols <= tiles_n * t
    if not covered:
        return "tiles do not cover the output exactly"
    if splitk > 1:
        if not tiles_k(Kd, splitk, kchunk):
            return "split-K slices do not tile K"
        if splitk * rows * cols > ws:
            return "split-K slabs exceed the workspace"
    elif splitk != 1 or kchunk != Kd:
        return "an unsplit plan with kchunk != K"
    return None


def _conv_sweep(name, wgrad):
    fn = getattr(Nat.load(), name)
    out = (ctypes.c_int64 * len(Nat.PLAN_FIELDS[name]))()
    plans = split = 0
    bad = []
    for a in conv_grid(wgrad):
        if fn(*a, out) != 0:        # refused: by a shape rule, never by anything else
            assert any(r in Nat.last_error() for r in SHAPE_RULES), (a, Nat.last_error())
            continue
        p = tuple(out)
        why = conv_violation(wgrad, a, p)
        if why:
            bad.append((why, a, p))
        plans += 1
        split += p[-2] > 1
    print(name, plans, "plans,", split, "split")
    assert not bad, f"{len(bad)} plans out of bounds, e.g. {bad[:3]}"
    assert plans > 5000 and 0 < split < plans


def test_conv_implicit_plans_stay_in_bounds():
    _conv_sweep("mmu_conv_implicit_plan", False)


def test_conv_wgrad_plans_stay_in_bounds():
    _conv_sweep("mmu_conv_wgrad_plan", True)


def test_plan_field_counts_match_the_header():
    """include/mmu.h's MMU_*_PLAN_FIELDS against the binding's field names"""
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmu.h")).read()
    counts = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define MMU_(\w+)_PLAN_FIELDS (\d+)", txt)}
    assert counts == {n[4:-5]: len(f) for n, f in Nat.PLAN_FIELDS.items()}


def test_queries_refuse_as_the_launch_does():
    """a refusal that belongs to the plan comes back through mmu_last_error, word for word"""
    with pytest.raises(Nat.NativeError, match="mmu_gemm: N=100 must be a multiple of 128"):
        K.gemm_plan(128, 100, 64)
    with pytest.raises(Nat.NativeError, match="mmu_gemm: M=130 must be a multiple of 128 when A is M-major"):
        K.gemm_plan(130, 128, 64, a_kmajor=False)
    with pytest.raises(Nat.NativeError, match="mmu_conv_implicit: map size out of range"):
        K.conv_plan(1, 15, 16, 64, 64)
    with pytest.raises(Nat.NativeError, match=r"mmu_conv_wgrad: bad geometry \(n=1 H=8 W=8 C=256 ksize=2 stride=1\)"):
        K.conv_wgrad_plan(1, 8, 8, 256, 128, ksize=2)
    with pytest.raises(Nat.NativeError, match="C=12 must be a multiple of 8"):
        K.batchnorm_plan(64, 12)
    with K.deterministic():
        with pytest.raises(Nat.NativeError, match="colsum with batch=2 splitk=1 has no partial-row path$"):
            K.gemm_plan(256, 256, 64, batch=2, kind=K.EPI_DGELU, colsum=True)
    assert K.gemm_plan(256, 256, 64, batch=2, kind=K.EPI_DGELU, colsum=True)["cs"] == "atomics"
