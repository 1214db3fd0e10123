"""Reference, launch plans and case lists for the image trunk's kernels: the implicit-im2col conv
products of csrc/gemm.hip (gemm_conva_small_kernel, gemm_conva_kernel, gemm_convw_kernel and the
split-K reduce kernels, behind mmu_conv_implicit[_stats], mmu_conv3x3_implicit[_bnb] and
mmu_conv[3x3]_wgrad), the stem pair of csrc/stem.hip, the max pool of csrc/pool.hip and the row pool
of csrc/embed.hip.  Pure torch; the same functions run on the CPU and on the device.  Used by
test_conv_reference.py (CPU), test_conv_edges_gpu.py, test_stem_edges_gpu.py and
test_pool_edges_gpu.py.

A conv is a GEMM on bf16 values once the gather is written down:
  im2col(x_nhwc, ks, stride)   [n Ho Wo, ks ks C], K ordered tap * C + c, pad ks // 2, zeros for the
                               padding -- explicit padded strided slices, the independent statement
                               of the gather (no conv2d, no unfold)
  forward / data gradient      Y = im2col(X) @ Wk^T, Wk [N][ks ks C]; the 3x3 / stride-1 data gradient
                               is the same product on dY with the flipped filter [Cin][3][3][Cout]
  weight gradient              dW[co, tap Cin + ci] = dY^T @ im2col(X): contraction over the output
                               pixels in pixel order
so the float64 reference, the float32 order model and the scales are gemm_harness.gemm_ref /
gemm_model32 unchanged (K in 32-deep steps in k order, split-K slabs by kchunk in slice order), and
the STATS / BNB tables are table_ref / table_model over the kernel's own stored C.
  stem_im2col      the stem's own K layout: tap * 4 + c, 49 taps padded to 56 (224 deep, seven
                   32-deep steps).  The filter gradient is referenced in float64 alone; its f32 model
                   is plain pixel-order accumulation (32 pixels a step into one accumulator), which
                   overestimates the error of the kernel's blocked order (per-block slabs, 16 slices)
                   and so is a safe basis for check_f32.
  maxpool_ref      MaxPool2d(3, 2, 1): scan row-major with v > max || isnan(v), the first in-image
                   element seeds -> values and the 0..8 window position
  row_pool_ref / row_pool_model   AdaptiveAvgPool2d((n, 1)): bins [floor(i Hh / n), ceil((i + 1) Hh / n))

conv_plan / wgrad_plan ASK the host for its plan (mmu_conv_implicit_plan / mmu_conv_wgrad_plan: the
plan functions of csrc/plan.h that the launches themselves run -- small or big kernel, tiles, splitk,
kchunk, few / many; the built library, no GPU).  As with gemm_plan they label the cases and hand the
summation order to the f32 model.

Input kinds: "int" X, dY in -3..3 and W in -2..2: |product| <= 9, and 9 K < 2^24 for every case, so
every f32 partial sum is exact in any order; "gauss" X, dY ~ N(0, 1), W ~ 0.1 N(0, 1).
"""
import torch

import gemm_harness as G

from src import kernels

bf16 = torch.bfloat16
SPLITK_WS_FLOATS = kernels.SPLITK_WS_FLOATS


def conv_out(h, w, ks, stride):
    pad = ks // 2
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


# ------------------------------------------------------------------------------- the gather
def _taps(x, ks, stride, pad, Ho, Wo):
    """x [n, H, W, C] -> the ks * ks shifted strided slices [n, Ho, Wo, C] of the zero-padded map"""
    n, H, W, C = x.shape
    xp = torch.zeros(n, H + 2 * pad, W + 2 * pad, C, dtype=x.dtype, device=x.device)
    xp[:, pad:pad + H, pad:pad + W] = x
    return [xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
            for kh in range(ks) for kw in range(ks)]


def im2col(x_nhwc, ks, stride):
    """[n, H, W, C] -> [n Ho Wo, ks ks C] (K = tap * C + c), same dtype"""
    n, H, W, C = x_nhwc.shape
    Ho, Wo = conv_out(H, W, ks, stride)
    return torch.stack(_taps(x_nhwc, ks, stride, ks // 2, Ho, Wo), 3).reshape(n * Ho * Wo, ks * ks * C)


def filter_rows(w_oihw):
    """a [Cout, Cin, k, k] filter -> Wk [Cout, k k Cin] (the memory of its channels-last copy)"""
    return w_oihw.permute(0, 2, 3, 1).reshape(w_oihw.shape[0], -1)


def dgrad_filter(w_oihw):
    """the 3x3 / stride-1 data gradient's filter: flipped and transposed, [Cin][3][3][Cout]"""
    return w_oihw.flip(2, 3).permute(1, 2, 3, 0).contiguous()


STEM_TAPS, STEM_KP = 49, 224


def stem_out(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def stem_im2col(x_nhwc):
    """[n, H, W, 3] -> [n Ho Wo, 224]: 7x7 / stride 2 / pad 3, K = tap * 4 + c, zero in the padding
    channel and in taps 49..55"""
    n, H, W, C = x_nhwc.shape
    Ho, Wo = stem_out(H, W)
    t = torch.stack(_taps(x_nhwc, 7, 2, 3, Ho, Wo), 3)                       # [n, Ho, Wo, 49, 3]
    col = torch.zeros(n, Ho, Wo, STEM_KP // 4, 4, dtype=x_nhwc.dtype, device=x_nhwc.device)
    col[:, :, :, :STEM_TAPS, :3] = t
    return col.reshape(n * Ho * Wo, STEM_KP)


def stem_filter_rows(w_oihw):
    """[64, 3, 7, 7] -> [64, 224] in the stem's K layout"""
    o = w_oihw.shape[0]
    wk = torch.zeros(o, STEM_KP // 4, 4, dtype=w_oihw.dtype, device=w_oihw.device)
    wk[:, :STEM_TAPS, :3] = w_oihw.permute(0, 2, 3, 1).reshape(o, STEM_TAPS, 3)
    return wk.reshape(o, STEM_KP)


def stem_unpack(dw_rows):
    """[64, 224] (stem K layout) -> [64, 147]: the memory of a channels-last [64, 3, 7, 7]"""
    o = dw_rows.shape[0]
    return dw_rows.reshape(o, STEM_KP // 4, 4)[:, :STEM_TAPS, :3].reshape(o, STEM_TAPS * 3)


def stem_tiles(n, H, W):
    """the stem kernels' tiles (2 output rows x 64 output columns) -> (tiles per image, n_tiles)"""
    Ho, Wo = stem_out(H, W)
    per = ((Ho + 1) // 2) * ((Wo + 63) // 64)
    return per, n * per


# ------------------------------------------------------------------------------- inputs
def conv_inputs(kind, shapes, seed, device="cpu"):
    """-> one bf16 tensor per entry of shapes = ((role, shape), ...); role "x" (a map: X, dY) or "w"
    (a filter).  "int": maps in -3..3, filters in -2..2; "gauss": maps N(0, 1), filters 0.1 N(0, 1)"""
    g = torch.Generator(device=device).manual_seed(seed)
    out = []
    for role, shape in shapes:
        if kind == "int":
            lim = 3 if role == "x" else 2
            t = torch.randint(-lim, lim + 1, shape, generator=g, device=device).float()
        else:
            t = torch.randn(*shape, generator=g, device=device) * (1.0 if role == "x" else 0.1)
        out.append(t.to(bf16))
    return out


def int_sum_bound(c):
    """the largest |partial sum| an "int" case can reach: max |product| x the contraction depth"""
    if c["op"] == "wgrad":
        return 9 * wgrad_plan_of(c)["K"]
    return 6 * conv_plan_of(c)["K"]


# ------------------------------------------------------------------------------- the host's plans
def _slices(p):
    """the K depth of every slice of a queried plan"""
    return [min(p["kchunk"], p["K"] - i * p["kchunk"]) for i in range(p["splitk"])]


def conv_plan(n, H, W, C, N, ks, stride, ws_floats=SPLITK_WS_FLOATS):
    """the host's plan for the forward / data-gradient product (kernels.conv_plan:
    mmu_conv_implicit_plan runs the function mmu_conv_implicit runs) -> its dict M, K, Ho, Wo, tiles_m,
    tiles_n, splitk, kchunk, and the labels kernel "small" | "big", tiles, slices (the K depth of
    every slice), split ("unsplit" | "split-even" | "split-uneven")"""
    p = kernels.conv_plan(n, H, W, C, N, ks, stride, ws_floats)
    p.update(kernel="small" if p["small"] else "big", tiles=p["tiles_m"] * p["tiles_n"], slices=_slices(p))
    p["split"] = "unsplit" if p["splitk"] == 1 else "split-even" if p["slices"][-1] == p["kchunk"] else "split-uneven"
    return p


def wgrad_plan(n, H, W, Cin, Cout, ks, stride, ws_floats=SPLITK_WS_FLOATS):
    """the host's plan for the weight gradient (kernels.conv_wgrad_plan: mmu_conv_wgrad_plan) -> its
    dict K (output pixels), Ho, Wo, tiles_m, tiles_n, few, splitk, kchunk, and the labels tiles,
    slices, path ("few-unsplit" | "few-split" | "many-unsplit" | "many-split")"""
    p = kernels.conv_wgrad_plan(n, H, W, Cin, Cout, ks, stride, ws_floats)
    p.update(few=bool(p["few"]), tiles=p["tiles_m"] * p["tiles_n"], slices=_slices(p))
    p["path"] = ("few" if p["few"] else "many") + ("-unsplit" if p["splitk"] == 1 else "-split")
    return p


# ------------------------------------------------------------------------------- the sweep's cases
def fcase(n, H, W, C, N, ks=3, s=1, inp="int", epi="store", mask=False, dgrad=False):
    """one forward / data-gradient launch.  epi: "store" | "stats" | "bnb"; dgrad: the product runs on
    dY [n, N, H, W] with the flipped filter, so the kernel sees N input and C output channels"""
    c = dict(op="dgrad" if dgrad else "fwd", n=n, H=H, W=W, C=C, N=N, ks=ks, s=s, inp=inp, epi=epi, mask=mask)
    c["name"] = (f"{c['op']} {n}x{H}x{W} {C}->{N} {ks}/{s} {inp} {epi}{' mask' if mask else ''}")
    return c


def conv_plan_of(c):
    cin, cout = (c["N"], c["C"]) if c["op"] == "dgrad" else (c["C"], c["N"])
    return conv_plan(c["n"], c["H"], c["W"], cin, cout, c["ks"], c["s"])


# (n, H, W, C, N, ks, stride): the smallest shapes that reach each path
FWD_ROWS = (
    (1, 16, 16, 64, 64, 3, 1),      # small: M = 256 exactly, N = 64 half tile, split 320 + 256
    (3, 7, 13, 128, 128, 3, 1),     # small: M tail 17 rows, tiles straddle images, 320/320/320/192 crossing taps
    (1, 16, 16, 256, 64, 3, 1),     # small: nine even slices of 256 (one tap each)
    (16, 32, 32, 64, 64, 3, 1),     # small: 128 tiles, unsplit
    (2, 12, 12, 64, 192, 1, 1),     # small: K = 64 unsplit, second column tile 64 wide
    (8, 17, 17, 64, 128, 3, 3), (8, 17, 17, 64, 128, 1, 3),       # stride 3
    (11, 18, 18, 128, 64, 3, 4), (11, 18, 18, 128, 64, 1, 4),     # stride 4
    (2, 1, 128, 64, 64, 3, 1), (2, 128, 1, 64, 64, 3, 1),         # one-row / one-column maps
    (3, 7, 13, 256, 256, 3, 1),     # big: M = 273, nine even slices
    (1, 7, 73, 64, 384, 3, 1), (1, 27, 19, 64, 384, 3, 1),        # big: M = 511 / 513, N = 384, 320 + 256
    (5, 15, 15, 512, 512, 3, 2), (4, 16, 16, 512, 512, 1, 2),     # big: odd / even strided maps
    (5, 23, 23, 256, 256, 3, 3), (8, 21, 21, 256, 256, 1, 4),     # big: strides 3 and 4 (M = 320, 288)
    (32, 32, 32, 64, 256, 3, 1),    # big: 128 tiles, unsplit
)
# rows that also run with a table: (row, epilogues)
STATS_ROWS = {(1, 16, 16, 64, 64, 3, 1), (3, 7, 13, 128, 128, 3, 1), (16, 32, 32, 64, 64, 3, 1),
              (8, 17, 17, 64, 128, 3, 3), (3, 7, 13, 256, 256, 3, 1), (1, 7, 73, 64, 384, 3, 1),
              (5, 15, 15, 512, 512, 3, 2), (32, 32, 32, 64, 256, 3, 1)}
BNB_ROWS = {(3, 7, 13, 128, 128, 3, 1), (16, 32, 32, 64, 64, 3, 1), (3, 7, 13, 256, 256, 3, 1),
            (32, 32, 32, 64, 256, 3, 1)}
LARGE_ROWS = {(16, 32, 32, 64, 64, 3, 1), (32, 32, 32, 64, 256, 3, 1)}     # the two 128-tile rows


def cases_fwd(rows=None):
    out = []
    for i, row in enumerate(FWD_ROWS):
        if rows is not None and row not in rows:
            continue
        n, H, W, C, N, ks, s = row
        out.append(fcase(*row, inp="int"))
        if row not in LARGE_ROWS:
            out.append(fcase(*row, inp="gauss"))
        if row in STATS_ROWS:
            out.append(fcase(*row, inp="gauss" if i % 2 else "int", epi="stats"))
        if (ks, s) == (3, 1):
            out.append(fcase(*row, inp="int" if i % 2 else "gauss", dgrad=True))
        if row in BNB_ROWS:     # (a data gradient in the trunk; the kernel sees the same product)
            out.append(fcase(*row, inp="gauss", epi="bnb", mask=False))
            out.append(fcase(*row, inp="int", epi="bnb", mask=True))
    return out


def wcase(n, H, W, Cin, Cout, ks=3, s=1, inp="int", acc=False):
    c = dict(op="wgrad", n=n, H=H, W=W, C=Cin, N=Cout, ks=ks, s=s, inp=inp, acc=acc)
    c["name"] = f"wgrad {n}x{H}x{W} {Cin}->{Cout} {ks}/{s} {inp}{' acc' if acc else ''}"
    return c


def wgrad_plan_of(c):
    return wgrad_plan(c["n"], c["H"], c["W"], c["C"], c["N"], c["ks"], c["s"])


WGRAD_ROWS = (
    (1, 1, 1, 256, 128, 3, 1),                                    # K = 1: only the centre tap is not all padding
    (1, 7, 9, 256, 128, 3, 1), (1, 8, 8, 256, 128, 3, 1), (1, 5, 13, 256, 128, 3, 1),   # K = 63, 64, 65
    (2, 17, 17, 256, 128, 1, 1), (2, 17, 17, 256, 512, 1, 1),     # few-tile split, 320 + 258
    (2, 33, 33, 256, 256, 1, 2), (2, 33, 33, 256, 256, 3, 2),     # strided, odd map
    (700, 1, 3, 256, 128, 3, 1),    # K = 2100: many-tile split 1088 + 1012, pixel division with HW = 3, img <= 699
    (3, 27, 27, 256, 384, 3, 1),    # K = 2187, Cout 384 (half a second row tile)
    (6, 10, 10, 512, 128, 3, 3), (6, 10, 10, 512, 128, 1, 4),     # strides 3, 4
    (1, 1, 9, 256, 128, 3, 1),      # a 1 x W map: the top and bottom tap rows are all padding
)


def cases_wgrad():
    out = []
    for i, row in enumerate(WGRAD_ROWS):
        for acc in (False, True):
            out.append(wcase(*row, inp="int", acc=acc))
        out.append(wcase(*row, inp="gauss", acc=bool(i % 2)))
    return out


# the paths that must have a case: label -> predicate over (case, plan)
FWD_PATHS = {
    f"{k}/{sp}": (lambda c, p, k=k, sp=sp: p["kernel"] == k and p["split"] == sp)
    for k in ("small", "big") for sp in ("unsplit", "split-even", "split-uneven")}
FWD_PATHS.update({
    "STORE": lambda c, p: c["epi"] == "store",
    "STATS in-kernel": lambda c, p: c["epi"] == "stats" and p["splitk"] == 1,
    "STATS by the reduce kernel": lambda c, p: c["epi"] == "stats" and p["splitk"] > 1,
    "BNB in-kernel": lambda c, p: c["epi"] == "bnb" and p["splitk"] == 1,
    "BNB by the reduce kernel": lambda c, p: c["epi"] == "bnb" and p["splitk"] > 1,
    "split table with a partial last block": lambda c, p: c["epi"] != "store" and p["splitk"] > 1 and p["M"] % 64 != 0,
    "a slice crossing a tap": lambda c, p: p["splitk"] > 1 and p["kchunk"] % c["C" if c["op"] == "fwd" else "N"] != 0,
    "stride 3": lambda c, p: c["s"] == 3, "stride 4": lambda c, p: c["s"] == 4,
    "1x1 stride 1": lambda c, p: (c["ks"], c["s"]) == (1, 1),
    "tile straddling images": lambda c, p: c["n"] > 1 and (128 if p["kernel"] == "small" else 256) % (p["Ho"] * p["Wo"])
    and (p["Ho"] * p["Wo"]) % (128 if p["kernel"] == "small" else 256),
})
for _k in ("small", "big"):
    for _e in ("stats", "bnb"):
        for _sp in (False, True):
            FWD_PATHS[f"{_k} {_e} {'split' if _sp else 'unsplit'}"] = (
                lambda c, p, k=_k, e=_e, sp=_sp: p["kernel"] == k and c["epi"] == e and (p["splitk"] > 1) == sp)
WGRAD_PATHS = {
    "few-unsplit": lambda c, p: p["path"] == "few-unsplit", "few-split": lambda c, p: p["path"] == "few-split",
    "many-unsplit": lambda c, p: p["path"] == "many-unsplit", "many-split": lambda c, p: p["path"] == "many-split",
    "Cout 128": lambda c, p: c["N"] == 128, "Cout 256": lambda c, p: c["N"] == 256, "Cout 384": lambda c, p: c["N"] == 384,
    "uneven last slice": lambda c, p: p["splitk"] > 1 and p["slices"][-1] != p["kchunk"],
    "few-split uneven": lambda c, p: p["path"] == "few-split" and p["slices"][-1] != p["kchunk"],
    "K = 1": lambda c, p: p["K"] == 1, "K = 63": lambda c, p: p["K"] == 63, "K = 64": lambda c, p: p["K"] == 64,
    "K = 65": lambda c, p: p["K"] == 65,
    "stride 3": lambda c, p: c["s"] == 3, "stride 4": lambda c, p: c["s"] == 4,
    "many images of a tiny map": lambda c, p: c["n"] >= 512 and (p["Ho"] * p["Wo"]) & (p["Ho"] * p["Wo"] - 1) != 0,
}


def padding_taps(H, W, ks, stride):
    """the taps of a ks x ks / pad ks // 2 conv that read padding alone on an H x W map -> bool [ks ks]"""
    Ho, Wo = conv_out(H, W, ks, stride)
    pad = ks // 2
    dead = []
    for kh in range(ks):
        for kw in range(ks):
            rows = any(0 <= ho * stride - pad + kh < H for ho in range(Ho))
            cols = any(0 <= wo * stride - pad + kw < W for wo in range(Wo))
            dead.append(not (rows and cols))
    return torch.tensor(dead)


# ------------------------------------------------------------------------------- stem reference
def stem_fwd_ref(x_nhwc, w_oihw):
    """-> (A [1, M, 224], B [1, 64, 224]) for gemm_ref / gemm_model32"""
    return stem_im2col(x_nhwc)[None], stem_filter_rows(w_oihw)[None]


def stem_wgrad_ref(dy_nhwc, x_nhwc, c0=None):
    """float64 filter gradient [64, 147] (+ c0) and its scale (the sum of the absolute contributions)"""
    col = stem_im2col(x_nhwc).double()
    d = dy_nhwc.reshape(-1, 64).double()
    ref, sc = stem_unpack(d.t() @ col), stem_unpack(d.abs().t() @ col.abs())
    if c0 is not None:
        ref, sc = ref + c0.double(), sc + c0.double().abs()
    return ref, sc


def stem_wgrad_model(dy_nhwc, x_nhwc, c0=None):
    """f32, plain pixel order: 32 pixels a step into one accumulator (gemm_harness._acc32)"""
    col = stem_im2col(x_nhwc)
    d = dy_nhwc.reshape(-1, 64)
    out = stem_unpack(G._acc32(d.t()[None], col.t()[None])[0])
    return out if c0 is None else c0.float() + out


# ------------------------------------------------------------------------------- pools
def pool_out(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def maxpool_ref(x_nhwc):
    """MaxPool2d(3, 2, 1) of [B, H, W, C] (any float dtype) -> (values [B, OH, OW, C] of x's dtype,
    window position [B, OH, OW, C] uint8 in 0..8).  Row-major scan with v > max || isnan(v): the
    first maximal element wins ties, the LAST NaN of a window wins; the first in-image element seeds"""
    B, H, W, C = x_nhwc.shape
    OH, OW = pool_out(H, W)
    dev = x_nhwc.device
    x = x_nhwc.float()
    mx = torch.full((B, OH, OW, C), float("-inf"), device=dev)
    arg = torch.full((B, OH, OW, C), 255, dtype=torch.int64, device=dev)
    oy, ox = torch.arange(OH, device=dev), torch.arange(OW, device=dev)
    for kh in range(3):
        iy = 2 * oy - 1 + kh
        for kw in range(3):
            ix = 2 * ox - 1 + kw
            ok = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]          # [OH, OW]
            v = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]                         # [B, OH, OW, C]
            upd = ok[None, :, :, None] & ((arg == 255) | (v > mx) | torch.isnan(v))
            mx = torch.where(upd, v, mx)
            arg = torch.where(upd, torch.full_like(arg, 3 * kh + kw), arg)
    return mx.to(x_nhwc.dtype), arg.to(torch.uint8)


def maxpool_bwd_ref(dy_nhwc, arg, H, W):
    """float64 [B, H, W, C]: every window's gradient goes to the element its position names"""
    B, OH, OW, C = dy_nhwc.shape
    dev = dy_nhwc.device
    a = arg.to(torch.int64)
    iy = (2 * torch.arange(OH, device=dev) - 1)[None, :, None, None] + a // 3
    ix = (2 * torch.arange(OW, device=dev) - 1)[None, None, :, None] + a % 3
    b = torch.arange(B, device=dev)[:, None, None, None]
    c = torch.arange(C, device=dev)[None, None, None, :]
    flat = ((b * H + iy) * W + ix) * C + c
    dx = torch.zeros(B * H * W * C, dtype=torch.float64, device=dev)
    dx.index_add_(0, flat.reshape(-1), dy_nhwc.double().reshape(-1))
    return dx.view(B, H, W, C)


def row_bins(Hh, n):
    return [((i * Hh) // n, ((i + 1) * Hh + n - 1) // n) for i in range(n)]


def row_pool_ref(f_nhwc, n):
    """float64 -> (out [B, n, C], scale): the mean over rows [y0, y1) and all columns"""
    x = f_nhwc.double()
    out = torch.stack([x[:, y0:y1].mean((1, 2)) for y0, y1 in row_bins(x.shape[1], n)], 1)
    sc = torch.stack([x[:, y0:y1].abs().mean((1, 2)) for y0, y1 in row_bins(x.shape[1], n)], 1)
    return out, sc


def row_pool_model(f_nhwc, n):
    """f32 in the kernel's order: rows then columns into one accumulator, x the f32 reciprocal"""
    x = f_nhwc.float()
    B, Hh, Ww, C = x.shape
    out = []
    for y0, y1 in row_bins(Hh, n):
        acc = torch.zeros(B, C, dtype=torch.float32, device=x.device)
        for y in range(y0, y1):
            for xx in range(Ww):
                acc = acc + x[:, y, xx]
        inv = (torch.ones((), dtype=torch.float32) / torch.tensor(float((y1 - y0) * Ww), dtype=torch.float32)).item()
        out.append(acc * torch.tensor(inv, dtype=torch.float32, device=x.device))
    return torch.stack(out, 1)


def _row_pool_bwd(dt, dout, Hh, Ww, n):
    B, _, C = dout.shape
    g = torch.zeros(B, Hh, C, dtype=dt, device=dout.device)
    s = torch.zeros(B, Hh, C, dtype=torch.float64, device=dout.device)
    for i, (y0, y1) in enumerate(row_bins(Hh, n)):
        if dt == torch.float64:
            inv = 1.0 / ((y1 - y0) * Ww)
        else:
            inv = (torch.ones((), dtype=dt) / torch.tensor(float((y1 - y0) * Ww), dtype=dt)).item()
        g[:, y0:y1] = g[:, y0:y1] + (dout[:, i].to(dt) * torch.tensor(inv, dtype=dt, device=dout.device))[:, None]
        s[:, y0:y1] = s[:, y0:y1] + (dout[:, i].double().abs() / ((y1 - y0) * Ww))[:, None]
    return g[:, :, None, :].expand(B, Hh, Ww, C), s[:, :, None, :].expand(B, Hh, Ww, C)


def row_pool_bwd_ref(dout, Hh, Ww, n):
    """float64 -> (dfmap [B, Hh, Ww, C], scale)"""
    return _row_pool_bwd(torch.float64, dout, Hh, Ww, n)


def row_pool_bwd_model(dout, Hh, Ww, n):
    """f32 in the kernel's order (bins in order, d x the f32 reciprocal), rounded to bf16"""
    return G.bf16r(_row_pool_bwd(torch.float32, dout, Hh, Ww, n)[0])


POOL_SIZES = (1, 2, 3, 4, 5, 7, 8)
# every (odd | even | 1) x (odd | even | 1) pair, and both 7 and 8 against each other
POOL_HW = ((1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 2), (2, 3), (3, 2), (3, 3), (4, 5), (5, 4), (4, 4), (5, 5),
           (7, 8), (8, 7), (7, 7), (8, 8), (1, 8), (7, 1), (2, 7), (5, 8), (3, 4), (4, 2))
POOL_B, POOL_C = (1, 3), (8, 24, 64)
POOL_KINDS = ("ties", "equal", "neginf", "nan")


def maxpool_input(kind, B, H, W, C, seed, device="cpu"):
    """bf16 [B, H, W, C]: "ties" quarter-integers in -1..1 (nine levels: many ties); "equal" one value
    everywhere; "neginf" ties with a third of the elements -inf (whole windows of -inf among them);
    "nan" ties with a fifth of the elements NaN"""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randint(-4, 5, (B, H, W, C), generator=g, device=device).float() / 4
    if kind == "equal":
        x = torch.full_like(x, -1.25)
    elif kind == "neginf":
        x[torch.rand(B, H, W, C, generator=g, device=device) < 0.34] = float("-inf")
        x[:, :2, :2] = float("-inf")
    elif kind == "nan":
        x[torch.rand(B, H, W, C, generator=g, device=device) < 0.2] = float("nan")
    return x.to(bf16)


ROW_POOL_HW = ((7, 7), (5, 3), (1, 4), (8, 1))
ROW_POOL_C, ROW_POOL_B = (8, 24, 2048), (1, 3)
