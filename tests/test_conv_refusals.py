"""The conv, stem and pool entry points without a GPU: every refused call raises NativeError before
anything is launched -- the library's own refusals (csrc/capi.hip: called with made-up non-null
addresses, which a refused call never touches) and the dtype / shape / layout / alignment checks of
the src/kernels.py wrappers, which run before the device check (CPU tensors: an acceptable call gets
as far as "need tensors on a HIP" and no further, as in test_gemm_refusals.py).
"""
import pytest
import torch

from src import _native as N
from src import kernels as K
from src._native import NativeError

bf16, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
z = torch.zeros
BASELINE = "HIP"
P = 4096     # a made-up non-null, 16-B aligned address: refused calls do not dereference it
Q = P + 8    # and one that is not 16-B aligned
WS = 1 << 20


def conv(fn="mmu_conv_implicit", **o):
    a = dict(X=P, Wk=P, Y=P, n=1, H=16, W=16, C=64, N=64, ks=3, s=1, stats=P, ws=P, bn_x=P, bn_mask=None, bn_mean=P)
    a.update(o)
    geo = (a["X"], a["Wk"], a["Y"], a["n"], a["H"], a["W"], a["C"], a["N"])
    if fn == "mmu_conv_implicit":
        N.call(fn, *geo, a["ks"], a["s"], a["ws"], WS, None)
    elif fn == "mmu_conv_implicit_stats":
        N.call(fn, *geo, a["ks"], a["s"], a["stats"], a["ws"], WS, None)
    elif fn == "mmu_conv3x3_implicit":
        N.call(fn, *geo, a["ws"], WS, None)
    else:
        N.call(fn, *geo, a["bn_x"], a["bn_mask"], a["bn_mean"], a["stats"], a["ws"], WS, None)


def wgrad(fn="mmu_conv_wgrad", **o):
    a = dict(dY=P, X=P, dW=P, n=1, H=8, W=8, Cin=256, Cout=128, ks=3, s=1, ws=P)
    a.update(o)
    geo = (a["dY"], a["X"], a["dW"], a["n"], a["H"], a["W"], a["Cin"], a["Cout"])
    if fn == "mmu_conv_wgrad":
        N.call(fn, *geo, a["ks"], a["s"], 0, a["ws"], WS, None)
    else:
        N.call(fn, *geo, 0, a["ws"], WS, None)


def stem_fwd(**o):
    a = dict(X=P, Wk=P, Y=P, n=1, H=8, W=8)
    a.update(o)
    N.call("mmu_stem_conv_fwd", a["X"], a["Wk"], a["Y"], a["n"], a["H"], a["W"], None)


def stem_wgrad(**o):
    a = dict(dY=P, X=P, dW=P, n=1, H=8, W=8, ws=P, ws_floats=1 << 30)
    a.update(o)
    N.call("mmu_stem_conv_wgrad", a["dY"], a["X"], a["dW"], a["n"], a["H"], a["W"], 0, a["ws"], a["ws_floats"], None)


def maxpool(fn="mmu_maxpool_fwd", **o):
    a = dict(x=P, y=P, am=P, B=1, H=4, W=4, C=8)
    a.update(o)
    if fn == "mmu_maxpool_fwd":
        N.call(fn, a["x"], a["B"], a["H"], a["W"], a["C"], a["y"], a["am"], None)
    else:
        N.call(fn, a["y"], a["am"], a["B"], a["H"], a["W"], a["C"], a["x"], None)


def row_pool(fn="mmu_row_pool_fwd", **o):
    a = dict(f=P, v=P, B=1, Hh=4, Ww=4, C=8, n=2)
    a.update(o)
    if fn == "mmu_row_pool_fwd":
        N.call(fn, a["f"], a["B"], a["Hh"], a["Ww"], a["C"], a["n"], a["v"], None)
    else:
        N.call(fn, a["v"], a["B"], a["Hh"], a["Ww"], a["C"], a["n"], a["f"], None)


ALIGNED = "16-B aligned"
CAPI_REFUSALS = [
    # ---- the forward / data-gradient product
    (conv, dict(X=None), "null pointer"), (conv, dict(Wk=None), "null pointer"), (conv, dict(Y=None), "null pointer"),
    (conv, dict(X=Q), ALIGNED), (conv, dict(Wk=Q), ALIGNED), (conv, dict(Y=Q), ALIGNED), (conv, dict(ws=Q), ALIGNED),
    (conv, dict(fn="mmu_conv3x3_implicit", X=Q), ALIGNED),
    (conv, dict(fn="mmu_conv_implicit_stats", stats=None), "null stats"),
    (conv, dict(fn="mmu_conv_implicit_stats", stats=Q), ALIGNED),
    (conv, dict(fn="mmu_conv3x3_implicit_bnb", bn_x=None), "null table / bn_x / bn_mean"),
    (conv, dict(fn="mmu_conv3x3_implicit_bnb", bn_x=Q), ALIGNED),
    (conv, dict(fn="mmu_conv3x3_implicit_bnb", bn_mean=Q), ALIGNED),
    (conv, dict(fn="mmu_conv3x3_implicit_bnb", stats=Q), ALIGNED),
    (conv, dict(C=96), r"C % 64 == 0"), (conv, dict(C=32), r"C % 64 == 0"),
    (conv, dict(N=96), r"N % 64 == 0"), (conv, dict(N=0), r"N % 64 == 0"),
    (conv, dict(H=15), "map size out of range"),                       # M = 240 < 256
    (conv, dict(ks=1, s=2), "map size out of range"),                  # M = 64
    (conv, dict(ks=2), "bad geometry"), (conv, dict(ks=5), "bad geometry"), (conv, dict(ks=0), "bad geometry"),
    (conv, dict(s=0), "bad geometry"), (conv, dict(s=5), "bad geometry"), (conv, dict(s=-1), "bad geometry"),
    (conv, dict(n=0), "bad geometry"), (conv, dict(W=0), "bad geometry"),
    # ---- the weight gradient
    (wgrad, dict(dY=None), "null pointer"), (wgrad, dict(X=None), "null pointer"), (wgrad, dict(dW=None), "null pointer"),
    (wgrad, dict(dY=Q), ALIGNED), (wgrad, dict(X=Q), ALIGNED), (wgrad, dict(dW=Q), ALIGNED), (wgrad, dict(ws=Q), ALIGNED),
    (wgrad, dict(fn="mmu_conv3x3_wgrad", dW=Q), ALIGNED),
    (wgrad, dict(Cin=128), r"Cin % 256 == 0"), (wgrad, dict(Cin=320), r"Cin % 256 == 0"),
    (wgrad, dict(Cout=64), r"Cout % 128 == 0"), (wgrad, dict(Cout=192), r"Cout % 128 == 0"),
    (wgrad, dict(ks=2), "bad geometry"), (wgrad, dict(s=0), "bad geometry"), (wgrad, dict(s=5), "bad geometry"),
    # ---- the stem
    (stem_fwd, dict(X=None), "null pointer"), (stem_fwd, dict(Y=None), "null pointer"),
    (stem_fwd, dict(X=Q), ALIGNED), (stem_fwd, dict(Wk=Q), ALIGNED), (stem_fwd, dict(Y=Q), ALIGNED),
    (stem_fwd, dict(n=(1 << 20) + 1, H=1, W=1), "bad image batch"),
    (stem_fwd, dict(n=0), "bad image batch"), (stem_fwd, dict(H=0), "bad image batch"),
    (stem_fwd, dict(n=1 << 16, H=224, W=224), "bad image batch"),     # 3 n H W >= 2^31
    (stem_wgrad, dict(ws=None), "null pointer"), (stem_wgrad, dict(dW=None), "null pointer"),
    (stem_wgrad, dict(dY=Q), ALIGNED), (stem_wgrad, dict(X=Q), ALIGNED), (stem_wgrad, dict(dW=Q), ALIGNED),
    (stem_wgrad, dict(ws=Q), ALIGNED),
    (stem_wgrad, dict(n=(1 << 20) + 1, H=1, W=1), "bad image batch"),
    (stem_wgrad, dict(H=2, W=2, ws_floats=64 * 224 - 1), "ws needs"),  # one tile: one [64][224] slab
    (stem_wgrad, dict(ws_floats=0), "ws needs"),
    # ---- the pools
    (maxpool, dict(x=None), "bad args"), (maxpool, dict(C=12), "bad args"), (maxpool, dict(C=0), "bad args"),
    (maxpool, dict(H=65537), "bad args"), (maxpool, dict(W=65537), "bad args"),
    (maxpool, dict(x=Q), ALIGNED), (maxpool, dict(y=Q), ALIGNED), (maxpool, dict(am=Q), ALIGNED),
    (maxpool, dict(fn="mmu_maxpool_bwd", C=12), "bad args"), (maxpool, dict(fn="mmu_maxpool_bwd", H=65537), "bad args"),
    (maxpool, dict(fn="mmu_maxpool_bwd", x=Q), ALIGNED), (maxpool, dict(fn="mmu_maxpool_bwd", y=Q), ALIGNED),
    (maxpool, dict(fn="mmu_maxpool_bwd", am=Q), ALIGNED),
    (row_pool, dict(n=0), "bad args"), (row_pool, dict(n=-1), "bad args"), (row_pool, dict(n=5), "bad args"),
    (row_pool, dict(C=12), "bad args"), (row_pool, dict(f=None), "bad args"),
    (row_pool, dict(f=Q), ALIGNED), (row_pool, dict(v=Q), ALIGNED),
    (row_pool, dict(fn="mmu_row_pool_bwd", n=0), "bad args"), (row_pool, dict(fn="mmu_row_pool_bwd", n=5), "bad args"),
    (row_pool, dict(fn="mmu_row_pool_bwd", f=Q), ALIGNED), (row_pool, dict(fn="mmu_row_pool_bwd", v=Q), ALIGNED),
]


@pytest.mark.parametrize("i", range(len(CAPI_REFUSALS)))
def test_library_refuses(i):
    fn, over, msg = CAPI_REFUSALS[i]
    with pytest.raises(NativeError, match=msg):
        fn(**over)


def test_abi_is_unchanged():
    assert N.load().mmu_version() == 4 and N.ABI_VERSION == 4


# ------------------------------------------------------------------------------- the wrappers
def cl(n, c, h, w, dtype=bf16, off=0):
    """a channels-last [n, c, h, w] map, `off` elements into its storage"""
    return z(n * h * w * c + off, dtype=dtype)[off:].view(n, h, w, c).permute(0, 3, 1, 2)


n_, C_, H_, W_, No = 1, 64, 16, 16, 128


def w_conv(**o):
    a = dict(X=cl(n_, C_, H_, W_), Wk=z(No, 3, 3, C_, dtype=bf16), Y=cl(n_, No, H_, W_), ks=3, s=1, stats=None)
    a.update(o)
    K.conv_implicit(a["X"], a["Wk"], a["Y"], a["ks"], a["s"], a["stats"])


def w_bnb(**o):
    a = dict(X=cl(n_, C_, H_, W_), Wk=z(No, 3, 3, C_, dtype=bf16), Y=cl(n_, No, H_, W_), x=cl(n_, No, H_, W_),
             mean=z(No), table=z(4 * No * 2))
    a.update(o)
    K.conv3x3_implicit(a["X"], a["Wk"], a["Y"], bnb=(a["x"], None, a["mean"]), table=a["table"])


def w_wgrad(**o):
    a = dict(dY=cl(n_, No, H_, W_), X=cl(n_, C_, H_, W_), dW=cl(No, C_, 3, 3, f32), ks=3, s=1)
    a.update(o)
    K.conv_wgrad(a["dY"], a["X"], a["dW"], a["ks"], a["s"])


def w_stem(**o):
    a = dict(X=cl(2, 3, 9, 9), Wk=cl(64, 3, 7, 7), Y=cl(2, 64, 5, 5))
    a.update(o)
    K.stem_conv_fwd(a["X"], a["Wk"], a["Y"])


def w_stem_wgrad(**o):
    a = dict(dY=cl(2, 64, 5, 5), X=cl(2, 3, 9, 9), dW=cl(64, 3, 7, 7, f32))
    a.update(o)
    K.stem_conv_wgrad(a["dY"], a["X"], a["dW"])


def w_maxpool(**o):
    a = dict(x=cl(2, 8, 5, 4), y=cl(2, 8, 3, 2), am=z(2 * 3 * 2 * 8, dtype=u8))
    a.update(o)
    K.maxpool_fwd(a["x"], a["y"], a["am"])


def w_maxpool_bwd(**o):
    a = dict(dy=cl(2, 8, 3, 2), am=z(2 * 3 * 2 * 8, dtype=u8), dx=cl(2, 8, 5, 4))
    a.update(o)
    K.maxpool_bwd(a["dy"], a["am"], a["dx"])


def w_row_fwd(**o):
    a = dict(f=z(2, 5, 3, 8, dtype=bf16), n=3, out=z(2, 3, 8))
    a.update(o)
    K.row_pool_fwd(a["f"], a["n"], a["out"])


def w_row_bwd(**o):
    a = dict(d=z(2, 3, 8), n=3, df=z(2, 5, 3, 8, dtype=bf16))
    a.update(o)
    K.row_pool_bwd(a["d"], a["n"], a["df"])


ACCEPTED = [
    (w_conv, {}), (w_conv, dict(Wk=cl(No, C_, 3, 3))),                                  # both filter shapes
    (w_conv, dict(ks=1, Wk=z(No, 1, 1, C_, dtype=bf16))), (w_conv, dict(s=2, Y=cl(n_, No, 8, 8))),
    (w_conv, dict(stats=z(4 * No * 2))), (w_bnb, {}), (w_wgrad, {}),
    (w_wgrad, dict(ks=1, s=2, dY=cl(n_, No, 8, 8), dW=cl(No, C_, 1, 1, f32))),
    (w_stem, {}), (w_stem_wgrad, {}), (w_maxpool, {}), (w_maxpool_bwd, {}), (w_row_fwd, {}), (w_row_bwd, {}),
    (w_row_fwd, dict(out=z(2 * 3 * 8))), (w_conv, dict(X=cl(n_, C_, H_, W_, off=8))),    # 16 B into the storage
]

WRAP_REFUSALS = [
    # ---- conv_implicit
    (w_conv, dict(X=cl(n_, C_, H_, W_, f32)), "conv_implicit X: expected torch.bfloat16"),
    (w_conv, dict(Wk=z(No, 3, 3, C_)), "conv_implicit Wk: expected torch.bfloat16"),
    (w_conv, dict(Y=cl(n_, No, H_, W_, f32)), "conv_implicit: X channels-last"),
    (w_conv, dict(X=z(n_, C_, H_, W_, dtype=bf16)), "conv_implicit: X channels-last"),          # NCHW-contiguous
    (w_conv, dict(Y=z(n_, No, H_, W_, dtype=bf16)), "conv_implicit: X channels-last"),
    (w_conv, dict(Y=cl(n_, No, H_, W_ - 1)), "conv_implicit: X channels-last"),                 # wrong Y shape
    (w_conv, dict(s=2), "conv_implicit: X channels-last"),                                      # Y of the stride-1 conv
    (w_conv, dict(Wk=z(No, C_, 3, 3, dtype=bf16)), "conv_implicit: X channels-last"),           # an NCHW filter
    (w_conv, dict(Wk=z(No, 3, 3, C_ + 8, dtype=bf16)), "conv_implicit: X channels-last"),
    (w_conv, dict(X=z(n_ * H_ * W_, C_, dtype=bf16)), "4-D"),
    (w_conv, dict(stats=z(3 * No * 2)), "stats table too small"),
    (w_conv, dict(stats=z(4 * No * 2, dtype=torch.float64)), "stats table too small"),
    (w_conv, dict(X=cl(n_, C_, H_, W_, off=4)), "not 16-B aligned"),
    (w_conv, dict(Y=cl(n_, No, H_, W_, off=4)), "not 16-B aligned"),
    (w_conv, dict(Wk=z(No * 9 * C_ + 4, dtype=bf16)[4:].view(No, 3, 3, C_)), "not 16-B aligned"),
    (w_conv, dict(stats=z(4 * No * 2 + 2)[2:]), "not 16-B aligned"),
    # ---- conv3x3_implicit with the BatchNorm backward table
    (w_bnb, dict(x=cl(n_, No, H_, W_ - 1)), "conv3x3_implicit bnb: X / Y / x"),
    (w_bnb, dict(Wk=cl(No, C_, 3, 3)), "conv3x3_implicit bnb: X / Y / x"),
    (w_bnb, dict(table=z(3 * No * 2)), "table too small"),
    (w_bnb, dict(mean=z(No - 1)), "of a training BatchNorm"),
    (w_bnb, dict(x=cl(n_, No, H_, W_, f32)), "of a training BatchNorm"),
    (w_bnb, dict(x=cl(n_, No, H_, W_, off=4)), "not 16-B aligned"),
    (w_bnb, dict(mean=z(No + 1)[1:]), "not 16-B aligned"),
    # ---- conv_wgrad
    (w_wgrad, dict(X=cl(n_, C_, H_, W_, f32)), "conv_wgrad X: expected torch.bfloat16"),
    (w_wgrad, dict(dY=cl(n_, No, H_, W_, f32)), "conv_wgrad dY: expected torch.bfloat16"),
    (w_wgrad, dict(dW=cl(No, C_, 3, 3, bf16)), "conv_wgrad: X channels-last"),
    (w_wgrad, dict(dW=z(No, C_, 3, 3)), "conv_wgrad: X channels-last"),                         # an NCHW gradient
    (w_wgrad, dict(dW=cl(No, C_, 1, 1, f32)), "conv_wgrad: X channels-last"),                   # wrong dW shape
    (w_wgrad, dict(dY=cl(n_, No, H_ - 1, W_)), "conv_wgrad: X channels-last"),
    (w_wgrad, dict(X=z(n_, C_, H_, W_, dtype=bf16)), "conv_wgrad: X channels-last"),
    (w_wgrad, dict(dW=cl(No, C_, 3, 3, f32, off=2)), "not 16-B aligned"),
    (w_wgrad, dict(dY=cl(n_, No, H_, W_, off=4)), "not 16-B aligned"),
    # ---- the stem
    (w_stem, dict(X=cl(2, 3, 9, 9, f32)), "stem_conv_fwd: X must be channels-last bf16"),
    (w_stem, dict(X=z(2, 3, 9, 9, dtype=bf16)), "stem_conv_fwd: X must be channels-last bf16"),
    (w_stem, dict(X=cl(2, 4, 9, 9)), "stem_conv_fwd: X must be channels-last bf16"),
    (w_stem, dict(Wk=z(64, 3, 7, 7, dtype=bf16)), "Wk must be channels-last bf16"),
    (w_stem, dict(Y=cl(2, 64, 5, 4)), "Y must be channels-last bf16"),
    (w_stem, dict(Y=cl(2, 64, 5, 5, f32)), "Y must be channels-last bf16"),
    (w_stem, dict(Y=cl(2, 64, 5, 5, off=4)), "not 16-B aligned"),
    (w_stem, dict(X=cl(2, 3, 9, 9, off=1)), "not 16-B aligned"),
    (w_stem_wgrad, dict(dY=cl(2, 64, 4, 5)), "dY must be channels-last bf16"),
    (w_stem_wgrad, dict(dW=z(64, 3, 7, 7)), "dW must be channels-last f32"),
    (w_stem_wgrad, dict(dW=cl(64, 3, 7, 7, bf16)), "dW must be channels-last f32"),
    (w_stem_wgrad, dict(dW=cl(64, 3, 7, 7, f32, off=1)), "not 16-B aligned"),
    # ---- the max pool
    (w_maxpool, dict(x=cl(2, 8, 5, 4, f32)), "maxpool x: expected torch.bfloat16"),
    (w_maxpool, dict(x=z(2, 8, 5, 4, dtype=bf16)), "x must be a channels-last"),
    (w_maxpool, dict(y=cl(2, 8, 2, 2)), "MaxPool2d"),
    (w_maxpool, dict(am=z(2 * 3 * 2 * 8 - 1, dtype=u8)), "argmax must be a contiguous uint8"),
    (w_maxpool, dict(am=z(2 * 3 * 2 * 8, dtype=torch.int64)), "argmax must be a contiguous uint8"),
    (w_maxpool, dict(am=z(2 * 3 * 2 * 8 + 8, dtype=u8)[8:]), "not 16-B aligned"),
    (w_maxpool, dict(x=cl(2, 8, 5, 4, off=4)), "not 16-B aligned"),
    (w_maxpool_bwd, dict(dx=z(2, 8, 5, 4, dtype=bf16)), "dx must be a channels-last"),
    (w_maxpool_bwd, dict(dy=cl(2, 8, 3, 3)), "MaxPool2d"),
    (w_maxpool_bwd, dict(am=z(2 * 3 * 2 * 8 + 1, dtype=u8)), "argmax must be a contiguous uint8"),
    (w_maxpool_bwd, dict(dy=cl(2, 8, 3, 2, off=4)), "not 16-B aligned"),
    # ---- the row pool
    (w_row_fwd, dict(f=z(2, 5, 3, 8)), "row_pool_fwd fmap: expected torch.bfloat16"),
    (w_row_fwd, dict(f=z(2, 8, 5, 3, dtype=bf16).permute(0, 2, 3, 1)), "fmap must be a contiguous"),   # an NCHW map, permuted
    (w_row_fwd, dict(f=z(2 * 5, 3, 8, dtype=bf16)), "fmap must be a contiguous"),
    (w_row_fwd, dict(f=z(2, 5, 3, 12, dtype=bf16), out=z(2, 3, 12)), r"C % 8 == 0"),
    (w_row_fwd, dict(n=0), "n = 0 rows must be within 1 .. Hh = 5"),
    (w_row_fwd, dict(n=6, out=z(2, 6, 8)), "n = 6 rows must be within 1 .. Hh = 5"),
    (w_row_fwd, dict(out=z(2, 3, 8, dtype=bf16)), "row_pool_fwd out: expected torch.float32"),
    (w_row_fwd, dict(out=z(2, 2, 8)), "out must be a contiguous f32 tensor of B \\* n \\* C = 48"),      # a short out
    (w_row_fwd, dict(out=z(2, 3, 16)[:, :, :8]), "out must be a contiguous f32"),
    (w_row_fwd, dict(out=z(2 * 3 * 8 + 2)[2:]), "not 16-B aligned"),
    (w_row_fwd, dict(f=z(2 * 5 * 3 * 8 + 4, dtype=bf16)[4:].view(2, 5, 3, 8)), "not 16-B aligned"),
    (w_row_bwd, dict(df=z(2, 5, 3, 8)), "row_pool_bwd fmap: expected torch.bfloat16"),
    (w_row_bwd, dict(df=z(2, 8, 5, 3, dtype=bf16).permute(0, 2, 3, 1)), "fmap must be a contiguous"),
    (w_row_bwd, dict(d=z(2, 3, 8, dtype=torch.float64)), "row_pool_bwd dout: expected torch.float32"),
    (w_row_bwd, dict(d=z(2, 4, 8)), "dout must be a contiguous f32"),
    (w_row_bwd, dict(n=6), "n = 6 rows must be within"),
    (w_row_bwd, dict(d=z(2 * 3 * 8 + 1)[1:]), "not 16-B aligned"),
]


@pytest.mark.parametrize("i", range(len(ACCEPTED)))
def test_wrapper_accepts_the_baseline(i):
    fn, over = ACCEPTED[i]
    with pytest.raises(NativeError, match=BASELINE):
        fn(**over)


@pytest.mark.parametrize("i", range(len(WRAP_REFUSALS)))
def test_wrapper_refuses(i):
    fn, over, msg = WRAP_REFUSALS[i]
    with pytest.raises(NativeError, match=msg) as ei:
        fn(**over)
    assert BASELINE not in str(ei.value)
