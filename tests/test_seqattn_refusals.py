"""The sequence-attention entry points without a GPU: every refused call raises before anything is
launched -- the library's own refusals (csrc/capi.hip mmu_seqattn_fwd / mmu_seqattn_bwd: called with
made-up non-null addresses, which a refused call never touches) and the argument checks of the
src/kernels.py wrappers (CPU tensors: an acceptable call gets as far as the device check, "need
tensors on a HIP", and no further, as in test_rowops_refusals.py).
"""
import pytest
import torch

from src import _native as N
from src import kernels as K
from src._native import NativeError

bf16, f32 = torch.bfloat16, torch.float32
BASELINE = "HIP"
P = 4096   # a made-up non-null, 16-byte aligned address: refused calls do not dereference it
S, NT, HEADS, D = 5, 3, 2, 64
E = HEADS * D
INT32_MAX = 2 ** 31 - 1


def capi_fwd(**over):
    a = dict(QKV=P, ld_qkv=3 * E + 8, O=P, ld_o=E + 4, LSE2=P, S=S, N=NT, heads=HEADS, D=D)
    a.update(over)
    N.call("mmu_seqattn_fwd", a["QKV"], a["ld_qkv"], a["O"], a["ld_o"], a["LSE2"], a["S"], a["N"], a["heads"],
           a["D"], None)


def capi_bwd(**over):
    a = dict(QKV=P, ld_qkv=3 * E + 8, O=P, ld_o=E + 4, dO=P, ld_do=E + 8, LSE2=P, delta=P, dQKV=P, ld_dqkv=3 * E + 4,
             S=S, N=NT, heads=HEADS, D=D)
    a.update(over)
    N.call("mmu_seqattn_bwd", a["QKV"], a["ld_qkv"], a["O"], a["ld_o"], a["dO"], a["ld_do"], a["LSE2"], a["delta"],
           a["dQKV"], a["ld_dqkv"], a["S"], a["N"], a["heads"], a["D"], None)


SHARED = [  # refused by both entry points with the same words
    (dict(QKV=None), "null pointer"),
    (dict(O=None), "null pointer"),
    (dict(LSE2=None), "null pointer"),
    (dict(S=0), "bad shape"),
    (dict(S=-1), "bad shape"),
    (dict(N=0), "bad shape"),
    (dict(heads=0), "bad shape"),
    (dict(heads=-2), "bad shape"),
    (dict(D=32), "head_dim 32 not in"),
    (dict(D=96), "head_dim 96 not in"),
    (dict(D=512), "head_dim 512 not in"),
    (dict(ld_qkv=3 * E - 8), "ld_qkv too small / unaligned"),
    (dict(ld_qkv=3 * E + 4), "ld_qkv too small / unaligned"),
    (dict(N=21846, heads=3, ld_qkv=3 * 3 * D, ld_o=3 * D, ld_do=3 * D, ld_dqkv=3 * 3 * D), r"N\*heads > 65535"),
    (dict(S=INT32_MAX + 1), r"S = 2147483648 exceeds 2147483584"),
    (dict(S=INT32_MAX - 62), r"S = 2147483585 exceeds 2147483584"),
    (dict(S=2 ** 40), r"S = 1099511627776 exceeds"),
    (dict(QKV=P + 8), r"QKV = 0x1008 must be 16-byte aligned"),
    (dict(QKV=P + 2), r"QKV = 0x1002 must be 16-byte aligned"),
    (dict(O=P + 4), r"O = 0x1004 must be 8-byte aligned"),
    (dict(O=P + 2), r"O = 0x1002 must be 8-byte aligned"),
    (dict(LSE2=P + 2), r"LSE2 = 0x1002 must be 4-byte aligned"),
]
FWD_ONLY = [
    (dict(ld_o=E - 4), "bad ld_o"),
    (dict(ld_o=E + 2), "bad ld_o"),
]
BWD_ONLY = [
    (dict(dO=None), "null pointer"),
    (dict(delta=None), "null pointer"),
    (dict(dQKV=None), "null pointer"),
    (dict(ld_dqkv=3 * E - 4), "bad ld"),
    (dict(ld_dqkv=3 * E + 2), "bad ld"),
    (dict(ld_o=E + 2), "bad ld"),
    (dict(ld_do=E + 4), "bad ld"),
    (dict(ld_o=E - 4), "ld_o = 124 is smaller than heads\\*head_dim = 128"),
    (dict(ld_o=0), "ld_o = 0 is smaller than heads\\*head_dim = 128"),
    (dict(ld_do=E - 8), "ld_do = 120 is smaller than heads\\*head_dim = 128"),
    (dict(ld_do=-8), "ld_do = -8 is smaller than heads\\*head_dim = 128"),
    (dict(dO=P + 8), "dO = 0x1008 must be 16-byte aligned"),
    (dict(dQKV=P + 4), "dQKV = 0x1004 must be 8-byte aligned"),
    (dict(delta=P + 1), "delta = 0x1001 must be 4-byte aligned"),
    # the first S at which 5 items per sample need 2^31 blocks of 4 (one less: exactly 2^31 - 1 blocks)
    (dict(S=1717986918, N=5, heads=1), r"S\*N\*heads = 8589934590 needs more than 2147483647 delta blocks"),
    (dict(S=INT32_MAX - 63, N=3, heads=2), r"S\*N\*heads = 12884901504 needs more than 2147483647 delta blocks"),
    (dict(S=2 ** 30, N=3, heads=3, D=256, ld_qkv=9 * 256, ld_o=768, ld_do=768, ld_dqkv=9 * 256), "delta blocks"),
]
FWD = SHARED + FWD_ONLY
BWD = SHARED + BWD_ONLY


@pytest.mark.parametrize("i", range(len(FWD)))
def test_library_refuses_forward(i):
    over, msg = FWD[i]
    with pytest.raises(NativeError, match="mmu_seqattn_fwd: .*" + msg):
        capi_fwd(**over)


@pytest.mark.parametrize("i", range(len(BWD)))
def test_library_refuses_backward(i):
    over, msg = BWD[i]
    with pytest.raises(NativeError, match="mmu_seqattn_bwd: .*" + msg):
        capi_bwd(**over)


def test_forward_takes_the_row_count_the_backward_grid_refuses():
    """the delta-grid bound belongs to the backward alone: the forward's refusals at the same shape are
    about other arguments (it is never launched here: QKV is refused last, for its alignment)"""
    with pytest.raises(NativeError, match="QKV = 0x1008 must be 16-byte aligned"):
        capi_fwd(S=INT32_MAX - 63, N=2, heads=2, QKV=P + 8)


# ------------------------------------------------------------------------------- wrappers
def z(r, c, dt=bf16, ld=None):
    return torch.zeros(r, c, dtype=dt) if ld is None else torch.zeros(r, ld, dtype=dt)[:, :c]


def wrap_fwd(**over):
    a = dict(qkv=z(S * NT, 3 * E), O=z(S * NT, E), lse2=torch.zeros(NT * HEADS, S), S=S, N=NT, heads=HEADS)
    a.update(over)
    K.seqattn_fwd(a["qkv"], a["O"], a["lse2"], a["S"], a["N"], a["heads"])


def wrap_bwd(**over):
    a = dict(qkv=z(S * NT, 3 * E), O=z(S * NT, E), dO=z(S * NT, E), lse2=torch.zeros(NT * HEADS, S),
             delta=torch.zeros(NT * HEADS, S), dqkv=z(S * NT, 3 * E), S=S, N=NT, heads=HEADS)
    a.update(over)
    K.seqattn_bwd(a["qkv"], a["O"], a["dO"], a["lse2"], a["delta"], a["dqkv"], a["S"], a["N"], a["heads"])


ROWS = S * NT
WRAP_SHARED = [
    (dict(heads=5), r"3E divisible by 3\*heads = 15"),
    (dict(heads=0), "heads = 0 must be positive"),
    (dict(S=0), "S = 0, N = 3, heads = 2 must be positive"),
    (dict(N=-1), "N = -1, heads = 2 must be positive"),
    (dict(qkv=z(ROWS, 3 * E, f32)), "qkv: expected torch.bfloat16, got torch.float32"),
    (dict(qkv=torch.zeros(ROWS * 3 * E, dtype=bf16)), "qkv must be 2-D"),
    (dict(qkv=z(ROWS, 6 * E)[:, ::2]), "inner stride of qkv must be 1, got 2"),
    (dict(qkv=z(ROWS - 1, 3 * E)), "qkv has 14 rows, S\\*N = 15 are needed"),
    (dict(O=z(ROWS, E, f32)), "O: expected torch.bfloat16, got torch.float32"),
    (dict(O=z(ROWS, E, torch.float16)), "O: expected torch.bfloat16, got torch.float16"),
    (dict(O=z(ROWS, E - 8)), "O must be 2-D of width 128, got \\(15, 120\\)"),
    (dict(O=z(ROWS, 3 * E)), "O must be 2-D of width 128"),
    (dict(O=z(E, ROWS).t()), "inner stride of O must be 1, got 15"),
    (dict(O=z(ROWS - 1, E)), "O has 14 rows, S\\*N = 15 are needed"),
    (dict(lse2=torch.zeros(NT * HEADS, S, dtype=torch.float64)), "lse2: expected torch.float32, got torch.float64"),
    (dict(lse2=torch.zeros(NT * HEADS, S, dtype=bf16)), "lse2: expected torch.float32, got torch.bfloat16"),
    (dict(lse2=torch.zeros(NT * HEADS, 2 * S)[:, ::2]), "lse2 must be contiguous"),
]
WRAP_BWD_ONLY = [
    (dict(dO=z(ROWS, E, f32)), "dO: expected torch.bfloat16, got torch.float32"),
    (dict(dO=z(ROWS, E + 8)), "dO must be 2-D of width 128, got \\(15, 136\\)"),
    (dict(dO=z(ROWS, 2 * E)[:, ::2]), "inner stride of dO must be 1, got 2"),
    (dict(dO=z(ROWS - 3, E)), "dO has 12 rows, S\\*N = 15 are needed"),
    (dict(dqkv=z(ROWS, 3 * E, f32)), "dqkv: expected torch.bfloat16, got torch.float32"),
    (dict(dqkv=z(ROWS, E)), "dqkv must be 2-D of width 384, got \\(15, 128\\)"),
    (dict(dqkv=z(3 * E, ROWS).t()), "inner stride of dqkv must be 1, got 15"),
    (dict(dqkv=z(ROWS - 1, 3 * E)), "dqkv has 14 rows, S\\*N = 15 are needed"),
    (dict(delta=torch.zeros(NT * HEADS, S, dtype=torch.float64)), "delta: expected torch.float32, got torch.float64"),
    (dict(delta=torch.zeros(NT * HEADS, 2 * S)[:, ::2]), "delta must be contiguous"),
]
WRAP_FWD = WRAP_SHARED
WRAP_BWD = WRAP_SHARED + WRAP_BWD_ONLY


@pytest.mark.parametrize("i", range(len(WRAP_FWD)))
def test_wrapper_refuses_forward(i):
    over, msg = WRAP_FWD[i]
    with pytest.raises(NativeError, match="seqattn_fwd.*" + msg):
        wrap_fwd(**over)


@pytest.mark.parametrize("i", range(len(WRAP_BWD)))
def test_wrapper_refuses_backward(i):
    over, msg = WRAP_BWD[i]
    with pytest.raises(NativeError, match="seqattn_bwd.*" + msg):
        wrap_bwd(**over)


def test_wrapper_refuses_short_vectors():
    """the two size checks the wrappers had before (ValueError, as before)"""
    short = torch.zeros(NT * HEADS * S - 1)
    with pytest.raises(ValueError, match="seqattn_fwd: lse2 too small"):
        wrap_fwd(lse2=short)
    with pytest.raises(ValueError, match="seqattn_bwd: lse2 too small"):
        wrap_bwd(lse2=short)
    with pytest.raises(ValueError, match="seqattn_bwd: delta too small"):
        wrap_bwd(delta=short)


def test_wrappers_accept_the_baseline():
    """tight tensors, padded views (row stride > width), spare rows and spare vector elements all reach
    the device check"""
    pad = dict(qkv=z(ROWS, 3 * E, ld=3 * E + 8), O=z(ROWS, E, ld=E + 4))
    spare = dict(qkv=z(ROWS + 2, 3 * E), O=z(ROWS + 1, E), lse2=torch.zeros(NT * HEADS * S + 3))
    for over in (dict(), pad, spare):
        with pytest.raises(NativeError, match=BASELINE):
            wrap_fwd(**over)
    pad.update(dO=z(ROWS, E, ld=E + 8), dqkv=z(ROWS, 3 * E, ld=3 * E + 4))
    spare.update(dO=z(ROWS + 1, E), dqkv=z(ROWS + 4, 3 * E), delta=torch.zeros(NT * HEADS * S + 1))
    for over in (dict(), pad, spare):
        with pytest.raises(NativeError, match=BASELINE):
            wrap_bwd(**over)
