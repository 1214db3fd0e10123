"""The extent checks of kernels.gemm (src/kernels.py, _gemm_extents): a call whose last element,
(batch - 1) stride + (rows - 1) ld + width from a tensor's data pointer, lies outside that tensor's
storage is refused before anything is launched.  The checks are integer arithmetic on shapes and
storages, so the tensors here live on the CPU: a call whose arguments are all acceptable gets as
far as the device check ("need tensors on a HIP") and no further -- the baseline of every refusal.
The alignment refusals of the C side are in test_gemm_edges_gpu.py.
"""
import pytest
import torch

from src import kernels as K
from src._native import NativeError

bf16, f32 = torch.bfloat16, torch.float32
M, N, Kd, B = 130, 128, 64, 2
BASELINE = "HIP"
z = torch.zeros


def args(**over):
    a = dict(A=z(B * M, Kd, dtype=bf16), lda=Kd, ak=True, Bm=z(B * N, Kd, dtype=bf16), ldb=Kd, bk=True,
             C=z(B * M, N, dtype=bf16), ldc=N, M=M, N=N, K=Kd, batch=B, sA=M * Kd, sB=N * Kd, sC=M * N,
             kind=K.EPI_STORE, epi={})
    a.update(over)
    return a


def call(a):
    K.gemm(a["A"], a["lda"], a["ak"], a["Bm"], a["ldb"], a["bk"], a["C"], a["ldc"], a["M"], a["N"], a["K"],
           epi=K.epilogue(a["kind"], **a["epi"]), batch=a["batch"], sA=a["sA"], sB=a["sB"], sC=a["sC"])


def res(**kw):
    return dict(kind=K.EPI_ADD_RES, epi=dict(dict(residual=z(B * M, N, dtype=bf16), ldr=N, res_bstride=M * N), **kw))


def ln(**kw):
    e = dict(residual=z(B * M, N), ldr=N, res_bstride=M * N,
             res_ln=(z(B * M), z(B * M), z(B * N), z(B * N)), res_ln_bstride=N)
    e.update(kw)
    return dict(kind=K.EPI_BIAS_DROP_RES, C=z(B * M, N), epi=e)


def bnb(**kw):
    x = z(1, N, M, 1, dtype=bf16).contiguous(memory_format=torch.channels_last)
    e = dict(bn=(x, None, z(N)), colsum=z(3 * N * 2))       # (a mask would be device-checked by epilogue() itself)
    e.update(kw)
    return dict(kind=K.EPI_STORE_BNB, bk=False, Bm=z(Kd, N, dtype=bf16), ldb=N, batch=1, epi=e)


ACCEPTED = [
    {}, dict(epi=dict(bias=z(B * N), bias_bstride=N)), res(), ln(), bnb(),
    dict(sB=0, Bm=z(N, Kd, dtype=bf16)),                                           # one B for every batch item
    dict(A=z(Kd, B * M, dtype=bf16), ak=False, lda=B * M, sA=M, M=128, sC=128 * N),   # M-major, items side by side
    dict(A=z(B * M + 1, Kd, dtype=bf16)[1:]),                                      # a view that starts inside its storage
    dict(kind=K.EPI_BIAS_GELU, epi=dict(aux=z(B * M, N + 8, dtype=bf16), ldx=N + 8, aux_bstride=M * (N + 8))),
    dict(kind=K.EPI_DGELU, epi=dict(aux=z(B * M, N, dtype=bf16), aux_bstride=M * N, colsum=z(B * N), colsum_bstride=N)),
    dict(kind=K.EPI_STORE_STATS, batch=1, epi=dict(colsum=z(3 * N * 2))),
    dict(kind=K.EPI_ADD_RES, batch=1, epi=dict(residual=z(M, N, dtype=bf16), res_mask=z(M * N // 8, dtype=torch.uint8))),
]

REFUSED = [
    ("gemm A", dict(A=z(B * M - 1, Kd, dtype=bf16))),
    ("gemm A", dict(lda=Kd + 8)),                                                  # a pitch the tensor does not have
    ("gemm A", dict(sA=M * Kd + 8)),
    ("gemm A", dict(A=z(B * M, Kd, dtype=bf16)[1:])),                              # a view that starts one row in
    ("gemm A", dict(ak=False, lda=M, sA=M * Kd, M=128, sC=128 * N, K=Kd + 64)),
    ("gemm B", dict(Bm=z(B * N, Kd - 8, dtype=bf16))),
    ("gemm B", dict(bk=False, ldb=N, K=Kd + 1, ak=False, lda=128, M=128, A=z(B * (Kd + 1), 128, dtype=bf16),
                    sA=(Kd + 1) * 128, sC=128 * N)),
    ("gemm C", dict(C=z(B * M, N - 8, dtype=bf16))),
    ("gemm C", dict(C=z(B * M, N, dtype=bf16), ldc=N + 8)),
    ("gemm C", dict(sC=M * N + 8)),
    ("gemm C", dict(batch=B + 1, A=z((B + 1) * M, Kd, dtype=bf16), Bm=z((B + 1) * N, Kd, dtype=bf16))),
    ("gemm C", dict(C=z(B * M, N // 4))),                                          # an f32 C of a quarter of the width
    ("bad shape", dict(M=0)), ("bad shape", dict(batch=0)),
    ("negative", dict(sA=-M * Kd)), ("negative", dict(ldc=-N)),
    ("gemm bias", dict(epi=dict(bias=z(N), bias_bstride=N))),                      # one bias, two items' worth of stride
    ("gemm bias", dict(epi=dict(bias=z(B * N), bias_bstride=N + 4))),
    ("gemm bias", dict(epi=dict(bias=z(N - 1)), batch=1)),
    ("gemm residual", res(residual=z(B * M - 1, N, dtype=bf16))),
    ("gemm residual", res(ldr=N + 8)),
    ("gemm residual", res(res_bstride=M * N + 8)),
    ("gemm residual", ln(residual=z(B * M, N, dtype=bf16))),                       # bf16 rows read as f32
    ("gemm aux", dict(kind=K.EPI_BIAS_GELU, epi=dict(aux=z(B * M, N, dtype=bf16), ldx=N + 8, aux_bstride=M * N))),
    ("gemm aux", dict(kind=K.EPI_DGELU, epi=dict(aux=z(M, N, dtype=bf16), aux_bstride=M * N))),
    ("gemm colsum", dict(kind=K.EPI_DGELU, epi=dict(aux=z(B * M, N, dtype=bf16), aux_bstride=M * N, colsum=z(N),
                                                    colsum_bstride=N))),
    ("gemm colsum", dict(epi=dict(colsum=z(N - 1)), batch=1)),
    ("table", dict(kind=K.EPI_STORE_STATS, batch=1, epi=dict(colsum=z(2 * N * 2)))),   # 3 blocks of 64 rows, 2 given
    ("table", bnb(colsum=z(3 * N))),                                               # a float table, not float2
    ("res_ln mean", ln(res_ln=(z(B * M - 1), z(B * M), z(B * N), z(B * N)))),
    ("res_ln rstd", ln(res_ln=(z(B * M), z(M), z(B * N), z(B * N)))),
    ("res_ln w", ln(res_ln=(z(B * M), z(B * M), z(N), z(B * N)))),
    ("res_ln b", ln(res_ln=(z(B * M), z(B * M), z(B * N + 4), z(B * N)), res_ln_bstride=N + 4)),
    ("bn x", dict(bnb(), M=M + 1, A=z(M + 1, Kd, dtype=bf16), C=z(M + 1, N, dtype=bf16))),
]


@pytest.mark.parametrize("i", range(len(ACCEPTED)))
def test_gemm_accepts(i):
    with pytest.raises(NativeError, match=BASELINE):
        call(args(**ACCEPTED[i]))


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_gemm_refuses(i):
    msg, over = REFUSED[i]
    with pytest.raises(NativeError, match=msg) as ei:
        call(args(**over))
    assert BASELINE not in str(ei.value)


def test_epilogue_keeps_its_tensors():
    """a ctypes structure holds no references: the epilogue carries the tensors behind its pointers
    for the extent checks"""
    bias = z(N)
    e = K.epilogue(K.EPI_STORE, bias=bias)
    assert e.tensors["bias"] is bias and e.tensors["aux"] is None
