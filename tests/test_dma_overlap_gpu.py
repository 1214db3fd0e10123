"""The 256x256 LDS-DMA GEMM body with its transposed LDS reads issued in asm (csrc/gemm.hip
big_kstep, mmu_common.h lds_tr16 / lds_wait / lds_landed): the compiler no longer orders those
reads against the DMA or counts them, so the hand-placed waits carry the whole ordering.

A missing or short wait gives wrong numbers, never a fault: a read that runs ahead of its DMA sees
the tile of two K-steps earlier, a fragment used before its read returns is a stale register.  So
the operands differ in every K-step and the expectations are exact: integers in [-3, 3] stored as
bf16, f32 accumulation.  Every partial sum is an integer below 9 K <= 180000 < 2^24, so any
summation order (split-K slices included) gives the fp64 product exactly.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def K():
    from src import kernels
    return kernels


def ints(*shape, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).to(torch.bfloat16).to(dev)


def operand(rows, Kd, kmajor, dev, seed, batch=None):
    """stored tensor and its logical fp64 [rows, K] form"""
    shape = (rows, Kd) if kmajor else (Kd, rows)
    t = ints(*((batch,) + shape if batch else shape), dev=dev, seed=seed)
    return t, (t.double() if kmajor else t.double().transpose(-1, -2))


# 1, 2, 4 and 17 K-steps; 200 and 1032 end on a K tail.  The API takes a K tail only when both
# operands are M/N-major (zero-filled k-rows); with a K-major operand it refuses K % 64 != 0, so the
# mixed layouts check that refusal and run the same step counts as 256 and 1088 as well.
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("Kd", [64, 128, 200, 256, 1032, 1088])
@pytest.mark.parametrize("M,N", [(256, 256), (512, 256)])
@pytest.mark.parametrize("ak,bk", [(False, False), (True, False), (False, True)])
def test_gemm_big_exact(dev, ak, bk, M, N, Kd, accumulate):
    k = K()
    A, a64 = operand(M, Kd, ak, dev, seed=Kd + M)
    B, b64 = operand(N, Kd, bk, dev, seed=Kd + M + 1)
    C = torch.full((M, N), 5.0 if accumulate else float("nan"), dtype=torch.float32, device=dev)

    def run():
        k.gemm(A, A.shape[1], ak, B, B.shape[1], bk, C, N, M, N, Kd,
               epi=k.epilogue(k.EPI_STORE, accumulate=accumulate))

    if (ak or bk) and Kd % 64:
        from src._native import NativeError
        with pytest.raises(NativeError, match="multiple of 64"):
            run()
        return
    run()
    ref = a64 @ b64.t() + (5.0 if accumulate else 0.0)
    assert torch.equal(C.double(), ref), f"{(C.double() - ref).abs().max().item()} off at most"


def test_gemm_big_exact_splitk(dev):
    k = K()
    Ktok, M, N = 20000, 256, 256
    A, a64 = operand(M, Ktok, False, dev, seed=11)
    B, b64 = operand(N, Ktok, False, dev, seed=12)
    C = torch.full((M, N), -7.0, dtype=torch.float32, device=dev)
    k.gemm(A, M, False, B, N, False, C, N, M, N, Ktok, epi=k.epilogue(k.EPI_STORE, accumulate=True))
    assert torch.equal(C.double(), a64 @ b64.t() - 7.0)


def test_gemm_big_exact_batched(dev):
    k = K()
    Bt, M, N, Kd = 2, 256, 256, 200
    A, a64 = operand(M, Kd, False, dev, seed=21, batch=Bt)
    B, b64 = operand(N, Kd, False, dev, seed=22, batch=Bt)
    C = torch.full((Bt, M, N), float("nan"), dtype=torch.float32, device=dev)
    k.gemm(A, M, False, B, N, False, C, N, M, N, Kd, batch=Bt, sA=M * Kd, sB=N * Kd, sC=M * N)
    assert torch.equal(C.double(), a64 @ b64.transpose(1, 2))


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_filter_gradient_exact(dev, stride):
    """gemm_convw_kernel (the gathered B operand) through the 3x3 implicit filter gradient:
    Cin = Cout = 256, batch 2, a 5 x 7 map: 70 pixels (stride 1: two K-steps, the second a tail) or
    24 (stride 2: one partial K-step)"""
    k = K()
    cl = torch.channels_last
    n, c, h, w = 2, 256, 5, 7
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = ints(n, c, h, w, dev=dev, seed=31).contiguous(memory_format=cl)
    dy = ints(n, c, ho, wo, dev=dev, seed=32).contiguous(memory_format=cl)
    ref = torch.nn.grad.conv2d_weight(x.double().cpu(), (c, c, 3, 3), dy.double().cpu(), stride=stride, padding=1)
    dw = torch.full((c, c, 3, 3), 2.0, device=dev).contiguous(memory_format=cl)
    dw2 = torch.full((c, c, 3, 3), float("nan"), device=dev).contiguous(memory_format=cl)
    if stride == 1:
        k.conv3x3_wgrad(dy, x, dw, accumulate=True)
        k.conv3x3_wgrad(dy, x, dw2)
    else:
        k.conv_wgrad(dy, x, dw, 3, stride, accumulate=True)
        k.conv_wgrad(dy, x, dw2, 3, stride)
    assert torch.equal(dw.double().cpu(), ref + 2.0)
    assert torch.equal(dw2.double().cpu(), ref)


def test_gemm_big_add_res_mixed_layout(dev):
    """EPI_ADD_RES on a (K-major A, N-major B) product, bf16 out, against fp32 torch at the
    tolerance of test_kernels_gpu.test_gemm_big_tiles_epilogues (1e-2 of the output scale)"""
    k = K()
    M, N, Kd = 512, 256, 192
    g = torch.Generator(device="cpu").manual_seed(41)
    A = torch.randn(M, Kd, generator=g).to(dev).to(torch.bfloat16)
    W = (torch.randn(Kd, N, generator=g) * 0.1).to(dev).to(torch.bfloat16)
    R = torch.randn(M, N, generator=g).to(dev).to(torch.bfloat16)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    k.gemm(A, Kd, True, W, N, False, out, N, M, N, Kd, epi=k.epilogue(k.EPI_ADD_RES, residual=R))
    ref = R.float() + A.float() @ W.float()
    err, scale = (out.float() - ref).abs().max().item(), ref.abs().max().item() + 1e-6
    assert err <= 1e-2 * scale, f"max err {err:.3e} vs scale {scale:.3e}"
