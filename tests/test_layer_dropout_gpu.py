"""One fused BERT layer (src/encoder.py layer_forward / layer_backward) with attention and hidden
dropout ON, against a float64 layer that drops exactly the elements the kernels dropped.

Every model-level gradient test runs with both dropouts 0 (the reference's masks cannot be
reproduced); the benchmarked configuration trains with 0.1.  Here the float64 layer takes the
kernels' own bits: the attention keep from the keep words the forward stored
(kernels.dropmask_dense), the two hidden keeps from the BIAS_DROP_RES epilogue itself (the probe
GEMM of tests/guarded.py with seeds[1] and seeds[2]).  The forward's masks are thereby
fixed; the backward regenerates them in other kernels (ln_bwd_kernel from the seed, the attention
backward from the keep words), and a backward that masked other elements shows as a dX error of
>= 0.3 in the relative Frobenius norm at p = 0.1.

Bars on Y and dX, relative Frobenius error against float64: kernel <= 2 x a float32 torch layer that
rounds to bf16 where the fused layer stores bf16 (qkv, P, O, the LN outputs fed to GEMMs, gelu(.),
Y; the bf16 gradient stream at the same points), and <= 3e-2 outright.

Measured on an MI355X:
  (B, L) = (2, 37):   Y kernel 2.37e-3, float32 layer 2.37e-3 (1.00 x);  dX 3.94e-3 against 3.54e-3 (1.11 x)
  (B, L) = (3, 130):  Y kernel 2.33e-3, float32 layer 2.33e-3 (1.00 x);  dX 3.88e-3 against 3.44e-3 (1.13 x)
  the float32 layer's own dX with hidden masks of two other seeds: 0.32
With the mask index of ln_bwd_kernel shifted by one quad in a scratch build (not committed) the
kernel's dX error is 0.32 / 0.31 and both cases fail.
"""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from guarded import probe_keep

pytestmark = pytest.mark.gpu

HID, FFN, HEADS = 768, 3072, 12
P_ATTN = P_HID = 0.1
SEEDS = (11, 12, 13)
EPS = 1e-12
bf16 = torch.bfloat16


class _RoundBoth(torch.autograd.Function):
    """a tensor the fused layer stores in bf16: value and gradient both rounded"""

    @staticmethod
    def forward(ctx, x):
        return x.to(bf16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(bf16).to(g.dtype)


class _RoundGrad(torch.autograd.Function):
    """an f32 tensor whose gradient the fused layer stores in bf16"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(bf16).to(g.dtype)


def make_weights(dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s, sc=0.03: (torch.randn(*s, generator=g) * sc).to(dev)  # noqa: E731
    w = SimpleNamespace()
    for name, shape in (("wqkv", (3 * HID, HID)), ("wo", (HID, HID)), ("w1", (FFN, HID)), ("w2", (HID, FFN))):
        w16 = r(*shape).to(bf16)
        setattr(w, name + "16", w16)
        setattr(w, name + "t16", w16.t().contiguous())
    for name, n in (("bqkv", 3 * HID), ("bo", HID), ("b1", FFN), ("b2", HID), ("ln1b", HID), ("ln2b", HID)):
        setattr(w, name, r(n, sc=0.1))
    w.ln1w, w.ln2w = 1 + r(HID, sc=0.1), 1 + r(HID, sc=0.1)
    return w


def torch_layer(w, X, R, keymask, B, L, keepA, keep1, keep2, dt):
    """the layer in dtype dt on (X, R) -> Y.  float32: rounding to bf16 where the fused layer does"""
    rb = _RoundBoth.apply if dt == torch.float32 else (lambda t: t)
    rg = _RoundGrad.apply if dt == torch.float32 else (lambda t: t)
    c = lambda t: t.to(dt)  # noqa: E731
    za, zh = 1.0 / (1.0 - P_ATTN), 1.0 / (1.0 - P_HID)
    qkv = rb(X @ c(w.wqkv16).t() + c(w.bqkv))
    q, k, v = (t.reshape(B, L, HEADS, 64).transpose(1, 2) for t in qkv.split(HID, dim=1))
    S = q @ k.transpose(-1, -2) / 8.0 + c(keymask).view(B, 1, 1, L)
    Pm = rb(torch.softmax(S, -1) * c(keepA))
    O = rb(((Pm @ v) * za).transpose(1, 2).reshape(B * L, HID))
    S1 = rg(R + rg(O @ c(w.wo16).t() + c(w.bo)) * c(keep1) * zh)
    A32 = F.layer_norm(S1, (HID,), c(w.ln1w), c(w.ln1b), EPS)
    Hh = rb(F.gelu(rg(rb(A32) @ c(w.w116).t() + c(w.b1))))
    S2 = rg(A32 + rg(Hh @ c(w.w216).t() + c(w.b2)) * c(keep2) * zh)
    return rb(F.layer_norm(S2, (HID,), c(w.ln2w), c(w.ln2b), EPS))


def layer_and_grad(w, X, R, keymask, dY, B, L, keeps, dt):
    """-> Y, d<Y, dY> / d(hidden input): X and R are the same hidden state in two formats, the
    fused backward returns the sum of both paths' gradients"""
    z = torch.zeros(B * L, HID, dtype=dt, device=X.device, requires_grad=True)
    Y = torch_layer(w, X.to(dt) + z, R.to(dt) + z, keymask, B, L, *keeps, dt)
    (g,) = torch.autograd.grad(Y, z, dY.to(dt))
    return Y.detach(), g


def rel(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("B,L", [(2, 37), (3, 130)])
def test_fused_layer_with_dropout_matches_float64(dev, B, L):
    from src import encoder, kernels as K
    M = B * L
    w = make_weights(dev, seed=L)
    g = torch.Generator(device="cpu").manual_seed(B * L)
    R = torch.randn(M, HID, generator=g).to(dev)
    X = R.to(bf16)
    dY = torch.randn(M, HID, generator=g).to(dev).to(bf16)
    keymask = torch.zeros(B, L, device=dev)
    keymask[B - 1, L - L // 4:] = -10000.0
    Y, _, _, _, saved, _ = encoder.layer_forward(w, X, R, keymask, B, L, P_ATTN, P_HID, SEEDS, True)
    dX, _ = encoder.layer_backward(w, saved, dY, keymask, B, L, P_ATTN, P_HID, SEEDS, False)
    torch.cuda.synchronize()
    assert torch.isfinite(Y.float()).all() and torch.isfinite(dX.float()).all()
    keepA = K.dropmask_dense(saved[4], L).view(B, HEADS, L, L)
    keeps = (keepA, probe_keep(K, dev, M, HID, P_HID, SEEDS[1]), probe_keep(K, dev, M, HID, P_HID, SEEDS[2]))
    for kp in keeps:
        assert abs(1.0 - kp.float().mean().item() - 0.1) < 0.01
    Y64, g64 = layer_and_grad(w, X, R, keymask, dY, B, L, keeps, torch.float64)
    Y32, g32 = layer_and_grad(w, X, R, keymask, dY, B, L, keeps, torch.float32)
    eY, mY, eG, mG = rel(Y, Y64), rel(Y32, Y64), rel(dX, g64), rel(g32, g64)
    # a backward with another hidden mask, for scale (the float32 layer, masks of other seeds)
    other = (keepA, probe_keep(K, dev, M, HID, P_HID, SEEDS[1] + 100), probe_keep(K, dev, M, HID, P_HID, SEEDS[2] + 100))
    _, gw = layer_and_grad(w, X, R, keymask, dY, B, L, other, torch.float32)
    print(f"SUMMARY layer B={B} L={L}: Y kernel {eY:.3e} model {mY:.3e} ratio {eY / mY:.2f}; dX kernel {eG:.3e} model "
          f"{mG:.3e} ratio {eG / mG:.2f}; dX with other hidden masks {rel(gw, g64):.3f}")
    assert eY <= 2.0 * mY and eY <= 3e-2, f"Y: kernel {eY:.3e}, float32 layer {mY:.3e}"
    assert eG <= 2.0 * mG and eG <= 3e-2, f"dX: kernel {eG:.3e}, float32 layer {mG:.3e}"
