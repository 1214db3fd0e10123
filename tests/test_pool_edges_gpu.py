"""The max pool (csrc/pool.hip, kernels.maxpool_fwd / maxpool_bwd) and the row pool (csrc/embed.hip,
kernels.row_pool_fwd / row_pool_bwd) against conv_harness's references through guarded buffers.

Max pool: B in {1, 3}, every odd / even / size-1 pair of H and W out of {1, 2, 3, 4, 5, 7, 8}, C in
{8, 24, 64}; quarter-integer maps with many ties, an all-equal map, maps with -inf (whole windows of
it) and with NaN.  The forward's values equal the reference bit for bit, the argmax is the
reference's 0..8 window position (first maximum; the LAST NaN of a window, as torch); the backward
with integer dy is exact and writes every dx element (zeros where no window chose it).  The canaries
of these outputs are finite numbers the data cannot hold, since NaN and -inf are legitimate results.
Row pool: (Hh, Ww) in {(7, 7), (5, 3), (1, 4), (8, 1)}, every n in 1..Hh, C in {8, 24, 2048}, B in
{1, 3}: the forward within check_f32 of the f32 order model, the backward within check_bf16.

Measured on an MI355X: DESIGN.md, "Conv, stem and pool edge sweep".
"""
import pytest
import torch

import conv_harness as H
from guarded import NAN, Guarded, check_written, out_buf
from rowops_harness import Worst, check_bf16, check_f32

pytestmark = pytest.mark.gpu

bf16, f32t = torch.bfloat16, torch.float32
CANARY = 777.0        # bf16-exact, and no max-pool input or gradient sum reaches it


def K():
    from src import kernels
    return kernels


def cl(flat, b, h, w, c):
    return flat.view(b, h, w, c).permute(0, 3, 1, 2)


def guarded_map(dev, x_nhwc):
    g = Guarded(dev, x_nhwc.dtype, NAN, x_nhwc.numel())
    g.view.copy_(x_nhwc.reshape(-1))
    g.set_canary()
    return g, cl(g.view, *x_nhwc.shape)


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("kind", H.POOL_KINDS)
def test_maxpool_edges(dev, kind):
    k = K()
    fails = []
    i = 0
    for B in H.POOL_B:
        for (h, w) in H.POOL_HW:
            C = H.POOL_C[i % 3]
            i += 1
            tag = f"maxpool {kind} B{B} {h}x{w} C{C}"
            x = H.maxpool_input(kind, B, h, w, C, seed=1000 * i + h, device=dev)
            oh, ow = H.pool_out(h, w)
            val, arg = H.maxpool_ref(x)
            gx, X = guarded_map(dev, x)
            gy, yflat = out_buf(dev, bf16, B * oh * ow * C, fill=CANARY)
            ga, aflat = out_buf(dev, torch.uint8, B * oh * ow * C, fill=85, guard=16)
            k.maxpool_fwd(X, cl(yflat, B, oh, ow, C), aflat.view(B, oh, ow, C))
            torch.cuda.synchronize()
            if not (gy.guards_intact() and ga.guards_intact()):
                fails.append(f"{tag}: the forward wrote a guard element")
            if not gx.unchanged():
                fails.append(f"{tag}: x changed")
            if not torch.equal(bits(yflat), bits(val.reshape(-1))):
                fails.append(f"{tag}: values differ from the reference in "
                             f"{(bits(yflat) != bits(val.reshape(-1))).sum().item()} elements")
            if int(aflat.max()) > 8 or not torch.equal(aflat, arg.reshape(-1)):
                fails.append(f"{tag}: argmax differs from the reference in {(aflat != arg.reshape(-1)).sum().item()} "
                             f"elements (max {int(aflat.max())})")
            # backward from the REFERENCE argmax: exact integer sums, every element written
            g = torch.Generator(device=dev).manual_seed(i)
            dy = torch.randint(-3, 4, (B, oh, ow, C), generator=g, device=dev).float().to(bf16)
            gd, DY = guarded_map(dev, dy)
            gr = Guarded(dev, torch.uint8, 85, arg.numel(), guard=16)
            gr.view.copy_(arg.reshape(-1))
            gr.set_canary()
            gdx, dxflat = out_buf(dev, bf16, B * h * w * C, fill=CANARY)
            k.maxpool_bwd(DY, gr.view.view(B, oh, ow, C), cl(dxflat, B, h, w, C))
            torch.cuda.synchronize()
            if not gdx.guards_intact():
                fails.append(f"{tag}: the backward wrote a guard element")
            if not (gd.unchanged() and gr.unchanged()):
                fails.append(f"{tag}: dy / argmax changed")
            want = H.maxpool_bwd_ref(dy, arg, h, w).reshape(-1)
            if not torch.equal(dxflat.double(), want):
                fails.append(f"{tag}: dx differs from the exact gradient in {(dxflat.double() != want).sum().item()} "
                             f"elements")
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("hw", H.ROW_POOL_HW)
def test_row_pool_edges(dev, hw):
    k = K()
    Hh, Ww = hw
    fails, log, worst = [], [], Worst()
    for B in H.ROW_POOL_B:
        for C in H.ROW_POOL_C:
            g = torch.Generator(device=dev).manual_seed(B * 1000 + C + Hh)
            x = (torch.randn(B, Hh, Ww, C, generator=g, device=dev) * 2 + 0.5).to(bf16)
            gx = Guarded(dev, bf16, NAN, x.numel())
            gx.view.copy_(x.reshape(-1))
            gx.set_canary()
            for n in range(1, Hh + 1):
                tag = f"row_pool {Hh}x{Ww} B{B} C{C} n{n}"
                go, out = out_buf(dev, f32t, B, n, C)
                k.row_pool_fwd(gx.view.view(B, Hh, Ww, C), n, out)
                torch.cuda.synchronize()
                check_written({"out": go}, fails, tag)
                if not gx.unchanged():
                    fails.append(f"{tag}: fmap changed")
                ref, sc = H.row_pool_ref(x, n)
                worst.f32("row_pool out", *check_f32(f"{tag} out", out.reshape(B * n, C), H.row_pool_model(x, n).reshape(B * n, C),
                                                     ref.reshape(B * n, C), sc.reshape(B * n, C), fails, log))
                d = torch.randn(B, n, C, generator=g, device=dev)
                gd = Guarded(dev, f32t, NAN, d.numel())
                gd.view.copy_(d.reshape(-1))
                gd.set_canary()
                gf, df = out_buf(dev, bf16, B, Hh, Ww, C)
                k.row_pool_bwd(gd.view.view(B, n, C), n, df)
                torch.cuda.synchronize()
                check_written({"dfmap": gf}, fails, tag)
                if not gd.unchanged():
                    fails.append(f"{tag}: dout changed")
                bref, bsc = H.row_pool_bwd_ref(d, Hh, Ww, n)
                el, st = check_bf16(f"{tag} dfmap", df.reshape(-1, C), H.row_pool_bwd_model(d, Hh, Ww, n).reshape(-1, C),
                                    bref.reshape(-1, C), bsc.reshape(-1, C), fails, log)
                worst.bf("row_pool dfmap", el, st)
    print("\n".join(log))
    worst.report(f"row_pool {Hh}x{Ww}")
    assert not fails, "\n".join(fails[:40])


def test_pools_refuse_misaligned_tensors(dev):
    """views that start 8 B into an allocation: refused by the wrappers and by the library behind them"""
    from src import _native as Nat
    k = K()
    B, h, w, C = 1, 4, 4, 8
    big = torch.zeros(B * h * w * C + 16, dtype=bf16, device=dev)
    x, xo = cl(big[:B * h * w * C], B, h, w, C), cl(big[4:4 + B * h * w * C], B, h, w, C)
    y = cl(torch.zeros(B * 2 * 2 * C, dtype=bf16, device=dev), B, 2, 2, C)
    am = torch.zeros(B * 2 * 2 * C + 16, dtype=torch.uint8, device=dev)
    k.maxpool_fwd(x, y, am[:B * 2 * 2 * C])
    for args in ((xo, y, am[:B * 2 * 2 * C]), (x, y, am[8:8 + B * 2 * 2 * C])):
        with pytest.raises(Nat.NativeError, match="16-B aligned"):
            k.maxpool_fwd(*args)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(Nat.NativeError, match="mmu_maxpool_fwd: .*16-B aligned"):
        Nat.call("mmu_maxpool_fwd", big.data_ptr() + 8, B, h, w, C, y.data_ptr(), am.data_ptr(), st)
    out = torch.zeros(B * 2 * C + 8, device=dev)
    f = big[:B * h * w * C].view(B, h, w, C)
    k.row_pool_fwd(f, 2, out[:B * 2 * C])
    with pytest.raises(Nat.NativeError, match="16-B aligned"):
        k.row_pool_fwd(f, 2, out[2:2 + B * 2 * C])
    with pytest.raises(Nat.NativeError, match="mmu_row_pool_fwd: .*16-B aligned"):
        Nat.call("mmu_row_pool_fwd", f.data_ptr(), B, h, w, C, 2, out.data_ptr() + 8, st)
    torch.cuda.synchronize()
