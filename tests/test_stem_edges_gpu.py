"""The stem conv pair (csrc/stem.hip: stem_fwd_kernel, stem_wgrad_kernel, stem_wgrad_reduce_kernel,
through kernels.stem_conv_fwd / stem_conv_wgrad) against float64 through guarded buffers.

Both kernels are persistent, a grid of min(n_tiles, 2 x CUs) blocks over tiles of 2 output rows x 64
output columns.  Cases: a single output pixel; maps smaller than a tile; Wo = 64 and 65 (a second
column tile of one column); odd Ho (half a row pair); and the persistent loop itself -- batches of
5x130 images (4 tiles each: an odd Ho and a one-column tile) sized so that some blocks run two
tiles (n_tiles >= 2 CUs x 2 + 3) and three (n_tiles > 4 x CUs: the register prefetch under the
MFMAs, the buf ^= 1 ring back at buffer 0, an LDS patch that held another tile), and 4 x CUs + 1
images of 2x2 (one tile each).  Filter gradient: 1, 15, 16 and 17 block slabs around the reduce
kernel's 16 slices, accumulate off and on.

"int" inputs (x in -3..3, w in -2..2, dY in -3..3: every partial sum exact in f32 in any order) must
give the float64 reference exactly -- Y rounded to bf16, dW as it is; "gauss" inputs go through
rowops_harness.check_bf16 / check_f32 against the f32 order model.  Every case runs twice into fresh
buffers and must repeat bit for bit; inputs are NaN-surrounded and unchanged afterwards; the dW guard
catches a write past [64][147].

Measured on an MI355X: DESIGN.md, "Conv, stem and pool edge sweep".
"""
import pytest
import torch

import conv_harness as H
import gemm_harness as G
from guarded import check_written, out_buf
from rowops_harness import Worst, check_bf16, check_f32
from test_conv_edges_gpu import cl_view, map_input, same_bits

pytestmark = pytest.mark.gpu

bf16, f32t = torch.bfloat16, torch.float32
GEOMETRY = ((1, 1, 1), (2, 2, 2), (1, 3, 5), (2, 5, 127), (2, 6, 128), (1, 7, 129), (3, 37, 53))


def K():
    from src import kernels
    return kernels


def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def persistent_shapes(dev):
    """(n, H, W) whose tile counts put 2 and 3 tiles on some blocks of the 2 x CUs grid"""
    grid = 2 * cus(dev)
    per, _ = H.stem_tiles(1, 5, 130)
    two = (grid + 3 + per - 1) // per                     # n_tiles = grid + 3, rounded up to whole images
    three = (2 * grid + 1 + per - 1) // per               # n_tiles > 4 x CUs
    shapes = ((two, 5, 130), (three, 5, 130), (2 * grid + 1, 2, 2))
    assert grid < H.stem_tiles(*shapes[0])[1] <= 2 * grid < H.stem_tiles(*shapes[1])[1] <= 3 * grid
    assert H.stem_tiles(*shapes[2])[1] == 2 * grid + 1
    return shapes


def stem_inputs(kind, n, h, w, seed, dev):
    ho, wo = H.stem_out(h, w)
    x, dy, wt = H.conv_inputs(kind, (("x", (n, h, w, 3)), ("x", (n, ho, wo, 64)), ("w", (64, 3, 7, 7))), seed, device=dev)
    return x, dy, wt


def run_fwd(k, dev, kind, n, h, w, seed, fails, log, worst):
    tag = f"stem fwd {n}x{h}x{w} {kind} ({H.stem_tiles(n, h, w)[1]} tiles)"
    ho, wo = H.stem_out(h, w)
    x, _, wt = stem_inputs(kind, n, h, w, seed, dev)
    A, B = H.stem_fwd_ref(x, wt)
    ref, sc = G.gemm_ref(A, B)

    def launch():
        gx, X = map_input(dev, x)
        gw, Wt = map_input(dev, wt.permute(0, 2, 3, 1))
        gy, yflat = out_buf(dev, bf16, n * ho * wo * 64, guard=256 * 64)
        k.stem_conv_fwd(X, Wt, cl_view(yflat, n, ho, wo, 64))
        torch.cuda.synchronize()
        return {"X": gx, "Wk": gw}, {"Y": gy}

    ins, outs = launch()
    check_written(outs, fails, tag)
    for name, g in ins.items():
        if not g.unchanged():
            fails.append(f"{tag} {name}: an input was changed")
    _, outs2 = launch()
    if not same_bits(outs.values(), outs2.values()):
        fails.append(f"{tag}: two runs differ")
    Y = outs["Y"].view.view(n * ho * wo, 64)
    if not torch.isfinite(Y.float()).all():
        return
    if kind == "int":
        bad = (Y.float() != ref["C"][0].float().to(bf16).float()).sum().item()
        if bad:
            fails.append(f"{tag}: {bad} of {Y.numel()} elements differ from the exact product rounded to bf16")
    else:
        el, st = check_bf16(f"{tag} Y", Y, G.gemm_model32(A, B)["C"][0], ref["C"][0], sc["C"][0], fails, log)
        worst.bf("stem Y", el, st)


def run_wgrad(k, dev, kind, n, h, w, acc, seed, fails, log, worst):
    tag = f"stem wgrad {n}x{h}x{w} {kind}{' acc' if acc else ''} ({H.stem_tiles(n, h, w)[1]} tiles)"
    x, dy, _ = stem_inputs(kind, n, h, w, seed, dev)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    c0 = None
    if acc:
        c0 = (torch.randint(-4, 5, (64, 147), generator=g, device=dev).float() if kind == "int"
              else torch.randn(64, 147, generator=g, device=dev))
    ref, sc = H.stem_wgrad_ref(dy, x, c0)

    def launch():
        gx, X = map_input(dev, x)
        gd, DY = map_input(dev, dy)
        gw, wflat = out_buf(dev, f32t, 64 * 147, guard=4 * 147)
        if acc:
            wflat.copy_(c0.reshape(-1))
            gw.set_canary()
        k.stem_conv_wgrad(DY, X, cl_view(wflat, 64, 7, 7, 3), accumulate=acc)
        torch.cuda.synchronize()
        return {"X": gx, "dY": gd}, {"dW": gw}

    ins, outs = launch()
    check_written(outs, fails, tag)
    for name, gi in ins.items():
        if not gi.unchanged():
            fails.append(f"{tag} {name}: an input was changed")
    _, outs2 = launch()
    if not same_bits(outs.values(), outs2.values()):
        fails.append(f"{tag}: two runs differ")
    dW = outs["dW"].view.view(64, 147)
    if not torch.isfinite(dW).all():
        return
    if kind == "int":
        bad = (dW.double() != ref).sum().item()
        if bad:
            fails.append(f"{tag}: {bad} of {dW.numel()} elements of an exact filter gradient differ")
    else:
        r = check_f32(f"{tag} dW", dW, H.stem_wgrad_model(dy, x, c0), ref, sc, fails, log)
        worst.f32("stem dW", *r)


def finish(tag, fails, log, worst):
    print("\n".join(log))
    worst.report(tag)
    assert not fails, "\n".join(fails[:40])


def test_stem_forward_geometry(dev):
    k = K()
    fails, log, worst = [], [], Worst()
    for i, (n, h, w) in enumerate(GEOMETRY):
        run_fwd(k, dev, "int", n, h, w, 300 + i, fails, log, worst)
    run_fwd(k, dev, "gauss", 3, 37, 53, 320, fails, log, worst)
    run_fwd(k, dev, "gauss", 1, 7, 129, 321, fails, log, worst)
    finish("stem fwd geometry", fails, log, worst)


def test_stem_forward_persistent_loop(dev):
    k = K()
    fails, log, worst = [], [], Worst()
    for i, (n, h, w) in enumerate(persistent_shapes(dev)):
        run_fwd(k, dev, "int", n, h, w, 400 + i, fails, log, worst)
    n, h, w = persistent_shapes(dev)[1]
    run_fwd(k, dev, "gauss", n, h, w, 410, fails, log, worst)
    finish("stem fwd persistent", fails, log, worst)


def test_stem_wgrad_geometry(dev):
    k = K()
    fails, log, worst = [], [], Worst()
    for i, (n, h, w) in enumerate(GEOMETRY):
        for acc in (False, True):
            run_wgrad(k, dev, "int", n, h, w, acc, 500 + i, fails, log, worst)
    for acc in (False, True):
        run_wgrad(k, dev, "gauss", 3, 37, 53, acc, 520, fails, log, worst)
    finish("stem wgrad geometry", fails, log, worst)


def test_stem_wgrad_slabs(dev):
    """n_tiles = nslabs = 1, 15, 16, 17 (2x2 images, one tile each) and, with the persistent-loop
    shapes, more tiles than blocks: 2 x CUs slabs, each the sum of 2 or 3 tiles"""
    k = K()
    fails, log, worst = [], [], Worst()
    shapes = [(n, 2, 2) for n in (1, 15, 16, 17)] + list(persistent_shapes(dev))
    for i, (n, h, w) in enumerate(shapes):
        for acc in (False, True):
            run_wgrad(k, dev, "int", n, h, w, acc, 600 + i, fails, log, worst)
    n, h, w = persistent_shapes(dev)[0]
    run_wgrad(k, dev, "gauss", n, h, w, True, 620, fails, log, worst)
    run_wgrad(k, dev, "gauss", 17, 2, 2, False, 621, fails, log, worst)
    finish("stem wgrad slabs", fails, log, worst)
