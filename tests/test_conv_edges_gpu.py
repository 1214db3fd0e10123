"""The implicit-im2col conv products (csrc/gemm.hip: gemm_conva_small_kernel, gemm_conva_kernel,
gemm_convw_kernel, splitk_reduce_tab_kernel<>, splitk_reduce_bf16_kernel, through
kernels.conv_implicit / conv3x3_implicit / conv_wgrad) against float64 at the shapes where each
path of the host's plan begins, through guarded buffers.

Cases (conv_harness.cases_fwd / cases_wgrad, chosen and labelled by conv_plan / wgrad_plan): both
forward kernels unsplit, split into even slices and with an uneven last slice; slices that cross a
tap; M = 256 exactly and M tails of 17, 255 and 1 rows; tiles that straddle images; N = 64, 192
and 384 (half column tiles); ksize 1 and 3 at strides 1..4; one-row and one-column maps (two of
three tap rows all padding); the STATS and BNB tables by the epilogue and by the reduce kernel,
with a partial last 64-row block; the 3x3 data gradient with the flipped filter.  Weight gradient:
1, 63, 64 and 65 output pixels, few-tile and many-tile products unsplit and split with uneven last
slices, Cout 128 / 256 / 384 / 512, strides 2..4, 700 images of a 1x3 map (the pixel division by a
float reciprocal), all-padding taps (exact zeros; untouched under accumulate).

Buffers (tests/guarded.py): every map is a channels-last view of a guarded allocation.  Inputs are
NaN-surrounded and unchanged afterwards; Y is followed by 256 canary rows, dW and the tables by
canary blocks, and after every launch the live regions are finite and everything else bit-identical.

Bars: "int" cases -- bf16 Y / dX equals the float64 reference rounded to bf16, f32 dW equals it
exactly (as values); "gauss" cases -- rowops_harness.check_bf16 / check_f32 against the f32 order
model; tables against float64 sums over the kernel's own stored C.  Every case runs twice into
fresh buffers and must repeat bit for bit.

Measured on an MI355X over the whole sweep: DESIGN.md, "Conv, stem and pool edge sweep".
"""
import pytest
import torch

import conv_harness as H
import gemm_harness as G
from guarded import NAN, Guarded, check_written, guarded_input, out_buf
from rowops_harness import Worst, check_bf16, check_f32

pytestmark = pytest.mark.gpu

bf16, f32t = torch.bfloat16, torch.float32
GUARD_ROWS = 256


def K():
    from src import kernels
    return kernels


def cl_view(flat, n, h, w, c):
    """a flat [n h w c] buffer -> the channels-last [n, c, h, w] map over the same memory"""
    return flat.view(n, h, w, c).permute(0, 3, 1, 2)


def map_input(dev, x_nhwc):
    """an NHWC tensor (device) -> (Guarded, channels-last NCHW view) inside a NaN-surrounded buffer"""
    n, h, w, c = x_nhwc.shape
    g = Guarded(dev, x_nhwc.dtype, NAN, x_nhwc.numel())
    g.view.copy_(x_nhwc.reshape(-1))
    g.set_canary()
    return g, cl_view(g.view, n, h, w, c)


def pack_bits(mask):
    """[M, N] bool -> [M * N / 8] u8: bit e of byte (m, n / 8) = mask[m, n + e]"""
    M, N = mask.shape
    w = (1 << torch.arange(8, device=mask.device)).to(torch.int32)
    return (mask.view(M, N // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).reshape(-1)


def same_bits(a, b):
    return all(torch.equal(x._bits(x.alloc), y._bits(y.alloc)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------- forward / data gradient
def run_fwd(k, dev, c, seed, fails, log, worst, paths):
    tag = c["name"]
    n, Hh, Ww, ks, s = c["n"], c["H"], c["W"], c["ks"], c["s"]
    dgrad = c["op"] == "dgrad"
    cin, cout = (c["N"], c["C"]) if dgrad else (c["C"], c["N"])     # what the kernel sees
    pl = H.conv_plan_of(c)
    paths.add(f"{pl['kernel']}/{pl['split']}/{c['epi']}")
    ho, wo, M = pl["Ho"], pl["Wo"], pl["M"]
    x, wt = H.conv_inputs(c["inp"], (("x", (n, Hh, Ww, cin)), ("w", (c["N"], c["C"], ks, ks))), seed, device=dev)
    # the filter as the kernel reads it: [Nout][ks][ks][C]
    wk = H.dgrad_filter(wt) if dgrad else wt.permute(0, 2, 3, 1).contiguous()
    assert tuple(wk.shape) == (cout, ks, ks, cin)
    A, B = H.im2col(x, ks, s)[None], wk.reshape(cout, -1)[None]
    kind = {"store": G.STORE, "stats": G.STORE_STATS, "bnb": G.STORE_BNB}[c["epi"]]
    e = {}
    if kind == G.STORE_BNB:
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        ints = c["inp"] == "int"
        bx = (torch.randint(-4, 5, (M, cout), generator=g, device=dev).float() if ints
              else torch.randn(M, cout, generator=g, device=dev)).to(bf16)
        mask = (torch.rand(M, cout, generator=g, device=dev) < 0.6) if c["mask"] else None
        if mask is not None:
            mask[1::5] = False                                              # whole rows gated off
        mean = (torch.randint(-2, 3, (cout,), generator=g, device=dev).float() if ints
                else torch.randn(cout, generator=g, device=dev) * 0.3)
        e["bn"] = (bx, mask, mean)
    ref, sc = G.gemm_ref(A, B)
    exact = c["inp"] == "int"
    model = None if exact else G.gemm_model32(A, B, kchunk=pl["kchunk"] if pl["splitk"] > 1 else None)
    del A
    P = (M + 63) // 64

    def launch():
        ins = {}
        ins["X"], X = map_input(dev, x)
        ins["Wk"] = Guarded(dev, bf16, NAN, wk.numel())
        ins["Wk"].view.copy_(wk.reshape(-1))
        ins["Wk"].set_canary()
        Wk = ins["Wk"].view.view(cout, ks, ks, cin)
        if not dgrad and kind != G.STORE_BNB and seed % 2:                  # the other accepted filter shape
            Wk = Wk.permute(0, 3, 1, 2)
        outs = {}
        outs["Y"], yflat = out_buf(dev, bf16, M * cout, guard=GUARD_ROWS * cout)
        Y = cl_view(yflat, n, ho, wo, cout)
        table = None
        if kind != G.STORE:
            outs["table"], table = out_buf(dev, f32t, P * cout * 2, guard=8 * cout)
        if kind == G.STORE_BNB:
            bx, mask, mean = e["bn"]
            ins["bn_x"], BX = map_input(dev, bx.view(n, ho, wo, cout))
            mk = None if mask is None else guarded_input(dev, pack_bits(mask).cpu())
            k.conv3x3_implicit(X, Wk, Y, bnb=(BX, mk, guarded_input(dev, mean.cpu())), table=table)
        elif ks == 3 and s == 1 and kind == G.STORE and seed % 3 == 0:
            k.conv3x3_implicit(X, Wk, Y)
        else:
            k.conv_implicit(X, Wk, Y, ksize=ks, stride=s, stats=table)
        torch.cuda.synchronize()
        return ins, outs

    ins, outs = launch()
    check_written(outs, fails, tag)
    for name, g in ins.items():
        if not g.unchanged():
            fails.append(f"{tag} {name}: an input was changed")
    ins2, outs2 = launch()
    if not same_bits(outs.values(), outs2.values()):
        fails.append(f"{tag}: two runs differ")
    del ins2, outs2
    C = outs["Y"].view.view(M, cout)
    if not torch.isfinite(C.float()).all():
        return
    if exact:
        want = ref["C"][0].float().to(bf16)
        bad = (C.float() != want.float()).sum().item()
        if bad:
            fails.append(f"{tag}: {bad} of {C.numel()} elements differ from the exact product rounded to bf16")
    else:
        el, st = check_bf16(f"{tag} Y", C, model["C"][0], ref["C"][0], sc["C"][0], fails, log)
        worst.bf(f"{pl['kernel']} Y", el, st)
    if "table" in outs:
        tab = outs["table"].view.view(P, cout, 2)
        if torch.isfinite(tab).all():
            tref, tsc = G.table_ref(C, kind, e)
            r = check_f32(f"{tag} table", tab.reshape(-1), G.table_model(C, kind, e).reshape(-1), tref.reshape(-1),
                          tsc.reshape(-1), fails, log)
            worst.f32(f"{pl['kernel']} {c['epi']} table" + (" (reduce kernel)" if pl["splitk"] > 1 else ""), *r)


FWD_GROUPS = {
    "small-split": lambda c, p: p["kernel"] == "small" and p["splitk"] > 1,
    "small-unsplit": lambda c, p: p["kernel"] == "small" and p["splitk"] == 1 and p["tiles"] < 128,
    "small-128-tiles": lambda c, p: p["kernel"] == "small" and p["tiles"] >= 128,
    "big-split": lambda c, p: p["kernel"] == "big" and p["splitk"] > 1,
    "big-128-tiles": lambda c, p: p["kernel"] == "big" and p["splitk"] == 1,
}


def test_fwd_groups_partition_the_cases():
    for c in H.cases_fwd():
        p = H.conv_plan_of(c)
        assert sum(bool(f(c, p)) for f in FWD_GROUPS.values()) == 1, c["name"]


@pytest.mark.parametrize("group", list(FWD_GROUPS))
def test_conv_forward_edges(dev, group):
    k = K()
    fails, log, worst, paths = [], [], Worst(), set()
    for i, c in enumerate(H.cases_fwd()):
        if FWD_GROUPS[group](c, H.conv_plan_of(c)):
            run_fwd(k, dev, c, 1000 + 7 * i, fails, log, worst, paths)
    print("\n".join(log))
    print(f"PATHS conv {group}: {sorted(paths)}")
    worst.report(f"conv {group}")
    assert paths, "no case in this group"
    assert not fails, "\n".join(fails[:40])


# ------------------------------------------------------------------------------- weight gradient
def run_wgrad(k, dev, c, seed, fails, log, worst, paths):
    tag = c["name"]
    n, Hh, Ww, cin, cout, ks, s, acc = c["n"], c["H"], c["W"], c["C"], c["N"], c["ks"], c["s"], c["acc"]
    pl = H.wgrad_plan_of(c)
    paths.add(pl["path"])
    ho, wo, T = pl["Ho"], pl["Wo"], ks * ks
    x, dy = H.conv_inputs(c["inp"], (("x", (n, Hh, Ww, cin)), ("x", (n, ho, wo, cout))), seed, device=dev)
    exact = c["inp"] == "int"
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    c0 = None
    if acc:
        c0 = (torch.randint(-4, 5, (cout, T * cin), generator=g, device=dev).float() if exact
              else torch.randn(cout, T * cin, generator=g, device=dev))
    A, B = dy.reshape(-1, cout).t()[None], H.im2col(x, ks, s).t()[None]      # [1, Cout, pixels], [1, T Cin, pixels]
    e = {"c0": c0[None]} if acc else {}
    ref, sc = G.gemm_ref(A, B, G.STORE, e)
    model = None if exact else G.gemm_model32(A, B, G.STORE, e, c_f32=True,
                                              kchunk=pl["kchunk"] if pl["splitk"] > 1 else None)

    def launch():
        ins = {}
        ins["X"], X = map_input(dev, x)
        ins["dY"], DY = map_input(dev, dy)
        gw = Guarded(dev, f32t, NAN, cout * T * cin, guard=64 * T * cin)
        if acc:
            gw.view.copy_(c0.reshape(-1))
            gw.set_canary()
        dW = cl_view(gw.view, cout, ks, ks, cin)
        if (ks, s) == (3, 1) and seed % 2:
            k.conv3x3_wgrad(DY, X, dW, accumulate=acc)
        else:
            k.conv_wgrad(DY, X, dW, ksize=ks, stride=s, accumulate=acc)
        torch.cuda.synchronize()
        return ins, {"dW": gw}

    ins, outs = launch()
    check_written(outs, fails, tag)
    for name, gi in ins.items():
        if not gi.unchanged():
            fails.append(f"{tag} {name}: an input was changed")
    _, outs2 = launch()
    if not same_bits(outs.values(), outs2.values()):
        fails.append(f"{tag}: two runs differ")
    dW = outs["dW"].view.view(cout, T * cin)
    if not torch.isfinite(dW).all():
        return
    dead = H.padding_taps(Hh, Ww, ks, s).to(dev)                            # taps that read padding alone
    if dead.any():
        got, base = dW.view(cout, T, cin)[:, dead], (c0.view(cout, T, cin)[:, dead] if acc else None)
        if (acc and not torch.equal(got, base)) or (not acc and (got != 0).any()):
            fails.append(f"{tag}: an all-padding tap is not exactly {'unchanged' if acc else 'zero'}")
    if exact:
        bad = (dW.double() != ref["C"][0]).sum().item()
        if bad:
            fails.append(f"{tag}: {bad} of {dW.numel()} elements of an exact weight gradient differ")
    else:
        r = check_f32(f"{tag} dW", dW, model["C"][0], ref["C"][0], sc["C"][0], fails, log)
        worst.f32(f"dW {pl['path']}", *r)


@pytest.mark.parametrize("half", [0, 1])
def test_conv_wgrad_edges(dev, half):
    k = K()
    fails, log, worst, paths = [], [], Worst(), set()
    cases = H.cases_wgrad()
    for i, c in enumerate(cases):
        if (i * 2) // len(cases) == half:
            run_wgrad(k, dev, c, 2000 + 11 * i, fails, log, worst, paths)
    print("\n".join(log))
    print(f"PATHS wgrad {half}: {sorted(paths)}")
    worst.report(f"conv wgrad {half}")
    assert not fails, "\n".join(fails[:40])


# ------------------------------------------------------------------------------- the C side's refusals
def test_conv_refuses_misaligned_maps(dev):
    """a map that starts 8 B into its allocation is refused by the wrapper and, behind it, by the
    library; the refused calls stay inside their buffers if wrongly accepted"""
    from src import _native as Nat
    k = K()
    n, h, w, c, nout = 1, 16, 16, 64, 64
    big = torch.zeros(4 * n * h * w * c + 64, dtype=bf16, device=dev)
    X, Xo = cl_view(big[:n * h * w * c], n, h, w, c), cl_view(big[4:4 + n * h * w * c], n, h, w, c)
    Wk = torch.zeros(nout, 3, 3, c, dtype=bf16, device=dev)
    Y = cl_view(torch.zeros(n * h * w * nout, dtype=bf16, device=dev), n, h, w, nout)
    k.conv_implicit(X, Wk, Y)
    with pytest.raises(Nat.NativeError, match="16-B aligned"):
        k.conv_implicit(Xo, Wk, Y)
    ws = k._splitk_workspace(dev)
    st = torch.cuda.current_stream().cuda_stream
    for off in ((8, 0, 0), (0, 8, 0), (0, 0, 8)):
        with pytest.raises(Nat.NativeError, match="mmu_conv_implicit: .*16-B aligned"):
            Nat.call("mmu_conv_implicit", big.data_ptr() + off[0], Wk.data_ptr() + off[1], big.data_ptr() + off[2],
                     n, h, w, c, nout, 3, 1, ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
