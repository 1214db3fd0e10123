"""conv_harness on the CPU: the im2col statement of the gather against torch's own convolutions in
float64 (forward, data gradient, weight gradient; every (ksize, stride) in {1, 3} x {1, 2, 3, 4}; maps
with H or W = 1, odd and even; the 7x7 / stride-2 / pad-3 stem in its own K layout), the max-pool
scan against max_pool2d(return_indices=True) with ties, all-equal windows, -inf and NaN, the row pool
against adaptive_avg_pool2d, and the case lists of the GPU sweeps against the launch plans: every
path named by the sweep has a case, and every "int" case keeps its partial sums exact in f32.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_harness as H
import gemm_harness as G

f64 = torch.float64
MAPS = ((2, 5, 6), (1, 1, 7), (3, 8, 1), (2, 4, 4), (1, 7, 7), (2, 1, 1), (1, 9, 4))   # (n, H, W)


def nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2)


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("stride", [1, 2, 3, 4])
def test_im2col_is_the_convolution(ks, stride):
    g = torch.Generator().manual_seed(10 * ks + stride)
    cin, cout, pad = 5, 4, ks // 2
    for (n, h, w) in MAPS:
        x = torch.randn(n, h, w, cin, generator=g, dtype=f64)
        wt = torch.randn(cout, cin, ks, ks, generator=g, dtype=f64)
        ho, wo = H.conv_out(h, w, ks, stride)
        col = H.im2col(x, ks, stride)
        assert col.shape == (n * ho * wo, ks * ks * cin)
        # forward
        y = (col @ H.filter_rows(wt).t()).view(n, ho, wo, cout)
        ref = F.conv2d(nchw(x), wt, stride=stride, padding=pad)
        assert ref.shape == (n, cout, ho, wo)
        torch.testing.assert_close(nchw(y), ref, rtol=1e-12, atol=1e-12)
        # weight gradient: contraction over the output pixels
        dy = torch.randn(n, ho, wo, cout, generator=g, dtype=f64)
        dw = dy.reshape(-1, cout).t() @ col                                  # [cout, tap * cin + ci]
        rdw = torch.nn.grad.conv2d_weight(nchw(x), wt.shape, nchw(dy), stride=stride, padding=pad)
        torch.testing.assert_close(dw, H.filter_rows(rdw), rtol=1e-12, atol=1e-12)
        # data gradient of the 3x3 / stride-1 conv: the same product on dY with the flipped filter
        if (ks, stride) == (3, 1):
            dx = (H.im2col(dy, 3, 1) @ H.dgrad_filter(wt).reshape(cin, -1).t()).view(n, h, w, cin)
            rdx = torch.nn.grad.conv2d_input((n, cin, h, w), wt, nchw(dy), stride=1, padding=1)
            torch.testing.assert_close(nchw(dx), rdx, rtol=1e-12, atol=1e-12)


def test_im2col_padding_is_zero_and_order_is_tap_major():
    x = torch.arange(1, 1 + 2 * 3 * 4 * 2, dtype=f64).view(2, 3, 4, 2)
    col = H.im2col(x, 3, 1).view(2, 3, 4, 9, 2)
    assert torch.equal(col[:, :, :, 4], x)                                   # the centre tap is the map
    assert (col[:, 0, :, :3] == 0).all() and (col[:, :, 0, 0::3] == 0).all()  # top row / left column: padding
    assert torch.equal(col[:, 1:, 1:, 0], x[:, :-1, :-1])                    # tap (0, 0) reads (h - 1, w - 1)
    assert H.padding_taps(1, 1, 3, 1).tolist() == [True] * 4 + [False] + [True] * 4
    assert H.padding_taps(1, 9, 3, 1).tolist() == [True] * 3 + [False] * 3 + [True] * 3
    assert not H.padding_taps(2, 2, 3, 1).any()


def test_stem_im2col_is_the_stem_conv():
    g = torch.Generator().manual_seed(7)
    for (n, h, w) in MAPS + ((1, 3, 5), (2, 2, 2), (1, 7, 129)):
        x = torch.randn(n, h, w, 3, generator=g, dtype=f64)
        wt = torch.randn(64, 3, 7, 7, generator=g, dtype=f64)
        ho, wo = H.stem_out(h, w)
        col = H.stem_im2col(x)
        assert col.shape == (n * ho * wo, 224)
        assert (col.view(-1, 56, 4)[:, 49:] == 0).all() and (col.view(-1, 56, 4)[:, :, 3] == 0).all()
        y = (col @ H.stem_filter_rows(wt).t()).view(n, ho, wo, 64)
        torch.testing.assert_close(nchw(y), F.conv2d(nchw(x), wt, stride=2, padding=3), rtol=1e-12, atol=1e-12)
        dy = torch.randn(n, ho, wo, 64, generator=g, dtype=f64)
        dw, _ = H.stem_wgrad_ref(dy, x)
        rdw = torch.nn.grad.conv2d_weight(nchw(x), wt.shape, nchw(dy), stride=2, padding=3)
        torch.testing.assert_close(dw, H.filter_rows(rdw), rtol=1e-12, atol=1e-12)
        c0 = torch.randn(64, 147, generator=g, dtype=f64)
        torch.testing.assert_close(H.stem_wgrad_ref(dy, x, c0)[0], dw + c0, rtol=1e-12, atol=1e-12)
        m = H.stem_wgrad_model(dy.float(), x.float())
        torch.testing.assert_close(m.double(), dw, rtol=1e-4, atol=1e-4)
    assert H.stem_tiles(1, 1, 1) == (1, 1) and H.stem_tiles(3, 5, 130) == (4, 12) and H.stem_tiles(2, 2, 2) == (1, 2)
    assert H.stem_tiles(1, 7, 129) == (4, 4) and H.stem_tiles(2, 224, 224) == (112, 224)


def window_position(idx, OH, OW, W):
    """max_pool2d's flat input index h * W + w -> the 0..8 position in the output's 3x3 window"""
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    return 3 * (idx // W - (2 * oy - 1)) + (idx % W - (2 * ox - 1))


@pytest.mark.parametrize("kind", H.POOL_KINDS)
def test_maxpool_reference_is_torchs(kind):
    for i, (h, w) in enumerate(H.POOL_HW):
        B, C = H.POOL_B[i % 2], H.POOL_C[i % 3]
        x = H.maxpool_input(kind, B, h, w, C, seed=100 * h + w)
        val, arg = H.maxpool_ref(x)
        OH, OW = H.pool_out(h, w)
        assert val.shape == (B, OH, OW, C) and arg.dtype == torch.uint8 and int(arg.max()) <= 8
        rv, ri = F.max_pool2d(nchw(x).double().contiguous(), 3, 2, 1, return_indices=True)
        assert torch.equal(torch.isnan(nchw(val)), torch.isnan(rv))
        assert torch.equal(torch.nan_to_num(nchw(val).double(), nan=7.0), torch.nan_to_num(rv, nan=7.0)), (kind, h, w)
        assert torch.equal(nchw(arg).long(), window_position(ri, OH, OW, w)), (kind, h, w)
        # the backward reference against autograd, where the forward is differentiable (no NaN)
        if kind != "nan":
            xr = nchw(x).double().contiguous().requires_grad_(True)
            dy = torch.randint(-3, 4, (B, OH, OW, C)).double()
            (rdx,) = torch.autograd.grad(F.max_pool2d(xr, 3, 2, 1), xr, nchw(dy).contiguous())
            assert torch.equal(nchw(H.maxpool_bwd_ref(dy, arg, h, w)), rdx), (kind, h, w)
    if kind == "nan":       # the LAST NaN of a window wins
        x = torch.zeros(1, 3, 3, 8, dtype=torch.bfloat16)
        x[0, 0, 1], x[0, 1, 0] = float("nan"), float("nan")
        val, arg = H.maxpool_ref(x)
        # window (0, 0) covers rows / columns -1..1: (0, 1) is position 5, (1, 0) the later position 7
        assert torch.isnan(val[0, 0, 0]).all() and (arg[0, 0, 0] == 7).all()


@pytest.mark.parametrize("hw", H.ROW_POOL_HW)
def test_row_pool_reference_is_adaptive_avg_pool(hw):
    Hh, Ww = hw
    g = torch.Generator().manual_seed(Hh * 10 + Ww)
    x = torch.randn(2, Hh, Ww, 8, generator=g).to(torch.bfloat16)
    for n in range(1, Hh + 1):
        ref, sc = H.row_pool_ref(x, n)
        want = F.adaptive_avg_pool2d(nchw(x).double(), (n, 1)).flatten(2).transpose(1, 2)
        torch.testing.assert_close(ref, want, rtol=1e-13, atol=1e-13)
        assert (sc >= ref.abs() - 1e-12).all()
        torch.testing.assert_close(H.row_pool_model(x, n).double(), ref, rtol=1e-5, atol=1e-6)
        xr = nchw(x).double().requires_grad_(True)
        d = torch.randn(2, n, 8, generator=g)
        out = F.adaptive_avg_pool2d(xr, (n, 1)).flatten(2).transpose(1, 2)
        (gr,) = torch.autograd.grad(out, xr, d.double())
        bref, bsc = H.row_pool_bwd_ref(d, Hh, Ww, n)
        torch.testing.assert_close(nchw(bref), gr, rtol=1e-13, atol=1e-13)
        assert (bsc >= bref.abs() - 1e-12).all()
        assert (H.row_pool_bwd_model(d, Hh, Ww, n).double() - bref).abs().max() <= 2.0 ** -8 * bref.abs().max() + 1e-6


# ------------------------------------------------------------------------------- plans and case lists
def test_plans_reproduce_the_slices_the_sweep_names():
    p = H.conv_plan(1, 16, 16, 64, 64, 3, 1)
    assert (p["kernel"], p["M"], p["slices"]) == ("small", 256, [320, 256])
    p = H.conv_plan(3, 7, 13, 128, 128, 3, 1)
    assert (p["kernel"], p["M"], p["slices"]) == ("small", 273, [320, 320, 320, 192])
    assert H.conv_plan(16, 32, 32, 64, 64, 3, 1)["tiles"] == 128 and H.conv_plan(16, 32, 32, 64, 64, 3, 1)["splitk"] == 1
    assert H.conv_plan(2, 12, 12, 64, 192, 1, 1)["split"] == "unsplit"
    assert [H.conv_plan(1, h, w, 64, 384, 3, 1)["M"] for h, w in ((7, 73), (27, 19))] == [511, 513]
    assert H.conv_plan(32, 32, 32, 64, 256, 3, 1)["kernel"] == "big" and H.conv_plan(32, 32, 32, 64, 256, 3, 1)["splitk"] == 1
    assert H.conv_plan(4, 16, 16, 512, 512, 1, 2)["slices"] == [256, 256]
    assert [H.wgrad_plan(1, h, w, 256, 128, 3, 1)["K"] for h, w in ((1, 1), (7, 9), (8, 8), (5, 13))] == [1, 63, 64, 65]
    for cout in (128, 512):
        p = H.wgrad_plan(2, 17, 17, 256, cout, 1, 1)
        assert (p["path"], p["slices"]) == ("few-split", [320, 258])
    p = H.wgrad_plan(700, 1, 3, 256, 128, 3, 1)
    assert (p["path"], p["slices"]) == ("many-split", [1088, 1012])
    assert H.wgrad_plan(3, 27, 27, 256, 384, 3, 1)["K"] == 2187 and H.wgrad_plan(3, 27, 27, 256, 384, 3, 1)["tiles_m"] == 2
    assert H.wgrad_plan(6, 10, 10, 512, 128, 1, 4)["path"] == "few-unsplit"


def test_every_named_path_has_a_case():
    fwd = [(c, H.conv_plan_of(c)) for c in H.cases_fwd()]
    for name, pred in H.FWD_PATHS.items():
        assert any(pred(c, p) for c, p in fwd), f"forward / data gradient: no case reaches '{name}'"
    wg = [(c, H.wgrad_plan_of(c)) for c in H.cases_wgrad()]
    for name, pred in H.WGRAD_PATHS.items():
        assert any(pred(c, p) for c, p in wg), f"weight gradient: no case reaches '{name}'"
    # every row runs plain, every 3x3 / stride-1 row as a data gradient, every wgrad row both ways
    for row in H.FWD_ROWS:
        mine = [c for c, _ in fwd if (c["n"], c["H"], c["W"], c["C"], c["N"], c["ks"], c["s"]) == row]
        assert any(c["epi"] == "store" and c["op"] == "fwd" for c in mine)
        assert (row[5:] != (3, 1)) or any(c["op"] == "dgrad" for c in mine)
    for row in H.WGRAD_ROWS:
        mine = [c for c, _ in wg if (c["n"], c["H"], c["W"], c["C"], c["N"], c["ks"], c["s"]) == row]
        assert {c["acc"] for c in mine if c["inp"] == "int"} == {False, True}
    names = [c["name"] for c, _ in fwd + wg]
    assert len(set(names)) == len(names)


def test_cases_are_what_the_library_accepts():
    for c in H.cases_fwd():
        p = H.conv_plan_of(c)
        cin, cout = (c["N"], c["C"]) if c["op"] == "dgrad" else (c["C"], c["N"])
        assert cin % 64 == 0 and cout % 64 == 0 and p["M"] >= 256, c["name"]
        assert p["splitk"] * p["M"] * cout <= H.SPLITK_WS_FLOATS
        assert c["epi"] != "bnb" or (c["ks"], c["s"]) == (3, 1)
    for c in H.cases_wgrad():
        assert c["C"] % 256 == 0 and c["N"] % 128 == 0, c["name"]


def test_int_cases_are_exact_in_f32():
    for c in H.cases_fwd() + H.cases_wgrad():
        if c["inp"] == "int":
            assert H.int_sum_bound(c) < 2 ** 24, c["name"]
            p = H.wgrad_plan_of(c) if c["op"] == "wgrad" else H.conv_plan_of(c)
            assert 6 * p["K"] < 2 ** 24
    # and so the order model reproduces the reference bit for bit, whatever the slices
    x, w = H.conv_inputs("int", (("x", (3, 7, 13, 128)), ("w", (128, 9 * 128))), seed=3)
    A, B = H.im2col(x, 3, 1)[None], w[None]
    ref, _ = G.gemm_ref(A, B)
    for kchunk in (None, 320, 256):
        assert torch.equal(G.gemm_model32(A, B, c_f32=True, kchunk=kchunk)["C"].double(), ref["C"])
