"""The attention test harness (attn_harness.py) checked on the CPU: the bf16 rounding model stays
inside the derived cap, the float64 reference's gradient is right, and the bars flag two injected
defects of the kind the GPU sweep (test_attention_edges_gpu.py) exists to catch.  Without these
the sweep's bars could be vacuous."""
import pytest
import torch

import attn_harness as H

B, HEADS = 3, 3
LENGTHS = [9, 33, 65, 129, 192, 257, 513]


def _case(L, p, mask_kind, seed=None):
    qkv, km, dO = H.make_inputs(B, L, HEADS, seed=L if seed is None else seed, mask_kind=mask_kind)
    keep = H.random_keep(B, L, HEADS, p, seed=7 * L + 1)
    ref = H.ref64(qkv, km, dO, B, L, HEADS, keep, p)
    sc = H.scales(qkv, km, dO, B, L, HEADS, keep, p)
    return qkv, km, dO, keep, ref, sc


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("idx,L", list(enumerate(LENGTHS)))
def test_model32_within_cap(idx, L, p):
    """the rounding model alone: nerr <= 3 * 2^-9 on every row of O, dQ, dK, dV (item 1 random
    additive mask; item 2's -10000 mask trailing / leading / interior / all-but-one by case), its
    zero-scale rows exactly zero, and its LSE within the LSE bar"""
    qkv, km, dO, keep, (O64, lse64, g64), sc = _case(L, p, idx)
    Om, lsem, gm = H.model32(qkv, km, dO, B, L, HEADS, keep, p)
    parts = H.split_outputs(Om, gm, B, L, HEADS)
    refp = H.split_outputs(O64, g64, B, L, HEADS)
    for name in H.OUTPUTS:
        e, z = H.nerr(parts[name], refp[name], sc[name])
        print(f"[model32 L={L} p={p}] {name}: max {e.max().item():.2e} median {e.median().item():.2e}")
        assert e.max().item() <= H.CAP, (name, e.max().item())
        assert (z == 0).all(), name
    assert H.lse_violations(lsem, lse64, H.lse32(qkv, km, B, L, HEADS)) == []
    # comparing the model with itself holds every bar (the margins are not below 1)
    assert H.violations(H.evaluate((Om, gm), (Om, gm), (O64, g64), sc, B, L, HEADS)) == []


def test_ref64_gradient_matches_finite_differences():
    B1, L, heads, p = 1, 5, 1, 0.25
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(B1 * L, 192, generator=g, dtype=torch.float64)
    dO = torch.randn(B1 * L, 64, generator=g, dtype=torch.float64)
    km = torch.randn(B1, L, generator=g)
    keep = H.random_keep(B1, L, heads, p, seed=5)
    _, _, grad = H.ref64(x, km, dO, B1, L, heads, keep, p)
    f = lambda y: (H.forward64(y, km, B1, L, heads, keep, p)[0] * dO).sum().item()
    h = 1e-6
    fd = torch.zeros_like(x)
    for i in range(x.numel()):
        d = torch.zeros_like(x).view(-1)
        d[i] = h
        d = d.view_as(x)
        fd.view(-1)[i] = (f(x + d) - f(x - d)) / (2 * h)
    torch.testing.assert_close(grad, fd, rtol=1e-6, atol=1e-8)
    # and the LSE is the log of the softmax denominator
    _, lse, _ = H.forward64(x, km, B1, L, heads, keep, p)
    S = x[:, :64] @ x[:, 64:128].t() / 8 + km.double()
    torch.testing.assert_close(lse.view(-1), S.exp().sum(-1).log())


def test_harness_flags_shifted_mask():
    """injected defect: item 1's random additive mask read one key off (what a wrong
    keymask + b * L index does)"""
    L, p = 129, 0.0
    qkv, km, dO, keep, (O64, lse64, g64), sc = _case(L, p, 0)
    good = H.model32(qkv, km, dO, B, L, HEADS, keep, p)
    km_bad = km.clone()
    km_bad[1] = km[1].roll(1)
    bad = H.model32(qkv, km_bad, dO, B, L, HEADS, keep, p)
    assert H.violations(H.evaluate((good[0], good[2]), (good[0], good[2]), (O64, g64), sc, B, L, HEADS)) == []
    st = H.evaluate((bad[0], bad[2]), (good[0], good[2]), (O64, g64), sc, B, L, HEADS)
    msgs = H.violations(st)
    print(msgs)
    for name in H.OUTPUTS:  # every output is off by far more than its cap
        assert st[name]["max_k"] > 2 * H.CAP, (name, st[name])
        assert any(m.startswith(name + ":") for m in msgs)
    assert H.lse_violations(bad[1], lse64, H.lse32(qkv, km, B, L, HEADS)) != []


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_harness_flags_dropped_tail_rows(p):
    """injected defect: the last (L-1) % 16 + 1 query rows (L = 513: one) missing from the
    dK / dV sums -- the kind of slip a half-tile cut-off makes"""
    L = 513
    qkv, km, dO, keep, (O64, lse64, g64), sc = _case(L, p, 0)
    good = H.model32(qkv, km, dO, B, L, HEADS, keep, p)
    bad = H.model32(qkv, km, dO, B, L, HEADS, keep, p, dkdv_rows=L - ((L - 1) % 16 + 1))
    st = H.evaluate((bad[0], bad[2]), (good[0], good[2]), (O64, g64), sc, B, L, HEADS)
    msgs = H.violations(st)
    print(msgs)
    for name in ("dK", "dV"):
        assert st[name]["max_k"] > H.CAP, (name, st[name])
        assert any(m.startswith(name + ":") for m in msgs)
    assert not any(m.startswith(("O:", "dQ:")) for m in msgs)


def test_item2_mask_kinds():
    """the four -10000 patterns: each leaves a key unmasked; the leading one covers the whole
    first 64-key tile once L >= 128, the interior one straddles the tile edge"""
    for L in (8, 9, 63, 64, 65, 129, 192, 576):
        for kind in range(4):
            m = H.item2_mask(L, kind)
            assert m.any() and not m.all(), (L, kind)
    assert H.item2_mask(128, 1)[:64].all() and H.item2_mask(192, 2)[60:70].all()
    assert H.item2_mask(192, 3).sum() == 191 and not H.item2_mask(1, 3).any()
