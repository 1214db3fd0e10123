"""The LDS-DMA attention kernels (csrc/attention.hip: forward, dQ, dK/dV).  The backward kernels
issue their transposed LDS reads (and dQ its keep words) in asm: the compiler no longer drains the
DMA ring in front of them, so each ring runs at its real depth and the hand-placed counted waits
carry the ordering.  A short wait reads the tile that sat in the stage before (wrong numbers, no
fault), so the lengths make every ring wrap at least once and end on a partial tile (the forward,
which keeps the compiler-issued reads, runs in every case as the backward's input):

  L = 33, 65   one / two 32-row query tiles and 64-key tiles plus a one-row tail
  L = 161      the dK/dV ring (4 stages of 32-row query tiles) wraps: 6 query tiles
  L = 200      the dQ ring (3 stages of 64-key tiles) wraps: 4 key tiles; the forward's 2 stages twice
  L = 513      the workload's own length (B = 1)

Reference, rounding model, metric and bars are those of attn_harness as test_attention_edges_gpu
uses them (cap 3 * 2^-9; kernel <= 2 x the model's max and 1.5 x its median; LSE bar): none is
new.  With dropout the keep matrix is the one the kernel drew (its keep words, dropmask_dense):
the reference cannot choose it; without dropout it is attn_harness.random_keep's all-ones.
"""
import pytest
import torch

import attn_harness as H

pytestmark = pytest.mark.gpu

HEADS = 2
CASES = [(33, 2), (65, 2), (161, 2), (200, 2), (513, 1)]


def K():
    from src import kernels
    return kernels


def run(k, dev, qkv, km, dO, B, L, p, seed, train=True, backward=True):
    HD, BH = HEADS * 64, B * HEADS
    O = torch.full((B * L, HD), float("nan"), dtype=torch.bfloat16, device=dev)
    lse = torch.full((BH, L), float("nan"), device=dev)
    dm = k.dropmask_empty(B, L, HEADS, dev) if (p > 0 and train) else None
    k.attention_fwd(qkv, km, O, lse, B, L, heads=HEADS, drop_p=p, seed=seed, dropmask=dm)
    dqkv = None
    if backward:
        delta = torch.full((BH, L), float("nan"), device=dev)
        dqkv = torch.full((B * L, 3 * HD), float("nan"), dtype=torch.bfloat16, device=dev)
        k.attention_bwd(qkv, km, O, dO, lse, delta, dqkv, B, L, heads=HEADS, drop_p=p, seed=seed, dropmask=dm)
    torch.cuda.synchronize()
    return O, lse, dqkv, dm


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L,B", CASES, ids=[f"L{L}-B{B}" for L, B in CASES])
def test_attention_rings_wrap(dev, L, B, p):
    k = K()
    seed = 0xD3A0000 + L
    qkv_c, km_c, dO_c = H.make_inputs(B, L, HEADS, seed=7 * L + 1)
    qkv, km, dO = qkv_c.to(dev), km_c.to(dev), dO_c.to(dev)
    O, lse, dqkv, dm = run(k, dev, qkv, km, dO, B, L, p, seed)
    if p > 0:
        keep = k.dropmask_dense(dm, L).view(B, HEADS, L, L)
    else:
        keep = H.random_keep(B, L, HEADS, 0.0, seed).to(dev)
    O64, lse64, g64 = H.ref64(qkv, km, dO, B, L, HEADS, keep, p)
    Om, _, gm = H.model32(qkv, km, dO, B, L, HEADS, keep, p)
    sc = H.scales(qkv, km, dO, B, L, HEADS, keep, p)
    st = H.evaluate((O, dqkv), (Om, gm), (O64, g64), sc, B, L, HEADS)
    print({n: (f"{s['max_k']:.2e}", f"{s['max_m']:.2e}") for n, s in st.items()})
    bad = H.violations(st) + H.lse_violations(lse, lse64, H.lse32(qkv, km, B, L, HEADS))
    assert not bad, "\n".join(bad)


def test_attention_inference_dropout_forward(dev):
    """the forward without keep words (MC-dropout inference) at L = 200: same mask as the training
    forward of the same seed, same bars on O"""
    k = K()
    L, B, p, seed = 200, 2, 0.1, 0xD3A0000 + 200
    qkv_c, km_c, dO_c = H.make_inputs(B, L, HEADS, seed=7 * L + 1)
    qkv, km, dO = qkv_c.to(dev), km_c.to(dev), dO_c.to(dev)
    _, _, _, dm = run(k, dev, qkv, km, dO, B, L, p, seed, backward=False)
    keep = k.dropmask_dense(dm, L).view(B, HEADS, L, L)
    Oi, lsei, _, _ = run(k, dev, qkv, km, dO, B, L, p, seed, train=False, backward=False)
    O64, lse64, _ = H.ref64(qkv, km, dO, B, L, HEADS, keep, p)
    Om, _, _ = H.model32(qkv, km, dO, B, L, HEADS, keep, p)
    sc = H.scales(qkv, km, dO, B, L, HEADS, keep, p)
    st = H.evaluate((Oi, None), (Om, None), (O64, None), sc, B, L, HEADS, outputs=("O",))
    bad = H.violations(st) + H.lse_violations(lsei, lse64, H.lse32(qkv, km, B, L, HEADS))
    assert not bad, "\n".join(bad)
