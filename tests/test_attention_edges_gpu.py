"""The BERT-style attention kernels (csrc/attention.hip: forward with and without keep words, dQ,
dK/dV) against float64 at every length where they branch, through padded and guarded buffers.

Lengths: every half-tile cut-off on both sides (forward `two` and the P V skip, dQ's second-half
skip, dK/dV's second-16-rows skip, the dead second wave of a key block), nkv = ceil(L/64) = 1..9
(the dQ ring's prologue-only nkv = 2 and the forward's odd / even full-tile counts with and
without a partial tile), nq = ceil(L/32) with nq % 4 = 0, 1, 2, 3 and nq < 3 (the dK/dV ring), the
128-row query block with 1..4 live waves, and the API's maximum 576.

Shape: B = 3, heads = 3: the per-(b, head) work does not depend on `heads`; for odd L items 1 and 2
start at key-mask / LSE offsets that are only 4-byte aligned; the grid is no multiple of 8
(xcd_remap's remainder branch).  L = 129 and 512 also run heads = 12, B = 2 and heads = 1, B = 1.

Inputs (attn_harness.make_inputs): a Gaussian family and a non-negative one (|V|, |dO|: no
cancellation in O and dV).  Item 0 is unmasked, item 1 carries a random additive N(0, 1) mask,
item 2 a -10000 mask (trailing third / leading keys / keys 60..69 / all but one key, rotating
with the case).  A fully masked item is not tested: no caller produces one.

Buffers: every tensor is a view of a larger allocation with 2 guard rows on each side and the
tightest padded leading dimensions the C API accepts (ld_qkv = 3 HD + 8, ld_o = HD + 8, ld_do =
HD + 16, ld_dqkv = 3 HD + 4); the contiguous ones (key mask, LSE, delta, keep words, dbias parts)
have guard elements before and after.  Input guards and padding hold NaN: a read through them
poisons the result.  Outputs are pre-filled with a canary: afterwards the live region is finite and
everything else is bit-identical to the canary.

Bars: attn_harness (cap 3 * 2^-9 on the scale-normalised row error; kernel <= 2 x the rounding
model's max and <= 1.5 x its median; LSE within 8 x the error of a float32 logsumexp).

Measured on an MI355X over the whole sweep (run with -s for every case's figures):
  worst kernel / model ratio, cases with L > 1:   max      median    worst kernel nerr (cap 5.86e-3)
      O  (training and inference forward)          1.00     1.001     3.96e-3
      dQ                                           1.00     1.001     2.29e-3
      dK                                           1.00     1.010     1.72e-3
      dV                                           1.00     1.006     3.64e-3
  L = 1: no bf16 rounding on any path; dQ, dK 1.5e-8 against the model's 7e-9 (or 0): f32
      summation order, covered by attn_harness.F32_NOISE
  LSE: worst |lse - lse64| 1.9e-6; 1.5e-6 where a float32 logsumexp is at 9e-7: 0.21 of the bar
  dbias column sums: at most 9.5e-4 of the column-summed scale
The first run had O at 1.6 x and dQ / dK of the non-negative family at up to 4.4 x the model for
every L > 64: the model rounded P against the true row max (top key exactly 1), the forward
rounds it against its deferred max.  The model now mirrors the deferred max; the kernel is
unchanged ("Attention edge sweep").
"""
import math

import pytest
import torch

import attn_harness as H
from guarded import Guarded, guarded_input

pytestmark = pytest.mark.gpu

KEEP_CANARY = 0x5A5A5A5A5A5A5A5A

LENGTHS = [1, 8, 9, 16, 17, 32, 33, 40, 41, 48, 49, 63, 64, 65, 96, 97, 127, 128, 129, 160, 192, 193, 255, 256, 257,
           320, 384, 448, 449, 512, 575, 576]
CASES = [(i, L, 3, 3) for i, L in enumerate(LENGTHS)]
CASES += [(len(LENGTHS) + i, L, B, heads) for i, (L, B, heads) in
          enumerate([(129, 2, 12), (129, 1, 1), (512, 2, 12), (512, 1, 1)])]


def K():
    from src import kernels
    return kernels


# ------------------------------------------------------------------------------ buffers
class Buffers:
    """the outputs of one forward + backward, canary-filled"""

    def __init__(self, dev, B, L, heads):
        HD, BH, nkv = heads * 64, B * heads, (L + 63) // 64
        nan = float("nan")
        self.O = Guarded(dev, torch.bfloat16, nan, B * L, HD, HD + 8)
        self.dqkv = Guarded(dev, torch.bfloat16, nan, B * L, 3 * HD, 3 * HD + 4)
        self.lse = Guarded(dev, torch.float32, nan, BH * L)
        self.delta = Guarded(dev, torch.float32, nan, BH * L)
        self.keep = Guarded(dev, torch.int64, KEEP_CANARY, BH * L * nkv)
        self.parts = Guarded(dev, torch.float32, nan, ((L + 127) // 128 + 2 * nkv) * B * HD)
        self.shape = (B, L, heads, HD, BH, nkv)

    def all(self):
        return {"O": self.O, "dqkv": self.dqkv, "lse": self.lse, "delta": self.delta, "keep": self.keep,
                "parts": self.parts}

    def refill(self):
        for g in self.all().values():
            g.refill()


def run_kernels(k, buf, qkv, km, dO, p, seed, train=True, backward=True):
    """forward (training: keep words stored when p > 0; else the inference kernel) and backward
    into freshly canaried buffers; every output checked for finite live data and intact guards.
    -> O, lse, dqkv (None without backward), keep words view (None unless training dropout)"""
    B, L, heads, HD, BH, nkv = buf.shape
    buf.refill()
    lse, delta = buf.lse.view.view(BH, L), buf.delta.view.view(BH, L)
    dm = buf.keep.view.view(BH, L, nkv) if (p > 0 and train) else None
    k.attention_fwd(qkv, km, buf.O.view, lse, B, L, heads=heads, drop_p=p, seed=seed, dropmask=dm)
    written = ["O", "lse"]
    if backward:
        parts = buf.parts.view.view(-1, HD)
        k.attention_bwd(qkv, km, buf.O.view, dO, lse, delta, buf.dqkv.view, B, L, heads=heads, drop_p=p, seed=seed,
                        dropmask=dm, dbias_parts=parts)
        written += ["delta", "dqkv", "parts"]
    torch.cuda.synchronize()
    for name, g in buf.all().items():
        assert g.guards_intact(), f"{name}: a guard row / padding column / guard element was written"
        if name in written:
            assert torch.isfinite(g.view.float()).all(), f"{name}: live region not finite (unwritten or poisoned)"
        elif name != "keep":
            assert torch.isnan(g.view.float()).all(), f"{name}: written by a call that does not own it"
    if dm is not None:
        assert (buf.keep.view != KEEP_CANARY).all(), "keep words: a live word was not written"
    else:
        assert (buf.keep.view == KEEP_CANARY).all(), "keep words written without training dropout"
    return buf.O.view, lse, (buf.dqkv.view if backward else None), dm


def fmt(tag, stats):
    r = H.ratios(stats)
    return f"[{tag}] (max/median) " + " ".join(
        f"{n}: kernel {s['max_k']:.2e}/{s['med_k']:.2e} model {s['max_m']:.2e}/{s['med_m']:.2e} "
        f"ratio {r[n][0]:.2f}/{r[n][1]:.2f};" for n, s in stats.items())


@pytest.mark.parametrize("idx,L,B,heads", CASES, ids=[f"L{L}-B{B}-h{h}" for _, L, B, h in CASES])
def test_attention_edges(dev, idx, L, B, heads):
    k = K()
    HD, BH = heads * 64, B * heads
    seed = 0xA77E0000 + 977 * L + heads
    buf = Buffers(dev, B, L, heads)
    fails = []
    for nonneg in (False, True):
        qkv_c, km_c, dO_c = H.make_inputs(B, L, heads, seed=10 * L + heads, nonneg=nonneg, mask_kind=idx)
        qkv = guarded_input(dev, qkv_c, 3 * HD + 8)
        dO = guarded_input(dev, dO_c, HD + 16)
        km = guarded_input(dev, km_c)
        lse_f32 = H.lse32(qkv, km, B, L, heads)
        masked = km_c[2] == H.M10K if B > 2 else None
        for p in (0.0, 0.1):
            tag = f"L={L} B={B} h={heads} {'nonneg' if nonneg else 'gauss'} p={p}"
            O, lse, dqkv, dm = run_kernels(k, buf, qkv, km, dO, p, seed)
            O, lse, dqkv = O.clone(), lse.clone(), dqkv.clone()
            if p > 0:
                keep = k.dropmask_dense(dm, L).view(B, heads, L, L)
                n = keep.numel()
                if n >= 10 ** 4:
                    rate, tol = 1.0 - keep.mean().item(), 4.0 * math.sqrt(p * (1 - p) / n)
                    print(f"[{tag}] drop rate {rate:.5f} (p +- {tol:.5f})")
                    if abs(rate - p) > tol:
                        fails.append(f"{tag}: drop rate {rate:.5f} not within {tol:.5f} of {p}")
                dm = dm.clone()
            else:
                keep = torch.ones(B, heads, L, L, device=dev)
            O64, lse64, g64 = H.ref64(qkv, km, dO, B, L, heads, keep, p)
            Om, lsem, gm = H.model32(qkv, km, dO, B, L, heads, keep, p)
            sc = H.scales(qkv, km, dO, B, L, heads, keep, p)

            # training forward + backward against the bars
            st = H.evaluate((O, dqkv), (Om, gm), (O64, g64), sc, B, L, heads)
            print(fmt(tag, st))
            e, base, worst = H.lse_stats(lse, lse64, lse_f32)
            print(f"[{tag}] LSE err {e:.2e}, f32 logsumexp err {base:.2e}, {worst:.2f} x the bar")
            fails += [f"{tag}: {m}" for m in H.violations(st) + H.lse_violations(lse, lse64, lse_f32)]

            # dbias parts: column sums of the gradient (f32 accumulators, before the bf16 store)
            gb = torch.full((3 * HD,), 0.5, device=dev)
            k.attention_dbias_reduce(buf.parts.view.view(-1, HD), B, L, gb, heads=heads)
            colsc = torch.cat([H.rows_view(sc[n], B, L, heads).sum(0) for n in ("dQ", "dK", "dV")])
            berr = (gb.double() - 0.5 - g64.sum(0)).abs() / colsc.clamp_min(1e-300)
            berr = torch.where((colsc > 0) | (gb != 0.5), berr, torch.zeros_like(berr)).max().item()
            print(f"[{tag}] dbias err / column-summed scale {berr:.2e}")
            if not berr <= H.CAP:
                fails.append(f"{tag}: dbias column sums off by {berr:.3e} of the scale > {H.CAP:.3e}")

            # the -10000 keys of item 2: P underflows to exactly 0 -> their dK / dV rows are zero
            if masked is not None and masked.any():
                rows = (2 * L + torch.nonzero(masked).view(-1)).to(dev)
                if not (dqkv[rows, HD:] == 0).all():
                    fails.append(f"{tag}: dK / dV rows of -10000 keys are not exactly zero")

            # the inference forward (no keep words) applies the same mask
            if p > 0:
                Oi, lsei, _, _ = run_kernels(k, buf, qkv, km, dO, p, seed, train=False, backward=False)
                sti = H.evaluate((Oi, None), (Om, None), (O64, None), sc, B, L, heads, outputs=("O",))
                print(fmt(tag + " inference", sti))
                fails += [f"{tag} inference: {m}" for m in H.violations(sti) + H.lse_violations(lsei, lse64, lse_f32)]

            # a second identical call: bitwise-equal O, LSE, dQKV (and keep words)
            O2, lse2, dqkv2, dm2 = run_kernels(k, buf, qkv, km, dO, p, seed)
            same = torch.equal(O2.view(torch.int16), O.view(torch.int16)) and torch.equal(lse2, lse) and \
                torch.equal(dqkv2.view(torch.int16), dqkv.view(torch.int16)) and (dm is None or torch.equal(dm2, dm))
            if not same:
                fails.append(f"{tag}: two identical calls differ")

            # other finite K / V rows under the -10000 keys of item 2: nothing else may change
            if masked is not None and masked.any():
                g = torch.Generator(device="cpu").manual_seed(L)
                q2 = qkv_c.clone()
                rows_c = 2 * L + torch.nonzero(masked).view(-1)
                q2[rows_c, HD:] = (torch.randn(rows_c.numel(), 2 * HD, generator=g) * 3.0).to(torch.bfloat16)
                O3, lse3, dqkv3, _ = run_kernels(k, buf, guarded_input(dev, q2, 3 * HD + 8), km, dO, p, seed)
                sl = slice(2 * L, 3 * L)
                same = torch.equal(O3[sl].view(torch.int16), O[sl].view(torch.int16)) and \
                    torch.equal(lse3[2 * heads:], lse[2 * heads:]) and \
                    torch.equal(dqkv3[sl, :HD].contiguous().view(torch.int16), dqkv[sl, :HD].contiguous().view(torch.int16))
                if not same:
                    fails.append(f"{tag}: O / LSE / dQ of item 2 depend on the K / V rows of its -10000 keys")
    assert not fails, "\n".join(fails)


def test_attention_refused_arguments(dev):
    """calls the C API rejects before any launch (capi.hip attn_common and the ld checks)"""
    k = K()
    B, heads, HD = 1, 3, 192

    def bufs(L, ld_qkv=3 * HD + 8, ld_o=HD + 8, ld_dqkv=3 * HD + 4, ld_do=HD + 16):
        z = lambda r, c, dt=torch.bfloat16: torch.zeros(r, c, dtype=dt, device=dev)
        return dict(qkv=z(B * L, ld_qkv)[:, :min(ld_qkv, 3 * HD)], km=z(B, L, torch.float32),
                    O=z(B * L, ld_o)[:, :min(ld_o, HD)], dO=z(B * L, ld_do)[:, :min(ld_do, HD)],
                    lse=z(B * heads, L, torch.float32), delta=z(B * heads, L, torch.float32),
                    dqkv=z(B * L, ld_dqkv)[:, :min(ld_dqkv, 3 * HD)], dm=k.dropmask_empty(B, L, heads, dev))

    def fwd(t, L, p=0.0, dm=None):
        k.attention_fwd(t["qkv"], t["km"], t["O"], t["lse"], B, L, heads=heads, drop_p=p, seed=1, dropmask=dm)

    def bwd(t, L, p=0.0, dm=None):
        k.attention_bwd(t["qkv"], t["km"], t["O"], t["dO"], t["lse"], t["delta"], t["dqkv"], B, L, heads=heads,
                        drop_p=p, seed=1, dropmask=dm)

    from src._native import NativeError
    t = bufs(8)
    fwd(t, 8)  # the accepted baseline of every refused call below
    bwd(t, 8)
    torch.cuda.synchronize()
    t = bufs(577)
    with pytest.raises(NativeError, match="576"):
        fwd(t, 577)
    with pytest.raises(NativeError, match="576"):
        bwd(t, 577)
    t = bufs(8, ld_qkv=3 * HD + 4)
    with pytest.raises(NativeError, match="ld_qkv"):
        fwd(t, 8)
    with pytest.raises(NativeError, match="ld_qkv"):
        bwd(t, 8)
    with pytest.raises(NativeError, match="ld_o"):
        fwd(bufs(8, ld_o=HD - 8), 8)
    with pytest.raises(NativeError, match="bad ld"):
        bwd(bufs(8, ld_dqkv=3 * HD - 4), 8)
    with pytest.raises(NativeError, match="bad ld"):  # (the backward took these two before this sweep)
        bwd(bufs(8, ld_o=HD - 8), 8)
    with pytest.raises(NativeError, match="bad ld"):
        bwd(bufs(8, ld_do=HD - 8), 8)
    t = bufs(8)
    with pytest.raises(NativeError, match="drop_p"):
        fwd(t, 8, p=1.0, dm=t["dm"])
    with pytest.raises(NativeError, match="drop_p"):
        bwd(t, 8, p=1.0, dm=t["dm"])
    with pytest.raises(NativeError, match="dropmask"):
        bwd(t, 8, p=0.1)
    torch.cuda.synchronize()
