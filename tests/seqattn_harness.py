"""Reference, rounding model and error metric for the FLAVA sequence-attention kernels
(csrc/flava.hip: seqattn forward, delta, dQ, dK/dV; D in {64, 128, 256}).  Pure torch; the same
functions run on the CPU and on the device.  Used by test_seqattn_reference.py (CPU) and
test_seqattn_edges_gpu.py.  The generic pieces (bf16r, nerr, violations, ratios, the LSE bar, the
cap and the margins) are attn_harness.py's.

Layouts (those of the kernels): qkv [S*N, 3E] bf16, row s*N + n, column thirds Q | K | V, head h
at column h*D (E = heads*D); the softmax of each (n, h) runs over the S samples; O and dO
[S*N, E]; LSE2 and delta [N*heads, S]; dQKV like qkv.

  ref64    the operation in float64 with autograd (LSE in natural log)
  model32  the operation in float32, rounding to bf16 exactly where the kernels round (LSE2 in
           log2 units, as the kernels store it)
  scales   the per-(row, head) magnitudes the rounding errors are proportional to

Bars, both required on O, dQ, dK and dV (attn_harness.violations with noise = f32_noise(D)):
  cap     nerr <= 3 * 2^-9 on every row: at most three bf16 roundings on a path (P or dS; delta
          through the rounded O; the stored output), each at most 2^-9 of its scale term
  margin  max nerr(kernel) <= 2 x max nerr(model32), median <= 1.5 x median, per case and output.
          A kernel error at or below D * 2^-24, the rounding of a D-term f32 sum, passes the
          margin whatever the model's: at S = 1 no bf16 rounding occurs on any path (P = 1,
          O = V, dQ = dK = 0 up to summation order) and a ratio of two such errors says nothing
LSE:   LSE2 * ln 2 against ref64's LSE with attn_harness.lse_violations; the yardstick is lse32
delta: delta_violations: against a float64 sum of dO * O over the kernel's own bf16 O, within
       D * 2^-24 * sum |dO| |O| per element (an f32 D-term sum and nothing else)
"""
import math

import torch

from attn_harness import CAP, MAX_MARGIN, MED_MARGIN, LOG2E, OUTPUTS, bf16r, nerr, ratios  # noqa: F401
from attn_harness import f32_ulp, lse_stats, lse_violations  # noqa: F401
from attn_harness import violations as _violations

LN2 = math.log(2.0)
TILE = 64  # keys per forward tile (flava.hip SA_T)


def f32_noise(D):
    """the rounding of a D-term f32 sum (attn_harness.F32_NOISE is this at D = 64)"""
    return D * 2.0 ** -24


def violations(stats, D):
    return _violations(stats, noise=f32_noise(D))


def heads_view(x, S, N, heads, D):
    """[S*N, heads*D] -> [N, heads, S, D]"""
    return x.reshape(S, N, heads, D).permute(1, 2, 0, 3)


def rows_view(x, S, N, heads, D):
    """[N, heads, S, D] -> [S*N, heads*D]"""
    return x.permute(2, 0, 1, 3).reshape(S * N, heads * D)


def _qkv(x, S, N, heads, D):
    return x.reshape(S, N, 3, heads, D).permute(2, 1, 3, 0, 4)  # 3 x [N, heads, S, D]


def forward64(x, S, N, heads, D):
    """float64 forward on a float64 qkv (differentiable): O [S*N, E], LSE [N*heads, S], P"""
    q, k, v = _qkv(x, S, N, heads, D)
    sc = q @ k.transpose(-1, -2) / math.sqrt(D)
    P = torch.softmax(sc, -1)
    return rows_view(P @ v, S, N, heads, D), torch.logsumexp(sc, -1).reshape(N * heads, S), P


def ref64(qkv, dO, S, N, heads, D):
    """-> O, LSE (natural log), dQKV in float64 (autograd of O against dO)"""
    x = qkv.detach().double().requires_grad_(True)
    O, lse, _ = forward64(x, S, N, heads, D)
    (g,) = torch.autograd.grad(O, x, dO.double())
    return O.detach(), lse.detach(), g


def lse32(qkv, S, N, heads, D):
    """torch.logsumexp in float32 on the same inputs (the yardstick of the LSE bar)"""
    q, k, _ = _qkv(qkv.float(), S, N, heads, D)
    return torch.logsumexp(q @ k.transpose(-1, -2) / math.sqrt(D), -1).reshape(N * heads, S)


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def model32(qkv, dO, S, N, heads, D, drop_key=None, dkdv_rows=None, swap_v_halves=False):
    """The kernels' arithmetic in float32 -> O, LSE2 (log2 units), dQKV (f32 tensors holding bf16
    values).  Rounding points (flava.hip):
      * scores: Q K^T accumulates in f32, then is multiplied by c = f32(1/sqrt(D)) * log2(e) in f32;
      * forward: keys in 64-key tiles with a running max that moves at every tile (no deferral);
        P = exp2(s - m); the row sum over the unrounded P; P rounded to bf16 before P V; 1/sum
        applied in f32; O rounded at the store; LSE2 = m + log2(sum);
      * delta = sum_d dO * O with the rounded O, in f32;
      * backward: P = exp2(s - LSE2); dS = P (dP - delta) rounded to bf16, the same values for dQ
        and dK; P rounded to bf16 for dV; dQ and dK multiplied by the scale in f32 and rounded at
        the store; dV rounded at the store.
    Defect injection (tests only):
      drop_key       this key is missing from the forward P V and from the backward products
      dkdv_rows      the dK / dV sums run over the first dkdv_rows queries only
      swap_v_halves  the forward reads V's keys 32c + 4g + j and 32c + 16 + 4g + j swapped (the
                     two 4-index halves of the transposed operand: a tr_frag / acc_pair mismatch)"""
    q, k, v = _qkv(qkv.float(), S, N, heads, D)
    do = heads_view(dO.float(), S, N, heads, D)
    scale = (1.0 / torch.sqrt(_f32(float(D)))).item()
    c = (_f32(scale) * _f32(LOG2E)).item()
    s2 = (q @ k.transpose(-1, -2)) * c  # [N, heads, S(query), S(key)], log2 units
    keyok = torch.ones(S, device=qkv.device)
    if drop_key is not None:
        keyok[drop_key] = 0.0
    m = torch.full_like(s2[..., :1], float("-inf"))
    lsum = torch.zeros_like(m)
    acc = torch.zeros_like(v)
    swap = torch.arange(TILE, device=qkv.device) ^ 16
    for k0 in range(0, S, TILE):
        sj = s2[..., k0:k0 + TILE]
        mnew = torch.maximum(m, sj.amax(-1, keepdim=True))
        alpha = torch.exp2(m - mnew)  # first tile: exp2(-inf) = 0
        m, lsum, acc = mnew, lsum * alpha, acc * alpha
        Pu = torch.exp2(sj - m)
        lsum = lsum + Pu.sum(-1, keepdim=True)
        Pb, vj = bf16r(Pu) * keyok[k0:k0 + TILE], v[..., k0:k0 + TILE, :]
        if swap_v_halves:  # the staged tile holds zeros past key S - 1
            pad = TILE - vj.shape[-2]
            vj = torch.nn.functional.pad(vj, (0, 0, 0, pad))[..., swap, :]
            Pb = torch.nn.functional.pad(Pb, (0, pad))
        acc = acc + Pb @ vj
    O = bf16r(acc * (1.0 / lsum))
    lse2 = m + torch.log2(lsum)
    delta = (do * O).sum(-1, keepdim=True)
    P = torch.exp2(s2 - lse2) * keyok
    dS = bf16r(P * (do @ v.transpose(-1, -2) - delta))
    Pd = bf16r(P)
    dQ = bf16r((dS @ k) * scale)
    if dkdv_rows is not None:
        live = (torch.arange(S, device=qkv.device) < dkdv_rows).float().view(1, 1, S, 1)
        dS, Pd = dS * live, Pd * live
    dK = bf16r((dS.transpose(-1, -2) @ q) * scale)
    dV = bf16r(Pd.transpose(-1, -2) @ do)
    dqkv = torch.cat([rows_view(t, S, N, heads, D) for t in (dQ, dK, dV)], 1)
    return rows_view(O, S, N, heads, D), lse2.reshape(N * heads, S), dqkv


def scales(qkv, dO, S, N, heads, D):
    """float64 magnitudes [N, heads, S, D] the rounding errors scale with:
    sO = P |V|,  sV = P^T |dO|,  A = P (|dO| |V|^T + sum_d |dO| |O|),
    sQ = A |K| / sqrt(D),  sK = A^T |Q| / sqrt(D)"""
    x = qkv.double()
    O, _, P = forward64(x, S, N, heads, D)
    q, k, v = (t.abs() for t in _qkv(x, S, N, heads, D))
    do = heads_view(dO.double(), S, N, heads, D).abs()
    A = P * (do @ v.transpose(-1, -2) + (do * heads_view(O, S, N, heads, D).abs()).sum(-1, keepdim=True))
    r = math.sqrt(D)
    return {"O": P @ v, "dV": P.transpose(-1, -2) @ do, "dQ": A @ k / r, "dK": A.transpose(-1, -2) @ q / r}


def split_outputs(O, dqkv, S, N, heads, D):
    """-> {"O", "dQ", "dK", "dV"} as [N, heads, S, D]"""
    E = heads * D
    d = {"O": heads_view(O, S, N, heads, D)}
    for i, name in enumerate(("dQ", "dK", "dV")):
        d[name] = heads_view(dqkv[:, i * E:(i + 1) * E], S, N, heads, D)
    return d


def evaluate(got, model, ref, sc, S, N, heads, D):
    """got / model / ref: (O, dqkv) pairs -> {name: {"max_k", "med_k", "max_m", "med_m", "finite",
    "zero_ok"}}, the input of violations / ratios"""
    g, m, r = (split_outputs(O, dqkv, S, N, heads, D) for O, dqkv in (got, model, ref))
    stats = {}
    for name in OUTPUTS:
        ek, zk = nerr(g[name], r[name], sc[name])
        em, _ = nerr(m[name], r[name], sc[name])
        if ek.numel():
            st = {"max_k": ek.max().item(), "med_k": ek.median().item(),
                  "max_m": em.max().item(), "med_m": em.median().item()}
        else:
            st = {"max_k": 0.0, "med_k": 0.0, "max_m": 0.0, "med_m": 0.0}
        st["finite"] = bool(torch.isfinite(g[name].float()).all())
        st["zero_ok"] = bool((zk == 0).all())
        stats[name] = st
    return stats


def delta_stats(delta, O, dO, S, N, heads, D):
    """delta [N*heads, S] f32 of the kernel against sum_d dO * O in float64 over the kernel's own
    bf16 O -> (max |err|, worst err / bound); bound = D * 2^-24 * sum_d |dO| |O| per element"""
    prod = heads_view(dO.double(), S, N, heads, D) * heads_view(O.double(), S, N, heads, D)
    ref = prod.sum(-1).reshape(N * heads, S)
    bound = f32_noise(D) * prod.abs().sum(-1).reshape(N * heads, S)
    err = (delta.double() - ref).abs()
    worst = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return err.max().item(), worst.max().item()


def delta_violations(delta, O, dO, S, N, heads, D):
    if not torch.isfinite(delta).all():
        return ["delta: non-finite values"]
    e, worst = delta_stats(delta, O, dO, S, N, heads, D)
    return [f"delta: max err {e:.3e}: {worst:.2f} x the bound D * 2^-24 * sum |dO||O|"] if worst > 1.0 else []


def make_inputs(S, N, heads, D, seed, nonneg=False):
    """CPU generator, fixed seed -> qkv bf16 [S*N, 3E] (scale 1.5), dO bf16 [S*N, E] (scale 1).
    nonneg: V and dO replaced by their absolute values (O and dV then have no cancellation: a
    missing key's contribution shows at its full relative size)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    E = heads * D
    qkv = (torch.randn(S * N, 3 * E, generator=g) * 1.5).to(torch.bfloat16)
    dO = torch.randn(S * N, E, generator=g).to(torch.bfloat16)
    if nonneg:
        qkv[:, 2 * E:] = qkv[:, 2 * E:].abs()
        dO = dO.abs()
    return qkv, dO
