"""Reference, rounding model and error metric for the BERT-style attention kernels
(csrc/attention.hip: forward, dQ, dK/dV).  Pure torch; the same functions run on the CPU
and on the device.  Used by test_attention_reference.py (CPU) and test_attention_edges_gpu.py.

Layouts (those of the kernels): qkv [B*L, 3*heads*64] bf16 with the Q | K | V column thirds,
keymask [B, L] f32 additive, dO and O [B*L, heads*64], LSE [B*heads, L] (natural log),
keep [B, heads, L, L] dense 0/1 (all ones without dropout), dQKV like qkv.

  ref64    the operation in float64 with autograd
  model32  the operation in float32, rounding to bf16 exactly where the kernels round
  scales   the per-(token, head) magnitudes the rounding errors are proportional to
  nerr     per (token, head):  ||x - ref||_2 / ||s||_2  over the head's 64 columns

Bars (evaluate / violations), both required on O, dQ, dK and dV:
  cap     nerr <= 3 * 2^-9 on every row: each of the at most three bf16 roundings on a path
          (P or dS; delta through the rounded O; the stored output) contributes at most 2^-9
          of its scale term
  margin  max nerr(kernel) <= 2 x max nerr(model32),  median <= 1.5 x median, per case and
          output, both measured against ref64 on identical inputs (summation order, hardware
          exp2 / log).  A kernel error at or below F32_NOISE = 64 * 2^-24, the rounding of a
          64-term f32 sum, passes the margin whatever the model's: where no bf16 rounding
          occurs at all (L = 1: P = 1, O = V, dQ = dK = 0 exactly) model and kernel differ by
          summation order alone, 1e-8 against 7e-9 or against 0, and a ratio of the two says
          nothing.  It is a tenth of the model's smallest median error anywhere else (4e-5) and
          1/60 of its smallest max, so there the margin is the plain ratio
Rows whose scale is zero (dK / dV of a key masked with -10000; a row whose keys were all
dropped) must be exactly zero.
LSE (lse_violations): |lse - lse64| <= max(8 x max|logsumexp_f32 - lse64|, 4 f32 ulps of |lse64|).
"""
import torch

CAP = 3.0 * 2.0 ** -9
MAX_MARGIN, MED_MARGIN = 2.0, 1.5
F32_NOISE = 64.0 * 2.0 ** -24
LOG2E = 1.4426950408889634
OUTPUTS = ("O", "dQ", "dK", "dV")


def bf16r(x):
    """round an f32 tensor to bf16 (nearest even), kept in f32"""
    return x.to(torch.bfloat16).float()


def heads_view(x, B, L, heads):
    """[B*L, heads*64] -> [B, heads, L, 64]"""
    return x.reshape(B, L, heads, 64).permute(0, 2, 1, 3)


def rows_view(x, B, L, heads):
    """[B, heads, L, 64] -> [B*L, heads*64]"""
    return x.permute(0, 2, 1, 3).reshape(B * L, heads * 64)


def _qkv(x, B, L, heads):
    return x.reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)  # 3 x [B, heads, L, 64]


def forward64(x, keymask, B, L, heads, keep, p):
    """float64 forward on a float64 qkv (differentiable): O [B*L, HD], LSE [B*heads, L], P"""
    q, k, v = _qkv(x, B, L, heads)
    S = q @ k.transpose(-1, -2) / 8.0 + keymask.double().view(B, 1, 1, L)
    P = torch.softmax(S, -1)
    O = rows_view((P * keep.double() / (1.0 - p)) @ v, B, L, heads)
    return O, torch.logsumexp(S, -1).reshape(B * heads, L), P


def ref64(qkv, keymask, dO, B, L, heads, keep, p):
    """-> O, LSE, dQKV in float64 (autograd of O against dO)"""
    x = qkv.detach().double().requires_grad_(True)
    O, lse, _ = forward64(x, keymask, B, L, heads, keep, p)
    (g,) = torch.autograd.grad(O, x, dO.double())
    return O.detach(), lse.detach(), g


def lse32(qkv, keymask, B, L, heads):
    """torch.logsumexp in float32 on the same inputs (the yardstick of the LSE bar)"""
    q, k, _ = _qkv(qkv.float(), B, L, heads)
    S = q @ k.transpose(-1, -2) / 8.0 + keymask.float().view(B, 1, 1, L)
    return torch.logsumexp(S, -1).reshape(B * heads, L)


def model32(qkv, keymask, dO, B, L, heads, keep, p, dkdv_rows=None):
    """The kernels' arithmetic in float32 -> O, LSE, dQKV (f32 tensors holding bf16 values).
    Rounding points (attention.hip):
      * Q pre-scaled by 1/8 (exact); S accumulates in f32 on top of the mask;
      * forward: P = exp(S - m) in f32, the row sum over the undropped, unrounded P; the
        dropped P rounded to bf16 before P V; 1/(1-p) and 1/rowsum applied afterwards in f32;
        O rounded to bf16;  LSE = m + log(rowsum).  m is the kernel's DEFERRED max: keys come
        in 64-key tiles and a row's m moves to a tile's max only when that exceeds m by more
        than 8 in log2 units.  The reference point matters to the rounding: against the true
        max the row's top key is P = 1, exactly representable, against a deferred m it is
        not -- on peaked rows that is the whole P-rounding error of O (a model with the true
        max shows 0.6 x the kernel's worst O error once L > 64);
      * delta = rowsum(dO * O) with the rounded O;
      * backward: P = exp(S - LSE) in f32; dropped P rounded to bf16 before P^T dO;
        dS/zs = P (keep ? dP - delta/zs : -delta/zs) rounded to bf16, zs = 1/(1-p);
      * dQ, dK, dV rounded once, at the store.
    dkdv_rows (defect injection, tests only): the dK / dV sums run over the first dkdv_rows
    query rows only."""
    q, k, v = _qkv(qkv.float(), B, L, heads)
    do = heads_view(dO.float(), B, L, heads)
    keepf = keep.float()
    zs = (1.0 / (1.0 - torch.tensor(p, dtype=torch.float32))).item() if p > 0 else 1.0  # as the kernels: in f32
    S = (q * 0.125) @ k.transpose(-1, -2) + keymask.float().view(B, 1, 1, L)
    # forward: 64-key tiles in order with the kernel's deferred max (DEFER_LOG2 = 8)
    m = torch.full_like(S[..., :1], float("-inf"))
    lsum = torch.zeros_like(m)
    acc = torch.zeros_like(v)
    for k0 in range(0, L, 64):
        Sj = S[..., k0:k0 + 64]
        mx = Sj.amax(-1, keepdim=True)
        upd = (mx - m) * LOG2E > 8.0  # m = -inf: true
        mnew = torch.where(upd, mx, m)
        alpha = torch.where(upd, torch.exp2((m - mnew) * LOG2E), torch.ones_like(m))  # exp2(-inf) = 0
        m, lsum, acc = mnew, lsum * alpha, acc * alpha
        Pu = torch.exp2(Sj * LOG2E - m * LOG2E)
        lsum = lsum + Pu.sum(-1, keepdim=True)
        acc = acc + bf16r(Pu * keepf[..., k0:k0 + 64]) @ v[..., k0:k0 + 64, :]
    O = bf16r(acc * (zs / lsum))
    lse = m + torch.log(lsum)
    ndz = -(do * O).sum(-1, keepdim=True) / zs  # -delta / zs
    P = torch.exp(S - lse)
    dP = do @ v.transpose(-1, -2) + ndz  # the accumulators start at -delta/zs
    dS = bf16r(P * torch.where(keepf > 0, dP, ndz.expand_as(dP)))
    Pd = bf16r(P * keepf)
    dQ = bf16r((dS @ k) * (0.125 * zs))
    if dkdv_rows is not None:
        live = (torch.arange(L, device=qkv.device) < dkdv_rows).float().view(1, 1, L, 1)
        dS, Pd = dS * live, Pd * live
    dK = bf16r((dS.transpose(-1, -2) @ q) * (0.125 * zs))
    dV = bf16r((Pd.transpose(-1, -2) @ do) * zs)
    dqkv = torch.cat([rows_view(t, B, L, heads) for t in (dQ, dK, dV)], 1)
    return rows_view(O, B, L, heads), lse.reshape(B * heads, L), dqkv


def scales(qkv, keymask, dO, B, L, heads, keep, p):
    """float64 magnitudes [B, heads, L, 64] the rounding errors scale with:
    sO = (P keep zs) |V|,  sV = (P keep zs)^T |dO|,
    A = P (zs keep (|dO| |V|^T) + sum_d |dO| |O|),  sQ = A |K| / 8,  sK = A^T |Q| / 8"""
    x = qkv.double()
    O, _, P = forward64(x, keymask, B, L, heads, keep, p)
    q, k, v = (t.abs() for t in _qkv(x, B, L, heads))
    do = heads_view(dO.double(), B, L, heads).abs()
    zs = 1.0 / (1.0 - p)
    Pk = P * keep.double() * zs
    A = P * (zs * keep.double() * (do @ v.transpose(-1, -2))
             + (do * heads_view(O, B, L, heads).abs()).sum(-1, keepdim=True))
    return {"O": Pk @ v, "dV": Pk.transpose(-1, -2) @ do, "dQ": A @ k / 8.0, "dK": A.transpose(-1, -2) @ q / 8.0}


def nerr(x, ref, s):
    """x, ref, s [..., 64] -> (||x - ref|| / ||s|| of the rows with ||s|| > 0 (1-D),
    the rows of x whose scale is zero: they must be exactly zero)"""
    sn = s.double().norm(dim=-1)
    live = sn > 0
    e = (x.double() - ref.double()).norm(dim=-1)
    return e[live] / sn[live], x[~live]


def split_outputs(O, dqkv, B, L, heads):
    """-> {"O", "dQ", "dK", "dV"} as [B, heads, L, 64]"""
    HD = heads * 64
    d = {"O": heads_view(O, B, L, heads)}
    for i, name in enumerate(("dQ", "dK", "dV")):
        d[name] = heads_view(dqkv[:, i * HD:(i + 1) * HD], B, L, heads)
    return d


def evaluate(got, model, ref, sc, B, L, heads, outputs=OUTPUTS):
    """got / model / ref: (O, dqkv) pairs (dqkv may be None when `outputs` is ("O",)).
    -> {name: {"max_k", "med_k", "max_m", "med_m", "zero_ok"}}"""
    parts = []
    for O, dqkv in (got, model, ref):
        if dqkv is None:
            parts.append({"O": heads_view(O, B, L, heads)})
        else:
            parts.append(split_outputs(O, dqkv, B, L, heads))
    g, m, r = parts
    stats = {}
    for name in outputs:
        ek, zk = nerr(g[name], r[name], sc[name])
        em, zm = nerr(m[name], r[name], sc[name])
        if ek.numel():
            st = {"max_k": ek.max().item(), "med_k": ek.median().item(),
                  "max_m": em.max().item(), "med_m": em.median().item()}
        else:
            st = {"max_k": 0.0, "med_k": 0.0, "max_m": 0.0, "med_m": 0.0}
        st["finite"] = bool(torch.isfinite(g[name].float()).all())
        st["zero_ok"] = bool((zk == 0).all())
        stats[name] = st
    return stats


def violations(stats, noise=F32_NOISE):
    """the bars of the module docstring -> list of messages (empty: all held).  noise: the f32
    floor under the margin (seqattn_harness.py passes its own head dimension's)"""
    bad = []
    for name, st in stats.items():
        if not st["finite"]:
            bad.append(f"{name}: non-finite values")
        if not st["zero_ok"]:
            bad.append(f"{name}: a row with zero scale is not exactly zero")
        if not st["max_k"] <= CAP:
            bad.append(f"{name}: max nerr {st['max_k']:.3e} > cap {CAP:.3e}")
        if not st["max_k"] <= max(MAX_MARGIN * st["max_m"], noise):
            bad.append(f"{name}: max nerr {st['max_k']:.3e} > {MAX_MARGIN} x model {st['max_m']:.3e}")
        if not st["med_k"] <= max(MED_MARGIN * st["med_m"], noise):
            bad.append(f"{name}: median nerr {st['med_k']:.3e} > {MED_MARGIN} x model {st['med_m']:.3e}")
    return bad


def ratios(stats):
    """{name: (max ratio, median ratio)} kernel / model (inf where only the model's error is 0)"""
    def div(a, b):
        return a / b if b > 0 else (0.0 if a == 0 else float("inf"))
    return {n: (div(s["max_k"], s["max_m"]), div(s["med_k"], s["med_m"])) for n, s in stats.items()}


def f32_ulp(x):
    """the f32 unit in the last place at |x| (x float64)"""
    _, e = torch.frexp(x.abs().float().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 24).to(torch.int32))


def lse_stats(lse, lse64, lse_f32):
    """-> (max |lse - lse64|, max |logsumexp_f32 - lse64|, worst err / bar)"""
    err = (lse.double() - lse64).abs()
    base = (lse_f32.double() - lse64).abs().max()
    bar = torch.maximum(8.0 * base, 4.0 * f32_ulp(lse64))
    return err.max().item(), base.item(), (err / bar).max().item()


def lse_violations(lse, lse64, lse_f32):
    if not torch.isfinite(lse).all():
        return ["LSE: non-finite values"]
    e, base, worst = lse_stats(lse, lse64, lse_f32)
    return [f"LSE: max err {e:.3e}, f32 logsumexp err {base:.3e}: {worst:.2f} x the bar"] if worst > 1.0 else []


# ------------------------------------------------------------------------------- inputs
M10K = -10000.0


def item2_mask(L, kind):
    """the -10000 key mask of item 2 (bool [L], True = masked); `kind` rotates with the case"""
    km = torch.zeros(L, dtype=torch.bool)
    if L == 1:
        return km
    kind %= 4
    if kind == 0:    # trailing third
        km[L - max(1, L // 3):] = True
    elif kind == 1:  # leading keys: the whole first 64-key tile when L >= 128
        km[:min(70, L // 2)] = True
    elif kind == 2:  # straddles the first tile edge; shorter rows: the middle third
        if L >= 70:
            km[60:70] = True
        else:
            km[L // 3:max(L // 3 + 1, 2 * L // 3)] = True
    else:            # all but one key
        km[:] = True
        km[L // 2] = False
    return km


def make_inputs(B, L, heads, seed, nonneg=False, mask_kind=0):
    """CPU generator, fixed seed -> qkv bf16 [B*L, 3 HD] (scale 1.5), keymask f32 [B, L], dO bf16
    [B*L, HD] (scale 1).  nonneg: V and dO replaced by their absolute values (O and dV then have
    no cancellation: a missing tile's contribution shows at its full relative size).
    Item 0 is unmasked, item 1 carries a random additive N(0, 1) mask, item 2 a -10000 mask."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    HD = heads * 64
    qkv = (torch.randn(B * L, 3 * HD, generator=g) * 1.5).to(torch.bfloat16)
    dO = torch.randn(B * L, HD, generator=g).to(torch.bfloat16)
    km = torch.zeros(B, L)
    if B > 1:
        km[1] = torch.randn(L, generator=g)
    if B > 2:
        km[2, item2_mask(L, mask_kind)] = M10K
    if nonneg:
        qkv[:, 2 * HD:] = qkv[:, 2 * HD:].abs()
        dO = dO.abs()
    return qkv, km, dO


def random_keep(B, L, heads, p, seed):
    if p == 0:
        return torch.ones(B, heads, L, L)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(B, heads, L, L, generator=g) >= p).float()
