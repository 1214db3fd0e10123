"""Reference, rounding model and error metrics for the row kernels: LayerNorm forward / backward
(csrc/layernorm.hip) and the embedding forward / backward (csrc/embed.hip).  Pure torch; the same
functions run on the CPU and on the device.  Used by test_rowops_reference.py (CPU),
test_layernorm_edges_gpu.py and test_embed_edges_gpu.py.

Layouts (those of the kernels): X, Y, dY, dX, dXdrop, dRes [rows, H]; w, b flat f32, row r uses the
H parameters at (r // group_rows) * param_stride; mean, rstd [rows]; partial column sums
[ceil(rows / 64), H]; keep [rows, H] bool (all True without dropout).  Embedding: ids, seg,
txt_mask [B, T] int64, proj [B, n_img, H], source position s of a batch row: 0 [CLS], 1..n_img the
image tokens, n_img + 1 [SEP], then the T text tokens; output row (v, b, j) holds source position
idx[v, j] (or j).

  ln_fwd_ref / ln_bwd_ref / embed_fwd_ref / embed_bwd_ref     ref64: float64, gradients by autograd
  ln_fwd_model / ln_bwd_model / embed_fwd_model / embed_bwd_model
        model32: the same formulas in float32 in the kernels' order (two-pass mean and variance,
        x_hat from the stored f32 mean / rstd), rounding to bf16 only where the kernels store bf16
        (Y, dX, dXdrop, the embedding's X)
  every *_ref also returns the elementwise scales the rounding errors are proportional to:
        Y                  |x_hat| |w| + |b|
        dX                 rstd (|g| + |s1| + |x_hat s2|) [+ |dRes|],  g = dy w, s1 = mean g,
                           s2 = mean g x_hat;   x 1/(1-p) on the kept elements for dXdrop
        column / row sums  the sum of the absolute contributions (of the scales above where the
                           summed quantity is a dX); + |initial value| where the kernel accumulates
        mean               mean |x|;   rstd: rstd

Bars, all against ref64 on identical inputs:
  bf16_elem   |out - ref| <= 2^-8 |ref| + 64 * 2^-24 scale on every element: one bf16 rounding plus
              f32 summation noise
  rownorm     ||out - ref||_2 / ||scale||_2 per row; kernel max <= 2 x the model's max and kernel
              median <= 1.5 x the model's median, per case (summation order, hardware rsqrt): the
              margins of attn_harness
  f32_stats    f32 outputs: |out - ref| <= max(8 x the model's largest |err| / s of the case x s,
              4 f32 ulps of s) on every element, s = the root mean square of the scale over the
              element's row (the element's own scale for mean / rstd)
Dropped elements must be exactly zero; the key mask exactly 0 or -10000.
"""
import torch

MAX_MARGIN, MED_MARGIN = 2.0, 1.5
BF16_REL = 2.0 ** -8
F32_NOISE = 64.0 * 2.0 ** -24
F32_MARGIN, F32_ULPS = 8.0, 4.0
M10K = -10000.0
RPP = 64  # rows per partial column-sum row (kernels.LN_ROWS_PER_PART)


def bf16r(x):
    """round an f32 tensor to bf16 (nearest even), kept in f32"""
    return x.to(torch.bfloat16).float()


def f32_ulp(x):
    """the f32 unit in the last place at |x| (x float64)"""
    _, e = torch.frexp(x.abs().float().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 24).to(torch.int32))


# ------------------------------------------------------------------------------- metrics
def bf16_elem(out, ref, scale):
    """worst |out - ref| / (2^-8 |ref| + 64 * 2^-24 scale); <= 1 passes.  Elements whose bar is 0
    (ref and scale both 0) must be exactly 0: they count as inf otherwise."""
    err = (out.double() - ref.double()).abs()
    bar = BF16_REL * ref.double().abs() + F32_NOISE * scale.double()
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                    torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


def rownorm(out, ref, scale):
    """||out - ref||_2 / ||scale||_2 of every row whose scale is not all zero (1-D)"""
    sn = scale.double().norm(dim=-1)
    e = (out.double() - ref.double()).norm(dim=-1)
    live = sn > 0
    return e[live] / sn[live]


def rownorm_stats(out, model, ref, scale):
    """-> {"max_k", "med_k", "max_m", "med_m"} of the rownorm metric, kernel and model"""
    ek, em = rownorm(out, ref, scale), rownorm(model, ref, scale)
    if not ek.numel():
        return {"max_k": 0.0, "med_k": 0.0, "max_m": 0.0, "med_m": 0.0}
    return {"max_k": ek.max().item(), "med_k": ek.median().item(), "max_m": em.max().item(),
            "med_m": em.median().item()}


def rownorm_violations(name, st):
    bad = []
    if not st["max_k"] <= MAX_MARGIN * st["max_m"]:
        bad.append(f"{name}: max row error {st['max_k']:.3e} > {MAX_MARGIN} x model {st['max_m']:.3e}")
    if not st["med_k"] <= MED_MARGIN * st["med_m"]:
        bad.append(f"{name}: median row error {st['med_k']:.3e} > {MED_MARGIN} x model {st['med_m']:.3e}")
    return bad


def _row_rms(scale):
    return scale if scale.dim() < 2 else scale.pow(2).mean(-1, keepdim=True).sqrt().expand_as(scale)


def f32_stats(out, model, ref, scale):
    """-> (kernel's worst |err| / s, the model's, worst kernel err / bar), s = the root mean square
    of the scale over the element's row (the element's own scale for a 1-D output): a row's
    elements share the errors of its mean and rstd whatever their own size; bar as in the module
    docstring.  Rows with s = 0 must equal ref exactly."""
    ref, s = ref.double(), _row_rms(scale.double())
    ek, em = (out.double() - ref).abs(), (model.double() - ref).abs()
    live = s > 0
    if not live.any():
        return 0.0, 0.0, (float("inf") if (ek > 0).any() else 0.0)
    base = (em[live] / s[live]).max()
    bar = torch.maximum(F32_MARGIN * base * s, F32_ULPS * f32_ulp(s))
    worst = (ek[live] / bar[live]).max().item()
    if (ek[~live] > 0).any():
        worst = float("inf")
    return (ek[live] / s[live]).max().item(), base.item(), worst


def check_bf16(name, out, model, ref, scale, fails, log=None, elem=True):
    """both bf16 bars on one output of one case (elem False: the row-error bar alone); appends
    messages to `fails` -> (elementwise worst / bar, rownorm stats)"""
    if not torch.isfinite(out.float()).all():
        fails.append(f"{name}: non-finite values")
        return float("inf"), None
    el = bf16_elem(out, ref, scale)
    st = rownorm_stats(out, model, ref, scale)
    if log is not None:
        log.append(f"{name}: elem {el:.3f} of the bar; row error kernel {st['max_k']:.3e}/{st['med_k']:.3e} model "
                   f"{st['max_m']:.3e}/{st['med_m']:.3e}")
    if elem and not el <= 1.0:
        fails.append(f"{name}: elementwise error {el:.3f} x the bar")
    fails += rownorm_violations(name, st)
    return el, st


def check_f32(name, out, model, ref, scale, fails, log=None):
    if not torch.isfinite(out.float()).all():
        fails.append(f"{name}: non-finite values")
        return float("inf"), 0.0, float("inf")
    ek, em, worst = f32_stats(out, model, ref, scale)
    if log is not None:
        log.append(f"{name}: err / scale kernel {ek:.3e} model {em:.3e}, {worst:.3f} of the bar")
    if not worst <= 1.0:
        fails.append(f"{name}: f32 error {ek:.3e} of scale (model {em:.3e}): {worst:.2f} x the bar")
    return ek, em, worst


class Worst:
    """the sweep's worst figures per output, for the docstring record"""

    def __init__(self):
        self.d = {}

    def bf(self, name, el, st):
        if st is None:
            return
        w = self.d.setdefault(name, [0.0, 0.0, 0.0, 0.0])
        w[0] = max(w[0], el)
        w[1] = max(w[1], st["max_k"] / st["max_m"] if st["max_m"] > 0 else 0.0)
        w[2] = max(w[2], st["med_k"] / st["med_m"] if st["med_m"] > 0 else 0.0)
        w[3] = max(w[3], st["max_k"])

    def f32(self, name, ek, em, worst):
        w = self.d.setdefault(name, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], ek), max(w[1], em), max(w[2], worst)

    def report(self, tag):
        for n, w in self.d.items():
            if len(w) == 4:
                print(f"SUMMARY {tag} {n}: elem {w[0]:.3f} of bar, row max ratio {w[1]:.3f}, median ratio {w[2]:.3f}, "
                      f"worst row error {w[3]:.3e}")
            else:
                print(f"SUMMARY {tag} {n}: err/scale kernel {w[0]:.3e} model {w[1]:.3e}, {w[2]:.3f} of bar")


# ------------------------------------------------------------------------------- LayerNorm
def row_params(w, rows, H, group_rows=0, param_stride=0):
    """flat parameters -> the [rows, H] parameters of every row"""
    gr = group_rows if group_rows > 0 else rows
    off = (torch.arange(rows, device=w.device) // gr) * param_stride
    return w.reshape(-1)[off[:, None] + torch.arange(H, device=w.device)[None, :]]


def _ln64(x, wr, br, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rs = (var + eps).rsqrt()
    xh = (x - mu) * rs
    return xh * wr + br, mu.squeeze(-1), rs.squeeze(-1), xh


def ln_fwd_ref(X, w, b, eps, group_rows=0, param_stride=0):
    """-> ({"Y", "mean", "rstd"} float64, scales of the same keys)"""
    rows, H = X.shape
    wr, br = row_params(w.double(), rows, H, group_rows, param_stride), \
        row_params(b.double(), rows, H, group_rows, param_stride)
    x = X.double()
    y, mu, rs, xh = _ln64(x, wr, br, eps)
    return {"Y": y, "mean": mu, "rstd": rs}, {"Y": xh.abs() * wr.abs() + br.abs(), "mean": x.abs().mean(-1), "rstd": rs}


def ln_fwd_model(X, w, b, eps, group_rows=0, param_stride=0):
    """-> {"Y" (bf16 values), "Y32", "mean", "rstd"} float32"""
    rows, H = X.shape
    wr, br = row_params(w.float(), rows, H, group_rows, param_stride), \
        row_params(b.float(), rows, H, group_rows, param_stride)
    x = X.float()
    mu = x.sum(-1, keepdim=True) / H
    d = x - mu
    rs = torch.rsqrt((d * d).sum(-1, keepdim=True) / H + eps)
    y = d * rs * wr + br
    return {"Y": bf16r(y), "Y32": y, "mean": mu.squeeze(-1), "rstd": rs.squeeze(-1)}


def part_sums(t, rpp=RPP):
    """[rows, H] -> [ceil(rows / rpp), H]: the sums over consecutive blocks of rpp rows"""
    rows, H = t.shape
    parts = (rows + rpp - 1) // rpp
    pad = torch.zeros(parts * rpp, H, dtype=t.dtype, device=t.device)
    pad[:rows] = t
    return pad.view(parts, rpp, H).sum(1)


def ln_bwd_ref(dY, X, w, eps, dRes=None, keep=None, p=0.0, rpp=RPP):
    """float64 autograd of y = x_hat(x) * w against dY [+ dRes]; keep / p: the dropout whose
    backward the kernel fuses -> ({"dX", "dXdrop", "pdw", "pdb", "pdbias"}, scales).
    pdbias sums dXdrop when p > 0 or a keep mask is given, else dX (with dRes)."""
    rows, H = X.shape
    x = X.detach().double().requires_grad_(True)
    wr = w.double().view(1, H)
    y, mu, rs, xh = _ln64(x, wr, torch.zeros_like(wr), eps)
    dy = dY.double()
    (dx,) = torch.autograd.grad(y, x, dy)
    xh, rs = xh.detach(), rs.detach().unsqueeze(-1)
    g = dy * wr
    s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    sdx = rs * (g.abs() + s1.abs() + (xh * s2).abs())
    if dRes is not None:
        dx = dx + dRes.double()
        sdx = sdx + dRes.double().abs()
    kf = torch.ones_like(dx) if keep is None else keep.double()
    zs = 1.0 / (1.0 - p)
    dxd, sdxd = dx * kf * zs, sdx * kf * zs
    ref = {"dX": dx, "dXdrop": dxd, "pdw": part_sums(dy * xh, rpp), "pdb": part_sums(dy, rpp),
           "pdbias": part_sums(dxd, rpp)}
    sc = {"dX": sdx, "dXdrop": sdxd, "pdw": part_sums((dy * xh).abs(), rpp), "pdb": part_sums(dy.abs(), rpp),
          "pdbias": part_sums(sdxd, rpp)}
    return ref, sc


def ln_bwd_model(dY, X, mean, rstd, w, dRes=None, keep=None, p=0.0, rpp=RPP):
    """ln_bwd_kernel in float32: x_hat from the given f32 mean / rstd; dX and dXdrop rounded to
    bf16 at the store; the partial sums from the unrounded f32 values"""
    rows, H = X.shape
    x, dy, wr = X.float(), dY.float(), w.float().view(1, H)
    mu, rs = mean.float().view(rows, 1), rstd.float().view(rows, 1)
    xh = (x - mu) * rs
    g = dy * wr
    s1, s2 = g.sum(-1, keepdim=True) / H, (g * xh).sum(-1, keepdim=True) / H
    dx = rs * (g - s1 - xh * s2)
    if dRes is not None:
        dx = dx + dRes.float()
    zs = (1.0 / (1.0 - torch.tensor(p, dtype=torch.float32))).item() if p > 0 else 1.0
    dxd = dx * zs if keep is None else torch.where(keep, dx * zs, torch.zeros_like(dx))
    return {"dX": bf16r(dx), "dXdrop": bf16r(dxd), "pdw": part_sums(dy * xh, rpp), "pdb": part_sums(dy, rpp),
            "pdbias": part_sums(dxd, rpp)}


def ln_inputs(rows, H, kind, seed, groups=1, param_stride=None, f32=False):
    """CPU generator -> X (bf16 or f32), w, b (flat f32), dY, dRes (bf16).
    kind: "gauss" N(0, 2^2); "offset" the same + 8 (the mean dominates: cancellation in x - mean);
    "wide" row scales log-uniform in 1e-2 .. 10.
    The elementwise bar on the forward's Y is not applied to "offset" (ELEM_KINDS): there the f32
    subtraction x - mean alone is off by |mean| 2^-24 rstd |w| on every element of the row, which
    the scale |x_hat| |w| + |b| of an element near zero does not carry -- the float32 model
    itself misses that bar on such rows by up to 2.4 x.  The row-error and f32 bars, relative to
    the model on the same inputs, hold on all three, and so does the elementwise bar on dX and
    dXdrop: x_hat enters them through x_hat s2 alone, and their scale carries rstd |s1| on every
    element."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, H, generator=g) * 2.0
    if kind == "offset":
        x = x + 8.0
    elif kind == "wide":
        x = x * (10.0 ** (torch.rand(rows, 1, generator=g) * 3.0 - 2.0))
    if not f32:  # (the f32 draws carry 24-bit significands: values bf16 cannot hold)
        x = x.to(torch.bfloat16)
    ps = H if param_stride is None else param_stride
    n = (groups - 1) * ps + H
    w = torch.randn(n, generator=g) * 0.1 + 1.0
    b = torch.randn(n, generator=g) * 0.1
    dY = torch.randn(rows, H, generator=g).to(torch.bfloat16)
    dRes = torch.randn(rows, H, generator=g).to(torch.bfloat16)
    return x, w, b, dY, dRes


KINDS = ("gauss", "offset", "wide")
ELEM_KINDS = ("gauss", "wide")
LN_H = (256, 512, 768, 1024)
LN_FWD_ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33)
# (groups, group_rows, param_stride as a multiple of H): row per wave, pairs, one row per group, shared params
LN_FWD_GROUPED = ((3, 5, 1), (3, 6, 1), (7, 1, 1), (3, 5, 0))
LN_BWD_ROWS = (1, 3, 4, 5, 8, 9, 63, 64, 65, 127, 129)


def random_keep(rows, H, p, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(rows, H, generator=g) >= p


# ------------------------------------------------------------------------------- embedding
def _embed_sources(ids, seg, proj, word, pos, typ, cls_id, sep_id, T, n_img):
    """the pre-LayerNorm rows of every source position [B, n_img + 2 + T, H], summed in the
    kernel's order (word or image projection, + position, + token type)"""
    B = proj.shape[0]
    H = word.shape[1]
    head = torch.cat([word[cls_id].expand(B, 1, H), proj, word[sep_id].expand(B, 1, H)], 1)
    head = (head + pos[:n_img + 2].unsqueeze(0)) + typ[0]
    if T == 0:
        return head
    text = (word[ids] + pos[:T].unsqueeze(0)) + typ[seg]
    return torch.cat([head, text], 1)


def embed_layout(B, T, n_img, idx=None, V=1, Lout=None, device=None):
    """-> src [V, Lout] int64: the source position of every output column"""
    S = n_img + 2 + T
    if idx is None:
        return torch.arange(S, device=device).view(1, S).expand(V, S)
    return idx.view(V, Lout)


def _embed_fwd(dt, ids, seg, txt_mask, proj, word, pos, typ, ln_w, ln_b, eps, cls_id, sep_id, idx, V, B, T, n_img,
               Lout, keep, drop_txt, drop_img):
    H = word.shape[1]
    E = _embed_sources(ids, seg, proj.to(dt), word.to(dt), pos.to(dt), typ.to(dt), cls_id, sep_id, T, n_img)
    src = embed_layout(B, T, n_img, idx, V, Lout, device=E.device)
    Lo = src.shape[1]
    e = E[:, src].permute(1, 0, 2, 3).reshape(V * B * Lo, H)  # rows (v, b, j)
    s_row = src.unsqueeze(1).expand(V, B, Lo).reshape(-1)
    is_img = s_row <= n_img + 1
    if dt == torch.float64:
        y, mu, rs, xh = _ln64(e, ln_w.to(dt).view(1, H), ln_b.to(dt).view(1, H), eps)
    else:
        mu = e.sum(-1, keepdim=True) / H
        d = e - mu
        rs = torch.rsqrt((d * d).sum(-1, keepdim=True) / H + eps)
        xh = d * rs
        y = xh * ln_w.to(dt).view(1, H) + ln_b.to(dt).view(1, H)
        mu, rs = mu.squeeze(-1), rs.squeeze(-1)
    one = torch.ones((), dtype=dt, device=e.device)
    if dt == torch.float64:
        zs = torch.where(is_img, 1.0 / (1.0 - drop_img) * one, 1.0 / (1.0 - drop_txt) * one)
    else:  # as the kernel: 1 / (1 - p) in f32
        zi = 1.0 / (1.0 - torch.tensor(drop_img, dtype=dt)) if drop_img > 0 else one
        zt = 1.0 / (1.0 - torch.tensor(drop_txt, dtype=dt)) if drop_txt > 0 else one
        zs = torch.where(is_img, zi.to(e.device), zt.to(e.device))
    kf = torch.ones_like(y) if keep is None else keep.to(dt)
    out = y * zs.unsqueeze(-1) * kf
    km = torch.zeros(V * B * Lo, dtype=dt, device=e.device)
    if txt_mask is not None and T > 0:
        t_row = (s_row - n_img - 2).clamp_min(0)
        b_row = torch.arange(B, device=e.device).view(1, B, 1).expand(V, B, Lo).reshape(-1)
        km = torch.where(~is_img & (txt_mask[b_row, t_row] == 0), torch.full_like(km, M10K), km)
    scale = (xh.abs() * ln_w.to(dt).abs().view(1, H) + ln_b.to(dt).abs().view(1, H)) * zs.unsqueeze(-1) * kf
    return out, mu, rs, km, scale, (e, xh, is_img, zs)


def embed_fwd_ref(ids, seg, txt_mask, proj, word, pos, typ, ln_w, ln_b, eps, cls_id, sep_id, idx, V, B, T, n_img,
                  Lout, keep=None, drop_txt=0.0, drop_img=0.0):
    """float64 -> ({"X", "mean", "rstd", "keymask"}, scales of X / mean / rstd)"""
    out, mu, rs, km, scale, (e, _, _, _) = _embed_fwd(torch.float64, ids, seg, txt_mask, proj, word, pos, typ, ln_w,
                                                      ln_b, eps, cls_id, sep_id, idx, V, B, T, n_img, Lout, keep,
                                                      drop_txt, drop_img)
    return {"X": out, "mean": mu, "rstd": rs, "keymask": km}, {"X": scale, "mean": e.abs().mean(-1), "rstd": rs}


def embed_fwd_model(ids, seg, txt_mask, proj, word, pos, typ, ln_w, ln_b, eps, cls_id, sep_id, idx, V, B, T, n_img,
                    Lout, keep=None, drop_txt=0.0, drop_img=0.0):
    """float32 -> {"X" (bf16 values), "X32", "mean", "rstd", "keymask"}"""
    out, mu, rs, km, _, _ = _embed_fwd(torch.float32, ids, seg, txt_mask, proj, word, pos, typ, ln_w, ln_b, eps,
                                       cls_id, sep_id, idx, V, B, T, n_img, Lout, keep, drop_txt, drop_img)
    return {"X": bf16r(out), "X32": out, "mean": mu, "rstd": rs, "keymask": km}


GRADS = ("d_word", "d_pos", "d_type", "d_ln_w", "d_ln_b", "d_proj")


def embed_bwd_ref(dX, ids, seg, proj, word, pos, typ, ln_w, ln_b, eps, cls_id, sep_id, B, T, n_img, keep=None,
                  drop_txt=0.0, drop_img=0.0, init=None):
    """identity variant: float64 autograd of sum(X * dX) -> ({GRADS}, scales).  init: the values
    the accumulated gradient buffers (all but d_proj) held before the call"""
    leaves = [t.detach().double().requires_grad_(True) for t in (word, pos, typ, ln_w, ln_b, proj)]
    w_, p_, t_, lw_, lb_, pr_ = leaves
    S = n_img + 2 + T
    out, mu, rs, _, _, (e, xh, is_img, zs) = _embed_fwd(torch.float64, ids, seg, None, pr_, w_, p_, t_, lw_, lb_, eps,
                                                        cls_id, sep_id, None, 1, B, T, n_img, S, keep, drop_txt,
                                                        drop_img)
    gr = torch.autograd.grad(out, leaves, dX.double())
    ref = dict(zip(GRADS, gr))
    # scales: the sums of the absolute contributions
    kf = torch.ones_like(out) if keep is None else keep.double()
    dy = (dX.double() * zs.unsqueeze(-1) * kf).detach()
    xh, rs = xh.detach(), rs.detach().unsqueeze(-1)
    g = dy * ln_w.double().view(1, -1)
    s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    sdx = rs * (g.abs() + s1.abs() + (xh * s2).abs())
    sc = _embed_scatter(sdx, (dy * xh).abs(), dy.abs(), ids, seg, word.shape[0], pos.shape[0], cls_id, sep_id, B, T,
                        n_img)
    if init is not None:
        for k in GRADS[:5]:
            ref[k] = ref[k] + init[k].double()
            sc[k] = sc[k] + init[k].double().abs()
    return ref, sc


def _embed_scatter(dx, dyxh, dy, ids, seg, n_word, n_pos, cls_id, sep_id, B, T, n_img):
    """the embedding backward's sums of the row gradients dx [B * S, H] (any dtype)"""
    H = dx.shape[1]
    S = n_img + 2 + T
    d = dx.view(B, S, H)
    z = lambda n: torch.zeros(n, H, dtype=dx.dtype, device=dx.device)  # noqa: E731
    d_word, d_pos, d_type = z(n_word), z(n_pos), z(2)
    d_word[cls_id] += d[:, 0].sum(0)
    d_word[sep_id] += d[:, n_img + 1].sum(0)
    d_pos[:n_img + 2] += d[:, :n_img + 2].sum(0)
    d_type[0] += d[:, :n_img + 2].sum((0, 1))
    if T > 0:
        txt = d[:, n_img + 2:]
        d_word.index_add_(0, ids.reshape(-1), txt.reshape(-1, H))
        d_pos[:T] += txt.sum(0)
        d_type.index_add_(0, seg.reshape(-1), txt.reshape(-1, H))
    return {"d_word": d_word, "d_pos": d_pos, "d_type": d_type, "d_ln_w": dyxh.sum(0), "d_ln_b": dy.sum(0),
            "d_proj": d[:, 1:n_img + 1].clone()}


def embed_bwd_model(dX, ids, seg, proj, word, pos, typ, ln_w, mean, rstd, cls_id, sep_id, B, T, n_img, keep=None,
                    drop_txt=0.0, drop_img=0.0, init=None):
    """embed_bwd_rows_kernel in float32: dy = the kept dX / (1 - p), x_hat from the given f32 mean
    and rstd, the row gradients summed in f32"""
    S = n_img + 2 + T
    H = word.shape[1]
    e = _embed_sources(ids, seg, proj.float(), word.float(), pos.float(), typ.float(), cls_id, sep_id, T,
                       n_img).reshape(B * S, H)
    s_row = torch.arange(S, device=e.device).repeat(B)
    one = torch.ones((), dtype=torch.float32)
    zi = 1.0 / (1.0 - torch.tensor(drop_img)) if drop_img > 0 else one
    zt = 1.0 / (1.0 - torch.tensor(drop_txt)) if drop_txt > 0 else one
    zs = torch.where(s_row <= n_img + 1, zi.to(e.device), zt.to(e.device)).unsqueeze(-1)
    dy = dX.float() * zs
    if keep is not None:
        dy = torch.where(keep, dy, torch.zeros_like(dy))
    mu, rs = mean.float().view(-1, 1), rstd.float().view(-1, 1)
    xh = (e - mu) * rs
    g = dy * ln_w.float().view(1, H)
    s1, s2 = g.sum(-1, keepdim=True) / H, (g * xh).sum(-1, keepdim=True) / H
    dx = rs * (g - s1 - xh * s2)
    out = _embed_scatter(dx, dy * xh, dy, ids, seg, word.shape[0], pos.shape[0], cls_id, sep_id, B, T, n_img)
    if init is not None:
        for k in GRADS[:5]:
            out[k] = out[k] + init[k].float()
    return out


def embed_inputs(B, T, n_img, seed, vocab=300, n_pos=512, H=768, ids_kind="random", seg_kind="mixed", cls_id=101,
                 sep_id=102, mask_zeros=True):
    """CPU generator -> dict of ids, seg, txt_mask, proj, word, pos, typ, ln_w, ln_b, dX (bf16).
    ids_kind: "random" | "equal" (every id the same word row) | "special" (random, with [CLS] and
    [SEP] ids among them); seg_kind: "mixed" | "zeros" | "ones"."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    S = n_img + 2 + T
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = {"word": r(vocab, H) * 0.05, "pos": r(n_pos, H) * 0.05, "typ": r(2, H) * 0.05, "ln_w": 1 + 0.1 * r(H),
         "ln_b": 0.1 * r(H), "proj": r(B, n_img, H) * 0.05, "dX": r(B * S, H).to(torch.bfloat16)}
    ids = torch.randint(0, vocab, (B, T), generator=g)
    if ids_kind == "equal":
        ids = torch.full((B, T), 7)
    elif ids_kind == "special":
        ids.view(-1)[::2] = cls_id
        ids.view(-1)[1::3] = sep_id
    seg = torch.randint(0, 2, (B, T), generator=g)
    if seg_kind != "mixed":
        seg = torch.full((B, T), 0 if seg_kind == "zeros" else 1)
    tm = torch.ones(B, T, dtype=torch.int64)
    if mask_zeros:
        tm[torch.rand(B, T, generator=g) < 0.3] = 0
    d.update(ids=ids, seg=seg, txt_mask=tm, cls_id=cls_id, sep_id=sep_id)
    return d


# the embedding sweeps (test_rowops_reference.py runs the model over them, test_embed_edges_gpu.py the kernels)
EMBED_N_IMG = (1, 3)
EMBED_FWD_SHAPES = ((1, 1), (1, 16), (3, 17), (5, 2))     # (B, T): row totals that are no multiple of 4
EMBED_BWD_B = (1, 15, 16, 17, 33)                         # around the backward's 16 samples per block
EMBED_BWD_T = (1, 9, 17)
EMBED_BWD_KINDS = (("random", "mixed"), ("equal", "ones"), ("special", "zeros"))  # (ids_kind, seg_kind)
DROP_IMG, DROP_TXT = 0.3, 0.1


def index_sets(S, g):
    """three index sets for one launch, Lout = S + 2: a permutation (padded with two repeats),
    repeated positions, and a random draw"""
    perm = torch.randperm(S, generator=g)
    a = torch.cat([perm, perm[:2]])
    b = torch.cat([torch.zeros(3, dtype=torch.int64), torch.full((S - 1,), S - 1)])
    c = torch.randint(0, S, (S + 2,), generator=g)
    return torch.stack([a, b, c])


def embed_fwd_variants(B, T, n_img):
    """-> [(name, idx, V, Lout)]: identity, three index sets in one launch, a shorter gather"""
    S = n_img + 2 + T
    g = torch.Generator().manual_seed(B * T)
    return [("identity", None, 1, S), ("idx", index_sets(S, g), 3, S + 2),
            ("idx-short", torch.randint(0, S, (1, S - 2), generator=g), 1, S - 2)]
