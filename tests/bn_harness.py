"""Reference, rounding model, case lists and inputs for the BatchNorm kernels (csrc/batchnorm.hip).
Pure torch; the same functions run on the CPU and on the device.  Used by test_bn_reference.py (CPU)
and test_batchnorm_edges_gpu.py.  The metrics and their constants are rowops_harness's (bf16_elem,
rownorm_stats / rownorm_violations, f32_stats: MAX_MARGIN 2, MED_MARGIN 1.5, F32_MARGIN 8,
F32_ULPS 4, 2^-8, 64 * 2^-24); a "row" of the row-error bar is a channel here, so the maps are
transposed before it (check_map).

Layouts (those of the kernels): X, skip, dY, Y, dX, dSkip [rows, C] bf16 (an NHWC map as
[N*H*W, C]); w, b, the running and saved statistics, dweight, dbias [C] f32; the ReLU mask
[rows, C] bool here ([rows * C / 8] bytes, bit e of byte (r, c / 8) = element (r, c + e), in the
kernels: mask_bits / mask_bools convert); a stream residue [rows, C] int8.

  bn_fwd_ref / bn_bwd_ref       ref64: float64 on the same bf16 inputs
  bn_stats_model / bn_fwd_model / bn_bwd_sums_model / bn_bwd_model
        model32: the same in float32 in the kernels' order -- per-block f32 partials (a thread's
        rows r0 + rs, r0 + rs + rpi, ... summed in turn, sum2 by fused multiply-add, then the
        block's rpi row slots in turn), the finalize in float64 (var = s2 / n - mean^2 clamped
        at 0, invstd = float(1 / sqrt(var + eps))), scale = w invstd, shift = b - mean scale,
        Y = bf16(x scale + shift [+ skip [+ residue]]), dx = bf16(k1 g + (k2 x + k0)); rounding to
        bf16 only where the kernels store bf16.  The fused multiply-adds (the kernels' fmaf, and
        the contraction of b - mean * scale) are formed in float64 and rounded once.
  every *_ref also returns the elementwise scales the rounding errors are proportional to:
        Y          |x_hat| |w| + |b| (+ |skip|)
        dX         invstd |w| (|g| + mean |g| + |x_hat| mean |g x_hat|)
        dweight, dbias, mean     the sum (mean) of the absolute contributions, + |initial value|
                   where the kernel accumulates;  running mean / variance: (1 - mom) |old| + mom x
                   mean |x| / mean x^2 n / (n - 1)
        invstd     invstd

bn_geometry asks the host for bn_grid's choice (mmu_batchnorm_plan; the built library, no GPU).  It
chooses the row counts of the sweep (bn_rows), the two rows the "tail" inputs make large, and the
block split of the model's partial sums; the dense list BN_DENSE does not depend on it.
"""
import torch

from rowops_harness import bf16r, check_bf16
from src import kernels

BN_EPS = 1e-5
RES_BAR = 2.0 ** -13   # the decoded stream against the f32 value (test_batchnorm_stream_residue's bar)
RES_ROUNDTRIP = 2.0 ** -15
TINY, HUGE = 2.0 ** -126, 2.0 ** 127   # the residue's range: normal bf16 values below the top exponent


def eps32(eps=BN_EPS):
    """eps as the kernels see it: rounded to f32"""
    return torch.tensor(eps, dtype=torch.float32).double().item()


# ------------------------------------------------------------------------------- geometry
def bn_geometry(rows, C):
    """the host's own row-block grid for a [rows, C] map (kernels.batchnorm_plan: mmu_batchnorm_plan
    reports bn_grid of csrc/batchnorm.hip) -> {"CH", "rpi", "rpb", "blocks" (grid.x = nparts), "gy"
    (grid.y), "clamped"} and the label "tpr": the threads that share a row"""
    g = kernels.batchnorm_plan(rows, C)
    g.update(tpr=g["CH"] // 8, clamped=bool(g["clamped"]))
    return g


BN_C = (8, 24, 64, 96, 256, 520, 2048)      # CH = 8, 8 x 3, 64, 32 x 3, 256, 8 x 65, 512 x 4
BN_ALL_KINDS_C = (8, 96, 2048)              # every input kind here; "unit" and "tail" at the other C
KINDS = ("unit", "offset", "range", "const", "tail")
BN_DENSE = tuple((C, rows) for C in (2048, 256) for rows in range(2, 71))
# (C, rows) the list of the issue names but bn_grid cannot serve as meant: at C = 520 (CH = 8,
# rpb = 1024 at the 8 K-element floor) 33 rpb + 1 = 33 793 rows are 17.6 M elements, where bn_grid
# has left the floor (rpb 2304, 15 row blocks): no wrap of the 32 finalize slices, which C = 520
# reaches only past 262 144 rows = 136 M elements
BN_UNREACHABLE = ((520, 33793),)


def bn_rows(C):
    """the row counts of the sweep at C: 2, 3, rpi - 1, rpi + 1, rpb, rpb + 1, 2 rpb + rpi + 1,
    33 rpb + 1 (rpi, rpb at the 8 K-element floor), those kept at which bn_grid still has that rpb"""
    g = bn_geometry(2, C)
    rpi, rpb = g["rpi"], g["rpb"]
    out = []
    for r in (2, 3, rpi - 1, rpi + 1, rpb, rpb + 1, 2 * rpb + rpi + 1, 33 * rpb + 1):
        if r >= 2 and r not in out and (C, r) not in BN_UNREACHABLE:
            out.append(r)
    return out


def bn_cases(C):
    """-> [(rows, kind)] of the sweep at C: the grid and (C = 2048, 256) the dense list for
    "unit" and "tail", the grid alone for the other kinds at BN_ALL_KINDS_C"""
    grid = bn_rows(C)
    dense = [r for c, r in BN_DENSE if c == C and r not in grid]
    out = [(r, k) for k in ("unit", "tail") for r in grid + dense]
    if C in BN_ALL_KINDS_C:
        out += [(r, k) for k in ("offset", "range", "const") for r in grid]
    return out


# ------------------------------------------------------------------------------- inputs
CONST_CH = (0, 3, -1)   # the exactly constant channels of the "const" kind


def bn_inputs(rows, C, kind, seed):
    """CPU generator -> dict: X, skip, dY (bf16 [rows, C]), w, b, rm0, rv0, dw0, db0 (f32 [C]), and
    the skip as a residual stream: skip_s (bf16) + skip_res (int8 residue).
    kind: "unit" N(0, 1); "offset" N(8, 1): the mean is 8 x the spread, as after a ReLU (the
    cancellation in s2 / n - mean^2); "range" channel c scaled by 2^(c % 9 - 4); "const" channels
    CONST_CH exactly constant (var = 0, invstd = eps^-1/2); "tail" the last row and the first row
    of the last row block hold values 16 x the rest, so statistics that miss a row move visibly."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, C, generator=g)
    if kind == "offset":
        x = x + 8.0
    elif kind == "range":
        x = x * torch.ldexp(torch.ones(C), (torch.arange(C) % 9 - 4).to(torch.int32))
    elif kind == "const":
        for i, c in enumerate(CONST_CH):
            x[:, c] = (0.5, -1.25, 3.0)[i]
    elif kind == "tail":
        geo = bn_geometry(rows, C)
        first = (geo["blocks"] - 1) * geo["rpb"]
        x[rows - 1] *= 16.0
        if first != rows - 1:
            x[first] *= 16.0
    w = torch.rand(C, generator=g) + 0.5
    w[::5] = -w[::5]
    d = {"X": x.to(torch.bfloat16), "w": w, "b": torch.randn(C, generator=g) * 0.1,
         "skip": torch.randn(rows, C, generator=g).to(torch.bfloat16),
         "dY": torch.randn(rows, C, generator=g).to(torch.bfloat16),
         "rm0": torch.randn(C, generator=g) * 0.1, "rv0": torch.rand(C, generator=g) + 0.5,
         "dw0": torch.randn(C, generator=g) * 0.25, "db0": torch.randn(C, generator=g) * 0.5}
    # the skip as a stream: f32 values whose bf16 part is `skip` and whose rest is the residue
    s32 = d["skip"].float() * (1.0 + (torch.rand(rows, C, generator=g) - 0.5) * 2.0 ** -8)
    s32[0, :] = 0.0  # exact zeros in the stream
    hi, res = res_encode(s32)
    d["skip_s"], d["skip_res"] = hi, res
    return d


# ------------------------------------------------------------------------------- stream residue
def _res_scale(h):
    """2^(e - 15), e the binary exponent of h (f32); 0 for h == 0 or denormal (bn_res_scale)"""
    _, ex = torch.frexp(h)
    return torch.where(h.abs() < TINY, torch.zeros_like(h), torch.ldexp(torch.ones_like(h), ex - 16))


def res_encode(v):
    """bn_res_encode restated: f32 v -> (bf16(v), int8 rint((v - hi) 2^15 / 2^e) clamped to 127);
    no residue (0) where hi is zero, denormal or at the top exponent"""
    hi = v.to(torch.bfloat16)
    h = hi.float()
    none = (h.abs() < TINY) | (h.abs() >= HUGE)
    _, ex = torch.frexp(torch.where(none, torch.ones_like(h), h))
    q = ((v - h) * torch.ldexp(torch.ones_like(h), 16 - ex)).clamp(-127.0, 127.0).round()
    return hi, torch.where(none, torch.zeros_like(q), q).to(torch.int8)


def res_decode(hi, res, dtype=torch.float32):
    """the stream's value: hi + res 2^(e - 15)"""
    h = hi.float()
    return h.to(dtype) + res.to(dtype) * _res_scale(h).to(dtype)


def mask_bits(m):
    """[rows, C] bool -> the kernels' [rows * C / 8] uint8"""
    sh = torch.arange(8, device=m.device, dtype=torch.int32)
    return (m.reshape(-1, 8).to(torch.int32) << sh).sum(1).to(torch.uint8)


def mask_bools(bits, rows, C):
    sh = torch.arange(8, device=bits.device, dtype=torch.int32)
    return ((bits.to(torch.int32).unsqueeze(1) >> sh) & 1).bool().view(rows, C)


# ------------------------------------------------------------------------------- forward
def _momentum(momentum, nbt, dt):
    """the update factor: momentum, or (momentum < 0, torch's momentum=None) 1 / num_batches_tracked
    with this pass already counted"""
    if momentum >= 0:
        return torch.tensor(momentum, dtype=torch.float32).to(dt)
    return (1.0 / torch.tensor(float(nbt), dtype=torch.float32)).to(dt)


def bn_fwd_ref(X, w, b, eps=BN_EPS, training=True, rmean=None, rvar=None, momentum=0.1, nbt=1, relu=False,
               skip=None, skip_res=None):
    """float64 -> ({"Y" (unrounded), "mean", "invstd", "rmean", "rvar"}, scales of the same keys).
    training: batch statistics, the running ones updated (biased variance normalises, the unbiased
    one updates, factor as _momentum); eval: normalised by rmean / rvar.  skip (+ skip_res: its
    stream residue) is added before the ReLU."""
    x = X.double()
    n = x.shape[0]
    e = eps32(eps)
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
    else:
        mean, var = rmean.double(), rvar.double()
    invstd = (var + e).rsqrt()
    xh = (x - mean) * invstd
    y = xh * w.double() + b.double()
    sy = xh.abs() * w.double().abs() + b.double().abs()
    if skip is not None:
        s = skip.double() if skip_res is None else res_decode(skip, skip_res, torch.float64)
        y = y + s
        sy = sy + s.abs()
    if relu:
        y = y.clamp_min(0.0)
    ref = {"Y": y, "mean": mean, "invstd": invstd}
    sc = {"Y": sy, "mean": x.abs().mean(0), "invstd": invstd}
    if training and rmean is not None:
        mom = _momentum(momentum, nbt, torch.float64).to(x.device)
        ub = n / (n - 1.0)
        ref["rmean"] = (1.0 - mom) * rmean.double() + mom * mean
        ref["rvar"] = (1.0 - mom) * rvar.double() + mom * var * ub
        sc["rmean"] = (1.0 - mom) * rmean.double().abs() + mom * sc["mean"]
        sc["rvar"] = (1.0 - mom) * rvar.double().abs() + mom * (x * x).mean(0) * ub
    return ref, sc


def _fma(a, b, c):
    """f32 fused multiply-add: the product is exact in float64, the sum rounded once (twice, to
    f64 then f32: a difference only where the f64 sum lies within 2^-29 of an f32 tie)"""
    return (a.double() * b.double() + c.double()).float()


def _partials(a, p1, p2, geo):
    """the reduce passes' block partials in the kernels' order -> per channel (sum a, sum p1 p2)
    as the finalize's float64 totals.  a, p1, p2 [rows, C] f32."""
    rows, C = a.shape
    rpb, rpi = geo["rpb"], geo["rpi"]
    nblk, iters = geo["blocks"], rpb // rpi
    pad = nblk * rpb - rows

    def shaped(t):
        if pad:
            t = torch.cat([t, torch.zeros(pad, C, dtype=t.dtype, device=t.device)])
        return t.view(nblk, iters, rpi, C)

    a, p1, p2 = shaped(a), shaped(p1), shaped(p2)
    live = -(-min(rows, rpb) // rpi)  # iterations any block runs
    s = torch.zeros(nblk, rpi, C, dtype=torch.float32, device=a.device)
    q = torch.zeros_like(s)
    for it in range(live):
        s = s + a[:, it]
        q = _fma(p1[:, it], p2[:, it], q)
    S = torch.zeros(nblk, C, dtype=torch.float32, device=a.device)
    Q = torch.zeros_like(S)
    for r in range(min(rpi, rows)):
        S = S + s[:, r]
        Q = Q + q[:, r]
    return S.double().sum(0), Q.double().sum(0)


def bn_stats_model(X):
    """bn_stats_kernel + bn_sum_parts -> (sum x, sum x^2) per channel, float64"""
    x = X.float()
    return _partials(x, x, x, bn_geometry(*X.shape))


def bn_fwd_model(X, w, b, eps=BN_EPS, training=True, sums=None, rmean=None, rvar=None, momentum=0.1, nbt=1,
                 relu=False, skip=None, skip_res=None):
    """-> {"Y" (bf16 values), "V" (the f32 value before the store), "mean", "invstd", "rmean",
    "rvar"} float32.  sums = (s1, s2, n): the float64 totals of bn_stats_model (of this map, or
    the exchanged ones of a cross-rank pass); None: computed here."""
    x = X.float()
    e = eps32(eps)
    out = {}
    if training:
        if sums is None:
            sums = bn_stats_model(X) + (X.shape[0],)
        s1, s2, n = sums
        mean = s1 / n
        var = (s2 / n - mean * mean).clamp_min(0.0)
    else:
        mean, var = rmean.double(), rvar.double()
    invstd = (1.0 / (var + e).sqrt()).float()
    scale = w.float() * invstd
    shift = _fma(-mean.float(), scale, b.float())
    v = _fma(x, scale, shift)
    if skip is not None:
        s = skip.float()
        v = v + s
        if skip_res is not None:
            v = _fma(skip_res.float(), _res_scale(s), v)
    if relu:
        v = v.clamp_min(0.0)
    out.update(Y=bf16r(v), V=v, mean=mean.float(), invstd=invstd)
    if training and rmean is not None:
        mom = _momentum(momentum, nbt, torch.float32).to(x.device)
        out["rmean"] = (1.0 - mom) * rmean.float() + mom * mean.float()
        out["rvar"] = (1.0 - mom) * rvar.float() + mom * (var * n / (n - 1.0)).float()
    return out


# ------------------------------------------------------------------------------- backward
def bn_bwd_ref(dY, mask, X, w, mean, invstd, dw0=None, db0=None):
    """float64: g = dY * mask (mask [rows, C] bool or None: no ReLU), x_hat from the given mean /
    invstd [C] -> ({"dX", "dSkip", "dw", "db"}, scales).  dSkip = g exactly; dw / db added into
    the initial values dw0 / db0."""
    x, w = X.double(), w.double()
    mean, invstd = mean.double(), invstd.double()
    g = dY.double() if mask is None else dY.double() * mask.double()
    xh = (x - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    n = x.shape[0]
    dx = invstd * w * (g - dbeta / n - xh * dgamma / n)
    sdx = invstd * w.abs() * (g.abs() + g.abs().mean(0) + xh.abs() * (g * xh).abs().mean(0))
    z = torch.zeros_like(dbeta)
    dw0 = z if dw0 is None else dw0.double()
    db0 = z if db0 is None else db0.double()
    ref = {"dX": dx, "dSkip": g, "dw": dw0 + dgamma, "db": db0 + dbeta}
    sc = {"dX": sdx, "dSkip": g.abs(), "dw": dw0.abs() + (g * xh).abs().sum(0), "db": db0.abs() + g.abs().sum(0)}
    return ref, sc


def bn_bwd_sums_model(dY, mask, X, mean):
    """bn_bwd_reduce_kernel + bn_sum_parts -> (sum g, sum g (x - mean)) per channel, float64"""
    g = dY.float() if mask is None else torch.where(mask, dY.float(), torch.zeros((), device=dY.device))
    return _partials(g, g, X.float() - mean.float(), bn_geometry(*X.shape))


def bn_bwd_model(dY, mask, X, w, mean, invstd, dw0=None, db0=None, sums=None, local=None):
    """bn_bwd_finalize_kernel + bn_bwd_apply_kernel in float32 from the given f32 mean / invstd.
    sums = (s1, s2, n): as bn_fwd_model's; local = (s1, s2): the totals dweight / dbias take (a
    cross-rank pass adds this rank's own, bn_local_sums_kernel; else sums')."""
    x = X.float()
    g = dY.float() if mask is None else torch.where(mask, dY.float(), torch.zeros((), device=dY.device))
    if sums is None:
        sums = bn_bwd_sums_model(dY, mask, X, mean) + (X.shape[0],)
    dbeta, sgx, n = sums
    istd, mu = invstd.float().double(), mean.float().double()
    dgamma = sgx * istd
    a = w.double() * istd
    k2 = -a * istd * dgamma / n
    k0 = (-a * dbeta / n - k2 * mu).float()
    dx = _fma(a.float(), g, _fma(k2.float(), x, k0))
    l1, l2 = (dbeta, sgx) if local is None else local
    z = torch.zeros_like(k0)
    dw0 = z if dw0 is None else dw0.float()
    db0 = z if db0 is None else db0.float()
    return {"dX": bf16r(dx), "dSkip": g, "dw": dw0 + (l2 * istd).float(), "db": db0 + l1.float()}


# ------------------------------------------------------------------------------- checks
# The elementwise bar on Y is not applied to "offset" and "const": there the float32 model itself
# misses it (by up to 3.8 x and 47 x over the sweep).  Y = x scale + shift carries the rounding of
# shift = b - mean scale, |mean| invstd |w| 2^-24, on every element of the channel, which the scale
# |x_hat| |w| + |b| of an element near zero does not: "offset" has |mean| = 8 / invstd, a constant
# channel invstd = eps^-1/2 = 316 against x_hat = 0; and with few rows "offset" loses the variance
# itself to s2 / n - mean^2 (invstd off by up to 4e-5 of itself at 1024 rows of C = 8, the channel
# error 6.8e-3 at 2 rows).  The channel-error and f32 bars, relative to the model on the same
# inputs, hold on every kind, and so does the elementwise bar on dX -- but for "offset" against
# float64 statistics, where the model's invstd error puts it at 1.001 x the bar (33 793 rows of C = 8).
ELEM_Y_KINDS = ("unit", "range", "tail")


def elem_bar(name, kind, stats="own"):
    """is the elementwise bar applied to output `name` (Y / dX) of input kind `kind`; stats: the
    statistics the backward's reference takes ("own": the saved f32 ones, "f64")"""
    if name == "Y":
        return kind in ELEM_Y_KINDS
    return not (kind == "offset" and stats == "f64")


def check_map(name, out, model, ref, scale, fails, log=None, elem=True):
    """both bf16 bars on a [rows, C] map, the row-error bar per channel"""
    return check_bf16(name, out.t(), model.t(), ref.t(), scale.t(), fails, log, elem)


def stream_error(Y, y_res, ref):
    """worst |decoded stream - ref| / max |ref|"""
    m = ref.abs().max().item()
    return (res_decode(Y, y_res, torch.float64) - ref).abs().max().item() / m if m > 0 else 0.0


# the forward arms: name -> (training, relu, mask, skip, skip_res, y_res)
FWD_ARMS = {
    "plain": (True, False, False, False, False, False),
    "relu": (True, True, False, False, False, False),
    "relu+mask": (True, True, True, False, False, False),
    "skip+relu": (True, True, False, True, False, False),
    "skip+relu+mask": (True, True, True, True, False, False),
    "skip": (True, False, False, True, False, False),
    "yres": (True, False, False, False, False, True),
    "stream": (True, True, True, True, True, True),
    "stream-eval": (False, True, False, True, True, True),
    "eval": (False, False, False, False, False, False),
}
# the backward arms: name -> (relu, from the mask, dSkip)
BWD_ARMS = {
    "plain": (False, False, False),
    "plain+dskip": (False, False, True),
    "relu-y": (True, False, False),
    "relu-y+dskip": (True, False, True),
    "relu-mask": (True, True, False),
    "relu-mask+dskip": (True, True, True),
}
