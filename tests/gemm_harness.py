"""Reference, rounding model, launch plan and case lists for the MFMA GEMM and its fused epilogues
(csrc/gemm.hip, mmu_gemm / mmu_gemm_rows of include/mmu.h).  Pure torch (+ numpy for the dropout
hash); the same functions run on the CPU and on the device.  Used by test_gemm_reference.py (CPU),
test_gemm_edges_gpu.py and, for keep_np, test_kernels_gpu.py.

Layouts here are LOGICAL: A [batch, M, K], B [batch, N, K] (bf16 values), every epilogue operand
[batch, M, N] / [batch, N]; the GPU test lays them out K-major or M/N-major with padded leading
dimensions and gapped batch strides.  Epilogue operands travel in a dict `e` with the optional keys
  bias [batch, N] f32          residual [batch, M, N] bf16 (f32 for BIAS_DROP_RES into an f32 C)
  aux_in [batch, M, N] bf16    the DGELU input          c0 [batch, M, N] f32  C before `accumulate`
  cs0 [batch, N] f32           the column sums' initial value (its presence asks for column sums)
  ln = (mean, rstd [batch, M], w, b [batch, N])         the res_ln_* recomputed LayerNorm residual
  bn = (x [M, N] bf16, mask [M, N] bool or None, mean [N] f32)    res_mask [M, N] bool

  gemm_ref      float64 on the same bf16 inputs, every kind 0-8 -> (ref, scale) dicts with "C", "aux"
                (kinds 1, 5), "colsum"; GELU in the erf form.  The column sums are of the UNROUNDED
                epilogue values (epilogue_block adds v[e] before the bf16 store).
  gemm_model32  the same product in float32 in the kernels' order: K in 32-deep steps in k order,
                each step's products summed in float64 and rounded once into the f32 accumulator;
                split-K slabs (kchunk) summed in slice order; the split tail rows (tail = (m_main,
                chunk)) likewise; values rounded to bf16 only where the kernels store bf16.
  table_ref / table_model   the float2 tables of STORE_STATS / *_BNB from the values AS STORED in
                bf16: the table is compared against float64 sums over the kernel's own stored C,
                and C against gemm_ref, separately.
Scales (what each output's rounding error is proportional to):
  base                sum_k |a||b| + |bias| (+ |residual|, + |C0| with accumulate)
  dropout kinds       the product's part x 1/(1-p) on kept elements (0 on dropped ones)
  DGELU               the above x |aux|
  GELU / QuickGELU    the scale of z (their Lipschitz constants are <= 1.13 / 1.1); the QuickGELU
                      derivative aux carries the keep factor once more
  res_ln residual     |r - mean| rstd |w| + |b|
  column sums         sum_m of the scales + |initial value|
  tables              the sum of the absolute contributions
Bars are rowops_harness's: check_bf16 (2^-8 |ref| + 64 * 2^-24 scale on every element, row error
against the model) for bf16 outputs, check_f32 (8 x the model's error or 4 ulps) for f32 ones;
"int" inputs make every partial sum exact in f32 in any order, so an f32 C must equal the reference
bit for bit.

gemm_plan ASKS the host for its choice of tiling, tile order, split-K, split tail and column-sum
path (mmu_gemm_plan: the plan function of csrc/plan.h that mmu_gemm itself runs; it needs the built
library but no GPU).  The plan chooses and labels the cases (test_gemm_reference.py asserts that
every path has cases) and hands gemm_model32 the summation order the f32 bars rest on.
"""
import os

import numpy as np
import torch

from src import kernels

bf16 = torch.bfloat16
(STORE, BIAS_GELU, BIAS_DROP_RES, DGELU, ADD_RES, BIAS_DROP_QGELU, STORE_STATS, STORE_BNB, ADD_RES_BNB) = range(9)
KIND_NAMES = ("STORE", "BIAS_GELU", "BIAS_DROP_RES", "DGELU", "ADD_RES", "BIAS_DROP_QGELU", "STORE_STATS",
              "STORE_BNB", "ADD_RES_BNB")
INPUT_KINDS = ("gauss", "offset", "wide", "int")


def bf16r(x):
    return x.to(bf16).float()


# ------------------------------------------------------------------------------- dropout stream
def keep_np(seed, idx, p):
    """numpy restatement of mmu_keep4 / mmu_keep1 (csrc/mmu_common.h): the keep decision of
    element idx of a dropout stream"""
    M32 = np.uint64(0xFFFFFFFF)

    def lb(x):
        x = x.astype(np.uint64) & M32
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7FEB352D)) & M32
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846CA68B)) & M32
        x ^= x >> np.uint64(16)
        return x
    s32 = lb(np.uint64(seed & 0xFFFFFFFF) ^ lb(np.uint64((seed >> 32) ^ 0x68BC21EB)))
    idx = np.asarray(idx, dtype=np.uint64)
    quad = idx >> np.uint64(2)
    x = (((quad << np.uint64(1)) & M32) ^ (((quad >> np.uint64(31)) * np.uint64(0x9E3779B8)) & M32)) ^ s32
    h0, h1 = lb(x), lb(x ^ np.uint64(1))
    e = idx & np.uint64(3)
    draw = np.where(e == 0, h0 & np.uint64(0xFFFF), np.where(e == 1, h0 >> np.uint64(16),
                    np.where(e == 2, h1 & np.uint64(0xFFFF), h1 >> np.uint64(16))))
    return draw >= np.uint64(int(p * 65536.0 + 0.5))


def keep_bits(seed, M, N, batch, p, row_step=1, row_offset=0):
    """the keep decisions of a [batch, M, N] epilogue -> bool tensor (CPU): element (z, m, n) uses
    counter (row_offset + (z M + m) row_step) N + n, as q_l in epilogue_block does"""
    rows = np.uint64(row_offset) + np.arange(batch * M, dtype=np.uint64) * np.uint64(row_step)
    idx = rows[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
    return torch.from_numpy(keep_np(seed, idx, p)).view(batch, M, N)


# ------------------------------------------------------------------------------- inputs
def gemm_inputs(kind, M, N, K, batch, seed, device="cpu"):
    """-> A [batch, M, K], B [batch, N, K] bf16.  "gauss": A ~ N(0, 1), B ~ 0.1 N(0, 1); "offset":
    A mean 4; "wide": rows of A and of B scaled by 2^-4 .. 2^4 (small outputs beside large ones);
    "int": A in -3..3, B in -2..2 (every partial sum exact in f32)"""
    g = torch.Generator(device=device).manual_seed(seed)
    if kind == "int":
        A = torch.randint(-3, 4, (batch, M, K), generator=g, device=device).float()
        B = torch.randint(-2, 3, (batch, N, K), generator=g, device=device).float()
        return A.to(bf16), B.to(bf16)
    A = torch.randn(batch, M, K, generator=g, device=device)
    B = torch.randn(batch, N, K, generator=g, device=device) * 0.1
    if kind == "offset":
        A = A + 4.0
    elif kind == "wide":
        A = A * torch.exp2(torch.randint(-4, 5, (batch, M, 1), generator=g, device=device).float())
        B = B * torch.exp2(torch.randint(-4, 5, (batch, N, 1), generator=g, device=device).float())
    return A.to(bf16), B.to(bf16)


def epi_inputs(kind, M, N, batch, seed, c_f32=False, ints=False, bias=True, accumulate=False, colsum=False,
               res_ln=False, bn_mask=False, res_mask=False, device="cpu"):
    """the epilogue operands a case of `kind` reads -> dict `e` (module docstring)"""
    g = torch.Generator(device=device).manual_seed(seed + 7919)

    def r(*s):
        if ints:
            return torch.randint(-4, 5, s, generator=g, device=device).float()
        return torch.randn(*s, generator=g, device=device)
    e = {}
    if bias and kind not in (DGELU, ADD_RES, STORE_BNB, ADD_RES_BNB):
        e["bias"] = r(batch, N) * (1.0 if ints else 0.5)
    if kind in (BIAS_DROP_RES, ADD_RES, ADD_RES_BNB):
        res = r(batch, M, N)
        e["residual"] = res if (kind == BIAS_DROP_RES and c_f32) else res.to(bf16)
    if kind == DGELU:
        e["aux_in"] = (torch.rand(batch, M, N, generator=g, device=device) * 1.2 - 0.1).to(bf16)
    if accumulate:
        e["c0"] = r(batch, M, N)
    if colsum:
        e["cs0"] = r(batch, N) * 3.0
    if res_ln:
        x = e["residual"] = r(batch, M, N) * 2.0 + 0.7
        mean = x.mean(-1)
        rstd = torch.rsqrt(x.var(-1, unbiased=False) + 1e-12)
        e["ln"] = (mean, rstd, 1.0 + 0.1 * r(batch, N), 0.1 * r(batch, N))
    if kind in (STORE_BNB, ADD_RES_BNB):
        e["bn"] = (r(M, N).to(bf16), (torch.rand(M, N, generator=g, device=device) < 0.6) if bn_mask else None,
                   r(N) * 0.3)
    if res_mask:
        e["res_mask"] = torch.rand(M, N, generator=g, device=device) < 0.5
    return e


# ------------------------------------------------------------------------------- reference + model
def _gelu(z):
    """erf form: -> (z Phi(z), Phi(z) + z phi(z)); Phi through erfc (no cancellation at negative z)"""
    Phi = 0.5 * torch.erfc(z * -0.7071067811865476)
    pdf = torch.exp(-0.5 * z * z) * 0.3989422804014327
    return z * Phi, Phi + z * pdf


def _gelu_tanh_grad(z):
    """derivative of the tanh-form GELU (a negative control: NOT what the kernels compute)"""
    c, a = 0.7978845608028654, 0.044715
    t = torch.tanh(c * (z + a * z ** 3))
    return 0.5 * (1 + t) + 0.5 * z * (1 - t * t) * c * (1 + 3 * a * z * z)


def _keep_factor(dt, keep, p, like):
    """kz = keep / (1 - p) in dt, the factor in the kernels' own precision"""
    if p <= 0.0 or keep is None:
        return torch.ones((), dtype=dt, device=like.device).expand_as(like)
    zs = 1.0 / (1.0 - p) if dt == torch.float64 else (1.0 / (1.0 - torch.tensor(p, dtype=dt))).item()
    return keep.to(like.device).to(dt) * zs


def _residual(dt, e, kind):
    res = e["residual"].to(dt)
    sres = res.abs()
    if "ln" in e:
        mean, rstd, w, b = (t.to(dt) for t in e["ln"])
        d = (res - mean[..., None]) * rstd[..., None]
        res = d * w[:, None, :] + b[:, None, :]
        sres = d.abs() * w.abs()[:, None, :] + b.abs()[:, None, :]
    if e.get("res_mask") is not None:
        m = e["res_mask"].to(dt)
        res, sres = res * m, sres * m
    return res, sres


def _epilogue(dt, acc, sacc, kind, e, keep, p):
    """acc [batch, M, N] (dt) -> (v = the unrounded final C values, aux or None, scale of v, scale of aux)"""
    v, s = acc, sacc
    if e.get("bias") is not None and kind not in (DGELU, ADD_RES):
        v = v + e["bias"].to(dt)[:, None, :]
        s = s + e["bias"].double().abs()[:, None, :] if s is not None else None
    aux = saux = None
    if kind == BIAS_GELU:
        v, aux = _gelu(v)
        saux = s
    elif kind == BIAS_DROP_RES:
        kz = _keep_factor(dt, keep, p, v)
        res, sres = _residual(dt, e, kind)
        v = res + v * kz
        s = sres.double() + s * kz.double() if s is not None else None
    elif kind == BIAS_DROP_QGELU:
        kz = _keep_factor(dt, keep, p, v)
        u = v * kz
        sg = torch.sigmoid(1.702 * u)
        v = u * sg
        aux = kz * (sg + 1.702 * u * sg * (1 - sg))
        if s is not None:
            s = s * kz.double()
            saux = s * kz.double()
    elif kind == DGELU:
        v = v * e["aux_in"].to(dt)
        s = s * e["aux_in"].double().abs() if s is not None else None
    elif kind in (ADD_RES, ADD_RES_BNB):
        res, sres = _residual(dt, e, kind)
        v = v + res
        s = s + sres.double() if s is not None else None
    if e.get("c0") is not None:
        v = v + e["c0"].to(dt)
        s = s + e["c0"].double().abs() if s is not None else None
    return v, aux, s, saux


def gemm_ref(A, B, kind=STORE, e=None, keep=None, p=0.0):
    """float64 reference -> (ref, scale) dicts: "C", "aux" (kinds 1, 5), "colsum" (with e["cs0"])"""
    e = e or {}
    a, b = A.double(), B.double()
    acc = a @ b.transpose(-1, -2)
    sacc = a.abs() @ b.abs().transpose(-1, -2)
    v, aux, s, saux = _epilogue(torch.float64, acc, sacc, kind, e, keep, p)
    ref, sc = {"C": v}, {"C": s}
    if aux is not None:
        ref["aux"], sc["aux"] = aux, saux
    if e.get("cs0") is not None:
        ref["colsum"] = e["cs0"].double() + v.sum(1)
        sc["colsum"] = e["cs0"].double().abs() + s.sum(1)
    return ref, sc


def _acc32(A, B, kchunk=None, extra=None):
    """the f32 accumulator in the kernels' order: per K slice (kchunk; None = one slice) 32-deep
    steps in k order, each step's products summed in float64 and rounded once into f32; the slices
    summed in slice order.  extra: a k-step (start index) added twice -- a negative control"""
    K = A.shape[-1]
    kchunk = kchunk or K
    total = None
    for kb in range(0, K, kchunk):
        ke = min(kb + kchunk, K)
        acc = torch.zeros(A.shape[:-1] + (B.shape[-2],), dtype=torch.float32, device=A.device)
        for k0 in range(kb, ke, 32):
            k1 = min(k0 + 32, ke)
            step = A[..., k0:k1].double() @ B[..., k0:k1].double().transpose(-1, -2)
            reps = 2 if extra == k0 else 1
            for _ in range(reps):
                acc = (acc.double() + step).float()
        total = acc if total is None else total + acc
    return total


def gemm_model32(A, B, kind=STORE, e=None, keep=None, p=0.0, c_f32=False, kchunk=None, tail=None, extra=None):
    """float32 model -> {"C" (as stored: bf16 values unless c_f32), "C32" (unrounded), "aux", "colsum"}.
    kchunk: the split-K slice depth; tail = (m_main, chunk): rows >= m_main are split-K partial
    products of `chunk`-deep slices (the split tail rows of mmu_gemm)"""
    e = e or {}
    if tail is not None and tail[0] < A.shape[1]:
        m0, ch = tail
        acc = torch.cat([_acc32(A[:, :m0], B, kchunk), _acc32(A[:, m0:], B, ch)], 1)
    else:
        acc = _acc32(A, B, kchunk, extra)
    v, aux, _, _ = _epilogue(torch.float32, acc, None, kind, e, keep, p)
    out = {"C32": v, "C": v if c_f32 else bf16r(v)}
    if aux is not None:
        out["aux"] = bf16r(aux)
    if e.get("cs0") is not None:
        out["colsum"] = e["cs0"].float() + v.sum(1)
    return out


def _block_sums(t):
    """[M, N] -> [ceil(M / 64), N]: sums over 64-row blocks (the last one partly filled)"""
    M, N = t.shape
    P = (M + 63) // 64
    pad = torch.zeros(P * 64, N, dtype=t.dtype, device=t.device)
    pad[:M] = t
    return pad.view(P, 64, N).sum(1)


def _table(dt, Cst, kind, e):
    y = Cst.to(dt)
    if kind == STORE_STATS:
        return torch.stack([_block_sums(y), _block_sums(y * y)], -1), torch.stack([_block_sums(y.abs()),
                                                                                   _block_sums(y * y)], -1)
    x, mask, mean = e["bn"]
    g = y if mask is None else y * mask.to(dt)
    d = x.to(dt) - mean.to(dt)[None, :]
    return torch.stack([_block_sums(g), _block_sums(g * d)], -1), torch.stack([_block_sums(g.abs()),
                                                                               _block_sums((g * d).abs())], -1)


def table_ref(Cst, kind, e):
    """the float2 table [ceil(M / 64), N, 2] of kinds 6-8 from the STORED C [M, N] -> (ref, scale), float64"""
    r, s = _table(torch.float64, Cst, kind, e)
    return r, s.double()


def table_model(Cst, kind, e):
    return _table(torch.float32, Cst, kind, e)[0]


# ------------------------------------------------------------------------------- the host's plan
def gemm_plan(M, N, K, batch, a_kmajor, b_kmajor, kind, c_f32, env=None, lda=None, ldb=None, bias=False,
              colsum=False, ws_floats=kernels.SPLITK_WS_FLOATS):
    """the host's own plan for the product (kernels.gemm_plan: mmu_gemm_plan runs the function
    mmu_gemm runs), queried under the MMU_GEMM_* variables of `env` -> its dict: tiling ("small"
    128^2 | "big" 256^2 | "wide" 256 x 384), tiles_m, tiles_n, group_m, splitk, kchunk, m_main,
    tail_rows, tail_split, tail_chunk, cs ("none" | "atomics" | "rows" | "table"), cs_rows, cs_parts,
    and the label wgs: the workgroups of the main launch.  ws_floats: by default the wrapper's workspace."""
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env or {})
    try:
        pl = kernels.gemm_plan(M, N, K, batch, lda, ldb, a_kmajor, b_kmajor, c_f32, kind, bias, colsum, ws_floats)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    pl["wgs"] = (pl["m_main"] // 256 if pl["tail_rows"] else pl["tiles_m"]) * pl["tiles_n"] * pl["splitk"] * batch
    return pl


# ------------------------------------------------------------------------------- the sweep's cases
WIDE_ENV = {"MMU_GEMM_WIDE": "2", "MMU_GEMM_WIDE_MIN_TILES": "1"}
TAIL_ENV = {"MMU_GEMM_TAIL": "2"}
ATOMICS_ENV = {"MMU_GEMM_CS_PART": "0"}
ENV_KEYS = ("MMU_GEMM_WIDE", "MMU_GEMM_WIDE_MIN_TILES", "MMU_GEMM_TAIL", "MMU_GEMM_CS_PART")
SMALL_M = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 193, 255)
BIG_M = (256, 257, 263, 264, 319, 320, 321, 383, 384, 385, 511, 513)
WIDE_M = (256, 257, 320, 321, 511, 513)
K_KMAJOR = (64, 128, 192, 320)
K_MNMAJOR = (1, 7, 8, 9, 63, 64, 65, 127, 129, 1000)
STAT_M = (1, 63, 64, 65, 257, 321)
ROW_STEPS = ((1, 0), (3, 0), (513, 0), (5, 2), (1, (1 << 24) + 3))
PADS = (8, 16, 24)


def case(path, M, N, K, kind=STORE, c_f32=False, ak=True, bk=True, batch=1, inp="gauss", p=0.0, aux=True,
         colsum=False, accumulate=False, env=None, ws_slices=None, rows=None, bias=True, res_ln=False,
         bn_mask=False, res_mask=False, exact=False):
    """one launch of the sweep.  path: the list it belongs to; ws_slices: a caller-supplied workspace
    of that many slabs (None: the wrapper's); rows = (row_step, row_offset): mmu_gemm_rows;
    exact: "int" inputs into an f32 C, compared bit for bit"""
    c = dict(path=path, M=M, N=N, K=K, kind=kind, c_f32=c_f32, ak=ak, bk=bk, batch=batch, inp=inp, p=p, aux=aux,
             colsum=colsum, accumulate=accumulate, env=dict(env or {}), ws_slices=ws_slices, rows=rows, bias=bias,
             res_ln=res_ln, bn_mask=bn_mask, res_mask=res_mask, exact=exact)
    c["name"] = (f"{path}:{KIND_NAMES[kind]}{'/f32' if c_f32 else ''} M{M} N{N} K{K} b{batch} "
                 f"{'K' if ak else 'M'}{'K' if bk else 'N'} {inp} p{p}{'' if aux else ' noaux'}"
                 f"{' cs' if colsum else ''}{' acc' if accumulate else ''}{' ln' if res_ln else ''}"
                 f"{' bnmask' if bn_mask else ''}{' resmask' if res_mask else ''}"
                 f"{' ws' + str(ws_slices) if ws_slices else ''}{' rows' + str(rows) if rows else ''}"
                 f"{' ' + ','.join(k[9:] + '=' + v for k, v in c['env'].items()) if c['env'] else ''}")
    return c


def pad_of(c):
    """the padding of every bf16 leading dimension of the case (8, 16 or 24 elements; f32: 4)"""
    return PADS[(c["M"] + c["N"] // 128 + c["K"]) % 3]


def plan_of(c):
    """the host's plan for the case, queried under the case's own MMU_GEMM_* variables"""
    ws = kernels.SPLITK_WS_FLOATS if c["ws_slices"] is None else c["ws_slices"] * c["batch"] * c["M"] * c["N"]
    pad = pad_of(c)
    return gemm_plan(c["M"], c["N"], c["K"], c["batch"], c["ak"], c["bk"], c["kind"], c["c_f32"], c["env"],
                     lda=(c["K"] if c["ak"] else c["M"]) + pad, ldb=(c["K"] if c["bk"] else c["N"]) + pad,
                     bias=c["bias"] and c["kind"] not in (DGELU, ADD_RES, STORE_BNB, ADD_RES_BNB),
                     colsum=c["colsum"] or c["kind"] >= STORE_STATS, ws_floats=ws)


# (kind, c_f32, extra keywords): the epilogue variants that rotate through the shape lists
ROT = ((STORE, False, {}), (STORE, True, {}), (BIAS_GELU, False, {}), (BIAS_DROP_RES, False, dict(p=0.1)),
       (BIAS_DROP_RES, True, dict(p=0.1, res_ln=True)), (DGELU, False, {}), (ADD_RES, False, {}),
       (BIAS_DROP_QGELU, False, dict(p=0.1)))
INP3 = ("gauss", "offset", "wide")


def _rot(path, i, M, N, K, **kw):
    kind, f32_, extra = ROT[i % len(ROT)]
    return case(path, M, N, K, kind=kind, c_f32=f32_, inp=INP3[i % 3], **{**extra, **kw})


def cases_small():
    out = []
    for N in (128, 256):
        for i, M in enumerate(SMALL_M):
            out.append(_rot("small-m", i + N // 128, M, N, K_KMAJOR[i % 4], bk=(i % 2 == 0)))
    for i, (M, N) in enumerate(((128, 128), (128, 256), (256, 128))):
        for bk in (True, False):
            out.append(_rot("small-mmajor", 2 * i + bk, M, N, 128, ak=False, bk=bk))
    return out


def cases_big():
    out = []
    for j, N in enumerate((256, 384, 640)):
        for i, M in enumerate(BIG_M):
            out.append(_rot("big-m", i + j, M, N, K_KMAJOR[(i + j) % 4], bk=((i + j) % 2 == 0)))
    i = 0
    for M in (256, 384, 640):        # 384 and 640: half a tile of dead rows fed from NaN padding
        for N in (256, 384, 640):    # 384 and 640 with an N-major B: half a tile of dead columns
            for bk in (True, False):
                out.append(_rot("big-mmajor", i, M, N, 128, ak=False, bk=bk))
                i += 1
    return out


WIDE_ROT = ((STORE, False, {}), (STORE, True, {}), (STORE, True, dict(accumulate=True)), (BIAS_GELU, False, {}),
            (BIAS_DROP_RES, False, dict(p=0.1)), (BIAS_DROP_RES, True, dict(p=0.5)),
            (BIAS_DROP_RES, True, dict(p=0.1, res_ln=True)), (DGELU, False, {}), (ADD_RES, False, {}))


def cases_wide():
    out = []
    for N in (384, 768):
        for i, M in enumerate(WIDE_M):
            for j, (kind, f32_, extra) in enumerate(WIDE_ROT):
                out.append(case("wide", M, N, K_KMAJOR[(i + j) % 4], kind=kind, c_f32=f32_, inp=INP3[(i + j) % 3],
                                env=WIDE_ENV, **extra))
    return out


def cases_k():
    out = []
    for (M, N) in ((65, 128), (257, 256)):          # 1, 2, 3, 5 k-steps: both stage parities
        for K in K_KMAJOR:
            out.append(case("k-kmajor", M, N, K, c_f32=True, inp="gauss"))
            out.append(case("k-kmajor", M, N, K, c_f32=True, inp="int", exact=True, bias=False))
    for (M, N) in ((128, 128), (256, 256)):         # both operands M/N-major: any K
        for i, K in enumerate(K_MNMAJOR):
            out.append(case("k-mnmajor", M, N, K, c_f32=True, ak=False, bk=False, inp="int", exact=True, bias=False))
            out.append(case("k-mnmajor", M, N, K, c_f32=(i % 2 == 0), ak=False, bk=False, inp=INP3[i % 3]))
    return out


def cases_order():
    """tile order and XCD remap: "int" inputs, f32 C, bitwise; K = 64"""
    kw = dict(c_f32=True, inp="int", exact=True, bias=False)
    out = []
    for t in range(1, 9):                            # workgroup counts 1..8: every remainder mod 8
        out.append(case("order-rem", 128 * t - 5, 128, 64, **kw))
        out.append(case("order-rem", 256 * t - 3, 256, 64, bk=False, **kw))
    for t in (9, 11, 13, 15, 17, 19, 21, 23):        # and every remainder with more than one round of XCDs
        out.append(case("order-rem", 128 * t - 5, 128, 64, **kw))
    # tiles_m no multiple of group_m, tiles_n >= 4: group_m 2 (N-major B) and 8 (K-major B)
    out.append(case("order-group", 700, 1024, 64, bk=False, **kw))      # big: 3 x 4 tiles, groups of 2
    out.append(case("order-group", 2600, 1024, 64, bk=True, **kw))      # big: 11 x 4 tiles, groups of 8
    out.append(case("order-group", 1300, 1280, 64, bk=False, **kw))     # big: 6 x 5, N-major: a last group of 2
    out.append(case("order-group", 100, 512, 64, bk=False, **kw))       # small: 1 x 4, groups of 2
    out.append(case("order-group", 130, 512, 64, bk=True, **kw))        # small: 2 x 4, groups of 8
    for batch in (2, 3):
        out.append(case("order-batch", 300, 1024, 64, batch=batch, bk=True, **kw))
        out.append(case("order-batch", 129, 512, 64, batch=batch, bk=False, **kw))
        out.append(case("order-batch", 256, 256, 1024, batch=batch, **kw))           # split-K x batch
        out.append(case("order-batch", 128, 128, 1024, batch=batch, ak=False, bk=False, **kw))
    return out


def cases_splitk():
    """STORE, f32 C, workspace: "int" inputs, bitwise"""
    out = []
    shapes = ((128, 128), (256, 256), (512, 512))    # one small tile, one big tile, 2 x 2 big tiles
    for (M, N) in shapes:
        for i, K in enumerate((1024, 1088, 2048, 4160)):
            for batch in (1, 2):
                out.append(case("splitk", M, N, K, c_f32=True, inp="int", exact=True, bias=False, batch=batch,
                                accumulate=((i + batch) % 2 == 0)))
        for i, K in enumerate((1100, 2056)):         # a short last slice that ends inside a 64-step
            for batch in (1, 2):
                out.append(case("splitk", M, N, K, c_f32=True, inp="int", exact=True, bias=False, batch=batch,
                                ak=False, bk=False, accumulate=((i + batch) % 2 == 1)))
    for (M, N) in shapes[:2]:
        for acc in (False, True):
            out.append(case("splitk-cap3", M, N, 1024, c_f32=True, inp="int", exact=True, bias=False, ws_slices=3,
                            accumulate=acc))
            out.append(case("splitk-cap1", M, N, 1024, c_f32=True, inp="int", exact=True, bias=False, ws_slices=1,
                            accumulate=acc))
    out.append(case("splitk-gauss", 256, 256, 2048, c_f32=True, inp="gauss", bias=False))
    out.append(case("splitk-gauss", 128, 128, 1100, c_f32=True, inp="offset", bias=False, ak=False, bk=False))
    return out


TAIL_VARIANTS = ((STORE, False, {}), (STORE, True, {}), (BIAS_GELU, False, {}), (BIAS_DROP_RES, False, dict(p=0.1)),
                 (BIAS_DROP_RES, True, dict(p=0.1, res_ln=True)), (DGELU, False, dict(colsum=True)),
                 (ADD_RES, False, {}))


def cases_tail():
    """the split tail rows: N = 256 on the 256^2 tiling (MMU_GEMM_TAIL=2) and N = 384 on the wide
    one (its default), K = 512, M = 256 * 256 + {1, 129, 256}: the only large cases"""
    out = []
    for N, env in ((256, TAIL_ENV), (384, WIDE_ENV)):
        for i, extra_rows in enumerate((1, 129, 256)):
            for j, (kind, f32_, extra) in enumerate(TAIL_VARIANTS):
                out.append(case("tail", 256 * 256 + extra_rows, N, 512, kind=kind, c_f32=f32_,
                                inp=("gauss", "wide")[(i + j) % 2], env=env, **extra))
    return out


EPI_VARIANTS = ((STORE, False, {}), (STORE, True, {}), (STORE, True, dict(accumulate=True)),
                (BIAS_GELU, False, {}), (BIAS_GELU, False, dict(aux=False)),
                (BIAS_DROP_RES, False, dict(p=0.0)), (BIAS_DROP_RES, False, dict(p=0.1)),
                (BIAS_DROP_RES, False, dict(p=0.5)), (BIAS_DROP_RES, True, dict(p=0.5)),
                (BIAS_DROP_RES, True, dict(p=0.1, res_ln=True)), (BIAS_DROP_RES, True, dict(p=0.0, res_ln=True)),
                (DGELU, False, {}), (ADD_RES, False, {}),
                (BIAS_DROP_QGELU, False, dict(p=0.0)), (BIAS_DROP_QGELU, False, dict(p=0.5)),
                (BIAS_DROP_QGELU, False, dict(p=0.1, aux=False)))
LAYOUTS = ((True, True), (True, False), (False, False), (False, True))


def cases_epilogues(tiling):
    """every kind 0-5 in all four layouts, batch 2 with every batch stride non-trivial"""
    out = []
    for (ak, bk) in LAYOUTS:
        if tiling == "small":
            M, N, K = (193 if ak else 128), 128, 64
        else:
            M, N, K = (321 if ak else 384), 384, 128
        for j, (kind, f32_, extra) in enumerate(EPI_VARIANTS):
            out.append(case(f"epi-{tiling}", M, N, K, kind=kind, c_f32=f32_, ak=ak, bk=bk, batch=2,
                            inp=INP3[j % 3], **extra))
    return out


def cases_tables():
    """kinds 6-8 in their single allowed layout, with and without the masks"""
    out = []
    for i, M in enumerate(STAT_M):
        N = 128 if M < 256 else 256
        out.append(case("table", M, N, 128, kind=STORE_STATS, inp=INP3[i % 3], bias=(i % 2 == 0)))
        for bm in (False, True):
            out.append(case("table", M, N, 128, kind=STORE_BNB, bk=False, inp=INP3[(i + bm) % 3], bn_mask=bm))
            out.append(case("table", M, N, 128, kind=ADD_RES_BNB, bk=False, inp=INP3[(i + bm + 1) % 3], bn_mask=bm,
                            res_mask=not bm))
    out.append(case("table", 321, 256, 128, kind=ADD_RES, bk=False, res_mask=True))
    out.append(case("table", 65, 128, 128, kind=ADD_RES, bk=True, res_mask=True))
    return out


CS_KINDS = ((STORE, {}), (DGELU, {}), (ADD_RES, {}), (BIAS_GELU, {}), (BIAS_DROP_RES, dict(p=0.1)),
            (BIAS_DROP_QGELU, dict(p=0.1)))


def cases_colsum():
    """column sums from a non-zero initial value: partial rows and atomics, batch 1 and 2, the M and
    N lists of the two tilings and the dead-row / dead-column shapes"""
    out = []
    i = 0

    def add(M, N, K, **kw):
        nonlocal i
        kind, extra = CS_KINDS[i % len(CS_KINDS)]
        for env in ({}, ATOMICS_ENV):
            out.append(case("colsum", M, N, K, kind=kind, colsum=True, inp=INP3[i % 3], env=env, **{**extra, **kw}))
        i += 1
    for M in SMALL_M:
        add(M, 128, 64, bk=(i % 2 == 0))
    for M in BIG_M:
        add(M, 256, 64, bk=(i % 2 == 0))
    for N in (384, 640):
        add(257, N, 64, bk=False)
        add(384, N, 128, ak=False, bk=False)
        add(640, N, 64, ak=False, bk=True)
    for (M, N, ak) in ((65, 128, True), (129, 256, True), (321, 256, True), (384, 384, False)):
        kind, extra = CS_KINDS[i % len(CS_KINDS)]
        out.append(case("colsum-batch", M, N, 64, kind=kind, colsum=True, batch=2, ak=ak, bk=(i % 2 == 0),
                        inp=INP3[i % 3], **extra))
        i += 1
    for M in WIDE_M[1::2]:
        out.append(case("colsum-wide", M, 384, 64, kind=DGELU, colsum=True, env=WIDE_ENV))
        out.append(case("colsum-wide", M, 768, 64, kind=ADD_RES, colsum=True, env={**WIDE_ENV, **ATOMICS_ENV}))
    return out


def cases_rows():
    """mmu_gemm_rows: the row-stepped dropout counter; the last pair at N = 768 puts the counter
    above 2^33 (the high-word mix of mmu_keep4)"""
    out = []
    for (step, off) in ROW_STEPS:
        N = 768 if off > 1000 else 128
        out.append(case("rows", 65, N, 64, kind=BIAS_DROP_RES, p=0.1, rows=(step, off)))
        out.append(case("rows", 65, N, 64, kind=BIAS_DROP_QGELU, p=0.5, rows=(step, off), batch=2))
        out.append(case("rows", 257, 256 if N == 128 else N, 64, kind=BIAS_DROP_RES, c_f32=True, p=0.5,
                        rows=(step, off), bk=False))
    return out


# test id -> cases: one parametrized GPU test per group, each a few seconds
GROUPS = {
    "small": cases_small, "big": cases_big, "wide-384": lambda: [c for c in cases_wide() if c["N"] == 384],
    "wide-768": lambda: [c for c in cases_wide() if c["N"] == 768], "k": cases_k, "order": cases_order,
    "splitk": cases_splitk, "epi-small": lambda: cases_epilogues("small"), "epi-big": lambda: cases_epilogues("big"),
    "tables": cases_tables, "colsum": cases_colsum, "rows": cases_rows,
}
for _n in (256, 384):
    for _r in (1, 129, 256):
        GROUPS[f"tail-{_n}-{_r}"] = (lambda n=_n, r=_r: [c for c in cases_tail() if c["N"] == n
                                                         and c["M"] == 256 * 256 + r])


def all_cases():
    return [c for f in GROUPS.values() for c in f()]


# Cases of the lists above that the host cannot serve as meant: (case name, reason).  At most 5 % of
# the sweep; test_gemm_reference.py asserts the cap and that each is indeed not served as meant.
UNREACHABLE = ()

# Cases where the float32 model itself misses a bar: (case name fragment, output, the model's figure)
MODEL_MISSES = ()


def meant(c, pl):
    """does the plan serve the case as its list means it? -> None, or what is wrong"""
    path = c["path"]
    if (path.startswith("small") or path == "epi-small") and pl["tiling"] != "small":
        return "not the small tiling"
    if (path.startswith("big") or path == "epi-big") and pl["tiling"] != "big":
        return "not the 256^2 tiling"
    if path in ("wide", "colsum-wide") and pl["tiling"] != "wide":
        return "not the wide tiling"
    if path == "tail" and not pl["tail_rows"]:
        return "no split tail"
    if path == "tail" and pl["tiling"] != ("wide" if c["N"] == 384 else "big"):
        return "tail on the wrong tiling"
    if path == "splitk" and pl["splitk"] < 2:
        return "no split-K"
    if path == "splitk-cap3" and pl["splitk"] != 3:
        return "not capped at 3 slices"
    if path == "splitk-cap1" and pl["splitk"] != 1:
        return "split although capped at 1"
    if path == "colsum" and pl["cs"] != ("atomics" if c["env"].get("MMU_GEMM_CS_PART") == "0" else "rows"):
        return "wrong column-sum path"
    if path == "colsum-batch" and pl["cs"] != "atomics":
        return "batched column sums not by atomics"
    if path == "table" and c["kind"] >= STORE_STATS and pl["cs"] != "table":
        return "no table"
    return None


# ------------------------------------------------------------------------------- checks
def check_outputs(tag, out, model, ref, sc, c_f32, fails, log=None, worst=None):
    """every output of one case against its bars (rowops_harness): "C" and "aux" [batch, M, N],
    "colsum" [batch, N], "table" [P, N, 2] when present in `out`.  bf16 outputs: check_bf16; f32
    outputs (an f32 C, the column sums, the tables): check_f32, the sums and tables with each
    element's own scale"""
    import rowops_harness as R
    for key in ("C", "aux"):
        if key not in out:
            continue
        if key == "C" and c_f32:
            r = R.check_f32(f"{tag} C(f32)", out[key], model[key], ref[key], sc[key], fails, log)
            if worst is not None:
                worst.f32("C f32", *r)
        else:
            el, st = R.check_bf16(f"{tag} {key}", out[key], model[key], ref[key], sc[key], fails, log)
            if worst is not None:
                worst.bf(f"{key} bf16", el, st)
    for key in ("colsum", "table"):
        if key in out:
            r = R.check_f32(f"{tag} {key}", out[key].reshape(-1), model[key].reshape(-1), ref[key].reshape(-1),
                            sc[key].reshape(-1), fails, log)
            if worst is not None:
                worst.f32(key, *r)
