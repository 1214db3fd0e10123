"""torch-tensor front-end of the HIP kernels (pointers + current HIP stream).

Every function enqueues on ``torch.cuda.current_stream()`` of the tensors'
device and raises if a tensor is not on a HIP device or has the wrong
dtype/layout -- there is no CPU fallback ("no fallback").
"""
import ctypes
import weakref

import torch

from . import _native as N
from ._native import (Epilogue, EPI_STORE, EPI_BIAS_GELU, EPI_BIAS_DROP_RES, EPI_DGELU, EPI_ADD_RES,  # noqa: F401
                      EPI_BIAS_DROP_QGELU, EPI_STORE_STATS, EPI_STORE_BNB, EPI_ADD_RES_BNB)


def bn_stats_table(rows, C, device):
    """the float2 [ceil(rows / 64)][C] BatchNorm statistics table a conv's STORE_STATS epilogue
    writes (include/mmu.h MMU_EPI_STORE_STATS) -> (table, nparts)"""
    nparts = (rows + 63) // 64
    return torch.empty(nparts * C * 2, dtype=torch.float32, device=device), nparts


def set_deterministic(on):
    """Deterministic mode of the library (mmu_set_deterministic): with it on, no kernel sums through
    float atomics, so equal inputs give equal bits.  Host state read when a launch is chosen; a
    captured graph keeps the mode it was captured under.  -> the previous value"""
    return bool(N.load().mmu_set_deterministic(int(bool(on))))


def is_deterministic():
    return bool(N.load().mmu_get_deterministic())


class deterministic:
    """``with kernels.deterministic():`` turns the mode on (or off: ``deterministic(False)``) and
    restores the previous value on exit, after an exception too"""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        self.prev = set_deterministic(self.on)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


def embed_bwd_det_chunk():
    """tokens per wave of the deterministic embedding backward's segmented sum"""
    return int(N.load().mmu_embed_bwd_det_chunk())


def _dev_check(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise N.NativeError("mmu kernels need tensors on a HIP (cuda) device; got CPU tensor "
                                f"{tuple(t.shape)} {t.dtype}")


_raw_stream = torch._C._cuda_getCurrentRawStream  # (device index) -> the current hipStream_t as an int


def _stream(t):
    # the raw handle, without building a torch.cuda.Stream object: this runs once per kernel
    # launch, ~800 times per training step
    return _raw_stream(t.get_device())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _want(t, dtype, name):
    if t.dtype != dtype:
        raise N.NativeError(f"{name}: expected {dtype}, got {t.dtype}")


def epilogue(kind=EPI_STORE, bias=None, residual=None, aux=None, colsum=None, drop_p=0.0, seed=0, accumulate=False,
             ldr=0, ldx=0, bias_bstride=0, res_bstride=0, aux_bstride=0, colsum_bstride=0, res_ln=None,
             res_ln_bstride=0, bn=None, res_mask=None):
    """res_ln = (mean, rstd, w, b): with BIAS_DROP_RES into an f32 C, the residual is the LayerNorm
    output recomputed from the f32 ``residual`` rows (the previous LayerNorm's input).
    bn = (x, relu_mask or None, mean): with STORE_BNB / ADD_RES_BNB, the BatchNorm whose dY the
    product forms; colsum is then its backward reduction table (bn_stats_table of x's rows).
    res_mask (ADD_RES / ADD_RES_BNB): a ReLU mask [M*N/8] u8 gating the residual per element."""
    e = Epilogue()
    e.kind, e.accumulate = kind, int(accumulate)
    e.bias, e.bias_bstride = _ptr(bias), bias_bstride
    e.residual, e.ldr, e.res_bstride = _ptr(residual), ldr or (residual.shape[-1] if residual is not None else 0), \
        res_bstride
    e.aux, e.ldx, e.aux_bstride = _ptr(aux), ldx or (aux.shape[-1] if aux is not None else 0), aux_bstride
    e.colsum, e.colsum_bstride = _ptr(colsum), colsum_bstride
    e.drop_p, e.seed = float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF
    e.workspace, e.workspace_floats = None, 0
    if res_ln is not None:
        for t in res_ln:
            _want(t, torch.float32, "epilogue res_ln")
            if not t.is_contiguous():
                raise N.NativeError("epilogue res_ln tensors must be contiguous")
        e.res_ln_mean, e.res_ln_rstd, e.res_ln_w, e.res_ln_b = (_ptr(t) for t in res_ln)
        e.res_ln_bstride = res_ln_bstride
    if bn is not None:
        _bnb_check(*bn, "epilogue bn")
        e.bn_x, e.bn_mask, e.bn_mean = (_ptr(t) for t in bn)
    if res_mask is not None:
        if res_mask.dtype != torch.uint8 or not res_mask.is_contiguous() or residual is None \
                or res_mask.numel() * 8 != residual.numel():
            raise N.NativeError("epilogue res_mask: contiguous uint8 with numel = residual.numel() / 8")
        e.res_mask = _ptr(res_mask)
    # the tensors behind the pointers, for gemm's extent checks (a ctypes structure holds no references)
    e.tensors = dict(bias=bias, residual=residual, aux=aux, colsum=colsum, res_ln=res_ln, bn=bn, res_mask=res_mask)
    return e


def _room(t):
    """bytes from the tensor's data pointer to the end of its storage"""
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def _fits(name, t, batch, stride, rows, ld, width):
    """refuse a call whose last element, (batch - 1) stride + (rows - 1) ld + width elements from
    the tensor's data pointer, lies outside the tensor's storage"""
    if t is None:
        return
    if stride < 0 or ld < 0:
        raise N.NativeError(f"gemm {name}: negative stride or leading dimension")
    need = ((batch - 1) * stride + (rows - 1) * ld + width) * t.element_size()
    if need > _room(t):
        raise N.NativeError(f"gemm {name}: the call reaches {need} bytes from the tensor's pointer, its storage "
                            f"ends after {_room(t)} (batch {batch} stride {stride}, {rows} rows of pitch {ld}, "
                            f"width {width})")


_RES_KINDS = (EPI_BIAS_DROP_RES, EPI_ADD_RES, EPI_ADD_RES_BNB)
_AUX_KINDS = (EPI_BIAS_GELU, EPI_DGELU, EPI_BIAS_DROP_QGELU)
_TABLE_KINDS = (EPI_STORE_STATS, EPI_STORE_BNB, EPI_ADD_RES_BNB)


def _gemm_extents(A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, M, N_, K, epi, batch, sA, sB, sC):
    """plain integer checks of everything mmu_gemm will address (include/mmu.h) against the
    tensors' storages; they need no device, so they run before the device check"""
    if min(M, N_, K, batch) <= 0:
        raise N.NativeError(f"gemm: bad shape M={M} N={N_} K={K} batch={batch}")
    _fits("A", A, batch, sA, M if a_kmajor else K, lda, K if a_kmajor else M)
    _fits("B", B, batch, sB, N_ if b_kmajor else K, ldb, K if b_kmajor else N_)
    _fits("C", C, batch, sC, M, ldc, N_)
    t = getattr(epi, "tensors", None)
    if t is None:
        return
    kind = epi.kind
    # (the extents are counted in the tensors' own element sizes: what the kernels read must be that type)
    for name, dt in (("bias", torch.float32), ("colsum", torch.float32), ("aux", torch.bfloat16)):
        if t[name] is not None:
            _want(t[name], dt, f"gemm {name}")
    if kind not in (EPI_DGELU, EPI_ADD_RES):
        _fits("bias", t["bias"], batch, epi.bias_bstride, 1, 0, N_)
    if kind in _RES_KINDS and t["residual"] is not None:
        r32 = kind == EPI_BIAS_DROP_RES and C.dtype == torch.float32  # the f32 hidden stream
        _want(t["residual"], torch.float32 if r32 else torch.bfloat16, "gemm residual")
        _fits("residual", t["residual"], batch, epi.res_bstride, M, epi.ldr, N_)
    if kind in _AUX_KINDS:
        _fits("aux", t["aux"], batch, epi.aux_bstride, M, epi.ldx, N_)
    if kind in _TABLE_KINDS:
        _fits("colsum (table)", t["colsum"], 1, 0, (M + 63) // 64, 2 * N_, 2 * N_)
    else:
        _fits("colsum", t["colsum"], batch, epi.colsum_bstride, 1, 0, N_)
    if t["res_ln"] is not None:
        mean, rstd, w, b = t["res_ln"]
        _fits("res_ln mean", mean, 1, 0, 1, 0, batch * M)
        _fits("res_ln rstd", rstd, 1, 0, 1, 0, batch * M)
        _fits("res_ln w", w, batch, epi.res_ln_bstride, 1, 0, N_)
        _fits("res_ln b", b, batch, epi.res_ln_bstride, 1, 0, N_)
    if t["bn"] is not None:
        x, mask, mean = t["bn"]
        _fits("bn x", x, 1, 0, M, N_, N_)
        _fits("bn mask", mask, 1, 0, M, N_ // 8, N_ // 8)
        _fits("bn mean", mean, 1, 0, 1, 0, N_)
    if t["res_mask"] is not None:
        _fits("res_mask", t["res_mask"], 1, 0, M, N_ // 8, N_ // 8)


def _bnb_check(x, mask, mean, what):
    if (x.dtype != torch.bfloat16 or mean.dtype != torch.float32 or not mean.is_contiguous()
            or mean.numel() != x.shape[1] or not x.is_contiguous(memory_format=torch.channels_last)):
        raise N.NativeError(f"{what}: (x channels-last bf16, relu_mask, mean f32 [C]) of a training BatchNorm")
    _bn_mask_check(mask, x, what)


SPLITK_WS_FLOATS = 16 << 20  # 64 MiB per (device, stream), reused stream-ordered by every split-K product
_ws = {}
_side = {}


def _splitk_workspace(dev):
    key = (dev, _raw_stream(dev.index if dev.index is not None else torch.cuda.current_device()))
    t = _ws.get(key)
    if t is None:
        t = _ws[key] = torch.empty(SPLITK_WS_FLOATS, dtype=torch.float32, device=dev)
    return t


# ---- launch plans: what the host would choose, asked of the library itself (no launch, no GPU needed)
def _plan(name, *args):
    out = (ctypes.c_int64 * len(N.PLAN_FIELDS[name]))()
    N.call(name, *args, out)
    return dict(zip(N.PLAN_FIELDS[name], out))


def gemm_plan(M, N_, K, batch=1, lda=None, ldb=None, a_kmajor=True, b_kmajor=True, c_f32=False, kind=EPI_STORE,
              bias=False, colsum=False, ws_floats=SPLITK_WS_FLOATS):
    """mmu_gemm_plan (include/mmu.h) -> dict of its fields, "tiling" and "cs" by name: the plan of
    gemm() for this shape under the MMU_GEMM_* environment and the deterministic switch as they
    stand.  lda / ldb default to dense operands; ws_floats to the workspace gemm() passes."""
    d = _plan("mmu_gemm_plan", M, N_, K, batch, lda or (K if a_kmajor else M), ldb or (K if b_kmajor else N_),
              int(a_kmajor), int(b_kmajor), N.MMU_F32 if c_f32 else N.MMU_BF16, kind, int(bool(bias)),
              int(bool(colsum)), ws_floats)
    d["tiling"], d["cs"] = N.GEMM_TILINGS[d["tiling"]], N.GEMM_COLSUMS[d["cs"]]
    return d


def conv_plan(n, H, W, C, N_, ksize=3, stride=1, ws_floats=SPLITK_WS_FLOATS):
    """mmu_conv_implicit_plan -> dict: the plan of conv_implicit() / conv3x3_implicit()"""
    return _plan("mmu_conv_implicit_plan", n, H, W, C, N_, ksize, stride, ws_floats)


def conv_wgrad_plan(n, H, W, Cin, Cout, ksize=3, stride=1, ws_floats=SPLITK_WS_FLOATS):
    """mmu_conv_wgrad_plan -> dict: the plan of conv_wgrad() / conv3x3_wgrad()"""
    return _plan("mmu_conv_wgrad_plan", n, H, W, Cin, Cout, ksize, stride, ws_floats)


def batchnorm_plan(rows, C):
    """mmu_batchnorm_plan -> dict: the row-block grid of the batchnorm_* passes over a [rows, C] map"""
    return _plan("mmu_batchnorm_plan", rows, C)


SIDE_CU_FRAC = None  # e.g. 0.75: the side stream's kernels run on that fraction of every XCD's CUs


def _cu_masked_stream(dev, frac):
    """A stream whose dispatches are restricted to ``frac`` of the CUs (hipExtStreamCreateWithCUMask),
    so the side stream's weight-gradient GEMMs leave the rest to the main stream's chain.  The
    mask keeps whole 8-CU groups, 3 of every 4 for 0.75: balanced across the 8 XCDs whether the
    runtime numbers CUs XCD-blocked or XCD-interleaved."""
    import ctypes
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    groups = n_cu // 8
    keep = max(1, min(groups, round(frac * groups)))
    # spread the kept groups evenly over the group index (Bresenham)
    bits = [0] * ((n_cu + 31) // 32)
    for g in range(groups):
        if (g + 1) * keep // groups != g * keep // groups:
            for c in range(8 * g, 8 * g + 8):
                bits[c // 32] |= 1 << (c % 32)
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime torch already loaded (same soname)
    h = ctypes.c_void_p()
    arr = (ctypes.c_uint32 * len(bits))(*bits)
    with torch.cuda.device(dev):
        err = hip.hipExtStreamCreateWithCUMask(ctypes.byref(h), ctypes.c_uint32(len(bits)), arr)
    if err != 0:
        raise N.NativeError(f"hipExtStreamCreateWithCUMask failed ({err})")
    return torch.cuda.ExternalStream(h.value, device=dev)


def side_stream(dev):
    """The per-device stream the weight-gradient products run on, beside the data-gradient
    chain of the backward (src/encoder.py)."""
    dev = torch.device(dev)
    s = _side.get(dev)
    if s is None:
        s = _side[dev] = (_cu_masked_stream(dev, SIDE_CU_FRAC) if SIDE_CU_FRAC
                          else torch.cuda.Stream(device=dev))
    return s


_side_pump = None


def set_side_pump(fn):
    """src/encoder.py's pump_deferred: issues the side-stream work it has flushed"""
    global _side_pump
    _side_pump = fn


def side_pump(dev):
    """issue the encoder's flushed weight-gradient work (the trunk's BatchNorm backwards call this)"""
    if _side_pump is not None:
        _side_pump(dev)


def side_stream_if_any(dev):
    """the device's side stream if one was created, else None"""
    return _side.get(torch.device(dev))


_pending_join = set()


def join_at_backward_end(main, side):
    """Once per backward pass: ``main`` waits for ``side`` when the autograd engine finishes,
    so every consumer of .grad (optimizer, all-reduce, tests) sees the side stream's work."""
    key = (main.cuda_stream, side.cuda_stream)
    if key in _pending_join:
        return
    _pending_join.add(key)

    def join():
        _pending_join.discard(key)
        main.wait_stream(side)

    torch.autograd.Variable._execution_engine.queue_callback(join)


def gemm(A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, M, N_, K, epi=None, batch=1, sA=0, sB=0, sC=0, row_step=None,
         row_offset=0):
    """C[m,n] = sum_k A(m,k) B(n,k) (+ fused epilogue); see mmu_gemm in include/mmu.h.
    row_step (not None: mmu_gemm_rows) / row_offset: the epilogue's dropout decisions of row m are
    those of row row_offset + m * row_step of a dense product.
    A call that would address anything outside a tensor's storage is refused (_gemm_extents)."""
    _want(A, torch.bfloat16, "gemm A")
    _want(B, torch.bfloat16, "gemm B")
    cdt = N.MMU_F32 if C.dtype == torch.float32 else N.MMU_BF16
    if C.dtype not in (torch.float32, torch.bfloat16):
        raise N.NativeError("gemm C must be f32 or bf16")
    if epi is None:
        epi = epilogue(EPI_STORE)
    _gemm_extents(A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, M, N_, K, epi, batch, sA, sB, sC)
    _dev_check(A, B, C)
    # the per-stream f32 scratch serves the split-K weight gradients
    if not epi.workspace:  # (on a copy: a caller's epilogue may be reused on another stream)
        epi = type(epi).from_buffer_copy(epi)
        ws = _splitk_workspace(C.device)
        epi.workspace, epi.workspace_floats = ws.data_ptr(), ws.numel()
    if row_step is not None:
        N.call("mmu_gemm_rows", _ptr(A), lda, int(a_kmajor), _ptr(B), ldb, int(b_kmajor), _ptr(C), ldc, cdt, M, N_, K,
               batch, sA, sB, sC, ctypes.byref(epi), int(row_step), int(row_offset), _stream(C))
    else:
        N.call("mmu_gemm", _ptr(A), lda, int(a_kmajor), _ptr(B), ldb, int(b_kmajor), _ptr(C), ldc, cdt, M, N_, K,
               batch, sA, sB, sC, ctypes.byref(epi) if epi is not None else None, _stream(C))
    if _alg["on"]:
        _count_alg(M, N_, K, batch, 4 if cdt == N.MMU_F32 else 2, epi)
    return C


def colsum_reduce_multi(jobs, accumulate=False):
    """[(partial [parts_z, N], out [N]), ...] (1..4 jobs of one width N): one launch
    (mmu_colsum_reduce_multi)"""
    n = len(jobs)
    N_ = jobs[0][0].shape[1]
    for part, out in jobs:
        _dev_check(part, out)
        if part.dtype != torch.float32 or out.dtype != torch.float32 or part.shape[1] != N_ or out.numel() != N_ \
                or not part.is_contiguous() or not out.is_contiguous():
            raise N.NativeError("colsum_reduce_multi: f32 contiguous [parts, N] partials / [N] outputs of one N")
    parts_p = (ctypes.c_void_p * n)(*[p.data_ptr() for p, _ in jobs])
    rows = (ctypes.c_int64 * n)(*[p.shape[0] for p, _ in jobs])
    outs = (ctypes.c_void_p * n)(*[o.data_ptr() for _, o in jobs])
    N.call("mmu_colsum_reduce_multi", n, ctypes.cast(parts_p, ctypes.c_void_p), ctypes.cast(rows, ctypes.c_void_p),
           ctypes.cast(outs, ctypes.c_void_p), N_, int(accumulate), _stream(jobs[0][1]))


def colsum_reduce(partial, out, accumulate=False):
    _dev_check(partial, out)
    N.call("mmu_colsum_reduce", _ptr(partial), partial.shape[0], partial.shape[1], _ptr(out), int(accumulate),
           _stream(out))


def transpose_bf16_batched(jobs, n_jobs, max_rows, max_cols, stream_of):
    """dst = src^T for every (src ptr, dst ptr, rows, cols, src pitch, dst pitch) row of the
    int64 device table ``jobs`` [n_jobs, 6] (pitch 0: dense); see mmu_transpose_bf16_batched.
    ``stream_of``: a tensor on the target device (its current stream is used)."""
    _dev_check(jobs, stream_of)
    if jobs.dtype != torch.int64 or not jobs.is_contiguous() or jobs.numel() < 6 * n_jobs:
        raise N.NativeError("transpose_bf16_batched: jobs must be a contiguous int64 [n_jobs, 6] device table")
    N.call("mmu_transpose_bf16_batched", _ptr(jobs), int(n_jobs), int(max_rows), int(max_cols), _stream(stream_of))


def colsum_bf16(X, out, accumulate=False):
    _dev_check(X, out)
    M, N_ = X.shape
    # scratch for the per-block partial rows (>= ceil(M / 64) x N f32, see mmu_colsum_bf16)
    part = torch.empty(((M + 63) // 64) * N_, dtype=torch.float32, device=X.device)
    N.call("mmu_colsum_bf16", _ptr(X), M, N_, X.stride(0), _ptr(part), _ptr(out), int(accumulate), _stream(X))


def dropmask_empty(batch, L, heads=12, device=None):
    """Keep-bit buffer of the attention-probs dropout: [batch*heads, L, ceil(L/64)] words
    (int64 storage of the kernel's u64; bit k of word j = key 64j+k kept)."""
    return torch.empty(batch * heads, L, (L + 63) // 64, dtype=torch.int64, device=device)


def dropmask_dense(mask, L):
    """[BH, L, W] keep words -> [BH, L, L] float 0/1 (test/debug helper)."""
    bits = torch.arange(64, device=mask.device, dtype=torch.int64)
    d = (mask.unsqueeze(-1) >> bits) & 1
    return d.flatten(-2)[..., :L].float()


def attention_fwd(qkv, keymask, O, lse, batch, L, heads=12, drop_p=0.0, seed=0, dropmask=None):
    _dev_check(qkv, keymask, O, lse)
    _want(qkv, torch.bfloat16, "attention qkv")
    if dropmask is not None:
        _dev_check(dropmask)
        if dropmask.numel() < batch * heads * L * ((L + 63) // 64) or not dropmask.is_contiguous():
            raise ValueError("attention_fwd: dropmask too small / not contiguous")
    N.call("mmu_attention_fwd", _ptr(qkv), qkv.stride(0), _ptr(keymask), _ptr(O), O.stride(0), _ptr(lse), batch, L,
           heads, float(drop_p), int(seed), _ptr(dropmask) if dropmask is not None else None, _stream(qkv))


def attention_dbias_parts(batch, L, heads=12, device=None):
    """Scratch for the fused Q/K/V bias-gradient column sums of attention_bwd."""
    nqb, nkb = (L + 127) // 128, (L + 63) // 64
    return torch.empty((nqb + 2 * nkb) * batch, heads * 64, dtype=torch.float32, device=device)


def attention_dbias_reduce(parts, batch, L, g_bqkv, heads=12):
    """g_bqkv [3 * heads * 64] += the column sums held in `parts` (Q | K | V row ranges)."""
    nqb, nkb = (L + 127) // 128, (L + 63) // 64
    H = heads * 64
    r0, r1 = nqb * batch, (nqb + nkb) * batch
    colsum_reduce_multi([(parts[:r0], g_bqkv[:H]), (parts[r0:r1], g_bqkv[H:2 * H]), (parts[r1:], g_bqkv[2 * H:])],
                        accumulate=True)


def attention_bwd(qkv, keymask, O, dO, lse, delta, dqkv, batch, L, heads=12, drop_p=0.0, seed=0, dropmask=None,
                  dbias_parts=None):
    """`dropmask` = the buffer the forward filled (required when drop_p > 0); `seed` is
    kept for signature symmetry with the forward; `dbias_parts` (attention_dbias_parts)
    collects the Q/K/V bias-gradient column sums."""
    _dev_check(qkv, keymask, O, dO, lse, delta, dqkv)
    if dropmask is not None:
        _dev_check(dropmask)
        if dropmask.numel() < batch * heads * L * ((L + 63) // 64) or not dropmask.is_contiguous():
            raise ValueError("attention_bwd: dropmask too small / not contiguous")
    N.call("mmu_attention_bwd", _ptr(qkv), qkv.stride(0), _ptr(keymask), _ptr(O), O.stride(0), _ptr(dO), dO.stride(0),
           _ptr(lse), _ptr(delta), _ptr(dqkv), dqkv.stride(0), batch, L, heads, float(drop_p), int(seed),
           _ptr(dropmask) if dropmask is not None else None, _ptr(dbias_parts), _stream(qkv))


def _row0_check(who, batch, L, heads, *mats):
    """[batch * L, >= heads * 64] bf16 matrices with 16-B aligned rows (the C entry checks the pitches)"""
    for t in mats:
        _want(t, torch.bfloat16, who)
        if t.dim() != 2 or t.shape[0] < batch * L or t.shape[1] < heads * 64 or t.stride(1) != 1 \
                or t.stride(0) % 8 or t.data_ptr() % 16:
            raise N.NativeError(f"{who}: operands are [batch * L, cols] bf16 with 16-B aligned rows, got "
                                f"{tuple(t.shape)} strides {t.stride()}")


def attention_row0_fwd(qkv, keymask, O, lse, batch, L, heads=12, drop_p=0.0, seed=0, dropmask=None):
    """attention_fwd for query row 0 of every (batch, head) only: O row 0, lse[:, 0] and the keep
    words [:, 0] are written exactly where (and as) attention_fwd writes them; nothing else is."""
    _dev_check(qkv, keymask, O, lse)
    _row0_check("attention_row0_fwd", batch, L, heads, qkv, O)
    if dropmask is not None:
        _dev_check(dropmask)
        if dropmask.numel() < batch * heads * L * ((L + 63) // 64) or not dropmask.is_contiguous():
            raise ValueError("attention_row0_fwd: dropmask too small / not contiguous")
    if lse.numel() < batch * heads * L or keymask.numel() < batch * L:
        raise ValueError("attention_row0_fwd: lse [batch * heads, L] / keymask [batch, L] too small")
    N.call("mmu_attention_row0_fwd", _ptr(qkv), qkv.stride(0), _ptr(keymask), _ptr(O), O.stride(0), _ptr(lse), batch,
           L, heads, float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(dropmask), _stream(qkv))


def attention_row0_dbias(batch, heads=12, device=None):
    """the [3, batch, heads * 64] f32 column sums (dQ | dK | dV per batch item) of attention_row0_bwd"""
    return torch.empty(3, batch, heads * 64, dtype=torch.float32, device=device)


def attention_row0_bwd(qkv, keymask, O, dO, lse, dqkv, batch, L, heads=12, drop_p=0.0, dropmask=None,
                       dbias_sums=None):
    """Backward of attention_row0_fwd (dO read in row 0 of each batch item only): the dK | dV
    columns of dqkv for all rows, its dQ columns in row 0 only; see mmu_attention_row0_bwd."""
    _dev_check(qkv, keymask, O, dO, lse, dqkv, dbias_sums)
    _row0_check("attention_row0_bwd", batch, L, heads, qkv, dqkv, O, dO)
    if dropmask is not None:
        _dev_check(dropmask)
        if dropmask.numel() < batch * heads * L * ((L + 63) // 64) or not dropmask.is_contiguous():
            raise ValueError("attention_row0_bwd: dropmask too small / not contiguous")
    if dbias_sums is not None and (dbias_sums.dtype != torch.float32 or not dbias_sums.is_contiguous()
                                   or dbias_sums.numel() < 3 * batch * heads * 64):
        raise ValueError("attention_row0_bwd: dbias_sums must be contiguous f32 [3, batch, heads * 64]")
    N.call("mmu_attention_row0_bwd", _ptr(qkv), qkv.stride(0), _ptr(keymask), _ptr(O), O.stride(0), _ptr(dO),
           dO.stride(0), _ptr(lse), _ptr(dqkv), dqkv.stride(0), batch, L, heads, float(drop_p), _ptr(dropmask),
           _ptr(dbias_sums), _stream(qkv))


LN_ROWS_PER_PART = 64


def ln_parts(rows):
    return (rows + LN_ROWS_PER_PART - 1) // LN_ROWS_PER_PART


def _ln_rows(who, X, x_dtype, same=(), vecs=(), parts=()):
    """Host-side argument checks of the LayerNorm wrappers (shapes and dtypes only: no device
    read, no sync).  X: the [rows, H] input of dtype x_dtype; same: (name, tensor or None) bf16
    tensors of X's shape; vecs: (name, tensor or None) f32 per-row vectors of >= rows elements;
    parts: (name, tensor or None) f32 partial column sums of >= ln_parts(rows) * H elements.
    -> rows, H"""
    if X.dim() != 2 or not X.is_contiguous():
        raise N.NativeError(f"{who}: X must be a contiguous 2-D [rows, H] tensor, got {tuple(X.shape)}")
    _want(X, x_dtype, f"{who} X")
    rows, H = X.shape
    for name, t in same:
        if t is None:
            continue
        _want(t, torch.bfloat16, f"{who} {name}")
        if t.shape != X.shape or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must be contiguous [{rows}, {H}] like X, got {tuple(t.shape)}")
    for name, t in vecs:
        if t is None:
            continue
        _want(t, torch.float32, f"{who} {name}")
        if t.numel() < rows or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must hold >= {rows} contiguous elements, got {t.numel()}")
    need = ln_parts(rows) * H
    for name, t in parts:
        if t is None:
            continue
        _want(t, torch.float32, f"{who} {name}")
        if t.numel() < need or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must hold >= ln_parts(rows) x H = {need} contiguous elements, "
                                f"got {t.numel()}")
    return rows, H


def _ln_params(who, rows, H, group_rows, param_stride, **params):
    """f32 contiguous affine parameters of (groups - 1) * param_stride + H elements, rows a
    multiple of group_rows (0: one group)"""
    group_rows, param_stride = int(group_rows), int(param_stride)
    groups = 1
    if group_rows > 0:
        if rows % group_rows:
            raise N.NativeError(f"{who}: rows = {rows} is no multiple of group_rows = {group_rows}")
        groups = rows // group_rows
    if param_stride < 0:
        raise N.NativeError(f"{who}: bad param_stride {param_stride}")
    need = (groups - 1) * param_stride + H
    for name, t in params.items():
        _want(t, torch.float32, f"{who} {name}")
        if t.numel() < need or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must hold (groups - 1) * param_stride + H = {need} contiguous "
                                f"elements, got {t.numel()}")


def layernorm_fwd(X, w, b, Y, mean, rstd, eps=1e-12, group_rows=0, param_stride=0):
    rows, H = _ln_rows("layernorm_fwd", X, torch.bfloat16, same=(("Y", Y),), vecs=(("mean", mean), ("rstd", rstd)))
    _ln_params("layernorm_fwd", rows, H, group_rows, param_stride, w=w, b=b)
    _dev_check(X, w, b, Y, mean, rstd)
    N.call("mmu_layernorm_fwd", _ptr(X), _ptr(w), _ptr(b), _ptr(Y), _ptr(mean), _ptr(rstd), rows, H, float(eps),
           int(group_rows), int(param_stride), _stream(X))


def layernorm_fwd_f32(X, w, b, Y, Y32=None, mean=None, rstd=None, eps=1e-12, group_rows=0, param_stride=0):
    """LN of the f32 hidden stream: X f32 -> Y bf16 (GEMM operand) [+ Y32 f32 (next residual)]."""
    rows, H = _ln_rows("layernorm_fwd_f32", X, torch.float32, same=(("Y", Y),),
                       vecs=(("mean", mean), ("rstd", rstd)))
    if Y32 is not None:
        _want(Y32, torch.float32, "layernorm_fwd_f32 Y32")
        if Y32.shape != X.shape or not Y32.is_contiguous():
            raise N.NativeError(f"layernorm_fwd_f32: Y32 must be contiguous [{rows}, {H}] like X, got "
                                f"{tuple(Y32.shape)}")
    _ln_params("layernorm_fwd_f32", rows, H, group_rows, param_stride, w=w, b=b)
    _dev_check(X, w, b, Y, Y32, mean, rstd)
    N.call("mmu_layernorm_fwd_f32", _ptr(X), _ptr(w), _ptr(b), _ptr(Y), _ptr(Y32), _ptr(mean), _ptr(rstd), rows, H,
           float(eps), int(group_rows), int(param_stride), _stream(X))


def layernorm_bwd(dY, X, mean, rstd, w, dX, dXdrop=None, drop_p=0.0, seed=0, part_dw=None, part_db=None,
                  part_dbias=None, row_step=None, row_offset=0):
    """X: the forward's LN input, bf16 or f32 (the f32 hidden stream: mmu_layernorm_bwd_f32).
    row_step (not None: mmu_layernorm_bwd_f32_rows, f32 X only) / row_offset: row r of dXdrop
    draws the dropout decisions of row row_offset + r * row_step."""
    x32 = X.dtype == torch.float32
    stepped = row_step is not None
    if stepped and not x32:
        raise N.NativeError("layernorm_bwd: row_step / row_offset need an f32 X")
    rows, H = _ln_rows("layernorm_bwd", X, torch.float32 if x32 else torch.bfloat16,
                       same=(("dY", dY), ("dX", dX), ("dXdrop", dXdrop)), vecs=(("mean", mean), ("rstd", rstd)),
                       parts=(("part_dw", part_dw), ("part_db", part_db), ("part_dbias", part_dbias)))
    _ln_params("layernorm_bwd", rows, H, 0, 0, w=w)
    _dev_check(dY, X, mean, rstd, w, dX, dXdrop, part_dw, part_db, part_dbias)
    if stepped:
        N.call("mmu_layernorm_bwd_f32_rows", _ptr(dY), _ptr(X), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(dX),
               _ptr(dXdrop), float(drop_p), int(seed), _ptr(part_dw), _ptr(part_db), _ptr(part_dbias), rows, H,
               LN_ROWS_PER_PART, int(row_step), int(row_offset), _stream(X))
        return
    N.call("mmu_layernorm_bwd_f32" if x32 else "mmu_layernorm_bwd", _ptr(dY), _ptr(X), _ptr(mean), _ptr(rstd),
           _ptr(w), _ptr(dX), _ptr(dXdrop), float(drop_p), int(seed), _ptr(part_dw), _ptr(part_db), _ptr(part_dbias),
           rows, H, LN_ROWS_PER_PART, _stream(X))


def layernorm_bwd_res(dY, X, mean, rstd, w, dRes, dX, part_dw=None, part_db=None, part_dbias=None):
    """Pre-LN backward: dX = LN'(dY) + dRes (part_dbias = column sums of that dX)."""
    rows, H = _ln_rows("layernorm_bwd_res", X, torch.bfloat16, same=(("dY", dY), ("dRes", dRes), ("dX", dX)),
                       vecs=(("mean", mean), ("rstd", rstd)),
                       parts=(("part_dw", part_dw), ("part_db", part_db), ("part_dbias", part_dbias)))
    _ln_params("layernorm_bwd_res", rows, H, 0, 0, w=w)
    _dev_check(dY, X, mean, rstd, w, dRes, dX, part_dw, part_db, part_dbias)
    N.call("mmu_layernorm_bwd_res", _ptr(dY), _ptr(X), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(dRes), _ptr(dX),
           _ptr(part_dw), _ptr(part_db), _ptr(part_dbias), rows, H, LN_ROWS_PER_PART, _stream(X))


def _seqattn_refuse(who, qkv, S, N_, heads, rows=(), vecs=()):
    """Names what is wrong with the arguments of a seqattn wrapper (the slow path of the checks
    below: shapes, dtypes and strides only).  qkv: [>= S*N, 3E] bf16 rows; rows: (name, tensor, width
    in units of E) bf16 row sets of >= S*N rows (row stride free, inner stride 1); vecs: (name,
    tensor) contiguous f32 vectors of >= S*N*heads elements."""
    S, N_, heads = int(S), int(N_), int(heads)
    if S <= 0 or N_ <= 0 or heads <= 0:
        raise N.NativeError(f"{who}: S = {S}, N = {N_}, heads = {heads} must be positive")
    if qkv.dim() != 2 or qkv.shape[1] == 0 or qkv.shape[1] % (3 * heads):
        raise N.NativeError(f"{who}: qkv must be 2-D [S*N, 3E] with 3E divisible by 3*heads = {3 * heads}, got "
                            f"{tuple(qkv.shape)}")
    E = qkv.shape[1] // 3
    for name, t, w in (("qkv", qkv, 3),) + tuple(rows):
        _want(t, torch.bfloat16, f"{who} {name}")
        if t.dim() != 2 or t.shape[1] != w * E:
            raise N.NativeError(f"{who}: {name} must be 2-D of width {w * E}, got {tuple(t.shape)}")
        if t.stride(1) != 1:
            raise N.NativeError(f"{who}: the inner stride of {name} must be 1, got {t.stride(1)}")
        if t.shape[0] < S * N_:
            raise N.NativeError(f"{who}: {name} has {t.shape[0]} rows, S*N = {S * N_} are needed")
    for name, t in vecs:
        _want(t, torch.float32, f"{who} {name}")
        if t.numel() < S * N_ * heads:
            raise ValueError(f"{who}: {name} too small")
        if not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must be contiguous, got strides {tuple(t.stride())}")
    raise N.NativeError(f"{who}: arguments refused")  # not reached: _seq_ld / _seq_vec_ok test the same things


def _seq_ld(t, width, rows):
    """the row stride of a bf16 row set [>= rows, width] with inner stride 1, or -1 (the wrappers run
    once per layer and step: one pass, no message built unless something is wrong)"""
    sh, st = t.shape, t.stride()
    if t.dtype is torch.bfloat16 and len(sh) == 2 and sh[1] == width and sh[0] >= rows and st[1] == 1:
        return st[0]
    return -1


def _seq_vec_ok(t, n):
    return t.dtype is torch.float32 and t.numel() >= n and t.is_contiguous()


def seqattn_fwd(qkv, O, lse2, S, N_, heads):
    """FLAVA attention over the sequence (= batch) axis; see mmu_seqattn_fwd."""
    W = qkv.shape[1] if qkv.dim() == 2 else 0
    ok = S > 0 and N_ > 0 and heads > 0 and W > 0 and W % (3 * heads) == 0
    E, R = W // 3, S * N_
    if ok:
        ld_qkv, ld_o = _seq_ld(qkv, W, R), _seq_ld(O, E, R)
        ok = ld_qkv >= 0 and ld_o >= 0 and _seq_vec_ok(lse2, R * heads)
    if not ok:
        _seqattn_refuse("seqattn_fwd", qkv, S, N_, heads, rows=(("O", O, 1),), vecs=(("lse2", lse2),))
    _dev_check(qkv, O, lse2)
    N.call("mmu_seqattn_fwd", _ptr(qkv), ld_qkv, _ptr(O), ld_o, _ptr(lse2), S, N_, heads, E // heads, _stream(qkv))


def seqattn_bwd(qkv, O, dO, lse2, delta, dqkv, S, N_, heads):
    W = qkv.shape[1] if qkv.dim() == 2 else 0
    ok = S > 0 and N_ > 0 and heads > 0 and W > 0 and W % (3 * heads) == 0
    E, R = W // 3, S * N_
    if ok:
        ld_qkv, ld_o, ld_do, ld_dqkv = _seq_ld(qkv, W, R), _seq_ld(O, E, R), _seq_ld(dO, E, R), _seq_ld(dqkv, W, R)
        ok = ld_qkv >= 0 and ld_o >= 0 and ld_do >= 0 and ld_dqkv >= 0 and _seq_vec_ok(lse2, R * heads) \
            and _seq_vec_ok(delta, R * heads)
    if not ok:
        _seqattn_refuse("seqattn_bwd", qkv, S, N_, heads, rows=(("O", O, 1), ("dO", dO, 1), ("dqkv", dqkv, 3)),
                        vecs=(("lse2", lse2), ("delta", delta)))
    _dev_check(qkv, O, dO, lse2, delta, dqkv)
    N.call("mmu_seqattn_bwd", _ptr(qkv), ld_qkv, _ptr(O), ld_o, _ptr(dO), ld_do, _ptr(lse2), _ptr(delta), _ptr(dqkv),
           ld_dqkv, S, N_, heads, E // heads, _stream(qkv))


EMBED_WIDTHS = (768, 1024)  # the widths embed.hip instantiates (bert-base, bert-large)


def embed_bwd_ws_floats(B, T, n_img, H=768):
    """f32 elements of embed_bwd's workspace at width H, in the mode that is on now"""
    n = N.load().mmu_embed_bwd_ws_floats_h(int(B), int(T), int(n_img), int(H))
    if n < 0:
        raise N.NativeError(f"embed_bwd: H must be 768 or 1024, got {H}")
    return n


def _embed_common(who, ids, seg, proj, word, pos, typ, ln_w, cls_id, sep_id, B, T, n_img):
    """Host-side argument checks shared by embed_fwd / embed_bwd (shapes and dtypes only; the
    values of ids / seg / idx are not read).  Returns H, the width of the word table (768 or 1024),
    which every other tensor is held to."""
    B, T, n_img = int(B), int(T), int(n_img)
    for name, t in (("ids", ids), ("seg", seg)):
        _want(t, torch.int64, f"{who} {name}")
        if tuple(t.shape) != (B, T) or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must be contiguous int64 [B, T] = [{B}, {T}], got {tuple(t.shape)}")
    _want(proj, torch.float32, f"{who} proj")
    # the word table sets the width: an unknown one is named before anything else is held to it
    if word.dim() == 2 and word.shape[1] not in EMBED_WIDTHS:
        _want(word, torch.float32, f"{who} word")
        raise N.NativeError(f"{who}: word must be a contiguous f32 [n, 768] or [n, 1024] table (the widths the "
                            f"embedding kernels are built for), got {tuple(word.shape)}")
    H = word.shape[1] if word.dim() == 2 else 768
    if tuple(proj.shape) != (B, n_img, H) or not proj.is_contiguous():
        raise N.NativeError(f"{who}: proj must be contiguous f32 [B, n_img, {H}] = [{B}, {n_img}, {H}], got "
                            f"{tuple(proj.shape)}")
    for name, t in (("word", word), ("pos", pos), ("typ", typ)):
        _want(t, torch.float32, f"{who} {name}")
        if t.dim() != 2 or t.shape[1] != H or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must be a contiguous f32 [n, {H}] table, got {tuple(t.shape)}")
    _want(ln_w, torch.float32, f"{who} ln_w")
    if ln_w.numel() != H or not ln_w.is_contiguous():
        raise N.NativeError(f"{who}: ln_w must hold {H} contiguous elements, got {ln_w.numel()}")
    if max(n_img + 2, T) > pos.shape[0]:
        raise N.NativeError(f"{who}: max(n_img + 2, T) = {max(n_img + 2, T)} exceeds the {pos.shape[0]} position rows")
    if not (0 <= int(cls_id) < word.shape[0] and 0 <= int(sep_id) < word.shape[0]):
        raise N.NativeError(f"{who}: cls_id / sep_id = {cls_id} / {sep_id} outside the {word.shape[0]} word rows")
    if typ.shape[0] < 2:
        raise N.NativeError(f"{who}: typ must hold >= 2 token-type rows, got {typ.shape[0]}")
    return H


def embed_fwd(ids, seg, txt_mask, proj, word, pos, typ, ln_w, ln_b, eps, cls_id, sep_id, idx, V, B, T, n_img, Lout,
              X, keymask, mean=None, rstd=None, drop_txt=0.0, drop_img=0.0, seed=0, X32=None):
    """X32 (optional, f32 like X): the same rows in f32, the encoder's f32 hidden stream."""
    who = "embed_fwd"
    H = _embed_common(who, ids, seg, proj, word, pos, typ, ln_w, cls_id, sep_id, B, T, n_img)
    rows = int(V) * int(B) * int(Lout)
    if txt_mask is not None:
        _want(txt_mask, torch.int64, f"{who} txt_mask")
        if tuple(txt_mask.shape) != (B, T) or not txt_mask.is_contiguous():
            raise N.NativeError(f"{who}: txt_mask must be contiguous int64 [B, T] = [{B}, {T}], got "
                                f"{tuple(txt_mask.shape)}")
    _want(ln_b, torch.float32, f"{who} ln_b")
    if ln_b.numel() != H or not ln_b.is_contiguous():
        raise N.NativeError(f"{who}: ln_b must hold {H} contiguous elements, got {ln_b.numel()}")
    if idx is not None:
        _want(idx, torch.int64, f"{who} idx")
        if tuple(idx.shape) != (V, Lout) or not idx.is_contiguous():
            raise N.NativeError(f"{who}: idx must be contiguous int64 [V, Lout] = [{V}, {Lout}], got "
                                f"{tuple(idx.shape)}")
    for name, t, dt in (("X", X, torch.bfloat16), ("X32", X32, torch.float32)):
        if t is None:
            continue
        _want(t, dt, f"{who} {name}")
        if tuple(t.shape) != (rows, H) or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must be contiguous [V * B * Lout, {H}] = [{rows}, {H}], got "
                                f"{tuple(t.shape)}")
    for name, t in (("keymask", keymask), ("mean", mean), ("rstd", rstd)):
        if t is None:
            continue
        _want(t, torch.float32, f"{who} {name}")
        if t.numel() < rows or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must hold >= V * B * Lout = {rows} contiguous elements, got "
                                f"{t.numel()}")
    _dev_check(ids, seg, txt_mask, idx, proj, word, pos, typ, ln_w, ln_b, X, X32, keymask, mean, rstd)
    N.call("mmu_embed_fwd", _ptr(ids), _ptr(seg), _ptr(txt_mask), _ptr(proj), _ptr(word), _ptr(pos), _ptr(typ),
           _ptr(ln_w), _ptr(ln_b), float(eps), int(cls_id), int(sep_id), _ptr(idx), V, B, T, n_img, Lout, H,
           float(drop_txt), float(drop_img), int(seed), _ptr(X), _ptr(X32), _ptr(keymask), _ptr(mean), _ptr(rstd),
           _stream(X))


def embed_bwd(dX, ids, seg, proj, word, pos, typ, ln_w, mean, rstd, cls_id, sep_id, B, T, n_img, d_word, d_pos,
              d_type, d_ln_w, d_ln_b, d_proj, drop_txt=0.0, drop_img=0.0, seed=0):
    who = "embed_bwd"
    H = _embed_common(who, ids, seg, proj, word, pos, typ, ln_w, cls_id, sep_id, B, T, n_img)
    rows = int(B) * (int(n_img) + 2 + int(T))
    _want(dX, torch.bfloat16, f"{who} dX")
    if tuple(dX.shape) != (rows, H) or not dX.is_contiguous():
        raise N.NativeError(f"{who}: dX must be contiguous bf16 [B * (n_img + 2 + T), {H}] = [{rows}, {H}], got "
                            f"{tuple(dX.shape)}")
    for name, t in (("mean", mean), ("rstd", rstd)):
        _want(t, torch.float32, f"{who} {name}")
        if t.numel() < rows or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must hold >= {rows} contiguous elements, got {t.numel()}")
    for name, t, like in (("d_word", d_word, word), ("d_pos", d_pos, pos), ("d_type", d_type, typ),
                          ("d_ln_w", d_ln_w, ln_w), ("d_ln_b", d_ln_b, ln_w), ("d_proj", d_proj, proj)):
        _want(t, torch.float32, f"{who} {name}")
        if t.shape != like.shape or not t.is_contiguous():
            raise N.NativeError(f"{who}: {name} must be contiguous f32 {tuple(like.shape)} like its parameter, got "
                                f"{tuple(t.shape)}")
    _dev_check(dX, ids, seg, proj, word, pos, typ, ln_w, mean, rstd, d_word, d_pos, d_type, d_ln_w, d_ln_b, d_proj)
    ws = torch.empty(embed_bwd_ws_floats(B, T, n_img, H), dtype=torch.float32, device=dX.device)
    N.call("mmu_embed_bwd", _ptr(dX), _ptr(ids), _ptr(seg), _ptr(proj), _ptr(word), _ptr(pos), _ptr(typ),
           _ptr(ln_w), _ptr(mean), _ptr(rstd), int(cls_id), int(sep_id), B, T, n_img, H, float(drop_txt),
           float(drop_img), int(seed), _ptr(d_word),
           _ptr(d_pos), _ptr(d_type), _ptr(d_ln_w), _ptr(d_ln_b), _ptr(d_proj), _ptr(ws), _stream(dX))


def image_normalize(img_u8, mean, std, out):
    """uint8 HWC crops [B, H, W, 3] -> out = (x/255 - mean) / std as the channels-last
    [B, 3, H, W] image (f32 or bf16); see mmu_image_normalize."""
    _dev_check(img_u8, out)
    _want(img_u8, torch.uint8, "image_normalize input")
    if not img_u8.is_contiguous() or img_u8.shape[-1] != 3:
        raise N.NativeError("image_normalize: input must be contiguous [B, H, W, 3] uint8")
    if out.dtype not in (torch.float32, torch.bfloat16) or out.numel() != img_u8.numel() or \
            not out.is_contiguous(memory_format=torch.channels_last):
        raise N.NativeError("image_normalize: out must be a channels-last f32/bf16 [B, 3, H, W] of the same size")
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    N.call("mmu_image_normalize", _ptr(img_u8), img_u8.numel(), m, s, _ptr(out),
           N.MMU_F32 if out.dtype == torch.float32 else N.MMU_BF16, _stream(out))
    return out


def _aligned(who, *ts):
    """the conv / stem / pool kernels move 16 B per lane: a tensor that does not start on a 16-B
    boundary (a view into the middle of a row) is refused"""
    for t in ts:
        if t is not None and t.data_ptr() % 16:
            raise N.NativeError(f"{who}: a tensor {tuple(t.shape)} {t.dtype} is not 16-B aligned")


def maxpool_fwd(x, y, argmax):
    """MaxPool2d(3, 2, 1) of a channels-last bf16 [B, C, H, W] map -> y [B, C, OH, OW]
    (channels-last) and the uint8 argmax in y's NHWC layout; see mmu_maxpool_fwd."""
    _maxpool_check(x, y, argmax, "x", "y")
    _dev_check(x, y, argmax)
    B, C, H, W = x.shape
    N.call("mmu_maxpool_fwd", _ptr(x), B, H, W, C, _ptr(y), _ptr(argmax), _stream(x))


def maxpool_bwd(dy, argmax, dx):
    _maxpool_check(dx, dy, argmax, "dx", "dy")
    _dev_check(dy, argmax, dx)
    B, C, H, W = dx.shape
    N.call("mmu_maxpool_bwd", _ptr(dy), _ptr(argmax), B, H, W, C, _ptr(dx), _stream(dx))


def _maxpool_check(full, pooled, argmax, nf, np_):
    """The kernels index raw NHWC pointers: refuse any layout / size they do not assume."""
    for t, nm in ((full, nf), (pooled, np_)):
        _want(t, torch.bfloat16, f"maxpool {nm}")
        if t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last):
            raise N.NativeError(f"maxpool: {nm} must be a channels-last [B, C, H, W] bf16 map")
    B, C, H, W = full.shape
    oshape = (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    if tuple(pooled.shape) != oshape:
        raise N.NativeError(f"maxpool: {np_} is {tuple(pooled.shape)}, MaxPool2d(3, 2, 1) of "
                            f"{(B, C, H, W)} is {oshape}")
    if argmax.dtype != torch.uint8 or argmax.numel() != pooled.numel() or not argmax.is_contiguous():
        raise N.NativeError("maxpool: argmax must be a contiguous uint8 tensor with one entry per pooled element")
    _aligned("maxpool", full, pooled, argmax)


def _row_pool_check(who, fmap, n, vec, nv):
    """The kernels read fmap as raw [B][Hh][Ww][C] bf16 and vec as raw [B][n][C] f32."""
    _want(fmap, torch.bfloat16, f"{who} fmap")
    if fmap.dim() != 4 or not fmap.is_contiguous() or fmap.shape[3] % 8:
        raise N.NativeError(f"{who}: fmap must be a contiguous [B, Hh, Ww, C] bf16 map with C % 8 == 0 "
                            f"(got {tuple(fmap.shape)}, strides {tuple(fmap.stride())})")
    B, Hh, Ww, C = fmap.shape
    if not 1 <= n <= Hh:
        raise N.NativeError(f"{who}: n = {n} rows must be within 1 .. Hh = {Hh}")
    _want(vec, torch.float32, f"{who} {nv}")
    if not vec.is_contiguous() or vec.numel() != B * n * C:
        raise N.NativeError(f"{who}: {nv} must be a contiguous f32 tensor of B * n * C = {B * n * C} elements "
                            f"(got {tuple(vec.shape)})")
    _aligned(who, fmap, vec)
    return B, Hh, Ww, C


def row_pool_fwd(fmap_nhwc, n, out):
    """AdaptiveAvgPool2d((n, 1)) of a contiguous bf16 [B, Hh, Ww, C] map -> out f32 [B, n, C]"""
    B, Hh, Ww, C = _row_pool_check("row_pool_fwd", fmap_nhwc, n, out, "out")
    _dev_check(fmap_nhwc, out)
    N.call("mmu_row_pool_fwd", _ptr(fmap_nhwc), B, Hh, Ww, C, n, _ptr(out), _stream(out))


def row_pool_bwd(dout, n, dfmap_nhwc):
    B, Hh, Ww, C = _row_pool_check("row_pool_bwd", dfmap_nhwc, n, dout, "dout")
    _dev_check(dout, dfmap_nhwc)
    N.call("mmu_row_pool_bwd", _ptr(dout), B, Hh, Ww, C, n, _ptr(dfmap_nhwc), _stream(dout))


def _conv_out(h, w, ksize, stride):
    pad = ksize // 2
    return (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1


def conv_implicit(X, Wk, Y, ksize=3, stride=1, stats=None):
    """Y[p, n] = sum_{tap, c} X[input pixel of (p, tap), c] Wk[n, tap * C + c]: a ksize x ksize
    (3: pad 1, 1: pad 0) / stride conv as one implicit-im2col GEMM.  X [N, C, H, W] and Y
    [N, Nout, Ho, Wo] channels-last bf16, Wk bf16 with memory [Nout][ksize][ksize][C] (a
    channels-last [Nout, C, k, k] filter, or the flipped-transposed 3x3 one for dX).
    stats (optional, bn_stats_table of Y's rows): Y's BatchNorm statistics, written too."""
    _want(X, torch.bfloat16, "conv_implicit X")
    _want(Wk, torch.bfloat16, "conv_implicit Wk")
    if X.dim() != 4 or Y.dim() != 4:
        raise N.NativeError("conv_implicit: X and Y must be 4-D [N, C, H, W] maps")
    n, c, h, w = X.shape
    nout = Y.shape[1]
    ho, wo = _conv_out(h, w, ksize, stride)
    cl = torch.channels_last
    # the kernel reads Wk[n][tap * C + c]: either a [Nout, k, k, C] contiguous tensor or a
    # [Nout, C, k, k] filter whose memory is channels-last (both are [Nout][k][k][C] in memory)
    k = ksize
    wk_ok = Wk.dim() == 4 and (
        (tuple(Wk.shape) == (nout, k, k, c) and Wk.is_contiguous())
        or (tuple(Wk.shape) == (nout, c, k, k) and Wk.is_contiguous(memory_format=cl)))
    if (Y.shape != (n, nout, ho, wo) or Y.dtype != torch.bfloat16 or not wk_ok
            or not X.is_contiguous(memory_format=cl) or not Y.is_contiguous(memory_format=cl)):
        raise N.NativeError(f"conv_implicit: X channels-last bf16 [N, C, H, W], Y [N, Nout, {ho}, {wo}], "
                            f"Wk [Nout][{k}][{k}][C] bf16")
    if stats is not None and (stats.dtype != torch.float32 or not stats.is_contiguous()
                              or stats.numel() < ((n * ho * wo + 63) // 64) * nout * 2):
        raise N.NativeError("conv_implicit: stats table too small (kernels.bn_stats_table)")
    _aligned("conv_implicit", X, Wk, Y, stats)
    _dev_check(X, Wk, Y, stats)
    ws = _splitk_workspace(Y.device)  # split-K slabs for small maps (few tiles)
    if stats is not None:
        N.call("mmu_conv_implicit_stats", _ptr(X), _ptr(Wk), _ptr(Y), n, h, w, c, nout, ksize, stride, _ptr(stats),
               _ptr(ws), ws.numel(), _stream(X))
        return
    N.call("mmu_conv_implicit", _ptr(X), _ptr(Wk), _ptr(Y), n, h, w, c, nout, ksize, stride, _ptr(ws), ws.numel(),
           _stream(X))


def conv3x3_implicit(X, Wk, Y, bnb=None, table=None):
    """the 3x3 / stride-1 / pad-1 case of conv_implicit (Y and X share H, W).  bnb = (x, relu_mask,
    mean) with table (bn_stats_table of Y's rows): Y is the data gradient dY of that training
    BatchNorm, and the table receives its backward reduction (mmu_conv3x3_implicit_bnb)."""
    if bnb is None:
        conv_implicit(X, Wk, Y, 3, 1)
        return
    x, mask, mean = bnb
    if X.dim() != 4 or Y.dim() != 4 or x.dim() != 4 or table is None:
        raise N.NativeError("conv3x3_implicit bnb: X, Y and x must be 4-D [N, C, H, W] maps, with a table")
    n, c, h, w = X.shape
    nout = Y.shape[1]
    cl = torch.channels_last
    if (Y.shape != (n, nout, h, w) or x.shape != Y.shape or Y.dtype != torch.bfloat16 or X.dtype != torch.bfloat16
            or Wk.dtype != torch.bfloat16 or tuple(Wk.shape) != (nout, 3, 3, c) or not Wk.is_contiguous()
            or not X.is_contiguous(memory_format=cl) or not Y.is_contiguous(memory_format=cl)):
        raise N.NativeError("conv3x3_implicit bnb: X / Y / x channels-last bf16, Wk [Nout][3][3][C] bf16")
    if table.dtype != torch.float32 or not table.is_contiguous() or table.numel() < ((n * h * w + 63) // 64) * nout * 2:
        raise N.NativeError("conv3x3_implicit bnb: table too small (kernels.bn_stats_table)")
    _aligned("conv3x3_implicit bnb", X, Wk, Y, table, x, mean)
    _bnb_check(x, mask, mean, "conv3x3_implicit bnb")
    _dev_check(X, Wk, Y, table, x, mean)
    ws = _splitk_workspace(Y.device)
    N.call("mmu_conv3x3_implicit_bnb", _ptr(X), _ptr(Wk), _ptr(Y), n, h, w, c, nout, _ptr(x), _ptr(mask),
           _ptr(mean), _ptr(table), _ptr(ws), ws.numel(), _stream(X))


def _stem_check(X, what):
    if (X.dim() != 4 or X.dtype != torch.bfloat16 or X.shape[1] != 3
            or not X.is_contiguous(memory_format=torch.channels_last)):
        raise N.NativeError(f"{what}: X must be channels-last bf16 [N, 3, H, W] (got {tuple(X.shape)} {X.dtype})")


def stem_conv_fwd(X, Wk, Y):
    """Y = conv2d(X, Wk, stride 2, padding 3): the ResNet stem (7x7, 3 -> 64).  X [N, 3, H, W]
    and Y [N, 64, Ho, Wo] channels-last bf16; Wk bf16 [64, 3, 7, 7] channels-last (memory
    [64][7][7][3], the parameter store's filter copy)."""
    _stem_check(X, "stem_conv_fwd")
    n, _, h, w = X.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if (tuple(Wk.shape) != (64, 3, 7, 7) or Wk.dtype != torch.bfloat16
            or not Wk.is_contiguous(memory_format=torch.channels_last)):
        raise N.NativeError("stem_conv_fwd: Wk must be channels-last bf16 [64, 3, 7, 7]")
    if (tuple(Y.shape) != (n, 64, ho, wo) or Y.dtype != torch.bfloat16
            or not Y.is_contiguous(memory_format=torch.channels_last)):
        raise N.NativeError(f"stem_conv_fwd: Y must be channels-last bf16 [{n}, 64, {ho}, {wo}]")
    _aligned("stem_conv_fwd", X, Wk, Y)
    _dev_check(X, Wk, Y)
    N.call("mmu_stem_conv_fwd", _ptr(X), _ptr(Wk), _ptr(Y), n, h, w, _stream(X))


def stem_conv_wgrad(dY, X, dW, accumulate=False):
    """dW (+)= the stem conv's filter gradient: dY [N, 64, Ho, Wo] and X [N, 3, H, W]
    channels-last bf16, dW f32 [64, 3, 7, 7] channels-last."""
    _stem_check(X, "stem_conv_wgrad")
    n, _, h, w = X.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if (tuple(dY.shape) != (n, 64, ho, wo) or dY.dtype != torch.bfloat16
            or not dY.is_contiguous(memory_format=torch.channels_last)):
        raise N.NativeError(f"stem_conv_wgrad: dY must be channels-last bf16 [{n}, 64, {ho}, {wo}]")
    if (tuple(dW.shape) != (64, 3, 7, 7) or dW.dtype != torch.float32
            or not dW.is_contiguous(memory_format=torch.channels_last)):
        raise N.NativeError("stem_conv_wgrad: dW must be channels-last f32 [64, 3, 7, 7]")
    _aligned("stem_conv_wgrad", dY, X, dW)
    _dev_check(dY, X, dW)
    need = N.load().mmu_stem_conv_wgrad_ws_floats(n, h, w)
    ws = _splitk_workspace(X.device)
    if need < 0 or ws.numel() < need:
        raise N.NativeError(f"stem_conv_wgrad: workspace of {ws.numel()} floats, needs {need}")
    N.call("mmu_stem_conv_wgrad", _ptr(dY), _ptr(X), _ptr(dW), n, h, w, int(bool(accumulate)), _ptr(ws), ws.numel(),
           _stream(X))


def conv_wgrad(dY, X, dW, ksize=3, stride=1, accumulate=False):
    """dW (+)= weight gradient of a ksize x ksize (3: pad 1, 1: pad 0) / stride conv: X [N, Cin,
    H, W] and dY [N, Cout, Ho, Wo] channels-last bf16, dW f32 [Cout, Cin, k, k] channels-last
    (memory [Cout][k][k][Cin]).  Cin % 256 == 0, Cout % 128 == 0."""
    _want(X, torch.bfloat16, "conv_wgrad X")
    _want(dY, torch.bfloat16, "conv_wgrad dY")
    if X.dim() != 4 or dY.dim() != 4:
        raise N.NativeError("conv_wgrad: X and dY must be 4-D [N, C, H, W] maps")
    n, cin, h, w = X.shape
    cout = dY.shape[1]
    ho, wo = _conv_out(h, w, ksize, stride)
    cl = torch.channels_last
    if (dY.shape != (n, cout, ho, wo) or dW.shape != (cout, cin, ksize, ksize) or dW.dtype != torch.float32
            or not X.is_contiguous(memory_format=cl) or not dY.is_contiguous(memory_format=cl)
            or not dW.is_contiguous(memory_format=cl)):
        raise N.NativeError(f"conv_wgrad: X channels-last bf16 [N, C, H, W], dY [N, Cout, {ho}, {wo}], "
                            f"dW f32 channels-last [Cout, Cin, {ksize}, {ksize}]")
    _aligned("conv_wgrad", dY, X, dW)
    _dev_check(dY, X, dW)
    ws = _splitk_workspace(X.device)
    N.call("mmu_conv_wgrad", _ptr(dY), _ptr(X), _ptr(dW), n, h, w, cin, cout, ksize, stride, int(bool(accumulate)),
           _ptr(ws), ws.numel(), _stream(X))


def conv3x3_wgrad(dY, X, dW, accumulate=False):
    """the 3x3 / stride-1 / pad-1 case of conv_wgrad"""
    conv_wgrad(dY, X, dW, 3, 1, accumulate)


_bn_ws = {}


def _bn_workspace(dev):
    """per-device scratch for mmu_batchnorm_*, reused stream-ordered by every call"""
    t = _bn_ws.get(dev)
    if t is None:
        nbytes = N.load().mmu_batchnorm_ws_bytes(2048)
        t = _bn_ws[dev] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    return t


def _bn_mask_check(mask, X, what):
    if mask is None:
        return
    C = X.shape[1]
    if mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != X.numel() // 8 or C % 8:
        raise N.NativeError(f"{what}: relu_mask must be contiguous uint8 with numel = X.numel() / 8 "
                            f"(got {tuple(mask.shape)} {mask.dtype} for X {tuple(X.shape)})")
    _dev_check(mask, X)


def _bn_vec_check(name, C, *ts):
    """per-channel BatchNorm vectors must be f32 (the kernels read / write them as float[C]: a
    bf16 running_mean -- e.g. after module.to(bfloat16) -- would be written past its end).
    Only the dtype is checked per call (cheap: this runs ~300 times per train step)."""
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise N.NativeError(f"{name}: per-channel tensors must be f32 (got {t.dtype} {tuple(t.shape)})")


def _bn_map_check(name, X, *ts):
    for t in ts:
        if t is not None and t.dtype != torch.bfloat16:
            raise N.NativeError(f"{name}: maps must be bf16 (got {t.dtype} {tuple(t.shape)})")


def _bn_res_check(name, X, *ts):
    for t in ts:
        if t is not None and (t.dtype != torch.int8 or t.numel() != X.numel() or not t.is_contiguous()):
            raise N.NativeError(f"{name}: a stream residue must be a contiguous int8 tensor of X's size")


def batchnorm_fwd(X, Y, weight, bias, running_mean, running_var, training, momentum, eps, relu=False, skip=None,
                  num_batches_tracked=None, save_mean=None, save_invstd=None, relu_mask=None, skip_res=None,
                  y_res=None, parts=None):
    """X, Y, skip: channels-last bf16 [N, C, H, W] (contiguous as [N*H*W, C]).  relu_mask
    (optional, relu only): uint8 [N*H*W*C/8] written with the bits Y > 0 for batchnorm_bwd.
    y_res / skip_res (optional, int8 of X's size): the residual stream's 8-bit residue of Y /
    of skip (include/mmu.h).  parts (training only): (table, nparts) of X's statistics from the
    conv that produced X (bn_stats_table): no statistics pass (mmu_batchnorm_fwd_parts)."""
    _dev_check(X, Y)
    _want(X, torch.bfloat16, "batchnorm X")
    _bn_mask_check(relu_mask, X, "batchnorm_fwd")
    C = X.shape[1]
    _bn_vec_check("batchnorm_fwd", C, weight, bias, running_mean, running_var, save_mean, save_invstd)
    _bn_map_check("batchnorm_fwd", X, Y, skip)
    _bn_res_check("batchnorm_fwd", X, skip_res, y_res)
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise N.NativeError("batchnorm_fwd: num_batches_tracked must be int64")
    rows = X.numel() // C
    ws = _bn_workspace(X.device)
    if parts is not None:
        table, nparts = parts
        if not training or table.numel() < nparts * C * 2 or nparts != (rows + 63) // 64:
            raise N.NativeError("batchnorm_fwd: parts must be X's training statistics table (bn_stats_table)")
        N.call("mmu_batchnorm_fwd_parts", _ptr(X), _ptr(skip), _ptr(Y), rows, C, _ptr(table), nparts, _ptr(weight),
               _ptr(bias), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), float(momentum),
               float(eps), int(bool(relu)), _ptr(save_mean), _ptr(save_invstd), _ptr(relu_mask), _ptr(skip_res),
               _ptr(y_res), _ptr(ws), ws.numel() * 4, _stream(X))
        return
    N.call("mmu_batchnorm_fwd", _ptr(X), _ptr(skip), _ptr(Y), rows, C, _ptr(weight), _ptr(bias), _ptr(running_mean),
           _ptr(running_var), _ptr(num_batches_tracked), int(bool(training)), float(momentum), float(eps),
           int(bool(relu)), _ptr(save_mean), _ptr(save_invstd), _ptr(relu_mask), _ptr(skip_res), _ptr(y_res),
           _ptr(ws), ws.numel() * 4, _stream(X))


def batchnorm_bwd(dY, Y, X, weight, save_mean, save_invstd, relu, dX, dSkip=None, dweight=None, dbias=None,
                  relu_mask=None, parts=None):
    """relu: g = dY * [Y > 0] from relu_mask (batchnorm_fwd's) when given, else from Y.  parts:
    (table, nparts) of the reduction the product that formed dY wrote (STORE_BNB / ADD_RES_BNB,
    conv3x3_implicit bnb): no reduction pass (mmu_batchnorm_bwd_parts)."""
    _dev_check(dY, X, dX)
    _want(X, torch.bfloat16, "batchnorm_bwd X")
    _bn_mask_check(relu_mask, X, "batchnorm_bwd")
    C = X.shape[1]
    _bn_vec_check("batchnorm_bwd", C, weight, save_mean, save_invstd, dweight, dbias)
    _bn_map_check("batchnorm_bwd", X, dY, Y, dX, dSkip)
    rows = X.numel() // C
    ws = _bn_workspace(X.device)
    if parts is not None:
        table, nparts = parts
        if table.numel() < nparts * C * 2 or nparts != (rows + 63) // 64:
            raise N.NativeError("batchnorm_bwd: parts must be dY's reduction table (bn_stats_table)")
        N.call("mmu_batchnorm_bwd_parts", _ptr(dY), _ptr(Y), _ptr(relu_mask), _ptr(X), rows, C, _ptr(table), nparts,
               _ptr(weight), _ptr(save_mean), _ptr(save_invstd), int(bool(relu)), _ptr(dX), _ptr(dSkip),
               _ptr(dweight), _ptr(dbias), _ptr(ws), ws.numel() * 4, _stream(X))
        return
    N.call("mmu_batchnorm_bwd", _ptr(dY), _ptr(Y), _ptr(relu_mask), _ptr(X), rows, C, _ptr(weight), _ptr(save_mean),
           _ptr(save_invstd), int(bool(relu)), _ptr(dX), _ptr(dSkip), _ptr(dweight), _ptr(dbias), _ptr(ws),
           ws.numel() * 4, _stream(X))


def bn_sums_buffer(C, device):
    """[2C+1] f64: the per-channel sums of one cross-rank BatchNorm pass + its row count"""
    return torch.empty(2 * C + 1, dtype=torch.float64, device=device)


def batchnorm_stats(X, sums):
    """cross-rank BatchNorm, forward first half: sums = {sum x, sum x^2, rows} over X's rows"""
    _dev_check(X, sums)
    _want(X, torch.bfloat16, "batchnorm_stats X")
    C = X.shape[1]
    _bn_sums_check("batchnorm_stats", sums, C)
    _bn_map_check("batchnorm_stats", X)
    ws = _bn_workspace(X.device)
    N.call("mmu_batchnorm_stats", _ptr(X), X.numel() // C, C, _ptr(sums), _ptr(ws), ws.numel() * 4, _stream(X))


def batchnorm_fwd_sums(X, Y, sums, weight, bias, running_mean, running_var, momentum, eps, relu=False, skip=None,
                       num_batches_tracked=None, save_mean=None, save_invstd=None, relu_mask=None, skip_res=None,
                       y_res=None):
    """cross-rank BatchNorm, forward second half: batchnorm_fwd (training) with the statistics
    of the exchanged sums"""
    _dev_check(X, Y, sums)
    _want(X, torch.bfloat16, "batchnorm X")
    _bn_mask_check(relu_mask, X, "batchnorm_fwd_sums")
    C = X.shape[1]
    _bn_sums_check("batchnorm_fwd_sums", sums, C)
    _bn_vec_check("batchnorm_fwd_sums", C, weight, bias, running_mean, running_var, save_mean, save_invstd)
    _bn_map_check("batchnorm_fwd_sums", X, Y, skip)
    _bn_res_check("batchnorm_fwd_sums", X, skip_res, y_res)
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise N.NativeError("batchnorm_fwd_sums: num_batches_tracked must be int64")
    ws = _bn_workspace(X.device)
    N.call("mmu_batchnorm_fwd_sums", _ptr(X), _ptr(skip), _ptr(Y), X.numel() // C, C, _ptr(sums), _ptr(weight),
           _ptr(bias), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), float(momentum), float(eps),
           int(bool(relu)), _ptr(save_mean), _ptr(save_invstd), _ptr(relu_mask), _ptr(skip_res), _ptr(y_res),
           _ptr(ws), ws.numel() * 4, _stream(X))


def batchnorm_bwd_reduce(dY, Y, X, save_mean, save_invstd, relu, sums, dweight=None, dbias=None, relu_mask=None):
    """cross-rank BatchNorm, backward first half: sums = {sum g, sum g*(x-mean), rows};
    dweight / dbias += this rank's"""
    _dev_check(dY, X, sums)
    _want(X, torch.bfloat16, "batchnorm_bwd X")
    _bn_mask_check(relu_mask, X, "batchnorm_bwd_reduce")
    C = X.shape[1]
    _bn_sums_check("batchnorm_bwd_reduce", sums, C)
    _bn_vec_check("batchnorm_bwd_reduce", C, save_mean, save_invstd, dweight, dbias)
    _bn_map_check("batchnorm_bwd_reduce", X, dY, Y)
    ws = _bn_workspace(X.device)
    N.call("mmu_batchnorm_bwd_reduce", _ptr(dY), _ptr(Y), _ptr(relu_mask), _ptr(X), X.numel() // C, C,
           _ptr(save_mean), _ptr(save_invstd), int(bool(relu)), _ptr(sums), _ptr(dweight), _ptr(dbias), _ptr(ws),
           ws.numel() * 4, _stream(X))


def batchnorm_bwd_sums(dY, Y, X, sums, weight, save_mean, save_invstd, relu, dX, dSkip=None, relu_mask=None):
    """cross-rank BatchNorm, backward second half: dX (, dSkip) from the exchanged sums"""
    _dev_check(dY, X, dX, sums)
    _want(X, torch.bfloat16, "batchnorm_bwd X")
    _bn_mask_check(relu_mask, X, "batchnorm_bwd_sums")
    C = X.shape[1]
    _bn_sums_check("batchnorm_bwd_sums", sums, C)
    _bn_vec_check("batchnorm_bwd_sums", C, weight, save_mean, save_invstd)
    _bn_map_check("batchnorm_bwd_sums", X, dY, Y, dX, dSkip)
    ws = _bn_workspace(X.device)
    N.call("mmu_batchnorm_bwd_sums", _ptr(dY), _ptr(Y), _ptr(relu_mask), _ptr(X), X.numel() // C, C, _ptr(sums),
           _ptr(weight), _ptr(save_mean), _ptr(save_invstd), int(bool(relu)), _ptr(dX), _ptr(dSkip), _ptr(ws),
           ws.numel() * 4, _stream(X))


def _bn_sums_check(who, sums, C):
    if sums.dtype != torch.float64 or sums.numel() != 2 * C + 1 or not sums.is_contiguous():
        raise N.NativeError(f"{who}: sums must be a contiguous float64 [2C+1] = [{2 * C + 1}] tensor")


def bertadam_step(params, grads, m, v, bf16_copy, table, steps, n_tensors, n_chunks, lr_decay, lr_nodecay, wd,
                  warmup, t_total, b1, b2, eps, max_grad_norm, ws, grad_scale=1.0):
    _dev_check(params, grads, m, v, table, steps, ws)
    N.call("mmu_bertadam_step", _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(bf16_copy), _ptr(table),
           _ptr(steps), n_tensors, n_chunks, float(lr_decay), float(lr_nodecay), float(wd), float(warmup),
           float(t_total), float(b1), float(b2), float(eps), float(max_grad_norm), float(grad_scale), _ptr(ws),
           ws.numel(), _stream(params))


def uncertainty(logits, y, p_bar, nll, conf, correct):
    _dev_check(logits, y, p_bar, nll, conf, correct)
    S, R, C = logits.shape
    N.call("mmu_uncertainty", _ptr(logits), _ptr(y), S, R, C, _ptr(p_bar), _ptr(nll), _ptr(conf), _ptr(correct),
           _stream(logits))


def ece_bins(conf, correct, n_bins, out):
    _dev_check(conf, correct, out)
    N.call("mmu_ece_bins", _ptr(conf), _ptr(correct), conf.numel(), n_bins, _ptr(out), _stream(conf))


# include/mmu.h MMU_UNC_*: the columns of uncertainty_decompose's stats
UNC_COLUMNS = ("total", "aleatoric", "mi_members", "mi_passes", "brier", "nll", "conf", "correct",
               "vote_disagreement")
UNC_NSTAT = len(UNC_COLUMNS)


_inv_temp_seen = None   # (weakref to the last table whose contents passed, its version counter)


def _inv_temp_check(who, inv_temp, shape, what):
    """an inverse-temperature table: contiguous f32 of the given shape, every entry finite and >= 0
    (the library cannot look into device memory).  Reading the verdict back synchronises the device, so
    it is done once per table: the same tensor, not written in place since, is not read again -- a meter
    that passes one [K] tensor on every update pays for the first."""
    global _inv_temp_seen
    _want(inv_temp, torch.float32, "inv_temp")
    if tuple(inv_temp.shape) != shape or not inv_temp.is_contiguous():
        raise N.NativeError(f"{who}: inv_temp must be contiguous f32 {what} = {list(shape)}, got "
                            f"{tuple(inv_temp.shape)}")
    if _inv_temp_seen is not None and _inv_temp_seen[0]() is inv_temp and _inv_temp_seen[1] == inv_temp._version:
        return
    if not bool((torch.isfinite(inv_temp) & (inv_temp >= 0)).all()):
        raise N.NativeError(f"{who}: every inverse temperature must be finite and >= 0")
    _inv_temp_seen = (weakref.ref(inv_temp), inv_temp._version)


def _labels(who, y, S):
    _want(y, torch.int64, "y")
    if tuple(y.shape) != (S,) or not y.is_contiguous():
        raise N.NativeError(f"{who}: y must be contiguous int64 [S] = [{S}], got {tuple(y.shape)}")


def _logit_stack(who, logits, y, axes, allow_3d=False):
    """The logit stack of an ensemble statistic: f32, 4-D with the axes named (3-D where allowed: the third
    axis is added with extent 1), any strides with a contiguous class axis; y contiguous int64 [S] (None:
    the caller checks the labels later, with _labels) -> the 4-D view, its four extents, its three strides."""
    _want(logits, torch.float32, "logits")
    if allow_3d and logits.dim() == 3:
        logits = logits.unsqueeze(2)
    if logits.dim() != 4:
        ax = axes.split(", ")
        alt = f" or 3-D [{', '.join(ax[:2] + ax[3:])}]" if allow_3d else ""
        raise N.NativeError(f"{who}: logits must be 4-D [{axes}]{alt}, got {tuple(logits.shape)}")
    *strides, sc = logits.stride()
    if sc != 1 and logits.shape[3] > 1:
        raise N.NativeError(f"{who}: the class axis of logits must be contiguous, got stride {sc}")
    if y is not None:
        _labels(who, y, logits.shape[0])
    return logits, tuple(logits.shape), strides


def _out_tensor(who, name, t, dtype, shape, required=True, what=None):
    """An output tensor: None only where it is not required, else the dtype, the shape, contiguous.
    what: how the message words dtype and shape (default: 'f32' and the shape as a list)."""
    if t is None:
        if required:
            raise N.NativeError(f"{who}: {name} is required")
        return
    _want(t, dtype, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise N.NativeError(f"{who}: {name} must be contiguous {what or f'f32 {list(shape)}'}, got {tuple(t.shape)}")


def uncertainty_decompose(logits, y, stats, p_bar, member_nll=None, inv_temp=None):
    """logits f32 [S, K, T, C], any strides with a contiguous class axis (``lo.permute(2, 0, 1, 3)`` of the
    [K, T, B, C] ensemble logits is read in place), y int64 [S] -> stats f32 [S, UNC_NSTAT] (columns
    UNC_COLUMNS), p_bar f32 [S, C], member_nll f32 [S, K] or None (mmu_uncertainty_decompose).
    inv_temp f32 [K], finite and >= 0: member k's logits are multiplied by inv_temp[k] first
    (mmu_uncertainty_decompose_scaled); None calls the unscaled symbol."""
    who = "uncertainty_decompose"
    logits, (S, Km, T, C), (ss, sk, st) = _logit_stack(who, logits, y, "S, K, T, C")
    _out_tensor(who, "stats", stats, torch.float32, (S, UNC_NSTAT))
    _out_tensor(who, "p_bar", p_bar, torch.float32, (S, C))
    _out_tensor(who, "member_nll", member_nll, torch.float32, (S, Km), required=False)
    if inv_temp is None:
        _dev_check(logits, y, stats, p_bar, member_nll)
        N.call("mmu_uncertainty_decompose", _ptr(logits), ss, sk, st, _ptr(y), S, Km, T, C, _ptr(stats),
               _ptr(p_bar), _ptr(member_nll), _stream(logits))
        return
    _inv_temp_check(who, inv_temp, (Km,), "[K]")
    _dev_check(logits, y, stats, p_bar, member_nll, inv_temp)
    N.call("mmu_uncertainty_decompose_scaled", _ptr(logits), ss, sk, st, _ptr(y), S, Km, T, C, _ptr(stats),
           _ptr(p_bar), _ptr(member_nll), _ptr(inv_temp), _stream(logits))


TEMPERATURE_MAX_CANDIDATES = 64   # include/mmu.h mmu_temperature_nll: J <= 64


def temperature_nll(logits, y, inv_temp, nll, nll_sum=None):
    """The ensemble NLL under J candidate inverse-temperature vectors in one read of the logits
    (mmu_temperature_nll).  logits f32 [S, K, T, C] as uncertainty_decompose takes them, y int64 [S],
    inv_temp f32 [J, K] (finite, >= 0; J <= 64) -> nll f32 [S, J], nll_sum f64 [J] = sum_s nll[s, j] or
    None."""
    who = "temperature_nll"
    logits, (S, Km, T, C), (ss, sk, st) = _logit_stack(who, logits, y, "S, K, T, C")
    if inv_temp is None or inv_temp.dim() != 2:
        raise N.NativeError(f"{who}: inv_temp must be a 2-D f32 [J, K] table")
    J = inv_temp.shape[0]
    if not 1 <= J <= TEMPERATURE_MAX_CANDIDATES:
        raise N.NativeError(f"{who}: J = {J} candidates, must be 1 .. {TEMPERATURE_MAX_CANDIDATES}")
    _inv_temp_check(who, inv_temp, (J, Km), "[J, K]")
    _out_tensor(who, "nll", nll, torch.float32, (S, J), what=f"f32 [S, J] = [{S}, {J}]")
    _out_tensor(who, "nll_sum", nll_sum, torch.float64, (J,), required=False, what=f"f64 [J] = [{J}]")
    _dev_check(logits, y, inv_temp, nll, nll_sum)
    N.call("mmu_temperature_nll", _ptr(logits), ss, sk, st, _ptr(y), S, Km, T, C, _ptr(inv_temp), J, _ptr(nll),
           _ptr(nll_sum), _stream(logits))


# include/mmu.h MMU_ROB_*: the columns of robustness_summary's stats
ROB_COLUMNS = ("p_full", "dp_image", "dp_image_control", "sd_image_control", "dp_text", "dp_text_control",
               "sd_text_control", "js_image", "js_image_control", "js_text", "js_text_control", "hit_full",
               "hit_image", "hit_text", "acc_image_control", "acc_text_control")
ROB_NSTAT = len(ROB_COLUMNS)


def robustness_summary(logits, y, stats, per_variant=None):
    """logits f32 [S, V, K, C] (or [S, V, C]: K = 1), any strides with a contiguous class axis
    (``lo.transpose(0, 1)`` of the [V, B, C] robustness tensor is read in place), V = 3 + 2n, y int64 [S]
    -> stats f32 [S, ROB_NSTAT] (columns ROB_COLUMNS), per_variant f32 [S, 3, V] = (p_label, js, hit) or
    None (mmu_robustness_summary)."""
    who = "robustness_summary"
    logits, (S, V, Km, C), (ss, sv, sk) = _logit_stack(who, logits, y, "S, V, K, C", allow_3d=True)
    _out_tensor(who, "stats", stats, torch.float32, (S, ROB_NSTAT))
    _out_tensor(who, "per_variant", per_variant, torch.float32, (S, 3, V), required=False)
    _dev_check(logits, y, stats, per_variant)
    N.call("mmu_robustness_summary", _ptr(logits), ss, sv, sk, _ptr(y), S, V, Km, C, _ptr(stats), _ptr(per_variant),
           _stream(logits))


# include/mmu.h MMU_DIV_*: the columns of ensemble_diversity's pair table
DIV_COLUMNS = ("js", "disagree", "tau")
DIV_NPAIR = len(DIV_COLUMNS)
DIV_MAX_MEMBERS = 16   # include/mmu.h mmu_ensemble_diversity: 2 <= K <= 16
DIV_MAX_TOP = 1024     # and 0 <= top <= 1024


def ensemble_diversity(logits, y, pair, counts, member_arg, top=5, mute_true=True):
    """Pairwise member agreement of one batch of the ensemble (mmu_ensemble_diversity).  logits f32
    [S, K, T, C] as uncertainty_decompose takes them (or [S, K, C]: T = 1, the heads of a head model),
    y int64 [S] -> pair f32 [S, P, DIV_NPAIR] (columns DIV_COLUMNS; P = K (K - 1) / 2 pairs in
    itertools.combinations order), counts int32 [S, P, 4] = (conc, disc, tx, ty) or None, member_arg
    int32 [S, K].  top: the probabilities each member keeps for Kendall's tau (0: all); mute_true: the
    true class is zeroed first."""
    who = "ensemble_diversity"
    logits, (S, Km, T, C), (ss, sk, st) = _logit_stack(who, logits, None, "S, K, T, C", allow_3d=True)
    if not 2 <= Km <= DIV_MAX_MEMBERS:
        raise N.NativeError(f"{who}: K = {Km} members, must be 2 .. {DIV_MAX_MEMBERS}")
    if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= DIV_MAX_TOP:
        raise N.NativeError(f"{who}: top = {top!r} must be an integer 0 .. {DIV_MAX_TOP} (0: no truncation)")
    if not isinstance(mute_true, (bool, int)) or mute_true not in (0, 1):
        raise N.NativeError(f"{who}: mute_true = {mute_true!r} must be a bool")
    _labels(who, y, S)
    P = Km * (Km - 1) // 2
    _out_tensor(who, "pair", pair, torch.float32, (S, P, DIV_NPAIR), what=f"float32 {[S, P, DIV_NPAIR]}")
    _out_tensor(who, "counts", counts, torch.int32, (S, P, 4), required=False, what=f"int32 {[S, P, 4]}")
    _out_tensor(who, "member_arg", member_arg, torch.int32, (S, Km), what=f"int32 {[S, Km]}")
    _dev_check(logits, y, pair, counts, member_arg)
    N.call("mmu_ensemble_diversity", _ptr(logits), ss, sk, st, _ptr(y), S, Km, T, C, top, int(mute_true),
           _ptr(pair), _ptr(counts), _ptr(member_arg), _stream(logits))


# include/mmu.h MMU_RANK_*: the columns of rank_table's two outputs, its tiling and its limits
RANK_COLUMNS = ("lt0", "eq0", "lt1", "eq1")
RANK_NRANK = len(RANK_COLUMNS)
RANK_COUNT_COLUMNS = ("n1", "n0", "gt", "eq", "nan")
RANK_NCOUNT = len(RANK_COUNT_COLUMNS)
RANK_BLOCK_ROWS = 1024   # samples per block
RANK_TILE = 1024         # candidates per LDS tile
RANK_MAX_S = 1 << 20     # the sweep is O(S^2) per column
RANK_MAX_J = 65535


def rank_table(x, group, rank=None, counts=None):
    """The exact rank table of J score columns (mmu_rank_table).  x f32 [S, J], any positive strides
    that do not overlap (``t.t()`` of a [J, S] table is read in place), NaN allowed; group bool / uint8
    [S], non-zero = group 1 (the positives, the wrong samples).  rank: None (no table), True (allocated
    here) or an int32 [J, S, RANK_NRANK] tensor: per column and sample, how many samples of group 0 / 1
    score lower (lt0, lt1) and how many score the same, itself included (eq0, eq1), as IEEE f32 compares.
    counts: None (allocated here) or an int64 [J, RANK_NCOUNT] tensor to write.
    -> (rank or None, counts int64 [J, RANK_NCOUNT] = (n1, n0, gt, eq, nan))."""
    who = "rank_table"
    _want(x, torch.float32, "x")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise N.NativeError(f"{who}: x must be a non-empty 2-D [S, J] table, got {tuple(x.shape)}")
    S, J = x.shape
    if S > RANK_MAX_S or J > RANK_MAX_J:
        raise N.NativeError(f"{who}: [S, J] = [{S}, {J}] exceeds [{RANK_MAX_S}, {RANK_MAX_J}]")
    if group.dtype == torch.bool:
        group = group.view(torch.uint8)
    _want(group, torch.uint8, "group")
    if tuple(group.shape) != (S,) or not group.is_contiguous():
        raise N.NativeError(f"{who}: group must be contiguous bool / uint8 [S] = [{S}], got {tuple(group.shape)}")
    if rank is True:
        _dev_check(x, group)
        rank = torch.empty(J, S, RANK_NRANK, dtype=torch.int32, device=x.device)
    _out_tensor(who, "rank", rank, torch.int32, (J, S, RANK_NRANK), required=False,
                what=f"int32 {[J, S, RANK_NRANK]}")
    _out_tensor(who, "counts", counts, torch.int64, (J, RANK_NCOUNT), required=False,
                what=f"int64 {[J, RANK_NCOUNT]}")
    _dev_check(x, group, rank, counts)
    if counts is None:
        counts = torch.empty(J, RANK_NCOUNT, dtype=torch.int64, device=x.device)
    N.call("mmu_rank_table", _ptr(x), x.stride(0), x.stride(1), _ptr(group), S, J, _ptr(rank), _ptr(counts),
           _stream(x))
    return rank, counts


_alg = {"on": False, "bytes": 0.0, "n": 0}


_seed_counter = None


def set_seed_offset(counter):
    """Dropout seeds under HIP-graph replay (include/mmu.h mmu_set_seed_offset): ``counter`` = a
    1-element int64 device tensor every later dropout launch folds into its seed when it runs
    (None = off).  The tensor is kept referenced here while it is set."""
    global _seed_counter
    if counter is not None:
        _want(counter, torch.int64, "seed counter")
        if counter.numel() != 1 or not counter.is_cuda:
            raise N.NativeError("seed counter: a 1-element int64 CUDA tensor")
    _seed_counter = counter
    N.call("mmu_set_seed_offset", _ptr(counter) if counter is not None else None)


def timing_enable(on=True):
    """HIP-event timing of every mmu_gemm launch (and a count of its algorithmic bytes)."""
    N.call("mmu_timing_enable", int(on))
    _alg.update(on=bool(on), bytes=0.0, n=0)


class timing_paused:
    """Context: mmu_gemm launches inside are neither event-timed nor counted (bench.py's
    GEMM roofline covers the BERT-layer products only)."""

    def __enter__(self):
        self.was = _alg["on"]
        if self.was:
            N.call("mmu_timing_pause", 1)
            _alg["on"] = False
        return self

    def __exit__(self, *exc):
        if self.was:
            N.call("mmu_timing_pause", 0)
            _alg["on"] = True
        return False


def timing_read():
    ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    N.call("mmu_timing_read", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
    return ms.value, n.value, fl.value


def timing_alg_bytes():
    """(algorithmic HBM bytes, launches) of the timed GEMMs: operands read once, C written
    once (read too when accumulating), residual / aux streams of the fused epilogues."""
    return _alg["bytes"], _alg["n"]


def _count_alg(M, N_, K, batch, c_bytes, epi):
    b = 2.0 * (M * K + N_ * K) + c_bytes * M * N_
    if epi is not None:
        if epi.accumulate:
            b += c_bytes * M * N_
        if epi.residual:  # f32 residual with an f32 BIAS_DROP_RES output (the hidden stream)
            b += (4.0 if (c_bytes == 4 and epi.kind == EPI_BIAS_DROP_RES) else 2.0) * M * N_
        if epi.aux:
            b += 2.0 * M * N_
    _alg["bytes"] += b * batch
    _alg["n"] += 1
