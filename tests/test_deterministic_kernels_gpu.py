"""Deterministic mode (include/mmu.h mmu_set_deterministic; src/kernels.py deterministic()): every
replacement of a float-atomic site against float64 of the same inputs, and 8 consecutive calls on
identical inputs bit for bit.

* embedding backward (csrc/embed.hip: embed_bwd_rows_kernel<true>, the radix sort, the segmented
  sum's chunk and carry kernels, the position fold): the shapes, id kinds and bars of
  test_embed_edges_gpu.py (rowops_harness: every f32 output within 8 x the float32 model's error or
  4 ulps of its scale), gradient buffers zero-filled and pre-filled; B * T around the chunk size
  read from the library; one run of equal ids over five chunks.
* column fold (csrc/gemm.hip colsum_fold_det_kernel / _multi_): bar parts * 2^-23 * sum|addend| per
  column (addends: the partial rows, and the output's initial value when accumulating).  An f32 sum
  of n addends in any order is within (n - 1) 2^-24 (1 + O(2^-24)) sum|addend| of the exact sum, so
  the bar holds twice that; _check_bar_on_cpu asserts it on a NumPy f32 sequential sum first.
* the GEMM's column sums (DGELU epilogue) with MMU_GEMM_CS_PART=0 in the environment, at the
  tolerance test_kernels_gpu.py::test_gemm_colsum_partial_rows_match_atomics holds the same sums to;
  batch > 1 with a colsum must raise.
* colsum_bf16 and the ECE bins.
* mode off: the atomic path still meets the same bars, and the context manager restores the flag.
"""
import numpy as np
import pytest
import torch

import rowops_harness as R
from guarded import check_written, out_buf

pytestmark = pytest.mark.gpu

EPS = 1e-12
bf16, f32t = torch.bfloat16, torch.float32
REPEATS = 8
U23 = 2.0 ** -23


def K():
    from src import kernels
    return kernels


def to_dev(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------- embedding backward
def _embed_fwd(k, dev, d, B, T, n_img, seed, pi, pt, ln=None):
    S = n_img + 2 + T
    rows = B * S
    X = torch.empty(rows, 768, dtype=bf16, device=dev)
    X32 = torch.empty(rows, 768, dtype=f32t, device=dev)
    km = torch.empty(B, S, dtype=f32t, device=dev)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    lw, lb = ln if ln is not None else (d["ln_w"], d["ln_b"])
    k.embed_fwd(d["ids"], d["seg"], d["txt_mask"], d["proj"], d["word"], d["pos"], d["typ"], lw, lb, EPS, d["cls_id"],
                d["sep_id"], None, 1, B, T, n_img, S, X, km, mean, rstd, drop_txt=pt, drop_img=pi, seed=seed, X32=X32)
    return X32, mean, rstd


def _keep(k, dev, d, B, T, n_img, seed, pi, pt):
    """the forward's keep bits from the forward itself (ln_w = 0, ln_b = 1: every output is 0 or 1/(1-p))"""
    X32, _, _ = _embed_fwd(k, dev, d, B, T, n_img, seed, pi, pt,
                           ln=(torch.zeros(768, device=dev), torch.ones(768, device=dev)))
    return X32 != 0


def _embed_bwd_case(k, dev, B, T, n_img, ids_kind, seg_kind, drop, prefill, fails, repeats=REPEATS, data_seed=None):
    S = n_img + 2 + T
    d = to_dev(R.embed_inputs(B, T, n_img, seed=13 * B + T if data_seed is None else data_seed, ids_kind=ids_kind,
                              seg_kind=seg_kind), dev)
    params = (d["word"], d["pos"], d["typ"], d["ln_w"], d["ln_b"])
    pi, pt = (R.DROP_IMG, R.DROP_TXT) if drop else (0.0, 0.0)
    seed = 0xDE70000 + 7 * B + T
    keep = _keep(k, dev, d, B, T, n_img, seed, pi, pt) if drop else None
    _, mean, rstd = _embed_fwd(k, dev, d, B, T, n_img, seed, pi, pt)
    tag = f"B={B} T={T} n_img={n_img} ids={ids_kind} seg={seg_kind} drop={drop} prefill={prefill} det={k.is_deterministic()}"
    gen = torch.Generator().manual_seed(B + T)
    init = {n: ((torch.randn(t.shape, generator=gen) * 0.1).to(dev) if prefill else torch.zeros_like(t))
            for n, t in zip(R.GRADS[:5], params)}
    first = None
    for rep in range(repeats):
        bufs, outs = {}, {}
        for n, t in zip(R.GRADS, params + (d["proj"],)):
            bufs[n], outs[n] = out_buf(dev, f32t, *t.shape)
            if n != "d_proj":  # (d_proj stays NaN-filled: it is overwritten, not accumulated)
                outs[n].copy_(init[n])
        k.embed_bwd(d["dX"], d["ids"], d["seg"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"], mean, rstd,
                    d["cls_id"], d["sep_id"], B, T, n_img, *(outs[n] for n in R.GRADS), drop_txt=pt, drop_img=pi,
                    seed=seed)
        torch.cuda.synchronize()
        check_written(bufs, fails, f"{tag} call {rep}")
        if first is None:
            first = {n: outs[n].clone() for n in R.GRADS}
        else:
            for n in R.GRADS:
                if not torch.equal(outs[n], first[n]):
                    fails.append(f"{tag} {n}: call {rep} differs from call 0 by "
                                 f"{(outs[n] - first[n]).abs().max().item():.3e}")
    bargs = (d["dX"], d["ids"], d["seg"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"])
    ref, sc = R.embed_bwd_ref(*bargs, d["ln_b"], EPS, d["cls_id"], d["sep_id"], B, T, n_img, keep=keep, drop_txt=pt,
                              drop_img=pi, init=init)
    m = R.embed_bwd_model(*bargs, mean, rstd, d["cls_id"], d["sep_id"], B, T, n_img, keep=keep, drop_txt=pt,
                          drop_img=pi, init=init)
    log = []
    for n in R.GRADS:
        R.check_f32(f"{tag} {n}", first[n], m[n], ref[n], sc[n], fails, log)
    print("\n".join(log))


@pytest.mark.parametrize("n_img", R.EMBED_N_IMG)
@pytest.mark.parametrize("B", (1, 16, 17, 33))
def test_embed_backward_deterministic(dev, B, n_img):
    k = K()
    fails = []
    with k.deterministic():
        for ti, T in enumerate(R.EMBED_BWD_T):
            for ci, (ids_kind, seg_kind) in enumerate(R.EMBED_BWD_KINDS):
                for drop in (True, False):
                    # zero-filled and pre-filled buffers: both for the first T, then rotating
                    for prefill in ((False, True) if ti == 0 else ((ci + drop) % 2 == 1,)):
                        _embed_bwd_case(k, dev, B, T, n_img, ids_kind, seg_kind, drop, prefill, fails)
    assert not k.is_deterministic()
    assert not fails, "\n".join(fails)


def _shape_of(tokens):
    """(B, T) with B * T == tokens, T <= 17 where a factor allows"""
    for T in range(17, 0, -1):
        if tokens % T == 0:
            return tokens // T, T
    raise AssertionError(tokens)


def test_embed_backward_chunk_boundaries(dev):
    """B * T = chunk - 1, chunk, chunk + 1 tokens of the segmented sum (the constant is the library's):
    one run that ends just before, at, and one token past the first chunk's end ("equal"), and
    mostly single-row runs around it ("random")"""
    k = K()
    chunk = k.embed_bwd_det_chunk()
    assert chunk >= 2
    fails = []
    with k.deterministic():
        for tokens in (chunk - 1, chunk, chunk + 1):
            B, T = _shape_of(tokens)
            for ids_kind, seg_kind in (("equal", "ones"), ("random", "mixed")):
                _embed_bwd_case(k, dev, B, T, 1, ids_kind, seg_kind, True, tokens == chunk, fails)
    assert not fails, "\n".join(fails)


def test_embed_backward_one_run_over_many_chunks(dev):
    """all ids equal over more than 4 chunks: the carry pass folds at least three carry rows behind
    the first; and "special", whose [CLS] / [SEP] runs cross chunks and meet the position sums"""
    k = K()
    chunk = k.embed_bwd_det_chunk()
    B, T = (4 * chunk + 16) // 17 + 1, 17
    assert B * T > 4 * chunk
    fails = []
    with k.deterministic():
        for ids_kind, seg_kind in (("equal", "mixed"), ("special", "zeros")):
            for prefill in (False, True):
                _embed_bwd_case(k, dev, B, T, 3, ids_kind, seg_kind, True, prefill, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------- column fold
def _check_bar_on_cpu(part, init, ref64, bar):
    """the bar's premise, on this very data: a NumPy f32 sum taken row after row is inside it"""
    s = init.astype(np.float32).copy()
    for r in range(part.shape[0]):
        s = (s + part[r]).astype(np.float32)
    assert (np.abs(s.astype(np.float64) - ref64) <= bar).all(), "the bar does not hold an f32 sequential sum"


def _fold_data(parts, N, seed, accumulate):
    g = torch.Generator().manual_seed(seed)
    part = torch.randn(parts, N, generator=g) * (10.0 ** (torch.rand(parts, 1, generator=g) * 2 - 1))
    init = torch.randn(N, generator=g) if accumulate else torch.zeros(N)
    ref = part.double().sum(0) + init.double()
    bar = parts * U23 * (part.double().abs().sum(0) + init.double().abs())
    _check_bar_on_cpu(part.numpy(), init.numpy(), ref.numpy(), bar.numpy())
    return part, init, ref, bar


FOLD_PARTS = (1, 15, 16, 17, 64, 65, 1026)
FOLD_N = (8, 768, 3072)


def _run_fold(k, dev, jobs_cpu, accumulate, fails, tag, repeats=REPEATS):
    """jobs_cpu: [(part, init, ref, bar)] of one N -> the first call's outputs; repeats compared bit for bit"""
    parts_dev = [p.to(dev) for p, _, _, _ in jobs_cpu]
    first = None
    for rep in range(repeats):
        bufs, outs = {}, []
        for z, (_, init, _, _) in enumerate(jobs_cpu):
            g, o = out_buf(dev, f32t, init.numel())  # NaN-filled: a fold that does not accumulate must overwrite
            if accumulate:
                o.copy_(init)
            bufs[f"out{z}"] = g
            outs.append(o)
        if len(jobs_cpu) == 1 and rep % 2 == 0:
            k.colsum_reduce(parts_dev[0], outs[0], accumulate=accumulate)
        else:
            k.colsum_reduce_multi(list(zip(parts_dev, outs)), accumulate=accumulate)
        torch.cuda.synchronize()
        check_written(bufs, fails, f"{tag} call {rep}")
        if first is None:
            first = [o.clone() for o in outs]
        elif not all(torch.equal(a, b) for a, b in zip(outs, first)):
            fails.append(f"{tag}: call {rep} differs from call 0")
    for z, (_, _, ref, bar) in enumerate(jobs_cpu):
        err = (first[z].double().cpu() - ref).abs()
        worst = (err / bar.clamp_min(1e-300)).max().item() if (bar > 0).all() else float("inf")
        print(f"{tag} job {z}: worst error {err.max().item():.3e}, {worst:.3f} of the bar")
        if not (err <= bar).all():
            fails.append(f"{tag} job {z}: error {worst:.3f} x the bar")
    return first


@pytest.mark.parametrize("N", FOLD_N)
def test_column_fold_deterministic(dev, N):
    """colsum_reduce (and, on odd calls, the same job through colsum_reduce_multi: equal bits, one
    body) for every parts, accumulate on and off"""
    k = K()
    fails = []
    with k.deterministic():
        for parts in FOLD_PARTS:
            for accumulate in (False, True):
                job = _fold_data(parts, N, 1000 * parts + N, accumulate)
                _run_fold(k, dev, [job], accumulate, fails, f"fold parts={parts} N={N} acc={accumulate}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N", FOLD_N)
def test_column_fold_multi_deterministic(dev, N):
    """4 jobs of unequal parts in one launch"""
    k = K()
    fails = []
    with k.deterministic():
        for group in ((1, 15, 16, 17), (64, 65, 1026, 1), (1026, 17, 65, 16)):
            for accumulate in (False, True):
                jobs = [_fold_data(p, N, 77 * p + N + z, accumulate) for z, p in enumerate(group)]
                _run_fold(k, dev, jobs, accumulate, fails, f"multi parts={group} N={N} acc={accumulate}")
    assert not fails, "\n".join(fails)


def test_column_fold_unaligned_partials(dev):
    """partial rows 4 B off a 16-B boundary take the 4-B walk: same bar, same repeatability"""
    k = K()
    fails = []
    with k.deterministic():
        part, init, ref, bar = _fold_data(65, 768, 5, True)
        big = torch.empty(65 * 768 + 1, device=dev)
        big[1:].copy_(part.reshape(-1))
        first = None
        for rep in range(REPEATS):
            o = init.to(dev)
            k.colsum_reduce(big[1:].view(65, 768), o, accumulate=True)
            first = o.clone() if first is None else first
            assert torch.equal(o, first)
        assert ((first.double().cpu() - ref).abs() <= bar).all()
    assert not fails


# ------------------------------------------------------------------------------- GEMM column sums
def _rnd(*shape, seed, scale=1.0, dev=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(bf16).to(dev)


@pytest.mark.parametrize("cs_part_env", (None, "0"))
@pytest.mark.parametrize("N", (256, 768))
@pytest.mark.parametrize("M", (64, 129, 513))
def test_gemm_colsum_deterministic(dev, monkeypatch, M, N, cs_part_env):
    """M = 513 runs the 256 x 256 tiling, 64 and 129 the small one.  MMU_GEMM_CS_PART=0 asks for the
    atomic epilogue: the mode overrides it (8 equal results; the atomics' order is free)."""
    k = K()
    if cs_part_env is None:
        monkeypatch.delenv("MMU_GEMM_CS_PART", raising=False)
    else:
        monkeypatch.setenv("MMU_GEMM_CS_PART", cs_part_env)
    Kd = 128
    A, Bm = _rnd(M, Kd, seed=171, dev=dev), _rnd(N, Kd, seed=172, scale=0.1, dev=dev)
    aux = (torch.rand(M, N, generator=torch.Generator().manual_seed(3)) + 0.5).to(bf16).to(dev)
    dg = (A.double() @ Bm.double().t()) * aux.double()
    want = dg.sum(0) + 1.0
    first = None
    with k.deterministic():
        for rep in range(REPEATS):
            o, cs = torch.empty(M, N, dtype=bf16, device=dev), torch.full((N,), 1.0, device=dev)
            k.gemm(A, Kd, True, Bm, Kd, True, o, N, M, N, Kd, epi=k.epilogue(k.EPI_DGELU, aux=aux, colsum=cs))
            torch.cuda.synchronize()
            if first is None:
                first = (o.clone(), cs.clone())
            assert torch.equal(o, first[0]) and torch.equal(cs, first[1]), f"call {rep} differs from call 0"
    print(f"M={M} N={N}: worst column-sum error {(first[1].double() - want).abs().max().item():.3e}")
    torch.testing.assert_close(first[1].double(), want, rtol=2e-3, atol=2e-3 * dg.abs().sum(0).max().item())
    torch.testing.assert_close(first[0].double(), dg, rtol=1e-2, atol=1e-2 * dg.abs().max().item())


def test_gemm_colsum_batched_is_refused(dev):
    """batch > 1 with a plain colsum has no partial-row path: in the mode it raises, and the colsum
    buffer is left alone; with the mode off the same call runs"""
    from src._native import NativeError
    k = K()
    M, N, Kd, batch = 128, 128, 64, 2
    A, Bm = _rnd(batch * M, Kd, seed=1, dev=dev), _rnd(batch * N, Kd, seed=2, dev=dev)
    aux = torch.ones(batch * M, N, dtype=bf16, device=dev)
    o, cs = torch.empty(batch * M, N, dtype=bf16, device=dev), torch.zeros(batch * N, device=dev)
    kw = dict(batch=batch, sA=M * Kd, sB=N * Kd, sC=M * N)

    def call():
        k.gemm(A, Kd, True, Bm, Kd, True, o, N, M, N, Kd,
               epi=k.epilogue(k.EPI_DGELU, aux=aux, aux_bstride=M * N, colsum=cs, colsum_bstride=N), **kw)
    with k.deterministic():
        with pytest.raises(NativeError, match="deterministic"):
            call()
        torch.cuda.synchronize()
        assert (cs == 0).all()
    call()
    torch.cuda.synchronize()
    want = (A.double().view(batch, M, Kd) @ Bm.double().view(batch, N, Kd).transpose(1, 2)).sum(1).reshape(-1)
    torch.testing.assert_close(cs.double(), want, rtol=2e-3, atol=2e-3 * want.abs().max().item())


# ------------------------------------------------------------------------------- colsum_bf16
@pytest.mark.parametrize("N", (8, 768))
@pytest.mark.parametrize("M", (63, 64, 65, 2049))
def test_colsum_bf16_deterministic(dev, M, N):
    from src import _native as Nat
    k = K()
    X = _rnd(M, N, seed=M + N, dev=dev)
    fails = []
    with k.deterministic():
        for accumulate in (False, True):
            init = torch.randn(N, generator=torch.Generator().manual_seed(9)) if accumulate else torch.zeros(N)
            ref = X.double().sum(0).cpu() + init.double()
            bar = M * U23 * (X.double().abs().sum(0).cpu() + init.double().abs())
            for scratch in (True, False):
                first = None
                for rep in range(REPEATS):
                    g, o = out_buf(dev, f32t, N)
                    if accumulate:
                        o.copy_(init)
                    if scratch:
                        k.colsum_bf16(X, o, accumulate=accumulate)
                    elif M > 1024:  # more than one row block and no table: refused, nothing written
                        with pytest.raises(Nat.NativeError, match="deterministic"):
                            Nat.call("mmu_colsum_bf16", X.data_ptr(), M, N, X.stride(0), None, o.data_ptr(),
                                     int(accumulate), torch.cuda.current_stream().cuda_stream)
                        break
                    else:
                        Nat.call("mmu_colsum_bf16", X.data_ptr(), M, N, X.stride(0), None, o.data_ptr(),
                                 int(accumulate), torch.cuda.current_stream().cuda_stream)
                    torch.cuda.synchronize()
                    check_written({"out": g}, fails, f"M={M} N={N} acc={accumulate} scratch={scratch} call {rep}")
                    first = o.clone() if first is None else first
                    if not torch.equal(o, first):
                        fails.append(f"M={M} N={N} acc={accumulate} scratch={scratch}: call {rep} differs")
                if first is not None and not ((first.double().cpu() - ref).abs() <= bar).all():
                    fails.append(f"M={M} N={N} acc={accumulate} scratch={scratch}: outside the bar")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------- ECE bins
def _ece_inputs(S, n_bins, seed):
    """conf with exact 0, exact 1 and values exactly on bin edges among random ones"""
    g = torch.Generator().manual_seed(seed)
    conf = torch.rand(S, generator=g)
    edges = [0.0, 1.0] + [b / n_bins for b in range(1, n_bins)]
    for i, e in enumerate(edges):
        if i < S:
            conf[(7 * i) % S] = e
    correct = (torch.rand(S, generator=g) < 0.6).float()
    return conf, correct


@pytest.mark.parametrize("n_bins", (1, 10, 15))
@pytest.mark.parametrize("S", (1, 63, 64, 65, 1000))
def test_ece_bins_deterministic(dev, S, n_bins):
    k = K()
    conf, correct = _ece_inputs(S, n_bins, 31 * S + n_bins)
    # the kernel's own binning rule in f32: bin = ceil(conf * n_bins) - 1, clamped
    b = (torch.ceil(conf * torch.tensor(float(n_bins))) - 1).clamp(0, n_bins - 1).long()
    cnt = torch.zeros(n_bins, dtype=torch.float64).index_add_(0, b, torch.ones(S, dtype=torch.float64))
    sc = torch.zeros(n_bins, dtype=torch.float64).index_add_(0, b, conf.double())
    sk = torch.zeros(n_bins, dtype=torch.float64).index_add_(0, b, correct.double())
    bar_c = S * U23 * torch.zeros(n_bins, dtype=torch.float64).index_add_(0, b, conf.double().abs())
    cd, kd = conf.to(dev), correct.to(dev)
    first, fails = None, []
    with k.deterministic():
        for rep in range(REPEATS):
            g, out = out_buf(dev, f32t, n_bins, 3)
            k.ece_bins(cd, kd, n_bins, out)
            torch.cuda.synchronize()
            check_written({"bins": g}, fails, f"call {rep}")
            first = out.clone() if first is None else first
            assert torch.equal(out, first), f"call {rep} differs from call 0"
    got = first.double().cpu()
    assert not fails, "\n".join(fails)
    assert torch.equal(got[:, 0], cnt), (got[:, 0], cnt)
    assert torch.equal(got[:, 2], sk), "sums of 0 / 1 flags are exact below 2^24"
    assert ((got[:, 1] - sc).abs() <= bar_c).all(), (got[:, 1] - sc, bar_c)


# ------------------------------------------------------------------------------- mode off
def test_mode_off_is_untouched(dev):
    """the default path (float atomics) still meets the same bars, and leaving the context manager
    leaves the mode off"""
    k = K()
    with k.deterministic():
        assert k.is_deterministic()
    assert k.is_deterministic() is False
    fails = []
    _embed_bwd_case(k, dev, 17, 9, 3, "special", "zeros", True, True, fails, repeats=1)
    job = _fold_data(65, 768, 11, True)
    _run_fold(k, dev, [job], True, fails, "mode off fold", repeats=1)
    job = _fold_data(1026, 768, 12, False)
    _run_fold(k, dev, [job], False, fails, "mode off fold", repeats=1)
    assert k.is_deterministic() is False
    assert not fails, "\n".join(fails)
