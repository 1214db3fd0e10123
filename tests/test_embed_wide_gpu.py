"""The embedding kernels at H = 1024 (csrc/embed.hip, the NV = 4 instantiations: embed_fwd_kernel,
embed_bwd_rows_kernel, the deterministic mode's chunk / carry / position kernels) against float64,
through guarded outputs, with both dropouts on: the twin of test_embed_edges_gpu.py (H = 768, which
stays the guard of that width) on the same shapes, index sets, id / segment kinds and bars.

Bars: rowops_harness (X: elementwise and row error against the float32 model; every f32 output
within 8 x the model's error or 4 ulps of its scale).  Deterministic mode: the same backward cases,
each run twice (bitwise equal) and held to the same bars; one case with B T over the segmented sum's
chunk and all ids equal, so that one word row's sum crosses chunk carries.  One H = 768 case per
direction runs through the same code here (the shared template still serves 768), and a 512-wide
call is refused by name.

Measured on an MI355X over the whole H = 1024 sweep (run with -s for every case's figures):
  X (bf16): elementwise 0.995 of the bar; kernel / model row error 1.000 (max)
  f32 outputs, worst share of the bar: X32 0.17, mean 0.03, rstd 0.31, d_word 0.35, d_pos 0.37,
      d_type 0.19, d_ln_w 0.22, d_ln_b 0.22, d_proj 0.16 (deterministic mode included)
  all per-segment drop rates within 4 sigma of 0.3 / 0.1; key mask exact; no guard written
"""
import math

import pytest
import torch

import rowops_harness as R
from guarded import check_written, out_buf
from rowops_harness import Worst

pytestmark = pytest.mark.gpu

EPS = 1e-12
WIDE = 1024
bf16, f32t = torch.bfloat16, torch.float32
DROP_IMG, DROP_TXT = R.DROP_IMG, R.DROP_TXT


def K():
    from src import kernels
    return kernels


def to_dev(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def run_fwd(k, dev, d, idx, V, B, T, n_img, Lout, seed, pi, pt, x32=True, stats=True, ln=None):
    """embed_fwd into NaN-filled guarded outputs -> (X, X32, keymask, mean, rstd, bufs)"""
    H = d["word"].shape[1]
    rows = V * B * Lout
    bufs = {}
    bufs["X"], X = out_buf(dev, bf16, rows, H)
    bufs["keymask"], km = out_buf(dev, f32t, V * B, Lout)
    X32 = mean = rstd = None
    if x32:
        bufs["X32"], X32 = out_buf(dev, f32t, rows, H)
    if stats:
        bufs["mean"], mean = out_buf(dev, f32t, rows)
        bufs["rstd"], rstd = out_buf(dev, f32t, rows)
    lw, lb = ln if ln is not None else (d["ln_w"], d["ln_b"])
    k.embed_fwd(d["ids"], d["seg"], d["txt_mask"], d["proj"], d["word"], d["pos"], d["typ"], lw, lb, EPS, d["cls_id"],
                d["sep_id"], idx, V, B, T, n_img, Lout, X, km, mean, rstd, drop_txt=pt, drop_img=pi, seed=seed,
                X32=X32)
    torch.cuda.synchronize()
    return X, X32, km, mean, rstd, bufs


def probe_keep(k, dev, d, idx, V, B, T, n_img, Lout, seed, pi, pt):
    """the forward's keep bits from the forward itself: ln_w = 0, ln_b = 1 -> X32 is exactly
    1/(1-p) of the row's segment (kept) or 0 (dropped)"""
    H = d["word"].shape[1]
    ln = (torch.zeros(H, device=dev), torch.ones(H, device=dev))
    _, X32, _, _, _, _ = run_fwd(k, dev, d, idx, V, B, T, n_img, Lout, seed, pi, pt, ln=ln)
    src = R.embed_layout(B, T, n_img, idx, V, Lout, device=dev)
    is_img = (src <= n_img + 1).unsqueeze(1).expand(V, B, src.shape[1]).reshape(-1, 1)
    zi = (1.0 / (1.0 - torch.tensor(pi, dtype=f32t))).item() if pi > 0 else 1.0
    zt = (1.0 / (1.0 - torch.tensor(pt, dtype=f32t))).item() if pt > 0 else 1.0
    want = torch.where(is_img, torch.full_like(X32, zi), torch.full_like(X32, zt))
    # (2 ulps: the kernel's own f32 reciprocal of 1 - p)
    assert ((X32 == 0) | ((X32 - want).abs() <= 2.0 ** -22 * want)).all(), \
        "probe: an output is neither 0 nor 1/(1-p) of its segment"
    return X32 != 0, is_img.view(-1)


def fwd_args(d, idx, V, B, T, n_img, Lout):
    return (d["ids"], d["seg"], d["txt_mask"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"], d["ln_b"], EPS,
            d["cls_id"], d["sep_id"], idx, V, B, T, n_img, Lout)


def forward_case(k, dev, B, T, n_img, H, fails, worst):
    d = to_dev(R.embed_inputs(B, T, n_img, seed=31 * B + T + n_img, H=H), dev)
    for vname, idx, V, Lout in R.embed_fwd_variants(B, T, n_img):
        idx = None if idx is None else idx.to(dev)
        args = fwd_args(d, idx, V, B, T, n_img, Lout)
        src = R.embed_layout(B, T, n_img, idx, V, Lout, device=dev)
        for drop in (False, True):
            pi, pt = (DROP_IMG, DROP_TXT) if drop else (0.0, 0.0)
            seed = 0xE3B0000 + 17 * B + T
            keep = None
            if drop:
                keep, is_img = probe_keep(k, dev, d, idx, V, B, T, n_img, Lout, seed, pi, pt)
                for name, sel, p in (("image segment", is_img, pi), ("text", ~is_img, pt)):
                    n = keep[sel].numel()
                    if n == 0:  # (a gather that holds no row of this segment)
                        continue
                    rate, tol = 1.0 - keep[sel].float().mean().item(), 4.0 * math.sqrt(p * (1 - p) / n)
                    print(f"[H={H} {vname} B={B} T={T} n_img={n_img}] {name} drop rate {rate:.4f} (p {p} +- {tol:.4f})")
                    if abs(rate - p) > tol:
                        fails.append(f"{vname} {name}: drop rate {rate:.4f} not within {tol:.4f} of {p}")
            ref, sc = R.embed_fwd_ref(*args, keep=keep, drop_txt=pt, drop_img=pi)
            m = R.embed_fwd_model(*args, keep=keep, drop_txt=pt, drop_img=pi)
            for x32, stats in ((True, True), (False, False)):
                tag = f"H={H} {vname} B={B} T={T} n_img={n_img} drop={drop} x32={x32} stats={stats}"
                log = []
                X, X32, km, mean, rstd, bufs = run_fwd(k, dev, d, idx, V, B, T, n_img, Lout, seed, pi, pt, x32, stats)
                check_written(bufs, fails, tag)
                worst.bf("X", *R.check_bf16(f"{tag} X", X, m["X"], ref["X"], sc["X"], fails, log))
                if x32:
                    worst.f32("X32", *R.check_f32(f"{tag} X32", X32, m["X32"], ref["X"], sc["X"], fails, log))
                if stats:
                    worst.f32("mean", *R.check_f32(f"{tag} mean", mean, m["mean"], ref["mean"], sc["mean"], fails, log))
                    worst.f32("rstd", *R.check_f32(f"{tag} rstd", rstd, m["rstd"], ref["rstd"], sc["rstd"], fails, log))
                if drop and not ((X[~keep] == 0).all() and (X32 is None or (X32[~keep] == 0).all())):
                    fails.append(f"{tag}: a dropped element is not exactly zero")
                # key mask: exactly -10000 on text rows whose txt_mask is 0, exactly 0 elsewhere
                if not torch.equal(km.reshape(-1).double(), ref["keymask"]):
                    fails.append(f"{tag}: key mask differs from 0 / -10000")
                img_cols = (src <= n_img + 1).unsqueeze(1).expand(V, B, Lout).reshape(V * B, Lout)
                if not (km[img_cols] == 0).all():
                    fails.append(f"{tag}: key mask not 0 on an image-segment row")
                print("\n".join(log))


@pytest.mark.parametrize("n_img", R.EMBED_N_IMG)
@pytest.mark.parametrize("B,T", R.EMBED_FWD_SHAPES)
def test_embed_forward_wide(dev, B, T, n_img):
    fails, worst = [], Worst()
    forward_case(K(), dev, B, T, n_img, WIDE, fails, worst)
    worst.report(f"embed fwd H={WIDE} B={B} T={T} n_img={n_img}")
    assert not fails, "\n".join(fails)


def backward_case(k, dev, B, T, n_img, H, ids_kind, seg_kind, drop, prefill, fails, worst, data_seed, repeats=1):
    """embed_bwd into guarded gradient buffers, `repeats` times on the same inputs (each bitwise the
    first), against the float64 reference and the float32 model, with the keep bits of a probe call"""
    S = n_img + 2 + T
    d = to_dev(R.embed_inputs(B, T, n_img, seed=data_seed, H=H, ids_kind=ids_kind, seg_kind=seg_kind), dev)
    params = (d["word"], d["pos"], d["typ"], d["ln_w"], d["ln_b"])
    pi, pt = (DROP_IMG, DROP_TXT) if drop else (0.0, 0.0)
    seed = 0xEB0000 + 7 * B + T
    keep = probe_keep(k, dev, d, None, 1, B, T, n_img, S, seed, pi, pt)[0] if drop else None
    _, _, _, mean, rstd, _ = run_fwd(k, dev, d, None, 1, B, T, n_img, S, seed, pi, pt)
    bargs = (d["dX"], d["ids"], d["seg"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"])
    tag = (f"H={H} B={B} T={T} n_img={n_img} ids={ids_kind} seg={seg_kind} drop={drop} prefill={prefill} "
           f"det={k.is_deterministic()}")
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
    ref, sc = R.embed_bwd_ref(*bargs, d["ln_b"], EPS, d["cls_id"], d["sep_id"], B, T, n_img, keep=keep, drop_txt=pt,
                              drop_img=pi, init=init)
    m = R.embed_bwd_model(*bargs, mean, rstd, d["cls_id"], d["sep_id"], B, T, n_img, keep=keep, drop_txt=pt,
                          drop_img=pi, init=init)
    log = []
    for n in R.GRADS:
        worst.f32(n, *R.check_f32(f"{tag} {n}", first[n], m[n], ref[n], sc[n], fails, log))
    print("\n".join(log))


def backward_sweep(k, dev, B, n_img, H, fails, worst, repeats=1):
    """T, (ids, seg) kinds, dropouts on and off, zero-filled and pre-filled gradient buffers (rotating:
    one of the two per case, both for the first T) -- the sweep of test_embed_edges_gpu.py"""
    for ti, T in enumerate(R.EMBED_BWD_T):
        for ci, (ids_kind, seg_kind) in enumerate(R.EMBED_BWD_KINDS):
            for drop in (True, False):
                for prefill in ((False, True) if ti == 0 else ((ci + drop) % 2 == 1,)):
                    backward_case(k, dev, B, T, n_img, H, ids_kind, seg_kind, drop, prefill, fails, worst,
                                  13 * B + T + ci, repeats)


@pytest.mark.parametrize("n_img", R.EMBED_N_IMG)
@pytest.mark.parametrize("B", R.EMBED_BWD_B)
def test_embed_backward_wide(dev, B, n_img):
    k = K()
    assert not k.is_deterministic()
    fails, worst = [], Worst()
    backward_sweep(k, dev, B, n_img, WIDE, fails, worst)
    worst.report(f"embed bwd H={WIDE} B={B} n_img={n_img}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n_img", R.EMBED_N_IMG)
@pytest.mark.parametrize("B", R.EMBED_BWD_B)
def test_embed_backward_wide_deterministic(dev, B, n_img):
    """the same cases with the mode on: two calls bitwise equal, both within the bars"""
    k = K()
    fails, worst = [], Worst()
    with k.deterministic():
        backward_sweep(k, dev, B, n_img, WIDE, fails, worst, repeats=2)
    assert not k.is_deterministic()
    worst.report(f"embed bwd deterministic H={WIDE} B={B} n_img={n_img}")
    assert not fails, "\n".join(fails)


def test_embed_backward_wide_one_run_over_chunks(dev):
    """deterministic mode, all ids equal over more than two chunks of the segmented sum (the constant
    is the library's): the one word row's sum goes through the chunks' carry rows"""
    k = K()
    chunk = k.embed_bwd_det_chunk()
    B, T = (2 * chunk + 16) // 17 + 1, 17
    assert B * T > 2 * chunk
    fails, worst = [], Worst()
    with k.deterministic():
        for prefill in (False, True):
            backward_case(k, dev, B, T, 3, WIDE, "equal", "mixed", True, prefill, fails, worst, 5 * B + T, repeats=2)
    worst.report(f"embed bwd deterministic H={WIDE} B={B} T={T}: one run over {B * T / chunk:.1f} chunks")
    assert not fails, "\n".join(fails)


def test_shared_template_still_serves_768(dev):
    """one forward and one backward case (atomics and deterministic) at H = 768 through this file's
    code; test_embed_edges_gpu.py and test_deterministic_kernels_gpu.py remain that width's guard"""
    k = K()
    fails, worst = [], Worst()
    forward_case(k, dev, 3, 17, 3, 768, fails, worst)
    backward_case(k, dev, 17, 9, 3, 768, "special", "mixed", True, True, fails, worst, 230)
    with k.deterministic():
        backward_case(k, dev, 17, 9, 3, 768, "special", "mixed", True, True, fails, worst, 230, repeats=2)
    worst.report("embed fwd + bwd H=768")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("which", ("fwd", "bwd"))
def test_other_widths_are_refused_by_name(dev, which):
    from src._native import NativeError
    k = K()
    B, T, n_img, H = 2, 3, 1, 512
    S = n_img + 2 + T
    d = to_dev(R.embed_inputs(B, T, n_img, seed=1, H=H), dev)
    with pytest.raises(NativeError, match=r"768.*1024"):
        if which == "fwd":
            k.embed_fwd(d["ids"], d["seg"], d["txt_mask"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"],
                        d["ln_b"], EPS, d["cls_id"], d["sep_id"], None, 1, B, T, n_img, S,
                        torch.empty(B * S, H, dtype=bf16, device=dev), torch.empty(B, S, device=dev))
        else:
            k.embed_bwd(d["dX"], d["ids"], d["seg"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"],
                        torch.zeros(B * S, device=dev), torch.ones(B * S, device=dev), d["cls_id"], d["sep_id"], B, T,
                        n_img, *(torch.zeros_like(t) for t in (d["word"], d["pos"], d["typ"], d["ln_w"], d["ln_b"],
                                                               d["proj"])))
    # the library's own entry refuses it too (a caller that bypasses the wrapper's checks)
    from src import _native as N
    with pytest.raises(NativeError, match=r"768 or 1024"):
        z = torch.zeros(4 * H, device=dev)
        N.call("mmu_embed_fwd", 0, 0, 0, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
               z.data_ptr(), EPS, 0, 0, 0, 1, 1, 0, 1, 3, H, 0.0, 0.0, 0, z.data_ptr(), 0, z.data_ptr(), 0, 0, 0)
