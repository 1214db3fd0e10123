"""The embedding kernels (csrc/embed.hip: embed_fwd_kernel, embed_bwd_rows_kernel + the column-sum
fold) against float64, through guarded outputs, with both dropouts on.

H = 768, n_img 1 and 3, 300 word rows, 512 position rows.  Forward: the identity variant at
(B, T) = (1, 1), (1, 16), (3, 17), (5, 2) (row totals that are no multiple of the 4 rows of a
block) and three index sets (a permutation, repeated positions, Lout != n_img + 2 + T) in one
launch; txt_mask with zeros (key mask exactly -10000 there, exactly 0 elsewhere, 0 on every
image-segment row); X32 / mean / rstd given and absent; dropout 0.3 on the image segment and 0.1
on the text, its keep bits taken from a probe call with ln_w = 0, ln_b = 1 (every output is then
exactly 1/(1-p) of its row's segment, or 0).  Backward, with the forward's keep bits: dropouts on
and off; B around EBW_B = 16; T = 1, 9, 17; all ids equal (every atomic hits one word row); ids that
include [CLS] and [SEP] (the scatter and the position sum meet in one row); segments all 0, all 1,
mixed; gradient buffers zero-filled and pre-filled (the kernel accumulates; d_proj is overwritten).

Bars: rowops_harness (X: elementwise and row error against the float32 model; every f32 output
within 8 x the model's error or 4 ulps of its scale).

Measured on an MI355X over the whole sweep (run with -s for every case's figures):
  X (bf16): elementwise 0.995 of the bar; kernel / model row error 1.000 (max), 1.000 (median);
      worst row error 1.78e-3
  f32 outputs: worst |err| / scale, kernel (model), share of the bar
      X32 8.8e-7 (9.0e-7) 0.15;  mean 1.8e-8 (1.3e-8) 0.04;  rstd 1.0e-7 (9.0e-8) 0.24
      d_word 1.0e-6 (1.0e-6) 0.32;  d_pos 7.5e-7 (7.5e-7) 0.25;  d_type 5.4e-7 (5.4e-7) 0.17
      d_ln_w 9.2e-6 (9.2e-6, B = T = 1: four rows, cancelling) 0.21;  d_ln_b 2.0e-7 (2.0e-7) 0.20
      d_proj 9.6e-7 (9.6e-7) 0.16
  all 46 per-segment drop rates within 4 sigma of 0.3 / 0.1; key mask exact; no guard written
No bar was exceeded and no kernel changed.
"""
import math

import pytest
import torch

import rowops_harness as R
from guarded import check_written, out_buf
from rowops_harness import Worst

pytestmark = pytest.mark.gpu

EPS = 1e-12
NAN = float("nan")
bf16, f32t = torch.bfloat16, torch.float32
DROP_IMG, DROP_TXT = R.DROP_IMG, R.DROP_TXT


def K():
    from src import kernels
    return kernels


def to_dev(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def run_fwd(k, dev, d, idx, V, B, T, n_img, Lout, seed, pi, pt, x32=True, stats=True, ln=None):
    """embed_fwd into NaN-filled guarded outputs -> (X, X32, keymask, mean, rstd, bufs)"""
    rows = V * B * Lout
    bufs = {}
    bufs["X"], X = out_buf(dev, bf16, rows, 768)
    bufs["keymask"], km = out_buf(dev, f32t, V * B, Lout)
    X32 = mean = rstd = None
    if x32:
        bufs["X32"], X32 = out_buf(dev, f32t, rows, 768)
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
    ln = (torch.zeros(768, device=dev), torch.ones(768, device=dev))
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


@pytest.mark.parametrize("n_img", R.EMBED_N_IMG)
@pytest.mark.parametrize("B,T", R.EMBED_FWD_SHAPES)
def test_embed_forward_edges(dev, B, T, n_img):
    k = K()
    fails, worst = [], Worst()
    S = n_img + 2 + T
    d = to_dev(R.embed_inputs(B, T, n_img, seed=31 * B + T + n_img), dev)
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
                    print(f"[{vname} B={B} T={T} n_img={n_img}] {name} drop rate {rate:.4f} (p {p} +- {tol:.4f})")
                    if abs(rate - p) > tol:
                        fails.append(f"{vname} {name}: drop rate {rate:.4f} not within {tol:.4f} of {p}")
            ref, sc = R.embed_fwd_ref(*args, keep=keep, drop_txt=pt, drop_img=pi)
            m = R.embed_fwd_model(*args, keep=keep, drop_txt=pt, drop_img=pi)
            for x32, stats in ((True, True), (False, False)):
                tag = f"{vname} B={B} T={T} n_img={n_img} drop={drop} x32={x32} stats={stats}"
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
    worst.report(f"embed fwd B={B} T={T} n_img={n_img}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n_img", R.EMBED_N_IMG)
@pytest.mark.parametrize("B", R.EMBED_BWD_B)
def test_embed_backward_edges(dev, B, n_img):
    k = K()
    fails, worst = [], Worst()
    for ti, T in enumerate(R.EMBED_BWD_T):
        S = n_img + 2 + T
        for ci, (ids_kind, seg_kind) in enumerate(R.EMBED_BWD_KINDS):
            d = to_dev(R.embed_inputs(B, T, n_img, seed=13 * B + T + ci, ids_kind=ids_kind, seg_kind=seg_kind), dev)
            params = (d["word"], d["pos"], d["typ"], d["ln_w"], d["ln_b"])
            for drop in (True, False):
                pi, pt = (DROP_IMG, DROP_TXT) if drop else (0.0, 0.0)
                seed = 0xEB0000 + 7 * B + T
                keep = probe_keep(k, dev, d, None, 1, B, T, n_img, S, seed, pi, pt)[0] if drop else None
                _, _, _, mean, rstd, _ = run_fwd(k, dev, d, None, 1, B, T, n_img, S, seed, pi, pt)
                bargs = (d["dX"], d["ids"], d["seg"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"])
                # zero-filled, and pre-filled gradient buffers (rotating: one of the two per case,
                # both for the first T)
                fills = (False, True) if ti == 0 else ((ci + drop) % 2 == 1,)
                for prefill in fills:
                    tag = f"B={B} T={T} n_img={n_img} ids={ids_kind} seg={seg_kind} drop={drop} prefill={prefill}"
                    log = []
                    gen = torch.Generator().manual_seed(B + T)
                    init = {n: ((torch.randn(t.shape, generator=gen) * 0.1).to(dev) if prefill else
                                torch.zeros_like(t)) for n, t in zip(R.GRADS[:5], params)}
                    bufs, outs = {}, {}
                    for n, t in zip(R.GRADS, params + (d["proj"],)):
                        bufs[n], outs[n] = out_buf(dev, f32t, *t.shape)
                        if n != "d_proj":  # (d_proj stays NaN-filled: it is overwritten, not accumulated)
                            outs[n].copy_(init[n])
                    k.embed_bwd(d["dX"], d["ids"], d["seg"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"], mean,
                                rstd, d["cls_id"], d["sep_id"], B, T, n_img, *(outs[n] for n in R.GRADS), drop_txt=pt,
                                drop_img=pi, seed=seed)
                    torch.cuda.synchronize()
                    check_written(bufs, fails, tag)
                    ref, sc = R.embed_bwd_ref(*bargs, d["ln_b"], EPS, d["cls_id"], d["sep_id"], B, T, n_img, keep=keep,
                                              drop_txt=pt, drop_img=pi, init=init)
                    m = R.embed_bwd_model(*bargs, mean, rstd, d["cls_id"], d["sep_id"], B, T, n_img, keep=keep,
                                          drop_txt=pt, drop_img=pi, init=init)
                    for n in R.GRADS:
                        worst.f32(n, *R.check_f32(f"{tag} {n}", outs[n], m[n], ref[n], sc[n], fails, log))
                    print("\n".join(log))
    worst.report(f"embed bwd B={B} n_img={n_img}")
    assert not fails, "\n".join(fails)
