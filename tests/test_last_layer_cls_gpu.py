"""The [CLS]-only last encoder layer (src/encoder.py LAST_LAYER_CLS) and the native entries it adds.

1. Row-stepped dropout streams (mmu_gemm_rows, mmu_layernorm_bwd_f32_rows): a compact problem
   whose row i stands for dense row i * row_step (+ row_offset) drops exactly the elements the
   existing entry drops in those rows of a dense run; with row_step = 1 the new entry reproduces
   the existing one bit for bit.  Values against float64 at the bars of the existing tests of the
   same kernels: test_kernels_gpu.py::test_gemm_bias_dropout_residual_f32_stream (kept elements
   rtol 1e-5 / atol 2e-5 max|y|, dropped ones within 1e-6 max|R| of the residual) and
   test_layernorm_edges_gpu.py (rowops_harness.check_bf16 / check_f32).
2. Attention for query row 0 (mmu_attention_row0_fwd / _bwd) through guarded, padded buffers:
   O / LSE of row 0 against float64 at attn_harness's bars, the keep words of row 0 bitwise those
   of the dense forward, nothing else written; dK / dV of all rows and dQ of row 0 against the
   float64 gradient of a dO that is zero outside row 0 (same bars) and against the dense backward
   fed that dO (each side is within CAP of float64 by its own bar, so they are within 2 CAP of
   each other on the same scale); the bias column sums at the dense test's bar (CAP of the
   column-summed scale).  The backward's dO / O / LSE / keep-word buffers hold NaN (canary words)
   outside row 0: a read of any other row poisons the result.
3. End to end: the small MMBT (2 layers), B = 3, L = 70, hidden / attention / embedding dropout
   0.1, fixed seeds; LAST_LAYER_CLS on against off: logits, loss, every parameter gradient and
   the gradient reaching the embeddings, within the relative bars test_mmbt_gpu.py holds the HIP
   path to (logits 1e-2 of their max, loss 1e-2, gradient norms 1e-2 per tensor above the noise
   floor of 1e-4 of the largest, the bf16 trunk's 0.1 each and 1e-2 in the median), and the l2
   distance of the non-trunk gradients within 1e-2 of their norms (_compare).  Both arms draw
   identical masks and run fixed convolution algorithms (a dense step then repeats bit for bit),
   so what remains is summation order and the f32 attention row, re-rounded by the bf16
   gradient stream.  Also with the last layer frozen, under torch.no_grad(), and one StepGraph
   replay against an eager step.

Measured on an MI355X (-s prints every case's figures):
  1. every drop decision equal; row_step = 1 bit-identical; LayerNorm dX / dXdrop at most 0.995 of
     the elementwise bar, row-error ratio to the model 1.000
  2. worst kernel / model ratio over the cases with L > 1 (max, median) and worst kernel nerr
     (cap 5.86e-3): O row 0 1.00, 0.95, 2.0e-3; dQ 1.13, 0.96, 3.3e-4; dK 0.82, 0.87, 1.6e-3; dV
     0.62, 0.79, 2.7e-3 (P and dS stay f32 here: below the rounding model); LSE at most 0.15 of its
     bar; bias column sums at most 3.2e-4 of the column-summed scale against float64, 2.0e-3
     against the dense parts
  3. train: logits 1.0e-3 of their max, loss 4.3e-5, non-trunk gradients: norms within 1.4e-3, l2
     distance at most 4.9e-3 (layer 0's query weight), trunk gradient norms median 5.2e-4 / max
     2.0e-3, the embedding gradient 3.2e-3 in l2 (6.5e-3 of its max elementwise: the bf16
     gradient stream re-rounded); a dense step against itself: 0 everywhere;
     graph replay against eager: loss and gradients bit-identical
"""
import pytest
import torch

import attn_harness as H
import rowops_harness as R
from guarded import Guarded, check_written, guarded_input, out_buf, probe_keep

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = 1e-12
bf16, f32t = torch.bfloat16, torch.float32
KEEP_CANARY = 0x5A5A5A5A5A5A5A5A


def K():
    from src import kernels
    return kernels


# ------------------------------------------------------------------------------- 1. row-stepped streams
ROWS = (1, 3, 130)
STEPS = (1, 7, 513)


def _dense_keep(k, dev, M, N, p, seed, step, off=0):
    """the existing entry's keep bits of rows off + i * step of a dense [.., N] product"""
    if p == 0:
        return torch.ones(M, N, dtype=torch.bool, device=dev)
    Md = off + (M - 1) * step + 1
    return probe_keep(k, dev, Md, N, p, seed)[off::step][:M].clone()


def _stepped_probe(k, dev, M, N, p, seed, step, off=0):
    """the row-stepped entry's keep bits, read like guarded.probe_keep reads the dense ones"""
    A = torch.zeros(M, 64, dtype=bf16, device=dev)
    Bm = torch.zeros(N, 64, dtype=bf16, device=dev)
    Z = torch.zeros(M, N, dtype=bf16, device=dev)
    C = torch.full((M, N), NAN, dtype=bf16, device=dev)
    k.gemm(A, 64, True, Bm, 64, True, C, N, M, N, 64, row_step=step, row_offset=off,
           epi=k.epilogue(k.EPI_BIAS_DROP_RES, bias=torch.ones(N, device=dev), residual=Z, drop_p=p, seed=seed))
    assert torch.isfinite(C.float()).all()
    return C != 0


@pytest.mark.parametrize("N", [768, 128])
@pytest.mark.parametrize("M", ROWS)
def test_gemm_rows_dropout_stream(dev, M, N):
    k = K()
    Kd, seed = 64, 0x51DE0000 + M + N
    g = torch.Generator(device="cpu").manual_seed(M * 1000 + N)
    A = torch.randn(M, Kd, generator=g).to(bf16).to(dev)
    Bm = (torch.randn(N, Kd, generator=g) * 0.1).to(bf16).to(dev)
    bias = (torch.randn(N, generator=g) * 0.1).to(dev)
    R32 = (torch.randn(M, N, generator=g) * 3.0 + 1.0 / 3.0).to(dev)
    y = (A.double() @ Bm.double().t() + bias.double())
    ymax = y.abs().max().item()
    for p in (0.0, 0.1):
        epi = lambda: k.epilogue(k.EPI_BIAS_DROP_RES, bias=bias, residual=R32, drop_p=p, seed=seed)  # noqa: E731
        for step, off in [(s, 0) for s in STEPS] + [(7, 5)]:
            tag = f"M={M} N={N} p={p} step={step} off={off}"
            keep = _dense_keep(k, dev, M, N, p, seed, step, off)
            got = _stepped_probe(k, dev, M, N, p, seed, step, off) if p > 0 else keep
            bad = (got != keep).sum().item()
            assert bad == 0, f"{tag}: {bad} of {keep.numel()} drop decisions differ from the dense run's rows"
            gb, out = out_buf(dev, f32t, M, N)
            k.gemm(A, Kd, True, Bm, Kd, True, out, N, M, N, Kd, epi=epi(), row_step=step, row_offset=off)
            torch.cuda.synchronize()
            fails = []
            check_written({"C": gb}, fails, tag)
            assert not fails, fails
            d = out.double() - R32.double()
            zs = 1.0 / (1.0 - p)
            torch.testing.assert_close(d[keep], (y * zs)[keep], rtol=1e-5, atol=2e-5 * ymax, msg=lambda m: f"{tag}: {m}")
            assert (d[~keep].abs() <= 1e-6 * R32.abs().max().item()).all(), f"{tag}: a dropped element is not the residual"
            if step == 1 and off == 0:  # the existing entry, bit for bit
                ref = torch.full((M, N), NAN, dtype=f32t, device=dev)
                k.gemm(A, Kd, True, Bm, Kd, True, ref, N, M, N, Kd, epi=epi())
                assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"{tag}: differs from mmu_gemm"


@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_bwd_rows_dropout_stream(dev, rows):
    k = K()
    Hd, seed = 768, 0xD20B0300 + rows
    Xc, wc, bc, dYc, _ = R.ln_inputs(rows, Hd, "gauss", seed=3 * rows + Hd, f32=True)
    X, w, b, dY = (guarded_input(dev, t) for t in (Xc, wc, bc, dYc))
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    k.layernorm_fwd_f32(X, w, b, torch.empty(rows, Hd, dtype=bf16, device=dev), None, mean, rstd, eps=EPS)
    mean, rstd = guarded_input(dev, mean.cpu()), guarded_input(dev, rstd.cpu())
    P = k.ln_parts(rows)
    fails, worst = [], R.Worst()

    def run(p, **kw):
        bufs, outs = {}, {}
        for name, shape, dt in (("dX", (rows, Hd), bf16), ("dXdrop", (rows, Hd), bf16), ("pdw", (P, Hd), f32t),
                                ("pdb", (P, Hd), f32t), ("pdbias", (P, Hd), f32t)):
            bufs[name], outs[name] = out_buf(dev, dt, *shape)
        k.layernorm_bwd(dY, X, mean, rstd, w, outs["dX"], outs["dXdrop"], p, seed, outs["pdw"], outs["pdb"],
                        outs["pdbias"], **kw)
        torch.cuda.synchronize()
        return bufs, outs

    for p in (0.0, 0.1):
        for step, off in [(s, 0) for s in STEPS] + [(7, 5)]:
            tag = f"rows={rows} p={p} step={step} off={off}"
            keep = _dense_keep(k, dev, rows, Hd, p, seed, step, off)
            ref, sc = R.ln_bwd_ref(dY, X, w, EPS, keep=keep, p=p)
            m = R.ln_bwd_model(dY, X, mean, rstd, w, keep=keep, p=p)
            bufs, o = run(p, row_step=step, row_offset=off)
            check_written(bufs, fails, tag)
            log = []
            for name in ("dX", "dXdrop"):
                el, st = R.check_bf16(f"{tag} {name}", o[name], m[name], ref[name], sc[name], fails, log)
                worst.bf(name, el, st)
            for name in ("pdw", "pdb", "pdbias"):
                worst.f32(name, *R.check_f32(f"{tag} {name}", o[name], m[name], ref[name], sc[name], fails, log))
            print("\n".join(log))
            # exactly the dense run's dropped set (a kept element is zero only where dX itself is)
            bad = ((o["dXdrop"] != 0) != (keep & (o["dX"] != 0))).sum().item()
            if bad:
                fails.append(f"{tag}: {bad} dXdrop elements disagree with the dense run's mask")
            if step == 1 and off == 0:  # the existing entry, bit for bit
                _, e = run(p)
                for name in o:
                    bits = {2: torch.int16, 4: torch.int32}[o[name].element_size()]
                    if not torch.equal(o[name].view(bits), e[name].view(bits)):
                        fails.append(f"{tag}: {name} differs from mmu_layernorm_bwd_f32")
    worst.report(f"ln bwd rows={rows}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------- 2. row-0 attention
HEADS = 12
ATT_CASES = [(L, B) for L in (1, 63, 64, 65, 129) for B in (1, 3)]


class _AttnBufs:
    """canary-filled outputs of a forward + backward (padded leading dimensions, guard rows)"""

    def __init__(self, dev, B, L):
        HD, BH, nkv = HEADS * 64, B * HEADS, (L + 63) // 64
        self.O = Guarded(dev, bf16, NAN, B * L, HD, HD + 8)
        self.dqkv = Guarded(dev, bf16, NAN, B * L, 3 * HD, 3 * HD + 8)
        self.lse = Guarded(dev, f32t, NAN, BH * L)
        self.keep = Guarded(dev, torch.int64, KEEP_CANARY, BH * L * nkv)

    def all(self):
        return {"O": self.O, "dqkv": self.dqkv, "lse": self.lse, "keep": self.keep}


def _row0_stats(got, model, ref, sc, names):
    """attn_harness.evaluate on the given [B, heads, rows, 64] slices -> its stats dict"""
    stats = {}
    for n in names:
        ek, zk = H.nerr(got[n], ref[n], sc[n])
        em, _ = H.nerr(model[n], ref[n], sc[n])
        st = {"max_k": 0.0, "med_k": 0.0, "max_m": 0.0, "med_m": 0.0}
        if ek.numel():
            st = {"max_k": ek.max().item(), "med_k": ek.median().item(), "max_m": em.max().item(),
                  "med_m": em.median().item()}
        st["finite"] = bool(torch.isfinite(got[n].float()).all())
        st["zero_ok"] = bool((zk == 0).all())
        stats[n] = st
    return stats


@pytest.mark.parametrize("L,B", ATT_CASES, ids=[f"L{L}-B{B}" for L, B in ATT_CASES])
def test_attention_row0(dev, L, B):
    k = K()
    HD, BH, nkv = HEADS * 64, B * HEADS, (L + 63) // 64
    seed = 0xA77E1000 + 977 * L + B
    fails = []
    r0 = torch.arange(B, device=dev) * L  # row 0 of every sequence
    other = torch.ones(B * L, dtype=torch.bool, device=dev)
    other[r0] = False
    # item 0 unmasked, item 1 a random additive mask, item 2 (B = 3): a padded tail / all but one key
    for mask_kind in ((0, 3) if B > 2 else (0,)):
        qkv_c, km_c, dO_c = H.make_inputs(B, L, HEADS, seed=10 * L + B, mask_kind=mask_kind)
        dO0_c = torch.zeros_like(dO_c)
        dO0_c[r0.cpu()] = dO_c[r0.cpu()]
        qkv = guarded_input(dev, qkv_c, 3 * HD + 8)
        km = guarded_input(dev, km_c)
        dO0 = guarded_input(dev, dO0_c, HD + 16)             # the dense backward's: zero outside row 0
        dOn_c = torch.full_like(dO_c, NAN)
        dOn_c[r0.cpu()] = dO_c[r0.cpu()]
        dOn = guarded_input(dev, dOn_c, HD + 16)             # the row-0 backward's: NaN outside row 0
        lse_f32 = H.lse32(qkv, km, B, L, HEADS)
        for p in (0.0, 0.1):
            tag = f"L={L} B={B} mask={mask_kind} p={p}"
            # ---- dense forward + backward (dO zero outside row 0)
            dn = _AttnBufs(dev, B, L)
            lse_d = dn.lse.view.view(BH, L)
            dm_d = dn.keep.view.view(BH, L, nkv) if p > 0 else None
            k.attention_fwd(qkv, km, dn.O.view, lse_d, B, L, heads=HEADS, drop_p=p, seed=seed, dropmask=dm_d)
            delta = torch.empty(BH, L, device=dev)
            parts = k.attention_dbias_parts(B, L, HEADS, dev)
            k.attention_bwd(qkv, km, dn.O.view, dO0, lse_d, delta, dn.dqkv.view, B, L, heads=HEADS, drop_p=p, seed=seed,
                            dropmask=dm_d, dbias_parts=parts)
            # ---- row-0 forward
            rw = _AttnBufs(dev, B, L)
            lse_r = rw.lse.view.view(BH, L)
            dm_r = rw.keep.view.view(BH, L, nkv) if p > 0 else None
            k.attention_row0_fwd(qkv, km, rw.O.view, lse_r, B, L, heads=HEADS, drop_p=p, seed=seed, dropmask=dm_r)
            torch.cuda.synchronize()
            for name, gd in rw.all().items():
                if not gd.guards_intact():
                    fails.append(f"{tag} fwd {name}: a guard row / padding column / guard element was written")
            if not torch.isnan(rw.O.view[other].float()).all() or not torch.isnan(rw.dqkv.view.float()).all():
                fails.append(f"{tag} fwd: a row of O other than row 0 (or dQKV) was written")
            if not torch.isnan(lse_r[:, 1:]).all():
                fails.append(f"{tag} fwd: an LSE entry other than row 0 was written")
            kw_all = rw.keep.view.view(BH, L, nkv)
            if not (kw_all[:, 1:] == KEEP_CANARY).all():
                fails.append(f"{tag} fwd: a keep word outside row 0 was written")
            if p > 0:
                if not torch.equal(kw_all[:, 0], dm_d[:, 0]):
                    fails.append(f"{tag} fwd: the keep words of row 0 differ from the dense forward's")
                keep = k.dropmask_dense(dm_d, L).view(B, HEADS, L, L)
            else:
                if not (kw_all == KEEP_CANARY).all():
                    fails.append(f"{tag} fwd: keep words written without dropout")
                keep = torch.ones(B, HEADS, L, L, device=dev)
            # ---- float64 reference, rounding model, scales (dO zero outside row 0)
            O64, lse64, g64 = H.ref64(qkv, km, dO0, B, L, HEADS, keep, p)
            Om, _, gm = H.model32(qkv, km, dO0, B, L, HEADS, keep, p)
            sc = H.scales(qkv, km, dO0, B, L, HEADS, keep, p)
            hv = lambda t: H.heads_view(t, B, L, HEADS)  # noqa: E731
            first = lambda t: t[:, :, :1]                # noqa: E731
            st = _row0_stats({"O": first(hv(rw.O.view))}, {"O": first(hv(Om))}, {"O": first(hv(O64))},
                             {"O": first(sc["O"])}, ("O",))
            e, base, worst = H.lse_stats(lse_r[:, 0], lse64[:, 0], lse_f32[:, 0])
            print(f"[{tag}] O row 0: kernel {st['O']['max_k']:.2e}/{st['O']['med_k']:.2e} model "
                  f"{st['O']['max_m']:.2e}/{st['O']['med_m']:.2e}; LSE err {e:.2e} ({worst:.2f} x the bar)")
            fails += [f"{tag} fwd: {m}" for m in H.violations(st) + H.lse_violations(lse_r[:, 0], lse64[:, 0], lse_f32[:, 0])]
            # ---- row-0 backward from the row-0 forward's own buffers (NaN / canary outside row 0)
            dbs_g, dbs = out_buf(dev, f32t, 3, B, HD)
            k.attention_row0_bwd(qkv, km, rw.O.view, dOn, lse_r, rw.dqkv.view, B, L, heads=HEADS, drop_p=p,
                                 dropmask=dm_r, dbias_sums=dbs)
            torch.cuda.synchronize()
            check_written({"dbias": dbs_g}, fails, f"{tag} bwd")
            for name, gd in rw.all().items():
                if not gd.guards_intact():
                    fails.append(f"{tag} bwd {name}: a guard row / padding column / guard element was written")
            dq = rw.dqkv.view
            if not torch.isnan(dq[other][:, :HD].float()).all():
                fails.append(f"{tag} bwd: a dQ row other than row 0 was written")
            if not torch.isfinite(dq[:, HD:].float()).all() or not torch.isfinite(dq[r0][:, :HD].float()).all():
                fails.append(f"{tag} bwd: dK / dV (all rows) or dQ (row 0) not finite (unwritten or poisoned)")
                continue
            got = dq.clone()
            got[other, :HD] = 0  # (the dense result there: exactly zero, checked on the dense side below)
            if not (dn.dqkv.view[other][:, :HD] == 0).all():
                fails.append(f"{tag}: the dense backward's dQ outside row 0 is not zero")
            parts_k = {n: hv(got[:, i * HD:(i + 1) * HD]) for i, n in enumerate(("dQ", "dK", "dV"))}
            parts_m = {n: hv(gm[:, i * HD:(i + 1) * HD]) for i, n in enumerate(("dQ", "dK", "dV"))}
            parts_r = {n: hv(g64[:, i * HD:(i + 1) * HD]) for i, n in enumerate(("dQ", "dK", "dV"))}
            stb = _row0_stats(parts_k, parts_m, parts_r, sc, ("dQ", "dK", "dV"))
            print(f"[{tag}] " + " ".join(f"{n}: kernel {s['max_k']:.2e}/{s['med_k']:.2e} model {s['max_m']:.2e}/"
                                         f"{s['med_m']:.2e};" for n, s in stb.items()))
            fails += [f"{tag} bwd: {m}" for m in H.violations(stb)]
            # against the dense backward: each within CAP of float64 on this scale -> 2 CAP apart
            parts_d = {n: hv(dn.dqkv.view[:, i * HD:(i + 1) * HD]) for i, n in enumerate(("dQ", "dK", "dV"))}
            for n in ("dQ", "dK", "dV"):
                ed, _ = H.nerr(parts_k[n], parts_d[n].float(), sc[n])
                if ed.numel() and not ed.max().item() <= 2 * H.CAP:
                    fails.append(f"{tag} bwd: {n} is {ed.max().item():.3e} of its scale from the dense backward's")
            # bias column sums: [3][B][HD] summed over B, at the dense test's bar; and the dense parts
            colsc = torch.cat([H.rows_view(sc[n], B, L, HEADS).sum(0) for n in ("dQ", "dK", "dV")])
            mine = dbs.double().sum(1).reshape(-1)
            berr = (mine - g64.sum(0)).abs() / colsc.clamp_min(1e-300)
            berr = torch.where((colsc > 0) | (mine != 0), berr, torch.zeros_like(berr)).max().item()
            gb = torch.zeros(3 * HD, device=dev)
            k.attention_dbias_reduce(parts, B, L, gb, heads=HEADS)
            derr = ((mine - gb.double()).abs() / colsc.clamp_min(1e-300))
            derr = torch.where(colsc > 0, derr, torch.zeros_like(derr)).max().item()
            print(f"[{tag}] dbias err / column-summed scale {berr:.2e}; against the dense parts {derr:.2e}")
            if not berr <= H.CAP:
                fails.append(f"{tag}: dbias column sums off by {berr:.3e} of the scale > {H.CAP:.3e}")
            if not derr <= 2 * H.CAP:
                fails.append(f"{tag}: dbias column sums {derr:.3e} of the scale from the dense backward's")
            # the per-item dQ slab is dQ row 0 itself (before its bf16 rounding)
            if not torch.allclose(dbs[0], dq[r0][:, :HD].float(), rtol=2.0 ** -8, atol=0):
                fails.append(f"{tag}: dbias slab 0 is not dQ row 0")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------- 3. end to end
B3, T3, P3 = 3, 65, 0.1  # L = num_image_embeds + 2 + T = 70
REL = 1e-2               # test_mmbt_gpu.py: tol_check's relative bar / GRAD_REL
FLOOR = 1e-4             # ... its gradient noise floor, as a share of the largest gradient norm
TRUNK_MEDIAN, TRUNK_MAX = 1e-2, 0.1  # ... and its bars on the bf16 product trunk's gradient norms


def _e2e_model(freeze_last=False):
    from oracle.weights import SMALL, make_state_dict
    from src.mmbt import MultimodalBertClf
    from src.testing import small_args
    torch.manual_seed(0)
    m = MultimodalBertClf(small_args(bert_hidden_dropout=P3, bert_attn_dropout=P3, dropout=P3))
    m.load_state_dict(make_state_dict(0, SMALL), strict=True)
    m = m.to("cuda:0").train()
    if freeze_last:
        last = max(int(n.split("encoder.layer.")[1].split(".")[0]) for n, _ in m.named_parameters()
                   if "encoder.layer." in n)
        for n, prm in m.named_parameters():
            if f"encoder.layer.{last}." in n:
                prm.requires_grad_(False)
    return m


def _e2e_batch():
    from oracle.weights import SMALL
    from src.testing import synthetic_batch
    x, y = synthetic_batch(B3, T3, vocab=SMALL.vocab, lens=[65, 40, 9], seed=4)
    return tuple(t.to("cuda:0") for t in x), y.to("cuda:0")


def _arm(on, freeze_last=False, grad=True):
    """one seeded step of a fresh model -> logits, loss, {name: grad}, the gradient reaching the embeddings"""
    from src import encoder, mmbt
    m = _e2e_model(freeze_last)
    x, y = _e2e_batch()
    emb_grad = []
    stack = mmbt.encoder_stack

    def tapped(lws, X, *a, **kw):
        if X.requires_grad:
            X.register_hook(lambda gX: emb_grad.append(gX.detach().float().clone()))
        return stack(lws, X, *a, **kw)

    old, old_det = encoder.LAST_LAYER_CLS, torch.backends.cudnn.deterministic
    encoder.LAST_LAYER_CLS = on
    mmbt.encoder_stack = tapped
    # (without fixed convolution algorithms two runs of ONE arm differ by 2e-3 in the logits)
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(11)  # the host-drawn dropout seeds (src/mmbt.py _seed)
        if not grad:
            with torch.no_grad():
                logits = m(*x)
            return logits.float().cpu(), None, {}, None
        m.store.zero_grad()
        logits = m(*x)
        loss = m.compute_loss(logits, y)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        encoder.LAST_LAYER_CLS = old
        mmbt.encoder_stack = stack
        torch.backends.cudnn.deterministic = old_det
    grads = {n: prm.grad.detach().float().cpu().clone() for n, prm in m.named_parameters() if prm.grad is not None}
    return logits.detach().float().cpu(), loss.item(), grads, (emb_grad[0].cpu() if emb_grad else None)


def _compare(tag, a, b):
    """arm a (LAST_LAYER_CLS on) against arm b (off) at test_mmbt_gpu.py's relative bars: logits
    within REL of their max, loss within REL, per-tensor gradient norms within REL above the noise
    floor (the bf16 trunk's: each within TRUNK_MAX, their median within TRUNK_MEDIAN); on top of
    those, the l2 distance of every non-trunk gradient above the floor, and of the gradient
    reaching the embeddings, within REL of the tensor's norm (a norm alone cannot see a rotated
    gradient).  The arms are deterministic (fixed convolution algorithms), so the figures repeat."""
    la, lossa, ga, ea = a
    lb, lossb, gb, eb = b
    lerr = (la - lb).abs().max().item() / lb.abs().max().item()
    msg = f"[{tag}] logits max err / max {lerr:.2e}"
    assert lerr <= REL, msg
    if lossb is None:
        print(msg)
        return
    loss_err = abs(lossa - lossb) / abs(lossb)
    assert loss_err < REL, f"{tag}: loss {lossa} vs {lossb}"
    assert set(ga) == set(gb), f"{tag}: the arms produce gradients for different parameters"
    norm = {n: t.double().norm().item() for n, t in gb.items()}
    floor = FLOOR * max(norm.values())
    trunk, worst_n, worst_l2 = [], (0.0, None), (0.0, None)
    for n in gb:
        na = ga[n].double().norm().item()
        is_trunk = "img_encoder" in n
        bar = TRUNK_MAX if is_trunk else REL
        assert abs(na - norm[n]) <= bar * norm[n] + floor, f"{tag}: grad norm of {n}: {na:.6e} vs {norm[n]:.6e}"
        if norm[n] <= floor:
            continue
        e = abs(na - norm[n]) / norm[n]
        if is_trunk:
            trunk.append(e)
            continue
        l2 = (ga[n].double() - gb[n].double()).norm().item() / norm[n]
        assert l2 <= REL, f"{tag}: grad {n}: l2 distance {l2:.3e} of its norm"
        worst_n, worst_l2 = max(worst_n, (e, n)), max(worst_l2, (l2, n))
    trunk.sort()
    tmed, tmax = (trunk[len(trunk) // 2], trunk[-1]) if trunk else (0.0, 0.0)
    assert tmed <= TRUNK_MEDIAN, f"{tag}: trunk grad-norm errors: median {tmed:.3e}"
    el2 = (ea - eb).norm().item() / eb.norm().item()
    emax = (ea - eb).abs().max().item() / eb.abs().max().item()
    assert el2 <= REL, f"{tag}: the gradient reaching the embeddings differs by {el2:.3e} of its norm"
    print(f"{msg}; loss rel err {loss_err:.2e}; non-trunk gradients: worst norm err {worst_n[0]:.2e} ({worst_n[1]}), "
          f"worst l2 distance {worst_l2[0]:.2e} ({worst_l2[1]}); trunk grad-norm errors median {tmed:.2e} max "
          f"{tmax:.2e}; embedding gradient l2 {el2:.2e}, max elementwise {emax:.2e} of its max")


@pytest.fixture(scope="module")
def dense_arm(dev):
    return _arm(False)


def test_last_layer_cls_equals_dense_step(dev, dense_arm):
    _compare("train", _arm(True), dense_arm)


def test_last_layer_cls_equals_dense_step_frozen_last_layer(dev):
    a, b = _arm(True, freeze_last=True), _arm(False, freeze_last=True)
    for arm in (a, b):  # (the store's gradient views exist for frozen tensors too: they stay zero)
        assert all((g == 0).all() for n, g in arm[2].items() if "encoder.layer.1." in n), \
            "a frozen layer received gradients"
    assert any((g != 0).any() for n, g in a[2].items() if "encoder.layer.0." in n)
    _compare("frozen last layer", a, b)


def test_last_layer_cls_equals_dense_no_grad(dev):
    _compare("no_grad", _arm(True, grad=False), _arm(False, grad=False))


def test_last_layer_cls_graph_replay_equals_eager(dev):
    """one StepGraph replay (capture after one warm-up step) against the eager steps with the
    capture's host seeds and the replay's counter value; LAST_LAYER_CLS at its default (on)."""
    from src import encoder, kernels as k
    from src.graphs import StepGraph
    assert encoder.LAST_LAYER_CLS
    torch.backends.cudnn.deterministic = True  # (as test_graph_gpu.py)
    x, y = _e2e_batch()

    def stepper(m):
        def step():
            m.store.zero_grad()
            loss = m.compute_loss(m(*x), y)
            loss.backward()
            return loss
        return step

    ma = _e2e_model()
    torch.manual_seed(21)
    g = StepGraph(stepper(ma), dev, warmup=1)
    loss_a = g.replay().item()
    torch.cuda.synchronize()
    grad_a = ma.store.grad.clone()
    ctr_a = int(g.counter.item())
    g.release()
    del g

    def eager():
        mb = _e2e_model()
        step_b = stepper(mb)
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        k.set_seed_offset(ctr)
        try:
            torch.manual_seed(21)
            ctr.fill_(1)
            step_b()                     # the StepGraph's warm-up step (counter 1)
            ctr.fill_(ctr_a)             # the replay's first node advanced the counter to 2
            loss_b = step_b().item()     # (the capture drew its host seeds right after the warm-up's)
            torch.cuda.synchronize()
        finally:
            k.set_seed_offset(None)
        return loss_b, mb.store.grad.clone()

    (loss_b, grad_b), (loss_c, grad_c) = eager(), eager()
    rel = lambda u, v: ((u - v).norm() / v.norm()).item()  # noqa: E731
    d, noise = rel(grad_a, grad_b), rel(grad_c, grad_b)
    print(f"[graph] loss replay {loss_a:.6f} eager {loss_b:.6f} / {loss_c:.6f}; grad rel diff replay vs eager {d:.2e}, "
          f"eager vs eager {noise:.2e}")
    assert ctr_a == 2
    # the bars of test_graph_gpu.py: loss to 1e-5, the rest to 1e-4 or 3 x the eager step's own
    # run-to-run spread (float-atomic summation order)
    assert abs(loss_a - loss_b) <= max(1e-5 * abs(loss_b), 3 * abs(loss_c - loss_b)), (loss_a, loss_b, loss_c)
    assert d <= max(1e-4, 3 * noise), (d, noise)
