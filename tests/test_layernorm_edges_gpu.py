"""The LayerNorm kernels (csrc/layernorm.hip: ln_fwd2 row pairs, ln_fwd row per wave, ln_fwd32,
ln_bwd with bf16 / f32 X, dropout and residual arms) against float64 at every row count where
they branch, through guarded buffers, and the agreement of the backward's regenerated dropout
mask with the bits the producing GEMM epilogue drew.

Forward: H = 256 / 512 / 768 / 1024; rows 1..33 around the 16-row block, the 8-row wave stride, the
`+4` second row (or pair) in flight and an odd last pair; grouped parameters 3 x 5 rows (row per
wave), 3 x 6 (pairs), 7 x 1, and 3 x 5 with param_stride 0 (pairs again); mean / rstd given and
absent, Y32 given and absent.  Backward: rows 1..129 around the 64-row part edge and the ends of the
two-rows-per-step loop; X bf16 and f32; plain, dXdrop (p = 0.1, keep bits from the probe GEMM) and
dRes arms; partial buffers of exactly ln_parts(rows) rows, each given and absent.

Inputs (rowops_harness.ln_inputs): Gaussian, mean-offset (+8) and wide-range rows (the elementwise
bar on Y is not applied to the mean-offset family: ln_inputs says why).  Buffers: every
tensor is a view inside a larger allocation (tests/guarded.py); input guards hold NaN, outputs are
NaN-filled: afterwards the live region is finite and the guards are bit-identical.

Bars: rowops_harness (elementwise 2^-8 |ref| + 64 * 2^-24 scale; row error <= 2 x / 1.5 x the
float32 model's max / median; f32 outputs within 8 x the model's error or 4 ulps).

Mask agreement: a BIAS_DROP_RES GEMM with A = 0, bias = 1, residual 0 writes exactly 1/(1-p) or 0:
the forward's keep bits from the forward's own kernel.  layernorm_bwd with the same seed must give
(dXdrop != 0) == keep & (dX != 0) bit for bit: small tile, big tile with a partial last tile row,
batched; seeds 0, 1, 2^40 + 5; p = 0.1, 0.5; and under a non-zero seed offset counter.

Measured on an MI355X over the whole sweep (run with -s for every case's figures):
  bf16 outputs (all H, X bf16 and f32)        elementwise / bar   kernel / model row error (max, median)   worst row error
      Y                                       0.995               1.000, 1.000                             1.91e-3
      dX                                      0.995               1.000, 1.000                             1.85e-3
      dXdrop                                  0.995               1.000, 1.000                             1.92e-3
      dX + dRes                               0.995               1.000, 1.000                             1.78e-3
  f32 outputs: worst |err| / scale, kernel (model), share of the bar
      Y32 7.7e-7 (1.2e-6) 0.22;  mean 1.3e-7 (1.8e-7) 0.36;  rstd 1.2e-7 (1.1e-7) 0.23
      partial sums: dy x_hat 8.3e-7 (8.3e-7) 0.26;  dy 2.6e-8 (1.9e-8) 0.09;  dXdrop / dX 7.0e-7 (7.0e-7) 0.31
  mask agreement: 0 disagreeing elements in every shape, seed and p; no dX element was zero;
      drop rates 0.0979 .. 0.1003 at p = 0.1 and 0.4985 .. 0.5009 at p = 0.5
No bar was exceeded and no kernel changed.  With the mask index of ln_bwd_kernel shifted by one quad
in a scratch build (row * H + c + 4, not committed) 18 % of the dXdrop elements disagree with the
forward mask at p = 0.1 and all four mask tests fail ("Row-kernel edge sweep").
"""
import pytest
import torch

import rowops_harness as R
from guarded import check_written, guarded_input, out_buf, probe_keep
from rowops_harness import Worst

pytestmark = pytest.mark.gpu

EPS = 1e-12
NAN = float("nan")
bf16, f32t = torch.bfloat16, torch.float32


def K():
    from src import kernels
    return kernels


# ------------------------------------------------------------------------------- forward
FWD_CASES = [(rows, 1, 0, 0) for rows in R.LN_FWD_ROWS] + [(g * gr, g, gr, ps) for g, gr, ps in R.LN_FWD_GROUPED]


@pytest.mark.parametrize("H", R.LN_H)
@pytest.mark.parametrize("x32", [False, True], ids=["bf16", "f32"])
def test_layernorm_forward_edges(dev, H, x32):
    k = K()
    fails, worst = [], Worst()
    for kind in R.KINDS:
        for rows, groups, gr, psm in FWD_CASES:
            ps = psm * H
            Xc, wc, bc, _, _ = R.ln_inputs(rows, H, kind, seed=rows + H, groups=groups, param_stride=ps, f32=x32)
            X, w, b = guarded_input(dev, Xc), guarded_input(dev, wc), guarded_input(dev, bc)
            ref, sc = R.ln_fwd_ref(X, w, b, EPS, gr, ps)
            m = R.ln_fwd_model(X, w, b, EPS, gr, ps)
            for stats in (True, False):
                for y32 in ((True, False) if x32 else (False,)):
                    tag = f"{kind} H={H} rows={rows} groups={groups}x{gr} stride={ps} stats={stats} y32={y32}"
                    log = []
                    bufs = {}
                    bufs["Y"], Y = out_buf(dev, bf16, rows, H)
                    mean = rstd = Y32 = None
                    if stats:
                        bufs["mean"], mean = out_buf(dev, f32t, rows)
                        bufs["rstd"], rstd = out_buf(dev, f32t, rows)
                    if y32:
                        bufs["Y32"], Y32 = out_buf(dev, f32t, rows, H)
                    if x32:
                        k.layernorm_fwd_f32(X, w, b, Y, Y32, mean, rstd, eps=EPS, group_rows=gr, param_stride=ps)
                    else:
                        k.layernorm_fwd(X, w, b, Y, mean, rstd, eps=EPS, group_rows=gr, param_stride=ps)
                    torch.cuda.synchronize()
                    check_written(bufs, fails, tag)
                    el, st = R.check_bf16(f"{tag} Y", Y, m["Y"], ref["Y"], sc["Y"], fails, log, kind in R.ELEM_KINDS)
                    worst.bf("Y", el if kind in R.ELEM_KINDS else 0.0, st)
                    if y32:
                        worst.f32("Y32", *R.check_f32(f"{tag} Y32", Y32, m["Y32"], ref["Y"], sc["Y"], fails, log))
                    if stats:
                        worst.f32("mean", *R.check_f32(f"{tag} mean", mean, m["mean"], ref["mean"], sc["mean"], fails,
                                                       log))
                        worst.f32("rstd", *R.check_f32(f"{tag} rstd", rstd, m["rstd"], ref["rstd"], sc["rstd"], fails,
                                                       log))
                    print("\n".join(log))
    worst.report(f"fwd H={H} {'f32' if x32 else 'bf16'}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------- backward
PART_COMBOS = [(True, True, True), (False, False, False), (True, False, False), (False, True, False),
               (False, False, True)]


@pytest.mark.parametrize("H", R.LN_H)
@pytest.mark.parametrize("x32", [False, True], ids=["bf16", "f32"])
def test_layernorm_backward_edges(dev, H, x32):
    k = K()
    fails, worst = [], Worst()
    p, seed = 0.1, 0xD20B0000 + H
    for ki, kind in enumerate(R.KINDS):
        for ri, rows in enumerate(R.LN_BWD_ROWS):
            Xc, wc, bc, dYc, dRc = R.ln_inputs(rows, H, kind, seed=3 * rows + H, f32=x32)
            X, w, b, dY, dRes = (guarded_input(dev, t) for t in (Xc, wc, bc, dYc, dRc))
            mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
            Yt = torch.empty(rows, H, dtype=bf16, device=dev)
            if x32:
                k.layernorm_fwd_f32(X, w, b, Yt, None, mean, rstd, eps=EPS)
            else:
                k.layernorm_fwd(X, w, b, Yt, mean, rstd, eps=EPS)
            mean, rstd = guarded_input(dev, mean.cpu()), guarded_input(dev, rstd.cpu())
            # (the counter of element (m, n) is m H + n whatever M: a whole 128-row tile for the probe)
            keep = probe_keep(k, dev, -(-rows // 128) * 128, H, p, seed)[:rows]
            arms = [("plain", {}), ("drop", {"keep": keep, "p": p})] + ([] if x32 else [("res", {"dRes": dRes})])
            P = k.ln_parts(rows)
            for arm, kw in arms:
                ref, sc = R.ln_bwd_ref(dY, X, w, EPS, **kw)
                m = R.ln_bwd_model(dY, X, mean, rstd, w, **kw)
                first = None
                # every partial buffer given, then one other combination (rotating with the case)
                for combo in (PART_COMBOS[0], PART_COMBOS[1 + (ri + ki) % 4]):
                    tag = f"{kind} H={H} rows={rows} x32={x32} {arm} parts={combo}"
                    log = []
                    bufs = {}
                    bufs["dX"], dX = out_buf(dev, bf16, rows, H)
                    dXd = None
                    if arm == "drop":
                        bufs["dXdrop"], dXd = out_buf(dev, bf16, rows, H)
                    parts = []
                    for name, on in zip(("pdw", "pdb", "pdbias"), combo):
                        t = None
                        if on:
                            bufs[name], t = out_buf(dev, f32t, P, H)
                        parts.append(t)
                    if arm == "res":
                        k.layernorm_bwd_res(dY, X, mean, rstd, w, dRes, dX, *parts)
                    else:
                        k.layernorm_bwd(dY, X, mean, rstd, w, dX, dXd, p if arm == "drop" else 0.0, seed, *parts)
                    torch.cuda.synchronize()
                    check_written(bufs, fails, tag)
                    if first is not None:  # the same numbers whatever partial sums are asked for
                        if not torch.equal(dX.view(torch.int16), first[0].view(torch.int16)) or \
                                (dXd is not None and not torch.equal(dXd.view(torch.int16), first[1].view(torch.int16))):
                            fails.append(f"{tag}: dX / dXdrop differ from the call with every partial buffer")
                        for t, f in zip(parts, first[2]):
                            if t is not None and not torch.equal(t, f):
                                fails.append(f"{tag}: a partial buffer differs from the call with all three")
                        continue
                    first = (dX.clone(), None if dXd is None else dXd.clone(), [t.clone() for t in parts])
                    el, st = R.check_bf16(f"{tag} dX", dX, m["dX"], ref["dX"], sc["dX"], fails, log)
                    worst.bf("dX+dRes" if arm == "res" else "dX", el, st)
                    if arm == "drop":
                        el, st = R.check_bf16(f"{tag} dXdrop", dXd, m["dXdrop"], ref["dXdrop"], sc["dXdrop"], fails, log)
                        worst.bf("dXdrop", el, st)
                        if not (dXd[~keep] == 0).all():
                            fails.append(f"{tag}: a dropped dXdrop element is not exactly zero")
                    for name, t in zip(("pdw", "pdb", "pdbias"), parts):
                        worst.f32(name, *R.check_f32(f"{tag} {name}", t, m[name], ref[name], sc[name], fails, log))
                    print("\n".join(log))
    worst.report(f"bwd H={H} {'f32' if x32 else 'bf16'}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------- mask agreement
def _ln_bwd_bits(k, dev, rows, H, p, seed, x32=False):
    """layernorm_bwd with dropout on Gaussian inputs -> (dX != 0, dXdrop != 0)"""
    Xc, wc, bc, dYc, _ = R.ln_inputs(rows, H, "gauss", seed=rows + H, f32=x32)
    X, w, b, dY = (t.to(dev) for t in (Xc, wc, bc, dYc))
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    Y = torch.empty(rows, H, dtype=bf16, device=dev)
    (k.layernorm_fwd_f32 if x32 else k.layernorm_fwd)(X, w, b, Y, mean=mean, rstd=rstd, eps=EPS)
    dX = torch.full((rows, H), NAN, dtype=bf16, device=dev)
    dXd = torch.full((rows, H), NAN, dtype=bf16, device=dev)
    k.layernorm_bwd(dY, X, mean, rstd, w, dX, dXd, p, seed)
    torch.cuda.synchronize()
    assert torch.isfinite(dX.float()).all() and torch.isfinite(dXd.float()).all()
    return dX != 0, dXd != 0


MASK_SHAPES = [(300, 256, 1), (512 + 37, 768, 1), (130, 768, 3)]


@pytest.mark.parametrize("M,N,batch", MASK_SHAPES, ids=[f"M{m}-N{n}-b{b}" for m, n, b in MASK_SHAPES])
def test_layernorm_bwd_mask_is_the_gemm_epilogues(dev, M, N, batch):
    """the backward's regenerated keep bits are the bits the BIAS_DROP_RES epilogue drew: the
    GEMM's counter (z M + m) N + n and the LayerNorm's row H + c name the same element"""
    k = K()
    rows = batch * M
    for seed in (0, 1, 2 ** 40 + 5):
        for p in (0.1, 0.5):
            keep = probe_keep(k, dev, M, N, p, seed, batch)
            nz, nzd = _ln_bwd_bits(k, dev, rows, N, p, seed, x32=(seed == 1))
            excluded = (~nz).sum().item() / nz.numel()
            rate = 1.0 - keep.float().mean().item()
            print(f"[M={M} N={N} batch={batch} seed={seed} p={p}] drop rate {rate:.4f}, dX == 0 share {excluded:.2e}")
            assert excluded <= 1e-4, f"seed={seed} p={p}: {excluded:.3e} of dX is zero"
            assert abs(rate - p) <= 4.0 * (p * (1 - p) / keep.numel()) ** 0.5, f"seed={seed} p={p}: drop rate {rate}"
            bad = (nzd != (keep & nz)).sum().item()
            assert bad == 0, f"seed={seed} p={p}: {bad} of {keep.numel()} dXdrop elements disagree with the forward mask"


def test_layernorm_bwd_mask_follows_the_seed_offset(dev):
    """under a non-zero seed-offset counter (graph replays) both kernels fold it in alike: the
    bits still agree with each other, and differ from the zero-offset bits"""
    k = K()
    M, N, p, seed = 549, 768, 0.1, 7
    keep0 = probe_keep(k, dev, M, N, p, seed)
    ctr = torch.tensor([5], dtype=torch.int64, device=dev)
    try:
        k.set_seed_offset(ctr)
        keep = probe_keep(k, dev, M, N, p, seed)
        nz, nzd = _ln_bwd_bits(k, dev, M, N, p, seed)
        ctr.zero_()  # a counter of 0 leaves the seed as given
        keep_z = probe_keep(k, dev, M, N, p, seed)
        _, nzd_z = _ln_bwd_bits(k, dev, M, N, p, seed)
    finally:
        k.set_seed_offset(None)
    assert torch.equal(nzd, keep & nz)
    assert not torch.equal(keep, keep0)
    assert (keep != keep0).float().mean().item() > 0.5 * 2 * p * (1 - p)  # an independent draw differs on 2 p (1-p)
    assert torch.equal(keep_z, keep0) and torch.equal(nzd_z, keep0 & nz)
