"""The BatchNorm kernels (csrc/batchnorm.hip: bn_stats, bn_fwd_finalize, the nine bn_apply arms,
bn_bwd_reduce / _finalize / _apply, bn_local_sums and the cross-rank halves) against float64 at
every work split bn_grid chooses, through guarded buffers.

Cases (bn_harness.bn_cases): C = 8, 24, 64, 96, 256, 520, 2048 (channel chunk CH = 8, 8 x 3, 64,
32 x 3, 256, 8 x 65, 512 x 4: one thread per row up to 64, grid.y 1 to 65); rows 2, 3, rpi - 1,
rpi + 1, rpb, rpb + 1, 2 rpb + rpi + 1 and 33 rpb + 1 (a last block shorter than one iteration, one
to three row blocks, 34 partials wrapping the finalize's 32 slices), and every row count 2..70 at
C = 2048 and 256; inputs N(0, 1), mean 8 x the spread, channel scales 2^-4..2^4, exactly constant
channels, and a last row / first row of the last block 16 x the rest ("unit" and "tail" everywhere,
the others at C = 8, 96, 2048).  Rows are the H of a [1, C, rows, 1] channels-last map.  The grid
rows run every arm, the dense rows three forward and two backward arms rotating with the row count
(the arms differ in the elementwise part alone, the row count in the loops every arm shares).

Buffers: X, skip, dY, Y, dX, dSkip, the ReLU mask, both stream residues, every per-channel f32
vector, the f64 sums and num_batches_tracked are views inside larger allocations (tests/guarded.py):
input guards hold NaN, outputs a canary; afterwards the live region is written and the guards are
bit-identical.  The 8-element margin keeps every alignment the kernels assume: 16 B for the bf16
maps (bf16x8 accesses), 8 B for the int8 residues (uint2), 32 B for the f32 vectors (float4 loads of
the saved mean), 64 B for the f64 sums.

Bars (rowops_harness / bn_harness): elementwise 2^-8 |ref| + 64 * 2^-24 scale (not on Y for the
"offset" and "const" inputs, nor on dX for "offset" against float64 statistics, where the float32
model itself misses it: bn_harness.ELEM_Y_KINDS); channel error <= 2 x / 1.5 x the model's max /
median; f32 outputs within 8 x the model's error or 4 ulps; mask bits == (Y > 0) of the kernel's own
Y; the decoded stream within 2^-13 of max |ref|; masked and unmasked arms bit-identical;
num_batches_tracked exact.  The backward is compared twice: with the float64 reference fed the
kernel's own saved mean / invstd (the backward kernels alone) and fed float64 statistics (end to
end; the model then runs from the model's own forward statistics).

Measured on an MI355X over the whole sweep: DESIGN.md, "BatchNorm and BertAdam edge sweeps".
"""
import pytest
import torch

import bn_harness as B
import rowops_harness as R
from guarded import check_written, guarded_input, inout_buf, out_buf
from rowops_harness import Worst

pytestmark = pytest.mark.gpu

bf16, f32t = torch.bfloat16, torch.float32
EPS = B.BN_EPS


def K():
    from src import kernels
    return kernels


def as_map(t):
    """[rows, C] -> the [1, C, rows, 1] channels-last map over the same memory"""
    rows, C = t.shape
    return t.view(1, rows, 1, C).permute(0, 3, 1, 2)


def _dense(C, rows):
    return rows not in B.bn_rows(C)


def _dev_inputs(dev, d):
    return {k: guarded_input(dev, v) for k, v in d.items()}


# ------------------------------------------------------------------------------- forward
def _run_fwd(k, dev, g, arm, rows, C, mom, nbt0, sums=None):
    """one forward launch of `arm` on the device inputs g -> (bufs, outputs dict)"""
    training, relu, mask, skip, sres, yres = B.FWD_ARMS[arm]
    bufs, o = {}, {}
    bufs["Y"], o["Y"] = out_buf(dev, bf16, rows, C)
    bufs["rmean"], o["rmean"] = inout_buf(dev, g["rm0"])
    bufs["rvar"], o["rvar"] = inout_buf(dev, g["rv0"])
    bufs["nbt"], o["nbt"] = inout_buf(dev, torch.tensor([nbt0], dtype=torch.int64), fill=-7)
    kw = {}
    if training:
        bufs["mean"], o["mean"] = out_buf(dev, f32t, C)
        bufs["invstd"], o["invstd"] = out_buf(dev, f32t, C)
        kw.update(save_mean=o["mean"], save_invstd=o["invstd"])
    if mask:
        bufs["mask"], o["mask"] = out_buf(dev, torch.uint8, rows * C // 8, fill=0xA5)
        kw["relu_mask"] = o["mask"]
    if yres:
        bufs["yres"], o["yres"] = out_buf(dev, torch.int8, rows * C, fill=85)
        kw["y_res"] = o["yres"]
    if skip:
        kw["skip"] = as_map(g["skip_s"] if sres else g["skip"])
    if sres:
        kw["skip_res"] = g["skip_res"].view(-1)
    X, Y = as_map(g["X"]), as_map(o["Y"])
    if sums is not None:
        k.batchnorm_fwd_sums(X, Y, sums, g["w"], g["b"], o["rmean"], o["rvar"], mom, EPS, relu=relu,
                             num_batches_tracked=o["nbt"], **kw)
    else:
        k.batchnorm_fwd(X, Y, g["w"], g["b"], o["rmean"], o["rvar"], training, mom, EPS, relu=relu,
                        num_batches_tracked=o["nbt"], **kw)
    torch.cuda.synchronize()
    return bufs, o


def _check_fwd(tag, arm, kind, o, m, ref, sc, mom, nbt0, g, fails, log, worst):
    training, relu, mask, skip, sres, yres = B.FWD_ARMS[arm]
    rows, C = o["Y"].shape
    el, st = B.check_map(f"{tag} Y", o["Y"], m["Y"], ref["Y"], sc["Y"], fails, log, B.elem_bar("Y", kind))
    worst.bf("Y", el if B.elem_bar("Y", kind) else 0.0, st)
    if training:
        for key in ("mean", "invstd", "rmean", "rvar"):
            worst.f32(key, *R.check_f32(f"{tag} {key}", o[key], m[key], ref[key], sc[key], fails, log))
        want = nbt0 + 1 if mom >= 0 else nbt0
    else:
        want = nbt0
        if not (torch.equal(o["rmean"], g["rm0"]) and torch.equal(o["rvar"], g["rv0"])):
            fails.append(f"{tag}: eval changed the running statistics")
    if o["nbt"].item() != want:
        fails.append(f"{tag}: num_batches_tracked {o['nbt'].item()}, expected {want}")
    if mask and not torch.equal(B.mask_bools(o["mask"], rows, C), o["Y"].float() > 0):
        fails.append(f"{tag}: mask bits differ from Y > 0")
    if yres:
        se = B.stream_error(o["Y"], o["yres"].view(rows, C), ref["Y"])
        worst.f32("stream (of max |ref|, bar 2^-13)", se, 0.0, se / B.RES_BAR)
        if not se <= B.RES_BAR:
            fails.append(f"{tag}: decoded stream {se:.3e} of max |ref| > 2^-13")


def _fwd_kwargs(arm, g, mom, nbt):
    training, relu, _, skip, sres, _ = B.FWD_ARMS[arm]
    return dict(training=training, rmean=g["rm0"], rvar=g["rv0"], momentum=mom, nbt=nbt, relu=relu,
                skip=(g["skip_s"] if sres else g["skip"]) if skip else None, skip_res=g["skip_res"] if sres else None)


FWD = list(B.FWD_ARMS)
SAME_Y = (("relu", "relu+mask"), ("skip+relu", "skip+relu+mask"))


@pytest.mark.parametrize("C", B.BN_C)
def test_batchnorm_forward_edges(dev, C):
    k = K()
    fails, worst = [], Worst()
    for idx, (rows, kind) in enumerate(B.bn_cases(C)):
        g = _dev_inputs(dev, B.bn_inputs(rows, C, kind, seed=C + rows))
        sums = B.bn_stats_model(g["X"]) + (rows,)
        # momentum 0.1 (the kernel counts the pass) or the cumulative average at a count of 3 (it does not)
        mom, nbt0 = (0.1, 0) if idx % 2 else (-1.0, 3)
        nbt = nbt0 + 1 if mom >= 0 else nbt0
        arms = FWD if not _dense(C, rows) else ["stream", FWD[rows % len(FWD)], FWD[(rows + 3) % len(FWD)]]
        ys = {}
        for arm in arms:
            tag = f"{kind} C={C} rows={rows} {arm}"
            log = []
            kw = _fwd_kwargs(arm, g, mom, nbt)
            ref, sc = B.bn_fwd_ref(g["X"], g["w"], g["b"], EPS, **kw)
            m = B.bn_fwd_model(g["X"], g["w"], g["b"], EPS, sums=sums if kw["training"] else None, **kw)
            bufs, o = _run_fwd(k, dev, g, arm, rows, C, mom, nbt0)
            check_written(bufs, fails, tag)
            _check_fwd(tag, arm, kind, o, m, ref, sc, mom, nbt0, g, fails, log, worst)
            ys[arm] = o["Y"]
            print("\n".join(log))
        for a, b in SAME_Y:
            if a in ys and b in ys and not torch.equal(ys[a].view(torch.int16), ys[b].view(torch.int16)):
                fails.append(f"{kind} C={C} rows={rows}: Y of {a} and {b} differ")
    worst.report(f"bn fwd C={C}")
    assert not fails, "\n".join(fails[:40])


# ------------------------------------------------------------------------------- backward
def _own_forward(k, dev, g, rows, C):
    """the kernel's own forward (ReLU + mask): Y, the mask bytes, the saved mean / invstd"""
    Y = torch.empty(rows, C, dtype=bf16, device=dev)
    mask = torch.empty(rows * C // 8, dtype=torch.uint8, device=dev)
    sm, si = torch.empty(C, device=dev), torch.empty(C, device=dev)
    k.batchnorm_fwd(as_map(g["X"]), as_map(Y), g["w"], g["b"], None, None, True, 0.1, EPS, relu=True, save_mean=sm,
                    save_invstd=si, relu_mask=mask)
    return (guarded_input(dev, Y.cpu()), guarded_input(dev, mask.cpu()), guarded_input(dev, sm.cpu()),
            guarded_input(dev, si.cpu()))


def _run_bwd(k, dev, g, arm, Y, mask, sm, si, rows, C, sums=None, init=None):
    relu, from_mask, dskip = B.BWD_ARMS[arm]
    bufs, o = {}, {}
    bufs["dX"], o["dX"] = out_buf(dev, bf16, rows, C)
    if dskip:
        bufs["dSkip"], o["dSkip"] = out_buf(dev, bf16, rows, C)
    dS = as_map(o["dSkip"]) if dskip else None
    yk = as_map(Y) if relu and not from_mask else None
    mk = mask if relu and from_mask else None
    if sums is not None:
        k.batchnorm_bwd_sums(as_map(g["dY"]), yk, as_map(g["X"]), sums, g["w"], sm, si, relu, as_map(o["dX"]), dS,
                             relu_mask=mk)
    else:
        bufs["dw"], o["dw"] = inout_buf(dev, g["dw0"] if init is None else init[0])
        bufs["db"], o["db"] = inout_buf(dev, g["db0"] if init is None else init[1])
        k.batchnorm_bwd(as_map(g["dY"]), yk, as_map(g["X"]), g["w"], sm, si, relu, as_map(o["dX"]), dS, o["dw"],
                        o["db"], relu_mask=mk)
    torch.cuda.synchronize()
    return bufs, o


def _check_bwd(tag, kind, o, refs, fails, log, worst, grads=True):
    """refs: [(which, ref, scales, model)] -- the reference fed the kernel's own statistics, then float64 ones"""
    for which, ref, sc, m in refs:
        elem = B.elem_bar("dX", kind, which)
        el, st = B.check_map(f"{tag} dX ({which} stats)", o["dX"], m["dX"], ref["dX"], sc["dX"], fails, log, elem)
        worst.bf(f"dX {which}", el if elem else 0.0, st)
        if grads:
            for key in ("dw", "db"):
                worst.f32(f"{key} {which}", *R.check_f32(f"{tag} {key} ({which} stats)", o[key], m[key], ref[key],
                                                         sc[key], fails, log))
    if "dSkip" in o and not torch.equal(o["dSkip"].float().double(), refs[0][1]["dSkip"]):
        fails.append(f"{tag}: dSkip is not dY * mask")


def _bwd_refs(g, mask_b, sm, si, fm, fr, dw0, db0, **model_kw):
    own = B.bn_bwd_ref(g["dY"], mask_b, g["X"], g["w"], sm, si, dw0, db0)
    f64 = B.bn_bwd_ref(g["dY"], mask_b, g["X"], g["w"], fr["mean"], fr["invstd"], dw0, db0)
    return [("own", own[0], own[1], B.bn_bwd_model(g["dY"], mask_b, g["X"], g["w"], sm, si, dw0, db0, **model_kw)),
            ("f64", f64[0], f64[1], B.bn_bwd_model(g["dY"], mask_b, g["X"], g["w"], fm["mean"], fm["invstd"], dw0, db0,
                                                  **{k: v for k, v in model_kw.items() if k != "sums"}))]


BWD = list(B.BWD_ARMS)
BWD_DENSE = (("relu-y+dskip", "relu-mask+dskip"), ("plain+dskip", "relu-mask"), ("relu-y", "relu-mask"), ("plain",
                                                                                                         "relu-y+dskip"))
SAME_DX = (("relu-y", "relu-mask"), ("relu-y+dskip", "relu-mask+dskip"))


@pytest.mark.parametrize("C", B.BN_C)
def test_batchnorm_backward_edges(dev, C):
    k = K()
    fails, worst = [], Worst()
    for idx, (rows, kind) in enumerate(B.bn_cases(C)):
        g = _dev_inputs(dev, B.bn_inputs(rows, C, kind, seed=C + rows))
        Y, mask, sm, si = _own_forward(k, dev, g, rows, C)
        fm = B.bn_fwd_model(g["X"], g["w"], g["b"], EPS)
        fr, _ = B.bn_fwd_ref(g["X"], g["w"], g["b"], EPS)
        arms = BWD if not _dense(C, rows) else BWD_DENSE[rows % len(BWD_DENSE)]
        refs, outs = {}, {}
        for arm in arms:
            relu = B.BWD_ARMS[arm][0]
            tag = f"{kind} C={C} rows={rows} {arm}"
            log = []
            if relu not in refs:  # g = dY * (the kernel's own Y > 0): a ReLU tie at zero is never a failure
                refs[relu] = _bwd_refs(g, (Y.float() > 0) if relu else None, sm, si, fm, fr, g["dw0"], g["db0"])
            bufs, o = _run_bwd(k, dev, g, arm, Y, mask, sm, si, rows, C)
            check_written(bufs, fails, tag)
            _check_bwd(tag, kind, o, refs[relu], fails, log, worst)
            outs[arm] = o
            print("\n".join(log))
        for a, b in SAME_DX:
            if a in outs and b in outs:
                for key in outs[a]:
                    if not torch.equal(outs[a][key], outs[b][key]):
                        fails.append(f"{kind} C={C} rows={rows}: {key} of {a} and {b} differ")
    worst.report(f"bn bwd C={C}")
    assert not fails, "\n".join(fails[:40])


# ------------------------------------------------------------------------------- cross-rank halves
def _splits(C):
    """ragged splits of a batch over two ranks: 2 rows | the rest, and rpb + 1 | rpi - 1"""
    g0 = B.bn_geometry(2, C)
    rpi, rpb = g0["rpi"], g0["rpb"]
    return [(2, 2 * rpb + rpi - 1), (rpb + 1, rpi - 1)]


def _half(d, lo, hi):
    return {k: (v[lo:hi] if v.dim() == 2 else v) for k, v in d.items()}


@pytest.mark.parametrize("C", B.BN_C)
def test_batchnorm_cross_rank_edges(dev, C):
    """batchnorm_stats -> add -> batchnorm_fwd_sums and batchnorm_bwd_reduce -> add ->
    batchnorm_bwd_sums over two ragged halves, every half against the float64 whole-batch
    reference with the sweep's bars; the halves' dweight / dbias sum to the reference's."""
    k = K()
    fails, worst = [], Worst()
    kinds = B.KINDS if C in B.BN_ALL_KINDS_C else ("unit", "tail")
    for si_, (r0, r1) in enumerate(_splits(C)):
        rows = r0 + r1
        for kind in kinds:
            d = B.bn_inputs(rows, C, kind, seed=C + rows + 1)
            whole = {k_: v.to(dev) for k_, v in d.items()}
            halves = [_dev_inputs(dev, _half(d, 0, r0)), _dev_inputs(dev, _half(d, r0, rows))]
            hrows = (r0, r1)
            # forward first half: the local sums
            lsums, msum = [], [0.0, 0.0]
            for h, gh in enumerate(halves):
                gs, sv = out_buf(dev, torch.float64, 2 * C + 1)
                k.batchnorm_stats(as_map(gh["X"]), sv)
                torch.cuda.synchronize()
                check_written({"sums": gs}, fails, f"{kind} C={C} split={r0}|{r1} stats rank {h}")
                if sv[2 * C].item() != hrows[h]:
                    fails.append(f"{kind} C={C} split={r0}|{r1}: rank {h} row count {sv[2 * C].item()}")
                lsums.append(sv)
                ms = B.bn_stats_model(gh["X"])
                msum = [msum[0] + ms[0], msum[1] + ms[1]]
            tot = guarded_input(dev, (lsums[0] + lsums[1]).cpu())
            sums_m = (msum[0], msum[1], rows)
            for arm in ("plain", "skip+relu+mask", "stream"):
                mom, nbt0 = (0.1, 0) if si_ else (-1.0, 3)
                nbt = nbt0 + 1 if mom >= 0 else nbt0
                ref, sc = B.bn_fwd_ref(whole["X"], whole["w"], whole["b"], EPS, **_fwd_kwargs(arm, whole, mom, nbt))
                saved = []
                for h, gh in enumerate(halves):
                    lo, hi = (0, r0) if h == 0 else (r0, rows)
                    tag = f"{kind} C={C} split={r0}|{r1} rank {h} {arm}"
                    log = []
                    m = B.bn_fwd_model(gh["X"], gh["w"], gh["b"], EPS, sums=sums_m, **_fwd_kwargs(arm, gh, mom, nbt))
                    bufs, o = _run_fwd(k, dev, gh, arm, hrows[h], C, mom, nbt0, sums=tot)
                    check_written(bufs, fails, tag)
                    rh = dict(ref, Y=ref["Y"][lo:hi])
                    sh = dict(sc, Y=sc["Y"][lo:hi])
                    _check_fwd(tag, arm, kind, o, m, rh, sh, mom, nbt0, gh, fails, log, worst)
                    saved.append(o)
                    print("\n".join(log))
                if not (torch.equal(saved[0]["mean"], saved[1]["mean"]) and
                        torch.equal(saved[0]["invstd"], saved[1]["invstd"])):
                    fails.append(f"{kind} C={C} split={r0}|{r1} {arm}: the ranks' saved statistics differ")
                if arm != "skip+relu+mask":
                    continue
                # backward: reduce -> add -> apply, from the mask (skip + ReLU) and without ReLU
                sm, si = guarded_input(dev, saved[0]["mean"].cpu()), guarded_input(dev, saved[0]["invstd"].cpu())
                fm = B.bn_fwd_model(whole["X"], whole["w"], whole["b"], EPS, sums=sums_m)
                for relu in (True, False):
                    barm = "relu-mask+dskip" if relu else "plain"
                    Ys = [guarded_input(dev, o["Y"].cpu()) for o in saved]
                    Ms = [guarded_input(dev, o["mask"].cpu()) for o in saved]
                    mask_w = (torch.cat([o["Y"] for o in saved]).float() > 0) if relu else None
                    bsums, dws, dbs, mloc, inits = [], [], [], [], []
                    for h, gh in enumerate(halves):
                        tag = f"{kind} C={C} split={r0}|{r1} rank {h} reduce relu={relu}"
                        gs, sv = out_buf(dev, torch.float64, 2 * C + 1)
                        init = (gh["dw0"] * (0.5 * (h + 1)), gh["db0"] * (0.5 * (h + 1)))
                        gw, dw = inout_buf(dev, init[0])
                        gb, db = inout_buf(dev, init[1])
                        k.batchnorm_bwd_reduce(as_map(gh["dY"]), None, as_map(gh["X"]), sm, si, relu, sv, dw, db,
                                               relu_mask=Ms[h] if relu else None)
                        torch.cuda.synchronize()
                        check_written({"sums": gs, "dw": gw, "db": gb}, fails, tag)
                        if sv[2 * C].item() != hrows[h]:
                            fails.append(f"{tag}: row count {sv[2 * C].item()}")
                        bsums.append(sv)
                        dws.append(dw.double())
                        dbs.append(db.double())
                        inits.append(init)
                        mh = None if mask_w is None else (mask_w[:r0] if h == 0 else mask_w[r0:])
                        mloc.append(B.bn_bwd_sums_model(gh["dY"], mh, gh["X"], sm))
                    btot = guarded_input(dev, (bsums[0] + bsums[1]).cpu())
                    bs_m = (mloc[0][0] + mloc[1][0], mloc[0][1] + mloc[1][1], rows)
                    dw0 = inits[0][0].double() + inits[1][0].double()
                    db0 = inits[0][1].double() + inits[1][1].double()
                    fr, _ = B.bn_fwd_ref(whole["X"], whole["w"], whole["b"], EPS)
                    refs = _bwd_refs(whole, mask_w, sm, si, fm, fr, dw0, db0, sums=bs_m)
                    # the halves' dweight / dbias (each rank's model: its own sums into its own initial values)
                    md = {"dw": 0.0, "db": 0.0}
                    for h, gh in enumerate(halves):
                        mh = None if mask_w is None else (mask_w[:r0] if h == 0 else mask_w[r0:])
                        mm = B.bn_bwd_model(gh["dY"], mh, gh["X"], gh["w"], sm, si, inits[h][0], inits[h][1], sums=bs_m,
                                            local=mloc[h])
                        md = {key: md[key] + mm[key].double() for key in md}
                    tag = f"{kind} C={C} split={r0}|{r1} relu={relu}"
                    log = []
                    own = refs[0]
                    worst.f32("dw halves", *R.check_f32(f"{tag} dw halves", dws[0] + dws[1], md["dw"], own[1]["dw"],
                                                        own[2]["dw"], fails, log))
                    worst.f32("db halves", *R.check_f32(f"{tag} db halves", dbs[0] + dbs[1], md["db"], own[1]["db"],
                                                        own[2]["db"], fails, log))
                    for h, gh in enumerate(halves):
                        lo, hi = (0, r0) if h == 0 else (r0, rows)
                        htag = f"{tag} rank {h} {barm}"
                        bufs, o = _run_bwd(k, dev, gh, barm, Ys[h], Ms[h], sm, si, hrows[h], C, sums=btot)
                        check_written(bufs, fails, htag)
                        hrefs = [(w_, {"dX": r_["dX"][lo:hi], "dSkip": r_["dSkip"][lo:hi]}, {"dX": s_["dX"][lo:hi]},
                                  {"dX": m_["dX"][lo:hi]}) for w_, r_, s_, m_ in refs]
                        _check_bwd(htag, kind, o, hrefs, fails, log, worst, grads=False)
                    print("\n".join(log))
    worst.report(f"bn cross-rank C={C}")
    assert not fails, "\n".join(fails[:40])
