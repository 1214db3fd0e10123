"""The MFMA GEMM and its fused epilogues (csrc/gemm.hip through kernels.gemm), and the column-sum,
column-fold and transpose kernels of the same file, against float64 at the shapes where each path
of the host's plan begins, through guarded buffers.

Cases (gemm_harness.GROUPS, chosen and labelled by gemm_harness.gemm_plan): the M boundaries of the
lane-row groups (8), MFMA sub-tiles (16), wave blocks (64 / 128) and tiles in the 128^2, 256^2 and
256 x 384 tilings; M-major A and N-major B with half a tile of dead rows / columns; 1, 2, 3, 5
k-steps K-major and K = 1 .. 1000 with both operands M/N-major; tile order and XCD remap at every
workgroup count mod 8, ragged groups of 2 and 8, batch 2 and 3; split-K with short last slices and
capped workspaces; the split tail rows on both big tilings (the only large shapes); every epilogue
kind 0-5 in all four layouts at batch 2 with every batch stride gapped, aux present and NULL, drop_p
0 / 0.1 / 0.5; the table kinds 6-8 with partly filled last blocks; column sums by partial rows and
by atomics from a non-zero initial value; mmu_gemm_rows' row-stepped dropout counter up to 2^33.

Buffers (tests/guarded.py): every operand is a view inside a larger allocation with a padded leading
dimension (+8, +16 or +24 elements; f32 +4) and, at batch > 1, gap rows between the batch items.
Input guards, paddings and gaps hold NaN: with M-major A / N-major B the accumulators of the dead
rows and columns of a tile are fed from them, and none of it may reach C, the column sums or the
tables.  Outputs are followed by 256 canary rows, so a store that ignores m < M lands in the canary;
after every launch the live regions are finite, everything else is bit-identical, and the inputs
are unchanged.

Bars (rowops_harness): bf16 outputs 2^-8 |ref| + 64 * 2^-24 scale on every element and the row error
against the float32 model; f32 outputs within 8 x the model's error or 4 ulps; "int" inputs into an
f32 C bit for bit; dropped elements exactly the residual (bf16, f32) or exactly 0 (QuickGELU, C and
aux); tables against float64 sums over the kernel's own stored C.

Measured on an MI355X over the whole sweep: DESIGN.md, "GEMM edge sweep".
"""
import pytest
import torch

import gemm_harness as H
from guarded import NAN, Guarded, check_written, guarded_input, out_buf, probe_keep
from rowops_harness import Worst, check_f32

pytestmark = pytest.mark.gpu

bf16, f32t = torch.bfloat16, torch.float32
GUARD_ROWS = 256
SEED = 0x5EED0001234
ENV_KEYS = ("MMU_GEMM_WIDE", "MMU_GEMM_WIDE_MIN_TILES", "MMU_GEMM_TAIL", "MMU_GEMM_CS_PART")


def K():
    from src import kernels
    return kernels


def as_map(t):
    """[rows, C] -> the [1, C, rows, 1] channels-last map over the same memory"""
    rows, C = t.shape
    return t.view(1, rows, 1, C).permute(0, 3, 1, 2)


def pack_bits(mask):
    """[M, N] bool -> [M * N / 8] u8: bit e of byte (m, n / 8) = mask[m, n + e]"""
    M, N = mask.shape
    w = (1 << torch.arange(8, device=mask.device)).to(torch.int32)
    return (mask.view(M, N // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).reshape(-1)


def place_rows(dev, dtype, batch, R, W, pad, gap, data=None, guard=None):
    """batch items of [R, W] in rows of pitch W + pad, `gap` rows between the items, NaN everywhere
    else -> (Guarded, ld, batch stride).  data [batch, R, W] or None (an output left at the canary)"""
    ld, rows = W + pad, batch * (R + gap) - gap
    live = torch.zeros(rows, dtype=torch.bool)
    for z in range(batch):
        live[z * (R + gap):z * (R + gap) + R] = True
    g = Guarded(dev, dtype, NAN, rows, W, ld, guard=guard, live=live)
    if data is not None:
        for z in range(batch):
            g.view[z * (R + gap):z * (R + gap) + R] = data[z].to(dtype)
        g.set_canary()
    return g, ld, (R + gap) * ld


def read_rows(g, batch, R, gap):
    return torch.stack([g.view[z * (R + gap):z * (R + gap) + R] for z in range(batch)])


def place_vec(dev, data, stride, dtype=f32t):
    """[batch, n] -> a contiguous guarded vector with item z at z * stride, NaN between"""
    batch, n = data.shape
    total = (batch - 1) * stride + n
    live = torch.zeros(total, dtype=torch.bool)
    for z in range(batch):
        live[z * stride:z * stride + n] = True
    g = Guarded(dev, dtype, NAN, total, live=live)
    for z in range(batch):
        g.view[z * stride:z * stride + n] = data[z]
    g.set_canary()
    return g


def read_vec(g, batch, n, stride):
    return torch.stack([g.view[z * stride:z * stride + n] for z in range(batch)])


def run_case(k, dev, mp, c, seed, fails, log, worst):
    tag = c["name"]
    for key in ENV_KEYS:
        mp.delenv(key, raising=False)
    for key, v in c["env"].items():
        mp.setenv(key, v)
    M, N, Kd, batch, kind, c_f32, p = c["M"], c["N"], c["K"], c["batch"], c["kind"], c["c_f32"], c["p"]
    ak, bk, rows = c["ak"], c["bk"], c["rows"]
    A, B = H.gemm_inputs(c["inp"], M, N, Kd, batch, seed, device=dev)
    e = H.epi_inputs(kind, M, N, batch, seed, c_f32=c_f32, ints=(c["inp"] == "int"), bias=c["bias"],
                     accumulate=c["accumulate"], colsum=c["colsum"], res_ln=c["res_ln"], bn_mask=c["bn_mask"],
                     res_mask=c["res_mask"], device=dev)
    drop = kind in (H.BIAS_DROP_RES, H.BIAS_DROP_QGELU) and p > 0
    keep = H.keep_bits(SEED, M, N, batch, p, *(rows or (1, 0))).to(dev) if drop else None
    pl = H.plan_of(c)
    ref, sc = H.gemm_ref(A, B, kind, e, keep, p)
    if c["exact"]:
        model = {"C": ref["C"].float()}
    else:
        model = H.gemm_model32(A, B, kind, e, keep, p, c_f32=c_f32, kchunk=pl["kchunk"] if pl["splitk"] > 1 else None,
                               tail=(pl["m_main"], pl["tail_chunk"]) if pl["tail_rows"] else None)
    # ---- buffers
    pad = H.pad_of(c)
    pads = [H.PADS[(H.PADS.index(pad) + j) % 3] for j in range(5)]
    gapA, gapB, gapC, gapR, gapX = (3, 1, 5, 2, 4) if batch > 1 else (0, 0, 0, 0, 0)
    ins, outs = {}, {}
    a_st = A if ak else A.transpose(1, 2)
    b_st = B if bk else B.transpose(1, 2)
    ins["A"], lda, sA = place_rows(dev, bf16, batch, a_st.shape[1], a_st.shape[2], pads[0], gapA, a_st)
    ins["B"], ldb, sB = place_rows(dev, bf16, batch, b_st.shape[1], b_st.shape[2], pads[1], gapB, b_st)
    bnb = kind in (H.STORE_BNB, H.ADD_RES_BNB)
    cdt = f32t if c_f32 else bf16
    outs["C"], ldc, sC = place_rows(dev, cdt, batch, M, N, 0 if bnb else 4 if c_f32 else pads[2], gapC, e.get("c0"),
                                    guard=GUARD_ROWS)
    kw = {}
    BS, CS, LS = N + 12, N + 20, N + 8      # bias / colsum / res_ln batch strides: none of them N
    if "bias" in e:
        ins["bias"] = place_vec(dev, e["bias"], BS)
        kw.update(bias=ins["bias"].view, bias_bstride=BS)
    if "residual" in e:
        r32 = e["residual"].dtype == f32t
        ins["residual"], ldr, sR = place_rows(dev, e["residual"].dtype, batch, M, N,
                                              0 if c["res_mask"] else 4 if r32 else pads[3], gapR, e["residual"])
        kw.update(residual=ins["residual"].view, ldr=ldr, res_bstride=sR)
    if kind == H.DGELU:
        ins["aux"], ldx, sX = place_rows(dev, bf16, batch, M, N, pads[4], gapX, e["aux_in"])
        kw.update(aux=ins["aux"].view, ldx=ldx, aux_bstride=sX)
    elif kind in (H.BIAS_GELU, H.BIAS_DROP_QGELU) and c["aux"]:
        outs["aux"], ldx, sX = place_rows(dev, bf16, batch, M, N, pads[4], gapX, guard=GUARD_ROWS)
        kw.update(aux=outs["aux"].view, ldx=ldx, aux_bstride=sX)
    P = (M + 63) // 64
    if kind >= H.STORE_STATS:
        outs["table"], table = out_buf(dev, f32t, P * N * 2, guard=8 * N)
        kw.update(colsum=table)
    elif "cs0" in e:
        outs["colsum"] = place_vec(dev, e["cs0"], CS)
        kw.update(colsum=outs["colsum"].view, colsum_bstride=CS)
    if "ln" in e:
        mean, rstd, w, b = e["ln"]
        ins["ln_w"], ins["ln_b"] = place_vec(dev, w, LS), place_vec(dev, b, LS)
        kw.update(res_ln=(guarded_input(dev, mean.reshape(-1).cpu()), guarded_input(dev, rstd.reshape(-1).cpu()),
                          ins["ln_w"].view, ins["ln_b"].view), res_ln_bstride=LS)
    if "bn" in e:
        x, mask, mean = e["bn"]
        ins["bn_x"], _, _ = place_rows(dev, bf16, 1, M, N, 0, 0, x[None])
        kw.update(bn=(as_map(ins["bn_x"].view), None if mask is None else guarded_input(dev, pack_bits(mask).cpu()),
                      guarded_input(dev, mean.cpu())))
    if e.get("res_mask") is not None:
        kw.update(res_mask=guarded_input(dev, pack_bits(e["res_mask"]).cpu()))
    epi = k.epilogue(kind, drop_p=p, seed=SEED, accumulate=c["accumulate"], **kw)
    if c["ws_slices"] is not None:
        outs["workspace"], ws = out_buf(dev, f32t, c["ws_slices"] * batch * M * N, guard=1024)
        epi.workspace, epi.workspace_floats = ws.data_ptr(), ws.numel()

    def launch(with_rows):
        k.gemm(ins["A"].view, lda, ak, ins["B"].view, ldb, bk, outs["C"].view, ldc, M, N, Kd, epi=epi, batch=batch,
               sA=sA, sB=sB, sC=sC, row_step=rows[0] if with_rows else None, row_offset=rows[1] if with_rows else 0)
        torch.cuda.synchronize()
    launch(rows is not None)
    # ---- what was written, and where
    ws_buf = outs.pop("workspace", None)
    if ws_buf is not None and not ws_buf.guards_intact():
        fails.append(f"{tag}: wrote outside the caller's workspace")
    if ws_buf is not None:      # ("int" inputs: every slab element is finite) the launch followed the queried plan
        used, slabs = int(torch.isfinite(ws_buf.view).sum()), pl["splitk"] * batch * M * N if pl["splitk"] > 1 else 0
        if used != slabs:
            fails.append(f"{tag}: {used} workspace floats written, the queried plan ({pl['splitk']} slices) has {slabs}")
    check_written(outs, fails, tag)
    for name, g in ins.items():
        if not g.unchanged():
            fails.append(f"{tag} {name}: an input was changed")
    out = {"C": read_rows(outs["C"], batch, M, gapC)}
    if "aux" in outs:
        out["aux"] = read_rows(outs["aux"], batch, M, gapX)
    if "colsum" in outs:
        out["colsum"] = read_vec(outs["colsum"], batch, N, CS)
    if "table" in outs:
        out["table"] = outs["table"].view.view(P, N, 2)
        ref["table"], sc["table"] = H.table_ref(out["C"][0], kind, e)
        model["table"] = H.table_model(out["C"][0], kind, e)
    if not all(torch.isfinite(v.float()).all() for v in out.values()):
        return                                              # (check_written has said so)
    H.check_outputs(tag, out, model, ref, sc, c_f32, fails, log, worst)
    if c["exact"] and not torch.equal(out["C"], ref["C"].float()):
        fails.append(f"{tag}: {(out['C'] != ref['C'].float()).sum().item()} elements of an exact f32 product differ")
    if drop:
        d = ~keep
        if kind == H.BIAS_DROP_RES and "ln" not in e and not torch.equal(out["C"][d], e["residual"][d]):
            fails.append(f"{tag}: a dropped element is not exactly the residual")
        if kind == H.BIAS_DROP_QGELU and ((out["C"][d] != 0).any() or ("aux" in out and (out["aux"][d] != 0).any())):
            fails.append(f"{tag}: a dropped element of C / aux is not exactly 0")
    if rows == (1, 0):                                      # mmu_gemm_rows(1, 0) is mmu_gemm, bit for bit
        first = {n: g.alloc.clone() for n, g in outs.items()}
        for g in outs.values():
            g.refill()
        launch(False)
        for n, g in outs.items():
            if not torch.equal(g._bits(g.alloc), g._bits(first[n])):
                fails.append(f"{tag} {n}: mmu_gemm_rows(1, 0) differs from mmu_gemm")


@pytest.mark.parametrize("group", list(H.GROUPS))
def test_gemm_edges(dev, monkeypatch, group):
    k = K()
    fails, log, worst = [], [], Worst()
    unreachable = dict(H.UNREACHABLE)
    for i, c in enumerate(H.GROUPS[group]()):
        if c["name"] in unreachable:
            continue
        run_case(k, dev, monkeypatch, c, 100 * len(group) + i, fails, log, worst)
    print("\n".join(log))
    worst.report(f"gemm {group}")
    assert not fails, "\n".join(fails[:40])


def test_keep_bits_agree_with_the_epilogue(dev):
    """gemm_harness.keep_bits (the restatement the sweep uses) against guarded.probe_keep (the bits read
    from the code under test), batched and at both dropout rates"""
    k = K()
    for (M, N, p, batch) in ((65, 128, 0.1, 1), (130, 256, 0.5, 2), (257, 256, 0.1, 1)):
        got = probe_keep(k, dev, M, N, p, SEED, batch=batch)
        want = H.keep_bits(SEED, M, N, batch, p).view(batch * M, N).to(dev)
        assert torch.equal(got, want), (M, N, p, batch)


def test_gemm_shared_b_interleaved_c(dev):
    """sB = 0 (one weight for every batch item) with the items' C rows interleaved in one matrix
    (sC = N, ldc = batch * N + pad), as the projection of src/model.py launches it"""
    k = K()
    fails, worst = [], Worst()
    for (M, N, Kd, batch) in ((65, 128, 64, 3), (257, 256, 128, 2)):
        A, B = H.gemm_inputs("wide", M, N, Kd, batch, seed=M, device=dev)
        B = B[:1].expand(batch, N, Kd)
        e = H.epi_inputs(H.STORE, M, N, 1, seed=M, device=dev)
        e["bias"] = e["bias"].expand(batch, N)
        ref, sc = H.gemm_ref(A, B, H.STORE, e)
        model = H.gemm_model32(A, B, H.STORE, e)
        gA, lda, sA = place_rows(dev, bf16, batch, M, Kd, 8, 2, A)
        gB, ldb, _ = place_rows(dev, bf16, 1, N, Kd, 16, 0, B[:1])
        gb = place_vec(dev, e["bias"][:1], N)
        gC = Guarded(dev, bf16, NAN, M, batch * N, batch * N + 8, guard=GUARD_ROWS)
        k.gemm(gA.view, lda, True, gB.view, ldb, True, gC.view, batch * N + 8, M, N, Kd, batch=batch, sA=sA, sB=0, sC=N,
               epi=k.epilogue(k.EPI_STORE, bias=gb.view, bias_bstride=0))
        torch.cuda.synchronize()
        check_written({"C": gC}, fails, f"interleaved M{M}")
        out = {"C": gC.view.reshape(M, batch, N).transpose(0, 1)}
        if torch.isfinite(out["C"].float()).all():
            H.check_outputs(f"interleaved M{M}", out, model, ref, sc, False, fails, None, worst)
        assert gA.unchanged() and gB.unchanged() and gb.unchanged()
    worst.report("gemm interleaved")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------- the other kernels of gemm.hip
CS_ROWS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1025)
CS_N = (8, 24, 512, 520)


@pytest.mark.parametrize("det", [False, True])
def test_colsum_bf16_edges(dev, det):
    """mmu_colsum_bf16: ldx > N, with and without the partial table, accumulate on and off"""
    from src import _native as Nat
    k = K()
    fails, worst = [], Worst()
    with k.deterministic(det):
        for i, rows in enumerate(CS_ROWS):
            for j, N in enumerate(CS_N):
                g = torch.Generator(device=dev).manual_seed(rows * 1000 + N)
                X = (torch.randn(rows, N, generator=g, device=dev)
                     * torch.exp2(torch.randint(-4, 5, (1, N), generator=g, device=dev).float())).to(bf16)
                gX, ldx, _ = place_rows(dev, bf16, 1, rows, N, H.PADS[(i + j) % 3], 0, X[None])
                init = torch.randn(1, N, generator=g, device=dev) * 3
                for with_part in (False, True):
                    for acc in (False, True):
                        tag = f"colsum_bf16 rows{rows} N{N} part{with_part} acc{acc} det{det}"
                        gO = place_vec(dev, init, N)
                        gP, part = out_buf(dev, f32t, ((rows + 63) // 64) * N, guard=2 * N)
                        args = ("mmu_colsum_bf16", gX.view.data_ptr(), rows, N, ldx, part.data_ptr() if with_part else None,
                                gO.view.data_ptr(), int(acc), torch.cuda.current_stream().cuda_stream)
                        if det and not with_part and rows > 1024:
                            with pytest.raises(Nat.NativeError):
                                Nat.call(*args)
                            continue
                        Nat.call(*args)
                        torch.cuda.synchronize()
                        check_written({"out": gO}, fails, tag)
                        if not gP.guards_intact():
                            fails.append(f"{tag}: wrote outside the partial table")
                        if not gX.unchanged():
                            fails.append(f"{tag}: X changed")
                        base = init[0] if acc else torch.zeros_like(init[0])
                        ref = base.double() + X.double().sum(0)
                        scale = base.double().abs() + X.double().abs().sum(0)
                        model = base + X.float().sum(0)
                        worst.f32("colsum_bf16", *check_f32(tag, gO.view, model, ref, scale, fails))
    worst.report(f"colsum_bf16 det={det}")
    assert not fails, "\n".join(fails[:40])


FOLD_PARTS = (1, 15, 16, 17, 63, 64, 65)
FOLD_N = (4, 6, 256, 260)


@pytest.mark.parametrize("det", [False, True])
def test_colsum_reduce_edges(dev, det):
    """mmu_colsum_reduce and _multi (1-4 jobs of different `parts`): vector and scalar folds"""
    k = K()
    fails, worst = [], Worst()

    def job(parts, N, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        part = torch.randn(parts, N, generator=g) * torch.exp2(torch.randint(-4, 5, (1, N), generator=g).float())
        init = torch.randn(1, N, generator=g) * 3
        return guarded_input(dev, part), place_vec(dev, init.to(dev), N), init[0].to(dev)

    def check(tag, part, gO, init, acc):
        check_written({"out": gO}, fails, tag)
        base = init if acc else torch.zeros_like(init)
        ref = base.double() + part.double().sum(0)
        scale = base.double().abs() + part.double().abs().sum(0)
        worst.f32("colsum_reduce", *check_f32(tag, gO.view, base + part.sum(0), ref, scale, fails))
    with k.deterministic(det):
        for N in FOLD_N:
            for acc in (False, True):
                for parts in FOLD_PARTS:
                    part, gO, init = job(parts, N, parts * 7 + N)
                    k.colsum_reduce(part, gO.view, accumulate=acc)
                    torch.cuda.synchronize()
                    check(f"colsum_reduce parts{parts} N{N} acc{acc} det{det}", part, gO, init, acc)
                for n_jobs in (1, 2, 3, 4):
                    js = [job(FOLD_PARTS[(n_jobs + 2 * z) % 7], N, 31 * z + N) for z in range(n_jobs)]
                    k.colsum_reduce_multi([(pt, gO.view) for pt, gO, _ in js], accumulate=acc)
                    torch.cuda.synchronize()
                    for z, (pt, gO, init) in enumerate(js):
                        check(f"colsum_reduce_multi {n_jobs} jobs, job {z} N{N} acc{acc} det{det}", pt, gO, init, acc)
    worst.report(f"colsum_reduce det={det}")
    assert not fails, "\n".join(fails[:40])


TR_DIMS = (1, 3, 4, 7, 8, 9, 63, 64, 65, 130)


def test_transpose_batched_edges(dev):
    """mmu_transpose_bf16_batched, bit-exact: jobs of different shapes in one launch, dense (pitch 0)
    and padded pitches, guarded sources and destinations"""
    k = K()
    fails = []
    for padded in (False, True):
        for shift in range(0, len(TR_DIMS), 2):
            shapes = [(r, TR_DIMS[(i + shift) % len(TR_DIMS)]) for i, r in enumerate(TR_DIMS)]
            srcs, dsts, rows_tab = [], [], []
            for i, (r, c) in enumerate(shapes):
                X = torch.randn(r, c, generator=torch.Generator().manual_seed(r * 131 + c)).to(bf16)
                gs, sld, _ = place_rows(dev, bf16, 1, r, c, (8 + 3 * (i % 2)) if padded else 0, 0, X[None])
                gd, dld, _ = place_rows(dev, bf16, 1, c, r, (16 - 3 * (i % 2)) if padded else 0, 0, guard=8)
                srcs.append((gs, X.to(dev)))
                dsts.append(gd)
                rows_tab.append([gs.view.data_ptr(), gd.view.data_ptr(), r, c, sld if padded else 0, dld if padded else 0])
            jobs = torch.tensor(rows_tab, dtype=torch.int64).to(dev)
            k.transpose_bf16_batched(jobs, len(shapes), max(r for r, _ in shapes), max(c for _, c in shapes), jobs)
            torch.cuda.synchronize()
            for (gs, X), gd, (r, c) in zip(srcs, dsts, shapes):
                tag = f"transpose {r}x{c} padded={padded}"
                check_written({"dst": gd}, fails, tag)
                if not gs.unchanged():
                    fails.append(f"{tag}: source changed")
                if not torch.equal(gd.view, X.t()):
                    fails.append(f"{tag}: not the transpose")
    assert not fails, "\n".join(fails[:40])


# ------------------------------------------------------------------------------- the C side's refusals
def test_gemm_refuses_misaligned_arguments(dev):
    """mmu_gemm refuses what its 16-B vector accesses do not allow.  Every refused call uses buffers
    large and aligned enough that it would stay inside them if it were wrongly accepted."""
    from src._native import NativeError
    k = K()
    M, N, Kd, batch = 130, 128, 64, 2
    big = lambda dt=bf16: torch.zeros(4 * batch * (M + 8) * (N + 64), dtype=dt, device=dev)  # noqa: E731
    A, B, C, C32, R, R32, X = big(), big(), big(), big(f32t), big(), big(f32t), big()
    vec = lambda: torch.zeros(8 * N, device=dev)  # noqa: E731
    bias, cs, lw, lb, mean, rstd = vec(), vec(), vec(), vec(), torch.zeros(batch * M + 8, device=dev), \
        torch.ones(batch * M + 8, device=dev)

    def call(A=A, lda=Kd, B=B, ldb=Kd, bk=True, C=C, ldc=N, sA=M * Kd, sB=N * Kd, sC=M * N, batch=batch,
             kind=k.EPI_STORE, **kw):
        k.gemm(A, lda, True, B, ldb, bk, C, ldc, M, N, Kd, batch=batch, sA=sA, sB=sB, sC=sC, epi=k.epilogue(kind, **kw))
    res = dict(kind=k.EPI_ADD_RES, residual=R, ldr=N, res_bstride=M * N)
    res32 = dict(kind=k.EPI_BIAS_DROP_RES, C=C32, residual=R32, ldr=N, res_bstride=M * N)
    gelu = dict(kind=k.EPI_BIAS_GELU, aux=X, ldx=N, aux_bstride=M * N)
    ln = dict(res32, res_ln=(mean, rstd, lw, lb), res_ln_bstride=N)
    stats = dict(kind=k.EPI_STORE_STATS, batch=1, colsum=torch.zeros(16 * N, device=dev))
    bn_x = lambda off: as_map(torch.zeros(M * N + 8, dtype=bf16, device=dev)[off:off + M * N].view(M, N))  # noqa: E731
    bn_mean = lambda off: torch.zeros(N + 4, device=dev)[off:off + N]  # noqa: E731
    bnb = dict(kind=k.EPI_STORE_BNB, batch=1, bk=False, ldb=N, colsum=torch.zeros(16 * N, device=dev),
               bn=(bn_x(0), None, bn_mean(0)))
    # the baselines: acceptable arguments pass
    for base in (dict(), dict(bias=bias, bias_bstride=N), res, res32, gelu, ln, stats, bnb, dict(C=C32, ldc=N + 4),
                 dict(ldc=N + 8), dict(kind=k.EPI_DGELU, aux=X, ldx=N + 8, aux_bstride=M * (N + 8), colsum=cs[1:])):
        call(**base)
    torch.cuda.synchronize()
    refused = [
        ("ldc", dict(ldc=N + 4)),                                      # bf16 C stored as bf16x8
        ("aligned", dict(A=A[1:])), ("aligned", dict(B=B[4:])), ("aligned", dict(C=C[2:])),
        ("aligned", dict(C=C32[2:], ldc=N)),
        ("batch strides", dict(sA=M * Kd + 4)), ("batch strides", dict(sB=N * Kd + 1)),
        ("batch strides", dict(sC=M * N + 4)), ("batch strides", dict(C=C32, sC=M * N + 2)),
        ("residual", dict(res, ldr=N + 4)), ("residual", dict(res, residual=R[4:])),
        ("residual", dict(res, res_bstride=M * N + 4)),
        ("16-B", dict(res32, ldr=N + 2)), ("residual", dict(res32, residual=R32[1:])),
        ("residual", dict(res32, res_bstride=M * N + 2)),
        ("aux", dict(gelu, ldx=N + 4)), ("aux", dict(gelu, aux=X[1:])), ("aux", dict(gelu, aux_bstride=M * N + 4)),
        ("aux", dict(kind=k.EPI_DGELU, aux=X, ldx=N + 12, aux_bstride=M * (N + 12))),
        ("bias", dict(bias=bias[1:], bias_bstride=N)), ("bias", dict(bias=bias, bias_bstride=N + 2)),
        ("res_ln", dict(ln, res_ln=(mean, rstd, lw[2:], lb))), ("res_ln", dict(ln, res_ln=(mean, rstd, lw, lb[1:]))),
        ("res_ln", dict(ln, res_ln_bstride=N + 1)),
        ("table", dict(stats, colsum=stats["colsum"][2:])),
        ("table", dict(bnb, colsum=bnb["colsum"][1:])),
        ("bn_x", dict(bnb, bn=(bn_x(4), None, bn_mean(0)))), ("bn_x", dict(bnb, bn=(bn_x(0), None, bn_mean(1)))),
    ]
    for msg, kw in refused:
        with pytest.raises(NativeError, match=msg):
            call(**kw)
    # batch 1: the batch strides are not used, whatever they are
    call(batch=1, sA=3, sB=5, sC=7)
    torch.cuda.synchronize()
