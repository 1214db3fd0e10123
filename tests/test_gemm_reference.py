"""The GEMM sweep's own tools, on the CPU: the float32 model of the kernels (gemm_harness.gemm_model32)
passes every bar against the float64 reference for every input kind and epilogue kind; each of a
list of wrong results, built in torch, is rejected by the same bars (a control the bars could not
see would be a finding about the bars); the dropout restatement keeps its counter layout; and,
according to gemm_plan, every path of test_gemm_edges_gpu.py has cases that the host serves as meant.
"""
import collections

import pytest
import torch

import gemm_harness as H

M, N, K, BATCH = 65, 128, 128, 2
SEED = 4242


def _case(kind, inp, c_f32=False, p=0.0, **kw):
    A, B = H.gemm_inputs(inp, M, N, K, BATCH, seed=11 + kind)
    e = H.epi_inputs(kind, M, N, BATCH if kind < H.STORE_STATS else 1, seed=kind, c_f32=c_f32, ints=(inp == "int"),
                     **kw)
    if kind >= H.STORE_STATS:
        A, B = A[:1], B[:1]
    keep = H.keep_bits(SEED, M, N, A.shape[0], p) if kind in (H.BIAS_DROP_RES, H.BIAS_DROP_QGELU) else None
    return A, B, e, keep


def _run(kind, A, B, e, keep, p, c_f32, **kw):
    ref, sc = H.gemm_ref(A, B, kind, e, keep, p)
    model = H.gemm_model32(A, B, kind, e, keep, p, c_f32=c_f32, **kw)
    if kind >= H.STORE_STATS:
        ref["table"], sc["table"] = H.table_ref(model["C"][0], kind, e)
        model["table"] = H.table_model(model["C"][0], kind, e)
    return ref, sc, model


VARIANTS = [(H.STORE, False, {}), (H.STORE, True, dict(accumulate=True)), (H.BIAS_GELU, False, {}),
            (H.BIAS_DROP_RES, False, dict(p=0.1)), (H.BIAS_DROP_RES, True, dict(p=0.5)),
            (H.BIAS_DROP_RES, True, dict(p=0.1, res_ln=True)), (H.DGELU, False, dict(colsum=True)),
            (H.ADD_RES, False, dict(colsum=True)), (H.BIAS_DROP_QGELU, False, dict(p=0.5)),
            (H.STORE_STATS, False, {}), (H.STORE_BNB, False, dict(bn_mask=True)),
            (H.ADD_RES_BNB, False, dict(bn_mask=True, res_mask=True))]


@pytest.mark.parametrize("inp", H.INPUT_KINDS)
def test_model_within_bars(inp):
    fails, log = [], []
    for kind, c_f32, kw in VARIANTS:
        kw = dict(kw)
        p = kw.pop("p", 0.0)
        A, B, e, keep = _case(kind, inp, c_f32, p, **kw)
        for kchunk in (None, 64):
            ref, sc, model = _run(kind, A, B, e, keep, p, c_f32, kchunk=kchunk)
            out = {k: v for k, v in model.items() if k != "C32"}
            H.check_outputs(f"{H.KIND_NAMES[kind]} {inp} kchunk={kchunk}", out, model, ref, sc, c_f32, fails, log)
        if inp == "int" and c_f32 and kind == H.STORE:
            assert torch.equal(model["C"].double(), ref["C"]), f"{H.KIND_NAMES[kind]}: int inputs not exact in f32"
    print("\n".join(log))
    assert not fails, "\n".join(fails)


def _rejected(tag, out, model, ref, sc, c_f32=False):
    fails = []
    H.check_outputs(tag, out, model, ref, sc, c_f32, fails)
    assert fails, f"negative control '{tag}' passes the bars"


@pytest.mark.parametrize("c_f32", [False, True])
def test_negative_controls_product_and_bias(c_f32):
    kind = H.STORE
    A, B, e, keep = _case(kind, "gauss", c_f32)
    ref, sc, good = _run(kind, A, B, e, None, 0.0, c_f32)
    bad = lambda **kw: {"C": H.gemm_model32(kw.get("A", A), B, kind, kw.get("e", e), c_f32=c_f32,  # noqa: E731
                                            extra=kw.get("extra"))["C"]}
    _rejected("bias shifted by one column", bad(e={**e, "bias": e["bias"].roll(1, -1)}), good, ref, sc, c_f32)
    b01 = e["bias"].clone()
    b01[1] = b01[0]
    _rejected("bias of batch item 0 used for item 1", bad(e={**e, "bias": b01}), good, ref, sc, c_f32)
    A8 = A.clone()
    A8[1, 37, K - 8:] = 0
    _rejected("last 8 of K dropped in one row", bad(A=A8), good, ref, sc, c_f32)
    _rejected("one 32-deep k-step added twice", bad(extra=32), good, ref, sc, c_f32)


def test_negative_controls_residual_and_aux():
    kind = H.ADD_RES
    A, B, e, _ = _case(kind, "gauss")
    ref, sc, good = _run(kind, A, B, e, None, 0.0, False)
    ldr = N + 8       # the residual lives in rows of pitch ldr; reading it with pitch N walks off the rows
    padded = torch.zeros(BATCH, M, ldr, dtype=H.bf16)
    padded[:, :, :N] = e["residual"]
    wrong = padded.view(BATCH, -1)[:, :M * N].reshape(BATCH, M, N)
    _rejected("residual read with ld = N where ldr > N",
              {"C": H.gemm_model32(A, B, kind, {**e, "residual": wrong})["C"]}, good, ref, sc)
    kind = H.DGELU
    A, B, e, _ = _case(kind, "gauss")
    ref, sc, good = _run(kind, A, B, e, None, 0.0, False)
    _rejected("aux row m + 1 used", {"C": H.gemm_model32(A, B, kind, {**e, "aux_in": e["aux_in"].roll(-1, 1)})["C"]},
              good, ref, sc)


@pytest.mark.parametrize("kind,c_f32", [(H.BIAS_DROP_RES, False), (H.BIAS_DROP_RES, True), (H.BIAS_DROP_QGELU, False)])
def test_negative_controls_dropout(kind, c_f32):
    p = 0.5
    A, B, e, keep = _case(kind, "gauss", c_f32, p)
    ref, sc, good = _run(kind, A, B, e, keep, p, c_f32)
    kept = keep.nonzero()[7]
    dropped = (~keep).nonzero()[5]
    for name, at in (("a kept element dropped", kept), ("a dropped element kept", dropped)):
        k2 = keep.clone()
        k2[tuple(at)] = ~k2[tuple(at)]
        m = H.gemm_model32(A, B, kind, e, k2, p, c_f32=c_f32)
        _rejected(name, {"C": m["C"]}, good, ref, sc, c_f32)
        if kind == H.BIAS_DROP_QGELU:
            _rejected(name + " (aux)", {"aux": m["aux"]}, good, ref, sc, c_f32)


def test_negative_control_dead_row_in_colsum():
    for kind in (H.DGELU, H.ADD_RES):
        A, B, e, _ = _case(kind, "gauss", colsum=True)
        ref, sc, good = _run(kind, A, B, e, None, 0.0, False)
        dead = good["C32"][:, 3]      # a NaN-free row that is not part of the sum (here: one counted twice)
        _rejected("column sums that include a dead row", {"colsum": good["colsum"] + dead}, good, ref, sc)


def test_negative_control_tanh_gelu_derivative():
    kind = H.BIAS_GELU
    A, B, e, _ = _case(kind, "wide")
    ref, sc, good = _run(kind, A, B, e, None, 0.0, False)
    z = H._acc32(A, B) + e["bias"][:, None, :]
    _rejected("tanh-form GELU' on the wide inputs", {"aux": H.bf16r(H._gelu_tanh_grad(z))}, good, ref, sc)


@pytest.mark.parametrize("kind", [H.STORE_STATS, H.STORE_BNB])
def test_negative_control_table_row_shift(kind):
    A, B, e, _ = _case(kind, "gauss", bn_mask=True)
    ref, sc, good = _run(kind, A, B, e, None, 0.0, False)
    assert good["table"].shape == ((M + 63) // 64, N, 2)
    # the table of the rows shifted by 64: block 1 (the partly filled one) where block 0 belongs
    _rejected("one table row shifted by 64 rows", {"table": good["table"].flip(0)}, good, ref, sc)


def test_keep_bits_counter_layout():
    """keep_bits is keep_np at counter (row_offset + (z M + m) row_step) N + n; (1, 0) is the dense stream"""
    import numpy as np
    p, Mk, Nk = 0.3, 5, 8
    dense = H.keep_bits(SEED, 40, Nk, 1, p)[0]
    step = H.keep_bits(SEED, Mk, Nk, 2, p, row_step=3, row_offset=2)
    for z in range(2):
        for m in range(Mk):
            assert torch.equal(step[z, m], dense[2 + (z * Mk + m) * 3])
    hi = H.keep_bits(SEED, 2, 768, 1, p, row_step=1, row_offset=(1 << 24) + 3)
    idx = (np.uint64((1 << 24) + 3) * np.uint64(768)) + np.arange(768, dtype=np.uint64)
    assert int(idx[0]) > 1 << 33 and torch.equal(hi[0, 0], torch.from_numpy(H.keep_np(SEED, idx, p)))
    assert 0.6 < dense.float().mean() < 0.8 and H.keep_bits(SEED, 4, 8, 1, 0.0).all()


def test_every_path_has_cases():
    cases = H.all_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names), "duplicate case names"
    unreachable = dict(H.UNREACHABLE)
    assert len(unreachable) * 20 <= len(cases), "UNREACHABLE holds more than 5 % of the cases"
    assert set(unreachable) <= set(names)
    served = collections.Counter()
    for c in cases:
        pl = H.plan_of(c)
        wrong = H.meant(c, pl)
        if c["name"] in unreachable:
            assert wrong, f"{c['name']} is listed UNREACHABLE but the plan serves it"
            continue
        assert not wrong, f"{c['name']}: {wrong} ({pl})"
        served[c["path"]] += 1
        served["tiling " + pl["tiling"]] += 1
        served["cs " + pl["cs"]] += 1
        if pl["splitk"] > 1:
            served["split-K"] += 1
            if c["K"] % pl["kchunk"] % 64:
                served["split-K short last slice"] += 1
        if pl["tail_rows"]:
            served[f"tail {pl['tiling']}"] += 1
        if pl["group_m"] > 1 and pl["tiles_m"] % pl["group_m"]:
            served[f"ragged group of {pl['group_m']}"] += 1
        served[f"wgs mod 8 = {pl['wgs'] % 8}"] += 1
        if c["rows"] and (c["rows"][1] + 1) * c["N"] > 1 << 33:
            served["counter above 2^33"] += 1
    paths = {c["path"] for c in cases}
    want = paths | {"tiling small", "tiling big", "tiling wide", "cs rows", "cs atomics", "cs table", "split-K",
                    "split-K short last slice", "tail big", "tail wide", "ragged group of 2", "ragged group of 8",
                    "counter above 2^33"} | {f"wgs mod 8 = {r}" for r in range(8)}
    missing = [w for w in want if not served[w]]
    assert not missing, f"paths without a case: {missing}"
    # the lists of the sweep, in full
    assert {c["M"] for c in cases if c["path"] == "small-m"} == set(H.SMALL_M)
    assert {c["M"] for c in cases if c["path"] == "big-m"} == set(H.BIG_M)
    assert {c["M"] for c in cases if c["path"] == "wide"} == set(H.WIDE_M)
    assert {c["K"] for c in cases if c["path"] == "k-mnmajor"} == set(H.K_MNMAJOR)
    assert {c["rows"] for c in cases if c["path"] == "rows"} == set(H.ROW_STEPS)
    for tiling in ("small", "big"):
        seen = {(c["kind"], c["ak"], c["bk"]) for c in cases if c["path"] == f"epi-{tiling}"}
        assert seen == {(k, a, b) for k in range(6) for (a, b) in H.LAYOUTS}
