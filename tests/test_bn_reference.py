"""CPU checks of tests/bn_harness.py: the float32 rounding model alone meets every absolute bar on
every (C, rows, kind) of the BatchNorm sweep (so the bars of test_batchnorm_edges_gpu.py measure the
kernels, not the harness), the float64 reference equals F.batch_norm in float64 (forward, backward,
running statistics, eval), the stream residue's restatement round-trips, bn_geometry's case list
leaves nothing out and never reaches bn_grid's max_parts clamp.  No kernel runs here.

Every case runs the statistics once and two forward and two backward arms, rotating with the case,
so that every arm meets every kind and every channel count; the richest arm (skip + both residues +
ReLU + mask) runs on every case.
"""
import pytest
import torch
import torch.nn.functional as F

import bn_harness as B
import rowops_harness as R

# the model's own caps, as test_rowops_reference.py's: a bf16 output within the elementwise bar, its
# channel error at most the 2^-8 that bar implies; an f32 output within the f32 summation noise of
# its scale.  Not held where the variance cancels ("offset": B.ELEM_Y_KINDS says why), nor against
# float64 statistics, where the error of the model's own statistics is part of the figure: the
# bars of the GPU sweep are relative to the model there.
ROW_CAP = R.BF16_REL + R.F32_NOISE
CAP_FREE = {("Y row", "offset"), ("invstd", "offset")}
FWD = list(B.FWD_ARMS)
BWD = list(B.BWD_ARMS)


def _f32(name, out, ref, scale, bad, cap=True):
    ek, _, _ = R.f32_stats(out, out, ref, scale)
    if cap and not ek <= R.F32_NOISE:
        bad.append(f"{name}: model error {ek:.3e} of scale > {R.F32_NOISE:.3e}")
    return ek


def _bf16(name, out, ref, scale, bad, elem=True, row=True):
    el = R.bf16_elem(out, ref, scale)
    rn = R.rownorm(out.t(), ref.t(), scale.t())
    rn = rn.max().item() if rn.numel() else 0.0
    if elem and not el <= 1.0:
        bad.append(f"{name}: model elementwise error {el:.3f} x the bar")
    if row and not rn <= ROW_CAP:
        bad.append(f"{name}: model channel error {rn:.3e} > {ROW_CAP:.3e}")
    return el, rn


def model_case(C, rows, kind, idx, bad, fig=None):
    """the model against ref64 on one case; messages into `bad`, worst figures into `fig`"""
    d = B.bn_inputs(rows, C, kind, seed=C + rows)
    X, w, b = d["X"], d["w"], d["b"]
    tag = f"C={C} rows={rows} {kind}"
    sums = B.bn_stats_model(X) + (rows,)
    arms = {"stream", FWD[idx % len(FWD)], FWD[(idx + 4) % len(FWD)]}

    def note(k, v):
        if fig is not None:
            fig[k] = max(fig.get(k, 0.0), v)

    fm = None
    for arm in sorted(arms):
        training, relu, _, skip, sres, yres = B.FWD_ARMS[arm]
        mom, nbt = ((0.1, 1) if idx % 2 else (-1.0, 3))
        kw = dict(training=training, rmean=d["rm0"], rvar=d["rv0"], momentum=mom, nbt=nbt, relu=relu,
                  skip=(d["skip_s"] if sres else d["skip"]) if skip else None, skip_res=d["skip_res"] if sres else None)
        ref, sc = B.bn_fwd_ref(X, w, b, **kw)
        m = B.bn_fwd_model(X, w, b, sums=sums if training else None, **kw)
        el, rn = _bf16(f"{tag} {arm} Y", m["Y"], ref["Y"], sc["Y"], bad, elem=B.elem_bar("Y", kind),
                       row=("Y row", kind) not in CAP_FREE)
        note(f"Y elem {kind}", el)
        note(f"Y row {kind}", rn)
        if training:
            fm = m
            for k in ("mean", "invstd", "rmean", "rvar"):
                note(f"{k} {kind}", _f32(f"{tag} {arm} {k}", m[k], ref[k], sc[k], bad, cap=(k, kind) not in CAP_FREE))
        if yres:
            hi, res = B.res_encode(m["V"])
            assert torch.equal(hi.float(), m["Y"])
            se = B.stream_error(hi, res, ref["Y"])
            note(f"stream {kind}", se)
            if not se <= B.RES_BAR:
                bad.append(f"{tag} {arm}: decoded stream {se:.3e} of max |ref| > 2^-13")
    fr, _ = B.bn_fwd_ref(X, w, b)
    relu_mask = fm["Y"] > 0
    for arm in (BWD[idx % len(BWD)], BWD[(idx + 3) % len(BWD)]):
        relu, _, _ = B.BWD_ARMS[arm]
        mask = relu_mask if relu else None
        # the model's own statistics on both sides (the backward alone), then float64 statistics
        for which, mean, invstd in (("own", fm["mean"], fm["invstd"]), ("f64", fr["mean"], fr["invstd"])):
            ref, sc = B.bn_bwd_ref(d["dY"], mask, X, w, mean, invstd, d["dw0"], d["db0"])
            m = B.bn_bwd_model(d["dY"], mask, X, w, fm["mean"], fm["invstd"], d["dw0"], d["db0"])
            el, rn = _bf16(f"{tag} {arm} {which} dX", m["dX"], ref["dX"], sc["dX"], bad,
                           elem=B.elem_bar("dX", kind, which))
            note(f"dX elem {which} {kind}", el)
            note(f"dX row {which} {kind}", rn)
            for k in ("dw", "db"):
                note(f"{k} {which} {kind}", _f32(f"{tag} {arm} {which} {k}", m[k], ref[k], sc[k], bad,
                                                 cap=which == "own"))
            assert torch.equal(m["dSkip"].double(), ref["dSkip"])


@pytest.mark.parametrize("C", B.BN_C)
def test_bn_model_meets_the_bars(C):
    bad = []
    for idx, (rows, kind) in enumerate(B.bn_cases(C)):
        model_case(C, rows, kind, idx, bad)
    assert not bad, "\n".join(bad)


def test_bn_case_list_leaves_nothing_out():
    seen = set()
    for C in B.BN_C:
        g0 = B.bn_geometry(2, C)
        rpi, rpb = g0["rpi"], g0["rpb"]
        want = {2, 3, rpi - 1, rpi + 1, rpb, rpb + 1, 2 * rpb + rpi + 1, 33 * rpb + 1}
        want = {r for r in want if r >= 2 and (C, r) not in B.BN_UNREACHABLE}
        cases = B.bn_cases(C)
        assert len(cases) == len(set(cases))
        for kind in B.KINDS if C in B.BN_ALL_KINDS_C else ("unit", "tail"):
            assert want <= {r for r, k in cases if k == kind}, (C, kind)
        for kind in ("unit", "tail"):
            assert {r for c, r in B.BN_DENSE if c == C} <= {r for r, k in cases if k == kind}
        for r, _ in cases:
            g = B.bn_geometry(r, C)
            assert (g["rpi"], g["rpb"]) == (rpi, rpb) and not g["clamped"], (C, r)
            assert r * C <= 16 << 20
            seen.add((g["CH"], g["gy"], min(g["blocks"], 34), r % rpb < rpi and r % rpb > 0))
        blocks = {B.bn_geometry(r, C)["blocks"] for r, _ in cases}
        assert {1, 2, 3} <= blocks and ((C, 33 * rpb + 1) in B.BN_UNREACHABLE or 34 in blocks)
    assert {s[0] for s in seen} == {8, 32, 64, 256, 512} and {s[1] for s in seen} == {1, 3, 4, 65}
    assert any(s[3] for s in seen)  # a last block with fewer rows than one iteration
    # the unreachable case is unreachable: bn_grid has left the floor there, without the wrap
    for C, r in B.BN_UNREACHABLE:
        g = B.bn_geometry(r, C)
        assert g["rpb"] != B.bn_geometry(2, C)["rpb"] and g["blocks"] <= 32 and r * C > 16 << 20


def test_bn_grid_clamp_is_out_of_reach():
    """bn_grid's max_parts clamp needs rows x C >= 2^27 elements: without it the row blocks number
    at most rows C / 8192 (the floor), ~1024 CH / C (the 1024-block target) and rows CH / 65536 (the
    64 K cap), against max_parts = 2^20 / C.  Checked here at every channel count up to 16 M
    elements (the block count rises with the rows only along those three laws)."""
    for C in range(8, 2049, 8):
        top = (16 << 20) // C
        for rows in {top, top // 2, 8192 * 1024 // C, 8192 * 1024 // C + 1, 65536 * 1024 // C, 1024, 4096} | \
                set(range(2, top, max(1, top // 64))):
            if 2 <= rows <= top:
                assert not B.bn_geometry(rows, C)["clamped"], (C, rows)


@pytest.mark.parametrize("rows,C", [(2, 8), (37, 24), (300, 64)])
def test_bn_reference_is_batch_norm(rows, C):
    d = B.bn_inputs(rows, C, "unit", seed=rows)
    e = B.eps32()
    for mom, nbt in ((0.1, 1), (-1.0, 3)):
        x = d["X"].double().t().reshape(1, C, rows, 1).requires_grad_(True)
        w, b = d["w"].double().requires_grad_(True), d["b"].double().requires_grad_(True)
        s = d["skip"].double().t().reshape(1, C, rows, 1)
        rm, rv = d["rm0"].double().clone(), d["rv0"].double().clone()
        y = torch.relu(F.batch_norm(x, rm, rv, w, b, True, B._momentum(mom, nbt, torch.float64).item(), e) + s)
        ref, _ = B.bn_fwd_ref(d["X"], d["w"], d["b"], rmean=d["rm0"], rvar=d["rv0"], momentum=mom, nbt=nbt, relu=True,
                              skip=d["skip"])
        tt = dict(rtol=1e-12, atol=1e-12)  # (the factor in f32, as the kernels take and form it)
        torch.testing.assert_close(ref["Y"], y.detach().view(C, rows).t(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ref["rmean"], rm, **tt)
        torch.testing.assert_close(ref["rvar"], rv, **tt)
        dY = d["dY"].double().t().reshape(1, C, rows, 1)
        gx, gw, gb = torch.autograd.grad(y, [x, w, b], dY)
        bref, _ = B.bn_bwd_ref(d["dY"], ref["Y"] > 0, d["X"], d["w"], ref["mean"], ref["invstd"], d["dw0"], d["db0"])
        torch.testing.assert_close(bref["dX"], gx.view(C, rows).t(), rtol=1e-9, atol=1e-12)
        torch.testing.assert_close(bref["dw"] - d["dw0"].double(), gw, rtol=1e-9, atol=1e-12)
        torch.testing.assert_close(bref["db"] - d["db0"].double(), gb, rtol=1e-9, atol=1e-12)
        torch.testing.assert_close(bref["dSkip"], (dY * (y > 0)).view(C, rows).t(), rtol=0, atol=0)
    ev, _ = B.bn_fwd_ref(d["X"], d["w"], d["b"], training=False, rmean=d["rm0"], rvar=d["rv0"])
    y = F.batch_norm(d["X"].double(), d["rm0"].double(), d["rv0"].double(), d["w"].double(), d["b"].double(), False,
                     0.1, e)
    torch.testing.assert_close(ev["Y"], y, rtol=1e-12, atol=1e-12)


def test_bn_residue_round_trips():
    g = torch.Generator().manual_seed(4)
    v = torch.randn(4096, generator=g) * torch.ldexp(torch.ones(4096), torch.randint(-20, 20, (4096,), generator=g,
                                                                                     dtype=torch.int32))
    v[:7] = torch.tensor([0.0, -0.0, 1.0, 1.00390625, -3.0e38, 1e-39, 255.5])  # zero, a tie, near overflow, denormal
    hi, res = B.res_encode(v)
    assert res.abs().max().item() <= 127 and res.dtype == torch.int8
    err = (B.res_decode(hi, res, torch.float64) - v.double()).abs()
    inside = (hi.float().abs() >= B.TINY) & (hi.float().abs() < B.HUGE)
    assert (~inside).sum().item() == 4 and (res[~inside] == 0).all()
    assert (err <= B.RES_ROUNDTRIP * v.double().abs())[inside].all()   # every element to 2^-15 of itself,
    assert err[inside].max().item() <= B.RES_ROUNDTRIP * v[inside].abs().max().item()  # so the tensor to 2^-15 of its maximum
    assert (err[:2] == 0).all() and (res[:2] == 0).all()
    m = torch.rand(16, 24, generator=g) > 0.5
    assert torch.equal(B.mask_bools(B.mask_bits(m), 16, 24), m)
