"""CPU checks of tests/bertadam_harness.py: the table covers every alignment arm it claims, the
gradient roles clip as stated, the schedule crosses the knee, reaches t_total and clamps, and the
float32 rounding model meets the bars of test_bertadam_edges_gpu.py against the float64 reference
on every run, step and tensor: p, m and v within 4 f32 ulps of their scales (|p| + lr |u|, |m|,
|v|).  The GPU test's bar is max(8 x the model's largest error on the tensor, 4 ulps): with the
model inside 4 ulps it never asks more of the kernel than f32 arithmetic gives.  No kernel runs here.
"""
import pytest
import torch

import bertadam_harness as A
import rowops_harness as R
from oracle.bertadam_ref import schedule_factor


def test_table_covers_every_alignment_arm():
    L = A.layout()
    n = len(L["sizes"])
    assert sorted(L["sizes"]) == sorted([1, 3, 5, 255, 257, A.CH - 1, A.CH + 1, 2 * A.CH + 3, A.BIG_CH + 5, 7, 2])
    act = [t for t in range(n) if L["active"][t]]
    assert {L["offs"][t] % 4 for t in act} == {0, 1, 2, 3}
    arms = {(L["offs"][t] % 4 == 0, L["coffs"][t] % 4 == 0) for t in act if L["coffs"][t] >= 0}
    assert arms == {(True, True), (True, False), (False, True), (False, False)}
    assert any(L["coffs"][t] < 0 for t in act)
    assert {L["groups"][t] for t in act} == {0, 1}
    inactive = [t for t in range(n) if not L["active"][t]]
    assert len(inactive) == 2 and all(0 < t < n - 1 and L["active"][t - 1] and L["active"][t + 1] for t in inactive)
    assert any(L["coffs"][t] >= 0 for t in inactive) and any(L["coffs"][t] < 0 for t in inactive)
    # packed as ParamStore packs: no padding in either buffer, the copies in their own order
    assert L["offs"] == [sum(L["sizes"][:t]) for t in range(n)]
    c = 0
    for t in A.COPY_ORDER:
        assert L["coffs"][t] == c
        c += L["sizes"][t]
    assert c == L["ctotal"] and any(L["coffs"][t] != L["offs"][t] for t in A.COPY_ORDER)
    # the chunk table: every tensor covered once, the big tensor at the production chunk length
    tab = L["table"]
    chunks = tab[7 * n:].view(-1, 3).tolist()
    assert [tuple(ck) for ck in chunks] == L["chunks"]
    for t in range(n):
        off, numel, grp, coff, active, first, nch = tab[7 * t:7 * t + 7].tolist()
        mine = chunks[first:first + nch]
        assert all(ck[0] == t for ck in mine) and sum(ck[2] for ck in mine) == numel == L["sizes"][t]
        assert [ck[1] for ck in mine] == [sum(x[2] for x in mine[:i]) for i in range(nch)]
    big = L["sizes"].index(A.BIG_CH + 5)
    assert [ck[2] for ck in chunks if ck[0] == big] == [A.BIG_CH, 5]
    assert max(ck[2] for ck in chunks if ck[0] != big) == A.CH
    # a vector body with a scalar tail, a chunk that is all tail, and heads of 1, 2 and 3 elements
    assert {(-L["offs"][t]) % 4 for t in act if L["sizes"][t] > 8} == {0, 1, 2, 3}


def test_gradient_roles():
    L = A.layout()
    for step in range(A.STEPS):
        g = A.grads(L, step)
        for t, (n, active, _, _, role) in enumerate(A.TENSORS):
            gt = g[L["offs"][t]:L["offs"][t] + n]
            if not active:
                assert torch.isnan(gt).all()
                continue
            norm = gt.double().norm().item()
            if role == "zero":
                assert (gt == 0).all()
            elif role == "under":
                assert 0.99 < norm < 1.0
            elif role == "between":
                assert norm > 1.0 and 0.5 * norm < 1.0
            elif role == "clip":
                assert 0.5 * norm > 1.0
            if L["offs"][t] % 4 and n >= 6:  # the norm lives in the scalar head and tail
                ends = torch.cat([gt[:3], gt[-3:]]).double().norm().item()
                assert ends > 0.9 * norm and gt[3:-3].abs().max() < 0.1 * gt[:3].abs().min()
        if step:
            assert not torch.equal(g.nan_to_num(), A.grads(L, step - 1).nan_to_num())  # fresh on every step


def test_schedule_crosses_the_knee_and_clamps():
    _, t_total, warmup, _, _ = A.RUNS[0]
    f = [schedule_factor(s, warmup, t_total) for s in range(A.STEPS)]
    assert f[0] == 0.0 and 0 < f[1] < f[2] and f[2] > f[3] > f[4] > 0 and f[5] == 0.0
    assert abs(f[2] - 1.0) < 1e-6 and A.STEPS - 1 == t_total  # the knee, and step t_total is reached
    assert schedule_factor(3, warmup, -1.0) == 1.0


@pytest.mark.parametrize("run", A.RUNS, ids=[r[0] for r in A.RUNS])
def test_model_meets_the_bars(run):
    L = A.layout()
    p, m, v, _ = A.initial(L)
    ref, mod = A.Track(L, p, m, v, torch.float64), A.Track(L, p, m, v, torch.float32)
    worst = 0.0
    for step in range(A.STEPS):
        g = A.grads(L, step, run[3])
        ref.load(*mod.flat((p, m, v)))  # every step from the model's own state: one step's errors
        ref.step(g, run)
        mod.step(g, run)
        for t in ref.act:
            for key, got, want in (("p", mod.p[t], ref.p[t]), ("m", mod.m[t], ref.m[t]), ("v", mod.v[t], ref.v[t])):
                s = ref.scale[t][key]
                err = (got.double() - want).abs()
                assert (err[s == 0] == 0).all(), (step, t, key)
                ulps = (err[s > 0] / R.f32_ulp(s[s > 0])).max().item() if (s > 0).any() else 0.0
                worst = max(worst, ulps)
                assert ulps <= R.F32_ULPS, f"step {step} tensor {t} {key}: the model is {ulps:.2f} ulps off"
        assert mod.steps == ref.steps == {t: step + 1 for t in ref.act}
    print(f"{run[0]}: the model's worst error {worst:.2f} f32 ulps of the scale")
