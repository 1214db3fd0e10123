"""The sequence-attention test harness (seqattn_harness.py) checked on the CPU: the bf16 rounding
model stays inside the derived cap at every case of the GPU sweep (test_seqattn_edges_gpu.py), the
float64 reference's gradient is right, and the bars flag three injected defects of the kind the
sweep exists to catch.  Without these the sweep's bars could be vacuous."""
import pytest
import torch

import seqattn_harness as H
from test_seqattn_edges_gpu import CASES, case_id, case_seed

# what the reference side alone (model32 against ref64) may use: O and dV have two bf16 roundings on
# their path (P; the stored output), dQ and dK all three of the cap's (dS; delta through the rounded
# O; the stored output)
MODEL_CAP = {"O": 2 * 2.0 ** -9, "dV": 2 * 2.0 ** -9, "dQ": H.CAP, "dK": H.CAP}


def _case(S, N, heads, D, nonneg=False, seed=None):
    qkv, dO = H.make_inputs(S, N, heads, D, seed=case_seed(S, N, heads, D) if seed is None else seed, nonneg=nonneg)
    return qkv, dO, H.ref64(qkv, dO, S, N, heads, D), H.scales(qkv, dO, S, N, heads, D)


def _stats(got, good, ref, sc, shape):
    return H.evaluate((got[0], got[2]), (good[0], good[2]), (ref[0], ref[2]), sc, *shape)


@pytest.mark.parametrize("nonneg", [False, True], ids=["gauss", "nonneg"])
@pytest.mark.parametrize("S,N,heads,D", CASES, ids=[case_id(*c) for c in CASES])
def test_model32_within_cap(S, N, heads, D, nonneg):
    """the rounding model alone: nerr <= 2 * 2^-9 (O, dV) and <= the cap 3 * 2^-9 (dQ, dK) on every row, no
    zero-scale rows, its LSE2 * ln 2 within the LSE bar, and compared with itself it holds every bar"""
    qkv, dO, (O64, lse64, g64), sc = _case(S, N, heads, D, nonneg)
    Om, lse2m, gm = H.model32(qkv, dO, S, N, heads, D)
    parts = H.split_outputs(Om, gm, S, N, heads, D)
    refp = H.split_outputs(O64, g64, S, N, heads, D)
    for name in H.OUTPUTS:
        e, z = H.nerr(parts[name], refp[name], sc[name])
        print(f"[model32 {case_id(S, N, heads, D)} nonneg={nonneg}] {name}: max {e.max().item():.2e} "
              f"median {e.median().item():.2e}")
        assert e.max().item() <= MODEL_CAP[name], (name, e.max().item())
        assert z.numel() == 0, name
    assert H.lse_violations(lse2m * H.LN2, lse64, H.lse32(qkv, S, N, heads, D)) == []
    assert H.violations(H.evaluate((Om, gm), (Om, gm), (O64, g64), sc, S, N, heads, D), D) == []
    assert H.delta_violations((H.heads_view(dO.float(), S, N, heads, D) * H.heads_view(Om, S, N, heads, D))
                              .sum(-1).reshape(N * heads, S), Om, dO, S, N, heads, D) == []


def test_ref64_gradient_matches_finite_differences():
    S, N, heads, D = 5, 2, 1, 64
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(S * N, 3 * D, generator=g, dtype=torch.float64)
    dO = torch.randn(S * N, D, generator=g, dtype=torch.float64)
    _, _, grad = H.ref64(x, dO, S, N, heads, D)
    f = lambda y: (H.forward64(y, S, N, heads, D)[0] * dO).sum().item()
    h = 1e-6
    fd = torch.zeros_like(x)
    for i in range(x.numel()):
        d = torch.zeros_like(x).view(-1)
        d[i] = h
        d = d.view_as(x)
        fd.view(-1)[i] = (f(x + d) - f(x - d)) / (2 * h)
    torch.testing.assert_close(grad, fd, rtol=1e-6, atol=1e-8)
    # the softmax runs over the S samples of one token position: item n of sample s is row s*N + n
    _, lse, _ = H.forward64(x, S, N, heads, D)
    for n in range(N):
        rows = x[n::N]
        sc = rows[:, :D] @ rows[:, D:2 * D].t() / 8.0
        torch.testing.assert_close(lse[n], sc.exp().sum(-1).log())


@pytest.mark.parametrize("nonneg", [False, True], ids=["gauss", "nonneg"])
@pytest.mark.parametrize("S,D", [(65, 64), (129, 128), (193, 256), (257, 64)])
def test_harness_flags_dropped_key(S, D, nonneg):
    """injected defect (a): key S - 1, the one live key of the last tile at S = 64 k + 1, missing from
    the forward P V and from the backward products (what an off-by-one key predicate does)"""
    N, heads = 3, 2
    shape = (S, N, heads, D)
    qkv, dO, ref, sc = _case(*shape, nonneg=nonneg)
    good = H.model32(qkv, dO, *shape)
    bad = H.model32(qkv, dO, *shape, drop_key=S - 1)
    assert H.violations(_stats(good, good, ref, sc, shape), D) == []
    st = _stats(bad, good, ref, sc, shape)
    msgs = H.violations(st, D)
    print(msgs)
    for name in ("O", "dQ", "dV"):
        assert st[name]["max_k"] > 2 * H.CAP, (name, st[name])
        assert any(m.startswith(name + ":") for m in msgs)
    # dK: the dropped key's own rows are all zero.  dK cancels heavily (the dS of a query sum to 0),
    # so a zeroed row is as little as 5e-3 of its scale: under the cap, but each such row alone is
    # over the margin, 2 x the model's worst row of the whole case
    assert any(m.startswith("dK:") for m in msgs)
    kb, kr = (H.split_outputs(t[0], t[2], *shape)["dK"] for t in (bad, ref))
    assert (kb[:, :, S - 1] == 0).all()
    e, _ = H.nerr(kb[:, :, S - 1], kr[:, :, S - 1], sc["dK"][:, :, S - 1])
    assert e.min().item() > max(H.MAX_MARGIN * st["dK"]["max_m"], H.f32_noise(D)), (e.min().item(), st["dK"])


@pytest.mark.parametrize("S,D", [(257, 64), (80, 128), (193, 256)])
def test_harness_flags_dropped_tail_queries(S, D):
    """injected defect (b): the last (S-1) % 16 + 1 queries missing from the dK / dV sums -- the
    kind of slip a partial-wave or partial-tile predicate makes"""
    N, heads = 3, 2
    shape = (S, N, heads, D)
    qkv, dO, ref, sc = _case(*shape)
    good = H.model32(qkv, dO, *shape)
    bad = H.model32(qkv, dO, *shape, dkdv_rows=S - ((S - 1) % 16 + 1))
    st = _stats(bad, good, ref, sc, shape)
    msgs = H.violations(st, D)
    print(msgs)
    for name in ("dK", "dV"):
        assert st[name]["max_k"] > H.CAP, (name, st[name])
        assert any(m.startswith(name + ":") for m in msgs)
    assert not any(m.startswith(("O:", "dQ:")) for m in msgs)


@pytest.mark.parametrize("nonneg", [False, True], ids=["gauss", "nonneg"])
@pytest.mark.parametrize("S,D", [(17, 64), (64, 128), (129, 256)])
def test_harness_flags_swapped_contraction_halves(S, D, nonneg):
    """injected defect (c): the forward multiplies P of key 32c + 4g + j with V of key
    32c + 16 + 4g + j and the reverse -- a tr_frag / acc_pair order mismatch"""
    N, heads = 3, 2
    shape = (S, N, heads, D)
    qkv, dO, ref, sc = _case(*shape, nonneg=nonneg)
    good = H.model32(qkv, dO, *shape)
    bad = H.model32(qkv, dO, *shape, swap_v_halves=True)
    st = _stats(bad, good, ref, sc, shape)
    msgs = H.violations(st, D)
    print(msgs)
    assert st["O"]["max_k"] > 2 * H.CAP, st["O"]
    assert any(m.startswith("O:") for m in msgs)


def test_sweep_reaches_every_branch_size():
    """the GPU sweep's case list: every length of the issue at all three head dimensions, the
    narrow and wide rows, and a delta grid ending on 1, 2, 3 and 4 live waves"""
    from test_seqattn_edges_gpu import LENGTHS
    assert LENGTHS == [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 127, 128, 129, 191, 192,
                       193, 256, 257]
    for S in LENGTHS:
        assert {(S, 3, 2, 64), (S, 3, 2, 128), (S, 2, 3, 256)} <= set(CASES)
    assert {(129, 1, 1, 64), (64, 1, 1, 64), (129, 2, 12, 64), (64, 2, 12, 64), (5, 3, 3, 256)} <= set(CASES)
    assert {S * N * heads % 4 for S, N, heads, _ in CASES} == {0, 1, 2, 3}
    assert len(set(CASES)) == len(CASES)


def test_noise_floor_follows_the_head_dimension():
    import attn_harness as A
    assert H.f32_noise(64) == A.F32_NOISE and H.f32_noise(256) == 4 * A.F32_NOISE
    st = {"O": dict(max_k=5e-6, med_k=5e-6, max_m=1e-9, med_m=0.0, finite=True, zero_ok=True)}
    assert len(H.violations(st, 64)) == 2   # 64 * 2^-24 = 3.8e-6: max and median margins fire
    assert H.violations(st, 128) == []      # 128 * 2^-24 = 7.6e-6
