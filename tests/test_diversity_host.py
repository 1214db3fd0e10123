"""Ensemble diversity on the host (no GPU): the numpy reference of the GPU tests against
scipy.stats.kendalltau and against the reference notebook's pooled formulation, DiversityMeter's analysis
against one written from scratch, and the new eval_robustness.py flags.
"""
import argparse
import itertools
import json

import numpy as np
import pytest

from diversity_ref import (diversity_ref, kendall_counts, kendall_counts_brute, make_ladder, make_logits, tau_b,
                           truncate)

CASES = [(C, K, T) for C in (1, 2, 5, 6, 63, 64, 65, 101, 129) for K, T in ((2, 1), (3, 1), (2, 3))]


def test_grouped_counts_equal_the_walk_over_class_pairs():
    g = np.random.default_rng(0)
    for n in (1, 2, 3, 7, 64, 130):
        for levels in (1, 2, 3, 1000):           # few levels: many ties, and arbitrarily many in one group
            for _ in range(4):
                a, b = g.integers(0, levels, n) / 7.0, g.integers(0, levels, n) / 3.0
                assert kendall_counts(a, b) == kendall_counts_brute(a, b), (n, levels)
    a = np.zeros(50)
    assert kendall_counts(a, a) == (0, 0, 1225, 1225) and np.isnan(tau_b(kendall_counts(a, a), 50))
    assert kendall_counts(np.arange(4.0), -np.arange(4.0)) == (0, 6, 0, 0)


@pytest.mark.parametrize("mute", [True, False])
def test_tau_is_scipys_tau_b_per_sample(mute):
    stats = pytest.importorskip("scipy.stats")
    worst = 0.0
    for i, (C, K, T) in enumerate(CASES):
        for scale in (0, 1, 8):
            for top in (5, 0):
                z, y = make_logits(C, K, T, 1, scale, 100 + i, 5)
                r = diversity_ref(z, y, top, mute, np.float64)
                for q, (a, b) in enumerate(itertools.combinations(range(K), 2)):
                    want = stats.kendalltau(r["x"][0, a], r["x"][0, b]).statistic
                    got = r["tau"][0, q]
                    assert np.isnan(want) == np.isnan(got), (C, K, T, scale, top)
                    if not np.isnan(want):
                        worst = max(worst, abs(want - got))
    print(f"\nlargest |tau - scipy tau-b| {worst:.3e}")
    assert worst <= 1e-12


def trunk_pred_top(pred, test_cls, top, mute_true=False):
    """what the reference notebook computes (notebooks/analysis_round_1.py: the true class zeroed, the
    threshold taken from the unmuted row by a partition, smaller values zeroed), restated"""
    out = []
    for i in range(len(pred)):
        p = pred[i].copy()
        if mute_true:
            p[test_cls[i]] = 0
        value = np.partition(pred[i].flatten(), -top)[-top]
        out.append(np.where(p >= value, p, 0.0))
    return np.array(out)


def test_one_sample_is_the_notebooks_pooled_statistic():
    """the notebook pools all S x C values of two sub-networks into one Kendall tau; for S = 1 that is
    the per-sample figure, truncation quirk included (the threshold from the unmuted row)"""
    stats = pytest.importorskip("scipy.stats")
    for i, (C, K, T) in enumerate(c for c in CASES if c[0] >= 5):
        z, y = make_logits(C, K, T, 1, 1, 300 + i, 5)
        r = diversity_ref(z, y, 5, True, np.float64)
        muted = [trunk_pred_top(r["p"][:, k], y, 5, mute_true=True) for k in range(K)]
        for k in range(K):
            assert np.array_equal(muted[k], r["x"][:, k])
        pooled = [stats.kendalltau(a, b).statistic for a, b in itertools.combinations(muted, 2)]
        assert np.abs(np.array(pooled) - r["tau"][0]).max() <= 1e-12


def test_truncation_keeps_ties_and_takes_the_threshold_from_the_unmuted_row():
    p = np.array([[[0.4, 0.3, 0.1, 0.1, 0.1]]])
    assert truncate(p, np.array([0]), 3, False)[0, 0].tolist() == [0.4, 0.3, 0.1, 0.1, 0.1]     # 3 tied at the threshold
    assert truncate(p, np.array([0]), 2, True)[0, 0].tolist() == [0.0, 0.3, 0.0, 0.0, 0.0]      # not the top 2 of the rest
    assert truncate(p, np.array([7]), 2, True)[0, 0].tolist() == [0.4, 0.3, 0.0, 0.0, 0.0]      # label out of range
    assert truncate(p, np.array([1]), 0, True)[0, 0].tolist() == [0.4, 0.0, 0.1, 0.1, 0.1]      # top = 0 keeps all
    assert truncate(p, np.array([1]), 9, False)[0, 0].tolist() == [0.4, 0.3, 0.1, 0.1, 0.1]     # top > C


def test_ladder_data_is_separated():
    z, y = make_ladder(65, 3, 2, 2, 1)
    r = diversity_ref(z, y, 0, False, np.float64)
    s = np.sort(r["p"], axis=-1)
    assert np.allclose(s[..., 1:] / s[..., :-1], np.exp(0.1), rtol=1e-5) and (r["x"] > 0).all()


# ------------------------------------------------------------------------------- the meter
def analysis_from_scratch(js, dis, tau, arg, y):
    """the figures of DiversityMeter.result() written out again, pair by pair"""
    n, K = arg.shape
    out = []
    for q, (i, j) in enumerate(itertools.combinations(range(K), 2)):
        a, b = arg[:, i] == y, arg[:, j] == y
        n11, n10, n01, n00 = (int(v.sum()) for v in (a & b, a & ~b, ~a & b, ~a & ~b))
        t = tau[:, q][~np.isnan(tau[:, q])]
        qd = n11 * n00 + n01 * n10
        va, vb = a.astype(np.float64), b.astype(np.float64)
        phi = None if va.std() == 0 or vb.std() == 0 else float(np.corrcoef(va, vb)[0, 1])
        out.append(dict(js=float(np.mean(js[:, q])), disagree=float(np.mean(dis[:, q])),
                        tau=float(t.mean()) if t.size else None, tau_n=int(t.size), contingency=[n11, n10, n01, n00],
                        double_fault=n00 / n, q=(n11 * n00 - n01 * n10) / qd if qd else None, phi=phi))
    return out


def rows(K, n, seed, always_right=None):
    g = np.random.default_rng(seed)
    P = K * (K - 1) // 2
    y = g.integers(0, 4, n)
    arg = g.integers(0, 4, (n, K))
    if always_right is not None:
        arg[:, always_right] = y
    pair = np.stack([g.random((n, P)) * 0.6, (g.random((n, P)) < 0.4).astype(float), g.random((n, P)) * 2 - 1], axis=2)
    pair[g.random((n, P)) < 0.3, 2] = np.nan
    return pair, arg, y


@pytest.mark.parametrize("K,always_right", [(2, None), (2, 1), (5, None), (5, 0), (16, 3)])
def test_meter_against_a_from_scratch_analysis(K, always_right):
    from src.diversity import DiversityMeter
    from src.robustness import json_safe
    parts = [rows(K, n, 10 * K + i, always_right) for i, n in enumerate((7, 1, 12))]
    whole, a, b = DiversityMeter(5, True), DiversityMeter(5, True), DiversityMeter(5, True)
    for i, part in enumerate(parts):
        whole.update_rows(*part)
        (a if i < 2 else b).update_rows(*part)
    a.merge(b.state())
    a.merge(DiversityMeter(5, True).state())                       # an empty meter merges as nothing
    res = whole.result()
    assert a.result() == res
    json.dumps(json_safe(res), allow_nan=False)
    assert json_safe(res) == res                                   # undefined figures are None already
    pair, arg, y = (np.concatenate([p[i] for p in parts]) for i in range(3))
    want = analysis_from_scratch(pair[:, :, 0], pair[:, :, 1], pair[:, :, 2], arg, y)
    pairs = list(itertools.combinations(range(K), 2))
    assert res["n"] == 20 and res["K"] == K and res["pairs"] == [list(p) for p in pairs]
    assert (res["top"], res["mute_true"]) == (5, True)
    for q, (i, j) in enumerate(pairs):
        for name, v in want[q].items():
            got = res[name][q]
            if v is None or isinstance(v, (int, list)):
                assert got == v, (name, q)
            else:
                assert got is not None and abs(got - v) <= 1e-12, (name, q, got, v)
            if name in res["matrix"]:
                assert res["matrix"][name][i][j] == got and res["matrix"][name][j][i] == got
    for name, mat in res["matrix"].items():
        assert [mat[k][k] for k in range(K)] == [0.0 if name in ("js", "disagree") else None] * K
    assert np.allclose(res["member_acc"], (arg == y[:, None]).mean(0), atol=1e-15)
    for name in ("js", "disagree", "tau", "double_fault", "q", "phi"):
        vals = [w[name] for w in want if w[name] is not None]
        if vals:
            assert abs(res["mean"][name] - np.mean(vals)) <= 1e-12
        else:
            assert res["mean"][name] is None
    if always_right is not None:                                   # a member that is always right: Q and phi undefined
        for q, (i, j) in enumerate(pairs):
            if always_right in (i, j):
                assert res["q"][q] is None and res["phi"][q] is None and res["double_fault"][q] == 0.0
        assert res["member_acc"][always_right] == 1.0
    if K == 2 and always_right is not None:
        assert res["mean"]["q"] is None and res["mean"]["phi"] is None
    ps = whole.per_sample()
    assert np.array_equal(ps["tau"], pair[:, :, 2], equal_nan=True) and np.array_equal(ps["member_arg"], arg)
    assert np.array_equal(ps["y"], y) and set(ps) == {"js", "disagree", "tau", "member_arg", "y"}


def test_meter_from_the_reference_rows_and_its_refusals():
    from src.diversity import DiversityMeter
    z, y = make_logits(11, 3, 2, 7, 1, 5, 5)
    r = diversity_ref(z, y, 5, True, np.float64)
    m = DiversityMeter()
    assert (m.top, m.mute_true, m.columns) == (5, True, ("js", "disagree", "tau"))
    assert m.result() == {"n": 0, "K": None, "top": 5, "mute_true": True}
    m.update_rows(np.stack([r["js"], r["disagree"], r["tau"]], axis=2), r["member_arg"], y)
    res = m.result()
    assert res["n"] == 7 and np.allclose(res["js"], r["js"].mean(0)) and res["tau_n"] == [7, 7, 7]
    assert np.allclose(res["member_acc"], (r["member_arg"] == y[:, None]).mean(0))
    with pytest.raises(ValueError, match="holds 2 members, the meter 3"):
        m.update_rows(np.zeros((1, 1, 3)), np.zeros((1, 2)), np.zeros(1))
    with pytest.raises(ValueError, match="pair must be"):
        m.update_rows(np.zeros((1, 2, 3)), np.zeros((1, 3)), np.zeros(1))
    with pytest.raises(ValueError, match="y must be"):
        m.update_rows(np.zeros((1, 3, 3)), np.zeros((1, 3)), np.zeros(2))
    with pytest.raises(ValueError, match="K >= 2"):
        DiversityMeter().update_rows(np.zeros((1, 0, 3)), np.zeros((1, 1)), np.zeros(1))
    with pytest.raises(ValueError, match="merge"):
        m.merge(DiversityMeter(3, True).state())
    with pytest.raises(ValueError, match="merge"):
        m.merge(DiversityMeter(5, False).state())
    for top in (-1, 1025, 2.5, True):
        with pytest.raises(ValueError, match="top"):
            DiversityMeter(top)
    import torch
    with pytest.raises(ValueError, match="layout"):
        m.update(torch.zeros(3, 2, 7, 11), torch.zeros(7, dtype=torch.int64), layout="BKTC")
    with pytest.raises(ValueError, match="layout"):
        m.update(torch.zeros(3, 7, 11), torch.zeros(7, dtype=torch.int64))            # 3-D only as [S, K, C]
    with pytest.raises(ValueError, match="at least 2 members"):
        m.update(torch.zeros(1, 2, 7, 11), torch.zeros(7, dtype=torch.int64))


# ------------------------------------------------------------------------------- flags
def parse(argv):
    import eval_robustness as E
    p = argparse.ArgumentParser()
    E.get_args(p)
    return p.parse_args(["--save_path", "out"] + argv)


def test_flags_parse_and_default():
    a = parse([])
    assert (a.diversity, a.diversity_top, a.diversity_keep_true, a.diversity_from) == (False, 5, False, None)
    a = parse(["--mmbt", "--diversity", "--diversity_top", "3", "--diversity_keep_true"])
    assert (a.diversity, a.diversity_top, a.diversity_keep_true) == (True, 3, True)
    assert parse(["--diversity_from", "lo.npy", "y.npy"]).diversity_from == ["lo.npy", "y.npy"]
    with pytest.raises(SystemExit):
        parse(["--diversity_from", "lo.npy"])
    with pytest.raises(SystemExit):
        parse(["--diversity_top", "five"])


def test_diversity_with_one_member_is_refused_before_any_model(monkeypatch, tmp_path):
    import eval_mmbt_robustness as M
    import eval_robustness as E
    from src.diversity import check_diversity_flags

    def boom(*a, **k):
        raise AssertionError("the data was loaded / a model was built")
    monkeypatch.setattr(M, "load_data", boom)
    common = ["--mmbt", "--synthetic", "3", "--save_path", str(tmp_path), "--diversity"]
    with pytest.raises(ValueError, match="--diversity compares pairs of members: 1 member"):
        E.main(common)
    with pytest.raises(ValueError, match="--diversity compares pairs of members: 1 member"):
        E.main(common + ["--checkpoint_path", "one.pt"])
    with pytest.raises(ValueError, match="--diversity compares pairs of members: 1 member"):
        E.main(common + ["--checkpoint_paths", "one.pt"])
    with pytest.raises(ValueError, match="at most 16 members, got 17"):
        E.main(common + ["--checkpoint_paths"] + [f"{i}.pt" for i in range(17)])
    for top in ("-1", "1025"):
        with pytest.raises(ValueError, match="--diversity_top"):
            E.main(common + ["--checkpoint_paths", "a.pt", "b.pt", "--diversity_top", top])
    with pytest.raises(AssertionError, match="the data was loaded"):     # two members pass the check
        E.main(common + ["--checkpoint_paths", "a.pt", "b.pt"])
    check_diversity_flags(2, 0)
    check_diversity_flags(16, 1024)
