"""Ranking metrics without a GPU: the fp64 host functions of src/ranking.py on the brute-force rank table of
ranking_ref.py (what mmu_rank_table must equal exactly, tests/test_rank_table_gpu.py), against sklearn's
roc_auc_score, against uncertainty.auroc and against the definitions written out -- the sort for tie-free
scores, the enumeration of every tie order for S <= 7.

Bars: 1e-12 throughout.  An AUROC is an exact rational (gt + eq / 2) / (n1 n0) rounded once here and a
handful of times by the references; the risk-coverage area is a sum of at most S harmonic-number
differences of size <= ln S + 1, each good to a few ulp (S <= 1000: well under 1e-13)."""
import itertools

import numpy as np
import pytest
import torch
from sklearn.metrics import roc_auc_score

import ranking_ref as R
from src import kernels as K
from src import ranking
from src.uncertainty import auroc as host_auroc

BAR = 1e-12


def _scores(kind, S, rng):
    if kind == "distinct":
        return rng.permutation(S).astype(np.float32) * 0.37 - 5
    if kind == "gauss":
        return rng.standard_normal(S).astype(np.float32)
    if kind == "ties":
        return rng.integers(0, 4, S).astype(np.float32)
    if kind == "equal":
        return np.full(S, 0.25, dtype=np.float32)
    raise AssertionError(kind)


def test_the_column_names_follow_the_header_enums():
    import os
    import re
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmu.h")
    enum = {n: int(v) for n, v in re.findall(r"\bMMU_RANK_(\w+) = (\d+)", open(header).read())}
    assert [enum[c.upper()] for c in K.RANK_COLUMNS] == list(range(K.RANK_NRANK)) and enum["NRANK"] == K.RANK_NRANK
    assert [enum[c.upper()] for c in K.RANK_COUNT_COLUMNS] == list(range(K.RANK_NCOUNT))
    assert enum["NCOUNT"] == K.RANK_NCOUNT
    assert (enum["BLOCK_ROWS"], enum["TILE"], enum["MAX_J"]) == (K.RANK_BLOCK_ROWS, K.RANK_TILE, K.RANK_MAX_J)
    assert K.RANK_MAX_S == 1 << 20
    assert (R.LT0, R.EQ0, R.LT1, R.EQ1) == tuple(K.RANK_COLUMNS.index(c) for c in ("lt0", "eq0", "lt1", "eq1"))
    assert (R.N1, R.N0, R.GT, R.EQ, R.NAN) == tuple(K.RANK_COUNT_COLUMNS.index(c)
                                                   for c in ("n1", "n0", "gt", "eq", "nan"))


@pytest.mark.parametrize("kind", ["distinct", "gauss", "ties", "equal"])
@pytest.mark.parametrize("S", [2, 17, 1000])
def test_auroc_from_counts_against_sklearn_and_the_host_auroc(kind, S):
    rng = np.random.default_rng(S * 7 + len(kind))
    x = np.stack([_scores(kind, S, rng) for _ in range(3)], axis=1)
    pos = rng.random(S) < 0.3
    pos[0], pos[1] = True, False
    _, counts = R.rank_table_ref(x, pos)
    got = ranking.auroc_from_counts(counts)
    for j in range(3):
        worst = max(abs(got[j] - roc_auc_score(pos, x[:, j].astype(np.float64))),
                    abs(got[j] - host_auroc(x[:, j], pos)), abs(got[j] - R.auroc_ref(x[:, j], pos)))
        print(f"{kind} S={S} column {j}: |d auroc| = {worst:.3g}")
        assert worst <= BAR
    assert ranking.auroc_from_counts(counts[1]) == got[1]
    if kind == "equal":
        assert got == [0.5, 0.5, 0.5]


@pytest.mark.parametrize("all_positive", [False, True])
def test_auroc_is_none_with_one_group_empty(all_positive):
    x = np.arange(6, dtype=np.float32).reshape(6, 1)
    _, counts = R.rank_table_ref(x, np.full(6, all_positive))
    assert ranking.auroc_from_counts(counts) == [None]
    assert host_auroc(x[:, 0], np.full(6, all_positive)) is None


def test_auroc_refuses_a_nan_column():
    x = np.array([[0.0, 1.0], [np.nan, 2.0], [3.0, 0.5]], dtype=np.float32)
    _, counts = R.rank_table_ref(x, [1, 0, 0])
    assert counts[0, R.NAN] == 1 and counts[1, R.NAN] == 0
    with pytest.raises(ValueError, match="column 0 holds 1 NaN"):
        ranking.auroc_from_counts(counts)
    assert ranking.auroc_from_counts(counts[1]) == 0.5


@pytest.mark.parametrize("S", [1, 2, 5, 64, 1000])
def test_aurc_against_the_sort_definition_on_tie_free_scores(S):
    rng = np.random.default_rng(S)
    x = _scores("distinct", S, rng).reshape(S, 1)
    wrong = rng.random(S) < 0.35
    rank, _ = R.rank_table_ref(x, wrong)
    got = ranking.aurc_from_ranks(rank[0], wrong)
    want = R.aurc_sorted_ref(x[:, 0], wrong)
    print(f"S={S}: |d aurc| = {abs(got['aurc'] - want):.3g}")
    assert abs(got["aurc"] - want) <= BAR
    n_w = int(wrong.sum())
    assert abs(got["eaurc"] - (want - R.ideal_aurc_ref(S, n_w))) <= BAR
    assert abs(ranking.ideal_aurc(S, n_w) - R.ideal_aurc_ref(S, n_w)) <= BAR


def test_aurc_against_every_tie_order_up_to_seven_samples():
    rng = np.random.default_rng(11)
    worst, n = 0.0, 0
    for S in range(1, 8):
        cases = [rng.integers(0, 3, S) for _ in range(6)] + [np.zeros(S), np.arange(S), np.arange(S) // 2]
        for vals in cases:
            for wrong in ([False] * S, [True] * S, list(rng.random(S) < 0.5), list(rng.random(S) < 0.5)):
                x = np.asarray(vals, dtype=np.float32).reshape(S, 1)
                rank, _ = R.rank_table_ref(x, wrong)
                got = ranking.aurc_from_ranks(rank[0], wrong)["aurc"]
                worst, n = max(worst, abs(got - R.aurc_enumerated_ref(x[:, 0], wrong))), n + 1
    print(f"{n} cases: worst |d aurc| = {worst:.3g}")
    assert worst <= BAR


def test_eaurc_is_zero_for_a_perfect_score_and_positive_otherwise():
    rng = np.random.default_rng(3)
    S = 50
    wrong = rng.random(S) < 0.3
    perfect = (rng.random(S) + wrong * 2.0).astype(np.float32).reshape(S, 1)   # every wrong sample above every right
    rank, _ = R.rank_table_ref(perfect, wrong)
    assert abs(ranking.aurc_from_ranks(rank[0], wrong)["eaurc"]) <= BAR
    for other in (-perfect, np.zeros_like(perfect), rng.permutation(perfect)):
        rank, _ = R.rank_table_ref(other, wrong)
        assert ranking.aurc_from_ranks(rank[0], wrong)["eaurc"] > 1e-3
    # nobody wrong: the area and its excess are both 0
    rank, _ = R.rank_table_ref(perfect, np.zeros(S, bool))
    assert ranking.aurc_from_ranks(rank[0], np.zeros(S, bool)) == {"aurc": 0.0, "eaurc": 0.0}


def test_aurc_refuses_nan_ranks_and_bad_shapes():
    x = np.array([[0.0], [np.nan], [3.0]], dtype=np.float32)
    rank, _ = R.rank_table_ref(x, [1, 0, 0])
    with pytest.raises(ValueError, match="NaN scores"):
        ranking.aurc_from_ranks(rank[0], [1, 0, 0])
    with pytest.raises(ValueError, match="rank_column"):
        ranking.aurc_from_ranks(rank[0], [1, 0])
    with pytest.raises(ValueError, match="rank_column"):
        ranking.aurc_from_ranks(rank[0][:, :3], [1, 0, 0])


# ---------------------------------------------------------------- the meters, the launch replaced by the reference
def _fake_rank_table(calls):
    def fake(x, group, rank=None, counts=None):
        calls.append(tuple(x.shape))
        r, c = R.rank_table_ref(x.cpu().numpy(), group.cpu().numpy())
        return (torch.from_numpy(r) if rank is not None else None), torch.from_numpy(c)
    return fake


def _separated_logits(rng, S, V, Kp, C, positive_class):
    """logits whose fp64 positive-class probabilities are, per variant, relatively 1e-4 apart at least"""
    while True:
        z = rng.standard_normal((S, V, Kp, C)) * 2.0
        p = R.softmax64(z)[..., positive_class].mean(axis=2)
        srt = np.sort(p, axis=0)
        if ((srt[1:] - srt[:-1]) >= 1e-4 * srt[1:]).all():
            return z.astype(np.float32), p


def test_auc_table_state_and_merge_round_trip(monkeypatch):
    calls = []
    monkeypatch.setattr(K, "rank_table", _fake_rank_table(calls))
    rng = np.random.default_rng(5)
    n, S, C = 2, 41, 2
    V = 3 + 2 * n
    z, _ = _separated_logits(rng, S, V, 1, C, 1)
    z = torch.from_numpy(z[:, :, 0])
    y = torch.from_numpy(rng.integers(0, C, S))
    whole = ranking.AucTable(n)
    whole.update(z, y)
    a, b = ranking.AucTable(n), ranking.AucTable(n)
    a.update(z[:17], y[:17])
    b.update(z[17:].transpose(0, 1).contiguous(), y[17:], layout="VBC")
    st = b.state()
    assert set(st) == {"n_repeats", "positive_class", "scores", "pos"}
    assert isinstance(st["scores"], np.ndarray) and st["scores"].dtype == np.float32 and st["scores"].shape == (24, V)
    assert isinstance(st["pos"], np.ndarray) and st["pos"].shape == (24,)
    a.merge(st)
    a.merge(ranking.AucTable(n).state())                        # an empty shard adds nothing
    assert a.result() == whole.result() and calls == [(S, V)] * 2
    assert a.gather() is a                                      # one process: itself
    re = ranking.AucTable(n)
    re.merge(a.state())
    assert re.result() == whole.result()
    with pytest.raises(ValueError, match="merge"):
        ranking.AucTable(n + 1).merge(st)
    with pytest.raises(ValueError, match="merge"):
        ranking.AucTable(n, positive_class=0).merge(st)
    res = whole.result()
    assert set(res) == {"n", "n_pos", "auc"} and res["n"] == S and res["n_pos"] == int((y == 1).sum())
    assert set(res["auc"]) == set(ranking.VARIANT_KEYS)
    assert set(res["auc"]["image_control"]) == {"mean", "std", "values"} and len(res["auc"]["text_control"]["values"]) == n
    empty = ranking.AucTable(n).result()
    assert empty["n"] == 0 and empty["auc"]["full"] is None and empty["auc"]["text_control"]["mean"] is None
    # one class only: every AUC undefined
    only = ranking.AucTable(n)
    only.update(z, torch.ones(S, dtype=torch.int64))
    assert only.result()["auc"]["full"] is None and only.result()["auc"]["image_control"]["values"] == [None] * n
    logs = ranking.auc_logs(res, "val")
    assert list(logs) == [f"val_rel_auc_{k}" for k in ranking.VARIANT_KEYS] and all(np.isfinite(v) for v in logs.values())
    assert all(np.isnan(v) for v in ranking.auc_logs(only.result(), "val").values())


@pytest.mark.parametrize("Kp", [0, 3])
def test_ensemble_auc_against_sklearn_on_fp64_softmax_means(monkeypatch, Kp):
    calls = []
    monkeypatch.setattr(K, "rank_table", _fake_rank_table(calls))
    rng = np.random.default_rng(8 + Kp)
    n, S, C, F = 2, 60, 2, 3
    V = 3 + 2 * n
    while True:                                                  # the condition on the data, for the means too
        files = [_separated_logits(rng, S, V, max(Kp, 1), C, 1) for _ in range(F)]
        mean = np.mean([p for _, p in files], axis=0)
        srt = np.sort(mean, axis=0)
        if ((srt[1:] - srt[:-1]) >= 1e-4 * srt[1:]).all():
            break
    y = rng.integers(0, C, S)
    stacks = [z if Kp else z[:, :, 0] for z, _ in files]
    got = ranking.ensemble_auc(stacks, y, n, device="cpu")
    assert calls == [(S, F + V)]                                 # one launch
    assert (got["n"], got["n_pos"], got["n_files"]) == (S, int((y == 1).sum()), F)
    for f in range(F):
        assert abs(got["full"][f] - roc_auc_score(y == 1, files[f][1][:, 0])) <= BAR
    want = [roc_auc_score(y == 1, mean[:, v]) for v in range(V)]
    e = got["ensemble"]
    flat = [e["full"], e["image"], e["text"]] + e["image_control"]["values"] + e["text_control"]["values"]
    assert max(abs(a - b) for a, b in zip(flat, want)) <= BAR
    assert abs(e["image_control"]["mean"] - np.mean(want[3:3 + n])) <= BAR
    assert abs(e["text_control"]["std"] - np.std(want[3 + n:])) <= BAR
    with pytest.raises(ValueError, match="prediction stack"):
        ranking.ensemble_auc([stacks[0][:, :4]], y, n, device="cpu")
    with pytest.raises(ValueError, match="at least one"):
        ranking.ensemble_auc([], y, n, device="cpu")


def test_selective_is_one_launch_over_all_columns(monkeypatch):
    calls = []
    monkeypatch.setattr(K, "rank_table", _fake_rank_table(calls))
    rng = np.random.default_rng(2)
    S = 90
    wrong = rng.random(S) < 0.25
    scores = {"a": rng.standard_normal(S), "b": rng.integers(0, 3, S).astype(np.float64), "c": np.zeros(S)}
    got = ranking.selective(scores, wrong, "cpu")
    assert calls == [(S, 3)] and set(got) == {"a", "b", "c", "n", "error_rate"}
    assert got["n"] == S and got["error_rate"] == float(wrong.mean())
    for name, s in scores.items():
        s32 = s.astype(np.float32)
        assert set(got[name]) == {"auroc", "aurc", "eaurc"}
        assert abs(got[name]["auroc"] - host_auroc(s32, wrong)) <= BAR
        rank, _ = R.rank_table_ref(s32.reshape(S, 1), wrong)
        assert got[name]["aurc"] == ranking.aurc_from_ranks(rank[0], wrong)["aurc"]
    assert abs(got["a"]["aurc"] - R.aurc_sorted_ref(scores["a"].astype(np.float32), wrong)) <= BAR
    assert got["c"]["auroc"] == 0.5
    # all equal: the expected number of wrong samples among the first k is k n_w / S, so every term is the error rate
    assert abs(got["c"]["aurc"] - wrong.mean()) <= BAR
