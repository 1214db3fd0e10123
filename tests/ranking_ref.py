"""Brute-force references for the ranking metrics (csrc/ranking.hip mmu_rank_table, src/ranking.py): the
rank table by O(S^2) numpy compares on the f32 values themselves, and fp64 AUROC and risk-coverage area
taken straight from their definitions.  Nothing here shares code with the package."""
import itertools

import numpy as np

LT0, EQ0, LT1, EQ1 = range(4)
N1, N0, GT, EQ, NAN = range(5)


def rank_table_ref(x, group):
    """x f32 [S, J] (any strides), group [S] (non-zero = group 1) -> rank int32 [J, S, 4], counts int64 [J, 5]"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    g = np.asarray(group).reshape(-1) != 0
    S, J = x.shape
    assert g.shape == (S,)
    rank = np.zeros((J, S, 4), dtype=np.int32)
    counts = np.zeros((J, 5), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(J):
            v = x[:, j]
            lt = v[None, :] < v[:, None]          # [i, i']: x[i'] < x[i]; IEEE: false with a NaN on either side
            eq = v[None, :] == v[:, None]
            rank[j, :, LT0] = np.count_nonzero(lt & ~g, axis=1)
            rank[j, :, EQ0] = np.count_nonzero(eq & ~g, axis=1)
            rank[j, :, LT1] = np.count_nonzero(lt & g, axis=1)
            rank[j, :, EQ1] = np.count_nonzero(eq & g, axis=1)
            nan = np.isnan(v)
            counts[j] = ((g & ~nan).sum(), (~g & ~nan).sum(), rank[j, g, LT0].astype(np.int64).sum(),
                         rank[j, g, EQ0].astype(np.int64).sum(), nan.sum())
    return rank, counts


def auroc_ref(score, positive):
    """P(positive scores higher) + P(tie) / 2 over all (positive, negative) pairs, fp64; None without both groups"""
    s = np.asarray(score, dtype=np.float64).reshape(-1)
    p = np.asarray(positive).reshape(-1).astype(bool)
    a, b = s[p], s[~p]
    if a.size == 0 or b.size == 0:
        return None
    gt = (a[:, None] > b[None, :]).sum()
    eq = (a[:, None] == b[None, :]).sum()
    return float((gt + 0.5 * eq) / (a.size * float(b.size)))


def aurc_of_order(wrong_in_order):
    """(1 / S) sum_{k = 1 .. S} (wrong among the first k) / k for one acceptance order"""
    w = np.asarray(wrong_in_order, dtype=np.float64)
    k = np.arange(1, w.size + 1, dtype=np.float64)
    return float((np.cumsum(w) / k).sum() / w.size)


def aurc_sorted_ref(score, wrong):
    """tie-free scores: the definition on the ascending sort"""
    s = np.asarray(score).reshape(-1)
    assert np.unique(s).size == s.size
    return aurc_of_order(np.asarray(wrong).reshape(-1)[np.argsort(s, kind="stable")])


def aurc_enumerated_ref(score, wrong):
    """the mean of the definition over every acceptance order that sorts the scores (all tie orders, each
    equally likely); S! permutations are walked, so S <= 7"""
    s = np.asarray(score).reshape(-1)
    w = np.asarray(wrong).reshape(-1)
    assert s.size <= 7
    vals = [aurc_of_order(w[list(perm)]) for perm in itertools.permutations(range(s.size))
            if all(s[perm[i]] <= s[perm[i + 1]] for i in range(s.size - 1))]
    return float(np.mean(vals))


def ideal_aurc_ref(S, n_wrong):
    return aurc_of_order([0] * (S - n_wrong) + [1] * n_wrong)


def softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)
