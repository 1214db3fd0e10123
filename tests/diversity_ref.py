"""The definitions of include/mmu.h's ensemble diversity restated in numpy, for the diversity tests
(test_diversity_host.py, test_diversity_gpu.py, test_diversity_entry_gpu.py):
  p_k = mean_t softmax(z[s, k, t, :]);  member_arg = argmax_c p_k (ties to the lowest class);
  per pair (i, j), i < j, in itertools.combinations order:
    js = H[(p_i + p_j) / 2] - (H[p_i] + H[p_j]) / 2,  disagree = 1[member_arg_i != member_arg_j],
    tau = Kendall tau-b of the truncated vectors x_i, x_j over the C classes, from the four counts
    (conc, disc, tx, ty) over the n0 = C (C - 1) / 2 class pairs.
  Truncation: thr_k = the m-th largest p_k[c] (m = min(top, C), true class included), x_k[c] = p_k[c]
  where p_k[c] >= thr_k else 0, then x_k[y] = 0 if muting and 0 <= y < C; top = 0 keeps every class.

kendall_counts counts by groups of equal (x_i[c], x_j[c]) value pairs -- exact however many values tie,
and quick where most classes are truncated to (0, 0); kendall_counts_brute walks the class pairs, and
test_diversity_host.py holds the two (and scipy.stats.kendalltau) against each other.
"""
import itertools

import numpy as np


def xlogx(q):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(q > 0, q * np.log(q), q.dtype.type(0))


def member_probs(z, dt):
    """z f32 [S, K, T, C] -> p_k [S, K, C] at precision dt"""
    d = z.astype(dt)
    e = np.exp(d - d.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True, dtype=dt)).mean(2, dtype=dt)


def truncate(p, y, top, mute):
    """p [S, K, C] -> x [S, K, C]: see the module docstring"""
    S, K, C = p.shape
    x = p.copy()
    if top > 0:
        m = min(top, C)
        thr = np.partition(p, C - m, axis=-1)[..., C - m]
        x = np.where(p >= thr[..., None], p, p.dtype.type(0))
    if mute:
        for s in range(S):
            if 0 <= y[s] < C:
                x[s, :, y[s]] = 0
    return x


def kendall_counts_brute(a, b):
    """(conc, disc, tx, ty) of two vectors by walking every class pair"""
    n = len(a)
    iu = np.triu_indices(n, 1)
    sx = np.sign(a[:, None] - a[None, :])[iu]
    sy = np.sign(b[:, None] - b[None, :])[iu]
    return (int((sx * sy > 0).sum()), int((sx * sy < 0).sum()), int((sx == 0).sum()), int((sy == 0).sum()))


def kendall_counts(a, b):
    """the same four counts from the distinct (a[c], b[c]) value pairs and their multiplicities"""
    u, w = np.unique(a + 1j * b, return_counts=True)             # (a complex number is a pair of reals)
    w = w.astype(np.int64)
    # ordered class pairs (c, c') between groups g and h, c = c' included: each unordered pair twice, and
    # the len(a) pairs of a class with itself, which are tied in both
    ww = w[:, None] * w[None, :]
    sx = np.sign(u.real[:, None] - u.real[None, :])
    sy = np.sign(u.imag[:, None] - u.imag[None, :])
    ss = sx * sy
    return (int(ww[ss > 0].sum()) // 2, int(ww[ss < 0].sum()) // 2, (int(ww[sx == 0].sum()) - len(a)) // 2,
            (int(ww[sy == 0].sum()) - len(a)) // 2)


def tau_b(counts, C):
    """fp64 tau-b from (conc, disc, tx, ty): NaN when the denominator is 0"""
    conc, disc, tx, ty = (int(v) for v in counts)
    n0 = C * (C - 1) // 2
    den = (n0 - tx) * (n0 - ty)
    return (conc - disc) / np.sqrt(np.float64(den)) if den > 0 else np.nan


def diversity_ref(z, y, top, mute, dt, p=None, with_counts=True):
    """z f32 [S, K, T, C], y int [S] -> {"js" [S, P], "disagree" [S, P], "tau" [S, P] (fp64 from the
    counts), "counts" int64 [S, P, 4], "member_arg" int64 [S, K], "p" [S, K, C], "x" [S, K, C]} at precision
    dt.  p: the member_probs(z, dt) of an earlier call, to spare the softmax; with_counts=False leaves
    counts and tau unset (a caller that wants js alone)"""
    S, K, T, C = z.shape
    p = member_probs(z, dt) if p is None else p
    x = truncate(p, y, top, mute)
    arg = p.argmax(-1)
    H = lambda q: -xlogx(q).sum(-1, dtype=dt)                      # noqa: E731
    pairs = list(itertools.combinations(range(K), 2))
    js = np.empty((S, len(pairs)), dtype=dt)
    dis = np.empty((S, len(pairs)), dtype=np.float64)
    tau = np.empty((S, len(pairs)), dtype=np.float64)
    counts = np.empty((S, len(pairs), 4), dtype=np.int64)
    ent = H(p)
    for q, (i, j) in enumerate(pairs):
        js[:, q] = H((p[:, i] + p[:, j]) / dt(2)) - (ent[:, i] + ent[:, j]) / dt(2)
        dis[:, q] = arg[:, i] != arg[:, j]
        for s in range(S if with_counts else 0):
            counts[s, q] = kendall_counts(x[s, i], x[s, j])
            tau[s, q] = tau_b(counts[s, q], C)
    return {"js": js, "disagree": dis, "tau": tau, "counts": counts, "member_arg": arg.astype(np.int64), "p": p,
            "x": x}


def make_logits(C, K, T, S, scale, seed, top):
    """f32 [S, K, T, C] and labels [S].  Per-sample, per-member and per-pass Gaussian noise (1, 0.7,
    0.3); for every (s, k) a podium of npod = min(top + 1, C) distinct classes set to
    (largest logit of the member's T rows) + 0.5 (npod - r) for rank r, the same in every pass, so the
    kept probabilities and the first one dropped are 0.5 x scale apart in the logits of every pass;
    then x scale, cast to f32.  For every second sample member k's podium is a permutation of member
    0's podium classes, so that pairs have concordant and discordant kept classes (at large C two free
    podiums barely overlap).  Labels: the first member's winner for even samples, any class for odd."""
    g = np.random.default_rng(seed)
    z = (g.standard_normal((S, 1, 1, C)) + 0.7 * g.standard_normal((S, K, 1, C))
         + 0.3 * g.standard_normal((S, K, T, C)))
    npod = min(top + 1, C)
    win = np.empty(S, dtype=np.int64)
    for s in range(S):
        first = None
        for k in range(K):
            if first is None or s % 2 == 0:
                pod = g.choice(C, npod, replace=False)
            else:
                pod = g.permutation(first)
            first = pod if first is None else first
            base = z[s, k].max()
            for r, c in enumerate(pod):
                z[s, k, :, c] = base + 0.5 * (npod - r)
        win[s] = first[0]
    z = (z * scale).astype(np.float32)
    y = np.where(np.arange(S) % 2 == 0, win, g.integers(0, C, S)).astype(np.int64)
    return z, y


def make_ladder(C, K, T, S, seed, step=0.1):
    """f32 [S, K, T, C] whose every row is a permutation (one per (s, k)) of the ladder 0, step, 2 step, ...
    plus a per-pass constant the softmax ignores: all C probabilities of a member are a factor
    exp(step) apart -- the data of the untruncated (top = 0) cases at a C above the podium"""
    g = np.random.default_rng(seed)
    z = np.empty((S, K, T, C))
    for s in range(S):
        for k in range(K):
            z[s, k] = (step * g.permutation(C))[None, :] + g.integers(-2, 3, (T, 1))
    return z.astype(np.float32), g.integers(0, C, S).astype(np.int64)


def min_kept_gap(ref, top):
    """the smallest relative gap that an ordering the outputs depend on rests on: between neighbouring
    distinct non-zero values of any x_k, between a member's two largest probabilities (its argmax), and
    between the last probability kept and the first one dropped.  Exactly equal values (equal logits)
    are ties at every precision and are not gaps."""
    C = ref["p"].shape[-1]
    gap = np.inf

    def rel(hi, lo):
        return float((hi - lo) / hi) if hi > lo else np.inf

    for x in ref["x"].reshape(-1, C):
        nz = np.sort(x[x > 0])
        for lo, hi in zip(nz[:-1], nz[1:]):
            gap = min(gap, rel(hi, lo))
    for p in ref["p"].reshape(-1, C):
        srt = np.sort(p)[::-1]
        if C > 1:
            gap = min(gap, rel(srt[0], srt[1]))
        if 0 < top < C:
            gap = min(gap, rel(srt[top - 1], srt[top]))
    return gap
