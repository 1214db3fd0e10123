"""Ranking metrics from the exact rank table (csrc/ranking.hip, kernels.rank_table).

The reference's AUC table and epoch-ensemble AUC (notebooks/hatefulmeme_robustness.py:22-41 AUC_table,
:234-247 ensemble_overtime; restated), the AUROC of an uncertainty score, and the area under its
risk-coverage curve.  All are functions of ranks: one launch counts, per score column and sample, how
many samples of each group score lower or the same (IEEE f32 compares), and everything here is fp64 on
the host from those integers -- a figure depends on the scores alone, not on summation order, launch
shape or determinism mode.  Ties count half in the AUROC (the trapezoid rule of sklearn's
roc_auc_score) and are averaged over uniformly random tie orders in the risk-coverage area.
"""
import os

import numpy as np
import torch

from . import kernels

VARIANT_KEYS = ("full", "image", "text", "image_control", "text_control")


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ---------------------------------------------------------------------------- figures from the integers
def auroc_from_counts(counts):
    """counts int [J, RANK_NCOUNT] (or one row [RANK_NCOUNT]) = (n1, n0, gt, eq, nan) per column ->
    [(gt + eq / 2) / (n1 n0)] per column in fp64 (a float for one row); None where a group is empty.
    Raises if a column holds a NaN score: its samples were ranked by nobody."""
    c = _np(counts).astype(np.int64)
    one = c.ndim == 1
    c = c.reshape(-1, kernels.RANK_NCOUNT)
    col = kernels.RANK_COUNT_COLUMNS.index
    bad = np.nonzero(c[:, col("nan")] > 0)[0]
    if bad.size:
        raise ValueError(f"auroc_from_counts: column {int(bad[0])} holds {int(c[bad[0], col('nan')])} NaN score(s)")
    out = []
    for n1, n0, gt, eq in c[:, :4].tolist():             # python ints: n1 n0 and 2 gt + eq are exact
        out.append(None if n1 * n0 == 0 else float((2 * gt + eq) / (2 * n1 * n0)))
    return out[0] if one else out


def _harmonic(S):
    """H[p] = sum_{k <= p} 1 / k for p = 0 .. S, and PH[p] = sum_{q < p} H[q] for p = 0 .. S + 1 (long double)"""
    H = np.zeros(S + 1, dtype=np.float64)
    H[1:] = np.cumsum(1.0 / np.arange(1, S + 1, dtype=np.float64))
    PH = np.zeros(S + 2, dtype=np.longdouble)
    PH[1:] = np.cumsum(H.astype(np.longdouble))
    return H, PH


def ideal_aurc(S, n_wrong):
    """the risk-coverage area of the best possible order, all wrong samples last:
    (1 / S) sum_{k = S - n_w + 1 .. S} (k - (S - n_w)) / k"""
    if n_wrong == 0:
        return 0.0
    k = np.arange(S - n_wrong + 1, S + 1, dtype=np.float64)
    return float(((k - (S - n_wrong)) / k).sum() / S)


def aurc_from_ranks(rank_column, wrong):
    """The area under the risk-coverage curve of one score column, the samples accepted in order of
    ascending score (the score is an uncertainty): (1 / S) sum_{k = 1 .. S} (wrong among the first k) / k,
    ties averaged over uniformly random tie orders.  rank_column int [S, RANK_NRANK] = (lt0, eq0, lt1,
    eq1) of kernels.rank_table, wrong bool [S].  With a_i = lt0 + lt1, e_i = eq0 + eq1 and
    H_p = sum_{k <= p} 1 / k:
        AURC = (1 / S) sum_{i wrong} [ H_S - (1 / e_i) sum_{p = a_i}^{a_i + e_i - 1} H_p ]
    (a wrong sample at 0-based position p is among the first k for every k > p, which adds H_S - H_p; under a
    uniformly random tie order its position is uniform over its tie group's e_i places).
    -> {"aurc", "eaurc"}, eaurc = AURC - ideal_aurc.  Raises on a NaN score (a sample with e_i = 0)."""
    r = _np(rank_column).astype(np.int64)
    w = _np(wrong).reshape(-1).astype(bool)
    if r.ndim != 2 or r.shape[1] != kernels.RANK_NRANK or r.shape[0] != w.size or w.size == 0:
        raise ValueError(f"aurc_from_ranks: rank_column [S, {kernels.RANK_NRANK}] and wrong [S], got {r.shape} and "
                         f"{w.shape}")
    S = w.size
    a, e = r[:, 0] + r[:, 2], r[:, 1] + r[:, 3]
    if (e <= 0).any():
        raise ValueError(f"aurc_from_ranks: {int((e <= 0).sum())} sample(s) tie with nobody, themselves included "
                         "(NaN scores)")
    if (a + e > S).any():
        raise ValueError("aurc_from_ranks: the counts exceed the number of samples")
    H, PH = _harmonic(S)
    a, e = a[w], e[w]
    mean_h = np.where(e == 1, H[a], ((PH[a + e] - PH[a]) / e).astype(np.float64))
    aurc = float((H[S] - mean_h).sum() / S)
    return {"aurc": aurc, "eaurc": aurc - ideal_aurc(S, int(w.sum()))}


# ---------------------------------------------------------------------------- selective prediction
def selective(scores, wrong, device):
    """What each uncertainty score is worth for selective prediction.  scores {name: [S] values}, rounded
    to f32 (the kernel ranks f32; the decomposition's columns are f32 already); wrong bool [S].  One
    rank_table launch over all columns -> {name: {"auroc", "aurc", "eaurc"}, "n": S, "error_rate"}: auroc
    of the score ranking the wrong samples above the right ones (None when all are right or all wrong),
    aurc / eaurc of accepting by ascending score."""
    names = list(scores)
    w = _np(wrong).reshape(-1).astype(bool)
    if not names or w.size == 0:
        raise ValueError("selective: needs at least one score column and one sample")
    cols = [np.asarray(_np(scores[n]), dtype=np.float32).reshape(-1) for n in names]
    for n, c in zip(names, cols):
        if c.size != w.size:
            raise ValueError(f"selective: score {n!r} has {c.size} values for {w.size} samples")
    x = torch.from_numpy(np.stack(cols)).to(device)                      # [J, S], read in place as [S, J]
    group = torch.from_numpy(w.astype(np.uint8)).to(device)
    rank, counts = kernels.rank_table(x.t(), group, rank=True)
    rank, auc = _np(rank), auroc_from_counts(counts)
    out = {}
    for j, n in enumerate(names):
        out[n] = {"auroc": auc[j], **aurc_from_ranks(rank[j], w)}
    out["n"] = int(w.size)
    out["error_rate"] = float(w.mean())
    return out


SELECTIVE_SCORES = ("total", "mi", "one_minus_conf", "vote_disagreement")   # those of UncertaintyMeter's "auroc"


def selective_of_meter(meter, device):
    """selective() of an UncertaintyMeter(decompose=True)'s per-sample columns: how well total / mi /
    1 - conf / vote_disagreement rank the misclassified samples last among the accepted"""
    ps = meter.per_sample()
    scores = {"total": ps["total"], "mi": ps["mi"], "one_minus_conf": 1.0 - ps["conf"],
              "vote_disagreement": ps["vote_disagreement"]}
    return selective(scores, ps["correct"] == 0, device)


# ---------------------------------------------------------------------------- the AUC table
def positive_prob(logits, positive_class):
    """[..., C] logits -> the f32 softmax probability of the positive class (a torch op: plumbing)"""
    C = logits.shape[-1]
    if not 0 <= positive_class < C:
        raise ValueError(f"positive_class = {positive_class} is outside the {C} classes")
    return torch.softmax(logits.float(), dim=-1)[..., positive_class]


def _variant_prob(logits, positive_class, V):
    """[B, V, C] or [B, V, K, C] -> f32 [B, V] = mean_k softmax(...)[positive_class]"""
    if logits.dim() not in (3, 4) or logits.shape[1] != V:
        raise ValueError(f"logits must hold V = {V} variants on axis 1 of [B, V, (K,) C], got {tuple(logits.shape)}")
    p = positive_prob(logits, positive_class)
    return p.mean(dim=2) if p.dim() == 3 else p


def _control(values):
    vals = list(values)
    if any(v is None for v in vals):
        return {"mean": None, "std": None, "values": vals}
    a = np.asarray(vals, dtype=np.float64)
    return {"mean": float(a.mean()), "std": float(a.std()), "values": [float(v) for v in a]}


def auc_block(aucs, n_repeats):
    """the per-variant AUCs [3 + 2n] in the stack's order -> {"full", "image", "text", "image_control":
    {"mean", "std", "values"}, "text_control": {...}} (std over the n repeats, population form like
    RelianceMeter's; a control with an undefined repeat has mean and std None)"""
    r = n_repeats
    return {"full": aucs[0], "image": aucs[1], "text": aucs[2], "image_control": _control(aucs[3:3 + r]),
            "text_control": _control(aucs[3 + r:3 + 2 * r])}


def _table_aucs(x, pos):
    _, counts = kernels.rank_table(x, pos)
    return auroc_from_counts(counts)


class AucTable:
    """The reference's AUC_table over an evaluation set: the AUROC of the positive class's probability
    under every variant of the robustness stack.  update() keeps the batch's f32 scores [B, V] and
    y == positive_class on the device; result() is one rank_table launch over [S, V]."""

    def __init__(self, n_repeats, positive_class=1, device=None):
        if n_repeats < 1:
            raise ValueError(f"n_repeats = {n_repeats} must be at least 1")
        if positive_class < 0:
            raise ValueError(f"positive_class = {positive_class} must not be negative")
        self.n_repeats, self.positive_class = int(n_repeats), int(positive_class)
        self.V = 3 + 2 * self.n_repeats
        self.device = None if device is None else torch.device(device)
        self.scores, self.pos = [], []        # per batch: f32 [B, V], uint8 [B]

    def update(self, logits, y, layout="BVC"):
        """logits [B, V, C] or [B, V, K, C] (layout "BVC"), or the [V, B, C] tensor of
        robustness_logits(transpose=False) (layout "VBC"); y int [B]"""
        if layout not in ("BVC", "VBC"):
            raise ValueError(f"layout must be 'BVC' or 'VBC', got {layout!r}")
        if layout == "VBC":
            if logits.dim() != 3:
                raise ValueError(f"layout 'VBC' takes the 3-D [V, B, C] tensor, got {tuple(logits.shape)}")
            logits = logits.transpose(0, 1)
        p = _variant_prob(logits, self.positive_class, self.V)
        if tuple(y.shape) != (p.shape[0],):
            raise ValueError(f"y must be [B] = [{p.shape[0]}], got {tuple(y.shape)}")
        if self.device is None:
            self.device = p.device
        self.scores.append(p.to(self.device))
        self.pos.append((y.to(self.device) == self.positive_class).to(torch.uint8))

    def _all(self):
        if not self.scores:
            return (torch.zeros(0, self.V, dtype=torch.float32, device=self.device),
                    torch.zeros(0, dtype=torch.uint8, device=self.device))
        return torch.cat(self.scores).contiguous(), torch.cat(self.pos).contiguous()

    def state(self):
        """plain numpy, picklable: what merge() of another table takes"""
        x, pos = self._all()
        return {"n_repeats": self.n_repeats, "positive_class": self.positive_class,
                "scores": x.cpu().numpy(), "pos": pos.cpu().numpy()}

    def merge(self, state):
        if (state["n_repeats"], state["positive_class"]) != (self.n_repeats, self.positive_class):
            raise ValueError(f"merge: (n_repeats, positive_class) = ({state['n_repeats']}, {state['positive_class']}) "
                             f"!= ({self.n_repeats}, {self.positive_class})")
        x = np.asarray(state["scores"], dtype=np.float32)
        pos = np.asarray(state["pos"], dtype=np.uint8)
        if x.ndim != 2 or x.shape[1] != self.V or pos.shape != (x.shape[0],):
            raise ValueError(f"merge: scores [n, {self.V}] and pos [n], got {x.shape} and {pos.shape}")
        if len(x):
            self.scores.append(torch.from_numpy(x.copy()).to(self.device or "cpu"))
            self.pos.append(torch.from_numpy(pos.copy()).to(self.device or "cpu"))

    def gather(self):
        """data parallel: every rank's state exchanged and merged in rank order (as gather_meters does), so
        all ranks hold the whole set's table; a single process gets itself back"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return self
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, self.state())
        whole = AucTable(self.n_repeats, self.positive_class, self.device)
        for st in parts:
            whole.merge(st)
        return whole

    def result(self):
        """-> {"n", "n_pos", "auc": auc_block}; an undefined AUC (no positive or no negative) is None"""
        x, pos = self._all()
        n = int(x.shape[0])
        if n == 0:
            return {"n": 0, "n_pos": 0, "auc": auc_block([None] * self.V, self.n_repeats)}
        return {"n": n, "n_pos": int(pos.sum()), "auc": auc_block(_table_aucs(x, pos), self.n_repeats)}


AUC_LOG_COLUMNS = tuple(f"auc_{k}" for k in VARIANT_KEYS)


def auc_logs(result, prefix):
    """the history columns of one AucTable.result(): {prefix}_rel_auc_{full, image, text, image_control,
    text_control}, control = the mean over the repeats, NaN where undefined"""
    nan = float("nan")
    auc = result["auc"]
    vals = [auc["full"], auc["image"], auc["text"], auc["image_control"]["mean"], auc["text_control"]["mean"]]
    return {f"{prefix}_rel_{c}": nan if v is None else float(v) for c, v in zip(AUC_LOG_COLUMNS, vals)}


# ---------------------------------------------------------------------------- saved prediction stacks
def _stack_prob(stack, positive_class, V, device, batch=4096):
    """a saved [S, V, (K,) C] prediction stack -> f32 [S, V] on the device"""
    a = _np(stack)
    if a.ndim not in (3, 4) or a.shape[1] != V:
        raise ValueError(f"a prediction stack must be [S, V = {V}, (K,) C], got {a.shape}")
    out = [_variant_prob(torch.from_numpy(np.array(a[i:i + batch])).to(device), positive_class, V)
           for i in range(0, a.shape[0], batch)]
    return torch.cat(out)


def ensemble_auc(stacks, labels, n_repeats, positive_class=1, device="cuda"):
    """The reference's ensemble_overtime: stacks = the saved [S, V, (K,) C] predictions of several
    checkpoints, labels [S].  -> {"n", "n_pos", "n_files", "full": each file's full-variant AUC,
    "ensemble": auc_block of the mean over the files of the per-file probabilities} (softmax, then mean:
    the reference's np.array(predictions).mean(0)); one launch over the F + V columns."""
    if not len(stacks):
        raise ValueError("ensemble_auc: needs at least one prediction stack")
    V = 3 + 2 * int(n_repeats)
    y = _np(labels).reshape(-1)
    probs = [_stack_prob(s, positive_class, V, device) for s in stacks]
    for p in probs:
        if p.shape[0] != y.size:
            raise ValueError(f"ensemble_auc: a stack of {p.shape[0]} samples for {y.size} labels")
    mean = torch.stack(probs).mean(dim=0)                                       # [S, V]
    x = torch.cat([torch.stack([p[:, 0] for p in probs], dim=1), mean], dim=1).contiguous()
    pos = torch.from_numpy((y == positive_class).astype(np.uint8)).to(device)
    aucs = _table_aucs(x, pos)
    F = len(probs)
    return {"n": int(y.size), "n_pos": int((y == positive_class).sum()), "n_files": F, "full": aucs[:F],
            "ensemble": auc_block(aucs[F:], n_repeats)}


def auc_from_files(labels_path, pred_paths, positive_class=1, device="cuda"):
    """eval_mmbt_robustness.py --auc_from: the AUC table of the first saved stack and, with several, the
    ensemble block; n_repeats from the stacks' variant axis (V = 3 + 2n; the reference saves V = 43)"""
    y = np.load(labels_path).reshape(-1)
    stacks = [np.load(p, mmap_mode="r") for p in pred_paths]
    V = stacks[0].shape[1] if stacks[0].ndim in (3, 4) else 0
    if V < 5 or V % 2 == 0:
        raise ValueError(f"{pred_paths[0]}: a prediction stack is [S, V = 3 + 2n, (K,) C], got {stacks[0].shape}")
    n = (V - 3) // 2
    table = AucTable(n, positive_class, device)
    for i in range(0, y.size, 4096):
        table.update(torch.from_numpy(np.array(stacks[0][i:i + 4096])).to(device),
                     torch.from_numpy(y[i:i + 4096]).to(device))
    if stacks[0].shape[0] != y.size:
        raise ValueError(f"{pred_paths[0]}: {stacks[0].shape[0]} samples for {y.size} labels")
    out = table.result()
    out["n_repeats"], out["positive_class"] = n, int(positive_class)
    out["files"] = [os.path.basename(str(p)) for p in pred_paths]
    if len(stacks) > 1:
        ens = ensemble_auc(stacks, y, n, positive_class, device)
        out["ensemble"] = {"n_files": ens["n_files"], "full": ens["full"], "auc": ens["ensemble"]}
    return out
