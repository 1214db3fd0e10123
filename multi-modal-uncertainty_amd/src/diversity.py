"""Ensemble diversity: which members of a K-member ensemble (or which heads of a multi-head model)
disagree with which, by how much, and whether their errors coincide.

The reference's "Prediction Diversity Analysis" (notebooks/analysis_round_1.py:68-113) mutes the true
class, keeps each sub-network's top-5 probabilities and reports the Kendall tau between two
sub-networks next to their accuracies.  kernels.ensemble_diversity (csrc/diversity.hip, include/mmu.h
mmu_ensemble_diversity) forms, per sample and per pair of members, the Jensen-Shannon divergence of the
two predictions, whether their argmax classes differ, and that Kendall tau-b -- per sample, where the
reference pools all samples' values into one rank statistic (the two coincide for one sample) -- from
the [K, T, B, C] logits read in place.  DiversityMeter accumulates those rows (numpy only) and
result() is the analysis, in fp64 on the host: the pairwise means, and from member_arg == y the
classical diversity measures of the members' error indicators.
"""
import itertools

import numpy as np
import torch


def _mean_or_none(values):
    vals = [v for v in values if v is not None]
    return float(np.mean(vals)) if vals else None


class DiversityMeter:
    """Accumulates the per-sample rows of kernels.ensemble_diversity over an evaluation set.

    update() runs the kernel on a batch; update_rows() is the host-only accumulator (fp64 pair rows
    [B, P, DIV_NPAIR], member_arg [B, K], y [B]); result() is the analysis.  The number of members is
    fixed by the first rows."""

    def __init__(self, top=5, mute_true=True):
        from . import kernels
        if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 0 <= top <= kernels.DIV_MAX_TOP:
            raise ValueError(f"top = {top!r} must be an integer 0 .. {kernels.DIV_MAX_TOP} (0: no truncation)")
        self.top, self.mute_true = int(top), bool(mute_true)
        self.columns = kernels.DIV_COLUMNS
        self.K = None
        self.pair, self.member_arg, self.y = [], [], []

    # ---------------------------------------------------------------- accumulation
    def update(self, logits, y, layout="KTBC"):
        """logits [K, T, B, C] as EnsembleMMBT.logits returns them (layout "KTBC", read in place through
        their strides), or [S, K, T, C] / the [S, K, C] heads of a head model (layout "SKTC"); y [B].
        -> the pair tensor f32 [B, P, DIV_NPAIR]"""
        from . import kernels
        if layout not in ("KTBC", "SKTC"):
            raise ValueError(f"layout must be 'KTBC' or 'SKTC', got {layout!r}")
        if logits.dim() != 4 and not (layout == "SKTC" and logits.dim() == 3):
            raise ValueError("DiversityMeter.update: logits [K, T, B, C] (layout 'KTBC') or [S, K, T, C] / "
                             f"[S, K, C] (layout 'SKTC'), got {tuple(logits.shape)} with layout {layout!r}")
        lo = logits.float()                                       # (f32 already: no copy)
        lo = lo.permute(2, 0, 1, 3) if layout == "KTBC" else lo   # a view: the kernel takes the strides
        S, Km = lo.shape[0], lo.shape[1]
        if Km < 2:
            raise ValueError(f"diversity needs at least 2 members, got K = {Km}")
        P = Km * (Km - 1) // 2
        pair = torch.empty(S, P, kernels.DIV_NPAIR, dtype=torch.float32, device=lo.device)
        arg = torch.empty(S, Km, dtype=torch.int32, device=lo.device)
        y = y.long().contiguous()
        kernels.ensemble_diversity(lo, y, pair, None, arg, top=self.top, mute_true=self.mute_true)
        self.update_rows(pair.double().cpu().numpy(), arg.cpu().numpy(), y.cpu().numpy())
        return pair

    def update_rows(self, pair, member_arg, y):
        pair = np.asarray(pair, dtype=np.float64)
        member_arg, y = np.asarray(member_arg).astype(np.int64), np.asarray(y).astype(np.int64)
        if member_arg.ndim != 2 or member_arg.shape[1] < 2:
            raise ValueError(f"member_arg must be [B, K] with K >= 2, got {member_arg.shape}")
        B, Km = member_arg.shape
        if self.K is not None and Km != self.K:
            raise ValueError(f"member_arg holds {Km} members, the meter {self.K}")
        if pair.shape != (B, Km * (Km - 1) // 2, len(self.columns)):
            raise ValueError(f"pair must be [B, P, {len(self.columns)}] = [{B}, {Km * (Km - 1) // 2}, "
                             f"{len(self.columns)}], got {pair.shape}")
        if y.shape != (B,):
            raise ValueError(f"y must be [{B}], got {y.shape}")
        self.K = Km
        self.pair.append(pair.copy())
        self.member_arg.append(member_arg.copy())
        self.y.append(y.copy())

    def _all(self):
        Km = self.K or 2
        if not self.pair:
            return (np.zeros((0, Km * (Km - 1) // 2, len(self.columns))), np.zeros((0, Km), dtype=np.int64),
                    np.zeros(0, dtype=np.int64))
        return np.concatenate(self.pair), np.concatenate(self.member_arg), np.concatenate(self.y)

    def per_sample(self):
        """{column: fp64 [n, P]}, "member_arg" [n, K] and "y" [n]"""
        pair, arg, y = self._all()
        out = {c: pair[:, :, i].copy() for i, c in enumerate(self.columns)}
        out.update(member_arg=arg, y=y)
        return out

    def state(self):
        """plain numpy, picklable: what merge() of another meter takes"""
        pair, arg, y = self._all()
        return {"top": self.top, "mute_true": self.mute_true, "K": self.K, "pair": pair, "member_arg": arg, "y": y}

    def merge(self, state):
        if (state["top"], state["mute_true"]) != (self.top, self.mute_true):
            raise ValueError(f"merge: (top, mute_true) {(state['top'], state['mute_true'])} != "
                             f"{(self.top, self.mute_true)}")
        if len(state["y"]):
            self.update_rows(state["pair"], state["member_arg"], state["y"])

    # ---------------------------------------------------------------- analysis
    def result(self):
        """fp64 on the host.  Per pair (lists in itertools.combinations order, "pairs") and as K x K
        symmetric matrices ("matrix"; the diagonal is 0 for js / disagree and None elsewhere):
          js, disagree: means over the samples;  tau: the mean over the samples where it is defined, and
          tau_n, how many those were;  contingency [N11, N10, N01, N00] of the error indicators
          member_arg == y (1: right; first index member i);  double_fault = N00 / N;  q = Yule's
          (N11 N00 - N01 N10) / (N11 N00 + N01 N10);  phi, the correlation of the two indicators.
        "member_acc" per member, "mean": each figure's mean over the pairs where it is defined.
        A figure that is not defined (no sample, a zero denominator) is None."""
        pair, arg, y = self._all()
        n = int(len(y))
        out = {"n": n, "K": self.K, "top": self.top, "mute_true": self.mute_true}
        if self.K is None:
            return out
        Km = self.K
        pairs = list(itertools.combinations(range(Km), 2))
        col = {c: i for i, c in enumerate(self.columns)}
        hit = arg == y[:, None]
        fig = {k: [] for k in ("js", "disagree", "tau", "tau_n", "contingency", "double_fault", "q", "phi")}
        for q, (i, j) in enumerate(pairs):
            fig["js"].append(float(pair[:, q, col["js"]].mean()) if n else None)
            fig["disagree"].append(float(pair[:, q, col["disagree"]].mean()) if n else None)
            tau = pair[:, q, col["tau"]]
            ok = np.isfinite(tau)
            fig["tau_n"].append(int(ok.sum()))
            fig["tau"].append(float(tau[ok].mean()) if ok.any() else None)
            n11 = int((hit[:, i] & hit[:, j]).sum())
            n10 = int((hit[:, i] & ~hit[:, j]).sum())
            n01 = int((~hit[:, i] & hit[:, j]).sum())
            n00 = int((~hit[:, i] & ~hit[:, j]).sum())
            fig["contingency"].append([n11, n10, n01, n00])
            fig["double_fault"].append(n00 / n if n else None)
            num, den = float(n11 * n00 - n01 * n10), float(n11 * n00 + n01 * n10)
            fig["q"].append(num / den if den > 0 else None)
            den = float(n11 + n10) * float(n01 + n00) * float(n11 + n01) * float(n10 + n00)
            fig["phi"].append(num / float(np.sqrt(den)) if den > 0 else None)
        out["pairs"] = [list(p) for p in pairs]
        out.update(fig)
        out["member_acc"] = [float(hit[:, k].mean()) if n else None for k in range(Km)]
        out["matrix"] = {}
        for name in ("js", "disagree", "tau", "double_fault", "q", "phi"):
            mat = [[0.0 if (name in ("js", "disagree") and a == b) else None for b in range(Km)] for a in range(Km)]
            for (i, j), v in zip(pairs, fig[name]):
                mat[i][j] = mat[j][i] = v
            out["matrix"][name] = mat
        out["mean"] = {name: _mean_or_none(fig[name]) for name in ("js", "disagree", "tau", "double_fault", "q", "phi")}
        return out


def check_diversity_flags(n_members, top):
    """what eval_robustness.py --diversity needs, before any model is built"""
    from . import kernels
    if n_members < 2:
        raise ValueError(f"--diversity compares pairs of members: {n_members} member(s) given "
                         "(--checkpoint_paths with at least 2 checkpoints)")
    if n_members > kernels.DIV_MAX_MEMBERS:
        raise ValueError(f"--diversity takes at most {kernels.DIV_MAX_MEMBERS} members, got {n_members}")
    if not 0 <= top <= kernels.DIV_MAX_TOP:
        raise ValueError(f"--diversity_top {top} must be 0 .. {kernels.DIV_MAX_TOP} (0: no truncation)")


def diversity_from_files(logits_path, labels_path, device, top=5, mute_true=True, batch=4096):
    """the meter alone over a saved [S, K, T, C] logits file (what eval_robustness.py --mmbt writes)
    and its [S] labels; no model is built"""
    z, y = np.load(logits_path), np.load(labels_path)
    if z.ndim not in (3, 4) or y.shape != (z.shape[0],):
        raise ValueError(f"expected logits [S, K, T, C] (or [S, K, C]) and labels [S], got {z.shape} and {y.shape}")
    check_diversity_flags(z.shape[1], top)
    meter = DiversityMeter(top, mute_true)
    for a in range(0, z.shape[0], batch):
        lo = torch.from_numpy(np.ascontiguousarray(z[a:a + batch], dtype=np.float32)).to(device)
        meter.update(lo, torch.from_numpy(np.asarray(y[a:a + batch]).astype(np.int64)).to(device), layout="SKTC")
    return meter
