"""Temperature scaling of the K-member x T-pass ensemble (DESIGN §3 "Temperature scaling").

Inverse temperature beta = 1 / tau, one per member.  For sample s with rows z_kt and label y
(include/mmu.h mmu_temperature_nll):
  p_kt(beta) = softmax(beta_k z_kt)    p_k = mean_t p_kt    p(beta) = mean_k p_k
  nll_s(beta) = -ln max(p(beta)_y, 1e-12)
"shared": all beta_k equal; "per_member": beta a free K-vector; beta = 1 is the unscaled pipeline.

fit_temperature is a pure host function (numpy): it asks an ``evaluate`` callable for the mean NLL of
up to 64 candidate vectors at a time and never looks at logits, so it runs on the CPU against a numpy
evaluator.  TemperatureScaler supplies the evaluator that launches kernels.temperature_nll on the
logits where they lie; this module does no torch math of its own.
"""
import json

import numpy as np

MODES = ("shared", "per_member")
MAX_GRID = 64           # kernels.TEMPERATURE_MAX_CANDIDATES: one pass of the line search is one launch
REL_STOP = 1e-7         # per_member: a round that lowers the mean NLL by less than this (relative) is the last


def _grid(a, b, n):
    """n points uniform in [a, b] with exact ends; a point that is 0 up to rounding is 0 (tau = 1)"""
    u = a + (b - a) * (np.arange(n, dtype=np.float64) / (n - 1))
    u[0], u[-1] = a, b
    u[np.abs(u) <= 1e-12 * (b - a)] = 0.0
    return u


def _argmin(f, u):
    """ties go to the candidate with the smallest |u|, then to the lower index"""
    best = 0
    for i in range(1, len(f)):
        if f[i] < f[best] or (f[i] == f[best] and abs(u[i]) < abs(u[best])):
            best = i
    return best


def _line_search(f_of_u, lo, hi, grid, tol, incumbent=None):
    """Derivative-free search of u = ln tau over the range [lo, hi] (the NLL is not convex in tau):
    evaluate ``grid`` points uniform over the bracket (first the range), take the argmin, make its two
    neighbours on that uniform grid the new bracket -- one spacing either side, clamped at the RANGE ends,
    so an argmin on a bracket end moves the bracket rather than pinning it -- and repeat until the bracket
    is <= tol wide.  With grid = 3 and the middle point best the neighbours are the bracket itself; it is
    then halved around that point.  The bracket shrinks, or (grid = 3) moves to a point that is no worse,
    on every pass, so the search ends even for a tol below fp64's spacing: the bracket collapses to one value.
    f_of_u(u [grid]) -> mean NLL [grid].  -> (u, f, passes, f(0) or None): the best point over all
    passes (and ``incumbent`` = (u, f), when given: it is kept unless a point is strictly lower)."""
    a, b = lo, hi
    best, passes, f_zero = incumbent, 0, None
    while True:
        u = _grid(a, b, grid)
        f = np.asarray(f_of_u(u), dtype=np.float64)
        if f.shape != (grid,) or not np.isfinite(f).all():
            raise ValueError(f"fit_temperature: evaluate must return {grid} finite values, got {f!r}")
        passes += 1
        if f_zero is None and (u == 0.0).any():
            f_zero = float(f[int(np.argmax(u == 0.0))])
        i = _argmin(f, u)
        if best is None or f[i] < best[1] or (incumbent is None and f[i] == best[1] and abs(u[i]) < abs(best[0])):
            best = (float(u[i]), float(f[i]))
        h = (b - a) / (grid - 1)
        na = float(u[i - 1]) if i > 0 else max(lo, a - h)
        nb = float(u[i + 1]) if i < grid - 1 else min(hi, b + h)
        if nb - na >= b - a and na == a and nb == b:    # grid = 3, the middle point best
            na, nb = 0.5 * (a + float(u[i])), 0.5 * (float(u[i]) + b)
        a, b = na, nb
        if b - a <= tol:
            return best[0], best[1], passes, f_zero


def fit_temperature(evaluate, K, mode="shared", tau_range=(0.05, 20.0), grid=33, tol=1e-4, max_rounds=8):
    """Fit the ensemble's temperature(s) on the mean NLL.  evaluate(beta f64 [J, K]) -> f64 [J], the mean
    NLL under each of the J <= grid inverse-temperature vectors.
    shared: one line search (see _line_search) with all columns equal -- 4 passes with the defaults.
    per_member: start from the shared fit, then coordinate descent: a line search over u_k with the
    other members fixed, k = 0 .. K-1; a coordinate move is accepted only if it lowers the mean NLL;
    stop after a round that lowers it by less than 1e-7 relative, or after max_rounds.
    -> {mode, tau [K], nll_before (beta = 1), nll_after, passes (evaluate calls), rounds, at_bound [K]
    (a final u_k sits on a range end)}."""
    if mode not in MODES:
        raise ValueError(f"fit_temperature: mode must be one of {MODES}, got {mode!r}")
    if int(K) != K or K < 1:
        raise ValueError(f"fit_temperature: K = {K!r} must be a positive integer")
    if int(grid) != grid or not 3 <= grid <= MAX_GRID:
        raise ValueError(f"fit_temperature: grid = {grid!r} must be 3 .. {MAX_GRID}")
    try:
        t_lo, t_hi = (float(v) for v in tau_range)
    except (TypeError, ValueError):
        raise ValueError(f"fit_temperature: tau_range must be a (low, high) pair, got {tau_range!r}") from None
    if not (np.isfinite(t_lo) and np.isfinite(t_hi) and 0.0 < t_lo < t_hi):
        raise ValueError(f"fit_temperature: tau_range = {tau_range!r} must be positive with low < high")
    if not t_lo <= 1.0 <= t_hi:
        raise ValueError(f"fit_temperature: tau_range = {tau_range!r} must contain tau = 1")
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError(f"fit_temperature: tol = {tol!r} must be positive")
    if int(max_rounds) != max_rounds or max_rounds < 1:
        raise ValueError(f"fit_temperature: max_rounds = {max_rounds!r} must be a positive integer")
    K, grid = int(K), int(grid)
    lo, hi = float(np.log(t_lo)), float(np.log(t_hi))
    if t_lo == 1.0:
        lo = 0.0
    if t_hi == 1.0:
        hi = 0.0
    if t_lo * t_hi == 1.0:      # a range symmetric in ln tau is exactly so: an odd grid then holds u = 0
        lo = -hi
    calls = [0]

    def ev(beta):
        calls[0] += 1
        return np.asarray(evaluate(np.ascontiguousarray(beta, dtype=np.float64)), dtype=np.float64).reshape(-1)

    u_s, f_s, _, f_one = _line_search(lambda u: ev(np.repeat(np.exp(-u)[:, None], K, axis=1)), lo, hi, grid, tol)
    if f_one is None:           # no grid point was tau = 1 (an even grid, a lopsided range)
        f_one = float(ev(np.ones((1, K)))[0])
    u = np.full(K, u_s)
    f_cur, rounds = f_s, 0
    if mode == "per_member":
        for _ in range(int(max_rounds)):
            f_start = f_cur
            for k in range(K):
                def along(uk, k=k):
                    beta = np.repeat(np.exp(-u)[None, :], len(uk), axis=0)
                    beta[:, k] = np.exp(-uk)
                    return ev(beta)
                u_k, f_k, _, _ = _line_search(along, lo, hi, grid, tol, incumbent=(float(u[k]), f_cur))
                if f_k < f_cur:
                    u[k], f_cur = u_k, f_k
            rounds += 1
            if f_start - f_cur < REL_STOP * abs(f_start):
                break
    return {"mode": mode, "tau": [float(v) for v in np.exp(u)], "nll_before": float(f_one),
            "nll_after": float(f_cur), "passes": calls[0], "rounds": rounds,
            "at_bound": [bool(v == lo or v == hi) for v in u]}


RESULT_KEYS = ("mode", "tau", "nll_before", "nll_after", "passes", "rounds", "at_bound")


class TemperatureScaler:
    """Fits and applies the ensemble's temperature(s).
        sc = TemperatureScaler("shared")
        for x, y in dev_split: sc.add(ens.logits(...), y)        # [K, T, B, C], kept where they are
        sc.fit(); meter = UncertaintyMeter(15, decompose=True, inv_temp=sc.inv_temp(device))
    add() keeps the device tensors it is given and makes no copy: S K T C 4 bytes stay alive until fit()
    has run (303 MB for Food-101's 5,000-sample dev split at K = 5, T = 30, C = 101); clear() drops them.
    Every pass of the search is one kernels.temperature_nll launch per chunk with one [J, K] table."""

    def __init__(self, mode="shared", **fit_options):
        if mode not in MODES:
            raise ValueError(f"TemperatureScaler: mode must be one of {MODES}, got {mode!r}")
        self.mode, self.fit_options = mode, dict(fit_options)
        self.chunks, self.result = [], None
        self.extra = {}     # load(): what the file held beside the fit result (the entry point's fit_phase)

    def add(self, logits, y, layout="KTBC"):
        """logits f32 [K, T, B, C] as EnsembleMMBT.logits returns them (layout "KTBC", read in place through
        their strides) or [S, K, T, C] (layout "SKTC"), on the device; y [S]."""
        import torch
        if layout not in ("KTBC", "SKTC") or logits.dim() != 4:
            raise ValueError("TemperatureScaler.add: logits [K, T, B, C] (layout 'KTBC') or [S, K, T, C] (layout "
                             f"'SKTC'), got {tuple(logits.shape)} with layout {layout!r}")
        if logits.dtype != torch.float32:
            raise ValueError(f"TemperatureScaler.add: logits must be float32 (they are kept, not copied), got "
                             f"{logits.dtype}")
        lo = logits.permute(2, 0, 1, 3) if layout == "KTBC" else logits     # a view: the kernel takes the strides
        if self.chunks and lo.shape[1] != self.chunks[0][0].shape[1]:
            raise ValueError(f"TemperatureScaler.add: {lo.shape[1]} members, the earlier chunks had "
                             f"{self.chunks[0][0].shape[1]}")
        if y.shape != (lo.shape[0],):
            raise ValueError(f"TemperatureScaler.add: y must be [S] = [{lo.shape[0]}], got {tuple(y.shape)}")
        self.chunks.append((lo, y.long().contiguous()))

    def clear(self):
        self.chunks = []

    @property
    def count(self):
        return sum(lo.shape[0] for lo, _ in self.chunks)

    def mean_nll(self, beta):
        """beta f64 [J, K] -> f64 [J]: the chunks' nll_sum added in chunk order in f64, over the sample count"""
        import torch
        from . import kernels
        beta = np.asarray(beta, dtype=np.float64)
        dev = self.chunks[0][0].device
        table = torch.from_numpy(beta.astype(np.float32)).to(dev)
        sums = []
        for lo, y in self.chunks:
            nll = torch.empty(lo.shape[0], beta.shape[0], dtype=torch.float32, device=dev)
            nll_sum = torch.empty(beta.shape[0], dtype=torch.float64, device=dev)
            kernels.temperature_nll(lo, y, table, nll, nll_sum)
            sums.append(nll_sum)
        total = np.zeros(beta.shape[0], dtype=np.float64)
        for s in sums:
            total += s.cpu().numpy()
        return total / self.count

    def fit(self):
        if not self.chunks:
            raise ValueError("TemperatureScaler.fit: no logits were added")
        self.result = fit_temperature(self.mean_nll, self.chunks[0][0].shape[1], mode=self.mode, **self.fit_options)
        return self.result

    def _need_result(self, who):
        if self.result is None:
            raise ValueError(f"TemperatureScaler.{who}: nothing fitted or loaded yet")

    def inv_temp(self, device=None):
        """-> f32 [K] = 1 / tau, on ``device`` (what UncertaintyMeter(inv_temp=...) takes)"""
        import torch
        self._need_result("inv_temp")
        beta = (1.0 / np.asarray(self.result["tau"], dtype=np.float64)).astype(np.float32)
        return torch.from_numpy(beta).to(device) if device is not None else torch.from_numpy(beta)

    def save(self, path):
        """the fit result as strict JSON"""
        self._need_result("save")
        with open(path, "w") as f:
            json.dump({k: self.result[k] for k in RESULT_KEYS}, f, indent=1, allow_nan=False)

    @classmethod
    def load(cls, path):
        """a scaler holding the fit result of ``path`` (a save() file, or any JSON object that has its keys)"""
        with open(path) as f:
            d = json.load(f)
        missing = [k for k in RESULT_KEYS if k not in d] if isinstance(d, dict) else list(RESULT_KEYS)
        if missing:
            raise ValueError(f"TemperatureScaler.load: {path} lacks {missing}")
        tau = d["tau"]
        if d["mode"] not in MODES or not isinstance(tau, list) or not tau or not all(
                isinstance(v, (int, float)) and np.isfinite(v) and v > 0 for v in tau):
            raise ValueError(f"TemperatureScaler.load: {path} holds no valid fit (mode {d['mode']!r}, tau {tau!r})")
        sc = cls(d["mode"])
        sc.result = {k: d[k] for k in RESULT_KEYS}
        sc.extra = {k: v for k, v in d.items() if k not in RESULT_KEYS}
        return sc
