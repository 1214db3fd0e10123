"""Table, gradients, reference and rounding model for the fused BertAdam step (csrc/optim.hip).
Pure torch on the CPU.  Used by test_bertadam_reference.py (CPU) and test_bertadam_edges_gpu.py.

Reference: oracle/bertadam_ref.py on float64 tensors; rounding model: the same on float32 tensors
(clip coefficient from the float64 norm, moments and update in f32 in the kernel's order).  Both
take the hyperparameters rounded to f32, as they cross the C ABI (mmu_bertadam_step takes floats):
the kernel forms 1 - b2 from the f32 b2 = 0.99900001287, i.e. 0.00099998713, 1.3e-5 below the
0.001 a double-precision BertAdam multiplies by.  That offset is the ABI's, not a rounding error of
the kernels, so it is on both sides of the comparison here ("BatchNorm and BertAdam edge
sweeps").

Table (layout): packed as src/params.py ParamStore.build packs it -- f32 offsets cumulative in
flat order with no padding, the bf16 copies cumulative over their own subset in their own order
(COPY_ORDER).  Sizes 1, 3, 5, 255, 257, CH - 1, CH + 1, 2 CH + 3 with the test chunk length CH =
1024, one tensor of 65536 + 5 elements chunked at the production 65536, and two inactive tensors
between active ones.  Active tensors start at f32 offsets = 0, 1, 2 and 3 (mod 4); (f32 offset,
copy offset) mod 4 covers aligned / aligned, aligned / misaligned, misaligned / aligned,
misaligned / misaligned and no copy: every arm of adam_update_kernel's `vec` and both the scalar
head and the 16-B body of adam_sqnorm_kernel.

Gradients (grads): fresh magnitudes on every step with a fixed sign per element (so m never
cancels and |m| is the scale of its own rounding errors); tensors at a misaligned offset carry
their largest magnitudes, 100 x the rest, in the first three and the last three elements, so the
clip coefficient depends on the scalar head and tail of the norm; roles: "zero" an all-zero
gradient, "under" a norm of 0.999 max_grad_norm (unclipped), "between" a norm of 1.5 max_grad_norm
(clipped, but unclipped once grad_scale = 0.5 halves it), "clip" far above, "small" far below.
"""
import torch

from oracle.bertadam_ref import bertadam_step, schedule_factor

CH, BIG_CH = 1024, 65536
# (numel, active, weight-decay group, chunk length, gradient role) in flat order
TENSORS = (
    (255, 1, 0, CH, "under"),
    (CH - 1, 1, 1, CH, "clip"),
    (7, 0, 0, CH, None),
    (2 * CH + 3, 1, 0, CH, "clip"),
    (BIG_CH + 5, 1, 1, BIG_CH, "clip"),
    (3, 1, 0, CH, "zero"),
    (257, 1, 0, CH, "between"),
    (1, 1, 1, CH, "clip"),
    (CH + 1, 1, 1, CH, "small"),
    (2, 0, 1, CH, None),
    (5, 1, 1, CH, "small"),
)
COPY_ORDER = (4, 0, 1, 3, 6, 8, 9, 10)   # the tensors with a bf16 copy, in the copy buffer's order


def f32(x):
    """a hyperparameter as the kernel receives it"""
    return torch.tensor(x, dtype=torch.float32).double().item()


def layout():
    """-> dict: offs, sizes, active, groups, roles, coffs (-1: no copy), chunks [(tensor, start,
    len)], first [first chunk of each tensor], table (int64: 7 per tensor, then 3 per chunk),
    total, ctotal"""
    sizes = [t[0] for t in TENSORS]
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    coffs, c = [-1] * len(sizes), 0
    for t in COPY_ORDER:
        coffs[t] = c
        c += sizes[t]
    chunks, rows = [], []
    for t, (n, act, grp, ch, _) in enumerate(TENSORS):
        first = len(chunks)
        for s in range(0, n, ch):
            chunks.append((t, s, min(ch, n - s)))
        rows.append((offs[t], n, grp, coffs[t], act, first, len(chunks) - first))
    table = torch.tensor([x for r in rows for x in r] + [x for ck in chunks for x in ck], dtype=torch.int64)
    return {"offs": offs, "sizes": sizes, "active": [t[1] for t in TENSORS], "groups": [t[2] for t in TENSORS],
            "roles": [t[4] for t in TENSORS], "coffs": coffs, "chunks": chunks, "table": table, "total": sum(sizes),
            "ctotal": c}


def grads(L, step, max_grad_norm=1.0):
    """the flat f32 gradient of one step (NaN in the inactive tensors: never read)"""
    flat = torch.full((L["total"],), float("nan"))
    mx = max_grad_norm if max_grad_norm > 0 else 1.0
    for t, (n, act, _, _, role) in enumerate(TENSORS):
        if not act:
            continue
        sign = torch.where(torch.rand(n, generator=torch.Generator().manual_seed(100 + t)) < 0.5, -1.0, 1.0)
        g = torch.rand(n, generator=torch.Generator().manual_seed(1000 * step + t)).double() + 0.5
        if L["offs"][t] % 4 and n >= 6:
            g[:3] *= 100.0
            g[-3:] *= 100.0
        norm = {"zero": 0.0, "under": 0.999 * mx, "between": 1.5 * mx, "clip": 7.0 * mx * (1 + step),
                "small": 0.02 * mx}[role]
        flat[L["offs"][t]:L["offs"][t] + n] = (g * (norm / g.norm()) * sign).float()
    return flat


def initial(L, seed=0):
    """-> flat p, m, v (f32) and the bf16 copy buffer.  Active moments start at zero (a first
    step), the inactive tensors' hold values that must survive; the copies start as bf16(p)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(L["total"], generator=g)
    m, v = torch.zeros(L["total"]), torch.zeros(L["total"])
    copy = torch.zeros(L["ctotal"], dtype=torch.bfloat16)
    for t, n in enumerate(L["sizes"]):
        o = L["offs"][t]
        if not L["active"][t]:
            m[o:o + n] = torch.randn(n, generator=g)
            v[o:o + n] = torch.rand(n, generator=g)
        if L["coffs"][t] >= 0:
            copy[L["coffs"][t]:L["coffs"][t] + n] = p[o:o + n].to(torch.bfloat16)
    return p, m, v, copy


HYPER = dict(lr_decay=f32(1e-3), lr_nodecay=f32(3e-3), wd=f32(0.01), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-6))
# the runs: (name, t_total, warmup, max_grad_norm, grad_scale).  t_total = 5 with warmup 0.4 crosses
# the warmup knee at step 2, reaches t_total at step 5 and clamps at 0 there
RUNS = (("sched", 5.0, f32(0.4), 1.0, 1.0), ("sched-half", 5.0, f32(0.4), 1.0, 0.5), ("flat", -1.0, f32(0.4), 1.0, 1.0),
        ("noclip-half", 5.0, f32(0.4), 0.0, 0.5))
STEPS = 6


class Track:
    """the state of every active tensor in one dtype (float64: the reference, float32: the model),
    stepped by oracle.bertadam_ref.bertadam_step"""

    def __init__(self, L, p, m, v, dtype):
        self.L, self.dt = L, dtype
        self.act = [t for t in range(len(L["sizes"])) if L["active"][t]]
        cut = lambda flat, t: flat[L["offs"][t]:L["offs"][t] + L["sizes"][t]].to(dtype).clone()  # noqa: E731
        self.p, self.m, self.v = ({t: cut(f, t) for t in self.act} for f in (p, m, v))
        self.steps = {t: 0 for t in self.act}
        self.scale = {}

    def load(self, p, m, v):
        """restart from flat f32 buffers (the kernel's or the model's state): every step is then
        compared on its own, one step's rounding errors against one step's"""
        L = self.L
        for t in self.act:
            for mine, flat in ((self.p, p), (self.m, m), (self.v, v)):
                mine[t] = flat[L["offs"][t]:L["offs"][t] + L["sizes"][t]].to(self.dt).clone()

    def flat(self, like):
        """the state as flat f32 buffers (the inactive tensors from `like` = (p, m, v))"""
        out = [f.clone() for f in like]
        for t in self.act:
            o, n = self.L["offs"][t], self.L["sizes"][t]
            for f, mine in zip(out, (self.p, self.m, self.v)):
                f[o:o + n] = mine[t].float()
        return out

    def step(self, g, run):
        _, t_total, warmup, max_norm, gscale = run
        L, H = self.L, HYPER
        for t in self.act:
            grp = L["groups"][t]
            lr, wd = (H["lr_decay"], H["wd"]) if grp == 0 else (H["lr_nodecay"], 0.0)
            p_old = self.p[t].clone()
            st = self.steps[t]
            gt = g[L["offs"][t]:L["offs"][t] + L["sizes"][t]].to(self.dt)
            (self.steps[t],) = bertadam_step([self.p[t]], [gt], [self.m[t]], [self.v[t]], [st], lr, [wd], warmup, t_total,
                                             H["b1"], H["b2"], H["eps"], max_norm, gscale)
            if self.dt == torch.float64:  # the scales: |p| + lr |u|, |m|, |v|
                lr_eff = lr * schedule_factor(st, warmup, t_total)
                u = (self.m[t] / (self.v[t].sqrt() + H["eps"])).abs() + wd * p_old.abs()
                self.scale[t] = {"p": self.p[t].abs() + lr_eff * u, "m": self.m[t].abs(), "v": self.v[t].abs()}
