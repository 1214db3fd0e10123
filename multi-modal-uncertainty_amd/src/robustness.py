"""Batched modality-robustness pass (eval_mmbt_robustness.py:76-103 semantics).

Per batch the reference runs 3 + 2*n_repeats full pipelines (full, image-only,
text-only, n image-control and n text-control forwards), recomputing ResNet-152
and both embeddings every time.  Here the image features / projection are
computed ONCE per batch and the 43 encoder passes are batched by sequence length:
  L = 5+T : full                                    1 variant
  L = 5   : image-only + n image controls           1+n variants, one embed + one encoder pass
  L = 1+T : text-only + n text controls             1+n variants, one embed + one encoder pass
The control index sets are drawn from the global torch RNG in exactly the
reference's order (all image draws, then all text draws; src/mmbt.py:198-201),
so the same seed gives the same variants.  Output: [B, 3 + 2n, n_classes] logits
in the reference's stacking order.

The answer the stack is raw material for -- how much the model relies on each modality
(notebooks/food101_robustness.py, notebooks/utils.py: the label probability's shift under a
modality-only forward set against its mean shift under the controls, Pearson's R of the two over
the samples, accuracy per variant) -- is formed on the device per sample by
kernels.robustness_summary (csrc/robustness.hip) and accumulated by RelianceMeter (numpy only);
RelianceCallback tracks it per epoch during training.
"""
import numpy as np
import torch

from .callbacks import Callback
from .mmbt import control_indices


@torch.no_grad()
def robustness_logits(model, txt, mask, segment, img, n_repeats=20, transpose=True):
    """model(*x) order: (txt, mask, segment, img) as forward(txt, mask, segment, img) sees them.
    transpose=False: the [3 + 2n, B, C] tensor as the three launches left it, without the final
    transposed copy (RelianceMeter.update(..., layout="VBC") reads it in place)."""
    enc = model.enc
    enc._prepare()
    B, T = txt.shape
    n_img = enc.n_img
    S = n_img + 2 + T
    dev = img.device
    proj = enc.img_embeddings.project(enc._image_feats(img))
    img_idx = [control_indices(S, n_img + 1) for _ in range(n_repeats)]
    txt_idx = [control_indices(S, T) for _ in range(n_repeats)]

    def run(idx_list, Lout):
        V = len(idx_list)
        idx = torch.stack(idx_list).to(dev) if idx_list[0] is not None else None
        X, km, L = enc._embed(txt, mask, segment, proj, idx=idx, Lout=Lout, V=V)
        h = enc._encode(X, km, V * B, L)
        return model.clf(enc._pool(h, V * B, L)).view(V, B, -1)

    full = run([None], S)
    img_only = torch.arange(n_img + 2)
    txt_only = torch.cat([torch.zeros(1, dtype=torch.long), torch.arange(T) + n_img + 2])
    short = run([img_only] + img_idx, n_img + 2)
    long_ = run([txt_only] + txt_idx, T + 1)
    out = torch.cat([full, short[:1], long_[:1], short[1:], long_[1:]], dim=0)  # [3+2n, B, C]
    if not transpose:
        return out
    return out.transpose(0, 1).contiguous()


def pearson(a, b):
    """Pearson's R of two equally long fp64 vectors, signed; None for fewer than 2 points or a constant side"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size < 2 or np.ptp(a) == 0 or np.ptp(b) == 0:
        return None
    da, db = a - a.mean(), b - b.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return float((da * db).sum() / den) if den > 0 else None


class RelianceMeter:
    """Accumulates the per-sample rows of kernels.robustness_summary over an evaluation set.

    update() runs the kernel on a batch of the stack; update_rows() is the host-only accumulator
    (fp64 rows [B, ROB_NSTAT] and the per-variant hit sums [V]); result() is the analysis."""

    def __init__(self, n_repeats):
        from . import kernels
        if n_repeats < 1:
            raise ValueError(f"n_repeats = {n_repeats} must be at least 1")
        self.n_repeats = int(n_repeats)
        self.V = 3 + 2 * self.n_repeats
        self.columns = kernels.ROB_COLUMNS
        self.rows = []
        self.hits = np.zeros(self.V, dtype=np.float64)

    # ---------------------------------------------------------------- accumulation
    def update(self, logits, y, layout="BVC"):
        """logits [B, V, C] or [B, V, K, C] (layout "BVC"), or the [V, B, C] tensor of
        robustness_logits(transpose=False) (layout "VBC"), read in place; y int64 [B].
        -> the per_variant tensor f32 [B, 3, V] = (p_label, js, hit)"""
        from . import kernels
        if layout not in ("BVC", "VBC"):
            raise ValueError(f"layout must be 'BVC' or 'VBC', got {layout!r}")
        if layout == "VBC":
            if logits.dim() != 3:
                raise ValueError(f"layout 'VBC' takes the 3-D [V, B, C] tensor, got {tuple(logits.shape)}")
            logits = logits.transpose(0, 1)
        if logits.dim() not in (3, 4) or logits.shape[1] != self.V:
            raise ValueError(f"logits must hold V = {self.V} variants on axis 1 of [B, V, (K,) C], got "
                             f"{tuple(logits.shape)}")
        if logits.dtype != torch.float32:
            logits = logits.float()
        B = logits.shape[0]
        stats = torch.empty(B, kernels.ROB_NSTAT, dtype=torch.float32, device=logits.device)
        pv = torch.empty(B, 3, self.V, dtype=torch.float32, device=logits.device)
        kernels.robustness_summary(logits, y, stats, pv)
        self.update_rows(stats.double().cpu().numpy(), pv[:, 2].double().sum(0).cpu().numpy())
        return pv

    def update_rows(self, stats, hits):
        stats, hits = np.asarray(stats, dtype=np.float64), np.asarray(hits, dtype=np.float64)
        if stats.ndim != 2 or stats.shape[1] != len(self.columns):
            raise ValueError(f"stats must be [B, {len(self.columns)}], got {stats.shape}")
        if hits.shape != (self.V,):
            raise ValueError(f"hits must be [{self.V}], got {hits.shape}")
        self.rows.append(stats.copy())
        self.hits += hits

    def _all_rows(self):
        return np.concatenate(self.rows) if self.rows else np.zeros((0, len(self.columns)))

    def per_sample(self):
        rows = self._all_rows()
        return {c: rows[:, i].copy() for i, c in enumerate(self.columns)}

    def state(self):
        """plain numpy, picklable: what merge() of another meter takes"""
        return {"n_repeats": self.n_repeats, "rows": self._all_rows(), "hits": self.hits.copy()}

    def merge(self, state):
        if state["n_repeats"] != self.n_repeats:
            raise ValueError(f"merge: n_repeats {state['n_repeats']} != {self.n_repeats}")
        if len(state["rows"]):
            self.update_rows(state["rows"], state["hits"])

    # ---------------------------------------------------------------- analysis
    def result(self):
        ps, n, r = self.per_sample(), sum(len(x) for x in self.rows), self.n_repeats
        frac = self.hits / n if n else np.zeros(self.V)
        ctl = lambda v: {"mean": float(v.mean()), "std": float(v.std())}  # noqa: E731  over the n repeats
        out = {"n": int(n),
               "acc": {"full": float(frac[0]), "image": float(frac[1]), "text": float(frac[2]),
                       "image_control": ctl(frac[3:3 + r]), "text_control": ctl(frac[3 + r:])},
               "corr": {m: pearson(ps[f"dp_{m}"], ps[f"dp_{m}_control"]) for m in ("image", "text")},
               "js_corr": {m: pearson(ps[f"js_{m}"], ps[f"js_{m}_control"]) for m in ("image", "text")}}
        for c in self.columns:
            out[c] = float(ps[c].mean()) if n else float("nan")
        return out


def json_safe(obj):
    """a result() for a strict JSON writer: NaN / inf floats (column means of an empty meter) become None
    like an undefined correlation, containers are walked"""
    if isinstance(obj, dict):
        return {k: json_safe(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [json_safe(v) for v in obj]
    if isinstance(obj, float) and not np.isfinite(obj):
        return None
    return obj


REL_COLUMNS = ("corr_image", "corr_text", "acc_full", "acc_image", "acc_text", "acc_image_control",
               "acc_text_control", "js_image", "js_text")


def reliance_logs(result, prefix):
    """the history columns of one RelianceMeter.result(): accuracies in percent like the framework's acc"""
    nan = float("nan")
    acc, corr = result["acc"], result["corr"]
    vals = {"corr_image": nan if corr["image"] is None else corr["image"],
            "corr_text": nan if corr["text"] is None else corr["text"],
            "acc_full": 100.0 * acc["full"], "acc_image": 100.0 * acc["image"], "acc_text": 100.0 * acc["text"],
            "acc_image_control": 100.0 * acc["image_control"]["mean"],
            "acc_text_control": 100.0 * acc["text_control"]["mean"],
            "js_image": result["js_image"], "js_text": result["js_text"]}
    return {f"{prefix}_rel_{c}": float(vals[c]) for c in REL_COLUMNS}


def run_reliance(model, loader, device, n_repeats, steps=None, auc_table=None):
    """the robustness pass over `loader` (collate order ((txt, segment, mask, img), y), at most `steps`
    batches) into a fresh RelianceMeter; the caller sets the mode, the seed and no_grad.  auc_table: a
    ranking.AucTable fed the same logits (None: none)"""
    meter = RelianceMeter(n_repeats)
    for i, (x, y) in enumerate(loader):
        if steps is not None and i >= steps:
            break
        txt, segment, mask, img = (t.to(device) for t in x)
        # model(*x) binds mask <- segment, segment <- mask (eval_mmbt_robustness.py)
        lo = robustness_logits(model, txt, segment, mask, img, n_repeats, transpose=False)
        meter.update(lo, y.to(device), layout="VBC")
        if auc_table is not None:
            auc_table.update(lo, y.to(device), layout="VBC")
    return meter


class RelianceCallback(Callback):
    """Modality reliance of the live model at the end of every `every`-th epoch: the robustness pass over
    `loader` under torch.manual_seed(seed) (the same control index sets every epoch), logged as
    {prefix}_rel_* columns; NaN on the epochs it skips.  Place it before the history callbacks.  The
    model's train / eval mode and the torch CPU and device generator states are put back as found, so
    training proceeds as it would without the callback (shown bitwise for one process,
    tests/test_reliance_gpu.py).  Data parallel: every rank runs its own `loader` shard, the meters'
    states are exchanged and merged in rank order.  There train.py averages the BatchNorm running
    statistics over the ranks whenever the model LEAVES training mode (dp.sync_buffers_on_eval); the
    framework calls on_epoch_end after its evaluation loops, with the model already in eval mode, so the
    callback causes no further averaging -- called on a model in training mode it would cause one (on
    every rank alike), which can move those buffers by a rounding when the world size is no power of two.
    auc=True (a binary task, or positive_class against the rest): the same logits also feed a
    ranking.AucTable, logged as {prefix}_rel_auc_{full, image, text, image_control, text_control}
    (control: the mean over the repeats; NaN where a class is missing); off, nothing changes."""

    def __init__(self, model, loader, device, n_repeats=20, every=1, steps=None, seed=0, prefix="val", auc=False,
                 positive_class=1):
        super().__init__()
        if every < 1:
            raise ValueError(f"every = {every} must be at least 1")
        self.rel_model, self.loader, self.device = model, loader, torch.device(device)
        self.n_repeats, self.every, self.steps, self.seed, self.prefix = n_repeats, every, steps, seed, prefix
        self.auc, self.positive_class = bool(auc), positive_class
        self.last_result = None
        self.last_auc = None

    def columns(self):
        cols = [f"{self.prefix}_rel_{c}" for c in REL_COLUMNS]
        if self.auc:
            from .ranking import AUC_LOG_COLUMNS
            cols += [f"{self.prefix}_rel_{c}" for c in AUC_LOG_COLUMNS]
        return cols

    def measure(self):
        """one seeded pass -> the merged meter (auc=True: and self.last_table, the merged AucTable); mode and
        generator states restored"""
        table = None
        if self.auc:
            from .ranking import AucTable
            table = AucTable(self.n_repeats, self.positive_class, self.device)
        model, on_gpu = self.rel_model, self.device.type == "cuda"
        was_training = model.training
        cpu_state = torch.get_rng_state()
        dev_state = torch.cuda.get_rng_state(self.device) if on_gpu else None
        try:
            model.eval()
            torch.manual_seed(self.seed)
            with torch.no_grad():
                if table is None:
                    meter = run_reliance(model, self.loader, self.device, self.n_repeats, self.steps)
                else:
                    meter = run_reliance(model, self.loader, self.device, self.n_repeats, self.steps, auc_table=table)
        finally:
            model.train(was_training)
            torch.set_rng_state(cpu_state)
            if on_gpu:
                torch.cuda.set_rng_state(dev_state, self.device)
        self.last_table = None if table is None else table.gather()
        return gather_meters(meter)

    def on_epoch_end(self, epoch, logs=None):
        logs = {} if logs is None else logs
        if epoch % self.every != 0:
            logs.update({c: float("nan") for c in self.columns()})
            return
        self.last_result = self.measure().result()
        logs.update(reliance_logs(self.last_result, self.prefix))
        if self.auc:
            from .ranking import auc_logs
            self.last_auc = self.last_table.result()
            logs.update(auc_logs(self.last_auc, self.prefix))


def gather_meters(meter):
    """data parallel: every rank's meter state exchanged and merged in rank order, so all ranks hold the
    whole set's meter; a single process gets its own meter back"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return meter
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, meter.state())
    whole = RelianceMeter(meter.n_repeats)
    for st in parts:
        whole.merge(st)
    return whole
