"""K-member deep ensemble x T-pass MC-dropout evaluation of MMBT, NLL and ECE.

North-star feature (absent from the reference code).
The K members share the architecture but not the weights; their encoder layers
run as ONE batched launch per op: every GEMM is batched over members (weight
stride = one member's matrix), attention is weight-free so all K*T*B sequences
go in one launch, and LayerNorm uses member-strided affine params
(mmu_layernorm_fwd group_rows).  MC-dropout replicates each batch T times inside
a member; dropout masks differ per row because the dropout counters include the
row index.  ResNet-152 (MIOpen) and the token embedding run per member.

Metrics (mmu_uncertainty / mmu_ece_bins):
  p_bar = mean over the K*T rows of softmax(logits)    (notebooks/food101_robustness.py:25-36)
  NLL   = -mean log p_bar[y]      (== reference CrossEntropyLoss at K = T = 1, src/mmbt.py:243)
  ECE   = sum_b (n_b/N) |acc_b - conf_b| over 15 equal-width bins of max p_bar (build-defined)
UncertaintyMeter(decompose=True) (mmu_uncertainty_decompose, the [K, T, B, C] logits read in place):
  total = H[p_bar], aleatoric = mean_kt H[p_kt], mi_members = H[p_bar] - mean_k H[p_k],
  mi_passes = mean_k H[p_k] - aleatoric, Brier, vote disagreement, per-member NLL, and the AUROC of
  the uncertainty scores as detectors of the misclassified samples
UncertaintyMeter(decompose=True, inv_temp=beta) reports the same table for softmax(beta_k z_kt): the
  ensemble under the temperatures src/calibration.py fits (mmu_uncertainty_decompose_scaled)
EnsembleMMBT.logits(variant=...) runs the same pass on the img-only / txt-only / control gathers.
"""
import numpy as np
import torch

from . import kernels as K
from .mmbt import LN_EPS, _mix, _seed, control_indices

bf16 = torch.bfloat16


class EnsembleMMBT:
    """Stacked view of K MultimodalBertClf members (all on one device, eval mode)."""

    KEYS = ("wqkv16", "bqkv", "wo16", "bo", "ln1w", "ln1b", "w116", "b1", "w216", "b2", "ln2w", "ln2b")

    def __init__(self, members):
        self.members = list(members)
        self.K = len(self.members)
        for m in self.members:
            m.eval()
            m.enc._prepare()
        lws = self.members[0].enc._lw
        n_layers = len(lws)
        self.hid, self.ffn, self.heads = lws[0].hid, lws[0].ffn, lws[0].heads  # (one architecture)
        if any((lw.hid, lw.ffn, lw.heads) != (self.hid, self.ffn, self.heads) for m in self.members for lw in m.enc._lw):
            raise ValueError("EnsembleMMBT: the members must share one BERT shape")
        self.layers = []
        for i in range(n_layers):
            self.layers.append({k: torch.stack([getattr(m.enc._lw[i], k) for m in self.members]).contiguous()
                                for k in self.KEYS})
        enc0 = self.members[0].enc
        self.pool_w = torch.stack([m.enc.pooler.dense.weight.detach() for m in self.members])
        self.pool_b = torch.stack([m.enc.pooler.dense.bias.detach() for m in self.members])
        self.clf_w = torch.stack([m.clf.weight.detach() for m in self.members])
        self.clf_b = torch.stack([m.clf.bias.detach() for m in self.members])
        self.hidden_dropout, self.attn_dropout = enc0.hidden_dropout, enc0.attn_dropout

    def _layer(self, lw, X, R, km, nb, L, p_attn, p_hid, seeds, res_ln=None, out32=False):
        """X bf16 [K*M, H] + its f32 residual -> (Y, S2, mean2, rstd2, Y32): src/encoder.py
        layer_forward batched over the members (the same f32 hidden stream: R is the embeddings'
        f32 rows, or the previous layer's S2 whose LayerNorm the epilogue recomputes from
        res_ln = (mean, rstd, gamma [K, H], beta [K, H]))."""
        HID, FFN, HEADS = self.hid, self.ffn, self.heads
        Km, M = self.K, nb * L
        dev = X.device
        f32 = torch.float32
        qkv = torch.empty(Km * M, 3 * HID, dtype=bf16, device=dev)
        K.gemm(X, HID, True, lw["wqkv16"], HID, True, qkv, 3 * HID, M, 3 * HID, HID, batch=Km, sA=M * HID,
               sB=3 * HID * HID, sC=M * 3 * HID, epi=K.epilogue(K.EPI_STORE, bias=lw["bqkv"], bias_bstride=3 * HID))
        O = torch.empty(Km * M, HID, dtype=bf16, device=dev)
        lse = torch.empty(Km * nb * HEADS, L, dtype=torch.float32, device=dev)
        K.attention_fwd(qkv, km, O, lse, Km * nb, L, HEADS, p_attn, seeds[0])
        S1 = torch.empty(Km * M, HID, dtype=f32, device=dev)
        K.gemm(O, HID, True, lw["wo16"], HID, True, S1, HID, M, HID, HID, batch=Km, sA=M * HID, sB=HID * HID,
               sC=M * HID, epi=K.epilogue(K.EPI_BIAS_DROP_RES, bias=lw["bo"], bias_bstride=HID, residual=R,
                                          res_bstride=M * HID, drop_p=p_hid, seed=seeds[1], res_ln=res_ln,
                                          res_ln_bstride=HID))
        del R
        A = torch.empty_like(O)
        mean1 = torch.empty(Km * M, dtype=f32, device=dev)
        rstd1 = torch.empty_like(mean1)
        K.layernorm_fwd_f32(S1, lw["ln1w"], lw["ln1b"], A, None, mean1, rstd1, eps=LN_EPS, group_rows=M,
                            param_stride=HID)
        Hh = torch.empty(Km * M, FFN, dtype=bf16, device=dev)
        K.gemm(A, HID, True, lw["w116"], HID, True, Hh, FFN, M, FFN, HID, batch=Km, sA=M * HID, sB=FFN * HID,
               sC=M * FFN, epi=K.epilogue(K.EPI_BIAS_GELU, bias=lw["b1"], bias_bstride=FFN))
        del A
        S2 = torch.empty(Km * M, HID, dtype=f32, device=dev)
        K.gemm(Hh, FFN, True, lw["w216"], FFN, True, S2, HID, M, HID, FFN, batch=Km, sA=M * FFN, sB=HID * FFN,
               sC=M * HID, epi=K.epilogue(K.EPI_BIAS_DROP_RES, bias=lw["b2"], bias_bstride=HID, residual=S1,
                                          res_bstride=M * HID, drop_p=p_hid, seed=seeds[2],
                                          res_ln=(mean1, rstd1, lw["ln1w"], lw["ln1b"]), res_ln_bstride=HID))
        del S1, Hh
        Y = torch.empty_like(O)
        Y32 = torch.empty_like(S2) if out32 else None
        mean2 = torch.empty(Km * M, dtype=f32, device=dev)
        rstd2 = torch.empty_like(mean2)
        K.layernorm_fwd_f32(S2, lw["ln2w"], lw["ln2b"], Y, Y32, mean2, rstd2, eps=LN_EPS, group_rows=M,
                            param_stride=HID)
        return Y, S2, mean2, rstd2, Y32

    VARIANTS = ("img_only", "txt_only", ("control", "image"), ("control", "text"))

    def variant_indices(self, variant, Tt):
        """the gather of MultimodalBertEncoder.forward_img_only / forward_txt_only / forward_control
        over the n_img + 2 + Tt embedding rows; a control draw comes from the global torch RNG"""
        n_img = self.members[0].enc.n_img
        if variant == "img_only":
            return torch.arange(n_img + 2)
        if variant == "txt_only":
            return torch.cat([torch.zeros(1, dtype=torch.long), torch.arange(Tt) + n_img + 2])
        if variant == ("control", "image"):
            return control_indices(n_img + 2 + Tt, n_img + 1)
        if variant == ("control", "text"):
            return control_indices(n_img + 2 + Tt, Tt)
        raise ValueError(f"EnsembleMMBT.logits: variant must be None or one of {self.VARIANTS}, got {variant!r}")

    @torch.no_grad()
    def logits(self, txt, mask, segment, img, mc_samples=1, mc_dropout=None, variant=None):
        """-> [K, T, B, n_classes] f32.  mc_dropout defaults to mc_samples > 1.
        variant: None (the full forward), "img_only", "txt_only", ("control", "image") or
        ("control", "text"): every member and pass runs on that gather of the embedding rows
        (src/mmbt.py forward_img_only / forward_txt_only / forward_control).  A control draw is made
        once per call, before anything else touches the torch RNG, and shared by all members and
        passes: under one seed it is the draw of a member's own forward_control."""
        vidx = None if variant is None else self.variant_indices(variant, txt.shape[1])
        mc = (mc_samples > 1) if mc_dropout is None else mc_dropout
        T_mc = int(mc_samples)
        B, Tt = txt.shape
        enc0 = self.members[0].enc
        S = enc0.n_img + 2 + Tt if vidx is None else vidx.numel()
        nb = T_mc * B
        M = nb * S
        dev = img.device
        HID = self.hid
        X = torch.empty(self.K * M, HID, dtype=bf16, device=dev)
        X32 = torch.empty(self.K * M, HID, dtype=torch.float32, device=dev)
        km = torch.empty(self.K * nb, S, dtype=torch.float32, device=dev)
        p_txt = self.hidden_dropout if mc else 0.0
        # T_mc copies of the identity gather, or of the variant's
        idx = (torch.arange(S, device=dev) if vidx is None else vidx.to(dev)).repeat(T_mc, 1)
        txt, segment, mask = (t.contiguous().long() for t in (txt, segment, mask))
        for k, m in enumerate(self.members):
            e = m.enc
            proj = e.img_embeddings.project(e._image_feats(img)).contiguous()
            et = e.txt_embeddings
            K.embed_fwd(txt, segment, mask, proj, et.word_embeddings.weight, et.position_embeddings.weight,
                        et.token_type_embeddings.weight, et.LayerNorm.weight, et.LayerNorm.bias, LN_EPS, e.cls_id,
                        e.sep_id, idx, T_mc, B, Tt, e.n_img, S, X[k * M:(k + 1) * M], km[k * nb:(k + 1) * nb],
                        drop_txt=p_txt, drop_img=0.0, seed=_seed() if mc else 0, X32=X32[k * M:(k + 1) * M])
        p_attn, p_hid = (self.attn_dropout, self.hidden_dropout) if mc else (0.0, 0.0)
        base = _seed() if mc else 0
        R, rln, n = X32, None, len(self.layers)
        del X32
        for i, lw in enumerate(self.layers):
            X, R, mu, rs, Y32 = self._layer(lw, X, R, km, nb, S, p_attn, p_hid,
                                            (_mix(base, 3 * i), _mix(base, 3 * i + 1), _mix(base, 3 * i + 2)),
                                            rln, out32=i == n - 1)
            rln = (mu, rs, lw["ln2w"], lw["ln2b"])
        h0 = Y32.view(self.K, nb, S, HID)[:, :, 0]                             # [K, nb, H] f32
        pooled = torch.tanh(torch.baddbmm(self.pool_b.unsqueeze(1), h0, self.pool_w.transpose(1, 2)))
        out = torch.baddbmm(self.clf_b.unsqueeze(1), pooled, self.clf_w.transpose(1, 2))
        return out.view(self.K, T_mc, B, -1)


def auroc(score, positive):
    """Area under the ROC curve of ``score`` detecting the ``positive`` samples: the rank statistic
    (sum of the positives' ranks - n_pos (n_pos + 1) / 2) / (n_pos n_neg) with average ranks on ties,
    in fp64.  None when the samples are all positive or all negative."""
    score = np.asarray(score, dtype=np.float64).reshape(-1)
    pos = np.asarray(positive).reshape(-1).astype(bool)
    n_pos = int(pos.sum())
    n_neg = pos.size - n_pos
    if n_pos == 0 or n_neg == 0:
        return None
    _, inv, cnt = np.unique(score, return_inverse=True, return_counts=True)
    last = np.cumsum(cnt).astype(np.float64)          # the highest 1-based rank of each tie group
    ranks = (last - (cnt - 1) / 2.0)[inv]
    return float((ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * float(n_neg)))


class UncertaintyMeter:
    """Accumulates NLL / ECE bins / accuracy over batches with the HIP reduction kernels.
    decompose=True: the entropy / mutual-information split of mmu_uncertainty_decompose as well
    (per-sample statistics kept on the host; see result()).
    inv_temp (decompose=True only): f32 [K] device tensor of inverse temperatures, e.g.
    calibration.TemperatureScaler.inv_temp(device); member k's logits are multiplied by inv_temp[k]
    before everything else (mmu_uncertainty_decompose_scaled).  None: the unscaled symbol, as before."""

    def __init__(self, n_bins=15, decompose=False, inv_temp=None):
        if inv_temp is not None and not decompose:
            raise ValueError("UncertaintyMeter: inv_temp needs decompose=True")
        self.n_bins = n_bins
        self.decompose = decompose
        self.inv_temp = inv_temp
        self.bins = None
        self.nll_sum = 0.0
        self.correct = 0.0
        self.count = 0
        self.stats, self.member_nll = [], []   # decompose: per batch [S, UNC_NSTAT] / [S, K] fp64

    def update(self, logits, y, layout="KTBC"):
        """logits [S, R, C] (R = members x passes), y [S].
        decompose=True: logits [K, T, B, C] as EnsembleMMBT.logits returns them (layout "KTBC", read in
        place through their strides) or [S, K, T, C] (layout "SKTC")."""
        if self.decompose:
            return self._update_decompose(logits, y, layout)
        S, R, C = logits.shape
        dev = logits.device
        p_bar = torch.empty(S, C, dtype=torch.float32, device=dev)
        nll, conf, cor = (torch.empty(S, dtype=torch.float32, device=dev) for _ in range(3))
        K.uncertainty(logits.float().contiguous(), y.long().contiguous(), p_bar, nll, conf, cor)
        self._bin(conf, cor)
        self.nll_sum += float(nll.double().sum())
        self.correct += float(cor.double().sum())
        self.count += S
        return p_bar

    def _bin(self, conf, cor):
        bins = torch.empty(3 * self.n_bins, dtype=torch.float32, device=conf.device)
        K.ece_bins(conf, cor, self.n_bins, bins)
        b = bins.double().cpu().numpy()
        self.bins = b if self.bins is None else self.bins + b

    def _update_decompose(self, logits, y, layout):
        if layout not in ("KTBC", "SKTC") or logits.dim() != 4:
            raise ValueError("UncertaintyMeter(decompose=True).update: logits [K, T, B, C] (layout 'KTBC') or "
                             f"[S, K, T, C] (layout 'SKTC'), got {tuple(logits.shape)} with layout {layout!r}")
        lo = logits.float()                                  # (f32 already: no copy)
        lo = lo.permute(2, 0, 1, 3) if layout == "KTBC" else lo   # a view: the kernel takes the strides
        S, Km, _, C = lo.shape
        dev = lo.device
        stats = torch.empty(S, K.UNC_NSTAT, dtype=torch.float32, device=dev)
        p_bar = torch.empty(S, C, dtype=torch.float32, device=dev)
        mnll = torch.empty(S, Km, dtype=torch.float32, device=dev)
        if self.inv_temp is None:
            K.uncertainty_decompose(lo, y.long().contiguous(), stats, p_bar, mnll)
        else:
            K.uncertainty_decompose(lo, y.long().contiguous(), stats, p_bar, mnll, inv_temp=self.inv_temp)
        col = K.UNC_COLUMNS.index
        nll, cor = stats[:, col("nll")], stats[:, col("correct")]
        self._bin(stats[:, col("conf")].contiguous(), cor.contiguous())
        self.nll_sum += float(nll.double().sum())
        self.correct += float(cor.double().sum())
        self.count += S
        self.stats.append(stats.double().cpu().numpy())
        self.member_nll.append(mnll.double().cpu().numpy())
        return p_bar

    def per_sample(self):
        """decompose=True: the per-sample statistics seen so far, {column or "mi": fp64 [n]}"""
        st = np.concatenate(self.stats)
        out = {name: st[:, i] for i, name in enumerate(K.UNC_COLUMNS)}
        out["mi"] = out["mi_members"] + out["mi_passes"]
        return out

    def result(self):
        """-> {nll, ece, acc, n}; decompose=True adds the mean of every statistic column ("nll" is that
        mean already), "mi" = mi_members + mi_passes, "member_nll" (mean per member), "ensemble_gain" =
        mean member NLL - ensemble NLL, and "auroc": how well total / mi / 1 - conf / vote_disagreement
        rank the misclassified samples first (None when all samples are correct or all are wrong)."""
        bb = self.bins.reshape(self.n_bins, 3)
        ece = float(np.abs(bb[:, 2] - bb[:, 1]).sum() / max(self.count, 1))
        res = {"nll": self.nll_sum / max(self.count, 1), "ece": ece, "acc": self.correct / max(self.count, 1),
               "n": self.count}
        if not self.decompose:
            return res
        ps = self.per_sample()
        for name in K.UNC_COLUMNS + ("mi",):
            if name not in ("nll", "correct"):       # today's "nll" and "acc"
                res[name] = float(ps[name].mean())
        member = np.concatenate(self.member_nll).mean(axis=0)
        res["member_nll"] = [float(v) for v in member]
        res["ensemble_gain"] = float(member.mean()) - res["nll"]
        wrong = ps["correct"] == 0
        res["auroc"] = {name: auroc(score, wrong) for name, score in
                        (("total", ps["total"]), ("mi", ps["mi"]), ("one_minus_conf", 1.0 - ps["conf"]),
                         ("vote_disagreement", ps["vote_disagreement"]))}
        return res
