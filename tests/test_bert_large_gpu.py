"""MMBT on bert-large-uncased shapes (1024 hidden, 16 x 64 heads, 4096 intermediate) through the HIP
path, against the CPU oracle (oracle/mmbt_ref.py, itself held to transformers' BertEncoder at this
width by tests/test_bert_large_host.py) on seeded weights: state-dict keys, eval logits of the four
forwards, one train step's loss and gradients, the [CLS]-only last layer against the dense one,
deterministic mode, the batched ensemble, and the full depth of 24 layers.

WIDE_SMALL keeps the layer shapes of bert-large and cuts depth, vocabulary and the ResNet (2 layers,
4096 words, one Bottleneck per stage), as oracle.weights.SMALL does for bert-base.  Bars are the
project's at 768: test_mmbt_gpu.py's tol_check (max err <= 1e-2 x max|ref|) and the fp32-trunk arm
of its train-step test; test_last_layer_cls_gpu.py's _compare.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle.weights import MMBTConfig

pytestmark = pytest.mark.gpu

WIDE_SMALL = MMBTConfig(n_layers=2, hidden=1024, heads=16, inter=4096, vocab=4096, resnet_blocks=(1, 1, 1, 1))
WIDE_DEEP = dataclasses.replace(WIDE_SMALL, n_layers=24)
B, T, LENS = 2, 16, (16, 9)
REL = 1e-2
CHAOS_LOGIT_X = 2.0  # test_mmbt_gpu.py: the factor a HIP result may stand above a bf16 comparator's error


def tol_check(got, ref, rel=REL, what=""):
    """test_mmbt_gpu.py's: max |err| <= rel x max|ref|; returns the error as a share of the scale"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"[bert-large] {what}: max err {err:.3e} on scale {scale:.3e} ({err / scale:.2e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"
    return err / scale


def build(dev, sd, **over):
    from src.mmbt import MultimodalBertClf
    from src.testing import small_args
    over.setdefault("img_precision", "fp32")
    torch.manual_seed(0)
    m = MultimodalBertClf(small_args(bert_model="bert-large-uncased", hidden_sz=1024, **over))
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def sd0():
    from oracle.weights import make_state_dict
    return make_state_dict(0, WIDE_SMALL)


@pytest.fixture(scope="module")
def batch():
    from src.testing import synthetic_batch
    return synthetic_batch(B, T, vocab=WIDE_SMALL.vocab, lens=list(LENS), seed=3)


def on(dev, x):
    return tuple(t.to(dev) for t in x)


def test_state_dict_keys_are_the_reference_s(dev, sd0):
    from oracle.weights import key_shapes
    m = build(dev, sd0)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {}
    for key, shape, _, alias in key_shapes(WIDE_SMALL):
        want[key] = tuple(shape) if alias is None else want[alias]
    assert list(got) and set(got) == set(want), sorted(set(got) ^ set(want))
    assert got == want, [(k, got[k], want[k]) for k in got if got[k] != want[k]]
    assert got["enc.encoder.layer.1.intermediate.dense.weight"] == (4096, 1024)
    assert [(lw.hid, lw.ffn, lw.heads) for lw in m.enc._lw] == [(1024, 4096, 16)] * 2


def test_eval_forwards_match_the_oracle(dev, sd0, batch):
    from oracle import mmbt_ref as R
    (txt, seg, mask, img), _ = batch
    m = build(dev, sd0).eval()
    x = on(dev, (txt, mask, seg, img))
    n_img = WIDE_SMALL.num_image_embeds
    idx = R.control_indices(T + n_img + 2, n_img + 1, torch.Generator().manual_seed(5))
    with torch.no_grad():
        feats = R.image_encoder(sd0, img, WIDE_SMALL)
        tol_check(m(*x).cpu(), R.forward(sd0, txt, mask, seg, img, WIDE_SMALL, feats=feats), what="forward")
        tol_check(m.forward_img_only(*x).cpu(), R.forward(sd0, txt, mask, seg, img, WIDE_SMALL, "img_only", feats=feats),
                  what="forward_img_only")
        tol_check(m.forward_txt_only(*x).cpu(), R.forward(sd0, txt, mask, seg, img, WIDE_SMALL, "txt_only", feats=feats),
                  what="forward_txt_only")
        tol_check(m.clf(m.enc._variant(*x, idx)).cpu(),
                  R.forward(sd0, txt, mask, seg, img, WIDE_SMALL, "control", indices=idx, feats=feats),
                  what="forward_control (one index set)")


def _oracle_step(sd, x, y, cfg):
    """forward(train=True) + cross entropy + autograd backward on copies of the state dict (aliases
    kept) -> loss, {key: grad}"""
    from oracle import mmbt_ref as R
    txt, seg, mask, img = x
    copies, g = {}, {}
    for k, v in sd.items():
        if id(v) not in copies:
            c = v.clone()
            if c.is_floating_point() and "running_" not in k:
                c.requires_grad_(True)
            copies[id(v)] = c
        g[k] = copies[id(v)]
    loss = R.cross_entropy(R.forward(g, txt, mask, seg, img, cfg, train=True), y)
    loss.backward()
    return loss.item(), {k: v.grad for k, v in g.items() if v.requires_grad}


def test_train_step_matches_the_oracle(dev, sd0, batch):
    """the bars of test_train_step_grads_match_reference_golden's fp32-trunk arm: loss within 1e-2
    (relative); every parameter's gradient norm within 1e-2 above the floor 1e-4 x max norm;
    clf.weight.grad elementwise at 1e-2"""
    (txt, seg, mask, img), y = batch
    ref_loss, ref = _oracle_step(sd0, (txt, seg, mask, img), y, WIDE_SMALL)
    m = build(dev, sd0, bert_hidden_dropout=0.0, bert_attn_dropout=0.0).train()
    m.store.zero_grad()
    loss = m.compute_loss(m(*on(dev, (txt, mask, seg, img))), y.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    lerr = abs(loss.item() - ref_loss) / abs(ref_loss)
    named = dict(m.named_parameters())
    assert set(named) <= set(ref)
    want = {n: ref[n].double().norm().item() for n in named}
    floor = 1e-4 * max(want.values())
    rows, bad = [], []
    for n, p in named.items():
        got = p.grad.double().norm().item()
        e = abs(got - want[n]) / max(want[n], 1e-30)
        if want[n] > floor:
            rows.append((e, n))
        if not abs(got - want[n]) <= REL * want[n] + floor:
            bad.append((n, got, want[n], e))
    rows.sort(reverse=True)
    print(f"[bert-large train step] loss {loss.item():.6f} vs {ref_loss:.6f} (rel {lerr:.2e}); grad-norm rel err over "
          f"{len(rows)} tensors above the floor: max {rows[0][0]:.2e} ({rows[0][1]}), median {rows[len(rows) // 2][0]:.2e}")
    assert lerr < REL
    assert not bad, f"{len(bad)} of {len(named)} grad norms off: worst {sorted(bad, key=lambda r: -r[3])[:5]}"
    tol_check(named["clf.weight"].grad.cpu(), ref["clf.weight"], what="clf.weight.grad")


# ------------------------------------------------------------------ the [CLS]-only last layer
def _arm(sd, cls_on, monkeypatch, grad=True):
    """test_last_layer_cls_gpu.py's _arm on the wide model: one seeded step of a fresh model
    (dropouts 0.1) -> logits, loss, {name: grad}, the gradient reaching the embeddings.  Its patches
    are undone when it returns, so the arms of one test do not wrap one another's tap."""
    with monkeypatch.context() as mp:
        return _arm_patched(sd, cls_on, mp, grad)


def _arm_patched(sd, cls_on, monkeypatch, grad):
    from src import encoder, mmbt
    from src.testing import synthetic_batch
    import test_last_layer_cls_gpu as C
    m = build("cuda:0", sd, img_precision="bf16", bert_hidden_dropout=C.P3, bert_attn_dropout=C.P3, dropout=C.P3).train()
    x, y = synthetic_batch(C.B3, C.T3, vocab=WIDE_SMALL.vocab, lens=[65, 40, 9], seed=4)
    x, y = on("cuda:0", x), y.to("cuda:0")
    emb_grad = []
    stack = mmbt.encoder_stack

    def tapped(lws, X, *a, **kw):
        if X.requires_grad:
            X.register_hook(lambda gX: emb_grad.append(gX.detach().float().clone()))
        return stack(lws, X, *a, **kw)

    monkeypatch.setattr(encoder, "LAST_LAYER_CLS", cls_on)
    monkeypatch.setattr(mmbt, "encoder_stack", tapped)
    # (fixed convolution algorithms, as there: two runs of one arm otherwise differ in the logits)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.manual_seed(11)  # the host-drawn dropout seeds
    if not grad:
        with torch.no_grad():
            return m(*x).float().cpu(), None, {}, None
    m.store.zero_grad()
    logits = m(*x)
    loss = m.compute_loss(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: prm.grad.detach().float().cpu().clone() for n, prm in m.named_parameters() if prm.grad is not None}
    return logits.detach().float().cpu(), loss.item(), grads, emb_grad[0].cpu()


def test_last_layer_cls_equals_dense_at_1024(dev, sd0, monkeypatch):
    import test_last_layer_cls_gpu as C
    C._compare("bert-large train", _arm(sd0, True, monkeypatch), _arm(sd0, False, monkeypatch))
    C._compare("bert-large no_grad", _arm(sd0, True, monkeypatch, grad=False), _arm(sd0, False, monkeypatch, grad=False))


# ------------------------------------------------------------------ deterministic mode
def test_deterministic_steps_repeat_bit_for_bit(dev, sd0, batch, monkeypatch):
    from src import kernels as K
    (txt, seg, mask, img), y = batch
    x, y = on(dev, (txt, mask, seg, img)), y.to(dev)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    runs = []
    with K.deterministic():
        for _ in range(2):
            m = build(dev, sd0, img_precision="bf16", bert_hidden_dropout=0.1, bert_attn_dropout=0.1, dropout=0.1).train()
            torch.manual_seed(11)
            m.store.zero_grad()
            loss = m.compute_loss(m(*x), y)
            loss.backward()
            torch.cuda.synchronize()
            runs.append((loss.item(), m.store.grad.clone()))
            del m
    assert not K.is_deterministic()
    (la, ga), (lb, gb) = runs
    print(f"[bert-large deterministic] losses {la} / {lb}; grad |sum| {ga.abs().sum().item():.4e}")
    assert la == lb and la == la
    assert ga.abs().sum().item() > 0
    assert torch.equal(ga, gb), f"gradients differ between two runs: max |diff| {(ga - gb).abs().max().item():.3e}"


# ------------------------------------------------------------------ ensemble
def test_ensemble_members_match_their_own_forward(dev, batch):
    from oracle.weights import make_state_dict
    from src.uncertainty import EnsembleMMBT
    (txt, seg, mask, img), _ = batch
    x = on(dev, (txt, mask, seg, img))
    ms = [build(dev, make_state_dict(k, WIDE_SMALL)).eval() for k in range(2)]
    ens = EnsembleMMBT(ms)
    assert (ens.hid, ens.ffn, ens.heads) == (1024, 4096, 16)
    with torch.no_grad():
        lo = ens.logits(*x, mc_samples=1)
        assert lo.shape == (2, 1, B, 101)
        for k, m in enumerate(ms):
            tol_check(lo[k, 0].cpu(), m(*x).cpu(), what=f"ensemble member {k} vs its own forward")


# ------------------------------------------------------------------ depth
def _bf16_operand_encoder(sd, txt, mask, seg, img, cfg, feats):
    """the oracle's forward with every linear's input and weight rounded to bf16 (f32 accumulation,
    f32 residual stream and LayerNorms): what bf16 GEMM operands alone cost at this depth"""
    from oracle import mmbt_ref as R
    rb = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    lin = R._lin
    R._lin = lambda sd_, p, x: (rb(x) @ rb(sd_[p + "weight"]).t() + sd_[p + "bias"]) if p.startswith(R.ENC) else lin(sd_, p, x)
    try:
        return R.forward(sd, txt, mask, seg, img, cfg, feats=feats)
    finally:
        R._lin = lin


def test_24_layers_match_the_oracle(dev, sd0, batch):
    """bert-large's own depth (dropping the bert_layers override gives the table's 24) on the other
    wide-small settings.  Bar: the project's 1e-2 x max|logit|; if 24 layers of bf16 operands alone
    exceed it, <= CHAOS_LOGIT_X x the error of the oracle with bf16-rounded linear operands."""
    from oracle import mmbt_ref as R
    from oracle.weights import make_state_dict
    from src.mmbt import _bert_shape
    from src.testing import make_args
    assert _bert_shape(make_args(bert_model="bert-large-uncased", hidden_sz=1024))[0] == 24
    (txt, seg, mask, img), _ = batch
    x = on(dev, (txt, mask, seg, img))
    with torch.no_grad():
        ref2 = R.forward(sd0, txt, mask, seg, img, WIDE_SMALL)
        got2 = build(dev, sd0).eval()(*x).cpu()
        e2 = (got2 - ref2).abs().max().item() / ref2.abs().max().item()
        sd = make_state_dict(0, WIDE_DEEP)
        feats = R.image_encoder(sd, img, WIDE_DEEP)
        ref = R.forward(sd, txt, mask, seg, img, WIDE_DEEP, feats=feats)
        m = build(dev, sd, bert_layers=24).eval()
        assert len(m.enc.encoder.layer) == 24
        got = m(*x).cpu()
        scale = ref.abs().max().item()
        e24 = (got - ref).abs().max().item() / scale
        print(f"[bert-large depth] logits max err / max|ref|: 24 layers {e24:.3e}, 2 layers {e2:.3e}")
        if e24 <= REL:
            return
        emu = _bf16_operand_encoder(sd, txt, mask, seg, img, WIDE_DEEP, feats)
        e_emu = (emu - ref).abs().max().item() / scale
        print(f"[bert-large depth] the oracle with bf16 linear operands: {e_emu:.3e}; HIP / emulation {e24 / e_emu:.2f}")
        assert e24 <= CHAOS_LOGIT_X * e_emu, f"24 layers: {e24:.3e} of scale vs the bf16-operand emulation's {e_emu:.3e}"
