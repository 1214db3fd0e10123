"""Deterministic mode on the whole training step: the small MMBT of test_graph_gpu.py (2 BERT layers,
one Bottleneck per stage, B = 8, T = 16, dropout 0.1 everywhere), forward + backward + fused
BertAdam, 4 optimizer steps.

With kernels.deterministic() on and torch.backends.cudnn.deterministic = True, two fresh models built
from one saved state and run from one host RNG state give the same 4 losses as floats, the same
gradient store after the last backward and the same parameters after the last step, bit for bit:
outside the ResNet trunk (the attention key biases included) and, as a test of its own, on the
trunk's slices.  Two StepGraphs captured under the mode from the same state and seeds replay to equal
losses and parameters (the sort and the scratch of the embedding backward are capture-safe).
Printed for the record, asserted nowhere: eager against replay under the mode, and the mode-off
eager step against itself.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, P = 8, 16, 0.1
STEPS = 4
TRUNK = "enc.img_encoder."


def _model(sd=None):
    from oracle.weights import SMALL, make_state_dict
    from src.mmbt import MultimodalBertClf
    from src.optim import BertAdam
    from src.testing import small_args
    torch.manual_seed(0)
    m = MultimodalBertClf(small_args(bert_hidden_dropout=P, bert_attn_dropout=P, dropout=P))
    m.load_state_dict(sd if sd is not None else make_state_dict(0, SMALL), strict=True)
    m = m.to("cuda:0").train()
    named = list(m.named_parameters())
    nd = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in named if not any(k in n for k in nd)], "weight_decay": 0.01},
              {"params": [p for n, p in named if any(k in n for k in nd)], "weight_decay": 0.0}]
    return m, BertAdam(groups, lr=1e-5, warmup=0.1, t_total=20.0)


def _batch():
    from oracle.weights import SMALL
    from src.testing import synthetic_batch
    x, y = synthetic_batch(B, T, vocab=SMALL.vocab, lens=[16, 9, 16, 12, 5, 16, 14, 16], seed=4)
    return tuple(t.to("cuda:0") for t in x), y.to("cuda:0")


def _state():
    m, _ = _model()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    del m
    return sd


def _eager(sd0, x, y, counter=None):
    """a fresh model from sd0, STEPS optimizer steps from the host RNG state of manual_seed(11) ->
    (losses, gradient store after the last backward, parameters after the last step, slices).
    counter: the dropout seed counter values of a StepGraph's warm-up and replays (None: no counter)"""
    from src import kernels as K
    m, o = _model(sd0)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda:0") if counter else None
    K.set_seed_offset(ctr)
    try:
        torch.manual_seed(11)
        rng = None
        losses = []
        for s in range(STEPS):
            if counter:  # a StepGraph's steps: the warm-up, then every replay from the capture's host seeds
                ctr.fill_(1 + s)
                if s == 1:
                    rng = torch.get_rng_state()
                if s >= 1:
                    torch.set_rng_state(rng)
            o.zero_grad()
            loss = m.compute_loss(m(*x), y)
            loss.backward()
            if s == STEPS - 1:
                torch.cuda.synchronize()
                grad = m.store.grad.clone()
            o.step()
            losses.append(loss.item())
        torch.cuda.synchronize()
    finally:
        K.set_seed_offset(None)
    st = m.store
    slices = {n: (st.offsets[n], st.offsets[n] + st.params[n].numel()) for n in st.names}
    out = (losses, grad, st.flat.clone(), slices)
    del m, o
    torch.cuda.empty_cache()
    return out


def _replayed(sd0, x, y, dev):
    from src.graphs import StepGraph
    m, o = _model(sd0)

    def step():
        o.zero_grad()
        loss = m.compute_loss(m(*x), y)
        loss.backward()
        o.step()
        return loss
    torch.manual_seed(11)
    g = StepGraph(step, dev, warmup=1)
    try:
        losses = [g.replay().item() for _ in range(STEPS - 1)]
        torch.cuda.synchronize()
        flat = m.store.flat.clone()
    finally:
        g.release()
    del g, m, o
    torch.cuda.empty_cache()
    return losses, flat


@pytest.fixture(scope="module")
def runs(dev):
    """the two deterministic eager arms, shared by the tests below (and left unchanged by them)"""
    from src import kernels as K
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        sd0 = _state()
        x, y = _batch()
        with K.deterministic():
            a = _eager(sd0, x, y)
            b = _eager(sd0, x, y)
        yield {"sd0": sd0, "x": x, "y": y, "a": a, "b": b}
    finally:
        torch.backends.cudnn.deterministic = prev


def _differing(a, b, slices, names):
    bad = []
    for n in names:
        lo, hi = slices[n]
        if not torch.equal(a[lo:hi], b[lo:hi]):
            bad.append(f"{n}: max |diff| {(a[lo:hi] - b[lo:hi]).abs().max().item():.3e}")
    return bad


def test_eager_steps_repeat_bit_for_bit(runs):
    (la, ga, fa, sl), (lb, gb, fb, _) = runs["a"], runs["b"]
    print(f"\n[deterministic step] losses {la} / {lb}")
    assert la == lb
    assert len(set(la)) == STEPS and all(l == l for l in la)
    names = [n for n in sl if not n.startswith(TRUNK)]
    assert any(n.endswith("attention.self.key.bias") for n in names)
    assert any("word_embeddings" in n for n in names)
    bad = _differing(ga, gb, sl, names)
    assert not bad, "gradients differ between two runs:\n" + "\n".join(bad)
    bad = _differing(fa, fb, sl, names)
    assert not bad, "parameters differ between two runs:\n" + "\n".join(bad)
    assert ga.abs().sum().item() > 0


def test_eager_steps_repeat_on_the_trunk(runs):
    """the trunk's own kernels hold no atomics; with MIOpen's deterministic algorithms every trunk
    parameter repeats too: nothing is excluded"""
    (_, ga, fa, sl), (_, gb, fb, _) = runs["a"], runs["b"]
    names = [n for n in sl if n.startswith(TRUNK)]
    assert names
    bad = _differing(ga, gb, sl, names) + _differing(fa, fb, sl, names)
    assert not bad, "trunk slices differ between two runs:\n" + "\n".join(bad)


def test_graph_replays_repeat_bit_for_bit(runs, dev):
    from src import kernels as K
    with K.deterministic():
        la, fa = _replayed(runs["sd0"], runs["x"], runs["y"], dev)
        lb, fb = _replayed(runs["sd0"], runs["x"], runs["y"], dev)
        # for the record: the eager steps with the replays' seeds and counter values
        le, _, fe, _ = _eager(runs["sd0"], runs["x"], runs["y"], counter=True)
    assert not K.is_deterministic()
    print(f"\n[deterministic graph] replay losses {la} / {lb}; eager with the same seeds {le[1:]}; "
          f"params replay vs eager: max |diff| {(fa - fe).abs().max().item():.3e} (not asserted)")
    assert la == lb and len(set(la)) == STEPS - 1
    assert torch.equal(fa, fb), f"max |diff| {(fa - fb).abs().max().item():.3e}"


def test_record_mode_off_spread(runs):
    """the default path against itself, printed only: the noise the mode removes"""
    from src import kernels as K
    assert not K.is_deterministic()
    la, ga, fa, _ = _eager(runs["sd0"], runs["x"], runs["y"])
    lb, gb, fb, _ = _eager(runs["sd0"], runs["x"], runs["y"])
    print(f"\n[mode off] losses {la} / {lb}; grad max |diff| {(ga - gb).abs().max().item():.3e}, "
          f"params max |diff| {(fa - fb).abs().max().item():.3e} (not asserted)")
