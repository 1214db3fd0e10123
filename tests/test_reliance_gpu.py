"""The modality-reliance summary end to end on MI355X (small model of src.testing.small_args /
oracle.weights.SMALL; MIOpen pinned to its deterministic solvers, since the tests compare separate runs).

* Meter against the stack: batch 3, T = 20 with lengths [20, 7, 13], n = 4: robustness_logits followed
  by RelianceMeter.update equals the fp64 restatement (test_robustness_summary_gpu.py summary_ref)
  applied to the returned stack within that file's bars; layout="VBC" on the transpose=False tensor
  gives bitwise the same rows; the default return is bitwise what it was.
* Entry point: eval_mmbt_robustness.main, patched to build the small model, on 8 synthetic samples and
  a saved checkpoint: without --summary exactly the two files of before; with it the same two files
  bit for bit, and a JSON and a rows file that agree with a meter run by hand on the written stack.
* Callback: two epochs of Model_.train_loop, dropout 0.1, under kernels.deterministic(True).  The
  callback-free run is repeated first (the training itself is repeatable); with the callback the final
  parameters and the loss history are bitwise those of the callback-free run, the generator states are
  equal before and after on_epoch_end, the model's mode is put back, and the logged columns -- all
  finite on run epochs, Pearson's R included -- equal a RelianceMeter run by a LambdaCallback right
  behind it.  The same two epochs with every=2: NaN in every column for the skipped epoch 1, and for
  epoch 2 what the every=1 run logged.
* train.py: train.main with --reliance_every 2, patched to build the small model: history.csv carries
  the columns (NaN, then finite), run_meta.json the flags.
"""
import json
import os

import numpy as np
import pytest
import torch

from test_robustness_summary_gpu import COLUMNS, same_f32, summary_ref, sweep

pytestmark = pytest.mark.gpu
P = 0.1


@pytest.fixture(scope="module", autouse=True)
def deterministic_convs():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def small_model(dev, wseed=3, **over):
    from oracle.weights import SMALL, make_state_dict
    from src.mmbt import MultimodalBertClf
    from src.testing import small_args
    torch.manual_seed(0)
    model = MultimodalBertClf(small_args(**over))
    model.load_state_dict(make_state_dict(wseed, SMALL), strict=True)
    return model.to(dev)


# ------------------------------------------------------------------------------- meter against the stack
def test_meter_against_the_stack(dev):
    from oracle.weights import SMALL
    from src.robustness import RelianceMeter, robustness_logits
    from src.testing import synthetic_batch
    model = small_model(dev, img_precision="fp32").eval()
    x, y = synthetic_batch(3, 20, vocab=SMALL.vocab, lens=[20, 7, 13], seed=8)
    x = tuple(t.to(dev) for t in x)
    n = 4
    torch.manual_seed(99)
    stack = robustness_logits(model, *x, n_repeats=n)
    torch.manual_seed(99)
    explicit = robustness_logits(model, *x, n_repeats=n, transpose=True)
    torch.manual_seed(99)
    vbc = robustness_logits(model, *x, n_repeats=n, transpose=False)
    assert stack.shape == (3, 3 + 2 * n, 101) and stack.is_contiguous() and vbc.shape == (3 + 2 * n, 3, 101)
    assert torch.equal(stack, explicit)
    assert torch.equal(stack, vbc.transpose(0, 1).contiguous())        # what the function returned before
    y = y.clone()
    y[0] = int(stack[0, 0].argmax())                                   # one sample the full forward gets right
    yd = y.to(dev)

    a = RelianceMeter(n)
    pv = a.update(stack.float(), yd)
    ref = summary_ref(stack.float().cpu().numpy()[:, :, None, :], y.numpy(), np.float64)
    bar = sweep()["bar"]
    ps = a.per_sample()
    print("\ncolumn, bar, error on the small model's stack")
    for c in COLUMNS:
        err = float(np.abs(ps[c] - ref[c]).max())
        print(f"  {c:18s} {bar[c]:.3e} {err:.3e}")
        assert err <= bar[c], f"{c}: {err:.3e} > bar {bar[c]:.3e}"
    for i, c in enumerate(("p_label", "js", "hit")):
        assert np.abs(pv[:, i].double().cpu().numpy() - ref[c]).max() <= bar[c], c
    for c in ("hit_full", "hit_image", "hit_text", "acc_image_control", "acc_text_control"):
        assert same_f32(ps[c], ref[c]), c
    assert np.array_equal(a.hits, ref["hit"].sum(0)) and a.hits[0] >= 1
    assert a.result()["n"] == 3

    b = RelianceMeter(n)
    b.update(vbc.float(), yd, layout="VBC")
    for c in COLUMNS:
        assert np.array_equal(b.per_sample()[c], ps[c]), c
    assert np.array_equal(a.hits, b.hits)
    two = RelianceMeter(n)                                             # and in two updates
    two.update(stack[:2].float(), yd[:2])
    two.update(vbc[:, 2:].float(), yd[2:], layout="VBC")
    for c in COLUMNS:
        assert np.array_equal(two.per_sample()[c], ps[c]), c
    with pytest.raises(ValueError, match="layout"):
        a.update(stack, yd, layout="CBV")
    with pytest.raises(ValueError, match="variants"):
        RelianceMeter(n + 1).update(stack, yd)


# ------------------------------------------------------------------------------- entry point
def test_entry_point_summary(dev, tmp_path, monkeypatch):
    import eval_mmbt_robustness as E
    from src.mmbt import MultimodalBertClf
    from src.robustness import RelianceMeter
    from src.testing import small_args

    def build(args):
        return MultimodalBertClf(small_args(n_classes=args.n_classes, vocab=args.vocab,
                                            vocab_size=args.vocab.vocab_sz,
                                            num_image_embeds=args.num_image_embeds))
    monkeypatch.setattr(E, "MultimodalBertClf", build)
    torch.manual_seed(5)
    from src.testing import _Vocab
    ck = build(type("A", (), dict(n_classes=101, vocab=_Vocab(), num_image_embeds=3)))
    path = str(tmp_path / "small_model.pt")
    torch.save({"model": ck.state_dict()}, path)
    del ck
    n = 2
    common = ["--phase", "val", "--batch_size", "3", "--checkpoint_path", path, "--synthetic", "8",
              "--max_seq_len", "24", "--n_repeats", str(n), "--seed", "13"]
    old_dir, new_dir = str(tmp_path / "old"), str(tmp_path / "new")
    assert E.main(common + ["--save_path", old_dir]) is None
    files = ["robustness_small_model_labels_val.npy", "robustness_small_model_predictions_val.npy"]
    assert sorted(os.listdir(old_dir)) == files
    summary = E.main(common + ["--save_path", new_dir, "--summary"])
    assert sorted(os.listdir(new_dir)) == files + ["robustness_small_model_reliance_val.npy",
                                                  "robustness_small_model_summary_val.json"]
    for f in files:
        assert open(os.path.join(old_dir, f), "rb").read() == open(os.path.join(new_dir, f), "rb").read(), f
    preds = np.load(os.path.join(new_dir, files[1]))
    labels = np.load(os.path.join(new_dir, files[0]))
    assert preds.shape == (8, 3 + 2 * n, 101) and preds.dtype == np.float32 and labels.shape == (8,)
    written = json.load(open(os.path.join(new_dir, "robustness_small_model_summary_val.json")))
    assert written == json.loads(json.dumps(summary))
    assert (written["n"], written["n_repeats"], written["seed"]) == (8, n, 13)
    assert written["columns"] == list(COLUMNS)
    by_hand = RelianceMeter(n)
    by_hand.update(torch.from_numpy(preds).to(dev), torch.from_numpy(labels).to(dev))
    want = json.loads(json.dumps(by_hand.result()))
    assert {k: written[k] for k in want} == want
    rows = np.load(os.path.join(new_dir, "robustness_small_model_reliance_val.npy"))
    assert rows.shape == (8, len(COLUMNS)) and rows.dtype == np.float64
    assert np.array_equal(rows, np.stack([by_hand.per_sample()[c] for c in COLUMNS], axis=1))


# ------------------------------------------------------------------------------- callback
def _train_setup(dev, sd0=None):
    from oracle.weights import SMALL, make_state_dict
    from src.framework import Model_
    from src.mmbt import MultimodalBertClf
    from src.optim import BertAdam
    from src.testing import small_args
    torch.manual_seed(0)
    model = MultimodalBertClf(small_args(bert_hidden_dropout=P, bert_attn_dropout=P, dropout=P))
    model.load_state_dict(sd0 if sd0 is not None else make_state_dict(0, SMALL), strict=True)
    model = model.to(dev)
    named = list(model.named_parameters())
    nd = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in named if not any(k in n for k in nd)], "weight_decay": 0.01},
              {"params": [p for n, p in named if any(k in n for k in nd)], "weight_decay": 0.0}]
    opt = BertAdam(groups, lr=1e-5, warmup=0.1, t_total=8.0)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "max", patience=2, factor=0.5)

    def acc(y_pred, y_true, eval, dummy_dim=False):
        return (y_pred.max(1)[1] == y_true).float().mean() * 100
    m = Model_(model=model, optimizer=opt, scheduler=sched, data_forming_func=lambda x, y, phase="train": (x, y),
               metrics=[acc], verbose=False)
    m.to(dev)
    return model, m


def _batches(n, B, T, seed):
    from oracle.weights import SMALL
    from src.testing import synthetic_batch
    lens = [T, max(3, T // 2), T - 3, T][:B]
    return [synthetic_batch(B, T, vocab=SMALL.vocab, lens=lens, seed=seed + i) for i in range(n)]


def _train(dev, make_callbacks, epochs=2):
    """a fresh model, `epochs` epochs of 2 steps from the host RNG state of manual_seed(11) ->
    (flat parameters, [logs per epoch], model)"""
    from src.callbacks import LambdaCallback
    model, m = _train_setup(dev)
    train, val = _batches(2, 4, 16, seed=40), _batches(1, 4, 16, seed=50)
    history = []
    cbs = make_callbacks(model) + [LambdaCallback(on_epoch_end=lambda e, logs: history.append(dict(logs)))]
    torch.manual_seed(11)
    m.train_loop(train, valid_generator=val, test_generator=val, steps_per_epoch=2, validation_steps=1, test_steps=1,
                 epochs=epochs, callbacks=cbs, patience=10, epoch_start=1, scheduler_step_on="epoch", auc=False,
                 vilt=False, mmbt=True, freeze_img=0, freeze_txt=0, gradient_accumulation_steps=1,
                 scheduler_metric="val_acc")
    torch.cuda.synchronize()
    return model.store.flat.clone(), history, model


def test_callback_leaves_training_as_it_was(dev):
    from src import kernels as K
    from src.callbacks import LambdaCallback
    from src.robustness import RelianceCallback, RelianceMeter, reliance_logs, robustness_logits
    n, seed = 2, 5
    rel_loader = _batches(2, 3, 12, seed=60)
    by_hand = []

    def hand(model, every=1):
        """the same pass spelled out: what the callback must have logged for this (run) epoch"""
        def on_epoch_end(epoch, logs):
            if epoch % every:
                return
            cpu, gpu, mode = torch.get_rng_state(), torch.cuda.get_rng_state(dev), model.training
            model.eval()
            torch.manual_seed(seed)
            meter = RelianceMeter(n)
            with torch.no_grad():
                for (txt, segment, mask, img), y in rel_loader:
                    lo = robustness_logits(model, txt.to(dev), segment.to(dev), mask.to(dev), img.to(dev), n)
                    meter.update(lo.float(), y.to(dev))
            by_hand.append(reliance_logs(meter.result(), "val"))
            model.train(mode)
            torch.set_rng_state(cpu)
            torch.cuda.set_rng_state(gpu, dev)
        return LambdaCallback(on_epoch_end=on_epoch_end)

    with K.deterministic(True):
        flat_a, hist_a, _ = _train(dev, lambda model: [])
        flat_b, hist_b, _ = _train(dev, lambda model: [])
        assert torch.equal(flat_a, flat_b), "the callback-free training is not repeatable"
        assert [h["loss"] for h in hist_a] == [h["loss"] for h in hist_b]
        flat_c, hist_c, model = _train(
            dev, lambda model: [RelianceCallback(model, rel_loader, dev, n_repeats=n, every=1, seed=seed),
                                hand(model)])
        assert torch.equal(flat_a, flat_c), "the callback changed the parameters"
        assert [h["loss"] for h in hist_a] == [h["loss"] for h in hist_c]
        assert [h["val_loss"] for h in hist_a] == [h["val_loss"] for h in hist_c]
        assert len(hist_c) == 2 and not any(k.startswith("val_rel_") for k in hist_a[0])
        cb = RelianceCallback(model, rel_loader, dev, n_repeats=n, every=1, seed=seed)
        cols = cb.columns()
        assert len(by_hand) == 2
        for h, mine in zip(hist_c, by_hand):
            assert [k for k in h if k.startswith("val_rel_")] == cols
            print({c: h[c] for c in cols})
            assert all(np.isfinite(h[c]) for c in cols), h            # Pearson's R included
            assert {c: h[c] for c in cols} == mine                    # exactly
            assert -1.0 <= h["val_rel_corr_image"] <= 1.0 and -1.0 <= h["val_rel_corr_text"] <= 1.0
            assert 0.0 <= h["val_rel_acc_full"] <= 100.0 and h["val_rel_js_image"] > 0.0
        assert hist_c[0]["val_rel_js_text"] != hist_c[1]["val_rel_js_text"], "the model did not move"
        assert hist_c[0]["val_rel_corr_text"] != hist_c[1]["val_rel_corr_text"]
        last = by_hand[-1]

        # every=2 through the framework: epoch 1 is skipped and logs NaN in every column, epoch 2 runs and
        # logs what the every=1 run logged for it (the same model, the same seed)
        del by_hand[:]
        flat_d, hist_d, model = _train(
            dev, lambda model: [RelianceCallback(model, rel_loader, dev, n_repeats=n, every=2, seed=seed),
                                hand(model, every=2)])
        assert torch.equal(flat_a, flat_d) and [h["loss"] for h in hist_a] == [h["loss"] for h in hist_d]
        assert [[k for k in h if k.startswith("val_rel_")] for h in hist_d] == [cols, cols]
        assert all(np.isnan(hist_d[0][c]) for c in cols)
        assert all(np.isfinite(hist_d[1][c]) for c in cols)
        assert by_hand == [last] and {c: hist_d[1][c] for c in cols} == last

        # the states it must put back, on direct calls in either mode: generators and mode
        for mode in (True, False):
            model.train(mode)
            torch.manual_seed(77)
            cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
            run = {}
            cb.rel_model = model
            cb.on_epoch_end(3, run)
            assert torch.equal(cpu, torch.get_rng_state()) and torch.equal(gpu, torch.cuda.get_rng_state(dev))
            assert model.training is mode
            assert list(run) == cols and run == last
        limited = {}
        RelianceCallback(model, rel_loader, dev, n_repeats=n, steps=1, seed=seed).on_epoch_end(1, limited)
        assert limited["val_rel_js_image"] != run["val_rel_js_image"]                        # one batch of the two


# ------------------------------------------------------------------------------- train.py
def test_train_main_with_reliance_every(dev, tmp_path, monkeypatch):
    """train.main on 8 synthetic samples, patched to build the small model and to write no checkpoints:
    --reliance_every 2 puts the callback ahead of the history callbacks, so history.csv carries the
    val_rel_* columns -- NaN for the skipped epoch 1, finite (both correlations included) for epoch 2 --
    and run_meta.json records the flags"""
    import pandas as pd
    import src.callbacks
    import src.mmbt
    import src.training_loop
    import train as T
    from src import kernels as K
    from src.robustness import REL_COLUMNS
    from src.testing import small_args
    real = src.mmbt.MultimodalBertClf

    def build(args):
        return real(small_args(n_classes=args.n_classes, vocab=args.vocab, vocab_size=args.vocab.vocab_sz,
                               num_image_embeds=args.num_image_embeds, dropout=args.dropout))
    monkeypatch.setattr(src.mmbt, "MultimodalBertClf", build)
    for mod in (src.training_loop, src.callbacks):
        monkeypatch.setattr(mod, "save_weights", lambda *a, **k: None)
    was = K.is_deterministic()
    try:
        T.main(["--save_path", str(tmp_path), "--framework", "mmbt", "--dataset", "food101", "--synthetic", "8",
                "--batch_size", "4", "--max_seq_len", "24", "--n_epochs", "2", "--gradient_accumulation_steps", "1",
                "--lr", "1e-5", "--use_gpu", "--reliance_every", "2", "--reliance_repeats", "2"])
    finally:
        K.set_deterministic(was)
    meta = json.load(open(os.path.join(str(tmp_path), "run_meta.json")))
    assert (meta["reliance_every"], meta["reliance_repeats"], meta["reliance_steps"]) == (2, 2, None)
    H = pd.read_csv(os.path.join(str(tmp_path), "history.csv"))
    cols = ["val_rel_" + c for c in REL_COLUMNS]
    assert [c for c in H.columns if "_rel_" in c] == cols and list(H["epoch"]) == [1, 2]
    print(H[cols].to_string())
    assert H[cols].iloc[0].isna().all(), "the skipped epoch must log NaN"
    assert np.isfinite(H[cols].iloc[1].to_numpy(dtype=np.float64)).all()
    assert list(H.columns).index(cols[0]) > list(H.columns).index("val_acc")    # appended, nothing displaced
