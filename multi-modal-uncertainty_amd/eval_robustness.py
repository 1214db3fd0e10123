#!/usr/bin/env python3
"""Robustness / uncertainty evaluation entry point (reference eval_robustness.py CLI, :20-34).

MMBT mode (the build's uncertainty pass, BASELINE config 3):
  --mmbt --checkpoint_paths ck1.pt ... ckK.pt [--mc_samples 30] --phase val
runs the K-member deep ensemble x T-pass MC-dropout as one batched encoder launch
per op (src/uncertainty.py) and writes
  <save_path>/uncertainty_<phase>_logits.npy   [S, K, T, n_classes]
  <save_path>/uncertainty_<phase>_labels.npy   [S]
  <save_path>/uncertainty_<phase>_metrics.json {nll, ece, acc, n, K, T}
With --decompose and / or --variants full img_only txt_only control_image control_text (any
subset) the metrics gain "decomposition" (the full forward's entropy / mutual-information split,
Brier score, vote disagreement, per-member NLL, ensemble gain and error-detection AUROCs:
src/uncertainty.py UncertaintyMeter(decompose=True)) and "variants" (the same, with nll / ece / acc,
per requested variant; every variant but full is a logits call of its own on the same batch and
also writes <save_path>/uncertainty_<phase>_<variant>_logits.npy).
With --decompose --selective the metrics, and every "variants" entry, gain "selective": for the same
four scores as the AUROCs (total, mi, one_minus_conf, vote_disagreement) {auroc, aurc, eaurc} -- the area
under the risk-coverage curve when samples are accepted by ascending score, and its excess over the
ideal order -- plus n and error_rate, formed from one exact rank table per meter (src/ranking.py).
With --calibrate {shared,per_member} [--calibrate_phase val] the ensemble first runs over the
calibration phase and its temperature(s) are fitted on the device (src/calibration.py); --temperature
FILE applies a saved fit instead.  Either way --phase then runs as above, a second decomposition meter
reads the same logits under the fitted temperatures, the metrics gain "calibrated" (and, with
"variants", "variants_calibrated": every variant under the full forward's temperature) and
  <save_path>/uncertainty_<phase>_calibration.json {mode, tau, nll_before, nll_after, passes, rounds,
      at_bound, fit_phase, eval_phase, same_split, before, after}
is written (before / after: nll, ece, brier, acc, total, mi); the file is itself a valid --temperature.
With --diversity [--diversity_top 5] [--diversity_keep_true] (at least 2 members) the logits already
computed also feed a src/diversity.py DiversityMeter, for the full forward and for every --variants entry:
per pair of members the Jensen-Shannon divergence, the disagreement rate, Kendall's tau-b of the top
probabilities with the true class muted (--diversity_keep_true: not muted), the double-fault rate, Yule's
Q and the phi correlation of the members' errors.  The metrics gain "diversity" (and, with other variants,
"variants_diversity") and
  <save_path>/uncertainty_<phase>_diversity.json {diversity[, variants_diversity]}
is written.  --diversity_from LOGITS.npy LABELS.npy runs the meter alone on a saved [S, K, T, C] logits
file and its labels (the files above) and writes that JSON; no model is built.
Without --mmbt: the reference's FashionMNIST MIMO robustness pass (eval_robustness.py:42-121,
BASELINE config 1's model family): each of the 4 quarter-crop views zeroed in turn (the
weight-sharing model sees the other 3), predictions [4, S, heads, 10] and labels written as
<checkpoint>_predictions_robustness.npy / <checkpoint>_labels.npy.  --data_dir / --sample_size
/ --synthetic_images as in train_fashionmnist.py (without image files the run fails unless
--synthetic_images is given).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

FLAGS = [
    ("--checkpoint_path", dict(type=str, default=None, help="Path to load the model")),
    ("--model_type", dict(type=str, default="Vanilla",
                          choices=["Vanilla", "MIMO-shuffle-instance", "MIMO-shuffle-view", "MultiHead",
                                   "MIMO-shuffle-all", "single-model-weight-sharing"])),
    ("--use_gpu", dict(action="store_true")), ("--device", dict(default=0, type=int)),
    ("--save_path", dict(type=str, required=True, help="Path to save the model")),
    ("--seed", dict(type=int, default=42)), ("--verbose", dict(action="store_true")),
    ("--batch_size", dict(type=int, default=64)), ("--transformer", dict(action="store_true")),
    ("--multimodal_num_attention_heads", dict(type=int, default=3)),
    ("--multimodal_num_hidden_layers", dict(type=int, default=3)), ("--dropout", dict(type=float, default=0)),
    # MMBT uncertainty mode
    ("--mmbt", dict(action="store_true")), ("--checkpoint_paths", dict(nargs="*", default=[])),
    ("--mc_samples", dict(type=int, default=1)), ("--n_bins", dict(type=int, default=15)),
    ("--phase", dict(type=str, default="val")), ("--synthetic", dict(type=int, default=0)),
    ("--datapath", dict(type=str, default=None)), ("--max_seq_len", dict(type=int, default=512)),
    ("--num_image_embeds", dict(type=int, default=3)), ("--n_workers", dict(type=int, default=0)),
    ("--bert_model", dict(type=str, default="bert-base-uncased")),
    ("--hidden_sz", dict(type=int, default=768, help="BERT hidden size: 768, or 1024 with bert-large-uncased")),
    ("--gin_file", dict(nargs="*", default=[])), ("--gin_param", dict(nargs="*", default=[])),
    ("--data_dir", dict(type=str, default=None)), ("--sample_size", dict(type=int, default=None)),
    ("--synthetic_images", dict(action="store_true")),
    # MMBT uncertainty mode: the entropy / mutual-information split, per modality variant
    ("--decompose", dict(action="store_true")),
    ("--variants", dict(nargs="+", default=["full"],
                        choices=["full", "img_only", "txt_only", "control_image", "control_text"])),
    # MMBT uncertainty mode: pairwise member agreement (src/diversity.py)
    ("--diversity", dict(action="store_true")),
    ("--diversity_top", dict(type=int, default=5, help="probabilities each member keeps for Kendall's tau (0: all)")),
    ("--diversity_keep_true", dict(action="store_true", help="do not mute the true class")),
    # MMBT uncertainty mode, with --decompose: what each uncertainty score is worth for selective prediction
    ("--selective", dict(action="store_true", help="with --decompose: AUROC, risk-coverage area (AURC) and its "
                                                   "excess over the ideal order for total / mi / 1 - conf / "
                                                   "vote_disagreement (src/ranking.py)")),
    ("--diversity_from", dict(nargs=2, default=None, metavar=("LOGITS.npy", "LABELS.npy"),
                              help="only the diversity meter, on a saved [S, K, T, C] logits file and its labels")),
    # MMBT uncertainty mode: temperature scaling (src/calibration.py)
    ("--calibrate", dict(type=str, default=None, choices=["shared", "per_member"],
                         help="fit the ensemble's temperature(s) on --calibrate_phase and report --phase under them")),
    ("--calibrate_phase", dict(type=str, default="val")),
    ("--temperature", dict(type=str, default=None, help="apply a saved fit (a calibration JSON) instead of fitting")),
]

# --variants name -> EnsembleMMBT.logits(variant=...)
VARIANTS = {"img_only": "img_only", "txt_only": "txt_only", "control_image": ("control", "image"),
            "control_text": ("control", "text")}


def get_args(parser):
    for flag, kw in FLAGS:
        parser.add_argument(flag, **kw)


def mmbt_model_args(args, n_classes, vocab):
    """the namespace MultimodalBertClf is built from: the reference's defaults with this run's flags"""
    from src.testing import make_args
    return make_args(n_classes=n_classes, vocab=vocab, num_image_embeds=args.num_image_embeds,
                     bert_model=args.bert_model, hidden_sz=args.hidden_sz)


# what uncertainty_<phase>_calibration.json compares before and after temperature scaling
CALIBRATION_KEYS = ("nll", "ece", "brier", "acc", "total", "mi")


def check_calibration_flags(args):
    if args.calibrate and args.temperature:
        raise ValueError("--calibrate fits a temperature and --temperature applies a saved one: give one of them")


def fit_temperature_on(args, ens, loader, dev):
    """--calibrate: the ensemble over ``loader``, its logits kept on the device, and the fit.  The torch
    generator states are put back afterwards, so the evaluation pass that follows draws the dropout
    seeds (and a shuffling loader's order) of a run without the flag."""
    from src.calibration import TemperatureScaler
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    scaler = TemperatureScaler(args.calibrate)
    try:
        with torch.no_grad():
            for x, y in loader:
                txt, segment, mask, img = (t.to(dev) for t in x)
                scaler.add(ens.logits(txt, segment, mask, img, mc_samples=args.mc_samples), y.to(dev))
        scaler.fit()
    finally:
        scaler.clear()
        torch.set_rng_state(cpu_state)
        torch.cuda.set_rng_state(dev_state, dev)
    return scaler


def write_diversity(args, blocks):
    from src.robustness import json_safe
    os.makedirs(args.save_path, exist_ok=True)
    with open(os.path.join(args.save_path, f"uncertainty_{args.phase}_diversity.json"), "w") as f:
        json.dump(json_safe(blocks), f, indent=1, allow_nan=False)


def run_diversity_from(args):
    """--diversity_from: the meter alone on saved logits and labels"""
    from src.diversity import diversity_from_files
    if not torch.cuda.is_available():
        raise RuntimeError("the diversity pass runs on MI355X HIP kernels: no GPU visible")
    dev = torch.device("cuda:{}".format(args.device))
    meter = diversity_from_files(args.diversity_from[0], args.diversity_from[1], dev, args.diversity_top,
                                 not args.diversity_keep_true)
    blocks = {"diversity": meter.result()}
    write_diversity(args, blocks)
    print(json.dumps(blocks))
    return blocks


def run_mmbt(args):
    from src import gin
    from src.mmbt import MultimodalBertClf
    from src.training_loop import _load_pretrained_model
    from src.uncertainty import EnsembleMMBT, UncertaintyMeter
    from src.utils import set_seed
    from eval_mmbt_robustness import load_data
    check_calibration_flags(args)
    if args.selective and not args.decompose:
        raise SystemExit("--selective ranks the columns of the decomposition: pass --decompose")
    if args.diversity:   # refused before the data is read and any model is built
        from src.diversity import DiversityMeter, check_diversity_flags
        check_diversity_flags(max(1, len(args.checkpoint_paths or [])), args.diversity_top)
    set_seed(args.seed)
    args.drop_img_percent = 0.0
    data, n_classes, vocab = load_data(args)
    paths = args.checkpoint_paths or ([args.checkpoint_path] if args.checkpoint_path else [])
    if not torch.cuda.is_available():
        raise RuntimeError("the MMBT uncertainty pass runs on MI355X HIP kernels: no GPU visible")
    dev = torch.device("cuda:{}".format(args.device))
    members = []
    for i, p in enumerate(paths or [None]):
        margs = mmbt_model_args(args, n_classes, vocab)
        torch.manual_seed(args.seed + i)
        m = MultimodalBertClf(margs)
        if p:
            _load_pretrained_model(m, p)
        members.append(m.to(dev))
    ens = EnsembleMMBT(members)
    # --decompose / --variants: the full forward's meter takes the [K, T, B, C] logits in place, and
    # every other variant is a logits call of its own on the same batch with a meter of its own
    decompose = args.decompose or list(args.variants) != ["full"]
    extra = [v for v in dict.fromkeys(args.variants) if v != "full"]
    meter = UncertaintyMeter(args.n_bins, decompose=decompose)
    vmeters = {v: UncertaintyMeter(args.n_bins, decompose=True) for v in extra}
    # --calibrate / --temperature: a second decompose meter reads the same logits under the fitted
    # temperatures (the ensemble is not run again), and one more per variant, under the full forward's
    scaler, fit_phase = None, None
    if args.temperature:
        from src.calibration import TemperatureScaler
        scaler = TemperatureScaler.load(args.temperature)
        fit_phase = scaler.extra.get("fit_phase")      # a calibration JSON names it, a bare save() file does not
    elif args.calibrate:
        scaler, fit_phase = fit_temperature_on(args, ens, data[args.calibrate_phase], dev), args.calibrate_phase
    if scaler is not None:
        if len(scaler.result["tau"]) != len(members):
            raise ValueError(f"the temperature fit holds {len(scaler.result['tau'])} members, the ensemble "
                             f"{len(members)}")
        same_split = None if fit_phase is None else fit_phase == args.phase
        if fit_phase is None:
            print(f"NOTE: {args.temperature} does not say which split it was fitted on: whether that was "
                  f"{args.phase} is not known")
        if same_split:
            print(f"WARNING: the temperature was fitted on the split it is evaluated on ({args.phase}): the "
                  "calibrated figures are optimistic")
        inv_temp = scaler.inv_temp(dev)
        before = meter if decompose else UncertaintyMeter(args.n_bins, decompose=True)
        after = UncertaintyMeter(args.n_bins, decompose=True, inv_temp=inv_temp)
        vafter = {v: UncertaintyMeter(args.n_bins, decompose=True, inv_temp=inv_temp) for v in extra}
    # --diversity: one more meter per forward, fed from the logits already computed
    dmeters = {}
    if args.diversity:
        dmeters = {v: DiversityMeter(args.diversity_top, not args.diversity_keep_true)
                   for v in dict.fromkeys(["full"] + extra)}
    all_logits, labels, vlogits = [], [], {v: [] for v in extra}
    with torch.no_grad():
        for x, y in data[args.phase]:
            txt, segment, mask, img = (t.to(dev) for t in x)
            lo = ens.logits(txt, segment, mask, img, mc_samples=args.mc_samples)   # [K, T, B, C]
            if scaler is not None:
                if before is not meter:
                    before.update(lo, y.to(dev))
                after.update(lo, y.to(dev))
            if decompose:
                meter.update(lo, y.to(dev))
            else:
                flat = lo.permute(2, 0, 1, 3).reshape(lo.shape[2], -1, lo.shape[3])  # [B, K*T, C]
                meter.update(flat, y.to(dev))
            if dmeters:
                dmeters["full"].update(lo, y.to(dev))
            all_logits.append(lo.permute(2, 0, 1, 3).cpu())
            labels.append(y)
            for v in extra:
                lv = ens.logits(txt, segment, mask, img, mc_samples=args.mc_samples, variant=VARIANTS[v])
                vmeters[v].update(lv, y.to(dev))
                if scaler is not None:
                    vafter[v].update(lv, y.to(dev))
                if dmeters:
                    dmeters[v].update(lv, y.to(dev))
                vlogits[v].append(lv.permute(2, 0, 1, 3).cpu())
    full = meter.result()
    res = dict({k: full[k] for k in ("nll", "ece", "acc", "n")}, K=len(members), T=args.mc_samples)
    if args.selective:   # one rank_table launch per meter over its four score columns
        from src.ranking import selective_of_meter
        res["selective"] = selective_of_meter(meter, dev)
        full = dict(full, selective=res["selective"])
    if decompose:
        res["decomposition"] = {k: v for k, v in full.items() if k not in ("nll", "ece", "acc", "n", "selective")}
        res["variants"] = {v: full if v == "full" else vmeters[v].result() for v in dict.fromkeys(args.variants)}
        if args.selective:
            for v in extra:
                res["variants"][v]["selective"] = selective_of_meter(vmeters[v], dev)
    os.makedirs(args.save_path, exist_ok=True)
    if dmeters:
        from src.robustness import json_safe
        blocks = {"diversity": json_safe(dmeters["full"].result())}
        if extra:
            blocks["variants_diversity"] = {v: blocks["diversity"] if v == "full" else json_safe(dmeters[v].result())
                                            for v in dict.fromkeys(args.variants)}
        res.update(blocks)
        write_diversity(args, blocks)
    if scaler is not None:
        cal_full = after.result()
        cal = dict(scaler.result, fit_phase=fit_phase, eval_phase=args.phase, same_split=same_split,
                   before={k: before.result()[k] for k in CALIBRATION_KEYS},
                   after={k: cal_full[k] for k in CALIBRATION_KEYS})
        res["calibrated"] = cal["after"]
        if decompose:
            res["variants_calibrated"] = {v: cal_full if v == "full" else vafter[v].result()
                                          for v in dict.fromkeys(args.variants)}
        with open(os.path.join(args.save_path, f"uncertainty_{args.phase}_calibration.json"), "w") as f:
            json.dump(cal, f, indent=1, allow_nan=False)
    np.save(os.path.join(args.save_path, f"uncertainty_{args.phase}_logits.npy"), torch.cat(all_logits).numpy())
    for v in extra:   # (the full forward's logits are the file above)
        np.save(os.path.join(args.save_path, f"uncertainty_{args.phase}_{v}_logits.npy"),
                torch.cat(vlogits[v]).numpy())
    np.save(os.path.join(args.save_path, f"uncertainty_{args.phase}_labels.npy"), torch.cat(labels).numpy())
    with open(os.path.join(args.save_path, f"uncertainty_{args.phase}_metrics.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return res


def run_fmnist(args):
    """eval_robustness.py:42-121: view i zeroed (or dropped for the weight-sharing model) for
    i = 0..3 over the test loader, in the reference's loop order."""
    from src import dataset
    from src.training_loop import _load_pretrained_model
    from train_fashionmnist import build_model
    if args.checkpoint_path is None:
        raise ValueError("--checkpoint_path is required without --mmbt")
    model = build_model(args)
    _, valid, _ = dataset.get_fmnist(datapath=args.data_dir, batch_size=args.batch_size, download=True,
                                     shuffle=True, sample_size=args.sample_size, seed=args.seed,
                                     synthetic_images=args.synthetic_images)
    if getattr(valid.dataset, "synthetic", False):
        print("WARNING: FashionMNIST images are SYNTHETIC (seeded noise, real labels)")
    print("Loading Checkpoint from {}".format(args.checkpoint_path))
    _load_pretrained_model(model, args.checkpoint_path)
    dev = torch.device("cuda:{}".format(args.device)) if args.use_gpu and torch.cuda.is_available() \
        else torch.device("cpu")
    model.to(dev).eval()
    outputs, labels, m = [], [], 4
    with torch.no_grad():
        for i in range(m):
            y_hat = []
            for x, y in valid:
                if args.model_type != "single-model-weight-sharing":
                    x, y = dataset.data_forming_func(x, y, "eval", model_type=args.model_type)
                    x_ = x.to(dev).clone()
                    x_[:, i] = 0  # view i zeroed, the others kept
                    y_ = model(x_)
                else:
                    b, mm, c, h, w = x.shape
                    keep = [j for j in range(mm) if j != i]
                    x_, y = dataset.data_forming_func(x[:, keep].contiguous(), y, "eval", model_type=args.model_type)
                    y_ = model(x_.to(dev)).view(b, mm - 1, -1)
                y_hat.append(y_.float().cpu().numpy())
                if i == 0:
                    labels.append(y.cpu().numpy())
            outputs.append(np.concatenate(y_hat, axis=0))
    outputs = np.stack(outputs, axis=0)
    M_, S, M, C = outputs.shape
    print("Gathered predictions of {} samples, {} views, {} dups, {} classes".format(S, M_, M, C))
    labels = np.concatenate(labels, axis=0)
    os.makedirs(args.save_path, exist_ok=True)
    name = args.checkpoint_path.split("/")[-1].split(".")[0]
    np.save(os.path.join(args.save_path, f"{name}_predictions_robustness.npy"), outputs)
    np.save(os.path.join(args.save_path, f"{name}_labels.npy"), labels)
    return outputs, labels


def main(argv=None):
    parser = argparse.ArgumentParser(description="Train Models")
    get_args(parser)
    args, remaining = parser.parse_known_args(argv)
    assert remaining == [], remaining
    from src import gin
    gin.load(args, args.gin_file, args.gin_param)
    if args.diversity_from:
        return run_diversity_from(args)
    return run_mmbt(args) if args.mmbt else run_fmnist(args)


if __name__ == "__main__":
    main()
