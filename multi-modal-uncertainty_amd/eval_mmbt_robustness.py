#!/usr/bin/env python3
"""Modality-robustness predictions of an MMBT checkpoint -- the reference
eval_mmbt_robustness.py command line and output files (:20-44, :94-110) on the
batched MI355X pass (src/robustness.py: image trunk once per batch, the 43
encoder passes grouped into 3 launches by sequence length).

Writes robustness_<ckpt>_predictions_<phase>.npy  [S, 3 + 2*n_repeats, n_classes]
       robustness_<ckpt>_labels_<phase>.npy       [S]
--summary additionally writes (and prints) the modality-reliance analysis of those predictions
(src/robustness.py RelianceMeter on the kernels.robustness_summary rows):
       robustness_<ckpt>_summary_<phase>.json     RelianceMeter.result() + n_repeats, seed, columns
       robustness_<ckpt>_reliance_<phase>.npy     [S, len(columns)] fp64, the per-sample rows
--auc_table [--positive_class 1] additionally writes the reference's AUC table (notebooks/
hatefulmeme_robustness.py AUC_table; src/ranking.py AucTable on the kernels.rank_table counts), with or
without --summary, whose files do not change:
       robustness_<ckpt>_auc_<phase>.json         AucTable.result() + n_repeats, seed, positive_class
--auc_from LABELS.npy PRED.npy [PRED.npy ...] builds no model and reads no dataset: the AUC table of the
first saved [S, 3 + 2n, (K,) C] prediction stack (the reference's [S, 43, K, C] files included) and, with
several, the "ensemble" block (each file's full-variant AUC, and the AUC table of the files' mean
probabilities: the reference's ensemble_overtime).  Only --save_path, --device and --positive_class are
read beside it:
       <first PRED's name>_auc_from.json
"""
import argparse
import json
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src import dataset  # noqa: E402
from src.mmbt import MultimodalBertClf  # noqa: E402
from src.robustness import RelianceMeter, json_safe, robustness_logits  # noqa: E402
from src.training_loop import _load_pretrained_model  # noqa: E402
from src.utils import set_seed, torch_to  # noqa: E402

logger = logging.getLogger(__name__)

FLAGS = [
    ("--save_path", dict(type=str, required=True, help="Path to save the model")),
    ("--phase", dict(type=str, required=True)), ("--batch_size", dict(type=int, required=True)),
    ("--checkpoint_path", dict(type=str, required=True, help="Path to load the model")),
    ("--use_gpu", dict(action="store_true")), ("--device", dict(default=0, type=int)),
    ("--seed", dict(type=int, default=42)), ("--verbose", dict(action="store_true")),
    ("--n_repeats", dict(type=int, default=20, help="Number of times to repeat the random sampling")),
    ("--dataset", dict(type=str, choices=["food101", "hateful-meme-dataset"], default="hateful-meme-dataset")),
    ("--num_image_embeds", dict(type=int, default=3)), ("--drop_img_percent", dict(type=float, default=0.0)),
    ("--dropout", dict(type=float, default=0.1)), ("--datapath", dict(type=str)),
    ("--bert_model", dict(type=str, default="bert-base-uncased", choices=["bert-base-uncased", "bert-large-uncased"])),
    ("--max_seq_len", dict(type=int, default=512)), ("--n_workers", dict(type=int, default=0)),
    ("--hidden", dict(nargs="*", type=int, default=[])), ("--hidden_sz", dict(type=int, default=768)),
    ("--img_embed_pool_type", dict(type=str, default="avg", choices=["max", "avg"])),
    ("--img_hidden_sz", dict(type=int, default=2048)), ("--include_bn", dict(type=int, default=True)),
    ("--synthetic", dict(type=int, default=0, help="N synthetic samples instead of the dataset")),
    ("--summary", dict(action="store_true", help="also write the modality-reliance summary (JSON) and its "
                                                 "per-sample rows")),
    ("--auc_table", dict(action="store_true", help="also write the AUC of the positive class's probability under "
                                                   "every variant (JSON)")),
    ("--positive_class", dict(type=int, default=1, help="the class whose probability --auc_table / --auc_from rank")),
]
AUC_FROM = ("--auc_from", dict(nargs="+", default=None, metavar="NPY",
                               help="LABELS.npy PRED.npy [PRED.npy ...]: the AUC table of saved prediction stacks, "
                                    "no model and no dataset"))


def get_args(parser):
    for flag, kw in FLAGS:
        parser.add_argument(flag, **kw)


def load_data(args):
    if args.synthetic:
        from src.testing import _Vocab
        T = args.max_seq_len - args.num_image_embeds - 1
        ds = dataset.SyntheticFood101(args.synthetic, max_text=T, min_text=T // 2, seed=2)
        ld = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=False,
                                         num_workers=args.n_workers, collate_fn=dataset.collate_fn)
        return {"train": ld, "val": ld, "test": ld}, 101, _Vocab()
    tr, va, te, n_classes, vocab = dataset.get_food101(datapath=args.datapath, batch_size=args.batch_size,
                                                       drop_img_percent=args.drop_img_percent,
                                                       max_seq_len=args.max_seq_len,
                                                       num_image_embeds=args.num_image_embeds,
                                                       n_workers=args.n_workers)
    return {"train": tr, "val": va, "test": te}, n_classes, vocab


def write_json(path, obj):
    # strict JSON: an undefined figure (an AUC without both classes, a correlation of a constant column) is null
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, allow_nan=False)


def run_auc_from(argv):
    """--auc_from: the AUC table (and ensemble block) of saved prediction stacks"""
    from src.ranking import auc_from_files
    parser = argparse.ArgumentParser(description="AUC table of saved robustness predictions")
    parser.add_argument(AUC_FROM[0], **AUC_FROM[1])
    parser.add_argument("--save_path", type=str, required=True)
    parser.add_argument("--device", default=0, type=int)
    parser.add_argument("--positive_class", type=int, default=1)
    args, _ = parser.parse_known_args(argv)
    if len(args.auc_from) < 2:
        raise SystemExit("--auc_from takes LABELS.npy and at least one PRED.npy")
    if not torch.cuda.is_available():
        raise RuntimeError("the AUC table runs on MI355X HIP kernels: no GPU visible")
    out = json_safe(auc_from_files(args.auc_from[0], args.auc_from[1:], args.positive_class,
                                   torch.device("cuda:{}".format(args.device))))
    name = os.path.basename(args.auc_from[1]).rsplit(".", 1)[0]
    os.makedirs(args.save_path, exist_ok=True)
    write_json(os.path.join(args.save_path, f"{name}_auc_from.json"), out)
    print(json.dumps(out, allow_nan=False))
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if any(a == AUC_FROM[0] or a.startswith(AUC_FROM[0] + "=") for a in argv):
        return run_auc_from(argv)
    parser = argparse.ArgumentParser(description="Eval Models")
    get_args(parser)
    parser.add_argument(AUC_FROM[0], **AUC_FROM[1])   # (for --help; handled above)
    args, remaining = parser.parse_known_args(argv)
    assert remaining == [], remaining
    set_seed(args.seed)
    data, args.n_classes, args.vocab = load_data(args)
    model = MultimodalBertClf(args)
    _load_pretrained_model(model, args.checkpoint_path)
    if not torch.cuda.is_available():
        raise RuntimeError("the MMBT robustness pass runs on MI355X HIP kernels: no GPU visible")
    dev = torch.device("cuda:{}".format(args.device))
    model.to(dev)
    model.eval()
    preds, labels = [], []
    meter = RelianceMeter(args.n_repeats) if args.summary else None
    table = None
    if args.auc_table:
        from src.ranking import AucTable
        if not 0 <= args.positive_class < args.n_classes:
            raise SystemExit(f"--positive_class {args.positive_class} is outside the {args.n_classes} classes")
        table = AucTable(args.n_repeats, args.positive_class, dev)
    with torch.no_grad():
        for x, y in data[args.phase]:
            x, y = torch_to(x, dev), torch_to(y, dev)
            txt, segment, mask, img = x  # collate order; model(*x) binds mask<-segment, segment<-mask
            lo = robustness_logits(model, txt, segment, mask, img, args.n_repeats).float()
            if meter is not None:
                meter.update(lo, y)
            if table is not None:
                table.update(lo, y)
            preds.append(lo.cpu())
            labels.append(y.cpu())
    preds = torch.cat(preds).numpy()
    labels = torch.cat(labels).numpy()
    name = args.checkpoint_path.split("/")[-1].split(".")[0]
    os.makedirs(args.save_path, exist_ok=True)
    np.save(os.path.join(args.save_path, f"robustness_{name}_predictions_{args.phase}.npy"), preds)
    np.save(os.path.join(args.save_path, f"robustness_{name}_labels_{args.phase}.npy"), labels)
    S, M, C = preds.shape
    print("Gathered predictions of {} samples, {} variants, {} classes".format(S, M, C))
    print("Gathered labels of {} samples".format(len(labels)))
    auc = None
    if table is not None:
        auc = json_safe(dict(table.result(), n_repeats=args.n_repeats, seed=args.seed,
                             positive_class=args.positive_class))
        write_json(os.path.join(args.save_path, f"robustness_{name}_auc_{args.phase}.json"), auc)
        print(json.dumps(auc, allow_nan=False))
    if meter is not None:
        # strict JSON: an undefined figure (a correlation of a constant column, a mean over no samples) is null
        summary = json_safe(dict(meter.result(), n_repeats=args.n_repeats, seed=args.seed,
                                 columns=list(meter.columns)))
        with open(os.path.join(args.save_path, f"robustness_{name}_summary_{args.phase}.json"), "w") as f:
            json.dump(summary, f, indent=1, allow_nan=False)
        rows = meter.per_sample()
        np.save(os.path.join(args.save_path, f"robustness_{name}_reliance_{args.phase}.npy"),
                np.stack([rows[c] for c in meter.columns], axis=1))
        print(json.dumps(summary, allow_nan=False))
        return summary
    return auc


if __name__ == "__main__":
    main()
