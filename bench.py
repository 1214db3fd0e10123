"""MMBT (BERT-base + ResNet-152) training throughput on MI355X -- the BASELINE.json metric.

One step = one optimizer step of the reference train loop over a synthetic Food-101
batch (src/framework.py:276-319 with accum = 1, freeze epochs over, every one of the
169.3 M parameters trainable): ResNet-152 + 12 fused BERT layers forward, CE loss,
backward, (N>1: RCCL gradient all-reduce), fused BertAdam.  The global batch is the metric's
bs = 256 (224x224 image, 508 word-pieces -> 513 tokens), split evenly over the N ranks
(BASELINE config 4 / SURVEY §8d: "bs=256 global, 32 per GPU at 8 GPUs"): total work is fixed
as N grows, "scaling": "strong".  --per-rank-batch B (without --global-batch) keeps B samples
per rank instead ("scaling": "weak"; DESIGN.md §6 has both).

  python bench.py [--gpus N] [--steps K] [--warmup W]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N
  python bench.py --workload flava     BASELINE config 5: the FLAVA fusion transformer
                                       (src/model.py) train step on synthetic embeddings
  python bench.py --workload uncertainty   BASELINE config 3: 5-member deep ensemble x
                                       MC-dropout T=30 evaluation (NLL / ECE) of MMBT
  python bench.py --workload encoders  BASELINE config 5's producer: the FLAVA image + text
                                       encoders (data/encoding_with_flava.py) on HIP kernels
  python bench.py --workload vilt      ViLT classification inference (train.py setup_vilt model)
  python bench.py --workload vilt_train   ViLT classification training step (forward, backward, AdamW)

Rank 0 prints one JSON line (see README/DESIGN for the field definitions).

A plain run sets up, warms up, times the K steps and prints the line.  --full adds what takes
runs of its own: the CPU baseline (the oracle on the host cores; --no-cpu-baseline drops it
again) and, where the step is replayed as a HIP graph, the eager steps that time the GEMM /
fused-block rooflines.  --dump-outputs DIR writes what the last timed step returned (loss,
logits, a seeded sample of the updated parameters, ...) as DIR/<name>.npy; the inputs and the
initial weights are seeded, so two builds run with the same arguments compare output for output.
"""
import argparse
import json
import os
import platform
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REPO, "multi-modal-uncertainty_amd"), REPO]


def _miopen_user_db():
    """A working copy (under the ignored build/ directory) of the find-db shipped in
    multi-modal-uncertainty_amd/miopen_db: MIOpen rewrites its user db whenever it searches a
    shape that is not in it yet, and that must not touch the committed files."""
    import shutil
    src = os.path.join(REPO, "multi-modal-uncertainty_amd", "miopen_db")
    dst = os.path.join(REPO, "multi-modal-uncertainty_amd", "build", "miopen_db")
    try:
        os.makedirs(dst, exist_ok=True)
        for name in os.listdir(src):
            have = os.path.join(dst, name)
            if name.endswith(".txt") and not (os.path.exists(have) and
                                              os.path.getmtime(have) >= os.path.getmtime(os.path.join(src, name))):
                tmp = os.path.join(dst, f".{name}.{os.getpid()}")
                shutil.copyfile(os.path.join(src, name), tmp)
                os.replace(tmp, os.path.join(dst, name))   # ranks starting together: whole files only
    except OSError:
        return src
    return dst


# MIOpen reads its user db path when its first handle is created (first conv)
os.environ.setdefault("MIOPEN_USER_DB_PATH", _miopen_user_db())
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

BERT_FLOP_PER_SAMPLE_LAYER_FWD = None  # filled from the shape: L*(24H^2 + 4LH)
RESNET152_FWD_FLOP = 23.0e9            # per 224x224 sample (11.5 GMAC)
PEAK_BF16_TFLOPS = 2500.0              # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks (one per GPU). Without WORLD_SIZE in the environment and N > 1, bench.py starts "
                         "N ranks itself under torch.distributed.run (a child process); under an external "
                         "launcher N must equal WORLD_SIZE (default: WORLD_SIZE, else 1)")
    ap.add_argument("--dry-run", action="store_true",
                    help="start the ranks and the process group, print the JSON line's rank / world fields and "
                         "stop (no GPU work: the launcher's CPU test)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--global-batch", type=int, default=None,
                    help="samples per step split over the ranks (strong scaling; default 256)")
    ap.add_argument("--per-rank-batch", type=int, default=None,
                    help="samples per rank per step instead (weak scaling)")
    ap.add_argument("--text-len", type=int, default=508, help="word-pieces per sample (L = 5 + this)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what needs runs of its own: the CPU baseline and, under --graph, the "
                         "rooflines' eager steps before the capture (a plain run leaves those fields out / null)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one returned as DIR/<name>.npy (float32; "
                         "a seeded sample of anything too large, at most 64 MB in all)")
    ap.add_argument("--sync-bn", action="store_true",
                    help="mmbt, N > 1: the trunk's BatchNorms normalise over the whole global batch (cross-rank sums)")
    ap.add_argument("--main-priority", default="normal", choices=["normal", "high"],
                    help="mmbt: run the step on a high-priority stream (the side stream's weight-gradient work "
                         "then yields to the main stream's critical path)")
    ap.add_argument("--defer-gb", type=float, default=None,
                    help="mmbt: encoder.DEFER_MAX_BYTES in GB (deferred weight-gradient inputs retained before "
                         "an early flush; default a quarter of HBM: everything deferred to the trunk backward)")
    ap.add_argument("--side-cu-frac", type=float, default=None,
                    help="mmbt: restrict the side stream (weight-gradient GEMMs) to this fraction of the CUs "
                         "(hipExtStreamCreateWithCUMask), leaving the rest to the main stream's chain")
    ap.add_argument("--graph", default="auto", choices=["off", "on", "auto"],
                    help="mmbt: capture the whole step (forward, backward, fused BertAdam) once into a HIP graph "
                         "and replay it (src/graphs.py; the GEMM / block rooflines then come from 2 eager steps "
                         "before the capture); auto = on for a single process at per-rank batch <= 64, where the "
                         "step is launch-bound (profiles/r5_graph_b32.txt), off otherwise")
    ap.add_argument("--no-stream-residue", action="store_true",
                    help="mmbt: the trunk's residual stream in plain bf16 (the round-4 trunk; for same-box A/Bs)")
    ap.add_argument("--workload", default="mmbt",
                    choices=["mmbt", "flava", "uncertainty", "encoders", "vilt", "vilt_train"])
    ap.add_argument("--enc-batch", type=int, default=128, help="encoders / vilt: samples per rank per step")
    ap.add_argument("--members", type=int, default=5, help="uncertainty: deep-ensemble members K")
    ap.add_argument("--mc-samples", type=int, default=30, help="uncertainty: MC-dropout passes T")
    ap.add_argument("--eval-batch", type=int, default=32, help="uncertainty: samples per rank per step")
    ap.add_argument("--flava-batch", type=int, default=128, help="FLAVA per-rank batch (train.py --batch_size)")
    ap.add_argument("--flava-tokens", type=str, default="197,77", help="FLAVA image,text embedding lengths")
    ap.add_argument("--cpu-batch", type=int, default=8,
                    help="samples per oracle step of the CPU baseline (SURVEY §8(d): B = 8, 3 steps)")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="CPU-baseline threads (0: os.cpu_count(), SURVEY §8(d)'s torch.set_num_threads(os.cpu_count()))")
    return ap.parse_args(argv)


DUMP_BUDGET_BYTES = 60 << 20   # of the 64 MB a dump may take (the .npy headers are small)
PARAM_SAMPLE = 4096            # elements kept of every parameter tensor


def _sample(t, n, seed):
    """``t`` flattened; when it has more than ``n`` elements, the ones at ``n`` seeded random
    positions (the same positions for the same shape and seed, whatever the build)."""
    flat = t.detach().reshape(-1)
    if flat.numel() <= n:
        return flat
    idx = torch.randint(0, flat.numel(), (n,), generator=torch.Generator().manual_seed(seed))
    return flat[idx.to(flat.device)]


def params_sample(params):
    """A fixed sample of the parameters a train step updated: PARAM_SAMPLE seeded positions of each."""
    return torch.cat([_sample(p, PARAM_SAMPLE, 7000 + i).float() for i, p in enumerate(params)])


def _tensors(obj, prefix, out):
    """Flatten what a step returned (tensor, tuple / list / dict of them, a transformers
    ModelOutput) into name -> tensor."""
    if torch.is_tensor(obj):
        out[prefix] = obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _tensors(v, f"{prefix}_{k}", out)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            _tensors(v, f"{prefix}_{i}", out)
    return out


def dump_outputs(path, arrays):
    """Write name -> tensor as path/<name>.npy in float32 (float64 stays); every array gets an equal
    share of DUMP_BUDGET_BYTES and is a seeded sample of itself where it is larger."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(len(arrays), 1)
    for i, (name, t) in enumerate(sorted(arrays.items())):
        t = torch.as_tensor(t).detach()
        dt = torch.float64 if t.dtype == torch.float64 else torch.float32
        n = share // (8 if dt == torch.float64 else 4)
        if t.numel() > n:
            t = _sample(t, n, 9000 + i)
        np.save(os.path.join(path, name + ".npy"), t.to(dt).cpu().numpy())


def rank_launch_cmd(n, argv, port):
    """The child command that starts ``n`` ranks of this script on one node (the driver's own
    form: torch.distributed.run, rendezvous on 127.0.0.1), passing ``argv`` through."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
            "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + list(argv)


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def resolve_world(args, env=None):
    """-> (world, launch): the rank count this process belongs to, and whether it must first start
    that many ranks itself.  Runs before anything touches the GPU (no HIP call, no exec)."""
    env = os.environ if env is None else env
    if "WORLD_SIZE" in env:
        world = int(env["WORLD_SIZE"])
        if args.gpus is not None and args.gpus != world:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
        return world, False
    n = 1 if args.gpus is None else args.gpus
    if n < 1:
        raise SystemExit(f"bench.py: --gpus {n}")
    return n, n > 1


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def _cgroup_cpus():
    """CPUs the process's cgroup may run on at once (cpu.max quota / period), or None."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else max(1, int(int(q) / int(p)))
    except (OSError, ValueError):
        return None


def _cpu_threads(args):
    """Host threads for the CPU baseline: --cpu-threads, else SURVEY §8(d)'s os.cpu_count(),
    capped only by the CPUs this process can actually run on (its affinity mask and its cgroup's
    CPU quota): more threads than those would time OpenMP oversubscription, not the reference."""
    if args.cpu_threads:
        return args.cpu_threads
    n = min(os.cpu_count() or 1, len(os.sched_getaffinity(0)))
    q = _cgroup_cpus()
    return min(n, q) if q else n


def cpu_baseline(args, L_text):
    """The oracle (fp32 CPU restatement, oracle/mmbt_ref.py -- the reference's algorithm,
    pinned to it by tests/golden) on the host cores: the train step (fwd + bwd + BertAdam,
    what ``value`` reports), the eval full forward, and the 43-variant robustness pass of
    eval_mmbt_robustness.py:77-93."""
    from oracle import mmbt_ref as R
    from oracle.bertadam_ref import bertadam_step
    from oracle.weights import FULL, make_state_dict
    threads = _cpu_threads(args)
    torch.set_num_threads(threads)
    sd = make_state_dict(0, FULL)
    params = {}
    for k, v in sd.items():
        if v.is_floating_point() and id(v) not in {id(p) for p in params.values()} and "running" not in k:
            params[k] = v.requires_grad_(True)
    uniq = list({id(v): v for v in params.values()}.values())
    ms = [torch.zeros_like(p) for p in uniq]
    vs = [torch.zeros_like(p) for p in uniq]
    steps = [0] * len(uniq)
    B = args.cpu_batch
    g = torch.Generator().manual_seed(0)
    txt = torch.randint(1000, 30522, (B, L_text), generator=g)
    mask = torch.ones(B, L_text, dtype=torch.long)
    img = torch.randn(B, 3, 224, 224, generator=g)
    y = torch.randint(0, 101, (B,), generator=g)
    gen = torch.Generator().manual_seed(1)

    def one():
        nonlocal steps
        for p in uniq:
            p.grad = None
        logits = R.forward(sd, txt, mask, mask, img, FULL, train=True, dropout=0.1, gen=gen)
        R.cross_entropy(logits, y).backward()
        with torch.no_grad():
            steps = bertadam_step(uniq, [p.grad for p in uniq], ms, vs, steps, 5e-5, [0.01] * len(uniq), 0.1, 1000.0)

    def timed(fn, n):
        fn()  # warm-up
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) / n

    n = 3
    t_train = timed(one, n)
    with torch.no_grad():
        t_eval = timed(lambda: R.forward(sd, txt, mask, mask, img, FULL), n)
        torch.manual_seed(0)
        t_rob = timed(lambda: R.robustness(sd, txt[:1], mask[:1], mask[:1], img[:1], FULL, n_repeats=20), 1)
    return {"value": round(B / t_train, 4), "unit": "samples/s", "cores": threads, "kind": "port",
            "cpu_model": _cpu_model(), "host_cpus": os.cpu_count(),
            "affinity_cpus": len(os.sched_getaffinity(0)), "cgroup_cpus": _cgroup_cpus(),
            "eval_forward": {"value": round(B / t_eval, 4), "unit": "samples/s"},
            "robustness_43": {"value": round(1 / t_rob, 4), "unit": "samples/s",
                              "sample": "1 sample x 43 variants (full, img-only, txt-only, 20+20 controls), "
                                        "trunk computed once"},
            "sample": f"oracle fp32 train step (fwd+bwd+BertAdam), B={B}, L={L_text + 5}, {n} timed steps after 1 "
                      f"warm-up; eval forward B={B}; torch CPU {torch.get_num_threads()} threads"}


def gemm_traffic(per_rank_batch):
    """Per-launch HBM bytes of the GEMMs from the newest committed PMC summary
    (profiles/r*_gemm_traffic.json, written by tools/pmc_traffic.py from two rocprofv3
    --pmc passes of this script: FETCH_SIZE, WRITE_SIZE; gfx950 FETCH correction applied).
    Those passes ran the default per-rank batch (256): at any other batch the launches move
    other byte counts, so traffic is null there rather than a number from another workload."""
    import glob
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "profiles", "r*_gemm_traffic.json")))
    if not files:
        return {"bytes": None, "source": None}
    d = json.load(open(files[-1]))
    if per_rank_batch != d.get("per_rank_batch", 256):
        return {"bytes": None, "source": f"{os.path.relpath(files[-1], here)} (measured at per-rank batch "
                                          f"{d.get('per_rank_batch', 256)}, not this one)"}
    return {"bytes": round(d["traffic_bytes_per_launch"]), "source": os.path.relpath(files[-1], here)}


def flava_cpu_baseline(args, L_img, L_txt, B=16):
    """The oracle's fp32 FLAVA train step (oracle/flava_ref.py) on host cores."""
    from oracle import flava_ref as FR
    torch.set_num_threads(_cpu_threads(args))
    cfg = FR.FlavaConfig(out_dim=2)
    sd = {k: v.requires_grad_(True) for k, v in FR.make_state_dict(0, cfg).items()}
    img, txt, y = FR.make_inputs(B, L_img, L_txt, 2, 2, 0)
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-4, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.001)

    def one():
        opt.zero_grad()
        i2, t2, y2 = FR.data_forming(img, txt, y, "train", "MultiHead")
        FR.compute_loss(FR.forward(sd, i2, t2, cfg, train=True), y2).backward()
        opt.step()
    one()
    n = 3
    t0 = time.perf_counter()
    for _ in range(n):
        one()
    dt = time.perf_counter() - t0
    return {"value": round(B * n / dt, 3), "unit": "samples/s", "cores": _cpu_threads(args), "kind": "port",
            "sample": f"oracle fp32 FLAVA train step (fwd+bwd+AdamW), B={B}, L={L_img}+{L_txt}, {n} timed steps "
                      f"after 1 warm-up, torch CPU {torch.get_num_threads()} threads"}


def bench_flava(args, world, rank, dev):
    """BASELINE config 5: one optimizer step of the FLAVA fusion transformer (reference
    train.py:184-216 setup: MultiHead out_dim 2, AdamW, per-batch cosine schedule) on a
    synthetic batch of precomputed FLAVA embeddings [B, 197, 768] + [B, 77, 768]."""
    from src import encoder
    from src.model import FlavaFusionTransfomer
    from transformers.optimization import get_cosine_schedule_with_warmup
    L_img, L_txt = (int(v) for v in args.flava_tokens.split(","))
    B = args.flava_batch
    torch.manual_seed(1234)
    model = FlavaFusionTransfomer(out_dim=2, num_classes=2, avg_pool=False).to(dev)
    if world > 1:
        for p in model.parameters():
            dist.broadcast(p.data, 0)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.001)
    sched = get_cosine_schedule_with_warmup(opt, 100, 10000)
    g = torch.Generator().manual_seed(100 + rank)
    img = torch.randn(B, L_img, 768, generator=g).to(dev)
    txt = torch.randn(B, L_txt, 768, generator=g).to(dev)
    y = torch.randint(0, 2, (B,), generator=g).to(dev).unsqueeze(1).repeat(1, 2)
    model.train()
    params = list(model.parameters())

    def step():
        opt.zero_grad()
        logits = model((img, txt))
        loss = model.compute_loss(logits, y)
        loss.backward()
        if world > 1:
            grads = [p.grad for p in params]
            flat = torch._utils._flatten_dense_tensors(grads)
            dist.all_reduce(flat)
            flat.mul_(1.0 / world)
            for gr, f in zip(grads, torch._utils._unflatten_dense_tensors(flat, grads)):
                gr.copy_(f)
        opt.step()
        sched.step()
        return loss, logits

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    encoder.block_timing(True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, logits = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    block_ms, block_n = encoder.block_timing_read()
    encoder.block_timing(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(_tensors(logits, "logits", {}), loss=loss,
                                             params_sample=params_sample(params)))
    if world > 1:
        t = torch.tensor([dt], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    E, L = 768, L_img + L_txt
    # per sample and layer, forward: L (24 E^2 + 4 S E) with the attention's sequence S = B
    layer_fwd = L * (24 * E * E + 4 * B * E)
    block_tf = 3 * layer_fwd * B * (block_n / 2) / (block_ms * 1e-3) / 1e12 if block_ms > 0 else 0.0
    ms_step = 1000.0 * dt / args.steps
    out = {
        "metric": "FLAVA fusion-transformer train samples/sec (BASELINE config 5, Hateful Memes embeddings)",
        "value": round(B * world * args.steps / dt, 3), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic (seeded FLAVA-shaped embeddings; random-init weights)",
        "config": {"workload": "flava_fusion_train_step", "model": "FlavaFusionTransfomer 3 layers x 768, 3 heads",
                   "per_rank_batch": B, "global_batch": B * world, "tokens": f"{L_img}+{L_txt}",
                   "model_type": "MultiHead", "optimizer": "AdamW (torch)", "parallelism": f"dp{world}"},
        "fused_block_roofline": {
            "bound": "mfma", "flop_per_sample_per_layer": 3 * layer_fwd, "achieved": round(block_tf, 1),
            "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(block_tf / PEAK_BF16_TFLOPS, 4),
            "ms_per_layer_fwd_bwd": round(block_ms / max(block_n, 1) * 2, 4), "layer_passes_timed": block_n,
            "share_of_step": round(block_ms / args.steps / ms_step, 3) if ms_step else None},
        "final_loss": round(float(loss.item()), 4),
    }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = flava_cpu_baseline(args, L_img, L_txt)
    return out


def uncertainty_cpu_baseline(args, L_text, B=2, passes=2):
    """The oracle's fp32 MC-dropout forward (oracle/mmbt_ref.py) on host cores: one member,
    ResNet features computed once (as the HIP path does), ``passes`` dropout passes."""
    from oracle import mmbt_ref as R
    from oracle.weights import FULL, make_state_dict
    torch.set_num_threads(_cpu_threads(args))
    sd = make_state_dict(0, FULL)
    g = torch.Generator().manual_seed(0)
    txt = torch.randint(1000, 30522, (B, L_text), generator=g)
    mask = torch.ones(B, L_text, dtype=torch.long)
    img = torch.randn(B, 3, 224, 224, generator=g)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        t0 = time.perf_counter()
        feats = R.image_encoder(sd, img, FULL)
        t1 = time.perf_counter()
        for _ in range(passes):
            R.forward(sd, txt, mask, mask, img, FULL, dropout=0.1, gen=gen, feats=feats)
        t2 = time.perf_counter()
    # one evaluated sample = K ResNet trunks + K x T MC-dropout encoder passes
    per_sample = (args.members * (t1 - t0) + args.members * args.mc_samples * (t2 - t1) / passes) / B
    return {"value": round(1.0 / per_sample, 5), "unit": "samples/s", "cores": _cpu_threads(args), "kind": "port",
            "sample": f"oracle fp32 eval: 1 member, ResNet once + {passes} MC-dropout encoder passes, B={B}, "
                      f"L={L_text + 5}, timed and scaled to K={args.members} trunks + K x T={args.mc_samples} "
                      f"encoder passes per sample, torch CPU {torch.get_num_threads()} threads"}


def bench_uncertainty(args, world, rank, dev):
    """BASELINE config 3: a K-member deep ensemble x T-pass MC-dropout evaluation of MMBT
    (src/uncertainty.py; K = 5, T = 30 by default) on a synthetic batch per rank: the K
    ResNet-152 trunks once per batch, the K*T*B encoder passes as ONE batched launch per op,
    then NLL / ECE over the batch (mmu_uncertainty, mmu_ece_bins).  Samples are sharded over
    ranks (weak scaling; the only exchange is the metric sums, outside the timed loop)."""
    from src.mmbt import MultimodalBertClf
    from src.testing import make_args, synthetic_batch
    from src.uncertainty import EnsembleMMBT, UncertaintyMeter
    torch.backends.cudnn.benchmark = os.environ.get("MMU_MIOPEN_FIND", "1") == "1"
    Km, T_mc, B, T = args.members, args.mc_samples, args.eval_batch, args.text_len
    L = T + 5
    members = []
    for k in range(Km):
        torch.manual_seed(1000 + k)
        members.append(MultimodalBertClf(make_args()).to(dev).eval())
    ens = EnsembleMMBT(members)
    x, y = synthetic_batch(B, T, seed=200 + rank, device=dev)
    events = []
    layer = ens._layer

    def timed_layer(*a, **kw):
        if not timing:
            return layer(*a, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = layer(*a, **kw)
        e1.record()
        events.append((e0, e1))
        return out
    ens._layer = timed_layer
    timing = False
    meter = UncertaintyMeter(15)

    def step():
        with torch.no_grad():
            lo = ens.logits(*x, mc_samples=T_mc)                         # [K, T, B, C]
            flat = lo.permute(2, 0, 1, 3).reshape(B, Km * T_mc, lo.shape[-1])
            meter.update(flat, y)
        return lo

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    timing = True
    meter = UncertaintyMeter(15)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        lo = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    timing = False
    layer_ms = sum(a.elapsed_time(b) for a, b in events)
    if world > 1:
        t = torch.tensor([dt], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    res = meter.result()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"logits": lo, "metrics": torch.tensor(
            [res["nll"], res["ece"], res["acc"]], dtype=torch.float64)})
    H = 768
    layer_fwd = L * (24 * H * H + 4 * L * H)             # per sequence per layer, forward
    seqs = Km * T_mc * B
    block_tf = layer_fwd * seqs * len(events) / (layer_ms * 1e-3) / 1e12 if layer_ms else 0.0
    flop_step = seqs * 12 * layer_fwd + Km * B * RESNET152_FWD_FLOP
    ms_step = 1000.0 * dt / args.steps
    out = {
        "metric": "MMBT deep-ensemble x MC-dropout eval samples/sec (BASELINE config 3; NLL / ECE)",
        "value": round(B * world * args.steps / dt, 3), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic (seeded; random-init members)",
        "config": {"workload": "mmbt_ensemble_mc_dropout_eval", "model": "MMBT bert-base-uncased + resnet152",
                   "members": Km, "mc_samples": T_mc, "per_rank_batch": B, "global_batch": B * world,
                   "seq_len": 512, "tokens": L, "encoder_passes_per_step": seqs, "parallelism": f"dp{world}"},
        # the batched encoder layer (all K*T*B sequences of one layer: QKV / attention / Wo /
        # LN / FFN / LN forward), timed by HIP events around every layer launch group
        "fused_block_roofline": {
            "bound": "mfma", "flop_per_sequence_per_layer": layer_fwd, "achieved": round(block_tf, 1),
            "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(block_tf / PEAK_BF16_TFLOPS, 4),
            "ms_per_layer": round(layer_ms / max(len(events), 1), 3), "layer_launch_groups_timed": len(events),
            "share_of_step": round(layer_ms / args.steps / ms_step, 3) if ms_step else None},
        "model_tflops_achieved": round(flop_step * world / (ms_step * 1e-3) / 1e12, 1),
        "nll": round(res["nll"], 5), "ece": round(res["ece"], 5), "acc": round(res["acc"], 5),
    }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = uncertainty_cpu_baseline(args, T)
    return out


def _encoder_cpu_baseline(args, run, B, what):
    """the transformers module itself (the reference's own third-party encoder: the class it
    loads pretrained) in fp32 on host cores, B samples, 1 warm-up + 2 timed calls"""
    torch.set_num_threads(_cpu_threads(args))
    with torch.no_grad():
        run()
        n = 2
        t0 = time.perf_counter()
        for _ in range(n):
            run()
        dt = time.perf_counter() - t0
    return {"value": round(B * n / dt, 3), "unit": "samples/s", "cores": _cpu_threads(args), "kind": "reference",
            "sample": f"transformers {what} fp32 forward (random init, eval), B={B}, {n} timed calls after 1 warm-up, "
                      f"torch CPU {torch.get_num_threads()} threads"}


def bench_vilt_train(args, world, rank, dev):
    """The reference's ViLT training step (train.py:164-182 setup_vilt: ViltForImagesAndTextClassification,
    AdamW over its parameters; src/framework.py:262-300: outputs = model(**batch), loss.backward(),
    optimizer.step()) on the HIP kernels (src/vilt.py ViltTrainHIP): 384^2 image -> 145 tokens + 40
    text tokens, B samples per rank.  Random-init weights, synthetic inputs; the gradient
    all-reduce over ranks (flat, like --workload flava) when N > 1."""
    from src import kernels as K
    from src.vilt import ViltTrainHIP
    from transformers import ViltConfig, ViltForImagesAndTextClassification
    B = args.enc_batch
    torch.manual_seed(1234)
    cfg = ViltConfig(num_images=1, num_labels=2)
    model = ViltForImagesAndTextClassification(cfg).to(dev).train()
    if world > 1:
        for p in model.parameters():
            dist.broadcast(p.data, 0)
    hip = ViltTrainHIP(model)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    params = list(model.parameters())
    g = torch.Generator().manual_seed(300 + rank)
    Lt = cfg.max_position_embeddings
    batch = dict(input_ids=torch.randint(1000, cfg.vocab_size, (B, Lt), generator=g).to(dev),
                 attention_mask=torch.ones(B, Lt, dtype=torch.long, device=dev),
                 pixel_values=torch.randn(B, 1, 3, cfg.image_size, cfg.image_size, generator=g).to(dev),
                 labels=torch.randint(0, 2, (B,), generator=g).to(dev))

    last = [None]

    def step():
        opt.zero_grad()
        out = hip(**batch)
        out.loss.backward()
        last[0] = out
        if world > 1:
            grads = [p.grad for p in params]
            flat = torch._utils._flatten_dense_tensors(grads)
            dist.all_reduce(flat)
            flat.mul_(1.0 / world)
            for gr, f in zip(grads, torch._utils._unflatten_dense_tensors(flat, grads)):
                gr.copy_(f)
        opt.step()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    K.timing_enable(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    gemm_ms, gemm_n, gemm_flop = K.timing_read()
    K.timing_enable(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": last[0].loss, "logits": last[0].logits,
                                         "params_sample": params_sample(params)})
    if world > 1:
        t = torch.tensor([dt], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    H, L = 768, Lt + (cfg.image_size // cfg.patch_size) ** 2 + 1
    flop_sample = 3 * cfg.num_hidden_layers * L * (24 * H * H + 4 * L * H)  # forward + backward
    ms_step = 1000.0 * dt / args.steps
    gemm_tf = gemm_flop / (gemm_ms * 1e-3) / 1e12 if gemm_ms else 0.0
    out = {
        "metric": "ViLT classification train samples/sec (train.py setup_vilt, AdamW)",
        "value": round(B * world * args.steps / dt, 3), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic (seeded images / token ids; random-init weights)",
        "config": {"workload": "vilt_train", "model": "ViltForImagesAndTextClassification", "per_rank_batch": B,
                   "global_batch": B * world, "tokens": str(L), "parallelism": f"dp{world}"},
        "roofline": {"bound": "mfma", "achieved": round(gemm_tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(gemm_tf / PEAK_BF16_TFLOPS, 4), "traffic": None,
                     "gemm_launches_timed": gemm_n, "gemm_ms_per_step": round(gemm_ms / args.steps, 3)},
        "model_tflops_achieved": round(flop_sample * B * world / (ms_step * 1e-3) / 1e12, 1),
    }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        ref = ViltForImagesAndTextClassification(cfg).train()
        ropt = torch.optim.AdamW(ref.parameters(), lr=1e-4)
        cb = {k: v[:2].cpu() for k, v in batch.items()}
        torch.set_num_threads(_cpu_threads(args))

        def cpu_step():
            ropt.zero_grad()
            ref(**cb).loss.backward()
            ropt.step()
        cpu_step()
        t0 = time.perf_counter()
        for _ in range(2):
            cpu_step()
        cdt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(2 * 2 / cdt, 3), "unit": "samples/s", "cores": _cpu_threads(args),
                               "kind": "reference", "sample": "transformers ViltForImagesAndTextClassification fp32 "
                               "train step (forward, backward, AdamW; random init), B=2, 2 timed steps after 1 warm-up, "
                               f"torch CPU {torch.get_num_threads()} threads"}
    return out


def bench_encoders(args, world, rank, dev):
    """BASELINE config 5's producer (reference data/encoding_with_flava.py:11-41): FLAVA image
    (224^2 -> 197 tokens) + text (77 tokens) encoders of a transformers FlavaModel on the HIP
    kernels (src/flava_encoders.py), B memes per rank per step; --workload vilt: ViLT
    classification (train.py setup_vilt: ViltForImagesAndTextClassification, 384^2 image ->
    145 tokens + 40 text tokens, src/vilt.py).  Random-init weights (no offline checkpoint),
    synthetic inputs; samples shard over ranks (weak scaling, no exchange)."""
    from src import kernels as K
    vilt = args.workload == "vilt"
    B = args.enc_batch
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(300 + rank)
    if vilt:
        from transformers import ViltConfig, ViltForImagesAndTextClassification
        from src.vilt import ViltHIP
        cfg = ViltConfig(num_images=1, num_labels=2)
        ref = ViltForImagesAndTextClassification(cfg).eval()
        hip = ViltHIP(ref, dev)
        Lt = cfg.max_position_embeddings
        ids = torch.randint(1000, cfg.vocab_size, (B, Lt), generator=g)
        pix = torch.randn(B, 1, 3, cfg.image_size, cfg.image_size, generator=g)
        mask = torch.ones(B, Lt, dtype=torch.long)
        inputs = [t.to(dev) for t in (ids, mask)] + [None, pix.to(dev), None]
        L_tok = Lt + (cfg.image_size // cfg.patch_size) ** 2 + 1
        passes = [(L_tok, cfg.num_hidden_layers)]
        run = lambda: hip(*inputs)  # noqa: E731
        cpu_run = lambda: ref(input_ids=ids[:2], attention_mask=mask[:2], pixel_values=pix[:2])  # noqa: E731
        what = "ViltForImagesAndTextClassification"
    else:
        from transformers import FlavaConfig, FlavaModel
        from src.flava_encoders import FlavaEncodersHIP
        ref = FlavaModel(FlavaConfig()).eval()
        hip = FlavaEncodersHIP(ref, dev)
        Lt, Li = 77, 197
        ids = torch.randint(1000, 30000, (B, Lt), generator=g)
        pix = torch.randn(B, 3, 224, 224, generator=g)
        mask = torch.ones(B, Lt, dtype=torch.long)
        inputs = (pix.to(dev), ids.to(dev), mask.to(dev))
        passes = [(Li, ref.config.image_config.num_hidden_layers), (Lt, ref.config.text_config.num_hidden_layers)]
        run = lambda: hip(*inputs)  # noqa: E731
        cpu_run = lambda: (ref.image_model(pixel_values=pix[:2]), ref.text_model(input_ids=ids[:2],  # noqa: E731
                                                                                 attention_mask=mask[:2]))
        what = "FlavaModel image_model + text_model"
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    K.timing_enable(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    gemm_ms, gemm_n, gemm_flop = K.timing_read()
    K.timing_enable(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, _tensors(res.to_tuple() if hasattr(res, "to_tuple") else res, "out", {}))
    if world > 1:
        t = torch.tensor([dt], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    H = 768
    # forward FLOPs per sample: sum over the encoder passes of layers * L (24 H^2 + 4 L H)
    flop_sample = sum(n * L * (24 * H * H + 4 * L * H) for L, n in passes)
    ms_step = 1000.0 * dt / args.steps
    gemm_tf = gemm_flop / (gemm_ms * 1e-3) / 1e12 if gemm_ms else 0.0
    out = {
        "metric": ("ViLT classification inference samples/sec" if vilt else
                   "FLAVA image+text encoding samples/sec (BASELINE config 5 producer, Hateful Memes)"),
        "value": round(B * world * args.steps / dt, 3), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic (seeded images / token ids; random-init weights)",
        "config": {"workload": "vilt_classification" if vilt else "flava_encoders",
                   "model": what, "per_rank_batch": B, "global_batch": B * world,
                   "tokens": "+".join(str(L) for L, _ in passes), "parallelism": f"dp{world}"},
        # every encoder-layer mmu_gemm launch bracketed by HIP events on its stream
        "roofline": {"bound": "mfma", "achieved": round(gemm_tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(gemm_tf / PEAK_BF16_TFLOPS, 4), "traffic": None,
                     "gemm_launches_timed": gemm_n, "gemm_ms_per_step": round(gemm_ms / args.steps, 3)},
        "model_tflops_achieved": round(flop_sample * B * world / (ms_step * 1e-3) / 1e12, 1),
    }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = _encoder_cpu_baseline(args, cpu_run, 2, what)
    return out


def main():
    args = parse()
    # Which solvers MIOpen's find may try (read at the first conv; set here, not at import, so
    # that only benchmark runs are affected).  Every new process searches each conv shape again
    # whatever the find-db holds (the records come back rewritten with new timings), and the
    # search compiles and times the naive direct convolutions too: 20-300 ms a run at batch 256
    # against 0.06-0.3 ms for the implicit-GEMM solvers that always win (miopen_db/*.ufdb.txt),
    # ~30 s before the first step ends.  Without them the find picks the same solvers.
    for d in ("FWD", "BWD", "WRW"):
        os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + d, "0")
    world, launch = resolve_world(args)
    if launch:
        # no launcher around us: start the N ranks (one per GPU) as a child torch.distributed.run
        # and exit with its status -- a child process, never an exec, and before any HIP call
        one_dev = os.environ.get("MMU_BENCH_ONE_DEVICE") == "1"
        if not args.dry_run and not one_dev and torch.cuda.device_count() < world:
            raise SystemExit(f"bench.py: --gpus {world} but {torch.cuda.device_count()} GPUs are visible")
        import subprocess
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.call(rank_launch_cmd(world, sys.argv[1:], _free_port()), env=env))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # MMU_BENCH_BACKEND=gloo MMU_BENCH_ONE_DEVICE=1: a one-GPU rehearsal of the N > 1 path (every
    # rank on cuda:0, collectives over gloo) -- the glue, bucketing and timing code of an 8-GPU run,
    # not its performance; the default is one rank per GPU over RCCL
    backend = os.environ.get("MMU_BENCH_BACKEND", "nccl")
    if os.environ.get("MMU_BENCH_ONE_DEVICE") == "1":
        local = 0
    if args.dry_run:
        # the launcher's check: ranks, process group and the world size the backend reports
        if world > 1:
            dist.init_process_group(backend)
        out = {"n_gpus": world, "world_size_reported": dist.get_world_size() if world > 1 else 1,
               "rank": rank, "backend": backend if world > 1 else None, "dry_run": True}
        if world > 1:
            seen = [None] * world
            dist.all_gather_object(seen, rank)
            out["ranks_seen"] = seen
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps(out), flush=True)
        return
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
        if dist.get_world_size() != world:
            raise SystemExit(f"bench.py: WORLD_SIZE {world} but the process group reports {dist.get_world_size()}")
    dev = torch.device("cuda", local)
    if args.workload in ("flava", "uncertainty", "encoders", "vilt", "vilt_train"):
        fn = {"flava": bench_flava, "uncertainty": bench_uncertainty, "encoders": bench_encoders,
              "vilt": bench_encoders, "vilt_train": bench_vilt_train}[args.workload]
        out = fn(args, world, rank, dev)
        out["world_size_reported"] = dist.get_world_size() if dist.is_initialized() else 1
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    if args.global_batch is None and args.per_rank_batch is not None:
        args.global_batch = args.per_rank_batch * world
        scaling = "weak"
    else:
        if args.global_batch is None:
            args.global_batch = 256
        if args.global_batch % world:
            raise SystemExit("global batch must divide evenly over ranks")
        scaling = "strong"
    B = args.global_batch // world
    T = args.text_len
    L = T + 5

    from src.mmbt import MultimodalBertClf
    from src.optim import BertAdam
    from src.testing import make_args, synthetic_batch
    from src import kernels as K
    from src.dp import GradBucketer, broadcast_parameters, convert_sync_batchnorm
    from src import encoder
    from src import resnet

    resnet.STREAM_RESIDUE = not args.no_stream_residue
    if args.defer_gb is not None:
        encoder.DEFER_MAX_BYTES = int(args.defer_gb * 1e9)
    if args.side_cu_frac:
        from src import kernels
        kernels.SIDE_CU_FRAC = args.side_cu_frac
    if args.main_priority == "high":
        torch.cuda.set_stream(torch.cuda.Stream(device=dev, priority=-1))
    # MIOpen solver choice for the ResNet convs: "find" mode over the find-db shipped in
    # multi-modal-uncertainty_amd/miopen_db (per-rank batches 256/128/64/32 pre-searched on
    # MI355X, so no search runs here); MMU_MIOPEN_FIND=0 = MIOpen's immediate-mode heuristics
    torch.backends.cudnn.benchmark = os.environ.get("MMU_MIOPEN_FIND", "1") == "1"
    torch.manual_seed(1234)
    margs = make_args()
    model = MultimodalBertClf(margs).to(dev)
    named = list(model.named_parameters())
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
              {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
    opt = BertAdam(groups, lr=5e-5, warmup=0.1, t_total=10000.0)
    bucketer = None
    if world > 1:
        broadcast_parameters(model)
        if args.sync_bn:
            convert_sync_batchnorm(model)
        bucketer = GradBucketer(model, optimizer=opt)  # 1/world folded into the fused BertAdam
    x, y = synthetic_batch(B, T, seed=100 + rank, device=dev)
    model.train()

    def step():
        opt.zero_grad()
        logits = model(*x)
        loss = model.compute_loss(logits, y)
        loss.backward()
        if bucketer is not None:
            bucketer.finish()
        opt.step()
        return loss, logits

    graph = args.graph == "on" or (args.graph == "auto" and world == 1 and B <= 64)
    if graph and world > 1:
        # (the bucketed all-reduce inside a captured backward needs RCCL graph capture, which the
        # one-GPU boxes this was developed on cannot exercise)
        raise SystemExit("--graph on: single-process runs only (N = 1)")
    run = step
    rooflines = args.full or not graph   # eager steps time their own launches; a replay needs steps apart
    if graph:
        if rooflines:
            # the rooflines' per-launch timings from 2 eager steps (the same kernels the graph replays)
            step()
            K.timing_enable(True)
            encoder.block_timing(True)
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            gemm_ms, gemm_n, gemm_flops = K.timing_read()
            alg_bytes, _ = K.timing_alg_bytes()
            K.timing_enable(False)
            block_ms, block_n = encoder.block_timing_read()
            encoder.block_timing(False)
            timed_steps = 2
            torch.cuda.empty_cache()
        from src.graphs import StepGraph
        sg = StepGraph(step, dev, warmup=2)
        run = sg.replay
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    if not graph:
        K.timing_enable(True)
        encoder.block_timing(True)
        timed_steps = args.steps
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, logits = run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if not graph:
        gemm_ms, gemm_n, gemm_flops = K.timing_read()
        alg_bytes, _ = K.timing_alg_bytes()
        K.timing_enable(False)
        block_ms, block_n = encoder.block_timing_read()
        encoder.block_timing(False)
    if world > 1:
        t = torch.tensor([dt], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": loss, "logits": logits,
                                         "params_sample": params_sample(model.parameters())})
    ms_step = 1000.0 * dt / args.steps
    traffic = gemm_traffic(B)
    value = args.global_batch * args.steps / dt
    H = 768
    layer_fwd = L * (24 * H * H + 4 * L * H)
    model_flop = 3 * (12 * layer_fwd + RESNET152_FWD_FLOP)
    if not rooflines:
        gemm_ms = gemm_n = gemm_flops = alg_bytes = block_ms = block_n = 0
        timed_steps = 1
    achieved = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
    block_tf = 3 * layer_fwd * B * (block_n / 2) / (block_ms * 1e-3) / 1e12 if block_ms > 0 else 0.0
    out = {
        "metric": "image+text samples/sec/node, MMBT Food-101 bs=256 seq=512; ECE/NLL parity",
        "value": round(value, 3), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True,
        "scaling": scaling, "vs_baseline": None, "dtype": "bf16", "data": "synthetic (seeded; random-init weights)",
        "config": {"workload": "mmbt_train_step", "model": "MMBT bert-base-uncased + resnet152",
                   "global_batch": args.global_batch, "per_rank_batch": B, "seq_len": 512, "tokens": L,
                   "parallelism": f"dp{world}", "grad_accum": 1, "optimizer": "BertAdam (fused HIP)",
                   "batchnorm": "whole-batch (cross-rank sums)" if (args.sync_bn and world > 1) else "per-rank batch",
                   "trunk_stream": "bf16 + 8-bit residue" if resnet.STREAM_RESIDUE else "bf16",
                   "launch": "HIP graph replay of the whole step" if graph else "eager (per-kernel launches)",
                   "trainable_params": sum(p.numel() for p in model.parameters())},
        "roofline": {"bound": "mfma", "kernel": "mmu_gemm (all BERT-layer GEMMs, fwd + bwd)",
                     "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": traffic["bytes"],
                     "traffic_unit": "bytes/launch (PMC, corrected)", "traffic_source": traffic["source"],
                     "algorithmic_bytes_per_launch": round(alg_bytes / max(gemm_n, 1)),
                     "launches": gemm_n, "avg_launch_ms": round(gemm_ms / max(gemm_n, 1), 4),
                     "gemm_share_of_step": round(gemm_ms / timed_steps / ms_step, 3) if ms_step else None,
                     "timed_over": "2 eager steps before the graph capture" if graph else "the timed steps"},
        # BASELINE north star: >= 40 % of the bf16 MFMA peak on the fused MMBT block (one
        # BertLayer fwd + bwd = 3 x L (24 H^2 + 4 L H) flop per sample), timed by HIP events
        # around every layer's forward and backward (GEMMs, attention, LayerNorms, reductions)
        "fused_block_roofline": {
            "bound": "mfma", "flop_per_sample_per_layer": 3 * layer_fwd,
            "achieved": round(block_tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(block_tf / PEAK_BF16_TFLOPS, 4), "target_frac": 0.40,
            "ms_per_layer_fwd_bwd": round(block_ms / max(block_n, 1) * 2, 4), "layer_passes_timed": block_n,
            "share_of_step": round(block_ms / timed_steps / ms_step, 3) if ms_step else None},
        "model_tflops_per_step_per_rank": round(B * model_flop / 1e12, 2),
        "model_tflops_achieved": round(B * model_flop * world / (ms_step * 1e-3) / 1e12, 1),
        "final_loss": round(float(loss.item()), 4),
        "hbm_peak_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 1),
    }
    if not rooflines:
        # a graph replay has no per-launch events and a plain run no eager steps for them
        out["roofline"] = out["fused_block_roofline"] = None
    out["world_size_reported"] = dist.get_world_size() if dist.is_initialized() else 1
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, T)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
