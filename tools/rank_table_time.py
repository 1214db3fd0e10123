"""mmu_rank_table at (S, J) = (1000, 47) and (10000, 47): warm launches timed with device events, the spread
over repeats; beside it the host uncertainty.auroc looped over the same 47 columns (context only)."""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-modal-uncertainty_amd"))
import numpy as np, torch
from src import kernels as K
from src.uncertainty import auroc
from src.ranking import auroc_from_counts
dev = torch.device("cuda:0")
out = {}
for S, J in ((1000, 47), (10000, 47)):
    g = torch.Generator().manual_seed(S)
    x = torch.randn(S, J, generator=g)
    pos = torch.rand(S, generator=g) < 0.35
    xd, pd = x.to(dev), pos.to(dev).to(torch.uint8)
    rank = torch.empty(J, S, 4, dtype=torch.int32, device=dev)
    counts = torch.empty(J, 5, dtype=torch.int64, device=dev)
    for with_rank in (True, False):
        r = rank if with_rank else None
        for _ in range(20):
            K.rank_table(xd, pd, rank=r, counts=counts)
        torch.cuda.synchronize()
        reps, inner = 15, max(20, int(200000 // S))
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                K.rank_table(xd, pd, rank=r, counts=counts)
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / inner)
        ms = np.array(ms)
        key = f"S={S} J={J} rank={'yes' if with_rank else 'no'}"
        out[key] = dict(median_us=float(np.median(ms) * 1e3), min_us=float(ms.min() * 1e3), max_us=float(ms.max() * 1e3),
                        repeats=reps, launches_per_repeat=inner)
        print(key, out[key], flush=True)
    dev_auc = auroc_from_counts(counts)
    xs, ps = x.double().numpy(), pos.numpy()
    host = []
    for _ in range(7):
        t = time.perf_counter()
        h = [auroc(xs[:, j], ps) for j in range(J)]
        host.append(time.perf_counter() - t)
    host = np.array(host)
    out[f"S={S} J={J} host auroc x{J}"] = dict(median_us=float(np.median(host) * 1e6), min_us=float(host.min() * 1e6),
                                              max_us=float(host.max() * 1e6), repeats=7)
    print(f"S={S} host auroc loop", out[f"S={S} J={J} host auroc x{J}"], "max |device - host| =",
          max(abs(a - b) for a, b in zip(dev_auc, h)), flush=True)
os.makedirs("bench_out", exist_ok=True)
json.dump(out, open("bench_out/rank_table_time.json", "w"), indent=1)
