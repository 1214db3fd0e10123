"""The fused BertAdam step (csrc/optim.hip: adam_sqnorm_kernel, adam_coef_kernel,
adam_update_kernel) against float64 on a table packed as ParamStore packs it, through guarded
buffers: every alignment arm of the update's `vec` and of the norm's scalar head / 16-B body / tail,
both weight-decay groups, inactive tensors between active ones, a chunk at the production length.
Table, gradients, runs and the float32 rounding model: tests/bertadam_harness.py (its CPU checks:
test_bertadam_reference.py).

Runs (bertadam_harness.RUNS), six steps each with fresh gradients: t_total = 5 with warmup 0.4 (lr 0
at step 0, the knee at step 2, t_total reached at step 5 where the schedule clamps at 0) at
grad_scale 1 and 0.5; t_total = -1 (no schedule); max_grad_norm = 0 (no clipping) at grad_scale 0.5.

Checked after every step, the float64 reference and the model restarted from the kernel's own state
(so each step is one step's rounding errors against one step's):
  p, m, v of every active tensor: |err| <= max(8 x the model's largest |err| / scale on that
      tensor x scale, 4 f32 ulps of the scale), scale = |p| + lr |u|, |m|, |v| (rowops_harness.f32_stats);
      an element whose scale is 0 (the zero gradient's m and v) must be exact
  the bf16 copy bit-equal to bf16(the kernel's own p) for every active tensor that has one
  steps exact; the inactive tensors' p, m, v, copy and step bit-unchanged
  the guards of the flat p, g, m, v, copy, steps and workspace buffers intact (the 8-element margin
  keeps their 16-B alignment, so a tensor's alignment is its offset's)

Measured on an MI355X: DESIGN.md, "BatchNorm and BertAdam edge sweeps".
"""
import pytest
import torch

import bertadam_harness as A
import rowops_harness as R
from guarded import Guarded, check_written, guarded_input, inout_buf

pytestmark = pytest.mark.gpu


def K():
    from src import kernels
    return kernels


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize("run", A.RUNS, ids=[r[0] for r in A.RUNS])
def test_bertadam_edges(dev, run):
    k = K()
    _, t_total, warmup, max_norm, gscale = run
    L, H = A.layout(), A.HYPER
    n, n_chunks = len(L["sizes"]), len(L["chunks"])
    p0, m0, v0, c0 = A.initial(L)
    bufs = {}
    bufs["p"], P = inout_buf(dev, p0)
    bufs["m"], M = inout_buf(dev, m0)
    bufs["v"], V = inout_buf(dev, v0)
    bufs["copy"], C = inout_buf(dev, c0)
    steps0 = torch.tensor([0 if a else 11 for a in L["active"]], dtype=torch.int32)
    bufs["steps"], S = inout_buf(dev, steps0, fill=-7)
    bufs["ws"] = Guarded(dev, torch.float32, float("nan"), n_chunks + 2 * n)
    ws = bufs["ws"].view
    table = guarded_input(dev, L["table"])
    ref, mod = A.Track(L, p0, m0, v0, torch.float64), A.Track(L, p0, m0, v0, torch.float32)
    inactive = [t for t in range(n) if not L["active"][t]]
    cut = lambda flat, t: flat[L["offs"][t]:L["offs"][t] + L["sizes"][t]]  # noqa: E731
    ccut = lambda flat, t: flat[L["coffs"][t]:L["coffs"][t] + L["sizes"][t]]  # noqa: E731
    fails, worst = [], {"p": [0.0, 0.0, 0.0], "m": [0.0, 0.0, 0.0], "v": [0.0, 0.0, 0.0]}
    for step in range(A.STEPS):
        g = A.grads(L, step, max_norm)
        before = (P.cpu(), M.cpu(), V.cpu())
        ref.load(*before)
        mod.load(*before)
        ref.step(g, run)
        mod.step(g, run)
        bufs["g"] = Guarded(dev, torch.float32, float("nan"), L["total"])
        bufs["g"].view.copy_(g)
        k.bertadam_step(P, bufs["g"].view, M, V, C, table, S, n, n_chunks, H["lr_decay"], H["lr_nodecay"], H["wd"],
                        warmup, t_total, H["b1"], H["b2"], H["eps"], max_norm, ws, grad_scale=gscale)
        torch.cuda.synchronize()
        tag = f"{run[0]} step {step}"
        check_written({kk: vv for kk, vv in bufs.items() if kk != "g"}, fails, tag)
        if not bufs["g"].guards_intact() or not torch.equal(_bits(bufs["g"].view.cpu()), _bits(g)):
            fails.append(f"{tag}: the gradient buffer or its guards changed")
        got = {"p": P.cpu(), "m": M.cpu(), "v": V.cpu()}
        copy, st = C.cpu(), S.cpu().tolist()
        for t in ref.act:
            for key, rr, mm in (("p", ref.p, mod.p), ("m", ref.m, mod.m), ("v", ref.v, mod.v)):
                ek, em, w = R.f32_stats(cut(got[key], t), mm[t], rr[t], ref.scale[t][key])
                ww = worst[key]
                ww[0], ww[1], ww[2] = max(ww[0], ek), max(ww[1], em), max(ww[2], w)
                if not w <= 1.0:
                    fails.append(f"{tag} tensor {t} (numel {L['sizes'][t]}, offset {L['offs'][t]}) {key}: error {ek:.3e} "
                                 f"of scale (model {em:.3e}): {w:.2f} x the bar")
            if L["coffs"][t] >= 0 and not torch.equal(_bits(ccut(copy, t)), _bits(cut(got["p"], t).to(torch.bfloat16))):
                fails.append(f"{tag} tensor {t}: the bf16 copy is not bf16(p)")
            if st[t] != step + 1:
                fails.append(f"{tag} tensor {t}: step count {st[t]}")
        for t in inactive:
            same = all(torch.equal(_bits(cut(got[key], t)), _bits(cut(f0, t))) for key, f0 in
                       (("p", p0), ("m", m0), ("v", v0)))
            if L["coffs"][t] >= 0:
                same = same and torch.equal(_bits(ccut(copy, t)), _bits(ccut(c0, t)))
            if not same or st[t] != 11:
                fails.append(f"{tag} inactive tensor {t}: p, m, v, copy or step changed")
    for key, (ek, em, w) in worst.items():
        print(f"SUMMARY bertadam {run[0]} {key}: err/scale kernel {ek:.3e} model {em:.3e}, {w:.3f} of bar")
    assert not fails, "\n".join(fails[:40])
