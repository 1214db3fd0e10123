"""Guarded device buffers for the kernel edge sweeps (test_attention_edges_gpu.py,
test_layernorm_edges_gpu.py, test_embed_edges_gpu.py, test_batchnorm_edges_gpu.py,
test_bertadam_edges_gpu.py, test_gemm_edges_gpu.py, test_conv_edges_gpu.py, test_stem_edges_gpu.py,
test_pool_edges_gpu.py, test_seqattn_edges_gpu.py): every tensor a kernel sees is a view of a larger allocation.  Input guards hold NaN, so a read through them poisons the result; outputs are
pre-filled with a canary, and afterwards everything outside the view must be bit-identical to it.
  out_buf / check_written: NaN-filled contiguous outputs and their check after a launch;
  probe_keep: the keep bits of the GEMM's BIAS_DROP_RES epilogue, read from the epilogue itself.
"""
import torch

NAN = float("nan")
bf16 = torch.bfloat16

G = 2          # guard rows on each side of a 2-D buffer
G1 = 8         # guard elements on each side of a contiguous buffer


class Guarded:
    """a [rows, width] view (leading dimension ld) inside a [rows + 2G, ld] allocation, or a
    contiguous n-element view inside n + 2 G1 elements (ld = None)"""

    def __init__(self, dev, dtype, fill, rows, width=None, ld=None, guard=None, live=None):
        """guard: guard rows (2-D) / elements (contiguous) on each side, default G / G1.
        live: bool mask over the view's rows (2-D) or elements -- what a kernel may write; the rest of
        the view (the gaps between batch items) is guard like everything outside it"""
        self.ld = ld
        if ld is None:
            self.g = G1 if guard is None else guard
            self.alloc = torch.full((rows + 2 * self.g,), fill, dtype=dtype, device=dev)
            self.view = self.alloc[self.g:self.g + rows]
        else:
            self.g = G if guard is None else guard
            self.alloc = torch.full((rows + 2 * self.g, ld), fill, dtype=dtype, device=dev)
            self.view = self.alloc[self.g:self.g + rows, :width]
        self.live_mask = None if live is None else live.to(self.alloc.device)
        self.canary = self.alloc.clone()

    def set_canary(self):
        """the present contents (initial values written through the view) become the canary"""
        self.canary = self.alloc.clone()

    def unchanged(self):
        """an input: the whole allocation is bit-identical to the canary (set_canary after the fill)"""
        return torch.equal(self._bits(self.alloc), self._bits(self.canary))

    def live(self):
        """the elements a kernel may write (1-D when a live mask is set)"""
        return self.view if self.live_mask is None else self.view[self.live_mask]

    def _bits(self, t):
        return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])

    def refill(self):
        self.alloc.copy_(self.canary)

    def guards_intact(self):
        """everything outside the view is bit-identical to the canary"""
        a, c = self._bits(self.alloc).clone(), self._bits(self.canary).clone()
        g = self.g
        for t in (a, c):
            v = t[g:g + self.view.shape[0]] if self.ld is None else t[g:g + self.view.shape[0], :self.view.shape[1]]
            if self.live_mask is None:
                v.zero_()
            else:
                v[self.live_mask] = 0
        return torch.equal(a, c)


def guarded_input(dev, data, ld=None):
    """data (CPU) copied into a NaN-surrounded device buffer (integer data: 85-surrounded) -> the view"""
    if ld is None:
        g = Guarded(dev, data.dtype, float("nan") if data.is_floating_point() else 85, data.numel())
        g.view.copy_(data.reshape(-1))
        return g.view.view(data.shape)
    g = Guarded(dev, data.dtype, float("nan"), data.shape[0], data.shape[1], ld)
    g.view.copy_(data)
    return g.view


def inout_buf(dev, data, fill=NAN):
    """data (CPU or device) copied into a guarded buffer a kernel updates in place -> (Guarded, view)"""
    g = Guarded(dev, data.dtype, fill, data.numel())
    g.view.copy_(data.reshape(-1))
    return g, g.view.view(data.shape)


def out_buf(dev, dtype, *shape, fill=NAN, guard=None):
    n = 1
    for s in shape:
        n *= s
    g = Guarded(dev, dtype, fill, n, guard=guard)
    return g, g.view.view(*shape)


def check_written(bufs, fails, tag):
    for name, g in bufs.items():
        if not g.guards_intact():
            fails.append(f"{tag} {name}: a guard element was written")
        if not torch.isfinite(g.live().float()).all():
            fails.append(f"{tag} {name}: live region not finite (unwritten or poisoned)")


def probe_keep(k, dev, M, N, p, seed, batch=1):
    """the keep bits of the BIAS_DROP_RES epilogue, from the epilogue itself: A = 0 (K = 64),
    bias = 1, residual 0 -> C is exactly 1/(1-p) (kept) or 0 (dropped); [batch * M, N] bool"""
    A = torch.zeros(batch * M, 64, dtype=bf16, device=dev)
    Bm = torch.zeros(batch * N, 64, dtype=bf16, device=dev)
    bias = torch.ones(N, device=dev)
    Z = torch.zeros(batch * M, N, dtype=bf16, device=dev)
    C = torch.full((batch * M, N), NAN, dtype=bf16, device=dev)
    k.gemm(A, 64, True, Bm, 64, True, C, N, M, N, 64, batch=batch, sA=M * 64, sB=N * 64, sC=M * N,
           epi=k.epilogue(k.EPI_BIAS_DROP_RES, bias=bias, residual=Z, res_bstride=M * N, drop_p=p, seed=seed))
    kept = bf16_of(1.0 / (1.0 - p)) if p > 0 else 1.0
    assert ((C == 0) | (C.float() == kept)).all(), "probe GEMM: an output is neither 0 nor 1/(1-p)"
    return C != 0


def bf16_of(x):
    return torch.tensor(x, dtype=torch.float32).to(bf16).float().item()
