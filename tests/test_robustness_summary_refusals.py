"""The robustness summary without a GPU: every refused call raises NativeError before anything is
launched -- the library's own refusals (csrc/capi.hip mmu_robustness_summary: called with made-up
non-null addresses, which a refused call never touches) and the argument checks of the src/kernels.py
wrapper (CPU tensors: an acceptable call gets as far as the device check, "need tensors on a HIP", and
no further, as in test_uncertainty_decompose_refusals.py) -- plus what needs no device: the column
names against the header enum, the ABI version, and the fp64 reference of
test_robustness_summary_gpu.py (the top-two gap, float32 hits equal to fp64's, the JS range, the
floors that set the kernel's tolerance).
"""
import os
import re

import numpy as np
import pytest
import torch

from src import _native as N
from src import kernels as K
from src._native import NativeError

f32, i64 = torch.float32, torch.int64
z = torch.zeros
BASELINE = "HIP"
S, V, KH, C = 3, 7, 2, 10
P = 64   # a made-up non-null address: refused calls do not dereference it


def capi(**over):
    a = dict(logits=P, ss=V * KH * C, sv=KH * C, sk=C, y=P, S=S, V=V, K=KH, C=C, stats=P, per_variant=None)
    a.update(over)
    N.call("mmu_robustness_summary", a["logits"], a["ss"], a["sv"], a["sk"], a["y"], a["S"], a["V"], a["K"], a["C"],
           a["stats"], a["per_variant"], None)


CAPI_REFUSALS = [
    (dict(logits=None), "logits is null"),
    (dict(y=None), "y is null"),
    (dict(stats=None), "stats is null"),
    (dict(S=0), "S = 0 must be positive"),
    (dict(S=-2), "S = -2 must be positive"),
    (dict(K=0), "K = 0 must be positive"),
    (dict(K=-1), "K = -1 must be positive"),
    (dict(C=0), "C = 0 must be positive"),
    (dict(C=-3), "C = -3 must be positive"),
    (dict(V=3), "V = 3 is fewer than the 5 variants"),
    (dict(V=4), "V = 4 is fewer than the 5 variants"),
    (dict(V=0), "V = 0 is fewer than the 5 variants"),
    (dict(V=6), "V = 6 must be odd"),
    (dict(V=44), "V = 44 must be odd"),
    (dict(V=1025, ss=1025 * KH * C), "V = 1025 exceeds 1023"),
    (dict(C=1025, sk=1025, sv=KH * 1025, ss=V * KH * 1025), "C = 1025 exceeds 1024"),
    (dict(sk=C - 1), "sk = 9 is smaller than the 10 elements the C axis"),
    (dict(sk=0), "sk = 0 is smaller"),
    (dict(sk=-C), "sk = -10 is smaller"),
    (dict(sv=KH * C - 1), "sv = 19 is smaller than the 20 elements the sk axis"),
    (dict(ss=V * KH * C - 1), "ss = 139 is smaller than the 140 elements the sv axis"),
    # [V, S, K, C] in place: sk = C, ss = K * C, sv = S * K * C; each one short in turn
    (dict(sk=C - 1, ss=KH * C, sv=S * KH * C), "sk = 9 is smaller than the 10 elements the C axis"),
    (dict(sk=C, ss=KH * C - 1, sv=S * KH * C), "ss = 19 is smaller than the 20 elements the sk axis"),
    (dict(sk=C, ss=KH * C, sv=S * KH * C - 1), "sv = 59 is smaller than the 60 elements the ss axis"),
    (dict(sk=C, ss=C, sv=S * KH * C), "is smaller than the 30 elements"),          # two axes on top of each other
]


@pytest.mark.parametrize("i", range(len(CAPI_REFUSALS)))
def test_library_refuses(i):
    over, msg = CAPI_REFUSALS[i]
    with pytest.raises(NativeError, match="mmu_robustness_summary: .*" + msg):
        capi(**over)


def test_library_still_reports_abi_4():
    assert N.load().mmu_version() == 4 and N.ABI_VERSION == 4
    assert "mmu_robustness_summary" in N.SIGNATURES


def test_column_names_follow_the_header_enum():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmu.h")
    enum = {name.lower(): int(v) for name, v in re.findall(r"\bMMU_ROB_(\w+) = (\d+)", open(header).read())}
    assert enum.pop("nstat") == K.ROB_NSTAT == len(K.ROB_COLUMNS) == 16
    assert enum == {name: i for i, name in enumerate(K.ROB_COLUMNS)}


def wrap(**over):
    a = dict(logits=z(S, V, KH, C), y=z(S, dtype=i64), stats=z(S, K.ROB_NSTAT), per_variant=z(S, 3, V))
    a.update(over)
    K.robustness_summary(a["logits"], a["y"], a["stats"], a["per_variant"])


WRAP_REFUSALS = [
    (dict(logits=z(S, V, KH, C, dtype=torch.bfloat16)), "logits: expected torch.float32"),
    (dict(logits=z(S, V, KH, C, dtype=torch.float64)), "logits: expected torch.float32"),
    (dict(logits=z(S * V, C)), "4-D"),
    (dict(logits=z(S, V, KH, 1, C)), "4-D"),
    (dict(logits=z(S, V, KH, 2 * C)[..., ::2]), "class axis of logits must be contiguous"),
    (dict(logits=z(S, V, C, KH).transpose(2, 3)), "class axis of logits must be contiguous"),
    (dict(logits=z(S, V, 2 * C)[..., ::2]), "class axis of logits must be contiguous"),
    (dict(y=z(S, dtype=torch.int32)), "y: expected torch.int64"),
    (dict(y=z(S + 1, dtype=i64)), "y must be contiguous int64"),
    (dict(y=z(2 * S, dtype=i64)[::2]), "y must be contiguous int64"),
    (dict(stats=None), "stats is required"),
    (dict(stats=z(S, K.ROB_NSTAT, dtype=torch.float64)), "stats: expected torch.float32"),
    (dict(stats=z(S, K.ROB_NSTAT - 1)), "stats must be contiguous f32"),
    (dict(stats=z(S - 1, K.ROB_NSTAT)), "stats must be contiguous f32"),
    (dict(stats=z(S, 2 * K.ROB_NSTAT)[:, :K.ROB_NSTAT]), "stats must be contiguous f32"),
    (dict(per_variant=z(S, 3, V, dtype=torch.float64)), "per_variant: expected torch.float32"),
    (dict(per_variant=z(S, V, 3)), "per_variant must be contiguous f32"),
    (dict(per_variant=z(S, 3, V + 2)), "per_variant must be contiguous f32"),
    (dict(per_variant=z(S, V, 3).transpose(1, 2)), "per_variant must be contiguous f32"),
]


def test_wrapper_accepts_the_baseline():
    for over in (dict(), dict(per_variant=None),
                 dict(logits=z(S, V, C), per_variant=None),                       # a 3-D stack: K = 1
                 dict(logits=z(V, S, C).transpose(0, 1)),                         # robustness_logits' tensor in place
                 dict(logits=z(V, S, KH, C).permute(1, 0, 2, 3)),
                 dict(logits=z(S, V, KH, C + 6)[..., :C])):                       # a padded class stride
        with pytest.raises(NativeError, match=BASELINE):
            wrap(**over)


@pytest.mark.parametrize("i", range(len(WRAP_REFUSALS)))
def test_wrapper_refuses(i):
    over, msg = WRAP_REFUSALS[i]
    with pytest.raises(NativeError, match=msg):
        wrap(**over)


def test_wrapper_leaves_the_variant_count_to_the_library():
    """V is the library's to judge (test_library_refuses): the wrapper passes an even V on, so on the CPU
    such a call ends at the device check like any well-formed one"""
    with pytest.raises(NativeError, match=BASELINE):
        wrap(logits=z(S, 6, KH, C), per_variant=z(S, 3, 6))


def test_reference_of_the_gpu_sweep():
    """the fp64 reference of the GPU sweep, on the CPU: the top-two gap of the head-mean logits and the
    float32 hits equal to fp64's are asserted while the sweep is built; here the JS range, the exact
    zero of both std columns at n = 1, and the floors"""
    import test_robustness_summary_gpu as G
    assert G.COLUMNS == K.ROB_COLUMNS
    sw = G.sweep()
    assert len(sw["cases"]) == 9 * 4 * 3 * 2 * 4
    for (Cc, n, Kh, Ss, scale), (zz, y, r64) in sw["cases"].items():
        assert r64["js"].min() >= -1e-12 and r64["js"].max() <= G.LN2 + 1e-12, (Cc, n, Kh, Ss, scale)
        assert np.array_equal(r64["js"][:, 0], np.zeros(Ss))
        if n == 1:
            assert not r64["sd_image_control"].any() and not r64["sd_text_control"].any()
        if scale == 0:
            assert np.abs(r64["p_full"] - 1.0 / Cc).max() < 1e-15 and np.abs(r64["js"]).max() < 1e-12
    print("\ncolumn, f32-numpy floor")
    for c, v in sw["floor"].items():
        print(f"  {c:18s} {v:.3e}")
        assert np.isfinite(v)
        assert (v == 0.0) == (c in ("hit_full", "hit_image", "hit_text", "hit")), c
    assert all(v < 1e-5 for v in sw["floor"].values())
