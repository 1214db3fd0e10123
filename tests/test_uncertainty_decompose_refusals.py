"""The uncertainty decomposition without a GPU: every refused call raises NativeError before anything
is launched -- the library's own refusals (csrc/capi.hip mmu_uncertainty_decompose: called with
made-up non-null addresses, which a refused call never touches) and the argument checks of the
src/kernels.py wrapper (CPU tensors: an acceptable call gets as far as the device check, "need
tensors on a HIP", and no further, as in test_rowops_refusals.py) -- plus the host side that needs no
device: the ABI version, the new eval_robustness.py flags, the AUROC helper, and the fp64 reference of
test_uncertainty_decompose_gpu.py (Jensen's inequality, no near-ties in the sweep's data).
"""
import argparse

import numpy as np
import pytest
import torch

from src import _native as N
from src import kernels as K
from src._native import NativeError

f32, i64 = torch.float32, torch.int64
z = torch.zeros
BASELINE = "HIP"
S, KM, T, C = 3, 2, 4, 10
P = 64   # a made-up non-null address: refused calls do not dereference it


def capi(**over):
    a = dict(logits=P, ss=KM * T * C, sk=T * C, st=C, y=P, S=S, K=KM, T=T, C=C, stats=P, p_bar=P, member_nll=None)
    a.update(over)
    N.call("mmu_uncertainty_decompose", a["logits"], a["ss"], a["sk"], a["st"], a["y"], a["S"], a["K"], a["T"], a["C"],
           a["stats"], a["p_bar"], a["member_nll"], None)


CAPI_REFUSALS = [
    (dict(logits=None), "logits is null"),
    (dict(y=None), "y is null"),
    (dict(stats=None), "stats is null"),
    (dict(p_bar=None), "p_bar is null"),
    (dict(S=0), "S = 0 must be positive"),
    (dict(S=-2), "S = -2 must be positive"),
    (dict(K=0), "K = 0 must be positive"),
    (dict(T=0), "T = 0 must be positive"),
    (dict(T=-1), "T = -1 must be positive"),
    (dict(C=0), "C = 0 must be positive"),
    (dict(C=1025, st=1025, sk=T * 1025, ss=KM * T * 1025), "C = 1025 exceeds 1024"),
    (dict(st=C - 1), "st = 9 is smaller than the 10 elements the C axis"),
    (dict(st=0), "st = 0 is smaller"),
    (dict(st=-C), "st = -10 is smaller"),
    (dict(sk=T * C - 1), "sk = 39 is smaller than the 40 elements the st axis"),
    (dict(ss=KM * T * C - 1), "ss = 79 is smaller than the 80 elements the sk axis"),
    # [K, T, S, C] in place: ss = C, st = S * C, sk = T * S * C; each one short in turn
    (dict(ss=C - 1, st=S * C, sk=T * S * C), "ss = 9 is smaller than the 10 elements the C axis"),
    (dict(ss=C, st=S * C - 1, sk=T * S * C), "st = 29 is smaller than the 30 elements the ss axis"),
    (dict(ss=C, st=S * C, sk=T * S * C - 1), "sk = 119 is smaller than the 120 elements the st axis"),
    (dict(ss=C, st=C, sk=T * S * C), "is smaller than the 30 elements"),          # two axes on top of each other
]


@pytest.mark.parametrize("i", range(len(CAPI_REFUSALS)))
def test_library_refuses(i):
    over, msg = CAPI_REFUSALS[i]
    with pytest.raises(NativeError, match="mmu_uncertainty_decompose: .*" + msg):
        capi(**over)


def test_library_still_reports_abi_4():
    assert N.load().mmu_version() == 4 and N.ABI_VERSION == 4
    assert "mmu_uncertainty_decompose" in N.SIGNATURES


def test_column_names_follow_the_header_enum():
    import os
    import re
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmu.h")
    enum = {name.lower(): int(v) for name, v in re.findall(r"\bMMU_UNC_(\w+) = (\d+)", open(header).read())}
    assert enum.pop("nstat") == K.UNC_NSTAT == len(K.UNC_COLUMNS)
    assert enum == {name: i for i, name in enumerate(K.UNC_COLUMNS)}


def wrap(**over):
    a = dict(logits=z(S, KM, T, C), y=z(S, dtype=i64), stats=z(S, K.UNC_NSTAT), p_bar=z(S, C), member_nll=z(S, KM))
    a.update(over)
    K.uncertainty_decompose(a["logits"], a["y"], a["stats"], a["p_bar"], a["member_nll"])


WRAP_REFUSALS = [
    (dict(logits=z(S, KM, T, C, dtype=torch.bfloat16)), "logits: expected torch.float32"),
    (dict(logits=z(S, KM, T, C, dtype=torch.float64)), "logits: expected torch.float32"),
    (dict(logits=z(S, KM * T, C)), "4-D"),
    (dict(logits=z(S, KM, T, 2 * C)[..., ::2]), "class axis of logits must be contiguous"),
    (dict(logits=z(S, KM, C, T).transpose(2, 3)), "class axis of logits must be contiguous"),
    (dict(y=z(S, dtype=torch.int32)), "y: expected torch.int64"),
    (dict(y=z(S + 1, dtype=i64)), "y must be contiguous int64"),
    (dict(y=z(2 * S, dtype=i64)[::2]), "y must be contiguous int64"),
    (dict(stats=None), "stats is required"),
    (dict(stats=z(S, K.UNC_NSTAT, dtype=torch.float64)), "stats: expected torch.float32"),
    (dict(stats=z(S, K.UNC_NSTAT - 1)), "stats must be contiguous f32"),
    (dict(stats=z(S - 1, K.UNC_NSTAT)), "stats must be contiguous f32"),
    (dict(stats=z(S, 2 * K.UNC_NSTAT)[:, :K.UNC_NSTAT]), "stats must be contiguous f32"),
    (dict(p_bar=None), "p_bar is required"),
    (dict(p_bar=z(S, C, dtype=torch.bfloat16)), "p_bar: expected torch.float32"),
    (dict(p_bar=z(S, C - 1)), "p_bar must be contiguous f32"),
    (dict(p_bar=z(C, S).t()), "p_bar must be contiguous f32"),
    (dict(member_nll=z(S, KM, dtype=torch.float64)), "member_nll: expected torch.float32"),
    (dict(member_nll=z(S, KM + 1)), "member_nll must be contiguous f32"),
    (dict(member_nll=z(S, T)), "member_nll must be contiguous f32"),
]


def test_wrapper_accepts_the_baseline():
    for over in (dict(), dict(member_nll=None),
                 dict(logits=z(KM, T, S, C).permute(2, 0, 1, 3)),                # the ensemble's tensor in place
                 dict(logits=z(S, KM, T, C + 6)[..., :C])):                       # a padded pass stride
        with pytest.raises(NativeError, match=BASELINE):
            wrap(**over)


@pytest.mark.parametrize("i", range(len(WRAP_REFUSALS)))
def test_wrapper_refuses(i):
    over, msg = WRAP_REFUSALS[i]
    with pytest.raises(NativeError, match=msg):
        wrap(**over)


# ------------------------------------------------------------------------------- host side
def test_meter_default_is_unchanged_and_checks_its_layout():
    from src.uncertainty import UncertaintyMeter
    m = UncertaintyMeter()
    assert (m.n_bins, m.decompose) == (15, False)
    with pytest.raises(NativeError, match=BASELINE):                  # the existing kernel's wrapper
        m.update(z(S, KM * T, C), z(S, dtype=i64))
    d = UncertaintyMeter(15, decompose=True)
    with pytest.raises(ValueError, match="layout"):
        d.update(z(S, KM * T, C), z(S, dtype=i64))
    with pytest.raises(ValueError, match="layout"):
        d.update(z(KM, T, S, C), z(S, dtype=i64), layout="BKTC")
    for lo, layout in ((z(KM, T, S, C), "KTBC"), (z(S, KM, T, C), "SKTC")):
        with pytest.raises(NativeError, match=BASELINE):
            d.update(lo, z(S, dtype=i64), layout=layout)


def test_ensemble_refuses_an_unknown_variant():
    from src.uncertainty import EnsembleMMBT
    ens = EnsembleMMBT.__new__(EnsembleMMBT)
    ens.members = [argparse.Namespace(enc=argparse.Namespace(n_img=3))]
    assert ens.variant_indices("img_only", 7).tolist() == [0, 1, 2, 3, 4]
    assert ens.variant_indices("txt_only", 3).tolist() == [0, 5, 6, 7]
    torch.manual_seed(5)
    a = ens.variant_indices(("control", "image"), 7)
    torch.manual_seed(5)
    from src.mmbt import control_indices
    assert torch.equal(a, control_indices(12, 4)) and a.numel() == 5 and a[0] == 0
    assert ens.variant_indices(("control", "text"), 7).numel() == 8
    with pytest.raises(ValueError, match="variant"):
        ens.variant_indices("audio_only", 7)
    with pytest.raises(ValueError, match="variant"):
        ens.variant_indices(("control", "audio"), 7)


def parse(argv):
    import eval_robustness as E
    p = argparse.ArgumentParser()
    E.get_args(p)
    return p.parse_args(["--save_path", "out"] + argv)


def test_flags_parse_and_default():
    import eval_robustness as E
    a = parse([])
    assert a.decompose is False and a.variants == ["full"]
    a = parse(["--mmbt", "--decompose"])
    assert a.decompose is True and a.variants == ["full"]
    every = ["full", "img_only", "txt_only", "control_image", "control_text"]
    a = parse(["--mmbt", "--decompose", "--variants"] + every)
    assert a.variants == every
    assert parse(["--variants", "txt_only", "control_text"]).variants == ["txt_only", "control_text"]
    with pytest.raises(SystemExit):
        parse(["--variants", "audio_only"])
    assert E.VARIANTS == {"img_only": "img_only", "txt_only": "txt_only", "control_image": ("control", "image"),
                          "control_text": ("control", "text")}
    assert set(E.VARIANTS) | {"full"} == set(every)


def brute_auroc(score, pos):
    """P(score of a positive > score of a negative) + P(equal) / 2, by counting every pair"""
    n = d = 0.0
    for sp, pp in zip(score, pos):
        for sn, pn in zip(score, pos):
            if pp and not pn:
                d += 1
                n += 1.0 if sp > sn else (0.5 if sp == sn else 0.0)
    return n / d


def test_auroc_equals_pair_counting():
    from src.uncertainty import auroc
    g = np.random.default_rng(3)
    for n, levels in ((2, 2), (5, 3), (17, 4), (40, 6), (64, 1000)):
        for _ in range(5):
            score = g.integers(0, levels, n) / 7.0                    # few levels: many ties
            pos = g.integers(0, 2, n).astype(bool)
            pos[0], pos[1] = True, False
            assert abs(auroc(score, pos) - brute_auroc(score, pos)) < 1e-12
    assert auroc([0.1, 0.2, 0.3, 0.4], [0, 0, 1, 1]) == 1.0
    assert auroc([0.1, 0.2, 0.3, 0.4], [1, 1, 0, 0]) == 0.0
    assert auroc([1.0, 1.0, 1.0], [1, 0, 0]) == 0.5
    assert auroc([0.3, 0.1, 0.2], [1, 1, 1]) is None
    assert auroc([0.3, 0.1, 0.2], [0, 0, 0]) is None


def test_reference_has_no_near_ties_and_obeys_jensen():
    """the fp64 reference of the GPU sweep, on the CPU: both mutual-information parts >= -1e-12, every
    row's top-two gap >= 1e-3 in probability (asserted while the sweep is built), and the f32-numpy
    floor that sets the kernel's tolerance is where it was measured (2.4e-6 on mi_passes, 4e-7 on brier)"""
    import test_uncertainty_decompose_gpu as G
    assert G.COLUMNS == K.UNC_COLUMNS                       # the reference's columns are the header's
    sw = G.sweep()
    assert len(sw["cases"]) == 9 * 4 * 3 * 4
    for case, (_, _, r64, _) in sw["cases"].items():
        assert r64["mi_members"].min() >= -1e-12 and r64["mi_passes"].min() >= -1e-12, case
    assert 1e-6 < sw["floor"]["mi_passes"] < 5e-6 and 1e-7 < sw["floor"]["brier"] < 1e-6
    assert sw["floor"]["correct"] == 0.0
