"""Ensemble diversity without a GPU: every refused call raises NativeError before anything is launched --
the library's own refusals (csrc/capi.hip mmu_ensemble_diversity: called with made-up non-null
addresses, which a refused call never touches) and the argument checks of the src/kernels.py wrapper
(CPU tensors: an acceptable call gets as far as the device check, "need tensors on a HIP", and no
further, as in test_uncertainty_decompose_refusals.py) -- plus the ABI version, the header's column
enum, and which C symbol the default paths name.
"""
import os
import re

import pytest
import torch

from src import _native as N
from src import kernels as K
from src._native import NativeError

f32, i32, i64 = torch.float32, torch.int32, torch.int64
z = torch.zeros
BASELINE = "HIP"
S, KM, T, C = 3, 3, 4, 10
NP = KM * (KM - 1) // 2
P = 64   # a made-up non-null address: refused calls do not dereference it
SYMBOL = "mmu_ensemble_diversity"


def capi(**over):
    a = dict(logits=P, ss=KM * T * C, sk=T * C, st=C, y=P, S=S, K=KM, T=T, C=C, top=5, mute=1, pair=P, counts=None,
             member_arg=P)
    a.update(over)
    N.call(SYMBOL, a["logits"], a["ss"], a["sk"], a["st"], a["y"], a["S"], a["K"], a["T"], a["C"], a["top"],
           a["mute"], a["pair"], a["counts"], a["member_arg"], None)


CAPI_REFUSALS = [
    (dict(logits=None), "logits is null"),
    (dict(y=None), "y is null"),
    (dict(pair=None), "pair is null"),
    (dict(member_arg=None), "member_arg is null"),
    (dict(S=0), "S = 0 must be positive"),
    (dict(S=-2), "S = -2 must be positive"),
    (dict(T=0), "T = 0 must be positive"),
    (dict(T=-1), "T = -1 must be positive"),
    (dict(C=0), "C = 0 must be positive"),
    (dict(C=1025, st=1025, sk=T * 1025, ss=KM * T * 1025), "C = 1025 exceeds 1024"),
    (dict(K=1), "K = 1 is fewer than the 2 members"),
    (dict(K=0), "K = 0 is fewer than the 2 members"),
    (dict(K=17, ss=17 * T * C), "K = 17 exceeds 16 members"),
    (dict(top=-1), "top = -1 must not be negative"),
    (dict(top=1025), "top = 1025 exceeds 1024"),
    (dict(mute=2), "mute_true = 2 must be 0 or 1"),
    (dict(mute=-1), "mute_true = -1 must be 0 or 1"),
    (dict(S=1 << 31, ss=KM * T * C), "S = 2147483648 exceeds the grid limit 2147483647"),
    (dict(st=C - 1), "st = 9 is smaller than the 10 elements the C axis"),
    (dict(st=0), "st = 0 is smaller"),
    (dict(st=-C), "st = -10 is smaller"),
    (dict(sk=T * C - 1), "sk = 39 is smaller than the 40 elements the st axis"),
    (dict(ss=KM * T * C - 1), "ss = 119 is smaller than the 120 elements the sk axis"),
    # [K, T, S, C] in place: ss = C, st = S * C, sk = T * S * C; each one short in turn
    (dict(ss=C - 1, st=S * C, sk=T * S * C), "ss = 9 is smaller than the 10 elements the C axis"),
    (dict(ss=C, st=S * C - 1, sk=T * S * C), "st = 29 is smaller than the 30 elements the ss axis"),
    (dict(ss=C, st=S * C, sk=T * S * C - 1), "sk = 119 is smaller than the 120 elements the st axis"),
    (dict(ss=C, st=C, sk=T * S * C), "is smaller than the 30 elements"),          # two axes on top of each other
]


@pytest.mark.parametrize("i", range(len(CAPI_REFUSALS)))
def test_library_refuses(i):
    over, msg = CAPI_REFUSALS[i]
    with pytest.raises(NativeError, match=SYMBOL + ": .*" + msg):
        capi(**over)


def test_library_still_reports_abi_4():
    assert N.load().mmu_version() == 4 and N.ABI_VERSION == 4
    assert SYMBOL in N.SIGNATURES


def test_column_names_follow_the_header_enum():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmu.h")
    enum = {name.lower(): int(v) for name, v in re.findall(r"\bMMU_DIV_(\w+) = (\d+)", open(header).read())}
    assert enum.pop("npair") == K.DIV_NPAIR == len(K.DIV_COLUMNS)
    assert enum == {name: i for i, name in enumerate(K.DIV_COLUMNS)}
    assert (K.DIV_MAX_MEMBERS, K.DIV_MAX_TOP) == (16, 1024)


def wrap(**over):
    a = dict(logits=z(S, KM, T, C), y=z(S, dtype=i64), pair=z(S, NP, 3), counts=z(S, NP, 4, dtype=i32),
             member_arg=z(S, KM, dtype=i32), top=5, mute_true=True)
    a.update(over)
    K.ensemble_diversity(a["logits"], a["y"], a["pair"], a["counts"], a["member_arg"], top=a["top"],
                         mute_true=a["mute_true"])


WRAP_REFUSALS = [
    (dict(logits=z(S, KM, T, C, dtype=torch.bfloat16)), "logits: expected torch.float32"),
    (dict(logits=z(S, KM, T, C, dtype=torch.float64)), "logits: expected torch.float32"),
    (dict(logits=z(S * KM * T, C)), "4-D .S, K, T, C. or 3-D"),
    (dict(logits=z(1, S, KM, T, C)), "4-D .S, K, T, C. or 3-D"),
    (dict(logits=z(S, KM, T, 2 * C)[..., ::2]), "class axis of logits must be contiguous"),
    (dict(logits=z(S, KM, C, T).transpose(2, 3)), "class axis of logits must be contiguous"),
    (dict(logits=z(S, 1, T, C), pair=z(S, 0, 3), counts=None, member_arg=z(S, 1, dtype=i32)), "K = 1 members, must be 2 .. 16"),
    (dict(logits=z(S, 17, T, C), pair=z(S, 136, 3), counts=None, member_arg=z(S, 17, dtype=i32)),
     "K = 17 members, must be 2 .. 16"),
    (dict(top=-1), "top = -1 must be an integer 0 .. 1024"),
    (dict(top=1025), "top = 1025 must be an integer 0 .. 1024"),
    (dict(top=5.0), "top = 5.0 must be an integer"),
    (dict(top=True), "top = True must be an integer"),
    (dict(mute_true=2), "mute_true = 2 must be a bool"),
    (dict(mute_true=None), "mute_true = None must be a bool"),
    (dict(y=z(S, dtype=torch.int32)), "y: expected torch.int64"),
    (dict(y=z(S + 1, dtype=i64)), "y must be contiguous int64"),
    (dict(y=z(2 * S, dtype=i64)[::2]), "y must be contiguous int64"),
    (dict(pair=None), "pair is required"),
    (dict(pair=z(S, NP, 3, dtype=torch.float64)), "pair: expected torch.float32"),
    (dict(pair=z(S, NP, 4)), "pair must be contiguous float32"),
    (dict(pair=z(S, NP + 1, 3)), "pair must be contiguous float32"),
    (dict(pair=z(S, NP, 6)[..., :3]), "pair must be contiguous float32"),
    (dict(counts=z(S, NP, 4)), "counts: expected torch.int32"),
    (dict(counts=z(S, NP, 4, dtype=i64)), "counts: expected torch.int32"),
    (dict(counts=z(S, NP, 3, dtype=i32)), "counts must be contiguous int32"),
    (dict(counts=z(S, 4, NP, dtype=i32).transpose(1, 2)), "counts must be contiguous int32"),
    (dict(member_arg=None), "member_arg is required"),
    (dict(member_arg=z(S, KM, dtype=i64)), "member_arg: expected torch.int32"),
    (dict(member_arg=z(S, KM + 1, dtype=i32)), "member_arg must be contiguous int32"),
    (dict(member_arg=z(KM, S, dtype=i32).t()), "member_arg must be contiguous int32"),
]


@pytest.mark.parametrize("i", range(len(WRAP_REFUSALS)))
def test_wrapper_refuses(i):
    over, msg = WRAP_REFUSALS[i]
    with pytest.raises(NativeError, match=msg):
        wrap(**over)


def test_wrapper_accepts_the_baseline():
    for over in (dict(), dict(counts=None), dict(top=0), dict(top=1024), dict(mute_true=False), dict(mute_true=0),
                 dict(logits=z(S, KM, C), ),                                      # the heads of a head model: T = 1
                 dict(logits=z(KM, T, S, C).permute(2, 0, 1, 3)),                # the ensemble's tensor in place
                 dict(logits=z(S, KM, T, C + 6)[..., :C]),                        # a padded pass stride
                 dict(logits=z(S, 16, T, C), pair=z(S, 120, 3), counts=z(S, 120, 4, dtype=i32),
                      member_arg=z(S, 16, dtype=i32))):
        with pytest.raises(NativeError, match=BASELINE):
            wrap(**over)


def test_the_wrapper_names_the_symbol_and_the_defaults_never_do(monkeypatch):
    """which C symbol each call names: the wrapper the new one (a 3-D stack as the T = 1 call, through its
    strides), the meters of the existing passes never"""
    from src.uncertainty import UncertaintyMeter
    calls = []
    monkeypatch.setattr(N, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(K, "_dev_check", lambda *ts: None)
    monkeypatch.setattr(K, "_stream", lambda t: None)
    monkeypatch.setattr(K, "ece_bins", lambda *a: None)
    wrap()
    lo = z(S, KM, C + 2)[..., :C]
    wrap(logits=lo, top=0, mute_true=False, counts=None)
    assert [c[0] for c in calls] == [SYMBOL] * 2
    a = calls[1][1]
    # (st belongs to an axis of extent 1, which never steps)
    assert a[1:3] == (KM * (C + 2), C + 2) and a[5:11] == (S, KM, 1, C, 0, 0) and a[12] is None
    assert calls[0][1][5:11] == (S, KM, T, C, 5, 1)
    del calls[:]
    UncertaintyMeter(15, decompose=True).update(z(KM, T, S, C), z(S, dtype=i64))
    K.uncertainty_decompose(z(S, KM, T, C), z(S, dtype=i64), z(S, K.UNC_NSTAT), z(S, C))
    K.robustness_summary(z(S, 5, 1, C), z(S, dtype=i64), z(S, K.ROB_NSTAT))
    assert calls and SYMBOL not in [c[0] for c in calls]
