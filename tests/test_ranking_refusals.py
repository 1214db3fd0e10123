"""The rank table without a GPU: every refused call raises NativeError before anything is launched -- the
library's own refusals (csrc/capi.hip mmu_rank_table: called with made-up non-null addresses, which a
refused call never touches) and the argument checks of the src/kernels.py wrapper (CPU tensors: an
acceptable call gets as far as the device check, "need tensors on a HIP", and no further) -- plus the ABI
version and which C symbol the new and the existing paths name.
"""
import numpy as np
import pytest
import torch

from src import _native as N
from src import kernels as K
from src._native import NativeError

f32, i32, i64, u8 = torch.float32, torch.int32, torch.int64, torch.uint8
z = torch.zeros
BASELINE = "HIP"
S, J = 6, 3
P = 64   # a made-up non-null address, 8-byte aligned: refused calls do not dereference it
SYMBOL = "mmu_rank_table"


def capi(**over):
    a = dict(x=P, ss=J, sj=1, group=P, S=S, J=J, rank=P, counts=P)
    a.update(over)
    N.call(SYMBOL, a["x"], a["ss"], a["sj"], a["group"], a["S"], a["J"], a["rank"], a["counts"], None)


CAPI_REFUSALS = [
    (dict(x=None), "x is null"),
    (dict(group=None), "group is null"),
    (dict(counts=None), "counts is null"),
    (dict(S=0), "S = 0 must be positive"),
    (dict(S=-3), "S = -3 must be positive"),
    (dict(J=0), "J = 0 must be positive"),
    (dict(J=-1), "J = -1 must be positive"),
    (dict(S=(1 << 20) + 1, ss=1, sj=(1 << 20) + 1), r"S = 1048577 exceeds 1048576 samples \(the sweep is O\(S\^2\)"),
    (dict(J=65536, ss=65536), "J = 65536 exceeds 65535 columns"),
    (dict(ss=0), "ss = 0 must be positive"),
    (dict(ss=-J), "ss = -3 must be positive"),
    (dict(sj=0), "sj = 0 must be positive"),
    (dict(sj=-1), "sj = -1 must be positive"),
    (dict(ss=1 << 61), "ss = 2305843009213693952 overflows"),
    # overlapping axes: the larger stride must clear extent x the smaller
    (dict(ss=J - 1, sj=1), "ss = 2 is smaller than the 3 elements the sj axis below it spans"),
    (dict(ss=1, sj=S - 1), "sj = 5 is smaller than the 6 elements the ss axis below it spans"),
    (dict(ss=2, sj=2 * S - 1), "sj = 11 is smaller than the 12 elements the ss axis"),
    (dict(ss=1, sj=1), "is smaller than the"),
    (dict(x=P + 2), "x is not 4-byte aligned"),
    (dict(x=P + 1), "x is not 4-byte aligned"),
    (dict(rank=P + 2), "rank is not 4-byte aligned"),
    (dict(counts=P + 4), "counts is not 8-byte aligned"),
    # precedence: the extents before the strides, the strides before the alignment
    (dict(S=0, ss=0, x=P + 1), "S = 0 must be positive"),
    (dict(ss=0, x=P + 1), "ss = 0 must be positive"),
]


@pytest.mark.parametrize("i", range(len(CAPI_REFUSALS)))
def test_library_refuses(i):
    over, msg = CAPI_REFUSALS[i]
    with pytest.raises(NativeError, match=SYMBOL + ": .*" + msg):
        capi(**over)


def test_a_stride_of_an_axis_that_never_steps_is_not_looked_at(monkeypatch):
    """extent 1: any stride passes the stride checks (the call then fails further on, at the alignment put
    there for the purpose), as torch reports arbitrary strides for such axes"""
    for over in (dict(S=1, ss=0), dict(S=1, ss=-5), dict(J=1, sj=0, ss=1), dict(J=1, sj=-7, ss=1),
                 dict(S=1, J=1, ss=0, sj=0)):
        with pytest.raises(NativeError, match="counts is not 8-byte aligned"):
            capi(counts=P + 4, **over)


def test_library_still_reports_abi_4():
    assert N.load().mmu_version() == 4 and N.ABI_VERSION == 4
    assert SYMBOL in N.SIGNATURES


def wrap(**over):
    a = dict(x=z(S, J), group=z(S, dtype=u8), rank=None, counts=None)
    a.update(over)
    return K.rank_table(a["x"], a["group"], rank=a["rank"], counts=a["counts"])


WRAP_REFUSALS = [
    (dict(x=z(S, J, dtype=torch.float64)), "x: expected torch.float32"),
    (dict(x=z(S, J, dtype=torch.bfloat16)), "x: expected torch.float32"),
    (dict(x=z(S)), "x must be a non-empty 2-D"),
    (dict(x=z(S, J, 1)), "x must be a non-empty 2-D"),
    (dict(x=z(0, J), group=z(0, dtype=u8)), "x must be a non-empty 2-D"),
    (dict(x=z(S, 0)), "x must be a non-empty 2-D"),
    (dict(x=z(1, 65536).expand(S, 65536)), "exceeds"),
    (dict(group=z(S, dtype=i64)), "group: expected torch.uint8"),
    (dict(group=z(S)), "group: expected torch.uint8"),
    (dict(group=z(S + 1, dtype=u8)), "group must be contiguous bool / uint8"),
    (dict(group=z(2 * S, dtype=u8)[::2]), "group must be contiguous bool / uint8"),
    (dict(group=z(S, 1, dtype=torch.bool)), "group must be contiguous bool / uint8"),
    (dict(rank=z(J, S, 4)), "rank: expected torch.int32"),
    (dict(rank=z(J, S, 4, dtype=i64)), "rank: expected torch.int32"),
    (dict(rank=z(S, J, 4, dtype=i32)), "rank must be contiguous int32"),
    (dict(rank=z(J, S, 5, dtype=i32)), "rank must be contiguous int32"),
    (dict(rank=z(J, 4, S, dtype=i32).transpose(1, 2)), "rank must be contiguous int32"),
    (dict(counts=z(J, 5, dtype=i32)), "counts: expected torch.int64"),
    (dict(counts=z(J, 4, dtype=i64)), "counts must be contiguous int64"),
    (dict(counts=z(5, J, dtype=i64).t()), "counts must be contiguous int64"),
]


@pytest.mark.parametrize("i", range(len(WRAP_REFUSALS)))
def test_wrapper_refuses(i):
    over, msg = WRAP_REFUSALS[i]
    with pytest.raises(NativeError, match=msg):
        wrap(**over)


def test_wrapper_accepts_the_baseline():
    for over in (dict(), dict(rank=True), dict(rank=z(J, S, 4, dtype=i32)), dict(counts=z(J, 5, dtype=i64)),
                 dict(group=z(S, dtype=torch.bool)),
                 dict(x=z(J, S).t()),                        # a [J, S] table in place
                 dict(x=z(S, J + 5)[:, :J]),                 # a padded row stride
                 dict(x=z(1, 1), group=z(1, dtype=u8))):
        with pytest.raises(NativeError, match=BASELINE):
            wrap(**over)


def test_the_wrapper_names_the_symbol_and_the_existing_meters_never_do(monkeypatch):
    """which C symbol each call names and with which strides; RelianceMeter, UncertaintyMeter.result() and
    uncertainty.auroc stay off the new symbol"""
    from src.robustness import RelianceMeter
    from src.uncertainty import UncertaintyMeter
    calls = []
    monkeypatch.setattr(N, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(K, "_dev_check", lambda *ts: None)
    monkeypatch.setattr(K, "_stream", lambda t: None)
    monkeypatch.setattr(K, "ece_bins", lambda *a: None)
    rank, counts = wrap()
    assert rank is None and counts.shape == (J, K.RANK_NCOUNT) and counts.dtype == i64
    rank, _ = wrap(x=z(J, S + 2)[:, :S].t(), rank=True)
    assert rank.shape == (J, S, K.RANK_NRANK) and rank.dtype == i32
    assert [c[0] for c in calls] == [SYMBOL] * 2
    assert calls[0][1][1:3] == (J, 1) and calls[0][1][4:6] == (S, J) and calls[0][1][6] is None
    assert calls[1][1][1:3] == (1, S + 2) and calls[1][1][6] == rank.data_ptr()
    del calls[:]
    RelianceMeter(1).update(z(S, 5, 4), z(S, dtype=i64))
    m = UncertaintyMeter(15, decompose=True)
    m.update(z(2, 3, S, 4), z(S, dtype=i64))
    assert calls and SYMBOL not in [c[0] for c in calls]
