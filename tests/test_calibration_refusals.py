"""Temperature scaling without a GPU: every refused call raises NativeError before anything is launched
-- the library's own refusals (csrc/capi.hip mmu_temperature_nll and mmu_uncertainty_decompose_scaled:
called with made-up non-null addresses, which a refused call never touches) and the argument checks of
the src/kernels.py wrappers (CPU tensors: an acceptable call gets as far as the device check, "need
tensors on a HIP", and no further, as in test_uncertainty_decompose_refusals.py) -- plus the ABI version
and the CPU side of test_temperature_nll_gpu.py's sweep: the float32 floor that sets the kernel's bar.
"""
import numpy as np
import pytest
import torch

from src import _native as N
from src import kernels as K
from src._native import NativeError

f32, f64, i64 = torch.float32, torch.float64, torch.int64
z = torch.zeros
BASELINE = "HIP"
S, KM, T, C, J = 3, 2, 4, 10, 5
P = 64   # a made-up non-null address: refused calls do not dereference it

# the stride refusals both symbols share with mmu_uncertainty_decompose
STRIDES = [
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
    (dict(ss=2 ** 62), "ss = 4611686018427387904 overflows"),
]
SHAPES = [
    (dict(logits=None), "logits is null"),
    (dict(y=None), "y is null"),
    (dict(S=0), "S = 0 must be positive"),
    (dict(S=-2), "S = -2 must be positive"),
    (dict(S=2 ** 31), "S = 2147483648 exceeds the grid limit"),
    (dict(K=0), "K = 0 must be positive"),
    (dict(T=0), "T = 0 must be positive"),
    (dict(T=-1), "T = -1 must be positive"),
    (dict(C=0), "C = 0 must be positive"),
    (dict(C=1025, st=1025, sk=T * 1025, ss=KM * T * 1025), "C = 1025 exceeds 1024"),
]


def capi_nll(**over):
    a = dict(logits=P, ss=KM * T * C, sk=T * C, st=C, y=P, S=S, K=KM, T=T, C=C, inv_temp=P, J=J, nll=P, nll_sum=None)
    a.update(over)
    N.call("mmu_temperature_nll", a["logits"], a["ss"], a["sk"], a["st"], a["y"], a["S"], a["K"], a["T"], a["C"],
           a["inv_temp"], a["J"], a["nll"], a["nll_sum"], None)


NLL_REFUSALS = SHAPES + [
    (dict(inv_temp=None), "inv_temp is null"),
    (dict(nll=None), "nll is null"),
    (dict(J=0), "J = 0 must be positive"),
    (dict(J=-1), "J = -1 must be positive"),
    (dict(J=65), "J = 65 exceeds 64 candidates"),
] + STRIDES


@pytest.mark.parametrize("i", range(len(NLL_REFUSALS)))
def test_temperature_nll_library_refuses(i):
    over, msg = NLL_REFUSALS[i]
    with pytest.raises(NativeError, match="mmu_temperature_nll: .*" + msg):
        capi_nll(**over)


def capi_scaled(**over):
    a = dict(logits=P, ss=KM * T * C, sk=T * C, st=C, y=P, S=S, K=KM, T=T, C=C, stats=P, p_bar=P, member_nll=None,
             inv_temp=P)
    a.update(over)
    N.call("mmu_uncertainty_decompose_scaled", a["logits"], a["ss"], a["sk"], a["st"], a["y"], a["S"], a["K"], a["T"],
           a["C"], a["stats"], a["p_bar"], a["member_nll"], a["inv_temp"], None)


SCALED_REFUSALS = SHAPES + [
    (dict(stats=None), "stats is null"),
    (dict(p_bar=None), "p_bar is null"),
    (dict(stats=None, inv_temp=None), "stats is null"),          # a null inv_temp is "all ones", not a refusal
] + STRIDES


@pytest.mark.parametrize("i", range(len(SCALED_REFUSALS)))
def test_decompose_scaled_library_refuses(i):
    over, msg = SCALED_REFUSALS[i]
    with pytest.raises(NativeError, match="mmu_uncertainty_decompose_scaled: .*" + msg):
        capi_scaled(**over)


def test_library_still_reports_abi_4():
    assert N.load().mmu_version() == 4 and N.ABI_VERSION == 4
    assert "mmu_temperature_nll" in N.SIGNATURES and "mmu_uncertainty_decompose_scaled" in N.SIGNATURES
    assert len(N.SIGNATURES["mmu_temperature_nll"][1]) == 14
    assert len(N.SIGNATURES["mmu_uncertainty_decompose_scaled"][1]) == len(N.SIGNATURES["mmu_uncertainty_decompose"][1]) + 1
    assert K.TEMPERATURE_MAX_CANDIDATES == 64


# ------------------------------------------------------------------------------- wrappers
ones = torch.ones


def wrap_nll(**over):
    a = dict(logits=z(S, KM, T, C), y=z(S, dtype=i64), inv_temp=ones(J, KM), nll=z(S, J), nll_sum=z(J, dtype=f64))
    a.update(over)
    K.temperature_nll(a["logits"], a["y"], a["inv_temp"], a["nll"], a["nll_sum"])


NLL_WRAP_REFUSALS = [
    (dict(logits=z(S, KM, T, C, dtype=torch.bfloat16)), "logits: expected torch.float32"),
    (dict(logits=z(S, KM, T, C, dtype=f64)), "logits: expected torch.float32"),
    (dict(logits=z(S, KM * T, C)), "4-D"),
    (dict(logits=z(S, KM, T, 2 * C)[..., ::2]), "class axis of logits must be contiguous"),
    (dict(logits=z(S, KM, C, T).transpose(2, 3)), "class axis of logits must be contiguous"),
    (dict(y=z(S, dtype=torch.int32)), "y: expected torch.int64"),
    (dict(y=z(S + 1, dtype=i64)), "y must be contiguous int64"),
    (dict(y=z(2 * S, dtype=i64)[::2]), "y must be contiguous int64"),
    (dict(inv_temp=None), "inv_temp must be a 2-D"),
    (dict(inv_temp=ones(KM)), "inv_temp must be a 2-D"),
    (dict(inv_temp=ones(J, KM, dtype=f64)), "inv_temp: expected torch.float32"),
    (dict(inv_temp=ones(J, KM + 1)), "inv_temp must be contiguous f32 .J, K."),
    (dict(inv_temp=ones(KM, J).t()), "inv_temp must be contiguous f32 .J, K."),
    (dict(inv_temp=ones(0, KM), nll=z(S, 0), nll_sum=z(0, dtype=f64)), "J = 0 candidates, must be 1 .. 64"),
    (dict(inv_temp=ones(65, KM), nll=z(S, 65), nll_sum=z(65, dtype=f64)), "J = 65 candidates, must be 1 .. 64"),
    (dict(inv_temp=torch.tensor([[1.0, -0.5]] * J)), "finite and >= 0"),
    (dict(inv_temp=torch.tensor([[1.0, float("nan")]] * J)), "finite and >= 0"),
    (dict(inv_temp=torch.tensor([[float("inf"), 1.0]] * J)), "finite and >= 0"),
    (dict(nll=None), "nll is required"),
    (dict(nll=z(S, J, dtype=f64)), "nll: expected torch.float32"),
    (dict(nll=z(S, J + 1)), "nll must be contiguous f32 .S, J."),
    (dict(nll=z(J, S).t()), "nll must be contiguous f32 .S, J."),
    (dict(nll_sum=z(J)), "nll_sum: expected torch.float64"),
    (dict(nll_sum=z(J + 1, dtype=f64)), "nll_sum must be contiguous f64 .J."),
    (dict(nll_sum=z(2 * J, dtype=f64)[::2]), "nll_sum must be contiguous f64 .J."),
]


@pytest.mark.parametrize("i", range(len(NLL_WRAP_REFUSALS)))
def test_temperature_nll_wrapper_refuses(i):
    over, msg = NLL_WRAP_REFUSALS[i]
    with pytest.raises(NativeError, match="temperature_nll: .*" + msg if "expected" not in msg else msg):
        wrap_nll(**over)


def test_temperature_nll_wrapper_accepts_the_baseline():
    for over in (dict(), dict(nll_sum=None),
                 dict(inv_temp=z(J, KM)),                                          # beta = 0 is allowed
                 dict(inv_temp=ones(1, KM), nll=z(S, 1), nll_sum=z(1, dtype=f64)),
                 dict(inv_temp=ones(64, KM), nll=z(S, 64), nll_sum=z(64, dtype=f64)),
                 dict(logits=z(KM, T, S, C).permute(2, 0, 1, 3)),                # the ensemble's tensor in place
                 dict(logits=z(S, KM, T, C + 6)[..., :C])):                       # a padded pass stride
        with pytest.raises(NativeError, match=BASELINE):
            wrap_nll(**over)


def wrap_scaled(**over):
    a = dict(logits=z(S, KM, T, C), y=z(S, dtype=i64), stats=z(S, K.UNC_NSTAT), p_bar=z(S, C), member_nll=z(S, KM),
             inv_temp=ones(KM))
    a.update(over)
    K.uncertainty_decompose(a["logits"], a["y"], a["stats"], a["p_bar"], a["member_nll"], inv_temp=a["inv_temp"])


SCALED_WRAP_REFUSALS = [
    (dict(inv_temp=ones(KM, dtype=f64)), "inv_temp: expected torch.float32"),
    (dict(inv_temp=ones(KM + 1)), "inv_temp must be contiguous f32 .K."),
    (dict(inv_temp=ones(1, KM)), "inv_temp must be contiguous f32 .K."),
    (dict(inv_temp=ones(2 * KM)[::2]), "inv_temp must be contiguous f32 .K."),
    (dict(inv_temp=torch.tensor([1.0, -1e-3])), "finite and >= 0"),
    (dict(inv_temp=torch.tensor([float("nan"), 1.0])), "finite and >= 0"),
    (dict(inv_temp=torch.tensor([1.0, float("inf")])), "finite and >= 0"),
    # and the checks in front of it are those of the unscaled call
    (dict(logits=z(S, KM * T, C)), "4-D"),
    (dict(stats=None), "stats is required"),
    (dict(p_bar=z(S, C - 1)), "p_bar must be contiguous f32"),
    (dict(member_nll=z(S, KM + 1)), "member_nll must be contiguous f32"),
]


@pytest.mark.parametrize("i", range(len(SCALED_WRAP_REFUSALS)))
def test_decompose_scaled_wrapper_refuses(i):
    over, msg = SCALED_WRAP_REFUSALS[i]
    with pytest.raises(NativeError, match=msg):
        wrap_scaled(**over)


def test_decompose_scaled_wrapper_accepts_the_baseline():
    for over in (dict(), dict(member_nll=None), dict(inv_temp=z(KM)), dict(inv_temp=None),
                 dict(logits=z(KM, T, S, C).permute(2, 0, 1, 3))):
        with pytest.raises(NativeError, match=BASELINE):
            wrap_scaled(**over)


def test_inv_temp_none_calls_the_old_symbol_and_a_tensor_the_new(monkeypatch):
    """the default path never reaches the new symbols: which C symbol each call names"""
    called = []
    monkeypatch.setattr(N, "call", lambda name, *a: called.append(name))
    monkeypatch.setattr(K, "_dev_check", lambda *ts: None)
    monkeypatch.setattr(K, "_stream", lambda t: None)
    wrap_scaled(inv_temp=None)
    K.uncertainty_decompose(z(S, KM, T, C), z(S, dtype=i64), z(S, K.UNC_NSTAT), z(S, C))
    assert called == ["mmu_uncertainty_decompose"] * 2
    wrap_scaled()
    wrap_nll()
    assert called[2:] == ["mmu_uncertainty_decompose_scaled", "mmu_temperature_nll"]


def test_a_table_is_read_back_once(monkeypatch):
    """the contents check synchronises the device, so the same tensor, unwritten since, is checked once: a
    meter passing one [K] tensor on every update pays for the first; a write or another tensor is checked"""
    reads = []
    real = torch.isfinite
    monkeypatch.setattr(torch, "isfinite", lambda t: reads.append(1) or real(t))
    t = ones(KM)
    for _ in range(3):
        with pytest.raises(NativeError, match=BASELINE):
            wrap_scaled(inv_temp=t)
    assert len(reads) == 1
    t[1] = -1.0                                                   # written in place: read again, and refused
    for _ in range(2):
        with pytest.raises(NativeError, match="finite and >= 0"):
            wrap_scaled(inv_temp=t)
    assert len(reads) == 3
    with pytest.raises(NativeError, match=BASELINE):
        wrap_scaled(inv_temp=ones(KM))
    with pytest.raises(NativeError, match=BASELINE):
        wrap_nll(inv_temp=ones(J, KM))
    assert len(reads) == 5


# ------------------------------------------------------------------------------- the sweep's CPU side
def test_sweep_floor_is_a_few_f32_roundings():
    """the yardstick of test_temperature_nll_gpu.py, computed here without a device.  The f32 evaluation
    rounds the exponent beta (z - m) (|.| up to some tens where the label still has p_y > 1e-12, at 6e-8
    relative) and the logarithm's result near 27.6 (ulp 1.9e-6): a floor between 1e-6 and 1e-5.  The fp64
    reference gives ln C at beta = 0 and -ln 1e-12 for the out-of-range label of every case."""
    import test_temperature_nll_gpu as G
    sw = G.sweep()
    assert len(sw["cases"]) == 9 * 4 * 3 * 4 + 1
    print(f"f32-numpy floor {sw['floor']:.3e}, bar {sw['bar']:.3e}")
    assert 1e-6 < sw["floor"] < 1e-5 and sw["bar"] == 4 * sw["floor"]
    for (C_, K_, T_, S_, scale), (zz, y, beta, r64) in sw["cases"].items():
        assert y[-1] == C_ and (y[:-1] < C_).all() and beta.shape == (64, K_) and beta.dtype == np.float32
        assert (beta[G.ONES] == 1).all() and (beta[G.ZEROS] == 0).all()
        assert (beta[:62] >= np.float32(0.05)).all() and (beta[:62] <= np.float32(20.0)).all()
        assert np.array_equal(r64[-1], np.full(64, -np.log(1e-12)))
        assert np.abs(r64[:-1, G.ZEROS] - np.log(C_)).max(initial=0.0) < 1e-12
        assert np.isfinite(r64).all()
    assert G.NLL_FLOOR == np.float32(27.631021)
