"""The GEMM products of a bert-large layer (N = 1024, 3072, 4096 with K = 1024, 4096) with the
epilogues src/encoder.py gives them, through test_gemm_edges_gpu.py's run_case and gemm_harness'
float64 reference, float32 model and bars, unchanged: the first time these widths meet those
epilogues (the edge sweep's shapes stop at N = 768).

Token rows M = 130 (128^2 tiles, a 2-row last block) and M = 257 (256^2 and 256 x 384 tiles, a 1-row
last block):
* QKV (bias, bf16): N = 3072 on 256^2 and, with the wide rule's tile-count floor lowered, on 256 x 384;
* Wo and W2 (bias + dropout + residual into f32, the residual a LayerNorm recomputed in the
  epilogue, N = 1024);
* FFN1 (bias + GELU, gelu' to aux);
* dZ (DGELU with aux and the column sums);
* the W1 weight gradient dZ^T A (both operands M-major, accumulated into f32) over those rows, and
  over 1100 rows, where it is split along K.
"""
import pytest

import gemm_harness as H
from rowops_harness import Worst
from test_gemm_edges_gpu import K, run_case

pytestmark = pytest.mark.gpu

HID, FFN = 1024, 4096
ROWS = (130, 257)


def layer_cases(M):
    drop = dict(kind=H.BIAS_DROP_RES, c_f32=True, p=0.1, res_ln=True)
    return [
        H.case("large-qkv", M, 3 * HID, HID, kind=H.STORE),
        # the 256 x 384 tile under its own rule (N >= 2304, N % 384 == 0) at this test's tile count
        H.case("large-qkv-wide", M, 3 * HID, HID, kind=H.STORE, env={"MMU_GEMM_WIDE_MIN_TILES": "1"}),
        H.case("large-wo", M, HID, HID, **drop),
        H.case("large-ffn1", M, FFN, HID, kind=H.BIAS_GELU, aux=True, inp="offset"),
        H.case("large-w2", M, HID, FFN, **drop),
        H.case("large-dz", M, FFN, HID, kind=H.DGELU, colsum=True),
        H.case("large-wgrad", FFN, HID, M, c_f32=True, ak=False, bk=False, bias=False, accumulate=True),
    ]


@pytest.mark.parametrize("M", ROWS)
def test_bert_large_layer_products(dev, monkeypatch, M):
    k = K()
    fails, log, worst = [], [], Worst()
    cases = layer_cases(M)
    plans = {c["path"]: H.plan_of(c) for c in cases}
    assert plans["large-qkv-wide"]["tiling"] == ("wide" if M >= 256 else "small")
    assert plans["large-ffn1"]["tiling"] == ("big" if M >= 256 else "small")   # 4096 % 384 != 0: stays on 256^2
    for i, c in enumerate(cases):
        run_case(k, dev, monkeypatch, c, 1024 + 10 * M + i, fails, log, worst)
    print("\n".join(log))
    worst.report(f"gemm bert-large M={M}")
    assert not fails, "\n".join(fails[:40])


def test_bert_large_weight_gradient_split_along_k(dev, monkeypatch):
    c = H.case("large-wgrad-splitk", FFN, HID, 1100, c_f32=True, ak=False, bk=False, bias=False, accumulate=True)
    assert H.plan_of(c)["splitk"] > 1
    fails, log, worst = [], [], Worst()
    run_case(K(), dev, monkeypatch, c, 4096, fails, log, worst)
    print("\n".join(log))
    worst.report("gemm bert-large split-K weight gradient")
    assert not fails, "\n".join(fails[:40])
