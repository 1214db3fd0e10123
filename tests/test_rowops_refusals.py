"""The argument checks of the LayerNorm and embedding wrappers (src/kernels.py): every refused call
raises NativeError before anything is launched.  The checks read shapes and dtypes only, so the
tensors here live on the CPU: a call whose arguments are all acceptable gets as far as the device
check ("need tensors on a HIP") and no further -- that is the baseline of every refusal below.
"""
import pytest
import torch

from src import kernels as K
from src._native import NativeError

bf16, f32, i64 = torch.bfloat16, torch.float32, torch.int64
ROWS, H = 130, 512
BASELINE = "HIP"


def ln_args(**over):
    P = K.ln_parts(ROWS)
    a = dict(X=torch.zeros(ROWS, H, dtype=bf16), X32=torch.zeros(ROWS, H), w=torch.ones(H), b=torch.zeros(H),
             Y=torch.zeros(ROWS, H, dtype=bf16), Y32=torch.zeros(ROWS, H), mean=torch.zeros(ROWS),
             rstd=torch.zeros(ROWS), dY=torch.zeros(ROWS, H, dtype=bf16), dX=torch.zeros(ROWS, H, dtype=bf16),
             dXdrop=torch.zeros(ROWS, H, dtype=bf16), dRes=torch.zeros(ROWS, H, dtype=bf16),
             pdw=torch.zeros(P, H), pdb=torch.zeros(P, H), pdbias=torch.zeros(P, H), group_rows=0, param_stride=0)
    a.update(over)
    return a


def call_ln(which, a):
    if which == "fwd":
        K.layernorm_fwd(a["X"], a["w"], a["b"], a["Y"], a["mean"], a["rstd"], group_rows=a["group_rows"],
                        param_stride=a["param_stride"])
    elif which == "fwd_f32":
        K.layernorm_fwd_f32(a["X32"], a["w"], a["b"], a["Y"], a["Y32"], a["mean"], a["rstd"],
                            group_rows=a["group_rows"], param_stride=a["param_stride"])
    elif which == "bwd":
        K.layernorm_bwd(a["dY"], a["X"], a["mean"], a["rstd"], a["w"], a["dX"], a["dXdrop"], 0.1, 3, a["pdw"],
                        a["pdb"], a["pdbias"])
    elif which == "bwd_f32":
        K.layernorm_bwd(a["dY"], a["X32"], a["mean"], a["rstd"], a["w"], a["dX"], a["dXdrop"], 0.1, 3, a["pdw"],
                        a["pdb"], a["pdbias"])
    else:
        K.layernorm_bwd_res(a["dY"], a["X"], a["mean"], a["rstd"], a["w"], a["dRes"], a["dX"], a["pdw"], a["pdb"],
                            a["pdbias"])


LN_ALL = ("fwd", "fwd_f32", "bwd", "bwd_f32", "bwd_res")
z = torch.zeros
LN_REFUSALS = [
    # (wrappers, overrides, message)
    (("fwd", "bwd_res"), dict(X=z(ROWS, H)), "X: expected torch.bfloat16"),          # an f32 X read as bf16
    (("fwd_f32",), dict(X32=z(ROWS, H, dtype=bf16)), "X: expected torch.float32"),
    (("bwd",), dict(X=z(ROWS, H, dtype=torch.float16)), "X: expected"),
    (("fwd", "bwd"), dict(X=z(2, ROWS // 2, H, dtype=bf16)), "2-D"),
    (("fwd", "bwd"), dict(X=z(ROWS, 2 * H, dtype=bf16)[:, :H]), "contiguous"),
    (("fwd", "fwd_f32"), dict(Y=z(ROWS, H)), "Y: expected torch.bfloat16"),
    (("fwd", "fwd_f32"), dict(Y=z(ROWS - 1, H, dtype=bf16)), "Y must be contiguous"),
    (("fwd_f32",), dict(Y32=z(ROWS, H, dtype=bf16)), "Y32: expected torch.float32"),
    (("fwd_f32",), dict(Y32=z(ROWS, H + 256)), "Y32 must be contiguous"),
    (LN_ALL, dict(mean=z(ROWS - 1)), "mean must hold"),                              # a short mean is written past its end
    (LN_ALL, dict(rstd=z(ROWS - 1)), "rstd must hold"),
    (LN_ALL, dict(mean=z(ROWS, dtype=torch.float64)), "mean: expected torch.float32"),
    (LN_ALL, dict(w=z(H - 1)), "w must hold"),
    (LN_ALL, dict(w=z(H, dtype=bf16)), "w: expected torch.float32"),
    (("fwd", "fwd_f32"), dict(b=z(H - 1)), "b must hold"),
    (("fwd", "fwd_f32"), dict(group_rows=7), "no multiple of group_rows"),
    (("fwd", "fwd_f32"), dict(group_rows=65, param_stride=H), "w must hold"),         # 2 groups, 1 group of parameters
    (("fwd", "fwd_f32"), dict(group_rows=65, param_stride=-H), "param_stride"),
    (("bwd", "bwd_f32", "bwd_res"), dict(dY=z(ROWS, H)), "dY: expected torch.bfloat16"),
    (("bwd", "bwd_f32", "bwd_res"), dict(dY=z(ROWS + 1, H, dtype=bf16)), "dY must be contiguous"),
    (("bwd", "bwd_f32", "bwd_res"), dict(dX=z(ROWS, H)), "dX: expected torch.bfloat16"),
    (("bwd", "bwd_f32", "bwd_res"), dict(dX=z(ROWS, H - 256, dtype=bf16)), "dX must be contiguous"),
    (("bwd", "bwd_f32"), dict(dXdrop=z(ROWS, H)), "dXdrop: expected torch.bfloat16"),
    (("bwd", "bwd_f32"), dict(dXdrop=z(ROWS - 1, H, dtype=bf16)), "dXdrop must be contiguous"),
    (("bwd_res",), dict(dRes=z(ROWS, H)), "dRes: expected torch.bfloat16"),
    (("bwd_res",), dict(dRes=z(ROWS - 1, H, dtype=bf16)), "dRes must be contiguous"),
    (("bwd", "bwd_f32", "bwd_res"), dict(pdw=z(K.ln_parts(ROWS) - 1, H)), "part_dw must hold"),
    (("bwd", "bwd_f32", "bwd_res"), dict(pdb=z(K.ln_parts(ROWS) * H - 1)), "part_db must hold"),
    (("bwd", "bwd_f32", "bwd_res"), dict(pdbias=z(K.ln_parts(ROWS), H, dtype=bf16)), "part_dbias: expected"),
]


@pytest.mark.parametrize("which", LN_ALL)
def test_layernorm_wrappers_accept_the_baseline(which):
    with pytest.raises(NativeError, match=BASELINE):
        call_ln(which, ln_args())
    # optional outputs absent, grouped parameters with and without a stride
    with pytest.raises(NativeError, match=BASELINE):
        call_ln(which, ln_args(mean=None, rstd=None, Y32=None) if which.startswith("fwd") else
                ln_args(dXdrop=None, pdw=None, pdb=None, pdbias=None))
    if which.startswith("fwd"):
        with pytest.raises(NativeError, match=BASELINE):
            call_ln(which, ln_args(group_rows=65, param_stride=H, w=z(2 * H), b=z(2 * H)))
        with pytest.raises(NativeError, match=BASELINE):
            call_ln(which, ln_args(group_rows=13, param_stride=0))


@pytest.mark.parametrize("i", range(len(LN_REFUSALS)))
def test_layernorm_wrappers_refuse(i):
    whichs, over, msg = LN_REFUSALS[i]
    for which in whichs:
        with pytest.raises(NativeError, match=msg):
            call_ln(which, ln_args(**over))


# ------------------------------------------------------------------------------- embedding
B, T, NI, V, VOC, NPOS = 3, 5, 2, 2, 300, 512
S = NI + 2 + T
LO = S + 1


def emb_args(**over):
    a = dict(ids=z(B, T, dtype=i64), seg=z(B, T, dtype=i64), txt_mask=z(B, T, dtype=i64), proj=z(B, NI, 768),
             word=z(VOC, 768), pos=z(NPOS, 768), typ=z(2, 768), ln_w=z(768), ln_b=z(768), cls_id=101, sep_id=102,
             idx=z(V, LO, dtype=i64), V=V, B=B, T=T, n_img=NI, Lout=LO, X=z(V * B * LO, 768, dtype=bf16),
             X32=z(V * B * LO, 768), keymask=z(V * B, LO), mean=z(V * B * LO), rstd=z(V * B * LO),
             dX=z(B * S, 768, dtype=bf16), bmean=z(B * S), brstd=z(B * S), d_word=z(VOC, 768), d_pos=z(NPOS, 768),
             d_type=z(2, 768), d_ln_w=z(768), d_ln_b=z(768), d_proj=z(B, NI, 768))
    a.update(over)
    return a


def call_emb(which, a):
    if which == "fwd":
        K.embed_fwd(a["ids"], a["seg"], a["txt_mask"], a["proj"], a["word"], a["pos"], a["typ"], a["ln_w"], a["ln_b"],
                    1e-12, a["cls_id"], a["sep_id"], a["idx"], a["V"], a["B"], a["T"], a["n_img"], a["Lout"], a["X"],
                    a["keymask"], a["mean"], a["rstd"], X32=a["X32"])
    else:
        K.embed_bwd(a["dX"], a["ids"], a["seg"], a["proj"], a["word"], a["pos"], a["typ"], a["ln_w"], a["bmean"],
                    a["brstd"], a["cls_id"], a["sep_id"], a["B"], a["T"], a["n_img"], a["d_word"], a["d_pos"],
                    a["d_type"], a["d_ln_w"], a["d_ln_b"], a["d_proj"])


BOTH = ("fwd", "bwd")
EMB_REFUSALS = [
    (BOTH, dict(ids=z(B, T, dtype=torch.int32)), "ids: expected torch.int64"),
    (BOTH, dict(ids=z(B, T + 1, dtype=i64)), "ids must be contiguous int64"),
    (BOTH, dict(seg=z(B, T, dtype=torch.int32)), "seg: expected torch.int64"),
    (BOTH, dict(seg=z(B + 1, T, dtype=i64)), "seg must be contiguous int64"),
    (("fwd",), dict(txt_mask=z(B, T)), "txt_mask: expected torch.int64"),
    (("fwd",), dict(txt_mask=z(B * T, dtype=i64)), "txt_mask must be contiguous int64"),
    (BOTH, dict(proj=z(B, NI, 768, dtype=bf16)), "proj: expected torch.float32"),
    (BOTH, dict(proj=z(B, NI + 1, 768)), "proj must be contiguous f32"),
    (BOTH, dict(proj=z(B, NI, 2 * 768)[:, :, :768]), "proj must be contiguous f32"),
    (BOTH, dict(word=z(VOC, 512)), "word must be a contiguous f32"),
    (BOTH, dict(pos=z(NPOS, 768, dtype=bf16)), "pos: expected torch.float32"),
    (("fwd",), dict(X=z(V * B * LO, 768)), "X: expected torch.bfloat16"),
    (("fwd",), dict(X=z(V * B * LO - 1, 768, dtype=bf16)), "X must be contiguous"),
    (("fwd",), dict(X32=z(V * B * LO, 768, dtype=bf16)), "X32: expected torch.float32"),
    (("fwd",), dict(X32=z(B * LO, 768)), "X32 must be contiguous"),
    (("fwd",), dict(keymask=z(V * B * LO - 1)), "keymask must hold"),
    (("fwd",), dict(mean=z(V * B * LO - 1)), "mean must hold"),
    (("fwd",), dict(rstd=z(V * B * LO, dtype=torch.float64)), "rstd: expected torch.float32"),
    (("fwd",), dict(idx=z(V, LO, dtype=torch.int32)), "idx: expected torch.int64"),
    (("fwd",), dict(idx=z(V, LO - 1, dtype=i64)), "idx must be contiguous int64"),
    (BOTH, dict(pos=z(T - 1, 768)), "position rows"),
    (BOTH, dict(pos=z(NI + 1, 768), T=1, ids=z(B, 1, dtype=i64), seg=z(B, 1, dtype=i64),
                txt_mask=z(B, 1, dtype=i64)), "position rows"),
    (BOTH, dict(cls_id=VOC), "word rows"),
    (BOTH, dict(sep_id=VOC + 5), "word rows"),
    (BOTH, dict(typ=z(1, 768)), "token-type rows"),
    (BOTH, dict(ln_w=z(767)), "ln_w must hold"),
    (("fwd",), dict(ln_b=z(768, dtype=bf16)), "ln_b: expected torch.float32"),
    (("bwd",), dict(dX=z(B * S, 768)), "dX: expected torch.bfloat16"),
    (("bwd",), dict(dX=z(B * S + 1, 768, dtype=bf16)), "dX must be contiguous bf16"),
    (("bwd",), dict(bmean=z(B * S - 1)), "mean must hold"),
    (("bwd",), dict(brstd=z(B * S - 1)), "rstd must hold"),
    (("bwd",), dict(d_word=z(VOC - 1, 768)), "d_word must be contiguous f32"),
    (("bwd",), dict(d_pos=z(NPOS, 768, dtype=bf16)), "d_pos: expected torch.float32"),
    (("bwd",), dict(d_pos=z(S, 768)), "d_pos must be contiguous f32"),
    (("bwd",), dict(d_type=z(3, 768)), "d_type must be contiguous f32"),
    (("bwd",), dict(d_ln_w=z(1, 768)), "d_ln_w must be contiguous f32"),
    (("bwd",), dict(d_ln_b=z(769)), "d_ln_b must be contiguous f32"),
    (("bwd",), dict(d_proj=z(B, NI, 767)), "d_proj must be contiguous f32"),
]


@pytest.mark.parametrize("which", BOTH)
def test_embedding_wrappers_accept_the_baseline(which):
    with pytest.raises(NativeError, match=BASELINE):
        call_emb(which, emb_args())
    if which == "fwd":  # the identity variant without the optional outputs
        with pytest.raises(NativeError, match=BASELINE):
            call_emb(which, emb_args(idx=None, V=1, Lout=S, X=z(B * S, 768, dtype=bf16), X32=None, keymask=z(B, S),
                                     mean=None, rstd=None, txt_mask=None))


@pytest.mark.parametrize("i", range(len(EMB_REFUSALS)))
def test_embedding_wrappers_refuse(i):
    whichs, over, msg = EMB_REFUSALS[i]
    for which in whichs:
        with pytest.raises(NativeError, match=msg):
            call_emb(which, emb_args(**over))
