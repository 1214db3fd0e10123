"""CPU checks of tests/rowops_harness.py: the float32 rounding model alone meets every absolute
bar on every case of the LayerNorm and embedding sweeps (so the bars measure the kernels, not the
harness), the float64 embedding reference equals a plain nn.Embedding + F.layer_norm
construction, and the LayerNorm one equals F.layer_norm.  No kernel runs here.
"""
import pytest
import torch
import torch.nn.functional as F

import rowops_harness as R

EPS = 1e-12
# the model's own caps: a bf16 output within the elementwise bar, its row error at most the
# 2^-8 that bar implies; an f32 output within the f32 summation noise of its scale
ROW_CAP = R.BF16_REL + R.F32_NOISE


def _assert_bf16(name, out, ref, scale, elem=True):
    assert not elem or R.bf16_elem(out, ref, scale) <= 1.0, name
    assert R.rownorm(out, ref, scale).max().item() <= ROW_CAP, name


def _assert_f32(name, out, ref, scale):
    ek, _, _ = R.f32_stats(out, out, ref, scale)
    assert ek <= R.F32_NOISE, (name, ek)


@pytest.mark.parametrize("H", R.LN_H)
@pytest.mark.parametrize("kind", R.KINDS)
def test_ln_forward_model_meets_the_bars(H, kind):
    cases = [(rows, 1, 0, 0) for rows in R.LN_FWD_ROWS] + [(g * gr, g, gr, ps * H) for g, gr, ps in R.LN_FWD_GROUPED]
    for f32 in (False, True):
        for rows, groups, gr, ps in cases:
            X, w, b, _, _ = R.ln_inputs(rows, H, kind, seed=rows + H, groups=groups, param_stride=ps, f32=f32)
            ref, sc = R.ln_fwd_ref(X, w, b, EPS, gr, ps)
            m = R.ln_fwd_model(X, w, b, EPS, gr, ps)
            tag = f"{kind} H={H} rows={rows} groups={groups} f32={f32}"
            _assert_bf16(tag + " Y", m["Y"], ref["Y"], sc["Y"], kind in R.ELEM_KINDS)
            _assert_f32(tag + " Y32", m["Y32"], ref["Y"], sc["Y"])
            _assert_f32(tag + " mean", m["mean"], ref["mean"], sc["mean"])
            _assert_f32(tag + " rstd", m["rstd"], ref["rstd"], sc["rstd"])


@pytest.mark.parametrize("H", R.LN_H)
@pytest.mark.parametrize("kind", R.KINDS)
def test_ln_backward_model_meets_the_bars(H, kind):
    for f32 in (False, True):
        for rows in R.LN_BWD_ROWS:
            X, w, b, dY, dRes = R.ln_inputs(rows, H, kind, seed=3 * rows + H, f32=f32)
            fm = R.ln_fwd_model(X, w, b, EPS)
            keep = R.random_keep(rows, H, 0.1, seed=rows)
            for arm, kw in (("plain", {}), ("drop", {"keep": keep, "p": 0.1}), ("res", {"dRes": dRes})):
                ref, sc = R.ln_bwd_ref(dY, X, w, EPS, **kw)
                m = R.ln_bwd_model(dY, X, fm["mean"], fm["rstd"], w, **kw)
                tag = f"{kind} H={H} rows={rows} f32={f32} {arm}"
                _assert_bf16(tag + " dX", m["dX"], ref["dX"], sc["dX"])
                _assert_bf16(tag + " dXdrop", m["dXdrop"], ref["dXdrop"], sc["dXdrop"])
                if arm == "drop":
                    assert (m["dXdrop"][~keep] == 0).all()
                for k in ("pdw", "pdb", "pdbias"):
                    _assert_f32(f"{tag} {k}", m[k], ref[k], sc[k])


def test_ln_reference_is_layer_norm():
    X, w, b, dY, _ = R.ln_inputs(9, 768, "gauss", seed=1)
    ref, _ = R.ln_fwd_ref(X, w, b, EPS)
    x = X.double().requires_grad_(True)
    y = F.layer_norm(x, (768,), w.double(), b.double(), EPS)
    torch.testing.assert_close(ref["Y"], y.detach(), rtol=1e-12, atol=1e-12)
    (g,) = torch.autograd.grad(y, x, dY.double())
    bref, _ = R.ln_bwd_ref(dY, X, w, EPS)
    torch.testing.assert_close(bref["dX"], g, rtol=1e-12, atol=1e-12)
    # grouped parameters: group g of rows uses w[g * stride : g * stride + H]
    X, w, b, _, _ = R.ln_inputs(15, 256, "gauss", seed=2, groups=3, param_stride=256)
    ref, _ = R.ln_fwd_ref(X, w, b, EPS, 5, 256)
    for gi in range(3):
        y = F.layer_norm(X[5 * gi:5 * gi + 5].double(), (256,), w[256 * gi:256 * gi + 256].double(),
                         b[256 * gi:256 * gi + 256].double(), EPS)
        torch.testing.assert_close(ref["Y"][5 * gi:5 * gi + 5], y, rtol=1e-12, atol=1e-12)


def _plain_embedding(d, B, T, n_img, idx, V, Lout):
    """the reference's construction: nn.Embedding tables, [CLS] | image tokens | [SEP] with
    positions 0.. and token type 0 through one LayerNorm, the text through the same LayerNorm,
    concatenated, then the control gather"""
    H = d["word"].shape[1]
    word = torch.nn.Embedding.from_pretrained(d["word"].double())
    pos = torch.nn.Embedding.from_pretrained(d["pos"].double())
    typ = torch.nn.Embedding.from_pretrained(d["typ"].double())
    ln = lambda e: F.layer_norm(e, (H,), d["ln_w"].double(), d["ln_b"].double(), EPS)  # noqa: E731
    cls = word(torch.full((B, 1), d["cls_id"]))
    sep = word(torch.full((B, 1), d["sep_id"]))
    tok = torch.cat([cls, d["proj"].double(), sep], 1)
    img = ln(tok + pos(torch.arange(n_img + 2)).unsqueeze(0) + typ(torch.zeros(B, n_img + 2, dtype=torch.long)))
    txt = ln(word(d["ids"]) + pos(torch.arange(T)).unsqueeze(0) + typ(d["seg"]))
    full = torch.cat([img, txt], 1)
    km = torch.cat([torch.zeros(B, n_img + 2, dtype=torch.float64), (1.0 - d["txt_mask"].double()) * R.M10K], 1)
    if idx is None:
        return full.reshape(-1, H), km.reshape(-1)
    return torch.stack([full[:, idx[v]] for v in range(V)]).reshape(-1, H), \
        torch.stack([km[:, idx[v]] for v in range(V)]).reshape(-1)


@pytest.mark.parametrize("B,T,n_img", [(1, 1, 1), (3, 17, 3), (5, 2, 1)])
def test_embedding_reference_is_the_plain_construction(B, T, n_img):
    d = R.embed_inputs(B, T, n_img, seed=B + T)
    S = n_img + 2 + T
    args = (d["ids"], d["seg"], d["txt_mask"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"], d["ln_b"], EPS,
            d["cls_id"], d["sep_id"])
    ref, _ = R.embed_fwd_ref(*args, None, 1, B, T, n_img, S)
    X, km = _plain_embedding(d, B, T, n_img, None, 1, S)
    torch.testing.assert_close(ref["X"], X, rtol=1e-12, atol=1e-12)
    assert torch.equal(ref["keymask"], km)
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, S, (2, S + 3), generator=g)
    ref, _ = R.embed_fwd_ref(*args, idx, 2, B, T, n_img, S + 3)
    X, km = _plain_embedding(d, B, T, n_img, idx, 2, S + 3)
    torch.testing.assert_close(ref["X"], X, rtol=1e-12, atol=1e-12)
    assert torch.equal(ref["keymask"], km)


def _fwd_args(d, idx, V, B, T, n_img, Lout):
    return (d["ids"], d["seg"], d["txt_mask"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"], d["ln_b"], EPS,
            d["cls_id"], d["sep_id"], idx, V, B, T, n_img, Lout)


@pytest.mark.parametrize("n_img", R.EMBED_N_IMG)
@pytest.mark.parametrize("B,T", R.EMBED_FWD_SHAPES)
def test_embedding_forward_model_meets_the_bars(B, T, n_img):
    d = R.embed_inputs(B, T, n_img, seed=31 * B + T + n_img)
    for vname, idx, V, Lout in R.embed_fwd_variants(B, T, n_img):
        args = _fwd_args(d, idx, V, B, T, n_img, Lout)
        for drop in (False, True):
            pi, pt = (R.DROP_IMG, R.DROP_TXT) if drop else (0.0, 0.0)
            keep = R.random_keep(V * B * Lout, 768, 0.2, seed=B) if drop else None
            ref, sc = R.embed_fwd_ref(*args, keep=keep, drop_txt=pt, drop_img=pi)
            m = R.embed_fwd_model(*args, keep=keep, drop_txt=pt, drop_img=pi)
            tag = f"{vname} drop={drop} "
            _assert_bf16(tag + "X", m["X"], ref["X"], sc["X"])
            _assert_f32(tag + "X32", m["X32"], ref["X"], sc["X"])
            _assert_f32(tag + "mean", m["mean"], ref["mean"], sc["mean"])
            _assert_f32(tag + "rstd", m["rstd"], ref["rstd"], sc["rstd"])
            assert torch.equal(m["keymask"].double(), ref["keymask"])
            assert ((ref["keymask"] == 0) | (ref["keymask"] == R.M10K)).all()
            if drop:
                assert (m["X"][~keep] == 0).all()


@pytest.mark.parametrize("n_img", R.EMBED_N_IMG)
@pytest.mark.parametrize("B", R.EMBED_BWD_B)
def test_embedding_backward_model_meets_the_bars(B, n_img):
    for T in R.EMBED_BWD_T:
        S = n_img + 2 + T
        for ci, (ids_kind, seg_kind) in enumerate(R.EMBED_BWD_KINDS):
            d = R.embed_inputs(B, T, n_img, seed=13 * B + T + ci, ids_kind=ids_kind, seg_kind=seg_kind)
            g = torch.Generator().manual_seed(B + T)
            init = {k: torch.randn(t.shape, generator=g) * 0.1 for k, t in
                    zip(R.GRADS[:5], (d["word"], d["pos"], d["typ"], d["ln_w"], d["ln_b"]))}
            for drop in (True, False):
                pi, pt = (R.DROP_IMG, R.DROP_TXT) if drop else (0.0, 0.0)
                keep = R.random_keep(B * S, 768, 0.2, seed=B) if drop else None
                m = R.embed_fwd_model(*_fwd_args(d, None, 1, B, T, n_img, S), keep=keep, drop_txt=pt, drop_img=pi)
                bargs = (d["dX"], d["ids"], d["seg"], d["proj"], d["word"], d["pos"], d["typ"], d["ln_w"])
                for ini in (None, init):
                    bref, bsc = R.embed_bwd_ref(*bargs, d["ln_b"], EPS, d["cls_id"], d["sep_id"], B, T, n_img,
                                                keep=keep, drop_txt=pt, drop_img=pi, init=ini)
                    bm = R.embed_bwd_model(*bargs, m["mean"], m["rstd"], d["cls_id"], d["sep_id"], B, T, n_img,
                                           keep=keep, drop_txt=pt, drop_img=pi, init=ini)
                    for k in R.GRADS:
                        _assert_f32(f"T={T} {ids_kind} {seg_kind} drop={drop} init={ini is not None} {k}", bm[k],
                                    bref[k], bsc[k])
