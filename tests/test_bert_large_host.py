"""bert-large-uncased (1024 hidden, 16 heads, 4096 intermediate, 24 layers), host side (no GPU):
the shape table and its refusals (src/mmbt.py _bert_shape), the oracle at that width against
transformers' own BertEncoder (the ruler of tests/test_bert_large_gpu.py, not the feature), and the
width-taking embedding-backward workspace query (include/mmu.h mmu_embed_bwd_ws_floats_h)."""
import pytest
import torch

from oracle.weights import MMBTConfig

WIDE_SMALL = MMBTConfig(n_layers=2, hidden=1024, heads=16, inter=4096, vocab=4096, resnet_blocks=(1, 1, 1, 1))


def test_bert_shape_accepts_large_and_names_the_width_to_pass():
    from src.mmbt import _bert_shape
    from src.testing import make_args, small_args
    base = (12, 768, 12, 3072, 30522, 512, 2)
    large = (24, 1024, 16, 4096, 30522, 512, 2)
    assert _bert_shape(make_args()) == base  # bert-base: as before
    assert _bert_shape(small_args()) == (2, 768, 12, 3072, 4096, 512, 2)
    assert _bert_shape(make_args(bert_model="bert-large-uncased", hidden_sz=1024)) == large
    # the overrides the small test models use keep working at the new width
    assert _bert_shape(small_args(bert_model="bert-large-uncased", hidden_sz=1024)) == (2, 1024, 16, 4096, 4096, 512, 2)
    with pytest.raises(NotImplementedError, match="1024"):
        _bert_shape(make_args(bert_model="bert-large-uncased", hidden_sz=768))
    with pytest.raises(NotImplementedError, match="768"):
        _bert_shape(make_args(bert_model="bert-base-uncased", hidden_sz=1024))
    with pytest.raises(NotImplementedError, match="bert-large-uncased"):  # the refusal lists what is built
        _bert_shape(make_args(bert_model="bert-base-cased"))


def test_oracle_encoder_at_1024_matches_transformers():
    """oracle.mmbt_ref.encoder at WIDE_SMALL against transformers' BertEncoder (eager attention,
    dropout 0) holding the same seeded weights: B = 2, L = 21, keys 12.. of sample 1 masked.
    Bar: max abs <= 1e-5 x max|ref| (two f32 evaluations that differ in summation order; measured
    3e-7 of scale)."""
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertEncoder
    from oracle import mmbt_ref as R
    from oracle.weights import make_state_dict
    cfg = WIDE_SMALL
    sd = make_state_dict(0, cfg)
    hf_cfg = BertConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.n_layers,
                        num_attention_heads=cfg.heads, intermediate_size=cfg.inter, hidden_act="gelu",
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, layer_norm_eps=cfg.ln_eps,
                        max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab)
    hf_cfg._attn_implementation = "eager"
    enc = BertEncoder(hf_cfg).eval()
    missing = enc.load_state_dict({k[len(R.ENC):]: v for k, v in sd.items() if k.startswith(R.ENC)}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    B, L = 2, 21
    g = torch.Generator().manual_seed(1024)
    x = torch.randn(B, L, cfg.hidden, generator=g)
    m = torch.ones(B, L, dtype=torch.long)
    m[1, 12:] = 0
    ext = R.extended_mask(m)
    with torch.no_grad():
        ours = R.encoder(sd, x, ext, cfg)
        ref = enc(x, attention_mask=ext)[0]
    err, scale = (ours - ref).abs().max().item(), ref.abs().max().item()
    print(f"oracle encoder vs transformers BertEncoder at 1024 / 16 / 4096 x 2: max abs {err:.3e} on a {scale:.2f} scale "
          f"({err / scale:.1e} of scale)")
    assert err <= 1e-5 * scale


@pytest.fixture()
def lib():
    from src import _native
    lib = _native.load()  # (loads without a GPU)
    prev = lib.mmu_get_deterministic()
    yield lib
    lib.mmu_set_deterministic(prev)


@pytest.mark.parametrize("B,T,n_img", [(1, 1, 1), (17, 9, 3), (33, 17, 1)])
def test_embed_bwd_workspace_by_width(lib, B, T, n_img):
    nby, S = (B + 15) // 16, n_img + 2 + T
    for mode in (0, 1):
        lib.mmu_set_deterministic(mode)
        assert lib.mmu_embed_bwd_ws_floats_h(B, T, n_img, 768) == lib.mmu_embed_bwd_ws_floats(B, T, n_img)
        assert lib.mmu_embed_bwd_ws_floats_h(B, T, n_img, 512) < 0  # a width mmu_embed_bwd refuses
    lib.mmu_set_deterministic(0)
    off = lib.mmu_embed_bwd_ws_floats_h(B, T, n_img, 1024)
    assert off == 4 * ((S + 3) // 4) * nby * 1024  # the [4, blocks, H] partial rows
    lib.mmu_set_deterministic(1)
    on = lib.mmu_embed_bwd_ws_floats_h(B, T, n_img, 1024)
    lib.mmu_set_deterministic(0)
    assert lib.mmu_embed_bwd_ws_floats_h(B, T, n_img, 1024) == off
    assert on >= off + (B * T + nby * S) * 1024


def test_abi_version_unchanged_by_the_new_symbol(lib):
    from src import _native
    assert lib.mmu_version() == 4 == _native.ABI_VERSION


@pytest.mark.parametrize("entry", ["train", "eval_mmbt_robustness", "eval_robustness"])
def test_entry_points_take_the_bert_large_flags(entry):
    """each command line parses `--bert_model bert-large-uncased --hidden_sz 1024`, and the namespace
    it builds the model from passes _bert_shape (eval_robustness.py --mmbt builds its own)"""
    import argparse
    import importlib
    from src.mmbt import _bert_shape
    from src.testing import _Vocab
    mod = importlib.import_module(entry)
    parser = argparse.ArgumentParser()
    mod.get_args(parser)
    argv = ["--save_path", "x", "--bert_model", "bert-large-uncased", "--hidden_sz", "1024"]
    argv += {"eval_robustness": ["--mmbt"], "train": [],
             "eval_mmbt_robustness": ["--phase", "val", "--batch_size", "4", "--checkpoint_path", "x"]}[entry]
    args, remaining = parser.parse_known_args(argv)
    assert remaining == []
    if entry == "eval_robustness":
        margs = mod.mmbt_model_args(args, 101, _Vocab())
        assert _bert_shape(mod.mmbt_model_args(parser.parse_args(["--save_path", "x", "--mmbt"]), 101, _Vocab()))[1] == 768
        args.hidden_sz = 768  # the mismatch is refused with advice this command line accepts
        with pytest.raises(NotImplementedError, match="--hidden_sz 1024"):
            _bert_shape(mod.mmbt_model_args(args, 101, _Vocab()))
    else:
        margs = args
    assert _bert_shape(margs) == (24, 1024, 16, 4096, 30522, 512, 2)
