"""CPU: the stock open_clip configuration (causal text tower pooled at the EOT token, image tower with ln_pre and 'tok' pooling) on the
host side: config, attribute tree and state-dict contract against the reference-generated fixture (tests/golden/stock_tiny.npz, made
by tests/golden/make_golden_stock.py), what stays refused, and that OpenVision configs are as they were."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from openvision_amd import _lib, checkpoint, config as ovcfg, preset, synth
from openvision_amd.model import CLIP, LayerNorm, create_model

T = 77


def stock_cfg():
    """The fixture's model (make_golden_stock.config): CLIPVisionCfg / CLIPTextCfg defaults where OpenVision departs from them."""
    return {
        "embed_dim": 64,
        "vision_cfg": {"image_size": 64, "patch_size": 16, "width": 192, "head_width": 64, "layers": 2, "pool_type": "tok",
                       "no_ln_pre": False, "final_ln_after_pool": False},
        "text_cfg": {"context_length": T, "vocab_size": 1000, "width": 192, "heads": 3, "layers": 3, "pool_type": "argmax",
                     "no_causal_mask": False},
    }


@pytest.fixture(scope="module")
def g(gold):
    return gold("stock_tiny.npz")


def test_the_stock_text_config_is_accepted():
    t = ovcfg.text_cfg_from(stock_cfg()["text_cfg"])
    assert t.no_causal_mask is False and t.pool_type == "argmax"
    d = ovcfg.text_cfg_from({})                                  # CLIPTextCfg(): every LAION / DataComp ViT text tower
    assert d.no_causal_mask is False and d.pool_type == "argmax" and d.context_length == 77 and d.vocab_size == 49408
    v = ovcfg.vision_cfg_from({})                                # CLIPVisionCfg(): ln_pre, 'tok', ln_post before the pool
    assert v.no_ln_pre is False and v.pool_type == "tok" and v.final_ln_after_pool is False
    u = ovcfg.text_cfg_from({**stock_cfg()["text_cfg"], "no_causal_mask": True})     # EOT pooling without the mask
    assert u.no_causal_mask and u.pool_type == "argmax"


def test_what_stays_refused_says_so():
    c = stock_cfg()
    for key, val in (("embed_cls", True), ("proj_bias", True), ("ls_init_value", 1e-5), ("hf_model_name", "roberta-base")):
        with pytest.raises(ValueError, match=key):
            ovcfg.text_cfg_from({**c["text_cfg"], key: val})
    with pytest.raises(ValueError, match="pool_type"):
        ovcfg.text_cfg_from({**c["text_cfg"], "pool_type": "none"})
    with pytest.raises(ValueError, match="argmax"):              # the causal tower is built with the stock pooling only
        ovcfg.text_cfg_from({**c["text_cfg"], "pool_type": "last"})
    with pytest.raises(NotImplementedError, match="quick_gelu"):
        CLIP(c["embed_dim"], c["vision_cfg"], c["text_cfg"], quick_gelu=True)
    with pytest.raises(NotImplementedError, match="OpenAI"):
        create_model({**c, "quick_gelu": True})


def test_attribute_tree_keys_and_mask_against_the_reference(g):
    cfg = stock_cfg()
    sd = synth.make_state_dict(cfg)
    assert "visual.ln_pre.weight" in sd and "visual.ln_pre.bias" in sd
    m = create_model(cfg, state_dict=sd)                         # strict load
    assert sorted(m.state_dict().keys()) == [str(k) for k in g["keys"]] == sorted(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert "attn_mask" not in m.state_dict() and "attn_mask" in dict(m.named_buffers())
    assert m.attn_mask.dtype == torch.float32 and np.array_equal(m.attn_mask.numpy(), g["attn_mask"])
    mask = m.attn_mask
    assert tuple(mask.shape) == (T, T) and bool((mask.triu(1) == float("-inf"))[torch.ones(T, T).triu(1) > 0].all())
    assert bool((mask.tril() == 0).all())
    assert m.transformer.causal_prefix == 0 and m.visual.transformer.causal_prefix is None
    assert m.text_pool_type == "argmax" and m.context_length == T and m.vocab_size == 1000
    v = m.visual
    assert isinstance(v.ln_pre, LayerNorm) and v.pool_type == "tok" and v.final_ln_after_pool is False
    assert any(p is v.ln_pre.weight for p in v._lock_groups()[0])            # the embedding group of lock_image_tower holds ln_pre
    # the buffer follows .to() / .float(), and the text stack still knows it as its own
    m2 = m.to(torch.float32)
    assert m2.transformer._is_own_causal_mask(m2.attn_mask)
    assert not m2.transformer._is_own_causal_mask(m2.attn_mask.clone())
    assert not m2.transformer._is_own_causal_mask(m2.attn_mask[:10, :10])
    assert not m2.visual.transformer._is_own_causal_mask(m2.attn_mask)


def test_synth_draws_are_name_seeded_so_no_existing_tensor_moves():
    cfg = stock_cfg()
    sd = synth.make_state_dict(cfg)
    bare = dict(cfg, vision_cfg=dict(cfg["vision_cfg"], no_ln_pre=True))
    sd0 = synth.make_state_dict(bare)
    assert set(sd) - set(sd0) == {"visual.ln_pre.weight", "visual.ln_pre.bias"}
    for k in sd0:
        assert torch.equal(sd[k], sd0[k]), k
    tiny = preset("vit-tiny-patch16-160")
    assert len(synth.make_state_dict(tiny)) == 300               # the OpenVision key set (tests/test_host.py) is as it was


def test_openvision_presets_stay_unmasked():
    m = create_model(preset("vit-tiny-patch16-160"))
    assert m.attn_mask is None and m.transformer.causal_prefix is None and m.visual.transformer.causal_prefix is None
    assert m.text_pool_type == "last" and "attn_mask" not in m.state_dict()
    m.set_precision("fp8")                                       # still allowed there
    m.set_precision("bf16")


def test_fp8_is_refused_on_a_causal_model_and_points_at_the_image_tower():
    m = create_model(stock_cfg())
    for p in ("fp8", "fp8-mixed"):
        with pytest.raises(ValueError, match=r"model\.visual\.transformer\.set_precision"):
            m.set_precision(p)
    assert m.transformer._cache.precision == "bf16" and m.visual.transformer._cache.precision == "bf16"     # nothing half-applied
    m.set_precision("bf16")
    m.visual.transformer.set_precision("fp8")                    # the way the message names
    assert m.visual.transformer._cache.precision == "fp8" and m.transformer._cache.precision == "bf16"
    with pytest.raises(ValueError):
        m.set_precision("int4")


def test_a_foreign_mask_and_cpu_tensors_still_raise():
    m = create_model(stock_cfg())
    x = torch.zeros(1, T, 192)
    with pytest.raises(NotImplementedError, match="attn_mask"):
        m.transformer(x, attn_mask=m.attn_mask.clone())
    with pytest.raises(NotImplementedError, match="attn_mask"):
        m.visual.transformer(x, attn_mask=m.attn_mask)
    with pytest.raises(_lib.OvhipError):                         # the own mask is accepted; what stops it is the CPU tensor
        m.transformer(x, attn_mask=m.attn_mask)
    ov = create_model(preset("vit-tiny-patch16-160"))
    with pytest.raises(NotImplementedError):
        ov.transformer(torch.zeros(1, 80, 192), attn_mask=torch.zeros(80, 80))


def test_a_stock_config_directory_loads(tmp_path):
    cfg = stock_cfg()
    m = create_model(cfg, state_dict=synth.make_state_dict(cfg))
    d = str(tmp_path / "stock")
    checkpoint.save_pretrained(m, dict(cfg, quick_gelu=False), d, safetensors=False)
    m2, pp = checkpoint.from_pretrained(d, device=None)
    assert m2.transformer.causal_prefix == 0 and m2.text_pool_type == "argmax" and isinstance(m2.visual.ln_pre, LayerNorm)
    assert m2.visual.ln_pre.eps == 1e-6 and m2.ln_final.eps == 1e-6          # the vendored reference's default
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    up = dict(cfg, vision_cfg=dict(cfg["vision_cfg"], norm_kwargs={"eps": 1e-5}), text_cfg=dict(cfg["text_cfg"], norm_kwargs={"eps": 1e-5}))
    checkpoint.save_pretrained(m, up, d, safetensors=False)
    m3, _ = checkpoint.from_pretrained(d, device=None)
    assert m3.visual.ln_pre.eps == 1e-5 and m3.ln_final.eps == 1e-5 and m3.transformer.resblocks[0].ln_1.eps == 1e-5


def test_text_workspace_grows_for_argmax_only_and_bad_modes_are_invalid():
    lib = _lib.load()
    cfg = _lib.TowerCfg(192, 3, 3, 768, 768, 0, 1e-6)
    t = lib.ov_tower_create(C.byref(cfg))
    try:
        sizes = {}
        for mode in (0, 1, 2):
            head = _lib.TextHead(T, 1000, mode, 64, None, None, None, None, None)
            sizes[mode] = [lib.ov_text_workspace_bytes(t, C.byref(head), b) for b in (1, 3, 64, 65)]
        assert sizes[0] == sizes[1] and all(s > 0 for s in sizes[0])
        assert [a - b for a, b in zip(sizes[2], sizes[0])] == [256, 256, 256, 512]        # int32 [B], rounded up to 256 bytes
        for mode in (-1, 3):
            head = _lib.TextHead(T, 1000, mode, 64, None, None, None, None, None)
            assert lib.ov_text_workspace_bytes(t, C.byref(head), 3) == 0
            dummy = C.c_void_p(16)
            assert lib.ov_encode_text(t, C.byref(head), dummy, 3, dummy, 0, None, dummy, 1 << 30, None) == -1
        assert _lib.TEXT_POOL == {"first": 0, "last": 1, "argmax": 2}
    finally:
        lib.ov_tower_destroy(t)
    assert lib.ov_token_argmax(None, None, 1, 1, None) == -1
    assert lib.ov_gather_rows_at(None, 8, None, None, 8, 1, 1, 8, None) == -1
    addr = C.c_void_p(4096)
    assert lib.ov_gather_rows_at(addr, 12, addr, addr, 12, 1, 1, 12, None) == -1       # D % 8
    assert lib.ov_token_argmax(addr, addr, 0, 77, None) == -1 and lib.ov_token_argmax(addr, addr, 3, 0, None) == -1
