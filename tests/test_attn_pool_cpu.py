"""CPU: attentional pooling below the kernels -- the config keys, the module tree and its state-dict names in both layouts of
nn.MultiheadAttention against the reference-generated fixture tests/golden/attnpool_tiny.npz (tests/golden/make_golden_attnpool.py),
the synthetic weights, locking, weight decay, and the new kernels' build (no scratch, no early inline-asm read of an MFMA result).
On the parent commit the config raises on ``attentional_pool=True``."""
import re

import numpy as np
import pytest
import torch

from openvision_amd import config as ovcfg, synth, training
from openvision_amd.config import preset
from openvision_amd.model import AttentionalPooler, create_model
from oracle import clip_ref as R
from conftest import golden
from test_stock_cpu import stock_cfg
from test_build_scratch import device_asm, inline_asm_mfma_hazards, kernel_scratch

T, VOCAB = 32, 1000
WEIGHTS = {"a": ("sharp", 28), "b": ("v1", 39)}            # make_golden_attnpool.WEIGHTS (also stored in the fixture)


def pool_cfg(which):
    """The fixture's two models (make_golden_attnpool.config): a = separate q / k / v weights, 'tok'; b = packed in_proj_weight, 'avg'."""
    wide = which == "a"
    return {
        "embed_dim": 64,
        "vision_cfg": {"image_size": 64, "patch_size": 16, "width": 192 if wide else 64, "head_width": 64, "layers": 2,
                       "pool_type": "tok" if wide else "avg", "no_ln_pre": False, "final_ln_after_pool": False,
                       "attentional_pool": True, "attn_pooler_queries": 5, "attn_pooler_heads": 2},
        "text_cfg": {"context_length": T, "vocab_size": VOCAB, "width": 128, "heads": 2, "layers": 2, "pool_type": "last",
                     "no_causal_mask": True, "act_kwargs": {"approximate": "tanh"}},
    }


def pool_state_dict(which):
    variant, seed = WEIGHTS[which]
    return synth.make_state_dict(pool_cfg(which), seed, variant)


@pytest.fixture(scope="module")
def g():
    return golden("attnpool_tiny.npz")


def test_config_accepts_the_bool_form_and_refuses_the_rest():
    v = pool_cfg("a")["vision_cfg"]
    c = ovcfg.vision_cfg_from(v, 64)
    assert c.attentional_pool is True and c.attn_pooler_queries == 5 and c.attn_pooler_heads == 2
    d = ovcfg.vision_cfg_from({k: x for k, x in v.items() if not k.startswith("attn_pooler")} | {"attentional_pool": True})
    assert d.attn_pooler_queries == 256 and d.attn_pooler_heads == 8                  # the reference's defaults
    for form in ("parallel", "cascade"):
        with pytest.raises(ValueError, match="bool form"):
            ovcfg.vision_cfg_from({**v, "attentional_pool": form})
    with pytest.raises(ValueError, match="multiple of attn_pooler_heads"):
        ovcfg.vision_cfg_from({**v, "attn_pooler_heads": 3}, 64)
    with pytest.raises(ValueError, match="head dim"):
        ovcfg.vision_cfg_from({**v, "attn_pooler_heads": 16}, 64)                     # head dim 4
    with pytest.raises(ValueError, match="head dim"):
        ovcfg.vision_cfg_from({**v, "attn_pooler_heads": 1}, 128)                     # head dim 128 > 96
    with pytest.raises(ValueError, match="attn_pooler_queries"):
        ovcfg.vision_cfg_from({**v, "attn_pooler_queries": 257}, 64)
    with pytest.raises(ValueError, match="final_ln_after_pool=false"):              # the flag the pooled branch would ignore
        ovcfg.vision_cfg_from({**v, "final_ln_after_pool": True})
    with pytest.raises(ValueError, match="final_ln_after_pool=false"):              # so an OpenVision preset needs it switched off
        ovcfg.vision_cfg_from({**preset("vit-tiny-patch16-160")["vision_cfg"], "attentional_pool": True})
    assert ovcfg.vision_cfg_from({**preset("vit-tiny-patch16-160")["vision_cfg"], "attentional_pool": True,
                                  "final_ln_after_pool": False}, 192).attentional_pool is True
    with pytest.raises(ValueError, match="timm / layer-scale"):
        ovcfg.vision_cfg_from({**v, "timm_model_name": "vit_base"})
    with pytest.raises(ValueError, match="timm / layer-scale"):
        ovcfg.vision_cfg_from({**v, "ls_init_value": 1e-5})
    with pytest.raises(ValueError, match="head dim"):                                # the model checks what the config alone cannot
        create_model({**pool_cfg("a"), "embed_dim": 200})


@pytest.mark.parametrize("which", ["a", "b"])
def test_both_layouts_have_the_reference_keys_and_round_trip(which, g):
    cfg = pool_cfg(which)
    assert str(g[which + "/weights_variant"]) == WEIGHTS[which][0] and int(g[which + "/weights_seed"]) == WEIGHTS[which][1]
    m = create_model(cfg)
    want = [str(k) for k in g[which + "/keys"]]
    assert sorted(m.state_dict().keys()) == want
    sd = pool_state_dict(which)
    assert sorted(sd) == want
    m = create_model(cfg, state_dict=sd)                              # strict
    back = m.state_dict()
    for k in want:
        assert torch.equal(back[k], sd[k]), k
    pool = m.visual.attn_pool
    assert isinstance(pool, AttentionalPooler) and pool.ln_q.eps == 1e-5 and pool.ln_k.eps == 1e-5
    e, w = 64, cfg["vision_cfg"]["width"]
    shapes = {n: tuple(p.shape) for n, p in pool.named_parameters()}
    common = {"query": (5, e), "attn.in_proj_bias": (3 * e,), "attn.out_proj.weight": (e, e), "attn.out_proj.bias": (e,),
              "ln_q.weight": (e,), "ln_q.bias": (e,), "ln_k.weight": (w,), "ln_k.bias": (w,)}
    layout = ({"attn.in_proj_weight": (3 * e, e)} if which == "b" else
              {"attn.q_proj_weight": (e, e), "attn.k_proj_weight": (e, w), "attn.v_proj_weight": (e, w)})
    assert shapes == {**common, **layout}
    assert tuple(m.visual.ln_post.weight.shape) == (e,) and tuple(m.visual.proj.shape) == (e, e)
    assert tuple(pool.attn.kv_weight().shape) == (2 * e, w) and tuple(pool.attn.q_weight().shape) == (e, e)
    # the stored gradients name parameters of this layout
    named = dict(m.named_parameters())
    grads = [k[len(which) + 6:] for k in g.files if k.startswith(which + "/grad/")]
    assert len(grads) == 6
    for n in grads:
        assert tuple(named[n].shape) == g[f"{which}/grad/{n}"].shape, n


def test_synthetic_weights_without_a_pooler_are_what_the_golden_files_hold():
    """make_state_dict draws nothing differently for a config without a pooler.  The tiny preset: the oracle on these weights gives the
    features the REFERENCE gave on them when tiny16_160.npz was made (every tensor of both towers is on that path).  The stock config:
    the key set stock_tiny.npz stores, with no pooler key and ln_post / proj at the tower's width."""
    cfg = preset("vit-tiny-patch16-160")
    sd = synth.make_state_dict(cfg, 0)
    assert len(sd) == 300 and not any("attn_pool" in k for k in sd)
    gt = golden("tiny16_160.npz")
    img, tok = torch.from_numpy(gt["images"]), torch.from_numpy(gt["tokens"])
    np.testing.assert_allclose(torch.nn.functional.conv2d(img, sd["visual.conv1.weight"], None, stride=16).numpy(), gt["conv1"], atol=1e-5)
    np.testing.assert_allclose(R.encode_image(img, sd, cfg).numpy(), gt["image_features"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(R.encode_text(tok, sd, cfg).numpy(), gt["text_features"], atol=1e-4, rtol=1e-4)
    scfg = stock_cfg()
    ssd = synth.make_state_dict(scfg)
    assert sorted(ssd) == [str(k) for k in golden("stock_tiny.npz")["keys"]]
    assert tuple(ssd["visual.proj"].shape) == (192, 64) and tuple(ssd["visual.ln_post.weight"].shape) == (192,)
    # a pooler changes no tensor outside it and the two it resizes
    psd = synth.make_state_dict({**scfg, "vision_cfg": {**scfg["vision_cfg"], "attentional_pool": True, "attn_pooler_queries": 5,
                                                        "attn_pooler_heads": 2}})
    for k, t in ssd.items():
        if k not in ("visual.proj", "visual.ln_post.weight", "visual.ln_post.bias"):
            assert torch.equal(psd[k], t), k
    assert sorted(set(psd) - set(ssd)) == sorted("visual.attn_pool." + n for n in (
        "query", "attn.q_proj_weight", "attn.k_proj_weight", "attn.v_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
        "attn.out_proj.bias", "ln_q.weight", "ln_q.bias", "ln_k.weight", "ln_k.bias"))


@pytest.mark.parametrize("which", ["a", "b"])
def test_lock_never_thaws_the_pooler(which):
    m = create_model(pool_cfg(which))
    layers = 2
    seen = set()
    for k in range(0, layers + 4):
        m.requires_grad_(True)
        m.lock_image_tower(k)
        on = {n for n, p in m.visual.named_parameters() if p.requires_grad}
        assert not any(n.startswith("attn_pool.") for n in on), (k, on)
        seen |= on
    # everything else does thaw at some k: the groups are the reference's
    assert seen == {n for n, _ in m.visual.named_parameters() if not n.startswith("attn_pool.")}
    assert all(p.requires_grad for n, p in m.named_parameters() if not n.startswith("visual."))


def test_weight_decay_skips_the_query_and_takes_the_projections():
    m = create_model(pool_cfg("a"))
    dec = {n: training.default_decay_filter(n, p) for n, p in m.named_parameters() if n.startswith("visual.attn_pool.")}
    assert dec == {"visual.attn_pool." + n: v for n, v in {
        "query": False, "attn.q_proj_weight": True, "attn.k_proj_weight": True, "attn.v_proj_weight": True, "attn.in_proj_bias": False,
        "attn.out_proj.weight": True, "attn.out_proj.bias": False, "ln_q.weight": False, "ln_q.bias": False, "ln_k.weight": False,
        "ln_k.bias": False}.items()}
    mb = create_model(pool_cfg("b"))
    assert training.default_decay_filter("visual.attn_pool.attn.in_proj_weight", mb.visual.attn_pool.attn.in_proj_weight)
    assert not training.default_decay_filter("visual.attn_pool.query", mb.visual.attn_pool.query)


@pytest.mark.timeout(900)
def test_pool_kernels_build_without_scratch_and_hazards():
    scratch = {k: v for k, v in kernel_scratch("attn_pool.hip").items() if re.search(r"pool_", k)}
    assert len(scratch) == 7, sorted(scratch)                         # forward, dQ and dK / dV passes in two widths, the dq sum
    assert not any(scratch.values()), scratch
    asm = device_asm("attn_pool.hip")
    assert len(re.findall(r"^_Z\w*pool_fwd\w*:", asm, re.M)) == 2
    bad = inline_asm_mfma_hazards(asm, r"pool_")
    assert not bad, f"inline-asm VALU reads of MFMA results inside the hazard window: {bad[:5]} ({len(bad)} in all)"
