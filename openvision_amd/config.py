"""Model configuration: the ``open_clip_config.json`` schema and the OpenVision size table.

Mirrors the dataclasses the reference builds its towers from
(``src/convert_upload/open_clip/model.py:27-84`` ``CLIPVisionCfg`` / ``CLIPTextCfg``) and the
size tables of the JAX->HF converter (``src/convert_upload/transfer_jax2hf.py:76-92``).
Only the fields the encode-and-contrast path reads are kept: the OpenVision towers and the stock
open_clip ones (causal text with 'argmax' pooling, ln_pre, 'tok' pooling).  ``vision_cfg.attentional_pool=True``
(the open_clip CoCa image pooler, with ``attn_pooler_queries`` / ``attn_pooler_heads``) is built; its string forms are not.  Anything
that would select a different architecture (timm/HF towers, quick_gelu, layer-scale, embed_cls, proj_bias) is rejected loudly instead
of being silently ignored.

``vision_cfg.pos_embed_type`` selects the image position table (``openvision_amd.posembed``):

    'learnable'    (default) a trained table, as before.
    'sin_cos_2d'   the reference's torch meaning (transformer.py:477-484): the fixed MAE-form table, ``requires_grad=False``.
    'sincos2d'     an EXTENSION, the JAX recipe's own name (configs/openvision.py:164): the fixed MoCo-v3-form table the
                   converter writes into OpenVision checkpoints.  The vendored open_clip raises on this value, so a config
                   handed back to the reference's loader says 'learnable' (the table is in the state dict either way).

Any other value raises.  Both fixed forms need a width that is a multiple of 4.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field, asdict
from typing import Any, Dict, Optional, Tuple, Union


@dataclass
class CLIPVisionCfg:
    # reference: open_clip/model.py:27-55
    layers: int = 12
    width: int = 768
    head_width: int = 64
    mlp_ratio: float = 4.0
    patch_size: int = 16
    image_size: int = 224
    ls_init_value: Optional[float] = None
    patch_dropout: float = 0.0
    attentional_pool: bool = False
    attn_pooler_queries: int = 256
    attn_pooler_heads: int = 8
    no_ln_pre: bool = False
    pos_embed_type: str = "learnable"
    final_ln_after_pool: bool = False
    pool_type: str = "tok"
    output_tokens: bool = False
    act_kwargs: Optional[dict] = None
    norm_kwargs: Optional[dict] = None
    timm_model_name: Optional[str] = None


@dataclass
class CLIPTextCfg:
    # reference: open_clip/model.py:58-84
    context_length: int = 77
    vocab_size: int = 49408
    hf_tokenizer_name: Optional[str] = None
    tokenizer_kwargs: Optional[dict] = None
    width: int = 512
    heads: int = 8
    layers: int = 12
    mlp_ratio: float = 4.0
    ls_init_value: Optional[float] = None
    embed_cls: bool = False
    pad_id: int = 0
    no_causal_mask: bool = False
    final_ln_after_pool: bool = False
    pool_type: str = "argmax"
    proj_bias: bool = False
    output_tokens: bool = False
    act_kwargs: Optional[dict] = None
    norm_kwargs: Optional[dict] = None
    hf_model_name: Optional[str] = None


POS_EMBED_TYPES = ("learnable", "sin_cos_2d", "sincos2d")      # posembed.py: trained | fixed MAE form | fixed MoCo-v3 form


def _from_dict(cls, d: Union[dict, Any]):
    if isinstance(d, cls):
        return d
    known = {f for f in cls.__dataclass_fields__}
    extra = {k: v for k, v in d.items() if k not in known}
    # Unknown keys that only matter for other model families are tolerated when falsy.
    for k, v in extra.items():
        if v not in (None, False, 0, 0.0, "", [], {}):
            raise ValueError(f"{cls.__name__}: unsupported config key {k!r}={v!r} "
                             f"(outside the OpenVision encode-and-contrast path)")
    return cls(**{k: v for k, v in d.items() if k in known})


def attn_pool_head_dim(embed_dim: int, heads: int) -> int:
    """Head dim of the attentional pooler (AttentionalPooler(d_model=embed_dim, n_head=heads), transformer.py:187-207), checked
    against what ``ov_attn_pool`` takes: a multiple of 8, at most 96."""
    if heads <= 0 or embed_dim % heads:
        raise ValueError(f"attentional pool: embed_dim {embed_dim} must be a multiple of attn_pooler_heads {heads}")
    hd = embed_dim // heads
    if hd % 8 or hd > 96:
        raise ValueError(f"attentional pool: head dim {hd} (embed_dim {embed_dim} / attn_pooler_heads {heads}) must be a multiple "
                         f"of 8 and at most 96")
    return hd


def vision_cfg_from(d, embed_dim: Optional[int] = None) -> CLIPVisionCfg:
    """``embed_dim`` (the model's, when the caller knows it) lets the pooler's head dim be checked here."""
    c = _from_dict(CLIPVisionCfg, d)
    if c.timm_model_name or c.ls_init_value is not None:
        raise ValueError("vision_cfg selects a tower outside the OpenVision ViT path (timm / layer-scale)")
    if c.attentional_pool:
        if c.attentional_pool is not True:
            # the reference's 'parallel' / 'cascade' string forms: "untested, WIP" there (transformer.py:626-634)
            raise ValueError(f"vision attentional_pool={c.attentional_pool!r}: only the bool form (the open_clip CoCa pooler) is built")
        if c.final_ln_after_pool:
            # the reference does not consult the flag on the pooled branch (transformer.py:636-640: ln_post always runs on the pooler's
            # rows, before 'tok' / 'avg'); a config that asks for both would be silently given something else, so it is refused.  No
            # open_clip coca_* config sets it; an OpenVision preset (final_ln_after_pool=true) needs it switched off with the pooler
            raise ValueError("vision attentional_pool=true with final_ln_after_pool=true: the pooled branch applies ln_post to the "
                             "pooler's rows before pooling, whatever the flag says; set final_ln_after_pool=false")
        if not 1 <= int(c.attn_pooler_queries) <= 256:
            raise ValueError(f"vision attn_pooler_queries must lie in [1, 256], got {c.attn_pooler_queries!r}")
        if int(c.attn_pooler_heads) < 1:
            raise ValueError(f"vision attn_pooler_heads must be positive, got {c.attn_pooler_heads!r}")
        if embed_dim is not None:
            attn_pool_head_dim(int(embed_dim), int(c.attn_pooler_heads))
    if not 0 <= float(c.patch_dropout) < 1:                      # PatchDropout's own assertion (transformer.py:56)
        raise ValueError(f"vision patch_dropout must lie in [0, 1), got {c.patch_dropout!r}")
    if c.pool_type not in ("avg", "tok"):
        raise ValueError(f"vision pool_type {c.pool_type!r} not supported (OpenVision uses 'avg')")
    if c.width % c.head_width:
        raise ValueError("vision width must be a multiple of head_width")
    if c.image_size % c.patch_size:
        raise ValueError("image_size must be a multiple of patch_size")
    if c.pos_embed_type not in POS_EMBED_TYPES:
        raise ValueError(f"vision pos_embed_type {c.pos_embed_type!r}: expected one of {POS_EMBED_TYPES}")
    if c.pos_embed_type != "learnable" and c.width % 4:
        raise ValueError(f"vision pos_embed_type {c.pos_embed_type!r} needs a width that is a multiple of 4, got {c.width}")
    return c


def text_cfg_from(d) -> CLIPTextCfg:
    c = _from_dict(CLIPTextCfg, d)
    for key, bad, what in (("hf_model_name", bool(c.hf_model_name), "a Hugging Face text tower"),
                           ("ls_init_value", c.ls_init_value is not None, "layer scale"),
                           ("embed_cls", bool(c.embed_cls), "the appended CLS embedding of CoCa text towers"),
                           ("proj_bias", bool(c.proj_bias), "a biased text projection")):
        if bad:
            raise ValueError(f"text_cfg.{key}={getattr(c, key)!r}: {what} is not built here (supported: the OpenVision text "
                             f"tower, unmasked with 'last' / 'first' pooling, and the stock open_clip one, causal with 'argmax')")
    if c.pool_type not in ("last", "first", "argmax"):
        raise ValueError(f"text pool_type {c.pool_type!r} not supported: 'last' / 'first' (OpenVision) or 'argmax' (stock "
                         f"open_clip: the EOT token's row); attentional and no pooling are not built")
    if not c.no_causal_mask and c.pool_type != "argmax":
        # the stock pair is causal + 'argmax'; a causal tower pooled at a fixed position appears in open_clip only with embed_cls
        raise ValueError(f"causal text attention (no_causal_mask=false) is built for pool_type 'argmax', the stock open_clip "
                         f"text tower; with pool_type {c.pool_type!r} set no_causal_mask=true (OpenVision towers are unmasked)")
    if c.width % c.heads:
        raise ValueError("text width must be a multiple of heads")
    return c


def gelu_is_tanh(act_kwargs: Optional[dict]) -> bool:
    """nn.GELU(**act_kwargs): 'none' (erf) unless approximate == 'tanh' (model.py:196-197)."""
    if not act_kwargs:
        return False
    a = act_kwargs.get("approximate", "none")
    if a not in ("none", "tanh"):
        raise ValueError(f"GELU approximate={a!r}")
    return a == "tanh"


def ln_eps(norm_kwargs: Optional[dict]) -> float:
    """The vendored LayerNorm defaults to eps=1e-6 (transformer.py:458,690)."""
    if norm_kwargs and "eps" in norm_kwargs:
        return float(norm_kwargs["eps"])
    return 1e-6


# OpenVision size table: (vision width, layers, mlp_ratio), text (width, layers, heads), embed_dim.
# transfer_jax2hf.py:76-92, configs/openvision.py:257-263.
_SIZES = {
    "Ti":     dict(vw=192,  vl=12, vmr=4.0,    tw=192,  tl=12, th=3,  e=192,  hw=64),
    "S":      dict(vw=384,  vl=12, vmr=4.0,    tw=384,  tl=12, th=6,  e=384,  hw=64),
    "B":      dict(vw=768,  vl=12, vmr=4.0,    tw=512,  tl=12, th=8,  e=512,  hw=64),
    "L":      dict(vw=1024, vl=24, vmr=4.0,    tw=768,  tl=12, th=12, e=768,  hw=64),
    "So400m": dict(vw=1152, vl=27, vmr=3.7362, tw=1152, tl=27, th=16, e=1152, hw=72, tmr=3.7362),
    "H":      dict(vw=1280, vl=32, vmr=4.0,    tw=1024, tl=24, th=16, e=1024, hw=80),
}


def openvision_model_cfg(size: str, patch: int, image: int, *, context_length: int = 80,
                         vocab_size: int = 32000, pos_embed_type: Optional[str] = None) -> Dict[str, Any]:
    """``model_cfg`` block of an OpenVision ``open_clip_config.json``.  ``pos_embed_type``: added to ``vision_cfg``
    only when given (converted checkpoints carry none: 'learnable'); 'sincos2d' keeps the recipe's table fixed in training."""
    s = _SIZES[size]
    cfg = {
        "embed_dim": s["e"],
        "vision_cfg": {
            "image_size": image, "patch_size": patch, "layers": s["vl"], "width": s["vw"],
            "head_width": s["hw"], "mlp_ratio": s["vmr"], "pool_type": "avg",
            "final_ln_after_pool": True, "no_ln_pre": True,
        },
        "text_cfg": {
            "context_length": context_length, "vocab_size": vocab_size, "layers": s["tl"],
            "width": s["tw"], "heads": s["th"], "mlp_ratio": s.get("tmr", 4.0),
            "pool_type": "last", "no_causal_mask": True,
            "act_kwargs": {"approximate": "tanh"},
        },
    }
    if pos_embed_type is not None:
        if pos_embed_type not in POS_EMBED_TYPES:
            raise ValueError(f"pos_embed_type {pos_embed_type!r}: expected one of {POS_EMBED_TYPES}")
        cfg["vision_cfg"]["pos_embed_type"] = pos_embed_type
    return cfg


PRESETS = {
    "vit-tiny-patch16-160": ("Ti", 16, 160),
    "vit-small-patch8-384": ("S", 8, 384),
    "vit-base-patch16-224": ("B", 16, 224),
    "vit-large-patch14-224": ("L", 14, 224),
    "vit-so400m-patch14-224": ("So400m", 14, 224),
    "vit-huge-patch14-224": ("H", 14, 224),
}


def preset(name: str) -> Dict[str, Any]:
    return openvision_model_cfg(*PRESETS[name])


DEFAULT_PREPROCESS = {"mean": [0.48145466, 0.4578275, 0.40821073],
                      "std": [0.26862954, 0.26130258, 0.27577711]}


def load_config_dir(path: str) -> Tuple[Dict[str, Any], Dict[str, Any]]:
    """Read ``<dir>/open_clip_config.json`` the way ov-zero-shot-test.py:38-49 does.

    Returns (model_cfg, preprocess_cfg)."""
    with open(os.path.join(path, "open_clip_config.json"), "r") as f:
        cfg = json.load(f)
    return cfg["model_cfg"], cfg.get("preprocess_cfg", dict(DEFAULT_PREPROCESS))


def mlp_width(width: int, mlp_ratio: float) -> int:
    return int(width * mlp_ratio)   # transformer.py:231
