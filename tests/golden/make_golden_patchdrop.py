#!/usr/bin/env python3
"""Generate tests/golden/patchdrop_tiny16_160.npz by RUNNING THE REFERENCE's patch dropout (build container only).

    python tests/golden/make_golden_patchdrop.py --ref REFERENCE_ROOT

The reference CLIP is built as make_golden.py builds it (Ti/16@160, the 'v1' formula weights) with ``vision_cfg.patch_dropout = 0.5``,
so that ``VisionTransformer`` holds ``PatchDropout(0.5)`` (model.py:157, transformer.py:481): G = 100 patches, K = 50 kept, L' = 51.
In ``train()`` mode, after ``torch.manual_seed(SEED)``, one ``model(images, tokens)`` + ``ClipLoss`` + backward is run.  Stored: the
patch indices the reference drew (``torch.randn(B, G).topk(K).indices`` replayed under the same seed, checked against the tokens a
forward hook on ``visual.patch_dropout`` saw leave the module), the image features, the loss, and the gradients of conv1.weight,
class_embedding, positional_embedding, one early and one late block weight and proj (the large ones as fp16).  Inputs are rebuilt in
the tests from ``openvision_amd.synth`` (IMG_SEED / TOK_SEED).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True          # no __pycache__ under tests/golden/ (fixtures live there)

import make_golden as mg                              # noqa: E402
from openvision_amd import config as ovcfg            # noqa: E402
from openvision_amd import synth                      # noqa: E402

PRESET = "vit-tiny-patch16-160"
P_DROP = 0.5
BATCH = 4
SEED = 1234
IMG_SEED = TOK_SEED = 31
GRADS = ["visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding",
         "visual.transformer.resblocks.0.attn.out_proj.weight", "visual.transformer.resblocks.11.mlp.c_proj.weight", "visual.proj"]
FP16 = {"visual.conv1.weight", "visual.transformer.resblocks.0.attn.out_proj.weight", "visual.transformer.resblocks.11.mlp.c_proj.weight",
        "visual.proj"}


def config():
    cfg = ovcfg.preset(PRESET)
    cfg = dict(cfg, vision_cfg=dict(cfg["vision_cfg"], patch_dropout=P_DROP))
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "patchdrop_tiny16_160.npz"))
    a = ap.parse_args()
    m, lossmod, _ = mg.import_reference(a.ref)
    cfg = config()
    model = mg.build_ref(m, cfg)
    model.train()
    assert type(model.visual.patch_dropout).__name__ == "PatchDropout" and model.visual.patch_dropout.prob == P_DROP
    img = synth.make_images(BATCH, 160, seed=IMG_SEED)
    tok = synth.make_captions(BATCH, seed=TOK_SEED)
    g = (160 // 16) ** 2
    k = max(1, int(g * (1 - P_DROP)))
    torch.manual_seed(SEED)
    keep = torch.randn(BATCH, g).topk(k, dim=-1).indices
    seen = {}
    hook = model.visual.patch_dropout.register_forward_hook(
        lambda mod, inp, out: seen.update(x=inp[0].detach().clone(), y=out.detach().clone()))
    torch.manual_seed(SEED)
    fi, ft, scale = model(img, tok)
    hook.remove()
    x, y = seen["x"], seen["y"]
    assert y.shape == (BATCH, 1 + k, x.shape[-1])
    assert torch.equal(y[:, 0], x[:, 0])
    assert torch.equal(y[:, 1:], x[:, 1:][torch.arange(BATCH)[:, None], keep]), "replayed draw differs from the reference's"
    loss = lossmod.ClipLoss()(fi, ft, scale)
    loss.backward()
    named = dict(model.named_parameters())
    out = dict(preset=np.array(PRESET), p=np.float64(P_DROP), seed=np.int64(SEED), img_seed=np.int64(IMG_SEED),
               tok_seed=np.int64(TOK_SEED), keep=keep.numpy().astype(np.int64), image_features=mg.f32(fi),
               text_features=mg.f32(ft), loss=mg.f32(loss))
    for n in GRADS:
        gr = named[n].grad.detach().float().numpy()
        out["grad/" + n] = gr.astype(np.float16) if n in FP16 else gr
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes; loss", float(loss))


if __name__ == "__main__":
    main()
