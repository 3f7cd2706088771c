#!/usr/bin/env python3
"""Generate tests/golden/featviz_tiny16_160.npz by RUNNING THE REFERENCE's feature-visualisation objective (build container only).

    python tests/golden/make_golden_featviz.py --ref REFERENCE_ROOT

The objective of ov-feature-visualization.py:211 is ``ViTEnsFeatHook(ClipOVGeLUHook(model, sl=slice(layer, layer + 1)), key='high',
feat=feature)``: a forward hook on ``visual.transformer.resblocks[layer].mlp.gelu`` (cliptoolsoptimized.py:1149-1164) and

    all_feats = hidden[:, 1:, :].mean(dim=1);  loss = -all_feats[:min(all_feats.shape), feature].diag().mean()

(cliptoolsoptimized.py:995-999; ``.diag()`` of a vector is a B x B matrix, so the mean is over B^2 entries).  ``cliptoolsoptimized``
itself does not import without torchvision, so the same hook and expression are applied here to the reference's own
``open_clip.model.CLIP`` (imported as make_golden.py does), with ``loss.backward()`` to the image.  Weights: the 'v1' formula
weights of Ti/16@160 (openvision_amd.synth, not stored); images: three structured images whose pixel gradients differ (pairwise
cosine < 0.9).  The 'sharp' weights were tried and dropped: they amplify rounding so much that the reference's own bf16 mode is at
gradient cosine 0.988 at layer 11, outside any useful bound for a bf16 path.

Kept small: the images are not stored but regenerated from their seed (``image_sum`` checks the regeneration), and the pixel
gradient is stored one step before the pixels, at conv1's output [B, D, g, g]: conv1 has stride = kernel, so the pixel gradient is
exactly ``conv_transpose2d(that, conv1.weight, stride=P)`` (what autograd computes for conv2d's input), rebuilt by the tests.  It is
quantised to int8 per (image, patch) group of D values with an fp32 scale per group (cosine to the exact gradient > 0.99995).

Stored per (layer, feature) pair k: m_k [B] (= all_feats[:, feature]), loss_k, conv1-output gradient (``convgrad_q_k`` int8,
``convgrad_s_k`` fp32), the pixel gradient's norm, and from the reference's bf16 mode (factory.py:275-296) on the same inputs m, loss,
the pixel gradient's cosine to the fp32 one and its norm -- the distance from the fp32 run is the error budget of a bf16 path.
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

PRESET, SIZE, SEED, VARIANT, IMG_SEED, B = "vit-tiny-patch16-160", 160, 0, "v1", 51, 3
LAYERS = (0, 5, 11)


def objective(model, img, layer, feature):
    """The script's loss on the reference model: (m [B], loss, d loss / d img, d loss / d conv1 output)."""
    acts = {}
    hook = model.visual.transformer.resblocks[layer].mlp.gelu.register_forward_hook(lambda mod, inp, out: acts.__setitem__("h", out))

    def keep_conv(mod, inp, out):
        out.retain_grad()
        acts["conv"] = out

    hook2 = model.visual.conv1.register_forward_hook(keep_conv)
    x = img.clone().requires_grad_(True)
    model.encode_image(x)
    hook.remove()
    hook2.remove()
    all_feats = acts["h"][:, 1:, :].mean(dim=1)
    mn = min(all_feats.shape)
    loss = -all_feats[:mn, feature].diag().mean()
    loss.backward()
    return all_feats[:, feature].detach().float(), loss.detach().float(), x.grad.detach().float(), acts["conv"].grad.detach().float()


def quantise(gc):
    """[B, D, g, g] -> int8 [B, D, g, g] and fp32 scales [B, g, g]: one scale per (image, patch) group of D values."""
    s = gc.abs().amax(dim=1) / 127.0
    s = torch.where(s > 0, s, torch.ones_like(s))
    return torch.round(gc / s[:, None]).clamp(-127, 127).to(torch.int8), s


def dequantise_to_pixels(q, s, conv_w, patch):
    return torch.nn.functional.conv_transpose2d(q.float() * s[:, None], conv_w.float(), stride=patch)


def pick_feature(model, img, layer):
    """The unit with the largest mean GELU output over the batch: well inside the GELU's linear part, so its gradient is not small."""
    acts = {}
    hook = model.visual.transformer.resblocks[layer].mlp.gelu.register_forward_hook(lambda mod, inp, out: acts.__setitem__("h", out))
    with torch.no_grad():
        model.encode_image(img)
    hook.remove()
    return int(acts["h"][:, 1:, :].mean(dim=1).mean(dim=0).argmax())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    torch.manual_seed(0)
    m, _, _ = mg.import_reference(a.ref)
    cfg = ovcfg.preset(PRESET)
    img = synth.make_structured_images(B, SIZE, seed=IMG_SEED).half().float()       # stored as fp16: run on the stored values
    model = mg.build_ref(m, cfg, seed=SEED, variant=VARIANT)
    mb = mg.build_ref(m, cfg, seed=SEED, cast_dtype=torch.bfloat16, variant=VARIANT)
    res = dict(preset=np.array(PRESET), seed=np.int64(SEED), variant=np.array(VARIANT), image_seed=np.int64(IMG_SEED),
               batch=np.int64(B), image_size=np.int64(SIZE), image_sum=np.float64(img.double().sum().item()),
               image_abs_sum=np.float64(img.double().abs().sum().item()), layers=np.array(LAYERS, dtype=np.int64))
    conv_w = synth.make_state_dict(cfg, SEED, VARIANT)["visual.conv1.weight"]
    patch = cfg["vision_cfg"]["patch_size"]
    feats = []
    for k, layer in enumerate(LAYERS):
        f = pick_feature(model, img, layer)
        feats.append(f)
        mm, loss, g, gc = objective(model, img, layer, f)
        mb_, lossb, gb, _ = objective(mb, img.to(torch.bfloat16), layer, f)
        q, sc = quantise(gc)
        qcos = torch.nn.functional.cosine_similarity(dequantise_to_pixels(q, sc, conv_w, patch).flatten(), g.flatten(), dim=0).item()
        assert qcos > 0.99995, qcos
        gn, gbn = g.norm(), gb.norm()
        gflat = g.reshape(B, -1)
        cos = torch.nn.functional.cosine_similarity(gflat[:, None], gflat[None], dim=-1)
        off = cos[~torch.eye(B, dtype=torch.bool)].abs().max().item()
        print(f"layer {layer} feature {f}: m {mm.tolist()} loss {loss.item():.6f} |grad| {gn:.3e}  bf16: loss {lossb.item():.6f} "
              f"cos {torch.nn.functional.cosine_similarity(g.flatten(), gb.flatten(), dim=0).item():.5f} |grad| {gbn:.3e}  "
              f"max |cos| between images {off:.3f}  stored gradient cos {qcos:.6f}")
        assert off < 0.9, "image gradients too similar"
        res.update({f"m_{k}": mm.numpy(), f"loss_{k}": loss.numpy(), f"convgrad_q_{k}": q.numpy(), f"convgrad_s_{k}": sc.numpy(),
                    f"grad_norm_{k}": gn.numpy(), f"m_refbf16_{k}": mb_.numpy(), f"loss_refbf16_{k}": lossb.numpy(),
                    f"grad_cos_refbf16_{k}": torch.nn.functional.cosine_similarity(g.flatten(), gb.flatten(), dim=0).numpy(),
                    f"grad_norm_refbf16_{k}": gbn.numpy()})
    res["features"] = np.array(feats, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "featviz_tiny16_160.npz"), **res)


if __name__ == "__main__":
    main()
