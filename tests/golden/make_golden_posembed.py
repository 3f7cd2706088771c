#!/usr/bin/env python3
"""Generate tests/golden/posembed_tiny.npz by RUNNING THE REFERENCE on the CPU (build container only).

    python tests/golden/make_golden_posembed.py --ref REFERENCE_ROOT

Tiny OpenVision model (``config``): width 192, 3 heads, 2 layers per tower, patch 16, 'avg' pooling, ``synth`` weights (seed 0), at the
image sizes 64, 96 and 128, i.e. L = 17, 37 and 65 tokens (37 is L/14 at 84 px; 65 = 64 + 1 runs the attention's lone-key tail).

Stored:

(a) ``mae/G``: the reference's ``get_2d_sincos_pos_embed(192, G, cls_token=True)`` ``.float()``, G = 4, 6, 8.
(b) ``rand/4``, ``rand/6``: name-seeded normal tables of std 0.5 (random, so that interpolation kinds are far apart), and what the
    reference's ``resize_pos_embed`` makes of them: ``resized/4to6``, ``resized/4to8``, ``resized/6to4`` (the antialiased
    direction).  ``text/80``, ``text/48`` (width 32) and the reference's ``resize_text_pos_embed``: ``text/80to48``, ``text/48to80``.
(c) For three structured images (``synth.make_structured_images(3, 128, seed=3).half().float()``; the 96 px images are their top
    left 96 x 96 corner; only a checksum is stored, the images are regenerated) the reference's raw image features and its
    post-block patch tokens (fp16) at 96 and 128 from two models: ``fixed`` (``pos_embed_type='sin_cos_2d'``) and ``resized`` (the
    learnable model whose table is ``rand/4`` resized by the reference).
(d) ``grad/NAME``: the gradients of one ``train()`` step of the reference (model forward + ClipLoss) at 96 on the ``resized`` model,
    for the parameters of ``make_golden_stock.GRADS`` that this model has (no ln_pre, two text blocks) and the image position table.

Asserted here, on the reference: each wrong alternative -- the grid-4 table tiled instead of resized, the grid transposed, a zero
table, bilinear in place of bicubic -- moves the quantity the GPU test compares (max over images of 1 - cos of the features; where
those do not reach it, max over patch tokens of 1 - cos) by at least 5 x COS_TOL = 5e-3.  ``quantity/MODEL/SIZE`` names the one used.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True          # no __pycache__ under tests/golden/ (fixtures live there)

import make_golden as mg                              # noqa: E402
from make_golden_stock import GRADS                   # noqa: E402
from openvision_amd import synth                      # noqa: E402

WIDTH, PATCH, T, VOCAB, TEXT_W = 192, 16, 80, 1000, 32
SIZES = (64, 96, 128)
IMG_SEED, TOK_SEED, BATCH = 3, 3, 3
MARGIN = 5e-3                                         # 5 x COS_TOL of tests/test_gpu_model.py
FP16 = {n for n in GRADS if n.endswith(".weight")}


def config(size=64, pos_embed_type=None):
    v = {"image_size": size, "patch_size": PATCH, "width": WIDTH, "head_width": 64, "layers": 2, "mlp_ratio": 4.0, "pool_type": "avg",
         "final_ln_after_pool": True, "no_ln_pre": True}
    if pos_embed_type is not None:
        v["pos_embed_type"] = pos_embed_type
    return {"embed_dim": 64, "vision_cfg": v,
            "text_cfg": {"context_length": T, "vocab_size": VOCAB, "width": WIDTH, "heads": 3, "layers": 2, "mlp_ratio": 4.0,
                         "pool_type": "last", "no_causal_mask": True, "act_kwargs": {"approximate": "tanh"}}}


def rand_table(name, rows, width=WIDTH):
    return synth._normal("posembed." + name, (rows, width), 0.5, 0)


def images(size):
    return synth.make_structured_images(BATCH, 128, seed=IMG_SEED).half().float()[:, :, :size, :size].contiguous()


def omc(a, b):
    return float((1.0 - F.cosine_similarity(a.double(), b.double(), dim=-1)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "posembed_tiny.npz"))
    ap.add_argument("--variant", default="v1", choices=("v1", "sharp"))
    a = ap.parse_args()
    m, lossmod, _ = mg.import_reference(a.ref)
    pe = __import__("open_clip.pos_embed", fromlist=["get_2d_sincos_pos_embed"])
    out = dict(config_json=np.array(json.dumps(config(), sort_keys=True)), variant=np.array(a.variant))

    # (a)
    for g in (4, 6, 8):
        out[f"mae/{g}"] = torch.from_numpy(pe.get_2d_sincos_pos_embed(WIDTH, g, cls_token=True)).float().numpy()

    # (b)
    def ref_resize(table, g):
        sd = {"visual.positional_embedding": table.clone()}
        m.resize_pos_embed(sd, types.SimpleNamespace(visual=types.SimpleNamespace(grid_size=(g, g))))
        return sd["visual.positional_embedding"]

    def ref_resize_text(table, n):
        sd = {"positional_embedding": table.clone()}
        m.resize_text_pos_embed(sd, types.SimpleNamespace(positional_embedding=torch.empty(n, table.shape[1])))
        return sd["positional_embedding"]

    r4, r6 = rand_table("g4", 17), rand_table("g6", 37)
    out["rand/4"], out["rand/6"] = r4.numpy(), r6.numpy()
    for src, name, g in ((r4, "4to6", 6), (r4, "4to8", 8), (r6, "6to4", 4)):
        out["resized/" + name] = mg.f32(ref_resize(src, g))
        assert torch.equal(ref_resize(src, g)[0], src[0])                      # the class row is kept
    t80, t48 = rand_table("t80", 80, TEXT_W), rand_table("t48", 48, TEXT_W)
    out["text/80"], out["text/48"] = t80.numpy(), t48.numpy()
    out["text/80to48"], out["text/48to80"] = mg.f32(ref_resize_text(t80, 48)), mg.f32(ref_resize_text(t48, 80))

    # (c)
    def build(size, table, pos_embed_type=None):
        cfg = config(size, pos_embed_type)
        model = m.CLIP(embed_dim=cfg["embed_dim"], vision_cfg=dict(cfg["vision_cfg"]), text_cfg=dict(cfg["text_cfg"]))
        sd = synth.make_state_dict(cfg, 0, a.variant)
        sd["visual.positional_embedding"] = model.visual.positional_embedding.detach().clone() if table is None else table
        model.load_state_dict(sd, strict=True)
        return model.eval()

    def run(model, img):
        outs = mg.tokens_after_blocks(model, img, [1])
        with torch.no_grad():
            return model.encode_image(img), outs[1][:, 1:]

    def interp(table, g, mode, antialias):
        g0 = int(round((table.shape[0] - 1) ** 0.5))
        x = table[1:].reshape(1, g0, g0, -1).permute(0, 3, 1, 2)
        x = F.interpolate(x, size=(g, g), mode=mode, antialias=antialias, align_corners=False)
        return torch.cat([table[:1], x.permute(0, 2, 3, 1).reshape(g * g, -1)], dim=0)

    def tiled(table, g):
        g0 = int(round((table.shape[0] - 1) ** 0.5))
        idx = torch.arange(g) % g0
        return torch.cat([table[:1], table[1:].reshape(g0, g0, -1)[idx][:, idx].reshape(g * g, -1)], dim=0)

    def transposed(table):
        g = int(round((table.shape[0] - 1) ** 0.5))
        return torch.cat([table[:1], table[1:].reshape(g, g, -1).transpose(0, 1).reshape(g * g, -1)], dim=0)

    cks = {}
    for size in SIZES[1:]:
        g = size // PATCH
        img = images(size)
        cks[size] = np.array([float(img.double().sum()), float(img.double().abs().sum())])
        out[f"images_checksum/{size}"] = cks[size]
        fixed = build(size, None, "sin_cos_2d")
        assert not fixed.visual.positional_embedding.requires_grad
        assert torch.equal(fixed.visual.positional_embedding, torch.from_numpy(out[f"mae/{g}"]))
        right = {"fixed": fixed.visual.positional_embedding.detach().clone(), "resized": ref_resize(r4, g)}
        mae4 = torch.from_numpy(out["mae/4"])
        wrong = {"fixed": {"tiled": tiled(mae4, g), "transposed": transposed(right["fixed"]), "zero": torch.zeros_like(right["fixed"])},
                 "resized": {"tiled": tiled(r4, g), "transposed": transposed(right["resized"]), "zero": torch.zeros_like(right["resized"]),
                             "bilinear": interp(r4, g, "bilinear", True)}}
        for name in ("fixed", "resized"):
            feats, toks = run(fixed if name == "fixed" else build(size, right[name]), img)
            out[f"features/{name}/{size}"], out[f"tokens/{name}/{size}"] = mg.f32(feats), mg.f32(toks).astype(np.float16)
            moved = {}
            for alt, table in wrong[name].items():
                f2, t2 = run(build(size, table), img)
                moved[alt] = (omc(f2, feats), omc(t2, toks))
                print(f"{name} @ {size}, {alt}: features move by {moved[alt][0]:.3e}, tokens by {moved[alt][1]:.3e}")
            if min(v[0] for v in moved.values()) >= MARGIN:
                quantity = "features"
            else:
                quantity = "tokens"
                assert min(v[1] for v in moved.values()) >= MARGIN, (name, size, moved)
            out[f"quantity/{name}/{size}"] = np.array(quantity)
            print(f"{name} @ {size}: compared on the {quantity}")

    # (d)
    size = 96
    img = images(size)
    tok = synth.make_captions(BATCH, T, VOCAB, seed=TOK_SEED)
    model = build(size, ref_resize(r4, size // PATCH))
    model.train()
    fi, ft, scale = model(img, tok)
    loss = lossmod.ClipLoss()(fi, ft, scale)
    loss.backward()
    named = dict(model.named_parameters())
    out.update(tokens=tok.numpy(), train_image_features=mg.f32(fi), train_text_features=mg.f32(ft), loss=mg.f32(loss))
    stored = [n for n in GRADS if n in named] + ["visual.positional_embedding"]
    for n in stored:
        gr = named[n].grad.detach().float().numpy()
        out["grad/" + n] = gr.astype(np.float16) if n in FP16 else gr
    print("gradients stored for", stored, "; not in this model:", [n for n in GRADS if n not in named])
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes; loss", float(loss.detach()))


if __name__ == "__main__":
    main()
