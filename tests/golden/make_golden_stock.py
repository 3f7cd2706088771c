#!/usr/bin/env python3
"""Generate tests/golden/stock_tiny.npz by RUNNING THE REFERENCE on a stock open_clip configuration (build container only).

    python tests/golden/make_golden_stock.py --ref REFERENCE_ROOT

The reference ``CLIP`` is built as make_golden.py builds it, on a tiny model with the DEFAULTS of ``CLIPVisionCfg`` / ``CLIPTextCfg``
where OpenVision departs from them: a causal text tower pooled at the EOT token (``no_causal_mask=False, pool_type='argmax'``) and an
image tower with ``ln_pre``, 'tok' pooling and ``ln_post`` before the pool.  Weights: ``synth`` 'v1', seed 0 (on the 'sharp' set the
mask moves the row whose EOT sits at the last position by 1.1e-3 only: too thin to tell a missing mask from rounding).

Inputs: three structured images and two 8-row token tables (stored).  EOT id = vocab - 1 = 999, ids in [1, 998) before it:

    row 0..5   EOT at 0, 76, 31, 32, 5, 9; the EOT-at-9 row carries a second 999 at 40 (the first one must win)
    row 6      all 7s (argmax 0)
    row 7      EOT at 20 followed by random ids below 999

``tokens_b`` differs from ``tokens`` only AFTER each row's pooled position and keeps every argmax (ids below 7 in the all-7s row), so a
causal tower gives the same features for both, and an unmasked one does not.  This script asserts, on the reference:

    masked:    features(tokens_b) == features(tokens), max |delta| = 0.0
    unmasked:  the same pair moves every row but the EOT-at-76 one (identical rows) by 1 - cos >= 0.031
    masked vs unmasked features of ``tokens``: 1 - cos >= 5.5e-3 on every row
    text rows pairwise at cos <= 0.88, images at cos <= 0.973 (to three places: the closest pair is at 0.97301)

so the suite's COS_TOL = 1e-3 separates a missing mask, a wrong pooled row and swapped rows.  Stored besides: the state-dict key list,
the mask, both feature sets (eval mode), the logits and the ClipLoss value, and the gradients of one ``train()`` step on the images
and the first 3 text rows (the matrices as fp16).
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
from openvision_amd import synth                      # noqa: E402

T, VOCAB, EOT = 77, 1000, 999
EOT_AT = [0, 76, 31, 32, 5, 9]
ROW_LAST, ROW_TWICE, ROW_SEVENS, ROW_TAIL = 1, 5, 6, 7
IMG_SEED, TOK_SEED = 3, 3
TRAIN_ROWS = 3
GRADS = ["visual.ln_pre.weight", "visual.conv1.weight", "token_embedding.weight", "positional_embedding",
         "visual.transformer.resblocks.0.attn.out_proj.weight", "visual.transformer.resblocks.1.attn.out_proj.weight",
         "transformer.resblocks.0.attn.out_proj.weight", "transformer.resblocks.2.attn.out_proj.weight", "text_projection"]
FP16 = {n for n in GRADS if n.endswith(".weight") and n != "visual.ln_pre.weight"}


def config():
    return {
        "embed_dim": 64,
        "vision_cfg": {"image_size": 64, "patch_size": 16, "width": 192, "head_width": 64, "layers": 2, "pool_type": "tok",
                       "no_ln_pre": False, "final_ln_after_pool": False},
        "text_cfg": {"context_length": T, "vocab_size": VOCAB, "width": 192, "heads": 3, "layers": 3, "pool_type": "argmax",
                     "no_causal_mask": False},
    }


def token_tables():
    g = np.random.Generator(np.random.Philox(key=[TOK_SEED, 0]))
    a = np.zeros((8, T), dtype=np.int64)
    for r, e in enumerate(EOT_AT):
        a[r, :e] = g.integers(1, 998, size=e)
        a[r, e] = EOT                                  # zero padding behind it, as the tokenizer leaves it
    a[ROW_TWICE, 40] = EOT
    a[ROW_SEVENS, :] = 7
    a[ROW_TAIL, :20] = g.integers(1, 998, size=20)
    a[ROW_TAIL, 20] = EOT
    a[ROW_TAIL, 21:] = g.integers(1, 999, size=T - 21)
    pooled = a.argmax(axis=1)
    assert pooled.tolist() == EOT_AT + [0, 20]
    b = a.copy()
    for r in range(8):
        n = T - 1 - pooled[r]
        b[r, pooled[r] + 1:] = g.integers(1, 7 if r == ROW_SEVENS else 999, size=n)
    b[ROW_TWICE, 40] = EOT                             # the second EOT stays: the first still wins
    assert b.argmax(axis=1).tolist() == pooled.tolist()
    for r in range(8):
        assert np.array_equal(a[r, :pooled[r] + 1], b[r, :pooled[r] + 1])
        assert r == ROW_LAST or not np.array_equal(a[r], b[r])
    return a, b


def one_minus_cos(x, y):
    return 1.0 - torch.nn.functional.cosine_similarity(x.double(), y.double(), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "stock_tiny.npz"))
    a = ap.parse_args()
    m, lossmod, _ = mg.import_reference(a.ref)
    cfg = config()
    model = mg.build_ref(m, cfg)                       # strict load of synth 'v1', seed 0; eval mode
    mask = model.attn_mask
    assert mask is not None and tuple(mask.shape) == (T, T) and "attn_mask" not in model.state_dict()
    assert model.text_pool_type == "argmax" and type(model.visual.ln_pre).__name__ == "LayerNorm"
    img = synth.make_structured_images(3, 64, seed=IMG_SEED).half().float()     # stored as fp16: run on what is stored
    ta, tb = (torch.from_numpy(x) for x in token_tables())
    with torch.no_grad():
        fi, ft, scale = model(img, ta)
        ft_b = model.encode_text(tb, normalize=True)
        raw_i, raw_t = model.encode_image(img), model.encode_text(ta)
        li, lt = model.get_logits(img, ta)
        loss3 = lossmod.ClipLoss()(fi, ft[:TRAIN_ROWS], scale)
        model.attn_mask = None                         # the same weights without the mask
        un_a, un_b = model.encode_text(ta, normalize=True), model.encode_text(tb, normalize=True)
        model.attn_mask = mask
    # what the fixture is good for
    same = float((ft - ft_b).abs().max())
    moved = one_minus_cos(un_a, un_b)
    by_mask = one_minus_cos(ft, un_a)
    ct, ci = (ft @ ft.T).fill_diagonal_(-1.0), (fi @ fi.T).fill_diagonal_(-1.0)
    print("masked: max |features(b) - features(a)| =", same)
    print("unmasked: 1 - cos(a, b) per row =", moved.numpy().round(4))
    print("masked vs unmasked 1 - cos per row =", by_mask.numpy().round(5))
    print("largest pairwise cos: text", float(ct.max()), "images", float(ci.max()))
    assert same == 0.0
    others = [r for r in range(8) if r != ROW_LAST]
    assert float(moved[ROW_LAST]) == 0.0 and float(moved[others].min()) >= 0.031
    assert float(by_mask.min()) >= 5.5e-3
    assert float(ct.max()) <= 0.88 and round(float(ci.max()), 3) <= 0.973       # the closest image pair: 0.97301

    model.train()
    fi_t, ft_t, scale_t = model(img, ta[:TRAIN_ROWS])
    loss = lossmod.ClipLoss()(fi_t, ft_t, scale_t)
    loss.backward()
    assert abs(float(loss.detach()) - float(loss3)) < 1e-5     # no dropout anywhere: train() and eval() agree
    named = dict(model.named_parameters())
    out = dict(keys=np.array(sorted(model.state_dict().keys())), attn_mask=mg.f32(mask), images=img.numpy().astype(np.float16),
               tokens=ta.numpy(), tokens_b=tb.numpy(), image_features=mg.f32(fi), text_features=mg.f32(ft),
               image_features_raw=mg.f32(raw_i), text_features_raw=mg.f32(raw_t), logits_per_image=mg.f32(li),
               logit_scale=mg.f32(scale), loss=mg.f32(loss), train_rows=np.int64(TRAIN_ROWS))
    for n in GRADS:
        gr = named[n].grad.detach().float().numpy()
        out["grad/" + n] = gr.astype(np.float16) if n in FP16 else gr
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes; loss", float(loss))


if __name__ == "__main__":
    main()
