#!/usr/bin/env python3
"""Generate tests/golden/attnpool_tiny.npz by RUNNING THE REFERENCE on two tiny image towers with ``attentional_pool=True`` (build
container only).

    python tests/golden/make_golden_attnpool.py --ref REFERENCE_ROOT

The reference ``CLIP`` is built as make_golden.py builds it (``synth`` weights, strict load).  Two configs, keys prefixed ``a/`` and ``b/``:

    a   embed_dim 64, vision width 192 (head_width 64, 2 layers, image 64 / patch 16: L = 17), 5 queries, 2 pooler heads, 'tok' pooling:
        kdim != embed_dim, so nn.MultiheadAttention keeps q / k / v_proj_weight apart
    b   the same at width 64 with 'avg' pooling: kdim == embed_dim, the packed in_proj_weight layout

Stored per config: the sorted state-dict key list, the images (fp16; the reference runs on what is stored), the tokens of a small
unmasked text tower, pooled features (raw and normalised), ``tokens`` = ln_post(pool(x))[:, 1:] from ``visual(...)`` with
``output_tokens=True``, the logits, and the gradients of one ``train()`` step of ClipLoss on the pooler's query, K projection (or packed
in-projection), in_proj_bias, out_proj.weight and ln_k.weight and on the first block's out_proj.weight (matrices as fp16).

What the fixture can tell apart is asserted here on the reference itself: each of these changes moves EVERY image's features by at
least 10 x the suite's COS_TOL (1 - cos >= 1e-2), and the rows of ``tokens`` differ pairwise by as much.  Measured (weights: see
WEIGHTS below), smallest 1 - cos over the images, config a / b:

    ln_k left out                                  0.0439 / 0.0156
    K and V projections swapped                    0.6993 / 1.0578
    CLS excluded from the keys                     0.0372 / 0.0225
    uniform attention (the mean of the tokens)     0.1650 / 0.0283
    tokens rows pairwise                           0.0433 / 0.0243
    the reference's bf16 twin, largest 1 - cos     6.9e-5 / 6.6e-5    (a ceiling, FORMAT_NOISE: see WEIGHTS)

"Uniform attention" is the pooler replaced by the mean of the tokens: with a zero query projection every score is equal, and each
query's output is the mean of the value rows.
"""
from __future__ import annotations

import argparse
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True          # no __pycache__ under tests/golden/ (fixtures live there)

import make_golden as mg                              # noqa: E402
from openvision_amd import synth                      # noqa: E402

# synth weights per config, chosen on the reference alone from a scan over 'v1' / 'sharp' at seeds 0..39: among the sets whose margins
# all reach MARGIN and on which the reference's OWN bf16 twin (the same model under .to(torch.bfloat16)) stays within FORMAT_NOISE of
# its fp32 features and tokens, the one with the largest smallest margin.  Both conditions are asserted below.  (At 'v1' seed 0
# leaving the CLS token out of the keys moves the features by 4e-3 only, one key of 17; on 'sharp' seed 18 of config b the reference's
# bf16 twin moves a token row by 4.5e-4, half of COS_TOL from the number format alone.)
WEIGHTS = {"a": ("sharp", 28), "b": ("v1", 39)}
FORMAT_NOISE = 1e-4                                    # COS_TOL / 10: the tolerance sits as far above bf16's noise as the margins above it
IMG_SEED, N_IMG, T, VOCAB = 3, 3, 32, 1000
MARGIN = 1e-2                                          # 10 x COS_TOL
POOL_GRADS = ["query", "attn.in_proj_bias", "attn.out_proj.weight", "ln_k.weight"]
BLOCK_GRAD = "visual.transformer.resblocks.0.attn.out_proj.weight"


def config(which: str):
    wide = which == "a"
    return {
        "embed_dim": 64,
        "vision_cfg": {"image_size": 64, "patch_size": 16, "width": 192 if wide else 64, "head_width": 64, "layers": 2,
                       "pool_type": "tok" if wide else "avg", "no_ln_pre": False, "final_ln_after_pool": False,
                       "attentional_pool": True, "attn_pooler_queries": 5, "attn_pooler_heads": 2},
        "text_cfg": {"context_length": T, "vocab_size": VOCAB, "width": 128, "heads": 2, "layers": 2, "pool_type": "last",
                     "no_causal_mask": True, "act_kwargs": {"approximate": "tanh"}},
    }


def grad_names(which: str):
    w = "attn.k_proj_weight" if which == "a" else "attn.in_proj_weight"
    return ["visual.attn_pool." + n for n in POOL_GRADS + [w]] + [BLOCK_GRAD]


def one_minus_cos(x, y):
    return 1.0 - torch.nn.functional.cosine_similarity(x.double(), y.double(), dim=-1)


def broken(model, how: str):
    """A copy of the reference model with one thing about the pooler changed."""
    m = copy.deepcopy(model)
    pool, a = m.visual.attn_pool, m.visual.attn_pool.attn
    e = a.embed_dim
    with torch.no_grad():
        if how == "no_ln_k":
            pool.ln_k = torch.nn.Identity()
        elif how == "swap_kv":
            if a.in_proj_weight is not None:
                w = a.in_proj_weight.clone()
                a.in_proj_weight[e:2 * e], a.in_proj_weight[2 * e:] = w[2 * e:], w[e:2 * e]
            else:
                k = a.k_proj_weight.clone()
                a.k_proj_weight.copy_(a.v_proj_weight)
                a.v_proj_weight.copy_(k)
            b = a.in_proj_bias.clone()
            a.in_proj_bias[e:2 * e], a.in_proj_bias[2 * e:] = b[2 * e:], b[e:2 * e]
        elif how == "no_cls":
            pool.register_forward_pre_hook(lambda mod, args: (args[0][:, 1:],))
        elif how == "uniform":                         # zero query projection: equal scores, the softmax is the mean over the tokens
            (a.in_proj_weight[:e] if a.in_proj_weight is not None else a.q_proj_weight).zero_()
            a.in_proj_bias[:e].zero_()
        else:
            raise ValueError(how)
    return m


def run(m, lossmod, which: str, out: dict):
    cfg = config(which)
    variant, seed = WEIGHTS[which]
    model = mg.build_ref(m, cfg, seed=seed, variant=variant)
    pool = model.visual.attn_pool
    assert type(pool).__name__ == "AttentionalPooler" and model.visual.attn_pool_contrastive is None
    assert (pool.attn.in_proj_weight is None) == (which == "a") and pool.ln_k.eps == 1e-5 and pool.ln_q.eps == 1e-5
    img = synth.make_structured_images(N_IMG, 64, seed=IMG_SEED).half().float()
    tok = synth.make_captions(N_IMG, T, VOCAB, seed=1)
    with torch.no_grad():
        fi, ft, scale = model(img, tok)
        raw = model.encode_image(img)
        li, _ = model.get_logits(img, tok)
        model.visual.output_tokens = True
        pooled, tokens = model.visual(img)
        model.visual.output_tokens = False
    assert torch.equal(pooled, raw) and tuple(tokens.shape) == (N_IMG, 4, 64)
    margins = {}
    for how in ("no_ln_k", "swap_kv", "no_cls", "uniform"):
        with torch.no_grad():
            margins[how] = float(one_minus_cos(broken(model, how).encode_image(img), raw).min())
    rows = torch.nn.functional.normalize(tokens.double(), dim=-1)
    cos = rows @ rows.transpose(-1, -2)
    cos = cos + torch.eye(4).double() * -2.0
    margins["tokens"] = float(1.0 - cos.max())
    print(f"config {which}: " + "  ".join(f"{k} {v:.4f}" for k, v in margins.items()))
    for k, v in margins.items():
        assert v >= MARGIN, (which, k, v)
    twin = copy.deepcopy(model).to(torch.bfloat16)
    twin.visual.output_tokens = True
    with torch.no_grad():
        p16, t16 = twin.visual(img.to(torch.bfloat16))
    noise = (float(one_minus_cos(p16.float(), raw).max()), float(one_minus_cos(t16.float(), tokens).max()))
    print(f"config {which}: the reference's bf16 twin against fp32, largest 1 - cos: features {noise[0]:.2e}  tokens {noise[1]:.2e}")
    assert max(noise) <= FORMAT_NOISE, (which, noise)

    model.train()
    fi_t, ft_t, scale_t = model(img, tok)
    loss = lossmod.ClipLoss()(fi_t, ft_t, scale_t)
    loss.backward()
    named = dict(model.named_parameters())
    p = which + "/"
    out.update({p + "keys": np.array(sorted(model.state_dict().keys())), p + "images": img.numpy().astype(np.float16),
                p + "text": tok.numpy(), p + "image_features": mg.f32(fi), p + "text_features": mg.f32(ft),
                p + "image_features_raw": mg.f32(raw), p + "tokens": mg.f32(tokens), p + "logits_per_image": mg.f32(li),
                p + "logit_scale": mg.f32(scale), p + "loss": mg.f32(loss), p + "weights_variant": np.array(variant),
                p + "weights_seed": np.int64(seed)})
    for n in grad_names(which):
        gr = named[n].grad.detach().float().numpy()
        out[p + "grad/" + n] = gr.astype(np.float16) if gr.ndim == 2 and not n.endswith("query") else gr
    return margins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "attnpool_tiny.npz"))
    a = ap.parse_args()
    m, lossmod, _ = mg.import_reference(a.ref)
    out = {}
    for which in ("a", "b"):
        run(m, lossmod, which, out)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
