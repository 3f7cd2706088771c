#!/usr/bin/env python3
"""Feature-visualisation step cost at L/14@224, B = 8 (the script's RepeatBatch(8)): ms per optimisation step (objective forward +
backward to the pixels) for

  hip        openvision_amd.visualize.MLPFeatureLoss: blocks [0, layer) + the tap block's attention half + the tap kernels, input-only
             backward (no weight gradients, nothing of the tap block's MLP but one column)
  full_bwd   the composition the training path offers: blocks [0, layer] as one _TowerFn node (ov_tower_forward_saving /
             ov_tower_backward, weight gradients included, the tap block's whole MLP) -- what the step costs without the tap path
  oracle     fp32 torch eager on the device (oracle/clip_ref.py pieces: the reference's arithmetic, not its hook machinery)

    python tools/featviz_probe.py [--layers 0,11,23] [--iters 10] [--out featviz_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from openvision_amd import preset, synth, training  # noqa: E402
from openvision_amd.model import create_model  # noqa: E402
from openvision_amd.visualize import MLPFeatureLoss  # noqa: E402
from test_featviz_cpu import featviz_oracle  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="0,11,23")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = preset("vit-large-patch14-224")
    sd = synth.make_state_dict(cfg, 0, "v1")
    model = create_model(cfg, device=DEV, state_dict=sd)
    for p in model.parameters():
        p.requires_grad_(True)           # as in the script: the model's parameters are leaves (the tap path writes no .grad)
    vcfg = cfg["vision_cfg"]
    sdv = {k: v.to(DEV).float() for k, v in sd.items() if k.startswith("visual.")}
    img = synth.make_structured_images(a.batch, 224, seed=61).to(DEV).requires_grad_(True)
    v = model.visual
    rows = []
    for layer in [int(x) for x in a.layers.split(",")]:
        feature = 37
        lf = MLPFeatureLoss(model, layer, feature)

        def hip():
            img.grad = None
            lf(img).backward()

        blocks = list(v.transformer.resblocks)[:layer + 1]
        params = [p for blk in blocks for p in training._block_tensors(blk)]

        def full_bwd():
            img.grad = None
            x = training._LinearFn.apply(
                img.reshape(a.batch, 3, 16, 14, 16, 14).permute(0, 2, 4, 1, 3, 5).reshape(a.batch * 256, 588),
                v.conv1.weight.detach().reshape(v.conv1.weight.shape[0], -1), None).view(a.batch, 256, -1)
            x = torch.cat([v.class_embedding.detach().float().expand(a.batch, 1, -1), x], dim=1) + v.positional_embedding.detach().float()
            y = training._TowerFn.apply(v.transformer, 0, layer + 1, x, *params)
            y[:, 1:, feature].float().mean().backward()
            for p in params:
                p.grad = None

        def oracle():
            img.grad = None
            _, loss = featviz_oracle(img, sdv, vcfg, layer, feature)
            loss.backward()

        r = dict(layer=layer, batch=a.batch, hip_ms=timed(hip, a.iters), full_bwd_ms=timed(full_bwd, a.iters),
                 oracle_fp32_ms=timed(oracle, max(2, a.iters // 2)))
        r["speedup_vs_full_bwd"] = r["full_bwd_ms"] / r["hip_ms"]
        r["speedup_vs_oracle"] = r["oracle_fp32_ms"] / r["hip_ms"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    assert all(p.grad is None for p in model.parameters())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
