#!/usr/bin/env python3
"""Feature-visualisation step cost at L/14@224, B = 8 (the script's RepeatBatch(8)): ms per optimisation step (objective forward +
backward to the pixels) for

  hip        openvision_amd.visualize.MLPFeatureLoss: blocks [0, layer) + the tap block's attention half + the tap kernels, input-only
             backward (no weight gradients, nothing of the tap block's MLP but one column)
  full_bwd   the composition the training path offers: blocks [0, layer] as one _TowerFn node (ov_tower_forward_saving /
             ov_tower_backward, weight gradients included, the tap block's whole MLP) -- what the step costs without the tap path
  oracle     fp32 torch eager on the device (oracle/clip_ref.py pieces: the reference's arithmetic, not its hook machinery)

    python tools/featviz_probe.py [--layers 0,11,23] [--iters 10] [--out featviz_probe.json]

With ``--loop`` the whole optimisation step instead, on one device in alternating rounds:

  parent     the script's loop body with MLPFeatureLoss in it: the eager augmentations (their draws and uploads per step, as the script
             makes them), the eager front end of mlp_feature, TotalVariation, torch.optim.Adamax, CosineAnnealingLR and the clamp
  fused      openvision_amd.visualize.FeatureVisualizer.step

    python tools/featviz_probe.py --loop [--layers 0,11,23] [--rounds 5] [--iters 20] [--window-ms 500] [--out featviz_loop.json]

(a window: as many steps as keep the fused loop busy for --window-ms, at least --iters)

Launches per step around the objective's own, counted from the code: the fused step makes 11 (ov_viz_augment, ov_gemm,
ov_patch_keep_assemble, ov_convert, ov_viz_tv, ov_convert, ov_patch_keep_assemble_backward, the transpose and the GEMM of
ov_linear_backward, ov_viz_augment_backward, ov_adamax_clip_step).  The parent's forward makes 51 torch calls that launch (uploads 3,
their arithmetic 10; repeat, sub, div, add, roll 2; the patch gather 1, _LinearFn's zeros, copy, GEMM and slice-to-float 4, cat, add,
cast and clone 4; TotalVariation's 4 sub, 4 norm, 4 mean, 3 add, mul, div; the loss's sum, neg, div, 2 mul, add), autograd answers most
of them with at least one launch each, and the update adds 7 (Adamax's lerp, mul, abs, add, maximum, addcdiv; the clamp).
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


FUSED_GLUE_LAUNCHES, PARENT_FORWARD_CALLS, PARENT_UPDATE_CALLS = 11, 51, 7         # counted from the code: see the module docstring


def loop_rows(model, layers, rounds, min_iters, window_ms, repeat=8, size=224, lr=1.0, c_tv=5e-5):
    """ms per optimisation step of the parent composition and of the fused loop, `rounds` alternating windows each.  A window is as many
    steps as make the FASTER side (the fused loop) run for `window_ms`, at least `min_iters`: a shallow layer's step is a third of a
    millisecond, and a window of a few milliseconds would time the clock."""
    import math
    import random

    import viz_restate as V
    from openvision_amd.visualize import FeatureVisualizer, new_init

    rows = []
    for layer in layers:
        feature = 37
        torch.manual_seed(6247423)
        random.seed(6247423)
        trial = FeatureVisualizer(model, layer, feature, steps=2 * min_iters, lr=lr, tv_coefficient=c_tv, repeat=repeat)
        trial.begin(new_init(size, 1))
        at = iter(range(2 * min_iters))
        timed(lambda: trial.step(next(at)), min_iters, warmup=0)
        iters = max(min_iters, math.ceil(window_ms / timed(lambda: trial.step(next(at)), min_iters, warmup=0)))
        total = (rounds + 1) * iters
        viz = FeatureVisualizer(model, layer, feature, steps=total, lr=lr, tv_coefficient=c_tv, repeat=repeat)
        start = new_init(size, 1)
        viz.begin(start)
        img = start.clone().requires_grad_(True)
        opt = torch.optim.Adamax([img], lr=lr, betas=(0.5, 0.99), eps=1e-8)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, total, 0.0)
        lf = MLPFeatureLoss(model, layer, feature)
        state = {"rem": 398, "i": 0}

        def parent():
            opt.zero_grad()
            mean = (torch.rand(repeat, 3, 1, 1).cuda() - 0.5) * 2 * 1.0
            std = ((torch.rand(repeat, 3, 1, 1).cuda() - 0.5) * 2 * 1.0).exp()
            noise = torch.randn(repeat, 3, 1, 1).cuda() * state["rem"] * 0.5 / 400
            state["rem"] = (state["rem"] - 1 + 400) % 400
            aug = V.augment(img, mean, std, noise, random.randint(-32, 32), random.randint(-32, 32), repeat)
            loss = lf(aug) + c_tv * V.tv_value(aug, size)
            loss.backward()
            opt.step()
            sched.step()
            img.data = img.data.clamp(0, 1)

        def fused():
            viz.step(state["i"])
            state["i"] += 1

        windows = {"parent": [], "fused": []}
        for rnd in range(rounds + 1):                     # window 0 warms both up and is dropped
            for name, fn in (("parent", parent), ("fused", fused)):
                windows[name].append(timed(fn, iters, warmup=0))
        r = dict(mode="loop", layer=layer, batch=repeat, iters=iters, parent_ms=windows["parent"][1:], fused_ms=windows["fused"][1:],
                 fused_glue_launches=FUSED_GLUE_LAUNCHES, parent_forward_calls=PARENT_FORWARD_CALLS,
                 parent_update_calls=PARENT_UPDATE_CALLS)
        r["parent_median_ms"] = sorted(r["parent_ms"])[rounds // 2]
        r["fused_median_ms"] = sorted(r["fused_ms"])[rounds // 2]
        r["speedup"] = r["parent_median_ms"] / r["fused_median_ms"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    assert all(p.grad is None for p in model.parameters())
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="0,11,23")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default="")
    ap.add_argument("--loop", action="store_true", help="time the whole optimisation step: the parent composition against the fused loop")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=500.0, help="--loop: least length of a timing window of the faster side")
    a = ap.parse_args()
    cfg = preset("vit-large-patch14-224")
    sd = synth.make_state_dict(cfg, 0, "v1")
    model = create_model(cfg, device=DEV, state_dict=sd)
    for p in model.parameters():
        p.requires_grad_(True)           # as in the script: the model's parameters are leaves (the tap path writes no .grad)
    if a.loop:
        rows = loop_rows(model, [int(x) for x in a.layers.split(",")], a.rounds, a.iters, a.window_ms, repeat=a.batch)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        return
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
