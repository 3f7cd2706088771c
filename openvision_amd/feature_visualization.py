"""Counterpart of the fork's ``ov-feature-visualization.py`` on the MI355X path.

    python -m openvision_amd.feature_visualization --use_model DIR --layer_range 0-23 --feature_range 37-42 [--steps 400] [--lr 1.0]
        [--tv 1.0] [--coeff 0.00005] [--output_folder ovFeatureViz] [--save_intermediate] [--deterministic]

For every (layer, feature) pair the script builds its augmentations, draws a random image and runs 401 Adamax steps that raise one
hidden unit of one vision block's MLP (ov-feature-visualization.py:203-221); here the pair is one ``visualize.FeatureVisualizer`` and
every step is HIP launches.  The arguments, the order of the random draws (``--deterministic`` seeds as the script's
``fix_random_seed(6247423)`` does), the printed loss rows (every 10 steps) and the file names
``{folder}/{name}_L{layer}_F{feature}.png`` and, with ``--save_intermediate``, ``steps/{name}_L{layer}-F{feature}/step{i}.png`` are the
script's.  ``DIR`` is loaded through ``checkpoint.from_pretrained``.  PNGs are written with Pillow, a pixel as ``x * 255 + 0.5`` clamped
and truncated to uint8 (torchvision's ``save_image`` arithmetic).
"""
from __future__ import annotations

import argparse
import os
import re
from typing import List, Optional, Sequence

import numpy as np
import torch

from .visualize import SEED, FeatureVisualizer, fix_random_seed, new_init  # noqa: F401  (SEED, fix_random_seed: this module's names too)


def parse_range(text: str) -> List[int]:
    """'5-10' (inclusive) or '5,6,8'."""
    if "-" in text:
        lo, hi = map(int, text.split("-"))
        return list(range(lo, hi + 1))
    return [int(t) for t in text.split(",")]


def safe_name(path: str, max_len: int = 64) -> str:
    return re.sub(r"[^a-zA-Z0-9\-_.]+", "_", os.path.basename(os.path.normpath(path)))[:max_len]


def to_uint8(image: torch.Tensor) -> np.ndarray:
    """[1, 3, S, S] or [3, S, S] in [0, 1] -> uint8 [S, S, 3]."""
    x = image.detach().float().reshape(-1, *image.shape[-2:])
    return (x * 255 + 0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).cpu().numpy()


def save_png(image: torch.Tensor, path: str) -> None:
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(to_uint8(image)).save(path)


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(description="OpenVision model feature activation max visualization (MI355X)")
    ap.add_argument("--use_model", required=True, help="directory with open_clip_config.json and the weights")
    ap.add_argument("--layer_range", default="0-23")
    ap.add_argument("--feature_range", default="37-42")
    ap.add_argument("--steps", default=400, type=int)
    ap.add_argument("--lr", default=1.0, type=float)
    ap.add_argument("--tv", default=1.0, type=float)
    ap.add_argument("--coeff", default=0.00005, type=float, help="the total-variation term is weighted tv * coeff")
    ap.add_argument("--output_folder", default="ovFeatureViz")
    ap.add_argument("--save_intermediate", action="store_true")
    ap.add_argument("--deterministic", action="store_true")
    a = ap.parse_args(argv)
    from .checkpoint import from_pretrained
    os.makedirs(a.output_folder, exist_ok=True)
    name = safe_name(a.use_model)
    print(name)
    if a.deterministic:
        fix_random_seed()
    model, _ = from_pretrained(a.use_model, device="cuda:0")
    size = model.visual.image_size[0]
    for layer in parse_range(a.layer_range):
        for feature in parse_range(a.feature_range):
            print(f"Generating visualization for Layer {layer}, Feature {feature}...")
            viz = FeatureVisualizer(model, layer, feature, steps=a.steps, lr=a.lr, tv_coefficient=a.coeff * a.tv)
            image = new_init(size, 1)
            print("#i\tloss\tMLPFeat\tTotalVariation", flush=True)
            steps_dir = os.path.join("steps", f"{name}_L{layer}-F{feature}")
            image = viz(image, print_every=10, on_print=lambda i, row: print(f"{i}\t" + "\t".join(f"{v:.4g}" for v in row), flush=True),
                        save_every=10 if a.save_intermediate else 0,
                        on_save=lambda i, img: save_png(img, os.path.join(steps_dir, f"step{i}.png")))
            save_png(image, os.path.join(a.output_folder, f"{name}_L{layer}_F{feature}.png"))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
