#!/usr/bin/env python3
"""Generate tests/golden/lock_groups_tiny16_160.json by RUNNING THE REFERENCE's LiT locking (build container only).

    python tests/golden/make_golden_lock.py --ref REFERENCE_ROOT

The reference's ``CLIP.lock_image_tower(unlocked_groups)`` (model.py:256-258) calls ``VisionTransformer.lock`` (transformer.py:542-572):
every image-tower parameter is frozen, then the last ``unlocked_groups`` of [conv1, class_embedding, positional_embedding, ln_pre],
resblocks[0], ..., resblocks[-2], [resblocks[-1], ln_post], proj are unlocked again.  The reference CLIP is built as make_golden.py
builds it (Ti/16@160, the 'v1' formula weights); for each k the sorted names of the parameters that still require grad are stored.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True          # no __pycache__ under tests/golden/ (fixtures live there)

import make_golden as mg                              # noqa: E402
from openvision_amd import config as ovcfg            # noqa: E402

PRESET = "vit-tiny-patch16-160"


def unlocked_counts(layers: int):
    return [0, 1, 2, 3, layers, layers + 1, layers + 2, layers + 5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "lock_groups_tiny16_160.json"))
    a = ap.parse_args()
    m, _, _ = mg.import_reference(a.ref)
    cfg = ovcfg.preset(PRESET)
    layers = cfg["vision_cfg"]["layers"]
    out = {"preset": PRESET, "layers": layers, "trainable": {}}
    for k in unlocked_counts(layers):
        model = mg.build_ref(m, cfg)
        for p in model.parameters():
            p.requires_grad_(True)
        model.lock_image_tower(unlocked_groups=k)
        out["trainable"][str(k)] = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    out["all"] = sorted(n for n, _ in mg.build_ref(m, cfg).named_parameters())
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out, {k: len(v) for k, v in out["trainable"].items()})


if __name__ == "__main__":
    main()
