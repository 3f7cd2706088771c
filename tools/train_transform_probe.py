"""Timing of the batched training transform against the per-image preprocess it sits beside, on one MI355X:
64 images of 480 x 640 -> 224 x 224, bicubic, full-frame boxes, no colour operations (the geometry of DESIGN.md §7's front-end row).

  python tools/train_transform_probe.py [--out profiles/train_transform_time.json]

Three things are timed, in alternating rounds inside one process, each round ending in a device synchronise:
  preprocess            per-image ov_preprocess_image (2 launches per image) on device-resident images, as tools/frontend_probe.py
  launch                ov_train_transform alone (4 launches for the batch) on inputs already staged on the device
  train_transform       the whole call from host arrays: packing into the pinned buffer, two copies, the kernels
and for train_transform also the host-side time of the call (until it returns, nothing synchronised).  The outputs of the two paths
are compared bit for bit first.  Launch counts are read off the code (csrc/preprocess.hip, csrc/augment.hip), not traced."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd import augment as A                      # noqa: E402
from openvision_amd.config import DEFAULT_PREPROCESS as PP   # noqa: E402
from openvision_amd.preprocess import preprocess             # noqa: E402

B, H, W, S, INTERP, DEV = 64, 480, 640, 224, "bicubic", "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_transform_time.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_transform_probe: needs the GPU (a CPU run measures nothing)")
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(B)]
    dev_imgs = [torch.from_numpy(x).to(DEV) for x in imgs]
    shapes = np.array([[H, W]] * B, np.int32)
    boxes = np.array([[0, 0, H, W]] * B, np.int32)
    ops, factors = np.zeros((B, 4), np.int32), np.zeros((B, 4), np.float32)
    mean, std = PP["mean"], PP["std"]
    out = torch.empty(B, 3, S, S, device=DEV)
    pixels, tables = A.stage(imgs, [shapes, boxes, ops, factors], torch.device(DEV))

    def parent():
        return preprocess(dev_imgs, S, mean, std, "squash", INTERP, device=DEV)

    def launch():
        A.launch(pixels, tables, boxes, ops, S, INTERP, mean, std, out)

    def whole():
        return A.train_transform(imgs, S, mean, std, INTERP, boxes=boxes, color_ops=(ops, factors), device=DEV)

    same = bool(torch.equal(parent(), whole()))
    launch()
    same = same and bool(torch.equal(parent(), out))
    torch.cuda.synchronize()

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t2 - t0) / reps, (t1 - t0) / reps

    for fn in (parent, launch, whole):                      # warm every shape the timed window uses
        timed(fn, 3)
    res = {"parent": [], "launch": [], "whole": [], "whole_host": [], "parent_host": [], "launch_host": []}
    for _ in range(a.rounds):
        for name, fn in (("parent", parent), ("launch", launch), ("whole", whole)):
            t, th = timed(fn, a.reps)
            res[name].append(t)
            res[name + "_host"].append(th)
    ms = {k: {"median_ms": statistics.median(v) * 1e3, "min_ms": min(v) * 1e3, "max_ms": max(v) * 1e3} for k, v in res.items()}
    rec = {"what": f"{B} x ({H}x{W} -> {S}x{S}), {INTERP}, full-frame boxes, no colour operations, fp32 out, one MI355X",
           "method": f"{a.rounds} alternating rounds x {a.reps} calls, host clock around calls ending in a device synchronise; "
                     "*_host = time until the calls returned, before the synchronise",
           "outputs_bitwise_equal": same,
           "launches": {"preprocess": 2 * B, "train_transform": 4, "train_transform_with_contrast": 5},
           "copies": {"preprocess": "none timed (device-resident images)", "launch": "none (staged once)",
                      "train_transform": f"2 host-to-device ({B * H * W * 3} pixel bytes + {B * (8 + 8 + 16 + 16 + 16)} table bytes)"},
           "preprocess_per_image": ms["parent"], "preprocess_per_image_host": ms["parent_host"],
           "ov_train_transform": ms["launch"], "ov_train_transform_host": ms["launch_host"],
           "train_transform_from_host_arrays": ms["whole"], "train_transform_from_host_arrays_host": ms["whole_host"],
           "images_per_second": {"preprocess_per_image": B / statistics.median(res["parent"]),
                                 "ov_train_transform": B / statistics.median(res["launch"]),
                                 "train_transform_from_host_arrays": B / statistics.median(res["whole"])}}
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
