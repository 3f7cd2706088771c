#!/usr/bin/env python3
"""Generate tests/golden/multicap_grad.npz by RUNNING THE REFERENCE's ClipLoss once per caption set (build container only).

    python tests/golden/make_golden_multicap.py --ref REFERENCE_ROOT

The contrastive term OpenVision trains with (``bidirectional_contrastive_loss`` with ``local_loss``, src/losses/common.py:120-189)
is JAX, and jax is not installed anywhere this project runs.  It equals the mean over the caption sets of the one-caption InfoNCE,
so the pinned reference is the vendored torch ``open_clip.loss.ClipLoss`` (loss.py:66-131), imported as make_golden.py does and run
in float64 with ``world_size`` gloo processes: each rank holds its [b, E] image rows and its stacked [C b, E] text rows, calls
ClipLoss on (image, text set c) for every c and averages.  Per rank, what autograd leaves before any DDP averaging: the loss and
the gradients of the image features, the stacked text features and ``logit_scale`` (the multiplier, a leaf).

Kept small: the inputs are not stored but regenerated from their seed by tests/multicap_restate.case_inputs and checked against
the stored sums; results are stored as float32 (the kernels under test are fp32).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True          # no __pycache__ under tests/golden/ (fixtures live there)

import make_golden as mg                              # noqa: E402
import multicap_restate as MR                         # noqa: E402


def _worker(rank, ws, store, ref_root, case, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=ws)
    _, lossmod, _ = mg.import_reference(ref_root)
    name, _, b, e, c, local_loss, gwg, s, seed = case
    img, sets = MR.case_inputs(ws, b, e, c, seed)
    li = img[rank * b:(rank + 1) * b].clone().requires_grad_(True)
    lt = MR.stack_local(sets, rank, b).clone().requires_grad_(True)
    sc = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    fn = lossmod.ClipLoss(local_loss=local_loss, gather_with_grad=gwg, rank=rank, world_size=ws)
    loss = sum(fn(li, lt[k * b:(k + 1) * b], sc) for k in range(c)) / c
    loss.backward()
    q.put((rank, (float(loss.detach()), li.grad.numpy(), lt.grad.numpy(), float(sc.grad))))
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    res = {"cases": np.array([c[0] for c in MR.CASES])}
    for case in MR.CASES:
        name, ws, b, e, c, local_loss, gwg, s, seed = case
        img, sets = MR.case_inputs(ws, b, e, c, seed)
        with tempfile.TemporaryDirectory() as d:
            q = ctx.Queue()
            ps = [ctx.Process(target=_worker, args=(r, ws, os.path.join(d, "store"), a.ref, case, q)) for r in range(ws)]
            [p.start() for p in ps]
            got = dict(q.get(timeout=600) for _ in range(ws))
            [p.join() for p in ps]
        print(f"{name}: loss {[round(got[r][0], 6) for r in range(ws)]}  log N {np.log(ws * b):.3f}")
        res.update({f"{name}_img_sum": np.float64(img.sum()), f"{name}_img_abs_sum": np.float64(img.abs().sum()),
                    f"{name}_txt_sum": np.float64(sets.sum()), f"{name}_txt_abs_sum": np.float64(sets.abs().sum()),
                    f"{name}_loss": np.array([got[r][0] for r in range(ws)], dtype=np.float64),
                    f"{name}_dimg": np.stack([got[r][1] for r in range(ws)]).astype(np.float32),
                    f"{name}_dtxt": np.stack([got[r][2] for r in range(ws)]).astype(np.float32),
                    f"{name}_dscale": np.array([got[r][3] for r in range(ws)], dtype=np.float64)})
    out = os.path.join(HERE, "multicap_grad.npz")
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
