#!/usr/bin/env python3
"""Generate tests/golden/siglip_grad.npz by RUNNING THE REFERENCE's SigLipLoss over gloo (build container only).

    python tests/golden/make_golden_siglip.py --ref REFERENCE_ROOT

The reference's ``open_clip.loss.SigLipLoss`` (loss.py:307-414) is imported as make_golden.py does and run in float64 with
``world_size`` gloo processes, each holding its [b, E] slice of the case's features: the text blocks travel round its
neighbour-exchange ring (``bidir`` True: both directions with the remainder branch at even world sizes; False: one direction).
Per rank, what its autograd leaves before any DDP averaging: the loss and the gradients of the image features, the text
features (the ring's backward has already returned every block's gradient to its owner), ``logit_scale`` (the multiplier, a
leaf) and ``logit_bias``.

Kept small: the inputs are not stored but regenerated from their seed by tests/siglip_restate.case_inputs, and checked against
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
import siglip_restate as SR                           # noqa: E402


def _worker(rank, ws, store, ref_root, case, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=ws)
    _, lossmod, _ = mg.import_reference(ref_root)
    name, _, b, e, s, beta, bidir, seed = case
    img, txt = SR.case_inputs(ws, b, e, seed)
    li = img[rank * b:(rank + 1) * b].clone().requires_grad_(True)
    lt = txt[rank * b:(rank + 1) * b].clone().requires_grad_(True)
    sc = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    bi = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    loss = lossmod.SigLipLoss(rank=rank, world_size=ws, bidir=bidir)(li, lt, sc, bi)
    loss.backward()
    q.put((rank, (float(loss.detach()), li.grad.numpy(), lt.grad.numpy(), float(sc.grad), float(bi.grad))))
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    res = {"cases": np.array([c[0] for c in SR.CASES])}
    for case in SR.CASES:
        name, ws, b, e, s, beta, bidir, seed = case
        img, txt = SR.case_inputs(ws, b, e, seed)
        with tempfile.TemporaryDirectory() as d:
            q = ctx.Queue()
            ps = [ctx.Process(target=_worker, args=(r, ws, os.path.join(d, "store"), a.ref, case, q)) for r in range(ws)]
            [p.start() for p in ps]
            got = dict(q.get(timeout=600) for _ in range(ws))
            [p.join() for p in ps]
        pos = (s * (img * txt).sum(-1) + beta)
        print(f"{name}: loss {[round(got[r][0], 6) for r in range(ws)]}  positive logits {pos.min():.1f}..{pos.max():.1f}")
        res.update({f"{name}_img_sum": np.float64(img.sum()), f"{name}_img_abs_sum": np.float64(img.abs().sum()),
                    f"{name}_txt_sum": np.float64(txt.sum()), f"{name}_txt_abs_sum": np.float64(txt.abs().sum()),
                    f"{name}_loss": np.array([got[r][0] for r in range(ws)], dtype=np.float64),
                    f"{name}_dimg": np.stack([got[r][1] for r in range(ws)]).astype(np.float32),
                    f"{name}_dtxt": np.stack([got[r][2] for r in range(ws)]).astype(np.float32),
                    f"{name}_dscale": np.array([got[r][3] for r in range(ws)], dtype=np.float64),
                    f"{name}_dbias": np.array([got[r][4] for r in range(ws)], dtype=np.float64)})
    out = os.path.join(HERE, "siglip_grad.npz")
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
