#!/usr/bin/env python3
"""Generate tests/golden/distill_grad.npz by RUNNING THE REFERENCE's DistillClipLoss (build container only).

    python tests/golden/make_golden_distill.py --ref REFERENCE_ROOT

The vendored torch ``open_clip.loss.DistillClipLoss`` (loss.py:180-216) is imported as make_golden.py does and run in float64 with
``world_size`` gloo processes: each rank holds its [b, E] student rows (leaves) and its [b, Et] teacher rows (no gradient), calls the
class and differentiates ``g_c contrastive + g_d distill`` for the upstream pair of tests/distill_restate.GRADS.  Per rank, what
autograd leaves before any DDP averaging: both losses and the gradients of the image features, the text features and
``logit_scale`` (the multiplier, a leaf).

Before a case is stored its teacher is checked to matter: in float64 the distill loss must move by at least 5 % when the teacher's
softmax is replaced by a uniform one and when it is replaced by the one-hot labels, on every rank.

Kept small: the inputs are not stored but regenerated from their seed by tests/distill_restate.case_inputs and checked against the
stored sums; the gradients are stored as float32 (the kernels under test are fp32) next to their float64 sums, the scalars as float64.
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
import distill_restate as DR                          # noqa: E402

KEYS = ("img", "txt", "timg", "ttxt")


def _worker(rank, ws, store, ref_root, case, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=ws)
    _, lossmod, _ = mg.import_reference(ref_root)
    name, _, b, e, et, local_loss, gwg, s, st, seed = case
    img, txt, t_img, t_txt = DR.case_inputs(ws, b, e, et, seed)
    sl = slice(rank * b, (rank + 1) * b)
    li, lt = img[sl].clone().requires_grad_(True), txt[sl].clone().requires_grad_(True)
    sc = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    fn = lossmod.DistillClipLoss(local_loss=local_loss, gather_with_grad=gwg, rank=rank, world_size=ws)
    c, d = fn(li, lt, sc, t_img[sl].clone(), t_txt[sl].clone(), torch.tensor(st, dtype=torch.float64))
    (DR.GRADS[0] * c + DR.GRADS[1] * d).backward()
    q.put((rank, (float(c.detach()), float(d.detach()), li.grad.numpy(), lt.grad.numpy(), float(sc.grad))))
    dist.barrier()
    dist.destroy_process_group()


def teacher_matters(case):
    """Relative change of the distill loss, per rank, under a uniform and under a one-hot (label) teacher: both >= 5 %."""
    name, ws, b, e, et, local_loss, gwg, s, st, seed = case
    inputs = DR.case_inputs(ws, b, e, et, seed)
    worst = [float("inf"), float("inf")]
    for r in range(ws):
        args, off = DR.rank_args(inputs, r, ws, local_loss)
        d = float(DR.strip_losses(*args, s, st, off)[1])
        rows, n = args[0].shape[0], args[2].shape[0]
        uniform = torch.full((rows, n), 1.0 / n, dtype=torch.float64)
        onehot = torch.zeros(rows, n, dtype=torch.float64)
        onehot[torch.arange(rows), torch.arange(rows) + off] = 1.0
        for k, qm in enumerate((uniform, onehot)):
            worst[k] = min(worst[k], abs(float(DR.distill_under(qm, qm, *args[:4], s)) - d) / d)
    assert min(worst) >= 0.05, (name, worst)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    res = {"cases": np.array([c[0] for c in DR.CASES]), "grads": np.array(DR.GRADS, dtype=np.float64)}
    for case in DR.CASES:
        name, ws, b, e, et, local_loss, gwg, s, st, seed = case
        worst = teacher_matters(case)
        inputs = DR.case_inputs(ws, b, e, et, seed)
        with tempfile.TemporaryDirectory() as d:
            q = ctx.Queue()
            ps = [ctx.Process(target=_worker, args=(r, ws, os.path.join(d, "store"), a.ref, case, q)) for r in range(ws)]
            [p.start() for p in ps]
            got = dict(q.get(timeout=600) for _ in range(ws))
            [p.join() for p in ps]
        print(f"{name}: contrastive {[round(got[r][0], 5) for r in range(ws)]} distill {[round(got[r][1], 5) for r in range(ws)]}  "
              f"uniform teacher {worst[0] * 100:.0f} % off, one-hot teacher {worst[1] * 100:.1f} % off")
        for key, x in zip(KEYS, inputs):
            res[f"{name}_{key}_sum"] = np.float64(x.sum())
            res[f"{name}_{key}_abs_sum"] = np.float64(x.abs().sum())
        res.update({f"{name}_contrastive": np.array([got[r][0] for r in range(ws)], dtype=np.float64),
                    f"{name}_distill": np.array([got[r][1] for r in range(ws)], dtype=np.float64),
                    f"{name}_dimg": np.stack([got[r][2] for r in range(ws)]).astype(np.float32),
                    f"{name}_dtxt": np.stack([got[r][3] for r in range(ws)]).astype(np.float32),
                    f"{name}_dscale": np.array([got[r][4] for r in range(ws)], dtype=np.float64)})
        for k, key in ((2, "dimg"), (3, "dtxt")):            # float64 sums of the gradients, which themselves are stored as float32
            res[f"{name}_{key}_sum"] = np.array([got[r][k].sum() for r in range(ws)], dtype=np.float64)
            res[f"{name}_{key}_abs_sum"] = np.array([np.abs(got[r][k]).sum() for r in range(ws)], dtype=np.float64)
    out = os.path.join(HERE, "distill_grad.npz")
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
