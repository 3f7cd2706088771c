"""Drop path on the complete training step (forward keeping activations + InfoNCE + backward + FusedAdamW), ONE GPU, L/14@224 at
B = 256 by default (MODEL / BATCH select another preset / batch; REPS the steps per rate, default 7).

The rates 0, 0.1, 0.2, 0.4 (both towers) alternate within one process, a fresh table per tower and step, drawn from a seeded
generator and handed to ``clip_forward`` (so that the counts are known); per rate the median and the range of the step time are
printed (host clock around a step that ends in a device synchronise).  Beside them:

  floor   the step under tables that keep NOBODY: every branch is a copy and zero-filled gradients -- what drop path cannot remove
          (front end, heads, loss, optimiser, the copies);
  ideal   floor + f (t(rate 0) - floor), f = the kept fraction of the branch work, computed exactly from the drawn counts with each
          tower's branches weighted by layers x tokens x width^2;
  glue    the step's ov_sample_gather / ov_sample_scatter_axpy launches replayed ALONE at the last step's counts, between device
          events (per compact branch: forward 1 gather + 1 scatter, backward 2 gathers + 1 scatter) -- not a trace of the step.

One JSON line per rate at the end."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd import _lib, preset, synth, training          # noqa: E402
from openvision_amd._lib import check, ptr, stream_ptr            # noqa: E402
from openvision_amd.loss import ClipLoss                          # noqa: E402
from openvision_amd.model import create_model                     # noqa: E402

name = os.environ.get("MODEL", "vit-large-patch14-224")
B = int(os.environ.get("BATCH", "256"))
REPS = int(os.environ.get("REPS", "7"))
RATES = (0.0, 0.1, 0.2, 0.4)
cfg = preset(name)
m = create_model(cfg, device="cuda", state_dict=synth.make_state_dict(cfg)).train()
S = cfg["vision_cfg"]["image_size"]
img = synth.make_images(B, S, seed=1).to("cuda")
tok = synth.make_captions(B, seed=1).to("cuda")
loss_fn = ClipLoss()
opt = training.FusedAdamW(m, lr=1e-6, clip_norm=1.0)
gen = torch.Generator().manual_seed(1)
towers = (m.visual.transformer, m.transformer)
tokens = (m.visual.num_patches + 1, tok.shape[1])
weight = [len(t.resblocks) * n * t.width ** 2 for t, n in zip(towers, tokens)]


def tables(rate, nobody=False):
    out = []
    for t in towers:
        t.set_drop_path(rate)
        if nobody:
            keep = torch.zeros(len(t.resblocks), 2, B, dtype=torch.bool)
            out.append(training.drop_path_table(t, B, keep=keep, scale=[1.0] * len(t.resblocks)))
        else:
            out.append(training.drop_path_table(t, B, generator=gen))
    return tuple(out)


def kept_fraction(drop):
    num = sum(w * (1.0 if d is None else float(d.keep.float().mean())) for w, d in zip(weight, drop))
    return num / sum(weight)


def step(rate, nobody=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    drop = tables(rate, nobody)
    opt.zero_grad()
    fi, ft, sc = training.clip_forward(m, img, tok, drop=drop)
    loss = loss_fn(fi, ft, sc)
    loss.backward()
    opt.step(grad_scale=opt.all_reduce_gradients(1))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, drop, float(loss.detach())


def glue_ms(drop):
    """The glue launches of one step at these tables' counts, alone between two events."""
    lib = _lib.load()
    total = 0.0
    for t, n, d in zip(towers, tokens, drop):
        if d is None:
            continue
        D = t.width
        idx, slot = d.device_tables("cuda")
        a, b, c = (torch.randn(B * n, D, device="cuda").to(torch.bfloat16) for _ in range(3))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(d.layers):
            for j in range(2):
                k, sc = d.counts[i][j], float(d.scale[i])
                if k == B and sc == 1.0 or k == 0:
                    continue
                ii, ss = idx[i, j], slot[i, j]
                check(lib.ov_sample_gather(ptr(a), ptr(ii), ptr(b), B, k, n, D, 1.0, stream_ptr()), "gather")          # forward: x
                check(lib.ov_sample_scatter_axpy(ptr(a), ptr(b), ptr(ss), ptr(c), B, k, n, D, sc, stream_ptr()), "scatter")
                check(lib.ov_sample_gather(ptr(a), ptr(ii), ptr(b), B, k, n, D, sc, stream_ptr()), "gather")           # backward: dy / keep
                check(lib.ov_sample_gather(ptr(c), ptr(ii), ptr(b), B, k, n, D, 1.0, stream_ptr()), "gather")          # backward: x
                check(lib.ov_sample_scatter_axpy(ptr(a), ptr(b), ptr(ss), ptr(c), B, k, n, D, 1.0, stream_ptr()), "scatter")
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
    return total


for r in RATES:                       # every shape of the timed window once (a table's counts change the GEMM shapes: twice each)
    step(r)
    step(r)
step(0.0, nobody=True)
times = {r: [] for r in RATES}
fracs = {r: [] for r in RATES}
floor, last = [], {}
for rep in range(REPS):
    for r in RATES:
        ms, drop, _ = step(r)
        times[r].append(ms)
        fracs[r].append(kept_fraction(drop) if r > 0 else 1.0)
        last[r] = drop
    floor.append(step(0.0, nobody=True)[0])
t_floor, t0 = statistics.median(floor), statistics.median(times[0.0])
print(f"{name} B={B}: floor (every branch dropped) {t_floor:.2f} ms [{min(floor):.2f}, {max(floor):.2f}]", flush=True)
for r in RATES:
    med, f = statistics.median(times[r]), statistics.mean(fracs[r])
    rec = dict(model=name, batch=B, rate=r, reps=REPS, step_ms_median=round(med, 3), step_ms_min=round(min(times[r]), 3),
               step_ms_max=round(max(times[r]), 3), kept_fraction=round(f, 4), ideal_ms=round(t_floor + f * (t0 - t_floor), 3),
               glue_ms_replayed=round(glue_ms(last[r]), 3) if r > 0 else 0.0, floor_ms=round(t_floor, 3))
    print(json.dumps(rec), flush=True)
