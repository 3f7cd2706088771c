"""Timing of the distillation loss kernels (ov_distill_loss / ov_distill_loss_backward) against InfoNCE's (ov_clip_loss /
ov_clip_loss_backward) on the student operands in the same process, at the recipe's per-GPU shape: b = 4096 of N = 32768, E = 768,
Et = 1024.  Each call is bracketed by its own pair of device events after a warm-up; the figure is the median over the repeats.
Logit work by arithmetic alone: the student's tiles cost what InfoNCE's do, the teacher's tiles Et / E of that, once in the lse
pass, once in the forward and once per side in the backward."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hipops as H                                          # noqa: E402
from openvision_amd import _lib                             # noqa: E402
from openvision_amd._lib import check, ptr, stream_ptr      # noqa: E402


def distill_fns(x, y, u, v, s, st, off, gathered=True):
    """x / u: local (img, txt) of student / teacher; y / v: gathered (img, txt).  Contiguous operands."""
    lib = _lib.load()
    (b, e), et, n = x[0].shape, u[0].shape[1], y[0].shape[0]
    nf, nb = lib.ov_distill_loss_workspace_bytes(b, n), lib.ov_distill_loss_backward_workspace_bytes(b, n)
    wf = torch.empty(nf + 16, dtype=torch.uint8, device="cuda")
    wb = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    terms = torch.empty(12, b, dtype=torch.float32, device="cuda")
    d_img, d_txt = torch.empty_like(x[0]), torch.empty_like(x[1])
    d_all = torch.empty(2, n, e, dtype=torch.float32, device="cuda")
    d_s = torch.empty(1, dtype=torch.float32, device="cuda")
    ones = torch.ones(2, dtype=torch.float32, device="cuda")

    def fwd():
        check(lib.ov_distill_loss(ptr(x[0]), ptr(x[1]), ptr(y[0]), ptr(y[1]), e, ptr(u[0]), ptr(u[1]), ptr(v[0]), ptr(v[1]), et, b, n, e, et,
                                  ptr(s), ptr(st), off, ptr(out[0:]), ptr(out[1:]), ptr(terms), ptr(wf), nf, stream_ptr()))

    def bwd():
        check(lib.ov_distill_loss_backward(ptr(x[0]), ptr(x[1]), ptr(y[0]), ptr(y[1]), e, ptr(u[0]), ptr(u[1]), ptr(v[0]), ptr(v[1]), et, b, n,
                                           e, et, ptr(s), ptr(st), off, ptr(terms), ptr(ones[0:]), ptr(ones[1:]), ptr(d_img), ptr(d_txt),
                                           ptr(d_all[0]) if gathered else None, ptr(d_all[1]) if gathered else None, e if gathered else 0,
                                           ptr(d_s), ptr(wb), nb, stream_ptr()))
    return fwd, bwd


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    b, N, E, Et, off, reps = 4096, 32768, 768, 1024, 4096, 7
    g = torch.Generator(device="cuda").manual_seed(0)
    nrm = torch.nn.functional.normalize

    def pair(width):
        a = nrm(torch.randn(N, width, device="cuda", generator=g), dim=-1)
        return a, nrm(a * 0.5 + torch.randn(N, width, device="cuda", generator=g) * 0.05, dim=-1)

    y, v = pair(E), pair(Et)
    x = tuple(t[off:off + b].contiguous() for t in y)
    u = tuple(t[off:off + b].contiguous() for t in v)
    s, st = torch.full((1,), 1 / 0.07, device="cuda"), torch.full((1,), 20.0, device="cuda")
    df, db = distill_fns(x, y, u, v, s, st, off)
    _, db_local = distill_fns(x, y, u, v, s, st, off, gathered=False)
    df()
    _, terms = H.clip_loss(x[0], x[1], y[0], y[1], 1 / 0.07, off)
    cf = lambda: H.clip_loss(x[0], x[1], y[0], y[1], 1 / 0.07, off)                              # noqa: E731
    cb = lambda: H.clip_loss_backward(x[0], x[1], y[0], y[1], 1 / 0.07, off, terms)              # noqa: E731
    cb_local = lambda: H.clip_loss_backward(x[0], x[1], y[0], y[1], 1 / 0.07, off, terms, gathered=False)   # noqa: E731
    rows = []
    for loss, part, fn in (("distill", "forward", df), ("infonce", "forward", cf), ("distill", "backward", db), ("infonce", "backward", cb),
                           ("distill", "backward, local side only", db_local), ("infonce", "backward, local side only", cb_local),
                           ("distill", "forward+backward", lambda: (df(), db())), ("infonce", "forward+backward", lambda: (cf(), cb()))):
        med, lo, hi = timed(fn, reps)
        rows.append(dict(loss=loss, part=part, b=b, N=N, E=E, Et=Et, reps=reps, ms_median=round(med, 3), ms_min=round(lo, 3),
                         ms_max=round(hi, 3)))
        print(f"b {b} N {N} E {E} Et {Et} {loss:8s} {part:28s}: median {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} repeats)", flush=True)
    by = {(r["loss"], r["part"]): r["ms_median"] for r in rows}
    for part in ("forward", "backward", "backward, local side only", "forward+backward"):
        ratio = by[("distill", part)] / by[("infonce", part)]
        rows.append(dict(part=part, ratio_distill_over_infonce=round(ratio, 3)))
        print(f"{part}: distill / infonce = {ratio:.3f}", flush=True)
    if len(sys.argv) > 1:                                   # optional: the rows as JSON
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
