"""Timing of the InfoNCE forward and backward (ov_clip_loss / ov_clip_loss_backward) at the bench shape (b = N = 256) and at
config #5's per-GPU shape (b = 4096 of N = 32768), E = 768, and of the two-caption loss (ov_clip_loss_multi*, C = 2, the packed
[N, 3 E] gathered layout) at the second shape.  Each call is bracketed by its own pair of device events after a warm-up; the
figure is the median over the repeats.  FLOP model: forward 4 C b N E (two logit strips per caption set), backward 16 C b N E
(each strip recomputed twice, once per output side, plus the two P.X products per strip)."""
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


def multi_fns(packed, b, E, C, s, off):
    """packed: the all-gather's [N, (1 + C) E] rows (image, then the C caption sets); the local rows are rows off ... off + b."""
    lib = _lib.load()
    N, ld = packed.shape
    img = packed[off:off + b, :E].contiguous()
    txt = torch.cat([packed[off:off + b, (1 + c) * E:(2 + c) * E] for c in range(C)]).contiguous()
    nf, nb = lib.ov_clip_loss_multi_workspace_bytes(b, N, C), lib.ov_clip_loss_multi_backward_workspace_bytes(b, N, C)
    wf = torch.empty(nf + 16, dtype=torch.uint8, device="cuda")
    wb = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    terms = torch.empty(4 * C, b, dtype=torch.float32, device="cuda")
    d_img, d_txt, d_packed = torch.empty_like(img), torch.empty_like(txt), torch.empty_like(packed)
    d_s = torch.empty(1, dtype=torch.float32, device="cuda")
    sc = torch.full((1,), s, dtype=torch.float32, device="cuda")

    def fwd():
        check(lib.ov_clip_loss_multi(ptr(img), ptr(txt), ptr(packed), ptr(packed[:, E:]), ld, E, b, N, E, C, ptr(sc), off, ptr(loss),
                                     ptr(terms), ptr(wf), nf, stream_ptr()))

    def bwd(gathered=True):
        check(lib.ov_clip_loss_multi_backward(ptr(img), ptr(txt), ptr(packed), ptr(packed[:, E:]), ld, E, b, N, E, C, ptr(sc), off, ptr(terms),
                                              None, ptr(d_img), ptr(d_txt), ptr(d_packed) if gathered else None,
                                              ptr(d_packed[:, E:]) if gathered else None, ld, E, ptr(d_s), ptr(wb), nb, stream_ptr()))
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
    return statistics.median(ms)


def main():
    rows = []
    E, s = 768, 1 / 0.07
    nrm = torch.nn.functional.normalize
    for b, N in [(256, 256), (4096, 32768)]:
        g = torch.Generator(device="cuda").manual_seed(0)
        ai = nrm(torch.randn(N, E, device="cuda", generator=g), dim=-1)
        at = nrm(ai * 0.5 + torch.randn(N, E, device="cuda", generator=g) * 0.05, dim=-1)
        img, txt = ai[:b].contiguous(), at[:b].contiguous()
        _, terms = H.clip_loss(img, txt, ai, at, s, 0)
        jobs = [("infonce", 1, "forward", lambda: H.clip_loss(img, txt, ai, at, s, 0), 4.0),
                ("infonce", 1, "backward local side only", lambda: H.clip_loss_backward(img, txt, ai, at, s, 0, terms, gathered=False), 8.0),
                ("infonce", 1, "backward both sides", lambda: H.clip_loss_backward(img, txt, ai, at, s, 0, terms), 16.0)]
        if N > 256:
            C = 2
            at2 = nrm(ai * 0.5 + torch.randn(N, E, device="cuda", generator=g) * 0.05, dim=-1)
            packed = torch.cat([ai, at, at2], dim=1).contiguous()
            mf, mb = multi_fns(packed, b, E, C, s, 0)
            mf()                                            # the terms the backward reads
            jobs += [("multicap", C, "forward", mf, 4.0 * C), ("multicap", C, "backward local side only", lambda: mb(False), 8.0 * C),
                     ("multicap", C, "backward both sides", mb, 16.0 * C)]
        reps = 21 if N <= 256 else 7
        for loss, C, name, fn, mult in jobs:
            ms = timed(fn, reps)
            flops = mult * b * N * E
            rows.append(dict(loss=loss, C=C, part=name, b=b, N=N, E=E, reps=reps, ms_median=round(ms, 4)))
            print(f"b {b} N {N} E {E} {loss} C {C} {name}: {ms:.3f} ms = {flops / ms / 1e9:.1f} TFLOP/s fp32 (peak 157.3)", flush=True)
    if len(sys.argv) > 1:                                   # optional: the rows as JSON
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
