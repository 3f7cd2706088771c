"""Timing of the SigLIP loss kernels (ov_siglip_loss / ov_siglip_loss_backward) against InfoNCE's (ov_clip_loss /
ov_clip_loss_backward) in the same process, at the bench shape (b = N = 256) and at config #5's per-GPU shape (b = 4096 of
N = 32768), E = 768.  Device events around `reps` calls after a warm-up.
FLOP model: SigLIP forward 2 b N E (one logit strip), backward 8 b N E with both sides (the strip recomputed once per side, plus
one g.X product per side); InfoNCE forward 4 b N E, backward 16 b N E.  fp32 matrix peak: 157.3 TFLOP/s."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hipops as H                                          # noqa: E402
from openvision_amd import _lib                             # noqa: E402
from openvision_amd._lib import check, ptr, stream_ptr      # noqa: E402

PEAK = 157.3


def siglip_fns(img, all_txt, scale, bias, off):
    lib = _lib.load()
    b, e = img.shape
    n = all_txt.shape[0]
    nf, nb = lib.ov_siglip_loss_workspace_bytes(b, n), lib.ov_siglip_loss_backward_workspace_bytes(b, n)
    wf = torch.empty(nf + 16, dtype=torch.uint8, device="cuda")
    wb = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    out = torch.empty(1, dtype=torch.float32, device="cuda")
    dx, dy = torch.empty_like(img), torch.empty_like(all_txt)
    dsb = torch.empty(2, dtype=torch.float32, device="cuda")
    grad = torch.ones(1, dtype=torch.float32, device="cuda")

    def fwd():
        check(lib.ov_siglip_loss(ptr(img), ptr(all_txt), b, n, e, ptr(scale), ptr(bias), off, ptr(out), ptr(wf), nf, stream_ptr()))

    def bwd():
        check(lib.ov_siglip_loss_backward(ptr(img), ptr(all_txt), b, n, e, ptr(scale), ptr(bias), off, ptr(grad), ptr(dx), ptr(dy),
                                          ptr(dsb[0:]), ptr(dsb[1:]), ptr(wb), nb, stream_ptr()))
    return fwd, bwd


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    rows = []
    for b, N in [(256, 256), (4096, 32768)]:
        E = 768
        g = torch.Generator(device="cuda").manual_seed(0)
        ai = torch.nn.functional.normalize(torch.randn(N, E, device="cuda", generator=g), dim=-1)
        at = torch.nn.functional.normalize(ai * 0.5 + torch.randn(N, E, device="cuda", generator=g) * 0.05, dim=-1)
        img, txt = ai[:b].contiguous(), at[:b].contiguous()
        reps = 50 if N <= 256 else 5
        scale = torch.full((1,), 10.0, device="cuda")
        bias = torch.full((1,), -10.0, device="cuda")
        sf, sb = siglip_fns(img, at, scale, bias, 0)
        _, terms = H.clip_loss(img, txt, ai, at, 1 / 0.07, 0)
        cf = lambda: H.clip_loss(img, txt, ai, at, 1 / 0.07, 0)                          # noqa: E731
        cb = lambda: H.clip_loss_backward(img, txt, ai, at, 1 / 0.07, 0, terms)          # noqa: E731
        bne = float(b) * N * E
        for loss, name, fn, flops in (("siglip", "forward", sf, 2 * bne), ("siglip", "backward", sb, 8 * bne),
                                      ("siglip", "forward+backward", lambda: (sf(), sb()), 10 * bne),
                                      ("infonce", "forward", cf, 4 * bne), ("infonce", "backward", cb, 16 * bne),
                                      ("infonce", "forward+backward", lambda: (cf(), cb()), 20 * bne)):
            ms = timed(fn, reps)
            tf = flops / ms / 1e9
            rows.append(dict(loss=loss, part=name, b=b, N=N, E=E, ms=round(ms, 4), tflops=round(tf, 1),
                             peak_share=round(tf / PEAK, 3)))
            print(f"b {b} N {N} E {E} {loss:8s} {name:17s}: {ms:8.3f} ms = {tf:6.1f} TFLOP/s fp32 ({tf / PEAK:.1%} of {PEAK})",
                  flush=True)
    if len(sys.argv) > 1:                                   # optional: the rows as JSON
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
