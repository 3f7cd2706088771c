"""Timing of gradient accumulation for the InfoNCE (openvision_amd.accumulate): one device, one process, device events, the calls of
a comparison alternated in one session, median and range over the repeats.

  kernels  at (b, N, E) = (256, 16384, 768), C = 1 and 2, over the packed bank:
             window     ov_clip_loss_window_backward of one window
             local      ov_clip_loss_multi_backward of the same rows with the gathered side NULL: the same tiles, one exponential fewer
             spliced    ov_clip_loss_multi + ov_clip_loss_multi_backward (both sides) at b = N: what evaluating the whole N x N loss
                        once per micro-batch costs
  step     (``--step``) ViT-L/14: training.accumulated_step at A = 4 x b = 256 against four ordinary steps of 256 (forward, ClipLoss,
             backward; no optimiser in either)

usage: accum_probe.py [--step] [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd import _lib, preset, synth, training    # noqa: E402
from openvision_amd._lib import check, ptr, stream_ptr      # noqa: E402
from openvision_amd.loss import ClipLoss                    # noqa: E402
from openvision_amd.model import create_model               # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternated(fns, reps, warm=1):
    """name -> list of ms; one round runs every fn once, in order."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    return ms


def summary(ms):
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), reps=len(ms))


def kernel_rows(b=256, N=16384, E=768, s=1 / 0.07, w0=4096):
    lib = _lib.load()
    rows = []
    nrm = torch.nn.functional.normalize
    f32 = dict(dtype=torch.float32, device="cuda")
    for C in (1, 2):
        g = torch.Generator(device="cuda").manual_seed(C)
        ai = nrm(torch.randn(N, E, device="cuda", generator=g), dim=-1)
        sets = [nrm(ai * 0.5 + torch.randn(N, E, device="cuda", generator=g) * 0.05, dim=-1) for _ in range(C)]
        packed = torch.cat([ai] + sets, dim=1).contiguous()
        ld = (1 + C) * E
        all_img, all_txt = ai.contiguous(), torch.cat(sets).contiguous()                  # the bank as local rows: [N, E], [C N, E]
        loc_img, loc_txt = all_img[w0:w0 + b].contiguous(), torch.cat([t[w0:w0 + b] for t in sets]).contiguous()
        sc, loss, d_s = torch.full((1,), s, **f32), torch.empty(1, **f32), torch.empty(1, **f32)
        terms_n, terms_b = torch.empty(4 * C, N, **f32), torch.empty(4 * C, b, **f32)
        nf, nfb = lib.ov_clip_loss_multi_workspace_bytes(N, N, C), lib.ov_clip_loss_multi_workspace_bytes(b, N, C)
        nb, nbb = lib.ov_clip_loss_multi_backward_workspace_bytes(N, N, C), lib.ov_clip_loss_multi_backward_workspace_bytes(b, N, C)
        nw = lib.ov_clip_loss_window_backward_workspace_bytes(b, N, C)
        ws = torch.empty(max(nf, nfb, nb, nbb, nw) + 16, dtype=torch.uint8, device="cuda")
        d_img, d_txt = torch.empty(b, E, **f32), torch.empty(C * b, E, **f32)
        dn_img, dn_txt, dn_packed = torch.empty(N, E, **f32), torch.empty(C * N, E, **f32), torch.empty_like(packed)

        def forward_n():
            check(lib.ov_clip_loss_multi(ptr(all_img), ptr(all_txt), ptr(packed), ptr(packed[:, E:]), ld, E, N, N, E, C, ptr(sc), 0,
                                         ptr(loss), ptr(terms_n), ptr(ws), nf, stream_ptr()))

        def window():
            check(lib.ov_clip_loss_window_backward(ptr(packed), ptr(packed[:, E:]), ld, E, N, E, C, ptr(sc), ptr(terms_n), None, w0, b, N,
                                                   ptr(d_img), ptr(d_txt), ptr(d_s), ptr(ws), nw, stream_ptr()))

        def local():
            check(lib.ov_clip_loss_multi_backward(ptr(loc_img), ptr(loc_txt), ptr(packed), ptr(packed[:, E:]), ld, E, b, N, E, C, ptr(sc),
                                                  w0, ptr(terms_b), None, ptr(d_img), ptr(d_txt), None, None, 0, 0, ptr(d_s), ptr(ws),
                                                  nbb, stream_ptr()))

        def spliced():
            forward_n()
            check(lib.ov_clip_loss_multi_backward(ptr(all_img), ptr(all_txt), ptr(packed), ptr(packed[:, E:]), ld, E, N, N, E, C, ptr(sc),
                                                  0, ptr(terms_n), None, ptr(dn_img), ptr(dn_txt), ptr(dn_packed), ptr(dn_packed[:, E:]),
                                                  ld, E, ptr(d_s), ptr(ws), nb, stream_ptr()))

        check(lib.ov_clip_loss_multi(ptr(loc_img), ptr(loc_txt), ptr(packed), ptr(packed[:, E:]), ld, E, b, N, E, C, ptr(sc), w0, ptr(loss),
                                     ptr(terms_b), ptr(ws), nfb, stream_ptr()))            # the terms the local backward reads
        forward_n()
        pair = alternated(dict(window=window, local=local), reps=15, warm=2)
        whole = alternated(dict(forward_n=forward_n, spliced=spliced), reps=3)
        for name, ms in (*pair.items(), *whole.items()):
            rows.append(dict(part=name, b=b, N=N, E=E, C=C, **summary(ms)))
            print(rows[-1], flush=True)
        del packed, dn_packed, dn_img, dn_txt
    return rows


def step_rows(A=4, b=256, name="vit-large-patch14-224"):
    cfg = preset(name)
    size = cfg["vision_cfg"]["image_size"]
    m = create_model(cfg, device="cuda", state_dict=synth.make_state_dict(cfg))
    for p in m.parameters():
        p.requires_grad_(True)
    batches = [(synth.make_images(b, size, seed=10 + j).to("cuda"), synth.make_captions(b, seed=10 + j).to("cuda")) for j in range(A)]
    loss = ClipLoss()

    def accumulated():
        m.zero_grad(set_to_none=True)
        training.accumulated_step(m, batches, loss)

    def ordinary():
        m.zero_grad(set_to_none=True)
        for img, tok in batches:
            loss(*training.clip_forward(m, img, tok)).backward()

    def pass_one():
        with torch.no_grad():
            for img, tok in batches:
                training.clip_forward(m, img, tok)

    ms = alternated(dict(accumulated=accumulated, ordinary=ordinary, pass_one=pass_one), reps=5)
    rows = []
    for k, v in ms.items():
        rows.append(dict(part=f"step {k}", model=name, A=A, b=b, **summary(v)))
        print(rows[-1], flush=True)
    return rows


def main():
    args = [a for a in sys.argv[1:] if a != "--step"]
    rows = kernel_rows()
    if "--step" in sys.argv:
        rows += step_rows()
    if args:
        with open(args[0], "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
