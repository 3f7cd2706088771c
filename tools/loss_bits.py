"""SHA-256 of every output of the four fused contrastive losses (InfoNCE, multi-caption, distillation, SigLIP) and of ov_logits,
forward and backward through the C ABI, on seeded inputs.  Their summation orders are fixed, so two builds of the library that
compute the same thing print the same digests; a tolerance would hide a reordered sum in the outputs that cancel to ~1e-7.

    python tools/loss_bits.py [out.json]                    # the in-tree library
    OVHIP_LIB=/path/libovhip_other.so python tools/loss_bits.py [other.json]

Shapes (b of N rows at label offset off, width E; distillation adds the teacher's width Et): a ragged row tile where two waves own
no e-tile, an e-tile count that is no multiple of 4, the width limit, several column splits; SigLIP adds a ragged e-tile (E = 40).
Both output sides, upstream gradient 0.5, logit multiplier 1 / 0.07 (teacher 20, SigLIP 10 with bias -10)."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd import _lib                             # noqa: E402
from openvision_amd._lib import check, ptr, stream_ptr      # noqa: E402

SHAPES = [(13, 39, 13, 64, 48), (45, 135, 45, 96, 72), (32, 96, 32, 1152, 8), (100, 700, 300, 384, 512)]     # b, N, off, E, Et
SIGLIP_EXTRA = (13, 39, 13, 40)
C = 2
DEV = "cuda"


def features(n, width, seed):
    """Two correlated sets of unit rows [n, width], drawn on the host so that the values do not depend on the device."""
    g = torch.Generator().manual_seed(seed)
    nrm = torch.nn.functional.normalize
    a = nrm(torch.randn(n, width, generator=g), dim=-1)
    return a.to(DEV), nrm(a * 0.5 + torch.randn(n, width, generator=g) * 0.05, dim=-1).to(DEV)


def zeros(*shape):
    return torch.zeros(*shape, dtype=torch.float32, device=DEV)


def scalar(v):
    return torch.full((1,), v, dtype=torch.float32, device=DEV)


def workspace(nbytes):
    return torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV)


def infonce(lib, b, N, off, E):
    ai, at = features(N, E, 1)
    img, txt = ai[off:off + b].contiguous(), at[off:off + b].contiguous()
    s, g = scalar(1 / 0.07), scalar(0.5)
    loss, terms = zeros(1), zeros(4, b)
    nf, nb = lib.ov_clip_loss_workspace_bytes(b, N), lib.ov_clip_loss_backward_workspace_bytes(b, N)
    wf, wb = workspace(nf), workspace(nb)
    check(lib.ov_clip_loss(ptr(img), ptr(txt), ptr(ai), ptr(at), b, N, E, ptr(s), off, ptr(loss), ptr(terms), ptr(wf), nf, stream_ptr()))
    d_img, d_txt, d_ai, d_at, d_s = zeros(b, E), zeros(b, E), zeros(N, E), zeros(N, E), zeros(1)
    check(lib.ov_clip_loss_backward(ptr(img), ptr(txt), ptr(ai), ptr(at), b, N, E, ptr(s), off, ptr(terms), ptr(g), ptr(d_img), ptr(d_txt),
                                    ptr(d_ai), ptr(d_at), ptr(d_s), ptr(wb), nb, stream_ptr()))
    return dict(loss=loss, terms=terms, d_img=d_img, d_txt=d_txt, d_all_img=d_ai, d_all_txt=d_at, d_scale=d_s)


def multicap(lib, b, N, off, E):
    """C caption sets in the all-gather's packed [N, (1 + C) E] layout, the gathered-side gradient written packed."""
    ld = (1 + C) * E
    packed, gpacked = zeros(N, ld), zeros(N, ld)
    packed[:, :E], packed[:, E:2 * E] = features(N, E, 2)
    for c in range(1, C):
        packed[:, (1 + c) * E:(2 + c) * E] = features(N, E, 2 + c)[1]
    img = packed[off:off + b, :E].contiguous()
    txt = torch.cat([packed[off:off + b, (1 + c) * E:(2 + c) * E] for c in range(C)]).contiguous()
    s, g = scalar(1 / 0.07), scalar(0.5)
    loss, terms = zeros(1), zeros(4 * C, b)
    nf, nb = lib.ov_clip_loss_multi_workspace_bytes(b, N, C), lib.ov_clip_loss_multi_backward_workspace_bytes(b, N, C)
    wf, wb = workspace(nf), workspace(nb)
    all_img, all_txt = packed, packed[:, E:]
    check(lib.ov_clip_loss_multi(ptr(img), ptr(txt), ptr(all_img), ptr(all_txt), ld, E, b, N, E, C, ptr(s), off, ptr(loss), ptr(terms),
                                 ptr(wf), nf, stream_ptr()))
    d_img, d_txt, d_s = zeros(b, E), zeros(C * b, E), zeros(1)
    check(lib.ov_clip_loss_multi_backward(ptr(img), ptr(txt), ptr(all_img), ptr(all_txt), ld, E, b, N, E, C, ptr(s), off, ptr(terms), ptr(g),
                                          ptr(d_img), ptr(d_txt), ptr(gpacked), ptr(gpacked[:, E:]), ld, E, ptr(d_s), ptr(wb), nb,
                                          stream_ptr()))
    return dict(loss=loss, terms=terms, d_img=d_img, d_txt=d_txt, d_all_packed=gpacked, d_scale=d_s)


def distill(lib, b, N, off, E, Et):
    y, v = features(N, E, 5), features(N, Et, 6)
    x = [t[off:off + b].contiguous() for t in y]
    u = [t[off:off + b].contiguous() for t in v]
    s, st, gc, gd = scalar(1 / 0.07), scalar(20.0), scalar(0.5), scalar(0.5)
    out, terms = zeros(2), zeros(12, b)
    nf, nb = lib.ov_distill_loss_workspace_bytes(b, N), lib.ov_distill_loss_backward_workspace_bytes(b, N)
    wf, wb = workspace(nf), workspace(nb)
    check(lib.ov_distill_loss(ptr(x[0]), ptr(x[1]), ptr(y[0]), ptr(y[1]), E, ptr(u[0]), ptr(u[1]), ptr(v[0]), ptr(v[1]), Et, b, N, E, Et,
                              ptr(s), ptr(st), off, ptr(out[0:]), ptr(out[1:]), ptr(terms), ptr(wf), nf, stream_ptr()))
    d_img, d_txt, d_ai, d_at, d_s = zeros(b, E), zeros(b, E), zeros(N, E), zeros(N, E), zeros(1)
    check(lib.ov_distill_loss_backward(ptr(x[0]), ptr(x[1]), ptr(y[0]), ptr(y[1]), E, ptr(u[0]), ptr(u[1]), ptr(v[0]), ptr(v[1]), Et, b, N,
                                       E, Et, ptr(s), ptr(st), off, ptr(terms), ptr(gc), ptr(gd), ptr(d_img), ptr(d_txt), ptr(d_ai),
                                       ptr(d_at), E, ptr(d_s), ptr(wb), nb, stream_ptr()))
    return dict(losses=out, terms=terms, d_img=d_img, d_txt=d_txt, d_all_img=d_ai, d_all_txt=d_at, d_scale=d_s)


def siglip(lib, b, N, off, E):
    ai, at = features(N, E, 7)
    img = ai[off:off + b].contiguous()
    s, beta, g = scalar(10.0), scalar(-10.0), scalar(0.5)
    loss = zeros(1)
    nf, nb = lib.ov_siglip_loss_workspace_bytes(b, N), lib.ov_siglip_loss_backward_workspace_bytes(b, N)
    wf, wb = workspace(nf), workspace(nb)
    check(lib.ov_siglip_loss(ptr(img), ptr(at), b, N, E, ptr(s), ptr(beta), off, ptr(loss), ptr(wf), nf, stream_ptr()))
    dx, dy, dsb = zeros(b, E), zeros(N, E), zeros(2)
    check(lib.ov_siglip_loss_backward(ptr(img), ptr(at), b, N, E, ptr(s), ptr(beta), off, ptr(g), ptr(dx), ptr(dy), ptr(dsb[0:]),
                                      ptr(dsb[1:]), ptr(wb), nb, stream_ptr()))
    return dict(loss=loss, d_img=dx, d_all_txt=dy, d_scale_bias=dsb)


def logits(lib, b, N, off, E):
    ai, at = features(N, E, 8)
    out = zeros(b, N)
    check(lib.ov_logits(ptr(ai[off:off + b].contiguous()), ptr(at), ptr(out), N, b, N, E, 1.0, ptr(scalar(1 / 0.07)), stream_ptr()))
    return dict(logits=out)


def main():
    lib = _lib.load()
    digests = {}

    def record(name, shape, outs):
        torch.cuda.synchronize()
        for key, t in outs.items():
            h = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
            digests[f"{name} {shape} {key}"] = h
            print(f"{h}  {name} {shape} {key}", flush=True)

    for b, N, off, E, Et in SHAPES:
        shape = f"b{b} N{N} off{off} E{E}"
        record("infonce", shape, infonce(lib, b, N, off, E))
        record(f"multicap C{C}", shape, multicap(lib, b, N, off, E))
        record("distill", f"{shape} Et{Et}", distill(lib, b, N, off, E, Et))
        record("siglip", shape, siglip(lib, b, N, off, E))
        record("logits", shape, logits(lib, b, N, off, E))
    b, N, off, E = SIGLIP_EXTRA
    record("siglip", f"b{b} N{N} off{off} E{E}", siglip(lib, b, N, off, E))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(dict(library=os.path.basename(_lib.LIB_PATH), digests=digests), f, indent=1)


if __name__ == "__main__":
    main()
