"""Time of one gradient-ascent step (ov-gradient-ascent.py) at L/14@224, B = 13, K = 4, one configuration per process:

    hip         GradientAscent.step: ov_ga_affine, encode_image, ov_ga_sample, the row gather, the input-only text tower forward and
                backward, ov_ga_cosine_loss, ov_ga_token_grad, ov_ga_adam
    eager       the composition the loop replaces, on the same towers: F.affine_grid + F.grid_sample + normalisation, encode_image,
                F.gumbel_softmax(hard=True), torch.cat with the pad one-hots, training.encode_text(soft) (the [B 80, V] x [V, D] fp32
                product), torch.cosine_similarity, autograd, torch.optim.Adam, loss.item()
    token_grad  ov_ga_token_grad alone at R = 52, V = 32000, D = the text width: W is rotated through COPIES separate tables (8 x 49 MB,
                more than the 256 MB Infinity Cache), so that every launch reads its table from HBM as a step of the loop does

Run each configuration as its own step, each under its own time limit, and stop at the first failure:

    timeout -k 10 300 python tools/ascent_step_probe.py hip && timeout -k 10 300 python tools/ascent_step_probe.py eager && \
    timeout -k 10 300 python tools/ascent_step_probe.py token_grad

Protocol: one warm-up window, then ROUNDS windows of ITERS steps (launches for token_grad), device events around each window; prints
one JSON line with the windows' ms per step, their median and, for token_grad, the bytes of W over the median as a fraction of
HBM_TBS (8 TB/s, MI355X_MICROARCH.md)."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd import _lib, preset, synth, training  # noqa: E402
from openvision_amd.gradient_ascent import GradientAscent, affine_theta  # noqa: E402
from openvision_amd.model import create_model  # noqa: E402

CONFIGS = ("hip", "eager", "token_grad")
HBM_TBS = 8.0


def windows(fn, iters, rounds):
    """ms per call of fn over `rounds` windows of `iters` calls, after one warm-up window."""
    out = []
    for w in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(w * iters + i)
        b.record()
        torch.cuda.synchronize()
        if w:
            out.append(a.elapsed_time(b) / iters)
    return out


def main():
    which = sys.argv[1] if len(sys.argv) == 2 else ""
    if which not in CONFIGS:
        sys.exit(f"usage: ascent_step_probe.py {{{'|'.join(CONFIGS)}}}")
    name = os.environ.get("MODEL", "vit-large-patch14-224")
    batch, k = int(os.environ.get("BATCH", "13")), int(os.environ.get("TOKENS", "4"))
    iters, rounds = int(os.environ.get("ITERS", "20")), int(os.environ.get("ROUNDS", "5"))
    cfg = preset(name)
    model = create_model(cfg, device="cuda", state_dict=synth.make_state_dict(cfg))
    size = cfg["vision_cfg"]["image_size"]
    vocab, d = model.token_embedding.weight.shape
    t = model.context_length
    torch.manual_seed(0)
    image = torch.rand(3, size, size).cuda()
    steps = iters * (rounds + 1)
    extra = {}
    if which == "hip":
        loop = GradientAscent(model, batch_size=batch, tokens=k, steps=steps)
        loop.begin(image)
        ms = windows(loop.step, iters, rounds)
        loop.end()
        extra["best_loss"] = loop.best_loss
    elif which == "eager":
        loop = GradientAscent(model, batch_size=batch, tokens=k, steps=steps)       # for its draws and its frozen parameters only
        loop.begin(image)
        theta = affine_theta(loop._s.mats.double(), size, size).float()
        mean, std = loop._s.mean.view(1, 3, 1, 1), loop._s.std.view(1, 3, 1, 1)
        normu = loop.normu.clone().requires_grad_(True)
        opt = torch.optim.Adam([normu], lr=5.0)
        pad = torch.zeros(batch, t - k, vocab, device="cuda")
        pad[:, :, 0] = 1
        src = image.unsqueeze(0).expand(batch, -1, -1, -1)
        best = [float("inf")]

        def step(i):
            with torch.no_grad():
                grid = F.affine_grid(theta[i], (batch, 3, size, size), align_corners=False)
                aug = (F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False) - mean) / std
                feats = model.encode_image(aug, normalize=False)
            soft = F.gumbel_softmax(normu, tau=1000.0, dim=-1, hard=True)
            tx = training.encode_text(model, torch.cat([pad, soft], dim=1), normalize=False)
            loss1 = -100 * torch.cosine_similarity(tx.unsqueeze(0), feats.unsqueeze(1), -1).view(-1, batch).T.mean(1)
            loss = loss1.mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            best[0] = min(best[0], loss.item())                  # the script's per-step read of the loss

        ms = windows(step, iters, rounds)
        loop.end()
        extra["best_loss"] = best[0]
    else:
        lib, copies, r = _lib.load(), int(os.environ.get("COPIES", "8")), batch * k
        iters = int(os.environ.get("ITERS", "5000"))
        g = torch.Generator().manual_seed(1)
        tables = [(torch.randn(vocab, d, generator=g) * 0.5).to(torch.bfloat16).cuda() for _ in range(copies)]
        dx = (torch.randn(r, d, generator=g) * 1e-3).to(torch.bfloat16).cuda()
        normu, e = torch.randn(r, vocab, generator=g).cuda(), torch.empty(r, vocab).exponential_(generator=g).cuda()
        idx, zmax, zsum = torch.zeros(r, dtype=torch.int32, device="cuda"), torch.zeros(r, device="cuda"), torch.zeros(r, device="cuda")
        gy, parts, z = torch.zeros(r, vocab, device="cuda"), torch.zeros(r, lib.ov_ga_parts_blocks(vocab), device="cuda"), torch.zeros(r, vocab, device="cuda")
        st = _lib.stream_ptr()
        _lib.check(lib.ov_ga_sample(_lib.ptr(normu), _lib.ptr(e), 1000.0, r, vocab, 0, 0, _lib.ptr(z), _lib.ptr(idx), _lib.ptr(zmax), _lib.ptr(zsum),
                                    None, None, st), "ov_ga_sample")

        def launch(i):
            _lib.check(lib.ov_ga_token_grad(_lib.ptr(dx), _lib.ptr(tables[i % copies]), _lib.ptr(z), _lib.ptr(zmax), _lib.ptr(zsum), r, vocab, d,
                                            _lib.ptr(gy), _lib.ptr(parts), st), "ov_ga_token_grad")

        ms = windows(launch, iters, rounds)
        w_bytes = vocab * d * 2
        extra.update(rows=r, w_bytes=w_bytes, copies=copies,
                     w_read_fraction_of_hbm=round(w_bytes / (statistics.median(ms) * 1e-3) / (HBM_TBS * 1e12), 3))
    print(json.dumps(dict(config=which, model=name, batch=batch, tokens=k, vocab=vocab, width=d, iters=iters, rounds=rounds,
                          ms=[round(x, 4) for x in ms], median_ms=round(statistics.median(ms), 4), **extra)), flush=True)


if __name__ == "__main__":
    main()
