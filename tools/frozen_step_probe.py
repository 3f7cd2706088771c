"""Time per step and peak device memory of training with frozen parameters, one configuration per process:

    image_all    L/14@224, B = 256: every parameter trainable      (clip_forward + ClipLoss + backward + FusedAdamW step)
    image_lit    the same after model.lock_image_tower()           (LiT: the image tower frozen, text tower trained)
    image_lit2   the same after model.lock_image_tower(2)          (resblocks[-1], ln_post and proj unlocked)
    text_train   text-side gradient-ascent step (ov-gradient-ascent.py) at B = 13, L/14's text tower, parameters trainable
    text_frozen  the same step with model.requires_grad_(False)     (input-only text backward)

--patch-dropout P (image configurations): the vision tower's patch_dropout = P, model in training mode, so that every step keeps
K = max(1, int(G (1 - P))) patches per image, drawn as the reference draws them (FLIP; FLIP + LiT with image_lit).

Run each configuration as its own step, each under its own time limit, and stop at the first failure:

    timeout -k 10 600 python tools/frozen_step_probe.py image_all && timeout -k 10 600 python tools/frozen_step_probe.py image_lit && ...
    timeout -k 10 600 python tools/frozen_step_probe.py image_all --patch-dropout 0.5 && ...

Prints one JSON line per configuration: ms per step (mean of STEPS timed steps after one warm-up step) and
torch.cuda.max_memory_allocated over the timed steps (model, optimiser state and the training path's buffer pool included)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd import preset, synth, training  # noqa: E402
from openvision_amd.loss import ClipLoss  # noqa: E402
from openvision_amd.model import create_model  # noqa: E402

CONFIGS = ("image_all", "image_lit", "image_lit2", "text_train", "text_frozen")


def main():
    args = sys.argv[1:]
    which = args[0] if args else ""
    pdrop = 0.0
    if len(args) == 3 and args[1] == "--patch-dropout" and which.startswith("image"):
        pdrop = float(args[2])
    elif len(args) != 1:
        which = ""
    if which not in CONFIGS:
        sys.exit(f"usage: frozen_step_probe.py {{{'|'.join(CONFIGS)}}} [--patch-dropout P]")
    name = os.environ.get("MODEL", "vit-large-patch14-224")
    steps = int(os.environ.get("STEPS", "3"))
    cfg = preset(name)
    sd = synth.make_state_dict(cfg)
    if pdrop > 0:
        cfg = dict(cfg, vision_cfg=dict(cfg["vision_cfg"], patch_dropout=pdrop))
    m = create_model(cfg, device="cuda", state_dict=sd)
    if pdrop > 0:
        m.train()                                   # patch dropout acts in training mode only
        torch.manual_seed(0)
    if which.startswith("image"):
        B = int(os.environ.get("BATCH", "256"))
        if which == "image_lit":
            m.lock_image_tower()
        elif which == "image_lit2":
            m.lock_image_tower(2)
        opt = training.FusedAdamW(m, lr=1e-6, clip_norm=1.0)             # after locking: it collects what requires grad
        img = synth.make_images(B, cfg["vision_cfg"]["image_size"], seed=1).to("cuda")
        tok = synth.make_captions(B, seed=1).to("cuda")
        loss_fn = ClipLoss()

        def step():
            opt.zero_grad()
            loss = loss_fn(*training.clip_forward(m, img, tok))
            loss.backward()
            opt.step()
            return loss
    else:
        B = int(os.environ.get("BATCH", "13"))
        m.requires_grad_(which == "text_train")
        V, T = cfg["text_cfg"]["vocab_size"], cfg["text_cfg"]["context_length"]
        g = torch.Generator().manual_seed(1)
        ids = synth.make_captions(B, seed=1)
        soft = (torch.nn.functional.one_hot(ids, V).float() * 0.9 + torch.rand(B, T, V, generator=g) * (0.1 / V)).to("cuda")
        soft.requires_grad_(True)
        target = torch.nn.functional.normalize(torch.randn(B, cfg["embed_dim"], generator=g), dim=-1).to("cuda")

        def step():
            m.zero_grad(set_to_none=True)
            soft.grad = None
            loss = -(training.encode_text(m, soft, normalize=True) * target).sum(-1).mean()
            loss.backward()
            return loss

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    trainable = sum(p.numel() for p in m.parameters() if p.requires_grad)
    print(json.dumps(dict(config=which, model=name, batch=B, patch_dropout=pdrop, steps=steps, ms_per_step=round(ms, 2),
                          max_memory_allocated_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                          trainable_params=trainable, loss=float(loss.detach()))), flush=True)


if __name__ == "__main__":
    main()
