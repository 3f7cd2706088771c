"""Time per step and peak device memory of training with and without activation recomputation (model.set_grad_checkpointing),
one configuration per process:

    l14_save    L/14@224, B = 256, every intermediate kept (the default)     (clip_forward + ClipLoss + backward + FusedAdamW step)
    l14_remat   the same with model.set_grad_checkpointing()                 (block inputs kept, intermediates recomputed)
    h14_remat   H/14@224 at B = 768 with recomputation: a batch whose saving path does not fit in HBM (never run without it;
                the line also prints what the saving path would keep, from ov_tower_saved_bytes -- CPU arithmetic, no launch)

BATCH overrides the batch, STEPS the number of timed steps (default 3).  Run each configuration as its own step, each under its
own time limit, and stop at the first failure:

    timeout -k 10 600 python tools/remat_step_probe.py l14_save && timeout -k 10 600 python tools/remat_step_probe.py l14_remat && \\
    timeout -k 10 900 python tools/remat_step_probe.py h14_remat

Prints one JSON line per configuration: ms per step (mean of STEPS timed steps after one warm-up step) and
torch.cuda.max_memory_allocated over the timed steps (model, optimiser state and the training path's buffer pools included)."""
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd import _lib, preset, synth, training  # noqa: E402
from openvision_amd.loss import ClipLoss  # noqa: E402
from openvision_amd.model import create_model  # noqa: E402

CONFIGS = {"l14_save": ("vit-large-patch14-224", 256, False), "l14_remat": ("vit-large-patch14-224", 256, True),
           "h14_remat": ("vit-huge-patch14-224", 768, True)}


def tower_bytes(transformer, B, L):
    """(ov_tower_saved_bytes, ov_tower_checkpoint_bytes + ov_tower_slot_bytes) of one tower: host arithmetic only."""
    lib = _lib.load()
    b0 = transformer.resblocks[0]
    cfg = _lib.TowerCfg(b0.attn.embed_dim, len(transformer.resblocks), b0.attn.num_heads, b0.mlp_dim, b0.mlp_pad, int(b0.gelu_tanh),
                        float(b0.ln_1.eps))
    t = lib.ov_tower_create(C.byref(cfg))
    try:
        return lib.ov_tower_saved_bytes(t, B, L), lib.ov_tower_checkpoint_bytes(t, 0, B, L) + lib.ov_tower_slot_bytes(t, B, L)
    finally:
        lib.ov_tower_destroy(t)


def main():
    args = sys.argv[1:]
    if len(args) != 1 or args[0] not in CONFIGS:
        sys.exit(f"usage: remat_step_probe.py {{{'|'.join(CONFIGS)}}}")
    which = args[0]
    name, B, remat = CONFIGS[which]
    B = int(os.environ.get("BATCH", B))
    steps = int(os.environ.get("STEPS", "3"))
    cfg = preset(name)
    m = create_model(cfg, device="cuda", state_dict=synth.make_state_dict(cfg))
    m.set_grad_checkpointing(remat)
    grid = cfg["vision_cfg"]["image_size"] // cfg["vision_cfg"]["patch_size"]
    Li, Lt = grid * grid + 1, cfg["text_cfg"]["context_length"]
    img_saved, img_remat = tower_bytes(m.visual.transformer, B, Li)
    txt_saved, txt_remat = tower_bytes(m.transformer, B, Lt)
    opt = training.FusedAdamW(m, lr=1e-6, clip_norm=1.0)
    img = synth.make_images(B, cfg["vision_cfg"]["image_size"], seed=1).to("cuda")
    tok = synth.make_captions(B, seed=1).to("cuda")
    loss_fn = ClipLoss()

    def step():
        opt.zero_grad()
        loss = loss_fn(*training.clip_forward(m, img, tok))
        loss.backward()
        opt.step()
        return loss

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    gib = 2 ** 30
    print(json.dumps(dict(config=which, model=name, batch=B, grad_checkpointing=remat, steps=steps, ms_per_step=round(ms, 2),
                          img_per_s=round(B / ms * 1e3, 1), max_memory_allocated_gib=round(torch.cuda.max_memory_allocated() / gib, 2),
                          saving_path_saved_gib=dict(image=round(img_saved / gib, 2), text=round(txt_saved / gib, 2)),
                          remat_kept_gib=dict(image=round(img_remat / gib, 2), text=round(txt_remat / gib, 2)),
                          hbm_gib=round(torch.cuda.get_device_properties(0).total_memory / gib, 1), loss=float(loss.detach()))),
          flush=True)


if __name__ == "__main__":
    main()
