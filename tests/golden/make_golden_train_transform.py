"""Generate tests/golden/train_transform.npz: outputs of Pillow itself for the training image transform's pinned half.

    python tests/golden/make_golden_train_transform.py

Per case: ``Image.fromarray(x).crop(box).resize((32, 32), filter)``, then the colour operations the way torchvision applies them to a
PIL image (``ImageEnhance.Brightness / Contrast / Color(img).enhance(factor)``; ``Grayscale(3)`` = ``convert("L")`` stacked three
times), then ToTensor (x / 255) and Normalize ((x - mean) / std) in numpy float32.  Inputs are seeded; Pillow 12.2.0 wrote the
committed file.  Keys per case name: ``<name>_in`` uint8 [H, W, 3], ``<name>_box`` (top, left, h, w), ``<name>_ops`` /
``<name>_factors`` (operation codes 1 brightness, 2 contrast, 3 saturation, 4 grayscale, in application order, and float32 factors),
``<name>_u8`` Pillow's uint8 image, ``<name>_out`` float32 [3, 32, 32]; ``names`` / ``interps`` list the cases.
"""
import os

import numpy as np
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
SIZE = 32
MEAN = np.asarray([0.48145466, 0.4578275, 0.40821073], np.float32)
STD = np.asarray([0.26862954, 0.26130258, 0.27577711], np.float32)
ENHANCE = {1: ImageEnhance.Brightness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Color}

# name, (H, W), box (top, left, h, w), filter, [(op, factor), ...]
CASES = [
    ("crop_bicubic", (48, 40), (10, 7, 31, 29), "bicubic", []),
    ("strip_bilinear_bright", (20, 30), (3, 4, 9, 17), "bilinear", [(1, 1.32)]),
    ("full_saturation", (40, 40), (0, 0, 40, 40), "bicubic", [(3, 1.32)]),
    ("contrast_last", (72, 56), (8, 5, 60, 49), "bicubic", [(1, 0.68), (3, 1.32), (2, 1.32)]),
    ("jitter_then_gray", (33, 47), (1, 2, 32, 45), "bilinear", [(2, 0.7), (1, 1.2), (3, 0.5), (4, 0.0)]),
]


def make_input(rng, h, w):
    """smooth ramps plus noise: resampling and every colour operation have something to act on"""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * xx / max(w - 1, 1), 255.0 * yy / max(h - 1, 1), 255.0 * (xx + yy) / max(h + w - 2, 1)], axis=-1)
    return np.clip(0.6 * base + 0.4 * rng.integers(0, 256, (h, w, 3)), 0, 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(20)
    d = {}
    for name, (h, w), box, interp, chain in CASES:
        x = make_input(rng, h, w)
        top, left, bh, bw = box
        im = Image.fromarray(x).crop((left, top, left + bw, top + bh))
        im = im.resize((SIZE, SIZE), Image.BICUBIC if interp == "bicubic" else Image.BILINEAR).convert("RGB")
        factors = np.asarray([f for _, f in chain], np.float32)
        for (op, _), f in zip(chain, factors):
            if op == 4:
                l = np.array(im.convert("L"))
                im = Image.fromarray(np.dstack([l, l, l]), "RGB")
            else:
                im = ENHANCE[op](im).enhance(float(f))
        u8 = np.asarray(im)
        out = ((u8.astype(np.float32) / np.float32(255.0) - MEAN) / STD).transpose(2, 0, 1)
        d.update({f"{name}_in": x, f"{name}_box": np.asarray(box, np.int32), f"{name}_ops": np.asarray([o for o, _ in chain], np.int32),
                  f"{name}_factors": factors, f"{name}_u8": u8, f"{name}_out": np.ascontiguousarray(out)})
    path = os.path.join(HERE, "train_transform.npz")
    np.savez_compressed(path, names=np.array([c[0] for c in CASES]), interps=np.array([c[3] for c in CASES]), **d)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
