"""Numpy restatement of the training image transform's pinned half (tests only; independent of the HIP kernels).

Colour stage, in Pillow 12.2.0's arithmetic:
  convert("L")            src/libImaging/Convert.c rgb2l     L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16
  ImageEnhance.*          PIL/ImageEnhance.py                Image.blend(degenerate, image, factor); degenerate = black (Brightness),
                                                             the constant int(mean(L) + 0.5) (Contrast), L (Color = saturation)
  Image.blend             src/libImaging/Blend.c             fp32 degenerate + factor * (image - degenerate), product and sum rounded
                                                             separately; truncated for 0 <= factor <= 1, else clipped then truncated
Resize: ``oracle.preprocess_ref.pil_resize_u8`` on the cropped sub-array (crop().resize() builds its tables for the crop extent).
PARITY PINNING: tests/test_train_transform_cpu.py holds this file against Pillow itself and against the committed Pillow outputs in
tests/golden/train_transform.npz (tests/golden/make_golden_train_transform.py).
"""
from functools import lru_cache

import numpy as np

from oracle.preprocess_ref import pil_resize_u8

NONE, BRIGHTNESS, CONTRAST, SATURATION, GRAYSCALE = range(5)
_WR, _WG, _WB = 19595, 38470, 7471


def luma(img: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] -> uint8 [...]"""
    v = img.astype(np.int64)
    return ((v[..., 0] * _WR + v[..., 1] * _WG + v[..., 2] * _WB + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate: np.ndarray, img: np.ndarray, factor) -> np.ndarray:
    """Image.blend(degenerate, img, factor) on uint8 arrays of one shape."""
    f = np.float32(factor)
    d = degenerate.astype(np.int32)
    prod = f * (img.astype(np.int32) - d).astype(np.float32)            # float32, rounded
    t = d.astype(np.float32) + prod                                     # float32, rounded again
    assert prod.dtype == np.float32 and t.dtype == np.float32
    if np.float32(0) <= f <= np.float32(1):
        return t.astype(np.uint8)                                        # in [0, 255]: the cast truncates
    return np.where(t <= 0, np.float32(0), np.where(t >= 255, np.float32(255), t)).astype(np.uint8)


def contrast_mean(img: np.ndarray) -> int:
    """ImageEnhance.Contrast: int(ImageStat.Stat(image.convert("L")).mean[0] + 0.5)"""
    l = luma(img)
    return int(int(l.astype(np.int64).sum()) / l.size + 0.5)


def apply_op(img: np.ndarray, op: int, factor) -> np.ndarray:
    if op == NONE:
        return img
    if op == GRAYSCALE:
        return np.repeat(luma(img)[..., None], 3, axis=-1)
    if op == BRIGHTNESS:
        deg = np.zeros_like(img)
    elif op == CONTRAST:
        deg = np.full_like(img, contrast_mean(img))
    elif op == SATURATION:
        deg = np.repeat(luma(img)[..., None], 3, axis=-1)
    else:
        raise ValueError(op)
    return blend(deg, img, factor)


def apply_ops(img: np.ndarray, ops, factors) -> np.ndarray:
    for op, f in zip(ops, factors):
        img = apply_op(img, int(op), f)
    return img


def to_tensor_normalize(u8: np.ndarray, mean, std) -> np.ndarray:
    x = u8.astype(np.float32) / np.float32(255.0)
    x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def train_transform_u8(img: np.ndarray, box, size: int, interpolation: str, ops=(), factors=()) -> np.ndarray:
    top, left, h, w = (int(v) for v in box)
    return apply_ops(pil_resize_u8(img[top:top + h, left:left + w], size, size, interpolation), ops, factors)


def train_transform(img, box, size, interpolation, ops, factors, mean, std) -> np.ndarray:
    """uint8 [H, W, 3] -> float32 [3, size, size]"""
    return to_tensor_normalize(train_transform_u8(img, box, size, interpolation, ops, factors), mean, std)


# ---- the saturation image that a contracted multiply-add cannot pass ---------------------------------------------------------------
@lru_cache(maxsize=1)
def saturation_pairs_image():
    """uint8 [256, 256, 3]: pixel (d, p) has L == d and one channel == p wherever an RGB triple with both exists; the others are the
    gray (p, p, p).  L is a weighted mean of the three channels, so a pair (d, p) far from the diagonal exists in no RGB image (with
    the blue channel == p, L lies within [0.114 p, 0.114 p + 226]): ``reachable`` [256, 256] bool marks the pairs present, 58 096 of
    the 65 536, among them 280 of the 309 pairs on which a fused multiply-add changes the byte at factor 1.32."""
    img = np.empty((256, 256, 3), np.uint8)
    reachable = np.zeros((256, 256), bool)
    p = np.arange(256, dtype=np.int64)[:, None]           # the pinned channel's value
    a = np.arange(256, dtype=np.int64)[None, :]           # the second channel's value; the third is solved for
    weights = (_WR, _WG, _WB)
    for d in range(256):
        img[d] = np.arange(256, dtype=np.uint8)[:, None]
        for c in (2, 0, 1):                                # blue has the smallest weight: widest range of L for a given p
            ca, cb = [k for k in range(3) if k != c]
            rest = weights[c] * p + weights[ca] * a + 0x8000
            lo = (d << 16) - rest                          # need lo <= w_b * b <= lo + 65535
            b = np.maximum(-(-lo // weights[cb]), 0)
            ok = (b <= 255) & (weights[cb] * b <= lo + 65535)
            has = ok.any(axis=1) & ~reachable[d]
            first = ok.argmax(axis=1)
            rows = np.nonzero(has)[0]
            img[d, rows, c] = rows
            img[d, rows, ca] = first[rows]
            img[d, rows, cb] = b[rows, first[rows]]
            reachable[d, rows] = True
    assert np.array_equal(luma(img)[reachable], np.nonzero(reachable)[0].astype(np.uint8))
    return img, reachable


def fma_sensitive(degenerate: np.ndarray, img: np.ndarray, factor) -> np.ndarray:
    """Where Image.blend's result changes if degenerate + factor * (image - degenerate) is rounded once (a fused multiply-add): the
    sum is exact in float64 (24-bit factor x 9-bit difference + 8-bit integer), so one conversion to float32 is the fused result."""
    f = np.float32(factor)
    d = degenerate.astype(np.int32)
    t = (d.astype(np.float64) + np.float64(f) * (img.astype(np.int32) - d).astype(np.float64)).astype(np.float32)
    if np.float32(0) <= f <= np.float32(1):
        fused = t.astype(np.uint8)
    else:
        fused = np.where(t <= 0, np.float32(0), np.where(t >= 255, np.float32(255), t)).astype(np.uint8)
    return fused != blend(degenerate, img, factor)
