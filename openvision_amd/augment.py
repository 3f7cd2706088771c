"""Training image transform on the device: batched random-resized crop, colour jitter, grayscale, ToTensor, Normalize.

Reference: the ``is_train=True`` branch of ``open_clip.transform.image_transform``
(``src/convert_upload/open_clip/transform.py:307-358``): ``RandomResizedCrop(size, scale, BICUBIC) -> _convert_to_rgb ->
[color_jitter] -> [gray_scale] -> ToTensor -> Normalize`` on PIL images; the OpenVision recipe's ``inception_crop(size, area_min=40,
method="bilinear")`` + ``simclr_jitter_gray`` (``src/configs/openvision.py:127-130``) is the same chain with ``interpolation=
"bilinear"`` and ``scale=(0.4, 1.0)``.

Two halves with different standing:

* The random numbers (``sample_crop_boxes``, ``sample_color_ops``) restate torchvision's ``RandomResizedCrop.get_params`` and
  ``ColorJitter.get_params`` and the reference's ``random.random() < p`` gates on the host.  torchvision is not installed where
  this project runs, so the draws are **parity unpinned**.
* Everything downstream of the drawn numbers runs in ``csrc/augment.hip`` in Pillow's own arithmetic (``crop().resize()``,
  ``ImageEnhance.Brightness / Contrast / Color``, ``convert("L")``) and is pinned bit for bit against Pillow
  (``tests/golden/train_transform.npz``, ``tests/train_transform_restate.py``).

The evaluation branch stays ``openvision_amd.preprocess.preprocess``.
"""
from __future__ import annotations

import ctypes
import math
import random
import warnings
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream_ptr, check
from .config import DEFAULT_PREPROCESS
from .preprocess import FILTERS, preprocess

OP_NONE, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_GRAYSCALE = range(5)      # include/ovhip.h enum ov_color_op
INTERPOLATION = {"bilinear": 0, "bicubic": 1}                                     # include/ovhip.h enum ov_interp
WORKSPACE_LIMIT = 1 << 30                # a batch whose workspace would exceed this is run in consecutive chunks


@dataclass
class AugmentationCfg:
    """The reference's ``AugmentationCfg`` (``transform.py:61-72``), same fields and defaults."""
    scale: Tuple[float, float] = (0.9, 1.0)
    ratio: Optional[Tuple[float, float]] = None
    color_jitter: Optional[Union[float, Tuple[float, float, float], Tuple[float, float, float, float]]] = None
    re_prob: Optional[float] = None
    re_count: Optional[int] = None
    use_timm: bool = False
    color_jitter_prob: Optional[float] = None        # params for simclr_jitter_gray
    gray_scale_prob: Optional[float] = None

    def __post_init__(self):
        if self.use_timm:
            raise NotImplementedError("AugmentationCfg.use_timm: the timm transform is not implemented")
        unused = [k for k in ("ratio", "re_prob", "re_count") if getattr(self, k) is not None]
        if unused:      # transform.py:356-357: without use_timm the crop keeps torchvision's default ratio and nothing is erased
            warnings.warn(f"Unused augmentation cfg items, specify `use_timm` to use ({unused}).")


def max_taps(extent: int, out: int, interpolation: str) -> int:
    """Row length of Pillow's coefficient table for extent -> out (``resize_plan(...)[2]``), without building the table."""
    return int(math.ceil(FILTERS[interpolation][1] * max(extent / out, 1.0))) * 2 + 1


# ---- the random numbers (host; restated from torchvision, parity unpinned) --------------------------------------------------------
def _uniform(lo: float, hi: float) -> float:
    return torch.empty(1).uniform_(lo, hi).item()


def sample_crop_boxes(shapes: Sequence[Tuple[int, int]], scale: Tuple[float, float] = (0.9, 1.0),
                      ratio: Tuple[float, float] = (3.0 / 4.0, 4.0 / 3.0)) -> np.ndarray:
    """``RandomResizedCrop.get_params`` per (H, W) in order, from torch's CPU default generator: int32 [B, 4] = (top, left, h, w)."""
    log_ratio = torch.log(torch.tensor(ratio))
    boxes = np.zeros((len(shapes), 4), np.int32)
    for n, (height, width) in enumerate(shapes):
        height, width = int(height), int(width)
        area = height * width
        for _ in range(10):
            target_area = area * _uniform(scale[0], scale[1])
            aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < w <= width and 0 < h <= height:
                top = torch.randint(0, height - h + 1, size=(1,)).item()
                left = torch.randint(0, width - w + 1, size=(1,)).item()
                break
        else:                                        # fall back to the central crop, clamped to the ratio range
            in_ratio = float(width) / float(height)
            if in_ratio < min(ratio):
                w = width
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = height
                w = int(round(h * max(ratio)))
            else:
                w, h = width, height
            top, left = (height - h) // 2, (width - w) // 2
        boxes[n] = (top, left, h, w)
    return boxes


def _jitter_strengths(color_jitter) -> Tuple[float, float, float]:
    if color_jitter is None:
        raise ValueError("color_jitter_prob is set but color_jitter is not")
    if isinstance(color_jitter, (int, float)):
        color_jitter = (color_jitter,) * 3
    cj = tuple(float(v) for v in color_jitter)
    if len(cj) not in (3, 4):
        raise ValueError("color_jitter: a strength, or (brightness, contrast, saturation[, hue])")
    if len(cj) == 4 and cj[3] != 0.0:
        raise NotImplementedError("color_jitter: hue is not implemented (hue must be 0)")
    if min(cj[:3]) < 0:
        raise ValueError("color_jitter: strengths must be non-negative")
    return cj[:3]


def sample_color_ops(B: int, color_jitter=None, color_jitter_prob: Optional[float] = None,
                     gray_scale_prob: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The colour operations of B images in application order: ops int32 [B, 4] (OP_*), factors float32 [B, 4].

    Per image, as the reference's wrappers (``transform.py:242-271``): ``random.random() < color_jitter_prob`` gates a
    ``ColorJitter`` — ``torch.randperm(4)`` over (brightness, contrast, saturation, hue), then one ``uniform_(max(0, 1 - s), 1 + s)``
    per non-zero strength in that fixed order; a zero strength draws nothing and keeps its place in the permutation — and
    ``random.random() < gray_scale_prob`` gates ``Grayscale(3)`` after it."""
    ops = np.zeros((B, 4), np.int32)
    factors = np.zeros((B, 4), np.float32)
    strengths = _jitter_strengths(color_jitter) if color_jitter_prob else None
    for n in range(B):
        k = 0
        if color_jitter_prob and random.random() < color_jitter_prob:
            perm = torch.randperm(4).tolist()
            drawn = [_uniform(max(0.0, 1.0 - s), 1.0 + s) if s != 0.0 else None for s in strengths]
            for fn in perm:
                if fn < 3 and drawn[fn] is not None:
                    ops[n, k], factors[n, k] = OP_BRIGHTNESS + fn, drawn[fn]
                    k += 1
        if gray_scale_prob and random.random() < gray_scale_prob:
            ops[n, k] = OP_GRAYSCALE
    return ops, factors


# ---- the device call ----------------------------------------------------------------------------------------------------------------
class _Staging:
    """A pinned host buffer reused from call to call.  Before it is overwritten the host waits for the last copy out of it — an
    event recorded right behind that copy, so never for a kernel."""

    def __init__(self):
        self.buf = None
        self.event = None

    def host(self, nbytes: int) -> np.ndarray:
        if self.event is not None:
            self.event.synchronize()
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self.buf.numpy()[:nbytes]

    def to_device(self, nbytes: int, dev: torch.device) -> torch.Tensor:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out.copy_(self.buf[:nbytes], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        return out


_pixel_staging, _table_staging = _Staging(), _Staging()


def check_boxes(shapes: np.ndarray, boxes: np.ndarray) -> None:
    for n, ((H, W), (top, left, h, w)) in enumerate(zip(shapes.tolist(), boxes.tolist())):
        if h <= 0 or w <= 0 or top < 0 or left < 0 or top + h > H or left + w > W:
            raise ValueError(f"train_transform: box {(top, left, h, w)} of image {n} is empty or outside its {H} x {W} image")


def plan_chunks(boxes: np.ndarray, size: int, interpolation: str, limit: Optional[int] = None) -> List[Tuple[int, int, int, int, int, int]]:
    """Consecutive chunks (start, stop, max_rows, max_taps_x, max_taps_y, workspace_bytes) of the batch, each within ``limit`` bytes
    (``WORKSPACE_LIMIT`` by default) of workspace; a single image that exceeds it still gets a chunk of its own."""
    lib = _lib.load()
    limit = WORKSPACE_LIMIT if limit is None else limit

    def need(a, b):
        rows = int(boxes[a:b, 2].max())
        kx = max_taps(int(boxes[a:b, 3].max()), size, interpolation)
        ky = max_taps(rows, size, interpolation)
        return rows, kx, ky, int(lib.ov_train_transform_workspace_bytes(b - a, size, size, rows, kx, ky))

    chunks, start, B = [], 0, len(boxes)
    while start < B:
        stop = B
        while True:
            rows, kx, ky, nbytes = need(start, stop)
            if nbytes <= limit or stop - start == 1:
                break
            stop = start + (stop - start + 1) // 2
        chunks.append((start, stop, rows, kx, ky, nbytes))
        start = stop
    return chunks


def stage(arrays: Sequence[np.ndarray], tables: Sequence[np.ndarray], dev: torch.device):
    """The images packed back to back into the pinned pixel buffer and copied in one non-blocking copy; their offsets (int64, first:
    every table then starts on its own alignment) and ``tables`` packed into the second buffer and copied in another.  Returns the
    device pixels and one device byte view per table, offsets first."""
    sizes = np.array([a.size for a in arrays], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    total = int(sizes.sum())
    host = _pixel_staging.host(total)
    for a, o in zip(arrays, offsets.tolist()):
        host[o:o + a.size] = a.reshape(-1)
    pixels = _pixel_staging.to_device(total, dev)
    tables = [offsets] + list(tables)
    at = np.cumsum([0] + [t.nbytes for t in tables]).tolist()
    host = _table_staging.host(at[-1])
    for t, a in zip(tables, at):
        host[a:a + t.nbytes] = t.reshape(-1).view(np.uint8)
    tab = _table_staging.to_device(at[-1], dev)
    return pixels, [tab[a:a + t.nbytes] for t, a in zip(tables, at)]


def launch(pixels: torch.Tensor, tables: Sequence[torch.Tensor], boxes: np.ndarray, ops: np.ndarray, size: int, interpolation: str,
           mean, std, out: torch.Tensor) -> None:
    """ov_train_transform on staged inputs (``stage``), chunk by chunk, into ``out`` [B, 3, size, size]; ``boxes`` / ``ops`` are the
    host copies the workspace and the number of statistics passes are sized from."""
    lib = _lib.load()
    d_offsets, d_shapes, d_boxes, d_ops, d_factors = tables
    cm = (ctypes.c_float * 3)(*mean)
    cs = (ctypes.c_float * 3)(*std)
    code = {torch.float32: _lib.OV_F32, torch.bfloat16: _lib.OV_BF16}[out.dtype]
    for start, stop, rows, kx, ky, nbytes in plan_chunks(boxes, size, interpolation):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
        passes = int((ops[start:stop] == OP_CONTRAST).sum(axis=1).max())
        check(lib.ov_train_transform(ptr(pixels), pixels.numel(), ptr(d_offsets[8 * start:]), ptr(d_shapes[8 * start:]),
                                     ptr(d_boxes[16 * start:]), ptr(d_ops[16 * start:]), ptr(d_factors[16 * start:]), stop - start, size,
                                     size, rows, INTERPOLATION[interpolation], kx, ky, passes, cm, cs, ptr(out[start:]), code, ptr(ws),
                                     nbytes, stream_ptr()), "ov_train_transform")


def train_transform(images: Sequence, size: int, mean=None, std=None, interpolation: str = "bicubic", aug_cfg=None, boxes=None,
                    color_ops=None, dtype: torch.dtype = torch.float32, device="cuda:0") -> torch.Tensor:
    """uint8 RGB images [H, W, 3] on the host (any sizes; numpy arrays or torch tensors) -> one training batch
    [B, 3, size, size] on the device.

    ``boxes`` (int [B, 4] = top, left, h, w) and ``color_ops`` ((ops int [B, 4], factors float [B, 4])) override the draws; without
    them each image draws its crop, then its colour operations, from ``aug_cfg`` (an ``AugmentationCfg`` or its dict).  The images
    go through one pinned staging buffer and one non-blocking copy, every table through a second; the kernels follow on the current
    stream and nothing waits for them."""
    if interpolation not in INTERPOLATION:
        raise NotImplementedError(f"interpolation {interpolation!r} (only 'bilinear' and 'bicubic')")
    if isinstance(aug_cfg, dict):
        aug_cfg = AugmentationCfg(**aug_cfg)
    cfg = aug_cfg or AugmentationCfg()
    mean = list(mean if mean is not None else DEFAULT_PREPROCESS["mean"])
    std = list(std if std is not None else DEFAULT_PREPROCESS["std"])
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("train_transform: dtype is torch.float32 or torch.bfloat16")
    _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.OvhipError("train_transform: needs an MI355X device (no CPU fallback)")

    arrays = [im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im) for im in images]
    B = len(arrays)
    for a in arrays:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] == 0 or a.shape[1] == 0:
            raise ValueError("train_transform: expected uint8 [H, W, 3] RGB images")
    shapes = np.array([a.shape[:2] for a in arrays], np.int32).reshape(B, 2)
    if boxes is None or color_ops is None:
        drawn_boxes, drawn_ops, drawn_factors = np.zeros((B, 4), np.int32), np.zeros((B, 4), np.int32), np.zeros((B, 4), np.float32)
        for n in range(B):                           # per image: the crop's draws, then the jitter's
            if boxes is None:
                drawn_boxes[n] = sample_crop_boxes([shapes[n]], cfg.scale)[0]
            if color_ops is None:
                o, f = sample_color_ops(1, cfg.color_jitter, cfg.color_jitter_prob, cfg.gray_scale_prob)
                drawn_ops[n], drawn_factors[n] = o[0], f[0]
        boxes = drawn_boxes if boxes is None else boxes
        color_ops = (drawn_ops, drawn_factors) if color_ops is None else color_ops
    boxes = np.ascontiguousarray(np.asarray(boxes, np.int64).reshape(B, 4))
    check_boxes(shapes, boxes)
    ops = np.ascontiguousarray(np.asarray(color_ops[0], np.int32).reshape(B, 4))
    factors = np.ascontiguousarray(np.asarray(color_ops[1], np.float32).reshape(B, 4))
    if ops.min(initial=0) < OP_NONE or ops.max(initial=0) > OP_GRAYSCALE:
        raise ValueError("train_transform: colour operations are 0 (none) .. 4 (grayscale)")
    boxes = boxes.astype(np.int32)

    out = torch.empty(B, 3, size, size, dtype=dtype, device=dev)
    if B == 0:
        return out
    pixels, tables = stage(arrays, [shapes, boxes, ops, factors], dev)
    launch(pixels, tables, boxes, ops, size, interpolation, mean, std, out)
    return out


def image_transform(image_size: int, is_train: bool, mean=None, std=None, resize_mode: Optional[str] = None,
                    interpolation: Optional[str] = None, aug_cfg=None, dtype: torch.dtype = torch.float32, device="cuda:0"):
    """The reference's ``image_transform`` (``transform.py:274-390``) over a LIST of images: a callable returning the device batch.
    ``is_train=False``: the existing ``preprocess`` (``resize_mode`` 'shortest' and 'bicubic' by default, as the reference).
    ``is_train=True``: ``train_transform``, always bicubic like the reference's ``RandomResizedCrop``."""
    if isinstance(image_size, (tuple, list)):
        if len(set(image_size)) != 1:
            raise NotImplementedError("image_transform: square output sizes only")
        image_size = image_size[0]
    if isinstance(aug_cfg, dict):
        aug_cfg = AugmentationCfg(**aug_cfg)
    if is_train:
        return lambda images: train_transform(images, image_size, mean, std, "bicubic", aug_cfg, dtype=dtype, device=device)
    mode, interp = resize_mode or "shortest", interpolation or "bicubic"
    return lambda images: preprocess(images, image_size, mean, std, mode, interp, dtype=dtype, device=device)
