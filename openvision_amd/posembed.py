"""Fixed sin-cos position tables of the image tower, and the resizers that carry a learned table to another resolution.

The reference trains in stages (``scripts/project/openvision/train.sh``: pre-training at 84 px, then 224, then 336 / 384, each stage
started from the previous one's parameters).  Two things make a change of resolution possible there, and both live here:

* the image position table is a fixed function of the patch grid, regenerated when the grid changes (``src/models/vit.py:152-178``
  and ``:922-927``; the torch side as ``pos_embed_type='sin_cos_2d'``, ``open_clip/transformer.py:477-484``);
* a learned table is resampled when a checkpoint is loaded (``open_clip/model.py:523-586``: bicubic with antialiasing for the image
  grid, linear for the text positions).

Two forms of the fixed table exist and they are NOT the same numbers (0.022 apart already at a 4x4 grid of width 192):

    'sin_cos_2d'   MAE form, ``open_clip/pos_embed.py:20-67``: [sin w | cos w | sin h | cos h] halves of width / 4 frequencies
                   omega_k = 10000^(-k / (width/4)), computed in float64.
    'sincos2d'     MoCo-v3 form of the JAX recipe (``configs/openvision.py:164``), the one the converter writes into OpenVision
                   checkpoints (``transfer_jax2hf.py:98-112``): omega_k = 10000^(-k / (width/4 - 1)), computed in float32.

Everything here is load-time host arithmetic in numpy / torch on the CPU, with the reference's own operations, so that the tables
match the reference's.  Nothing here touches the device.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from .config import POS_EMBED_TYPES
from .convert_jax import posemb_sincos_2d as _moco_v3_table

FIXED_TYPES = tuple(t for t in POS_EMBED_TYPES if t != "learnable")
FORM_TOL = 1e-3           # a checkpoint's fixed table against the same form at its own grid: fp32 evaluations differ by ~ g * 2^-23


def _sincos_1d(dim: int, pos: np.ndarray) -> np.ndarray:
    """pos_embed.py:49-67: [sin(pos * omega) | cos(pos * omega)], omega_k = 10000^(-k / (dim/2)), float64."""
    omega = np.arange(dim // 2, dtype=float)
    omega /= dim / 2.
    omega = 1. / 10000 ** omega
    out = np.einsum("m,d->md", pos.reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def sincos_2d_mae(width: int, grid: int) -> torch.Tensor:
    """fp32 [1 + grid * grid, width]: the reference's ``get_2d_sincos_pos_embed(width, grid, cls_token=True)`` followed by
    ``.float()`` (transformer.py:483-484).  The meshgrid is w-major: the first half of the columns encodes the column index."""
    if width % 4:
        raise ValueError(f"pos_embed_type 'sin_cos_2d' needs a width that is a multiple of 4 (two halves, each sin | cos), got {width}")
    ax = np.arange(grid, dtype=np.float32)
    mesh = np.stack(np.meshgrid(ax, ax), axis=0).reshape([2, 1, grid, grid])        # here w goes first
    emb = np.concatenate([_sincos_1d(width // 2, mesh[0]), _sincos_1d(width // 2, mesh[1])], axis=1)
    emb = np.concatenate([np.zeros([1, width]), emb], axis=0)
    return torch.from_numpy(emb).float()


def sincos_2d_openvision(h: int, w: int, width: int) -> torch.Tensor:
    """fp32 [1 + h * w, width]: the MoCo-v3 table of the OpenVision recipe, exactly what the converter stores in a checkpoint."""
    return torch.from_numpy(_moco_v3_table(h, w, width, cls_token=True))


def fixed_table(pos_embed_type: str, grid: int, width: int) -> torch.Tensor:
    """The table of a fixed ``pos_embed_type`` on a square grid."""
    if pos_embed_type == "sin_cos_2d":
        return sincos_2d_mae(width, grid)
    if pos_embed_type == "sincos2d":
        return sincos_2d_openvision(grid, grid, width)
    raise ValueError(f"pos_embed_type {pos_embed_type!r} is not a fixed table (fixed: {FIXED_TYPES})")


def square_grid(num_patch_rows: int) -> int:
    """Side of the square grid behind a table's patch rows; ValueError when they do not form a square."""
    g = math.isqrt(int(num_patch_rows))
    if g * g != num_patch_rows or g == 0:
        raise ValueError(f"a position table with {num_patch_rows} patch rows is not a square grid")
    return g


def _to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


def resize_pos_embed(state_dict, model, interpolation: str = "bicubic", antialias: bool = True):
    """open_clip/model.py:523-554: resample ``state_dict['visual.positional_embedding']`` to ``model.visual.grid_size``, in place in
    the dict.  Returns without touching the dict when the key is missing or the table already has the model's length.  The class row
    is kept as it is.  A table whose patch rows are not a square raises ValueError."""
    old_pos_embed = state_dict.get("visual.positional_embedding", None)
    if old_pos_embed is None or not hasattr(model.visual, "grid_size"):
        return
    grid_size = _to_2tuple(model.visual.grid_size)
    extra_tokens = 1
    new_seq_len = grid_size[0] * grid_size[1] + extra_tokens
    if new_seq_len == old_pos_embed.shape[0]:
        return
    pos_emb_tok, pos_emb_img = old_pos_embed[:extra_tokens], old_pos_embed[extra_tokens:]
    old = square_grid(len(pos_emb_img))
    pos_emb_img = pos_emb_img.reshape(1, old, old, -1).permute(0, 3, 1, 2)
    pos_emb_img = F.interpolate(pos_emb_img, size=grid_size, mode=interpolation, antialias=antialias, align_corners=False)
    pos_emb_img = pos_emb_img.permute(0, 2, 3, 1).reshape(1, grid_size[0] * grid_size[1], -1)[0]
    state_dict["visual.positional_embedding"] = torch.cat([pos_emb_tok, pos_emb_img], dim=0)


def resize_text_pos_embed(state_dict, model, interpolation: str = "linear", antialias: bool = False):
    """open_clip/model.py:557-586: resample ``state_dict['positional_embedding']`` along the positions to the model's context length,
    in place in the dict; returns untouched when the key is missing or the lengths agree."""
    old_pos_embed = state_dict.get("positional_embedding", None)
    if old_pos_embed is None:
        return
    model_pos_embed = getattr(model, "positional_embedding", None)
    if model_pos_embed is None:
        model_pos_embed = getattr(model.text, "positional_embedding", None)
    old_num_pos, old_width = old_pos_embed.shape[0], old_pos_embed.shape[1]
    num_pos, width = model_pos_embed.shape[0], model_pos_embed.shape[1]
    assert old_width == width, "text pos_embed width changed!"
    if old_num_pos == num_pos:
        return
    old_pos_embed = old_pos_embed.reshape(1, old_num_pos, old_width).permute(0, 2, 1)
    old_pos_embed = F.interpolate(old_pos_embed, size=num_pos, mode=interpolation, antialias=antialias, align_corners=False)
    state_dict["positional_embedding"] = old_pos_embed.permute(0, 2, 1)[0]


def regenerate_fixed(state_dict, model) -> None:
    """A model with a fixed table, a checkpoint at another grid: the checkpoint's table is replaced by the regenerated one, never
    interpolated (vit.py:922-927).  Before that the checkpoint's table is compared against the same form generated at the
    checkpoint's OWN grid: more than ``FORM_TOL`` apart means a table of the other form or a trained one, and raises ValueError
    rather than continue a run on a table the weights were not trained with.  In place in the dict; no-op for a learnable model, a
    missing key or an equal length."""
    v = model.visual
    kind = getattr(v, "pos_embed_type", "learnable")
    old = state_dict.get("visual.positional_embedding", None)
    if kind not in FIXED_TYPES or old is None or old.shape[0] == v.positional_embedding.shape[0]:
        return
    g_old = square_grid(old.shape[0] - 1)
    width = v.positional_embedding.shape[1]
    if old.shape[1] != width:
        raise ValueError(f"visual.positional_embedding: width {old.shape[1]} in the checkpoint, {width} in the model")
    diff = float((old.detach().float().cpu() - fixed_table(kind, g_old, width)).abs().max())
    if not diff <= FORM_TOL:
        raise ValueError(f"pos_embed_type={kind!r}: the checkpoint's position table is not that form at its own {g_old}x{g_old} grid "
                         f"(max |delta| = {diff:.3g} > {FORM_TOL:g}): it is a table of another form ({' / '.join(FIXED_TYPES)}) or a "
                         f"trained one; load it with the matching pos_embed_type, or as 'learnable' to resample it")
    state_dict["visual.positional_embedding"] = fixed_table(kind, v.grid_size[0], width)


def resize_for(state_dict, model) -> None:
    """What a load into ``model`` at another resolution does to the state dict, in place: a fixed image table is regenerated
    (``regenerate_fixed``), a learned one resampled (``resize_pos_embed``), and the text table resampled (``resize_text_pos_embed``)."""
    regenerate_fixed(state_dict, model)
    resize_pos_embed(state_dict, model)
    resize_text_pos_embed(state_dict, model)
