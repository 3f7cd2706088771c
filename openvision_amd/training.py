"""Training-side forward with gradients: the block stacks and the InfoNCE loss are autograd nodes whose
forward AND backward are the HIP kernels (``ov_tower_forward_saving_from`` / ``ov_tower_backward_partial`` or, under recomputation,
``ov_tower_forward_checkpointed`` / ``ov_tower_backward_checkpointed``; ``ov_clip_loss_multi`` / ``ov_clip_loss_multi_backward`` at
C = 1, ``openvision_amd.loss``).  The tower handles and the packed weights they borrow are ``model._TowerCache``'s.  The light ends
around the towers run on the HIP operators too: the patch projection and the output projections are autograd nodes over ``ov_gemm`` /
``ov_linear_backward``, ``ln_post`` / ``ln_final`` over ``ov_layernorm`` / ``ov_layernorm_backward``
(open_clip/transformer.py:609-651, model.py:265-315); what is left to torch autograd is data movement and element-wise plumbing
(class / positional embedding adds, token gather, mean pooling, L2 normalisation) -- no aten GEMM.

Opt-in: the inference entry points of ``openvision_amd.model`` never build a graph; a training loop calls

    img_f, txt_f, scale = training.clip_forward(model, images, tokens)       # features carry grad
    loss = ClipLoss(...)(img_f, txt_f, scale)                               # openvision_amd.loss.ClipLoss
    loss.backward()                                                         # .grad on every parameter, as with the reference

Activation memory: by default the tower keeps, per layer and token, the block input, the packed qkv, the attention output, the
mid-block residual, both LayerNorm outputs and the c_fc pre-activation and activation (8 D + 2 mlp bf16: 52 GB for L/14 at B=256);
the backward runs nothing of the forward again.  ``model.set_grad_checkpointing()`` (the reference's remat='full' per block) keeps
only each block's input (D bf16 per layer and token: 3.2 GB) plus one layer's intermediates, and the backward recomputes each
block's intermediates with the forward's own launches just before that block's backward: the same loss and gradients, bit for bit.
Every preset is covered: head dims 72 / 80 (So400m, H/14) take the streaming attention backward with d zero-padded to 96, an MLP
width that is not a multiple of 64 (So400m) is zero-padded.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, ptr, stream_ptr
from .model import _dtype_flag, _gemm_bias, _kernel_input, _pack_matrix, _pack_vec, _round_up

_NAMES = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b")


def _block_tensors(blk) -> List[torch.Tensor]:
    """The module's own parameters in ov_block_weights order (reference names: transformer.py:210-236)."""
    return [blk.ln_1.weight, blk.ln_1.bias, blk.attn.in_proj_weight, blk.attn.in_proj_bias, blk.attn.out_proj.weight,
            blk.attn.out_proj.bias, blk.ln_2.weight, blk.ln_2.bias, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias,
            blk.mlp.c_proj.weight, blk.mlp.c_proj.bias]


class _Pool:
    """Grow-only pool of device buffers, one free list per purpose ("saved": the activations a forward keeps for its backward, or the
    block inputs under recomputation; "slot": one layer's intermediates under recomputation; "ws": kernel workspaces): a step takes
    what it needs in forward and hands it back at the end of backward, so
    steady-state training allocates nothing per step.  Retention sizes itself: per purpose the pool keeps as many free buffers as
    were ever outstanding at once (one saved buffer per chunk of `set_backward_chunk_layers`, one workspace), and a request is served
    by the SMALLEST free buffer of its own purpose that fits, so a workspace never takes a saved-activation buffer."""

    def __init__(self):
        self.lists = {}                    # purpose -> free buffers, ascending size
        self.out = {}                      # purpose -> buffers currently handed out
        self.peak = {}                     # purpose -> high-water mark of `out`
        self.out_bytes = {}                # purpose -> bytes requested by the buffers currently handed out

    @property
    def free(self) -> List[torch.Tensor]:
        return [t for lst in self.lists.values() for t in lst]

    def take(self, nbytes: int, device, kind: str = "ws") -> torch.Tensor:
        lst = self.lists.setdefault(kind, [])
        self.out[kind] = self.out.get(kind, 0) + 1
        self.peak[kind] = max(self.peak.get(kind, 0), self.out[kind])
        self.out_bytes[kind] = self.out_bytes.get(kind, 0) + int(nbytes)
        for i, t in enumerate(lst):
            if t.device == device and t.numel() >= nbytes:
                t = lst.pop(i)
                t._ovhip_gen += 1              # whoever still holds it from an earlier step can tell it was recycled
                t._ovhip_req = int(nbytes)
                return t
        t = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
        t._ovhip_gen, t._ovhip_kind, t._ovhip_req = 0, kind, int(nbytes)
        return t

    def give(self, t: torch.Tensor) -> None:
        kind = getattr(t, "_ovhip_kind", "ws")
        lst = self.lists.setdefault(kind, [])
        if any(u is t for u in lst):
            return
        self.out[kind] = max(0, self.out.get(kind, 0) - 1)
        self.out_bytes[kind] = max(0, self.out_bytes.get(kind, 0) - getattr(t, "_ovhip_req", 0))
        lst.append(t)
        lst.sort(key=lambda x: x.numel())
        del lst[:-max(1, self.peak.get(kind, 1))]        # too many: the smallest go (a grown request made them useless)


def _pool(transformer) -> _Pool:
    """The tower's pool, made on first use and kept on the module."""
    pool = getattr(transformer, "_ovhip_pool", None)
    if pool is None:
        pool = _Pool()
        object.__setattr__(transformer, "_ovhip_pool", pool)
    return pool


def drop_path_rates(rate: float, layers: int) -> np.ndarray:
    """The per-block drop rates of a tower of ``layers`` blocks: ``np.linspace(0, rate, layers)`` (vit.py:358,
    text_transformer.py:533-536) -- block 0 never drops, the top block drops with ``rate``."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"drop_path rate {rate} outside [0, 1)")
    return np.linspace(0, rate, int(layers))


class DropPathTable:
    """Which samples each residual branch of each block keeps in ONE training forward and its backward: ``keep`` bool [layers, 2, B]
    on the host (branch 0 = attention, 1 = MLP) and ``scale`` fp32 [layers] = 1 / (1 - r_i), the factor of a kept sample's branch
    (DropPath, common.py:659-675).  ``counts[i][j]`` kept samples; ``device_tables(device)`` -> int32 ``idx`` / ``slot`` [layers, 2, B]
    on the device (``ov_tower_set_drop_path``'s layout: the kept samples' numbers first in ascending order, then the dropped ones';
    ``slot`` the inverse, -1 for a dropped sample), made on first use from a pinned staging copy by an asynchronous upload: no host
    synchronisation.  ``slice(lo, hi)``: the table of blocks [lo, hi), sharing the device arrays."""

    def __init__(self, keep: torch.Tensor, scale: torch.Tensor):
        if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool:
            raise TypeError("keep must be a torch.bool tensor [layers, 2, batch]")
        if keep.dim() != 3 or keep.shape[1] != 2 or keep.shape[0] < 1 or keep.shape[2] < 1:
            raise ValueError(f"keep must be [layers, 2, batch], got {tuple(keep.shape)}")
        scale = torch.as_tensor(scale, dtype=torch.float32).detach().cpu().reshape(-1)
        if scale.shape[0] != keep.shape[0] or not bool(torch.isfinite(scale).all()) or not bool((scale > 0).all()):
            raise ValueError("scale must hold one finite positive factor per layer")
        self.keep = keep.detach().cpu().contiguous()
        self.scale = scale.contiguous()
        self.layers, _, self.batch = self.keep.shape
        self.counts = self.keep.sum(dim=-1).tolist()
        self._host = None
        self._dev = {}
        self._parent = None

    def host_tables(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(idx, slot), int32 [layers, 2, B] on the host."""
        if self._host is None:
            idx = torch.argsort((~self.keep).to(torch.uint8), dim=-1, stable=True)
            rank = torch.empty_like(idx).scatter_(-1, idx, torch.arange(self.batch).expand_as(idx).contiguous())
            slot = torch.where(self.keep, rank, torch.full_like(rank, -1))
            self._host = torch.stack([idx.to(torch.int32), slot.to(torch.int32)]).contiguous()
        return self._host[0], self._host[1]

    def device_tables(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        device = torch.device(device)
        if self._parent is not None:                          # a slice: rows [lo, hi) of the parent's arrays (contiguous views)
            parent, lo, hi = self._parent
            idx, slot = parent.device_tables(device)
            return idx[lo:hi], slot[lo:hi]
        dev = self._dev.get(device)
        if dev is None:
            self.host_tables()
            if device.type == "cuda" and not self._host.is_pinned():
                self._host = self._host.pin_memory()          # kept alive here: the copy below may still be reading it
            dev = self._dev[device] = self._host.to(device, non_blocking=True)
        return dev[0], dev[1]

    def slice(self, lo: int, hi: int) -> "DropPathTable":
        if lo == 0 and hi == self.layers:
            return self
        sub = DropPathTable(self.keep[lo:hi], self.scale[lo:hi])
        sub._parent = (self, lo, hi)
        return sub


def drop_path_table(transformer, batch: int, generator: Optional[torch.Generator] = None, keep: Optional[torch.Tensor] = None,
                    scale=None) -> Optional[DropPathTable]:
    """The drop-path table of one forward of ``transformer`` over ``batch`` samples.  Without ``keep`` it is drawn as the reference
    draws it (common.py:673-674): per block, branch and sample ``floor(keep_i + U)`` with ``U = torch.rand`` on the CPU (``generator``,
    or the default one), ``keep_i = 1 - linspace(0, transformer.drop_path, layers)[i]``; a rate of 0 makes no table (None).  ``keep``
    (bool [layers, 2, batch]) replaces the draw; ``scale`` ([layers], default 1 / keep_i) replaces the factors.  The masks are not
    seed-compatible with the JAX reference's generator."""
    layers = len(transformer.resblocks)
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be positive")
    rates = drop_path_rates(getattr(transformer, "drop_path", 0.0), layers)
    keep_p = torch.from_numpy(1.0 - rates).to(torch.float32)
    if keep is None:
        if rates[-1] == 0.0:
            return None
        u = torch.rand(layers, 2, batch, generator=generator)
        keep = torch.floor(keep_p[:, None, None] + u) >= 1.0
    else:
        if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool:
            raise TypeError("keep must be a torch.bool tensor [layers, 2, batch]")
        if tuple(keep.shape) != (layers, 2, batch):
            raise ValueError(f"keep must be [{layers}, 2, {batch}], got {tuple(keep.shape)}")
    return DropPathTable(keep, 1.0 / keep_p if scale is None else scale)


def _own_drop(transformer, batch: int, drop: Optional[DropPathTable]) -> Optional[DropPathTable]:
    """The table a forward of ``transformer`` runs under: the caller's whatever the mode, else one drawn when the transformer is in
    training mode with ``drop_path`` > 0, else none."""
    if drop is not None:
        if not isinstance(drop, DropPathTable):
            raise TypeError("drop must be a training.DropPathTable (training.drop_path_table)")
        if drop.layers != len(transformer.resblocks) or drop.batch != int(batch):
            raise ValueError(f"drop table is [{drop.layers}, 2, {drop.batch}], the forward needs [{len(transformer.resblocks)}, 2, {batch}]")
        return drop
    if transformer.training and getattr(transformer, "drop_path", 0.0) > 0:
        return drop_path_table(transformer, batch)
    return None


@contextlib.contextmanager
def _drop_scope(lib, handle, drop: Optional[DropPathTable], bsz: int, seq: int, pool, device):
    """The handle carries ``drop`` (``ov_tower_set_drop_path``, with its scratch from the pool) for the native calls made inside, and
    no table again afterwards, on success and on error alike: the cached handle is shared with whoever runs this tower next."""
    if drop is None:
        yield
        return
    nbytes = lib.ov_tower_drop_path_workspace_bytes(handle, bsz, seq)
    ws = pool.take(nbytes, device, "drop")
    try:
        idx, slot = drop.device_tables(device)
        counts = (ctypes.c_int * (2 * drop.layers))(*[int(c) for row in drop.counts for c in row])
        scales = (ctypes.c_float * drop.layers)(*drop.scale.tolist())
        check(lib.ov_tower_set_drop_path(handle, ptr(idx), ptr(slot), counts, scales, bsz, ptr(ws), nbytes), "ov_tower_set_drop_path")
        try:
            yield
        finally:
            lib.ov_tower_set_drop_path(handle, None, None, None, None, 0, None, 0)
    finally:
        pool.give(ws)


class _TowerFn(torch.autograd.Function):
    """Transformer.forward (transformer.py:355-366) as one autograd node over the blocks [lo, hi) (all of them by default; several
    consecutive nodes when ``tower_forward`` is asked for chunks, so that parameter gradients become available chunk by chunk).

    Frozen parameters (``requires_grad=False``: ``lock_image_tower``, a frozen text tower under gradient ascent) are honoured per
    (weight, bias) pair of a block: a pair is frozen when both of its tensors are.  ``first`` is 0 when x needs a gradient, else the
    lowest block with a trainable pair: the blocks below it run without keeping anything (``ov_tower_forward_saving_from``) and the
    backward stops at it (``ov_tower_backward_partial``, the requested pairs only); frozen blocks above it run input-only.  With
    everything trainable that is the full backward's launches, and every gradient that is computed is bitwise the all-trainable one.

    Recomputation (``transformer.grad_checkpointing``): the same calls' checkpointed forms.  ``ov_tower_forward_checkpointed`` keeps
    only the inputs of layers [first, hi - lo) ("saved") and one layer's intermediates ("slot"); ``ov_tower_backward_checkpointed``
    rebuilds each block's slot before its backward.  The node holding the tower's last block keeps its slot until its backward (no
    recompute of that block); every other node hands its slot back after the forward.  Loss and gradients are bitwise those without
    it.  In both modes a failed native call hands every pool buffer it took back.

    The handle is ``transformer._cache``'s over the span [lo, hi), bf16 over the module's own LayerNorms; the ctx keeps it, so the
    backward runs the very handle of the forward.  ``_PrefixTowerFn`` below is the same node with a prefix-causal attention mask,
    which is part of what the cache builds the handle for."""

    NARGS = 3            # non-tensor arguments in front of x

    @classmethod
    def _split(cls, args):
        return None, args[0], args[1:]

    @classmethod
    def _drop(cls, args):
        return None

    @classmethod
    def forward(cls, ctx, transformer, lo, hi, *args):
        prefix, x, params = cls._split(args)
        drop = cls._drop(args)
        ctx.nargs = cls.NARGS
        blocks = list(transformer.resblocks)[lo:hi]
        b0 = blocks[0]
        d, heads = b0.attn.embed_dim, b0.attn.num_heads
        if d % 64 or d % heads or (d // heads) % 8 or d // heads > 96:
            raise _lib.OvhipError("training path: width % 64 == 0 and head_dim % 8 == 0, <= 96 are required")
        bsz, seq, _ = x.shape
        layers = len(blocks)
        need_x, need_p = ctx.needs_input_grad[ctx.nargs], ctx.needs_input_grad[ctx.nargs + 1:]
        if prefix is not None and not 0 <= int(prefix) <= seq:
            raise ValueError(f"causal prefix {prefix} outside [0, {seq}]")
        pairs = [[need_p[12 * i + 2 * k] or need_p[12 * i + 2 * k + 1] for k in range(6)] for i in range(layers)]
        first = 0 if need_x else next((i for i, pr in enumerate(pairs) if any(pr)), layers)
        tower = transformer._cache.get(blocks, prefix, first=lo, plain=True)      # built when a weight or the prefix changed, not per step
        lib, handle = tower.lib, tower.handle
        pool = _pool(transformer)
        remat = bool(getattr(transformer, "grad_checkpointing", False))
        saved = slot = None
        try:
            xb = x.detach().to(torch.bfloat16).contiguous().clone()
            if remat:        # the kept layers' inputs, and one layer's intermediates (the layers below `first` use them as scratch)
                nsaved, nslot, kind = (lib.ov_tower_checkpoint_bytes(handle, first, bsz, seq), lib.ov_tower_slot_bytes(handle, bsz, seq),
                                       "slot")
            else:            # the kept layers' slots, and a workspace for the intermediates of the layers below `first` (none if first = 0)
                nsaved, nslot, kind = (lib.ov_tower_saved_bytes_from(handle, first, bsz, seq),
                                       lib.ov_tower_forward_saving_from_workspace_bytes(handle, first, bsz, seq), "ws")
            if first < layers:
                saved = pool.take(nsaved, x.device, "saved")
            if nslot:
                slot = pool.take(nslot, x.device, kind)
            with _drop_scope(lib, handle, drop, bsz, seq, pool, x.device):
                if remat:
                    check(lib.ov_tower_forward_checkpointed(handle, first, ptr(xb), ptr(saved), ptr(slot), nslot, bsz, seq, stream_ptr()),
                          "ov_tower_forward_checkpointed")
                else:
                    check(lib.ov_tower_forward_saving_from(handle, first, ptr(xb), ptr(saved), bsz, seq, ptr(slot), nslot, stream_ptr()),
                          "ov_tower_forward_saving_from")
        except BaseException:
            for t in (saved, slot):
                if t is not None:
                    pool.give(t)
            raise
        if slot is not None and (not remat or saved is None or hi < len(transformer.resblocks)):
            pool.give(slot)                   # only the top node under recomputation keeps its slot for the backward
            slot = None
        ctx.tower, ctx.saved, ctx.shape, ctx.pool = tower, saved, (bsz, seq, d), pool      # the backward runs the forward's handle:
        ctx.first, ctx.pairs, ctx.need = first, pairs, (need_x, need_p)                    # its weights and its mask
        ctx.saved_gen = saved._ovhip_gen if saved is not None else None
        ctx.remat, ctx.slot = remat, slot
        ctx.drop = drop                       # the backward and its recompute run under the forward's table
        ctx.x_dtype, ctx.p_dtypes = x.dtype, [p.dtype for p in params]
        return xb.to(x.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        tower = ctx.tower
        lib, handle, layers = tower.lib, tower.handle, tower.layers
        bsz, seq, d = ctx.shape
        if ctx.saved is None or ctx.saved._ovhip_gen != ctx.saved_gen:
            raise _lib.OvhipError("training path: the saved activations of this graph were recycled by a later forward; a second "
                                  "backward over the same graph must come before the next forward of this tower")
        need_x, need_p = ctx.need
        first, pool = ctx.first, ctx.pool
        # frozen pairs: NULL in ov_block_grads, no buffers, no work; with everything trainable every pair is requested
        grads = [[None] * 12 for _ in range(first)]
        grads += [[torch.empty_like(t) if ctx.pairs[i][j // 2] else None for j, t in enumerate(tower.keep[i])] for i in range(first, layers)]
        garr = (_lib.BlockGrads * (layers - first))(*[_lib.BlockGrads(*[ptr(t) for t in g]) for g in grads[first:]])
        dx = grad_out.detach().to(torch.bfloat16).contiguous().clone()
        slot, holds = ctx.slot, ctx.slot is not None
        ctx.slot = None                       # the backward overwrites it: a second backward over this graph recomputes the top block
        ws = None
        try:
            nbytes = lib.ov_tower_backward_partial_workspace_bytes(handle, bsz, seq)
            ws = pool.take(nbytes, dx.device)
            if ctx.remat:
                nslot = lib.ov_tower_slot_bytes(handle, bsz, seq)
                if slot is None:
                    slot = pool.take(nslot, dx.device, "slot")
            with _drop_scope(lib, handle, ctx.drop, bsz, seq, pool, dx.device):
                if ctx.remat:
                    check(lib.ov_tower_backward_checkpointed(handle, first, ptr(ctx.saved), ptr(slot), nslot, int(holds), ptr(dx), garr,
                                                             int(need_x), bsz, seq, ptr(ws), nbytes, stream_ptr()),
                          "ov_tower_backward_checkpointed")
                else:
                    check(lib.ov_tower_backward_partial(handle, first, ptr(ctx.saved), ptr(dx), garr, int(need_x), bsz, seq, ptr(ws),
                                                        nbytes, stream_ptr()), "ov_tower_backward_partial")
        finally:                              # on success and on error alike; ordered on the stream: the next forward's writes come
            for t in (slot, ws, ctx.saved):   # after this backward's reads
                if t is not None:
                    pool.give(t)
        mlp = tower.cfg.mlp                                       # drop the (exactly zero) gradients of the MLP padding
        for gs in grads:
            if gs[8] is not None:
                gs[8], gs[9] = gs[8][:mlp], gs[9][:mlp]
            if gs[10] is not None:
                gs[10] = gs[10][:, :mlp]
        # the frozen half of a mixed pair was computed with its partner and is dropped here
        flat = [g.to(ctx.p_dtypes[12 * i + j]) if g is not None and need_p[12 * i + j] else None
                for i, gs in enumerate(grads) for j, g in enumerate(gs)]
        return (*([None] * ctx.nargs), dx.view(bsz, seq, d).to(ctx.x_dtype) if need_x else None, *flat)


class _PrefixTowerFn(_TowerFn):
    """``_TowerFn`` under the prefix-causal mask: apply(transformer, lo, hi, prefix, x, *params)."""

    NARGS = 4

    @classmethod
    def _split(cls, args):
        return int(args[0]), args[1], args[2:]


class _DropTowerFn(_TowerFn):
    """``_TowerFn`` under a drop-path table (and a prefix-causal mask, or None): apply(transformer, lo, hi, prefix, table, x, *params).
    The table (``DropPathTable`` of the node's blocks) stays on the ctx: the backward, and under recomputation the rebuild of each
    block's intermediates, run the forward's masks."""

    NARGS = 5

    @classmethod
    def _split(cls, args):
        return (None if args[0] is None else int(args[0])), args[2], args[3:]

    @classmethod
    def _drop(cls, args):
        return args[1]


class _LinearFn(torch.autograd.Function):
    """y = x W^T (+ b) on ov_gemm, backward on ov_linear_backward: the light-end projections of the towers (patch projection
    transformer.py:610-612 as a GEMM over patch rows, `@ proj` :645-646, `@ text_projection` model.py:282) -- no aten / hipBLASLt GEMM
    on the training path.  x [M, K] any float dtype, w [N, K]; K and N are zero-padded to the kernels' 64 granule."""

    @staticmethod
    def forward(ctx, x, w, bias):
        lib = _lib.load()
        m, k = x.shape
        n = w.shape[0]
        kp, npad = _round_up(k, 64), _round_up(n, 64)
        xb = torch.zeros(m, kp, dtype=torch.bfloat16, device=x.device)
        xb[:, :k] = x.detach()
        wb = _pack_matrix(w, npad, kp)
        bb = _pack_vec(bias, npad, x.device) if bias is not None else None
        out = torch.empty(m, npad, dtype=torch.bfloat16, device=x.device)
        _gemm_bias(ptr(xb), kp, ptr(wb), kp, ptr(bb), ptr(out), npad, m, npad, kp, stream_ptr())
        ctx.save_for_backward(xb, wb)
        ctx.dims = (m, n, k, kp, npad, bias is not None, x.dtype, w.dtype, bias.dtype if bias is not None else None)
        return out[:, :n].float()

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        xb, wb = ctx.saved_tensors
        m, n, k, kp, npad, has_b, xd, wd, bd = ctx.dims
        dyb = torch.zeros(m, npad, dtype=torch.bfloat16, device=dy.device)
        dyb[:, :n] = dy.detach()
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = torch.empty(m, kp, dtype=torch.bfloat16, device=dy.device) if need_x else None
        dw = torch.empty(npad, kp, dtype=torch.bfloat16, device=dy.device) if need_w else None
        db = torch.empty(npad, dtype=torch.float32, device=dy.device) if has_b else None
        nb = lib.ov_linear_backward_workspace_bytes(m, npad, kp)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=dy.device)
        check(lib.ov_linear_backward(ptr(dyb), npad, ptr(xb), kp, ptr(wb), kp, m, npad, kp, ptr(dx), kp, ptr(dw), kp, ptr(db), ptr(ws), nb,
                                     stream_ptr()), "ov_linear_backward")
        return (dx[:, :k].to(xd) if need_x else None, dw[:n, :k].to(wd) if need_w else None, db[:n].to(bd) if has_b else None)


class _AttnPoolFn(torch.autograd.Function):
    """The pooler's cross-attention core with gradients: out [B n_q, E] = softmax(scale q k_b^T) v_b on ``ov_attn_pool`` (which keeps the
    row log-sum-exp), backward on ``ov_attn_pool_backward``.  q [n_q, E]: the projected queries, shared by every image, so d q is the
    sum over the batch (fixed order, no atomics: bitwise repeatable); kv [B L, 2E]: the K | V projection of the tokens."""

    @staticmethod
    def forward(ctx, q, kv, bsz, seq, heads):
        lib = _lib.load()
        nq, e = q.shape
        hd = e // heads
        qb = q.detach().to(torch.bfloat16).contiguous()
        kvb = kv.detach().to(torch.bfloat16).contiguous()
        out = torch.empty(bsz * nq, e, dtype=torch.bfloat16, device=q.device)
        lse = torch.empty(bsz * heads, _round_up(nq, 32), dtype=torch.float32, device=q.device)
        check(lib.ov_attn_pool(ptr(qb), e, ptr(kvb), 2 * e, ptr(out), e, ptr(lse), bsz, seq, nq, heads, hd, hd ** -0.5, stream_ptr()),
              "ov_attn_pool")
        ctx.save_for_backward(qb, kvb, out, lse)
        ctx.dims = (bsz, seq, nq, heads, hd, q.dtype, kv.dtype)
        return out.float()

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        qb, kvb, out, lse = ctx.saved_tensors
        bsz, seq, nq, heads, hd, qd, kvd = ctx.dims
        e = heads * hd
        dob = dout.detach().to(torch.bfloat16).contiguous()
        dq = torch.empty(nq, e, dtype=torch.float32, device=dout.device)
        dkv = torch.empty(bsz * seq, 2 * e, dtype=torch.bfloat16, device=dout.device)
        nb = lib.ov_attn_pool_backward_workspace_bytes(bsz, seq, nq, heads, hd)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=dout.device)
        check(lib.ov_attn_pool_backward(ptr(qb), e, ptr(kvb), 2 * e, ptr(out), e, ptr(dob), e, ptr(lse), ptr(dq), e, ptr(dkv), 2 * e, bsz, seq,
                                        nq, heads, hd, hd ** -0.5, ptr(ws), nb, stream_ptr()), "ov_attn_pool_backward")
        return (dq.to(qd) if ctx.needs_input_grad[0] else None, dkv.to(kvd) if ctx.needs_input_grad[1] else None, None, None, None)


def attn_pool_forward(pool, x: torch.Tensor) -> torch.Tensor:
    """``model.AttentionalPooler`` with gradients (transformer.py:201-207): x [B, L, context] -> [B, n_queries, d_model] fp32.  ln_k
    and ln_q on ``_LayerNormFn``, the three projections and out_proj on ``_LinearFn``, the attention on ``_AttnPoolFn``."""
    a = pool.attn
    bsz, seq, d = x.shape
    e, nq = a.embed_dim, pool.query.shape[0]
    xk = _LayerNormFn.apply(x, pool.ln_k.weight, pool.ln_k.bias, pool.ln_k.eps)
    qn = _LayerNormFn.apply(pool.query, pool.ln_q.weight, pool.ln_q.bias, pool.ln_q.eps)
    qp = _LinearFn.apply(qn, a.q_weight(), a.in_proj_bias[:e])
    kv = _LinearFn.apply(xk.reshape(bsz * seq, d), a.kv_weight(), a.in_proj_bias[e:])
    o = _AttnPoolFn.apply(qp, kv, bsz, seq, a.num_heads)
    return _LinearFn.apply(o, a.out_proj.weight, a.out_proj.bias).view(bsz, nq, e)


class _LayerNormFn(torch.autograd.Function):
    """LayerNorm (transformer.py:15-30: fp32 statistics) on ov_layernorm / ov_layernorm_backward: ln_post on the pooled rows, ln_final
    on the text tokens."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        lib = _lib.load()
        d = x.shape[-1]
        xb = x.detach().to(torch.bfloat16).contiguous().view(-1, d)
        g, b = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        y = torch.empty(xb.shape, dtype=torch.float32, device=x.device)
        check(lib.ov_layernorm(ptr(xb), _lib.OV_BF16, d, ptr(g), ptr(b), ptr(y), _lib.OV_F32, d, xb.shape[0], d, float(eps), stream_ptr()),
              "ov_layernorm")
        ctx.save_for_backward(xb, g)
        ctx.meta = (x.shape, float(eps), x.dtype, weight.dtype, bias.dtype)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        xb, g = ctx.saved_tensors
        shape, eps, xd, wd, bd = ctx.meta
        rows, d = xb.shape
        dyb = dy.detach().to(torch.bfloat16).contiguous().view(rows, d)
        dx = torch.empty_like(xb)
        dg = torch.empty(d, dtype=torch.float32, device=dy.device)
        db = torch.empty(d, dtype=torch.float32, device=dy.device)
        nb = lib.ov_layernorm_backward_workspace_bytes(rows, d)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=dy.device)
        check(lib.ov_layernorm_backward(ptr(xb), d, ptr(g), ptr(dyb), d, None, 0, ptr(dx), d, ptr(dg), ptr(db), rows, d, eps, ptr(ws), nb,
                                        stream_ptr()), "ov_layernorm_backward")
        return dx.view(shape).to(xd), dg.to(wd), db.to(bd), None


def _patch_tokens_forward(cols, w, cls, pos, keep, gg: int, y, x, st) -> None:
    """The launch form of the image front end on the caller's buffers (no autograd, allocation or host read): y [B K, npad] = cols [B K,
    kp] w^T in bf16 (``_gemm_bias``), then ``x[b, 0] = cls + pos[0]``, ``x[b, 1 + j] = y[b, j] + pos[1 + keep[b, j]]`` in fp32
    (``ov_patch_keep_assemble``) -> x [B, 1 + K, D].  ``_PatchKeepFn`` and ``visualize.FeatureVisualizer.step`` run it."""
    (bsz, seq, d), (npad, kp) = x.shape, w.shape
    _gemm_bias(ptr(cols), kp, ptr(w), kp, None, ptr(y), npad, cols.shape[0], npad, kp, st)
    check(_lib.load().ov_patch_keep_assemble(ptr(y), npad, ptr(cls), ptr(pos), ptr(keep), ptr(x), bsz, seq - 1, gg, d, st), "ov_patch_keep_assemble")


def _patch_tokens_backward(dx, inv, gg: int, dy, w, ws, ws_bytes: int, st, dpos=None, dcls=None, cols=None, dcols=None, dw=None) -> None:
    """Its backward, on the same terms: dx fp32 [B, 1 + K, D] -> ``ov_patch_keep_assemble_backward`` -> dy [B K, npad] bf16 and the
    optional dpos / dcls (fixed-order sums over the batch; 0 for a position no image kept), then ``ov_linear_backward`` -> the optional
    dcols [B K, kp] and dw [npad, kp] (dw from the forward's ``cols``).  Without dy the assembly's backward runs alone."""
    lib, (bsz, seq, d), (npad, kp) = _lib.load(), dx.shape, w.shape
    check(lib.ov_patch_keep_assemble_backward(ptr(dx), ptr(inv), bsz, seq - 1, gg, d, ptr(dpos), ptr(dcls), ptr(dy), npad, st),
          "ov_patch_keep_assemble_backward")
    if dy is not None:
        check(lib.ov_linear_backward(ptr(dy), npad, ptr(cols), kp if cols is not None else 0, ptr(w), kp, dy.shape[0], npad, kp, ptr(dcols), kp,
                                     ptr(dw), kp if dw is not None else 0, None, ptr(ws), ws_bytes, st), "ov_linear_backward")


class _PatchKeepFn(torch.autograd.Function):
    """Patch dropout's front end (transformer.py:610-619 with PatchDropout): the kept patches' conv1 operand rows (``ov_im2col_patches_keep``)
    through ``_patch_tokens_forward`` -> x [B, 1 + K, D].  Backward: ``_patch_tokens_backward`` (its GEMM half only when the image or the
    weight needs a gradient), then ``ov_col2im_patches_keep`` for the image (dropped patches 0).  keep / inv: int32 [B, K] / [B, G] on the device."""

    @staticmethod
    def forward(ctx, image, w, cls, pos, keep, inv, patch):
        lib = _lib.load()
        bsz, _, s, _ = image.shape
        g = s // patch
        nk = keep.shape[1]
        d = w.shape[0]
        k, kp, npad = 3 * patch * patch, _round_up(3 * patch * patch, 64), _round_up(d, 64)
        img = _kernel_input(image.detach())
        st = stream_ptr()
        cols = torch.empty(bsz * nk, kp, dtype=torch.bfloat16, device=image.device)
        check(lib.ov_im2col_patches_keep(ptr(img), _dtype_flag(img), ptr(keep), ptr(cols), bsz, s, patch, nk, kp, st), "ov_im2col_patches_keep")
        wb = _pack_matrix(w, npad, kp)
        y = torch.empty(bsz * nk, npad, dtype=torch.bfloat16, device=image.device)
        cls32, pos32 = cls.detach().float().contiguous(), pos.detach().float().contiguous()
        x = torch.empty(bsz, 1 + nk, d, dtype=torch.float32, device=image.device)
        _patch_tokens_forward(cols, wb, cls32, pos32, keep, g * g, y, x, st)
        ctx.save_for_backward(cols, wb, keep, inv)
        ctx.dims = (bsz, s, patch, g * g, nk, d, k, kp, npad, img.dtype, image.dtype, w.dtype, cls.dtype, pos.dtype)
        return x

    @staticmethod
    def backward(ctx, dx):
        lib = _lib.load()
        cols, wb, keep, inv = ctx.saved_tensors
        bsz, s, patch, gg, nk, d, k, kp, npad, img_dt, xd, wd, cd, pd = ctx.dims
        need_img, need_w, need_cls, need_pos = ctx.needs_input_grad[:4]
        dev = dx.device
        st = stream_ptr()
        m = bsz * nk
        dx = dx.detach().float().contiguous()
        dpos = torch.empty(1 + gg, d, dtype=torch.float32, device=dev) if need_pos else None
        dcls = torch.empty(d, dtype=torch.float32, device=dev) if need_cls else None
        nb, dyb, dcols, dwb, ws = 0, None, None, None, None
        if need_img or need_w:
            dyb = (torch.empty if npad == d else torch.zeros)(m, npad, dtype=torch.bfloat16, device=dev)
            dcols = torch.empty(m, kp, dtype=torch.bfloat16, device=dev) if need_img else None
            dwb = torch.empty(npad, kp, dtype=torch.bfloat16, device=dev) if need_w else None
            nb = lib.ov_linear_backward_workspace_bytes(m, npad, kp)
            ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        _patch_tokens_backward(dx, inv, gg, dyb, wb, ws, nb, st, dpos, dcls, cols, dcols, dwb)
        dimg = None
        if need_img:
            dimg = torch.empty(bsz, 3, s, s, dtype=img_dt, device=dev)
            check(lib.ov_col2im_patches_keep(ptr(dcols), kp, ptr(inv), ptr(dimg), _dtype_flag(dimg), bsz, s, patch, nk, st), "ov_col2im_patches_keep")
            dimg = dimg.to(xd)
        return dimg, dwb[:d, :k].to(wd) if need_w else None, dcls.to(cd) if need_cls else None, dpos.to(pd) if need_pos else None, None, None, None


def patch_keep_tables(model, keep: torch.Tensor, batch: int, device, validate: bool = True):
    """int32 device copies of a keep table [B, K] of patch indices and its inverse map [B, G] (``ov_patch_keep_inverse``).  With
    ``validate`` the device's duplicate / range flag is read back (one host synchronisation) and a bad table raises IndexError."""
    from .model import check_keep, keep_to_device
    v = model.visual
    gg = v.num_patches
    check_keep(keep, batch, gg)
    lib = _lib.load()
    kd = keep_to_device(keep, device)
    inv = torch.empty(batch, gg, dtype=torch.int32, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device) if validate else None
    check(lib.ov_patch_keep_inverse(ptr(kd), ptr(inv), batch, kd.shape[1], gg, ptr(err), stream_ptr()), "ov_patch_keep_inverse")
    if validate and int(err.item()) != 0:
        raise IndexError(f"keep: a patch index is repeated within an image or lies outside [0, {gg})")
    return kd, inv


def _patch_tokens_eager(image, p: int, w, cls, pos) -> torch.Tensor:
    """The eager form of the image front end, every patch: conv1 (transformer.py:610-612, stride = kernel, no bias) as patch rows times W^T
    (F.conv2d's sums as a plain GEMM for autograd: MIOpen's fp32 convolution costs tens of ms per step here), then [cls; y] + pos in fp32
    (:615-617).  Dense training is NOT on the launch form above: its fixed-order dpos / dcls sums differ from torch's broadcast reduction
    and the launch count changes -- new results and speed, for a change of its own that re-records the pinned digests."""
    bsz, _, hh, ww = image.shape
    gh, gw = hh // p, ww // p
    patches = image.reshape(bsz, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(bsz * gh * gw, 3 * p * p)
    x = _LinearFn.apply(patches, w.reshape(w.shape[0], -1), None).view(bsz, gh * gw, -1)
    return torch.cat([cls.float().expand(bsz, 1, -1), x], dim=1) + pos.float()


CHUNK_LAYERS = [max(0, int(os.environ.get("OVHIP_TRAIN_CHUNK_LAYERS", "0") or 0))]   # > 0: towers run as consecutive autograd nodes of that many blocks


def set_backward_chunk_layers(n: int) -> None:
    """Run every tower as consecutive autograd nodes of ``n`` blocks each (0 = one node per tower, the default).  The arithmetic
    is unchanged; what changes is WHEN parameter gradients exist: after each chunk's backward instead of after the whole tower's,
    which is what lets ``FusedAdamW.overlap_gradient_exchange`` start a bucket's all-reduce while earlier blocks are still in
    their backward (the reference leaves this to DistributedDataParallel's bucket hooks)."""
    CHUNK_LAYERS[0] = max(0, int(n))


_OWN = object()


def tower_forward(transformer, x: torch.Tensor, prefix=_OWN, drop: Optional[DropPathTable] = None) -> torch.Tensor:
    """``transformer(x)`` with gradients: x [B, L, D] on the device -> same shape; d x and every block parameter receive grad.
    ``prefix``: the attention mask of every block -- by default the transformer's own ``causal_prefix``; None = unmasked; an int P =
    key j visible to query i iff j < P or j <= i.  It is kept on the autograd node, so the backward uses the forward's value.

    ``drop``: the drop-path table of this forward (``drop_path_table``), used whatever the mode; by default one is drawn when the
    transformer is in training mode with ``drop_path`` > 0.  Each branch of each block then runs on its kept samples only."""
    if prefix is _OWN:
        prefix = getattr(transformer, "causal_prefix", None)
    if not x.is_cuda:
        raise _lib.OvhipError("training path: tensors must live on an MI355X device (no CPU fallback)")
    blocks = list(transformer.resblocks)
    drop = _own_drop(transformer, x.shape[0], drop)
    step = CHUNK_LAYERS[0] if CHUNK_LAYERS[0] > 0 else len(blocks)
    for lo in range(0, len(blocks), step):
        hi = min(len(blocks), lo + step)
        params = [p for blk in blocks[lo:hi] for p in _block_tensors(blk)]
        if drop is not None:
            x = _DropTowerFn.apply(transformer, lo, hi, prefix, drop.slice(lo, hi), x, *params)
        else:
            x = _TowerFn.apply(transformer, lo, hi, x, *params) if prefix is None else _PrefixTowerFn.apply(transformer, lo, hi, prefix, x, *params)
    return x


def encode_image(model, image: torch.Tensor, normalize: bool = True, keep: torch.Tensor = None, output_tokens: bool = False,
                 drop: Optional[DropPathTable] = None):
    """CLIP.encode_image (model.py:265-267) with gradients.  VisionTransformer.forward, transformer.py:609-651: the OpenVision
    configuration (no ln_pre, pool -> ln_post -> proj) and the stock one (ln_pre, ln_post -> 'tok' pool -> proj).

    Patch dropout (transformer.py:619): when the vision tower is in training mode with ``patch_dropout`` p > 0, the kept patches are
    drawn as the reference draws them (``PatchDropout.sample``: CPU default generator) and the tower runs on those 1 + K tokens.
    ``keep`` (integer [B, K], patch indices in [0, G), no repeats within an image) overrides the draw, whatever the mode and p; such
    a table is checked on the device and the flag read back (one host synchronisation), a bad one raises IndexError.

    ``output_tokens``: also return what the reference hands to the caption decoder (vit.py:753,786): the block stack's output without
    the CLS token and BEFORE ln_post, [B, L - 1, width] (the kept patches under patch dropout), with gradients into the tower.

    A tower with ``attentional_pool`` (transformer.py:636-640) pools all 1 + K tokens with ``attn_pool_forward``, applies ln_post to
    the n_q pooled rows and takes 'tok' / 'avg' over them; its ``output_tokens`` are the reference's for that branch,
    ``ln_post(pool(x))[:, 1:]`` [B, n_q - 1, embed_dim].

    ``drop``: the image tower's drop-path table (``tower_forward``)."""
    v = model.visual
    p = v.patch_size[0]
    w = v.conv1.weight
    if image.dim() != 4 or image.shape[1] != 3 or tuple(image.shape[2:]) != tuple(v.image_size):
        raise ValueError(f"expected images [B,3,{v.image_size[0]},{v.image_size[1]}] (the model's size; model.set_input_size changes "
                         f"it), got {tuple(image.shape)}")
    bsz, _, hh, ww = image.shape
    gh, gw = hh // p, ww // p
    explicit = keep is not None
    if explicit:
        from .model import check_keep
        check_keep(keep, bsz, gh * gw)
    if keep is None and v.dropout_active():
        keep = v.patch_dropout.sample(bsz, gh * gw)
    if keep is not None:
        if not image.is_cuda:
            raise _lib.OvhipError("training path: tensors must live on an MI355X device (no CPU fallback)")
        if hh != ww or hh % p:
            raise ValueError(f"expected square images of a multiple of the patch size, got {tuple(image.shape)}")
        kd, inv = patch_keep_tables(model, keep, bsz, image.device, validate=explicit)
        x = _PatchKeepFn.apply(image, w.reshape(w.shape[0], -1), v.class_embedding, v.positional_embedding, kd, inv, p)
    else:
        x = _patch_tokens_eager(image, p, w, v.class_embedding, v.positional_embedding)
    if not isinstance(v.ln_pre, torch.nn.Identity):                # :620, after the patch dropout: on the kept tokens only
        x = _LayerNormFn.apply(x, v.ln_pre.weight, v.ln_pre.bias, v.ln_pre.eps)
    x = tower_forward(v.transformer, x, drop=drop)
    tokens = x[:, 1:]
    if v.attn_pool is not None:                                    # :636-640: pool all tokens, ln_post, then 'tok' / 'avg' over the queries
        xx = _LayerNormFn.apply(attn_pool_forward(v.attn_pool, x), v.ln_post.weight, v.ln_post.bias, v.ln_post.eps)
        pooled, tokens = (xx[:, 1:].mean(dim=1) if v.pool_type == "avg" else xx[:, 0]), xx[:, 1:]
    elif v.final_ln_after_pool:
        pooled = x[:, 1:].mean(dim=1) if v.pool_type == "avg" else x[:, 0]
        pooled = _LayerNormFn.apply(pooled, v.ln_post.weight, v.ln_post.bias, v.ln_post.eps)
    else:
        xx = _LayerNormFn.apply(x, v.ln_post.weight, v.ln_post.bias, v.ln_post.eps)
        pooled = xx[:, 1:].mean(dim=1) if v.pool_type == "avg" else xx[:, 0]
    out = _LinearFn.apply(pooled, v.proj.t(), None)
    out = F.normalize(out, dim=-1) if normalize else out
    return (out, tokens) if output_tokens else out


def encode_text_embeddings(model, x: torch.Tensor, normalize: bool = True, pool_index=None, output_tokens: bool = False,
                           drop: Optional[DropPathTable] = None):
    """The text tower from token EMBEDDINGS x [B, T, width] (before the positional embedding), with gradients to x: the entry of
    ov-gradient-ascent.py:102-127, which feeds `soft_one_hot @ token_embedding.weight` instead of token ids.  `pool_index` (int64 [B])
    selects the pooled position for text_pool_type 'argmax' (ids are not available here).  ``drop``: the text tower's drop-path table
    (``tower_forward``)."""
    x = x.float() + model.positional_embedding.float()[: x.shape[1]]
    x = tower_forward(model.transformer, x, drop=drop)
    tokens = x[:, :-1]             # output_tokens: the stack's output without its last position, before ln_final (text_transformer.py:676-682)
    x = _LayerNormFn.apply(x, model.ln_final.weight, model.ln_final.bias, model.ln_final.eps)
    pool = getattr(model, "text_pool_type", "last")
    if pool == "last":
        pooled = x[:, -1]
    elif pool == "first":
        pooled = x[:, 0]
    elif pool == "argmax":
        if pool_index is None:
            raise _lib.OvhipError("training path: text pool type 'argmax' needs pool_index when embeddings are given")
        pooled = x[torch.arange(x.shape[0], device=x.device), pool_index]
    else:
        raise _lib.OvhipError(f"training path: text pool type {pool!r} is not supported")
    out = _LinearFn.apply(pooled, model.text_projection.t(), None)
    out = F.normalize(out, dim=-1) if normalize else out
    return (out, tokens) if output_tokens else out


def encode_text(model, text: torch.Tensor, normalize: bool = True, output_tokens: bool = False, drop: Optional[DropPathTable] = None):
    """CLIP.encode_text (model.py:269-284) with gradients: the tower's own mask (none for OpenVision; causal for a stock open_clip
    config, whose ``CLIP`` sets ``transformer.causal_prefix = 0``), ln_final on all tokens, pool per text_pool_type ('argmax': the row
    of each caption's largest id, ``text.argmax(-1)``, the first of equals as on the inference path).  `text`: int64
    token ids [B, T], or a float [B, T, vocab] matrix of (soft) one-hot rows (ov-gradient-ascent.py:105: `text @ token_embedding.weight`,
    gradients flow to the rows).  ``drop``: the text tower's drop-path table (``tower_forward``); with C caption sets stacked its batch
    is C B."""
    if text.is_floating_point():
        if text.dim() != 3 or text.shape[-1] != model.token_embedding.weight.shape[0]:
            raise ValueError("soft tokens must be [B, T, vocab_size]")
        return encode_text_embeddings(model, text.float() @ model.token_embedding.weight.float(), normalize,
                                      text.argmax(dim=-1).argmax(dim=-1), output_tokens, drop=drop)
    x = F.embedding(text, model.token_embedding.weight.float())
    return encode_text_embeddings(model, x, normalize, text.argmax(dim=-1), output_tokens, drop=drop)


def caption_sets(image: torch.Tensor, text: torch.Tensor) -> int:
    """C for an image batch [B, ...] and a token batch [C B, T]: the caption sets per image, stacked set by set (the reference's
    ``concatenate([labels1, labels2])``, src/main_clip.py:408-411).  Raises unless the text rows are a positive multiple of B."""
    nb, nt = image.shape[0], text.shape[0]
    if nb <= 0 or nt < nb or nt % nb:
        raise ValueError(f"text batch of {nt} rows is not a multiple of the image batch of {nb}: stack C caption sets as [C * B, T]")
    return nt // nb


def _drop_pair(drop, n: int = 2):
    """``drop`` of the model-level entry points: None, or one table (or None) per tower."""
    if drop is None:
        return (None,) * n
    drop = tuple(drop)
    if not 2 <= len(drop) <= n:
        raise ValueError(f"drop must be a pair (image_table, text_table){' or a triple with the decoder table' if n > 2 else ''}")
    return drop + (None,) * (n - len(drop))


def _drop_kw(table) -> dict:
    """The ``drop=`` keyword of a tower-level entry point, passed only when there is a table (as ``keep`` is)."""
    return {} if table is None else {"drop": table}


def clip_forward(model, image: torch.Tensor, text: torch.Tensor, keep: torch.Tensor = None, drop=None) -> Tuple[torch.Tensor, ...]:
    """CLIP.forward (model.py:295-315) with gradients: (image_features, text_features, logit_scale.exp()), and ``logit_bias`` (the
    parameter itself, so its gradient flows) as a fourth element when the model has one (SigLIP).  Patch dropout as in
    ``encode_image`` (drawn when the vision tower is in training mode with p > 0; ``keep`` overrides the draw, as there).

    ``text`` may stack C caption sets per image as [C B, T]: the text tower runs once on all rows and ``text_features`` is [C B, E],
    the input of ``MultiCaptionClipLoss(num_captions=C)``.

    ``drop``: a pair ``(image_table, text_table)`` of drop-path tables (``drop_path_table``; either may be None), used whatever the
    mode; by default each tower in training mode with ``drop_path`` > 0 draws its own (``CLIP.set_drop_path``)."""
    caption_sets(image, text)
    kw = {} if keep is None else {"keep": keep}
    drop_i, drop_t = _drop_pair(drop)
    out = (encode_image(model, image, True, **kw, **_drop_kw(drop_i)), encode_text(model, text, True, **_drop_kw(drop_t)),
           model.logit_scale.exp())
    if getattr(model, "logit_bias", None) is not None:
        return out + (model.logit_bias,)
    return out


def decode(decoder, image_tokens: torch.Tensor, text_tokens: torch.Tensor, drop: Optional[DropPathTable] = None) -> torch.Tensor:
    """``caption.TextDecoder.forward`` with gradients (text_decoder.py:436-576, concat fusion): bias-free projections of both token
    sets (``_LinearFn``), ``[image | text | learnable]`` through the decoder's blocks under the prefix-LM mask with prefix =
    L_image + L_text (``tower_forward``), the last T_out positions through ``decoder_norm`` (``_LayerNormFn``) and the bias-free
    vocabulary head (``_LinearFn``) -> fp32 logits [B, T_out, vocab].  Gradients reach the decoder's parameters and both inputs.
    ``drop``: the decoder stack's drop-path table (``tower_forward``)."""
    bsz, li, _ = image_tokens.shape
    lt = text_tokens.shape[1]
    w = decoder.width
    if image_tokens.shape[-1] != decoder.image_projection.in_features:
        raise ValueError(f"decode: image tokens of width {image_tokens.shape[-1]}, but the decoder was built with image_width="
                         f"{decoder.image_projection.in_features} (a tower with attentional_pool hands over its pooler's tokens, of "
                         f"width embed_dim)")
    xi = _LinearFn.apply(image_tokens.reshape(bsz * li, -1), decoder.image_projection.weight, None).view(bsz, li, w)
    xt = _LinearFn.apply(text_tokens.reshape(bsz * lt, -1), decoder.text_projection.weight, None).view(bsz, lt, w)
    lr = decoder.learnable_tokens.float().unsqueeze(0).expand(bsz, -1, -1)
    x = torch.cat([xi, xt, lr], dim=1)
    x = tower_forward(decoder.transformer, x, prefix=li + lt, drop=drop)
    n = decoder.num_learnable_tokens
    y = _LayerNormFn.apply(x[:, -n:].contiguous(), decoder.decoder_norm.weight, decoder.decoder_norm.bias, decoder.decoder_norm.eps)
    return _LinearFn.apply(y.reshape(bsz * n, w), decoder.head.weight, None).view(bsz, n, -1)


def coca_forward(model, decoder, image: torch.Tensor, text: torch.Tensor, keep: torch.Tensor = None, drop=None):
    """The reference trainer's 'coca' forward (src/main_clip.py:448-465): both towers once, their features for the contrastive loss
    and their tokens through the caption decoder -> (image_features, text_features, logit_scale.exp(), caption_logits).

    OpenVision's recipe carries two captions per image: ``text`` stacks them as [2 B, T] (src/main_clip.py:408-411), the text tower
    runs once on all rows, and the decoder sees the first set's tokens only (src/models/two_towers.py:95-98), so ``labels`` and
    ``mask`` are the first set's:

        img_f, txt_f, scale, cap = training.coca_forward(model, decoder, images, torch.cat([tokens1, tokens2]))
        loss = MultiCaptionClipLoss(2)(img_f, txt_f, scale) + 2 * CaptionLoss()(cap, labels, mask)

    With one caption per image ([B, T] tokens) it is

        img_f, txt_f, scale, cap = training.coca_forward(model, decoder, images, tokens)
        loss = ClipLoss()(img_f, txt_f, scale) + 2 * CaptionLoss()(cap, labels, mask)

    ``keep`` overrides the patch-dropout draw, as in ``encode_image``.  ``drop``: ``(image_table, text_table)`` or ``(image_table,
    text_table, decoder_table)`` of drop-path tables, as in ``clip_forward``."""
    sets = caption_sets(image, text)
    kw = {} if keep is None else {"keep": keep}
    drop_i, drop_t, drop_d = _drop_pair(drop, 3)
    img_f, img_tok = encode_image(model, image, True, output_tokens=True, **kw, **_drop_kw(drop_i))
    txt_f, txt_tok = encode_text(model, text, True, output_tokens=True, **_drop_kw(drop_t))
    if sets > 1:
        txt_tok = txt_tok[:image.shape[0]]
    return img_f, txt_f, model.logit_scale.exp(), decode(decoder, img_tok, txt_tok, **_drop_kw(drop_d))


def accumulated_step(model, batches, loss, decoder=None, caption_targets=None, caption_weight: float = 2.0,
                     check: bool = False) -> torch.Tensor:
    """Forward and backward of ONE training step over A micro-batches whose contrastive loss is the full-batch InfoNCE of all A b
    pairs (times the world size), exactly (``accumulate.ContrastiveAccumulator``): the parameters' ``.grad`` receive the gradient the
    one-batch step would give, at a micro-batch's activation memory.  ``batches``: a sequence of ``(image, text)`` micro-batches of one
    size, text stacked [C b, T]; ``loss``: a ``ClipLoss`` or ``MultiCaptionClipLoss`` (``gather_with_grad=True`` under data
    parallelism).  Returns the step's loss (device scalar, no grad).

      pass 1  every micro-batch through ``clip_forward`` under ``torch.no_grad()``: the tower nodes see no requested gradient and run
              the training path's own operators while keeping nothing, so the features are bitwise those of pass 2;
      close   one forward over the bank of features (one all-gather of the packed rows under data parallelism);
      pass 2  per micro-batch: forward with gradients, the window's loss, ``.backward()``; each graph is freed before the next
              forward.

    ``decoder`` (a ``caption.TextDecoder``): pass 2 runs ``coca_forward`` and adds ``caption_weight * CaptionLoss()(logits, labels_j,
    mask_j) / A`` to window j's loss, ``caption_targets[j] = (labels, mask)``.  Patch dropout and drop path: one draw per micro-batch
    (and tower), made before pass 1 and used by both passes.  Recomputation, frozen parameters and ``lock_image_tower`` work as in a one-batch step.
    ``check=True`` verifies that pass 2 recomputed pass 1's features bitwise (one host synchronisation per micro-batch).

    The optimiser is not touched: call ``FusedAdamW.zero_grad(windows=A)`` before and ``all_reduce_gradients`` / ``step`` after."""
    from .accumulate import ContrastiveAccumulator
    batches = list(batches)
    if not batches:
        raise ValueError("accumulated_step: no micro-batch")
    if decoder is not None and (caption_targets is None or len(caption_targets) != len(batches)):
        raise ValueError("accumulated_step: with a decoder, caption_targets holds one (labels, mask) pair per micro-batch")
    acc = ContrastiveAccumulator(loss)
    v = model.visual
    keeps = [v.patch_dropout.sample(image.shape[0], v.num_patches) if v.dropout_active() else None for image, _ in batches]
    drops = [(_own_drop(v.transformer, image.shape[0], None), _own_drop(model.transformer, text.shape[0], None)) for image, text in batches]
    with torch.no_grad():
        for (image, text), keep, drop in zip(batches, keeps, drops):
            img_f, txt_f = clip_forward(model, image, text, keep=keep, drop=drop)[:2]
            acc.add(img_f, txt_f)
        total = acc.close(model.logit_scale.exp()).clone()
    if decoder is not None:
        from .caption import CaptionLoss
        cap_loss = CaptionLoss()
    for j, ((image, text), keep, drop) in enumerate(zip(batches, keeps, drops)):
        if decoder is None:
            img_f, txt_f, scale = clip_forward(model, image, text, keep=keep, drop=drop)[:3]
            part = acc.window_loss(j, img_f, txt_f, scale, check=check)
        else:
            img_f, txt_f, scale, cap = coca_forward(model, decoder, image, text, keep=keep, drop=drop)
            labels, mask = caption_targets[j]
            cpart = caption_weight * cap_loss(cap, labels, mask) / len(batches)
            total += cpart.detach()
            part = acc.window_loss(j, img_f, txt_f, scale, check=check) + cpart
        part.backward()
        del part, img_f, txt_f, scale
    return total


# --------------------------------------------------------------------------------------------------------------------------
# parameter update + data-parallel gradient exchange: what closes the training step (src/main_clip.py:480-483)
# --------------------------------------------------------------------------------------------------------------------------
def default_decay_filter(name: str, p: torch.Tensor) -> bool:
    """The reference decays '.*/kernel$' only (build_optax.py:259: Dense / Conv kernels): here the 2-D (and conv) weight matrices;
    biases, LayerNorm parameters, class / positional / token embeddings, the attentional pooler's ``query`` (no kernel in that rule; its projection matrices are decayed), the logit scale and the
    logit bias are not decayed."""
    if (name.endswith("token_embedding.weight") or "positional_embedding" in name or name.endswith("class_embedding")
            or name.endswith("learnable_tokens") or name.endswith("attn_pool.query")):
        return False
    return p.dim() >= 2


class FusedAdamW:
    """The reference trainer's update (optax chain of src/optim/build_optax.py:272-278 with config.optax = scale_by_adam(b1=0.9,
    b2=0.95, mu_dtype=bfloat16), decoupled weight decay scaled by the learning rate, optional global-norm clipping) as ONE HIP launch
    per parameter group over flat buffers (``ov_adamw_step``), plus the data-parallel gradient exchange.

    Parameters are re-homed into two flat fp32 buffers (decayed / not decayed) and their ``.grad`` into matching flat gradient
    buffers, so the all-reduce works on a few large contiguous buckets (xGMI rings are per-link bound: few, large messages) and the
    update is two launches.  fp32 parameters only.  After ``step()`` the packed bf16 copies of the model are invalidated (the
    kernel writes parameters without touching ``_version``).  ``model`` may be a list of modules (CLIP + caption decoder)."""

    def __init__(self, model, lr: float, b1: float = 0.9, b2: float = 0.95, eps: float = 1e-8, wd: float = 0.2,
                 clip_norm: float = None, decay_filter=default_decay_filter, bucket_bytes: int = 256 << 20):
        self.model, self.lr, self.b1, self.b2, self.eps, self.wd, self.clip_norm = model, lr, b1, b2, eps, wd, clip_norm
        self.bucket_bytes = int(bucket_bytes)
        self.t = 0
        # `model`: one module, or a list / tuple of modules (the CLIP model and its caption decoder): names get the module's index
        mods = list(model) if isinstance(model, (list, tuple)) else [model]
        named = [((f"{i}." if len(mods) > 1 else "") + n, p) for i, m in enumerate(mods) for n, p in m.named_parameters() if p.requires_grad]
        if not named:
            raise ValueError("no trainable parameters")
        dev = named[0][1].device          # CPU tensors: buffers and the gradient exchange work (gloo tests); step() refuses
        self.groups = []
        for decayed in (True, False):
            ps = [(n, p) for n, p in named if bool(decay_filter(n, p)) == decayed]
            if not ps:
                continue
            if any(p.dtype != torch.float32 for _, p in ps):
                raise _lib.OvhipError("FusedAdamW: fp32 master parameters only")
            offs, total = [], 0
            for _, p in ps:
                offs.append(total)
                total += (p.numel() + 3) // 4 * 4                       # every tensor starts 16-byte aligned
            flat = torch.zeros(total, dtype=torch.float32, device=dev)
            grad = torch.zeros(total, dtype=torch.float32, device=dev)
            with torch.no_grad():
                for (_, p), o in zip(ps, offs):
                    flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
                    p.data = flat[o:o + p.numel()].view(p.shape)
                    p.grad = grad[o:o + p.numel()].view(p.shape)
            self.groups.append(dict(params=ps, offs=offs, flat=flat, grad=grad, wd=wd if decayed else 0.0,
                                    mu=torch.zeros(total, dtype=torch.bfloat16, device=dev),
                                    nu=torch.zeros(total, dtype=torch.float32, device=dev)))
        self._gn = torch.zeros(1, dtype=torch.float32, device=dev)
        self._ws = torch.empty(4096 + 256, dtype=torch.uint8, device=dev)            # >= ov_sumsq_workspace_bytes()
        from .model import invalidate_packed
        invalidate_packed()

    def state_dict(self) -> dict:
        """Step count and the flat moments per group, with the names, shapes and offsets that say what lies where (the reference
        trainer checkpoints its optax state the same way: src/main_clip.py, the `opt` entry of the checkpoint tree)."""
        return dict(t=self.t, hyper=dict(b1=self.b1, b2=self.b2, eps=self.eps),
                    groups=[dict(names=[n for n, _ in g["params"]], shapes=[tuple(p.shape) for _, p in g["params"]], offs=list(g["offs"]),
                                 wd=g["wd"], mu=g["mu"].detach().clone(), nu=g["nu"].detach().clone()) for g in self.groups])

    def load_state_dict(self, sd: dict) -> None:
        """Restore what `state_dict` returned; the parameter layout (names, shapes, offsets per group) must be the one of this model."""
        if len(sd["groups"]) != len(self.groups):
            raise ValueError(f"optimizer state has {len(sd['groups'])} groups, this optimizer {len(self.groups)}")
        for g, s in zip(self.groups, sd["groups"]):
            mine = ([n for n, _ in g["params"]], [tuple(p.shape) for _, p in g["params"]], list(g["offs"]))
            if (list(s["names"]), [tuple(x) for x in s["shapes"]], list(s["offs"])) != mine:
                raise ValueError("optimizer state was saved for a different parameter layout")
        for g, s in zip(self.groups, sd["groups"]):
            g["mu"].copy_(s["mu"].to(g["mu"].device, torch.bfloat16))
            g["nu"].copy_(s["nu"].to(g["nu"].device, torch.float32))
        self.t = int(sd["t"])

    def zero_grad(self, windows: int = 1) -> None:
        """Zero the flat gradient buffers; ``.grad`` stays a view of them (set_to_none would detach the views).

        ``windows``: the number of backward passes that accumulate into the buffers before the exchange (gradient accumulation:
        ``accumulated_step`` over A micro-batches runs A backwards, so call ``zero_grad(windows=A)`` before it).  After
        ``overlap_gradient_exchange`` each bucket then waits for its parameters' gradients of every window and starts with the last
        window's, instead of sending the first window's partial sums.  1 is one backward per step, as before."""
        if int(windows) < 1:
            raise ValueError("windows must be at least 1")
        for g in self.groups:
            g["grad"].zero_()
            for (_, p), o in zip(g["params"], g["offs"]):
                want = g["grad"][o:o + p.numel()]
                if p.grad is None or p.grad.data_ptr() != want.data_ptr():
                    p.grad = want.view(p.shape)
        self._rearm(int(windows))

    def _collect(self) -> None:
        """A ``.grad`` that autograd replaced instead of accumulating in place is copied back into its flat slot; the slot of a
        parameter whose ``.grad`` is None (set_to_none by someone else's zero_grad) is zeroed, so no stale gradient is applied."""
        for g in self.groups:
            for (_, p), o in zip(g["params"], g["offs"]):
                want = g["grad"][o:o + p.numel()]
                if p.grad is None:                                   # model.zero_grad(set_to_none=True): no gradient this step,
                    want.zero_()                                     # not last step's values
                    p.grad = want.view(p.shape)
                elif p.grad.data_ptr() != want.data_ptr():
                    want.copy_(p.grad.detach().reshape(-1).float())
                    p.grad = want.view(p.shape)

    def buckets(self):
        """The flat gradient buffers cut into contiguous chunks of at most ``bucket_bytes``."""
        per = max(1, self.bucket_bytes // 4)
        for g in self.groups:
            n = g["grad"].numel()
            for s in range(0, n, per):
                yield g["grad"][s:min(n, s + per)]

    def overlap_gradient_exchange(self, world_size: int, group=None, always_collective: bool = False) -> None:
        """Start each bucket's SUM all-reduce from autograd, as soon as the last parameter gradient that lies in the bucket has been
        accumulated (post-accumulate-grad hooks), instead of after the whole backward -- DistributedDataParallel's bucket overlap
        (the reference trainer: src/main_clip.py wraps the model the same way) on the flat buffers of this optimiser.  With
        ``set_backward_chunk_layers(n)`` the towers' gradients arrive chunk by chunk, so the exchange of the later blocks' buckets
        runs under the backward of the earlier ones.  ``all_reduce_gradients`` then only launches what is left and waits.  Call
        ``zero_grad()`` (this class's) before every backward: it re-arms the buckets.  ``always_collective`` issues the collectives
        in a world of one rank as well (exercises the RCCL calls on a single GPU)."""
        for h in getattr(self, "_ov_hooks", []):                # a second call (new bucket size, new group) replaces the hooks:
            h.remove()                                          # two hooks per parameter would arm the buckets at half the gradients
        self._ov_hooks = []
        self._ov = dict(world=int(world_size), group=group, works=[], pending=[], launched=[], force=bool(always_collective))
        self._ov_buckets = []                                   # (group index, start, stop)
        per = max(1, self.bucket_bytes // 4)
        for gi, g in enumerate(self.groups):
            n = g["grad"].numel()
            self._ov_buckets += [(gi, s, min(n, s + per)) for s in range(0, n, per)]
        self._ov_members = [[] for _ in self._ov_buckets]       # parameters overlapping each bucket
        for gi, g in enumerate(self.groups):
            for pi, ((_, p), o) in enumerate(zip(g["params"], g["offs"])):
                mine = [bi for bi, (bg, s, e) in enumerate(self._ov_buckets) if bg == gi and s < o + p.numel() and o < e]
                for bi in mine:
                    self._ov_members[bi].append((gi, pi))
                self._ov_hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(gi, pi, o, mine)))
        self._rearm()

    def _rearm(self, windows: int = 1) -> None:
        ov = getattr(self, "_ov", None)
        if ov is not None:
            ov["works"], ov["launched"] = [], [False] * len(self._ov_buckets)
            ov["pending"] = [len(m) * windows for m in self._ov_members]      # every member's gradient lands once per window

    def _launch_bucket(self, bi: int) -> None:
        import torch.distributed as dist
        ov = self._ov
        gi, s, e = self._ov_buckets[bi]
        ov["launched"][bi] = True
        if ov["world"] > 1 or ov["force"]:             # force: issue the collective in a world of one rank too (RCCL path test)
            ov["works"].append(dist.all_reduce(self.groups[gi]["grad"][s:e], op=dist.ReduceOp.SUM, group=ov["group"], async_op=True))

    def _make_hook(self, gi: int, pi: int, off: int, buckets):
        def hook(p):
            want = self.groups[gi]["grad"][off:off + p.numel()]
            if p.grad is not None and p.grad.data_ptr() != want.data_ptr():      # autograd replaced the view: fold it back first
                want.copy_(p.grad.detach().reshape(-1).float())
                p.grad = want.view(p.shape)
            ov = self._ov
            for bi in buckets:
                ov["pending"][bi] -= 1
                if ov["pending"][bi] == 0 and not ov["launched"][bi]:
                    self._launch_bucket(bi)
        return hook

    def all_reduce_gradients(self, world_size: int, group=None) -> float:
        """SUM all-reduce of every bucket (RCCL when the backend is 'nccl'), all issued before any is waited for; returns the factor
        (1 / world_size) that ``step(grad_scale=...)`` folds into the update instead of a separate averaging pass.  After
        ``overlap_gradient_exchange`` most buckets are already in flight: the rest (parameters that received no gradient) is
        launched here, then everything is waited for."""
        import torch.distributed as dist
        ov = getattr(self, "_ov", None)
        if ov is not None:
            self._collect()
            for bi in range(len(self._ov_buckets)):
                if not ov["launched"][bi]:
                    self._launch_bucket(bi)
            for w in ov["works"]:
                w.wait()
            ov["works"] = []
            return 1.0 / ov["world"]
        self._collect()
        if world_size > 1:
            works = [dist.all_reduce(b, op=dist.ReduceOp.SUM, group=group, async_op=True) for b in self.buckets()]
            for w in works:
                w.wait()
        return 1.0 / world_size

    def step(self, lr: float = None, grad_scale: float = 1.0) -> None:
        """One update at learning rate ``lr`` (default: the constructor's; the caller evaluates its schedule on the host)."""
        if self._gn.device.type != "cuda":
            raise _lib.OvhipError("FusedAdamW.step: parameters must live on an MI355X device (no CPU fallback)")
        lib = _lib.load()
        if self._ws.numel() < lib.ov_sumsq_workspace_bytes():
            self._ws = torch.empty(lib.ov_sumsq_workspace_bytes() + 256, dtype=torch.uint8, device=self._gn.device)
        self._collect()
        self.t += 1
        lr = self.lr if lr is None else lr
        gn = None
        if self.clip_norm is not None:
            for i, g in enumerate(self.groups):
                check(lib.ov_sumsq(ptr(g["grad"]), g["grad"].numel(), ptr(self._gn), int(i > 0), ptr(self._ws), self._ws.numel(),
                                   stream_ptr()), "ov_sumsq")
            gn = self._gn
        for g in self.groups:
            check(lib.ov_adamw_step(ptr(g["flat"]), ptr(g["grad"]), ptr(g["mu"]), ptr(g["nu"]), g["flat"].numel(), float(lr), self.b1,
                                    self.b2, self.eps, float(g["wd"]), self.t, float(grad_scale), ptr(gn) if gn is not None else None,
                                    float(self.clip_norm or 0.0), stream_ptr()), "ov_adamw_step")
        from .model import invalidate_packed
        invalidate_packed()
