"""MI355X-native counterpart of ``open_clip.loss.ClipLoss`` (reference ``src/convert_upload/open_clip/loss.py:19-131``).

Data-parallel InfoNCE: each rank holds ``[b, E]`` L2-normalised image and text embeddings; ONE RCCL all-gather of
the packed ``[b, 2E]`` buffer (``torch.distributed`` backend "nccl" == RCCL over xGMI) yields the rank-ordered global
sets (loss.py:52-61), then the fused HIP kernel computes the local ``[b, N]`` logit strips both ways with labels
``i + b*rank`` (loss.py:93-94,108-110) without materialising them.

Gradients: when a feature tensor or ``logit_scale`` requires grad, the loss is an autograd node whose backward is the
HIP kernel behind ``ov_clip_loss_backward`` (d loss / d features and d loss / d logit_scale); ``openvision_amd.training``
carries the gradient on through the towers.  The gathered-side terms are routed as
``gather_features`` does (loss.py:19-63): own chunk only, or summed over ranks (reduce-scatter) with ``gather_with_grad``.
``use_horovod`` is rejected (RCCL via torch.distributed is the only transport here).

``MultiCaptionClipLoss`` is the InfoNCE OpenVision trains with: C caption sets per image (src/losses/common.py:120-189, C = 2), the
mean over the sets of ``ClipLoss(image, text_c)`` in one fused forward and backward (``ov_clip_loss_multi*``) on one packed gather.

``DistillClipLoss`` (loss.py:180-216) adds the cross entropy under a frozen teacher's softmax to ``ClipLoss``: two outputs from one fused
forward and backward (``ov_distill_loss*``) on one packed gather of the student's and the teacher's rows.

``SigLipLoss`` (loss.py:307-414) is the pairwise sigmoid objective on the same transport: one all-gather of the text features,
one fused strip kernel (``ov_siglip_loss``), and in the backward the gathered side summed over ranks.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.distributed as dist
from torch import nn

from . import _lib
from ._lib import ptr, stream_ptr, check


_COMM_LOG = None      # diagnostics (bench.py --gpus N): a list that gather_features appends one (start, end) pair per collective to


def record_comm(log) -> None:
    """Diagnostics: pass a list to have every all-gather of gather_features bracketed by a pair of timing marks appended to it --
    ``torch.cuda.Event``s recorded on the current stream for device tensors (the collective is stream-ordered: the current stream waits
    for it), ``time.perf_counter()`` floats on the CPU (gloo rehearsal).  ``None`` turns it off.  Nothing is synchronised here."""
    global _COMM_LOG
    _COMM_LOG = log


def gather_features(image_features: torch.Tensor, text_features: torch.Tensor, local_loss: bool = False,
                    gather_with_grad: bool = False, rank: int = 0, world_size: int = 1, use_horovod: bool = False,
                    group=None, force: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """loss.py:19-63.  One all_gather_into_tensor of the packed [b, 2E] buffer instead of two list gathers;
    the result is identical: rows in rank order (torch.cat(gathered, dim=0), loss.py:60-61)."""
    if use_horovod:
        raise NotImplementedError("horovod transport is not supported; use torch.distributed (RCCL)")
    if world_size == 1 and not force:          # force: run the collective anyway (tests drive the RCCL path in a world of one)
        return image_features, text_features
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("world_size > 1 needs an initialised torch.distributed process group (caller owns init)")
    b, e = image_features.shape
    packed = torch.cat([image_features.detach().float(), text_features.detach().float()], dim=1).contiguous()
    out = _all_gather_rows(packed, world_size, group)
    return out[:, :e].contiguous(), out[:, e:].contiguous()


def _all_gather_rows(x: torch.Tensor, world_size: int, group=None) -> torch.Tensor:
    """[b, C] on every rank -> [world_size * b, C] in rank order: one all_gather_into_tensor, bracketed for record_comm."""
    out = torch.empty(world_size * x.shape[0], x.shape[1], dtype=x.dtype, device=x.device)
    if _COMM_LOG is None:
        dist.all_gather_into_tensor(out, x, group=group)
    elif x.is_cuda:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dist.all_gather_into_tensor(out, x, group=group)
        e1.record()
        _COMM_LOG.append((e0, e1))
    else:
        import time
        t0 = time.perf_counter()
        dist.all_gather_into_tensor(out, x, group=group)
        _COMM_LOG.append((t0, time.perf_counter()))
    return out


class ClipLoss(nn.Module):
    """Same constructor and call signature as the reference (loss.py:68-83,120-131)."""

    def __init__(self, local_loss: bool = False, gather_with_grad: bool = False, cache_labels: bool = False,
                 rank: int = 0, world_size: int = 1, use_horovod: bool = False, group=None):
        super().__init__()
        self.group = group          # process group of the gather / reduce-scatter (None = the default group, as the reference)
        if use_horovod:
            raise NotImplementedError("horovod transport is not supported; use torch.distributed (RCCL)")
        self.local_loss, self.gather_with_grad, self.cache_labels = local_loss, gather_with_grad, cache_labels
        self.rank, self.world_size, self.use_horovod = rank, world_size, use_horovod
        self.always_collective = False   # tests only: take the world_size > 1 path (gather / reduce-scatter) in a world of one rank
        self._ws: Optional[torch.Tensor] = None
        self.last_terms: Optional[torch.Tensor] = None     # [4, b]: lse_img, diag_img, lse_txt, diag_txt

    @staticmethod
    def _device_scale(logit_scale, device) -> torch.Tensor:
        """The logit multiplier as a 1-element fp32 DEVICE tensor.  It never visits the host (ovhip.h ABI 2): `float(logit_scale)`
        would drain the stream after both towers before the loss could be enqueued."""
        if isinstance(logit_scale, torch.Tensor):
            if not logit_scale.is_cuda:
                return logit_scale.detach().float().reshape(1).to(device, non_blocking=True)
            return logit_scale.detach().float().reshape(1)
        return torch.full((1,), float(logit_scale), dtype=torch.float32, device=device)

    def _loss_strips(self, img, txt, all_img, all_txt, scale: torch.Tensor, label_offset: int) -> torch.Tensor:
        if not img.is_cuda:
            raise _lib.OvhipError("ClipLoss: features must live on an MI355X device (no CPU fallback)")
        lib = _lib.load()
        img, txt = img.detach().float().contiguous(), txt.detach().float().contiguous()
        all_img, all_txt = all_img.detach().float().contiguous(), all_txt.detach().float().contiguous()
        b, e = img.shape
        n = all_img.shape[0]
        nbytes = lib.ov_clip_loss_workspace_bytes(b, n)
        if self._ws is None or self._ws.device != img.device or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=img.device)
        out = torch.empty(1, dtype=torch.float32, device=img.device)
        terms = torch.empty(4, b, dtype=torch.float32, device=img.device)
        check(lib.ov_clip_loss(ptr(img), ptr(txt), ptr(all_img), ptr(all_txt), b, n, e, ptr(scale), int(label_offset),
                               ptr(out), ptr(terms), ptr(self._ws), nbytes, stream_ptr()), "ov_clip_loss")
        self.last_terms = terms
        return out[0]

    def forward(self, image_features, text_features, logit_scale, output_dict: bool = False):
        needs_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                     for t in (image_features, text_features, logit_scale))
        if needs_grad:
            if not isinstance(logit_scale, torch.Tensor):
                logit_scale = torch.tensor(float(logit_scale), device=image_features.device)
            loss = _ClipLossFn.apply(self, image_features, text_features, logit_scale)
            return {"contrastive_loss": loss} if output_dict else loss
        if not image_features.is_cuda:
            raise _lib.OvhipError("ClipLoss: features must live on an MI355X device (no CPU fallback)")
        scale = self._device_scale(logit_scale, image_features.device)
        if self.world_size > 1 or self.always_collective:
            all_img, all_txt = gather_features(image_features, text_features, self.local_loss, self.gather_with_grad,
                                               self.rank, self.world_size, self.use_horovod, self.group, self.always_collective)
            if self.local_loss:
                loss = self._loss_strips(image_features, text_features, all_img, all_txt, scale,
                                         image_features.shape[0] * self.rank)
            else:   # global [N,N] logits on every rank (loss.py:111-113): the strips of the full set
                loss = self._loss_strips(all_img, all_txt, all_img, all_txt, scale, 0)
        else:
            loss = self._loss_strips(image_features, text_features, image_features, text_features, scale, 0)
        return {"contrastive_loss": loss} if output_dict else loss


def _sum_over_ranks_own_chunk(full: torch.Tensor, b: int, rank: int, group=None) -> torch.Tensor:
    """Backward of ``torch.distributed.nn.all_gather`` (loss.py:49-50): every rank's [N, 2E] gathered-side gradient summed,
    this rank keeps rows [rank*b, (rank+1)*b).  One reduce-scatter on RCCL; gloo has none, so all-reduce + slice there."""
    if dist.get_backend(group) == "nccl":
        out = torch.empty(b, full.shape[1], dtype=full.dtype, device=full.device)
        dist.reduce_scatter_tensor(out, full.contiguous(), group=group)
        return out
    full = full.contiguous()
    dist.all_reduce(full, group=group)
    return full[rank * b:(rank + 1) * b]


class _ClipLossFn(torch.autograd.Function):
    """ClipLoss as an autograd node.  forward = the fused strip kernel; backward = ov_clip_loss_backward plus the routing of
    the gathered-side gradient that the reference gets from autograd through gather_features (loss.py:19-63)."""

    @staticmethod
    def forward(ctx, mod: "ClipLoss", image_features, text_features, logit_scale):
        ws, rank = mod.world_size, mod.rank
        img, txt = image_features.detach().float().contiguous(), text_features.detach().float().contiguous()
        b = img.shape[0]
        multi = ws > 1 or mod.always_collective
        if multi:
            all_img, all_txt = gather_features(img, txt, mod.local_loss, mod.gather_with_grad, rank, ws, mod.use_horovod, mod.group,
                                               mod.always_collective)
        else:
            all_img, all_txt = img, txt
        if multi and not mod.local_loss:
            x_img, x_txt, off = all_img, all_txt, 0          # every rank evaluates the global loss (loss.py:111-113)
        else:
            x_img, x_txt, off = img, txt, b * rank
        scale = mod._device_scale(logit_scale, img.device)
        loss = mod._loss_strips(x_img, x_txt, all_img, all_txt, scale, off)
        ctx.mod, ctx.off, ctx.b, ctx.multi = mod, off, b, multi
        ctx.in_dtypes = (image_features.dtype, text_features.dtype, logit_scale.dtype)
        ctx.save_for_backward(x_img, x_txt, all_img, all_txt, mod.last_terms, scale)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        mod: "ClipLoss" = ctx.mod
        x_img, x_txt, all_img, all_txt, terms, scale = ctx.saved_tensors
        lib = _lib.load()
        ws, rank, b = mod.world_size, mod.rank, ctx.b
        bx, e = x_img.shape
        n = all_img.shape[0]
        # the gathered side carries gradient when it IS the local tensor (world_size 1), when the own chunk was put back
        # (not local_loss, loss.py:57-59) or when the gather itself is differentiable (gather_with_grad)
        single = not ctx.multi                      # world of one without the collectives: both sides are the same tensors
        gathered_grad = single or not mod.local_loss or mod.gather_with_grad
        d_img, d_txt = torch.empty_like(x_img), torch.empty_like(x_txt)
        d_all = torch.empty(2, n, e, dtype=torch.float32, device=x_img.device) if gathered_grad else None
        d_scale = torch.empty(1, dtype=torch.float32, device=x_img.device)
        grad = grad_out.detach().float().reshape(1).contiguous()        # device scalar: no host round trip
        nbytes = lib.ov_clip_loss_backward_workspace_bytes(bx, n)
        wsb = torch.empty(nbytes + 256, dtype=torch.uint8, device=x_img.device)
        check(lib.ov_clip_loss_backward(ptr(x_img), ptr(x_txt), ptr(all_img), ptr(all_txt), bx, n, e, ptr(scale), ctx.off, ptr(terms),
                                        ptr(grad), ptr(d_img), ptr(d_txt), ptr(d_all[0]) if gathered_grad else None,
                                        ptr(d_all[1]) if gathered_grad else None, ptr(d_scale), ptr(wsb), nbytes, stream_ptr()),
              "ov_clip_loss_backward")
        if single:
            g_img, g_txt = d_img + d_all[0], d_txt + d_all[1]
        elif mod.local_loss:
            g_img, g_txt = d_img, d_txt
            if mod.gather_with_grad:
                own = _sum_over_ranks_own_chunk(torch.cat([d_all[0], d_all[1]], dim=1), b, rank, mod.group)
                g_img, g_txt = g_img + own[:, :e], g_txt + own[:, e:]
        else:
            tot = torch.cat([d_img + d_all[0], d_txt + d_all[1]], dim=1)          # [N, 2E]: both sides are the global set
            own = _sum_over_ranks_own_chunk(tot, b, rank, mod.group) if mod.gather_with_grad else tot[rank * b:(rank + 1) * b]
            g_img, g_txt = own[:, :e], own[:, e:]
        dt_i, dt_t, dt_s = ctx.in_dtypes
        return None, g_img.to(dt_i), g_txt.to(dt_t), d_scale[0].to(dt_s)


def pack_caption_features(image_features: torch.Tensor, text_features: torch.Tensor, num_captions: int) -> torch.Tensor:
    """[b, E] image rows and the stacked [C b, E] text rows (set c in rows c b ...) -> one [b, (1 + C) E] buffer: the image in
    columns 0 ... E, set c in columns (1 + c) E ...  The layout ``ov_clip_loss_multi`` reads in place after the all-gather."""
    b = image_features.shape[0]
    return torch.cat([image_features] + [text_features[c * b:(c + 1) * b] for c in range(num_captions)], dim=1)


def unpack_caption_features(packed: torch.Tensor, num_captions: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inverse of ``pack_caption_features`` on [n, (1 + C) E] rows: ([n, E] image rows, [C n, E] stacked text rows)."""
    e = packed.shape[1] // (1 + num_captions)
    return packed[:, :e], torch.cat([packed[:, (1 + c) * e:(2 + c) * e] for c in range(num_captions)], dim=0)


def gather_caption_features(image_features: torch.Tensor, text_features: torch.Tensor, num_captions: int, world_size: int,
                            group=None) -> torch.Tensor:
    """ONE all_gather_into_tensor of the packed rows -> [world_size * b, (1 + C) E] in rank order (seen by ``record_comm``)."""
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("world_size > 1 needs an initialised torch.distributed process group (caller owns init)")
    packed = pack_caption_features(image_features.detach().float(), text_features.detach().float(), num_captions).contiguous()
    return _all_gather_rows(packed, world_size, group)


def route_packed_gradient(full: torch.Tensor, b: int, rank: int, gather_with_grad: bool, group=None) -> torch.Tensor:
    """What reaches this rank's own features from a packed [N, (1 + C) E] gradient of the gathered rows: with ``gather_with_grad``
    the sum over ranks of rows [rank b, (rank + 1) b) (the backward of the differentiable all-gather: one reduce-scatter), else
    this rank's own rows of its own gradient (the chunk put back into the detached gather).  Works on CPU tensors over gloo."""
    if gather_with_grad:
        return _sum_over_ranks_own_chunk(full, b, rank, group)
    return full[rank * b:(rank + 1) * b]


class MultiCaptionClipLoss(nn.Module):
    """InfoNCE with ``num_captions`` caption sets per image: what OpenVision trains with (``bidirectional_contrastive_loss``,
    src/losses/common.py:120-189, two sets, ``local_loss=True``).  ``text_features`` holds the sets stacked ``[C b, E]`` (set c in
    rows ``c b ...``, the reference's ``ztxt[:half] / ztxt[half:]``); the loss is the mean over the sets of ``ClipLoss(image, text_c)``,
    computed by one fused forward and one backward (``ov_clip_loss_multi*``): one all-gather of the packed ``[b, (1 + C) E]`` rows
    read in place, the image-side gradients accumulated over the sets inside the kernel, and under ``gather_with_grad`` one
    reduce-scatter of the packed gathered-side gradient.  Constructor as ``ClipLoss``, plus ``num_captions`` in front; the
    reference's ``pmean`` over ranks is left to the gradient averaging, as in ``ClipLoss``."""

    def __init__(self, num_captions: int = 2, local_loss: bool = False, gather_with_grad: bool = False, cache_labels: bool = False,
                 rank: int = 0, world_size: int = 1, use_horovod: bool = False, group=None):
        super().__init__()
        if use_horovod:
            raise NotImplementedError("horovod transport is not supported; use torch.distributed (RCCL)")
        if not 1 <= int(num_captions) <= 4:
            raise ValueError("num_captions must be 1 ... 4")
        self.num_captions = int(num_captions)
        self.group = group
        self.local_loss, self.gather_with_grad, self.cache_labels = local_loss, gather_with_grad, cache_labels
        self.rank, self.world_size, self.use_horovod = rank, world_size, use_horovod
        self.always_collective = False   # tests only: take the world_size > 1 path (gather / reduce-scatter) in a world of one rank
        self._ws: Optional[torch.Tensor] = None
        self.last_terms: Optional[torch.Tensor] = None     # [4 C, b]: per set lse_img, diag_img, lse_txt, diag_txt

    def _operands(self, img: torch.Tensor, txt: torch.Tensor):
        """(x_img, x_txt, gathered operand, its image / text views, ld, set_stride, label offset) for this rank."""
        c, b, e = self.num_captions, img.shape[0], img.shape[1]
        if not (self.world_size > 1 or self.always_collective):
            return img, txt, img, txt, e, b * e, 0
        packed = gather_caption_features(img, txt, c, self.world_size, self.group)
        if self.local_loss:
            x_img, x_txt, off = img, txt, b * self.rank
        else:                       # the global loss on every rank (loss.py:111-113): the local rows are the gathered rows
            x_img, x_txt = (t.contiguous() for t in unpack_caption_features(packed, c))
            off = 0
        return x_img, x_txt, packed, packed[:, e:], (1 + c) * e, e, off

    def _loss_strips(self, x_img, x_txt, all_img, all_txt, ld: int, set_stride: int, scale: torch.Tensor, off: int) -> torch.Tensor:
        lib = _lib.load()
        b, e = x_img.shape
        n = all_img.shape[0]
        nbytes = lib.ov_clip_loss_multi_workspace_bytes(b, n, self.num_captions)
        if self._ws is None or self._ws.device != x_img.device or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=x_img.device)
        out = torch.empty(1, dtype=torch.float32, device=x_img.device)
        terms = torch.empty(4 * self.num_captions, b, dtype=torch.float32, device=x_img.device)
        check(lib.ov_clip_loss_multi(ptr(x_img), ptr(x_txt), ptr(all_img), ptr(all_txt), ld, set_stride, b, n, e, self.num_captions,
                                     ptr(scale), int(off), ptr(out), ptr(terms), ptr(self._ws), nbytes, stream_ptr()),
              "ov_clip_loss_multi")
        self.last_terms = terms
        return out[0]

    def _check(self, image_features, text_features):
        if image_features.dim() != 2 or text_features.dim() != 2 or image_features.shape[1] != text_features.shape[1] \
                or text_features.shape[0] != self.num_captions * image_features.shape[0]:
            raise ValueError(f"MultiCaptionClipLoss: text_features must be [{self.num_captions} * b, E] for image_features [b, E], "
                             f"got {tuple(text_features.shape)} for {tuple(image_features.shape)}")
        if not (image_features.is_cuda and text_features.is_cuda):
            raise _lib.OvhipError("MultiCaptionClipLoss: features must live on an MI355X device (no CPU fallback)")

    def forward(self, image_features, text_features, logit_scale, output_dict: bool = False):
        self._check(image_features, text_features)
        needs_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                     for t in (image_features, text_features, logit_scale))
        if needs_grad:
            if not isinstance(logit_scale, torch.Tensor):
                logit_scale = torch.tensor(float(logit_scale), device=image_features.device)
            loss = _MultiCaptionClipLossFn.apply(self, image_features, text_features, logit_scale)
        else:
            img, txt = image_features.detach().float().contiguous(), text_features.detach().float().contiguous()
            scale = ClipLoss._device_scale(logit_scale, img.device)
            x_img, x_txt, all_img, all_txt, ld, ss, off = self._operands(img, txt)
            loss = self._loss_strips(x_img, x_txt, all_img, all_txt, ld, ss, scale, off)
        return {"contrastive_loss": loss} if output_dict else loss


class _MultiCaptionClipLossFn(torch.autograd.Function):
    """MultiCaptionClipLoss as an autograd node.  forward = ov_clip_loss_multi on the packed gather; backward =
    ov_clip_loss_multi_backward, the gathered side written as one packed [N, (1 + C) E] gradient and routed as ``_ClipLossFn``
    routes its two halves (own chunk, or one reduce-scatter with gather_with_grad)."""

    @staticmethod
    def forward(ctx, mod: "MultiCaptionClipLoss", image_features, text_features, logit_scale):
        img, txt = image_features.detach().float().contiguous(), text_features.detach().float().contiguous()
        scale = ClipLoss._device_scale(logit_scale, img.device)
        x_img, x_txt, all_img, all_txt, ld, ss, off = mod._operands(img, txt)
        loss = mod._loss_strips(x_img, x_txt, all_img, all_txt, ld, ss, scale, off)
        ctx.mod, ctx.off, ctx.b, ctx.lay = mod, off, img.shape[0], (ld, ss)
        ctx.multi = mod.world_size > 1 or mod.always_collective
        ctx.in_dtypes = (image_features.dtype, text_features.dtype, logit_scale.dtype)
        ctx.save_for_backward(x_img, x_txt, all_img, all_txt, mod.last_terms, scale)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        mod: "MultiCaptionClipLoss" = ctx.mod
        x_img, x_txt, all_img, all_txt, terms, scale = ctx.saved_tensors
        lib = _lib.load()
        c, rank, b = mod.num_captions, mod.rank, ctx.b
        bx, e = x_img.shape
        n = all_img.shape[0]
        ld, ss = ctx.lay
        single = not ctx.multi                      # world of one without the collectives: both sides are the same tensors
        gathered_grad = single or not mod.local_loss or mod.gather_with_grad
        dev = x_img.device
        d_img, d_txt = torch.empty_like(x_img), torch.empty_like(x_txt)
        d_scale = torch.empty(1, dtype=torch.float32, device=dev)
        if not gathered_grad:
            d_all, p_ai, p_at, ldg, gss = None, None, None, 0, 0
        elif single:                                # laid out as the features themselves: [b, E] and [C b, E]
            d_all = torch.empty((1 + c) * n, e, dtype=torch.float32, device=dev)
            p_ai, p_at, ldg, gss = ptr(d_all), ptr(d_all[n:]), e, n * e
        else:                                       # packed as the gather: [N, (1 + C) E]
            d_all = torch.empty(n, (1 + c) * e, dtype=torch.float32, device=dev)
            p_ai, p_at, ldg, gss = ptr(d_all), ptr(d_all[:, e:]), (1 + c) * e, e
        grad = grad_out.detach().float().reshape(1).contiguous()        # device scalar: no host round trip
        nbytes = lib.ov_clip_loss_multi_backward_workspace_bytes(bx, n, c)
        wsb = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        check(lib.ov_clip_loss_multi_backward(ptr(x_img), ptr(x_txt), ptr(all_img), ptr(all_txt), ld, ss, bx, n, e, c, ptr(scale),
                                              ctx.off, ptr(terms), ptr(grad), ptr(d_img), ptr(d_txt), p_ai, p_at, ldg, gss,
                                              ptr(d_scale), ptr(wsb), nbytes, stream_ptr()), "ov_clip_loss_multi_backward")
        if single:
            g_img, g_txt = d_img + d_all[:n], d_txt + d_all[n:]
        elif mod.local_loss:
            g_img, g_txt = d_img, d_txt
            if mod.gather_with_grad:
                o_img, o_txt = unpack_caption_features(route_packed_gradient(d_all, b, rank, True, mod.group), c)
                g_img, g_txt = g_img + o_img, g_txt + o_txt
        else:                                       # both sides are the global set: [N, (1 + C) E] in all
            tot = d_all + pack_caption_features(d_img, d_txt, c)
            g_img, g_txt = unpack_caption_features(route_packed_gradient(tot, b, rank, mod.gather_with_grad, mod.group), c)
        dt_i, dt_t, dt_s = ctx.in_dtypes
        return None, g_img.to(dt_i), g_txt.to(dt_t), d_scale[0].to(dt_s)


class SigLipLoss(nn.Module):
    """Same constructor and call signature as the reference's SigLIP loss (loss.py:307-414), plus ``group``.

    Each rank holds ``[b, E]`` image and text embeddings.  The reference passes text blocks round a neighbour-exchange ring
    (loss.py:219-304) and adds one ``[b, b]`` sigmoid loss per block; here ONE all-gather of the text features gives the
    rank-ordered ``[N, E]`` set and the fused HIP kernel (``ov_siglip_loss``) sums the whole ``[b, N]`` strip, labels ``+1`` at
    ``i + b*rank`` and ``-1`` elsewhere.  Every rank's loss is the same sum over all text blocks, and the ring's backward hands
    each block's gradient back to its owner, as the reduce-scatter of the gathered-side gradient does here: only the order of
    the sums differs.  ``bidir`` only chooses the ring's direction in the reference, so it is accepted and has no effect.

    ``logit_bias`` (a 0-d tensor, a float, or None for no bias) and ``logit_scale`` (the multiplier, already ``exp``'d) stay on the
    device.  The loss is an autograd node whenever an input requires grad (backward: ``ov_siglip_loss_backward``)."""

    def __init__(self, cache_labels: bool = False, rank: int = 0, world_size: int = 1, bidir: bool = True,
                 use_horovod: bool = False, group=None):
        super().__init__()
        if use_horovod:
            raise NotImplementedError("horovod transport is not supported; use torch.distributed (RCCL)")
        self.cache_labels, self.rank, self.world_size, self.bidir, self.use_horovod = cache_labels, rank, world_size, bidir, use_horovod
        self.group = group
        self.always_collective = False   # tests only: take the world_size > 1 path (gather / reduce-scatter) in a world of one rank
        self._ws: Optional[torch.Tensor] = None

    def _gather_text(self, text: torch.Tensor) -> torch.Tensor:
        if self.world_size == 1 and not self.always_collective:
            return text
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("world_size > 1 needs an initialised torch.distributed process group (caller owns init)")
        return _all_gather_rows(text, self.world_size, self.group)

    def _loss_strip(self, img, all_txt, scale: torch.Tensor, bias: Optional[torch.Tensor], label_offset: int) -> torch.Tensor:
        lib = _lib.load()
        b, e = img.shape
        n = all_txt.shape[0]
        nbytes = lib.ov_siglip_loss_workspace_bytes(b, n)
        if self._ws is None or self._ws.device != img.device or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=img.device)
        out = torch.empty(1, dtype=torch.float32, device=img.device)
        check(lib.ov_siglip_loss(ptr(img), ptr(all_txt), b, n, e, ptr(scale), ptr(bias) if bias is not None else None,
                                 int(label_offset), ptr(out), ptr(self._ws), nbytes, stream_ptr()), "ov_siglip_loss")
        return out[0]

    def forward(self, image_features, text_features, logit_scale, logit_bias=None, output_dict: bool = False):
        if not (image_features.is_cuda and text_features.is_cuda):
            raise _lib.OvhipError("SigLipLoss: features must live on an MI355X device (no CPU fallback)")
        needs_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                     for t in (image_features, text_features, logit_scale, logit_bias))
        if needs_grad:
            dev = image_features.device
            if not isinstance(logit_scale, torch.Tensor):
                logit_scale = torch.tensor(float(logit_scale), device=dev)
            if logit_bias is not None and not isinstance(logit_bias, torch.Tensor):
                logit_bias = torch.tensor(float(logit_bias), device=dev)
            loss = _SigLipLossFn.apply(self, image_features, text_features, logit_scale, logit_bias)
        else:
            img = image_features.detach().float().contiguous()
            all_txt = self._gather_text(text_features.detach().float().contiguous())
            scale = ClipLoss._device_scale(logit_scale, img.device)
            bias = ClipLoss._device_scale(logit_bias, img.device) if logit_bias is not None else None
            loss = self._loss_strip(img, all_txt, scale, bias, img.shape[0] * self.rank)
        return {"contrastive_loss": loss} if output_dict else loss


class _SigLipLossFn(torch.autograd.Function):
    """SigLipLoss as an autograd node.  forward = the fused strip kernel; backward = ov_siglip_loss_backward, then the gathered
    side's gradient summed over ranks (own chunk kept): what the reference's NeighbourExchange backward returns to each block's
    owner (loss.py:273-280)."""

    @staticmethod
    def forward(ctx, mod: "SigLipLoss", image_features, text_features, logit_scale, logit_bias):
        img, txt = image_features.detach().float().contiguous(), text_features.detach().float().contiguous()
        b = img.shape[0]
        ctx.multi = mod.world_size > 1 or mod.always_collective
        all_txt = mod._gather_text(txt)
        off = b * mod.rank
        scale = ClipLoss._device_scale(logit_scale, img.device)
        bias = ClipLoss._device_scale(logit_bias, img.device) if logit_bias is not None else None
        loss = mod._loss_strip(img, all_txt, scale, bias, off)
        ctx.mod, ctx.off, ctx.has_bias = mod, off, bias is not None
        ctx.in_dtypes = (image_features.dtype, text_features.dtype, logit_scale.dtype,
                         logit_bias.dtype if logit_bias is not None else None)
        ctx.save_for_backward(img, all_txt, scale, bias)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        mod: "SigLipLoss" = ctx.mod
        img, all_txt, scale, bias = ctx.saved_tensors
        lib = _lib.load()
        b, e = img.shape
        n = all_txt.shape[0]
        d_img, d_all = torch.empty_like(img), torch.empty_like(all_txt)
        d_sc = torch.empty(2, dtype=torch.float32, device=img.device)            # d scale, d bias
        grad = grad_out.detach().float().reshape(1).contiguous()                  # device scalar: no host round trip
        nbytes = lib.ov_siglip_loss_backward_workspace_bytes(b, n)
        wsb = torch.empty(nbytes + 256, dtype=torch.uint8, device=img.device)
        check(lib.ov_siglip_loss_backward(ptr(img), ptr(all_txt), b, n, e, ptr(scale), ptr(bias) if ctx.has_bias else None, ctx.off,
                                          ptr(grad), ptr(d_img), ptr(d_all), ptr(d_sc[0:]), ptr(d_sc[1:]) if ctx.has_bias else None,
                                          ptr(wsb), nbytes, stream_ptr()), "ov_siglip_loss_backward")
        # text appears on the gathered side only: at world_size 1 its gradient IS d_all (nothing to add)
        d_txt = _sum_over_ranks_own_chunk(d_all, b, mod.rank, mod.group) if ctx.multi else d_all
        dt_i, dt_t, dt_s, dt_b = ctx.in_dtypes
        return (None, d_img.to(dt_i), d_txt.to(dt_t), d_sc[0].to(dt_s), d_sc[1].to(dt_b) if ctx.has_bias else None)


def pack_distill_features(image_features: torch.Tensor, text_features: torch.Tensor, dist_image_features: torch.Tensor,
                          dist_text_features: torch.Tensor) -> torch.Tensor:
    """Student rows [b, E] (image, text) and teacher rows [b, Et] (image, text) -> one [b, 2E + 2Et] buffer: student image in columns
    0 ... E, student text in E ... 2E, teacher image in 2E ... 2E + Et, teacher text behind it.  The layout ``ov_distill_loss`` reads
    in place after the all-gather (ld = ldt = 2E + 2Et)."""
    return torch.cat([image_features, text_features, dist_image_features, dist_text_features], dim=1)


def unpack_distill_features(packed: torch.Tensor, embed_dim: int):
    """Inverse of ``pack_distill_features`` on [n, 2E + 2Et] rows, E = ``embed_dim``: four column views (student image, student text,
    teacher image, teacher text)."""
    e = embed_dim
    et = (packed.shape[1] - 2 * e) // 2
    return packed[:, :e], packed[:, e:2 * e], packed[:, 2 * e:2 * e + et], packed[:, 2 * e + et:]


def gather_distill_features(image_features, text_features, dist_image_features, dist_text_features, world_size: int,
                            group=None) -> torch.Tensor:
    """ONE all_gather_into_tensor of the packed rows -> [world_size * b, 2E + 2Et] in rank order (seen by ``record_comm``)."""
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("world_size > 1 needs an initialised torch.distributed process group (caller owns init)")
    packed = pack_distill_features(*(t.detach().float() for t in (image_features, text_features, dist_image_features,
                                                                  dist_text_features))).contiguous()
    return _all_gather_rows(packed, world_size, group)


class DistillClipLoss(ClipLoss):
    """Distillation from a frozen teacher: the reference's ``DistillClipLoss`` (loss.py:180-216).  Constructor as ``ClipLoss``; the
    call takes the student's features and multiplier, then the teacher's, and returns ``(contrastive_loss, distill_loss)``: the
    student's InfoNCE and the cross entropy of the student's log-softmax under the teacher's softmax, both ways.  One fused forward
    and one backward (``ov_distill_loss*``) on ONE all-gather of the packed ``[b, 2E + 2Et]`` rows read in place; the teacher's
    embedding width may differ from the student's.  The student's gathered-side gradient is routed as ``ClipLoss`` routes it (own
    chunk, or one reduce-scatter of the packed ``[N, 2E]`` gradient under ``gather_with_grad``); the teacher's share of the gather is
    never exchanged back.

    The teacher is frozen HERE: the reference would differentiate through teacher tensors that require grad, this build computes no
    such gradient and therefore refuses them (``ValueError``) instead of returning none silently.

    ``last_terms`` is the forward's [12, b] block: the student's lse_img, diag_img, lse_txt, diag_txt, then the teacher's lse and the
    cross sum of the image strip and of the text strip, then the low parts of the four lse (ovhip.h)."""

    _ws_bwd: Optional[torch.Tensor] = None      # the backward's workspace, kept like the forward's ``_ws``

    def _check(self, image_features, text_features, dist_image_features, dist_text_features, dist_logit_scale):
        s, t = (image_features, text_features), (dist_image_features, dist_text_features)
        if any(x.dim() != 2 for x in s + t) or s[0].shape != s[1].shape or t[0].shape != t[1].shape or s[0].shape[0] != t[0].shape[0]:
            raise ValueError("DistillClipLoss: student features must be two [b, E] tensors and teacher features two [b, Et] tensors "
                             f"with the same b, got {[tuple(x.shape) for x in s + t]}")
        if any(isinstance(x, torch.Tensor) and x.requires_grad for x in t + (dist_logit_scale,)):
            raise ValueError("DistillClipLoss: the teacher is frozen here (no gradient is computed for dist_image_features, "
                             "dist_text_features or dist_logit_scale): run the teacher under torch.no_grad() or detach its outputs")
        if not all(x.is_cuda for x in s + t):
            raise _lib.OvhipError("DistillClipLoss: features must live on an MI355X device (no CPU fallback)")

    def _operands(self, img, txt, t_img, t_txt):
        """(local student rows, local teacher rows, the four gathered operands, ld, ldt, label offset) for this rank."""
        b, e = img.shape
        et = t_img.shape[1]
        if not (self.world_size > 1 or self.always_collective):
            return (img, txt), (t_img, t_txt), (img, txt, t_img, t_txt), e, et, 0
        packed = gather_distill_features(img, txt, t_img, t_txt, self.world_size, self.group)
        views = unpack_distill_features(packed, e)
        if self.local_loss:
            x, u, off = (img, txt), (t_img, t_txt), b * self.rank
        else:                       # the global loss on every rank (loss.py:111-113): the local rows are the gathered rows
            x, u, off = (views[0].contiguous(), views[1].contiguous()), (views[2].contiguous(), views[3].contiguous()), 0
        return x, u, views, packed.shape[1], packed.shape[1], off

    def _distill_strips(self, x, u, g, ld: int, ldt: int, scale: torch.Tensor, t_scale: torch.Tensor, off: int):
        lib = _lib.load()
        b, e = x[0].shape
        et, n, dev = u[0].shape[1], g[0].shape[0], x[0].device
        nbytes = lib.ov_distill_loss_workspace_bytes(b, n)
        if self._ws is None or self._ws.device != dev or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        terms = torch.empty(12, b, dtype=torch.float32, device=dev)
        check(lib.ov_distill_loss(ptr(x[0]), ptr(x[1]), ptr(g[0]), ptr(g[1]), ld, ptr(u[0]), ptr(u[1]), ptr(g[2]), ptr(g[3]), ldt, b, n, e,
                                  et, ptr(scale), ptr(t_scale), int(off), ptr(out[0:]), ptr(out[1:]), ptr(terms), ptr(self._ws), nbytes,
                                  stream_ptr()), "ov_distill_loss")
        self.last_terms = terms
        return out[0], out[1]

    def forward(self, image_features, text_features, logit_scale, dist_image_features, dist_text_features, dist_logit_scale,
                output_dict: bool = False):
        self._check(image_features, text_features, dist_image_features, dist_text_features, dist_logit_scale)
        needs_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                     for t in (image_features, text_features, logit_scale))
        if needs_grad:
            if not isinstance(logit_scale, torch.Tensor):
                logit_scale = torch.tensor(float(logit_scale), device=image_features.device)
            c, d = _DistillClipLossFn.apply(self, image_features, text_features, logit_scale, dist_image_features, dist_text_features,
                                            dist_logit_scale)
        else:
            img, txt, t_img, t_txt = (t.detach().float().contiguous() for t in (image_features, text_features, dist_image_features,
                                                                                 dist_text_features))
            scale, t_scale = self._device_scale(logit_scale, img.device), self._device_scale(dist_logit_scale, img.device)
            x, u, g, ld, ldt, off = self._operands(img, txt, t_img, t_txt)
            c, d = self._distill_strips(x, u, g, ld, ldt, scale, t_scale, off)
        return {"contrastive_loss": c, "distill_loss": d} if output_dict else (c, d)


class _DistillClipLossFn(torch.autograd.Function):
    """DistillClipLoss as an autograd node with two outputs.  forward = ov_distill_loss on the packed gather; backward =
    ov_distill_loss_backward with both upstream gradients as device scalars, the student's gathered side written as one packed
    [N, 2E] gradient and routed as ``_ClipLossFn`` routes its two halves.  The teacher inputs get None."""

    @staticmethod
    def forward(ctx, mod: "DistillClipLoss", image_features, text_features, logit_scale, dist_image_features, dist_text_features,
                dist_logit_scale):
        img, txt, t_img, t_txt = (t.detach().float().contiguous() for t in (image_features, text_features, dist_image_features,
                                                                             dist_text_features))
        scale, t_scale = mod._device_scale(logit_scale, img.device), mod._device_scale(dist_logit_scale, img.device)
        x, u, g, ld, ldt, off = mod._operands(img, txt, t_img, t_txt)
        c, d = mod._distill_strips(x, u, g, ld, ldt, scale, t_scale, off)
        ctx.mod, ctx.off, ctx.b, ctx.lay = mod, off, img.shape[0], (ld, ldt)
        ctx.multi = mod.world_size > 1 or mod.always_collective
        ctx.in_dtypes = (image_features.dtype, text_features.dtype, logit_scale.dtype)
        ctx.save_for_backward(*x, *u, *g, mod.last_terms, scale, t_scale)
        return c, d

    @staticmethod
    def backward(ctx, grad_c, grad_d):
        mod: "DistillClipLoss" = ctx.mod
        x_img, x_txt, u_img, u_txt, y_img, y_txt, v_img, v_txt, terms, scale, t_scale = ctx.saved_tensors
        lib = _lib.load()
        rank, b = mod.rank, ctx.b
        bx, e = x_img.shape
        et, n, dev = u_img.shape[1], y_img.shape[0], x_img.device
        ld, ldt = ctx.lay
        single = not ctx.multi                      # world of one without the collectives: both sides are the same tensors
        gathered_grad = single or not mod.local_loss or mod.gather_with_grad
        d_img, d_txt = torch.empty_like(x_img), torch.empty_like(x_txt)
        d_scale = torch.empty(1, dtype=torch.float32, device=dev)
        if not gathered_grad:
            d_all, p_ai, p_at, ldg = None, None, None, 0
        elif single:                                # laid out as the features themselves: two [b, E] arrays
            d_all = torch.empty(2, n, e, dtype=torch.float32, device=dev)
            p_ai, p_at, ldg = ptr(d_all[0]), ptr(d_all[1]), e
        else:                                       # packed [N, 2E]: the student's half of the gather's layout, for one reduce-scatter
            d_all = torch.empty(n, 2 * e, dtype=torch.float32, device=dev)
            p_ai, p_at, ldg = ptr(d_all), ptr(d_all[:, e:]), 2 * e
        g_c = grad_c.detach().float().reshape(1).contiguous()           # device scalars: no host round trip
        g_d = grad_d.detach().float().reshape(1).contiguous()
        nbytes = lib.ov_distill_loss_backward_workspace_bytes(bx, n)
        wsb = mod._ws_bwd
        if wsb is None or wsb.device != dev or wsb.numel() < nbytes:
            wsb = mod._ws_bwd = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        check(lib.ov_distill_loss_backward(ptr(x_img), ptr(x_txt), ptr(y_img), ptr(y_txt), ld, ptr(u_img), ptr(u_txt), ptr(v_img),
                                           ptr(v_txt), ldt, bx, n, e, et, ptr(scale), ptr(t_scale), ctx.off, ptr(terms), ptr(g_c), ptr(g_d),
                                           ptr(d_img), ptr(d_txt), p_ai, p_at, ldg, ptr(d_scale), ptr(wsb), nbytes, stream_ptr()),
              "ov_distill_loss_backward")
        if single:
            g_img, g_txt = d_img + d_all[0], d_txt + d_all[1]
        elif mod.local_loss:
            g_img, g_txt = d_img, d_txt
            if mod.gather_with_grad:
                own = route_packed_gradient(d_all, b, rank, True, mod.group)
                g_img, g_txt = g_img + own[:, :e], g_txt + own[:, e:]
        else:                                       # both sides are the global set: [N, 2E] in all
            own = route_packed_gradient(d_all + torch.cat([d_img, d_txt], dim=1), b, rank, mod.gather_with_grad, mod.group)
            g_img, g_txt = own[:, :e], own[:, e:]
        dt_i, dt_t, dt_s = ctx.in_dtypes
        return None, g_img.to(dt_i), g_txt.to(dt_t), d_scale[0].to(dt_s), None, None, None
