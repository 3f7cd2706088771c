"""MI355X-native counterpart of ``open_clip.loss.ClipLoss`` (reference ``src/convert_upload/open_clip/loss.py:19-131``).

Data-parallel InfoNCE: each rank holds ``[b, E]`` L2-normalised image and text embeddings; ONE RCCL all-gather of
the packed ``[b, 2E]`` buffer (``torch.distributed`` backend "nccl" == RCCL over xGMI) yields the rank-ordered global
sets (loss.py:52-61), then the fused HIP kernel computes the local ``[b, N]`` logit strips both ways with labels
``i + b*rank`` (loss.py:93-94,108-110) without materialising them, reading the gathered buffer in place.

``MultiCaptionClipLoss`` is the InfoNCE OpenVision trains with: C caption sets per image (src/losses/common.py:120-189, C = 2), the
mean over the sets of ``ClipLoss(image, text_c)`` in one fused forward and backward (``ov_clip_loss_multi*``) on one packed gather.
``ClipLoss`` is its C = 1 case: both are ``_InfoNCELoss``, one forward launch and one autograd node.

``DistillClipLoss`` (loss.py:180-216) adds the cross entropy under a frozen teacher's softmax to ``ClipLoss``: two outputs from one fused
forward and backward (``ov_distill_loss*``) on one packed gather of the student's and the teacher's rows.

``SigLipLoss`` (loss.py:307-414) is the pairwise sigmoid objective on the same transport: one all-gather of the text features,
one fused strip kernel (``ov_siglip_loss``), and in the backward the gathered side summed over ranks.

Gradients: when a feature tensor or ``logit_scale`` requires grad, a loss is an autograd node whose forward is the launch the
no-grad call makes and whose backward is the matching HIP kernel; ``openvision_amd.training`` carries the gradient on through the
towers.  What reaches a rank's own features from the gathered side is decided in ONE place, ``route_gradient``, the way
``gather_features`` makes it flow in the reference (loss.py:19-63): own chunk only, or summed over ranks (reduce-scatter) with
``gather_with_grad``.  ``use_horovod`` is rejected (RCCL via torch.distributed is the only transport here).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.distributed as dist
from torch import nn

from . import _lib
from ._lib import ptr, stream_ptr, check
from .model import _Workspace


_COMM_LOG = None      # diagnostics (bench.py --gpus N): a list that every all-gather appends one (start, end) pair to


def record_comm(log) -> None:
    """Diagnostics: pass a list to have every all-gather of this module bracketed by a pair of timing marks appended to it --
    ``torch.cuda.Event``s recorded on the current stream for device tensors (the collective is stream-ordered: the current stream waits
    for it), ``time.perf_counter()`` floats on the CPU (gloo rehearsal).  ``None`` turns it off.  Nothing is synchronised here."""
    global _COMM_LOG
    _COMM_LOG = log


def _all_gather_rows(x: torch.Tensor, world_size: int, group=None) -> torch.Tensor:
    """[b, C] on every rank -> [world_size * b, C] in rank order: one all_gather_into_tensor, bracketed for record_comm.  Every
    gather of this module ends here, so this is where the process group is asked for."""
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("world_size > 1 needs an initialised torch.distributed process group (caller owns init)")
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


def _gather_packed(blocks, world_size: int, group=None):
    """[b, w_k] column blocks -> (the [world_size * b, sum w_k] rows of ONE all-gather of their concatenation, in rank order, and
    that buffer's column views, one per block: what the kernels read in place with ld = sum w_k)."""
    packed = torch.cat([t.detach().float() for t in blocks], dim=1).contiguous()
    out = _all_gather_rows(packed, world_size, group)
    return out, out.split([t.shape[1] for t in blocks], dim=1)


def gather_features(image_features: torch.Tensor, text_features: torch.Tensor, local_loss: bool = False,
                    gather_with_grad: bool = False, rank: int = 0, world_size: int = 1, use_horovod: bool = False,
                    group=None, force: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """loss.py:19-63.  One all-gather of the packed [b, 2E] buffer instead of two list gathers;
    the result is identical: rows in rank order (torch.cat(gathered, dim=0), loss.py:60-61)."""
    if use_horovod:
        raise NotImplementedError("horovod transport is not supported; use torch.distributed (RCCL)")
    if world_size == 1 and not force:          # force: run the collective anyway (tests drive the RCCL path in a world of one)
        return image_features, text_features
    all_img, all_txt = _gather_packed([image_features, text_features], world_size, group)[1]
    return all_img.contiguous(), all_txt.contiguous()


def _caption_blocks(image_features: torch.Tensor, text_features: torch.Tensor, num_captions: int):
    b = image_features.shape[0]
    return [image_features] + [text_features[c * b:(c + 1) * b] for c in range(num_captions)]


def pack_caption_features(image_features: torch.Tensor, text_features: torch.Tensor, num_captions: int) -> torch.Tensor:
    """[b, E] image rows and the stacked [C b, E] text rows (set c in rows c b ...) -> one [b, (1 + C) E] buffer: the image in
    columns 0 ... E, set c in columns (1 + c) E ...  The layout ``ov_clip_loss_multi`` reads in place after the all-gather."""
    return torch.cat(_caption_blocks(image_features, text_features, num_captions), dim=1)


def unpack_caption_features(packed: torch.Tensor, num_captions: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inverse of ``pack_caption_features`` on [n, (1 + C) E] rows: ([n, E] image rows, [C n, E] stacked text rows)."""
    e = packed.shape[1] // (1 + num_captions)
    return packed[:, :e], torch.cat([packed[:, (1 + c) * e:(2 + c) * e] for c in range(num_captions)], dim=0)


def gather_caption_features(image_features: torch.Tensor, text_features: torch.Tensor, num_captions: int, world_size: int,
                            group=None) -> torch.Tensor:
    """ONE all-gather of the packed rows -> [world_size * b, (1 + C) E] in rank order (seen by ``record_comm``)."""
    return _gather_packed(_caption_blocks(image_features, text_features, num_captions), world_size, group)[0]


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
    """ONE all-gather of the packed rows -> [world_size * b, 2E + 2Et] in rank order (seen by ``record_comm``)."""
    return _gather_packed([image_features, text_features, dist_image_features, dist_text_features], world_size, group)[0]


def _sum_over_ranks_own_chunk(full: torch.Tensor, b: int, rank: int, group=None) -> torch.Tensor:
    """Backward of ``torch.distributed.nn.all_gather`` (loss.py:49-50): every rank's [N, W] gathered-side gradient summed,
    this rank keeps rows [rank*b, (rank+1)*b).  One reduce-scatter on RCCL; gloo has none, so all-reduce + slice there."""
    if dist.get_backend(group) == "nccl":
        out = torch.empty(b, full.shape[1], dtype=full.dtype, device=full.device)
        dist.reduce_scatter_tensor(out, full.contiguous(), group=group)
        return out
    full = full.contiguous()
    dist.all_reduce(full, group=group)
    return full[rank * b:(rank + 1) * b]


def route_packed_gradient(full: torch.Tensor, b: int, rank: int, gather_with_grad: bool, group=None) -> torch.Tensor:
    """What reaches this rank's own features from a packed [N, (1 + C) E] gradient of the gathered rows: with ``gather_with_grad``
    the sum over ranks of rows [rank b, (rank + 1) b) (the backward of the differentiable all-gather: one reduce-scatter), else
    this rank's own rows of its own gradient (the chunk put back into the detached gather).  Works on CPU tensors over gloo."""
    if gather_with_grad:
        return _sum_over_ranks_own_chunk(full, b, rank, group)
    return full[rank * b:(rank + 1) * b]


def route_gradient(d_local: torch.Tensor, d_gathered: Optional[torch.Tensor], b: int, rank: int, collective: bool, local_loss: bool,
                   gather_with_grad: bool, group=None) -> torch.Tensor:
    """The gradient of this rank's own features, packed [b, W], from the two sides of an InfoNCE-type backward: ``d_local`` is the
    packed gradient of the rows this rank evaluated (its own [b, W], or all [N, W] for the global loss), ``d_gathered`` the packed
    [N, W] gradient of the gathered rows (None where a detached gather under ``local_loss`` carries none).  As autograd through
    ``gather_features`` (loss.py:19-63):
      * no collective: both sides are the same tensors, local + gathered (any common layout);
      * ``local_loss``: local (as it stands, in whatever layout), plus with ``gather_with_grad`` every rank's gathered side summed,
        own rows kept (one reduce-scatter);
      * global loss: both sides are the global set; own rows of local + gathered, summed over ranks under ``gather_with_grad``.
    Works on CPU tensors over gloo."""
    assert (d_gathered is None) == (collective and local_loss and not gather_with_grad), "gathered side: given iff it carries gradient"
    if not collective:
        return d_local + d_gathered
    if local_loss:
        return d_local + _sum_over_ranks_own_chunk(d_gathered, b, rank, group) if gather_with_grad else d_local
    return route_packed_gradient(d_local + d_gathered, b, rank, gather_with_grad, group)


def gathered_gradient_buffer(n: int, e: int, num_captions: int, packed: bool, device):
    """Where a backward kernel writes the gradient of the n gathered rows, and how it addresses it: (buffer, pointer to the image
    part, pointer to caption set 0, ldg, gset_stride), in floats; element k of row j lies ldg j + k behind its part's pointer and
    set c a further c gset_stride.  Not ``packed``: the features' own layout [(1 + C) n, E], image rows first, then set c in rows
    (1 + c) n ... (a world of one adds it to the local side as it stands).  ``packed``: [n, (1 + C) E], the layout of the gather, for
    one reduce-scatter.  DistillClipLoss's student half is the C = 1 case."""
    c = num_captions
    if packed:
        buf = torch.empty(n, (1 + c) * e, dtype=torch.float32, device=device)
        return buf, ptr(buf), ptr(buf[:, e:]), (1 + c) * e, e
    buf = torch.empty((1 + c) * n, e, dtype=torch.float32, device=device)
    return buf, ptr(buf), ptr(buf[n:]), e, n * e


def _collective(mod) -> bool:
    return mod.world_size > 1 or mod.always_collective


def _needs_grad(*inputs) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs)


def _device_scalar(x, device) -> torch.Tensor:
    """A logit multiplier or bias as a 1-element fp32 DEVICE tensor.  It never visits the host (ovhip.h ABI 2): `float(logit_scale)`
    would drain the stream after both towers before the loss could be enqueued."""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            return x.detach().float().reshape(1).to(device, non_blocking=True)
        return x.detach().float().reshape(1)
    return torch.full((1,), float(x), dtype=torch.float32, device=device)


def _as_node_input(x, device):
    """A float handed to an autograd node becomes a 0-d tensor: the node returns a gradient of its dtype.  None stays None."""
    return x if x is None or isinstance(x, torch.Tensor) else torch.tensor(float(x), device=device)


def _backward_buffers(mod, collective: bool, bx: int, n: int, e: int, num_captions: int, device):
    """The feature-gradient outputs of an InfoNCE-type backward: (d_local [(1 + C) bx, E], the local side in the features' own
    layout; d_gathered or None; (image pointer, text pointer, ldg, gset_stride) of d_gathered for the kernel).  The gathered side
    carries gradient when it IS the local tensor (no collective), when the own chunk was put back (not local_loss, loss.py:57-59)
    or when the gather itself is differentiable (gather_with_grad)."""
    d_local = torch.empty((1 + num_captions) * bx, e, dtype=torch.float32, device=device)
    if collective and mod.local_loss and not mod.gather_with_grad:
        return d_local, None, (None, None, 0, 0)
    d_gathered, *addr = gathered_gradient_buffer(n, e, num_captions, collective, device)
    return d_local, d_gathered, addr


def _own_gradients(mod, collective: bool, d_local: torch.Tensor, d_gathered: Optional[torch.Tensor], b: int, num_captions: int):
    """(d image_features [b, E], d text_features [C b, E]) of this rank from the buffers of ``_backward_buffers`` after the kernel.
    Where nothing is exchanged (no collective, or no gathered side) the rule is applied in the features' own layout; otherwise the
    local side is packed like the gather first: one copy, and the results are column views or a copy of the packed rows."""
    if not collective or d_gathered is None:
        own = route_gradient(d_local, d_gathered, b, mod.rank, collective, mod.local_loss, mod.gather_with_grad, mod.group)
        return own[:b], own[b:]
    bx = d_local.shape[0] // (1 + num_captions)
    own = route_gradient(pack_caption_features(d_local[:bx], d_local[bx:], num_captions), d_gathered, b, mod.rank, True,
                         mod.local_loss, mod.gather_with_grad, mod.group)
    return unpack_caption_features(own, num_captions)


class _InfoNCELoss(nn.Module):
    """``ClipLoss`` and ``MultiCaptionClipLoss``: InfoNCE over ``num_captions`` caption sets, the reference's constructor
    (loss.py:68-83) plus ``group``.  One forward launch (``ov_clip_loss_multi``), one autograd node (``_InfoNCEFn``)."""

    num_captions = 1

    def __init__(self, local_loss: bool = False, gather_with_grad: bool = False, cache_labels: bool = False,
                 rank: int = 0, world_size: int = 1, use_horovod: bool = False, group=None):
        super().__init__()
        if use_horovod:
            raise NotImplementedError("horovod transport is not supported; use torch.distributed (RCCL)")
        self.group = group          # process group of the gather / reduce-scatter (None = the default group, as the reference)
        self.local_loss, self.gather_with_grad, self.cache_labels = local_loss, gather_with_grad, cache_labels
        self.rank, self.world_size, self.use_horovod = rank, world_size, use_horovod
        self.always_collective = False   # tests only: take the world_size > 1 path (gather / reduce-scatter) in a world of one rank
        self._ws, self._ws_bwd = _Workspace(), _Workspace()
        self.last_terms: Optional[torch.Tensor] = None     # [4 C, b]: per set lse_img, diag_img, lse_txt, diag_txt

    def _check(self, image_features, text_features):
        name = type(self).__name__
        if image_features.dim() != 2 or text_features.dim() != 2 or image_features.shape[1] != text_features.shape[1] \
                or text_features.shape[0] != self.num_captions * image_features.shape[0]:
            raise ValueError(f"{name}: text_features must be [{self.num_captions} * b, E] for image_features [b, E], "
                             f"got {tuple(text_features.shape)} for {tuple(image_features.shape)}")
        if not (image_features.is_cuda and text_features.is_cuda):
            raise _lib.OvhipError(f"{name}: features must live on an MI355X device (no CPU fallback)")

    def _operands(self, img: torch.Tensor, txt: torch.Tensor):
        """(x_img, x_txt, gathered operand, its text view, ld, set_stride, label offset) for this rank."""
        c, b, e = self.num_captions, img.shape[0], img.shape[1]
        if not _collective(self):
            return img, txt, img, txt, e, b * e, 0
        packed = gather_caption_features(img, txt, c, self.world_size, self.group)
        if self.local_loss:
            x_img, x_txt, off = img, txt, b * self.rank
        else:                       # the global loss on every rank (loss.py:111-113): the local rows are the gathered rows
            x_img, x_txt = (t.contiguous() for t in unpack_caption_features(packed, c))
            off = 0
        return x_img, x_txt, packed, packed[:, e:], (1 + c) * e, e, off

    def _launch(self, image_features, text_features, logit_scale):
        """The forward, with or without grad: (loss, what the backward needs as tensors, (ld, set_stride, label offset))."""
        lib = _lib.load()
        img, txt = image_features.detach().float().contiguous(), text_features.detach().float().contiguous()
        scale = _device_scalar(logit_scale, img.device)
        x_img, x_txt, all_img, all_txt, ld, ss, off = self._operands(img, txt)
        (b, e), n, c = x_img.shape, all_img.shape[0], self.num_captions
        nbytes = lib.ov_clip_loss_multi_workspace_bytes(b, n, c)
        out = torch.empty(1, dtype=torch.float32, device=img.device)
        terms = torch.empty(4 * c, b, dtype=torch.float32, device=img.device)
        check(lib.ov_clip_loss_multi(ptr(x_img), ptr(x_txt), ptr(all_img), ptr(all_txt), ld, ss, b, n, e, c, ptr(scale), int(off),
                                     ptr(out), ptr(terms), ptr(self._ws.get(nbytes, img.device)), nbytes, stream_ptr()),
              "ov_clip_loss_multi")
        self.last_terms = terms
        return out[0], (x_img, x_txt, all_img, all_txt, terms, scale), (ld, ss, off)

    def forward(self, image_features, text_features, logit_scale, output_dict: bool = False):
        self._check(image_features, text_features)
        if _needs_grad(image_features, text_features, logit_scale):
            loss = _InfoNCEFn.apply(self, image_features, text_features, _as_node_input(logit_scale, image_features.device))
        else:
            loss = self._launch(image_features, text_features, logit_scale)[0]
        return {"contrastive_loss": loss} if output_dict else loss


class _InfoNCEFn(torch.autograd.Function):
    """``_InfoNCELoss`` as an autograd node.  forward = the module's launch; backward = ov_clip_loss_multi_backward, the gathered
    side written in the layout ``route_gradient`` wants it in."""

    @staticmethod
    def forward(ctx, mod: _InfoNCELoss, image_features, text_features, logit_scale):
        loss, saved, ctx.lay = mod._launch(image_features, text_features, logit_scale)
        ctx.mod, ctx.b, ctx.collective = mod, image_features.shape[0], _collective(mod)
        ctx.in_dtypes = (image_features.dtype, text_features.dtype, logit_scale.dtype)
        ctx.save_for_backward(*saved)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        mod: _InfoNCELoss = ctx.mod
        x_img, x_txt, all_img, all_txt, terms, scale = ctx.saved_tensors
        lib = _lib.load()
        (bx, e), n, c, dev = x_img.shape, all_img.shape[0], mod.num_captions, x_img.device
        ld, ss, off = ctx.lay
        d_local, d_all, (p_ai, p_at, ldg, gss) = _backward_buffers(mod, ctx.collective, bx, n, e, c, dev)
        d_scale = torch.empty(1, dtype=torch.float32, device=dev)
        grad = grad_out.detach().float().reshape(1).contiguous()        # device scalar: no host round trip
        nbytes = lib.ov_clip_loss_multi_backward_workspace_bytes(bx, n, c)
        check(lib.ov_clip_loss_multi_backward(ptr(x_img), ptr(x_txt), ptr(all_img), ptr(all_txt), ld, ss, bx, n, e, c, ptr(scale), off,
                                              ptr(terms), ptr(grad), ptr(d_local), ptr(d_local[bx:]), p_ai, p_at, ldg, gss, ptr(d_scale),
                                              ptr(mod._ws_bwd.get(nbytes, dev)), nbytes, stream_ptr()), "ov_clip_loss_multi_backward")
        g_img, g_txt = _own_gradients(mod, ctx.collective, d_local, d_all, ctx.b, c)
        dt_i, dt_t, dt_s = ctx.in_dtypes
        return None, g_img.to(dt_i), g_txt.to(dt_t), d_scale[0].to(dt_s)


class ClipLoss(_InfoNCELoss):
    """Same constructor and call signature as the reference (loss.py:68-83,120-131).  ``last_terms`` is [4, b]."""


class MultiCaptionClipLoss(_InfoNCELoss):
    """InfoNCE with ``num_captions`` caption sets per image: what OpenVision trains with (``bidirectional_contrastive_loss``,
    src/losses/common.py:120-189, two sets, ``local_loss=True``).  ``text_features`` holds the sets stacked ``[C b, E]`` (set c in
    rows ``c b ...``, the reference's ``ztxt[:half] / ztxt[half:]``); the loss is the mean over the sets of ``ClipLoss(image, text_c)``,
    computed by one fused forward and one backward (``ov_clip_loss_multi*``): one all-gather of the packed ``[b, (1 + C) E]`` rows
    read in place, the image-side gradients accumulated over the sets inside the kernel, and under ``gather_with_grad`` one
    reduce-scatter of the packed gathered-side gradient.  Constructor as ``ClipLoss``, plus ``num_captions`` in front; the
    reference's ``pmean`` over ranks is left to the gradient averaging, as in ``ClipLoss``."""

    def __init__(self, num_captions: int = 2, local_loss: bool = False, gather_with_grad: bool = False, cache_labels: bool = False,
                 rank: int = 0, world_size: int = 1, use_horovod: bool = False, group=None):
        super().__init__(local_loss, gather_with_grad, cache_labels, rank, world_size, use_horovod, group)
        if not 1 <= int(num_captions) <= 4:
            raise ValueError("num_captions must be 1 ... 4")
        self.num_captions = int(num_captions)


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
        self._ws, self._ws_bwd = _Workspace(), _Workspace()

    def _launch(self, image_features, text_features, logit_scale, logit_bias):
        """The forward, with or without grad: (loss, what the backward needs as tensors, label offset)."""
        lib = _lib.load()
        img, txt = image_features.detach().float().contiguous(), text_features.detach().float().contiguous()
        all_txt = _all_gather_rows(txt, self.world_size, self.group) if _collective(self) else txt
        scale = _device_scalar(logit_scale, img.device)
        bias = _device_scalar(logit_bias, img.device) if logit_bias is not None else None
        (b, e), n, off = img.shape, all_txt.shape[0], img.shape[0] * self.rank
        nbytes = lib.ov_siglip_loss_workspace_bytes(b, n)
        out = torch.empty(1, dtype=torch.float32, device=img.device)
        check(lib.ov_siglip_loss(ptr(img), ptr(all_txt), b, n, e, ptr(scale), ptr(bias) if bias is not None else None, int(off),
                                 ptr(out), ptr(self._ws.get(nbytes, img.device)), nbytes, stream_ptr()), "ov_siglip_loss")
        return out[0], (img, all_txt, scale, bias), off

    def forward(self, image_features, text_features, logit_scale, logit_bias=None, output_dict: bool = False):
        if not (image_features.is_cuda and text_features.is_cuda):
            raise _lib.OvhipError("SigLipLoss: features must live on an MI355X device (no CPU fallback)")
        if _needs_grad(image_features, text_features, logit_scale, logit_bias):
            dev = image_features.device
            loss = _SigLipLossFn.apply(self, image_features, text_features, _as_node_input(logit_scale, dev),
                                       _as_node_input(logit_bias, dev))
        else:
            loss = self._launch(image_features, text_features, logit_scale, logit_bias)[0]
        return {"contrastive_loss": loss} if output_dict else loss


class _SigLipLossFn(torch.autograd.Function):
    """SigLipLoss as an autograd node.  forward = the module's launch; backward = ov_siglip_loss_backward, then the gathered
    side's gradient summed over ranks (own chunk kept): what the reference's NeighbourExchange backward returns to each block's
    owner (loss.py:273-280)."""

    @staticmethod
    def forward(ctx, mod: SigLipLoss, image_features, text_features, logit_scale, logit_bias):
        loss, saved, ctx.off = mod._launch(image_features, text_features, logit_scale, logit_bias)
        ctx.mod, ctx.collective, ctx.has_bias = mod, _collective(mod), logit_bias is not None
        ctx.in_dtypes = (image_features.dtype, text_features.dtype, logit_scale.dtype,
                         logit_bias.dtype if logit_bias is not None else None)
        ctx.save_for_backward(*saved)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        mod: SigLipLoss = ctx.mod
        img, all_txt, scale, bias = ctx.saved_tensors
        lib = _lib.load()
        b, e = img.shape
        n = all_txt.shape[0]
        d_img, d_all = torch.empty_like(img), torch.empty_like(all_txt)
        d_sc = torch.empty(2, dtype=torch.float32, device=img.device)            # d scale, d bias
        grad = grad_out.detach().float().reshape(1).contiguous()                  # device scalar: no host round trip
        nbytes = lib.ov_siglip_loss_backward_workspace_bytes(b, n)
        check(lib.ov_siglip_loss_backward(ptr(img), ptr(all_txt), b, n, e, ptr(scale), ptr(bias) if ctx.has_bias else None, ctx.off,
                                          ptr(grad), ptr(d_img), ptr(d_all), ptr(d_sc[0:]), ptr(d_sc[1:]) if ctx.has_bias else None,
                                          ptr(mod._ws_bwd.get(nbytes, img.device)), nbytes, stream_ptr()), "ov_siglip_loss_backward")
        # text appears on the gathered side only: at world_size 1 its gradient IS d_all (nothing to add); under a collective the
        # gather is always differentiable here
        d_txt = _sum_over_ranks_own_chunk(d_all, b, mod.rank, mod.group) if ctx.collective else d_all
        dt_i, dt_t, dt_s, dt_b = ctx.in_dtypes
        return (None, d_img.to(dt_i), d_txt.to(dt_t), d_sc[0].to(dt_s), d_sc[1].to(dt_b) if ctx.has_bias else None)


class DistillClipLoss(ClipLoss):
    """Distillation from a frozen teacher: the reference's ``DistillClipLoss`` (loss.py:180-216).  Constructor as ``ClipLoss``; the
    call takes the student's features and multiplier, then the teacher's, and returns ``(contrastive_loss, distill_loss)``: the
    student's InfoNCE and the cross entropy of the student's log-softmax under the teacher's softmax, both ways.  One fused forward
    and one backward (``ov_distill_loss*``) on ONE all-gather of the packed ``[b, 2E + 2Et]`` rows read in place; the teacher's
    embedding width may differ from the student's.  The student's gathered-side gradient is routed as ``ClipLoss`` routes it
    (``route_gradient`` on the packed ``[N, 2E]`` student half); the teacher's share of the gather is never exchanged back.

    The teacher is frozen HERE: the reference would differentiate through teacher tensors that require grad, this build computes no
    such gradient and therefore refuses them (``ValueError``) instead of returning none silently.

    ``last_terms`` is the forward's [12, b] block: the student's lse_img, diag_img, lse_txt, diag_txt, then the teacher's lse and the
    cross sum of the image strip and of the text strip, then the low parts of the four lse (ovhip.h)."""

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
        if not _collective(self):
            return (img, txt), (t_img, t_txt), (img, txt, t_img, t_txt), e, et, 0
        packed = gather_distill_features(img, txt, t_img, t_txt, self.world_size, self.group)
        views = unpack_distill_features(packed, e)
        if self.local_loss:
            x, u, off = (img, txt), (t_img, t_txt), b * self.rank
        else:                       # the global loss on every rank (loss.py:111-113): the local rows are the gathered rows
            x, u, off = (views[0].contiguous(), views[1].contiguous()), (views[2].contiguous(), views[3].contiguous()), 0
        return x, u, views, packed.shape[1], packed.shape[1], off

    def _launch(self, image_features, text_features, logit_scale, dist_image_features, dist_text_features, dist_logit_scale):
        """The forward, with or without grad: ((contrastive, distill), what the backward needs as tensors, (ld, ldt, label offset))."""
        lib = _lib.load()
        img, txt, t_img, t_txt = (t.detach().float().contiguous() for t in (image_features, text_features, dist_image_features,
                                                                             dist_text_features))
        dev = img.device
        scale, t_scale = _device_scalar(logit_scale, dev), _device_scalar(dist_logit_scale, dev)
        x, u, g, ld, ldt, off = self._operands(img, txt, t_img, t_txt)
        (b, e), et, n = x[0].shape, u[0].shape[1], g[0].shape[0]
        nbytes = lib.ov_distill_loss_workspace_bytes(b, n)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        terms = torch.empty(12, b, dtype=torch.float32, device=dev)
        check(lib.ov_distill_loss(ptr(x[0]), ptr(x[1]), ptr(g[0]), ptr(g[1]), ld, ptr(u[0]), ptr(u[1]), ptr(g[2]), ptr(g[3]), ldt, b, n, e,
                                  et, ptr(scale), ptr(t_scale), int(off), ptr(out[0:]), ptr(out[1:]), ptr(terms),
                                  ptr(self._ws.get(nbytes, dev)), nbytes, stream_ptr()), "ov_distill_loss")
        self.last_terms = terms
        return (out[0], out[1]), (*x, *u, *g, terms, scale, t_scale), (ld, ldt, off)

    def forward(self, image_features, text_features, logit_scale, dist_image_features, dist_text_features, dist_logit_scale,
                output_dict: bool = False):
        self._check(image_features, text_features, dist_image_features, dist_text_features, dist_logit_scale)
        args = (image_features, text_features, logit_scale, dist_image_features, dist_text_features, dist_logit_scale)
        if _needs_grad(image_features, text_features, logit_scale):
            c, d = _DistillClipLossFn.apply(self, image_features, text_features, _as_node_input(logit_scale, image_features.device),
                                            *args[3:])
        else:
            c, d = self._launch(*args)[0]
        return {"contrastive_loss": c, "distill_loss": d} if output_dict else (c, d)


class _DistillClipLossFn(torch.autograd.Function):
    """DistillClipLoss as an autograd node with two outputs.  forward = the module's launch; backward = ov_distill_loss_backward
    with both upstream gradients as device scalars, the student's gathered side written and routed as ``_InfoNCEFn`` does at
    C = 1.  The teacher inputs get None."""

    @staticmethod
    def forward(ctx, mod: DistillClipLoss, image_features, text_features, logit_scale, dist_image_features, dist_text_features,
                dist_logit_scale):
        (c, d), saved, ctx.lay = mod._launch(image_features, text_features, logit_scale, dist_image_features, dist_text_features,
                                             dist_logit_scale)
        ctx.mod, ctx.b, ctx.collective = mod, image_features.shape[0], _collective(mod)
        ctx.in_dtypes = (image_features.dtype, text_features.dtype, logit_scale.dtype)
        ctx.save_for_backward(*saved)
        return c, d

    @staticmethod
    def backward(ctx, grad_c, grad_d):
        mod: DistillClipLoss = ctx.mod
        x_img, x_txt, u_img, u_txt, y_img, y_txt, v_img, v_txt, terms, scale, t_scale = ctx.saved_tensors
        lib = _lib.load()
        (bx, e), et, n, dev = x_img.shape, u_img.shape[1], y_img.shape[0], x_img.device
        ld, ldt, off = ctx.lay
        d_local, d_all, (p_ai, p_at, ldg, _) = _backward_buffers(mod, ctx.collective, bx, n, e, 1, dev)
        d_scale = torch.empty(1, dtype=torch.float32, device=dev)
        g_c = grad_c.detach().float().reshape(1).contiguous()           # device scalars: no host round trip
        g_d = grad_d.detach().float().reshape(1).contiguous()
        nbytes = lib.ov_distill_loss_backward_workspace_bytes(bx, n)
        check(lib.ov_distill_loss_backward(ptr(x_img), ptr(x_txt), ptr(y_img), ptr(y_txt), ld, ptr(u_img), ptr(u_txt), ptr(v_img),
                                           ptr(v_txt), ldt, bx, n, e, et, ptr(scale), ptr(t_scale), off, ptr(terms), ptr(g_c), ptr(g_d),
                                           ptr(d_local), ptr(d_local[bx:]), p_ai, p_at, ldg, ptr(d_scale),
                                           ptr(mod._ws_bwd.get(nbytes, dev)), nbytes, stream_ptr()), "ov_distill_loss_backward")
        g_img, g_txt = _own_gradients(mod, ctx.collective, d_local, d_all, ctx.b, 1)
        dt_i, dt_t, dt_s = ctx.in_dtypes
        return None, g_img.to(dt_i), g_txt.to(dt_t), d_scale[0].to(dt_s), None, None, None
