"""Gradient accumulation for the InfoNCE: the full-batch contrastive loss over A micro-batches, exactly.

A contrastive loss cannot be accumulated by adding micro-batch losses: every row's softmax runs over the whole batch.  open_clip's
``--accum-freq`` therefore runs a no-grad pass that collects every micro-batch's features and then, per micro-batch, evaluates the
whole N x N loss with the fresh chunk spliced in.  Here the second pass costs one b x N strip per micro-batch instead:

  pass 1   ``add``         every micro-batch's features, detached, into a bank of N = A b rows (times the world size)
           ``close``       ONE forward over the bank (``ov_clip_loss_multi``): the loss and the two log-sum-exp vectors of every row
  pass 2   ``window_loss`` an autograd node per micro-batch whose backward is ``ov_clip_loss_window_backward``: with the bank and
                           its log-sum-exps fixed, the exact gradient of the full-batch loss with respect to the window's rows

The windows' gradients are the rows of the one-batch gradient, and their ``logit_scale`` shares sum to the one-batch gradient (the
spliced scheme adds the full ``logit_scale`` gradient once per micro-batch, so it arrives A times too large).

Data parallel (``world_size > 1``): one all-gather of every rank's packed ``[A b, (1 + C) E]`` rows, the local-strip forward on the
rank's own A b rows, one small all-gather of the ``[4 C, A b]`` terms.  No rank computes N x N and the backward needs no collective:
a window's gradient already holds what every other rank's rows contribute.  The loss is normalised by the rank's own A b rows, as under
``local_loss``, so the rank-AVERAGE of the parameter gradients is the global-batch gradient (``FusedAdamW.all_reduce_gradients`` and
``step(grad_scale=1 / world_size)`` unchanged).  That is the gradient of a differentiable gather, so the loss module must have
``gather_with_grad=True`` there.

``training.accumulated_step`` runs both passes through the towers."""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _lib
from ._lib import ptr, stream_ptr, check
from .loss import (DistillClipLoss, _InfoNCELoss, _all_gather_rows, _as_node_input, _collective, _device_scalar,
                   gather_caption_features)
from .model import _Workspace


class WindowLayout:
    """Where the windows of an accumulated batch lie in the bank: host-side bookkeeping only.  Every window has b rows; rank r's
    micro-batch j is window j of that rank and starts at bank row ``(r A + j) b``, A the number of windows per rank (known at
    ``close``)."""

    def __init__(self, num_captions: int = 1, rank: int = 0, world_size: int = 1):
        self.num_captions, self.rank, self.world_size = int(num_captions), int(rank), int(world_size)
        self.b = self.embed_dim = None
        self.windows = 0
        self.closed = False

    def validate(self, image_shape, text_shape) -> None:
        """What ``admit`` would refuse, without registering anything."""
        if self.closed:
            raise RuntimeError("ContrastiveAccumulator: add() after close(); reset() starts the next accumulated batch")
        c = self.num_captions
        if len(image_shape) != 2 or len(text_shape) != 2 or image_shape[1] != text_shape[1] or text_shape[0] != c * image_shape[0] \
                or image_shape[0] <= 0:
            raise ValueError(f"ContrastiveAccumulator: text_features must be [{c} * b, E] for image_features [b, E], got "
                             f"{tuple(text_shape)} for {tuple(image_shape)}")
        if self.b is not None and (int(image_shape[0]), int(image_shape[1])) != (self.b, self.embed_dim):
            raise ValueError(f"ContrastiveAccumulator: every window must be [{self.b}, {self.embed_dim}] like the first, got "
                             f"{tuple(image_shape)}")

    def admit(self, image_shape, text_shape) -> int:
        """Register one more window of features [b, E] / [C b, E]; returns its index."""
        self.validate(image_shape, text_shape)
        self.b, self.embed_dim = int(image_shape[0]), int(image_shape[1])
        self.windows += 1
        return self.windows - 1

    def close(self) -> None:
        if self.closed:
            raise RuntimeError("ContrastiveAccumulator: close() twice; reset() starts the next accumulated batch")
        if not self.windows:
            raise RuntimeError("ContrastiveAccumulator: close() with no window added")
        self.closed = True

    @property
    def local_rows(self) -> int:
        """A b: the rows of this rank, and the number of rows its loss is the mean over."""
        return self.windows * self.b

    @property
    def bank_rows(self) -> int:
        return self.world_size * self.local_rows

    def start(self, j: int, rank: Optional[int] = None) -> int:
        """The first bank row of window j of ``rank`` (default: this rank)."""
        if not 0 <= j < self.windows:
            raise IndexError(f"window {j} outside [0, {self.windows})")
        return ((self.rank if rank is None else rank) * self.windows + j) * self.b


class ContrastiveAccumulator:
    """The bank, its forward and the per-window autograd node for a ``ClipLoss`` or ``MultiCaptionClipLoss`` (C, rank, world_size and
    group are read from it).  ``SigLipLoss`` and ``DistillClipLoss`` are not covered (``TypeError``)."""

    def __init__(self, loss):
        if isinstance(loss, DistillClipLoss) or not isinstance(loss, _InfoNCELoss):
            raise TypeError(f"ContrastiveAccumulator: needs a ClipLoss or MultiCaptionClipLoss, got {type(loss).__name__}")
        if loss.world_size > 1 and not loss.gather_with_grad:
            raise ValueError("ContrastiveAccumulator: under data parallelism the window gradient is that of a differentiable gather; "
                             "construct the loss with gather_with_grad=True")
        self.loss = loss
        self._ws = _Workspace()
        self.reset()

    def reset(self) -> None:
        """Forget the bank: ready for the next accumulated batch."""
        mod = self.loss
        self.layout = WindowLayout(mod.num_captions, mod.rank, mod.world_size)
        self._chunks: List[tuple] = []
        self._bank = None            # (all_img, all_txt, ld, set_stride) once closed
        self.terms: Optional[torch.Tensor] = None          # [4 C, N]
        self._scale = None

    def add(self, image_features: torch.Tensor, text_features: torch.Tensor) -> int:
        """Pass 1: a detached fp32 copy of one micro-batch's features ([b, E], [C b, E]) goes into the bank; returns its window index."""
        lay = self.layout
        lay.validate(image_features.shape, text_features.shape)     # state and shape errors before the device check
        if not (image_features.is_cuda and text_features.is_cuda):
            raise _lib.OvhipError("ContrastiveAccumulator: features must live on an MI355X device (no CPU fallback)")
        j = lay.admit(image_features.shape, text_features.shape)
        self._chunks.append((image_features.detach().float().clone(), text_features.detach().float().clone()))
        return j

    def close(self, logit_scale) -> torch.Tensor:
        """The bank's forward.  Returns this rank's loss (device scalar, no grad): the full-batch InfoNCE in a world of one, the
        mean over the rank's own A b rows under data parallelism.  Keeps ``terms`` [4 C, N] for the windows."""
        lay, mod = self.layout, self.loss
        lay.close()
        lib = _lib.load()
        c, b, e, a = lay.num_captions, lay.b, lay.embed_dim, lay.windows
        rows, dev = lay.local_rows, self._chunks[0][0].device
        # this rank's rows in the features' own layout: [A b, E] and the sets stacked [C A b, E] (set c in rows c A b ...)
        x_img = torch.cat([ch[0] for ch in self._chunks], dim=0)
        x_txt = torch.cat([ch[1][s * b:(s + 1) * b] for s in range(c) for ch in self._chunks], dim=0)
        self._chunks = []
        scale = _device_scalar(logit_scale, dev).clone()
        if _collective(mod):
            packed = gather_caption_features(x_img, x_txt, c, mod.world_size, mod.group)          # [N, (1 + C) E], rank order
            all_img, all_txt, ld, ss, off = packed, packed[:, e:], (1 + c) * e, e, mod.rank * rows
        else:
            all_img, all_txt, ld, ss, off = x_img, x_txt, e, rows * e, 0
        n = all_img.shape[0]
        nbytes = lib.ov_clip_loss_multi_workspace_bytes(rows, n, c)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        terms = torch.empty(4 * c, rows, dtype=torch.float32, device=dev)
        check(lib.ov_clip_loss_multi(ptr(x_img), ptr(x_txt), ptr(all_img), ptr(all_txt), ld, ss, rows, n, e, c, ptr(scale), int(off),
                                     ptr(out), ptr(terms), ptr(self._ws.get(nbytes, dev)), nbytes, stream_ptr()), "ov_clip_loss_multi")
        if _collective(mod):          # every rank's [4 C, A b] terms -> [4 C, N]: rows travel, so transpose around the gather
            terms = _all_gather_rows(terms.t().contiguous(), mod.world_size, mod.group).t().contiguous()
        self._bank, self.terms, self._scale = (all_img, all_txt, ld, ss), terms, scale
        assert n == lay.bank_rows and a * b == rows
        return out[0]

    def window_rows(self, j: int):
        """The bank's own rows of window j of this rank: (image [b, E], text [C b, E]), copies."""
        if self._bank is None:
            raise RuntimeError("ContrastiveAccumulator: close() comes before the windows")
        all_img, all_txt, ld, ss = self._bank
        lay = self.layout
        w0, b, e, c = lay.start(j), lay.b, lay.embed_dim, lay.num_captions
        if ld == e:                                                   # separate arrays: set s in rows s N ...
            n = lay.bank_rows
            return all_img[w0:w0 + b].clone(), torch.cat([all_txt[s * n + w0:s * n + w0 + b] for s in range(c)], dim=0)
        return all_img[w0:w0 + b, :e].clone(), torch.cat([all_txt[w0:w0 + b, s * e:(s + 1) * e] for s in range(c)], dim=0)

    def window_loss(self, j: int, image_features: torch.Tensor, text_features: torch.Tensor, logit_scale, check: bool = False):
        """Pass 2: window j's share of the loss as an autograd node.  The shares of a rank's windows sum to what ``close`` returned;
        the backward is one ``ov_clip_loss_window_backward`` and returns the exact gradient of the full-batch loss with respect to
        ``image_features``, ``text_features`` and ``logit_scale`` (the window's share), evaluated on the BANK's values: the features
        handed in must be the ones ``add`` saw (recompute them with the same operators).  ``check=True`` raises unless they are,
        bitwise; that costs one host synchronisation and is meant for tests and debugging."""
        if self._bank is None:
            raise RuntimeError("ContrastiveAccumulator: close() comes before the windows")
        lay = self.layout
        lay.start(j)
        c, b, e = lay.num_captions, lay.b, lay.embed_dim
        if tuple(image_features.shape) != (b, e) or tuple(text_features.shape) != (c * b, e):
            raise ValueError(f"ContrastiveAccumulator: window features must be [{b}, {e}] and [{c * b}, {e}], got "
                             f"{tuple(image_features.shape)} and {tuple(text_features.shape)}")
        if not (image_features.is_cuda and text_features.is_cuda):
            raise _lib.OvhipError("ContrastiveAccumulator: features must live on an MI355X device (no CPU fallback)")
        if check:
            w_img, w_txt = self.window_rows(j)
            if not (torch.equal(image_features.detach().float(), w_img) and torch.equal(text_features.detach().float(), w_txt)):
                raise _lib.OvhipError(f"ContrastiveAccumulator: the features of window {j} are not bitwise the rows add() stored: the "
                                      "second pass must recompute the first pass's features")
        return _WindowFn.apply(self, j, image_features, text_features, _as_node_input(logit_scale, image_features.device))


class _WindowFn(torch.autograd.Function):
    """One window of ``ContrastiveAccumulator``.  forward = the window's share of the loss, read from ``terms``; backward =
    ov_clip_loss_window_backward over the bank."""

    @staticmethod
    def forward(ctx, acc: ContrastiveAccumulator, j, image_features, text_features, logit_scale):
        lay = acc.layout
        c, b, n = lay.num_captions, lay.b, lay.bank_rows
        w0 = lay.start(j)
        t = acc.terms.view(c, 4, n)[:, :, w0:w0 + b]                  # per set lse_img, diag_img, lse_txt, diag_txt of the window
        ctx.acc, ctx.w0, ctx.bank, ctx.terms, ctx.scale = acc, w0, acc._bank, acc.terms, acc._scale
        ctx.dims = (b, n, lay.embed_dim, c, lay.local_rows)
        ctx.in_dtypes = (image_features.dtype, text_features.dtype, logit_scale.dtype)
        return ((t[:, 0] - t[:, 1]) + (t[:, 2] - t[:, 3])).sum() / (2.0 * c * lay.local_rows)

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        all_img, all_txt, ld, ss = ctx.bank
        b, n, e, c, norm_rows = ctx.dims
        dev = all_img.device
        d_img = torch.empty(b, e, dtype=torch.float32, device=dev)
        d_txt = torch.empty(c * b, e, dtype=torch.float32, device=dev)
        d_scale = torch.empty(1, dtype=torch.float32, device=dev)
        grad = grad_out.detach().float().reshape(1).contiguous()        # device scalar: no host round trip
        nbytes = lib.ov_clip_loss_window_backward_workspace_bytes(b, n, c)
        check(lib.ov_clip_loss_window_backward(ptr(all_img), ptr(all_txt), ld, ss, n, e, c, ptr(ctx.scale), ptr(ctx.terms), ptr(grad),
                                               ctx.w0, b, norm_rows, ptr(d_img), ptr(d_txt), ptr(d_scale),
                                               ptr(ctx.acc._ws.get(nbytes, dev)), nbytes, stream_ptr()), "ov_clip_loss_window_backward")
        dt_i, dt_t, dt_s = ctx.in_dtypes
        return None, None, d_img.to(dt_i), d_txt.to(dt_t), d_scale[0].to(dt_s)
