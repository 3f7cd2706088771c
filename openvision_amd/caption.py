"""The caption branch of the reference trainer (``loss_type = 'coca'``, src/configs/openvision.py:292-294: total loss = contrastive +
2 x caption): a text decoder over the two towers' tokens and the masked softmax cross-entropy of its logits.

``TextDecoder`` follows src/models/text_decoder.py ``_Model`` (:436-576) in ``concat`` fusion with ``casual_mask=True``: bias-free
projections of the image and text tokens to the decoder width, ``[image | text | learnable tokens]`` through a stack of the towers' own
pre-LN blocks (tanh GELU) under the prefix-LM mask of text_transformer.py:418-442 -- key j visible to query i iff j < L_image + L_text
or j <= i, ``ov_attention_prefix`` -- then the last ``num_learnable_tokens`` positions through a LayerNorm and a bias-free vocabulary
head.  No positional embedding (the reference has none here).

Inference (``forward`` under ``torch.no_grad()``) runs the stack through ``ov_tower_forward``; with gradients use
``training.decode(decoder, image_tokens, text_tokens)`` / ``training.coca_forward``.  ``CaptionLoss`` is an autograd node over
``ov_softmax_xent`` / ``ov_softmax_xent_backward``.  There is no CPU / eager fallback.

Not provided: ``cross_attn`` fusion, the reference's two-caption batch halving (two_towers.py:95-97), conversion of ``txt_decoder/*``
weights, fp8 under a mask, a head GEMM fused with the cross-entropy."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import check, ptr, stream_ptr
from .model import LayerNorm, Linear, Transformer


class TextDecoder(nn.Module):
    def __init__(self, image_width: int, text_width: int, width: int, depth: int, heads: int, mlp_dim: int, vocab_size: int,
                 num_learnable_tokens: int = 128, eps: float = 1e-6):
        super().__init__()
        self.width, self.vocab_size, self.num_learnable_tokens = width, vocab_size, num_learnable_tokens
        self.image_projection = Linear(image_width, width, bias=False)
        self.text_projection = Linear(text_width, width, bias=False)
        self.learnable_tokens = nn.Parameter(torch.randn(num_learnable_tokens, width) * width ** -0.5)
        self.transformer = Transformer(width, depth, heads, (mlp_dim + 0.5) / width, act_kwargs={"approximate": "tanh"}, eps=eps)
        self.transformer._cache.fold_ln = False       # the module's own LayerNorms: the launches of the training forward, bit for bit
        self.decoder_norm = LayerNorm(width, eps=eps)
        self.head = Linear(width, vocab_size, bias=False)

    def forward(self, image_tokens: torch.Tensor, text_tokens: torch.Tensor) -> torch.Tensor:
        """image_tokens [B, L_image, image_width], text_tokens [B, L_text, text_width] -> fp32 logits [B, T_out, vocab_size].  No
        autograd graph is built here (inference); ``training.decode`` is the same computation with gradients."""
        from . import training
        with torch.no_grad():
            bsz, li, _ = image_tokens.shape
            lt = text_tokens.shape[1]
            w, n = self.width, self.num_learnable_tokens
            xi = training._LinearFn.apply(image_tokens.reshape(bsz * li, -1), self.image_projection.weight, None).view(bsz, li, w)
            xt = training._LinearFn.apply(text_tokens.reshape(bsz * lt, -1), self.text_projection.weight, None).view(bsz, lt, w)
            x = torch.cat([xi, xt, self.learnable_tokens.float().unsqueeze(0).expand(bsz, -1, -1)], dim=1)
            self.transformer.set_causal_prefix(li + lt)
            x = self.transformer(x)                                               # ov_tower_forward under the prefix-LM mask
            y = training._LayerNormFn.apply(x[:, -n:].contiguous(), self.decoder_norm.weight, self.decoder_norm.bias, self.decoder_norm.eps)
            return training._LinearFn.apply(y.reshape(bsz * n, w), self.head.weight, None).view(bsz, n, -1)


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, mask):
        lib = _lib.load()
        if not logits.is_cuda:
            raise _lib.OvhipError("CaptionLoss: tensors must live on an MI355X device (no CPU fallback)")
        v = logits.shape[-1]
        lg = logits.detach().float().reshape(-1, v).contiguous()
        lb = labels.detach().to(torch.int64).reshape(-1).contiguous()
        mk = mask.detach().float().reshape(-1).contiguous()
        r = lg.shape[0]
        if lb.numel() != r or mk.numel() != r:
            raise ValueError("CaptionLoss: labels and mask must have one entry per logits row")
        loss = torch.empty(1, dtype=torch.float32, device=lg.device)
        lse = torch.empty(r, dtype=torch.float32, device=lg.device)
        nb = lib.ov_softmax_xent_workspace_bytes(r)
        ws = torch.empty(nb, dtype=torch.uint8, device=lg.device)
        check(lib.ov_softmax_xent(ptr(lg), v, ptr(lb), ptr(mk), r, v, ptr(loss), ptr(lse), ptr(ws), nb, stream_ptr()), "ov_softmax_xent")
        ctx.save_for_backward(lg, lb, mk, lse)
        ctx.meta = (logits.shape, logits.dtype)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        lg, lb, mk, lse = ctx.saved_tensors
        shape, dt = ctx.meta
        r, v = lg.shape
        gd = g.detach().float().reshape(1).contiguous()
        d = torch.empty_like(lg)
        nb = lib.ov_softmax_xent_workspace_bytes(r)
        ws = torch.empty(nb, dtype=torch.uint8, device=lg.device)
        check(lib.ov_softmax_xent_backward(ptr(lg), v, ptr(lb), ptr(mk), ptr(lse), ptr(gd), ptr(d), v, r, v, ptr(ws), nb, stream_ptr()),
              "ov_softmax_xent_backward")
        return d.view(shape).to(dt), None, None


class CaptionLoss(nn.Module):
    """softmax_xent(logits, labels, reduction=True, mask) of the reference (src/losses/common.py:225-251; no smoothing):
    sum_r nll_r mask_r / (sum_r mask_r + 1e-8) over all positions r; a label outside [0, vocab) contributes 0."""

    def forward(self, logits: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        return _XentFn.apply(logits, labels, mask)
