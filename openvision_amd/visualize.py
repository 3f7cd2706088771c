"""Feature visualisation: the differentiable MLP-feature objective of ``ov-feature-visualization.py`` on the HIP path.

The reference script reads one hidden unit of one vision block's MLP through a forward hook on ``resblocks[layer].mlp.gelu``
(``ViTEnsFeatHook(ClipOVGeLUHook(model, sl=slice(layer, layer + 1)), key='high', feat=feature)``: ov-feature-visualization.py:211,
cliptoolsoptimized.py:990-999, 1149-1164) and back-propagates to the pixels.  Here GELU is fused into the c_fc epilogue, so the unit is
computed directly:

    x_l   = blocks[0 .. layer)(embed(image))                       ov_tower_forward_saving / ov_tower_backward_input
    x1    = x_l + out_proj(attn(ln_1(x_l)))                        ov_block_attn_forward_saving / ov_block_attn_backward_input
    m_b   = mean_{t >= 1} gelu(ln_2(x1) . W_fc[f] + b_fc[f])       ov_mlp_feature_forward / ov_mlp_feature_backward
    loss  = -(1 / B^2) sum_b m_b                                   (the reference's ``-all_feats[:B, f].diag().mean()``)

Blocks after ``layer`` do not change the value and are not run; nothing of the tap block's MLP but the one column is computed.  The
model's parameters are constants: the backward computes input gradients only and writes no ``.grad``.  The path is bf16 whatever
``set_precision`` says.  In the script, line 211 becomes ``loss += MLPFeatureLoss(premodel, layer, feature)``.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .training import _LinearFn, _pool

__all__ = ["mlp_feature", "MLPFeatureLoss"]


def _a256(n: int) -> int:
    return (n + 255) // 256 * 256


class _FeatureFn(torch.autograd.Function):
    """Blocks [0, layer), the tap block's attention half and the tap kernels as one autograd node: x [B, L, D] -> m [B] (fp32)."""

    @staticmethod
    def forward(ctx, visual, layer, feature, x):
        lib = _lib.load()
        tr = visual.transformer
        blocks = list(tr.resblocks)[:layer + 1]
        b0 = blocks[0]
        d, heads, mlp, mlp_pad = b0.attn.embed_dim, b0.attn.num_heads, b0.mlp_dim, b0.mlp_pad
        eps, tanh = float(b0.ln_2.eps), int(b0.gelu_tanh)
        bsz, seq, _ = x.shape
        m = bsz * seq
        pool = _pool(tr)
        xb = x.detach().to(torch.bfloat16).contiguous().clone()
        saved = tower = None
        if layer > 0:                                   # blocks [0, layer): xb becomes the tap block's input
            tower = tr._cache.get(blocks[:layer], plain=True)
            saved = pool.take(lib.ov_tower_saved_bytes(tower.handle, bsz, seq), x.device, "saved")
            nbytes = lib.ov_tower_workspace_bytes(tower.handle, bsz, seq)
            ws = pool.take(nbytes, x.device)
            check(lib.ov_tower_forward_saving(tower.handle, ptr(xb), ptr(saved), bsz, seq, ptr(ws), nbytes, stream_ptr()),
                  "ov_tower_forward_saving")
            pool.give(ws)
        # the tap block: qkv | attention out | x1 | lse | pre, one pooled buffer
        lp = (seq + 31) // 32 * 32
        offs, total = [], 0
        for n in (m * 3 * d * 2, m * d * 2, m * d * 2, bsz * heads * lp * 4, m * 4):
            offs.append(total)
            total += _a256(n)
        tap = pool.take(total, x.device, "featviz")
        base = tap.data_ptr()
        qkv, attn_out, x1, lse, pre = [C.c_void_p(base + o) for o in offs]
        cfg1 = _lib.TowerCfg(d, 1, heads, mlp, mlp_pad, tanh, float(b0.ln_1.eps))
        wt, keep = blocks[layer].packed_block(fold_ln=False)          # the tap block's own LayerNorms and weights, ov_block_weights order
        check(lib.ov_block_attn_forward_saving(C.byref(cfg1), C.byref(wt), ptr(xb), qkv, attn_out, x1, lse, bsz, seq, stream_ptr()),
              "ov_block_attn_forward_saving")
        fc_w, fc_b, ln2_w, ln2_b = keep[8], keep[9], keep[6], keep[7]
        mean = torch.empty(bsz, dtype=torch.float32, device=x.device)
        check(lib.ov_mlp_feature_forward(x1, d, ptr(ln2_w), ptr(ln2_b), ptr(fc_w), d, ptr(fc_b), feature, mlp, tanh, bsz, seq, d, eps, pre,
                                         ptr(mean), stream_ptr()), "ov_mlp_feature_forward")
        if not ctx.needs_input_grad[3]:                 # no backward will come: hand the buffers back now
            pool.give(tap)
            if saved is not None:
                pool.give(saved)
            return mean
        ctx.pool, ctx.tower, ctx.tap_weights, ctx.cfg1 = pool, tower, (wt, keep), cfg1       # the backward runs the forward's handle and weights
        ctx.meta = (layer, feature, bsz, seq, d, mlp, tanh, eps, offs)
        ctx.xb, ctx.tap, ctx.saved, ctx.x_dtype = xb, tap, saved, x.dtype
        ctx.gens = (tap._ovhip_gen, saved._ovhip_gen if saved is not None else None)
        return mean

    @staticmethod
    def backward(ctx, dmean):
        lib = _lib.load()
        layer, feature, bsz, seq, d, mlp, tanh, eps, offs = ctx.meta
        tap, saved, pool = ctx.tap, ctx.saved, ctx.pool
        if tap._ovhip_gen != ctx.gens[0] or (saved is not None and saved._ovhip_gen != ctx.gens[1]):
            raise _lib.OvhipError("feature objective: the saved activations of this graph were recycled by a later forward; a second "
                                  "backward over the same graph must come before the next forward")
        m = bsz * seq
        base = tap.data_ptr()
        qkv, attn_out, x1, lse, pre = [C.c_void_p(base + o) for o in offs]
        wt, keep = ctx.tap_weights
        handle = ctx.tower.handle if ctx.tower is not None else None
        dm = dmean.detach().float().contiguous()
        attn_bytes = lib.ov_block_attn_backward_input_workspace_bytes(C.byref(ctx.cfg1), bsz, seq)
        tower_bytes = lib.ov_tower_backward_input_workspace_bytes(handle, bsz, seq) if handle else 0
        if attn_bytes == 0 or (handle and tower_bytes == 0):
            raise _lib.OvhipError("feature objective: width % 64 == 0 and head_dim % 8 == 0, <= 96 are required")
        dx1_off = _a256(max(attn_bytes, tower_bytes))
        ws = pool.take(dx1_off + m * d * 2, dm.device)
        dx1 = C.c_void_p(ws.data_ptr() + dx1_off)
        dx = torch.empty(m, d, dtype=torch.bfloat16, device=dm.device)
        check(lib.ov_mlp_feature_backward(x1, d, ptr(keep[6]), ptr(keep[8]), d, feature, mlp, tanh, pre, ptr(dm), dx1, d, bsz, seq, d, eps,
                                          stream_ptr()), "ov_mlp_feature_backward")
        check(lib.ov_block_attn_backward_input(C.byref(ctx.cfg1), C.byref(wt), ptr(ctx.xb), qkv, attn_out, lse, dx1, ptr(dx), bsz, seq,
                                               ptr(ws), attn_bytes, stream_ptr()), "ov_block_attn_backward_input")
        if handle:
            check(lib.ov_tower_backward_input(handle, ptr(saved), ptr(dx), bsz, seq, ptr(ws), tower_bytes, stream_ptr()),
                  "ov_tower_backward_input")
        pool.give(ws)             # ordered on the stream: the next forward's writes come after this backward's reads
        pool.give(tap)
        if saved is not None:
            pool.give(saved)
        return None, None, None, dx.view(bsz, seq, d).to(ctx.x_dtype)


def _check_args(visual, image, layer: int, feature: int):
    pd = getattr(visual, "patch_dropout", None)
    if visual.training and float(getattr(pd, "prob", 0.0)) > 0:
        raise _lib.OvhipError(f"feature objective: the vision tower is in training mode with patch_dropout = {pd.prob}; the objective reads "
                              "every patch token and does not drop any -- call model.eval() (or visual.eval()) first")
    if not isinstance(visual.ln_pre, torch.nn.Identity):
        raise _lib.OvhipError("feature objective: ln_pre is Identity for OpenVision towers")
    blocks = list(visual.transformer.resblocks)
    if not 0 <= int(layer) < len(blocks):
        raise _lib.OvhipError(f"feature objective: layer {layer} outside [0, {len(blocks)})")
    mlp = blocks[0].mlp_dim
    if not 0 <= int(feature) < mlp:
        raise _lib.OvhipError(f"feature objective: feature {feature} outside [0, {mlp})")
    if not image.is_cuda:
        raise _lib.OvhipError("feature objective: tensors must live on an MI355X device (no CPU fallback)")
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError("image must be [B, 3, H, W]")


def mlp_feature(model, image: torch.Tensor, layer: int, feature: int) -> torch.Tensor:
    """m_b = mean over the patch tokens of GELU unit ``feature`` of vision block ``layer``'s MLP: fp32 [B], differentiable with respect
    to ``image`` ([B, 3, H, W], fp32 or bf16, on the device).  ``model``: a CLIP model or its ``visual`` tower."""
    visual = getattr(model, "visual", model)
    _check_args(visual, image, layer, feature)
    p = visual.patch_size[0]
    w = visual.conv1.weight.detach()
    bsz, _, hh, ww = image.shape
    gh, gw = hh // p, ww // p
    # conv1 (transformer.py:610-612) as patch rows times W^T, the weight a constant; cls + pos (:615-617); ln_pre = Identity
    patches = image.reshape(bsz, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(bsz * gh * gw, 3 * p * p)
    x = _LinearFn.apply(patches, w.reshape(w.shape[0], -1), None).view(bsz, gh * gw, -1)
    cls = visual.class_embedding.detach().float().expand(bsz, 1, -1)
    x = torch.cat([cls, x], dim=1) + visual.positional_embedding.detach().float()
    return _FeatureFn.apply(visual, int(layer), int(feature), x)


class MLPFeatureLoss:
    """``ViTEnsFeatHook(ClipOVGeLUHook(model, sl=slice(layer, layer + 1)), key='high', feat=feature, coefficient)`` with the surface of
    the reference's ``InvLoss`` (cliptoolsoptimized.py:636-654) that ``LossArray`` uses: ``loss(x) = -(1/B^2) sum_b m_b``,
    ``__call__`` returns ``coefficient * loss`` and records ``last_value``."""

    def __init__(self, model, layer: int, feature: int, coefficient: float = 1.0):
        self.model, self.layer, self.f, self.c = model, int(layer), int(feature), coefficient
        self.name = "MLPFeat"
        self.last_value = 0

    def loss(self, x: torch.Tensor) -> torch.Tensor:
        m = mlp_feature(self.model, x, self.layer, self.f)
        return -m.sum() / float(m.shape[0] * m.shape[0])          # -all_feats[:B, f].diag().mean(): a B x B matrix, B^2 entries

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        tensor = self.loss(x)
        self.last_value = tensor.item()
        return self.c * tensor

    def __str__(self) -> str:
        return f"{self.c * self.last_value:.4g}({self.last_value:.4g})"

    def reset(self):
        return 0
