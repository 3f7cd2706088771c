"""MI355X-native counterpart of the reference's ``open_clip.model.CLIP`` for OpenVision configs.

Same constructor, attribute tree, state-dict keys and methods as the reference
(``src/convert_upload/open_clip/model.py:220-315``, ``transformer.py:210-265,319-366,434-651``), so that
``ov-zero-shot-test.py``-style callers (which walk ``model.visual.conv1 / .ln_pre / .transformer / .ln_post /
.proj`` and ``model.token_embedding / .transformer / .ln_final / .text_projection``) run unchanged — but every
module's ``forward`` enqueues hand-written gfx950 kernels through the C ABI of ``libovhip.so``.

Precision: the HIP path computes like the reference's 'bf16' mode (``factory.py:259,275-296``): bf16 weights and
activations with fp32 accumulation, LayerNorm statistics / affine, biases and the returned embeddings in fp32.
Parameters stay ordinary ``nn.Parameter``s (fp32 by default) so ``load_state_dict`` / ``.to()`` / ``.float()``
behave as usual; bf16 device copies in the kernels' packed layout are rebuilt lazily when a parameter changes.

These entry points are the inference path: they never build an autograd graph and their outputs have ``requires_grad=False``;
the training step with gradients is ``openvision_amd.training``.
There is NO CPU / eager fallback: calling any forward with CPU tensors, or without libovhip.so, raises.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import types
from collections import OrderedDict
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import OV_BF16, OV_F32, EPI_BIAS, EPI_GELU_ERF, EPI_GELU_TANH, EPI_RESIDUAL, ptr, stream_ptr, check
from . import posembed
from .config import (CLIPVisionCfg, CLIPTextCfg, POS_EMBED_TYPES, vision_cfg_from, text_cfg_from, gelu_is_tanh, ln_eps,
                     mlp_width, attn_pool_head_dim)

MAX_MICRO_BATCH = 1024          # encode_* split larger batches so the workspace stays bounded


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.OvhipError(f"{what}: expected a tensor on an MI355X device, got {t.device}. "
                              f"openvision_amd has no CPU fallback (the reference CPU path lives in oracle/ for tests).")


def _dtype_flag(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return OV_F32
    if t.dtype == torch.bfloat16:
        return OV_BF16
    raise TypeError(f"unsupported dtype {t.dtype} (float32 or bfloat16)")


def _gemm_bias(a, lda: int, w, ldw: int, bias, out, ldo: int, m: int, n: int, k: int, stream, what: str = "ov_gemm") -> None:
    """out [m, n] = a [m, k] w [n, k]^T (+ bias fp32 [n], or None) on ov_gemm: pointers and row pitches of bf16 operands padded already."""
    check(_lib.load().ov_gemm(a, lda, w, ldw, bias, out, ldo, m, n, k, EPI_BIAS, None, 0, 0, 0, 0, stream), what)


def _kernel_input(t: torch.Tensor) -> torch.Tensor:
    """t as the kernels read it: contiguous, in float32 or bfloat16 (any other dtype is converted to float32)."""
    return t.contiguous() if t.dtype in (torch.float32, torch.bfloat16) else t.float().contiguous()


class _Workspace:
    """Grow-only device scratch buffer, one per module tree and device."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.gen = 0            # bumped on every reallocation: captured hipGraphs hold the OLD buffer's address (_GraphCache)

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.device != device or self.buf.numel() < nbytes:
            self.buf = None
            self.buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
            self.gen += 1
        return self.buf


_PACK_EPOCH = [0]        # bumped by invalidate_packed(): every _Packed signature carries it


class _Packed:
    """Cache of packed device tensors keyed by the source parameters' (data_ptr, version).  Writes that bypass autograd's
    version counter (``p.data.copy_()``, ``p.data.mul_()``, EMA / weight surgery through ``.data``) are NOT seen: call
    ``invalidate_packed()`` (or ``CLIP.invalidate_packed()``) after them.  ``load_state_dict`` does it by itself."""

    def __init__(self):
        self.sig = None
        self.val = None

    def get(self, params, builder, extra=None):
        sig = (extra, _PACK_EPOCH[0]) + tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in params)
        if sig != self.sig:
            with torch.no_grad():
                self.val = builder()
            self.sig = sig
        return self.val


def invalidate_packed() -> None:
    """Drop every packed / folded / quantised device copy of every model in this process; they are rebuilt on next use."""
    _PACK_EPOCH[0] += 1


class _GraphCache:
    """hipGraph replay of a launch-bound encode call (batch-1 zero-shot path: ~170 kernel launches per image whose host-side
    launch cost exceeds their device time).  The launch sequence is captured ONCE per (shape, dtype, flags) on a capture stream
    (every kernel of libovhip goes to the current torch stream, so torch.cuda.graph records them as graph kernel nodes), then
    replayed: copy the input into the captured call's static input, one hipGraphLaunch, clone the static output.  Weights AND the
    grow-only workspaces are baked in as pointers: `sig_fn()` covers both (pack epoch, parameter versions, workspace generations);
    when it changes -- a parameter update, or a larger call (graphed or not) that made a workspace reallocate, after which the
    old buffer may belong to somebody else -- every graph is dropped and re-captured on next use."""

    def __init__(self):
        self.graphs = {}
        self.sig = None

    def run(self, key, sig_fn, x: torch.Tensor, fn):
        if self.sig != sig_fn():
            self.graphs.clear()
        ent = self.graphs.get(key)
        if ent is None:
            static_in = x.clone()
            fn(static_in)                                   # warm-up outside capture: packs weights, sizes workspaces, sets attributes
            torch.cuda.current_stream(x.device).synchronize()
            if self.sig != sig_fn():                        # the warm-up itself grew a workspace: the other graphs hold stale pointers
                self.graphs.clear()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_out = fn(static_in)
            ent = self.graphs[key] = (g, static_in, static_out)
            self.sig = sig_fn()
        g, static_in, static_out = ent
        static_in.copy_(x)
        g.replay()
        return static_out.clone()


def _pack_matrix(w: torch.Tensor, n_pad: int, k_pad: int) -> torch.Tensor:
    """[N,K] any float dtype -> zero-padded bf16 [n_pad, k_pad], contiguous.  Nothing to pad: one cast, no zero fill and no second copy
    (a block's weights are re-packed after every optimiser step)."""
    n, k = w.shape
    if (n, k) == (n_pad, k_pad):
        return w.detach().to(torch.bfloat16).contiguous()
    out = torch.zeros(n_pad, k_pad, dtype=torch.bfloat16, device=w.device)
    out[:n, :k] = w.detach()                   # the copy rounds as .to(torch.bfloat16) does
    return out


def _pack_vec(v: Optional[torch.Tensor], n_pad: int, device) -> torch.Tensor:
    """fp32 [n_pad], zero behind v's entries (all zero without v); an fp32 vector of that length is used as it lies."""
    if v is not None and v.numel() == n_pad:
        return v.detach().float().contiguous()
    out = torch.zeros(n_pad, dtype=torch.float32, device=device)
    if v is not None:
        out[: v.numel()] = v.detach().float()
    return out


# ------------------------------------------------------------------------------------------------------
# leaf modules
# ------------------------------------------------------------------------------------------------------
class LayerNorm(nn.LayerNorm):
    """transformer.py:24-30 / :15-21 — fp32 statistics, output cast back to the input dtype."""

    def __init__(self, normalized_shape, eps: float = 1e-6):
        super().__init__(normalized_shape, eps=eps)
        self._pk = _Packed()

    def packed(self) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._pk.get((self.weight, self.bias),
                            lambda: (self.weight.detach().float().contiguous(), self.bias.detach().float().contiguous()))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _require_cuda(x, "LayerNorm")
        d = self.normalized_shape[0]
        if x.shape[-1] != d:
            raise ValueError(f"LayerNorm: last dim {x.shape[-1]} != {d}")
        lib = _lib.load()
        xin = _kernel_input(x).view(-1, d)
        y = torch.empty_like(xin)
        g, b = self.packed()
        check(lib.ov_layernorm(ptr(xin), _dtype_flag(xin), d, ptr(g), ptr(b), ptr(y), _dtype_flag(y), d,
                               xin.shape[0], d, float(self.eps), stream_ptr()), "ov_layernorm")
        return y.view(x.shape).to(x.dtype)


class Linear(nn.Module):
    """Parameter holder with nn.Linear's attribute names; forward = ov_gemm (+bias)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        nn.init.normal_(self.weight, std=in_features ** -0.5)
        if bias:
            nn.init.zeros_(self.bias)
        self._pk = _Packed()

    def packed(self, n_pad: Optional[int] = None, k_pad: Optional[int] = None):
        n_pad = n_pad or _round_up(self.out_features, 8)
        k_pad = k_pad or _round_up(self.in_features, 64)
        ps = (self.weight,) if self.bias is None else (self.weight, self.bias)
        return self._pk.get(ps, lambda: (_pack_matrix(self.weight, n_pad, k_pad),
                                         _pack_vec(self.bias, n_pad, self.weight.device)), extra=(n_pad, k_pad))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _require_cuda(x, "Linear")
        k = self.in_features
        w, b = self.packed()
        n_pad, k_pad = w.shape
        a = x.reshape(-1, k).to(torch.bfloat16)
        if k_pad != k:
            a = torch.nn.functional.pad(a, (0, k_pad - k))
        a = a.contiguous()
        out = torch.empty(a.shape[0], n_pad, dtype=torch.bfloat16, device=x.device)
        _gemm_bias(ptr(a), k_pad, ptr(w), k_pad, ptr(b), ptr(out), n_pad, a.shape[0], n_pad, k_pad, stream_ptr())
        return out[:, : self.out_features].reshape(*x.shape[:-1], self.out_features).to(x.dtype)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}"


class GELU(nn.GELU):
    """Marker module (``mlp.gelu``): inside a block the activation is fused into the c_fc GEMM epilogue."""

    def forward(self, x):  # pragma: no cover - never on the product path
        raise _lib.OvhipError("GELU is fused into the c_fc GEMM epilogue on the HIP path; call the block or the mlp's "
                              "parent, not mlp.gelu directly")


class MultiheadAttention(nn.Module):
    """Parameter layout of nn.MultiheadAttention(batch_first=True) (packed in_proj, out_proj) — transformer.py:225."""

    def __init__(self, embed_dim: int, num_heads: int):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.batch_first = True
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = Linear(embed_dim, embed_dim, bias=True)
        nn.init.normal_(self.in_proj_weight, std=embed_dim ** -0.5)
        self._pk = _Packed()

    def packed_in(self):
        d = self.embed_dim
        return self._pk.get((self.in_proj_weight, self.in_proj_bias),
                            lambda: (_pack_matrix(self.in_proj_weight, 3 * d, _round_up(d, 64)),
                                     _pack_vec(self.in_proj_bias, 3 * d, self.in_proj_weight.device)))


class PoolAttention(nn.Module):
    """Parameter layout of ``nn.MultiheadAttention(embed_dim, num_heads, kdim=kdim, vdim=kdim, batch_first=True)``: the packed
    ``in_proj_weight`` [3E, E] when kdim == embed_dim, else ``q_proj_weight`` [E, E], ``k_proj_weight`` and ``v_proj_weight`` [E, kdim];
    ``in_proj_bias`` [3E] and ``out_proj`` in both.  The layout not in use is registered as None, as torch does."""

    def __init__(self, embed_dim: int, num_heads: int, kdim: int):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim, self.kdim = embed_dim, num_heads, embed_dim // num_heads, kdim
        self.batch_first = True
        self._qkv_same_embed_dim = kdim == embed_dim
        if self._qkv_same_embed_dim:
            self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
            nn.init.normal_(self.in_proj_weight, std=embed_dim ** -0.5)
            for n in ("q_proj_weight", "k_proj_weight", "v_proj_weight"):
                self.register_parameter(n, None)
        else:
            self.q_proj_weight = nn.Parameter(torch.empty(embed_dim, embed_dim))
            self.k_proj_weight = nn.Parameter(torch.empty(embed_dim, kdim))
            self.v_proj_weight = nn.Parameter(torch.empty(embed_dim, kdim))
            for w in (self.q_proj_weight, self.k_proj_weight, self.v_proj_weight):
                nn.init.normal_(w, std=w.shape[1] ** -0.5)
            self.register_parameter("in_proj_weight", None)
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = Linear(embed_dim, embed_dim, bias=True)

    def weight_params(self):
        return (self.in_proj_weight,) if self._qkv_same_embed_dim else (self.q_proj_weight, self.k_proj_weight, self.v_proj_weight)

    def q_weight(self) -> torch.Tensor:
        """[E, E]: the query projection (a view of the packed matrix in that layout)."""
        return self.in_proj_weight[: self.embed_dim] if self._qkv_same_embed_dim else self.q_proj_weight

    def kv_weight(self) -> torch.Tensor:
        """[2E, kdim]: the key rows above the value rows, the K | V column blocks ``ov_attn_pool`` reads."""
        if self._qkv_same_embed_dim:
            return self.in_proj_weight[self.embed_dim:]
        return torch.cat([self.k_proj_weight, self.v_proj_weight], dim=0)


class AttentionalPooler(nn.Module):
    """transformer.py:187-207: ``n_queries`` learned queries, shared by every image, attend to the tokens of each image:
    ``MultiheadAttention(d_model, n_head, kdim=context_dim)(ln_q(query) expanded over B, ln_k(x), ln_k(x))`` -> [B, n_queries, d_model].
    Both LayerNorms have the class default eps 1e-5, whatever the tower's ``norm_kwargs`` say (the reference passes them none).

    The parameters and their state-dict names are the reference's, in both layouts of ``nn.MultiheadAttention`` (``PoolAttention``).
    On the HIP path: ln_k and the K | V projection GEMM over all tokens, ``ov_attn_pool``, the out_proj GEMM.  The projected queries
    ``ln_q(query) Wq^T + bq`` do not depend on the input: they are computed once and cached with the packed weights (``_Packed``)."""

    def __init__(self, d_model: int, context_dim: int, n_head: int = 8, n_queries: int = 256):
        super().__init__()
        attn_pool_head_dim(d_model, n_head)
        if not 1 <= n_queries <= 256:
            raise ValueError(f"attentional pool: n_queries {n_queries} outside [1, 256]")
        if context_dim % 64:
            raise ValueError(f"attentional pool: context width {context_dim} must be a multiple of 64")
        self.query = nn.Parameter(torch.randn(n_queries, d_model))
        self.attn = PoolAttention(d_model, n_head, context_dim)
        self.ln_q = LayerNorm(d_model, eps=1e-5)
        self.ln_k = LayerNorm(context_dim, eps=1e-5)
        self._pk = _Packed()
        self._ws = _Workspace()

    def packed(self):
        """(projected queries [n_q, E] bf16, K | V weight [2E, context] bf16, K | V bias [2E] fp32, out_proj weight [E, E padded to 64]
        bf16, out_proj bias fp32)."""
        a = self.attn
        e, nq = a.embed_dim, self.query.shape[0]
        kp = _round_up(e, 64)

        def build():
            lib, st, dev = _lib.load(), stream_ptr(), self.query.device
            g, b = self.ln_q.packed()
            qsrc = self.query.detach().float().contiguous()
            qn = torch.zeros(nq, kp, dtype=torch.bfloat16, device=dev)
            check(lib.ov_layernorm(ptr(qsrc), OV_F32, e, ptr(g), ptr(b), ptr(qn), OV_BF16, kp, nq, e, float(self.ln_q.eps), st), "ov_layernorm(ln_q)")
            bias = a.in_proj_bias.detach().float()
            wq = _pack_matrix(a.q_weight(), e, kp)
            qp = torch.empty(nq, e, dtype=torch.bfloat16, device=dev)
            _gemm_bias(ptr(qn), kp, ptr(wq), kp, ptr(bias[:e].contiguous()), ptr(qp), e, nq, e, kp, st, "ov_gemm(pool q)")
            wkv = _pack_matrix(a.kv_weight(), 2 * e, a.kdim)
            wo, bo = a.out_proj.packed(e, kp)
            return qp, wkv, bias[e:].contiguous(), wo, bo
        return self._pk.get((self.query, self.ln_q.weight, self.ln_q.bias, *a.weight_params(), a.in_proj_bias, a.out_proj.weight,
                             a.out_proj.bias), build)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, L, context_dim] (any L >= 1) -> [B, n_queries, d_model] bf16."""
        _require_cuda(x, "AttentionalPooler")
        a = self.attn
        if x.dim() != 3 or x.shape[2] != a.kdim:
            raise ValueError(f"expected [batch, tokens, {a.kdim}], got {tuple(x.shape)}")
        lib, st = _lib.load(), stream_ptr()
        bsz, seq, d = x.shape
        e, nq, kp = a.embed_dim, self.query.shape[0], _round_up(a.embed_dim, 64)
        qp, wkv, bkv, wo, bo = self.packed()
        xb = x.detach().to(torch.bfloat16).contiguous().view(bsz * seq, d)
        g, b = self.ln_k.packed()
        xk = torch.empty_like(xb)
        check(lib.ov_layernorm(ptr(xb), OV_BF16, d, ptr(g), ptr(b), ptr(xk), OV_BF16, d, bsz * seq, d, float(self.ln_k.eps), st), "ov_layernorm(ln_k)")
        kv = torch.empty(bsz * seq, 2 * e, dtype=torch.bfloat16, device=x.device)
        _gemm_bias(ptr(xk), d, ptr(wkv), d, ptr(bkv), ptr(kv), 2 * e, bsz * seq, 2 * e, d, st, "ov_gemm(pool kv)")
        # the out_proj GEMM reads rows padded to its 64-column granule: ov_attn_pool writes into the wider pitch
        o = torch.zeros(bsz * nq, kp, dtype=torch.bfloat16, device=x.device) if kp != e else torch.empty(bsz * nq, e, dtype=torch.bfloat16, device=x.device)
        check(lib.ov_attn_pool(ptr(qp), e, ptr(kv), 2 * e, ptr(o), kp, None, bsz, seq, nq, a.num_heads, a.head_dim, a.head_dim ** -0.5, st),
              "ov_attn_pool")
        y = torch.empty(bsz * nq, e, dtype=torch.bfloat16, device=x.device)
        _gemm_bias(ptr(o), kp, ptr(wo), kp, ptr(bo), ptr(y), e, bsz * nq, e, kp, st, "ov_gemm(pool out_proj)")
        return y.view(bsz, nq, e)


class PatchConv(nn.Module):
    """conv1: Conv2d(3, width, kernel = stride = P, bias=False) (transformer.py:469) as im2col + MFMA GEMM."""

    def __init__(self, width: int, patch: int):
        super().__init__()
        self.in_channels, self.out_channels = 3, width
        self.kernel_size = self.stride = (patch, patch)
        self.weight = nn.Parameter(torch.empty(width, 3, patch, patch))
        nn.init.normal_(self.weight, std=(3 * patch * patch) ** -0.5)
        self.bias = None
        self._pk = _Packed()

    @property
    def kpad(self) -> int:
        return _round_up(3 * self.kernel_size[0] ** 2, 64)

    def packed(self) -> torch.Tensor:
        return self._pk.get((self.weight,), lambda: _pack_matrix(self.weight.reshape(self.out_channels, -1),
                                                                 self.out_channels, self.kpad))

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        """[B,3,S,S] -> [B, width, g, g] (what nn.Conv2d returns; ov-zero-shot-test.py:105)."""
        _require_cuda(image, "conv1")
        lib = _lib.load()
        p = self.kernel_size[0]
        bsz, _, s, _ = image.shape
        g = s // p
        img = _kernel_input(image)
        cols = torch.empty(bsz * g * g, self.kpad, dtype=torch.bfloat16, device=image.device)
        check(lib.ov_im2col_patches(ptr(img), _dtype_flag(img), ptr(cols), bsz, s, p, self.kpad, stream_ptr()), "ov_im2col")
        w = self.packed()
        out = torch.empty(bsz * g * g, self.out_channels, dtype=torch.bfloat16, device=image.device)
        _gemm_bias(ptr(cols), self.kpad, ptr(w), self.kpad, None, ptr(out), self.out_channels, bsz * g * g, self.out_channels, self.kpad,
                   stream_ptr(), "ov_gemm(conv1)")
        return out.view(bsz, g, g, self.out_channels).permute(0, 3, 1, 2).to(image.dtype)


class Embedding(nn.Embedding):
    """token_embedding.  As a stand-alone call it is a pure row gather (index_select, no arithmetic);
    ``CLIP.encode_text`` uses the fused HIP gather + pos-emb add instead."""

    def __init__(self, num_embeddings: int, embedding_dim: int):
        super().__init__(num_embeddings, embedding_dim)
        self._pk = _Packed()

    def packed(self) -> torch.Tensor:
        return self._pk.get((self.weight,), lambda: self.weight.detach().to(torch.bfloat16).contiguous())

    def forward(self, tokens: torch.Tensor) -> torch.Tensor:
        _require_cuda(tokens, "token_embedding")
        return self.weight.detach().index_select(0, tokens.reshape(-1)).view(*tokens.shape, -1)


# ------------------------------------------------------------------------------------------------------
# transformer
# ------------------------------------------------------------------------------------------------------
class ResidualAttentionBlock(nn.Module):
    """transformer.py:210-265 with ls_1 = ls_2 = Identity and no cross-attention."""

    def __init__(self, d_model: int, n_head: int, mlp_ratio: float = 4.0, act_kwargs: Optional[dict] = None,
                 eps: float = 1e-6):
        super().__init__()
        self.ln_1 = LayerNorm(d_model, eps=eps)
        self.attn = MultiheadAttention(d_model, n_head)
        self.ls_1 = nn.Identity()
        self.ln_2 = LayerNorm(d_model, eps=eps)
        mlp = mlp_width(d_model, mlp_ratio)
        self.mlp = nn.Sequential(OrderedDict([
            ("c_fc", Linear(d_model, mlp)),
            ("gelu", GELU(**(act_kwargs or {}))),
            ("c_proj", Linear(mlp, d_model)),
        ]))
        self.ls_2 = nn.Identity()
        self.gelu_tanh = gelu_is_tanh(act_kwargs)
        self.mlp_dim, self.mlp_pad = mlp, _round_up(mlp, 64)
        self._fold_pk = _Packed()
        self._fp8_pk = _Packed()

    def packed_block(self, fold_ln: bool = True):
        """Device weights of this block in the kernels' layout.  With ``fold_ln`` (default; ``OVHIP_NO_LN_FOLD=1`` disables)
        ln_1 / ln_2 are folded into the QKV / c_fc GEMMs: W' = bf16(gamma * W), colsum = sum_k W', cvec = beta @ W^T + b
        (see ov_gemm_ln in include/ovhip.h); the LayerNorm output is never materialised."""
        d = self.attn.embed_dim
        dev = self.attn.in_proj_weight.device
        g1, b1 = self.ln_1.packed()
        g2, b2 = self.ln_2.packed()
        wo, bo = self.attn.out_proj.packed(d, _round_up(d, 64))
        wp, bp = self.mlp.c_proj.packed(d, self.mlp_pad)
        if not fold_ln:
            wq, bq = self.attn.packed_in()
            wf, bf = self.mlp.c_fc.packed(self.mlp_pad, _round_up(d, 64))
            keep = (g1, b1, wq, bq, wo, bo, g2, b2, wf, bf, wp, bp)
            return _lib.BlockWeights(*[C.c_void_p(t.data_ptr()) for t in keep], None, None), keep

        def fold(w, b, gamma, beta, n_pad):
            w32 = w.detach().float()
            wg = _pack_matrix(w32 * gamma[None, :], n_pad, _round_up(d, 64))          # bf16(gamma * W), zero padded
            colsum = wg.float().sum(dim=1).contiguous()                               # sums of the ROUNDED weights
            cvec = _pack_vec((w32.to(torch.bfloat16).float() @ beta) + (b.detach().float() if b is not None else 0.0),
                             n_pad, dev)
            return wg, cvec, colsum

        key = (self.ln_1.weight, self.ln_1.bias, self.ln_2.weight, self.ln_2.bias, self.attn.in_proj_weight,
               self.attn.in_proj_bias, self.mlp.c_fc.weight, self.mlp.c_fc.bias)
        wq, cq, sq, wf, cf, sf = self._fold_pk.get(key, lambda: fold(self.attn.in_proj_weight, self.attn.in_proj_bias, g1, b1, 3 * d)
                                                    + fold(self.mlp.c_fc.weight, self.mlp.c_fc.bias, g2, b2, self.mlp_pad))
        keep = (g1, b1, wq, cq, wo, bo, g2, b2, wf, cf, wp, bp, sq, sf)
        return _lib.BlockWeights(*[C.c_void_p(t.data_ptr()) for t in keep]), keep

    def packed_block_fp8(self):
        """fp8 (OCP e4m3) copies of the four weight matrices for the fp8 path (BASELINE.json config #5): per-output-row absmax
        scaling (scale = max|w_row| / 448), zero padding as in the bf16 layout; biases as the module holds them."""
        d = self.attn.embed_dim
        dev = self.attn.in_proj_weight.device

        def q8(w, n_pad, k_pad):
            w32 = torch.zeros(n_pad, k_pad, dtype=torch.float32, device=dev)
            w32[: w.shape[0], : w.shape[1]] = w.detach().float()
            scale = (w32.abs().amax(dim=1) / 448.0).clamp_min(1e-30)
            return (w32 / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).contiguous(), scale.contiguous()

        def build():
            wq, sq = q8(self.attn.in_proj_weight, 3 * d, d)
            wo, so = q8(self.attn.out_proj.weight, d, d)
            wf, sf = q8(self.mlp.c_fc.weight, self.mlp_pad, d)
            wp, sp = q8(self.mlp.c_proj.weight, d, self.mlp_pad)
            bq = _pack_vec(self.attn.in_proj_bias, 3 * d, dev)
            bf = _pack_vec(self.mlp.c_fc.bias, self.mlp_pad, dev)
            return (wq, sq, bq, wo, so, wf, sf, bf, wp, sp)

        key = (self.attn.in_proj_weight, self.attn.in_proj_bias, self.attn.out_proj.weight, self.mlp.c_fc.weight,
               self.mlp.c_fc.bias, self.mlp.c_proj.weight)
        keep = self._fp8_pk.get(key, build)
        return _lib.BlockFp8(*[C.c_void_p(t.data_ptr()) for t in keep]), keep

    def forward(self, q_x: torch.Tensor, k_x=None, v_x=None, attn_mask=None, causal_prefix: Optional[int] = None) -> torch.Tensor:
        if k_x is not None or v_x is not None or attn_mask is not None:
            raise NotImplementedError("OpenVision blocks are unmasked self-attention (no k_x/v_x/attn_mask)")
        return _run_blocks([self], q_x, prefix=causal_prefix)


class _TowerHandle:
    """ov_tower handle + the packed tensors it borrows (kept alive here: `keep[i]` are block i's, in ov_block_weights order), its
    `cfg`, and the library object that created it, through which it is destroyed."""

    def __init__(self, blocks, fp8: bool = False, mask=None, prefix: Optional[int] = None, fold_ln: bool = True):
        self.lib = lib = _lib.load()
        if prefix is not None and fp8:
            raise _lib.OvhipError("a causal prefix needs bf16 precision (no fp8 under an attention mask)")
        b0 = blocks[0]
        d = b0.attn.embed_dim
        if d % 64:
            raise _lib.OvhipError(f"width {d} must be a multiple of 64 for the gfx950 kernels")
        self.cfg = cfg = _lib.TowerCfg(d, len(blocks), b0.attn.num_heads, b0.mlp_dim, b0.mlp_pad, int(b0.gelu_tanh), float(b0.ln_1.eps))
        self.handle = lib.ov_tower_create(C.byref(cfg))
        if not self.handle:
            raise _lib.OvhipError("ov_tower_create failed (invalid tower configuration)")
        self.keep, self.keep8 = [], []
        for i, blk in enumerate(blocks):
            bw, keep = blk.packed_block(fold_ln=fold_ln and os.environ.get("OVHIP_NO_LN_FOLD", "0") != "1")
            self.keep.append(keep)
            check(lib.ov_tower_set_block(self.handle, i, C.byref(bw)), "ov_tower_set_block")
            if fp8:
                b8, keep8 = blk.packed_block_fp8()
                self.keep8.append(keep8)
                check(lib.ov_tower_set_block_fp8(self.handle, i, C.byref(b8)), "ov_tower_set_block_fp8")
        self.width, self.layers, self.fp8 = d, len(blocks), fp8
        self.prefix = prefix
        if prefix is not None:              # every block's attention: key j visible to query i iff j < prefix or j <= i
            check(lib.ov_tower_set_prefix(self.handle, int(prefix)), "ov_tower_set_prefix")
        self.h_amax = None
        self.mask = [FP8_ALL] * len(blocks) if mask is None else list(mask)
        if fp8 and mask is not None:
            m8 = (C.c_ubyte * len(blocks))(*self.mask)
            check(lib.ov_tower_set_fp8_mask(self.handle, m8, len(blocks)), "ov_tower_set_fp8_mask")
        if fp8:
            # per-layer running maxima of the MLP hidden and of the attention output: recorded while they are quantised row by row
            # (mode 1), then the static scales of the fused c_fc -> c_proj and attention -> out_proj hand-overs (mode 2)
            # [hidden | attention out] maxima behind the scales, then the same two sets as recorded by the running forward
            self.h_amax = torch.zeros(4 * len(blocks), dtype=torch.float32, device=b0.attn.in_proj_weight.device)
            check(lib.ov_tower_set_fp8_hidden_scale(self.handle, ptr(self.h_amax), 1), "ov_tower_set_fp8_hidden_scale")

    def freeze_fp8_scales(self, delayed: bool = True) -> None:
        if not self.fp8:
            raise _lib.OvhipError("freeze_fp8_scales: the tower is not in fp8 precision")
        need = [(m & FP8_FC) and (m & FP8_PROJ) for m in self.mask] + [bool(m & FP8_OUT) for m in self.mask]   # scales the mask uses
        seen = (self.h_amax[: 2 * self.layers] > 0).tolist()
        if any(n and not s_ for n, s_ in zip(need, seen)):
            raise _lib.OvhipError("freeze_fp8_scales: run at least one forward in fp8 precision first (calibration)")
        check(self.lib.ov_tower_set_fp8_hidden_scale(self.handle, ptr(self.h_amax), 2 if delayed else 3), "ov_tower_set_fp8_hidden_scale")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.ov_tower_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def _block_params(blocks):
    ps = []
    for b in blocks:
        ps.extend(p for p in b.parameters())
    return ps


FP8_QKV, FP8_OUT, FP8_FC, FP8_PROJ, FP8_ALL = 1, 2, 4, 8, 15      # ovhip.h OV_FP8_*: which GEMMs of a block take e4m3 operands
PRECISIONS = ("bf16", "fp8", "fp8-mixed")


def fp8_mixed_mask(layers: int):
    """The "fp8-mixed" recipe (BASELINE.json config #5 inside a stated tolerance; DESIGN.md section 7, profiles/r03_fp8_ablation.md):
    e4m3 operands where the per-GEMM ablation showed them cheap in accuracy and rich in time -- the two MLP products (c_fc -> c_proj, the
    hidden handed over in e4m3 with a static scale) -- and bf16 for the attention projections (QKV, out_proj), whose quantisation is
    what moves the embeddings on ill-conditioned ('sharp') weights.  OVHIP_FP8_MIXED_MASK (an OV_FP8_* bit set) overrides it."""
    m = int(os.environ.get("OVHIP_FP8_MIXED_MASK", str(FP8_FC | FP8_PROJ)))
    return [m & FP8_ALL] * layers


def default_precision() -> str:
    """GEMM operand precision of the block stacks: "bf16" (default), "fp8" (OVHIP_PRECISION=fp8; e4m3 weights and activations on the
    MX-scaled MFMA for all four GEMMs of a block, BASELINE.json config #5) or "fp8-mixed" (fp8_mixed_mask)."""
    p = os.environ.get("OVHIP_PRECISION", "bf16").lower()
    if p not in PRECISIONS:
        raise ValueError(f"OVHIP_PRECISION={p!r}: expected one of {PRECISIONS}")
    return p


class _TowerCache:
    """The one place tower handles are built: inference, the autograd nodes of ``openvision_amd.training`` and the feature objective
    of ``openvision_amd.visualize`` all take theirs here.  One entry per span of blocks (index of its first block, count) and form
    (fp8, fold_ln), each rebuilt on its own when a parameter under it, the pack epoch, the fp8 mask or the prefix changes (``_Packed``);
    so inference and training of one tower, the chunks of ``set_backward_chunk_layers`` and the [0, layer) spans of feature visualisation
    do not evict each other.  The per-leaf packed tensors below the handles are shared between the forms.  Whoever still holds a replaced
    ``_TowerHandle`` (an autograd ctx) keeps it, and the weights it was built from, alive; it is destroyed with its last holder."""

    def __init__(self):
        self._entries = {}           # (first block, count, fp8, fold_ln) -> _Packed of a _TowerHandle
        self.precision = default_precision()
        self.mask = None             # explicit per-layer OV_FP8_* masks (set_fp8_mask); None = what the precision name implies
        self.fold_ln = True          # False: the module's own LayerNorms and weights, the launches of the training forward (caption decoder)

    def get(self, blocks, prefix: Optional[int] = None, first: int = 0, plain: bool = False) -> _TowerHandle:
        """The handle over `blocks` (`first`: the index of blocks[0] in its tower).  `plain`: bf16 over the module's own LayerNorms and
        weights whatever `precision` and `fold_ln` say -- the form training and feature visualisation are defined on."""
        fp8 = not plain and self.precision != "bf16"
        fold_ln = not plain and self.fold_ln
        mask = None
        if fp8:
            mask = self.mask if self.mask is not None else (fp8_mixed_mask(len(blocks)) if self.precision == "fp8-mixed" else None)
            if mask is not None and len(mask) != len(blocks):
                mask = (list(mask) + [mask[-1]] * len(blocks))[: len(blocks)]        # sub-stacks (exploded forward): layer-wise prefix
        entry = self._entries.setdefault((first, len(blocks), fp8, fold_ln), _Packed())
        return entry.get(_block_params(blocks), lambda: _TowerHandle(blocks, fp8=fp8, mask=mask, prefix=prefix, fold_ln=fold_ln),
                         extra=(None if mask is None else tuple(mask), prefix))


def _check_prefix(prefix: Optional[int], seq: Optional[int] = None) -> Optional[int]:
    if prefix is None:
        return None
    prefix = int(prefix)
    if prefix < 0 or (seq is not None and prefix > seq):
        raise ValueError(f"causal prefix {prefix} outside [0, {seq if seq is not None else 'L'}]")
    return prefix


def _run_blocks(blocks, x: torch.Tensor, cache: Optional[_TowerCache] = None, ws: Optional[_Workspace] = None,
                prefix: Optional[int] = None):
    """x [B, L, D] (fp32 or bf16, cuda) -> same shape/dtype after the given blocks (ov_tower_forward).  prefix: None = unmasked
    attention, else the prefix-causal mask of ov_attention_prefix in every block."""
    _require_cuda(x, "Transformer")
    if x.dim() != 3:
        raise ValueError("expected [batch, tokens, width]")
    lib = _lib.load()
    tower = (cache or _TowerCache()).get(blocks, _check_prefix(prefix, x.shape[1]))
    bsz, seq, d = x.shape
    if d != tower.width:
        raise ValueError(f"width {d} != {tower.width}")
    xb = x.detach().to(torch.bfloat16).contiguous().clone() if x.dtype == torch.bfloat16 else x.detach().to(torch.bfloat16).contiguous()
    nbytes = lib.ov_tower_workspace_bytes(tower.handle, bsz, seq)
    wsb = (ws or _Workspace()).get(nbytes, x.device)
    check(lib.ov_tower_forward(tower.handle, ptr(xb), bsz, seq, ptr(wsb), nbytes, stream_ptr()), "ov_tower_forward")
    return xb.to(x.dtype)


class Transformer(nn.Module):
    """transformer.py:319-366."""

    def __init__(self, width: int, layers: int, heads: int, mlp_ratio: float = 4.0, act_kwargs: Optional[dict] = None,
                 eps: float = 1e-6, batch_first: bool = True):
        super().__init__()
        self.width, self.layers, self.batch_first = width, layers, batch_first
        self.grad_checkpointing = False
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads, mlp_ratio, act_kwargs, eps)
                                        for _ in range(layers)])
        self._cache = _TowerCache()
        self._ws = _Workspace()
        self.causal_prefix: Optional[int] = None      # None = unmasked; see set_causal_prefix
        self._causal_mask = None                      # see adopt_causal_mask
        self.drop_path: float = 0.0                   # stochastic depth rate of the training path; see set_drop_path

    def set_drop_path(self, rate: float = 0.0) -> None:
        """Stochastic depth of the training path (the reference's ``drop_path``, vit.py:358 / text_transformer.py:533-536): block i of
        n drops each of its two residual branches per sample with probability ``linspace(0, rate, n)[i]``.  ``rate`` in [0, 1).  Only
        ``openvision_amd.training`` reads it, and only in training mode; every inference path ignores it."""
        rate = float(rate)
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"drop_path rate {rate} outside [0, 1)")
        self.drop_path = rate

    def set_causal_prefix(self, prefix: Optional[int]) -> None:
        """Attention mask of every block: None (default) = unmasked; an int P >= 0 = prefix-causal, key j is visible to query i iff
        j < P or j <= i (P = 0: causal; the text decoder runs its stack with P = image tokens + text tokens).  bf16 precision only."""
        self.causal_prefix = _check_prefix(prefix)

    def get_cast_dtype(self) -> torch.dtype:
        return self.resblocks[0].mlp.c_fc.weight.dtype          # transformer.py:350-353

    def tower(self) -> _TowerHandle:
        return self._cache.get(list(self.resblocks), self.causal_prefix)

    def set_precision(self, precision: str, mask=None) -> None:
        """"bf16", "fp8" (all four GEMMs of every block in e4m3) or "fp8-mixed" (fp8_mixed_mask); `mask`: an OV_FP8_* bit set for
        every layer, or one per layer, instead of what the name implies.  The tower is packed for it on next use; the bf16 and the fp8
        handle are separate entries of the cache, so coming back to fp8 with the same mask and weights finds its recorded maxima."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}")
        if mask is not None and precision == "bf16":
            raise ValueError("an fp8 mask needs an fp8 precision")
        self._cache.precision = precision
        self._cache.mask = None if mask is None else ([int(mask)] * self.layers if isinstance(mask, int) else [int(v) for v in mask])

    def freeze_fp8_scales(self, delayed: bool = True) -> None:
        """fp8 precision: after at least one forward (which records the per-layer maximum of the MLP hidden), switch c_fc -> c_proj to
        the fused hand-over with a static scale (2 x the recorded maximum / 448) -- no bf16 round trip of the hidden.  delayed=True
        (training-style): every forward first rolls the maxima recorded by the previous one into the scales (they only grow, and a
        changed scale re-rounds every e4m3 value downstream: results are then NOT bitwise repeatable from call to call);
        delayed=False (serving): the scales stay as they are: repeatable and independent of the batch composition."""
        self.tower().freeze_fp8_scales(delayed)

    def adopt_causal_mask(self, mask: Optional[torch.Tensor]) -> None:
        """The owning model's causal ``attn_mask`` buffer: the one tensor ``forward(x, attn_mask=...)`` accepts.  The owner adopts
        it again whenever ``.to()`` / ``.cuda()`` replace the buffer (``CLIP._apply``)."""
        self._causal_mask = mask

    def _is_own_causal_mask(self, attn_mask: torch.Tensor) -> bool:
        """attn_mask is the adopted buffer: same storage, offset, shape and strides -- no device read."""
        own = self._causal_mask
        return (own is not None and isinstance(attn_mask, torch.Tensor) and attn_mask.dtype == own.dtype
                and attn_mask.device == own.device and attn_mask.shape == own.shape and attn_mask.stride() == own.stride()
                and attn_mask.storage_offset() == own.storage_offset()
                and attn_mask.untyped_storage().data_ptr() == own.untyped_storage().data_ptr())

    def forward(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        prefix = self.causal_prefix
        if attn_mask is not None:
            # an arbitrary additive mask is not built; the owning CLIP's causal buffer (model.attn_mask, the exploded forward of
            # ov-zero-shot-test.py:103-155) is the mask of prefix 0
            if not self._is_own_causal_mask(attn_mask):
                raise NotImplementedError("attn_mask: only the owning model's causal `attn_mask` buffer is accepted (it runs as "
                                          "set_causal_prefix(0)); arbitrary additive masks are not built")
            if x.dim() == 3 and x.shape[1] > attn_mask.shape[0]:
                raise ValueError(f"sequence of {x.shape[1]} tokens under a causal mask for {attn_mask.shape[0]}")
            prefix = 0
        return _run_blocks(list(self.resblocks), x, self._cache, self._ws, prefix)


class PatchDropout(nn.Module):
    """PatchDropout (transformer.py:49-86, FLIP arXiv 2212.00794) with ``exclude_first_token=True``, as VisionTransformer builds it: in
    training mode each image keeps ``K = max(1, int(G * (1 - prob)))`` of its G patch tokens, those of the K largest entries of
    ``torch.randn(B, G)`` drawn from the CPU default generator, in ``topk`` order, behind its CLS token.  In eval mode nothing is drawn.

    ``sample`` is that draw on its own (int64 [B, K]); the HIP paths of ``VisionTransformer`` / ``CLIP`` / ``training.encode_image`` take
    it and run the tower on the kept tokens only.  ``forward`` is the reference module on a token tensor [B, 1 + G, D].  No parameters."""

    def __init__(self, prob: float, exclude_first_token: bool = True):
        super().__init__()
        if not 0 <= prob < 1.:
            raise ValueError(f"patch dropout probability must lie in [0, 1), got {prob!r}")
        if not exclude_first_token:
            raise NotImplementedError("VisionTransformer always excludes the CLS token from patch dropout")
        self.prob = float(prob)
        self.exclude_first_token = exclude_first_token

    def num_keep(self, num_tokens: int) -> int:
        return max(1, int(num_tokens * (1 - self.prob)))

    def sample(self, batch: int, num_tokens: int) -> torch.Tensor:
        """The reference's draw: int64 [batch, K] patch indices on the CPU (consumes the CPU default generator)."""
        rand = torch.randn(batch, num_tokens)
        return rand.topk(self.num_keep(num_tokens), dim=-1).indices

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training or self.prob == 0.:
            return x
        cls_tokens, x = x[:, :1], x[:, 1:]
        keep = self.sample(x.shape[0], x.shape[1]).to(x.device)
        x = x[torch.arange(x.shape[0], device=x.device)[:, None], keep]
        return torch.cat((cls_tokens, x), dim=1)


def check_keep(keep: torch.Tensor, batch: int, num_patches: int) -> None:
    """Host-side shape check of a patch-keep table [batch, K], 1 <= K <= num_patches (index values are checked on the device)."""
    if not isinstance(keep, torch.Tensor) or keep.dim() != 2 or keep.shape[0] != batch:
        raise ValueError(f"keep must be an integer tensor [{batch}, K], got {getattr(keep, 'shape', type(keep))}")
    if keep.is_floating_point() or keep.is_complex() or keep.dtype == torch.bool:
        raise ValueError(f"keep must hold integer patch indices, got {keep.dtype}")
    if not 1 <= keep.shape[1] <= num_patches:
        raise ValueError(f"keep: K = {keep.shape[1]} outside [1, {num_patches}]")


def keep_to_device(keep: torch.Tensor, device) -> torch.Tensor:
    """int32 copy of a keep table on `device`.  From the CPU through pinned memory and a non_blocking copy: the host does not wait."""
    k = keep.detach().to(torch.int32)
    if k.device.type == "cpu" and torch.device(device).type == "cuda":
        return k.contiguous().pin_memory().to(device, non_blocking=True)
    return k.to(device).contiguous()


class VisionTransformer(nn.Module):
    """transformer.py:434-651 restricted to what OpenVision and the stock open_clip towers instantiate, the bool form of
    ``attentional_pool`` (the open_clip CoCa pooler) included: then ``attn_pool`` is an ``AttentionalPooler`` over all tokens of the
    block stack, ``ln_post`` and ``proj`` have ``output_dim`` rows, and ``final_ln_after_pool`` is not consulted (:636-640;
    ``config.vision_cfg_from`` refuses the pooler together with ``final_ln_after_pool=true``)."""

    def __init__(self, image_size: int, patch_size: int, width: int, layers: int, heads: int, mlp_ratio: float,
                 output_dim: int, pool_type: str = "avg", final_ln_after_pool: bool = True, no_ln_pre: bool = True,
                 act_kwargs: Optional[dict] = None, eps: float = 1e-6, output_tokens: bool = False,
                 patch_dropout: float = 0.0, pos_embed_type: str = "learnable", attentional_pool: bool = False,
                 attn_pooler_queries: int = 256, attn_pooler_heads: int = 8):
        super().__init__()
        if pos_embed_type not in POS_EMBED_TYPES:
            raise ValueError(f"pos_embed_type {pos_embed_type!r}: expected one of {POS_EMBED_TYPES}")
        self.pos_embed_type = pos_embed_type
        self.output_tokens = output_tokens
        self.image_size = (image_size, image_size)
        self.patch_size = (patch_size, patch_size)
        self.grid_size = (image_size // patch_size, image_size // patch_size)
        self.final_ln_after_pool = final_ln_after_pool
        self.output_dim = output_dim
        self.conv1 = PatchConv(width, patch_size)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        if pos_embed_type == "learnable":
            self.positional_embedding = nn.Parameter(scale * torch.randn(self.grid_size[0] * self.grid_size[1] + 1, width))
        else:
            # transformer.py:477-484: a fixed table under the same name, in the state dict, never trained.  'sin_cos_2d' is the
            # reference's MAE form, 'sincos2d' the recipe's MoCo-v3 form (posembed.py)
            self.positional_embedding = nn.Parameter(posembed.fixed_table(pos_embed_type, self.grid_size[0], width),
                                                     requires_grad=False)
        # transformer.py:481: dropout only when p > 0 (the module has no parameters: the state dict is the same either way)
        self.patch_dropout = PatchDropout(patch_dropout) if patch_dropout > 0. else nn.Identity()
        self.ln_pre = nn.Identity() if no_ln_pre else LayerNorm(width, eps=eps)
        self.transformer = Transformer(width, layers, heads, mlp_ratio, act_kwargs, eps)
        if attentional_pool not in (False, True, None):
            raise ValueError(f"attentional_pool={attentional_pool!r}: only the bool form is built")
        self.attn_pool = AttentionalPooler(output_dim, width, n_head=attn_pooler_heads, n_queries=attn_pooler_queries) if attentional_pool else None
        pool_dim = output_dim if attentional_pool else width
        self.pool_type = pool_type
        self.ln_post = LayerNorm(pool_dim, eps=eps)
        self.proj = nn.Parameter(scale * torch.randn(pool_dim, output_dim))
        self._pk = _Packed()
        self._pool_pk = _Packed()
        self._ws = _Workspace()

    # -- packed head -----------------------------------------------------------------------------------
    def _head(self):
        def build():
            dev = self.proj.device
            pos32 = self.positional_embedding.detach().float().contiguous()
            keep = dict(conv=self.conv1.packed(), cls=self.class_embedding.detach().float().contiguous(),
                        pos=pos32.to(torch.bfloat16).contiguous(), pos32=pos32, ln=self.ln_post.packed(),
                        proj_t=self.proj.detach().t().to(torch.bfloat16).contiguous())
            e = self.output_dim
            if e % 8:
                raise _lib.OvhipError("embed_dim must be a multiple of 8")
            h = _lib.VisionHead(self.image_size[0], self.patch_size[0], self.conv1.kpad, int(self.pool_type == "avg"),
                                int(self.final_ln_after_pool), e, e, ptr(keep["conv"]), ptr(keep["cls"]), ptr(keep["pos"]),
                                ptr(keep["pos32"]), ptr(keep["ln"][0]), ptr(keep["ln"][1]), ptr(keep["proj_t"]))
            return h, keep
        return self._pk.get((self.conv1.weight, self.class_embedding, self.positional_embedding, self.ln_post.weight,
                             self.ln_post.bias, self.proj), build)

    def set_grad_checkpointing(self, enable=True):
        """transformer.py:596: recompute this tower's block intermediates in the training backward (see CLIP.set_grad_checkpointing)."""
        self.transformer.grad_checkpointing = enable

    def lock(self, unlocked_groups: int = 0, freeze_bn_stats: bool = False) -> None:
        """LiT locking (transformer.py:542-572): freeze the whole tower, then train again the last ``unlocked_groups`` of its
        parameter groups (``_lock_groups``).  ``freeze_bn_stats`` is accepted and has no effect, as in the reference (there is no
        BatchNorm).  Frozen parameters get no gradient from ``openvision_amd.training``, which then skips their work.

        The reference names no parameter of the attentional pooler in any group (transformer.py:542-573): ``lock`` freezes the
        pooler and no ``unlocked_groups`` value trains it again.  That is mirrored here."""
        self.requires_grad_(False)
        if unlocked_groups:
            for group in self._lock_groups()[-unlocked_groups:]:
                for p in group:
                    p.requires_grad_(True)

    def _lock_groups(self):
        """Parameters of the locking groups, input side first: the patch embedding with class / positional embeddings and ln_pre,
        one group per block, the last block together with ln_post, and the output projection."""
        blocks = list(self.transformer.resblocks)
        # a fixed sin-cos table (transformer.py:481-482: requires_grad=False from birth) is in no group: unlocking never trains it
        pos = [self.positional_embedding] if self.pos_embed_type == "learnable" else []
        embed = [*self.conv1.parameters(), self.class_embedding, *pos, *self.ln_pre.parameters()]
        top = [*blocks[-1].parameters(), *self.ln_post.parameters()]
        return [embed] + [list(b.parameters()) for b in blocks[:-1]] + [top, [self.proj]]

    def set_input_size(self, image_size: int) -> None:
        """Run this tower at another resolution (the stages of the reference's recipe: 84 -> 224 -> 336 px): ``image_size`` is a
        square size in pixels, a positive multiple of the patch size, else ValueError.  Updates ``image_size``, ``grid_size`` and the
        position table:

        * a fixed table ('sin_cos_2d' / 'sincos2d') is regenerated for the new grid (vit.py:922-927), bitwise the table of a model
          built at that size;
        * a 'learnable' one is resampled as ``posembed.resize_pos_embed`` does on load (bicubic, antialiased, class row kept).

        The table arithmetic is host work: a model that lives on the device is resized through ONE host round trip of the table (a
        few MB at most), nothing else moves.  The new table is a NEW ``nn.Parameter`` with the old one's ``requires_grad``, dtype
        and device; packed copies and captured graphs are dropped and rebuilt on next use.  An optimiser built before the call
        still holds the old parameter: build the optimiser of a stage AFTER ``set_input_size`` (as the recipe does, whose
        ``ft_from`` carries parameters only, no optimiser state)."""
        p = self.patch_size[0]
        if isinstance(image_size, bool) or not isinstance(image_size, int) or image_size <= 0 or image_size % p:
            raise ValueError(f"set_input_size: expected a square size as an int, a positive multiple of the patch size {p}, "
                             f"got {image_size!r}")
        g = image_size // p
        old = self.positional_embedding
        if g * g + 1 != old.shape[0]:
            if self.pos_embed_type == "learnable":
                sd = {"visual.positional_embedding": old.detach().float().cpu()}
                posembed.resize_pos_embed(sd, types.SimpleNamespace(visual=types.SimpleNamespace(grid_size=(g, g))))
                table = sd["visual.positional_embedding"]
            else:
                table = posembed.fixed_table(self.pos_embed_type, g, old.shape[1])
            self.positional_embedding = nn.Parameter(table.to(device=old.device, dtype=old.dtype).contiguous(),
                                                     requires_grad=old.requires_grad)
        self.image_size, self.grid_size = (image_size, image_size), (g, g)
        invalidate_packed()          # the head bakes the image size and the table's address in; graphs hold both

    def _check_image(self, x: torch.Tensor):
        _require_cuda(x, "VisionTransformer")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != self.image_size[0] or x.shape[3] != self.image_size[1]:
            raise ValueError(f"expected [B,3,{self.image_size[0]},{self.image_size[1]}], got {tuple(x.shape)}")

    @property
    def num_patches(self) -> int:
        return self.grid_size[0] * self.grid_size[1]

    def dropout_active(self) -> bool:
        """Patch dropout applies to the next forward: training mode and p > 0 (transformer.py:61)."""
        return self.training and isinstance(self.patch_dropout, PatchDropout) and self.patch_dropout.prob > 0

    def _draw_keep(self, bsz: int, device) -> torch.Tensor:
        return keep_to_device(self.patch_dropout.sample(bsz, self.num_patches), device)

    def _encode(self, x: torch.Tensor, normalize: bool, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Image features [B, output_dim].  keep (int32 device table [B, K]; drawn here when patch dropout is active): the tower runs on
        the kept patches only, L' = 1 + K tokens per image."""
        self._check_image(x)
        if keep is None and self.dropout_active():
            keep = self._draw_keep(x.shape[0], x.device)
        lib = _lib.load()
        head, _keep = self._head()
        tower = self.transformer.tower()
        img = _kernel_input(x.detach())
        bsz = img.shape[0]
        out = torch.empty(bsz, self.output_dim, dtype=torch.float32, device=x.device)
        st = stream_ptr()
        for b0 in range(0, bsz, MAX_MICRO_BATCH):
            nb = min(MAX_MICRO_BATCH, bsz - b0)
            kb = None if keep is None else keep[b0:b0 + nb]
            if self.attn_pool is not None:
                # the pooler reads every token of the full stack: no last-block shortcut, no fused head
                tok = self.transformer(self.ln_pre(self._embed_tokens(img[b0:b0 + nb], kb)))
                out[b0:b0 + nb] = self._pooled_head(tok, normalize)[0]
            elif not isinstance(self.ln_pre, nn.Identity):
                tok = self._embed_tokens(img[b0:b0 + nb], kb)
                tok = self.transformer(self.ln_pre(tok))
                out[b0:b0 + nb] = self._head_forward(tok, normalize)
            elif kb is None:
                nbytes = lib.ov_vision_workspace_bytes(tower.handle, C.byref(head), nb)
                ws = self._ws.get(nbytes, x.device)
                check(lib.ov_encode_image(tower.handle, C.byref(head), ptr(img[b0:]), _dtype_flag(img), nb, ptr(out[b0:]),
                                          int(normalize), ptr(ws), nbytes, st), "ov_encode_image")
            else:
                nk = kb.shape[1]
                nbytes = lib.ov_vision_keep_workspace_bytes(tower.handle, C.byref(head), nb, nk)
                ws = self._ws.get(nbytes, x.device)
                check(lib.ov_encode_image_keep(tower.handle, C.byref(head), ptr(img[b0:]), _dtype_flag(img), ptr(kb), nb, nk, ptr(out[b0:]),
                                               int(normalize), None, ptr(ws), nbytes, st), "ov_encode_image_keep")
        return out

    def _embed_tokens(self, img: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Tokens [B, L, D] bf16; keep (patch dropout): the kept patches' tokens, in keep order, behind the CLS token."""
        lib = _lib.load()
        head, _ = self._head()
        tower = self.transformer.tower()
        bsz = img.shape[0]
        nk = 0 if keep is None else keep.shape[1]
        tok = torch.empty(bsz, 1 + (nk or self.num_patches), tower.width, dtype=torch.bfloat16, device=img.device)
        nbytes = lib.ov_vision_embed_workspace_bytes(tower.handle, C.byref(head), bsz, nk)
        ws = self._ws.get(nbytes, img.device)
        if keep is not None:
            check(lib.ov_vision_embed_keep(tower.handle, C.byref(head), ptr(img), _dtype_flag(img), ptr(keep), bsz, nk, ptr(tok), None,
                                           ptr(ws), nbytes, stream_ptr()), "ov_vision_embed_keep")
        else:
            check(lib.ov_vision_embed(tower.handle, C.byref(head), ptr(img), _dtype_flag(img), bsz, ptr(tok), ptr(ws), nbytes,
                                      stream_ptr()), "ov_vision_embed")
        return tok

    def _head_forward(self, tok: torch.Tensor, normalize: bool) -> torch.Tensor:
        lib = _lib.load()
        head, _ = self._head()
        tower = self.transformer.tower()
        bsz, seq = tok.shape[0], tok.shape[1]
        tokb = tok.detach().to(torch.bfloat16).contiguous()
        out = torch.empty(bsz, self.output_dim, dtype=torch.float32, device=tok.device)
        nbytes = lib.ov_vision_head_workspace_bytes(tower.handle, C.byref(head), bsz)
        ws = self._ws.get(nbytes, tok.device)
        check(lib.ov_vision_head_forward_tokens(tower.handle, C.byref(head), ptr(tokb), bsz, seq, ptr(out), int(normalize), ptr(ws),
                                                nbytes, stream_ptr()), "ov_vision_head_forward_tokens")
        return out

    def _pooled_head(self, tok: torch.Tensor, normalize: bool):
        """The attentional-pool tail (transformer.py:636-646): attn_pool over all tokens -> ln_post -> 'tok' / 'avg' -> proj [-> L2].
        tok [B, L, width] -> (features [B, output_dim] fp32, tokens = ln_post(pool(x))[:, 1:] [B, n_q - 1, output_dim] fp32)."""
        lib, st = _lib.load(), stream_ptr()
        y = self.attn_pool(tok)                                    # [B, n_q, E] bf16
        bsz, nq, e = y.shape
        g, b = self.ln_post.packed()
        z = torch.empty(bsz, nq, e, dtype=torch.float32, device=tok.device)
        check(lib.ov_layernorm(ptr(y), OV_BF16, e, ptr(g), ptr(b), ptr(z), OV_F32, e, bsz * nq, e, float(self.ln_post.eps), st), "ov_layernorm(ln_post)")
        kp = _round_up(e, 64)
        pooled = torch.zeros(bsz, kp, dtype=torch.bfloat16, device=tok.device)
        if self.pool_type == "avg":
            if nq < 2:
                raise ValueError("attentional pool with pool_type 'avg' needs at least two queries (the mean runs over queries 1..)")
            pooled[:, :e] = z[:, 1:].mean(dim=1)
        else:
            pooled[:, :e] = z[:, 0]
        wp = self._pool_pk.get((self.proj,), lambda: _pack_matrix(self.proj.detach().t(), _round_up(self.output_dim, 8), kp))
        n = wp.shape[0]
        outb = torch.empty(bsz, n, dtype=torch.bfloat16, device=tok.device)
        _gemm_bias(ptr(pooled), kp, ptr(wp), kp, None, ptr(outb), n, bsz, n, kp, st, "ov_gemm(proj)")
        feats = outb[:, : self.output_dim].float()
        return (l2_normalize(feats) if normalize else feats), z[:, 1:]

    def forward(self, x: torch.Tensor):
        if self.output_tokens and self.attn_pool is not None:
            self._check_image(x)
            keep = self._draw_keep(x.shape[0], x.device) if self.dropout_active() else None
            tok = self.transformer(self.ln_pre(self._embed_tokens(_kernel_input(x.detach()), keep)))
            pooled, tokens = self._pooled_head(tok, False)
            return pooled, tokens.to(x.dtype)
        if self.output_tokens:
            self._check_image(x)
            keep = self._draw_keep(x.shape[0], x.device) if self.dropout_active() else None
            tok = self._embed_tokens(_kernel_input(x.detach()), keep)
            tok = self.transformer(self.ln_pre(tok))
            pooled = self._head_forward(tok, False)
            tokens = tok[:, 1:]
            if not self.final_ln_after_pool:        # transformer.py:641-645: ln_post runs on all tokens BEFORE pooling
                tokens = self.ln_post(tokens.contiguous())
            return pooled, tokens.to(x.dtype)
        return self._encode(x, False)


# ------------------------------------------------------------------------------------------------------
# CLIP
# ------------------------------------------------------------------------------------------------------
class CLIP(nn.Module):
    """Drop-in for ``open_clip.model.CLIP`` (model.py:220-315) on OpenVision configs and on the stock open_clip ones (a causal text
    tower pooled at the EOT token, an image tower with ln_pre and 'tok' pooling); ``quick_gelu`` is not built."""
    output_dict: torch.jit.Final[bool]

    def __init__(self, embed_dim: int, vision_cfg: Union[dict, CLIPVisionCfg], text_cfg: Union[dict, CLIPTextCfg],
                 quick_gelu: bool = False, init_logit_scale: float = np.log(1 / 0.07),
                 init_logit_bias: Optional[float] = None, cast_dtype: Optional[torch.dtype] = None,
                 output_dict: bool = False):
        super().__init__()
        if quick_gelu:
            raise NotImplementedError("quick_gelu=True (the OpenAI CLIP weights: x * sigmoid(1.702 x) in every MLP) is not built: the "
                                      "GEMM epilogues carry erf and tanh GELU only.  Stock open_clip models trained with nn.GELU "
                                      "(the LAION / DataComp checkpoints) load with quick_gelu=False")
        self.output_dict = output_dict
        v = vision_cfg_from(vision_cfg, embed_dim)
        t = text_cfg_from(text_cfg)
        self.vision_cfg, self.text_cfg, self.embed_dim = v, t, embed_dim
        self.visual = VisionTransformer(
            image_size=v.image_size, patch_size=v.patch_size, width=v.width, layers=v.layers,
            heads=v.width // v.head_width, mlp_ratio=v.mlp_ratio, output_dim=embed_dim, pool_type=v.pool_type,
            final_ln_after_pool=v.final_ln_after_pool, no_ln_pre=v.no_ln_pre, act_kwargs=v.act_kwargs,
            eps=ln_eps(v.norm_kwargs), output_tokens=v.output_tokens, patch_dropout=float(v.patch_dropout),
            pos_embed_type=v.pos_embed_type, attentional_pool=bool(v.attentional_pool),
            attn_pooler_queries=int(v.attn_pooler_queries), attn_pooler_heads=int(v.attn_pooler_heads))
        # text tower parts are adopted at the top level, as the reference does (model.py:239-248)
        self.transformer = Transformer(t.width, t.layers, t.heads, t.mlp_ratio, t.act_kwargs, ln_eps(t.norm_kwargs))
        self.context_length = t.context_length
        self.vocab_size = t.vocab_size
        self.token_embedding = Embedding(t.vocab_size, t.width)
        self.positional_embedding = nn.Parameter(torch.empty(t.context_length, t.width))
        nn.init.normal_(self.positional_embedding, std=0.01)
        self.ln_final = LayerNorm(t.width, eps=ln_eps(t.norm_kwargs))
        self.text_projection = nn.Parameter(torch.empty(t.width, embed_dim))
        nn.init.normal_(self.text_projection, std=t.width ** -0.5)
        self.text_pool_type = t.pool_type
        if t.no_causal_mask:
            self.register_buffer("attn_mask", None, persistent=False)     # no_causal_mask -> None (transformer.py:722-725)
        else:
            # the stock open_clip text tower: the reference's additive mask (build_causal_mask, transformer.py:761-767: -inf strictly
            # above the diagonal) as the same non-persistent buffer; the kernels run it as the prefix-causal mask with prefix 0
            mask = torch.full((t.context_length, t.context_length), float("-inf")).triu_(1)
            self.register_buffer("attn_mask", mask, persistent=False)
            self.transformer.set_causal_prefix(0)
            self.transformer.adopt_causal_mask(self.attn_mask)
        self.logit_scale = nn.Parameter(torch.ones([]) * float(init_logit_scale))
        # SigLIP (model.py:251-254): a learned scalar added to every logit; the loss is openvision_amd.loss.SigLipLoss
        self.logit_bias = nn.Parameter(torch.ones([]) * float(init_logit_bias)) if init_logit_bias is not None else None
        self._pk = _Packed()
        self._ws = _Workspace()
        self._err = None
        self._side_stream = None
        self._graphs = _GraphCache()
        self.graph_max_batch = int(os.environ.get("OVHIP_GRAPH_MAX_BATCH", "0"))    # 0 = off; see use_graphs()
        self.overlap_towers = os.environ.get("OVHIP_OVERLAP_TOWERS", "0") == "1"   # measured gain < 1 %: opt-in
        if cast_dtype is not None and cast_dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError("cast_dtype must be float32 or bfloat16")

    # -- text head -------------------------------------------------------------------------------------
    def _text_head(self):
        def build():
            keep = dict(tok=self.token_embedding.packed(),
                        pos=self.positional_embedding.detach().to(torch.bfloat16).contiguous(), ln=self.ln_final.packed(),
                        proj_t=self.text_projection.detach().t().to(torch.bfloat16).contiguous())
            if self.embed_dim % 8:
                raise _lib.OvhipError("embed_dim must be a multiple of 8")
            h = _lib.TextHead(self.context_length, self.vocab_size, _lib.TEXT_POOL[self.text_pool_type], self.embed_dim,
                              ptr(keep["tok"]), ptr(keep["pos"]), ptr(keep["ln"][0]), ptr(keep["ln"][1]), ptr(keep["proj_t"]))
            return h, keep
        return self._pk.get((self.token_embedding.weight, self.positional_embedding, self.ln_final.weight,
                             self.ln_final.bias, self.text_projection), build)

    # -- reference API -----------------------------------------------------------------------------------
    def set_precision(self, precision: str, mask=None) -> None:
        """GEMM operand precision of both block stacks: "bf16" (default), "fp8" (e4m3 weights and activations on the MX-scaled MFMA
        for all four GEMMs of every block) or "fp8-mixed" (e4m3 for the MLP products only: model.fp8_mixed_mask); `mask` = an explicit
        OV_FP8_* bit set instead.  Embedding, heads, attention, LayerNorm statistics and the loss stay as they are.

        A causal text tower (the stock open_clip configuration) has no fp8 form: the masked attention runs in bf16 only."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}")
        if precision != "bf16" and self.transformer.causal_prefix is not None:
            raise ValueError(f"set_precision({precision!r}): the text tower is causal, and there is no fp8 under an attention mask.  "
                             f"model.visual.transformer.set_precision({precision!r}) puts the image tower alone in fp8")
        self.visual.transformer.set_precision(precision, mask)
        self.transformer.set_precision(precision, mask)

    def freeze_fp8_scales(self, delayed: bool = True) -> None:
        """fp8 precision, after a calibration forward of both towers: static scales for the MLP hidden (see Transformer)."""
        self.visual.transformer.freeze_fp8_scales(delayed)
        self.transformer.freeze_fp8_scales(delayed)

    def use_graphs(self, max_batch: int = 8) -> None:
        """Replay encode_image / encode_text calls of at most `max_batch` rows as captured hipGraphs (0 turns it off).  For the
        launch-bound small-batch path (ov-zero-shot-test.py:167-195 encodes one image at a time); results are bitwise those of the
        plain launches."""
        self.graph_max_batch = int(max_batch)

    def _weights_sig(self):
        ws = (self._ws, self.visual._ws, self.visual.transformer._ws, self.transformer._ws)
        return (_PACK_EPOCH[0],) + tuple(w.gen for w in ws) + tuple((p.data_ptr(), p._version) for p in self.parameters())

    def encode_image(self, image: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """model.py:265-267.  Returns fp32 [B, embed_dim]."""
        if (0 < image.shape[0] <= self.graph_max_batch and image.is_cuda and not torch.cuda.is_current_stream_capturing()
                and not self.visual.dropout_active()):               # a captured graph would replay one draw of kept patches
            self.visual._check_image(image)
            x = _kernel_input(image.detach())
            return self._graphs.run(("img", tuple(x.shape), x.dtype, bool(normalize), self.visual.transformer._cache.precision,
                                     self.visual.transformer.causal_prefix),
                                    self._weights_sig, x, lambda t: self.visual._encode(t, normalize))
        return self.visual._encode(image, normalize)

    def encode_text(self, text: torch.Tensor, normalize: bool = False, _graphed: bool = False) -> torch.Tensor:
        """model.py:269-284.  ``text`` int64 [B, context_length] (the whole pos-emb is added: model.py:274)."""
        _require_cuda(text, "encode_text")
        if text.dim() != 2 or text.shape[1] != self.context_length:
            raise ValueError(f"expected tokens [B,{self.context_length}], got {tuple(text.shape)}")
        if 0 < text.shape[0] <= self.graph_max_batch and not torch.cuda.is_current_stream_capturing() and not _graphed:
            t = text.detach().to(torch.int64).contiguous()
            return self._graphs.run(("txt", tuple(t.shape), bool(normalize), self.transformer._cache.precision,
                                     self.transformer.causal_prefix), self._weights_sig,
                                    t, lambda z: self.encode_text(z, normalize, _graphed=True))
        lib = _lib.load()
        head, _keep = self._text_head()
        tower = self.transformer.tower()
        tok = text.detach().to(torch.int64).contiguous()
        bsz = tok.shape[0]
        out = torch.empty(bsz, self.embed_dim, dtype=torch.float32, device=text.device)
        if self._err is None or self._err.device != text.device:
            self._err = torch.zeros(1, dtype=torch.int32, device=text.device)
        st = stream_ptr()
        mb = MAX_MICRO_BATCH * 4
        for b0 in range(0, bsz, mb):
            nb = min(mb, bsz - b0)
            nbytes = lib.ov_text_workspace_bytes(tower.handle, C.byref(head), nb)
            ws = self._ws.get(nbytes, text.device)
            check(lib.ov_encode_text(tower.handle, C.byref(head), ptr(tok[b0:]), nb, ptr(out[b0:]), int(normalize),
                                     ptr(self._err), ptr(ws), nbytes, st), "ov_encode_text")
        return out

    def check_token_range(self) -> None:
        """Synchronising check of the device-side flag set when a token id was outside [0, vocab_size)
        (torch's nn.Embedding raises IndexError for that: model.py:272)."""
        if self._err is not None and int(self._err.item()) != 0:
            self._err.zero_()
            raise IndexError("token id out of range in encode_text")

    def get_logits(self, image, text):
        """model.py:286-293."""
        i = self.encode_image(image, normalize=True)
        t = self.encode_text(text, normalize=True)
        li = logits(i, t, self.logit_scale.detach().exp())       # the scale stays on the device (model.py:288)
        if self.logit_bias is not None:
            li += self.logit_bias.detach()                       # model.py:289-290, also on the device
        return li, li.T

    def forward(self, image: Optional[torch.Tensor] = None, text: Optional[torch.Tensor] = None):
        """model.py:295-315."""
        if image is not None and text is not None and self.overlap_towers and text.is_cuda:
            # The towers are independent until the loss: the text tower runs on a side stream so that its small,
            # launch/latency-bound kernels (and both towers' HBM-bound LayerNorms) fill CUs the other tower leaves idle.
            cur = torch.cuda.current_stream(text.device)
            if self._side_stream is None or self._side_stream.device != text.device:
                self._side_stream = torch.cuda.Stream(device=text.device)
            side = self._side_stream
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                text_features = self.encode_text(text, normalize=True)
            image_features = self.encode_image(image, normalize=True)
            cur.wait_stream(side)
            text_features.record_stream(cur)
        else:
            image_features = self.encode_image(image, normalize=True) if image is not None else None
            text_features = self.encode_text(text, normalize=True) if text is not None else None
        scale = self.logit_scale.detach().exp()
        bias = self.logit_bias.detach() if self.logit_bias is not None else None
        if self.output_dict:
            out = {"image_features": image_features, "text_features": text_features, "logit_scale": scale}
            if bias is not None:
                out["logit_bias"] = bias
            return out
        if bias is not None:
            return image_features, text_features, scale, bias
        return image_features, text_features, scale

    def invalidate_packed(self) -> None:
        """Forget the bf16 / fp8 packed copies, folded LayerNorm weights and tower handles (see ``_Packed``): required after
        in-place parameter writes through ``.data``, which leave ``_version`` unchanged."""
        invalidate_packed()

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)          # .to() / .cuda() / .float() replace the buffers: follow the causal mask
        if self.attn_mask is not None:
            self.transformer.adopt_causal_mask(self.attn_mask)
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        invalidate_packed()          # copy_ under no_grad bumps _version today; do not depend on it
        return out

    def lock_image_tower(self, unlocked_groups: int = 0, freeze_bn_stats: bool = False) -> None:
        """Lock the image tower as per LiT (model.py:256-258 of the reference); see ``VisionTransformer.lock``.  Build the optimiser
        afterwards: ``FusedAdamW`` collects the parameters that require grad when it is constructed."""
        self.visual.lock(unlocked_groups=unlocked_groups, freeze_bn_stats=freeze_bn_stats)

    def set_input_size(self, image_size: int) -> None:
        """Run the image tower at another resolution: ``VisionTransformer.set_input_size`` (one host round trip of the position
        table; build the stage's optimiser afterwards).  The text tower is untouched."""
        self.visual.set_input_size(image_size)
        self.vision_cfg = dataclasses.replace(self.vision_cfg, image_size=int(image_size))

    def set_drop_path(self, image: float = 0.0, text: float = 0.0) -> None:
        """Stochastic depth rates of the two towers on the training path (``Transformer.set_drop_path``; the reference's
        ``drop_path`` of vit.py:358 and text_transformer.py:533-536), each in [0, 1).  The inference entry points ignore them, and so
        does the training path of a tower in eval mode."""
        for rate in (image, text):
            if not 0.0 <= float(rate) < 1.0:
                raise ValueError(f"drop_path rate {rate} outside [0, 1)")
        self.visual.transformer.set_drop_path(image)
        self.transformer.set_drop_path(text)

    def set_grad_checkpointing(self, enable=True):
        """Activation recomputation on the training path (model.py:261-263 of the reference; its trainer's remat='full' per block):
        ``openvision_amd.training`` then keeps only each block's input and recomputes the block's intermediates just before its
        backward, bitwise the same loss and gradients.  The inference entry points ignore the flag."""
        self.visual.set_grad_checkpointing(enable)
        self.transformer.grad_checkpointing = enable


def logits(a: torch.Tensor, b: torch.Tensor, scale=1.0) -> torch.Tensor:
    """scale * a @ b.T for fp32 embeddings on device (exact-fp32 MFMA kernel).  `scale`: a float, or a 0-d / 1-element tensor that is
    read on the device (no host synchronisation)."""
    _require_cuda(a, "logits")
    sdev = None
    if isinstance(scale, torch.Tensor):
        sdev = scale.detach().float().reshape(1).to(a.device)
        scale = 1.0
    a32, b32 = a.detach().float().contiguous(), b.detach().float().contiguous()
    out = torch.empty(a32.shape[0], b32.shape[0], dtype=torch.float32, device=a.device)
    check(_lib.load().ov_logits(ptr(a32), ptr(b32), ptr(out), out.shape[1], a32.shape[0], b32.shape[0], a32.shape[1],
                                float(scale), ptr(sdev), stream_ptr()), "ov_logits")
    return out


def l2_normalize(x: torch.Tensor) -> torch.Tensor:
    """F.normalize(x, dim=-1) on device -> fp32."""
    _require_cuda(x, "l2_normalize")
    xin = _kernel_input(x.detach())
    x2 = xin.view(-1, xin.shape[-1])
    out = torch.empty(x2.shape, dtype=torch.float32, device=x.device)
    check(_lib.load().ov_l2norm(ptr(x2), _dtype_flag(x2), x2.shape[1], ptr(out), x2.shape[1], x2.shape[0], x2.shape[1],
                                stream_ptr()), "ov_l2norm")
    return out.view(x.shape)


def create_model(model_cfg: dict, device=None, state_dict: Optional[dict] = None, resize_pos_embed: bool = False, **kw) -> CLIP:
    """``CLIP(**model_cfg)`` + optional strict ``load_state_dict`` (ov-zero-shot-test.py:52-56).

    ``resize_pos_embed=True``: a state dict from another resolution (or text context length) loads, as the reference's
    ``load_checkpoint`` does it (factory.py:178): on a shallow copy of the dict, a fixed image table is regenerated for the model's
    grid after a check of its form, a learned one is resampled (bicubic, antialiased), the text table is resampled (linear) --
    ``posembed.resize_for`` -- and then the load is strict as ever.  Default False: a shape mismatch raises."""
    m = CLIP(embed_dim=model_cfg["embed_dim"], vision_cfg=model_cfg["vision_cfg"], text_cfg=model_cfg["text_cfg"],
             **{k: v for k, v in model_cfg.items() if k not in ("embed_dim", "vision_cfg", "text_cfg")}, **kw)
    if state_dict is not None and resize_pos_embed:
        state_dict = dict(state_dict)
        posembed.resize_for(state_dict, m)
    if state_dict is not None:
        m.load_state_dict(state_dict, strict=True)
    if device is not None:
        m = m.to(device)
    return m.eval()
