"""Stochastic depth ("drop path") of the reference's towers, restated in fp64 with explicit masks.

The operator, src/models/common.py:659-675 (DropPath.__call__), in training with rate r (keep = 1 - r):

    mask = floor(keep + uniform(rng, (B, 1, ..., 1)))          # :673-674, one number per sample
    return x / keep * mask                                      # identity when deterministic or r == 0

It wraps each of a block's two residual branches with a draw of its own -- src/models/vit.py:250,296,328 and
src/models/text_transformer.py:389,472,501 -- and block i of n gets the rate np.linspace(0, drop_path, n)[i] (vit.py:358,
text_transformer.py:533-536).  So for block i, with per-sample masks m_attn, m_mlp in {0, 1}^B and s = 1 / keep_i:

    x1 = x  + (m_attn[b] s) out_proj(attn(ln_1(x)))[b]
    y  = x1 + (m_mlp[b]  s) c_proj(gelu(c_fc(ln_2(x1))))[b]

The JAX generator is not reproduced: the masks are arguments.  Everything below is torch float64 on the CPU, and torch autograd is the
differentiator, so the gradients are those of exactly this forward.  The block itself is open_clip's ResidualAttentionBlock
(transformer.py:254-265) as the towers here run it: LayerNorm with a biased variance and eps inside the root, packed in_proj,
scaled-dot-product attention per head (unmasked, or key j visible to query i iff j < prefix or j <= i), exact-erf or tanh GELU."""
import math

import numpy as np
import torch

NAMES = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b")


def rates(rate, layers):
    """vit.py:358: dpr = [float(x) for x in np.linspace(0, drop_path, depth)]."""
    return np.linspace(0, rate, layers)


def draw(keep_prob, u):
    """common.py:673-674: floor(keep_prob + u) for u in [0, 1): 1 = the sample keeps the branch."""
    return np.floor(np.asarray(keep_prob, np.float64) + np.asarray(u, np.float64))


def block_params(blk):
    """The twelve parameters of a ResidualAttentionBlock module in NAMES order, fp64 leaves."""
    ts = [blk.ln_1.weight, blk.ln_1.bias, blk.attn.in_proj_weight, blk.attn.in_proj_bias, blk.attn.out_proj.weight, blk.attn.out_proj.bias,
          blk.ln_2.weight, blk.ln_2.bias, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias]
    return {n: t.detach().cpu().double().clone().requires_grad_(True) for n, t in zip(NAMES, ts)}


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _gelu(a, tanh):
    if tanh:
        return 0.5 * a * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a ** 3)))
    return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))


def _attn(qkv, heads, prefix):
    B, L, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    q, k, v = (t.reshape(B, L, heads, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if prefix is not None:
        i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
        s = s.masked_fill(~((j < prefix) | (j <= i)), float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, D)


def block(x, p, m_attn, m_mlp, scale, heads, tanh=False, prefix=None, eps=1e-6):
    """One block under the masks m_attn, m_mlp ([B], 0 / 1) and the factor `scale` of a kept sample's branch."""
    ma = (torch.as_tensor(m_attn).double() * scale)[:, None, None]
    mm = (torch.as_tensor(m_mlp).double() * scale)[:, None, None]
    a = _attn(_ln(x, p["ln1_w"], p["ln1_b"], eps) @ p["qkv_w"].T + p["qkv_b"], heads, prefix) @ p["out_w"].T + p["out_b"]
    x1 = x + ma * a
    h = _gelu(_ln(x1, p["ln2_w"], p["ln2_b"], eps) @ p["fc_w"].T + p["fc_b"], tanh) @ p["proj_w"].T + p["proj_b"]
    return x1 + mm * h


def tower(x, params, keep, scale, heads, tanh=False, prefix=None, eps=1e-6):
    """The block stack: params = [block_params per layer], keep bool / 0-1 [layers, 2, B] (None: nothing dropped), scale [layers]."""
    for i, p in enumerate(params):
        if keep is None:
            B = x.shape[0]
            x = block(x, p, torch.ones(B), torch.ones(B), 1.0, heads, tanh, prefix, eps)
        else:
            x = block(x, p, keep[i][0], keep[i][1], float(scale[i]), heads, tanh, prefix, eps)
    return x


def tower_grads(x, params, wout, keep, scale, heads, tanh=False, prefix=None, eps=1e-6):
    """(y, dx, [{name: grad} per layer]) of loss = sum(tower(x) * wout), all fp64."""
    xx = x.detach().double().clone().requires_grad_(True)
    for p in params:
        for t in p.values():
            t.grad = None
    y = tower(xx, params, keep, scale, heads, tanh, prefix, eps)
    (y * wout.double()).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad.clone()
    return y.detach(), zero(xx), [{n: zero(t) for n, t in p.items()} for p in params]
