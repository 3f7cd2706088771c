"""Restatements of the reference's caption branch in torch (fp64 unless said otherwise), with the reference's line numbers beside each
step, plus thin wrappers of the new C entry points.  jax / flax are not importable where these tests were written, so NO
reference-generated fixture backs the prefix / caption tests: these restatements are the oracle.

Reference files: src/models/text_transformer.py (Encoder1DBlock :404-473, the prefix-LM mask :418-442), src/models/text_decoder.py
(_Model :436-576, concat fusion), src/losses/common.py (softmax_xent :225-251)."""
import ctypes as C

import torch

from openvision_amd import _lib
from openvision_amd._lib import ptr, stream_ptr, check

from hipops import _split, REL

LOG2E = 1.4426950408889634


# ---- the mask --------------------------------------------------------------------------------------------------------------------
def rule_mask(L, P):
    """The kernels' rule: key j is visible to query i iff j < P or j <= i.  bool [L, L] (query, key)."""
    i = torch.arange(L)[:, None]
    j = torch.arange(L)[None, :]
    return (j < P) | (j <= i)


def reference_mask(L, P):
    """The mask as text_transformer.py builds it, block by block, with li = P, lt = L - P."""
    li, lt = P, L - P
    causal = torch.tril(torch.ones(lt, lt, dtype=torch.bool))        # :422  make_causal_mask(x[:, li:, 0])
    prefix = torch.ones(li, li, dtype=torch.bool)                    # :425  prefix_mask = ones(li, li)
    mask = torch.zeros(li + lt, li + lt, dtype=torch.bool)           # :429  zeros(l, l)
    mask[:li, :li] = prefix                                          # :432  image attends to image
    mask[li:, li:] = causal                                          # :435  text attends causally to itself
    mask[li:, :li] = True                                            # :438  text attends to all image embeddings
    return mask


# ---- attention under a mask --------------------------------------------------------------------------------------------------------
def masked_attn_ref64(qkv, B, L, Hh, hd, mask):
    """hipops.attn_ref64 with invisible keys at -inf: (ref, pv) [B*L, Hh*hd] fp64, pv = P.|V| over the visible keys."""
    q, k, v = _split(qkv, B, L, Hh, hd)
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    back = lambda t: t.transpose(1, 2).reshape(B * L, Hh * hd)
    return back(p @ v), back(p @ v.abs())


def masked_attn_grads64(qkv, dout, B, L, Hh, hd, mask):
    """fp64 autograd of the masked softmax attention: dqkv [B*L, 3*Hh*hd] fp64."""
    D = Hh * hd
    x = qkv[:, :3 * D].double().clone().requires_grad_(True)
    y = x.view(B, L, 3, Hh, hd)
    q, k, v = [y[:, :, j].transpose(1, 2) for j in range(3)]
    s = (q @ k.transpose(-1, -2) * hd ** -0.5).masked_fill(~mask, float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * L, D)
    o.backward(dout.double())
    return x.grad


def emulate_masked(qkv, B, L, Hh, hd, mask):
    """The kernel's arithmetic on the CPU (the idea of tests/test_attention_bound.py): fp32 scores in log2 units, -inf for masked keys,
    P = exp2(s - max) rounded to bf16 before P.V, fp32 row sum of the unrounded P, bf16 output.  Returns bf16 [B*L, Hh*hd]."""
    q, k, v = [t.float() for t in _split(qkv, B, L, Hh, hd)]
    s = (q @ k.transpose(-1, -2)) * (hd ** -0.5 * LOG2E)
    s = s.masked_fill(~mask, float("-inf"))
    p = torch.exp2(s - s.amax(dim=-1, keepdim=True))
    l = p.sum(dim=-1, keepdim=True)
    o = (p.to(torch.bfloat16).float() @ v) / l
    return o.transpose(1, 2).reshape(B * L, Hh * hd).to(torch.bfloat16)


def boundary_spiked_qkv(B, L, Hh, hd, P, seed, delta=6.0):
    """Random bf16 qkv whose mask-boundary keys carry a spike, so that an off-by-one mask moves the output far outside hipops.bound.
    Per head three probe queries (skipped where they do not exist):
      * i_d (a causal row >= P): key i_d (the diagonal, visible) and key i_d + 1 (the first invisible one) are both set to alpha Q[i_d],
        delta log2 units above the row's other scores -- dropping the diagonal or admitting one key too many changes row i_d's
        softmax weights by a large factor; V rows of the two keys differ (random), so the output moves.
      * i_p (the last prefix row, P - 1, if 1 <= P < L and P - 1 > 0 ... any row below P - 1 sees key P - 1 only through the prefix):
        key P - 1 spiked towards query 0 (visible to it only because P - 1 < P) and key P towards query 0 as well (invisible to it):
        a prefix off by one either hides the first or admits the second.
    Returns (qkv, probes) with probes = [(b, h, row)]."""
    D = Hh * hd
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * L, 3 * D, generator=g).to(torch.bfloat16)
    x = qkv.view(B, L, 3, Hh, hd)
    c = hd ** -0.5 * LOG2E
    probes = []

    def spike(b, h, qi_row, keys):
        qi = x[b, qi_row, 0, h].double()
        others = [j for j in range(L) if j not in keys]
        m_other = float((x[b, others, 1, h].double() @ qi).max()) * c if others else 0.0
        alpha = (m_other + delta) / (float(qi @ qi) * c)
        for j in keys:
            x[b, j, 1, h] = (alpha * qi).to(torch.bfloat16)
            x[b, j, 2, h] = x[b, j, 2, h] + (4.0 if j == keys[0] else -4.0)       # the two keys pull the output apart

    for b in range(B):
        for h in range(Hh):
            if P >= 2 and P < L:                    # prefix boundary: keys P - 1 (visible to row 0) and P (invisible to row 0)
                spike(b, h, 0, [P - 1, P])
                probes.append((b, h, 0))
            i_d = max(P, 1) + (L - max(P, 1)) // 2   # a causal row with a key above it, away from the prefix probe's keys
            if P + 2 <= i_d and i_d + 1 < L:
                spike(b, h, i_d, [i_d, i_d + 1])
                probes.append((b, h, i_d))
    return qkv, probes


# ---- wrappers of the new entry points ------------------------------------------------------------------------------------------------
def attention_prefix(qkv, B, L, H, hd, prefix, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty(B * L, H * hd, dtype=torch.bfloat16, device=qkv.device)
    check(lib.ov_attention_prefix(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), B, L, H, hd, hd ** -0.5, prefix, stream_ptr()),
          "ov_attention_prefix")
    return out


def attention_prefix_backward(qkv, out, dout, B, L, H, hd, prefix, dqkv=None, ws=None):
    """dqkv= / ws=: caller-owned buffers, as hipops.attention_backward takes them (a slice of a wider tensor; a workspace handed over
    with its own size)."""
    lib = _lib.load()
    nb = lib.ov_attention_prefix_backward_workspace_bytes(B, L, H, hd)
    if dqkv is None:
        dqkv = torch.zeros_like(qkv)
    assert dqkv.shape == qkv.shape and dqkv.dtype == torch.bfloat16 and dqkv.stride(1) == 1, (dqkv.shape, dqkv.dtype, dqkv.stride())
    if ws is None:
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=qkv.device)
    else:
        assert ws.dtype == torch.uint8 and ws.is_contiguous()
        nb = ws.numel()
    check(lib.ov_attention_prefix_backward(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), ptr(dout), dout.stride(0), ptr(dqkv),
                                           dqkv.stride(0), B, L, H, hd, hd ** -0.5, prefix, ptr(ws), nb, stream_ptr()),
          "ov_attention_prefix_backward")
    return dqkv


def softmax_xent(logits, labels, mask):
    """ov_softmax_xent: (loss [1], row_lse [R])."""
    lib = _lib.load()
    R, V = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    lse = torch.empty(R, dtype=torch.float32, device=logits.device)
    nb = lib.ov_softmax_xent_workspace_bytes(R)
    ws = torch.empty(nb, dtype=torch.uint8, device=logits.device)
    check(lib.ov_softmax_xent(ptr(logits), logits.stride(0), ptr(labels), ptr(mask), R, V, ptr(loss), ptr(lse), ptr(ws), nb, stream_ptr()),
          "ov_softmax_xent")
    return loss, lse


def softmax_xent_backward(logits, labels, mask, lse, grad, out=None):
    lib = _lib.load()
    R, V = logits.shape
    d = torch.empty_like(logits) if out is None else out
    g = torch.full((1,), float(grad), dtype=torch.float32, device=logits.device)
    nb = lib.ov_softmax_xent_workspace_bytes(R)
    ws = torch.empty(nb, dtype=torch.uint8, device=logits.device)
    check(lib.ov_softmax_xent_backward(ptr(logits), logits.stride(0), ptr(labels), ptr(mask), ptr(lse), ptr(g), ptr(d), d.stride(0), R, V,
                                       ptr(ws), nb, stream_ptr()), "ov_softmax_xent_backward")
    return d


def xent_ref64(logits, labels, mask):
    """softmax_xent (losses/common.py:225-251) in fp64: (loss, row lse, nll)."""
    x = logits.double()
    V = x.shape[1]
    inside = (labels >= 0) & (labels < V)
    onehot = torch.zeros_like(x)                                                    # :231  jax.nn.one_hot: zero row outside [0, V)
    onehot[inside, labels[inside]] = 1.0
    log_p = torch.log_softmax(x, dim=-1)                                            # :236
    nll = -(onehot * log_p).sum(-1)                                                 # :239
    m = mask.double()
    return (nll * m).sum() / (m.sum() + 1e-8), torch.logsumexp(x, dim=-1), nll      # :248


# ---- the decoder block and the decoder, restated (fp32 or fp64 tensors in, same dtype out) ---------------------------------------
def block_restated(x, w, heads, mask, eps=1e-6):
    """Encoder1DBlock (text_transformer.py:404-473): LN -> MHA(mask) -> + -> LN -> tanh-GELU MLP -> +.  w: dict of the module's
    tensors (ln1_w, ln1_b, qkv_w [3D, D], qkv_b, out_w, out_b, ln2_w, ln2_b, fc_w, fc_b, proj_w, proj_b) in x's dtype."""
    F = torch.nn.functional
    B, L, D = x.shape
    hd = D // heads
    y = F.layer_norm(x, (D,), w["ln1_w"], w["ln1_b"], eps)                          # :446
    qkv = (y @ w["qkv_w"].T + w["qkv_b"]).view(B, L, 3, heads, hd)                  # :454  MultiHeadDotProductAttention
    q, k, v = [qkv[:, :, j].transpose(1, 2) for j in range(3)]
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    s = s.masked_fill(~mask.to(s.device), float("-inf"))                            # :467  mask=mask
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, D)
    x = x + (o @ w["out_w"].T + w["out_b"])                                         # :472  x + y
    y = F.layer_norm(x, (D,), w["ln2_w"], w["ln2_b"], eps)
    h = F.gelu(y @ w["fc_w"].T + w["fc_b"], approximate="tanh")
    return x + (h @ w["proj_w"].T + w["proj_b"])
