"""Thin test-side wrappers: torch tensors -> C ABI calls of libovhip.so (granular operators)."""
import ctypes as C

import torch

from openvision_amd import _lib
from openvision_amd._lib import ptr, stream_ptr, check, OV_BF16, OV_F32


LOG2E = 1.4426950408889634
REL = 2.0 ** -8                  # the attention bound's relative terms (bound() below)


def _flag(t):
    return OV_F32 if t.dtype == torch.float32 else OV_BF16


def layernorm(x, g, b, eps=1e-6, out_dtype=None):
    lib = _lib.load()
    x2 = x.contiguous().view(-1, x.shape[-1])
    y = torch.empty(x2.shape, dtype=out_dtype or x.dtype, device=x.device)
    check(lib.ov_layernorm(ptr(x2), _flag(x2), x2.shape[1], ptr(g), ptr(b), ptr(y), _flag(y), x2.shape[1], x2.shape[0],
                           x2.shape[1], eps, stream_ptr()))
    return y.view(x.shape)


def gemm(a, w, bias=None, epi=0, resid=None, out=None, out_group=0, resid_mod=0, resid_off=0, out_rows=None):
    lib = _lib.load()
    m, k = a.shape
    n = w.shape[0]
    if out is None:
        out = torch.zeros(out_rows or m, n, dtype=torch.bfloat16, device=a.device)
    check(lib.ov_gemm(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(out), out.stride(0), m, n, k, epi,
                      ptr(resid), resid.stride(0) if resid is not None else 0, out_group, resid_mod, resid_off, stream_ptr()))
    return out


def gemm_keep(a, w, bias, epi, ldc=None, ldc2=None, fill=0.0):
    """C = gelu(a w^T + bias), C2 = a w^T + bias (both bf16) from one launch: ov_gemm_keep.  fill: what both outputs hold before."""
    lib = _lib.load()
    m, k = a.shape
    n = w.shape[0]
    out = torch.full((m, ldc or n), fill, dtype=torch.bfloat16, device=a.device)
    pre = torch.full((m, ldc2 or n), fill, dtype=torch.bfloat16, device=a.device)
    check(lib.ov_gemm_keep(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(out), out.stride(0), ptr(pre), pre.stride(0),
                           m, n, k, epi, stream_ptr()))
    return out, pre


def attention(qkv, B, L, H, hd=64, out=None):
    """out (optional): a caller-owned [B*L, >= H*hd] bf16 tensor; its row pitch is passed as ld_out (qkv's as ld_qkv)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(B * L, H * hd, dtype=torch.bfloat16, device=qkv.device)
    check(lib.ov_attention(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), B, L, H, hd, hd ** -0.5, stream_ptr()))
    return out


def clip_loss(img, txt, all_img, all_txt, scale, label_offset):
    lib = _lib.load()
    b, e = img.shape
    n = all_img.shape[0]
    nb = lib.ov_clip_loss_workspace_bytes(b, n)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=img.device)
    out = torch.empty(1, dtype=torch.float32, device=img.device)
    terms = torch.empty(4, b, dtype=torch.float32, device=img.device)
    sc = (scale.detach().float().reshape(1) if isinstance(scale, torch.Tensor) and scale.is_cuda
          else torch.full((1,), float(scale), dtype=torch.float32, device=img.device))
    check(lib.ov_clip_loss(ptr(img), ptr(txt), ptr(all_img), ptr(all_txt), b, n, e, ptr(sc), label_offset, ptr(out),
                           ptr(terms), ptr(ws), nb, stream_ptr()))
    return out[0], terms


def rowstats(x, eps=1e-6):
    lib = _lib.load()
    st = torch.empty(x.shape[0], 2, dtype=torch.float32, device=x.device)
    check(lib.ov_rowstats(ptr(x), x.stride(0), ptr(st), x.shape[0], x.shape[1], eps, stream_ptr()))
    return st


def rowparts(x):
    """Partial sums of the row statistics: [rows, D / 32, 2] fp32 (ov_rowparts)."""
    lib = _lib.load()
    parts = torch.empty(x.shape[0], x.shape[1] // 32, 2, dtype=torch.float32, device=x.device)
    check(lib.ov_rowparts(ptr(x), x.stride(0), ptr(parts), x.shape[0], x.shape[1], stream_ptr()))
    return parts


def rowstats_finalize(parts, eps=1e-6):
    lib = _lib.load()
    st = torch.empty(parts.shape[0], 2, dtype=torch.float32, device=parts.device)
    check(lib.ov_rowstats_finalize(ptr(parts), ptr(st), parts.shape[0], parts.shape[1] * 32, eps, stream_ptr()))
    return st


def gemm_rowparts(a, w, bias, resid, out=None, parts=None):
    """Residual GEMM that also leaves the partial sums of its output rows (ov_gemm_rowparts).  parts (optional): a caller-owned
    contiguous [M, N / 32, 2] fp32 tensor (e.g. a view of a larger buffer, to watch what lies behind it)."""
    lib = _lib.load()
    m, k = a.shape
    n = w.shape[0]
    if out is None:
        out = torch.zeros(m, n, dtype=torch.bfloat16, device=a.device)
    if parts is None:
        parts = torch.full((m, n // 32, 2), float("nan"), dtype=torch.float32, device=a.device)
    assert parts.shape == (m, n // 32, 2) and parts.is_contiguous()
    check(lib.ov_gemm_rowparts(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(out), out.stride(0), m, n, k,
                               ptr(resid), resid.stride(0), ptr(parts), stream_ptr()))
    return out, parts


def gemm_ln(x, wg, cvec, colsum, stats, epi=0, out=None):
    lib = _lib.load()
    m, k = x.shape
    n = wg.shape[0]
    if out is None:
        out = torch.empty(m, n, dtype=torch.bfloat16, device=x.device)
    check(lib.ov_gemm_ln(ptr(x), x.stride(0), ptr(wg), wg.stride(0), ptr(cvec), ptr(colsum), ptr(stats), ptr(out), out.stride(0),
                         m, n, k, epi, stream_ptr()))
    return out


def quantize_rows_e4m3(x):
    """Per-row absmax scaling to OCP e4m3fn (max 448): returns (uint8 view of the fp8 tensor, fp32 scales)."""
    amax = x.float().abs().amax(dim=1).clamp_min(1e-12)
    scale = amax / 448.0
    q = (x.float() / scale[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale.contiguous()


def _out_buf(out, m, n, dtype, fill, device):
    """The output of an fp8-path wrapper: the caller's buffer (out=, e.g. a column slice of a wider tensor: the pitch is its
    stride(0)), else a fresh [m, n] tensor holding `fill` (None: uninitialised)."""
    if out is not None:
        assert out.shape == (m, n) and out.dtype == dtype and out.stride(1) == 1, (out.shape, out.dtype, out.stride())
        return out
    if fill is None:
        return torch.empty(m, n, dtype=dtype, device=device)
    return torch.full((m, n), fill, dtype=dtype, device=device)


def gemm_fp8(aq, wq, rowscale, colscale, bias=None, epi=0, resid=None, out=None, fill=None):
    """Operands may be column slices of wider buffers (pitch = stride(0)).  out: a caller's bf16 [m, n] buffer; fill: what a fresh
    output holds before the launch."""
    lib = _lib.load()
    m, k = aq.shape
    n = wq.shape[0]
    out = _out_buf(out, m, n, torch.bfloat16, fill, aq.device)
    check(lib.ov_gemm_fp8(ptr(aq), aq.stride(0), ptr(wq), wq.stride(0), ptr(rowscale), ptr(colscale),
                          ptr(bias) if bias is not None else None, ptr(out), out.stride(0), m, n, k, epi,
                          ptr(resid) if resid is not None else None, resid.stride(0) if resid is not None else 0, stream_ptr()))
    return out


def quant_rows_fp8(x, gamma=None, beta=None, eps=1e-6, amax=None, out=None, fill=None):
    """bf16 [rows, D] -> (uint8 e4m3 [rows, D], fp32 scales); with gamma/beta: LayerNorm first.  x may be a column slice of a wider
    buffer; out: a caller's uint8 [rows, D] buffer; fill: the byte a fresh output holds before the launch."""
    lib = _lib.load()
    rows, d = x.shape
    q = _out_buf(out, rows, d, torch.uint8, fill, x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    if gamma is None:
        check(lib.ov_quant_rows_fp8(ptr(x), x.stride(0), ptr(q), q.stride(0), ptr(sc), rows, d,
                                    ptr(amax) if amax is not None else None, stream_ptr()))
    else:
        check(lib.ov_layernorm_quant_fp8(ptr(x), x.stride(0), ptr(gamma), ptr(beta), ptr(q), q.stride(0), ptr(sc), rows, d, eps,
                                         stream_ptr()))
    return q, sc


def gemm_fp8_static(aq, wq, colscale, bias, epi, rowscale=None, in_amax=None, out_amax=None, resid=None, amax_next=None, out=None,
                    fill=None):
    """out_amax: returns e4m3 bytes [m, n]; in_amax: returns bf16.  out / fill: as gemm_fp8 (uint8 with out_amax)."""
    lib = _lib.load()
    m, k = aq.shape
    n = wq.shape[0]
    out = _out_buf(out, m, n, torch.uint8 if out_amax is not None else torch.bfloat16, fill, aq.device)
    check(lib.ov_gemm_fp8_static(ptr(aq), aq.stride(0), ptr(wq), wq.stride(0), ptr(rowscale) if rowscale is not None else None,
                                 ptr(in_amax) if in_amax is not None else None, ptr(colscale), ptr(bias) if bias is not None else None,
                                 ptr(out), out.stride(0), ptr(out_amax) if out_amax is not None else None,
                                 ptr(amax_next) if amax_next is not None else None, m, n, k, epi,
                                 ptr(resid) if resid is not None else None, resid.stride(0) if resid is not None else 0, stream_ptr()))
    return out


def attention_fp8out(qkv, B, L, Hh, amax, amax_next=None, out=None, fill=None):
    """head_dim 64; returns e4m3 bytes [B*L, Hh*64] under the static scale 2 * amax / 448.  out / fill: as gemm_fp8 (uint8)."""
    lib = _lib.load()
    d = Hh * 64
    out = _out_buf(out, B * L, d, torch.uint8, fill, qkv.device)
    check(lib.ov_attention_fp8out(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), B, L, Hh, 64, 0.125, ptr(amax),
                                  ptr(amax_next) if amax_next is not None else None, stream_ptr()))
    return out


def amax_roll(cur, next):
    """ov_amax_roll: cur[i] = max(cur[i], next[i]) for i < len(next), in place; returns cur."""
    lib = _lib.load()
    check(lib.ov_amax_roll(ptr(cur), ptr(next), next.numel(), stream_ptr()), "ov_amax_roll")
    return cur


def clip_loss_backward(img, txt, all_img, all_txt, scale, label_offset, terms, grad=1.0, gathered=True):
    """ov_clip_loss_backward: returns (d_img, d_txt, d_all_img | None, d_all_txt | None, d_scale)."""
    lib = _lib.load()
    b, e = img.shape
    n = all_img.shape[0]
    d_img, d_txt = torch.empty_like(img), torch.empty_like(txt)
    d_ai = torch.empty_like(all_img) if gathered else None
    d_at = torch.empty_like(all_txt) if gathered else None
    d_s = torch.empty(1, dtype=torch.float32, device=img.device)
    nb = lib.ov_clip_loss_backward_workspace_bytes(b, n)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=img.device)
    sc = torch.full((1,), float(scale), dtype=torch.float32, device=img.device)
    gr = torch.full((1,), float(grad), dtype=torch.float32, device=img.device)
    check(lib.ov_clip_loss_backward(ptr(img), ptr(txt), ptr(all_img), ptr(all_txt), b, n, e, ptr(sc), label_offset, ptr(terms),
                                    ptr(gr), ptr(d_img), ptr(d_txt), ptr(d_ai) if gathered else None,
                                    ptr(d_at) if gathered else None, ptr(d_s), ptr(ws), nb, stream_ptr()), "ov_clip_loss_backward")
    return d_img, d_txt, d_ai, d_at, d_s


def linear_backward(dy, x, w, want=("dx", "dw", "db")):
    """ov_linear_backward for y = x w^T + b: returns (dX bf16 [M,K] | None, dW bf16 [N,K] | None, db fp32 [N] | None)."""
    lib = _lib.load()
    M, N = dy.shape
    K = x.shape[1]
    dx = torch.empty(M, K, dtype=torch.bfloat16, device=dy.device) if "dx" in want else None
    dw = torch.empty(N, K, dtype=torch.bfloat16, device=dy.device) if "dw" in want else None
    db = torch.empty(N, dtype=torch.float32, device=dy.device) if "db" in want else None
    nb = lib.ov_linear_backward_workspace_bytes(M, N, K)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dy.device)
    check(lib.ov_linear_backward(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(w), w.stride(0), M, N, K,
                                 ptr(dx) if dx is not None else None, K, ptr(dw) if dw is not None else None, K,
                                 ptr(db) if db is not None else None, ptr(ws), nb, stream_ptr()), "ov_linear_backward")
    return dx, dw, db


def transpose(x):
    lib = _lib.load()
    R, C = x.shape
    rp = (R + 63) // 64 * 64
    out = torch.full((C, rp), 7.0, dtype=torch.bfloat16, device=x.device)
    check(lib.ov_transpose_bf16(ptr(x), x.stride(0), R, C, ptr(out), rp, stream_ptr()), "ov_transpose_bf16")
    return out


def layernorm_backward(x, gamma, dy, eps=1e-6, dres=None):
    lib = _lib.load()
    rows, D = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(D, dtype=torch.float32, device=x.device)
    db = torch.empty(D, dtype=torch.float32, device=x.device)
    nb = lib.ov_layernorm_backward_workspace_bytes(rows, D)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=x.device)
    check(lib.ov_layernorm_backward(ptr(x), x.stride(0), ptr(gamma), ptr(dy), dy.stride(0), ptr(dres) if dres is not None else None,
                                    dres.stride(0) if dres is not None else 0, ptr(dx), dx.stride(0), ptr(dg), ptr(db),
                                    rows, D, eps, ptr(ws), nb, stream_ptr()), "ov_layernorm_backward")
    return dx, dg, db


def gelu_backward(a, dh, tanh, with_h=False):
    lib = _lib.load()
    rows, N = a.shape
    da = torch.empty_like(a)
    h = torch.empty_like(a) if with_h else None
    check(lib.ov_gelu_backward(ptr(a), a.stride(0), ptr(dh), dh.stride(0), ptr(da), da.stride(0), ptr(h) if with_h else None,
                               h.stride(0) if with_h else 0, rows, N, int(tanh), stream_ptr()), "ov_gelu_backward")
    return (da, h) if with_h else da


def block_backward(cfg, weights, x, dy, B, L):
    """ov_block_backward.  weights: dict of the module's own tensors (ln1_w, ln1_b fp32; qkv_w bf16 [3D, D]; qkv_b fp32; ...).
    Returns (dx bf16, grads dict)."""
    import ctypes as C
    lib = _lib.load()
    names = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b")
    wst = _lib.BlockWeights(*[C.c_void_p(weights[n].data_ptr()) for n in names], None, None)
    grads = {n: torch.empty_like(weights[n]) for n in names}
    gst = _lib.BlockGrads(*[C.c_void_p(grads[n].data_ptr()) for n in names])
    dx = torch.empty_like(x)
    nb = lib.ov_block_backward_workspace_bytes(C.byref(cfg), B, L)
    assert nb > 0
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=x.device)
    check(lib.ov_block_backward(C.byref(cfg), C.byref(wst), ptr(x), None, ptr(dy), ptr(dx), C.byref(gst), B, L, ptr(ws), nb, stream_ptr()),
          "ov_block_backward")
    return dx, grads


def tower1_forward_backward(cfg, weights, x, dy, B, L):
    """A one-layer tower through ov_tower_forward_saving + ov_tower_backward (every forward intermediate kept, fused backward
    epilogues): returns (y bf16, dx bf16, grads dict)."""
    import ctypes as C
    lib = _lib.load()
    names = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b")
    handle = lib.ov_tower_create(C.byref(cfg))
    assert handle
    try:
        wst = _lib.BlockWeights(*[C.c_void_p(weights[n].data_ptr()) for n in names], None, None)
        check(lib.ov_tower_set_block(handle, 0, C.byref(wst)), "ov_tower_set_block")
        y = x.clone()
        saved = torch.empty(lib.ov_tower_saved_bytes(handle, B, L) + 256, dtype=torch.uint8, device=x.device)
        nb = lib.ov_tower_workspace_bytes(handle, B, L)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=x.device)
        check(lib.ov_tower_forward_saving(handle, ptr(y), ptr(saved), B, L, ptr(ws), nb, stream_ptr()), "ov_tower_forward_saving")
        grads = {n: torch.empty_like(weights[n]) for n in names}
        garr = (_lib.BlockGrads * 1)(_lib.BlockGrads(*[C.c_void_p(grads[n].data_ptr()) for n in names]))
        dx = dy.clone()
        nb2 = lib.ov_tower_backward_workspace_bytes(handle, B, L)
        ws2 = torch.empty(nb2 + 256, dtype=torch.uint8, device=x.device)
        check(lib.ov_tower_backward(handle, ptr(saved), ptr(dx), garr, B, L, ptr(ws2), nb2, stream_ptr()), "ov_tower_backward")
        torch.cuda.synchronize()
    finally:
        lib.ov_tower_destroy(handle)
    return y, dx, grads


def _bwd_buffers(qkv, dqkv, ws, nb):
    """dqkv=: a caller-owned [B*L, 3 H hd] bf16 tensor, e.g. a column slice of a wider one (its pitch is stride(0)); ws=: a caller-owned
    uint8 workspace, handed over with its own size (e.g. a view of exactly `nb` bytes, to watch what lies behind it)."""
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    assert dqkv.shape == qkv.shape and dqkv.dtype == torch.bfloat16 and dqkv.stride(1) == 1, (dqkv.shape, dqkv.dtype, dqkv.stride())
    if ws is None:
        return dqkv, torch.empty(nb + 256, dtype=torch.uint8, device=qkv.device), nb
    assert ws.dtype == torch.uint8 and ws.is_contiguous()
    return dqkv, ws, ws.numel()


def attention_backward(qkv, out, dout, B, L, H, hd=64, dqkv=None, ws=None):
    lib = _lib.load()
    dqkv, ws, nb = _bwd_buffers(qkv, dqkv, ws, lib.ov_attention_backward_workspace_bytes(B, L, H, hd))
    check(lib.ov_attention_backward(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), ptr(dout), dout.stride(0), ptr(dqkv), dqkv.stride(0),
                                    B, L, H, hd, hd ** -0.5, ptr(ws), nb, stream_ptr()), "ov_attention_backward")
    return dqkv


def attention_lse(qkv, B, L, H, hd=64):
    """ov_attention_lse: (out, lse [B*H, L rounded up to 32] fp32 in log2 units)."""
    lib = _lib.load()
    out = torch.empty(B * L, H * hd, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.full((B * H, (L + 31) // 32 * 32), float("nan"), dtype=torch.float32, device=qkv.device)
    check(lib.ov_attention_lse(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), ptr(lse), B, L, H, hd, hd ** -0.5, stream_ptr()),
          "ov_attention_lse")
    return out, lse


def attention_backward_saved(qkv, out, dout, lse, B, L, H, hd=64, dqkv=None, ws=None):
    lib = _lib.load()
    dqkv, ws, nb = _bwd_buffers(qkv, dqkv, ws, lib.ov_attention_backward_workspace_bytes(B, L, H, hd))
    check(lib.ov_attention_backward_saved(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), ptr(dout), dout.stride(0), ptr(dqkv),
                                          dqkv.stride(0), ptr(lse), B, L, H, hd, hd ** -0.5, ptr(ws), nb, stream_ptr()),
          "ov_attention_backward_saved")
    return dqkv


def gemm_tn_batched(p, q, chunk, sums=False):
    """ov_gemm_tn_batched: partials [batch, NI, NJ] bf16 of P^T Q over row ranges of `chunk` contraction rows
    (sums=True: and the fp32 [batch, NI] column sums of P over the same ranges)."""
    lib = _lib.load()
    mc, ni = p.shape
    nj = q.shape[1]
    batch = (mc + chunk - 1) // chunk
    out = torch.empty(batch, ni, nj, dtype=torch.bfloat16, device=p.device)
    ps = torch.full((batch, ni), float("nan"), dtype=torch.float32, device=p.device) if sums else None
    check(lib.ov_gemm_tn_batched(ptr(p), p.stride(0), ptr(q), q.stride(0), ptr(out), nj, ni * nj, mc, ni, nj, chunk, batch, ptr(ps),
                                 stream_ptr()), "ov_gemm_tn_batched")
    return (out, ps) if sums else out


# ---- attention: an fp64 reference with a per-element bound that sees a single mis-handled key (test_gpu_attention_edges.py)


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _split(qkv, B, L, Hh, hd):
    """[B*L, >= 3 Hh hd] -> q, k, v as [B, Hh, L, hd] fp64."""
    D = Hh * hd
    x = qkv[:, :3 * D].double().view(B, L, 3, Hh, hd)
    return [x[:, :, j].transpose(1, 2) for j in range(3)]


def attn_ref64(qkv, B, L, Hh, hd):
    """Softmax attention in fp64 on the (bf16) inputs: (ref, pv), both [B*L, Hh*hd] fp64; pv = P.|V|."""
    q, k, v = _split(qkv, B, L, Hh, hd)
    p = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1)
    back = lambda t: t.transpose(1, 2).reshape(B * L, Hh * hd)
    return back(p @ v), back(p @ v.abs())


def bound(ref, pv):
    """Per-element bound: bf16 output rounding + P rounded to bf16 before P.V (each <= 2^-8 of its term, bf16's unit roundoff: REL is
    that figure with no factor on top)."""
    return REL * ref.abs() + REL * pv + 1e-6


def err_ratio(got, ref, pv):
    """max |got - ref| / bound (<= 1: inside)."""
    return float(((got.double() - ref).abs() / bound(ref, pv)).max())


def spiked_qkv(B, L, Hh, hd, seed, deltas=(4.0, 20.0)):
    """Random bf16 qkv in which, for head j = b * Hh + h, the lone (last) key is K[L-1] = alpha Q[i] with alpha chosen in fp64 so that
    row i's logit of that key exceeds its maximum over the other keys by deltas[j % 2] (log2 units): about 4 leaves the running max
    where it is (the fold's no-rescale branch, p > 1 accumulated), about 20 forces the fold's rescale.  Returns (qkv, [(b, h, i, delta
    realised after rounding K to bf16)])."""
    D = Hh * hd
    qkv = rnd(B * L, 3 * D, seed=seed).to(torch.bfloat16)
    x = qkv.view(B, L, 3, Hh, hd)
    c = hd ** -0.5 * LOG2E
    spikes = []
    for b in range(B):
        for h in range(Hh):
            j = b * Hh + h
            i = (97 * j + 5) % (L - 1)
            qi = x[b, i, 0, h].double()
            m_other = float((x[b, :L - 1, 1, h].double() @ qi).max()) * c
            alpha = (m_other + deltas[j % len(deltas)]) / (float(qi @ qi) * c)
            x[b, L - 1, 1, h] = (alpha * qi).to(torch.bfloat16)
            got = float(x[b, L - 1, 1, h].double() @ qi) * c - m_other
            spikes.append((b, h, i, got))
    for (_, _, _, got), want in zip(spikes, [deltas[j % len(deltas)] for j in range(B * Hh)]):
        assert abs(got - want) < 0.5, (got, want)                   # landed in the intended band after the bf16 rounding
    return qkv, spikes


# the spiked shapes: hd 64 persistent (257), hd 64 streaming (321, 2305), generic chunked (321 at hd 72, 577 at hd 80)
LONE_SPIKED = [(1, 257, 2, 64), (1, 321, 2, 64), (1, 2305, 2, 64), (1, 321, 2, 72), (1, 577, 2, 80)]


# ---- attention backward: an fp64 closed form with per-element bounds on dQ, dK, dV (test_gpu_attention_bwd_edges.py)

U_BWD = 2.0 ** -7                # twice bf16's unit roundoff 2^-8 (8 significant bits): derived in bwd_bound, not measured


def _heads(t, B, L, Hh, hd):
    """[B*L, >= Hh hd] -> [B, Hh, L, hd] fp64."""
    return t[:, :Hh * hd].double().view(B, L, Hh, hd).transpose(1, 2)


def _rows(t):
    """[B, Hh, L, hd] -> [B*L, Hh hd]."""
    B, Hh, L, hd = t.shape
    return t.transpose(1, 2).reshape(B * L, Hh * hd)


class BwdRef:
    """What attn_grads_ref64 returns: dq, dk, dv, o, pv as [B*L, Hh*hd] and p, ds as [B, Hh, L, L], all fp64; q, k, v, do (the inputs
    per head, [B, Hh, L, hd] fp64) and scale ride along for bwd_bound."""


def attn_grads_ref64(qkv, dout, B, L, Hh, hd, mask=None):
    """The attention backward in closed form, fp64 on the (bf16) inputs -- not autograd, because the bound needs P and dS:
        S = scale Q K^T, P = softmax(S) (0 for a pair the [L, L] bool `mask` hides), O = P V, delta = rowsum(dO * O),
        dV = P^T dO, dS = P * (dO V^T - delta), dQ = scale dS K, dK = scale dS^T Q.
    Also pv = P.|V| (the forward bound's second term)."""
    ref = BwdRef()
    ref.q, ref.k, ref.v = q, k, v = _split(qkv, B, L, Hh, hd)
    ref.do = do = _heads(dout, B, L, Hh, hd)
    ref.scale = scale = hd ** -0.5
    s = q @ k.transpose(-1, -2) * scale
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    ref.p = p = torch.softmax(s, dim=-1)
    o = p @ v
    ref.ds = ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    ref.o, ref.pv = _rows(o), _rows(p @ v.abs())
    ref.dq, ref.dk, ref.dv = _rows(ds @ k * scale), _rows(ds.transpose(-1, -2) @ q * scale), _rows(p.transpose(-1, -2) @ do)
    return ref


def bwd_bound(ref, q, k, v, do, scale, eo):
    """Per-element bounds (bound_dq, bound_dk, bound_dv), each [B*L, Hh*hd] fp64.  eo [B*L, Hh*hd]: a bound on |out - O| of the `out`
    tensor the kernel is handed (it forms delta from it).  With U = 2^-7:
        Ed[q]    = sum_d |dO[q, d]| eo[q, d]                   the error of delta
        W        = U |dS| + P Ed                               the error of the bf16 dS that enters the second products
        bound_dV = U |dV| + U (P^T |dO|)        + 1e-6         output rounding + P rounded to bf16
        bound_dQ = U |dQ| + scale (W |K|)       + 1e-6
        bound_dK = U |dK| + scale (W^T |Q|)     + 1e-6
    The kernels round P and dS to bf16 before the second products and their outputs to bf16; each such rounding is at most 2^-8 of
    its magnitude (bf16 has 8 significant bits).  With every rounding aligned the error is the expression above at 2^-8; U is twice
    that, which covers the fp32 exp2 / log2 and the accumulation order.  A derivation: U is not tuned to what the kernels give.
    (v is not needed: dP = dO V^T enters through dS.)"""
    B, Hh, L, hd = q.shape
    ed = (do.abs() * _heads(eo, B, L, Hh, hd)).sum(-1, keepdim=True)                   # [B, Hh, L, 1]
    w = U_BWD * ref.ds.abs() + ref.p * ed
    bdv = U_BWD * ref.dv.abs() + U_BWD * _rows(ref.p.transpose(-1, -2) @ do.abs()) + 1e-6
    bdq = U_BWD * ref.dq.abs() + scale * _rows(w @ k.abs()) + 1e-6
    bdk = U_BWD * ref.dk.abs() + scale * _rows(w.transpose(-1, -2) @ q.abs()) + 1e-6
    return bdq, bdk, bdv


def bwd_err_ratio(got_dqkv, ref, bounds):
    """max |got - ref| / bound for dq, dk, dv (<= 1: inside).  got_dqkv: [B*L, >= 3 Hh hd] as (dq | dk | dv)."""
    D = ref.dq.shape[1]
    got = got_dqkv.double()
    return tuple(float(((got[:, j * D:(j + 1) * D] - want).abs() / bd).max())
                 for j, (want, bd) in enumerate(zip((ref.dq, ref.dk, ref.dv), bounds)))


def spiked_bwd_case(B, L, Hh, hd, seed, boost=32.0):
    """Random bf16 (qkv, dout) for the backward's tails.  For head j = b * Hh + h and row i = (97 j + 5) % (L - 1), the last key is
    K[L-1] = alpha Q[i] with alpha chosen in fp64 so that its log2 logit in row i equals the log2-sum-exp of the other keys: key L - 1
    then holds half of row i's softmax, which maximises its dS (a spike that takes the whole row gives P ~ 1 and dS ~ 0: nothing for a
    backward to get wrong).  dout[L-1] is multiplied by `boost`, so that the last query -- alone in its tile or chunk at L = 32 k + 1 /
    256 k + 1 -- dominates its column of dK and dV.  Returns (qkv, dout, [(b, h, i, weight of key L - 1 in row i after the bf16
    rounding of K)]); the weight is asserted to lie in [0.3, 0.7]."""
    D = Hh * hd
    qkv = rnd(B * L, 3 * D, seed=seed).to(torch.bfloat16)
    dout = rnd(B * L, D, seed=seed + 1).to(torch.bfloat16)
    x = qkv.view(B, L, 3, Hh, hd)
    c = hd ** -0.5 * LOG2E
    probes = []
    for b in range(B):
        for h in range(Hh):
            i = (97 * (b * Hh + h) + 5) % (L - 1)
            qi = x[b, i, 0, h].double()
            lse_other = float(torch.logsumexp(x[b, :L - 1, 1, h].double() @ qi * (c / LOG2E), 0)) * LOG2E
            x[b, L - 1, 1, h] = (lse_other / (float(qi @ qi) * c) * qi).to(torch.bfloat16)
            logit = float(x[b, L - 1, 1, h].double() @ qi) * c
            weight = 1.0 / (1.0 + 2.0 ** (lse_other - logit))
            assert 0.3 <= weight <= 0.7, (b, h, i, weight)
            probes.append((b, h, i, weight))
    dout.view(B, L, D)[:, L - 1] *= boost
    return qkv, dout, probes
