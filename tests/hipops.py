"""Thin test-side wrappers: torch tensors -> C ABI calls of libovhip.so (granular operators)."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch

from openvision_amd import _lib
from openvision_amd._lib import ptr, stream_ptr, check, OV_BF16, OV_F32


LOG2E = 1.4426950408889634
REL = 2.0 ** -8                  # the attention bound's relative terms (bound() below)


def _flag(t):
    return OV_F32 if t.dtype == torch.float32 else OV_BF16


def layernorm(x, g, b, eps=1e-6, out_dtype=None, out=None):
    """x, out: bf16 or fp32, each side on its own.  A 2-D x with unit column stride goes in as it is, its row pitch as ldx (a view of
    a wider buffer, or rows L D apart); out (optional): a caller-owned [rows, >= D] view, its row pitch as ldy."""
    lib = _lib.load()
    D = x.shape[-1]
    x2 = x if x.dim() == 2 and x.stride(1) == 1 else x.contiguous().view(-1, D)
    y = out if out is not None else torch.empty(x2.shape, dtype=out_dtype or x.dtype, device=x.device)
    check(lib.ov_layernorm(ptr(x2), _flag(x2), x2.stride(0), ptr(g), ptr(b), ptr(y), _flag(y), y.stride(0), x2.shape[0],
                           D, eps, stream_ptr()), "ov_layernorm")
    return y if out is not None else y.view(x.shape)


def gemm(a, w, bias=None, epi=0, resid=None, out=None, out_group=0, resid_mod=0, resid_off=0, out_rows=None):
    lib = _lib.load()
    m, k = a.shape
    n = w.shape[0]
    if out is None:
        out = torch.zeros(out_rows or m, n, dtype=torch.bfloat16, device=a.device)
    check(lib.ov_gemm(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(out), out.stride(0), m, n, k, epi,
                      ptr(resid), resid.stride(0) if resid is not None else 0, out_group, resid_mod, resid_off, stream_ptr()))
    return out


def gemm_keep(a, w, bias, epi, ldc=None, ldc2=None, fill=0.0, out=None, pre=None):
    """C = gelu(a w^T + bias), C2 = a w^T + bias (both bf16) from one launch: ov_gemm_keep.  fill: what both outputs hold before.
    out= / pre=: caller-owned [M, >= N] bf16 outputs, each with its own row pitch."""
    lib = _lib.load()
    m, k = a.shape
    n = w.shape[0]
    if out is None:
        out = torch.full((m, ldc or n), fill, dtype=torch.bfloat16, device=a.device)
    if pre is None:
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


ATTN_FWD_KERNELS = ("persistent", "streaming", "generic")           # enum ov_attn_fwd_kernel
ATTN_BWD_KERNELS = ("resident", "streaming")                        # enum ov_attn_bwd_kernel


def attn_route(B, L, Hh, hd=64, prefix=None, out8=False, lse=False, ld_qkv=0, ld_out=0, cus=0):
    """What attention.hip / attention_bwd.hip decide for this call, from the library itself (ov_attention_route; it launches nothing;
    cus = 0: this device's CU count; under the OVHIP_ATTN_LONEKEY of THIS process).  prefix None: the unmasked entry points; ld_* 0:
    dense rows.  The fields of ov_attention_route_t under their own names, the two kernels as names (kernel: forward, bwd: backward),
    grid as a tuple, and the two forms as the tests' comments write them: form = persistent | streaming | generic resident | generic
    chunked (+ " mask"), bwd_form = resident | resident saved | stream<2> | stream<3> (+ " mask").  A combination no entry point
    admits raises (check)."""
    r = _lib.AttentionRoute()
    check(_lib.load().ov_attention_route(B, L, Hh, hd, ld_qkv, ld_out, -1 if prefix is None else prefix, int(out8), int(lse), cus,
                                         C.addressof(r)), "ov_attention_route")
    d = {n: getattr(r, n) for n, _ in r._fields_}
    for n in ("deep", "out8", "lse", "mask", "resident", "bwd_saved", "bwd_mask", "keep_lse"):
        d[n] = bool(d[n])
    kernel, bwd = ATTN_FWD_KERNELS[r.fwd_kernel], ATTN_BWD_KERNELS[r.bwd_kernel]
    form = kernel + ((" resident" if r.resident else " chunked") if kernel == "generic" else "") + (" mask" if r.mask else "")
    bwd_form = ("resident" + (" saved" if r.bwd_saved else "")) if bwd == "resident" else f"stream<{r.ndh}>" + (" mask" if r.bwd_mask else "")
    return SimpleNamespace(kernel=kernel, bwd=bwd, form=form, bwd_form=bwd_form, grid=(r.grid_x, r.grid_y), **d)


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


def _own_ws(ws, nb, device):
    """ws=None: a fresh workspace with 256 spare bytes, handed over as `nb` bytes; else the caller's uint8 tensor, handed over with
    its own size (e.g. a view of exactly `nb` bytes, to watch what lies behind it)."""
    if ws is None:
        return torch.empty(nb + 256, dtype=torch.uint8, device=device), nb
    assert ws.dtype == torch.uint8 and ws.is_contiguous()
    return ws, ws.numel()


def linear_backward(dy, x, w, want=("dx", "dw", "db"), dx=None, dw=None, db=None, ws=None):
    """ov_linear_backward for y = x w^T + b: returns (dX bf16 [M,K] | None, dW bf16 [N,K] | None, db fp32 [N] | None).  dx= / dw= /
    db=: caller-owned outputs for the gradients named in `want` (dx, dw with their own row pitch); ws=: a caller-owned workspace.
    x may be None when dX alone is wanted (the block chain's c_proj dX)."""
    lib = _lib.load()
    M, N = dy.shape
    K = w.shape[1]
    dx = _out_buf(dx, M, K, torch.bfloat16, None, dy.device) if "dx" in want else None
    dw = _out_buf(dw, N, K, torch.bfloat16, None, dy.device) if "dw" in want else None
    db = (db if db is not None else torch.empty(N, dtype=torch.float32, device=dy.device)) if "db" in want else None
    ws, nb = _own_ws(ws, lib.ov_linear_backward_workspace_bytes(M, N, K), dy.device)
    check(lib.ov_linear_backward(ptr(dy), dy.stride(0), ptr(x), x.stride(0) if x is not None else K, ptr(w), w.stride(0), M, N, K,
                                 ptr(dx) if dx is not None else None, dx.stride(0) if dx is not None else K,
                                 ptr(dw) if dw is not None else None, dw.stride(0) if dw is not None else K,
                                 ptr(db) if db is not None else None, ptr(ws), nb, stream_ptr()), "ov_linear_backward")
    return dx, dw, db


def linear_backward_plan(M, N, K):
    """ov_linear_backward_plan: (nz, chunk, tn_route) -- for coverage assertions only, never for a bound."""
    lib = _lib.load()
    nz, chunk, tn = C.c_int(-1), C.c_int64(-1), C.c_int(-1)
    check(lib.ov_linear_backward_plan(M, N, K, C.addressof(nz), C.addressof(chunk), C.addressof(tn)), "ov_linear_backward_plan")
    return nz.value, chunk.value, bool(tn.value)


def transpose(x):
    lib = _lib.load()
    R, C = x.shape
    rp = (R + 63) // 64 * 64
    out = torch.full((C, rp), 7.0, dtype=torch.bfloat16, device=x.device)
    check(lib.ov_transpose_bf16(ptr(x), x.stride(0), R, C, ptr(out), rp, stream_ptr()), "ov_transpose_bf16")
    return out


def layernorm_backward(x, gamma, dy, eps=1e-6, dres=None, dx=None, ws=None):
    """dx=: a caller-owned [rows, D] bf16 output with its own row pitch; ws=: a caller-owned workspace."""
    lib = _lib.load()
    rows, D = x.shape
    dx = _out_buf(dx, rows, D, torch.bfloat16, None, x.device)
    dg = torch.empty(D, dtype=torch.float32, device=x.device)
    db = torch.empty(D, dtype=torch.float32, device=x.device)
    ws, nb = _own_ws(ws, lib.ov_layernorm_backward_workspace_bytes(rows, D), x.device)
    check(lib.ov_layernorm_backward(ptr(x), x.stride(0), ptr(gamma), ptr(dy), dy.stride(0), ptr(dres) if dres is not None else None,
                                    dres.stride(0) if dres is not None else 0, ptr(dx), dx.stride(0), ptr(dg), ptr(db),
                                    rows, D, eps, ptr(ws), nb, stream_ptr()), "ov_layernorm_backward")
    return dx, dg, db


def gelu_backward(a, dh, tanh, with_h=False, da=None, h=None, inplace=False):
    """da= / h=: caller-owned [rows, N] bf16 outputs with their own row pitch (h= implies with_h); inplace=True: da is dh itself, as
    the block's backward chain calls it."""
    lib = _lib.load()
    rows, N = a.shape
    assert not (inplace and da is not None)
    da = dh if inplace else _out_buf(da, rows, N, torch.bfloat16, None, a.device)
    with_h = with_h or h is not None
    if with_h:
        h = _out_buf(h, rows, N, torch.bfloat16, None, a.device)
    check(lib.ov_gelu_backward(ptr(a), a.stride(0), ptr(dh), dh.stride(0), ptr(da), da.stride(0), ptr(h) if with_h else None,
                               h.stride(0) if with_h else 0, rows, N, int(tanh), stream_ptr()), "ov_gelu_backward")
    return (da, h) if with_h else da


def block_backward(cfg, weights, x, dy, B, L, saved=None, prefix=None):
    """ov_block_backward (prefix: ov_block_backward_prefix).  weights: dict of the module's own tensors (ln1_w, ln1_b fp32; qkv_w bf16
    [3D, D]; qkv_b fp32; ...); saved: an ov_block_saved (block_saved_of) or None, everything recomputed.  Returns (dx bf16, grads dict)."""
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
    sv = C.byref(saved) if saved is not None else None
    if prefix is None:
        check(lib.ov_block_backward(C.byref(cfg), C.byref(wst), ptr(x), sv, ptr(dy), ptr(dx), C.byref(gst), B, L, ptr(ws), nb, stream_ptr()),
              "ov_block_backward")
    else:
        check(lib.ov_block_backward_prefix(C.byref(cfg), C.byref(wst), ptr(x), sv, ptr(dy), ptr(dx), C.byref(gst), prefix, B, L, ptr(ws), nb,
                                           stream_ptr()), "ov_block_backward_prefix")
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
    return (dqkv,) + _own_ws(ws, nb, qkv.device)


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


# ---- linear / LayerNorm / GELU backward: fp64 closed forms with per-element bounds (test_gpu_param_grad_edges.py; what the bounds can
# see is pinned on the CPU by test_param_grad_bound.py)

U16 = 2.0 ** -8                  # bf16's unit roundoff: 8 significant bits, round to nearest
E32 = 2.0 ** -24                 # fp32's


def linear_grads_ref64(dy, x, w):
    """y = x w^T + b in fp64 on the (bf16) inputs: (dX [M, K], dW [N, K], db [N])."""
    dy, x, w = dy.double(), x.double(), w.double()
    return dy @ w, dy.T @ x, dy.sum(0)


def linear_bounds(dy, x, w):
    """Per-element bounds (bound_dX [M, K], bound_dW [N, K], bound_db [N]) on ov_linear_backward, fp64, from the inputs alone: nothing
    here knows the split-K plan, the route or the device.  u = 2^-8, e = 2^-24.

        bound_dX = u |dX| + N e (|dY| |W|) + 1e-6
    dX is one fp32-accumulated product over N (a sum of n terms in any order is off by at most n e sum|terms| to first order) and
    one bf16 rounding of the result.

        T[n, k]  = sum over 64-row tiles t of | sum_{m in t} dY[m, n] X[m, k] |          (rows past M: zeros)
        bound_dW = u (|dW| + T) + M e (|dY|^T |X|) + 1e-6
    dW is cut into row ranges; each range's fp32 product P_z is rounded to bf16 (at most u |P_z|), the partials are summed in fp32 and
    the sum is rounded to bf16 once more (u |dW|).  Whatever the plan, a range is a whole number of 64-row tiles (the K granule of
    the GEMM), so |P_z| <= sum of its tiles' |tile sum| and sum_z |P_z| <= T: the worst plan is one range per tile.  The fp32 work
    is `chunk` terms inside a range and `nz` terms across ranges, chunk + nz <= M + 2 terms in all; M e (|dY|^T |X|) covers it with
    the second-order terms in the + 1e-6.  With one range there is no partial rounding and the bound is merely not tight.

        bound_db = (M + 2) e sum_m |dY| + 1e-7
    an fp32 sum of M terms in any order (per tile, per range or per 256-row chunk first)."""
    M, N = dy.shape
    dy, x, w = dy.double(), x.double(), w.double()
    dx_ref, dw_ref, _ = linear_grads_ref64(dy, x, w)
    bdx = U16 * dx_ref.abs() + N * E32 * (dy.abs() @ w.abs()) + 1e-6
    mp = (M + 63) // 64 * 64
    dyp, xp = torch.zeros(mp, N, dtype=torch.float64), torch.zeros(mp, x.shape[1], dtype=torch.float64)
    dyp[:M], xp[:M] = dy, x
    t = torch.zeros_like(dw_ref)
    for i in range(0, mp, 64):
        t += (dyp[i:i + 64].T @ xp[i:i + 64]).abs()
    bdw = U16 * (dw_ref.abs() + t) + M * E32 * (dy.abs().T @ x.abs()) + 1e-6
    bdb = (M + 2) * E32 * dy.abs().sum(0) + 1e-7
    return bdx, bdw, bdb


def spiked_linear_case(M, N, K, seed, boost=8.0):
    """Gaussian bf16 (dy [M, N], x [M, K], w [N, K] / sqrt K) in which rows 0, 63, 64 and M - 1 (those that exist) of dy AND of x
    are `boost` times larger: each of these rows -- the first and last of the first 64-row tile, the first of the second, the last
    of all -- then carries boost^2 times an ordinary row's share of dW, so that dropping or doubling it stands far outside the
    bound."""
    dy, x = rnd(M, N, seed=seed), rnd(M, K, seed=seed + 1)
    w = (rnd(N, K, seed=seed + 2) * K ** -0.5).to(torch.bfloat16)
    for r in sorted({0, 63, 64, M - 1}):
        if r < M:
            dy[r] *= boost
            x[r] *= boost
    return dy.to(torch.bfloat16), x.to(torch.bfloat16), w


class LnRef:
    """What ln_grads_ref64 returns: dx [R, D], dgamma, dbeta [D] and the bounds bdx, bdg, bdb of the same shapes, all fp64."""


def ln_grads_ref64(x, gamma, dy, dres, eps):
    """The LayerNorm backward in closed form, fp64 on the inputs the kernel reads (bf16 x, dy, dres; fp32 gamma; dres may be None):
        xhat = (x - mean) rstd,  q = dy gamma,  dx = rstd (q - mean q - xhat mean(q xhat)) + dres,
        dgamma = sum_r dy xhat,  dbeta = sum_r dy
    with per-element bounds on what ov_layernorm_backward may return.  u = 2^-8, e = 2^-24, means over the D columns of a row.

    xhat first.  The fp32 mean is a D-term sum: off by at most D e mean|x|; x - mean adds one rounding, e (|x| + mean|x|); the
    variance is a D-term sum of squares whose first-order sensitivity to the mean's error vanishes (sum (x - mean) = 0), so rstd
    is off relatively by about (D / 2 + 3) e, rsqrt's ulp included; the product rounds once more:
        dxh = e ((D + 4) (|x| + mean|x|) rstd + (D + 6) |xhat|)
    (the first term is what grows when mean >> spread: cancellation in x - mean).

    dx: q is one rounding; mean q a D-term sum; mean(q xhat) a D-term fma chain over products that carry xhat's error; the bracket
    t = q - mean q - xhat mean(q xhat) is assembled with a few more roundings, multiplied by rstd (relative error as above), dres
    is added and the result is rounded to bf16 once:
        bdx = u |dx| + e (D + 8) rstd (|q| + mean|q| + |xhat| mean|q xhat|)                 the fp32 sums and roundings
                     + rstd (dxh |mean(q xhat)| + |xhat| mean(|q| dxh))                      xhat's error, both places it enters
                     + rstd (D + 6) e |t| + 1e-7                                             rstd's own error
    dgamma: an fp32 sum over R rows (per wave, then over the waves: any order) of products that carry xhat's error:
        bdg = (R + 2) e sum_r |dy xhat| + sum_r |dy| dxh + 1e-7
    dbeta: bdb = (R + 2) e sum_r |dy| + 1e-7."""
    x, g, dy = x.double(), gamma.double(), dy.double()
    R, D = x.shape
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = ((xc ** 2).mean(1, keepdim=True) + eps).rsqrt()
    xh = xc * rstd
    q = dy * g
    mq, mqx = q.mean(1, keepdim=True), (q * xh).mean(1, keepdim=True)
    t = q - mq - xh * mqx
    ref = LnRef()
    ref.dx = rstd * t + (dres.double() if dres is not None else 0.0)
    ref.dgamma, ref.dbeta = (dy * xh).sum(0), dy.sum(0)
    dxh = E32 * ((D + 4) * (x.abs() + x.abs().mean(1, keepdim=True)) * rstd + (D + 6) * xh.abs())
    ref.bdx = (U16 * ref.dx.abs()
               + E32 * (D + 8) * rstd * (q.abs() + q.abs().mean(1, keepdim=True) + xh.abs() * (q * xh).abs().mean(1, keepdim=True))
               + rstd * (dxh * mqx.abs() + xh.abs() * (q.abs() * dxh).mean(1, keepdim=True))
               + rstd * (D + 6) * E32 * t.abs() + 1e-7)
    ref.bdg = (R + 2) * E32 * (dy * xh).abs().sum(0) + (dy.abs() * dxh).sum(0) + 1e-7
    ref.bdb = (R + 2) * E32 * dy.abs().sum(0) + 1e-7
    return ref


def ln_err_ratio(dx, dg, db, ref):
    """max |got - ref| / bound for (dx, dgamma, dbeta) (<= 1: inside)."""
    return (float(((dx.double() - ref.dx).abs() / ref.bdx).max()), float(((dg.double() - ref.dgamma).abs() / ref.bdg).max()),
            float(((db.double() - ref.dbeta).abs() / ref.bdb).max()))


def spiked_ln_case(rows, D, seed, mean=0.2, spread=1.5, boost=32.0, tail=4.0):
    """(x bf16 [rows, D] ~ mean + spread N(0, 1), gamma fp32 [D] ~ 1 + 0.1 N(0, 1), dy bf16, dres bf16), rows 0 and rows - 1 of dy
    `boost` times larger: a first or last row that is dropped, or overwritten by a wave's next row, stands far outside the
    parameter bounds.  The last 8 columns of x (the last chunk, which a lone lane holds at D = 520, 1032, 1544, 2056) sit `tail`
    spreads higher, an outlier channel group: a row statistic that leaves that chunk out is visibly wrong in dx.  mean = 8 (with
    spread 1.5) is the cancellation case of the variance."""
    x = rnd(rows, D, seed=seed) * spread + mean
    x[:, D - 8:] += tail * spread
    x = x.to(torch.bfloat16)
    dy = rnd(rows, D, seed=seed + 1)
    dy[0] *= boost
    dy[rows - 1] *= boost if rows > 1 else 1.0
    gamma = rnd(D, seed=seed + 2) * 0.1 + 1
    dres = rnd(rows, D, seed=seed + 3).to(torch.bfloat16)
    return x, gamma, dy.to(torch.bfloat16), dres


# delta: the absolute error of the fp32 gelu' (and of Phi resp. sigmoid, which gives h = a Phi) as backward.hip evaluates them.
#   erf form:  Phi = 1 - half_erfc or half_erfc, half_erfc = 0.5 p(t) exp(-a^2 / 2).  A&S 7.1.26 is within 1.5e-7 of erfc, so 0.75e-7
#     of Phi.  t comes from a one-ulp rcp; the five-term Horner chain has intermediates <= 1.46 and t <= 1: <= 8 e on p t; exp2's
#     argument is rounded twice (its effect on exp2 is <= 2 e |arg| ln 2 exp2(arg) <= 0.74 e) and exp2 is within one ulp: <= 2 e;
#     half the sum, plus one rounding of 1 - half_erfc: <= 6 e on Phi.  gelu' adds a phi(a) (<= 0.242, relative error <= 5 e plus
#     the same argument term, <= 2 e absolute) and one fma rounding (<= 1.13 e): delta_erf = 0.75e-7 + 10 e = 6.7e-7.
#   tanh form: sg = rcp(1 + exp2(-2 log2(e) u)).  The argument's relative error is <= 4 e, which moves sg by <= 4 e |2u| sg (1 - sg)
#     <= 0.9 e; exp2, the addition and rcp add <= 2.3 e: <= 3.2 e on sg (h = a sg).  gelu' = sg + 2 a sg (1 - sg) u'.  Where sg is not
#     close to 1 the second term (<= 0.65 in magnitude) keeps a relative error <= 8 e and inherits sg's error times |2 a u' (1 - 2 sg)|:
#     <= 8 e in all, 4.8e-7.  For a > 2.6 this stops: 1 - sg cancels (sg carries an absolute error up to 2 e, 1 - sg is of that
#     order) while its factor 2 a u' grows like a^3, and the derivative's error reaches min(2 e, 1 - sg) 2 a u' = 3.7e-6 near a = 4.8
#     (1.9e-6 in the fp32 emulation of test_param_grad_bound.py; 0 again from a = 5.3, where sg is 1 exactly).  That is above the
#     1e-6 that the kernel's tests quote.  It is harmless -- gelu' is within 3 % of 1 there, so the bf16 rounding of da, 3.9e-3 |dh|,
#     is three orders larger -- and the kernel stays as it is (the GEMM's GELU_GRAD epilogue shares the form and is pinned bitwise).
#     DELTA_TANH is held at the quoted 1e-6 all the same: the tests do not widen it for that band.
DELTA_ERF = 0.75e-7 + 10 * E32
DELTA_TANH = 1e-6
assert DELTA_ERF <= 1e-6 and DELTA_TANH <= 1e-6
BF16_TINY = 2.0 ** -134          # half the spacing of the subnormal bf16 numbers


def gelu_grads_ref64(a, dh, tanh):
    """(da, h) = (dh gelu'(a), gelu(a)) in fp64 on the (bf16) inputs; erf form: Phi(a) + a phi(a) and a Phi(a) with Phi through
    erfc (no cancellation in the negative tail); tanh form through sigmoid(2u), u = sqrt(2 / pi) (a + 0.044715 a^3)."""
    a, dh = a.double(), dh.double()
    if tanh:
        c = 0.7978845608028654
        s = torch.sigmoid(2.0 * c * (a + 0.044715 * a ** 3))
        grad = s + 2.0 * a * s * (1.0 - s) * c * (1.0 + 3.0 * 0.044715 * a * a)
    else:
        s = 0.5 * torch.special.erfc(-a * 0.7071067811865476)
        grad = s + a * torch.exp(-0.5 * a * a) * 0.3989422804014327
    return dh * grad, a * s           # finite on |a| <= 2^16: every factor that saturates does so to exactly 0 or 1 beside finite ones


def gelu_bounds(a, dh, tanh, ref=None):
    """(bound_da, bound_h): |da err| <= u |da| + |dh| delta and |h err| <= u |h| + |a| delta -- one bf16 rounding of each output plus
    the fp32 formula's absolute error delta (DELTA_ERF / DELTA_TANH above), which reaches da through dh and h through a.  u |.| is
    the rounding of a normal bf16 result; a subnormal one (h = a Phi at the subnormal a of the all-values case) is rounded to the
    subnormal spacing 2^-133 instead, so half of that, BF16_TINY = 2^-134, is added to both.  ref: gelu_grads_ref64's result, if
    the caller has it."""
    da, h = ref if ref is not None else gelu_grads_ref64(a, dh, tanh)
    delta = DELTA_TANH if tanh else DELTA_ERF
    return U16 * da.abs() + dh.double().abs() * delta + BF16_TINY, U16 * h.abs() + a.double().abs() * delta + BF16_TINY


def gelu_err_ratio(da, h, a, dh, tanh):
    """max |got - ref| / bound for (da, h) (<= 1: inside); a NaN anywhere gives nan, which no `<= 1.0` passes."""
    ref = gelu_grads_ref64(a, dh, tanh)
    r = []
    for got, want, bd in zip((da, h), ref, gelu_bounds(a, dh, tanh, ref)):
        q = (got.double() - want).abs() / bd
        r.append(float("nan") if bool(torch.isnan(q).any()) else float(q.max()))
    return tuple(r)


def all_bf16_values(limit=2.0 ** 16):
    """Every finite bf16 value with |a| <= limit, -0.0 and the subnormals included, in bit-pattern order."""
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    f = bits.float()
    return bits[torch.isfinite(f) & (f.abs() <= limit)]


# the shapes of test_gpu_param_grad_edges.py (test_param_grad_bound.py runs its emulations at the same ones)
LINEAR_NK = [(64, 64), (192, 320), (320, 64)]          # the 256-wide output tile ragged in N, in K and in neither
LINEAR_TN_M = [64, 512, 1088, 2048, 16384]             # M % 64 == 0: dW straight from the row-major operands
LINEAR_TR_M = [70, 1100, 8200]                         # explicit transposes, zeros past M
DB_BOOST_LARGE_M = 512.0                               # the spike of the db-alone case at M = 33027, where bound_db is 52 per column
LN_SHAPES = [(1, 8), (5, 200), (129, 200), (37, 520), (9, 1032), (9, 1152), (5, 1544), (5, 2056), (5, 4096), (4099, 64), (8195, 1152)]
GELU_DH = (1.0, -3.0, 2.0 ** -20)


def gelu_all_values_case():
    """(a, dh) bf16 [3 * rows, 8]: every finite bf16 |a| <= 2^16 (padded with zeros to a multiple of 8) against each dh of GELU_DH."""
    v = all_bf16_values()
    pad = (-v.numel()) % 8
    v = torch.cat([v, torch.zeros(pad, dtype=torch.bfloat16)]).view(-1, 8)
    a = torch.cat([v] * len(GELU_DH))
    dh = torch.cat([torch.full(v.shape, d, dtype=torch.bfloat16) for d in GELU_DH])
    return a, dh


# ---- the bf16 GEMM kernels against fp64 (test_gpu_gemm_routes.py: the persistent kernel; test_gpu_gemm_small_routes.py: the skinny and
# plain kernels, ov_gemm_batched, the LN fold; what the bounds can see is pinned on the CPU by test_gemm_small_bound.py).  The bounds
# are derived in the module docstring of test_gpu_gemm_routes.py (bias, residual, GELU), at linear_ratios (GELU gradient) and at fold_bound below.

DEV = "cuda:0"
BM = BN = 256
SENT = 77.0
E_TANH = 1.1e-6
CHUNK = 4096                      # rows per fp64 chunk: 4096 x 4096 x 8 B = 128 MB for the widest N of the routes test


KERNELS = ("skinny", "plain", "persistent")            # enum ov_gemm_kernel


def route(M, N, K, epi=0, keep=False, fold=False, rowparts=False, mapped=False, cus=0):
    """What gemm.hip's launcher decides for this call, from the library itself (ov_gemm_route; cus = 0: this device's CU count, under
    the OVHIP_GEMM_* switches of THIS process), beside the shape arithmetic of the case: tm x tn = nwg tiles, rem columns in the last
    n-tile, pr = tm mod 8, W's bytes.  The instantiation flags and extra launches ride along under the names of ov_gemm_route_t."""
    r = _lib.GemmRoute()
    check(_lib.load().ov_gemm_route(M, N, K, epi, int(fold), int(keep), int(rowparts), int(mapped), cus, C.addressof(r)), "ov_gemm_route")
    cus = cus or torch.cuda.get_device_properties(0).multi_processor_count
    tm, tn = -(-M // BM), -(-N // BN)
    return SimpleNamespace(cus=cus, tm=tm, tn=tn, nwg=tm * tn, rem=N % BN, pr=tm & 7, wbytes=tn * BN * K * 2,
                           kernel=KERNELS[r.kernel], grouped=r.ngroup < tn, groups=tn // r.ngroup, rot=r.rotmask, rev=bool(r.rev),
                           st_plain=bool(r.st_plain), **{n: bool(getattr(r, n)) for n in ("fold", "direct", "mapped", "keep", "stats",
                                                                                           "keep_prepass", "rowparts_pass")})


def gelu64(x, tanh):
    return torch.nn.functional.gelu(x, approximate="tanh" if tanh else "none")


def _worst(err, bound, row0):
    q = err / bound
    k = int(q.argmax())
    return float(q.view(-1)[k]), row0 + k // q.shape[1], k % q.shape[1]


def _merge(res, name, item):
    old = res.get(name)
    if old is None or math.isnan(item[0]) or item[0] > old[0]:        # (a NaN is kept: it fails the assertion)
        res[name] = item


def linear_ratios(a, w, bias, outs, r=None):
    """outs: name -> (bf16 [M, >= N], kind), kind in pre | erf | tanh | res | res1 | gerf | gtanh (res1: the residual under the
    ONE-rounding bound, for the record; gerf / gtanh: the GELU-gradient epilogues, r = the pre-activation they differentiate at).  Returns name -> (max err / bound, row, column) against fp64 on the device, in row chunks."""
    M, K = a.shape
    N = w.shape[0]
    wd, wabs, bd = w.double(), w.float().abs(), bias.double()
    res = {}
    for i in range(0, M, CHUNK):
        sl = slice(i, min(M, i + CHUNK))
        pre = a[sl].double() @ wd.T + bd
        s = (a[sl].float().abs() @ wabs.T + bias.abs()).double()
        b_pre = REL * pre.abs() + K * 2.0 ** -24 * s + 1e-6
        for name, (got, kind) in outs.items():
            g = got[sl, :N].double()
            if kind == "pre":
                ref, bound = pre, b_pre
            elif kind in ("res", "res1"):
                rr = r[sl].double()
                ref = pre + rr
                bound = REL * ref.abs() + K * 2.0 ** -24 * (s + rr.abs()) + 1e-6
                if kind == "res":
                    bound = bound + REL * (1 + REL) * pre.abs()
            elif kind in GRAD_DELTA:
                # GELU-gradient epilogue, out = bf16(bf16(pre) g32(R)), against ref = pre g'(R) with the exact fp64 g'.  The rounded
                # pre is off by at most b_pre, and that error is carried with the factor |g32| <= |g'| + delta; g32 is within delta of
                # g', on the magnitude |pre|; the product is rounded once:
                #     |g'(R)| b_pre + delta (|pre| + b_pre) + REL |ref|
                gd = gelu_grads_ref64(r[sl], torch.ones_like(r[sl]), kind == "gtanh")[0]
                ref = pre * gd
                bound = gd.abs() * b_pre + GRAD_DELTA[kind] * (pre.abs() + b_pre) + REL * ref.abs()
            else:
                ref = gelu64(pre, kind == "tanh")
                e = E_TANH if kind == "tanh" else torch.clamp(6.6e-5 * pre.abs(), min=1.4e-4)
                bound = 1.13 * b_pre + REL * ref.abs() + e
            _merge(res, name, _worst((g - ref).abs(), bound, i))
    return res


def report(tag, res, skip=()):
    for name, (q, row, col) in res.items():
        print(f"{tag} {name}: max err / bound {q:.3f}")
    bad = {n: (q, f"row {row} column {col} = tile ({row // BM}, {col // BN})") for n, (q, row, col) in res.items()
           if n not in skip and not q <= 1.0}
    assert not bad, (tag, bad)


def sentinel(M, width):
    return torch.full((M, width), SENT, dtype=torch.bfloat16, device=DEV)


def padding_kept(out, N):
    return bool((out[:, N:] == SENT).all())




# delta of the GEMM's GELU-gradient epilogues (common.h): the absolute error of the fp32 gelu' against the exact fp64 derivative.
#   erf form (gelu_erf_grad_f2x2, a degree-7 polynomial fit): common.h states |error| <= 4.3e-4 everywhere; the figure is taken from
#     there (a restatement in fp32 on a 2^-12 grid over [-8, 8] gives 4.264e-4, at the clamp x = 4: test_gemm_small_bound.py prints it).
#   tanh form (gelu_tanh_grad_f2, the closed form through sigmoid(2u)): common.h states no figure.  The restatement in fp32, the same
#     operation order, on the 2^-12 grid over [-8, 8] differs from the fp64 derivative by at most 1.969e-6 (at x = 4.962, where 1 - sg
#     cancels: the band that DELTA_TANH's comment above describes); with the factor 2, as for E_TANH: 3.94e-6.
DELTA_GRAD_ERF = 4.3e-4
DELTA_GRAD_TANH = 3.94e-6
GRAD_DELTA = {"gerf": DELTA_GRAD_ERF, "gtanh": DELTA_GRAD_TANH}


def gemm_batched(a, lda, stride_a, w, ldw, stride_w, out, ldc, stride_c, M, N, K, batch):
    """ov_gemm_batched: C_z = A_z W_z^T for z < batch, every pointer, pitch and stride (in elements) as the caller gives it."""
    lib = _lib.load()
    check(lib.ov_gemm_batched(ptr(a), lda, stride_a, ptr(w), ldw, stride_w, ptr(out), ldc, stride_c, M, N, K, batch, stream_ptr()),
          "ov_gemm_batched")
    return out


def pitched(t, pad=8, fill=float("nan")):
    """t [rows, cols] as a view of a buffer `pad` columns wider whose padding holds `fill` (NaN: an operand read past its K or N
    columns poisons the output)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


# the shapes of test_gpu_gemm_small_routes.py (test_gemm_small_bound.py runs its emulation at the same ones): (M, N, K)
SKINNY_SHAPES = [(1, 8, 64),              # one row, one quad, one K-tile
                 (65, 72, 128),           # ragged both ways, 2 K-tiles
                 (130, 200, 192),         # 3 K-tiles = the prefetch depth
                 (257, 264, 256),         # 4 K-tiles = the ring
                 (63, 1096, 320),         # 5 K-tiles: the first slot reuse; the last n-tile holds 8 columns
                 (300, 96, 576)]          # two laps of the ring
PLAIN_SHAPES = [(24827, 8, 64),           # 97 tiles (97 mod 8 = 1 in the XCD map), one K-tile
                (1, 24584, 128),          # 97 column tiles, the last holds 8 columns; every A row clamped to row 0
                (2500, 2568, 192),        # 110 tiles (110 mod 8 = 6)
                (2305, 2816, 320)]        # 110 tiles
SKINNY_ALL_EPI = [(130, 200, 192), (63, 1096, 320)]
PLAIN_ALL_EPI = [(2500, 2568, 192)]
ROWMAP_CASE = (3, 50, 200, 192)           # (B, g^2, D, K): the patch embedding with row maps at a small batch (skinny kernel)
MAPPED_GELU_CASE = (25000, 200, 64, 50)   # (M, N, K, out_group): GELU-erf with out_group, which the ABI admits and the plain kernel runs
BATCHED_CASE = (300, 264, 128, 3)         # (M, N, K, batch)
ROWPARTS_SHAPES = [(257, 288, 256), (300, 96, 576), (2500, 2592, 192)]          # N / 32 odd in all three; the last is the plain kernel's
FOLD_SHAPES = [s for s in SKINNY_SHAPES if 128 <= s[2] <= 320] + PLAIN_SHAPES[2:]
FOLD_CLEAN_ONLY = (130, 200, 1024)        # K = 1024: the K S1 term is too pessimistic there for the double-rounding mistakes


def gemm_case(M, N, K, r_rows=None):
    """CPU operands (a bf16 [M, K], w bf16 [N, K] / sqrt K, bias fp32 [N], r bf16 [r_rows or M, N]), Gaussian; r (the residual, or the
    pre-activation the GELU-gradient epilogues differentiate at) with spread 2, so that 4.6 % of it lies beyond the erf form's clamp
    at |x| = 4 and in the tanh form's cancelling band."""
    g = torch.Generator().manual_seed(1000003 * K + 1009 * N + M + 5)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    return a, w, bias, (torch.randn(r_rows or M, N, generator=g) * 2.0).to(torch.bfloat16)


# ---- the LN fold, rstd (x W'^T - mean colsum) + cvec


def stats64(x, eps=1e-6):
    """{mean, rstd} per row, [M, 2] fp32: the fp64 statistics of the (bf16) rows rounded to fp32 -- not ov_rowstats' output, so a test
    that hands these to ov_gemm_ln does not depend on that kernel."""
    xd = x.double()
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    return torch.stack([mean, (var + eps).rsqrt()], 1).float()


def spiked_fold_case(M, N, K):
    """CPU operands of the fold, (x bf16 [M, K], wg bf16 [N, K], cvec fp32, colsum fp32, w, bias, gamma, beta fp32: the unfolded
    Linear and LayerNorm), the construction of test_gemm_ln_fold_matches_layernorm_then_linear (x = 0.4 + 1.7 N(0, 1)) with three
    spikes: the last row at mean / std = 8 (the row whose statistics a clamped or neighbouring read gets wrong: mean colsum is eight
    times the spread there, so the cancellation is at its worst), row 0 with spread 8 (rstd far from its neighbours'), and +40 on
    the last channel (an outlier channel, as trained towers have: whatever drops the end of K or mis-sums colsum shows)."""
    rnd_ = lambda *s, seed: torch.randn(*s, generator=torch.Generator().manual_seed(seed + M + N + K))
    x = rnd_(M, K, seed=130) * 1.7 + 0.4
    x[M - 1] = rnd_(K, seed=135) * 1.7 + 8 * 1.7
    x[0] = rnd_(K, seed=136) * 8.0 + 0.4
    x[:, K - 1] += 40.0
    x = x.to(torch.bfloat16)
    w, bias = rnd_(N, K, seed=131) / K ** 0.5, rnd_(N, seed=132) * 0.1
    gamma, beta = rnd_(K, seed=133) * 0.1 + 1, rnd_(K, seed=134) * 0.1
    wg = (w * gamma[None, :]).to(torch.bfloat16)
    colsum = wg.float().sum(1)
    cvec = w.to(torch.bfloat16).float() @ beta + bias
    return x, wg, cvec, colsum, w, bias, gamma, beta


def fold_bound(x, wg, colsum, cvec, stats, epi=0, stat_err=None):
    """(ref, bound), fp64 [M, N], of ov_gemm_ln's output under epilogue epi (0 bias, 1 GELU erf, 2 GELU tanh).

    The reference is the kernel's stated formula in fp64 on exactly the operands it receives (x, W' bf16; colsum, cvec, {mean, rstd}
    fp32):  ref = rstd t + cvec,  t = x W'^T - mean colsum.   e = 2^-24, REL = 2^-8, S1 = |x| |W'|^T:
        A     = rstd e (K S1 + 2 |t| + |mean colsum|) + 2 e |ref|
        bound = REL (|ref| + A) + A
    The kernel forms acc = x W'^T in fp32 (any order: off by at most K e S1), t32 = fma(colsum, -mean, acc) (one rounding, e |t|, of
    a value whose product term is exact inside the fma) and v = fma(t32, rstd, cvec) (one rounding, e |ref|); acc's error and t32's
    rounding are multiplied by rstd.  A carries each of these twice over where it costs nothing (2 |t|, 2 e |ref|) and |mean colsum|
    once more for the cancellation's second-order terms, so that no absolute floor is needed.  The output is v rounded to bf16 once:
    REL (|ref| + A).  With a GELU: 1.13 (= max |gelu'|) times the pre-activation's error, + the output rounding + the form's own error
    E (as in linear_ratios):  1.13 A (1 + REL) + REL |gelu(ref)| + E.
    No tuned term.  What it tells apart: test_gemm_small_bound.py.

    stat_err = (b_mean, dr), fp64 [M]: the statistics came from a kernel and are within b_mean of `stats`' mean and dr of its rstd
    (row_stats_ref64; `stats` then holds the fp64 statistics unrounded).  The mean's error reaches the output through
    (rstd + dr) b_mean |colsum|, rstd's through dr |t|, and A's own terms grow by 1 + dr / rstd.  The reference becomes
    Linear(LayerNorm(x)) on the folded operands, xhat W'^T + cvec = ref + d with d = rstd mean (colsum - sum_k W'): what the fp32
    colsum the kernel is handed differs from the exact row sums by, an operand's error and so added to A in full."""
    K = x.shape[1]
    xd, wd = x.double(), wg.double()
    mean, rstd = stats[:, 0:1].double(), stats[:, 1:2].double()
    mc = mean * colsum.double()
    t = xd @ wd.T - mc
    ref = rstd * t + cvec.double()
    s1 = (x.float().abs() @ wg.float().abs().T).double()
    a = rstd * E32 * (K * s1 + 2 * t.abs() + mc.abs()) + 2 * E32 * ref.abs()
    if stat_err is not None:
        bm, dr = (v.double().view(-1, 1) for v in stat_err)
        cs, d = colsum.double().abs(), rstd * mean * (colsum.double() - wd.sum(1))
        a = a * (1 + dr / rstd) + (rstd + dr) * bm * cs + dr * t.abs() + d.abs()
        ref = ref + d
    if epi == 0:
        return ref, REL * (ref.abs() + a) + a
    act = gelu64(ref, epi == 2)
    e = E_TANH if epi == 2 else torch.clamp(6.6e-5 * ref.abs(), min=1.4e-4)
    return act, 1.13 * (a * (1 + REL)) + REL * act.abs() + e


def fold_ratios_bound(x, wg, colsum, cvec, stats, outs):
    """outs: name -> (bf16 [M, >= N], epi 0 | 1 | 2).  name -> (max err / fold_bound, row, column), in row chunks."""
    M, N = x.shape[0], wg.shape[0]
    res = {}
    for i in range(0, M, CHUNK):
        sl = slice(i, min(M, i + CHUNK))
        for name, (got, epi) in outs.items():
            ref, bound = fold_bound(x[sl], wg, colsum, cvec, stats[sl], epi)
            _merge(res, name, _worst((got[sl, :N].double() - ref).abs(), bound, i))
    return res


def patch_rows(out, B, g2):
    """The rows a launch with out_group = g2 writes, [B g2, cols], of out [B (g2 + 1), cols] (row b (g2 + 1), image b's class row,
    is not written) -- through a view, restating none of the kernel's index arithmetic."""
    return out.unflatten(0, (B, g2 + 1))[:, 1:].reshape(B * g2, out.shape[1])


def class_rows(out, B, g2):
    return out.unflatten(0, (B, g2 + 1))[:, 0]


LN_RTOL, LN_ATOL = 1.5e-2, 2e-2


def ln_linear_ratios(operands, outs):
    """The tuned rule of test_gemm_ln_fold_matches_layernorm_then_linear, kept beside fold_bound: operands = (x, wg, cvec, colsum, w,
    bias, gamma, beta) as fold_operands / spiked_fold_case build them; outs: name -> (bf16 [M, >= N], epi 0 | 1 | 2) of ov_gemm_ln.
    name -> (max err / (LN_ATOL + LN_RTOL |ref|), row, column) against Linear(LayerNorm(x)) (then GELU) in fp64, in row chunks."""
    x, _, _, _, w, bias, gamma, beta = operands
    M, N = x.shape[0], w.shape[0]
    wd = w.double()
    res = {}
    for i in range(0, M, CHUNK):
        sl = slice(i, min(M, i + CHUNK))
        xd = x[sl].double()
        mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
        lin = ((xd - mu) * (var + 1e-6).rsqrt() * gamma.double() + beta.double()) @ wd.T + bias.double()
        for name, (got, epi) in outs.items():
            ref = gelu64(lin, epi == 2) if epi else lin
            _merge(res, name, _worst((got[sl, :N].double() - ref).abs(), LN_ATOL + LN_RTOL * ref.abs(), i))
    return res


# ---- the row passes: LayerNorm, the row statistics (two-pass and one-pass) and the rows around the towers' heads
#
# Closed forms in fp64 on the operands the kernels receive, with per-element bounds from u = 2^-8, e = 2^-24 and
# gamma_n = n e / (1 - n e) alone: no tuned term, no absolute floor, nothing of a kernel's summation order (derivations: DESIGN.md §4,
# "The row passes against fp64"; what the bounds tell apart: test_ln_rows_bound.py).


def gam(n):
    return n * E32 / (1 - n * E32)


def eps32(eps):
    """eps as the kernels receive it: a C float."""
    return float(torch.tensor(eps, dtype=torch.float32))


def rstd_interval(var, b_var, eps):
    """[lo, hi] of an fp32 rsqrtf(var^ + eps) whose var^ is within b_var of var (and >= 0): the eps add rounds once, rsqrtf is
    within one ulp (2 e): (1 +- 3 e) covers both."""
    return (var + eps + b_var).rsqrt() * (1 - 3 * E32), ((var - b_var).clamp_min(0) + eps).rsqrt() * (1 + 3 * E32)


class RowRef:
    """What row_stats_ref64 returns, all fp64 [R]: mean, var (biased), rstd; b_mean; b_var2 / b_var1 and the rstd intervals rstd2 /
    rstd1 = (lo, hi) of the two-pass (ov_layernorm, ov_rowstats) and one-pass (ov_rowstats_finalize) forms."""


def row_stats_ref64(x, eps=1e-6):
    """mean: a D-term fp32 sum in any order (gamma_{D-1} mean|x|), 1 / D rounded, one product: gamma_D mean|x| + e |mean|.
    Two-pass variance: d = x - mean^ rounds once (twice in d^2), the square once, D - 1 additions, 1 / D and the product: D + 4
    roundings of mean((x - mean^)^2) = var + (mean^ - mean)^2 <= var + b_mean^2.
    One-pass variance Q / D - mean^2: Q / D as the mean (the squares of bf16 values are exact in fp32); mean^2 carries the mean's
    error twice, 2 |mean| b_mean + b_mean^2, its rounding and the subtraction's: 2 e mean^2 + e var.  The clamp at 0 only helps."""
    xd = x.double()
    g = gam(xd.shape[1])
    r = RowRef()
    r.mean, r.eps = xd.mean(1), eps32(eps)
    r.var = ((xd - r.mean[:, None]) ** 2).mean(1)
    r.rstd = (r.var + r.eps).rsqrt()
    r.b_mean = g * xd.abs().mean(1) + E32 * r.mean.abs()
    r.b_var2 = (g + 4 * E32) * (r.var + r.b_mean ** 2) + r.b_mean ** 2
    r.b_var1 = ((g + 2 * E32) * (xd * xd).mean(1) + 2 * r.mean.abs() * r.b_mean + r.b_mean ** 2 + 2 * E32 * r.mean ** 2
                + E32 * r.var)
    r.rstd2, r.rstd1 = rstd_interval(r.var, r.b_var2, r.eps), rstd_interval(r.var, r.b_var1, r.eps)
    return r


def _over(num, den):
    """num / den with 0 / 0 = 0 (an all-zero row: bound 0, error 0) and a NaN numerator kept (it fails every assertion)."""
    return torch.where((num == 0) & (den == 0), torch.zeros_like(num), num / den)


def stats_ratios(st, ref, onepass=False):
    """(mean, rstd, rstd against the two-pass interval) of {mean, rstd} [R, 2]: |mean^ - mean| / b_mean, and how far rstd^ stands
    from rstd as a fraction of the interval's side it lies on (<= 1: inside), each the maximum over the rows, with the row."""
    got = st.double()
    qm = _over((got[:, 0] - ref.mean).abs(), ref.b_mean)
    res = [qm]
    for lo, hi in (ref.rstd1 if onepass else ref.rstd2, ref.rstd2):
        d = got[:, 1] - ref.rstd
        res.append(torch.where(d >= 0, d / (hi - ref.rstd), -d / (ref.rstd - lo)))
    out = []
    for q in res:
        q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
        k = int(q.argmax())
        out.append((float(q[k]), k))
    return out


def ln_ref64(x, gamma, beta, eps=1e-6, out_bf16=True):
    """(y, bound) fp64 [R, D] of ov_layernorm, y = (x - mean) rstd gamma + beta.  With dr the rstd interval's wider side and hi its
    upper end:  d^ = x - mean^ is off by b_mean + e (|x - mean| + b_mean);  d^ rstd^ by
        E1 = |x - mean| dr + hi (b_mean + e (|x - mean| + b_mean));
    that product and the one with gamma round once each, gamma_2 (|x - mean| rstd + E1), and the sum with beta once:
        E2 = |gamma| (E1 + gamma_2 (|x - mean| rstd + E1)),   bound = E2 + e (|y| + E2)   [+ u (|y| + bound) for a bf16 output]."""
    st = row_stats_ref64(x, eps)
    g, b = gamma.double(), beta.double()
    xc = (x.double() - st.mean[:, None]).abs()
    rstd, bm = st.rstd[:, None], st.b_mean[:, None]
    y = (x.double() - st.mean[:, None]) * rstd * g + b
    lo, hi = st.rstd2
    dr = torch.maximum(hi - st.rstd, st.rstd - lo)[:, None]
    e1 = xc * dr + hi[:, None] * (bm + E32 * (xc + bm))
    e2 = g.abs() * (e1 + gam(2) * (xc * rstd + e1))
    bound = e2 + E32 * (y.abs() + e2)
    return y, bound + U16 * (y.abs() + bound) if out_bf16 else bound


def ratio(got, ref, bound):
    """(max |got - ref| / bound, flat index), 0 / 0 = 0, NaN = inf."""
    q = _over((got.double() - ref).abs(), bound)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q).reshape(-1)
    k = int(q.argmax())
    return float(q[k]), k


LADDER = (0.0, 1.0, 8.0, 64.0, 512.0)     # mean / std of the statistics' rows
CONST_ROW = 100.0                         # the constant row's value: Q / D and mean^2 are 1e4, their roundings far above eps


def spiked_rows_case(rows, D, seed, f32=False):
    """(x [rows, D] bf16 or fp32, gamma, beta fp32) for ov_layernorm / ov_rowstats: x = 0.4 + 1.7 N(0, 1); the last 8 columns -- the
    chunk of the last live lane of the last c -- carry +40; the last row (in the grid-stride tail where there is one) has
    mean / std = 8; row 0 has spread 8; row 1 (rows >= 3) is constant.  beta's last 8 entries sit 2 higher: the outputs there are
    large (the +40), and a beta of 0.1 would hide in their bf16 rounding."""
    g = torch.Generator().manual_seed(7919 * D + rows + seed)
    x = torch.randn(rows, D, generator=g) * 1.7 + 0.4
    if rows > 1:
        x[0] = torch.randn(D, generator=g) * 8.0 + 0.4
    x[rows - 1] = torch.randn(D, generator=g) * 1.7 + 8 * 1.7
    x[:, D - 8:] += 40.0
    if rows >= 3:
        x[1] = CONST_ROW
    gamma, beta = torch.randn(D, generator=g) * 0.1 + 1, torch.randn(D, generator=g) * 0.1
    beta[D - 8:] += 2.0
    return (x if f32 else x.to(torch.bfloat16)), gamma, beta


def ladder_rows_case(rows, D, seed=0):
    """x bf16 [rows, D] for the statistics: row i = 1.7 N(0, 1) + 1.7 LADDER[i mod 5], +40 on the last eight channels; the row before
    the last (rows >= 7) is constant, and the one before that nearly so: 1000 with the last two channels one bf16 step higher, 1004
    (var = 0.03 against mean^2 = 1e6: the one-pass difference is all rounding there, and this is the row on which the clamp at 0
    acts -- an exactly constant row is summed exactly by any tree).  ladder_of(rows) gives each row's rung (-1, -2: these two)."""
    g = torch.Generator().manual_seed(104729 * D + rows + seed)
    x = torch.randn(rows, D, generator=g) * 1.7 + 1.7 * torch.tensor(LADDER)[torch.arange(rows) % 5, None]
    x[:, D - 8:] += 40.0
    if rows >= 7:
        x[rows - 2] = CONST_ROW
        x[rows - 3] = 1000.0
        x[rows - 3, D - 2:] = 1004.0
    return x.to(torch.bfloat16)


def ladder_of(rows):
    r = torch.arange(rows) % 5
    if rows >= 7:
        r[rows - 2], r[rows - 3] = -1, -2
    return r


LN_EDGE_D = [8, 192, 512, 520, 1152, 2048, 2056, 4304, 8192]      # NCH 1, 1, 1 full, 2 (one lane), 3, 4 full, 8 (one lane), 16, 16 full
LN_EDGE_ROWS = (1, 3, 5)
LN_LAP_CASE = (65541, 64)                 # 16384 workgroups x 4 rows + 5: the second grid-stride lap
LN_ALL_DTYPES_D = (520, 1152)
FINALIZE_G = [1, 6, 8, 9, 36, 128, 256]
FINALIZE_ROWS = (1, 31, 32, 33)
POOL_L = (2, 4, 5, 257)
POOL_D = (8, 520, 1152)
L2_E = (1, 40, 64, 65, 768)
L2_LAP_CASE = (32771, 40)                 # 8192 workgroups x 4 rows + 3


def parts_ref64(x):
    """(S, Q fp64 [R, D / 32], their bounds): a 32-term fp32 sum in any order, gamma_31 sum|x| and gamma_31 sum x^2 (the squares of
    bf16 values are exact in fp32)."""
    c = x.double().unflatten(1, (x.shape[1] // 32, 32))
    return c.sum(-1), (c * c).sum(-1), gam(31) * c.abs().sum(-1), gam(31) * (c * c).sum(-1)


def fold_chain_ratios(x, wg, colsum, cvec, outs, onepass, eps=1e-6):
    """outs: name -> (bf16 [M, >= N], epi) of ov_gemm_ln run on a statistics kernel's {mean, rstd}.  name -> (max err / bound, row,
    column) against Linear(LayerNorm(x)) in fp64 on the folded operands, ref = xhat W'^T + cvec: fold_bound at the fp64 statistics
    with the statistics' own bounds carried through (its stat_err)."""
    res = {}
    for i in range(0, x.shape[0], CHUNK):
        sl = slice(i, min(x.shape[0], i + CHUNK))
        st = row_stats_ref64(x[sl], eps)
        lo, hi = st.rstd1 if onepass else st.rstd2
        err = (st.b_mean, torch.maximum(hi - st.rstd, st.rstd - lo))
        for name, (got, epi) in outs.items():
            ref, bound = fold_bound(x[sl], wg, colsum, cvec, torch.stack([st.mean, st.rstd], 1), epi, stat_err=err)
            _merge(res, name, _worst((got[sl, :wg.shape[0]].double() - ref).abs(), bound, i))
    return res


def pool_case(B, L, D, seed=0):
    """x bf16 [B L, D] = 0.4 + 1.7 N(0, 1), each sequence's row 0 (the class row) 40 higher."""
    g = torch.Generator().manual_seed(31 * L + D + B + seed)
    x = torch.randn(B, L, D, generator=g) * 1.7 + 0.4
    x[:, 0] += 40.0
    return x.reshape(B * L, D).to(torch.bfloat16)


def mean_pool_ref64(x, B, L, first):
    """(ref, bound) fp64 [B, D]: the mean over tokens first .. L - 1, n = L - first terms in any order, 1 / n rounded, one product:
    gamma_n mean_t|x| + e |ref|."""
    t = x.double().unflatten(0, (B, L))[:, first:]
    ref = t.mean(1)
    return ref, gam(L - first) * t.abs().mean(1) + E32 * ref.abs()


def l2norm_case(rows, E, f32, seed=0):
    """x [rows, E] ~ N(0, 1), the last element of every row 8 times larger (in the lanes' tail when E % 64 != 0); with rows >= 3,
    row 1 is all zero and row 2 holds 1e-20 N(0, 1) (norm far below the 1e-12 clamp)."""
    g = torch.Generator().manual_seed(53 * E + rows + seed)
    x = torch.randn(rows, E, generator=g)
    x[:, E - 1] *= 8.0
    if rows >= 3:
        x[1] = 0.0
        x[2] = torch.randn(E, generator=g) * 1e-20
    return x if f32 else x.to(torch.bfloat16)


def l2norm_ref64(x):
    """(ref, bound) fp64 of ov_l2norm, y = x / max(|x|_2, 1e-12).  ss = sum x^2: products and E - 1 additions, gamma_E; sqrt halves it
    and rounds, the reciprocal and the product round: |y| (gamma_E / 2 + 4 e) (the second-order 3/8 gamma_E^2 sits inside the fourth
    e up to E = 6700).  Under the clamp y = x / fl32(1e-12): the division and the product round, 4 e |y| again; an all-zero row
    is 0 exactly (bound 0)."""
    xd = x.double()
    nrm = xd.pow(2).sum(1, keepdim=True).sqrt()
    clamp = float(torch.tensor(1e-12, dtype=torch.float32))
    ref = xd / nrm.clamp_min(clamp)
    return ref, ref.abs() * torch.where(nrm < clamp, torch.full_like(nrm, 4 * E32), torch.full_like(nrm, gam(x.shape[1]) / 2 + 4 * E32))


def cls_rows_ref(cls, pos0):
    return (cls.to(torch.bfloat16).float() + pos0.to(torch.bfloat16).float()).to(torch.bfloat16)


def mean_pool(x, B, L, first, out=None):
    """ov_mean_pool on x [B L, D] (any row pitch); out: a caller-owned contiguous fp32 [B, D]."""
    lib = _lib.load()
    D = x.shape[1]
    if out is None:
        out = torch.empty(B, D, dtype=torch.float32, device=x.device)
    check(lib.ov_mean_pool(ptr(x), x.stride(0), ptr(out), B, L, D, first, stream_ptr()), "ov_mean_pool")
    return out


def l2norm(x, out=None):
    """ov_l2norm on x [rows, E] bf16 or fp32 (any row pitch); out: a caller-owned fp32 [rows, >= E] view with its own pitch."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib.ov_l2norm(ptr(x), _flag(x), x.stride(0), ptr(out), out.stride(0), x.shape[0], x.shape[1], stream_ptr()), "ov_l2norm")
    return out


def gather_rows(x, B, L, t, out=None):
    lib = _lib.load()
    D = x.shape[1]
    if out is None:
        out = torch.empty(B, D, dtype=torch.bfloat16, device=x.device)
    check(lib.ov_gather_rows(ptr(x), x.stride(0), ptr(out), out.stride(0), B, L, t, D, stream_ptr()), "ov_gather_rows")
    return out


def cls_rows(x, cls, pos0, B, L):
    """ov_cls_rows in place on x [B L, >= D] bf16 (D = cls.numel())."""
    lib = _lib.load()
    check(lib.ov_cls_rows(ptr(x), x.stride(0), ptr(cls), ptr(pos0), B, L, cls.numel(), stream_ptr()), "ov_cls_rows")
    return x


# ---- the optimiser and the embedding / patch-dropout glue, bit for bit (test_gpu_optim_glue_edges.py on the device,
# test_optim_glue_cpu.py restated without one; tables and derivations: DESIGN.md §4, "The update and the glue, bit for bit").
# Every comparand is independent of the kernels' code: oracle/optim_ref.py for the update, integer sums and an fp64 sum for
# ov_sumsq, torch on the CPU (F.unfold, indexing, .to(bfloat16)) for the glue.  Inputs and comparands are CPU tensors.

LAP = 8192 * 256                          # work items of one grid-stride lap: grids are capped at 8192 workgroups of 256
ADAM_LAP_N = LAP * 4 + 1024 + 3           # four elements per work item: a second lap of 256 work items, then the n & 3 tail
SUMSQ_THREADS, SUMSQ_VEC, SUMSQ_PARTS = 256, 4, 1024      # optim.hip: 256 threads x one float4 per load, at most 1024 partial sums
SUMSQ_CAP = SUMSQ_VEC * SUMSQ_THREADS * SUMSQ_PARTS       # 1 048 576 elements: the largest n of a single lap
GUARD = 16                                # elements behind every optimiser state buffer, which must keep GUARD_VALUE
GUARD_VALUE = 77.0
INT_MAX = 2 ** 31 - 1


def bits(t):
    """A tensor's storage as integers of its element size."""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b, nan_ok=False):
    """Bit equality of two tensors of one shape and dtype; nan_ok: NaN matches NaN whatever its payload."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if nan_ok:
        na, nb = torch.isnan(a), torch.isnan(b)
        return bool(torch.equal(na, nb)) and bool(torch.equal(bits(a)[~na], bits(b)[~na]))
    return bool(torch.equal(bits(a), bits(b)))


def same_outputs(got, ref, nan_ok=False):
    """{name: tensor} against {name: tensor}: the names whose bits differ (empty: all equal)."""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return sorted(k for k in ref if not same_bits(got[k], ref[k], nan_ok))


def f32c(v):
    """v as a C float argument arrives: rounded to fp32, returned as a Python double."""
    return float(np.float32(v))


def np_bf16(x):
    """fp32 numpy -> the nearest-even bfloat16 values, as fp32 (torch's rounding, not the oracle's helper)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


# ---- ov_adamw_step

def _ac(n, steps=1, t0=1, b1=0.9, b2=0.95, wd=0.2, lr=1e-3, eps=1e-8, gs=1.0, clip="none", ties=False, mu_off=0, tiny=False, seed=0):
    return SimpleNamespace(n=n, steps=steps, t0=t0, b1=b1, b2=b2, wd=wd, lr=lr, eps=eps, gs=gs, clip=clip, ties=ties, mu_off=mu_off,
                           tiny=tiny, seed=seed)


CLIP_NORM = 0.25
GN_SQ = {"above": 7.3, "below": 1e-4, "zero": 0.0}        # sqrt(7.3) / 3 = 0.90 > 0.25 at the smallest grad_scale; sqrt(1e-4) = 0.01 < 0.25
ADAM_CASES = [_ac(1), _ac(2, wd=0.0), _ac(3), _ac(3, b1=0.5, b2=0.5, ties=True), _ac(4), _ac(5), _ac(7, gs=0.5),
              _ac(1023, t0=2, b2=0.999, wd=0.0, gs=0.5, clip="above"),
              _ac(2051, steps=3, gs=1 / 3, clip="above"),                       # three steps at a mid size
              _ac(2051, t0=1000, b2=0.999, eps=0.0),
              _ac(2051, t0=100000),                                             # both bias corrections are exactly 1
              _ac(2051, b1=0.5, b2=0.5, ties=True),
              _ac(2051, b1=0.5, b2=0.5, ties=True, gs=0.5, wd=0.0, t0=2),
              _ac(2051, b1=0.0, b2=0.0, t0=2),
              _ac(2051, lr=0.0),
              _ac(2051, clip="below", gs=0.5),
              _ac(2051, clip="zero"),
              _ac(1027, mu_off=4, clip="above"),                                # mu 8 bytes past a 16-byte boundary
              _ac(37, tiny=True),                                               # g^2 and (1 - b2) g^2 subnormal
              _ac(ADAM_LAP_N, clip="above")]                                    # second grid-stride lap + tail, one step
ADAM_MIN_N = 1023                         # below it a case holds too few elements for a value-only mistake to be sure to show
ADAM_CHAIN = (2051, 1023)                 # the two groups of the chained ov_sumsq -> ov_adamw_step case


def adam_id(c):
    return (f"n{c.n}-t{c.t0}x{c.steps}-b{c.b1}-{c.b2}-wd{c.wd}-lr{c.lr}-eps{c.eps}-gs{c.gs:.3f}-{c.clip}" +
            ("-ties" * c.ties) + ("-mu8" * bool(c.mu_off)) + ("-tiny" * c.tiny))


def adam_inputs(c):
    """p, mu (bf16 values held in fp32), nu and one g per step, numpy fp32: p of both signs, a third of it down to 1e-7 so that
    the last bit of the update shows in it; mu nonzero; g with exact zeros, +-1e4
    and +-1e-20; nu >= 0, exactly 0 where the first g is 0 (eps > 0 only: with eps = 0 the quotient needs nu > 0).  ties: the
    first min(n, 256) elements hold mu = 0 and g = +-2 (1 + (2k + 1) 2^-8) 2^e, k = 0 .. 127, e = 0 and -3: under b1 = 0.5 and a
    power-of-two gradient factor the fp32 moment is an exact bf16 tie, the kept bit of both parities.  tiny: |g| = j 1e-21, so
    that g^2 and (1 - b2) g^2 are subnormal, over nu = 0 and a subnormal nu."""
    r = np.random.default_rng(1000 + c.seed + c.n % 9973)
    n, idx = c.n, np.arange(c.n)
    sign = np.where(idx & 1, -1.0, 1.0).astype(np.float32)
    p = r.standard_normal(n)
    p = np.where(idx % 3 == 0, p * 10.0 ** (-7 * r.random(n)), p).astype(np.float32)      # a third of it small against lr u: the update's last bits show
    mu = np_bf16(r.standard_normal(n) * 0.05)
    mu[mu == 0] = 2.0 ** -7
    nu = ((r.standard_normal(n) * 0.1) ** 2).astype(np.float32) + np.float32(1e-12)
    gs = []
    for _ in range(c.steps):
        g = (r.standard_normal(n) * 0.1).astype(np.float32)
        g[idx % 11 == 3] = 0.0
        g[idx % 53 == 7] = (1e4 * sign)[idx % 53 == 7]
        g[idx % 59 == 9] = (1e-20 * sign)[idx % 59 == 9]
        if c.tiny:
            g = (sign * (idx + 1) * 1e-21).astype(np.float32)
        if c.ties:
            k = np.arange(256)
            t = (2.0 * (1 + (2 * (k % 128) + 1) * 2.0 ** -8) * np.where(k < 128, 1.0, 2.0 ** -3)).astype(np.float32)
            m = min(n, 256)
            g[:m] = (t * np.where(k % 3 == 0, -1, 1))[:m]
        gs.append(g)
    if c.eps > 0:
        nu[gs[0] == 0] = 0.0
    if c.tiny:
        nu = np.where(idx & 2, 0.0, 1e-41).astype(np.float32)
    if c.ties:
        mu[:256] = 0.0
    return SimpleNamespace(p=p, mu=mu, nu=nu, g=gs)


def adam_gnorm_sq(c):
    """The device scalar the test writes for the clip (fp32), or None without clipping."""
    return None if c.clip == "none" else np.float32(GN_SQ[c.clip])


def adam_ref(c, x, gn_sq="case"):
    """oracle.optim_ref.adamw_step over the case's steps, given what the kernel is given: the betas as the C ABI carries them
    (fp32), and the global norm as sqrt(fp32 gnorm_sq) * fp32 grad_scale.  -> {p, mu, nu} as torch tensors (mu bfloat16)."""
    from oracle import optim_ref as O
    gn_sq = adam_gnorm_sq(c) if isinstance(gn_sq, str) else gn_sq
    p, mu, nu = x.p, x.mu, x.nu
    for i, g in enumerate(x.g):
        clip = {} if gn_sq is None else dict(clip_norm=CLIP_NORM, gnorm=np.sqrt(np.float32(gn_sq)) * np.float32(c.gs))
        p, mu, nu = O.adamw_step(p, g, mu, nu, c.t0 + i, c.lr, f32c(c.b1), f32c(c.b2), c.eps, c.wd, c.gs, **clip)
    return adam_out(p, mu, nu)


def adam_out(p, mu, nu):
    assert p.dtype == np.float32 and mu.dtype == np.float32 and nu.dtype == np.float32
    mu_t = torch.from_numpy(np.ascontiguousarray(mu))
    assert bool(torch.equal(mu_t.to(torch.bfloat16).float(), mu_t) | bool(torch.isnan(mu_t).any())), "mu does not hold bf16 values"
    return dict(p=torch.from_numpy(np.ascontiguousarray(p)), mu=mu_t.to(torch.bfloat16), nu=torch.from_numpy(np.ascontiguousarray(nu)))


class AdamState:
    """p, nu (fp32) and mu (bf16) on the device, each with GUARD elements behind its n that must keep GUARD_VALUE; mu starts
    mu_off elements (2 bytes each) past a 256-byte boundary."""

    def __init__(self, x, mu_off=0):
        self.n = n = x.p.size
        def buf(a, dtype, off=0):
            b = torch.full((off + n + GUARD,), GUARD_VALUE, dtype=dtype, device=DEV)
            b[off:off + n] = torch.from_numpy(a).to(dtype)
            return b[off:]
        self.p, self.nu, self.mu = buf(x.p, torch.float32), buf(x.nu, torch.float32), buf(x.mu, torch.bfloat16, mu_off)
        assert self.p.data_ptr() % 16 == 0 and self.mu.data_ptr() % 16 == (2 * mu_off) % 16

    def step(self, g, c, t, gn_sq=None):
        """One ov_adamw_step; g: numpy fp32; gn_sq: None, or a device fp32 scalar handed over by pointer."""
        gd = torch.from_numpy(g).to(DEV)
        adamw_step(self.p, gd, self.mu, self.nu, self.n, c.lr, c.b1, c.b2, c.eps, c.wd, t, c.gs, gn_sq, CLIP_NORM if gn_sq is not None else 0.0)
        assert same_bits(gd, torch.from_numpy(g)), "g was written"

    def read(self):
        n = self.n
        for name in ("p", "nu", "mu"):
            assert bool((getattr(self, name)[n:] == GUARD_VALUE).all()), f"{name}: written past n"
        return dict(p=self.p[:n].cpu(), mu=self.mu[:n].cpu(), nu=self.nu[:n].cpu())


def adamw_step(p, g, mu, nu, n, lr, b1, b2, eps, wd, step, grad_scale, gnorm_sq=None, clip_norm=0.0):
    """ov_adamw_step in place on the caller's flat device buffers (views with guard elements behind n allowed)."""
    lib = _lib.load()
    check(lib.ov_adamw_step(ptr(p), ptr(g), ptr(mu), ptr(nu), n, lr, b1, b2, eps, wd, step, grad_scale, ptr(gnorm_sq), clip_norm,
                            stream_ptr()), "ov_adamw_step")


def sumsq(g, out, accumulate=0):
    """ov_sumsq into the caller's device scalar `out`; the workspace is exactly ov_sumsq_workspace_bytes() long, and the GUARD
    floats behind it must stay as they were."""
    lib = _lib.load()
    nb = lib.ov_sumsq_workspace_bytes()
    ws = torch.full((nb // 4 + GUARD,), GUARD_VALUE, dtype=torch.float32, device=g.device)
    check(lib.ov_sumsq(ptr(g), g.numel(), ptr(out), accumulate, ptr(ws), nb, stream_ptr()), "ov_sumsq")
    assert bool((ws[nb // 4:] == GUARD_VALUE).all()), "ov_sumsq wrote past its workspace"
    return out


# ---- ov_sumsq

SUMSQ_INT_N = [1, 2, 3, 4, 5, 1027, SUMSQ_CAP - 1, SUMSQ_CAP, SUMSQ_CAP + 1, SUMSQ_CAP + 3, ADAM_LAP_N]
SUMSQ_PRIOR = 12345.0
SUMSQ_NORMAL_N = (1 << 20) + 3


def sumsq_blocks(n):
    return min(max((n // 4 + SUMSQ_THREADS - 1) // SUMSQ_THREADS, 1), SUMSQ_PARTS)


def sumsq_int_case(n):
    """g in {0, +-1} (half of it 0) with +-2 on the tail, the last float4, and the element at 4 x 256 x blocks (the first of the
    second lap) where that lies inside n; -> (g numpy fp32, the exact integer sum of squares, < 2^24)."""
    r = np.random.default_rng(n)
    g = r.choice(np.array([0, 0, 1, -1], dtype=np.float32), size=n)
    probes = list(range(n - (n & 3), n)) + list(range(max(n - (n & 3) - 4, 0), n - (n & 3)))
    probes += [q for q in (SUMSQ_VEC * SUMSQ_THREADS * sumsq_blocks(n), SUMSQ_CAP) if q < n]
    for j, q in enumerate(probes):
        g[q] = 2.0 if j & 1 else -2.0
    total = int((g.astype(np.int64) ** 2).sum())
    assert total + int(SUMSQ_PRIOR) < 2 ** 24
    return g, total


def sumsq_chain_length(n, accumulate):
    """The most fp32 roundings a square passes through on its way into ov_sumsq's result, from n and the header's constants alone
    (derivation: DESIGN.md): per lap four fused multiply-adds into the thread's sum, one more for a tail element, six adds of the
    wave's exchange tree and two across the four waves; then ceil(blocks / 256) adds of the finishing thread over the partial
    sums, the same six and two, and the add onto the prior value."""
    blocks = sumsq_blocks(n)
    laps = -(-(n // 4) // (blocks * SUMSQ_THREADS))
    return SUMSQ_VEC * laps + (1 if n & 3 else 0) + 6 + 2 + -(-blocks // SUMSQ_THREADS) + 6 + 2 + (1 if accumulate else 0)


# ---- the glue of embed.hip: inputs on the CPU, comparands from torch alone

IM2COL_GEOM = [(28, 14, 592), (28, 14, 640), (160, 16, 768), (16, 8, 192)]       # (S, P, Kpad); 3 P^2 = 588, 588, 768, 192
IM2COL_LAP = (21850, 16, 8, 192)                                                 # B x 4 patches x 24 chunks = 2 097 600 > LAP
KEEP_GEOM = [(28, 14, 592), (56, 14, 640), (160, 16, 768)]                       # G = 4, 16, 100
COL2IM_GEOM = [(28, 14), (56, 14), (160, 16)]
INVERSE_G = (4, 100, 16384)
ASSEMBLE_D = (8, 192, 1152)
ASSEMBLE_BWD_B = (1, 3, 5, 9)
TEXT_CASES = [(3, 1, 8, 40000), (2, 80, 8, 40000), (3, 80, 192, 1000), (2, 80, 1152, 300), (5, 1, 1152, 300)]     # (B, T, D, V)
TEXT_LAP = (1093, 80, 192, 1000)                                                 # 87 440 rows x 24 chunks = 2 098 560 > LAP
CONVERT_COLS = (1, 7, 193, 1024)
CONVERT_LAP = (2049, 1024)                                                       # 2 098 176 elements > LAP
DTYPE_PAIRS = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32),
               (torch.bfloat16, torch.bfloat16)]


def image_case(B, S, dtype, seed=0):
    """[B, 3, S, S]: Gaussian values over sixteen binades, so that (nearly) every pixel has its own value, in bf16 as far as its
    4096 values of that range allow, and any permutation of pixels shows; the fp32 values are no bf16 values."""
    g = torch.Generator().manual_seed(seed)
    n = B * 3 * S * S
    img = torch.randn(n, generator=g) * 2.0 ** torch.randint(-8, 8, (n,), generator=g)
    return img.view(B, 3, S, S).to(dtype)


def im2col_ref(img, P, Kpad):
    """F.unfold's (c, ii, jj) columns per patch, patches row-major, rounded to bf16 once, zeros up to Kpad."""
    B = img.shape[0]
    cols = torch.nn.functional.unfold(img.float(), P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P).to(torch.bfloat16)
    out = torch.zeros(cols.shape[0], Kpad, dtype=torch.bfloat16)
    out[:, :3 * P * P] = cols
    return out


def keep_table(B, G, K, seed=0):
    """[B, K] int32: per image the first K of a random order of its G patches."""
    g = torch.Generator().manual_seed(seed + 17 * G + K)
    return torch.stack([torch.randperm(G, generator=g)[:K] for _ in range(B)]).to(torch.int32)


def keep_ks(G):
    return sorted({1, G // 2, G})


def gather_keep(rows, keep, G):
    """rows [B G, C] -> [B K, C]: image b's rows keep[b, :] in that order."""
    B, K = keep.shape
    idx = (torch.arange(B)[:, None] * G + keep.long()).reshape(-1)
    return rows[idx]


def inverse_ref(keep, G):
    inv = [[-1] * G for _ in range(keep.shape[0])]
    for b, row in enumerate(keep.tolist()):
        for j, idx in enumerate(row):
            inv[b][idx] = j
    return torch.tensor(inv, dtype=torch.int32)


def assemble_case(B, G, K, D, seed=0):
    g = torch.Generator().manual_seed(seed + D)
    return SimpleNamespace(B=B, G=G, K=K, D=D, y=torch.randn(B * K, D, generator=g).to(torch.bfloat16),
                           cls=torch.randn(D, generator=g), pos=torch.randn(1 + G, D, generator=g), keep=keep_table(B, G, K, seed))


def assemble_ref(c):
    y = c.y.float().view(c.B, c.K, c.D)
    return torch.cat([(c.cls + c.pos[0]).expand(c.B, 1, c.D), y + c.pos[1 + c.keep.long()]], dim=1)


def assemble_bwd_case(B, G, K, D, seed=0):
    """dx [B, 1 + K, D] fp32 over six decades of magnitude, so that the order of an fp32 sum over b shows in its bits."""
    g = torch.Generator().manual_seed(seed + 31 * B + D)
    dx = torch.randn(B, 1 + K, D, generator=g) * 10.0 ** (torch.rand(B, 1 + K, D, generator=g) * 6 - 3)
    keep = keep_table(B, G, K, seed + B)
    return SimpleNamespace(B=B, G=G, K=K, D=D, dx=dx, keep=keep, inv=inverse_ref(keep, G))


def assemble_bwd_ref(c):
    """dpos: zeros, then image 0, 1, ..., B - 1 added in that order, each to row 0 and to the rows 1 + keep[b, :]."""
    dpos = torch.zeros(1 + c.G, c.D)
    for b in range(c.B):
        dpos[0] += c.dx[b, 0]
        dpos[1 + c.keep[b].long()] += c.dx[b, 1:]
    return dict(dpos=dpos, dcls=dpos[0].clone(), dy=c.dx[:, 1:].reshape(c.B * c.K, c.D).to(torch.bfloat16))


def col2im_case(B, S, P, K, seed=0):
    g = torch.Generator().manual_seed(seed + S + K)
    G = (S // P) ** 2
    keep = keep_table(B, G, K, seed)
    dcols = torch.randn(B * K, 3 * P * P, generator=g).to(torch.bfloat16)
    dcols[0, :5] = torch.tensor([-0.0, 0.0, 1e-40, -1e-40, 3e38]).to(torch.bfloat16)
    return SimpleNamespace(B=B, S=S, P=P, K=K, G=G, keep=keep, inv=inverse_ref(keep, G), dcols=dcols)


def col2im_ref(c, dtype):
    """A pure gather: the kept rows scattered into [B, G, 3 P^2] zeros, then the axes (gy, gx, c, ii, jj) -> (c, gy, ii, gx, jj)."""
    g = c.S // c.P
    full = torch.zeros(c.B * c.G, 3 * c.P * c.P, dtype=torch.bfloat16)
    full[(torch.arange(c.B)[:, None] * c.G + c.keep.long()).reshape(-1)] = c.dcols
    return full.view(c.B, g, g, 3, c.P, c.P).permute(0, 3, 1, 4, 2, 5).reshape(c.B, 3, c.S, c.S).to(dtype)


def text_case(B, T, D, V, seed=0, bad=False):
    """tokens int64 [B, T] with 0 and V - 1 among them; bad: -1, V and 2^40 + 5 as well (three rows that must clamp)."""
    g = torch.Generator().manual_seed(seed + V + D + T)
    tok = torch.randint(0, V, (B * T,), generator=g)
    tok[0], tok[-1] = V - 1, 0
    if bad:
        assert B * T >= 5
        tok[1], tok[2], tok[3] = -1, V, 2 ** 40 + 5
    return SimpleNamespace(B=B, T=T, D=D, V=V, tokens=tok.view(B, T), table=torch.randn(V, D, generator=g).to(torch.bfloat16),
                           pos=torch.randn(T, D, generator=g).to(torch.bfloat16), bad=bad)


def text_ref(c):
    ids = c.tokens.clamp(0, c.V - 1).reshape(-1)
    t = torch.arange(c.B * c.T) % c.T
    return dict(x=(c.table[ids].float() + c.pos[t].float()).to(torch.bfloat16),
                err=torch.tensor([int(bool(((c.tokens < 0) | (c.tokens >= c.V)).any()))], dtype=torch.int32))


def convert_values(dtype):
    """Every bf16 bit pattern (both zeros, the subnormals, both infinities, the NaNs); as fp32, each pattern exact, just below the
    tie to the next one, on the tie, and just above it (low half 0, 0x7fff, 0x8000, 0x8001): 65 536 or 262 144 values."""
    hi = torch.arange(65536, dtype=torch.int64)
    if dtype == torch.bfloat16:
        return hi.to(torch.int32).to(torch.int16).view(torch.bfloat16)
    words = torch.cat([(hi << 16) | low for low in (0, 0x7FFF, 0x8000, 0x8001)])
    return (words - ((words >> 31) << 32)).to(torch.int32).view(torch.float32)


def convert_case(rows, cols, dtype):
    """[rows, cols]: convert_values(dtype), repeated from its start to fill the shape."""
    v = convert_values(dtype)
    n = rows * cols
    return v.repeat(-(-n // v.numel()))[:n].view(rows, cols)


def convert_rows(cols, dtype):
    return -(-convert_values(dtype).numel() // cols)


# thin wrappers: caller-owned outputs, every pointer and pitch as the caller's tensors have them

def im2col_patches(img, P, out):
    lib = _lib.load()
    B, _, S, _ = img.shape
    check(lib.ov_im2col_patches(ptr(img), _flag(img), ptr(out), B, S, P, out.stride(0), stream_ptr()), "ov_im2col_patches")
    return out


def im2col_patches_keep(img, keep, P, out):
    lib = _lib.load()
    B, _, S, _ = img.shape
    check(lib.ov_im2col_patches_keep(ptr(img), _flag(img), ptr(keep), ptr(out), B, S, P, keep.shape[1], out.stride(0), stream_ptr()),
          "ov_im2col_patches_keep")
    return out


def patch_keep_inverse(keep, inv, G, err):
    """-> the status (OV_OK, or OV_ERR_UNSUPPORTED above the LDS limit), unchecked."""
    return _lib.load().ov_patch_keep_inverse(ptr(keep), ptr(inv), keep.shape[0], keep.shape[1], G, ptr(err), stream_ptr())


def patch_keep_assemble(y, cls, pos, keep, x, G):
    lib = _lib.load()
    B, K = keep.shape
    check(lib.ov_patch_keep_assemble(ptr(y), y.stride(0), ptr(cls), ptr(pos), ptr(keep), ptr(x), B, K, G, cls.numel(), stream_ptr()),
          "ov_patch_keep_assemble")
    return x


def patch_keep_assemble_backward(dx, inv, K, dpos=None, dcls=None, dy=None):
    lib = _lib.load()
    B, _, D = dx.shape
    check(lib.ov_patch_keep_assemble_backward(ptr(dx), ptr(inv), B, K, inv.shape[1], D, ptr(dpos), ptr(dcls), ptr(dy),
                                              dy.stride(0) if dy is not None else 0, stream_ptr()), "ov_patch_keep_assemble_backward")


def col2im_patches_keep(dcols, inv, dimg, P, K):
    lib = _lib.load()
    B, _, S, _ = dimg.shape
    check(lib.ov_col2im_patches_keep(ptr(dcols), dcols.stride(0), ptr(inv), ptr(dimg), _flag(dimg), B, S, P, K, stream_ptr()),
          "ov_col2im_patches_keep")
    return dimg


def text_embed(tokens, table, pos, x, err=None):
    lib = _lib.load()
    B, T = tokens.shape
    check(lib.ov_text_embed(ptr(tokens), ptr(table), ptr(pos), ptr(x), x.stride(0), B, T, table.shape[1], table.shape[0], ptr(err),
                            stream_ptr()), "ov_text_embed")
    return x


def convert(src, dst):
    lib = _lib.load()
    check(lib.ov_convert(ptr(src), _flag(src), src.stride(0), ptr(dst), _flag(dst), dst.stride(0), src.shape[0], src.shape[1],
                         stream_ptr()), "ov_convert")
    return dst


# ---- the training block chain, stage by stage (test_gpu_block_chain.py; what the stage checks tell apart: test_block_chain_cpu.py).
# forward_saving_layer (tower.hip) and block_backward_chain (backward.hip) are sequences of launches of operators that each have an
# fp64 reference and a derived bound above.  Every stage is held to its operator's bound ON THE STAGE'S OWN INPUTS AS THE RUN PRODUCED
# THEM, so no bf16 error compounds from one stage into the next one's tolerance.

BLOCK_NAMES = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b")
SLOT_FIELDS = ("x", "qkv", "o", "x1", "ln_1", "ln_2", "pre", "act")        # ov_tower_forward_saving's slot, in its order; then the lse


def block_case(D, heads, mlp, B, L, tanh, seed, mlp_pad=None, device=DEV):
    """Random block: returns (reference-named fp32 state dict of bf16-rounded weights, C-ABI weight dict on `device`, x, dy)."""
    names = {"ln1_w": ("ln_1.weight", (D,), 1.0, 0.1), "ln1_b": ("ln_1.bias", (D,), 0.0, 0.1),
             "qkv_w": ("attn.in_proj_weight", (3 * D, D), 0.0, D ** -0.5), "qkv_b": ("attn.in_proj_bias", (3 * D,), 0.0, 0.05),
             "out_w": ("attn.out_proj.weight", (D, D), 0.0, D ** -0.5), "out_b": ("attn.out_proj.bias", (D,), 0.0, 0.05),
             "ln2_w": ("ln_2.weight", (D,), 1.0, 0.1), "ln2_b": ("ln_2.bias", (D,), 0.0, 0.1),
             "fc_w": ("mlp.c_fc.weight", (mlp, D), 0.0, D ** -0.5), "fc_b": ("mlp.c_fc.bias", (mlp,), 0.0, 0.05),
             "proj_w": ("mlp.c_proj.weight", (D, mlp), 0.0, mlp ** -0.5), "proj_b": ("mlp.c_proj.bias", (D,), 0.0, 0.05)}
    bf = lambda t: t.to(torch.bfloat16)
    sd, dev = {}, {}
    for i, (k, (ref, shape, mean, std)) in enumerate(names.items()):
        t = rnd(*shape, seed=seed + i) * std + mean
        if len(shape) == 2:
            t = bf(t)
            dev[k] = t.to(device)
        else:
            dev[k] = t.to(device)
        sd["b." + ref] = t.float()
    if mlp_pad and mlp_pad > mlp:                 # device copies zero-padded to the kernels' hidden pitch (as the forward packs them)
        pad = mlp_pad - mlp
        dev["fc_w"] = torch.cat([dev["fc_w"], torch.zeros(pad, D, dtype=torch.bfloat16, device=device)]).contiguous()
        dev["fc_b"] = torch.cat([dev["fc_b"], torch.zeros(pad, device=device)]).contiguous()
        dev["proj_w"] = torch.cat([dev["proj_w"], torch.zeros(D, pad, dtype=torch.bfloat16, device=device)], dim=1).contiguous()
    x, dy = bf(rnd(B, L, D, seed=seed + 20)), bf(rnd(B, L, D, seed=seed + 21))
    return names, sd, dev, x, dy


def slot_layout(D, F, heads, B, L):
    """One layer's slot of `saved` as tower.hip lays it out: ({field: (byte offset, rows, columns)}, bytes per layer).  The eight bf16
    fields of SLOT_FIELDS, then "lse": fp32 [B * heads, L rounded up to 32], its section rounded up to 16 bytes."""
    M, lp = B * L, (L + 31) // 32 * 32
    lay, off = {}, 0
    for name, cols in zip(SLOT_FIELDS, (D, 3 * D, D, D, D, D, F, F)):
        lay[name] = (2 * off, M, cols)
        off += M * cols
    lay["lse"] = (2 * off, B * heads, lp)
    off += (2 * B * heads * lp + 7) // 8 * 8
    return lay, 2 * off


def saved_slots(saved, D, F, heads, B, L, layers=1):
    """Views of a uint8 `saved` buffer (ov_tower_forward_saving), one dict per layer: the fields of SLOT_FIELDS as bf16 [M, columns]
    and "lse" as fp32 [B * heads, L rounded up to 32] (written only where the library keeps it: attn_route(...).keep_lse)."""
    lay, nb = slot_layout(D, F, heads, B, L)
    out = []
    for i in range(layers):
        s = {}
        for name, (off, rows, cols) in lay.items():
            dt, es = (torch.float32, 4) if name == "lse" else (torch.bfloat16, 2)
            s[name] = saved[i * nb + off:i * nb + off + rows * cols * es].view(dt).view(rows, cols)
        out.append(s)
    return out


def block_saved_of(slot, keep_lse):
    """The full ov_block_saved over one slot (tower.hip's block_saved_of)."""
    return _lib.BlockSaved(qkv=slot["qkv"].data_ptr(), attn_out=slot["o"].data_ptr(), x1=slot["x1"].data_ptr(), fc_pre=slot["pre"].data_ptr(),
                           ln1_out=slot["ln_1"].data_ptr(), ln2_out=slot["ln_2"].data_ptr(), fc_act=slot["act"].data_ptr(),
                           attn_lse=slot["lse"].data_ptr() if keep_lse else None)


class Tower:
    """An ov_tower over a list of per-layer weight dicts (block_case's), as the training step drives it."""

    def __init__(self, cfg, layer_weights):
        self.lib, self.cfg, self.w = _lib.load(), cfg, layer_weights
        assert cfg.layers == len(layer_weights)
        self.h = self.lib.ov_tower_create(C.byref(cfg))
        assert self.h
        for i, w in enumerate(layer_weights):
            wst = _lib.BlockWeights(*[ptr(w[n]) for n in BLOCK_NAMES], None, None)
            check(self.lib.ov_tower_set_block(self.h, i, C.byref(wst)), "ov_tower_set_block")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.ov_tower_destroy(self.h)

    def forward_saving(self, x, B, L):
        """(y, saved uint8 with a 256-byte 0xA5 tail that must survive)."""
        nbs = self.lib.ov_tower_saved_bytes(self.h, B, L)
        saved = torch.full((nbs + 256,), 0xA5, dtype=torch.uint8, device=x.device)
        nb = self.lib.ov_tower_workspace_bytes(self.h, B, L)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=x.device)
        y = x.clone()
        check(self.lib.ov_tower_forward_saving(self.h, ptr(y), ptr(saved), B, L, ptr(ws), nb, stream_ptr()), "ov_tower_forward_saving")
        torch.cuda.synchronize()
        assert bool((saved[nbs:] == 0xA5).all()), "ov_tower_forward_saving wrote past ov_tower_saved_bytes"
        return y, saved

    def backward(self, saved, dy, B, L):
        """(dx, [grads dict per layer]) of ov_tower_backward."""
        grads = [{n: torch.full_like(w[n], float("nan")) for n in BLOCK_NAMES} for w in self.w]
        garr = (_lib.BlockGrads * len(grads))(*[_lib.BlockGrads(*[ptr(g[n]) for n in BLOCK_NAMES]) for g in grads])
        nb = self.lib.ov_tower_backward_workspace_bytes(self.h, B, L)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=dy.device)
        dx = dy.clone()
        check(self.lib.ov_tower_backward(self.h, ptr(saved), ptr(dx), garr, B, L, ptr(ws), nb, stream_ptr()), "ov_tower_backward")
        torch.cuda.synchronize()
        return dx, grads


def block_chain_replay(cfg, w, x, slot, dy, B, L, prefix=None):
    """block_backward_chain (backward.hip), launch by launch through the operators the C ABI exports, in the chain's order: c_proj dX
    with the GELU derivative, c_proj dW / db, c_fc dX / dW / db, LN_2 backward with dres = dy, out_proj dX / dW / db, attention backward
    (over the kept lse; under a prefix the masked one), QKV dX / dW / db, LN_1 backward with dres = dx1.

    slot: one layer's dict out of saved_slots (the chain with a full ov_block_saved: the derivative rides on the epilogue of dy Wproj^T,
    which the ABI exports as ov_gemm over the transposed weight -- what ov_linear_backward itself launches for a dX), or None: the
    recomputing entry, whose forward is replayed first (ov_layernorm, ov_gemm, ov_attention[_prefix], ov_gemm + residual, ov_layernorm,
    ov_gemm) and whose GELU derivative is the element-wise ov_gelu_backward over dh = dy Wproj^T, which also leaves gelu(pre) for the
    c_proj dW.  Operands sit in buffers 8 columns wider whose padding holds NaN; every output starts as SENT in a buffer 8 columns
    wider.  Returns a namespace: f (the forward tensors the stages read: SLOT_FIELDS and lse), dh_lin (None on the fused route), dh,
    act (what the c_proj dW read), dn2, dx1, do, dqkv, dn1, dx, grads (the twelve, BLOCK_NAMES) and wides [(buffer, columns used)]."""
    import prefix_restate as PR
    D, Hh, F, tanh, eps = cfg.width, cfg.heads, cfg.mlp_pad, bool(cfg.gelu_tanh), cfg.ln_eps
    M, hd = B * L, cfg.width // cfg.heads
    r = SimpleNamespace(wides=[], grads={})

    def outb(rows, cols):
        wide = torch.full((rows, cols + 8), SENT, dtype=torch.bfloat16, device=x.device)
        r.wides.append((wide, cols))
        return wide[:, :cols]

    xp, dyp = pitched(x), pitched(dy)
    if slot is None:
        n1 = layernorm(xp, w["ln1_w"], w["ln1_b"], eps, out=outb(M, D))
        qkv = gemm(n1, w["qkv_w"], w["qkv_b"], 0, out=outb(M, 3 * D))
        o = attention(qkv, B, L, Hh, hd, out=outb(M, D)) if prefix is None else PR.attention_prefix(qkv, B, L, Hh, hd, prefix, out=outb(M, D))
        x1 = gemm(o, w["out_w"], w["out_b"], 3, resid=xp, out=outb(M, D))
        n2 = layernorm(x1, w["ln2_w"], w["ln2_b"], eps, out=outb(M, D))
        pre = gemm(n2, w["fc_w"], w["fc_b"], 0, out=outb(M, F))
        f = {"x": xp, "qkv": qkv, "o": o, "x1": x1, "ln_1": n1, "ln_2": n2, "pre": pre, "act": None, "lse": None}
    else:
        f = {k: pitched(slot[k]) for k in SLOT_FIELDS}
        f["x"] = xp
        f["lse"] = slot["lse"] if prefix is None and attn_route(B, L, Hh, hd).keep_lse else None
    r.f = f
    g = r.grads
    if f["act"] is not None:
        wt = transpose(w["proj_w"])                                    # [F, D]: the staging ov_linear_backward makes for a dX
        r.dh_lin, r.act = None, f["act"]
        r.dh = gemm(dyp, wt, None, 5 if tanh else 4, resid=f["pre"], out=outb(M, F))
    else:
        r.dh_lin = linear_backward(dyp, None, w["proj_w"], want=("dx",), dx=outb(M, F))[0]
        r.dh, r.act = gelu_backward(f["pre"], r.dh_lin, tanh, da=outb(M, F), h=outb(M, F))
    _, g["proj_w"], g["proj_b"] = linear_backward(dyp, r.act, w["proj_w"], want=("dw", "db"), dw=outb(D, F))
    r.dn2, g["fc_w"], g["fc_b"] = linear_backward(r.dh, f["ln_2"], w["fc_w"], dx=outb(M, D), dw=outb(F, D))
    r.dx1, g["ln2_w"], g["ln2_b"] = layernorm_backward(f["x1"], w["ln2_w"], r.dn2, eps, dres=dyp, dx=outb(M, D))
    r.do, g["out_w"], g["out_b"] = linear_backward(r.dx1, f["o"], w["out_w"], dx=outb(M, D), dw=outb(D, D))
    if prefix is None:
        r.dqkv = attention_backward_saved(f["qkv"], f["o"], r.do, f["lse"], B, L, Hh, hd, dqkv=outb(M, 3 * D))
    else:
        r.dqkv = PR.attention_prefix_backward(f["qkv"], f["o"], r.do, B, L, Hh, hd, prefix, dqkv=outb(M, 3 * D))
    r.dn1, g["qkv_w"], g["qkv_b"] = linear_backward(r.dqkv, f["ln_1"], w["qkv_w"], dx=outb(M, D), dw=outb(3 * D, D))
    r.dx, g["ln1_w"], g["ln1_b"] = layernorm_backward(f["x"], w["ln1_w"], r.dn1, eps, dres=r.dx1, dx=outb(M, D))
    return r


def _cpu(t):
    return None if t is None else t.detach().cpu()


def lse_ref64(qkv, B, L, Hh, hd, mask=None):
    """(lse, bound) fp64 [B * Hh, L] of the kept row log-sum-exp in log2 units, lse = log2 sum_j 2^(s_j), s = scale log2(e) Q K^T.
    s_j is an hd-term fp32 dot product times a rounded constant: off by at most (hd + 3) e scale log2(e) (|Q| . |K_j|); d lse / d s_j
    = P_j.  exp2 (one ulp each), the L-term fp32 sum and log2 move the sum by at most (L + 8) e relatively, log2(e) times that in
    lse; the max is added back with one rounding and the result stored: 2 e |lse|."""
    q, k, _ = _split(qkv, B, L, Hh, hd)
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1) * LOG2E
    p = torch.softmax(s, dim=-1)
    ds = (hd + 3) * E32 * hd ** -0.5 * LOG2E * (p * (q.abs() @ k.abs().transpose(-1, -2))).sum(-1)
    bound = ds + (L + 8) * E32 * LOG2E + 2 * E32 * lse.abs()
    return lse.reshape(B * Hh, L), bound.reshape(B * Hh, L)


def chain_forward_ratios(w, f, y, dims, prefix=None):
    """Every forward stage of one block against fp64 of that stage applied to the stage's own stored input.  w: the block's weights
    (BLOCK_NAMES); f: the slot's tensors (SLOT_FIELDS; "act" and "lse" may be None), y: the block output or None; dims = (D, heads,
    mlp, mlp_pad, tanh, B, L).  Tensors on any device: the references run in fp64 on the CPU.  Returns stage -> max err / bound;
    "mlp padding" is 0 when columns [mlp, mlp_pad) of pre and act hold exactly zero and inf otherwise."""
    import prefix_restate as PR
    D, Hh, mlp, F, tanh, B, L = dims
    hd = D // Hh
    w = {k: _cpu(v) for k, v in w.items()}
    f = {k: _cpu(v) for k, v in f.items()}
    mask = None if prefix is None else PR.rule_mask(L, prefix)
    res = {}
    res["ln_1"] = ratio(f["ln_1"], *ln_ref64(f["x"], w["ln1_w"], w["ln1_b"]))[0]
    res["qkv"] = linear_ratios(f["ln_1"], w["qkv_w"], w["qkv_b"], {"qkv": (f["qkv"], "pre")})["qkv"][0]
    ref, pv = attn_ref64(f["qkv"], B, L, Hh, hd) if mask is None else PR.masked_attn_ref64(f["qkv"], B, L, Hh, hd, mask)
    res["attn"] = err_ratio(f["o"], ref, pv)
    if f.get("lse") is not None:
        want, bd = lse_ref64(f["qkv"], B, L, Hh, hd, mask)
        res["lse"] = ratio(f["lse"][:, :L], want, bd)[0]
    res["x1"] = linear_ratios(f["o"], w["out_w"], w["out_b"], {"x1": (f["x1"], "res")}, r=f["x"])["x1"][0]
    res["ln_2"] = ratio(f["ln_2"], *ln_ref64(f["x1"], w["ln2_w"], w["ln2_b"]))[0]
    outs = {"pre": (f["pre"], "pre")}
    if f.get("act") is not None:
        outs["act"] = (f["act"], "tanh" if tanh else "erf")
    for k, v in linear_ratios(f["ln_2"], w["fc_w"], w["fc_b"], outs).items():
        res[k] = v[0]
    pads = [f[k][:, mlp:F] for k in ("pre", "act") if f.get(k) is not None]
    res["mlp padding"] = 0.0 if all(bool((t.float() == 0).all()) for t in pads) else float("inf")
    if y is not None:
        res["y"] = linear_ratios(f["act"], w["proj_w"], w["proj_b"], {"y": (_cpu(y), "res")}, r=f["x1"])["y"][0]
    return res


def _q(got, ref, bd):
    """|got - ref| / bound per element, 0 / 0 = 0, NaN = inf."""
    q = _over((got.double() - ref).abs(), bd)
    return torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)


def chain_backward_ratios(w, r, dy, dims, prefix=None):
    """Every stage of the backward chain against fp64 of that stage on the stage's own inputs.  r: what block_chain_replay returns (or
    an emulation of it); dy: the chain's input.  Returns (stage -> max err / bound, {"dx1" | "dqkv" | "dx": err / bound per element}).
    The stages: dh (fused: linear_ratios' gerf / gtanh on dy Wproj^T at pre; else dh_lin under the dX bound, then dh and act under
    gelu_bounds), the four linear backwards (dX, dW, db under linear_bounds), the two LayerNorm backwards (ln_grads_ref64), the
    attention backward (bwd_bound with eo = the forward's own enforced bound on the kept out).  "grad padding": 0 when rows [mlp,
    mlp_pad) of fc_w / fc_b and columns [mlp, mlp_pad) of proj_w hold exactly zero, inf otherwise."""
    import prefix_restate as PR
    D, Hh, mlp, F, tanh, B, L = dims
    hd = D // Hh
    w = {k: _cpu(v) for k, v in w.items()}
    f = {k: _cpu(v) for k, v in r.f.items()}
    g = {k: _cpu(v) for k, v in r.grads.items()}
    dy, dh, dn2, dx1, do, dqkv, dn1, dx = (_cpu(t) for t in (dy, r.dh, r.dn2, r.dx1, r.do, r.dqkv, r.dn1, r.dx))
    res, elem = {}, {}

    def lin(tag, dyy, xx, ww, dX, dW, db):
        ref, bd = linear_grads_ref64(dyy, xx, ww), linear_bounds(dyy, xx, ww)
        if dX is not None:
            res[tag + " dX"] = float(_q(dX, ref[0], bd[0]).max())
        res[tag + " dW"] = float(_q(dW, ref[1], bd[1]).max())
        res[tag + " db"] = float(_q(db, ref[2], bd[2]).max())

    def ln(tag, xx, gamma, dyy, dres, got, dgamma, dbeta):
        ref = ln_grads_ref64(xx, gamma, dyy, dres, 1e-6)
        q = _q(got, ref.dx, ref.bdx)
        res[tag + " dx"], res[tag + " dgamma"], res[tag + " dbeta"] = float(q.max()), float(_q(dgamma, ref.dgamma, ref.bdg).max()), \
            float(_q(dbeta, ref.dbeta, ref.bdb).max())
        return q

    if r.dh_lin is None:
        wt = w["proj_w"].T.contiguous()
        res["dh"] = linear_ratios(dy, wt, torch.zeros(F), {"dh": (dh, "gtanh" if tanh else "gerf")}, r=f["pre"])["dh"][0]
    else:
        dh_lin = _cpu(r.dh_lin)
        ref, bd = linear_grads_ref64(dy, torch.zeros(dy.shape[0], F), w["proj_w"]), linear_bounds(dy, torch.zeros(dy.shape[0], F), w["proj_w"])
        res["dh_lin"] = float(_q(dh_lin, ref[0], bd[0]).max())
        res["dh"], res["act"] = gelu_err_ratio(dh, _cpu(r.act), f["pre"], dh_lin, tanh)
    lin("c_proj", dy, _cpu(r.act), w["proj_w"], None, g["proj_w"], g["proj_b"])
    lin("c_fc", dh, f["ln_2"], w["fc_w"], dn2, g["fc_w"], g["fc_b"])
    elem["dx1"] = ln("ln_2", f["x1"], w["ln2_w"], dn2, dy, dx1, g["ln2_w"], g["ln2_b"])
    lin("out_proj", dx1, f["o"], w["out_w"], do, g["out_w"], g["out_b"])
    mask = None if prefix is None else PR.rule_mask(L, prefix)
    ref = attn_grads_ref64(f["qkv"], do, B, L, Hh, hd, mask)
    bds = bwd_bound(ref, ref.q, ref.k, ref.v, ref.do, ref.scale, bound(ref.o, ref.pv))
    qs = [_q(dqkv[:, j * D:(j + 1) * D], want, bd) for j, (want, bd) in enumerate(zip((ref.dq, ref.dk, ref.dv), bds))]
    res["attn dq"], res["attn dk"], res["attn dv"] = (float(q.max()) for q in qs)
    elem["dqkv"] = torch.cat(qs, dim=1)
    lin("qkv", dqkv, f["ln_1"], w["qkv_w"], dn1, g["qkv_w"], g["qkv_b"])
    elem["dx"] = ln("ln_1", f["x"], w["ln1_w"], dn1, dx1, dx, g["ln1_w"], g["ln1_b"])
    pads = (g["fc_w"][mlp:], g["fc_b"][mlp:], g["proj_w"][:, mlp:])
    res["grad padding"] = 0.0 if all(bool((t.float() == 0).all()) for t in pads) else float("inf")
    return res, elem


def chain_dy(kind, B, L, D, tanh, seed):
    """The two upstream gradients of the chain tests, bf16 [B * L, D].  "dense": Gaussian with rows 0, 63, 64 and M - 1 eight times
    larger (spiked_linear_case's rows) and rows 0 and M - 1 four times larger again (32 x in all: spiked_ln_case's).  "pooled": what a
    pooling head sends down -- non-zero on token 0 of each sequence only (class pooling), or, for the tanh (text-like) block, the
    constant 1 / L on tokens 1... and zero on token 0 (the mean pool)."""
    M = B * L
    if kind == "dense":
        dy = rnd(M, D, seed=seed)
        for row in sorted({0, 63, 64, M - 1}):
            if row < M:
                dy[row] *= 8.0
        dy[0] *= 4.0
        dy[M - 1] *= 4.0
        return dy.to(torch.bfloat16)
    dy = torch.zeros(B, L, D)
    if tanh:
        dy[:, 1:] = 1.0 / L
    else:
        dy[:, 0] = rnd(B, D, seed=seed)
    return dy.view(M, D).to(torch.bfloat16)
