"""Attentional pooling (attn_pool.hip): an fp64 closed form of the cross-attention forward and backward with per-element bounds, the
spiked inputs of the edge tests, and thin wrappers of the two entry points.  The bounds have the derivation of hipops.bound and
hipops.bwd_bound (the constants come from there); what they can tell apart is pinned on the CPU by test_attn_pool_bound.py.

Layouts are the kernels': q [n_q, Hh hd] (no batch), kv [B L, 2 Hh hd] = (k | v), out / dout [B n_q, Hh hd], dq [n_q, Hh hd] fp32 = the
sum over the B images, dkv [B L, 2 Hh hd] = (dk | dv)."""
import torch

from hipops import LOG2E, REL, U_BWD, rnd

LSE_ATOL = 1e-4


# ---- fp64 closed form ----------------------------------------------------------------------------------------------------------------
def _q_heads(q, Hh, hd):
    """[n_q, >= Hh hd] -> [Hh, n_q, hd] fp64."""
    return q[:, :Hh * hd].double().view(q.shape[0], Hh, hd).transpose(0, 1)


def _b_heads(t, B, rows, Hh, hd, col0=0):
    """[B rows, >= col0 + Hh hd] -> [B, Hh, rows, hd] fp64."""
    return t[:, col0:col0 + Hh * hd].double().view(B, rows, Hh, hd).transpose(1, 2)


def _b_rows(t):
    """[B, Hh, rows, hd] -> [B rows, Hh hd]."""
    B, Hh, rows, hd = t.shape
    return t.transpose(1, 2).reshape(B * rows, Hh * hd)


class PoolRef:
    """What pool_ref64 returns, all fp64: q [Hh, n_q, hd]; k, v [B, Hh, L, hd]; do [B, Hh, n_q, hd]; p, ds [B, Hh, n_q, L];
    lse [B Hh, n_q] (log2 units); o, pv [B n_q, E]; dq [n_q, E]; dq_img [B, n_q, E] (per image); dk, dv [B L, E]; scale."""


def pool_ref64(q, kv, dout, B, L, nq, Hh, hd):
    """S = scale Q K_b^T, P = softmax(S), O = P V_b; with dout: delta = rowsum(dO * O), dV = P^T dO, dS = P * (dO V^T - delta),
    dQ = scale sum_b dS_b K_b, dK = scale dS^T Q.  pv = P.|V|."""
    r = PoolRef()
    E = Hh * hd
    r.q = qh = _q_heads(q, Hh, hd)
    r.k, r.v = k, v = _b_heads(kv, B, L, Hh, hd), _b_heads(kv, B, L, Hh, hd, E)
    r.scale = scale = hd ** -0.5
    s = qh[None] @ k.transpose(-1, -2) * scale                      # [B, Hh, n_q, L]
    r.lse = (torch.logsumexp(s, -1) * LOG2E).reshape(B * Hh, nq)
    r.p = p = torch.softmax(s, -1)
    o = p @ v
    r.o, r.pv = _b_rows(o), _b_rows(p @ v.abs())
    if dout is not None:
        r.do = do = _b_heads(dout, B, nq, Hh, hd)
        r.ds = ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
        r.dq_img = (ds @ k * scale).transpose(1, 2).reshape(B, nq, E)
        r.dq = r.dq_img.sum(0)
        r.dk, r.dv = _b_rows(ds.transpose(-1, -2) @ qh[None] * scale), _b_rows(p.transpose(-1, -2) @ do)
    return r


def fwd_bound(r):
    """hipops.bound: bf16 output rounding + P rounded to bf16 before P.V, 2^-8 each."""
    return REL * r.o.abs() + REL * r.pv + 1e-6


def bwd_bounds(r, eo):
    """(bound_dq [n_q, E], bound_dk, bound_dv [B L, E]) as hipops.bwd_bound derives them, eo [B n_q, E] bounding |out - O|:
        Ed = sum_d |dO| eo,   W = U |dS| + P Ed
        bound_dV = U |dV| + U (P^T |dO|) + 1e-6,   bound_dK = U |dK| + scale (W^T |Q|) + 1e-6
        bound_dQ = sum over the images of scale (W_b |K_b|), + 1e-6: dq is fp32, so there is no output-rounding term."""
    B, Hh, nq, hd = r.do.shape
    ed = (r.do.abs() * _b_heads(eo, B, nq, Hh, hd)).sum(-1, keepdim=True)
    w = U_BWD * r.ds.abs() + r.p * ed
    bdv = U_BWD * r.dv.abs() + U_BWD * _b_rows(r.p.transpose(-1, -2) @ r.do.abs()) + 1e-6
    bdk = U_BWD * r.dk.abs() + r.scale * _b_rows(w.transpose(-1, -2) @ r.q.abs()[None]) + 1e-6
    bdq = r.scale * (w @ r.k.abs()).transpose(1, 2).reshape(B, nq, Hh * hd).sum(0) + 1e-6
    return bdq, bdk, bdv


def ratio(got, want, bd):
    """max |got - want| / bound (<= 1: inside)."""
    return float(((got.double().cpu() - want).abs() / bd).max())


def fwd_ratio(out, r):
    return ratio(out[:, :r.o.shape[1]], r.o, fwd_bound(r))


def bwd_ratios(dq, dkv, r, bounds):
    E = r.dq.shape[1]
    return (ratio(dq[:, :E], r.dq, bounds[0]), ratio(dkv[:, :E], r.dk, bounds[1]), ratio(dkv[:, E:2 * E], r.dv, bounds[2]))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def pool_case(B, L, nq, Hh, hd, seed):
    """Gaussian bf16 (q, kv, dout)."""
    E = Hh * hd
    return (rnd(nq, E, seed=seed).to(torch.bfloat16), rnd(B * L, 2 * E, seed=seed + 1).to(torch.bfloat16),
            rnd(B * nq, E, seed=seed + 2).to(torch.bfloat16))


def spiked_pool_case(B, L, nq, Hh, hd, seed, boost=32.0, delta=20.0):
    """pool_case with the last key of every (image, head) set to alpha Q[i], i = (97 j + 5) % n_q for head j = b Hh + h, as
    hipops.spiked_bwd_case / spiked_qkv build theirs.  Even j: alpha makes the key's log2 logit in row i equal the log2-sum-exp of the
    other keys, so it holds half of row i's softmax (weight asserted in [0.3, 0.7]).  Odd j: the logit exceeds row i's maximum over the
    other keys by `delta` log2 units, which forces the rescale when the key comes in a later tile.  The rows of dout that feed the last
    query are multiplied by `boost`.  L >= 2.  Returns (q, kv, dout, [(b, h, i, weight or realised delta)])."""
    q, kv, dout = pool_case(B, L, nq, Hh, hd, seed)
    E = Hh * hd
    qx = q.view(nq, Hh, hd)
    kx = kv.view(B, L, 2, Hh, hd)
    c = hd ** -0.5 * LOG2E
    probes = []
    for b in range(B):
        for h in range(Hh):
            j = b * Hh + h
            i = (97 * j + 5) % nq
            qi = qx[i, h].double()
            others = kx[b, :L - 1, 0, h].double() @ qi * c
            if j % 2 == 0:
                target = float(torch.logsumexp(others / LOG2E, 0)) * LOG2E
            else:
                target = float(others.max()) + delta
            kx[b, L - 1, 0, h] = (target / (float(qi @ qi) * c) * qi).to(torch.bfloat16)
            logit = float(kx[b, L - 1, 0, h].double() @ qi) * c
            if j % 2 == 0:
                weight = 1.0 / (1.0 + 2.0 ** (target - logit))
                assert 0.3 <= weight <= 0.7, (b, h, i, weight)
                probes.append((b, h, i, weight))
            else:
                got = logit - float(others.max())
                assert abs(got - delta) < 0.5, (b, h, i, got)
                probes.append((b, h, i, got))
    dout.view(B, nq, E)[:, nq - 1] *= boost
    return q, kv, dout, probes


# ---- an emulation of the kernels' arithmetic (CPU, fp32) -------------------------------------------------------------------------------
FWD_BUGS = ("drop_key", "norm_drop")
BWD_BUGS = {"drop_key": (0,), "drop_query": (1, 2), "drop_image": (0,), "norm_drop": (0, 1, 2), "delta_half": (0, 1)}


def _bf(t):
    return t.to(torch.bfloat16).float()


def emulate(q, kv, dout, out, B, L, nq, Hh, hd, bug=None):
    """The kernels' arithmetic on the CPU: fp32 scores in log2 units, fp32 row maximum / sum / lse, P rounded to bf16 before P.V, bf16 out;
    backward: p = exp2(s - lse), delta from the bf16 `out` handed in (None: the emulated forward's), dS and P rounded to bf16 before the
    fp32 second products, bf16 dk / dv, fp32 dq summed over the images in order.  Returns (out, lse [B Hh, n_q], dq, dkv) as fp32.
    bug: drop_key (the last key is left out of P.V and of dQ), drop_query (the last query out of dK / dV), drop_image (the last image
    out of dq), norm_drop (the normaliser misses the last key), delta_half (delta over d < 32 only)."""
    E = Hh * hd
    scale = hd ** -0.5
    qh = _q_heads(q, Hh, hd).float()
    k, v = _b_heads(kv, B, L, Hh, hd).float(), _b_heads(kv, B, L, Hh, hd, E).float()
    s = qh[None] @ k.transpose(-1, -2) * (scale * LOG2E)
    sn = s[..., :L - 1] if bug == "norm_drop" else s
    m = sn.amax(-1, keepdim=True)
    lsum = torch.exp2(sn - m).sum(-1, keepdim=True)
    lse = m + torch.log2(lsum)
    pf = torch.exp2(s - m)
    if bug == "drop_key":
        pf[..., L - 1] = 0.0
    o = _b_rows(_bf(_bf(pf) @ v / lsum))
    if dout is None:
        return o, lse.reshape(B * Hh, nq), None, None
    do = _b_heads(dout, B, nq, Hh, hd).float()
    oh = _b_heads(o if out is None else out, B, nq, Hh, hd).float()
    p = torch.exp2(s - lse)
    nd = 32 if bug == "delta_half" else hd
    delta = (do[..., :nd] * oh[..., :nd]).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - delta)
    ds2, p3, ds3 = ds.clone(), p.clone(), ds.clone()
    if bug == "drop_key":
        ds2[..., L - 1] = 0.0
    if bug == "drop_query":
        p3[:, :, nq - 1] = 0.0
        ds3[:, :, nq - 1] = 0.0
    dq_img = (_bf(ds2) @ k).transpose(1, 2).reshape(B, nq, E)
    dq = torch.zeros(nq, E)
    for b in range(B - 1 if bug == "drop_image" else B):
        dq = dq + dq_img[b]
    dk = _b_rows(_bf(_bf(ds3).transpose(-1, -2) @ qh[None] * scale))
    dv = _b_rows(_bf(_bf(p3).transpose(-1, -2) @ do))
    return o, lse.reshape(B * Hh, nq), dq * scale, torch.cat([dk, dv], 1)


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def attn_pool(q, kv, B, L, nq, Hh, hd, out=None, lse=True):
    """ov_attn_pool: (out [B n_q, E] bf16, lse [B Hh, n_q rounded up to 32] fp32, NaN where the kernel writes nothing)."""
    from openvision_amd import _lib
    lib = _lib.load()
    if out is None:
        out = torch.empty(B * nq, Hh * hd, dtype=torch.bfloat16, device=q.device)
    ls = torch.full((B * Hh, (nq + 31) // 32 * 32), float("nan"), dtype=torch.float32, device=q.device) if lse else None
    _lib.check(lib.ov_attn_pool(_lib.ptr(q), q.stride(0), _lib.ptr(kv), kv.stride(0), _lib.ptr(out), out.stride(0), _lib.ptr(ls), B, L, nq,
                                Hh, hd, hd ** -0.5, _lib.stream_ptr()), "ov_attn_pool")
    return out, ls


def attn_pool_backward(q, kv, out, dout, lse, B, L, nq, Hh, hd, dkv=None):
    """ov_attn_pool_backward: (dq [n_q, E] fp32, dkv [B L, 2 E] bf16)."""
    from openvision_amd import _lib
    lib = _lib.load()
    E = Hh * hd
    dq = torch.full((nq, E), float("nan"), dtype=torch.float32, device=q.device)
    if dkv is None:
        dkv = torch.empty(B * L, 2 * E, dtype=torch.bfloat16, device=q.device)
    nb = lib.ov_attn_pool_backward_workspace_bytes(B, L, nq, Hh, hd)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=q.device)
    _lib.check(lib.ov_attn_pool_backward(_lib.ptr(q), q.stride(0), _lib.ptr(kv), kv.stride(0), _lib.ptr(out), out.stride(0), _lib.ptr(dout),
                                         dout.stride(0), _lib.ptr(lse), _lib.ptr(dq), dq.stride(0), _lib.ptr(dkv), dkv.stride(0), B, L, nq,
                                         Hh, hd, hd ** -0.5, _lib.ptr(ws), nb, _lib.stream_ptr()), "ov_attn_pool_backward")
    return dq, dkv
