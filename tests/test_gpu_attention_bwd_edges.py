"""Attention backward at its edges, against an fp64 closed form with per-element bounds on dQ, dK and dV.

attention_bwd.hip holds the resident kernel (head_dim 64, short sequences; recomputing and saved-lse forms) and the two streaming kernels in
NDH = 2 / 3 form, each with and without the prefix mask.  The rule of the older backward tests, max|got - want| < 2e-2 max|want| +
1e-3 per component, cannot see anything below 2 % of the largest gradient element: a key missing from the normaliser only, a wrong
d slice of a small row, whole rows beside one large dout row.  These tests hold every element to

    Ed       = sum_d |dO| eo                      eo: a bound on |out - O| of the `out` handed to the kernel
    W        = U |dS| + P Ed
    |dV err| <= U |dV| + U (P^T |dO|)     + 1e-6
    |dQ err| <= U |dQ| + scale (W |K|)    + 1e-6
    |dK err| <= U |dK| + scale (W^T |Q|)  + 1e-6          U = 2^-7

(hipops.bwd_bound, where the terms are derived: U is twice bf16's unit roundoff, not a measured figure), on inputs whose last key
holds half of one row's softmax and whose last query carries a 32 x larger dout (hipops.spiked_bwd_case), resp. whose mask-boundary
keys are spiked (prefix_restate.boundary_spiked_qkv).  test_attention_bwd_bound.py (CPU) pins what the bound can see."""
import pytest
import torch

import hipops as H
from hipops import U_BWD, attn_grads_ref64, bwd_bound, bwd_err_ratio, spiked_bwd_case
import prefix_restate as PR
from test_gpu_prefix_attention import SHAPES as PREFIX_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def reference(qkv, dout, B, L, Hh, hd, mask=None):
    """(ref, bounds for out = bf16(reference O): eo = U |O|, that out on the device)."""
    ref = attn_grads_ref64(qkv, dout, B, L, Hh, hd, mask)
    bounds = bwd_bound(ref, ref.q, ref.k, ref.v, ref.do, ref.scale, U_BWD * ref.o.abs())
    return ref, bounds, ref.o.to(torch.bfloat16).to(DEV)


def check_ratios(tag, got, ref, bounds):
    r = bwd_err_ratio(got.cpu(), ref, bounds)
    print(f"attention backward {tag}: max err / bound dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")
    assert max(r) <= 1.0, r
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# A. every kernel and tail

# shape -> what the library's route must name for it (hipops.attn_route(...).bwd_form)
RES, S2, S3 = "resident", "stream<2>", "stream<3>"
BWD_FORMS = {
    # resident (head_dim 64, up to nine waves): one partial tile; a last tile of one row (33, 65, 257); full, nine waves
    (1, 31, 2, 64): RES, (2, 33, 2, 64): RES, (1, 65, 3, 64): RES, (2, 257, 4, 64): RES, (1, 288, 1, 64): RES,
    # Stream<2>: the first streaming L (second chunk of 33 rows); a last chunk of one row (513, 2305); the batch offset
    (1, 289, 2, 64): S2, (1, 513, 2, 64): S2, (2, 513, 2, 64): S2, (1, 2305, 1, 64): S2,
    # Stream<2>, head_dim < 64 at one chunk plus one row: the zero-fill paths (col < hd, 16 st + 8 h2 < hd, d0 < hd)
    (1, 257, 2, 8): S2, (1, 257, 2, 32): S2, (1, 257, 2, 56): S2,
    # Stream<3>: 730 a ragged last chunk; 769 at 96 no zero padding and a last chunk of one row
    (1, 257, 2, 72): S3, (1, 257, 2, 88): S3, (1, 257, 2, 96): S3, (1, 321, 2, 80): S3, (3, 257, 2, 80): S3, (1, 577, 2, 80): S3,
    (1, 730, 2, 72): S3, (1, 769, 1, 96): S3,
}
BWD_SHAPES = list(BWD_FORMS)
PITCH_FORMS = {(2, 257, 4, 64, None): "resident", (1, 513, 2, 64, None): "stream<2>", (2, 257, 3, 80, None): "stream<3>",
               (2, 307, 2, 64, 179): "stream<2> mask"}


@pytest.mark.parametrize("B,L,Hh,hd", BWD_SHAPES)
def test_attention_backward_edges(B, L, Hh, hd):
    assert H.attn_route(B, L, Hh, hd).bwd_form == BWD_FORMS[B, L, Hh, hd]      # the kernel the case is here for (a host call: no launch)
    qkv, dout, _ = spiked_bwd_case(B, L, Hh, hd, seed=L * 131 + hd)
    ref, bounds, out = reference(qkv, dout, B, L, Hh, hd)
    got = H.attention_backward(qkv.to(DEV), out, dout.to(DEV), B, L, Hh, hd)
    check_ratios(f"B={B} L={L} H={Hh} hd={hd}", got, ref, bounds)
    assert torch.equal(got, H.attention_backward(qkv.to(DEV), out, dout.to(DEV), B, L, Hh, hd))        # deterministic


# ------------------------------------------------------------------------------------------------------------------------------
# B. pitches and neighbours

PAD_SENTINEL = -1234.5
WS_SENTINEL = 0xA5


def padded(dense, pad):
    """`dense` as the leading columns of a tensor `pad` columns wider whose other columns hold NaN: (the slice, the wide tensor)."""
    wide = torch.full((dense.shape[0], dense.shape[1] + pad), float("nan"), dtype=torch.bfloat16)
    wide[:, :dense.shape[1]] = dense
    wide = wide.to(DEV)
    return wide[:, :dense.shape[1]], wide


@pytest.mark.parametrize("B,L,Hh,hd,P", [(2, 257, 4, 64, None), (1, 513, 2, 64, None), (2, 257, 3, 80, None), (2, 307, 2, 64, 179)])
def test_attention_backward_pitches_and_neighbours(B, L, Hh, hd, P):
    """Resident, Stream<2>, Stream<3> and the prefix call with row pitches 3D + 64 (qkv, dqkv), D + 64 (out) and D + 32 (dout).  The
    pad columns of the inputs hold NaN (a read of them would show); those of dqkv hold a sentinel that must survive bitwise; the
    workspace is a view of exactly *_workspace_bytes bytes with a 256-byte sentinel tail behind it that must survive.  The result is
    bitwise the dense call's and inside the bound."""
    D = Hh * hd
    lib = H._lib.load()
    route = H.attn_route(B, L, Hh, hd, prefix=P, ld_qkv=3 * D + 64, ld_out=D + 64)
    assert route.bwd_form == PITCH_FORMS[B, L, Hh, hd, P]
    if P is None:
        qkv, dout, _ = spiked_bwd_case(B, L, Hh, hd, seed=L + hd + 7)
        mask = None
        nb = lib.ov_attention_backward_workspace_bytes(B, L, Hh, hd)
        call = lambda q, o, d, **kw: H.attention_backward(q, o, d, B, L, Hh, hd, **kw)
    else:
        qkv = PR.boundary_spiked_qkv(B, L, Hh, hd, P, seed=L + hd + 7)[0]
        dout = H.rnd(B * L, D, seed=L + hd + 8).to(torch.bfloat16)
        mask = PR.rule_mask(L, P)
        nb = lib.ov_attention_prefix_backward_workspace_bytes(B, L, Hh, hd)
        call = lambda q, o, d, **kw: PR.attention_prefix_backward(q, o, d, B, L, Hh, hd, P, **kw)
    ref, bounds, out = reference(qkv, dout, B, L, Hh, hd, mask)
    want = call(qkv.to(DEV), out, dout.to(DEV))

    qkv_p, qkv_w = padded(qkv, 64)
    out_p, out_w = padded(out.cpu(), 64)
    dout_p, dout_w = padded(dout, 32)
    assert (qkv_p.stride(0), out_p.stride(0), dout_p.stride(0)) == (3 * D + 64, D + 64, D + 32)
    dq_w = torch.full((B * L, 3 * D + 64), PAD_SENTINEL, dtype=torch.bfloat16, device=DEV)
    buf = torch.full((nb + 256,), WS_SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0 and nb == route.bwd_workspace_bytes
    got = call(qkv_p, out_p, dout_p, dqkv=dq_w[:, :3 * D], ws=buf[:nb])
    torch.cuda.synchronize()
    assert got.stride(0) == 3 * D + 64
    assert bool((buf[nb:] == WS_SENTINEL).all()), "the workspace was overrun"
    assert torch.equal(dq_w[:, 3 * D:].view(torch.int16), torch.full_like(dq_w[:, 3 * D:], PAD_SENTINEL).view(torch.int16))
    check_ratios(f"padded B={B} L={L} H={Hh} hd={hd} P={P}", got, ref, bounds)
    assert torch.equal(got, want)                                     # the pitches change nothing else


# ------------------------------------------------------------------------------------------------------------------------------
# C. the saved-lse kernel against the truth


@pytest.mark.parametrize("B,L,Hh,hd", [(1, 33, 2, 64), (2, 257, 4, 64), (1, 288, 1, 64)])
def test_attention_backward_saved_lse_within_bound(B, L, Hh, hd):
    """out and lse from ov_attention_lse (lse entries [L, KC) hold NaN: hipops.attention_lse), so |out - O| is what the forward's own
    enforced bound allows: eo = hipops.bound(O, P.|V|)."""
    route = H.attn_route(B, L, Hh, hd, lse=True)
    assert route.bwd_form == "resident saved" and route.keep_lse and route.form == "persistent" and route.lse
    qkv, dout, _ = spiked_bwd_case(B, L, Hh, hd, seed=L * 131 + hd + 1)
    ref = attn_grads_ref64(qkv, dout, B, L, Hh, hd)
    bounds = bwd_bound(ref, ref.q, ref.k, ref.v, ref.do, ref.scale, H.bound(ref.o, ref.pv))
    out, lse = H.attention_lse(qkv.to(DEV), B, L, Hh, hd)
    got = H.attention_backward_saved(qkv.to(DEV), out, dout.to(DEV), lse, B, L, Hh, hd)
    check_ratios(f"saved lse B={B} L={L} H={Hh} hd={hd}", got, ref, bounds)


# ------------------------------------------------------------------------------------------------------------------------------
# D. the prefix backward on the boundary-spiked inputs

# prefixes on and next to a 256-row chunk edge
PREFIX_BWD_SHAPES = [s for s in PREFIX_SHAPES if s[1] >= 4] + [(1, 513, 2, 64, 256), (1, 513, 2, 64, 257), (1, 513, 1, 80, 512)]


@pytest.mark.parametrize("B,L,Hh,hd,P", PREFIX_BWD_SHAPES)
def test_prefix_backward_edges(B, L, Hh, hd, P):
    assert H.attn_route(B, L, Hh, hd, prefix=P).bwd_form == ("stream<2> mask" if hd == 64 else "stream<3> mask")    # always the streaming pair
    qkv = PR.boundary_spiked_qkv(B, L, Hh, hd, P, seed=L * 131 + hd + P)[0]
    dout = H.rnd(B * L, Hh * hd, seed=L * 131 + hd + P + 1).to(torch.bfloat16)
    ref, bounds, out = reference(qkv, dout, B, L, Hh, hd, PR.rule_mask(L, P))
    got = PR.attention_prefix_backward(qkv.to(DEV), out, dout.to(DEV), B, L, Hh, hd, P)
    check_ratios(f"prefix B={B} L={L} H={Hh} hd={hd} P={P}", got, ref, bounds)
