"""GPU: ov_attention_prefix / ov_attention_prefix_backward (key j visible to query i iff j < P or j <= i).

Oracle: the masked softmax attention in fp64 on the bf16 inputs (tests/prefix_restate.py, a restatement -- no reference-generated
fixture backs these tests: jax / flax were not importable where they were written).  The forward is held to the project's per-element
bound |got - ref| <= 2^-8 |ref| + 2^-8 (P.|V|) + 1e-6 (hipops.bound; P.|V| over the visible keys) on inputs whose mask-boundary keys
are spiked (tests/test_prefix_cpu.py shows that an off-by-one mask leaves that bound on exactly these inputs); the backward to the rule
of test_attention_backward_vs_oracle, max|got - want| < 2e-2 max|want| + 1e-3 per dq / dk / dv."""
import pytest
import torch

import hipops as H
from hipops import err_ratio
import prefix_restate as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, L, Hh, hd, P): the issue's shapes.  463 = 256 + 79 + 128 is the L/14 decoder, 307 the tiny preset's.
SHAPES = [(2, 80, 2, 64, 0), (2, 307, 2, 64, 179), (2, 463, 2, 64, 335), (1, 257, 2, 64, 1), (1, 257, 2, 64, 256), (2, 33, 2, 64, 32),
          (2, 65, 2, 64, 31), (2, 65, 2, 64, 33), (3, 1, 2, 64, 0), (1, 2305, 1, 64, 2000),
          (1, 207, 2, 72, 79), (1, 463, 2, 72, 335), (1, 207, 2, 80, 79), (1, 463, 2, 80, 335)]


def masked_route(B, L, Hh, hd, P, cus=0):
    """What the library reports for the masked call, held to what DESIGN.md states for every masked shape: the generic forward
    kernel's MASK form (head_dim 64 at its own width, the others padded to 96) and the masked streaming pair in the backward."""
    r = H.attn_route(B, L, Hh, hd, prefix=P, cus=cus)
    assert (r.kernel, r.mask, r.hdp) == ("generic", True, 64 if hd == 64 else 96), vars(r)
    assert (r.bwd, r.bwd_mask, r.keep_lse) == ("streaming", True, False) and r.bwd_workspace_bytes > 0, vars(r)
    return r


def inputs(B, L, Hh, hd, P, seed=0):
    if L >= 4:
        return PR.boundary_spiked_qkv(B, L, Hh, hd, P, seed)[0]
    return H.rnd(B * L, 3 * Hh * hd, seed=seed).to(torch.bfloat16)


@pytest.mark.parametrize("B,L,Hh,hd,P", SHAPES)
def test_prefix_forward_within_bound(B, L, Hh, hd, P):
    masked_route(B, L, Hh, hd, P)
    qkv = inputs(B, L, Hh, hd, P)
    got = PR.attention_prefix(qkv.to(DEV), B, L, Hh, hd, P).cpu()
    ref, pv = PR.masked_attn_ref64(qkv, B, L, Hh, hd, PR.rule_mask(L, P))
    r = err_ratio(got, ref, pv)
    print(f"prefix attention B={B} L={L} H={Hh} hd={hd} P={P}: max err / bound {r:.3f}")
    assert r <= 1.0, r


def test_prefix_forward_padded_pitch():
    B, L, Hh, hd, P = 2, 307, 2, 64, 179
    assert H.attn_route(B, L, Hh, hd, prefix=P, ld_qkv=3 * Hh * hd + 64, ld_out=Hh * hd + 32).form == masked_route(B, L, Hh, hd, P).form
    qkv = inputs(B, L, Hh, hd, P, seed=3)
    wide = torch.zeros(B * L, 3 * Hh * hd + 64, dtype=torch.bfloat16, device=DEV)
    wide[:, :3 * Hh * hd] = qkv.to(DEV)
    out = torch.full((B * L, Hh * hd + 32), 7.0, dtype=torch.bfloat16, device=DEV)
    PR.attention_prefix(wide, B, L, Hh, hd, P, out=out)
    ref, pv = PR.masked_attn_ref64(qkv, B, L, Hh, hd, PR.rule_mask(L, P))
    r = err_ratio(out[:, :Hh * hd].cpu(), ref, pv)
    print(f"prefix attention, padded pitches: max err / bound {r:.3f}")
    assert r <= 1.0, r
    assert bool((out[:, Hh * hd:] == 7.0).all())                      # nothing written past the heads


@pytest.mark.parametrize("B,L,Hh,hd", [(2, 257, 3, 64), (1, 463, 2, 64), (1, 207, 2, 72), (1, 463, 2, 80)])
def test_prefix_equal_L_is_bitwise_the_unmasked_call(B, L, Hh, hd):
    assert vars(H.attn_route(B, L, Hh, hd, prefix=L)) == vars(H.attn_route(B, L, Hh, hd)) and not H.attn_route(B, L, Hh, hd, prefix=L).mask
    qkv = H.rnd(B * L, 3 * Hh * hd, seed=5).to(torch.bfloat16).to(DEV)
    a = H.attention(qkv, B, L, Hh, hd)
    b = PR.attention_prefix(qkv, B, L, Hh, hd, L)
    assert torch.equal(a, b)
    dout = H.rnd(B * L, Hh * hd, seed=6).to(torch.bfloat16).to(DEV)
    da = H.attention_backward(qkv, a, dout, B, L, Hh, hd)
    db = PR.attention_prefix_backward(qkv, a, dout, B, L, Hh, hd, L)
    assert torch.equal(da, db)


@pytest.mark.parametrize("B,L,Hh,hd,P", [(1, 307, 2, 64, 179), (1, 463, 1, 64, 335), (1, 65, 2, 64, 33), (1, 207, 1, 72, 79),
                                         (1, 2305, 1, 64, 2000)])
def test_invisible_keys_do_not_touch_a_row(B, L, Hh, hd, P):
    """Changing K and V rows j > i, j >= P leaves output row i bitwise unchanged; two runs are bitwise equal."""
    D = Hh * hd
    qkv = H.rnd(B * L, 3 * D, seed=7).to(torch.bfloat16).to(DEV)
    base = PR.attention_prefix(qkv, B, L, Hh, hd, P)
    assert torch.equal(base, PR.attention_prefix(qkv, B, L, Hh, hd, P))
    for i in sorted({0, P // 2, max(P - 1, 0), P, min(P + 1, L - 2), (P + L) // 2, L - 2}):
        if i < 0 or i >= L - 1:
            continue
        lo = max(i + 1, P)                                             # the first key row i cannot see
        mod = qkv.clone().view(B, L, 3 * D)
        mod[:, lo:, D:] = (mod[:, lo:, D:].float() * -3.0 + 11.0).to(torch.bfloat16)
        got = PR.attention_prefix(mod.view(B * L, 3 * D), B, L, Hh, hd, P)
        assert torch.equal(got.view(B, L, D)[:, i], base.view(B, L, D)[:, i]), (i, lo)


@pytest.mark.parametrize("B,L,Hh,hd,P", [(1, 307, 2, 64, 179), (1, 463, 1, 64, 335), (1, 65, 2, 64, 33), (1, 207, 1, 80, 79)])
def test_backward_zero_structure_and_determinism(B, L, Hh, hd, P):
    """dout non-zero on one row i: dK, dV rows j > max(i, P - 1) are exactly 0, dQ rows other than i are exactly 0."""
    D = Hh * hd
    qkv = H.rnd(B * L, 3 * D, seed=8).to(torch.bfloat16).to(DEV)
    out = PR.attention_prefix(qkv, B, L, Hh, hd, P)
    for i in sorted({0, max(P - 1, 0), P, (P + L) // 2, L - 1}):
        dout = torch.zeros(B, L, D, dtype=torch.bfloat16, device=DEV)
        dout[:, i] = H.rnd(B, D, seed=9 + i).to(torch.bfloat16).to(DEV)
        d = PR.attention_prefix_backward(qkv, out, dout.view(B * L, D), B, L, Hh, hd, P)
        assert torch.equal(d, PR.attention_prefix_backward(qkv, out, dout.view(B * L, D), B, L, Hh, hd, P))
        d = d.view(B, L, 3, D)
        dq = d[:, :, 0].clone()
        assert float(dq[:, i].abs().max()) > 0
        dq[:, i] = 0
        assert not bool(dq.any()), i
        first_hidden = max(i, P - 1) + 1
        assert not bool(d[:, first_hidden:, 1:].any()), i
        assert torch.isfinite(d.float()).all()


@pytest.mark.parametrize("B,L,Hh,hd,P", SHAPES)
def test_prefix_backward_vs_fp64_autograd(B, L, Hh, hd, P):
    D = Hh * hd
    masked_route(B, L, Hh, hd, P)
    qkv = H.rnd(B * L, 3 * D, seed=11).to(torch.bfloat16)
    dout = H.rnd(B * L, D, seed=12).to(torch.bfloat16)
    out = PR.attention_prefix(qkv.to(DEV), B, L, Hh, hd, P)
    got = PR.attention_prefix_backward(qkv.to(DEV), out, dout.to(DEV), B, L, Hh, hd, P).cpu().double().view(B * L, 3, D)
    want = PR.masked_attn_grads64(qkv, dout, B, L, Hh, hd, PR.rule_mask(L, P)).view(B * L, 3, D)
    for j, name in enumerate(("dq", "dk", "dv")):
        err = float((got[:, j] - want[:, j]).abs().max())
        ref = float(want[:, j].abs().max())
        print(f"prefix backward L={L} hd={hd} P={P} {name}: max err {err:.3e} (max |want| {ref:.3e})")
        assert err < 2e-2 * ref + 1e-3, (name, err, ref)


def test_prefix_argument_checks_on_device():
    B, L, Hh, hd = 1, 40, 1, 64
    lib = H._lib.load()
    qkv = H.rnd(B * L, 3 * Hh * hd).to(torch.bfloat16).to(DEV)
    out = torch.empty(B * L, Hh * hd, dtype=torch.bfloat16, device=DEV)
    for p in (-1, L + 1):
        assert lib.ov_attention_prefix(H.ptr(qkv), 192, H.ptr(out), 64, B, L, Hh, hd, 0.125, p, H.stream_ptr()) == -1
