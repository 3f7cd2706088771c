"""The backward bound of test_gpu_attention_bwd_edges.py (hipops.bwd_bound) against an emulation of the kernels' arithmetic, no GPU.

As test_attention_bound.py does for the forward: the bound is only worth what it can tell apart.  One head is computed the way
attention_bwd.hip computes it -- fp32 scores in log2 units and an fp32 row lse, p = exp2(s - lse), delta from the bf16 `out`, dS and P
rounded to bf16 before fp32 second products, bf16 outputs -- and must sit inside half the bound on every component; the same emulation
with one of the mistakes below must leave the bound on every component the mistake touches.

    bug             what goes wrong                                                          leaves the bound on
    dq_drop_key     pass 2 leaves the last key out of dQ                                     dq
    kv_drop_query   pass 3 leaves the last query out of dK / dV                              dk, dv
    lse_drop        the last key is missing from the normaliser only (pass 1)                dq, dk, dv
    delta_half      delta summed over d < 32 only                                            dq, dk
    P+1, P-1        the prefix of the mask off by one (masked cases)                         dq, dk, dv
    strict          the diagonal is not visible (masked cases)                               dq, dk, dv
"""
import pytest
import torch

import hipops as H
from hipops import LOG2E, LONE_SPIKED, U_BWD, attn_grads_ref64, bwd_bound, bwd_err_ratio, spiked_bwd_case
import prefix_restate as PR

UNMASKED_BUGS = {"dq_drop_key": (0,), "kv_drop_query": (1, 2), "lse_drop": (0, 1, 2), "delta_half": (0, 1)}
MASK_BUGS = ("P+1", "P-1", "strict")
NAMES = ("dq", "dk", "dv")


def emulate_head(q, k, v, do, out, scale, mask=None, bug=None):
    """One head ([L, hd] fp32 tensors holding bf16 values; `out` is the bf16 forward output handed to the kernel; mask: [L, L] bool or
    None) -> dq, dk, dv as bf16-rounded fp32."""
    L = q.shape[0]
    bf = lambda t: t.to(torch.bfloat16).float()
    s = (q @ k.T) * (scale * LOG2E)                                  # fp32, log2 units
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    sn = s[:, :L - 1] if bug == "lse_drop" else s                    # pass 1: the normaliser
    m = sn.amax(1, keepdim=True)
    lse = m + torch.log2(torch.exp2(sn - m).sum(1, keepdim=True))
    p = torch.exp2(s - lse)                                          # 0 for a hidden pair: exp2(-inf)
    nd = 32 if bug == "delta_half" else q.shape[1]
    delta = (do[:, :nd] * out[:, :nd]).sum(1, keepdim=True)
    ds = p * (do @ v.T - delta)
    ds2 = ds.clone()                                                 # pass 2 (dQ) and pass 3 (dK, dV) recompute P and dS separately
    p3, ds3 = p.clone(), ds.clone()
    if bug == "dq_drop_key":
        ds2[:, L - 1] = 0.0
    if bug == "kv_drop_query":
        p3[L - 1] = 0.0
        ds3[L - 1] = 0.0
    return bf(bf(ds2) @ k * scale), bf(bf(ds3).T @ q * scale), bf(bf(p3).T @ do)


def emulate(qkv, dout, out, B, L, Hh, hd, mask=None, bug=None):
    """[B*L, 3 Hh hd] (dq | dk | dv) fp32 from emulate_head over every head."""
    q, k, v = [t.float() for t in H._split(qkv, B, L, Hh, hd)]
    do, o = H._heads(dout, B, L, Hh, hd).float(), H._heads(out, B, L, Hh, hd).float()
    res = torch.empty(3, B, Hh, L, hd)
    for b in range(B):
        for h in range(Hh):
            for j, t in enumerate(emulate_head(q[b, h], k[b, h], v[b, h], do[b, h], o[b, h], hd ** -0.5, mask, bug)):
                res[j, b, h] = t
    return torch.cat([H._rows(res[j]) for j in range(3)], dim=1)


def reference(qkv, dout, B, L, Hh, hd, mask=None):
    """(ref, bounds, out): out = bf16(reference O), so |out - O| <= 2^-8 |O|; the bound is taken with eo = U |O|."""
    ref = attn_grads_ref64(qkv, dout, B, L, Hh, hd, mask)
    bounds = bwd_bound(ref, ref.q, ref.k, ref.v, ref.do, ref.scale, U_BWD * ref.o.abs())
    return ref, bounds, ref.o.to(torch.bfloat16)


@pytest.mark.parametrize("B,L,Hh,hd", LONE_SPIKED + [(1, 33, 2, 64)])
def test_bwd_bound_tells_tail_mistakes_apart(B, L, Hh, hd):
    """No GPU.  spiked_bwd_case: the clean emulation is inside half the bound; each mistake leaves it on the components it touches."""
    qkv, dout, _ = spiked_bwd_case(B, L, Hh, hd, seed=L + hd)
    ref, bounds, out = reference(qkv, dout, B, L, Hh, hd)
    ok = bwd_err_ratio(emulate(qkv, dout, out, B, L, Hh, hd), ref, bounds)
    print(f"bwd bound L={L} hd={hd}: clean " + " ".join(f"{n} {r:.3f}" for n, r in zip(NAMES, ok)))
    assert max(ok) <= 0.5, ok
    for bug, touched in UNMASKED_BUGS.items():
        bad = bwd_err_ratio(emulate(qkv, dout, out, B, L, Hh, hd, bug=bug), ref, bounds)
        print(f"  {bug}: " + " ".join(f"{n} {r:.2f}" for n, r in zip(NAMES, bad)))
        for j in touched:
            assert bad[j] > 1.0, (bug, NAMES[j], bad, ok)


def wrong_mask(L, P, bug):
    i = torch.arange(L)[:, None]
    j = torch.arange(L)[None, :]
    return {"P+1": PR.rule_mask(L, P + 1), "P-1": PR.rule_mask(L, P - 1), "strict": (j < P) | (j < i)}[bug]


@pytest.mark.parametrize("B,L,Hh,hd,P", [(1, 307, 2, 64, 179), (1, 65, 2, 64, 33), (1, 463, 1, 80, 335)])
def test_bwd_bound_tells_mask_mistakes_apart(B, L, Hh, hd, P):
    """No GPU.  boundary_spiked_qkv with a Gaussian dout under the prefix-causal rule: clean inside half the bound, a prefix off by
    one or a hidden diagonal outside it on dq, dk and dv."""
    qkv, _ = PR.boundary_spiked_qkv(B, L, Hh, hd, P, seed=L + hd)
    dout = H.rnd(B * L, Hh * hd, seed=L + hd + 1).to(torch.bfloat16)
    mask = PR.rule_mask(L, P)
    ref, bounds, out = reference(qkv, dout, B, L, Hh, hd, mask)
    ok = bwd_err_ratio(emulate(qkv, dout, out, B, L, Hh, hd, mask), ref, bounds)
    print(f"bwd bound L={L} hd={hd} P={P}: clean " + " ".join(f"{n} {r:.3f}" for n, r in zip(NAMES, ok)))
    assert max(ok) <= 0.5, ok
    for bug in MASK_BUGS:
        bad = bwd_err_ratio(emulate(qkv, dout, out, B, L, Hh, hd, wrong_mask(L, P, bug)), ref, bounds)
        print(f"  {bug}: " + " ".join(f"{n} {r:.2f}" for n, r in zip(NAMES, bad)))
        assert min(bad) > 1.0, (bug, bad, ok)
