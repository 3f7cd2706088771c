"""The bounds of test_gpu_attn_pool.py (poolops.fwd_bound, poolops.bwd_bounds) against an emulation of attn_pool.hip's arithmetic, no GPU.

As test_attention_bwd_bound.py does for self-attention: a bound is only worth what it can tell apart.  poolops.emulate computes the
pooler the way the kernels do and must sit inside half the bound on every component; the same emulation with one of the mistakes
below must leave the bound on every component the mistake touches.

    bug          what goes wrong                                             leaves the bound on
    drop_key     the last key is left out of P.V and of dQ                   out, dq
    drop_query   the last query is left out of dK / dV                       dk, dv
    drop_image   the last image is left out of the dq sum                    dq
    norm_drop    the normaliser misses the last key                          out, lse, dq, dk, dv
    delta_half   delta summed over d < 32 only                               dq, dk
"""
import pytest
import torch

import poolops as PO
from hipops import U_BWD

NAMES = ("dq", "dk", "dv")
# (B, L, n_q, Hh, hd): the lone last key of a tile (33) and of a chunk (257); one, several and all eight query tiles
CASES = [(2, 33, 5, 2, 64), (2, 257, 33, 2, 96), (3, 65, 256, 2, 72), (2, 17, 1, 2, 64)]


@pytest.mark.parametrize("B,L,nq,Hh,hd", CASES)
def test_pool_bounds_tell_tail_mistakes_apart(B, L, nq, Hh, hd):
    q, kv, dout, _ = PO.spiked_pool_case(B, L, nq, Hh, hd, seed=L + hd + nq)
    r = PO.pool_ref64(q, kv, dout, B, L, nq, Hh, hd)
    out = r.o.to(torch.bfloat16)                                     # |out - O| <= 2^-8 |O|: the bound is taken with eo = U |O|
    bounds = PO.bwd_bounds(r, U_BWD * r.o.abs())
    o, lse, dq, dkv = PO.emulate(q, kv, dout, out, B, L, nq, Hh, hd)
    ok_f, ok_b = PO.fwd_ratio(o, r), PO.bwd_ratios(dq, dkv, r, bounds)
    lse_err = float((lse.double() - r.lse).abs().max())
    print(f"pool bound B={B} L={L} n_q={nq} hd={hd}: clean out {ok_f:.3f} lse {lse_err:.2e} " + " ".join(f"{n} {x:.3f}" for n, x in zip(NAMES, ok_b)))
    assert ok_f <= 0.5 and max(ok_b) <= 0.5 and lse_err <= PO.LSE_ATOL / 2, (ok_f, ok_b, lse_err)
    for bug in PO.FWD_BUGS:
        o2, lse2, _, _ = PO.emulate(q, kv, None, None, B, L, nq, Hh, hd, bug=bug)
        bad = PO.fwd_ratio(o2, r)
        print(f"  fwd {bug}: out {bad:.2f}")
        assert bad > 1.0, (bug, bad)
        if bug == "norm_drop":
            assert float((lse2.double() - r.lse).abs().max()) > PO.LSE_ATOL
    for bug, touched in PO.BWD_BUGS.items():
        _, _, dq2, dkv2 = PO.emulate(q, kv, dout, out, B, L, nq, Hh, hd, bug=bug)
        bad = PO.bwd_ratios(dq2, dkv2, r, bounds)
        print(f"  bwd {bug}: " + " ".join(f"{n} {x:.2f}" for n, x in zip(NAMES, bad)))
        for j in touched:
            assert bad[j] > 1.0, (bug, NAMES[j], bad, ok_b)
