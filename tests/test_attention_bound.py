"""The attention bound of test_gpu_attention_edges.py (hipops.bound) against an emulation of the kernels' arithmetic, no GPU.

The bound is only worth what it can tell apart.  An emulation of the forward kernels (fp32 logits, lazy rescale, P rounded to bf16
before P.V, a lone last key folded in with an unrounded weight) must sit well inside it, and the same emulation with the lone key
mis-handled must land outside it, on the spiked inputs where the lone key is the row maximum."""
import pytest
import torch

from hipops import LOG2E, LONE_SPIKED, _split, attn_ref64, err_ratio, spiked_qkv


def emulate_head(q, k, v, scale, bug=None):
    """One head [L, hd] (bf16 values) the way the forward kernels compute it: fp32 logits in log2 units, 32-key tiles with a lazy
    rescale decided per 32-row query tile (`__all(mx - m <= 8)`), P rounded to bf16 before an fp32 P.V, the row sum over the
    unrounded fp32 P, and a last tile of one key (L = 32 k + 1) folded in with an unrounded weight.  bug: None, "drop" (the lone key
    is left out), "double" (counted twice in the row sum: both lane halves add it) or "unscaled" (the fold moves the running max but
    does not rescale the accumulators, so the lone key's weight is on another scale than the keys before it).
    Returns (bf16-rounded output as fp32, whether the fold took its rescale branch per query tile)."""
    L, hd = q.shape
    assert L % 32 == 1 and L > 32
    c = scale * LOG2E
    t = (q.float() @ k.float().T) * c                               # [L, L] fp32, log2 units
    vf = v.float()
    nqt = (L + 31) // 32
    rows = nqt * 32
    pad = lambda x, fill: torch.cat([x, x.new_full((rows - L,) + x.shape[1:], fill)])
    t = pad(t, 0.0)
    m = torch.full((rows,), -float("inf"))
    lsum = torch.zeros(rows)
    o = torch.zeros(rows, hd)

    def rescale(mx, accumulators=True):
        nonlocal m, lsum, o
        go = ((mx - m) > 8.0).view(nqt, 32).any(1).repeat_interleave(32)
        mn = torch.where(go, torch.maximum(m, mx), m)
        alpha = torch.where(go, torch.exp2(m - mn), torch.ones(()))
        m = mn
        if accumulators:
            lsum = lsum * alpha
            o = o * alpha[:, None]
        return go.view(nqt, 32)[:, 0]

    for k0 in range(0, L - 1, 32):
        s = t[:, k0:k0 + 32]
        rescale(s.max(1).values)
        p = torch.exp2(s - m[:, None])
        lsum = lsum + p.sum(1)
        o = o + p.to(torch.bfloat16).float() @ vf[k0:k0 + 32]
    went = torch.zeros(nqt, dtype=torch.bool)
    if bug != "drop":
        mx = t[:, L - 1]
        went = rescale(mx, accumulators=bug != "unscaled")
        pk = torch.exp2(mx - m)
        lsum = lsum + (2 * pk if bug == "double" else pk)
        o = o + pk[:, None] * vf[L - 1]
    out = (o * (1.0 / lsum)[:, None]).to(torch.bfloat16).float()
    return out[:L], went


def emulate(qkv, B, L, Hh, hd, bug=None):
    q, k, v = _split(qkv.to(torch.bfloat16).float(), B, L, Hh, hd)
    out = torch.empty(B, Hh, L, hd)
    went = []
    for b in range(B):
        for h in range(Hh):
            out[b, h], w = emulate_head(q[b, h], k[b, h], v[b, h], hd ** -0.5, bug)
            went.append(w)
    return out.transpose(1, 2).reshape(B * L, Hh * hd), went



@pytest.mark.parametrize("B,L,Hh,hd", LONE_SPIKED)
def test_bound_tells_lone_key_mistakes_apart(B, L, Hh, hd):
    """No GPU.  On the spiked inputs of test_lone_key_as_the_row_max: the emulated kernel arithmetic is inside the bound (0.2-0.4 of
    it), a dropped, double-counted or unrescaled lone key is outside it -- so the bound cannot drift into uselessness unnoticed.  Also
    checks that the spikes reach the branches they are meant to: the fold rescales for the delta-20 head and not for the delta-4 one."""
    qkv, spikes = spiked_qkv(B, L, Hh, hd, seed=L + hd)
    ref, pv = attn_ref64(qkv, B, L, Hh, hd)
    out, went = emulate(qkv, B, L, Hh, hd)
    ok = err_ratio(out, ref, pv)
    assert ok < 0.5, ok
    for (b, h, i, delta), w in zip(spikes, went):
        assert bool(w[i // 32]) == (delta > 12), (b, h, i, delta)
    for bug in ("drop", "double", "unscaled"):
        bad = err_ratio(emulate(qkv, B, L, Hh, hd, bug)[0], ref, pv)
        assert bad > 1.0, (bug, bad, ok)
