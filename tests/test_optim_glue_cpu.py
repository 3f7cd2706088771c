"""The equalities of test_gpu_optim_glue_edges.py against restatements of the kernels' arithmetic, no GPU.

As test_ln_rows_bound.py and its siblings: a check is only worth what it can tell apart.  optim.hip's adam_one, sumsq_partial /
sumsq_final and embed.hip's index maps (im2col, the patch-dropout family, the text embedding) are restated here in numpy / torch
fp32, operation by operation.  The clean restatement must meet EVERY equality of the GPU file on the GPU file's own inputs (the
case tables and generators are hipops's); the same restatement with one of the mistakes below must change at least one bit of at
least one checked output in EVERY case the mistake touches.

The update (ov_adamw_step); `touches` is decided from the case's parameters alone, never from the outcome:

    mistake          what goes wrong                                          touches
    fused_moment     b1 mu + (1 - b1) g rounded once                          lr != 0 (the moment moves by one fp32 ulp, which the stored bf16 copy absorbs:
                                                                              it shows through p) and b1 not 0 or 0.5 (there both products are exact: one
                                                                              rounding either way)
    update_bf16      the update formed from the bf16-rounded moment           lr != 0
    t_minus_1        1 - b^(t-1) for 1 - b^t                                  lr != 0 and the fp32 constants differ (not at t = 100000, where both are 1)
    no_bias_corr     bias correction omitted                                  lr != 0 and a constant is not 1
    eps_in_sqrt      sqrt(v / bc2 + eps)                                      lr != 0, eps != 0
    coupled_decay    wd p added to the gradient                               wd != 0
    decay_after      decay applied to the updated p                           wd != 0, lr != 0
    clip_no_scale    the clip's norm without grad_scale                       clipping and the factor changes (not below the clip, not at grad_scale = 1)
    clip_twice       the clip factor applied twice                            clipping with a factor != 1
    assoc            ((1 - b2) g) g                                           b2 not 0 or 0.5 (1 g and 0.5 g are exact: the same product)
    mu_trunc         mu truncated to bf16                                     every case
    mu_half_up       mu rounded half-up                                       the tie block (ties differ from nearest-even only where the kept bit is even;
                                                                              off an exact tie the two roundings agree, and random data holds no tie)
    skip_tail        the n & 3 tail left as it was                            n & 3 != 0
    skip_lap2        float4s past the first 8192 x 256 left as they were      n / 4 > 8192 x 256
    beta_double      1 - b and 1 - b^t from the double b, rounded to fp32     a beta that is no fp32 value (0.9, 0.95, 0.999)

beta_double is the KNOWN DEVIATION of the kernel's ABI from the restated optax formulas (optim.hip's header): here it
shows that the equality sees it.  The value-only mistakes (all but skip_tail and skip_lap2) change an element with a probability
below one, so they are asserted at the cases of n >= 1023 elements, where each has hundreds of elements to show on; the cases
of n <= 7 and the subnormal case (n = 37) are there for the tail path and the subnormal arithmetic, and are asserted against
skip_tail (and, the subnormal case, flushing: below).  No other mistake is waived anywhere.

The glue (embed.hip):

    mistake             what goes wrong                                        touches
    col_order           operand columns in (ii, jj, c) order                   every im2col / im2col_keep case
    px_major            patches numbered px-major                              every full im2col case
    pad_unwritten       columns >= 3 P^2 left as they were                     Kpad > 3 P^2 (P = 14)
    pos_row_div         pos row t = row / T (wrapped into the table)           T > 1 and B > 1
    pos_no_plus1        pos[keep] for pos[1 + keep]                            every assemble case
    reverse_b           dpos summed over b = B-1 .. 0                          B >= 3 (one or two terms commute)
    dropped_unwritten   rows / patches nobody kept left as they were           dpos with K < G; col2im with K < G
    px_group            col2im takes px once per four-pixel group              P = 14 ONLY: at P = 16 no group straddles a patch, asserted both ways
    narrow_int32        token ids narrowed to int32 before the range check     the bad-id cases (2^40 + 5 becomes 5)
    no_flag_eq_V        no error flag on id == V                               a case whose only bad id is V
"""
import math

import numpy as np
import pytest
import torch

import hipops as H

f32, f64 = np.float32, np.float64
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------------------
# ov_adamw_step


def bf16_np(x, mode="even"):
    """fp32 numpy -> bf16 values in fp32, by integer arithmetic on the bits: nearest-even, truncated or half-up (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    add = {"even": 0x7FFF + ((u >> 16) & 1), "trunc": 0, "half_up": 0x8000}[mode]
    return (((u + add) >> 16) << 16).astype(np.uint32).view(f32)


def adam_constants(c, t, bug=None):
    """(1 - b1, 1 - b2, bc1, bc2) in fp32: from the fp32 betas as the kernel forms them (1.0f - b; 1 - pow(b, t) in double, rounded)."""
    b1, b2 = f32(c.b1), f32(c.b2)
    tb = t - 1 if bug == "t_minus_1" else t
    if bug == "beta_double":
        k = (f32(1.0 - c.b1), f32(1.0 - c.b2), f32(1.0 - math.pow(c.b1, tb)), f32(1.0 - math.pow(c.b2, tb)))
    else:
        k = (f32(1) - b1, f32(1) - b2, f32(1.0 - math.pow(float(b1), tb)), f32(1.0 - math.pow(float(b2), tb)))
    return k[:2] + (f32(1), f32(1)) if bug == "no_bias_corr" else k


def adam_factor(c, gn_sq, bug=None):
    """The one multiplier of every gradient: grad_scale times clip / max(sqrt(gnorm_sq) grad_scale, clip)."""
    gs = f32(c.gs)
    if gn_sq is None:
        return gs
    norm = np.sqrt(f32(gn_sq)) * (f32(1) if bug == "clip_no_scale" else gs)
    fac = f32(H.CLIP_NORM) / max(norm, f32(H.CLIP_NORM))
    return gs * fac * fac if bug == "clip_twice" else gs * fac


def adam_restate(c, x, bug=None, gn_sq="case"):
    """adamw_kernel over the case's steps, every product, sum, quotient and root rounded to fp32 on its own."""
    gn_sq = H.adam_gnorm_sq(c) if isinstance(gn_sq, str) else gn_sq
    b1, b2, lr, eps, wd = f32(c.b1), f32(c.b2), f32(c.lr), f32(c.eps), f32(c.wd)
    p, mu, nu = x.p.copy(), x.mu.copy(), x.nu.copy()
    n4 = c.n // 4
    live = np.ones(c.n, dtype=bool)
    if bug == "skip_tail":
        live[4 * n4:] = False
    if bug == "skip_lap2":
        live[4 * H.LAP:4 * n4] = False
    for i, g in enumerate(x.g):
        omb1, omb2, bc1, bc2 = adam_constants(c, c.t0 + i, bug)
        s = adam_factor(c, gn_sq, bug)
        with np.errstate(all="ignore"):
            g = g * s
            if bug == "coupled_decay":
                g = g + wd * p
            if bug == "fused_moment":
                m = (f64(b1) * mu.astype(f64) + f64(omb1) * g.astype(f64)).astype(f32)
            else:
                m = b1 * mu + omb1 * g
            v = b2 * nu + ((omb2 * g) * g if bug == "assoc" else omb2 * (g * g))
            mm = bf16_np(m) if bug == "update_bf16" else m
            root = np.sqrt(v / bc2 + eps) if bug == "eps_in_sqrt" else np.sqrt(v / bc2) + eps
            u = (mm / bc1) / root
            if bug == "decay_after":
                p1 = p - lr * u
                pn = p1 - lr * (wd * p1)
            else:
                pn = p - lr * (u + wd * p)
        mn = bf16_np(m, {"mu_trunc": "trunc", "mu_half_up": "half_up"}.get(bug, "even"))
        assert pn.dtype == f32 and v.dtype == f32 and m.dtype == f32
        p, mu, nu = np.where(live, pn, p), np.where(live, mn, mu), np.where(live, v, nu)
    return H.adam_out(p, mu, nu)


def _value_only(c):
    return c.n >= H.ADAM_MIN_N


def _consts_differ(bug):
    return lambda c: any(adam_constants(c, c.t0 + i, bug) != adam_constants(c, c.t0 + i) for i in range(c.steps))


def _factor_differs(bug):
    return lambda c: c.clip != "none" and adam_factor(c, H.adam_gnorm_sq(c), bug) != adam_factor(c, H.adam_gnorm_sq(c))


ADAM_MISTAKES = {
    "fused_moment": lambda c: _value_only(c) and c.lr != 0 and c.b1 not in (0.0, 0.5),
    "update_bf16": lambda c: _value_only(c) and c.lr != 0,
    "t_minus_1": lambda c: _value_only(c) and c.lr != 0 and _consts_differ("t_minus_1")(c),
    "no_bias_corr": lambda c: _value_only(c) and c.lr != 0 and _consts_differ("no_bias_corr")(c),
    "eps_in_sqrt": lambda c: _value_only(c) and c.lr != 0 and c.eps != 0,
    "coupled_decay": lambda c: _value_only(c) and c.wd != 0,
    "decay_after": lambda c: _value_only(c) and c.wd != 0 and c.lr != 0,
    "clip_no_scale": lambda c: _value_only(c) and _factor_differs("clip_no_scale")(c),
    "clip_twice": lambda c: _value_only(c) and _factor_differs("clip_twice")(c),
    "assoc": lambda c: _value_only(c) and c.b2 not in (0.0, 0.5),
    "mu_trunc": _value_only,
    "mu_half_up": lambda c: _value_only(c) and c.ties,
    "skip_tail": lambda c: c.n & 3 != 0,
    "skip_lap2": lambda c: c.n // 4 > H.LAP,
    "beta_double": lambda c: _value_only(c) and _consts_differ("beta_double")(c),
}


@pytest.mark.parametrize("c", H.ADAM_CASES, ids=H.adam_id)
def test_adam_restatement_meets_the_oracle_and_every_mistake_shows(c):
    x = H.adam_inputs(c)
    ref = H.adam_ref(c, x)
    assert H.same_outputs(adam_restate(c, x), ref) == [], H.adam_id(c)
    if c.lr == 0:
        assert H.same_bits(ref["p"], torch.from_numpy(x.p)) and not H.same_bits(ref["nu"], torch.from_numpy(x.nu))
    if c.clip in ("below", "zero"):
        assert H.same_outputs(H.adam_ref(c, x, gn_sq=None), ref) == [], "a clip factor of exactly 1 changed a bit"
    touched = [b for b, touches in ADAM_MISTAKES.items() if touches(c)]
    print(H.adam_id(c), "mistakes asserted:", touched)
    for bug in touched:
        assert H.same_outputs(adam_restate(c, x, bug), ref) != [], (bug, H.adam_id(c))


def test_every_adam_mistake_touches_a_case_and_the_inputs_hold_what_they_should():
    for bug, touches in ADAM_MISTAKES.items():
        assert any(touches(c) for c in H.ADAM_CASES), bug
    c = next(c for c in H.ADAM_CASES if c.ties and c.n >= 256 and c.gs == 1.0)
    x = H.adam_inputs(c)
    m = (f32(0.5) * x.g[0][:256]).view(np.uint32)
    assert ((m & 0xFFFF) == 0x8000).all(), "the tie block's moments are not exact ties"
    assert set(((m >> 16) & 1).tolist()) == {0, 1}, "one parity of the kept bit only"
    c = H.ADAM_CASES[8]
    x = H.adam_inputs(c)
    g = x.g[0]
    assert (g == 0).any() and (np.abs(g) == f32(1e4)).any() and (np.abs(g) == f32(1e-20)).any() and (x.p < 0).any() and (x.p > 0).any()
    assert (x.mu != 0).all() and (x.nu[g == 0] == 0).all() and (x.nu >= 0).all()
    c = next(c for c in H.ADAM_CASES if c.tiny)
    x = H.adam_inputs(c)
    g2 = x.g[0] * x.g[0]
    tiny = np.finfo(f32).tiny
    assert (g2 > 0).all() and (g2 < tiny).all() and ((f32(1) - f32(c.b2)) * g2 > 0).all()


def test_flushed_subnormals_would_show_in_the_subnormal_case():
    """The subnormal case apart: a device that flushes g^2 to zero leaves nu = b2 nu, and the case's equality fails."""
    c = next(c for c in H.ADAM_CASES if c.tiny)
    x = H.adam_inputs(c)
    ref = H.adam_ref(c, x)
    flushed = f32(c.b2) * np.where(x.nu < np.finfo(f32).tiny, f32(0), x.nu)
    assert not H.same_bits(torch.from_numpy(flushed), ref["nu"])


def test_known_deviation_of_the_fp32_betas_in_figures():
    """What DESIGN.md and optim.hip's header state: 1 - b from the fp32 b against fl32(1 - b) from the double b, and how many elements
    of a 65 536-element group differ after three steps (restatement against restatement; nothing here is measured against optax)."""
    rel = {b: abs(float(f32(1) - f32(b)) - float(f32(1.0 - b))) / float(f32(1.0 - b)) for b in (0.9, 0.95, 0.999)}
    print("relative difference of 1 - b:", rel)
    assert 2.0e-7 < rel[0.9] < 2.4e-7 and 2.0e-7 < rel[0.95] < 2.4e-7 and 1.2e-5 < rel[0.999] < 1.4e-5
    for b2 in (0.95, 0.999):
        c = H._ac(1 << 16, steps=3, b2=b2)
        x = H.adam_inputs(c)
        clean, dev = adam_restate(c, x), adam_restate(c, x, "beta_double")
        frac = {k: float((H.bits(clean[k]) != H.bits(dev[k])).float().mean()) for k in clean}
        print(f"betas (0.9, {b2}), three steps: fraction of elements whose bits differ {frac}")
        assert frac["nu"] > 0.25 and frac["p"] > 0.05


def test_chained_groups_restated():
    """The chained case's update half: whatever scalar the two ov_sumsq calls leave, both groups meet the oracle given that scalar."""
    for n, seed in zip(H.ADAM_CHAIN, (1, 2)):
        c = H._ac(n, gs=0.5, clip="above", seed=seed)
        x = H.adam_inputs(c)
        gn_sq = f32(sum(float((H.adam_inputs(H._ac(m, seed=s)).g[0].astype(f64) ** 2).sum()) for m, s in zip(H.ADAM_CHAIN, (1, 2))))
        assert H.same_outputs(adam_restate(c, x, gn_sq=gn_sq), H.adam_ref(c, x, gn_sq=gn_sq)) == []


# ------------------------------------------------------------------------------------------------------------------------------
# ov_sumsq: sumsq_partial's per-thread fused multiply-adds, the exchange tree 32 .. 1, the four waves, then sumsq_final


def _fma(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)      # the product of two fp32 is exact in fp64


def _block_sum(acc):
    """acc [blocks, 256] fp32 -> [blocks]: wave_sum's xor tree in each wave of 64, then (red0 + red1) + (red2 + red3)."""
    w = acc.reshape(-1, 4, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., idx ^ o]
    r = w[..., 0]
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def sumsq_restate(g, prior=None, bug=None):
    n = g.size
    n4, blocks = n // 4, H.sumsq_blocks(n)
    per_lap = blocks * 256
    laps = -(-n4 // per_lap) if n4 else 0
    v = np.zeros((max(laps, 1) * per_lap, 4), dtype=f32)
    v[:n4] = g[:4 * n4].reshape(n4, 4)
    acc = np.zeros(per_lap, dtype=f32)
    for lap in range(1 if bug == "skip_lap2" else laps):
        for e in range(4):
            acc = _fma(v[lap * per_lap:(lap + 1) * per_lap, e], v[lap * per_lap:(lap + 1) * per_lap, e], acc)
    if bug != "skip_tail":
        for j in range(n & 3):
            acc[j] = _fma(g[4 * n4 + j:4 * n4 + j + 1], g[4 * n4 + j:4 * n4 + j + 1], acc[j:j + 1])[0]
    part = np.zeros(1024, dtype=f32)
    part[:blocks] = _block_sum(acc.reshape(blocks, 256))
    fin = np.zeros(256, dtype=f32)
    for k in range(4):
        fin = fin + part[256 * k:256 * (k + 1)]
    total = _block_sum(fin.reshape(1, 256))[0]
    return (f32(0) if prior is None else f32(prior)) + total


@pytest.mark.parametrize("n", H.SUMSQ_INT_N)
def test_sumsq_restated_on_integers(n):
    g, total = H.sumsq_int_case(n)
    assert total < 2 ** 24 and (np.abs(g) == 2).sum() >= min(n, 4)
    assert sumsq_restate(g).view(np.uint32) == f32(total).view(np.uint32)
    assert sumsq_restate(g, H.SUMSQ_PRIOR).view(np.uint32) == f32(total + H.SUMSQ_PRIOR).view(np.uint32)
    if n & 3:
        assert sumsq_restate(g, bug="skip_tail") != f32(total)
    if n // 4 > H.sumsq_blocks(n) * 256:
        assert sumsq_restate(g, bug="skip_lap2") != f32(total)


def test_sumsq_chain_bound_holds_for_the_restatement():
    """Case (b): the restated kernel order sits inside gam(L) sum g^2, and L counts the restatement's own roundings."""
    n = H.SUMSQ_NORMAL_N
    g = np.random.default_rng(5).standard_normal(n).astype(f32)
    exact = float((g.astype(f64) ** 2).sum())
    L = H.sumsq_chain_length(n, 0)
    assert L == 4 * 1 + 1 + 6 + 2 + 4 + 6 + 2
    q = abs(float(sumsq_restate(g)) - exact) / (H.gam(L) * exact)
    print(f"sumsq n = {n}: L = {L}, restated |err| / bound = {q:.4f}")
    assert q <= 1.0
    assert H.sumsq_chain_length(H.ADAM_LAP_N, 1) == 4 * 9 + 1 + 6 + 2 + 4 + 6 + 2 + 1


# ------------------------------------------------------------------------------------------------------------------------------
# embed.hip


def _patch_of_row(R, g, bug=None):
    pr = torch.arange(R) % (g * g)
    return (pr % g, pr // g) if bug == "px_major" else (pr // g, pr % g)          # (py, px)


def im2col_restate(img, P, Kpad, keep=None, bug=None):
    """im2col_chunk's index map per output element; keep [B, K]: the kept rows only (im2col_keep_kernel).  The output starts as NaN."""
    B, _, S, _ = img.shape
    g, PP = S // P, P * P
    if keep is None:
        R = B * g * g
        b = torch.arange(R) // (g * g)
        py, px = _patch_of_row(R, g, bug)
    else:
        K = keep.shape[1]
        b = torch.arange(B * K) // K
        idx = keep.reshape(-1).long()
        py, px = idx // g, idx % g
    k = torch.arange(3 * PP)
    if bug == "col_order":
        c, ii, jj = k % 3, k // (3 * P), (k // 3) % P
    else:
        c, ii, jj = k // PP, (k % PP) // P, k % P
    vals = img.float()[b[:, None], c[None, :], py[:, None] * P + ii[None, :], px[:, None] * P + jj[None, :]]
    out = torch.full((b.numel(), Kpad), float("nan"), dtype=BF16)
    out[:, :3 * PP] = vals.to(BF16)
    if bug != "pad_unwritten":
        out[:, 3 * PP:] = 0
    return out


@pytest.mark.parametrize("S,P,Kpad", H.IM2COL_GEOM)
def test_im2col_restated(S, P, Kpad):
    for B in (1, 3):
        for dtype in (F32, BF16):
            img = H.image_case(B, S, dtype)
            if dtype == F32:
                assert img.flatten().unique().numel() > 0.99 * img.numel()              # every pixel its own value, near enough
            ref = H.im2col_ref(img, P, Kpad)
            assert H.same_bits(im2col_restate(img, P, Kpad), ref)
            for bug in ("col_order", "px_major") + (("pad_unwritten",) if Kpad > 3 * P * P else ()):
                assert not H.same_bits(im2col_restate(img, P, Kpad, bug=bug), ref, nan_ok=True), (bug, B, dtype)


def test_im2col_restated_second_lap():
    B, S, P, Kpad = H.IM2COL_LAP
    assert B * (S // P) ** 2 * (Kpad // 8) > H.LAP
    img = H.image_case(B, S, BF16)
    assert H.same_bits(im2col_restate(img, P, Kpad), H.im2col_ref(img, P, Kpad))


@pytest.mark.parametrize("S,P,Kpad", H.KEEP_GEOM)
def test_im2col_keep_restated(S, P, Kpad):
    G = (S // P) ** 2
    for K in H.keep_ks(G):
        for dtype in (F32, BF16):
            img, keep = H.image_case(3, S, dtype), H.keep_table(3, G, K)
            ref = H.gather_keep(H.im2col_ref(img, P, Kpad), keep, G)
            assert H.same_bits(im2col_restate(img, P, Kpad, keep), ref)
            assert not H.same_bits(im2col_restate(img, P, Kpad, keep, bug="col_order"), ref)


def inverse_restate(keep, G):
    """keep_inverse_kernel: scatter, then every writer checks that its slot still names it.  -> (inv, flag)"""
    B, K = keep.shape
    inv = torch.full((B, G), -1, dtype=torch.int32)
    ok = (keep >= 0) & (keep < G)
    bad = not bool(ok.all())
    for b in range(B):
        j = torch.arange(K, dtype=torch.int32)[ok[b]]
        inv[b, keep[b][ok[b]].long()] = j
        bad = bad or not bool((inv[b, keep[b][ok[b]].long()] == j).all())
    return inv, int(bad)


@pytest.mark.parametrize("G", H.INVERSE_G)
def test_inverse_restated(G):
    for K in (1, G):
        keep = H.keep_table(3, G, K)
        inv, flag = inverse_restate(keep, G)
        assert flag == 0 and H.same_bits(inv, H.inverse_ref(keep, G))
    for wrong in (-1, G, H.INT_MAX):
        keep = H.keep_table(3, G, min(G, 4))
        keep[1, 0] = wrong
        assert inverse_restate(keep, G)[1] == 1
    if G > 1:
        keep = H.keep_table(3, G, min(G, 4))
        keep[2, 1] = keep[2, 0]
        assert inverse_restate(keep, G)[1] == 1


def assemble_restate(c, bug=None):
    x = torch.empty(c.B, 1 + c.K, c.D)
    x[:, 0] = c.cls + c.pos[0]
    x[:, 1:] = c.y.float().view(c.B, c.K, c.D) + c.pos[(0 if bug == "pos_no_plus1" else 1) + c.keep.long()]
    return x


@pytest.mark.parametrize("D", H.ASSEMBLE_D)
def test_assemble_restated(D):
    for G, K in ((4, 1), (16, 8), (16, 16)):
        c = H.assemble_case(3, G, K, D)
        assert H.same_bits(assemble_restate(c), H.assemble_ref(c))
        assert not H.same_bits(assemble_restate(c, "pos_no_plus1"), H.assemble_ref(c))


def assemble_bwd_restate(c, bug=None):
    """keep_assemble_bwd_kernel through the inverse map, image after image."""
    acc = torch.zeros(1 + c.G, c.D)
    rows = torch.arange(1 + c.G)
    seen = torch.zeros(1 + c.G, dtype=torch.bool)
    for b in (reversed(range(c.B)) if bug == "reverse_b" else range(c.B)):
        t = torch.where(rows == 0, torch.zeros_like(rows), 1 + c.inv[b].long()[(rows - 1).clamp_min(0)])
        live = (t > 0) | (rows == 0)
        acc[live] = acc[live] + c.dx[b, t[live]]
        seen |= live
    if bug == "dropped_unwritten":
        acc[~seen] = float("nan")
    return dict(dpos=acc, dcls=acc[0].clone(), dy=c.dx[:, 1:].reshape(c.B * c.K, c.D).to(BF16))


@pytest.mark.parametrize("B", H.ASSEMBLE_BWD_B)
def test_assemble_backward_restated(B):
    for G, K, D in ((16, 8, 8), (16, 16, 192), (4, 1, 1152)):
        c = H.assemble_bwd_case(B, G, K, D)
        ref = H.assemble_bwd_ref(c)
        kept = torch.zeros(1 + G, dtype=torch.bool)
        kept[0] = True
        kept[1 + c.keep.long().reshape(-1)] = True
        assert bool((H.bits(ref["dpos"])[~kept] == 0).all()), "a row nobody kept is not +0"
        assert H.same_outputs(assemble_bwd_restate(c), ref) == []
        if B >= 3:
            assert H.same_outputs(assemble_bwd_restate(c, "reverse_b"), ref) != [], (B, G, K, D)
        if not bool(kept.all()):
            assert "dpos" in H.same_outputs(assemble_bwd_restate(c, "dropped_unwritten"), ref, nan_ok=True)


def col2im_restate(c, dtype, bug=None):
    """col2im_keep_kernel's arithmetic per pixel, reading dcols through a row pitch of 3 P^2 + 8 whose gap holds NaN."""
    S, P, g = c.S, c.P, c.S // c.P
    PP = P * P
    dcols = torch.full((c.B * c.K, 3 * PP + 8), float("nan"))
    dcols[:, :3 * PP] = c.dcols.float()
    xs = torch.arange(S)
    px = ((xs // 4 * 4) if bug == "px_group" else xs) // P
    jj = xs - px * P
    py, ii = xs // P, xs % P
    j = c.inv.long()[:, py[:, None] * g + px[None, :]]                                        # [B, y, x]
    col = torch.arange(3)[:, None, None] * PP + ii[None, :, None] * P + jj[None, None, :]     # [3, y, x]
    row = torch.arange(c.B)[:, None, None] * c.K + j.clamp_min(0)
    v = dcols[row[:, None], col[None]]                                                        # [B, 3, y, x]
    v = torch.where((j >= 0)[:, None], v, torch.full_like(v, float("nan") if bug == "dropped_unwritten" else 0.0))
    return v.to(dtype)


@pytest.mark.parametrize("S,P", H.COL2IM_GEOM)
def test_col2im_restated_and_the_group_mistake_shows_at_14_only(S, P):
    G = (S // P) ** 2
    for K in (1, G):
        for dtype in (F32, BF16):
            c = H.col2im_case(3, S, P, K)
            ref = H.col2im_ref(c, dtype)
            assert H.same_bits(col2im_restate(c, dtype), ref)
            grouped = H.same_bits(col2im_restate(c, dtype, "px_group"), ref, nan_ok=True)
            assert grouped == (P % 4 == 0), (S, P, K, "px once per group: unnoticed at P = 16, seen at P = 14")
            if K < G:
                assert not H.same_bits(col2im_restate(c, dtype, "dropped_unwritten"), ref, nan_ok=True)
                patch0 = ref.view(3, 3, S // P, P, S // P, P)
                dropped = H.inverse_ref(c.keep, G).view(3, S // P, S // P) < 0
                assert bool((H.bits(patch0.permute(0, 2, 4, 1, 3, 5)[dropped]) == 0).all()), "a dropped patch is not +0"


def text_restate(c, bug=None):
    row = torch.arange(c.B * c.T)
    t = (row // c.T) % c.T if bug == "pos_row_div" else row % c.T
    ids = c.tokens.reshape(-1)
    if bug == "narrow_int32":
        ids = ids.to(torch.int32).long()
    flag = bool(((ids < 0) | ((ids > c.V) if bug == "no_flag_eq_V" else (ids >= c.V))).any())
    ids = torch.where(ids < 0, torch.zeros_like(ids), torch.where(ids >= c.V, torch.full_like(ids, c.V - 1), ids))
    return dict(x=(c.table[ids].float() + c.pos[t].float()).to(BF16), err=torch.tensor([int(flag)], dtype=torch.int32))


@pytest.mark.parametrize("B,T,D,V", H.TEXT_CASES + [H.TEXT_LAP])
def test_text_embed_restated(B, T, D, V):
    for bad in (False, True):
        if bad and B * T < 5:
            continue
        c = H.text_case(B, T, D, V, bad=bad)
        ref = H.text_ref(c)
        assert int(ref["err"]) == int(bad)
        assert H.same_outputs(text_restate(c), ref) == []
        if T > 1 and B > 1:
            assert "x" in H.same_outputs(text_restate(c, "pos_row_div"), ref)
        if bad:
            assert "x" in H.same_outputs(text_restate(c, "narrow_int32"), ref)
    if B * T >= 5:
        c = H.text_case(B, T, D, V)
        c.tokens.view(-1)[2] = V
        assert H.same_outputs(text_restate(c), H.text_ref(c)) == []
        assert H.same_outputs(text_restate(c, "no_flag_eq_V"), H.text_ref(c)) == ["err"]
        c.tokens.view(-1)[2] = 2 ** 40 + 5
        assert H.same_outputs(text_restate(c, "narrow_int32"), H.text_ref(c)) == ["err", "x"]


def test_convert_comparand_is_nearest_even_on_every_pattern():
    """ov_convert's comparand is torch's .to(): here it is held to the integer definition of nearest-even on every value of the case
    (ties, subnormals, the overflow to infinity included); NaN stays NaN."""
    v = H.convert_values(F32)
    assert v.numel() == 4 * 65536 and H.convert_values(BF16).numel() == 65536
    got = v.to(BF16)
    nan = torch.isnan(v)
    assert bool(torch.equal(torch.isnan(got), nan))
    want = torch.from_numpy(bf16_np(v[~nan].numpy())).to(BF16)
    assert H.same_bits(got[~nan], want)
    up = torch.from_numpy(bf16_np(v[~nan].numpy(), "half_up")).to(BF16)
    down = torch.from_numpy(bf16_np(v[~nan].numpy(), "trunc")).to(BF16)
    assert not H.same_bits(got[~nan], up) and not H.same_bits(got[~nan], down)
    assert H.same_bits(H.convert_values(BF16).float().to(BF16), H.convert_values(BF16), nan_ok=True)
    for cols in H.CONVERT_COLS:
        assert H.convert_rows(cols, F32) * cols >= v.numel()
    assert H.CONVERT_LAP[0] * H.CONVERT_LAP[1] > H.LAP
