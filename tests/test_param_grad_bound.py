"""The bounds of test_gpu_param_grad_edges.py (hipops.linear_bounds, ln_grads_ref64, gelu_bounds) against emulations of the kernels'
arithmetic, no GPU.

As test_attention_bwd_bound.py does for the attention backward: a bound is only worth what it can tell apart.  The linear, LayerNorm
and GELU backward of backward.hip are computed here in torch fp32 the way the kernels compute them -- dW as bf16 partials per row
range, an fp32 sum and one rounding; two-pass row statistics and the kernel's dx formula; the A&S 7.1.26 and sigmoid forms of gelu' --
and must sit inside the bound on every element of every output, whatever the row ranges are (the bound knows no plan: chunk = 64, a
third of M and all of M are each emulated).  The same emulation with one of the mistakes below must land at >= 4 x the bound on at
least one element of every output the mistake touches.

    mistake            what goes wrong                                                              leaves the bound on
    drop_last          row M - 1 is missing from its range                                          dW, db
    double_first       the first row of the second range is counted twice                           dW, db
    skip_partial       the last range's partial is left out of the sum of the partials              dW
    dx_short           the dX contraction stops 8 columns short of N                                dX
    mean_tail          the last 8-column chunk of D is missing from the mean                        LN dx, dgamma
    mqx_tail           the same chunk is missing from mean(q xhat)                                  LN dx
    no_dres            dres is not added                                                            LN dx
    drop_last_row      the last row is missing from the parameter sums                              dgamma, dbeta
    overwrite          a wave's second row overwrites its sums instead of adding (rows > 4096)      dgamma, dbeta
    split_early        dgamma | dbeta split one column early (n_lo = D - 1)                         dgamma, dbeta
    phi_flip           erf form: Phi(-a) in place of Phi(a) for a < 0                               da, h at a in [-6, -3]
    no_cubic           tanh form: u' without its 3 * 0.044715 a^2 term                              da
"""
import pytest
import torch

import hipops as H
from hipops import DELTA_ERF, DELTA_TANH, GELU_DH, LINEAR_NK, LINEAR_TN_M, LINEAR_TR_M, LN_SHAPES

MIN_RATIO = 4.0                  # every mistake must land at least this far outside
bf = lambda t: t.to(torch.bfloat16).float()
pad64 = lambda v: (v + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------------------------------------
# linear backward


def emulate_linear(dy, x, w, chunk, bug=None):
    """(dX, dW, db) as fp32 tensors holding what the kernels would store; dW over row ranges of `chunk` rows (a multiple of 64)."""
    dy, x, w = dy.float(), x.float(), w.float()
    M, N = dy.shape
    nz = (M + chunk - 1) // chunk
    dX = bf(dy[:, :N - 8] @ w[:N - 8]) if bug == "dx_short" else bf(dy @ w)
    acc, db = torch.zeros(N, x.shape[1]), torch.zeros(N)
    for z in range(nz):
        lo, hi = z * chunk, min(M, (z + 1) * chunk)
        d, xx = dy[lo:hi].clone(), x[lo:hi]
        if bug == "drop_last" and hi == M:
            d[M - 1 - lo] = 0.0
        if bug == "double_first" and z == 1:
            d[0] *= 2.0
        p = d.T @ xx
        if not (bug == "skip_partial" and z == nz - 1):
            acc += bf(p) if nz > 1 else p
        db += d.sum(0)
    return dX, bf(acc), db


def linear_ratios(got, ref, bounds):
    return tuple(float(((g.double() - r).abs() / b).max()) for g, r, b in zip(got, ref, bounds))


@pytest.mark.parametrize("M", LINEAR_TN_M + LINEAR_TR_M)
def test_linear_bounds_hold_for_every_plan(M):
    """The clean emulation at every shape of the GPU file, with one range per tile, three ranges and one range."""
    for N, K in LINEAR_NK:
        dy, x, w = H.spiked_linear_case(M, N, K, seed=M + N)
        ref, bounds = H.linear_grads_ref64(dy, x, w), H.linear_bounds(dy, x, w)
        for chunk in sorted({64, pad64((M + 2) // 3), pad64(M)}):
            r = linear_ratios(emulate_linear(dy, x, w, chunk), ref, bounds)
            print(f"linear bound M={M} N={N} K={K} chunk={chunk}: clean dX {r[0]:.3f} dW {r[1]:.3f} db {r[2]:.3f}")
            assert max(r) <= 1.0, (M, N, K, chunk, r)


# (M, chunk): the ragged three-range plan of the towers' smallest M, one range per tile (the second range starts at the spiked row
# 64), and two plans whose last range ends in zero rows (M % 64 != 0)
LINEAR_BUG_PLANS = [(1088, 384), (1088, 64), (1100, 384), (2200, 448), (4160, 512)]
LINEAR_BUGS = {"drop_last": (1, 2), "skip_partial": (1,), "dx_short": (0,)}


@pytest.mark.parametrize("M,chunk", LINEAR_BUG_PLANS)
def test_linear_bounds_tell_mistakes_apart(M, chunk):
    names = ("dX", "dW", "db")
    for N, K in LINEAR_NK:
        dy, x, w = H.spiked_linear_case(M, N, K, seed=M + K)
        ref, bounds = H.linear_grads_ref64(dy, x, w), H.linear_bounds(dy, x, w)
        bugs = dict(LINEAR_BUGS)
        if chunk == 64:
            bugs["double_first"] = (1, 2)         # the second range then starts at a spiked row; an unspiked row of dW shows at 2-9 x only
        for bug, touched in bugs.items():
            r = linear_ratios(emulate_linear(dy, x, w, chunk, bug), ref, bounds)
            print(f"linear bound M={M} N={N} K={K} chunk={chunk} {bug}: " + " ".join(f"{names[j]} {r[j]:.1f}" for j in touched))
            for j in touched:
                assert r[j] >= MIN_RATIO, (bug, names[j], r)


def test_db_bound_sees_a_dropped_row_at_large_m():
    """The db-alone case of the GPU file, M = 33027: bound_db grows like M^2 and is 52 per column there, so an 8-fold spike on the
    last row would hide inside it; with the 512-fold spike of that case a db without row M - 1 is >= 4 x outside, and the clean
    fp32 sum (256-row chunks, then the chunk sums) far inside."""
    M, N, K = 33027, 64, 64
    dy, x, w = H.spiked_linear_case(M, N, K, seed=M, boost=H.DB_BOOST_LARGE_M)
    ref, bound = H.linear_grads_ref64(dy, x, w)[2], H.linear_bounds(dy, x, w)[2]
    chunks = lambda d: torch.stack([d[i:i + 256].sum(0) for i in range(0, d.shape[0], 256)]).sum(0)
    clean = float(((chunks(dy.float()).double() - ref).abs() / bound).max())
    bad = float(((chunks(dy.float()[:M - 1]).double() - ref).abs() / bound).max())
    print(f"linear bound db alone M={M}: bound {float(bound.min()):.1f}..{float(bound.max()):.1f}, clean {clean:.4f}, row M - 1 dropped {bad:.1f}")
    assert clean <= 1.0 and bad >= MIN_RATIO, (clean, bad)


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward


def emulate_ln(x, gamma, dy, dres, eps=1e-6, bug=None):
    """(dx, dgamma, dbeta) fp32 as layernorm_bwd_rows + rows_sum compute them: two-pass statistics, xhat = (x - mean) rstd,
    q = dy gamma, dx = bf16(rstd (q - mean q - xhat mean(q xhat)) + dres)."""
    x, dy, g = x.float(), dy.float(), gamma.float()
    R, D = x.shape
    inv = torch.tensor(1.0 / D)
    mean = (x[:, :D - 8] if bug == "mean_tail" else x).sum(1, keepdim=True) * inv
    xc = x - mean
    rstd = ((xc * xc).sum(1, keepdim=True) * inv + eps).rsqrt()
    xh = xc * rstd
    q = dy * g
    mq = q.sum(1, keepdim=True) * inv
    qx = q * xh
    mqx = (qx[:, :D - 8] if bug == "mqx_tail" else qx).sum(1, keepdim=True) * inv
    dx = rstd * (q - mq - xh * mqx)
    if dres is not None and bug != "no_dres":
        dx = dx + dres.float()
    t, d = dy * xh, dy
    if bug == "drop_last_row":
        t, d = t[:-1], d[:-1]
    if bug == "overwrite":                        # 4096 waves: rows 4096.. are second rows, of waves 0..; their first rows are lost
        assert R > 4096
        t, d = t[R - 4096:], d[R - 4096:]
    dg, db = t.sum(0), d.sum(0)
    if bug == "split_early":                      # column D - 1 of the partial rows goes to dbeta[0]; dgamma[D - 1] is never written
        both = torch.cat([dg, db])
        dg, db = torch.cat([both[:D - 1], torch.zeros(1)]), both[D - 1:2 * D - 1]
    return bf(dx), dg, db


@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_ln_bounds_hold(rows, D):
    for dres_on, mean in ((True, 0.2), (False, 0.2), (True, 8.0)):
        x, gamma, dy, dres = H.spiked_ln_case(rows, D, seed=rows + D, mean=mean)
        dres = dres if dres_on else None
        r = H.ln_err_ratio(*emulate_ln(x, gamma, dy, dres), H.ln_grads_ref64(x, gamma, dy, dres, 1e-6))
        print(f"LN bound rows={rows} D={D} dres={dres_on} mean={mean}: clean dx {r[0]:.3f} dgamma {r[1]:.3f} dbeta {r[2]:.3f}")
        assert max(r) <= 1.0, (rows, D, dres_on, mean, r)


LN_BUG_CASES = [
    # (rows, D, mean, {bug: outputs it must leave the bound on (0 dx, 1 dgamma, 2 dbeta)})
    (9, 1152, 0.2, {"mean_tail": (0, 1), "mqx_tail": (0,), "no_dres": (0,), "drop_last_row": (1, 2), "split_early": (1, 2)}),
    (37, 520, 0.2, {"mean_tail": (0, 1), "mqx_tail": (0,), "no_dres": (0,), "drop_last_row": (1, 2), "split_early": (1, 2)}),
    (9, 1152, 8.0, {"mean_tail": (0, 1), "mqx_tail": (0,), "no_dres": (0,), "drop_last_row": (1, 2)}),
    (129, 200, 0.2, {"drop_last_row": (1, 2), "split_early": (1, 2)}),
    (4099, 64, 0.2, {"overwrite": (1, 2), "drop_last_row": (1, 2), "split_early": (1, 2), "no_dres": (0,)}),
]


@pytest.mark.parametrize("rows,D,mean,bugs", LN_BUG_CASES)
def test_ln_bounds_tell_mistakes_apart(rows, D, mean, bugs):
    names = ("dx", "dgamma", "dbeta")
    x, gamma, dy, dres = H.spiked_ln_case(rows, D, seed=rows + D + 100, mean=mean)     # (at seed rows + D, dgamma[D - 1] of (9, 1152)
    ref = H.ln_grads_ref64(x, gamma, dy, dres, 1e-6)                                   # cancels to 0.06: nothing for split_early to lose)
    for bug, touched in bugs.items():
        r = H.ln_err_ratio(*emulate_ln(x, gamma, dy, dres, bug=bug), ref)
        print(f"LN bound rows={rows} D={D} mean={mean} {bug}: " + " ".join(f"{names[j]} {r[j]:.1f}" for j in touched))
        for j in touched:
            assert r[j] >= MIN_RATIO, (bug, names[j], r)


# ------------------------------------------------------------------------------------------------------------------------------
# GELU backward


def gelu_formula32(a, tanh, bug=None):
    """(gelu'(a), Phi resp. sigmoid) in fp32, operation for operation gelu_erf_both / gelu_tanh_both (torch's correctly rounded
    reciprocal and exp2 in place of the one-ulp v_rcp / v_exp)."""
    a = a.float()
    if tanh:
        a2 = a * a
        u = 0.7978845608028654 * a * (0.044715 * a2 + 1.0)
        sg = 1.0 / (1.0 + torch.exp2(-2.8853900817779268 * u))
        du = 0.7978845608028654 * ((0.0 if bug == "no_cubic" else 3.0 * 0.044715) * a2 + 1.0)
        return 2.0 * a * sg * (1.0 - sg) * du + sg, sg
    z = a.abs() * 0.70710678118654752440
    t = 1.0 / (0.3275911 * z + 1.0)
    p = t * 1.061405429 + -1.453152027
    p = t * p + 1.421413741
    p = t * p + -0.284496736
    p = t * p + 0.254829592
    p = p * t
    ex = torch.exp2(-1.4426950408889634 * z * z)
    he = 0.5 * p * ex
    phi = 1.0 - he if bug == "phi_flip" else torch.where(a >= 0, 1.0 - he, he)
    return a * 0.3989422804014327 * ex + phi, phi


def emulate_gelu(a, dh, tanh, bug=None):
    grad, s = gelu_formula32(a, tanh, bug)
    return bf(dh.float() * grad), bf(a.float() * s)


def gelu_cases():
    a_all, dh_all = H.gelu_all_values_case()
    yield "all values", a_all, dh_all
    for rows, N in ((3, 8), (300, 1544)):
        yield f"({rows}, {N})", (H.rnd(rows, N, seed=rows + N) * 2.0).to(torch.bfloat16), H.rnd(rows, N, seed=rows + N + 1).to(torch.bfloat16)


@pytest.mark.parametrize("tanh", [False, True])
def test_gelu_bounds_hold_and_tell_mistakes_apart(tanh):
    form = "tanh" if tanh else "erf"
    for tag, a, dh in gelu_cases():
        r = H.gelu_err_ratio(*emulate_gelu(a, dh, tanh), a, dh, tanh)
        print(f"GELU bound {form} {tag}: clean da {r[0]:.3f} h {r[1]:.3f}")
        assert max(r) <= 1.0, (form, tag, r)
    a, dh = H.gelu_all_values_case()
    if tanh:
        r = H.gelu_err_ratio(*emulate_gelu(a, dh, True, "no_cubic"), a, dh, True)
        print(f"GELU bound tanh no_cubic: da {r[0]:.1f}")
        assert r[0] >= MIN_RATIO, r
    else:
        tail = ((a.float() >= -6.0) & (a.float() <= -3.0)).any(1)          # whole 8-wide rows of the value table
        a, dh = a[tail], dh[tail]
        keep = (a.float() >= -6.0) & (a.float() <= -3.0)
        da, h = emulate_gelu(a, dh, False, "phi_flip")
        rda, rh = H.gelu_grads_ref64(a, dh, False)
        bda, bh = H.gelu_bounds(a, dh, False)
        qa = ((da.double() - rda).abs() / bda)[keep]
        qh = ((h.double() - rh).abs() / bh)[keep]
        print(f"GELU bound erf phi_flip, a in [-6, -3]: da min {float(qa.min()):.1f} max {float(qa.max()):.1f}; h min {float(qh.min()):.1f}"
              f" max {float(qh.max()):.1f}")
        assert float(qa.min()) >= MIN_RATIO and float(qh.min()) >= MIN_RATIO          # on EVERY element of the tail, not just one


# a band of the tanh form in which the fp32 derivative is further than DELTA_TANH from the truth (hipops: 1 - sg cancels)
TANH_BAND = (2.6, 5.3)


def test_gelu_delta_against_the_fp32_formulas():
    """The fp32 formulas against fp64 at every bf16 value up to 2^16: Phi, the sigmoid and the erf-form derivative stay inside their
    delta everywhere; the tanh-form derivative does outside TANH_BAND, and what it reaches inside is printed."""
    a = H.all_bf16_values()
    one = torch.ones_like(a)
    for tanh, delta in ((False, DELTA_ERF), (True, DELTA_TANH)):
        g64, h64 = H.gelu_grads_ref64(a, one, tanh)
        g32, s32 = gelu_formula32(a, tanh)
        assert not bool(torch.isnan(g32).any())
        eg = (g32.double() - g64).abs()
        nz = a.float() != 0
        es = ((s32.double() * a.double() - h64).abs() / a.double().abs())[nz]       # |a| |s err| / |a|
        inside = (a.float() > TANH_BAND[0]) & (a.float() < TANH_BAND[1]) if tanh else torch.zeros_like(nz)
        print(f"gelu {'tanh' if tanh else 'erf'}: max |gelu' err| {float(eg[~inside].max()):.3e} (delta {delta:.3e}), Phi / sigmoid "
              f"{float(es.max()):.3e}" + (f", in the band {TANH_BAND}: {float(eg[inside].max()):.3e}" if tanh else ""))
        assert float(eg[~inside].max()) <= delta and float(es.max()) <= delta
