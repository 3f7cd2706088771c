"""The bounds of test_gpu_gemm_small_routes.py (hipops.linear_ratios, fold_bound) against an emulation of the GEMM kernels' shared
epilogue arithmetic, no GPU.

As test_param_grad_bound.py does for the backward kernels: a bound is only worth what it can tell apart.  The epilogues of gemm.hip
(gemm_epilogue and its restatement in the skinny kernel; common.h: epi_combine and the GELU forms) are computed here in torch fp32 the
way the kernels compute them -- the product K-tile by K-tile in fp32, bias or the two fused multiply-adds of the LN fold, the
polynomial / closed-form GELUs, one bf16 rounding, then the second operand (residual: a second rounding; GELU gradient:
bf16(bf16(acc + bias) gelu'(R))) and the row maps' index arithmetic -- and must sit inside the bound on EVERY element at every shape
the GPU file runs.  The same emulation with one of the mistakes below must land at >= 4 x the bound, on an element the mistake
touches (every other element is the clean emulation's and inside).

    mistake            what goes wrong                                                           looked for on
    stats_neighbour    the last row folds with row M - 2's {mean, rstd}                          the last row
    colsum_quad        the last quad of columns folds with the quad before's colsum              the last 4 columns
    k_short            the product stops 8 columns short of K                                    every element
    rstd_on_cvec       rstd (t + cvec)                                                           every element
    no_cvec            rstd t                                                                    every element
    sub_after          rstd acc - mean colsum + cvec                                             every element
    acc_bf16           acc rounded to bf16 before the fold                                       every element
    t_bf16             t rounded to bf16 before the multiplication by rstd                       every element
    ring_stale         K-tile 4 read from the ring slot's previous occupant, K-tile 0 (K = 320)  every element
    bias_quad          the last quad of columns gets the quad before's bias (N % 16 == 8)        the last 4 columns
    resid_next_row     the last valid row adds R[M] instead of R[M - 1]                          the last row
    resid_off          the row-mapped residual ignores resid_off                                 the patch rows
    grad_row           gelu' evaluated at row m + 1 of R                                         every element

The fold mistakes run at the fold's GPU shapes, K <= 320; at K = 1024 the K S1 term of the bound admits the two double-rounding
mistakes (acc_bf16, t_bf16) at 2.8 x and 1.6 x only, so that shape runs for the clean bound alone (hipops.FOLD_CLEAN_ONLY)."""
import pytest
import torch

import hipops as H

MIN_RATIO = 4.0                  # every mistake must land at least this far outside (test_param_grad_bound.py)
F32 = torch.float32
bf = lambda t: t.to(torch.bfloat16).float()
c32 = lambda v: torch.tensor(v, dtype=F32)


def fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in fp64, one rounding of the sum."""
    return (a.double() * b.double() + c.double()).float()


def _horner(xc, coef):
    u = xc * xc
    q = fma(u, c32(coef[0]), c32(coef[1]))
    for c in coef[2:]:
        q = fma(q, u, c32(c))
    return fma(xc, q, c32(0.5))


ERF_COEF = (-1.832668545e-09, 1.370619420e-07, -4.476110938e-06, 8.535522916e-05, -1.079715229e-03, 9.774306659e-03, -6.634450104e-02,
            3.989241898e-01)
ERF_GRAD_COEF = (-1.933266631e-08, 1.391892320e-06, -4.282898866e-05, 7.424731401e-04, -8.057965438e-03, 5.721020480e-02,
                 -2.640489873e-01, 7.976477333e-01)
C0, C1 = 0.7978845608028654, 0.044715


def _sigmoid2u(x, x2_inside):
    """sg = 1 / (1 + exp2(-2 log2(e) u)), u = sqrt(2 / pi) x (1 + 0.044715 x^2), operation for operation gelu_tanh_f2 (x2_inside: the
    cubic term as fma(0.044715 x, x, 1)) or gelu_tanh_grad_f2 (fma(x^2, 0.044715, 1)); torch's correctly rounded exp2 and reciprocal
    in place of the one-ulp v_exp / v_rcp."""
    cub = fma(x * c32(C1), x, c32(1.0)) if x2_inside else fma(x * x, c32(C1), c32(1.0))
    u = x * c32(C0) * cub
    return 1.0 / (torch.exp2(u * c32(-2.8853900817779268)) + 1.0)


def gelu32(x, tanh):
    """gelu_erf_f2 / gelu_tanh_f2 (common.h) in torch fp32."""
    if tanh:
        return x * _sigmoid2u(x, True)
    return x * _horner(x.clamp(-4.0, 4.0), ERF_COEF)


def gelu_grad32(x, tanh):
    """gelu_erf_grad_f2x2 / gelu_tanh_grad_f2 (common.h) in torch fp32."""
    if not tanh:
        return _horner(x.clamp(-4.0, 4.0), ERF_GRAD_COEF)
    sg = _sigmoid2u(x, False)
    du = fma(x * x, c32(3.0) * c32(C1) * c32(C0), c32(C0))
    return fma(x * 2.0 * sg * (1.0 - sg), du, sg)


def product(a, w, bug=None):
    """a w^T in fp32, K-tile (64) by K-tile as the kernels accumulate it."""
    a, w = a.float(), w.float()
    nt = a.shape[1] // 64
    acc = torch.zeros(a.shape[0], w.shape[0])
    for t in range(nt):
        s = t - 4 if bug == "ring_stale" and t >= 4 else t
        at, wt = a[:, 64 * s:64 * s + 64], w[:, 64 * s:64 * s + 64]
        if bug == "k_short" and t == nt - 1:
            at = at.clone()
            at[:, 56:] = 0.0
        acc += at @ wt.T
    return acc


def emulate(a, w, bias, epi, r=None, fold=None, maps=(0, 0, 0), out_rows=None, bug=None):
    """What ov_gemm / ov_gemm_ln would store, as fp32 [out_rows or M, N] over the sentinel.  fold: (colsum, stats) -- bias is then
    cvec; maps: (out_group, resid_mod, resid_off); r: the second operand of epilogues 3-5."""
    acc = product(a, w, bug)
    M, N = acc.shape
    b = bias.float().clone() if bias is not None else torch.zeros(N)
    if bug == "bias_quad":
        b[N - 4:] = b[N - 8:N - 4]
    if fold is not None:
        colsum, stats = fold
        cs, mean, rstd = colsum.float()[None, :].clone(), stats[:, 0:1].clone(), stats[:, 1:2].clone()
        if bug == "stats_neighbour":
            mean[M - 1], rstd[M - 1] = mean[M - 2], rstd[M - 2]
        if bug == "colsum_quad":
            cs[:, N - 4:] = cs[:, N - 8:N - 4]
        if bug == "acc_bf16":
            acc = bf(acc)
        if bug == "sub_after":
            v = fma(cs, -mean, acc * rstd) + b
        else:
            t = fma(cs, -mean, acc)
            if bug == "t_bf16":
                t = bf(t)
            v = (t + b) * rstd if bug == "rstd_on_cvec" else t * rstd if bug == "no_cvec" else fma(t, rstd, b)
    else:
        v = acc + b
    if epi in (1, 2):
        v = gelu32(v, epi == 2)
    o = bf(v)
    rows = torch.arange(M)
    group, mod, off = maps
    if epi >= 3:
        rrow = rows % mod + (0 if bug == "resid_off" else off) if mod else rows.clone()
        if bug == "resid_next_row":
            rrow[M - 1] += 1
        if bug == "grad_row":
            rrow = (rrow + 1) % M
        rv = r.float()[rrow]
        o = bf(o + rv) if epi == 3 else bf(o * gelu_grad32(rv, epi == 5))
    out = torch.full((out_rows or M, N), H.SENT)
    out[rows + rows // group + 1 if group else rows] = o
    return out


KIND = {0: "pre", 1: "erf", 2: "tanh", 3: "res", 4: "gerf", 5: "gtanh"}
NAME = {0: "bias", 1: "gelu erf", 2: "gelu tanh", 3: "residual", 4: "gelu' erf", 5: "gelu' tanh"}


def linear_case_ratios(shape, epis, null_bias=False, bug=None):
    M, N, K = shape
    a, w, bias, r = H.gemm_case(M, N, K, r_rows=M + 1)
    outs = {NAME[e]: (emulate(a, w, None if null_bias else bias, e, r, bug=bug), KIND[e]) for e in epis}
    return H.linear_ratios(a, w, torch.zeros(N) if null_bias else bias, outs, r[:M])


def rowmap_case_ratios(bug=None):
    """The row-mapped launches of the GPU file: out_group = resid_mod = g^2, resid_off = 1; the patch rows against fp64 through views
    that restate no index arithmetic."""
    B, g2, D, K = H.ROWMAP_CASE
    a, w, bias, pos = H.gemm_case(B * g2, D, K, r_rows=g2 + 1)
    res = {}
    for epi in (0, 3):
        out = emulate(a, w, bias, epi, pos, maps=(g2, g2 if epi else 0, 1 if epi else 0), out_rows=B * (g2 + 1), bug=bug)
        assert bool((out.view(B, g2 + 1, D)[:, 0] == H.SENT).all())
        res.update(H.linear_ratios(a, w, bias, {NAME[epi]: (H.patch_rows(out, B, g2), KIND[epi])}, pos[1:].repeat(B, 1)))
    return res


def worst(res):
    return max(q for q, _, _ in res.values())


@pytest.mark.parametrize("shape", H.SKINNY_SHAPES + H.PLAIN_SHAPES + H.ROWPARTS_SHAPES + [H.MAPPED_GELU_CASE[:3], H.BATCHED_CASE[:3]])
def test_clean_epilogues_are_inside_the_bound(shape):
    """Every epilogue the GPU file runs at this shape (all six where it runs all six; a superset elsewhere costs nothing here)."""
    epis = (0, 1, 2, 3, 4, 5) if shape in H.SKINNY_ALL_EPI + H.PLAIN_ALL_EPI else (0, 1, 3)
    res = linear_case_ratios(shape, epis)
    res.update({k + ", no bias": v for k, v in linear_case_ratios(shape, (0,), null_bias=True).items()})
    for name, (q, row, col) in res.items():
        print(f"small bound {shape} {name}: clean {q:.3f}")
    assert worst(res) <= 1.0, res


def test_clean_row_maps_are_inside_the_bound():
    res = rowmap_case_ratios()
    print(f"small bound row maps {H.ROWMAP_CASE}: " + " ".join(f"{n} {q:.3f}" for n, (q, _, _) in res.items()))
    assert worst(res) <= 1.0, res
    M, N, K, group = H.MAPPED_GELU_CASE
    a, w, bias, _ = H.gemm_case(M, N, K, r_rows=1)
    out = emulate(a, w, bias, 1, maps=(group, 0, 0), out_rows=M + M // group)
    res = H.linear_ratios(a, w, bias, {"gelu erf": (H.patch_rows(out, M // group, group), "erf")})
    print(f"small bound out_group {H.MAPPED_GELU_CASE}: gelu erf {worst(res):.3f}")
    assert worst(res) <= 1.0, res


LINEAR_BUGS = [
    # bug, shape, epilogues, where the worst element must lie: (M, N) -> (row predicate, column predicate)
    ("ring_stale", (63, 1096, 320), (0,), None),
    ("bias_quad", (130, 200, 192), (0,), lambda M, N, row, col: col >= N - 4),
    ("resid_next_row", (130, 200, 192), (3,), lambda M, N, row, col: row == M - 1),
    ("grad_row", (130, 200, 192), (4, 5), None),
]


@pytest.mark.parametrize("bug,shape,epis,where", LINEAR_BUGS)
def test_bounds_tell_linear_mistakes_apart(bug, shape, epis, where):
    res = linear_case_ratios(shape, epis, bug=bug)
    for name, (q, row, col) in res.items():
        print(f"small bound {shape} {name} {bug}: {q:.1f} at ({row}, {col})")
        assert q >= MIN_RATIO, (bug, name, q)
        assert where is None or where(shape[0], shape[1], row, col), (bug, name, row, col)


def test_bounds_tell_an_ignored_resid_off_apart():
    res = rowmap_case_ratios(bug="resid_off")
    print(f"small bound row maps resid_off: residual {res['residual'][0]:.1f}")
    assert res["residual"][0] >= MIN_RATIO and res["bias"][0] <= 1.0, res


# ------------------------------------------------------------------------------------------------------------------------------
# the LN fold

FOLD_NAME = {0: "fold bias", 1: "fold gelu erf", 2: "fold gelu tanh"}
FOLD_BUGS = {
    "stats_neighbour": lambda M, N, row, col: row == M - 1,
    "colsum_quad": lambda M, N, row, col: col >= N - 4,
    "k_short": None, "rstd_on_cvec": None, "no_cvec": None, "sub_after": None, "acc_bf16": None, "t_bf16": None,
}


def fold_ratio(out, ref, bound):
    q = (out.double() - ref).abs() / bound
    k = int(q.argmax())
    return float(q.view(-1)[k]), k // q.shape[1], k % q.shape[1]


@pytest.mark.parametrize("shape", H.FOLD_SHAPES + [H.FOLD_CLEAN_ONLY])
def test_clean_fold_is_inside_the_bound(shape):
    x, wg, cvec, colsum = H.spiked_fold_case(*shape)[:4]
    st = H.stats64(x)
    for epi in (0, 1, 2):
        q, row, col = fold_ratio(emulate(x, wg, cvec, epi, fold=(colsum, st)), *H.fold_bound(x, wg, colsum, cvec, st, epi))
        print(f"fold bound {shape} {FOLD_NAME[epi]}: clean {q:.3f} at ({row}, {col})")
        assert q <= 1.0, (shape, epi, q, row, col)


@pytest.mark.parametrize("shape", H.FOLD_SHAPES)
def test_fold_bound_tells_mistakes_apart(shape):
    """On the bias epilogue, where nothing but the fold stands between the product and the output."""
    M, N, K = shape
    assert K <= 320
    x, wg, cvec, colsum = H.spiked_fold_case(M, N, K)[:4]
    st = H.stats64(x)
    ref, bound = H.fold_bound(x, wg, colsum, cvec, st)
    for bug, where in FOLD_BUGS.items():
        q, row, col = fold_ratio(emulate(x, wg, cvec, 0, fold=(colsum, st), bug=bug), ref, bound)
        print(f"fold bound {shape} {bug}: {q:.1f} at ({row}, {col})")
        assert q >= MIN_RATIO, (shape, bug, q)
        assert where is None or where(M, N, row, col), (shape, bug, row, col)


# ------------------------------------------------------------------------------------------------------------------------------
# delta of the GELU-gradient epilogues


def test_gelu_grad_delta_against_the_fp32_forms():
    """The fp32 restatements of gelu_erf_grad_f2x2 / gelu_tanh_grad_f2 against the exact fp64 derivative on the 2^-12 grid over
    [-8, 8]: the erf form inside the figure common.h states, the tanh form (no stated figure) inside half of DELTA_GRAD_TANH, which is
    twice the grid maximum; and at every finite bf16 value up to 2^16 -- what R can hold -- both inside their delta."""
    grid = torch.arange(-8 * 4096, 8 * 4096 + 1, dtype=torch.float64) / 4096
    vals = H.all_bf16_values().double()
    for tanh, delta, on_grid in ((False, H.DELTA_GRAD_ERF, 1.0), (True, H.DELTA_GRAD_TANH, 0.5)):
        worst_ = []
        for x in (grid, vals):
            err = (gelu_grad32(x.float(), tanh).double() - H.gelu_grads_ref64(x, torch.ones_like(x), tanh)[0]).abs()
            k = int(err.argmax())
            worst_.append((float(err[k]), float(x[k])))
        print(f"gelu' {'tanh' if tanh else 'erf'}: grid max {worst_[0][0]:.3e} at {worst_[0][1]:.4f}, bf16 values max {worst_[1][0]:.3e} at "
              f"{worst_[1][1]:.4f} (delta {delta:.3e})")
        assert worst_[0][0] <= on_grid * delta and worst_[1][0] <= delta, (tanh, worst_)
