"""The bounds of test_gpu_ln_rows_edges.py (hipops.row_stats_ref64, ln_ref64, parts_ref64, mean_pool_ref64, l2norm_ref64, fold_bound's
stat_err) against emulations of the row kernels' arithmetic, no GPU.

As test_param_grad_bound.py and test_gemm_small_bound.py: a bound is only worth what it can tell apart.  layernorm_rows /
rowstats_rows (per-lane sums over the lane's 16-byte chunks c = 0, 1, ..., then the xor tree 32 .. 1; two passes), rowparts_kernel
(stat_octet's fixed tree over a 32-column group), rowstats_finalize_kernel (eight lanes, groups k, k + 8, ..., the xor tree 1, 2, 4;
var = Q / D - mean^2 clamped at 0), mean_pool_kernel (four token-strided waves, summed in wave order) and l2norm_kernel (lanes
striding by 64, the xor tree) are computed here in torch fp32 in the kernels' order.  The order serves the emulation only: the bounds
know nothing of it.  The clean emulation must sit inside every bound on EVERY element at every shape the GPU file runs; the same
emulation with one of the mistakes below must land at >= 4 x the bound on an element the mistake touches.

    mistake        what goes wrong                                                        looked for on
    sum_tail       the last 8-column chunk missing from the sum                           LayerNorm output; rowstats mean
    sq_tail        the last chunk missing from the sum of squares only                    LayerNorm output; rowstats rstd
    gb_prev        chunk c >= 1 of a lane reads chunk c - 1's gamma / beta                output columns >= 512 (D > 512)
    dm1            D - 1 for D                                                            output; rowstats (D <= 1152, see below)
    no_eps         rsqrt(var)                                                             the constant row
    eps_after      rsqrt(var) + eps                                                       the constant row
    beta_tail      beta dropped in the last chunk                                         the last 8 columns
    via_bf16       an fp32 output written through bf16                                    fp32 outputs
    g_ge_8         finalize ignores the groups g >= 8                                     G > 8
    no_clamp       finalize without the clamp at 0                                        the nearly constant row
    q_neighbour    finalize takes the row before's Q                                      rows >= 2
    div_L          the pool divides by L                                                  first = 1
    with_cls       the pool's waves start at token 0                                      first = 1
    wave3          the pool misses the tokens t = first + 3 (mod 4)                       L - first >= 4
    l2_tail        l2norm misses the lanes' last, partial trip                            E % 64 != 0
    l2_no_clamp    l2norm without the 1e-12 clamp                                         the zero row and the 1e-20 row

dm1 moves the mean by |mean| / D and the variance by var / D, against bounds that grow like D e: the ratio cannot exceed
1 / (D^2 e) whatever the data, 4.0 at D = 2048 and 0.25 at D = 8192.  No order-blind bound sees it from D = 2048 on; it is asserted up
to D = 1152 (five shapes) and printed at the others.  Every other mistake is asserted at every shape it touches."""
import pytest
import torch

import hipops as H

MIN_RATIO = 4.0                  # every mistake must land at least this far outside (test_param_grad_bound.py)
EPS = 1e-6
F32 = torch.float32
bf = lambda t: t.to(torch.bfloat16).float()
c32 = lambda v: torch.tensor(v, dtype=F32)
rsqrt32 = lambda t: t.double().rsqrt().float()
WAVE = (32, 16, 8, 4, 2, 1)


def fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in fp64, one rounding of the sum."""
    return (a.double() * b.double() + c.double()).float()


def xor_tree(v, offsets):
    idx = torch.arange(v.shape[-1])
    for o in offsets:
        v = v + v[..., idx ^ o]
    return v[..., 0]


# ------------------------------------------------------------------------------------------------------------------------------
# layernorm_rows / rowstats_rows


def chunks(x):
    """x [R, D] as the lanes hold it: fp32 [R, NCH, 64, 8], zeros where a lane has no chunk, + live [NCH, 64]."""
    R, D = x.shape
    n = D // 8
    nch = -(-n // 64)
    v = torch.zeros(R, nch * 64, 8)
    v[:, :n] = x.float().view(R, n, 8)
    return v.view(R, nch, 64, 8), (torch.arange(nch * 64) < n).view(nch, 64)


def two_pass(x, bug=None):
    R, D = x.shape
    v, live = chunks(x)
    nch, last = v.shape[1], D // 8 - 1
    vs, lv = v.clone(), live.clone()
    if bug == "sum_tail":
        vs[:, last // 64, last % 64] = 0
    if bug == "sq_tail":
        lv[last // 64, last % 64] = False
    s = torch.zeros(R, 64)
    for c in range(nch):
        for e in range(8):
            s = s + vs[:, c, :, e]
    inv_d = c32(1.0) / c32(float(D - 1 if bug == "dm1" else D))
    mean = xor_tree(s, WAVE) * inv_d
    q = torch.zeros(R, 64)
    for c in range(nch):
        for e in range(8):
            d = v[:, c, :, e] - mean[:, None]
            q = torch.where(lv[c], fma(d, d, q), q)
    var = xor_tree(q, WAVE) * inv_d
    rstd = rsqrt32(var) if bug == "no_eps" else rsqrt32(var) + c32(EPS) if bug == "eps_after" else rsqrt32(var + c32(EPS))
    return mean, rstd, v


def emu_layernorm(x, gamma, beta, out_bf16, bug=None):
    R, D = x.shape
    mean, rstd, v = two_pass(x, bug)
    nch, last = v.shape[1], D // 8 - 1
    g, b = torch.zeros(nch * 512), torch.zeros(nch * 512)
    g[:D], b[:D] = gamma, beta
    g, b = g.view(nch, 64, 8).clone(), b.view(nch, 64, 8).clone()
    if bug == "gb_prev":
        g[1:], b[1:] = g[:-1].clone(), b[:-1].clone()
    if bug == "beta_tail":
        b[last // 64, last % 64] = 0
    y = fma((v - mean[:, None, None, None]) * rstd[:, None, None, None], g, b).reshape(R, -1)[:, :D]
    return bf(y) if out_bf16 or bug == "via_bf16" else y


LN_CASES = [(rows, D) for D in H.LN_EDGE_D for rows in H.LN_EDGE_ROWS] + [H.LN_LAP_CASE]


def ln_dtypes(D):
    return [(False, True), (False, False), (True, True), (True, False)] if D in H.LN_ALL_DTYPES_D else [(False, True)]


@pytest.mark.parametrize("D", H.LN_EDGE_D + [H.LN_LAP_CASE[1]])
def test_clean_layernorm_and_rowstats_are_inside_the_bounds(D):
    for rows in (H.LN_LAP_CASE[:1] if D == H.LN_LAP_CASE[1] else H.LN_EDGE_ROWS):
        for f32_in, bf16_out in ln_dtypes(D):
            x, g, b = H.spiked_rows_case(rows, D, 0, f32_in)
            q, k = H.ratio(emu_layernorm(x, g, b, bf16_out), *H.ln_ref64(x, g, b, EPS, bf16_out))
            print(f"layernorm ({rows}, {D}) {'fp32' if f32_in else 'bf16'} -> {'bf16' if bf16_out else 'fp32'}: clean {q:.3f} at "
                  f"({k // D}, {k % D})")
            assert q <= 1.0, (rows, D, f32_in, bf16_out, q)
        x = H.spiked_rows_case(rows, D, 0)[0]
        mean, rstd, _ = two_pass(x)
        (qm, rm), (qr, rr), _ = H.stats_ratios(torch.stack([mean, rstd], 1), H.row_stats_ref64(x, EPS))
        print(f"rowstats ({rows}, {D}): clean mean {qm:.3f} (row {rm}), rstd {qr:.3f} (row {rr})")
        assert qm <= 1.0 and qr <= 1.0, (rows, D, qm, qr)


def _cols(lo):
    return lambda rows, D: (slice(None), slice(lo if lo >= 0 else D + lo, None))


CONST = lambda rows, D: (slice(1, 2), slice(None))
# mistake -> (the elements it touches, the (rows, D, fp32 in, bf16 out) it is asserted at)
LN_BUGS = {
    "sum_tail": (None, lambda r, D, fi, bo: True),
    "sq_tail": (None, lambda r, D, fi, bo: True),
    "gb_prev": (_cols(512), lambda r, D, fi, bo: D > 512),
    "dm1": (None, lambda r, D, fi, bo: D <= 1152),
    "no_eps": (CONST, lambda r, D, fi, bo: r >= 3),
    "eps_after": (CONST, lambda r, D, fi, bo: r >= 3),
    "beta_tail": (_cols(-8), lambda r, D, fi, bo: True),
    "via_bf16": (None, lambda r, D, fi, bo: not bo),
}


@pytest.mark.parametrize("bug", LN_BUGS)
def test_layernorm_bound_tells_mistakes_apart(bug):
    where, at = LN_BUGS[bug]
    lows = {}
    for rows, D in LN_CASES[:-1]:
        for f32_in, bf16_out in ln_dtypes(D):
            x, g, b = H.spiked_rows_case(rows, D, 0, f32_in)
            ref, bound = H.ln_ref64(x, g, b, EPS, bf16_out)
            sl = where(rows, D) if where else (slice(None), slice(None))
            if ref[sl].numel() == 0 or (bug == "via_bf16" and bf16_out):
                continue
            q, _ = H.ratio(emu_layernorm(x, g, b, bf16_out, bug)[sl], ref[sl], bound[sl])
            held = at(rows, D, f32_in, bf16_out)
            lows[D, held] = min(lows.get((D, held), float("inf")), q)
            assert not held or q >= MIN_RATIO, (bug, rows, D, f32_in, bf16_out, q)
    print(f"layernorm {bug}: " + ", ".join(f"D = {D}: {q:.1f}{'' if held else ' (printed only)'}" for (D, held), q in lows.items()))
    assert sum(held for _, held in lows) >= 2, (bug, lows)


# which statistic shows the mistake (0 the mean, 1 rstd), on which rows, at which (rows, D)
STATS_BUGS = {
    "sum_tail": (0, None, lambda r, D: True),
    "sq_tail": (1, None, lambda r, D: True),
    "dm1": (0, None, lambda r, D: D <= 1152),
    "no_eps": (1, 1, lambda r, D: r >= 3),
    "eps_after": (1, 1, lambda r, D: r >= 3),
}


@pytest.mark.parametrize("bug", STATS_BUGS)
def test_rowstats_bound_tells_mistakes_apart(bug):
    j, row, at = STATS_BUGS[bug]
    lows = {}
    for rows, D in LN_CASES[:-1]:
        if row is not None and rows <= row:
            continue
        x = H.spiked_rows_case(rows, D, 0)[0]
        if row is not None:
            x = x[row:row + 1]
        mean, rstd, _ = two_pass(x, bug)
        q = H.stats_ratios(torch.stack([mean, rstd], 1), H.row_stats_ref64(x, EPS))[j][0]
        held = at(rows, D)
        lows[D, held] = min(lows.get((D, held), float("inf")), q)
        assert not held or q >= MIN_RATIO, (bug, rows, D, q)
    print(f"rowstats {bug} ({('mean', 'rstd')[j]}): " + ", ".join(f"D = {D}: {q:.1f}{'' if held else ' (printed only)'}" for (D, held), q in lows.items()))
    assert sum(held for _, held in lows) >= 2, (bug, lows)


# ------------------------------------------------------------------------------------------------------------------------------
# rowparts_kernel + rowstats_finalize_kernel


def _quad(t):
    """Two chained dot2 accumulations from 0 over t [..., 2 dwords, 2]: each adds a dword's two (exact) products to the accumulator
    and rounds once."""
    a = (t[..., 0, 0].double() + t[..., 0, 1].double()).float()
    return (a.double() + t[..., 1, 0].double() + t[..., 1, 1].double()).float()


def emu_parts(x):
    R, D = x.shape
    c = x.float().view(R, D // 32, 4, 2, 2, 2)            # group, octet, quad, dword, half
    out = []
    for t in (c, c * c):
        o = _quad(t)
        o = o[..., 0] + o[..., 1]
        out.append((o[..., 0] + o[..., 1]) + (o[..., 2] + o[..., 3]))
    return torch.stack(out, -1)


def emu_finalize(parts, bug=None):
    R, G = parts.shape[:2]
    D = 32 * G
    sums, sq = parts[..., 0], parts[..., 1]
    if bug == "q_neighbour":
        sq = torch.roll(sq, 1, 0)
    S, Q = torch.zeros(R, 8), torch.zeros(R, 8)
    for g in range(min(G, 8) if bug == "g_ge_8" else G):
        S[:, g % 8] = S[:, g % 8] + sums[:, g]
        Q[:, g % 8] = Q[:, g % 8] + sq[:, g]
    inv_d = c32(1.0) / c32(float(D))
    mean = xor_tree(S, (1, 2, 4)) * inv_d
    var = xor_tree(Q, (1, 2, 4)) * inv_d - mean * mean
    if bug != "no_clamp":
        var = var.clamp_min(0)
    return torch.stack([mean, rsqrt32(var + c32(EPS))], 1)


FIN_CASES = [(rows, 32 * G) for G in H.FINALIZE_G for rows in H.FINALIZE_ROWS] + [H.LN_LAP_CASE]


@pytest.mark.parametrize("G", H.FINALIZE_G + [H.LN_LAP_CASE[1] // 32])
def test_clean_parts_and_finalize_are_inside_the_bounds(G):
    D = 32 * G
    for rows in (H.LN_LAP_CASE[:1] if D == H.LN_LAP_CASE[1] else H.FINALIZE_ROWS):
        x = H.ladder_rows_case(rows, D)
        parts = emu_parts(x)
        s, q, bs, bq = H.parts_ref64(x)
        qs, qq = H.ratio(parts[..., 0], s, bs)[0], H.ratio(parts[..., 1], q, bq)[0]
        ref, rung = H.row_stats_ref64(x, EPS), H.ladder_of(rows)
        st = emu_finalize(parts)
        (qm, _), (q1, r1), (q2, r2) = H.stats_ratios(st, ref, onepass=True)
        print(f"finalize ({rows}, {D}): parts {qs:.3f} / {qq:.3f}; clean mean {qm:.3f}, rstd {q1:.3f} of the one-pass interval (row {r1}, "
              f"rung {int(rung[r1])}), {q2:.3f} of the two-pass interval (row {r2}, rung {int(rung[r2])})")
        assert max(qs, qq, qm, q1) <= 1.0, (rows, D, qs, qq, qm, q1)
        mean, rstd, _ = two_pass(x)
        (tm, _), (t2, _), _ = H.stats_ratios(torch.stack([mean, rstd], 1), ref)
        assert tm <= 1.0 and t2 <= 1.0, ("two-pass on the ladder", rows, D, tm, t2)


FIN_BUGS = {
    "g_ge_8": (0, lambda r, D: D > 256),
    "no_clamp": (1, lambda r, D: r >= 7),
    "q_neighbour": (1, lambda r, D: r >= 2),
}


@pytest.mark.parametrize("bug", FIN_BUGS)
def test_finalize_bound_tells_mistakes_apart(bug):
    """no_clamp touches a row only where the clamp acts: where Q / D - mean^2 comes out below 0.  On the exactly constant row it
    never does (every partial sum of a tree over equal values is exact, and so are Q / D and mean^2: the difference is 0 at every
    D); on the nearly constant row it does at D = 1152 and 4096 in this emulation, and rsqrt(var + eps) is then a NaN."""
    j, at = FIN_BUGS[bug]
    lows = {}
    for rows, D in FIN_CASES[:-1]:
        if not at(rows, D):
            continue
        x = H.ladder_rows_case(rows, D)
        if bug == "no_clamp":
            assert torch.equal(emu_finalize(emu_parts(x[rows - 2:rows - 1]), bug), emu_finalize(emu_parts(x[rows - 2:rows - 1])))
            x = x[rows - 3:rows - 2]
        parts = emu_parts(x)
        st = emu_finalize(parts, bug)
        if bug == "no_clamp" and torch.equal(st, emu_finalize(parts)):
            continue
        q = H.stats_ratios(st, H.row_stats_ref64(x, EPS), onepass=True)[j][0]
        lows[D] = min(lows.get(D, float("inf")), q)
        assert q >= MIN_RATIO, (bug, rows, D, q)
    print(f"finalize {bug} ({('mean', 'rstd')[j]}): " + ", ".join(f"D = {D}: {q:.1f}" for D, q in lows.items()))
    assert len(lows) >= 2, (bug, lows)


# ---- the one-pass domain

DOMAIN_D = (192, 384, 768, 1024, 1152, 4096)
HALF_ULP = 2.0 ** -8


def _domain_row(D, r, seed):
    g = torch.Generator().manual_seed(seed + D)
    x = torch.randn(8, D, generator=g).double() * 1.7 + r * 1.7
    x[:, D - 8:] += 40.0
    return x.float()          # fp32 rows for the fp64 statistics; the kernel's partial sums take their bf16 rounding


def test_one_pass_domain_table():
    """For each D, by bisection over mean / std on a geometric grid: where b_var1 / (var + eps) reaches 2^-8 (from there on the
    bound no longer promises an rstd within bf16's half ulp of the folded output), and where the emulated kernel's own
    |var^ - var| / (var + eps) does.  The bound must give way first."""
    grid = [2.0 ** (k / 4) for k in range(0, 4 * 14 + 1)]          # 1 .. 16384
    for D in DOMAIN_D:
        first_bound = first_emu = None
        for r in grid:
            x = _domain_row(D, r, 0).to(torch.bfloat16)
            ref = H.row_stats_ref64(x, EPS)
            st = emu_finalize(emu_parts(x)).double()
            var_hat = st[:, 1] ** -2 - ref.eps
            if first_bound is None and float((ref.b_var1 / (ref.var + ref.eps)).max()) >= HALF_ULP:
                first_bound = float((ref.mean.abs() / ref.var.sqrt()).min())
            if first_emu is None and float(((var_hat - ref.var).abs() / (ref.var + ref.eps)).max()) >= HALF_ULP:
                first_emu = float((ref.mean.abs() / ref.var.sqrt()).min())
        print(f"one-pass domain D = {D}: the bound reaches 2^-8 at mean / std = {first_bound:.1f}, the emulated kernel at "
              f"{'> 16384' if first_emu is None else f'{first_emu:.1f}'}")
        assert first_bound is not None and (first_emu is None or first_emu >= first_bound), (D, first_bound, first_emu)


# ------------------------------------------------------------------------------------------------------------------------------
# the chain: statistics kernel -> ov_gemm_ln


@pytest.mark.parametrize("shape", H.FOLD_SHAPES[:2])
def test_clean_chain_is_inside_the_combined_bound(shape):
    import test_gemm_small_bound as GS
    x, wg, cvec, colsum = H.spiked_fold_case(*shape)[:4]
    mean, rstd, _ = two_pass(x)
    for name, st, onepass in (("rowstats", torch.stack([mean, rstd], 1), False), ("rowparts + finalize", emu_finalize(emu_parts(x)), True)):
        outs = {GS.FOLD_NAME[epi]: (GS.emulate(x, wg, cvec, epi, fold=(colsum, st)), epi) for epi in (0, 1)}
        for form, (q, row, col) in H.fold_chain_ratios(x, wg, colsum, cvec, outs, onepass).items():
            print(f"chain {shape} {name} {form}: clean {q:.3f} at ({row}, {col})")
            assert q <= 1.0, (shape, name, form, q)


@pytest.mark.parametrize("shape", H.FOLD_SHAPES[:2])
def test_chain_bound_tells_statistics_mistakes_apart(shape):
    """A statistics mistake seen through the folded GEMM's bf16 output, bias epilogue."""
    import test_gemm_small_bound as GS
    x, wg, cvec, colsum = H.spiked_fold_case(*shape)[:4]
    for bug in ("sum_tail", "sq_tail"):
        mean, rstd, _ = two_pass(x, bug)
        outs = {"fold bias": (GS.emulate(x, wg, cvec, 0, fold=(colsum, torch.stack([mean, rstd], 1))), 0)}
        q = H.fold_chain_ratios(x, wg, colsum, cvec, outs, False)["fold bias"][0]
        print(f"chain {shape} rowstats {bug}: {q:.1f}")
        assert q >= MIN_RATIO, (shape, bug, q)
    for bug in ("q_neighbour",):
        outs = {"fold bias": (GS.emulate(x, wg, cvec, 0, fold=(colsum, emu_finalize(emu_parts(x), bug))), 0)}
        q = H.fold_chain_ratios(x, wg, colsum, cvec, outs, True)["fold bias"][0]
        print(f"chain {shape} finalize {bug}: {q:.1f}")
        assert q >= MIN_RATIO, (shape, bug, q)


# ------------------------------------------------------------------------------------------------------------------------------
# mean_pool_kernel, l2norm_kernel


def emu_pool(x, B, L, first, bug=None):
    t = x.float().view(B, L, -1)
    acc = torch.zeros(4, B, t.shape[2])
    start = 0 if bug == "with_cls" else first
    for tok in range(start, L):
        w = (tok - start) % 4
        if not (bug == "wave3" and w == 3):
            acc[w] = acc[w] + t[:, tok]
    return (((acc[0] + acc[1]) + acc[2]) + acc[3]) * (c32(1.0) / c32(float(L if bug == "div_L" else L - first)))


POOL_CASES = [(B, L, D, first) for first in (0, 1) for L in H.POOL_L for D in H.POOL_D for B in (1, 3)]


def test_clean_pool_is_inside_the_bound():
    worst = 0.0
    for B, L, D, first in POOL_CASES:
        x = H.pool_case(B, L, D)
        q, _ = H.ratio(emu_pool(x, B, L, first), *H.mean_pool_ref64(x, B, L, first))
        worst = max(worst, q)
        assert q <= 1.0, (B, L, D, first, q)
    print(f"mean_pool: clean max {worst:.3f} over {len(POOL_CASES)} cases")


POOL_BUGS = {"div_L": lambda L, first: first == 1, "with_cls": lambda L, first: first == 1, "wave3": lambda L, first: L - first >= 4}


@pytest.mark.parametrize("bug", POOL_BUGS)
def test_pool_bound_tells_mistakes_apart(bug):
    lo, hit = float("inf"), set()
    for B, L, D, first in POOL_CASES:
        if POOL_BUGS[bug](L, first):
            x = H.pool_case(B, L, D)
            q, _ = H.ratio(emu_pool(x, B, L, first, bug), *H.mean_pool_ref64(x, B, L, first))
            lo = min(lo, q)
            hit.add((L, D))
            assert q >= MIN_RATIO, (bug, B, L, D, first, q)
    print(f"mean_pool {bug}: min {lo:.1f} over {len(hit)} (L, D)")
    assert len(hit) >= 2


def emu_l2norm(x, bug=None):
    R, E = x.shape
    n = -(-E // 64)
    v = torch.zeros(R, n * 64)
    v[:, :E] = x.float()
    v = v.view(R, n, 64)
    ss = torch.zeros(R, 64)
    for c in range(E // 64 if bug == "l2_tail" else n):
        ss = fma(v[:, c], v[:, c], ss)
    nrm = xor_tree(ss, WAVE).double().sqrt().float()
    inv = c32(1.0) / (nrm if bug == "l2_no_clamp" else nrm.clamp_min(1e-12))
    return x.float() * inv[:, None]


L2_CASES = [(5, E, f32) for E in H.L2_E for f32 in (False, True)] + [H.L2_LAP_CASE + (False,)]


def test_clean_l2norm_is_inside_the_bound():
    for rows, E, f32 in L2_CASES:
        x = H.l2norm_case(rows, E, f32)
        y = emu_l2norm(x)
        q, _ = H.ratio(y, *H.l2norm_ref64(x))
        print(f"l2norm ({rows}, {E}) {'fp32' if f32 else 'bf16'}: clean {q:.3f}")
        assert q <= 1.0, (rows, E, f32, q)
        assert bool((y[1] == 0).all())


@pytest.mark.parametrize("bug", ["l2_tail", "l2_no_clamp"])
def test_l2norm_bound_tells_mistakes_apart(bug):
    hit = set()
    for rows, E, f32 in L2_CASES[:-1]:
        if bug == "l2_tail" and E % 64 == 0:
            continue
        x = H.l2norm_case(rows, E, f32)
        ref, bound = H.l2norm_ref64(x)
        y = emu_l2norm(x, bug)
        rws = [1, 2] if bug == "l2_no_clamp" else [0, 3, 4]
        for r in rws:
            q, _ = H.ratio(y[r], ref[r], bound[r])
            assert q >= MIN_RATIO, (bug, rows, E, f32, r, q)
        print(f"l2norm ({rows}, {E}) {'fp32' if f32 else 'bf16'} {bug}: rows {rws} all >= {MIN_RATIO}, the last {q:.1f}")
        hit.add(E)
    assert len(hit) >= 2
