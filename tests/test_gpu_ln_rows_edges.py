"""The row passes -- ov_layernorm, ov_rowstats, ov_rowparts + ov_rowstats_finalize -- and the rows around the towers' heads
(ov_mean_pool, ov_l2norm, ov_gather_rows, ov_cls_rows) against fp64 references under derived per-element bounds.

test_layernorm_bf16 holds ov_layernorm to rtol = atol = 8e-3 on Gaussian rows with dense pitches; ov_rowstats and the finalize kernel
were compared once, with each other; the head kernels only through whole-model goldens.  Here each meets a bound built from
u = 2^-8, e = 2^-24 and gamma_n alone (hipops.row_stats_ref64, ln_ref64, parts_ref64, mean_pool_ref64, l2norm_ref64; fold_bound's
stat_err for the chain into ov_gemm_ln) at the smallest shapes where its loops change form: every NCH specialisation at a partly and
a fully live last chunk, workgroups with idle waves, the grid-stride second lap, all four dtype pairs, row pitches wider than D and
the class-pool call's ldx = L D, finalize's stride-8 loop at one, exactly one and one-and-a-bit trips, the pool's empty waves.
Inputs are spiked (hipops.spiked_rows_case, ladder_rows_case, pool_case, l2norm_case); operands sit in NaN-padded buffers, outputs
start as the sentinel 77 in buffers wider than they need, whose padding must keep it.  The fp64 references are torch's, on the
device.  What the bounds tell apart is pinned without a GPU by test_ln_rows_bound.py."""
import pytest
import torch

import hipops as H
from hipops import DEV, SENT, pitched

pytestmark = pytest.mark.gpu

EPS = 1e-6
BF16, F32 = torch.bfloat16, torch.float32
NAME = {BF16: "bf16", F32: "fp32"}


def out_buf(rows, cols, dtype):
    return torch.full((rows, cols + 8), SENT, dtype=dtype, device=DEV)


def kept(buf, cols):
    return bool((buf[:, cols:] == SENT).all())


def run_layernorm(x, g, b, out_dtype):
    """ov_layernorm from a NaN-padded x into a sentinel-filled pitched output: (y, max err / bound, row, column)."""
    rows, D = x.shape
    buf = out_buf(rows, D, out_dtype)
    y = H.layernorm(pitched(x), g, b, out=buf[:, :D])
    assert kept(buf, D), (rows, D, "the output's padding")
    q, k = H.ratio(y, *H.ln_ref64(x, g, b, EPS, out_dtype == BF16))
    return y, q, k // D, k % D


def check_stats(tag, st, ref, onepass=False):
    (qm, rm), (q1, r1), (q2, r2) = H.stats_ratios(st, ref, onepass)
    print(f"{tag}: mean err / bound {qm:.3f} (row {rm}), rstd {q1:.3f} of its interval (row {r1})" +
          (f", {q2:.3f} of the two-pass interval (row {r2})" if onepass else ""))
    assert qm <= 1.0 and q1 <= 1.0, (tag, qm, rm, q1, r1)
    return qm, q1, q2


@pytest.mark.parametrize("D", H.LN_EDGE_D)
def test_layernorm_and_rowstats_at_every_chunk_count(D):
    """Rows 1, 3, 5 (a workgroup with idle waves) at each D of the table; all four dtype pairs at D = 520 and 1152; the same launch
    twice is bitwise the same."""
    pairs = [(BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32)] if D in H.LN_ALL_DTYPES_D else [(BF16, BF16)]
    for rows in H.LN_EDGE_ROWS:
        for din, dout in pairs:
            x, g, b = (t.to(DEV) for t in H.spiked_rows_case(rows, D, 0, din == F32))
            y, q, row, col = run_layernorm(x, g, b, dout)
            print(f"layernorm ({rows}, {D}) {NAME[din]} -> {NAME[dout]}: max err / bound {q:.3f} at ({row}, {col})")
            assert q <= 1.0, (rows, D, din, dout, q, row, col)
            assert torch.equal(y, run_layernorm(x, g, b, dout)[0])
        x = H.spiked_rows_case(rows, D, 0)[0].to(DEV)
        check_stats(f"rowstats ({rows}, {D})", H.rowstats(pitched(x), EPS), H.row_stats_ref64(x, EPS))


def test_layernorm_and_rowstats_second_grid_stride_lap():
    """65541 rows: 16384 workgroups of 4 rows and five rows more, the spiked last row among them."""
    rows, D = H.LN_LAP_CASE
    x, g, b = (t.to(DEV) for t in H.spiked_rows_case(rows, D, 0))
    _, q, row, col = run_layernorm(x, g, b, BF16)
    print(f"layernorm ({rows}, {D}): max err / bound {q:.3f} at ({row}, {col})")
    assert q <= 1.0, (q, row, col)
    check_stats(f"rowstats ({rows}, {D})", H.rowstats(pitched(x), EPS), H.row_stats_ref64(x, EPS))


@pytest.mark.parametrize("D", H.LN_ALL_DTYPES_D)
def test_layernorm_class_pool_pitch(D):
    """The class-pool head's call: rows = B, ldx = L D (row b of the input is token 0 of sequence b), fp32 in and bf16 in."""
    B, L = 3, 5
    for din, dout in ((BF16, BF16), (F32, BF16)):
        x, g, b = (t.to(DEV) for t in H.spiked_rows_case(B * L, D, 1, din == F32))
        buf = out_buf(B, D, dout)
        y = H.layernorm(x.view(B, L * D)[:, :D], g, b, out=buf[:, :D])
        assert kept(buf, D)
        q, k = H.ratio(y, *H.ln_ref64(x[::L].contiguous(), g, b, EPS, True))
        print(f"layernorm class rows (B = {B}, L = {L}, D = {D}) {NAME[din]} in: max err / bound {q:.3f}")
        assert q <= 1.0, (D, din, q, k // D, k % D)


def test_row_kernels_refuse_what_they_do_not_cover():
    bf = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)
    g = torch.ones(8200, device=DEV)
    unsupported, invalid = r"status -2\b", r"status -1\b"
    with pytest.raises(H._lib.OvhipError, match=unsupported):           # D % 8
        H.layernorm(bf(2, 12), g[:12], g[:12])
    with pytest.raises(H._lib.OvhipError, match=unsupported):           # D > 8192
        H.layernorm(bf(1, 8200), g, g)
    with pytest.raises(H._lib.OvhipError, match=unsupported):           # ldx % 8
        H.layernorm(bf(2, 20)[:, :16], g[:16], g[:16])
    with pytest.raises(H._lib.OvhipError, match=unsupported):           # ldy % 8
        H.layernorm(bf(2, 16), g[:16], g[:16], out=bf(2, 20)[:, :16])
    with pytest.raises(H._lib.OvhipError, match=unsupported):           # ldx < D
        H.layernorm(bf(32).as_strided((2, 16), (8, 1)), g[:16], g[:16])
    with pytest.raises(H._lib.OvhipError, match=unsupported):           # ldy < D
        H.layernorm(bf(2, 16), g[:16], g[:16], out=bf(32).as_strided((2, 16), (8, 1)))
    with pytest.raises(H._lib.OvhipError, match=invalid):               # x 8 bytes off a 16-byte boundary
        H.layernorm(bf(40)[4:36].view(2, 16), g[:16], g[:16])
    with pytest.raises(H._lib.OvhipError, match=invalid):               # y
        H.layernorm(bf(2, 16), g[:16], g[:16], out=bf(40)[4:36].view(2, 16))
    with pytest.raises(H._lib.OvhipError, match=invalid):               # gamma 4 bytes off
        H.layernorm(bf(2, 16), g[1:17], g[:16])
    with pytest.raises(H._lib.OvhipError, match=unsupported):
        H.rowstats(bf(2, 12))
    with pytest.raises(H._lib.OvhipError, match=unsupported):
        H.rowstats(bf(1, 8200))
    with pytest.raises(H._lib.OvhipError, match=unsupported):
        H.rowstats(bf(2, 20)[:, :16])
    with pytest.raises(H._lib.OvhipError, match=invalid):
        H.rowstats(bf(40)[4:36].view(2, 16))
    with pytest.raises(H._lib.OvhipError, match=unsupported):           # D % 32: the 4304-wide MLP has no partial sums
        H.rowparts(bf(2, 4304))


# ---- ov_rowparts + ov_rowstats_finalize


def run_finalize(rows, D):
    x = H.ladder_rows_case(rows, D).to(DEV)
    parts = H.rowparts(pitched(x))
    s, q, bs, bq = H.parts_ref64(x)
    qs, qq = H.ratio(parts[..., 0], s, bs)[0], H.ratio(parts[..., 1], q, bq)[0]
    print(f"rowparts ({rows}, {D}): sums {qs:.3f}, squares {qq:.3f} of their bounds")
    assert qs <= 1.0 and qq <= 1.0, (rows, D, qs, qq)
    flat = torch.full((2 * rows + 2,), SENT, dtype=F32, device=DEV)
    lib = H._lib.load()
    H.check(lib.ov_rowstats_finalize(H.ptr(parts), H.ptr(flat), rows, D, EPS, H.stream_ptr()), "ov_rowstats_finalize")
    assert bool((flat[-2:] == SENT).all())
    st = flat[:-2].view(rows, 2)
    assert torch.equal(st, H.rowstats_finalize(parts, EPS))
    ref = H.row_stats_ref64(x, EPS)
    res = check_stats(f"finalize ({rows}, {D})", st, ref, onepass=True)
    check_stats(f"rowstats ({rows}, {D}), the same rows", H.rowstats(pitched(x), EPS), ref)
    rung = H.ladder_of(rows).to(DEV)
    for j, r in enumerate(H.LADDER):
        if bool((rung == j).any()):
            sel = rung == j
            rel = ((st[sel, 1].double() - ref.rstd[sel]).abs() / ref.rstd[sel]).max()
            print(f"    mean / std = {r:g}: rstd off by {float(rel):.2e} relative")
    return res


@pytest.mark.parametrize("G", H.FINALIZE_G)
def test_rowparts_and_finalize_at_every_group_count(G):
    """Rows 1, 31, 32, 33 (32 rows fill one finalize workgroup) on the mean / std ladder 0 .. 512 with the constant and the nearly
    constant row: the partial sums against fp64 group sums, {mean, rstd} against the one-pass bounds; the ratio to the two-pass
    interval is printed (what the route gives up), not asserted.  ov_rowstats on the same rows stays inside the two-pass bounds."""
    for rows in H.FINALIZE_ROWS:
        run_finalize(rows, 32 * G)


def test_rowparts_and_finalize_second_grid_stride_lap():
    run_finalize(*H.LN_LAP_CASE)


# ---- the chain: a statistics kernel's output into ov_gemm_ln


@pytest.mark.parametrize("shape", H.FOLD_SHAPES[:2])
def test_statistics_into_the_folded_gemm(shape):
    """ov_rowstats -> ov_gemm_ln and ov_rowparts -> ov_rowstats_finalize -> ov_gemm_ln on hipops.spiked_fold_case against
    Linear(LayerNorm(x)) in fp64, bias and GELU-erf epilogues, under fold_bound with the statistics' bounds carried through; the
    tuned rule beside it."""
    M, N, K = shape
    ops = [t.to(DEV) for t in H.spiked_fold_case(M, N, K)]
    x, wg, cvec, colsum = pitched(ops[0]), pitched(ops[1]), ops[2], ops[3]
    for name, st, onepass in (("rowstats", H.rowstats(x, EPS), False), ("rowparts + finalize", H.rowstats_finalize(H.rowparts(x), EPS), True)):
        outs = {}
        for epi, form in ((0, "fold bias"), (1, "fold gelu erf")):
            outs[form] = (H.gemm_ln(x, wg, cvec, colsum, st, epi=epi, out=H.sentinel(M, N + 8)), epi)
            assert H.padding_kept(outs[form][0], N), (shape, name, form)
        H.report(f"{name} -> ov_gemm_ln {shape}", H.fold_chain_ratios(ops[0], ops[1], colsum, cvec, outs, onepass, EPS))
        H.report(f"{name} -> ov_gemm_ln {shape}, tuned rule", H.ln_linear_ratios(ops, outs))


# ---- the head rows


@pytest.mark.parametrize("L", H.POOL_L)
def test_mean_pool(L):
    """first 0 and 1, D = 8, 520, 1152 (grid.y 1, 2, 3, the last partly idle), B = 1 and 3; L - first < 4 leaves waves empty."""
    worst = 0.0
    for first in (0, 1):
        for D in H.POOL_D:
            for B in (1, 3):
                x = H.pool_case(B, L, D).to(DEV)
                flat = torch.full((B * D + 4,), SENT, dtype=F32, device=DEV)
                out = H.mean_pool(pitched(x), B, L, first, out=flat[:B * D].view(B, D))
                assert bool((flat[-4:] == SENT).all())
                q, k = H.ratio(out, *H.mean_pool_ref64(x, B, L, first))
                worst = max(worst, q)
                assert q <= 1.0, (B, L, D, first, q, k // D, k % D)
    print(f"mean_pool L = {L}: max err / bound {worst:.3f}")


@pytest.mark.parametrize("E", H.L2_E)
def test_l2norm(E):
    for f32 in (False, True):
        x = H.l2norm_case(5, E, f32).to(DEV)
        buf = out_buf(5, E, F32)
        y = H.l2norm(pitched(x), out=buf[:, :E])
        assert kept(buf, E)
        q, k = H.ratio(y, *H.l2norm_ref64(x))
        print(f"l2norm (5, {E}) {'fp32' if f32 else 'bf16'}: max err / bound {q:.3f}")
        assert q <= 1.0, (E, f32, q, k // E, k % E)
        assert bool((y[1] == 0).all())


def test_l2norm_second_grid_stride_lap():
    rows, E = H.L2_LAP_CASE
    x = H.l2norm_case(rows, E, False).to(DEV)
    buf = out_buf(rows, E, F32)
    y = H.l2norm(pitched(x), out=buf[:, :E])
    assert kept(buf, E)
    q, k = H.ratio(y, *H.l2norm_ref64(x))
    print(f"l2norm ({rows}, {E}): max err / bound {q:.3f}")
    assert q <= 1.0, (q, k // E, k % E)


def test_gather_rows_bitwise():
    B, L, D = 3, 5, 520
    x = H.rnd(B * L, D, seed=3).to(BF16).to(DEV)
    for t in (0, L - 1):
        buf = out_buf(B, D, BF16)
        out = H.gather_rows(pitched(x), B, L, t, out=buf[:, :D])
        assert kept(buf, D)
        assert torch.equal(out, x.view(B, L, D)[:, t])


def test_cls_rows_bitwise_and_nothing_else_written():
    B, L, D = 3, 5, 203
    cls, pos0 = H.rnd(D, seed=4).to(DEV), H.rnd(D, seed=5).to(DEV)
    buf = torch.full((B * L, D + 5), SENT, dtype=BF16, device=DEV)
    H.cls_rows(buf, cls, pos0, B, L)
    want = torch.full_like(buf, SENT)
    want[::L, :D] = H.cls_rows_ref(cls, pos0)
    assert torch.equal(buf, want)
