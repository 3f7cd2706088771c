"""The skinny and plain GEMM kernels, ov_gemm_batched and the LN fold against independent fp64 references.

test_gpu_gemm_routes.py holds the persistent kernel to derived per-element bounds; the launcher's other two bf16 kernels --
gemm_bf16_skinny (64 x 64 tiles, a four-stage LDS ring; every shape of at most 96 big tiles: one image's encode, both pooling heads,
the golden models) and gemm_bf16_pp ("plain": more than 96 tiles on a grid below the CU count or with K < 192; ov_gemm_keep's second
launch; ov_gemm_batched; GELU with row maps) -- were compared with rtol = atol = 1e-2 into zero-filled outputs, or bitwise with each
other.  Here they meet the same bounds (hipops.linear_ratios: bias, GELU, residual with its two roundings; the GELU-gradient
epilogues; hipops.fold_bound for the LN fold, in every kernel), at the shapes where their loops change form: one K-tile, the
prefetch depth, the ring's length, its first slot reuse and two laps; ragged last row and column tiles down to one row and one
8-column quad; tile counts that leave the XCD map's runs unequal.

Every case first asserts, on what the library itself reports for the call (hipops.route: ov_gemm_route, the launcher's own decision
on this device), that the kernel it names is the one selected.  Outputs start
as the bf16 sentinel 77 in buffers wider than N, whose padding must keep it; operands sit in buffers whose padding is NaN.  The fp64
references are torch's, on the device.  What the bounds tell apart is pinned without a GPU by test_gemm_small_bound.py."""
import functools

import pytest
import torch

import hipops as H
from hipops import DEV, SENT, fold_ratios_bound, linear_ratios, ln_linear_ratios, padding_kept, pitched, report, route, sentinel
import test_gpu_gemm_routes as RT

pytestmark = pytest.mark.gpu

KIND = {0: "pre", 1: "erf", 2: "tanh", 3: "res", 4: "gerf", 5: "gtanh"}
NAME = {0: "bias", 1: "gelu erf", 2: "gelu tanh", 3: "residual", 4: "gelu' erf", 5: "gelu' tanh"}
PLAIN_TILES = {(24827, 8, 64): 97, (1, 24584, 128): 97, (2500, 2568, 192): 110, (2305, 2816, 320): 110, (2500, 2592, 192): 110,
               (25000, 200, 64): 98}


def selected(shape, kernel, epi=0, keep=False, **operands):
    """Asserts that the launcher sends `shape` to `kernel` on this device.  operands: fold= / rowparts= / mapped= of the call."""
    M, N, K = shape
    r = route(M, N, K, epi, keep, **operands)
    assert r.kernel == kernel, (f"{shape}: {r.nwg} tiles on {r.cus} CUs, K = {K} selects the {r.kernel} kernel; the case is there for the "
                                f"{kernel} kernel")
    if kernel == "plain":
        assert r.nwg == PLAIN_TILES[shape] and r.nwg % 8 != 0, f"{shape}: {r.nwg} tiles, the case is there for {PLAIN_TILES[shape]}"
    return M, N, K


@functools.lru_cache(maxsize=None)
def operands(M, N, K, r_rows=None):
    """a, w (bf16, in NaN-padded buffers), bias (fp32), r (bf16, contiguous) on the device."""
    a, w, bias, r = H.gemm_case(M, N, K, r_rows)
    return pitched(a.to(DEV)), pitched(w.to(DEV)), bias.to(DEV), r.to(DEV)


def run_forms(shape, kernel, all_epilogues):
    """Every form the case table asks for at `shape`, one fp64 reference for all of them: bias and NULL bias; where all_epilogues, the
    two GELUs, the residual in place (C aliases R) and out of place (ldr != ldc), and the two GELU gradients."""
    M, N, K = shape
    a, w, bias, r = operands(M, N, K)
    outs, nobias = {}, {}
    for epi in (0, 1, 2) if all_epilogues else (0,):
        selected(shape, kernel, epi)
        outs[NAME[epi]] = (H.gemm(a, w, bias, epi=epi, out=sentinel(M, N + 8)), KIND[epi])
    nobias["bias = NULL"] = (H.gemm(a, w, None, epi=0, out=sentinel(M, N + 8)), "pre")
    if all_epilogues:
        for epi in (3, 4, 5):
            selected(shape, kernel, epi)
            outs[NAME[epi] + (", out of place" if epi == 3 else "")] = (
                H.gemm(a, w, bias, epi=epi, resid=pitched(r, 16), out=sentinel(M, N + 8)), KIND[epi])
        buf = sentinel(M, N + 8)
        buf[:, :N] = r
        outs["residual, in place"] = (H.gemm(a, w, bias, epi=3, resid=buf, out=buf), "res")
    tag = f"{kernel} {shape}"
    report(tag, linear_ratios(a, w, bias, outs, r))
    report(tag, linear_ratios(a, w, torch.zeros_like(bias), nobias))
    for name, (out, _) in {**outs, **nobias}.items():
        assert padding_kept(out, N), (tag, name)


@pytest.mark.parametrize("shape", H.SKINNY_SHAPES)
def test_skinny_epilogues_within_the_fp64_bound(shape):
    run_forms(shape, "skinny", shape in H.SKINNY_ALL_EPI)


@pytest.mark.parametrize("shape", H.PLAIN_SHAPES)
def test_plain_epilogues_within_the_fp64_bound(shape):
    run_forms(shape, "plain", shape in H.PLAIN_ALL_EPI)


def test_skinny_row_maps():
    """The patch embedding's launches at a small batch: out_group = g^2 leaves every image's class row alone (bias epilogue), and with
    resid_mod = g^2, resid_off = 1 patch p of every image adds row 1 + p of the [g^2 + 1, D] position table."""
    B, g2, D, K = H.ROWMAP_CASE
    for epi in (0, 3):
        selected((B * g2, D, K), "skinny", epi, mapped=True)
    a, w, bias, pos = operands(B * g2, D, K, g2 + 1)
    res = {}
    for epi in (0, 3):
        out = sentinel(B * (g2 + 1), D + 8)
        H.gemm(a, w, bias, epi=epi, resid=pitched(pos, 16) if epi else None, out=out, out_group=g2, resid_mod=g2 if epi else 0,
               resid_off=1 if epi else 0)
        assert bool((H.class_rows(out, B, g2) == SENT).all()) and padding_kept(out, D), NAME[epi]
        res.update(linear_ratios(a, w, bias, {NAME[epi]: (H.patch_rows(out, B, g2), KIND[epi])}, pos[1:].repeat(B, 1)))
    report(f"skinny row maps {H.ROWMAP_CASE}", res)


def test_plain_gelu_with_out_group():
    """GELU-erf with out_group: the ABI admits it, and no persistent form has it, so the plain kernel runs it at any size."""
    M, N, K, group = H.MAPPED_GELU_CASE
    selected((M, N, K), "plain", 1, mapped=True)
    a, w, bias, _ = operands(M, N, K, 1)
    out = H.gemm(a, w, bias, epi=1, out=sentinel(M + M // group, N + 8), out_group=group)
    assert bool((H.class_rows(out, M // group, group) == SENT).all()) and padding_kept(out, N)
    report(f"plain out_group {H.MAPPED_GELU_CASE}", linear_ratios(a, w, bias, {"gelu erf": (H.patch_rows(out, M // group, group), "erf")}))


def test_plain_keep_both_outputs():
    """ov_gemm_keep below the CU count: two launches of the plain kernel; the GELU output and the kept pre-activation, ldc != ldc2."""
    shape = H.PLAIN_ALL_EPI[0]
    M, N, K = selected(shape, "plain", 1, keep=True)
    a, w, bias, _ = operands(M, N, K)
    for epi in (1, 2):
        out, pre = H.gemm_keep(a, w, bias, epi, out=sentinel(M, N + 64), pre=sentinel(M, N + 8))
        report(f"plain {shape} keep", linear_ratios(a, w, bias, {NAME[epi]: (out, KIND[epi]), "pre-activation": (pre, "pre")}))
        assert padding_kept(out, N) and padding_kept(pre, N)


def test_batched_products_each_against_fp64():
    """ov_gemm_batched as ov_linear_backward calls it: A_z, W_z column ranges of one operand pair (lda = ldw = batch K, strides K),
    outputs stride_c > M ldc apart with sentinel rows between them; batch 1 is bitwise ov_gemm without a bias (the skinny kernel)."""
    M, N, K, batch = H.BATCHED_CASE
    g = torch.Generator().manual_seed(4242)
    a = torch.randn(M, batch * K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, batch * K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    ldc, gap = N + 8, 3
    buf = sentinel(batch * (M + gap), ldc)
    H.gemm_batched(a, batch * K, K, w, batch * K, K, buf, ldc, (M + gap) * ldc, M, N, K, batch)
    cz = buf.view(batch, M + gap, ldc)
    assert bool((cz[:, M:] == SENT).all()) and bool((cz[:, :, N:] == SENT).all())
    zero = torch.zeros(N, device=DEV)
    res = {}
    for z in range(batch):
        az, wz = a[:, z * K:(z + 1) * K], w[:, z * K:(z + 1) * K]
        res.update(linear_ratios(az, wz, zero, {f"C_{z}": (cz[z, :M], "pre")}))
    report(f"batched {H.BATCHED_CASE}", res)
    one = H.gemm_batched(a, batch * K, K, w, batch * K, K, sentinel(M, ldc), ldc, M * ldc, M, N, K, 1)
    selected((M, N, K), "skinny")
    assert torch.equal(one, H.gemm(a[:, :K], w[:, :K], None, epi=0, out=sentinel(M, ldc)))


# ---- the LN fold


@functools.lru_cache(maxsize=None)
def fold_operands(M, N, K):
    """hipops.spiked_fold_case on the device, x and W' in NaN-padded buffers, + the fp64 statistics rounded to fp32."""
    ops = [t.to(DEV) for t in H.spiked_fold_case(M, N, K)]
    ops[0], ops[1] = pitched(ops[0]), pitched(ops[1])
    return tuple(ops), H.stats64(ops[0])


FOLD_NAME = {0: "fold bias", 1: "fold gelu erf", 2: "fold gelu tanh"}


def run_fold(shape):
    M, N, K = shape
    ops, st = fold_operands(M, N, K)
    x, wg, cvec, colsum = ops[:4]
    outs = {FOLD_NAME[epi]: (H.gemm_ln(x, wg, cvec, colsum, st, epi=epi, out=sentinel(M, N + 8)), epi) for epi in (0, 1, 2)}
    for name, (out, _) in outs.items():
        assert padding_kept(out, N), (shape, name)
    return ops, st, outs


@pytest.mark.parametrize("shape", H.FOLD_SHAPES + [H.FOLD_CLEAN_ONLY])
def test_ln_fold_within_fold_bound(shape):
    """Epilogues 0, 1, 2 of ov_gemm_ln in the skinny and plain kernels on spiked inputs (hipops.spiked_fold_case), under fold_bound."""
    kernel = "plain" if shape in H.PLAIN_SHAPES else "skinny"
    for epi in (0, 1, 2):
        selected(shape, kernel, epi, fold=True)
    ops, st, outs = run_fold(shape)
    report(f"{kernel} {shape} LN fold", fold_ratios_bound(ops[0], ops[1], ops[3], ops[2], st, outs))


def test_ln_fold_persistent_within_both_rules():
    """Case 1 of the routes table (the persistent kernel, K = 192) on the spiked inputs: fold_bound, and beside it the tuned rule."""
    for epi in (0, 1, 2):
        shape = RT.selected(1, epi, fold=True)
    ops, st, outs = run_fold(shape)
    report(f"persistent {shape} LN fold", fold_ratios_bound(ops[0], ops[1], ops[3], ops[2], st, outs))
    report(f"persistent {shape} LN fold, tuned rule", ln_linear_ratios(ops, outs))


# ---- row statistics from the residual epilogue

E32 = H.E32


@pytest.mark.parametrize("shape", H.ROWPARTS_SHAPES)
def test_rowparts_output_and_sums(shape):
    """ov_gemm_rowparts in place, N / 32 odd: the output under the residual bound; parts bitwise ov_rowparts(output) -- the skinny
    kernel computes them in its epilogue, the plain kernel is followed by that pass -- and each {sum, sum of squares} within
    32 e sum|c| resp. 32 e sum c^2 of the fp64 sums of the stored bf16 values (a 32-term fp32 sum in any order; the bf16 products
    are exact in fp32); the word behind the parts buffer survives."""
    M, N, K = selected(shape, "plain" if shape[0] > 2000 else "skinny", 3, rowparts=True)
    assert (N // 32) % 2 == 1
    a, w, bias, r = operands(M, N, K)
    buf = sentinel(M, N + 8)
    buf[:, :N] = r
    flat = torch.full((M * (N // 32) * 2 + 4,), SENT, dtype=torch.float32, device=DEV)
    parts = flat[:-4].view(M, N // 32, 2)
    H.gemm_rowparts(a, w, bias, buf, out=buf, parts=parts)
    report(f"rowparts {shape}", linear_ratios(a, w, bias, {"residual": (buf, "res")}, r))
    assert padding_kept(buf, N) and bool((flat[-4:] == SENT).all())
    assert torch.equal(parts, H.rowparts(buf[:, :N]))
    c = buf[:, :N].double().reshape(M, N // 32, 32)
    for j, (want, mag) in enumerate(((c.sum(-1), c.abs().sum(-1)), ((c * c).sum(-1), (c * c).sum(-1)))):
        q = float(((parts[..., j].double() - want).abs() / (32 * E32 * mag)).max())
        print(f"rowparts {shape} {('sum', 'sum of squares')[j]}: max err / bound {q:.3f}")
        assert q <= 1.0, (shape, j, q)


def test_rowparts_refuses_n_not_a_multiple_of_32():
    M, N, K = 257, 264, 256
    a, w, bias, r = operands(M, N, K)
    with pytest.raises(H._lib.OvhipError, match=r"status -2\b"):
        H.gemm_rowparts(a, w, bias, r, parts=torch.empty(M, N // 32, 2, device=DEV))
