"""The kernels that move and update state around the compute -- ov_adamw_step and ov_sumsq (optim.hip), ov_im2col_patches(_keep),
ov_patch_keep_inverse / _assemble / _assemble_backward, ov_col2im_patches_keep, ov_text_embed and ov_convert (embed.hip) -- bit for bit
against comparands that know nothing of their code.

Their right answers are known to the bit, so every assertion here is an equality of bit patterns, with one exception.
  * ov_adamw_step against oracle/optim_ref.adamw_step, given what the kernel is given: the betas rounded to fp32 as the C ABI carries
    them, the global norm as sqrt(fp32 gnorm_sq) x fp32 grad_scale.  (With Python-double betas the oracle forms 1 - b from the
    double; the kernel forms it from the fp32 b: the known deviation of DESIGN.md, which test_optim_glue_cpu.py shows this
    equality sees.)  The n & 3 tail alone, the vector path with and without a tail, the second grid-stride lap, steps 1 .. 100000,
    four beta pairs, wd, lr = 0, eps = 0, three gradient scales, clipping above / below / at a zero norm, exact bf16 ties of both
    parities for the stored moment, subnormal squares, mu at an 8-byte address; guard elements behind every state buffer.
  * ov_sumsq (a) on integers whose every partial sum is exact in any order: the result is the integer, to the bit; (b) on Gaussian
    data against the fp64 sum under gam(L) sum g^2, L the longest chain of fp32 roundings a square passes through
    (hipops.sumsq_chain_length; DESIGN.md derives it): the one inequality of this file, its ratio printed.
  * the glue against torch on the CPU: F.unfold, indexing, an fp32 add, .to(bfloat16).  Operands in NaN-padded pitched buffers,
    outputs prefilled (NaN or the sentinel 77) with guard rows / columns that must stay; geometries whose 16-byte chunks and
    four-pixel groups straddle the operand's end and a patch boundary (P = 14), the second grid-stride lap of each, token ids
    outside the table and beyond int32, every bf16 tie through ov_convert.

What these equalities can tell apart is pinned without a GPU by test_optim_glue_cpu.py, on the same inputs (hipops's tables)."""
import numpy as np
import pytest
import torch

import hipops as H
from hipops import DEV, SENT, pitched, sentinel, padding_kept
from openvision_amd import _lib

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


def scalar(v):
    return torch.full((1,), float(v), dtype=F32, device=DEV)


def guarded(rows, cols, dtype, fill=NAN):
    """[rows + 1, cols] holding `fill`; the last row is a guard that must keep it (all_nan / the caller checks)."""
    return torch.full((rows + 1, cols), fill, dtype=dtype, device=DEV)


def all_nan(t):
    return bool(torch.isnan(t).all())


# ------------------------------------------------------------------------------------------------------------------------------
# ov_adamw_step


def run_adam(c, x, gn_sq):
    st = H.AdamState(x, c.mu_off)
    gn = None if gn_sq is None else scalar(gn_sq)
    for i, g in enumerate(x.g):
        st.step(g, c, c.t0 + i, gn)
    if gn is not None:
        assert H.same_bits(gn, torch.tensor([gn_sq], dtype=F32)), "gnorm_sq was written"
    return st.read()


@pytest.mark.parametrize("c", H.ADAM_CASES, ids=H.adam_id)
def test_adamw_step_is_the_oracle_bit_for_bit(c):
    x = H.adam_inputs(c)
    ref = H.adam_ref(c, x)
    got = run_adam(c, x, H.adam_gnorm_sq(c))
    for k in ("p", "mu", "nu"):
        print(f"{H.adam_id(c)} {k}: {int((H.bits(got[k]) != H.bits(ref[k])).sum())} of {c.n} elements differ in their bits")
    assert H.same_outputs(got, ref) == []
    if c.lr == 0:
        assert H.same_bits(got["p"], torch.from_numpy(x.p)) and not H.same_bits(got["nu"], torch.from_numpy(x.nu))
    if c.clip in ("below", "zero"):
        assert H.same_outputs(run_adam(c, x, None), got) == [], "a clip factor of exactly 1 is not the call without clipping"


def test_adamw_step_chained_to_sumsq_over_two_groups():
    """ov_sumsq(g0, accumulate = 0) then ov_sumsq(g1, accumulate = 1) into a NaN-prefilled scalar, which both groups' updates read
    through its pointer; the oracle is given the scalar as read back."""
    cases = [H._ac(n, gs=0.5, clip="above", seed=s) for n, s in zip(H.ADAM_CHAIN, (1, 2))]
    xs = [H.adam_inputs(c) for c in cases]
    gn = scalar(NAN)
    for i, x in enumerate(xs):
        H.sumsq(torch.from_numpy(x.g[0]).to(DEV), gn, accumulate=int(i > 0))
    gn_sq = np.float32(gn.cpu().numpy()[0])
    print(f"chained gnorm_sq = {float(gn_sq)!r}")
    assert np.sqrt(gn_sq) * np.float32(0.5) > H.CLIP_NORM                      # the clip acts
    for c, x in zip(cases, xs):
        st = H.AdamState(x)
        st.step(x.g[0], c, c.t0, gn)
        assert H.same_outputs(st.read(), H.adam_ref(c, x, gn_sq=gn_sq)) == [], c.n
    assert H.same_bits(gn, torch.tensor([gn_sq]))


# ------------------------------------------------------------------------------------------------------------------------------
# ov_sumsq


@pytest.mark.parametrize("n", H.SUMSQ_INT_N)
def test_sumsq_counts_every_element_once(n):
    g, total = H.sumsq_int_case(n)
    gd = torch.from_numpy(g).to(DEV)
    fresh = H.sumsq(gd, scalar(NAN), accumulate=0)
    added = H.sumsq(gd, scalar(H.SUMSQ_PRIOR), accumulate=1)
    print(f"sumsq n = {n}: {float(fresh)} (want {total}), onto {H.SUMSQ_PRIOR}: {float(added)}")
    assert H.same_bits(fresh, torch.tensor([float(total)], dtype=F32))
    assert H.same_bits(added, torch.tensor([float(total) + H.SUMSQ_PRIOR], dtype=F32))
    assert H.same_bits(gd, torch.from_numpy(g))


def test_sumsq_gaussian_within_its_chain_bound():
    n = H.SUMSQ_NORMAL_N
    g = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    exact = float((g.astype(np.float64) ** 2).sum())
    got = float(H.sumsq(torch.from_numpy(g).to(DEV), scalar(NAN)))
    L = H.sumsq_chain_length(n, 0)
    q = abs(got - exact) / (H.gam(L) * exact)
    print(f"sumsq n = {n}: L = {L}, |err| / (gam(L) sum g^2) = {q:.4f}")
    assert q <= 1.0, (got, exact, L)


# ------------------------------------------------------------------------------------------------------------------------------
# embed.hip


def run_im2col(img, P, Kpad, keep=None):
    g = img.shape[2] // P
    rows = img.shape[0] * (g * g if keep is None else keep.shape[1])
    buf = guarded(rows, Kpad, BF16)
    if keep is None:
        H.im2col_patches(img.to(DEV), P, buf[:rows])
    else:
        H.im2col_patches_keep(img.to(DEV), keep.to(DEV), P, buf[:rows])
    assert all_nan(buf[rows:]), "written past the last row"
    return buf[:rows].cpu()


@pytest.mark.parametrize("S,P,Kpad", H.IM2COL_GEOM)
def test_im2col_patches(S, P, Kpad):
    for B in (1, 3):
        for dtype in (F32, BF16):
            img = H.image_case(B, S, dtype)
            assert H.same_bits(run_im2col(img, P, Kpad), H.im2col_ref(img, P, Kpad)), (B, dtype)


def test_im2col_patches_second_lap():
    B, S, P, Kpad = H.IM2COL_LAP
    img = H.image_case(B, S, BF16)
    assert H.same_bits(run_im2col(img, P, Kpad), H.im2col_ref(img, P, Kpad))


@pytest.mark.parametrize("S,P,Kpad", H.KEEP_GEOM)
def test_im2col_patches_keep(S, P, Kpad):
    G = (S // P) ** 2
    for K in H.keep_ks(G):
        for dtype in (F32, BF16):
            img, keep = H.image_case(3, S, dtype), H.keep_table(3, G, K)
            assert H.same_bits(run_im2col(img, P, Kpad, keep), H.gather_keep(H.im2col_ref(img, P, Kpad), keep, G)), (K, dtype)


def run_inverse(keep, G):
    inv = torch.full((keep.shape[0] + 1, G), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(H.patch_keep_inverse(keep.to(DEV), inv[:-1], G, err), "ov_patch_keep_inverse")
    assert bool((inv[-1] == -7).all())
    return inv[:-1].cpu(), int(err)


@pytest.mark.parametrize("G", H.INVERSE_G)
def test_patch_keep_inverse(G):
    for K in (1, G):
        keep = H.keep_table(3, G, K)
        inv, flag = run_inverse(keep, G)
        assert H.same_bits(inv, H.inverse_ref(keep, G)) and flag == 0, (G, K)
    for wrong in (-1, G, H.INT_MAX):
        keep = H.keep_table(3, G, min(G, 4))
        keep[1, 0] = wrong
        inv, flag = run_inverse(keep, G)
        assert flag == 1, (G, wrong)
        assert H.same_bits(inv[[0, 2]], H.inverse_ref(keep[[0, 2]], G))           # the clean images' maps are whole
    keep = H.keep_table(3, G, min(G, 4))
    keep[2, 1] = keep[2, 0]
    assert run_inverse(keep, G)[1] == 1, "a duplicate index raised no flag"


def test_patch_keep_inverse_refuses_what_its_lds_cannot_hold():
    keep = H.keep_table(1, 16385, 4).to(DEV)
    inv = torch.full((1, 16385), -7, dtype=torch.int32, device=DEV)
    assert H.patch_keep_inverse(keep, inv, 16385, None) == -2                      # OV_ERR_UNSUPPORTED
    assert bool((inv == -7).all())


@pytest.mark.parametrize("D", H.ASSEMBLE_D)
def test_patch_keep_assemble(D):
    for G, K in ((4, 1), (16, 8), (16, 16)):
        c = H.assemble_case(3, G, K, D)
        rows = c.B * (1 + K)
        buf = guarded(rows, D, F32)
        H.patch_keep_assemble(pitched(c.y.to(DEV)), c.cls.to(DEV), c.pos.to(DEV), c.keep.to(DEV), buf[:rows], G)
        assert all_nan(buf[rows:])
        assert H.same_bits(buf[:rows].view(c.B, 1 + K, D), H.assemble_ref(c)), (G, K, D)


@pytest.mark.parametrize("B", H.ASSEMBLE_BWD_B)
def test_patch_keep_assemble_backward(B):
    for G, K, D in ((16, 8, 8), (16, 16, 192), (4, 1, 1152)):
        c = H.assemble_bwd_case(B, G, K, D)
        ref = H.assemble_bwd_ref(c)
        dx, inv = c.dx.to(DEV), c.inv.to(DEV)
        for want in (("dpos",), ("dcls",), ("dy",), ("dpos", "dcls", "dy")):
            dpos, dcls, dy = guarded(1 + G, D, F32), guarded(1, D, F32), sentinel(B * K, D + 8)
            H.patch_keep_assemble_backward(dx, inv, K, dpos[:-1] if "dpos" in want else None, dcls[0] if "dcls" in want else None,
                                           dy[:, :D] if "dy" in want else None)
            got = dict(dpos=dpos[:-1], dcls=dcls[0], dy=dy[:, :D])
            for k in ("dpos", "dcls", "dy"):
                if k in want:
                    assert H.same_bits(got[k], ref[k]), (B, G, K, D, want, k)
                else:
                    assert all_nan(got[k]) if k != "dy" else bool((got[k] == SENT).all()), (want, k, "written though not asked for")
            assert all_nan(dpos[-1]) and all_nan(dcls[1]) and padding_kept(dy, D)
        assert H.same_bits(dx, c.dx)


@pytest.mark.parametrize("S,P", H.COL2IM_GEOM)
def test_col2im_patches_keep(S, P):
    G = (S // P) ** 2
    for K in (1, G):
        for dtype in (F32, BF16):
            c = H.col2im_case(3, S, P, K)
            n = c.B * 3 * S * S
            buf = torch.full((n + H.GUARD,), NAN, dtype=dtype, device=DEV)
            H.col2im_patches_keep(pitched(c.dcols.to(DEV)), c.inv.to(DEV), buf[:n].view(c.B, 3, S, S), P, K)
            assert all_nan(buf[n:])
            assert H.same_bits(buf[:n].view(c.B, 3, S, S), H.col2im_ref(c, dtype)), (S, P, K, dtype)


def run_text(c):
    rows = c.B * c.T
    x = sentinel(rows, c.D + 8)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    H.text_embed(c.tokens.to(DEV), c.table.to(DEV), c.pos.to(DEV), x[:, :c.D], err)
    assert padding_kept(x, c.D)
    return dict(x=x[:, :c.D].cpu(), err=err.cpu())


@pytest.mark.parametrize("B,T,D,V", H.TEXT_CASES + [H.TEXT_LAP])
def test_text_embed(B, T, D, V):
    for bad in (False, True):
        if bad and B * T < 5:
            continue
        c = H.text_case(B, T, D, V, bad=bad)
        assert H.same_outputs(run_text(c), H.text_ref(c)) == [], (B, T, D, V, bad)
    c = H.text_case(B, T, D, V)
    x = sentinel(B * T, D + 8)
    H.text_embed(c.tokens.to(DEV), c.table.to(DEV), c.pos.to(DEV), x[:, :D], None)          # no flag asked for
    assert H.same_bits(x[:, :D], H.text_ref(c)["x"])


def run_convert(src, dst_dtype):
    rows, cols = src.shape
    dst = torch.full((rows, cols + 8), SENT, dtype=dst_dtype, device=DEV)
    H.convert(pitched(src.to(DEV)), dst[:, :cols])
    assert bool((dst[:, cols:] == SENT).all()), "a gap column was written"
    return dst[:, :cols].cpu()


@pytest.mark.parametrize("cols", H.CONVERT_COLS)
def test_convert_every_pattern(cols):
    for sd, dd in H.DTYPE_PAIRS:
        src = H.convert_case(H.convert_rows(cols, sd), cols, sd)
        assert H.same_bits(run_convert(src, dd), src.to(dd), nan_ok=True), (cols, sd, dd)


def test_convert_second_lap():
    rows, cols = H.CONVERT_LAP
    for sd, dd in H.DTYPE_PAIRS:
        src = H.convert_case(rows, cols, sd)
        assert H.same_bits(run_convert(src, dd), src.to(dd), nan_ok=True), (sd, dd)
