"""GPU: the gradient-ascent loop on HIP (csrc/ascent.hip, openvision_amd.gradient_ascent.GradientAscent and its command line).  The five
kernels alone first, each against the restatement in ascent_restate.py -- bit for bit where the arithmetic is exact, else within a
bound written from the operations the kernel performs (u = 2^-24) -- then one step and a free run on vit-tiny-patch16-160 against the
eager soft-token composition the loop replaces (training.encode_text on soft one-hot rows + autograd + torch.optim.Adam), and the
command line.  Every buffer a kernel writes or reads stands between guard words."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ascent_restate as A
from openvision_amd import _lib, checkpoint, gradient_ascent as ga, preset, synth, training
from openvision_amd._lib import ptr, stream_ptr
from openvision_amd.gradient_ascent import GradientAscent
from openvision_amd.model import create_model
from ranks import run_child

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = A.U
GUARD = 64                      # elements in front of and behind every buffer
MEAN, STD = torch.tensor([0.48145466, 0.4578275, 0.40821073]), torch.tensor([0.26862954, 0.26130258, 0.27577711])


class Guarded:
    """A device buffer of `shape` between two runs of GUARD sentinel elements; `t` is the view the kernels get: 16-byte aligned, or
    `shift` elements past that (a step's row inside a packed table)."""

    def __init__(self, shape, dtype=torch.float32, fill=None, shift=0):
        n = int(np.prod(shape))
        self.sent = 1234.5 if dtype.is_floating_point else 12345
        self.lo = GUARD + shift
        self.buf = torch.full((self.lo + n + GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool((self.buf[:self.lo] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())


def _sync():
    torch.cuda.synchronize()


# ---- 1. ov_ga_affine -------------------------------------------------------------------------------------------------------------------
def _case_mats(size, batch, g):
    """identity | integer shift | +10 deg | -10 deg with a fractional shift | everything outside, then host draws up to `batch` rows."""
    z = torch.zeros((), dtype=torch.float64)
    cases = [(False, 0.0, 0.0, 0.0), (True, 0.0, 3.0, -2.0), (True, 10.0, 0.0, 0.0), (True, -10.0, 1.25, -0.75), (True, 0.0, 3.0 * size, 0.0)]
    rows = [ga.inverse_matrices(torch.tensor(a), z + d, z + x, z + y, size) for a, d, x, y in cases]
    u = torch.rand(max(batch - 5, 0), 4, generator=g, dtype=torch.float64)
    rows += list(ga.inverse_matrices(u[:, 0] < 0.8, (2 * u[:, 1] - 1) * 10, (2 * u[:, 2] - 1) * 0.1 * size, (2 * u[:, 3] - 1) * 0.1 * size, size))
    return torch.stack(rows).float()


@pytest.mark.parametrize("size", [20, 35])
@pytest.mark.parametrize("batch", [1, 13])
def test_affine_identity_and_shift_bitwise_rotations_within_bound(size, batch):
    """Bound of a rotated pixel.  sx = (a0 x + a1 y) + a2 is four roundings on terms of magnitude mag_x = |a0 x| + |a1 y| + |a2|: |delta
    sx| <= 4 u mag_x, and the bilinear surface has slope <= 1 per pixel (values and the zero padding lie in [0, 1]), also across a
    floor that flips.  The weights' differences are exact; four weight products, four tap products and three additions on weights that
    sum to 1: <= 8 u.  Then (v - mean) / std: |delta| <= (4 u (mag_x + mag_y) + 8 u) / std + 3 u |out|."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(size * 100 + batch)
    img = torch.rand(3, size, size, generator=g)
    allm = _case_mats(size, 13, g)
    calls = [allm] if batch == 13 else [allm[i:i + 1] for i in range(5)]
    gi, gm, gs = Guarded(img.shape, fill=img), Guarded((3,), fill=MEAN), Guarded((3,), fill=STD)
    norm = (img - MEAN.view(3, 1, 1)) / STD.view(3, 1, 1)
    outside = ((0 - MEAN) / STD).view(3, 1, 1)
    for ci, mats in enumerate(calls):
        gt = Guarded(mats.shape, fill=mats, shift=ci % 3)             # a step's row of the packed table: 4-byte aligned
        out, outb = Guarded((mats.shape[0], 3, size, size)), Guarded((mats.shape[0], 3, size, size), torch.bfloat16)
        _lib.check(lib.ov_ga_affine(ptr(gi.t), ptr(gt.t), ptr(gm.t), ptr(gs.t), ptr(out.t), _lib.OV_F32, mats.shape[0], size, stream_ptr()), "f32")
        _lib.check(lib.ov_ga_affine(ptr(gi.t), ptr(gt.t), ptr(gm.t), ptr(gs.t), ptr(outb.t), _lib.OV_BF16, mats.shape[0], size, stream_ptr()), "bf16")
        _sync()
        assert out.intact() and outb.intact() and gi.intact() and gt.intact() and gm.intact() and gs.intact()
        got = out.t.cpu()
        assert torch.equal(outb.t.cpu().view(torch.int16), got.to(torch.bfloat16).view(torch.int16))
        want32 = A.affine(img, mats, MEAN, STD)                        # the fp32 form: the kernel's operations in its order
        want = A.affine(img.double(), mats, MEAN.double(), STD.double())
        _, _, mag_x, mag_y = A.affine_source(mats, size)
        bound = (4 * U * (mag_x + mag_y) + 8 * U).unsqueeze(1) / STD.double().view(1, 3, 1, 1) + 3 * U * want.abs()
        ratio = ((got.double() - want).abs() / bound).max().item()
        print(f"affine s{size} b{batch} call {ci}: worst |err| / bound = {ratio:.3f}; equals the fp32 form: {torch.equal(got, want32)}")
        assert ratio <= 1.0
        for r in range(mats.shape[0]):
            kind = ci if batch == 1 else r
            if kind == 0 or (kind >= 5 and torch.equal(mats[r], torch.tensor([1.0, 0, 0, 0, 1.0, 0]))):
                assert torch.equal(got[r], norm), (size, batch, r)
            if kind == 1:                                              # destination (y, x) reads source (y + 2, x - 3)
                assert torch.equal(got[r][:, : size - 2, 3:], norm[:, 2:, : size - 3])
                assert torch.equal(got[r][:, :, :3], outside.expand(3, size, 3))
                assert torch.equal(got[r][:, size - 2:, :], outside.expand(3, 2, size))
            if kind == 4:
                assert torch.equal(got[r], outside.expand(3, size, size))


# ---- 2. ov_ga_sample -------------------------------------------------------------------------------------------------------------------
# (R, V, K, T)
SAMPLE_SHAPES = [(1, 33, 1, 3), (52, 1000, 4, 7), (65, 257, 5, 9), (4, 32000, 4, 80)]


def _sample_inputs(r, v, seed):
    g = torch.Generator().manual_seed(seed)
    normu = torch.zeros(r, v).normal_(generator=g)
    e = torch.empty(r, v).exponential_(generator=g)
    return normu, e


@pytest.mark.parametrize("tau", [1.0, 1000.0])
@pytest.mark.parametrize("shape", SAMPLE_SHAPES, ids=lambda s: f"r{s[0]}_v{s[1]}")
def test_sample_index_maximum_and_sum(shape, tau):
    """The reference: z = (normu - log e) / tau in fp32 on the host (the correctly rounded logarithm, the rest IEEE), ys =
    softmax(z).  zsum against sum exp(z - zmax) in fp64 on that z: the subtraction rounds once (relative u: an absolute u |z - zmax|
    in the exponent), expf is within 1 ulp = 2 u, a thread adds ceil(V / 1024) terms, then 6 butterfly steps and 15 additions:
    relative (max |z - zmax| + ceil(V / 1024) + 24) u.  The stored z is the reference's bit for bit."""
    r, v, k, t = shape
    lib = _lib.load()
    normu, e = _sample_inputs(r, v, 7 * r + v)
    gn, ge = Guarded(normu.shape, fill=normu), Guarded(e.shape, fill=e)
    z = A.gumbel_z(normu, e, tau)
    ys = z.softmax(-1)
    top2 = ys.topk(2, dim=-1).values
    assert bool((top2[:, 0] != top2[:, 1]).all())                      # the condition on the inputs: no tie among the reference's ys
    want_idx = ys.max(-1)[1]
    assert torch.equal(want_idx, z.max(-1)[1])
    idx, zmax, zsum, zbuf = Guarded((r,), torch.int32), Guarded((r,)), Guarded((r,)), Guarded((r, v))
    hist = Guarded((3, r), torch.int32, shift=1)
    ids = Guarded((r // k, t), torch.int64, fill=torch.full((r // k, t), 777, dtype=torch.int64))
    row = _lib.c_void_p(hist.t.data_ptr() + r * 4)
    _lib.check(lib.ov_ga_sample(ptr(gn.t), ptr(ge.t), tau, r, v, k, t, ptr(zbuf.t), ptr(idx.t), ptr(zmax.t), ptr(zsum.t), row, ptr(ids.t),
                                stream_ptr()), "ov_ga_sample")
    _sync()
    assert all(b.intact() for b in (gn, ge, idx, zmax, zsum, zbuf, hist, ids))
    assert torch.equal(zbuf.t.cpu().view(torch.int32), z.view(torch.int32))
    assert torch.equal(idx.t.cpu().long(), want_idx)
    assert torch.equal(zmax.t.cpu().view(torch.int32), z.max(-1)[0].view(torch.int32))
    z64 = z.double()
    want_sum = (z64 - z64.max(-1, keepdim=True)[0]).exp().sum(-1)
    spread = (z64.max(-1)[0] - z64.min(-1)[0])
    bound = (spread + math.ceil(v / 1024) + 24) * U * want_sum
    err = (zsum.t.cpu().double() - want_sum).abs()
    print(f"sample r{r} v{v} tau {tau}: zsum worst |err| / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    h = hist.t.cpu()
    assert torch.equal(h[1].long(), want_idx) and bool((h[0] == hist.sent).all()) and bool((h[2] == hist.sent).all())
    m = ids.t.cpu()
    assert torch.equal(m[:, t - k:], want_idx.view(r // k, k)) and bool((m[:, : t - k] == 777).all())
    # without a history row and an id matrix: the three outputs alone
    idx2 = Guarded((r,), torch.int32)
    _lib.check(lib.ov_ga_sample(ptr(gn.t), ptr(ge.t), tau, r, v, 0, 0, ptr(zbuf.t), ptr(idx2.t), ptr(zmax.t), ptr(zsum.t), None, None, stream_ptr()),
               "plain")
    _sync()
    assert torch.equal(idx2.t.cpu().long(), want_idx) and idx2.intact()


# ---- 3. ov_ga_token_grad + ov_ga_adam --------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(1, 33, 64), (52, 1000, 192), (64, 257, 64), (65, 130, 128), (4, 32000, 64)]
LR, BETAS, EPS = 5.0, (0.9, 0.999), 1e-8


def _run_grad_adam(lib, state, dxs, tau, debug=True):
    """Three steps (sample, token_grad, adam) on copies of `state` = (normu, e, w); returns per step what the kernels wrote."""
    normu0, e, w = state
    r, v = normu0.shape
    d = w.shape[1]
    nblk = lib.ov_ga_parts_blocks(v)
    assert nblk == (v + 127) // 128
    gn, ge, gw = Guarded((r, v), fill=normu0), Guarded((r, v), fill=e), Guarded((v, d), torch.bfloat16, fill=w)
    ea, es = Guarded((r, v), fill=torch.zeros(r, v)), Guarded((r, v), fill=torch.zeros(r, v))
    idx, zmax, zsum, zbuf = Guarded((r,), torch.int32), Guarded((r,)), Guarded((r,)), Guarded((r, v))
    gy, parts, g = Guarded((r, v)), Guarded((r, nblk)), Guarded((r, v))
    out = []
    for t, dx in enumerate(dxs, start=1):
        gd = Guarded((r, d), torch.bfloat16, fill=dx)
        before = (gn.t.cpu().clone(), ea.t.cpu().clone(), es.t.cpu().clone())
        _lib.check(lib.ov_ga_sample(ptr(gn.t), ptr(ge.t), tau, r, v, 0, 0, ptr(zbuf.t), ptr(idx.t), ptr(zmax.t), ptr(zsum.t), None, None,
                                    stream_ptr()), "sample")
        _lib.check(lib.ov_ga_token_grad(ptr(gd.t), ptr(gw.t), ptr(zbuf.t), ptr(zmax.t), ptr(zsum.t), r, v, d, ptr(gy.t), ptr(parts.t),
                                        stream_ptr()), "ov_ga_token_grad")
        _lib.check(lib.ov_ga_adam(ptr(gy.t), ptr(parts.t), ptr(gn.t), ptr(zbuf.t), ptr(zmax.t), ptr(zsum.t), tau, r, v, ptr(ea.t), ptr(es.t),
                                  LR, BETAS[0], BETAS[1], EPS, 1 - BETAS[0] ** t, 1 - BETAS[1] ** t, ptr(g.t) if debug else None, stream_ptr()),
                   "ov_ga_adam")
        _sync()
        assert all(b.intact() for b in (gn, ge, gw, ea, es, idx, zmax, zsum, zbuf, gy, parts, g, gd)), t
        out.append(dict(before=before, gy=gy.t.cpu().clone(), parts=parts.t.cpu().clone(), g=g.t.cpu().clone(), p=gn.t.cpu().clone(),
                        ea=ea.t.cpu().clone(), es=es.t.cpu().clone()))
    return out


@pytest.mark.parametrize("scale", [1e-3, 1e3])
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: f"r{s[0]}_v{s[1]}_d{s[2]}")
def test_token_grad_and_adam_against_fp64(shape, scale):
    """tau = 1000 (the script's), and tau = 1 at the smallest shape.  With mag = sum_d |dx||w| (bf16 operands, exact products):
      gy   |err| <= gamma_D mag                                                  D fp32 additions in whatever order the MFMA takes
      ys   relative eps_ys <= 2 dz + (spread + ceil(V/1024) + 24) u + 4 u        dz = 4 u max(|normu| + |log e|) / tau bounds the fp32 z
                                                                                 against the fp64 one (log 1 ulp, -, /); then the exponent's
                                                                                 error twice (numerator, sum), zsum's bound of the sample
                                                                                 test, expf's 2 u, the division and ys's own rounding
      c    |err| <= sum_v (gamma_D mag + |gy| (eps_ys + (nblk + 8) u)) ys         products, 5 butterfly steps + 2 + nblk additions
      g    |err| <= ys (E_gy + E_c) / tau + |g| (eps_ys + 4 u)                    the subtraction, the product, the division
    The parameters: one step of the fp64 Adam from the kernel's own previous state on the gradient the kernel reports, the scalars
    rounded to float as the kernel holds them.  ea' = ea + w (g - ea): 3 u (|ea| + |g|); es' = es b2 + (w2 g) g, all terms positive:
    3 u es'; denom = sqrt(es') / c + eps: (1.5 + 1 + 1 + 1) u relative; ea' / denom, the product with the step size, the subtraction:
    |err p'| <= u |p'| + step (3 u (|ea| + |g|) + 8 u |ea'|) / denom."""
    r, v, d = shape
    lib = _lib.load()
    g = torch.Generator().manual_seed(r * 7 + v + d)
    normu0, e = _sample_inputs(r, v, r + v + d)
    w = (torch.randn(v, d, generator=g) * 0.5).to(torch.bfloat16)
    dxs = [(torch.randn(r, d, generator=g) * scale * (1 + t)).to(torch.bfloat16) for t in range(3)]
    taus = [1000.0] + ([1.0] if v == 33 else [])
    for tau in taus:
        runs = [_run_grad_adam(lib, (normu0, e, w), dxs, tau) for _ in range(2)]
        for a, b in zip(*runs):                                        # no atomics: two runs agree bit for bit
            for key in ("gy", "parts", "g", "p", "ea", "es"):
                assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key
        quiet = _run_grad_adam(lib, (normu0, e, w), dxs, tau, debug=False)
        assert bool((quiet[-1]["g"] == 1234.5).all()) and torch.equal(quiet[-1]["p"], runs[0][-1]["p"])      # g skipped, same update
        nblk = (v + 127) // 128
        seen = []
        for t, (dx, got) in enumerate(zip(dxs, runs[0]), start=1):
            p0, ea0, es0 = [x.double() for x in got["before"]]
            z64 = A.gumbel_z(p0, e.double(), tau)
            _, _, _, ys = A.sample(z64)
            gy64, c64, g64 = A.token_grad(dx.double(), w.double(), ys, tau)
            mag = dx.double().abs() @ w.double().abs().t()
            e_gy = A.gamma(d) * mag
            assert ((got["gy"].double() - gy64).abs() <= e_gy).all(), (shape, tau, t)
            dz = 4 * U * (p0.abs() + e.double().log().abs()).max(-1, keepdim=True)[0] / tau
            spread = z64.max(-1, keepdim=True)[0] - z64.min(-1, keepdim=True)[0]
            eps_ys = 2 * dz + (spread + math.ceil(v / 1024) + 24) * U + 4 * U
            e_c = ((e_gy + gy64.abs() * (eps_ys + (nblk + 8) * U)) * ys).sum(-1, keepdim=True)
            e_g = ys * (e_gy + e_c) / tau + g64.abs() * (eps_ys + 4 * U)
            ratio = ((got["g"].double() - g64).abs() / e_g).max().item()
            c_got = got["parts"].double().sum(-1, keepdim=True)
            assert ((c_got - c64).abs() <= e_c + nblk * U * (gy64.abs() * ys).sum(-1, keepdim=True)).all()
            # Adam, one step in fp64 from the kernel's state on the kernel's gradient
            k32 = A.adam_constants(t, LR, BETAS, EPS, torch.float32)
            k64 = {n: x.double() for n, x in k32.items()}
            gk = got["g"].double()
            p64, ea64, es64 = A.adam_step(p0, gk, ea0, es0, k64)
            denom = es64.sqrt() / k64["bc2_sqrt"] + k64["eps"]
            assert ((got["ea"].double() - ea64).abs() <= 3 * U * (ea0.abs() + gk.abs())).all()
            assert ((got["es"].double() - es64).abs() <= 3 * U * es64).all()
            e_p = U * p64.abs() + k64["step"] * (3 * U * (ea0.abs() + gk.abs()) + 8 * U * ea64.abs()) / denom
            p_ratio = ((got["p"].double() - p64).abs() / e_p).max().item()
            print(f"grad {shape} tau {tau} scale {scale} t={t}: |g| in [{g64.abs().min():.2e}, {g64.abs().max():.2e}], worst |err g| / bound "
                  f"= {ratio:.3f}, |err p| / bound = {p_ratio:.3f}")
            assert ratio <= 1.0 and p_ratio <= 1.0
            assert not torch.equal(got["p"], got["before"][0])
            seen.append(float(g64.abs().max()))
        if tau == 1000.0:
            assert (max(seen) < EPS) if scale < 1 and v == 32000 else True         # below Adam's eps at the script's vocabulary ...
            assert (max(seen) > EPS) if scale > 1 else True                          # ... and above it at the large scale


def test_token_grad_refuses_what_it_does_not_build():
    lib = _lib.load()
    a = Guarded((256,), torch.bfloat16)
    f = Guarded((256,))
    args = lambda d: (ptr(a.t), ptr(a.t), ptr(f.t), ptr(f.t), ptr(f.t), 1, 2, d, ptr(f.t), ptr(f.t), stream_ptr())
    assert lib.ov_ga_token_grad(*args(32)) == -2 and lib.ov_ga_token_grad(*args(72)) == -2
    assert lib.ov_ga_token_grad(None, *args(64)[1:]) == -1
    assert lib.ov_ga_cosine_loss(ptr(f.t), ptr(f.t), 65, 1, 0, ptr(f.t), ptr(f.t), ptr(f.t), ptr(f.t), ptr(f.t), stream_ptr()) == -2
    _sync()
    assert a.intact() and f.intact()


# ---- 4. ov_ga_cosine_loss --------------------------------------------------------------------------------------------------------------
def _cosine_bounds(tx, img, eps=1e-8):
    """n = ceil(E / 64) + 7: a lane's fmaf chain, six butterfly steps, one spare.  A dot carries gamma_n sum |x y|, a norm (n / 2 + 1) u
    relative.  cos_ji: |err| <= (gamma_n sum|xy| / (mt mi)) + |cos| (n + 6) u; loss1: B additions, the division, the product:
    100 (mean_i of that + (B + 2) u mean_i |cos|).  dtx_jk = coef sum_i (A_i - C_i), A_i = img_ik / (mt mi) carrying (n + 5) u and
    C_i = dot x_k / (mt^2 mi |x|) carrying gamma_n sum|xy| / |dot| + (2 n + 10) u, B additions: coef sum_i (|A_i| (n + B + 8) u +
    C^_i (3 n + B + 12) u) with C^_i formed from sum |x y| in place of |dot|."""
    b, e = tx.shape
    n = math.ceil(e / 64) + 7
    nt, ni = tx.norm(dim=-1), img.norm(dim=-1)
    mt, mi = nt.clamp_min(eps), ni.clamp_min(eps)
    absdots = tx.abs() @ img.abs().t()
    ratio = absdots / (mt.unsqueeze(1) * mi.unsqueeze(0))
    e_loss = 100 * (3 * n + b + 8) * U * ratio.mean(dim=1)
    a_i = img.abs().unsqueeze(0) / (mt.view(b, 1, 1) * mi.view(1, b, 1))
    live = (nt > eps).double()
    c_i = (absdots / ((mt * mt).unsqueeze(1) * mi.unsqueeze(0) * nt.clamp_min(1e-300).unsqueeze(1))).unsqueeze(-1) * tx.abs().unsqueeze(1)
    e_dtx = (100.0 / (b * b)) * ((a_i * (n + b + 8) * U).sum(1) + (c_i * (3 * n + b + 12) * U).sum(1) * live.unsqueeze(1))
    return e_loss, e_dtx


@pytest.mark.parametrize("shape", [(1, 8), (3, 192), (13, 768), (5, 100)], ids=lambda s: f"b{s[0]}_e{s[1]}")
def test_cosine_loss_gradient_and_best_tracking(shape):
    b, e = shape
    lib = _lib.load()
    g = torch.Generator().manual_seed(b * 1000 + e)
    img = torch.randn(b, e, generator=g)
    first = torch.randn(b, e, generator=g)
    if b > 1:
        first[b // 2] = 0                                              # a zero row: eps decides its cosine and its gradient
    # better (the first always is), worse (turned away from the images), better (towards them)
    seq = [first, -img.roll(1, 0) * 0.5 - img, img * 3 + 0.1 * torch.randn(b, e, generator=g)]
    gi = Guarded(img.shape, fill=img)
    hist, dtx, best_tx = Guarded((3, b), shift=3), Guarded((b, e)), Guarded((b, e))
    best = Guarded((1,), fill=torch.tensor([float("inf")]))
    best_step = Guarded((1,), torch.int32, fill=torch.tensor([-1], dtype=torch.int32))
    means, kept = [], None
    for i, tx in enumerate(seq):
        gt = Guarded(tx.shape, fill=tx)
        row = _lib.c_void_p(hist.t.data_ptr() + i * b * 4)
        _lib.check(lib.ov_ga_cosine_loss(ptr(gt.t), ptr(gi.t), b, e, i, row, ptr(dtx.t), ptr(best.t), ptr(best_step.t), ptr(best_tx.t),
                                         stream_ptr()), "ov_ga_cosine_loss")
        _sync()
        assert all(x.intact() for x in (gt, gi, hist, dtx, best_tx, best, best_step))
        want_l, want_d = A.cosine_loss(tx.double(), img.double())
        e_loss, e_dtx = _cosine_bounds(tx.double(), img.double())
        got_l, got_d = hist.t[i].cpu().double(), dtx.t.cpu().double()
        rl = ((got_l - want_l).abs() / e_loss.clamp_min(1e-300)).max().item()
        rd = ((got_d - want_d).abs() / e_dtx.clamp_min(1e-300)).max().item()
        print(f"cosine b{b} e{e} step {i}: loss1 {got_l.tolist()[:3]} worst |err| / bound = {rl:.3f}, dtx = {rd:.3f}")
        assert ((got_l - want_l).abs() <= e_loss).all() and ((got_d - want_d).abs() <= e_dtx).all()
        if i == 0 and b > 1:
            assert float(got_l[b // 2]) == 0 and float(got_d[b // 2].abs().max()) > 1e4
        mean = float(ga.mean_loss(hist.t[i]))
        means.append(mean)
        if mean < min(means[:-1], default=float("inf")):
            kept = (mean, i, tx)
        assert float(best.t.item()) == kept[0] and int(best_step.t.item()) == kept[1]
        assert torch.equal(best_tx.t.cpu(), kept[2])
        if i + 1 < 3:
            assert bool((hist.t[i + 1:] == hist.sent).all())
    assert means[1] > means[0] > means[2] and kept[1] == 2


# ---- 5, 6. the loop on vit-tiny-patch16-160 --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    cfg = preset("vit-tiny-patch16-160")
    model = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    for p in model.parameters():
        p.requires_grad_(True)                                # as in the script: the parameters are leaves, and get no .grad
    image = synth.make_images(1, 160, seed=4)[0]
    image = ((image - image.min()) / (image.max() - image.min())).to(DEV)
    return cfg, model, image


def _restated_grad(loop, start, noise, dx, tau):
    """d normu in fp64 from the rows dX the tower handed over, on the bf16 table."""
    r = dx.shape[0]
    v = start.shape[-1]
    z64 = A.gumbel_z(start.double().view(r, v).cpu(), noise.double().cpu(), tau)
    _, _, _, ys = A.sample(z64)
    w = loop.model.token_embedding.packed().double().cpu()
    gy, c, g = A.token_grad(dx.double().cpu(), w, ys, tau)
    return z64, ys, gy, g, dx.double().cpu().abs() @ w.abs().t()


def test_one_step_equals_the_eager_soft_token_composition(tiny):
    """B = 3, K = 2, three iterations, each started from the eager path's state (parameters and Adam moments), so that a flipped
    argmax cannot compound.  The difference to the eager gradient is measured, not fixed: the eager path's own distance from the
    fp64 restatement on the same dX, and the HIP path is allowed twice that."""
    cfg, model, image = tiny
    b, k, tau, lr = 3, 2, 1000.0, 5.0
    t, v = model.context_length, model.token_embedding.weight.shape[0]
    flags = [p.requires_grad for p in model.parameters()]
    loop = GradientAscent(model, batch_size=b, tokens=k, steps=3, lr=lr, tau=tau, debug=True)
    torch.manual_seed(31)
    loop.begin(image)
    leaf = loop.normu.clone().requires_grad_(True)
    opt = torch.optim.Adam([leaf], lr=lr)
    fixed = torch.zeros(b, t - k, dtype=torch.int64, device=DEV)
    w32 = model.token_embedding.weight.detach().float()
    try:
        for i in range(3):
            start = leaf.detach().clone()
            loop.normu.copy_(start)
            if i > 0:
                loop._s.ea.copy_(opt.state[leaf]["exp_avg"].view_as(loop._s.ea))
                loop._s.es.copy_(opt.state[leaf]["exp_avg_sq"].view_as(loop._s.es))
            torch.cuda.manual_seed(700 + i)
            loop.step(i)
            _sync()
            torch.cuda.manual_seed(700 + i)
            noise = torch.empty(b * k, v, device=DEV).exponential_()
            # the eager composition: the parent commit's way
            torch.cuda.manual_seed(700 + i)
            soft = F.gumbel_softmax(leaf, tau=tau, dim=-1, hard=True)
            idx = soft.detach().argmax(-1)
            assert torch.equal(loop.ids_history[i].long(), idx), i
            tokens = torch.cat([F.one_hot(fixed, v).float(), soft], dim=1)
            ids = tokens.detach().argmax(-1)
            assert torch.equal(loop._s.ids, ids)
            assert torch.equal(loop.last_x, F.embedding(ids, w32))             # what training.encode_text(model, ids) feeds the tower
            tx = training.encode_text(model, tokens, normalize=False)
            loss1 = A.cosine_loss_eager(tx, loop.last_img)
            opt.zero_grad()
            loss1.mean().backward()
            opt.step()
            _sync()
            # the loss on the loop's own features, within the cosine kernel's bound
            want_l, _ = A.cosine_loss(loop.last_tx.double().cpu(), loop.last_img.double().cpu())
            e_loss, _ = _cosine_bounds(loop.last_tx.double().cpu(), loop.last_img.double().cpu())
            assert ((loop.history[i].double().cpu() - want_l).abs() <= e_loss).all()
            # the hand-over: the learned rows of x.grad are bf16 values
            rows = loop.last_xgrad[:, t - k:, :]
            assert torch.equal(rows.to(torch.bfloat16).float(), rows.float()) and float(rows.abs().max()) > 0
            assert torch.equal(loop.last_dx.float().view(b, k, -1), rows.float())
            # the gradient against the fp64 restatement fed with the same dX
            z64, ys, gy, g64, mag = _restated_grad(loop, start, noise, loop.last_dx, tau)
            d = loop.last_dx.shape[1]
            nblk = (v + 127) // 128
            e_gy = A.gamma(d) * mag
            dz = 4 * U * (start.double().cpu().view(b * k, v).abs() + noise.double().cpu().log().abs()).max(-1, keepdim=True)[0] / tau
            spread = z64.max(-1, keepdim=True)[0] - z64.min(-1, keepdim=True)[0]
            eps_ys = 2 * dz + (spread + math.ceil(v / 1024) + 24) * U + 4 * U
            e_c = ((e_gy + gy.abs() * (eps_ys + (nblk + 8) * U)) * ys).sum(-1, keepdim=True)
            e_g = ys * (e_gy + e_c) / tau + g64.abs() * (eps_ys + 4 * U)
            hip = loop.last_grad.double().cpu().view(b * k, v)
            assert ((hip - g64).abs() <= e_g).all(), i
            eager = leaf.grad.double().cpu().view(b * k, v)
            d_eager, d_hip = float((eager - g64).abs().max()), float((hip - g64).abs().max())
            print(f"tiny step {i}: |g| max {float(g64.abs().max()):.3e}; distance from the fp64 restatement on the loop's dX: eager "
                  f"{d_eager:.3e}, HIP {d_hip:.3e}; loss1 HIP {loop.history[i].tolist()} eager {loss1.tolist()}")
            assert d_hip <= 2 * d_eager
    finally:
        loop.end()
    assert [p.requires_grad for p in model.parameters()] == flags and all(p.grad is None for p in model.parameters())


def _free_run(model, image, steps=6):
    torch.manual_seed(77)
    torch.cuda.manual_seed(77)
    loop = GradientAscent(model, batch_size=3, tokens=2, steps=steps)
    loop.begin(image)
    try:
        loop.step(0)
        _sync()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")            # launches only: a host synchronisation inside a step raises
        try:
            for i in range(1, steps):
                loop.step(i)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        _sync()
    finally:
        loop.end()
    return loop


def test_free_run_repeats_bitwise_and_tracks_its_best(tiny):
    cfg, model, image = tiny
    flags = [p.requires_grad for p in model.parameters()]
    a, b = _free_run(model, image), _free_run(model, image)
    assert torch.equal(a.history, b.history) and torch.equal(a.ids_history, b.ids_history) and torch.equal(a.normu, b.normu)
    assert torch.equal(a.best_text_embedding, b.best_text_embedding)
    hist = a.history.cpu()
    assert hist.shape == (6, 3) and bool(torch.isfinite(hist).all()) and bool((hist.abs() <= 100).all())
    means = ga.mean_loss(hist)
    assert a.best_loss == float(means.min()) and a.best_step == int(means.argmin())
    assert a.ids_history.shape == (6, 3, 2) and int(a.ids_history.min()) >= 0 and int(a.ids_history.max()) < model.token_embedding.weight.shape[0]
    assert not torch.equal(a.normu.cpu(), torch.zeros_like(a.normu.cpu()))
    # the best text embedding: the tower on that step's ids again, through the step's own path
    t, k = model.context_length, 2
    ids = torch.cat([torch.zeros(3, t - k, dtype=torch.int64, device=DEV), a.ids_history[a.best_step].long()], dim=1)
    for p in model.parameters():
        p.requires_grad_(False)
    try:
        x = F.embedding(ids, model.token_embedding.weight.detach().float()).requires_grad_(True)
        tx = training.encode_text_embeddings(model, x, normalize=False)
    finally:
        for p, f in zip(model.parameters(), flags):
            p.requires_grad_(f)
    assert torch.equal(tx.detach(), a.best_text_embedding)
    assert [p.requires_grad for p in model.parameters()] == flags and all(p.grad is None for p in model.parameters())


def test_gradient_ascent_refuses_what_it_does_not_build(tiny):
    cfg, model, image = tiny
    with pytest.raises(_lib.OvhipError):
        GradientAscent(model, steps=1)(image.cpu())
    with pytest.raises(ValueError):
        GradientAscent(model, steps=1)(torch.zeros(3, 96, 96, device=DEV))
    with pytest.raises(_lib.OvhipError):
        GradientAscent(model, batch_size=65, steps=1)(image)
    with pytest.raises(ValueError):
        GradientAscent(model, tokens=81, steps=1)(image)
    assert all(p.requires_grad for p in model.parameters())


# ---- 7. the command line ---------------------------------------------------------------------------------------------------------------
CLI = "os.chdir(sys.argv.pop(1))\nfrom openvision_amd.gradient_ascent import main\nraise SystemExit(main(sys.argv[1:]))\n"


@pytest.mark.timeout(600)
def test_command_line_writes_the_embedding_and_the_tokens(tmp_path):
    from PIL import Image
    cfg = preset("vit-tiny-patch16-160")
    ck = str(tmp_path / "tiny-ckpt")
    checkpoint.save_pretrained(create_model(cfg, state_dict=synth.make_state_dict(cfg)), cfg, ck, safetensors=False)
    rgb = np.random.default_rng(1).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "cat.png")
    run_child(CLI, str(tmp_path), "--use_model", ck, "--use_image", str(tmp_path / "cat.png"), "--steps", "3", "--batch_size", "3",
              "--tokens", "2", "--deterministic", timeout=300, gpu=True)
    emb = torch.load(tmp_path / "txtembeds" / "cat_text_embedding.pt", map_location="cpu")
    assert emb.shape == (3, cfg["embed_dim"]) and emb.dtype == torch.float32 and bool(torch.isfinite(emb).all()) and float(emb.abs().max()) > 0
    words = (tmp_path / "opinion-tokens" / "tokens_cat.txt").read_text(encoding="utf-8").split()
    assert words == sorted(set(words))
