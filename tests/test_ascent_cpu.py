"""CPU: the gradient-ascent loop's arithmetic as restated in tests/ascent_restate.py against eager torch (autograd through
F.gumbel_softmax(hard=True) + torch.cat + torch.optim.Adam; F.grid_sample), the host draws, Tokenizer.decode and the command line's
host pieces.  The GPU tests (test_gpu_ascent.py) hold the kernels to the same restatement."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ascent_restate as A
from openvision_amd import gradient_ascent as ga
from openvision_amd.tokenizer import DEFAULT_VOCAB, WordPieceTokenizer, clean

U64 = A.U64


# ---- 1. the restated step against eager autograd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1000.0, 1.0])
def test_restated_step_equals_eager_autograd_three_steps(tau):
    """V = 1000, R = 6 (B = 3, K = 2), D = 32, T = 5, a fixed linear map [T, D, E] standing in for the tower, all fp64, both sides
    seeded alike (torch.manual_seed(s); empty_like(normu).exponential_() is the stream F.gumbel_softmax consumes on the CPU).

    Bounds.  Both sides evaluate the same real function in fp64, so they differ by rounding alone.  With mag[r,v] = sum_d |dX||W| the
    products' magnitude, gy carries at most gamma_D mag, c = sum_v gy ys at most gamma_{V+D} sum_v mag ys, and the eager forward
    feeds (1 - ys) + ys instead of 1 at the sampled entry, a relative 2 u perturbation of x that reaches dX through the loss's
    second derivative; the constant 64 covers that and the softmax's own operations (exp, sum of V terms, division: < V + 8 u
    relative on ys).  |delta g| <= 64 (V + D) u ys (mag + sum_v mag ys) / tau.
    Adam: |d (ea / denom) / d g_k| <= (1 / eps) (w1_k + (|ea| / denom) d denom / d g_k) with |ea| / sqrt(es) <= 10 sqrt(bc1) (Cauchy-
    Schwarz, w1_k / w2_k <= 100) and d denom / d g_k <= sqrt(w2_k / bc2): below 1 / eps per past step, so after step t the parameters
    differ by at most sum_{s <= t} (lr / bc1_s) (s / eps) max |delta g| + 8 u |p|."""
    torch.manual_seed(1)
    v, b, k, d, t, e, lr, betas, eps = 1000, 3, 2, 32, 5, 16, 5.0, (0.9, 0.999), 1e-8
    r = b * k
    w = torch.randn(v, d, dtype=torch.float64) * 0.5
    tower = torch.randn(t, d, e, dtype=torch.float64) / math.sqrt(d * t)
    img = torch.randn(b, e, dtype=torch.float64)
    normu0 = torch.zeros(b, k, v, dtype=torch.float64).normal_()
    prompt, pad = [7], 0
    fixed = torch.tensor(prompt + [pad] * (t - k - len(prompt)))
    # eager: the script
    normu_e = normu0.clone().requires_grad_(True)
    opt = torch.optim.Adam([normu_e], lr=lr, betas=betas, eps=eps)
    # restated
    normu_r, ea, es = normu0.clone().view(r, v), torch.zeros(r, v, dtype=torch.float64), torch.zeros(r, v, dtype=torch.float64)
    dg_max, p_slack = 0.0, 0.0
    for step in range(1, 4):
        start = normu_e.detach().clone()              # each step of the restatement starts from the eager state: no compounding
        normu_r = start.view(r, v).clone()
        torch.manual_seed(100 + step)
        soft = F.gumbel_softmax(normu_e, tau=tau, dim=-1, hard=True)
        tokens = torch.cat([F.one_hot(fixed, v).double().expand(b, -1, -1), soft], dim=1)
        tx = torch.einsum("btd,tde->be", tokens @ w, tower)
        loss1 = A.cosine_loss_eager(tx, img)
        opt.zero_grad()
        loss1.mean().backward()
        g_eager = normu_e.grad.detach().clone().view(r, v)
        ea_prev = opt.state[normu_e]["exp_avg"].clone().view(r, v) if step > 1 else ea
        es_prev = opt.state[normu_e]["exp_avg_sq"].clone().view(r, v) if step > 1 else es
        opt.step()
        # the restatement
        torch.manual_seed(100 + step)
        noise = torch.empty_like(start).exponential_().view(r, v)
        idx, zmax, zsum, ys = A.sample(A.gumbel_z(normu_r, noise, tau))
        assert torch.equal(idx.view(b, k), soft.detach().argmax(-1)), step
        ids = torch.cat([fixed.expand(b, -1), idx.view(b, k)], dim=1)
        x = w[ids]
        tx_r = torch.einsum("btd,tde->be", x, tower)
        l1, dtx = A.cosine_loss(tx_r, img)
        assert torch.allclose(l1, loss1.detach(), rtol=1e-12, atol=1e-12)
        dx = torch.einsum("be,tde->btd", dtx, tower)[:, t - k:].reshape(r, d)
        gy, c, g = A.token_grad(dx, w, ys, tau)
        mag = dx.abs() @ w.abs().t()
        bound = 64 * (v + d) * U64 * ys * (mag + (mag * ys).sum(-1, keepdim=True)) / tau
        ratio = ((g - g_eager).abs() / bound).max().item()
        print(f"tau {tau} step {step}: |g| max {g_eager.abs().max():.3e}, worst |restated - eager| / bound = {ratio:.3e}")
        assert ratio <= 1.0
        assert g_eager.abs().max() > 0
        kk = A.adam_constants(step, lr, betas, eps, torch.float64)
        p_new, ea_new, es_new = A.adam_step(normu_r, g, ea_prev, es_prev, kk)
        p_bound = (lr / (1 - betas[0] ** step)) * (step / eps) * bound.max() + 8 * U64 * p_new.abs()
        p_ratio = ((p_new - normu_e.detach().view(r, v)).abs() / p_bound).max().item()
        print(f"tau {tau} step {step}: parameters, worst |restated - eager| / bound = {p_ratio:.3e}")
        assert p_ratio <= 1.0
        assert not torch.equal(p_new, normu_r)
        assert torch.allclose(ea_new, opt.state[normu_e]["exp_avg"].view(r, v), rtol=1e-9, atol=1e-30)


def test_token_grad_formula_is_the_softmax_backward_in_fp64():
    """d normu = ys (gy - c) / tau against autograd through the soft path alone (one_hot - ys.detach() + ys)."""
    g = torch.Generator().manual_seed(3)
    normu = torch.randn(4, 300, generator=g, dtype=torch.float64).requires_grad_(True)
    noise = torch.empty(4, 300, dtype=torch.float64).exponential_(generator=g)
    gy = torch.randn(4, 300, generator=g, dtype=torch.float64)
    for tau in (1.0, 1000.0):
        z = A.gumbel_z(normu, noise, tau)
        ys = z.softmax(-1)
        hard = F.one_hot(ys.argmax(-1), 300).double() - ys.detach() + ys
        (grad,) = torch.autograd.grad((hard * gy).sum(), normu)
        _, _, _, ys_r = A.sample(z.detach())
        c = (gy * ys_r).sum(-1, keepdim=True)
        want = ys_r * (gy - c) / tau
        assert torch.allclose(grad, want, rtol=1e-10, atol=1e-25)


def test_cosine_loss_formula_is_torch_cosine_similarity():
    g = torch.Generator().manual_seed(4)
    tx = torch.randn(5, 24, generator=g, dtype=torch.float64)
    tx[2] = 0                                             # a zero row: eps decides
    img = torch.randn(5, 24, generator=g, dtype=torch.float64)
    leaf = tx.clone().requires_grad_(True)
    loss1 = A.cosine_loss_eager(leaf, img)
    loss1.mean().backward()
    l1, dtx = A.cosine_loss(tx, img)
    assert torch.allclose(l1, loss1.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(dtx, leaf.grad, rtol=1e-10, atol=1e-14)
    assert float(l1[2]) == 0 and dtx[2].abs().max() > 1e6  # x / (eps |y|)


# ---- 2. the affine restatement against grid_sample -------------------------------------------------------------------------------------
def _mats(size):
    z = torch.zeros(())
    cases = {
        "identity": (False, 0.0, 0.0, 0.0),
        "shift": (True, 0.0, 3.0, -2.0),
        "rot+10": (True, 10.0, 0.0, 0.0),
        "rot-10": (True, -10.0, 1.25, -0.75),
        "gone": (True, 0.0, 3.0 * size, 0.0),
    }
    rows = [ga.inverse_matrices(torch.tensor(a), torch.tensor(d) + z, torch.tensor(x) + z, torch.tensor(y) + z, size) for a, d, x, y in cases.values()]
    return list(cases), torch.stack(rows)


@pytest.mark.parametrize("size", [20, 35])
def test_restated_affine_equals_grid_sample(size):
    g = torch.Generator().manual_seed(size)
    img = torch.rand(3, size, size, generator=g, dtype=torch.float64)
    mean, std = torch.tensor([0.48, 0.45, 0.40], dtype=torch.float64), torch.tensor([0.26, 0.27, 0.28], dtype=torch.float64)
    names, mats = _mats(size)
    got = A.affine(img, mats, mean, std)
    want = A.affine_grid_sample(img, mats, mean, std)
    # grid_sample reaches the source point through normalised coordinates and back: a few roundings of magnitude S, on a surface of
    # slope <= 1 per pixel (values in [0, 1]), divided by std
    assert (got - want).abs().max().item() <= 64 * size * U64 / 0.26
    norm = (img - mean.view(3, 1, 1)) / std.view(3, 1, 1)
    assert torch.equal(got[names.index("identity")], norm)
    shifted = got[names.index("shift")]                    # destination (y, x) reads source (y + 2, x - 3)
    assert torch.equal(shifted[:, : size - 2, 3:], norm[:, 2:, : size - 3])
    outside = ((0 - mean) / std).view(3, 1, 1)
    assert torch.equal(shifted[:, :, :3], outside.expand(3, size, 3)) and torch.equal(shifted[:, size - 2:, :], outside.expand(3, 2, size))
    assert torch.equal(got[names.index("gone")], outside.expand(3, size, size))
    assert not torch.equal(got[names.index("rot+10")], got[names.index("rot-10")])


# ---- 3. the host draws -------------------------------------------------------------------------------------------------------------------
def test_draw_affine_shapes_ranges_and_seed():
    torch.manual_seed(9)
    mats, params = ga.draw_affine(40, 13, 224, degrees=10.0, translate=0.1, p=0.8)
    assert mats.shape == (40, 13, 6) and mats.dtype == torch.float32 and params.shape == (40, 13, 4) and params.dtype == torch.float64
    apply, angle, tx, ty = params.unbind(-1)
    assert set(apply.unique().tolist()) == {0.0, 1.0} and 0.7 < apply.mean() < 0.9
    assert angle.abs().max() <= 10 and tx.abs().max() <= 22.4 and ty.abs().max() <= 22.4 and angle.abs().max() > 9
    ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0])
    assert torch.equal(mats[apply == 0], ident.expand(int((apply == 0).sum()), 6))
    # a rotation matrix, and the centre's image is the centre minus the translation rotated back
    on = apply == 1
    assert torch.allclose(mats[on][:, 0] ** 2 + mats[on][:, 1] ** 2, torch.ones(int(on.sum())), atol=1e-6)
    torch.manual_seed(9)
    again, _ = ga.draw_affine(40, 13, 224, degrees=10.0, translate=0.1, p=0.8)
    assert torch.equal(mats, again)
    none, pr = ga.draw_affine(5, 4, 32, p=0.0)
    assert torch.equal(none, ident.expand(5, 4, 6)) and float(pr[..., 0].sum()) == 0


def test_inverse_matrix_undoes_the_forward_map():
    size, ang, tx, ty = 33, 7.0, 2.5, -1.5
    m = ga.inverse_matrices(torch.tensor(True), torch.tensor(ang), torch.tensor(tx), torch.tensor(ty), size)
    c, s, ctr = math.cos(math.radians(ang)), math.sin(math.radians(ang)), (size - 1) / 2
    px, py = 4.0, 9.0
    qx = c * (px - ctr) - s * (py - ctr) + ctr + tx
    qy = s * (px - ctr) + c * (py - ctr) + ctr + ty
    assert abs(float(m[0] * qx + m[1] * qy + m[2]) - px) < 1e-12 and abs(float(m[3] * qx + m[4] * qy + m[5]) - py) < 1e-12


# ---- 4. decode ---------------------------------------------------------------------------------------------------------------------------
CAPTIONS = ["a photo of a cat", "A photo of a CAT.", "  two   dogs, running!  ", "naïve café déjà-vu", "state-of-the-art: 3.5x faster (really)",
            "unaffable antidisestablishmentarianism", "don't you think it's theirs? they're sure, we've said so", "",
            "[MASK] token [SEP] inside [UNK] text", "the quick brown fox jumps over the lazy dog " * 12]


def test_decode_equals_transformers_bert_tokenizer():
    transformers = pytest.importorskip("transformers")
    hf = transformers.BertTokenizer(DEFAULT_VOCAB)
    tok = WordPieceTokenizer()
    for text in CAPTIONS:
        ids = tok.encode(clean(text))
        for row in (ids, tok.frame(ids, 80)):
            for skip in (True, False):
                want = hf.decode(row, skip_special_tokens=skip, clean_up_tokenization_spaces=True)
                assert tok.decode(row, skip_special_tokens=skip, clean_up_tokenization_spaces=True) == want, (text, skip)


def test_decode_round_trips_encode():
    tok = WordPieceTokenizer()
    for text in CAPTIONS:
        ids = tok.encode(clean(text))
        back = tok.decode(ids)
        assert tok.encode(back) == [i for i in ids if i not in (0, 100, 101, 102, 103)], text
    assert tok.decode([2054, 2003, 2023]) == " ".join(tok._tokens[i] for i in (2054, 2003, 2023))
    assert tok.decode(torch.tensor([7592, 1010, 2088, 999])) == "hello, world!"
    assert tok.decode([7592, 1010, 2088, 999], clean_up_tokenization_spaces=False) == "hello , world !"
    assert tok.decode([0, 101, 7592, 102], skip_special_tokens=False) == "[PAD] [CLS] hello [SEP]"
    assert tok.decode([31999, -1, 7592]) == "hello"        # outside the file: [UNK], dropped as special


# ---- 5. checkin and the command line's host pieces ---------------------------------------------------------------------------------------
def test_checkin_rebuilds_bests_from_the_histories(tmp_path):
    tok = WordPieceTokenizer()
    ids = torch.tensor([[[7592, 2088], [4937, 3899]], [[4937, 4937], [3899, 1012]], [[2088, 2088], [7592, 7592]]], dtype=torch.int32)
    hist = torch.tensor([[-1.0, -3.0], [-2.0, -0.5], [-4.0, -5.0]])
    lines = []
    bests = ga.checkin(ids, hist, tok, "img", out_dir=str(tmp_path), log=lines.append)
    # step 0: new best (-2) and j % 50 == 0 -> visited twice; step 1: mean -1.25, no; step 2: mean -4.5, new best
    assert [round(k, 3) for k, _ in bests] == [-1.0, -3.0, -1.0, -3.0, -4.0, -5.0]
    assert [t for _, t in bests][-2:] == ["world world", "hello hello"]
    words = (tmp_path / "tokens_img.txt").read_text().split()
    assert words == sorted({"hello", "world", "cat", "dog"})
    assert any(l.startswith("New best loss: -4.500") for l in lines) and any(l.startswith("Iteration 0: Average Loss: -2.000") for l in lines)
    short = ga.checkin(ids, hist, tok, "img", upto=1, out_dir=None)
    assert [round(k, 3) for k, _ in short] == [1000.0, 1001.0, -1.0, -3.0, -1.0, -3.0]
    assert torch.equal(ga.mean_loss(hist), torch.tensor([-2.0, -1.25, -4.5]))


def test_command_line_arguments_and_load_image(tmp_path):
    from PIL import Image
    a = ga.parse_arguments([])
    assert (a.batch_size, a.img_folder, a.deterministic, a.steps, a.tokens) == (13, "None", False, 340, 4)
    a = ga.parse_arguments(["--batch_size", "3", "--use_model", "m", "--use_image", "x.png", "--deterministic", "--steps", "3", "--tokens", "2"])
    assert (a.batch_size, a.use_model, a.use_image, a.deterministic, a.steps, a.tokens) == (3, "m", "x.png", True, 3, 2)
    assert ga.image_paths(a) == ["x.png"]
    rgb = np.random.default_rng(0).integers(0, 256, size=(10, 14, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "b.png")
    Image.fromarray(rgb[:, :, 0]).save(tmp_path / "a.jpg")
    (tmp_path / "notes.txt").write_text("no image")
    a = ga.parse_arguments(["--img_folder", str(tmp_path)])
    assert [os.path.basename(p) for p in ga.image_paths(a)] == ["a.jpg", "b.png"]
    im = ga.load_image(str(tmp_path / "b.png"), 20, 28, device="cpu")
    assert im.shape == (1, 3, 20, 28) and im.dtype == torch.float32 and 0 <= float(im.min()) and float(im.max()) <= 1
    want = F.interpolate(torch.tensor(rgb).unsqueeze(0).permute(0, 3, 1, 2) / 255, (20, 28))
    assert torch.equal(im, want)
    assert torch.equal(im[0, :, ::2, ::2], torch.tensor(rgb).permute(2, 0, 1) / 255)          # nearest: every source pixel, twice
    grey = ga.load_image(str(tmp_path / "a.jpg"), 10, 14, device="cpu")
    assert grey.shape == (1, 3, 10, 14) and torch.equal(grey[0, 0], grey[0, 1])
