"""CPU: the host side of the feature-visualisation loop (openvision_amd.visualize.FeatureVisualizer, csrc/vizloop.hip) -- the draw
tables against the script's draw sequence bit for bit, the closed-form image gradient against torch autograd in fp64, the Adamax + cosine
+ clamp step against torch.optim, zero scratch in the new kernels, and the argument errors of the entry points and of the class."""
import ctypes
import random

import pytest
import torch

import viz_restate as V
from openvision_amd import _lib, visualize
from openvision_amd import build as B
from test_build_scratch import kernel_scratch
from test_patchdrop_cpu import tiny_model

U64 = 2.0 ** -53


@pytest.mark.parametrize("case", [dict(steps=7, n=1, repeat=3, max_iter=5), dict(steps=3, n=2, repeat=8, max_iter=400),
                                  dict(steps=2, n=1, repeat=2, max_iter=1)], ids=["rem_wraps", "script_defaults", "max_iter_1"])
def test_draw_tables_equal_the_script_draw_sequence(case):
    steps, n, repeat, max_iter = case["steps"], case["n"], case["repeat"], case["max_iter"]
    batch, size, lim = repeat * n, 8, 4
    torch.manual_seed(6247423)
    random.seed(6247423)
    image, means, stds, noises, offsets = V.script_draws(steps, n, repeat, size, 0.7, 0.9, 0.5, max_iter, lim)
    torch.manual_seed(6247423)
    random.seed(6247423)
    rem = visualize.constructor_draws(batch, max_iter)
    mine = visualize.new_init(size, n, device="cpu")
    table, offs, rem_after = visualize.draw_tables(steps, batch, 0.7, 0.9, 0.5, max_iter, lim, rem=rem)
    assert torch.equal(mine, image)
    assert table.shape == (steps + 1, 3, 3 * batch) and table.dtype == torch.float32
    for i in range(steps + 1):
        for k, want in enumerate((means[i], stds[i], noises[i])):
            assert torch.equal(table[i, k], want.flatten()), (i, k)
    assert offs == offsets and all(-lim <= o <= lim for pair in offs for o in pair)
    assert rem_after == (max_iter - 2 - (steps + 1)) % max_iter
    if max_iter == 5:                  # the counter wraps inside the run: 3, 2, 1, 0, 4, 3, 2, 1
        assert bool((table[3, 2] == 0).all()) and bool((table[4, 2] != 0).all()) and bool((table[2, 2] != 0).all())


def test_feature_visualizer_makes_the_constructor_draws_before_the_image():
    model = tiny_model(0.0)                               # its initialisation draws too: built before the seed
    torch.manual_seed(3)
    V._ColorJitter(8, 1.0, 1.0), V._GaussianNoise(8, 0.5, 400)
    want = torch.rand(1, 3, 4, 4)
    torch.manual_seed(3)
    viz = visualize.FeatureVisualizer(model, 0, 0)
    assert torch.equal(visualize.new_init(4, 1, device="cpu"), want) and viz._rem == 398


@pytest.mark.parametrize("shape", [(1, 8, 12), (2, 3, 9)], ids=["n1_r8", "n2_r3"])
def test_closed_form_gradient_equals_autograd_in_fp64(shape):
    n, repeat, s = shape
    b = n * repeat
    g = torch.Generator().manual_seed(17)
    rnd = lambda *sh: torch.rand(*sh, generator=g, dtype=torch.float64)
    std, mean, noise = (rnd(b, 3, 1, 1) - 0.5).mul(2).exp(), rnd(b, 3, 1, 1) - 0.5, rnd(b, 3, 1, 1) * 0.2
    w = (rnd(b, 3, s, s) - 0.5) * 30                      # d objective / d aug: a fixed linear functional, gradient scale 15
    c_tv, size = 0.3, 7
    for off1, off2 in [(0, 0), (-32, 32), (-7, 13), (s - 1, -(s - 1)), (5, 0)]:
        img = rnd(n, 3, s, s).requires_grad_(True)
        with torch.no_grad():
            img[0, 1] = 0.25                              # a constant plane: norm 0 in every row that repeats it
        aug = V.augment(img, mean, std, noise, off1, off2, repeat)
        ((aug * w).sum() + c_tv * V.tv_value(aug, size)).backward()
        got = V.closed_form_grad(w, aug.detach(), std, off1, off2, repeat, c_tv, size)
        assert torch.isfinite(got).all()
        assert (got - img.grad).abs().max().item() <= 1e-12, (off1, off2)


def test_adamax_cosine_clamp_step_equals_torch_optim():
    steps, lr, b1, b2, eps = 6, 1.0, 0.5, 0.99, 1e-8
    g = torch.Generator().manual_seed(23)
    p = torch.rand(4, 3, 5, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    opt = torch.optim.Adamax([p], lr=lr, betas=(b1, b2), eps=eps)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps, 0.0)
    lrs, clr = V.cosine_lr(steps, lr), visualize.step_sizes(steps, lr, b1)
    for i in range(steps + 1):
        grad = (torch.rand(p.shape, generator=g, dtype=torch.float64) - 0.5) * 10.0 ** float(-(i % 4))
        grad[0, 0] = 0                                    # g = 0: ei decays (or is eps at the first step)
        st = opt.state[p]
        ea0 = st["exp_avg"].clone() if st else torch.zeros_like(p)
        ei0 = st["exp_inf"].clone() if st else torch.zeros_like(p)
        p0 = p.detach().clone()
        assert abs(opt.param_groups[0]["lr"] - lrs[i]) <= 2e-16
        assert abs(clr[i] - lrs[i] / (1 - b1 ** (i + 1))) <= 4 * U64 * clr[i]
        p.grad = grad
        opt.step()
        sched.step()
        p.data.clamp_(0, 1)
        want_p, ea, ei = V.adamax_clip(p0, grad, ea0, ei0, lrs[i], i + 1, b1, b2, eps)
        st = opt.state[p]
        assert ((st["exp_avg"] - ea).abs() <= 3 * U64 * (ea0.abs() + grad.abs())).all()
        assert ((st["exp_inf"] - ei).abs() <= 2 * U64 * ei).all()
        bound = U64 * want_p.abs() + clr[i] * (8 * U64 * ea.abs() + 3 * U64 * (ea0.abs() + grad.abs())) / ei
        assert ((p.detach() - want_p).abs() <= bound).all(), i
    assert bool((p.detach() == 0).any()) or bool((p.detach() == 1).any())        # the clamp was reached


@pytest.mark.timeout(900)
def test_vizloop_kernels_use_no_scratch():
    scratch = kernel_scratch("vizloop.hip")
    assert "vizloop.hip" in B.SOURCES
    for name in ("viz_augment_kernel", "viz_tv_kernel", "viz_tv_total_kernel", "viz_augment_bwd_kernel", "adamax_clip_kernel"):
        assert any(name in k for k in scratch), (name, sorted(scratch))
    assert all(v == 0 for v in scratch.values()), scratch


def test_entry_points_validate_without_hip():
    lib = _lib.load()
    dummy = (ctypes.c_char * 64)()
    a = (ctypes.addressof(dummy) + 15) & ~15
    ok = lambda **kw: dict(dict(N=1, R=8, S=32, P=16, Kpad=768), **kw)

    def augment(img=a, table=a, cols=a, aug=a, **kw):
        k = ok(**kw)
        return lib.ov_viz_augment(img, table, k["N"], k["R"], k["S"], k["P"], k["Kpad"], 3, -3, cols, aug, None)

    def backward(dcols=a, aug=a, norms=a, table=a, m=a, dimg=a, hist=a, **kw):
        k = ok(**kw)
        return lib.ov_viz_augment_backward(dcols, k["Kpad"], aug, norms, table, m, k["N"], k["R"], k["S"], k["P"], 3, -3, k["S"], 1.0, 5e-5,
                                           dimg, hist, None)

    for fn, ptrs in ((augment, ("img", "table", "cols")), (backward, ("dcols", "aug", "norms", "table", "dimg"))):
        for name in ptrs:
            assert fn(**{name: None}) == -1, (fn.__name__, name)
        assert fn(S=40) == -2                              # S % P != 0
        assert fn(S=8, P=16) == -2                         # S < P
        assert fn(S=1040, P=16) == -2                      # S > 1024
        assert fn(N=513, R=8) == -2 and fn(N=1, R=4097) == -2          # R N > 4096
        assert fn(N=0) == -1 and fn(R=0) == -1
        assert fn(Kpad=760) == -1                          # fewer columns than 3 P^2
    assert augment(img=a + 4) == -1 and backward(aug=a + 4) == -1        # not 16-byte aligned
    # table, m and the history row are read and written one float at a time: a step's row of a packed table starts at any multiple of 4
    # bytes.  Alignment is checked before the shape, so the refused shape shows that the pointer passed (and nothing is launched)
    assert augment(table=a + 4, S=40) == -2 and backward(table=a + 4, m=a + 4, hist=a + 12, S=40) == -2
    assert augment(table=a + 2, S=40) == -1 and backward(table=a + 2, S=40) == -1 and backward(m=a + 2, S=40) == -1
    assert augment(img=a + 4, S=40) == -1 and backward(dimg=a + 4, S=40) == -1
    assert backward(m=None) == -1 and backward(hist=None) == -1          # the history row and m come together
    assert lib.ov_viz_tv(None, 8, 32, 32, a, a, None) == -1 and lib.ov_viz_tv(a, 8, 32, 32, None, a, None) == -1
    assert lib.ov_viz_tv(a, 8, 1040, 32, a, a, None) == -2 and lib.ov_viz_tv(a, 4097, 32, 32, a, a, None) == -2
    assert lib.ov_viz_tv(a, 0, 32, 32, a, a, None) == -1 and lib.ov_viz_tv(a, 8, 32, 0, a, a, None) == -1
    step = lambda img=a, g=a, ea=a, ei=a, n=16, b1=0.5, b2=0.99, eps=1e-8, lo=0.0, hi=1.0: \
        lib.ov_adamax_clip_step(img, g, ea, ei, n, 1.0, b1, b2, eps, lo, hi, None)
    for name in ("img", "g", "ea", "ei"):
        assert step(**{name: None}) == -1
    assert step(n=0) == -1 and step(b1=1.0) == -1 and step(b2=-0.1) == -1 and step(eps=-1.0) == -1 and step(lo=1.0, hi=0.0) == -1


def test_feature_visualizer_argument_errors():
    model = tiny_model(0.5)
    with pytest.raises(_lib.OvhipError, match="Tile"):
        visualize.FeatureVisualizer(model, 0, 0, tile=2)
    with pytest.raises(ValueError):
        visualize.FeatureVisualizer(model, 0, 0, steps=0)
    viz = visualize.FeatureVisualizer(model, 0, 0, steps=2)
    img = torch.zeros(1, 3, 160, 160)
    with pytest.raises(_lib.OvhipError, match="patch_dropout"):          # training mode with patch dropout
        viz(img)
    model.eval()
    with pytest.raises(_lib.OvhipError, match="MI355X"):                 # a CPU tensor: no fallback
        viz(img)
    with pytest.raises(_lib.OvhipError, match="layer"):
        visualize.FeatureVisualizer(model, 99, 0, steps=2)(img)
    ln = model.visual.ln_pre
    model.visual.ln_pre = torch.nn.LayerNorm(model.visual.positional_embedding.shape[1])
    with pytest.raises(_lib.OvhipError, match="ln_pre"):
        viz(img)
    model.visual.ln_pre = ln
