"""GPU: the feature-visualisation loop on HIP (csrc/vizloop.hip, openvision_amd.visualize.FeatureVisualizer, the
feature_visualization command line).  Kernels alone first -- the augmentation against the fp32 restatement bit for bit, the plane norms,
the image gradient and the Adamax step against fp64 within bounds written from the operations each performs (u = 2^-24) -- then one
fused step and a six-step run on vit-tiny-patch16-160 against the eager composition the loop replaces, and the command line.  Every
buffer a kernel writes or reads stands between guard words."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import viz_restate as V
from conftest import golden
from openvision_amd import _lib, checkpoint, preset, synth, visualize
from openvision_amd._lib import ptr, stream_ptr
from openvision_amd.feature_visualization import fix_random_seed, to_uint8
from openvision_amd.model import create_model
from openvision_amd.visualize import FeatureVisualizer, MLPFeatureLoss, mlp_feature
from ranks import run_child

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = V.U
GUARD = 64                      # elements in front of and behind every buffer
OFFSETS = lambda s: [(0, 0), (-32, 32), (-7, 13), (s - 1, -(s - 1)), (5, 0)]
# (N, R, S, p): the issue's three, then one whose side is no multiple of 4 (the kernels' scalar path) and one with a half-filled last group of 8
SHAPES = [(1, 8, 32, 16), (2, 3, 48, 16), (1, 8, 28, 14), (1, 2, 35, 7), (2, 2, 20, 4)]
IDS = ["n1_r8_s32_p16", "n2_r3_s48_p16", "n1_r8_s28_p14", "n1_r2_s35_p7", "n2_r2_s20_p4"]


class Guarded:
    """A device buffer of `shape` between two runs of GUARD sentinel elements; `t` is the view the kernels get: 16-byte aligned, or
    `shift` elements past that (a step's row inside a packed table)."""

    def __init__(self, shape, dtype=torch.float32, fill=None, shift=0):
        n = int(np.prod(shape))
        self.sent = 1234.5 if dtype != torch.int32 else 12345
        self.lo = GUARD + shift
        self.buf = torch.full((self.lo + n + GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool((self.buf[:self.lo] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())


def _table(g, batch):
    """mean | std | noise as draw_tables lays them out, [3, 3B], and the three as [B,3,1,1]."""
    mean = (torch.rand(batch, 3, 1, 1, generator=g) - 0.5) * 2
    std = ((torch.rand(batch, 3, 1, 1, generator=g) - 0.5) * 2).exp()
    noise = torch.randn(batch, 3, 1, 1, generator=g) * 0.4
    return torch.stack([mean.flatten(), std.flatten(), noise.flatten()]), mean, std, noise


def _kp(p):
    return (3 * p * p + 63) // 64 * 64


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_augment_equals_the_fp32_restatement_bit_for_bit(shape):
    n, r, s, p = shape
    lib = _lib.load()
    batch, grid, kp = n * r, (s // p) ** 2, _kp(p)
    g = torch.Generator().manual_seed(s)
    img = torch.rand(n, 3, s, s, generator=g)
    tab, mean, std, noise = _table(g, batch)
    gi, gt = Guarded(img.shape, fill=img), Guarded(tab.shape, fill=tab, shift=0 if r == 8 else 1)     # a table row 4 bytes off 16 as well
    for off1, off2 in OFFSETS(s):
        want = V.augment(img, mean, std, noise, off1, off2, r)                         # fp32 torch on the host: IEEE, one rounding per op
        want_cols = torch.zeros(batch * grid, kp, dtype=torch.bfloat16)
        want_cols[:, :3 * p * p] = V.patch_rows(want, p).to(torch.bfloat16)
        for with_aug in (True, False):
            cols, aug = Guarded((batch * grid, kp), torch.bfloat16), Guarded(want.shape)
            _lib.check(lib.ov_viz_augment(ptr(gi.t), ptr(gt.t), n, r, s, p, kp, off1, off2, ptr(cols.t), ptr(aug.t) if with_aug else None,
                                          stream_ptr()), "ov_viz_augment")
            torch.cuda.synchronize()
            tag = (shape, off1, off2, with_aug)
            assert torch.equal(cols.t.cpu().view(torch.int16), want_cols.view(torch.int16)), tag
            assert bool((cols.t[:, 3 * p * p:] == 0).all()), tag
            if with_aug:
                assert torch.equal(aug.t.cpu().view(torch.int32), want.view(torch.int32)), tag
            else:
                assert bool((aug.t == aug.sent).all()), tag
            assert cols.intact() and aug.intact() and gi.intact() and gt.intact(), tag


# ---- 2. total variation ----------------------------------------------------------------------------------------------------------------
def _smooth_planes(g, batch, s):
    """Planes with structure at every scale, one of them constant."""
    y, x = torch.meshgrid(torch.arange(s, dtype=torch.float32), torch.arange(s, dtype=torch.float32), indexing="ij")
    base = torch.sin(x / 3.0) * torch.cos(y / 5.0)
    a = base + torch.randn(batch, 3, s, s, generator=g) * torch.rand(batch, 3, 1, 1, generator=g)
    a[batch - 1, 1] = -0.75
    return a


@pytest.mark.parametrize("case", [(8, 32), (6, 48), (8, 28), (2, 35), (4, 20), (1, 1)], ids=lambda c: f"b{c[0]}_s{c[1]}")
def test_tv_plane_norms_and_scalar_within_n_plus_1_u_of_fp64(case):
    batch, s = case
    lib = _lib.load()
    size = 24
    g = torch.Generator().manual_seed(100 + s)
    a = _smooth_planes(g, batch, s) if s > 1 else torch.rand(batch, 3, 1, 1, generator=g)
    ga = Guarded(a.shape, fill=a)
    outs = []
    for _ in range(2):
        norms, tv = Guarded((4, 3 * batch)), Guarded((1,))
        _lib.check(lib.ov_viz_tv(ptr(ga.t), batch, s, size, ptr(norms.t), ptr(tv.t), stream_ptr()), "ov_viz_tv")
        torch.cuda.synchronize()
        assert norms.intact() and tv.intact() and ga.intact()
        outs.append((norms.t.cpu().double(), tv.t.cpu().double()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])        # no atomics: repeatable
    got, got_tv = outs[0]
    want = V.tv_norms(a.double()).reshape(4, 3 * batch)
    counts = [s * (s - 1), s * (s - 1), (s - 1) ** 2, (s - 1) ** 2]                            # differences per plane and field
    for k in range(4):
        err = (got[k] - want[k]).abs()
        print(f"tv b{batch} s{s} field {k}: max rel err {float((err / want[k].clamp_min(1e-30)).max()) / U:.2f} u, bound {counts[k] + 1} u")
        assert (err <= (counts[k] + 1) * U * want[k]).all(), (case, k)
    if s > 1:
        const = 3 * (batch - 1) + 1
        assert bool((got[:, const] == 0).all())                                                # the constant plane
    want_tv = float(V.tv_value(a.double(), size))
    print(f"tv b{batch} s{s} scalar: rel err {abs(float(got_tv) - want_tv) / max(want_tv, 1e-30) / U:.2f} u")
    assert abs(float(got_tv) - want_tv) <= (max(counts) + 1) * U * want_tv


# ---- 3. backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_augment_backward_within_its_bound_of_fp64(shape):
    n, r, s, p = shape
    lib = _lib.load()
    batch, grid, kp = n * r, (s // p) ** 2, _kp(p)
    g = torch.Generator().manual_seed(7 * s)
    size, c_feat, c_tv = s, 1.5, 0.5
    tab, _, std, _ = _table(g, batch)
    aug = _smooth_planes(g, batch, s)
    aug[0, 2] = 0.5                                                                           # a constant plane in a row every image pixel reads
    dcols = torch.randn(batch * grid, kp, generator=g).to(torch.bfloat16)                     # the padding columns too: they must not be read
    m = torch.randn(batch, generator=g)
    shift = 0 if r == 8 else 1                                                                # table, m and history 4 bytes off 16 as well
    ga, gt, gd, gm = Guarded(aug.shape, fill=aug), Guarded(tab.shape, fill=tab, shift=shift), \
        Guarded(dcols.shape, torch.bfloat16, fill=dcols), Guarded(m.shape, fill=m, shift=shift)
    norms = Guarded((4, 3 * batch))
    _lib.check(lib.ov_viz_tv(ptr(ga.t), batch, s, size, ptr(norms.t), None, stream_ptr()), "ov_viz_tv")
    g_aug = V.unpatch_rows(dcols.double(), batch, s, p)
    a64, std64 = aug.double(), std.double()
    want_tv = float(V.tv_value(a64, size))
    want_feat = c_feat * -float(m.double().sum()) / (batch * batch)
    for off1, off2 in OFFSETS(s):
        outs = []
        for _ in range(2):
            dimg, hist = Guarded((n, 3, s, s)), Guarded((3,), shift=shift)
            _lib.check(lib.ov_viz_augment_backward(ptr(gd.t), kp, ptr(ga.t), ptr(norms.t), ptr(gt.t), ptr(gm.t), n, r, s, p, off1, off2, size,
                                                   c_feat, c_tv, ptr(dimg.t), ptr(hist.t), stream_ptr()), "ov_viz_augment_backward")
            torch.cuda.synchronize()
            assert dimg.intact() and hist.intact() and ga.intact() and gt.intact() and gd.intact() and gm.intact() and norms.intact()
            outs.append((dimg.t.cpu(), hist.t.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        got, hist = outs[0][0].double(), outs[0][1].double()
        assert torch.isfinite(got).all()
        want = V.closed_form_grad(g_aug, a64, std64, off1, off2, r, c_tv, size)
        bound = V.grad_bound(g_aug, a64, std64, off1, off2, r, c_tv, size)
        ratio = ((got - want).abs() / bound).max().item()
        print(f"augment backward {shape} off ({off1}, {off2}): worst |err| / bound = {ratio:.3f}")
        assert ratio <= 1.0, (shape, off1, off2, ratio)
        # the history row: a B-term sum, the tv scalar of test 2, one product and one sum more each
        n_diff = s * (s - 1)
        assert abs(float(hist[1]) - want_feat) <= (batch + 3) * U * c_feat * float(m.double().abs().sum()) / (batch * batch)
        assert abs(float(hist[2]) - c_tv * want_tv) <= (n_diff + 3) * U * c_tv * want_tv
        assert abs(float(hist[0]) - (float(hist[1]) + float(hist[2]))) <= U * abs(float(hist[0]))
    # without the history row: the same gradient
    dimg = Guarded((n, 3, s, s))
    _lib.check(lib.ov_viz_augment_backward(ptr(gd.t), kp, ptr(ga.t), ptr(norms.t), ptr(gt.t), None, n, r, s, p, off1, off2, size, c_feat, c_tv,
                                           ptr(dimg.t), None, stream_ptr()), "ov_viz_augment_backward")
    torch.cuda.synchronize()
    assert torch.equal(dimg.t.cpu(), outs[0][0]) and dimg.intact()


# ---- 4. optimiser ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_step", [True, False], ids=["t1", "t7"])
def test_adamax_clip_step_within_its_bounds_of_fp64(first_step):
    lib = _lib.load()
    n = 4 * 1031 + 3                                         # several blocks and a tail of three
    g = torch.Generator().manual_seed(41)
    b1, b2, eps, lr = 0.5, 0.99, 1e-8, 1.0
    t = 1 if first_step else 7
    clr = lr * 0.93 / (1 - b1 ** t)
    mag = 10.0 ** (-6 * torch.rand(n, generator=g))          # magnitudes from 1e-6 to 1
    grad = torch.randn(n, generator=g).sign() * mag
    img = torch.rand(n, generator=g)
    if first_step:
        ea, ei = torch.zeros(n), torch.zeros(n)
    else:
        ea = torch.randn(n, generator=g) * 10.0 ** (-6 * torch.rand(n, generator=g))
        ei = ea.abs() * (1 + torch.rand(n, generator=g)) + 1e-7
    grad[:64] = 0                                             # g = 0: where ei > 0 it decays by b2, at t = 1 it becomes eps
    img[64:128] = torch.rand(64, generator=g) * 1e-3          # steps of size clr: both ends of the clamp are reached from here
    img[128:192] = 1 - torch.rand(64, generator=g) * 1e-3
    bufs = [Guarded((n,), fill=x) for x in (img, grad, ea, ei)]
    gp, gg, ga, gi = bufs
    _lib.check(lib.ov_adamax_clip_step(ptr(gp.t), ptr(gg.t), ptr(ga.t), ptr(gi.t), n, clr, b1, b2, eps, 0.0, 1.0, stream_ptr()),
               "ov_adamax_clip_step")
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs) and torch.equal(gg.t.cpu(), grad)
    p64, g64, ea64, ei64 = img.double(), grad.double(), ea.double(), ei.double()
    want_p, want_ea, want_ei = V.adamax_clip(p64, g64, ea64, ei64, clr * (1 - b1 ** t), t, b1, b2, eps)
    got_p, got_ea, got_ei = gp.t.cpu().double(), ga.t.cpu().double(), gi.t.cpu().double()
    assert ((got_ea - want_ea).abs() <= 3 * U * (ea64.abs() + g64.abs())).all()
    assert ((got_ei - want_ei).abs() <= 2 * U * want_ei).all()
    bound = U * want_p.abs() + clr * (8 * U * want_ea.abs() + 3 * U * (ea64.abs() + g64.abs())) / want_ei
    ratio = ((got_p - want_p).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"adamax t={t}: worst |err| / bound = {ratio:.3f}")
    assert ((got_p - want_p).abs() <= bound).all()
    assert bool((got_p == 0).any()) and bool((got_p == 1).any()) and bool(((got_p > 0) & (got_p < 1)).any())
    if not first_step:
        assert bool((got_ei[:64] > 0).all())


# ---- 5, 6. the loop on vit-tiny-patch16-160 --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    fv = golden("featviz_tiny16_160.npz")
    cfg = preset(str(fv["preset"]))
    sd = synth.make_state_dict(cfg, int(fv["seed"]), str(fv["variant"]))
    model = create_model(cfg, device=DEV, state_dict=sd)
    for p in model.parameters():
        p.requires_grad_(True)                                # as in the script: the parameters are leaves, and get no .grad
    return cfg, model, int(fv["features"][1])


def _rows(viz, i):
    """Iteration i's mean / std / noise as [B,3,1,1] on the device, and its offsets."""
    t = viz._s.table[i].view(3, -1, 3, 1, 1)
    return t[0], t[1], t[2], viz._s.offsets[i]


@pytest.mark.parametrize("layer", [0, 5])
def test_one_fused_step_equals_the_eager_composition(tiny, layer):
    _, model, feature = tiny
    c_feat, c_tv, size, repeat = 1.0, 5e-5, 160, 8
    torch.manual_seed(11)
    random.seed(11)
    viz = FeatureVisualizer(model, layer, feature, steps=2, tv_coefficient=c_tv, feature_coefficient=c_feat, debug=True)
    img = visualize.new_init(size, 1, device=DEV)
    viz.begin(img)
    viz.step(0)
    torch.cuda.synchronize()
    mean, std, noise, (off1, off2) = _rows(viz, 0)
    aug_host = V.augment(img.cpu(), mean.cpu(), std.cpu(), noise.cpu(), off1, off2, repeat)
    assert torch.equal(viz._s.aug.cpu(), aug_host)
    # the objective: the same operand rows through the same launches
    m_eager = mlp_feature(model, aug_host.to(DEV), layer, feature)
    assert torch.equal(viz.last_m, m_eager.detach()), (viz.last_m.tolist(), m_eager.tolist())
    # the gradient: the eager composition (torch augmentations + MLPFeatureLoss + the TotalVariation restatement, autograd in fp32)
    leaf = img.clone().requires_grad_(True)
    aug = V.augment(leaf, mean, std, noise, off1, off2, repeat)
    assert torch.equal(aug.detach().cpu(), aug_host)          # torch's device arithmetic is the host's here: the two sides see one aug
    loss = MLPFeatureLoss(model, layer, feature, c_feat)(aug) + c_tv * V.tv_value(aug, size)
    loss.backward()
    torch.cuda.synchronize()
    g_aug = V.unpatch_rows(viz._s.dcols.double().cpu(), repeat, size, 16)
    bound = 2 * V.grad_bound(g_aug, aug_host.double(), std.cpu().double(), off1, off2, repeat, c_tv, size)
    err = (viz.last_grad.cpu().double() - leaf.grad.cpu().double()).abs()
    ratio = (err / bound).max().item()
    print(f"fused step layer {layer}: worst |fused - eager| / (2 x bound) = {ratio:.3f}, |grad| max {float(leaf.grad.abs().max()):.3e}")
    assert ratio <= 1.0
    hist = viz.history[0].cpu()
    assert abs(float(hist[0]) - loss.item()) <= 1e-5 * (abs(float(hist[1])) + abs(float(hist[2])))
    assert all(p.grad is None for p in model.parameters())


# (layer, steps, repeat, images): the six-step run; then batches that are no multiple of 4, where a step's row of the packed table is
# not 16-byte aligned, one of them with two images (row b = r N + n)
@pytest.mark.parametrize("case", [(5, 5, 8, 1), (0, 2, 3, 1), (0, 2, 3, 2)], ids=["six_steps_r8", "three_steps_r3", "three_steps_n2_r3"])
def test_run_follows_the_parent_loop(tiny, case):
    _, model, feature = tiny
    layer, steps, repeat, images = case
    lr, c_feat, c_tv, size = 0.05, 1.0, 5e-5, 160
    torch.manual_seed(5)
    random.seed(5)
    viz = FeatureVisualizer(model, layer, feature, steps=steps, lr=lr, tv_coefficient=c_tv, feature_coefficient=c_feat, repeat=repeat,
                            images=images)
    start = visualize.new_init(size, images, device=DEV)
    viz.begin(start)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(steps + 1):
            viz.step(i)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    hist = viz.history.cpu()
    out = viz.image
    assert out.shape == start.shape and float(out.min()) >= 0 and float(out.max()) <= 1 and not torch.equal(out, start)
    # the parent path: the script's loop with MLPFeatureLoss in it, on the same draws
    img = start.clone().requires_grad_(True)
    opt = torch.optim.Adamax([img], lr=lr, betas=(0.5, 0.99), eps=1e-8)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps, 0.0)
    lf = MLPFeatureLoss(model, layer, feature, c_feat)
    losses = []
    for i in range(steps + 1):
        opt.zero_grad()
        mean, std, noise, (off1, off2) = _rows(viz, i)
        aug = V.augment(img, mean, std, noise, off1, off2, repeat)
        loss = lf(aug) + c_tv * V.tv_value(aug, size)
        losses.append(loss.item())
        loss.backward()
        opt.step()
        sched.step()
        img.data = img.data.clamp(0, 1)
    print(f"run {case}: fused", [f"{v:.5f}" for v in hist[:, 0].tolist()], "parent", [f"{v:.5f}" for v in losses])
    for a, b in zip(hist[:, 0].tolist(), losses):
        assert abs(a - b) <= 0.05 * abs(b), (hist[:, 0].tolist(), losses)
    if steps == 5:
        assert float(-hist[-1, 1]) > float(-hist[0, 1]), hist[:, 1].tolist()       # the feature term: c_feat * (1/B^2) sum_b m_b rises
    assert torch.allclose(hist[:, 0], hist[:, 1] + hist[:, 2], rtol=1e-6, atol=0)
    assert all(p.grad is None for p in model.parameters())


def test_feature_visualizer_refuses_what_it_does_not_build(tiny):
    _, model, feature = tiny
    viz = FeatureVisualizer(model, 0, feature, steps=2)
    with pytest.raises(_lib.OvhipError):
        viz(torch.zeros(1, 3, 160, 160))                      # a CPU tensor
    with pytest.raises(ValueError):
        viz(torch.zeros(1, 3, 152, 152, device=DEV))          # no multiple of the patch size
    with pytest.raises(ValueError):
        viz(torch.zeros(2, 3, 160, 160, device=DEV))          # built for one image


# ---- 7. the command line ---------------------------------------------------------------------------------------------------------------
CLI = "from openvision_amd.feature_visualization import main\nraise SystemExit(main(sys.argv[1:]))\n"


@pytest.mark.timeout(600)
def test_command_line_writes_the_png_of_the_in_process_run(tmp_path):
    from PIL import Image
    cfg = preset("vit-tiny-patch16-160")
    ck = str(tmp_path / "tiny-ckpt")
    checkpoint.save_pretrained(create_model(cfg, state_dict=synth.make_state_dict(cfg)), cfg, ck, safetensors=False)
    out = tmp_path / "out"
    run_child(CLI, "--use_model", ck, "--steps", "3", "--layer_range", "0", "--feature_range", "1", "--deterministic", "--output_folder",
              str(out), timeout=300, gpu=True)
    png = out / "tiny-ckpt_L0_F1.png"
    assert png.exists()
    pixels = np.asarray(Image.open(png))
    assert pixels.shape == (160, 160, 3) and pixels.dtype == np.uint8
    fix_random_seed()                                         # the command line's order: seed, load, construct, draw the image, run
    model, _ = checkpoint.from_pretrained(ck, device=DEV)
    viz = FeatureVisualizer(model, 0, 1, steps=3, lr=1.0, tv_coefficient=1.0 * 0.00005)
    image = viz(visualize.new_init(160, 1))
    assert np.array_equal(to_uint8(image), pixels)
