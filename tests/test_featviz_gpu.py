"""GPU: feature visualisation (openvision_amd.visualize) -- the tap kernels against fp32 torch, the input-only tower backward against
ov_tower_backward (bitwise), the objective and its image gradient against the reference's fixture and the fp32 oracle, a short
Adamax run, and the argument errors."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from openvision_amd import _lib, preset, synth
from openvision_amd._lib import ptr, stream_ptr
from openvision_amd.model import create_model
from openvision_amd.visualize import MLPFeatureLoss, mlp_feature
from conftest import golden
from oracle import clip_ref as R
from test_featviz_cpu import featviz_oracle, fixture_images, fixture_pixel_grad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gelu(a, tanh):
    return F.gelu(a, approximate="tanh" if tanh else "none")


# ---- tap kernels alone --------------------------------------------------------------------------------------------------------------
def _tap_case(lib, g, D, L, Bn, tanh, feature, mlp, mlp_pad):
    M = Bn * L
    x1 = (torch.randn(M, D, generator=g) * 1.5 + 0.2).to(torch.bfloat16)
    gam = torch.randn(D, generator=g) * 0.2 + 1.0
    bet = torch.randn(D, generator=g) * 0.1
    w = (torch.randn(mlp_pad, D, generator=g) * D ** -0.5).to(torch.bfloat16)
    w[mlp:] = 0
    b = torch.randn(mlp_pad, generator=g) * 0.5
    dmean = torch.randn(Bn, generator=g)
    # fp32 torch on the same (bf16-valued) inputs
    xr = x1.float().requires_grad_(True)
    pre_r = F.layer_norm(xr, (D,), gam, bet, 1e-6) @ w[feature].float() + b[feature]
    mean_r = _gelu(pre_r, tanh).view(Bn, L)[:, 1:].mean(dim=1)
    (mean_r * dmean).sum().backward()
    d = lambda t: t.to(DEV).contiguous()
    x1d, gd, bd, wd, bbd, dmd = d(x1), d(gam), d(bet), d(w), d(b), d(dmean)
    outs = []
    for _ in range(2):
        pre = torch.empty(M, device=DEV)
        mean = torch.empty(Bn, device=DEV)
        dx1 = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
        _lib.check(lib.ov_mlp_feature_forward(ptr(x1d), D, ptr(gd), ptr(bd), ptr(wd), D, ptr(bbd), feature, mlp, int(tanh), Bn, L, D, 1e-6,
                                              ptr(pre), ptr(mean), stream_ptr()), "ov_mlp_feature_forward")
        _lib.check(lib.ov_mlp_feature_backward(ptr(x1d), D, ptr(gd), ptr(wd), D, feature, mlp, int(tanh), ptr(pre), ptr(dmd), ptr(dx1), D,
                                               Bn, L, D, 1e-6, stream_ptr()), "ov_mlp_feature_backward")
        torch.cuda.synchronize()
        outs.append((pre.cpu(), mean.cpu(), dx1.cpu()))
    (pre, mean, dx1), (pre2, mean2, dx12) = outs
    tag = (D, L, Bn, tanh, feature)
    assert torch.equal(pre, pre2) and torch.equal(mean, mean2) and torch.equal(dx1, dx12), f"not bitwise repeatable {tag}"
    scale = pre_r.detach().abs().max().item() + 1
    assert (pre - pre_r.detach()).abs().max().item() < 2e-5 * scale * D ** 0.5, tag
    assert (mean - mean_r.detach()).abs().max().item() < 1e-4 * (mean_r.detach().abs().max().item() + 1), tag
    assert dx1.view(Bn, L, D)[:, 0].abs().max().item() == 0, tag                     # the CLS row is not in the objective
    cos = F.cosine_similarity(dx1.float().flatten(), xr.grad.flatten(), dim=0).item()
    assert cos >= 0.999, (tag, cos)


def test_tap_kernels_against_fp32_torch():
    lib = _lib.load()
    g = torch.Generator().manual_seed(7)
    mlps = {192: (768, 768), 1024: (4096, 4096), 1152: (4304, 4352), 1280: (5120, 5120)}
    for D, (mlp, mlp_pad) in mlps.items():
        for L in (101, 257):
            for Bn in (1, 8):
                for tanh in (False, True):
                    for feature in (0, mlp - 1):
                        _tap_case(lib, g, D, L, Bn, tanh, feature, mlp, mlp_pad)


# ---- input-only tower backward: bitwise the dx of the full backward -----------------------------------------------------------------
def _rand_tower(lib, g, D, layers, heads, mlp):
    cfg = _lib.TowerCfg(D, layers, heads, mlp, mlp, 0, 1e-6)
    t = lib.ov_tower_create(C.byref(cfg))
    assert t
    keep = []
    for i in range(layers):
        mat = lambda n, k: (torch.randn(n, k, generator=g) * k ** -0.5).to(torch.bfloat16).to(DEV)
        vec = lambda n, s=0.02, m=0.0: (torch.randn(n, generator=g) * s + m).to(DEV)
        ts = [vec(D, 0.1, 1.0), vec(D), mat(3 * D, D), vec(3 * D), mat(D, D), vec(D), vec(D, 0.1, 1.0), vec(D), mat(mlp, D), vec(mlp),
              mat(D, mlp), vec(D)]
        keep.append(ts)
        _lib.check(lib.ov_tower_set_block(t, i, C.byref(_lib.BlockWeights(*[C.c_void_p(x.data_ptr()) for x in ts], None, None))), "set")
    return t, keep


@pytest.mark.parametrize("shape", [(192, 3, 3, 768, 3, 101), (1024, 4, 16, 4096, 8, 257)], ids=["tiny_b3_l101", "l14_4blk_b8_l257"])
def test_tower_backward_input_bitwise_equals_full_backward(shape):
    D, layers, heads, mlp, Bn, L = shape
    lib = _lib.load()
    g = torch.Generator().manual_seed(11)
    t, keep = _rand_tower(lib, g, D, layers, heads, mlp)
    try:
        M = Bn * L
        x = torch.randn(M, D, generator=g).to(torch.bfloat16).to(DEV)
        dy = (torch.randn(M, D, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
        saved = torch.empty(lib.ov_tower_saved_bytes(t, Bn, L), dtype=torch.uint8, device=DEV)
        nb = lib.ov_tower_workspace_bytes(t, Bn, L)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ov_tower_forward_saving(t, ptr(x), ptr(saved), Bn, L, ptr(ws), nb, stream_ptr()), "forward_saving")
        grads = [[torch.empty_like(p) for p in ts] for ts in keep]
        garr = (_lib.BlockGrads * layers)(*[_lib.BlockGrads(*[C.c_void_p(p.data_ptr()) for p in gs]) for gs in grads])
        dx_full = dy.clone()
        nb = lib.ov_tower_backward_workspace_bytes(t, Bn, L)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ov_tower_backward(t, ptr(saved), ptr(dx_full), garr, Bn, L, ptr(ws), nb, stream_ptr()), "ov_tower_backward")
        dx_in = dy.clone()
        nbi = lib.ov_tower_backward_input_workspace_bytes(t, Bn, L)
        assert 0 < nbi < nb
        wsi = torch.empty(nbi, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ov_tower_backward_input(t, ptr(saved), ptr(dx_in), Bn, L, ptr(wsi), nbi, stream_ptr()), "ov_tower_backward_input")
        torch.cuda.synchronize()
        assert torch.isfinite(dx_full.float()).all() and dx_full.float().abs().max().item() > 0
        assert torch.equal(dx_in, dx_full)
    finally:
        lib.ov_tower_destroy(t)


# ---- model level --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fv():
    return golden("featviz_tiny16_160.npz")


@pytest.fixture(scope="module")
def tiny_fv(fv):
    cfg = preset(str(fv["preset"]))
    sd = synth.make_state_dict(cfg, int(fv["seed"]), str(fv["variant"]))
    return cfg, sd, create_model(cfg, device=DEV, state_dict=sd)


def _rel(a, b):
    return (torch.as_tensor(a, dtype=torch.float64) - torch.as_tensor(b, dtype=torch.float64)).abs().max().item() / \
        torch.as_tensor(b, dtype=torch.float64).abs().max().item()


def test_tiny_objective_and_image_gradient_against_reference_fixture(fv, tiny_fv):
    cfg, sd, model = tiny_fv
    img0 = fixture_images(fv).to(DEV)
    for k, (layer, feature) in enumerate(zip(fv["layers"].tolist(), fv["features"].tolist())):
        img = img0.clone().requires_grad_(True)
        m = mlp_feature(model, img, layer, feature)
        loss = -m.sum() / float(m.shape[0] ** 2)
        loss.backward()
        torch.cuda.synchronize()
        want_m, want_loss = fv[f"m_{k}"], float(fv[f"loss_{k}"])
        tol_m = max(2 * _rel(fv[f"m_refbf16_{k}"], want_m), 2e-3)
        tol_l = max(2 * _rel(float(fv[f"loss_refbf16_{k}"]), want_loss), 2e-3)
        assert _rel(m.detach().cpu(), want_m) <= tol_m, (layer, m.tolist(), want_m)
        assert _rel(loss.item(), want_loss) <= tol_l, (layer, loss.item(), want_loss)
        g = img.grad.float().cpu().flatten()
        gu = fixture_pixel_grad(fv, k, sd, cfg["vision_cfg"]).flatten()
        cos = F.cosine_similarity(g, gu, dim=0).item()
        ratio = g.norm().item() / float(fv[f"grad_norm_{k}"])
        assert cos >= 0.99 and abs(ratio - 1) < 0.05, (layer, cos, ratio, float(fv[f"grad_cos_refbf16_{k}"]))
    for name, p in model.named_parameters():
        assert p.grad is None, f"{name} received a gradient"


def test_mlp_feature_loss_surface_and_bf16_image(fv, tiny_fv):
    _, _, model = tiny_fv
    img = fixture_images(fv).to(DEV).to(torch.bfloat16).requires_grad_(True)
    layer, feature = int(fv["layers"][1]), int(fv["features"][1])
    lf = MLPFeatureLoss(model, layer, feature, coefficient=2.0)
    out = lf(img)
    out.backward()
    assert abs(out.item() - 2.0 * lf.last_value) < 1e-6 and img.grad is not None and img.grad.dtype == torch.bfloat16
    assert _rel(lf.last_value, float(fv["loss_1"])) < 2e-2
    assert lf.name and str(lf) and lf.reset() == 0


@pytest.mark.timeout(1800)
def test_large14_224_synthetic_against_device_oracle():
    cfg = preset("vit-large-patch14-224")
    sd = synth.make_state_dict(cfg, 0, "v1")          # 'sharp' amplifies rounding: 23 bf16 blocks land at gradient cosine 0.93 there
    model = create_model(cfg, device=DEV, state_dict=sd)
    vcfg = cfg["vision_cfg"]
    sdv = {k: v.to(DEV).float() for k, v in sd.items() if k.startswith("visual.")}
    sdb = {k: v.to(torch.bfloat16) for k, v in sdv.items()}
    img0 = synth.make_structured_images(8, 224, seed=61).to(DEV)
    heads = vcfg["width"] // vcfg["head_width"]
    for layer in (0, 23):
        with torch.no_grad():                          # the unit with the largest mean activation over the batch
            x = R.patch_embed(img0, sdv, vcfg["patch_size"])
            for i in range(layer):
                x = R.resblock(x, sdv, f"visual.transformer.resblocks.{i}.", heads, False)
            p = f"visual.transformer.resblocks.{layer}."
            x1 = x + R.mha(R.layer_norm(x, sdv[p + "ln_1.weight"], sdv[p + "ln_1.bias"]), sdv[p + "attn.in_proj_weight"],
                            sdv[p + "attn.in_proj_bias"], sdv[p + "attn.out_proj.weight"], sdv[p + "attn.out_proj.bias"], heads)
            hid = F.gelu(F.linear(R.layer_norm(x1, sdv[p + "ln_2.weight"], sdv[p + "ln_2.bias"]), sdv[p + "mlp.c_fc.weight"],
                                  sdv[p + "mlp.c_fc.bias"]))
            feature = int(hid[:, 1:].mean(dim=(0, 1)).argmax())
            del x, x1, hid
        ir = img0.clone().requires_grad_(True)
        m_r, loss_r = featviz_oracle(ir, sdv, vcfg, layer, feature)
        loss_r.backward()
        with torch.no_grad():
            m_b, loss_b = featviz_oracle(img0.to(torch.bfloat16), sdb, vcfg, layer, feature)   # bf16 budget of the same formula
        img = img0.clone().requires_grad_(True)
        m = mlp_feature(model, img, layer, feature)
        loss = -m.sum() / 64.0
        loss.backward()
        torch.cuda.synchronize()
        tol_m = max(2 * _rel(m_b.float().cpu(), m_r.detach().cpu()), 2e-3)
        tol_l = max(2 * _rel(loss_b.float().item(), loss_r.item()), 2e-3)
        assert _rel(m.detach().cpu(), m_r.detach().cpu()) <= tol_m, (layer, feature, m.tolist(), m_r.tolist())
        assert _rel(loss.item(), loss_r.item()) <= tol_l, (layer, loss.item(), loss_r.item())
        cos = F.cosine_similarity(img.grad.flatten(), ir.grad.flatten(), dim=0).item()
        ratio = img.grad.norm().item() / ir.grad.norm().item()
        assert cos >= 0.99 and abs(ratio - 1) < 0.05, (layer, feature, cos, ratio)
    assert all(p.grad is None for p in model.parameters())


def _tv(x, size):
    """TotalVariation(2, size) of the script (cliptoolsoptimized.py:719-730, 840-847), restated."""
    n = lambda t: t.norm(p=2, dim=(2, 3)).mean()
    tv = n(x[:, :, :, 1:] - x[:, :, :, :-1]) + n(x[:, :, 1:, :] - x[:, :, :-1, :]) + n(x[:, :, 1:, 1:] - x[:, :, :-1, :-1]) + \
        n(x[:, :, 1:, :-1] - x[:, :, :-1, 1:])
    return tv * x.shape[-2] * x.shape[-1] / (size * size)


def test_short_adamax_run_matches_oracle_objective(fv, tiny_fv):
    cfg, sd, model = tiny_fv
    vcfg = cfg["vision_cfg"]
    sdv = {k: v.to(DEV).float() for k, v in sd.items() if k.startswith("visual.")}
    layer, feature = int(fv["layers"][1]), int(fv["features"][1])
    g = torch.Generator().manual_seed(5)
    start = (torch.rand(1, 3, 160, 160, generator=g) * 0.2 - 0.1).to(DEV)
    tv_coef = 1.0 * 0.00005                                 # --tv 1.0 times --coeff 5e-5 (ov-feature-visualization.py:60-61)
    curves, feats = {}, {}
    for who in ("hip", "oracle"):
        img = start.clone().requires_grad_(True)
        opt = torch.optim.Adamax([img], lr=0.05)
        lf = MLPFeatureLoss(model, layer, feature)
        cur, ms = [], []
        for _ in range(5):
            opt.zero_grad()
            x = img.repeat(8, 1, 1, 1)                       # RepeatBatch(8)
            if who == "hip":
                obj = lf(x)
                ms.append(-lf.last_value * 64)
            else:
                m, obj = featviz_oracle(x, sdv, vcfg, layer, feature)
                ms.append(m.sum().item())
            loss = obj + tv_coef * _tv(x, 160)
            loss.backward()
            opt.step()
            cur.append(loss.item())
        curves[who], feats[who] = cur, ms
    for a, b in zip(curves["hip"], curves["oracle"]):
        assert abs(a - b) <= 0.05 * abs(b), (curves["hip"], curves["oracle"])
    assert feats["hip"][-1] > feats["hip"][0], feats["hip"]
    assert all(p.grad is None for p in model.parameters())


def test_argument_errors(tiny_fv):
    _, _, model = tiny_fv
    img = torch.zeros(1, 3, 160, 160, device=DEV)
    with pytest.raises(_lib.OvhipError):
        mlp_feature(model, img, 12, 0)                           # layer == layers
    with pytest.raises(_lib.OvhipError):
        mlp_feature(model, img, -1, 0)
    with pytest.raises(_lib.OvhipError):
        mlp_feature(model, img, 0, 768)                          # feature == mlp
    with pytest.raises(_lib.OvhipError):
        mlp_feature(model, img.cpu(), 0, 0)
    # So400m-shaped MLP: 4304 true hidden units padded to 4352 -- the padding columns are not features
    cfg = preset("vit-so400m-patch14-224")
    cfg["vision_cfg"]["layers"] = 1
    cfg["text_cfg"]["layers"] = 1
    so = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    blk = so.visual.transformer.resblocks[0]
    assert blk.mlp_dim == 4304 and blk.mlp_pad == 4352
    x = torch.zeros(1, 3, 224, 224, device=DEV)
    with pytest.raises(_lib.OvhipError):
        mlp_feature(so, x, 0, 4304)
    assert torch.isfinite(mlp_feature(so, x, 0, 4303)).all()    # the last true unit is one
