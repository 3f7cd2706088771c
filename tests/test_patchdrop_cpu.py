"""CPU: patch dropout's configuration, the reference's draw (PatchDropout.sample against a reference-generated fixture), the K formula,
eval mode consuming no random numbers, the argument errors of the Python surface and the C ABI (no HIP call), zero scratch of the
new kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

from openvision_amd import _lib, preset, training, visualize
from openvision_amd.config import vision_cfg_from
from openvision_amd.model import CLIP, PatchDropout, check_keep

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "patchdrop_tiny16_160.npz")


def tiny_cfg(p):
    cfg = preset("vit-tiny-patch16-160")
    return dict(cfg, vision_cfg=dict(cfg["vision_cfg"], patch_dropout=p))


def tiny_model(p):
    cfg = tiny_cfg(p)
    return CLIP(embed_dim=cfg["embed_dim"], vision_cfg=cfg["vision_cfg"], text_cfg=cfg["text_cfg"])


def test_config_accepts_patch_dropout_in_range():
    assert vision_cfg_from(tiny_cfg(0.5)["vision_cfg"]).patch_dropout == 0.5
    assert vision_cfg_from(tiny_cfg(0.0)["vision_cfg"]).patch_dropout == 0.0
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            vision_cfg_from(tiny_cfg(bad)["vision_cfg"])
    with pytest.raises(ValueError):            # still refused
        vision_cfg_from(dict(tiny_cfg(0.5)["vision_cfg"], ls_init_value=0.1))


def test_model_builds_with_patch_dropout_and_keeps_state_dict():
    m = tiny_model(0.5)
    assert isinstance(m.visual.patch_dropout, PatchDropout) and m.visual.patch_dropout.prob == 0.5
    m0 = tiny_model(0.0)
    assert isinstance(m0.visual.patch_dropout, torch.nn.Identity)
    assert sorted(m.state_dict()) == sorted(m0.state_dict())
    assert m.training and m.visual.dropout_active()
    m.eval()
    assert not m.visual.dropout_active()
    m.train()
    m.visual.eval()
    assert not m.visual.dropout_active()
    assert not m0.train().visual.dropout_active()


def test_sample_matches_reference_draw():
    g = np.load(GOLD)
    keep = torch.from_numpy(g["keep"])
    b, k = keep.shape
    assert (b, k) == (4, 50)
    pd = PatchDropout(float(g["p"]))
    torch.manual_seed(int(g["seed"]))
    got = pd.sample(b, 100)
    assert got.dtype == torch.int64 and torch.equal(got, keep)
    # the reference module's forward on a token tensor keeps the same rows, in that order, behind the CLS row
    x = torch.randn(b, 101, 8)
    torch.manual_seed(int(g["seed"]))
    y = pd.train()(x)
    assert torch.equal(y[:, 0], x[:, 0])
    assert torch.equal(y[:, 1:], x[:, 1:][torch.arange(b)[:, None], keep])


@pytest.mark.parametrize("p,g,k", [(0.5, 100, 50), (0.75, 256, 64), (0.5, 256, 128), (0.75, 2304, 576), (0.999, 100, 1),
                                   (0.3, 10, 7), (0.0001, 100, 99), (0.9, 5, 1)])
def test_num_keep_formula(p, g, k):
    pd = PatchDropout(p)
    assert pd.num_keep(g) == k == max(1, int(g * (1 - p)))
    torch.manual_seed(0)
    assert tuple(pd.sample(3, g).shape) == (3, k)


def test_probability_bounds():
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            PatchDropout(bad)


def test_eval_mode_consumes_no_rng():
    pd = PatchDropout(0.5).eval()
    x = torch.randn(2, 101, 8)
    state = torch.get_rng_state()
    assert pd(x) is x
    assert torch.equal(torch.get_rng_state(), state)
    pd.train()
    pd(x)
    assert not torch.equal(torch.get_rng_state(), state)          # training mode draws


def test_keep_table_checks_without_hip():
    check_keep(torch.zeros(2, 5, dtype=torch.int64), 2, 100)
    for bad, b in [(torch.zeros(3, 5, dtype=torch.int64), 2), (torch.zeros(2, 0, dtype=torch.int64), 2),
                   (torch.zeros(2, 101, dtype=torch.int64), 2), (torch.zeros(2, 5), 2), (torch.zeros(10, dtype=torch.int64), 2)]:
        with pytest.raises(ValueError):
            check_keep(bad, b, 100)
    m = tiny_model(0.5)
    img = torch.zeros(2, 3, 160, 160)
    with pytest.raises(ValueError):
        training.encode_image(m, img, keep=torch.zeros(2, 101, dtype=torch.int64))
    with pytest.raises(_lib.OvhipError):               # a CPU image: no fallback
        training.encode_image(m, img, keep=torch.arange(5).repeat(2, 1))


def test_feature_objective_refuses_active_dropout():
    m = tiny_model(0.5)
    img = torch.zeros(1, 3, 160, 160)
    with pytest.raises(_lib.OvhipError, match="patch_dropout"):
        visualize.mlp_feature(m, img, 0, 0)
    with pytest.raises(_lib.OvhipError, match="patch_dropout"):
        visualize.MLPFeatureLoss(m, 0, 0)(img)
    m.eval()
    with pytest.raises(_lib.OvhipError, match="MI355X"):            # past the dropout check: the CPU image is what is refused now
        visualize.mlp_feature(m, img, 0, 0)


def test_cabi_argument_validation():
    lib = _lib.load()
    a = ctypes.c_void_p(16)
    assert lib.ov_patch_keep_inverse(a, a, 2, 0, 100, None, None) == -1          # K outside [1, G]
    assert lib.ov_patch_keep_inverse(a, a, 2, 101, 100, None, None) == -1
    assert lib.ov_patch_keep_inverse(None, a, 2, 5, 100, None, None) == -1
    assert lib.ov_im2col_patches_keep(a, 0, a, a, 2, 160, 16, 0, 768, None) == -1
    assert lib.ov_im2col_patches_keep(a, 0, a, a, 2, 160, 16, 101, 768, None) == -1
    assert lib.ov_im2col_patches_keep(a, 0, None, a, 2, 160, 16, 5, 768, None) == -1
    assert lib.ov_patch_keep_assemble(a, 192, a, a, a, a, 2, 0, 100, 192, None) == -1
    assert lib.ov_patch_keep_assemble(a, 192, a, a, a, a, 2, 5, 100, 190, None) == -1
    assert lib.ov_patch_keep_assemble_backward(a, a, 2, 101, 100, 192, a, a, a, 192, None) == -1
    assert lib.ov_col2im_patches_keep(a, 768, a, a, 0, 2, 160, 16, 0, None) == -1
    assert lib.ov_col2im_patches_keep(a, 768, a, a, 0, 2, 162, 18, 5, None) == -1      # S % 4
    cfg = _lib.TowerCfg(192, 2, 3, 768, 768, 0, 1e-6)
    t = lib.ov_tower_create(ctypes.byref(cfg))
    try:
        h = _lib.VisionHead(160, 16, 768, 1, 1, 192, 192, a, a, a, a, a, a, a)
        assert lib.ov_vision_keep_workspace_bytes(t, ctypes.byref(h), 2, 0) == 0
        assert lib.ov_vision_keep_workspace_bytes(t, ctypes.byref(h), 2, 101) == 0
        n50 = lib.ov_vision_keep_workspace_bytes(t, ctypes.byref(h), 2, 50)
        assert 0 < n50 < lib.ov_vision_workspace_bytes(t, ctypes.byref(h), 2)
        assert lib.ov_encode_image_keep(t, ctypes.byref(h), a, 0, a, 2, 0, a, 1, None, a, 1 << 30, None) == -1
        assert lib.ov_encode_image_keep(t, ctypes.byref(h), a, 0, a, 2, 50, a, 1, None, a, n50 - 1, None) == -3
        assert lib.ov_vision_embed_keep(t, ctypes.byref(h), a, 0, a, 2, 101, a, None, a, 1 << 30, None) == -1
        assert lib.ov_vision_head_forward_tokens(t, ctypes.byref(h), a, 2, 1, a, 1, a, 1 << 30, None) == -1
    finally:
        lib.ov_tower_destroy(t)


@pytest.mark.timeout(900)
def test_patch_keep_kernels_use_no_scratch():
    from test_build_scratch import kernel_scratch
    res = kernel_scratch("embed.hip")
    names = ("im2col_keep_kernel", "keep_inverse_kernel", "keep_assemble_kernel", "keep_assemble_bwd_kernel", "col2im_keep_kernel")
    found = {k: v for k, v in res.items() if any(n in k for n in names)}
    assert len(found) == 7, sorted(res)                  # im2col / col2im: fp32 and bf16 images
    assert all(v == 0 for v in found.values()), found
