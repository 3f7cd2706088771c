"""CPU: the feature-visualisation objective (openvision_amd.visualize): C ABI of the tap kernels / input-only backward, zero scratch
of the new kernels, and an fp32 restatement from oracle pieces that reproduces the reference's fixture (featviz_tiny16_160.npz)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openvision_amd import _lib, synth
from openvision_amd import build as B
from openvision_amd.config import preset
from oracle import clip_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("ov_mlp_feature_forward", "ov_mlp_feature_backward", "ov_block_attn_forward_saving", "ov_block_attn_backward_input",
       "ov_block_attn_backward_input_workspace_bytes", "ov_tower_backward_input", "ov_tower_backward_input_workspace_bytes")


def featviz_oracle(image, sd, vcfg, layer, feature, eps=R.LN_EPS):
    """fp32 restatement of the script's objective: blocks [0, layer), the attention half of block `layer`, ln_2, one c_fc column, GELU,
    mean over the patch tokens; loss = -all_feats[:B, f].diag().mean() = -(1/B^2) sum_b m_b.  Returns (m [B], loss)."""
    heads = vcfg["width"] // vcfg["head_width"]
    x = R.patch_embed(image, sd, vcfg["patch_size"])
    for i in range(layer):
        x = R.resblock(x, sd, f"visual.transformer.resblocks.{i}.", heads, False, eps)
    p = f"visual.transformer.resblocks.{layer}."
    h = R.layer_norm(x, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"], eps)
    x1 = x + R.mha(h, sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"], sd[p + "attn.out_proj.weight"],
                   sd[p + "attn.out_proj.bias"], heads)
    n2 = R.layer_norm(x1, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"], eps)
    pre = n2 @ sd[p + "mlp.c_fc.weight"][feature] + sd[p + "mlp.c_fc.bias"][feature]
    m = R.gelu(pre, False)[:, 1:].mean(dim=1)
    return m, -m.sum() / float(m.shape[0] ** 2)


def test_new_symbols_exported_and_validate_without_hip():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert hasattr(raw, s) and s in _lib.SIGNATURES
    # null pointers / bad sizes: status codes before any HIP call (this machine has no device: a HIP call would fail differently)
    assert lib.ov_mlp_feature_forward(None, 192, None, None, None, 192, None, 0, 768, 0, 2, 101, 192, 1e-6, None, None, None) == -1
    assert lib.ov_mlp_feature_backward(None, 192, None, None, 192, 0, 768, 0, None, None, None, 192, 2, 101, 192, 1e-6, None) == -1
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    a = (buf.data_ptr() + 255) // 256 * 256
    # valid pointers, bad sizes / feature index: -1 (So400m: 4304 true hidden units, 4352 padded -- 4304 is not a feature)
    fwd = lambda f, mlp, B_, L, D: lib.ov_mlp_feature_forward(a, D, a, a, a, D, a, f, mlp, 0, B_, L, D, 1e-6, a, a, None)
    bwd = lambda f, mlp, B_, L, D: lib.ov_mlp_feature_backward(a, D, a, a, D, f, mlp, 0, a, a, a, D, B_, L, D, 1e-6, None)
    for fn in (fwd, bwd):
        assert fn(4304, 4304, 2, 257, 1152) == -1
        assert fn(-1, 768, 2, 101, 192) == -1
        assert fn(0, 768, 0, 101, 192) == -1
        assert fn(0, 768, 2, 1, 192) == -1            # L >= 2: the mean runs over tokens 1 .. L-1
        assert fn(0, 768, 2, 101, 0) == -1
        assert fn(0, 768, 2, 101, 196) == -2          # D % 8
    cfg = _lib.TowerCfg(192, 1, 3, 768, 768, 0, 1e-6)
    w = _lib.BlockWeights(*([a] * 12), None, None)
    assert lib.ov_block_attn_forward_saving(None, None, None, None, None, None, None, 2, 101, None) == -1
    assert lib.ov_block_attn_forward_saving(ctypes.byref(cfg), ctypes.byref(w), a, a, a, a, None, 0, 101, None) == -1
    assert lib.ov_block_attn_backward_input(None, None, None, None, None, None, None, None, 2, 101, None, 0, None) == -1
    assert lib.ov_block_attn_backward_input(ctypes.byref(cfg), ctypes.byref(w), a, a, a, None, a, a, 2, 0, a, 1 << 30, None) == -1
    assert lib.ov_block_attn_backward_input_workspace_bytes(None, 2, 101) == 0
    assert lib.ov_block_attn_backward_input_workspace_bytes(ctypes.byref(cfg), 2, 101) > 2 * 101 * 4 * 192 * 2
    assert lib.ov_block_attn_backward_input(ctypes.byref(cfg), ctypes.byref(w), a, a, a, None, a, a, 2, 101, a, 1024, None) == -3
    t = lib.ov_tower_create(ctypes.byref(_lib.TowerCfg(192, 2, 3, 768, 768, 0, 1e-6)))
    assert t
    assert lib.ov_tower_backward_input(t, None, None, 3, 101, None, 0, None) == -1
    assert lib.ov_tower_backward_input(t, a, a, 0, 101, a, 1 << 30, None) == -1
    assert lib.ov_tower_backward_input_workspace_bytes(None, 3, 101) == 0
    full, inp = lib.ov_tower_backward_workspace_bytes(t, 8, 257), lib.ov_tower_backward_input_workspace_bytes(t, 8, 257)
    assert 0 < inp < full                                  # no dW staging, partials or parameter sums
    assert lib.ov_tower_backward_input(t, a, a, 8, 257, a, inp - 1, None) == -3
    lib.ov_tower_destroy(t)


@pytest.mark.timeout(900)
def test_feature_kernels_use_no_scratch():
    out = subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", "-",
                          os.path.join(B.CSRC, "feature.hip")], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
    res = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", out)}
    mine = {k: v for k, v in res.items() if "mlp_feature" in k}
    assert len(mine) >= 3 * 5, sorted(res)                # pre / mean / bwd over the row-width variants
    assert all(v == 0 for v in mine.values()), mine
    assert "feature.hip" in B.SOURCES


def fixture_images(z):
    """The fixture's images, regenerated from their seed as the generator made them (stored as a checksum only)."""
    img = synth.make_structured_images(int(z["batch"]), int(z["image_size"]), seed=int(z["image_seed"])).half().float()
    assert abs(img.double().sum().item() - float(z["image_sum"])) <= 1e-6 * float(z["image_abs_sum"])
    assert abs(img.double().abs().sum().item() - float(z["image_abs_sum"])) <= 1e-6 * float(z["image_abs_sum"])
    return img


def fixture_pixel_grad(z, k, sd, vcfg):
    """The reference's d loss / d image of pair k: conv1 has stride = kernel, so it is conv_transpose2d of the stored (int8, per-group
    scaled) gradient at conv1's output -- what autograd computes for conv2d's input."""
    g = torch.from_numpy(z[f"convgrad_q_{k}"]).float() * torch.from_numpy(z[f"convgrad_s_{k}"])[:, None]
    return F.conv_transpose2d(g, sd["visual.conv1.weight"].float(), stride=vcfg["patch_size"])


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "featviz_tiny16_160.npz"))


def test_oracle_restatement_reproduces_reference_fixture(fixture):
    z = fixture
    cfg = preset(str(z["preset"]))
    sd = synth.make_state_dict(cfg, int(z["seed"]), str(z["variant"]))
    vcfg = cfg["vision_cfg"]
    img0 = fixture_images(z)
    for k, (layer, feature) in enumerate(zip(z["layers"].tolist(), z["features"].tolist())):
        img = img0.clone().requires_grad_(True)
        m, loss = featviz_oracle(img, sd, vcfg, layer, feature)
        loss.backward()
        want_m, want_loss = torch.from_numpy(z[f"m_{k}"]), float(z[f"loss_{k}"])
        assert torch.allclose(m.detach(), want_m, rtol=1e-4, atol=0), (layer, m, want_m)
        assert abs(loss.item() - want_loss) <= 1e-4 * abs(want_loss), (layer, loss.item(), want_loss)
        # the 1/B^2 factor is pinned: 1/B would be B times larger
        assert abs(-want_m.sum().item() / len(want_m) ** 2 - want_loss) <= 1e-4 * abs(want_loss)
        g = img.grad.flatten()
        gu = fixture_pixel_grad(z, k, sd, vcfg).flatten()
        assert F.cosine_similarity(g, gu, dim=0).item() >= 0.9999
        assert abs(g.norm().item() / float(z[f"grad_norm_{k}"]) - 1) < 1e-3
