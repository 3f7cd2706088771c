"""CPU: frozen-parameter training -- LiT locking (CLIP.lock_image_tower) against the reference's groups, the argument checks of the
partial tower entry points (no HIP call), and the parameter-only LayerNorm-backward rows' scratch."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest
import torch

from openvision_amd import _lib, preset
from openvision_amd import build as B
from openvision_amd.model import create_model
from conftest import GOLDEN


@pytest.fixture(scope="module")
def lock_groups():
    with open(os.path.join(GOLDEN, "lock_groups_tiny16_160.json")) as f:
        return json.load(f)


def test_lock_image_tower_matches_reference_groups(lock_groups):
    cfg = preset("vit-tiny-patch16-160")
    layers = cfg["vision_cfg"]["layers"]
    assert lock_groups["layers"] == layers
    m = create_model(cfg)
    assert sorted(n for n, _ in m.named_parameters()) == lock_groups["all"]
    ks = [0, 1, 2, 3, layers, layers + 1, layers + 2, layers + 5]
    assert sorted(int(k) for k in lock_groups["trainable"]) == sorted(ks)
    for k in ks:
        for p in m.parameters():
            p.requires_grad_(True)
        m.lock_image_tower(k)
        got = sorted(n for n, p in m.named_parameters() if p.requires_grad)
        assert got == lock_groups["trainable"][str(k)], k
    m.lock_image_tower(1, freeze_bn_stats=True)                   # accepted, no effect
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == lock_groups["trainable"]["1"]
    assert all(p.requires_grad for n, p in m.named_parameters() if not n.startswith("visual."))


def _tower(lib, D=192, layers=3, heads=3, mlp=768, blocks=True):
    """A tower whose blocks hold aligned placeholder pointers (never dereferenced: every call below fails validation first), so
    that each argument check is what rejects its case, not the missing blocks."""
    cfg = _lib.TowerCfg(D, layers, heads, mlp, mlp, 0, 1e-6)
    t = lib.ov_tower_create(C.byref(cfg))
    assert t
    if blocks:
        for i in range(layers):
            w = _lib.BlockWeights(*[C.c_void_p((1 << 24) + 4096 * (12 * i + j)) for j in range(12)], None, None)
            assert lib.ov_tower_set_block(t, i, C.byref(w)) == 0
    return t


def _grads(n, half=None, frozen=(), misaligned=None):
    gs = []
    for i in range(n):
        ptrs = [None if (i, j // 2) in frozen else C.c_void_p((1 << 20) + 256 * (12 * i + j)) for j in range(12)]
        if half is not None and half[0] == i:
            ptrs[half[1]] = None
        if misaligned is not None and misaligned[0] == i:
            ptrs[misaligned[1]] = C.c_void_p((1 << 20) + 256 * (12 * i + misaligned[1]) + 4)
        gs.append(_lib.BlockGrads(*ptrs))
    return (_lib.BlockGrads * n)(*gs)


def test_partial_entry_points_validate_without_hip():
    lib = _lib.load()
    layers, Bn, L = 3, 8, 257
    t = _tower(lib, layers=layers)
    try:
        full = lib.ov_tower_saved_bytes(t, Bn, L)
        for first in range(layers + 1):
            assert lib.ov_tower_saved_bytes_from(t, first, Bn, L) * layers == (layers - first) * full, first
        assert lib.ov_tower_saved_bytes_from(t, layers, Bn, L) == 0
        assert lib.ov_tower_saved_bytes_from(t, -1, Bn, L) == 0 and lib.ov_tower_saved_bytes_from(t, layers + 1, Bn, L) == 0
        assert lib.ov_tower_saved_bytes_from(None, 0, Bn, L) == 0
        # the layers below `first` need one slot's intermediates (its x part excepted); none when every layer is kept
        assert lib.ov_tower_forward_saving_from_workspace_bytes(t, 0, Bn, L) == 0
        one = lib.ov_tower_forward_saving_from_workspace_bytes(t, 1, Bn, L)
        assert 0 < one < full // layers and one == lib.ov_tower_forward_saving_from_workspace_bytes(t, layers, Bn, L)
        assert lib.ov_tower_backward_partial_workspace_bytes(t, Bn, L) == lib.ov_tower_backward_workspace_bytes(t, Bn, L)
        assert lib.ov_tower_backward_partial_workspace_bytes(None, Bn, L) == 0

        # every call below is invalid in exactly one argument (the blocks are set): nothing may get as far as a launch
        a = C.c_void_p(1 << 20)
        big = 1 << 40
        fwd = lib.ov_tower_forward_saving_from
        for first in (-1, layers + 1):
            assert fwd(t, first, a, a, Bn, L, a, big, None) == -1, first
        assert fwd(None, 0, a, a, Bn, L, a, big, None) == -1
        assert fwd(t, 0, None, a, Bn, L, a, big, None) == -1          # x
        assert fwd(t, 1, a, None, Bn, L, a, big, None) == -1          # saved, first < layers
        assert fwd(t, 1, a, a, Bn, L, None, big, None) == -1          # workspace, first > 0
        assert fwd(t, 1, a, a, Bn, L, a, one - 1, None) == -3         # workspace too small
        assert fwd(t, layers, a, None, Bn, L, a, one - 1, None) == -3
        assert fwd(t, 1, a, a, 0, L, a, big, None) == -1
        assert fwd(t, 0, C.c_void_p((1 << 20) + 2), a, Bn, L, a, big, None) == -1   # misaligned x
        assert fwd(t, 0, a, C.c_void_p((1 << 20) + 8), Bn, L, a, big, None) == -1   # misaligned saved

        bwd = lib.ov_tower_backward_partial
        nb = lib.ov_tower_backward_partial_workspace_bytes(t, Bn, L)
        for first in (-1, layers + 1):
            assert bwd(t, first, a, a, _grads(layers), 1, Bn, L, a, nb, None) == -1, first
        assert bwd(None, 0, a, a, _grads(layers), 1, Bn, L, a, nb, None) == -1
        assert bwd(t, 0, None, a, _grads(layers), 1, Bn, L, a, nb, None) == -1          # saved
        assert bwd(t, 0, a, None, _grads(layers), 1, Bn, L, a, nb, None) == -1          # dx
        assert bwd(t, 0, a, a, None, 1, Bn, L, a, nb, None) == -1                      # grads
        assert bwd(t, 0, a, a, _grads(layers), 1, Bn, L, None, nb, None) == -1         # workspace
        assert bwd(t, 0, a, a, _grads(layers), 1, 0, L, a, nb, None) == -1             # B
        for blk in range(layers):                                                       # a pair with one NULL pointer
            for j in (0, 3, 6, 9, 11):
                assert bwd(t, 0, a, a, _grads(layers, half=(blk, j)), 0, Bn, L, a, nb, None) == -1, (blk, j)
        assert bwd(t, 1, a, a, _grads(layers - 1, half=(layers - 2, 4)), 1, Bn, L, a, nb, None) == -1
        for blk, j in ((0, 1), (layers - 1, 10), (1, 7)):                              # a misaligned gradient pointer
            assert bwd(t, 0, a, a, _grads(layers, misaligned=(blk, j)), 1, Bn, L, a, nb, None) == -1, (blk, j)
        assert bwd(t, 0, a, a, _grads(layers), 1, Bn, L, a, nb - 1, None) == -3         # workspace too small
        frozen_all = _grads(layers, frozen={(i, k) for i in range(layers) for k in range(6)})
        assert bwd(t, 0, a, a, frozen_all, 1, Bn, L, a, nb - 1, None) == -3
        assert bwd(t, 0, C.c_void_p((1 << 20) + 4), a, _grads(layers), 1, Bn, L, a, nb, None) == -1   # misaligned saved
        assert bwd(t, 0, a, C.c_void_p((1 << 20) + 4), _grads(layers), 1, Bn, L, a, nb, None) == -1   # misaligned dx
        # nothing kept: nothing to do (and nothing read)
        assert bwd(t, layers, None, a, None, 1, Bn, L, None, 0, None) == 0
    finally:
        lib.ov_tower_destroy(t)


def test_partial_entry_points_need_every_block_without_hip():
    lib = _lib.load()
    t = _tower(lib, layers=3, blocks=False)
    try:
        a = C.c_void_p(1 << 20)
        nb = lib.ov_tower_backward_partial_workspace_bytes(t, 2, 101)
        assert lib.ov_tower_forward_saving_from(t, 3, a, None, 2, 101, a, 1 << 40, None) == -1
        assert lib.ov_tower_backward_partial(t, 0, a, a, _grads(3), 1, 2, 101, a, nb, None) == -1
    finally:
        lib.ov_tower_destroy(t)


def test_partial_backward_rejects_folded_weights_without_hip():
    lib = _lib.load()
    t = _tower(lib, layers=2, blocks=False)
    try:
        a = C.c_void_p(1 << 20)
        for i in range(2):
            w = _lib.BlockWeights(*([a] * 12), a, a)                 # LN folded (qkv_colsum / fc_colsum set)
            assert lib.ov_tower_set_block(t, i, C.byref(w)) == 0
        g = (_lib.BlockGrads * 2)(*[_lib.BlockGrads(*([a] * 12)) for _ in range(2)])
        nb = lib.ov_tower_backward_partial_workspace_bytes(t, 2, 101)
        assert lib.ov_tower_backward_partial(t, 0, a, a, g, 1, 2, 101, a, nb, None) == -1
        assert lib.ov_tower_forward_saving_from(t, 1, a, a, 2, 101, a, 1 << 40, None) == -1
    finally:
        lib.ov_tower_destroy(t)


def test_tower_backward_checks_every_layer_before_its_first_launch_without_hip():
    """ov_tower_backward needs every pair of every layer: a NULL or half-NULL pair, or a misaligned pointer, in a layer BELOW the top
    one is rejected before anything runs (not after the layers above have run); folded weights in any layer are OV_ERR_UNSUPPORTED."""
    lib = _lib.load()
    layers, Bn, L = 3, 8, 257
    t = _tower(lib, layers=layers)
    try:
        a = C.c_void_p(1 << 20)
        nb = lib.ov_tower_backward_workspace_bytes(t, Bn, L)
        bwd = lib.ov_tower_backward
        for blk in range(layers):
            for j in (0, 5, 11):
                assert bwd(t, a, a, _grads(layers, half=(blk, j)), Bn, L, a, nb, None) == -1, (blk, j)
            assert bwd(t, a, a, _grads(layers, frozen={(blk, 2)}), Bn, L, a, nb, None) == -1, blk
        assert bwd(t, a, a, _grads(layers, misaligned=(0, 7)), Bn, L, a, nb, None) == -1
        # the order of the codes: the top layer's checks, the workspace, the alignment, the layers below
        assert bwd(t, a, a, _grads(layers, half=(layers - 1, 4)), Bn, L, a, nb - 1, None) == -1
        assert bwd(t, a, a, _grads(layers, half=(0, 4)), Bn, L, a, nb - 1, None) == -3
        assert bwd(t, a, a, _grads(layers), Bn, L, a, nb - 1, None) == -3
        assert bwd(t, a, C.c_void_p((1 << 20) + 4), _grads(layers), Bn, L, a, nb, None) == -1
    finally:
        lib.ov_tower_destroy(t)
    t = _tower(lib, layers=2, blocks=False)
    try:
        a = C.c_void_p(1 << 20)
        nb = lib.ov_tower_backward_workspace_bytes(t, 2, 101)
        for folded in (0, 1):
            for i in range(2):
                w = _lib.BlockWeights(*([a] * 12), *((a, a) if i == folded else (None, None)))
                assert lib.ov_tower_set_block(t, i, C.byref(w)) == 0
            assert lib.ov_tower_backward(t, a, a, _grads(2), 2, 101, a, nb, None) == -2, folded
    finally:
        lib.ov_tower_destroy(t)


@pytest.mark.timeout(900)
def test_layernorm_backward_rows_use_no_scratch():
    out = subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", "-",
                          os.path.join(B.CSRC, "backward.hip")], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
    res = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", out)}
    rows = {k: v for k, v in res.items() if "layernorm_bwd_rows" in k}
    params_only = {k: v for k, v in rows.items() if "Lb1ELb0E" in k}     # <NCH, PARAMS = true, DX = false>
    assert len(params_only) == 5, sorted(rows)                           # NCH = 1, 2, 3, 4, 8
    assert all(v == 0 for v in rows.values()), rows
