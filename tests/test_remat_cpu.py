"""CPU: activation recomputation (CLIP.set_grad_checkpointing) -- the public flag, the checkpointed tower entry points' exports,
byte formulas and argument checks (no HIP call: every call below fails validation before its first launch)."""
import ctypes as C

from openvision_amd import _lib, preset
from openvision_amd.model import VisionTransformer, create_model

NEW = ("ov_tower_checkpoint_bytes", "ov_tower_slot_bytes", "ov_tower_forward_checkpointed", "ov_tower_backward_checkpointed")


def test_set_grad_checkpointing_sets_both_towers():
    m = create_model(preset("vit-tiny-patch16-160"))
    assert not m.visual.transformer.grad_checkpointing and not m.transformer.grad_checkpointing
    m.set_grad_checkpointing(True)
    assert m.visual.transformer.grad_checkpointing is True and m.transformer.grad_checkpointing is True
    m.set_grad_checkpointing(False)
    assert m.visual.transformer.grad_checkpointing is False and m.transformer.grad_checkpointing is False
    m.set_grad_checkpointing()                                         # enable=True by default, as in the reference
    assert m.visual.transformer.grad_checkpointing and m.transformer.grad_checkpointing
    assert callable(getattr(VisionTransformer, "set_grad_checkpointing", None))
    m.visual.set_grad_checkpointing(False)
    assert not m.visual.transformer.grad_checkpointing and m.transformer.grad_checkpointing


def test_checkpointed_symbols_exported_and_bound():
    lib = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    loaded = _lib.load()
    assert all(getattr(loaded, s).argtypes for s in NEW)


def _tower(lib, D=192, layers=3, heads=3, mlp=768, blocks=True):
    """Blocks with aligned placeholder pointers (never dereferenced: every call below fails validation first)."""
    cfg = _lib.TowerCfg(D, layers, heads, mlp, mlp, 0, 1e-6)
    t = lib.ov_tower_create(C.byref(cfg))
    assert t
    if blocks:
        for i in range(layers):
            w = _lib.BlockWeights(*[C.c_void_p((1 << 24) + 4096 * (12 * i + j)) for j in range(12)], None, None)
            assert lib.ov_tower_set_block(t, i, C.byref(w)) == 0
    return t


def _grads(n, half=None, misaligned=None):
    gs = []
    for i in range(n):
        ptrs = [C.c_void_p((1 << 20) + 256 * (12 * i + j)) for j in range(12)]
        if half is not None and half[0] == i:
            ptrs[half[1]] = None
        if misaligned is not None and misaligned[0] == i:
            ptrs[misaligned[1]] = C.c_void_p((1 << 20) + 256 * (12 * i + misaligned[1]) + 4)
        gs.append(_lib.BlockGrads(*ptrs))
    return (_lib.BlockGrads * n)(*gs)


def test_checkpoint_and_slot_bytes():
    lib = _lib.load()
    for D, layers, heads, mlp, Bn, L in ((192, 3, 3, 768, 8, 257), (1024, 24, 16, 4096, 256, 257), (640, 3, 8, 2560, 3, 101)):
        t = _tower(lib, D, layers, heads, mlp, blocks=False)
        try:
            for first in range(layers + 1):
                assert lib.ov_tower_checkpoint_bytes(t, first, Bn, L) == (layers - first) * Bn * L * D * 2, (D, first)
            slot = lib.ov_tower_slot_bytes(t, Bn, L)
            assert slot == lib.ov_tower_forward_saving_from_workspace_bytes(t, 1, Bn, L) > 0
            # a kept layer of the saving path = its x part + the slot
            assert lib.ov_tower_saved_bytes(t, Bn, L) == layers * (Bn * L * D * 2 + slot)
            for bad in ((-1, Bn, L), (layers + 1, Bn, L), (0, 0, L), (0, Bn, 0), (0, -2, L)):
                assert lib.ov_tower_checkpoint_bytes(t, *bad) == 0, bad
            assert lib.ov_tower_slot_bytes(t, 0, L) == 0 and lib.ov_tower_slot_bytes(t, Bn, 0) == 0
        finally:
            lib.ov_tower_destroy(t)
    assert lib.ov_tower_checkpoint_bytes(None, 0, 8, 257) == 0 and lib.ov_tower_slot_bytes(None, 8, 257) == 0


def test_checkpointed_entry_points_validate_without_hip():
    lib = _lib.load()
    layers, Bn, L = 3, 8, 257
    t = _tower(lib, layers=layers)
    try:
        a = C.c_void_p(1 << 20)
        big = 1 << 40
        ns = lib.ov_tower_slot_bytes(t, Bn, L)
        fwd = lib.ov_tower_forward_checkpointed
        for first in (-1, layers + 1):
            assert fwd(t, first, a, a, a, big, Bn, L, None) == -1, first
        assert fwd(None, 0, a, a, a, big, Bn, L, None) == -1
        assert fwd(t, 0, None, a, a, big, Bn, L, None) == -1            # x
        assert fwd(t, 1, a, None, a, big, Bn, L, None) == -1            # ckpt, first < layers
        assert fwd(t, 0, a, a, None, big, Bn, L, None) == -1            # slot
        assert fwd(t, 0, a, a, a, ns - 1, Bn, L, None) == -3            # slot too small
        assert fwd(t, layers, a, None, a, ns - 1, Bn, L, None) == -3
        assert fwd(t, 0, a, a, a, big, 0, L, None) == -1
        assert fwd(t, 0, a, a, a, big, Bn, 0, None) == -1
        assert fwd(t, 0, C.c_void_p((1 << 20) + 2), a, a, big, Bn, L, None) == -1   # misaligned x
        assert fwd(t, 0, a, C.c_void_p((1 << 20) + 8), a, big, Bn, L, None) == -1   # misaligned ckpt
        assert fwd(t, 0, a, a, C.c_void_p((1 << 20) + 4), big, Bn, L, None) == -1   # misaligned slot

        bwd = lib.ov_tower_backward_checkpointed
        nb = lib.ov_tower_backward_partial_workspace_bytes(t, Bn, L)
        g = _grads(layers)
        for first in (-1, layers + 1):
            assert bwd(t, first, a, a, ns, 0, a, g, 1, Bn, L, a, nb, None) == -1, first
        assert bwd(None, 0, a, a, ns, 0, a, g, 1, Bn, L, a, nb, None) == -1
        assert bwd(t, 0, None, a, ns, 0, a, g, 1, Bn, L, a, nb, None) == -1           # ckpt
        assert bwd(t, 0, a, None, ns, 0, a, g, 1, Bn, L, a, nb, None) == -1           # slot
        assert bwd(t, 0, a, a, ns, 0, None, g, 1, Bn, L, a, nb, None) == -1           # dx
        assert bwd(t, 0, a, a, ns, 0, a, None, 1, Bn, L, a, nb, None) == -1           # grads
        assert bwd(t, 0, a, a, ns, 0, a, g, 1, Bn, L, None, nb, None) == -1           # workspace
        assert bwd(t, 0, a, a, ns, 0, a, g, 1, 0, L, a, nb, None) == -1               # B
        for blk in range(layers):                                                    # a pair with one NULL pointer
            for j in (0, 3, 6, 9, 11):
                assert bwd(t, 0, a, a, ns, 1, a, _grads(layers, half=(blk, j)), 0, Bn, L, a, nb, None) == -1, (blk, j)
        assert bwd(t, 1, a, a, ns, 0, a, _grads(layers - 1, half=(layers - 2, 4)), 1, Bn, L, a, nb, None) == -1
        for blk, j in ((0, 1), (layers - 1, 10), (1, 7)):                           # a misaligned gradient pointer
            assert bwd(t, 0, a, a, ns, 0, a, _grads(layers, misaligned=(blk, j)), 1, Bn, L, a, nb, None) == -1, (blk, j)
        assert bwd(t, 0, a, a, ns, 0, a, g, 1, Bn, L, a, nb - 1, None) == -3          # workspace too small
        assert bwd(t, 0, a, a, ns - 1, 1, a, g, 1, Bn, L, a, nb, None) == -3          # slot too small
        assert bwd(t, 0, C.c_void_p((1 << 20) + 4), a, ns, 0, a, g, 1, Bn, L, a, nb, None) == -1   # misaligned ckpt
        assert bwd(t, 0, a, C.c_void_p((1 << 20) + 4), ns, 0, a, g, 1, Bn, L, a, nb, None) == -1   # misaligned slot
        assert bwd(t, 0, a, a, ns, 0, C.c_void_p((1 << 20) + 4), g, 1, Bn, L, a, nb, None) == -1   # misaligned dx
        # nothing kept: nothing to do (and nothing read)
        assert bwd(t, layers, None, None, 0, 0, a, None, 1, Bn, L, None, 0, None) == 0
    finally:
        lib.ov_tower_destroy(t)


def test_checkpointed_entry_points_need_every_block_without_hip():
    lib = _lib.load()
    t = _tower(lib, layers=3, blocks=False)
    try:
        a = C.c_void_p(1 << 20)
        ns = lib.ov_tower_slot_bytes(t, 2, 101)
        nb = lib.ov_tower_backward_partial_workspace_bytes(t, 2, 101)
        assert lib.ov_tower_forward_checkpointed(t, 3, a, None, a, ns, 2, 101, None) == -1
        assert lib.ov_tower_forward_checkpointed(t, 0, a, a, a, ns, 2, 101, None) == -1
        assert lib.ov_tower_backward_checkpointed(t, 0, a, a, ns, 0, a, _grads(3), 1, 2, 101, a, nb, None) == -1
    finally:
        lib.ov_tower_destroy(t)


def test_checkpointed_entry_points_reject_folded_weights_without_hip():
    lib = _lib.load()
    t = _tower(lib, layers=2, blocks=False)
    try:
        a = C.c_void_p(1 << 20)
        for i in range(2):
            w = _lib.BlockWeights(*([a] * 12), a, a)                 # LN folded (qkv_colsum / fc_colsum set)
            assert lib.ov_tower_set_block(t, i, C.byref(w)) == 0
        ns = lib.ov_tower_slot_bytes(t, 2, 101)
        nb = lib.ov_tower_backward_partial_workspace_bytes(t, 2, 101)
        assert lib.ov_tower_forward_checkpointed(t, 1, a, a, a, ns, 2, 101, None) == -1
        assert lib.ov_tower_backward_checkpointed(t, 0, a, a, ns, 0, a, _grads(2), 1, 2, 101, a, nb, None) == -1
    finally:
        lib.ov_tower_destroy(t)


def test_checkpointed_entry_points_reject_fp8_towers_without_hip():
    lib = _lib.load()
    layers, Bn, L = 2, 2, 101
    t = _tower(lib, D=384, layers=layers, heads=6, mlp=1536)
    try:
        a = C.c_void_p(1 << 20)
        for i in range(layers):
            q = _lib.BlockFp8(*[C.c_void_p((1 << 26) + 4096 * (10 * i + j)) for j in range(10)])
            assert lib.ov_tower_set_block_fp8(t, i, C.byref(q)) == 0
        ns = lib.ov_tower_slot_bytes(t, Bn, L)
        nb = lib.ov_tower_backward_partial_workspace_bytes(t, Bn, L)
        assert lib.ov_tower_forward_checkpointed(t, 0, a, a, a, ns, Bn, L, None) == -2
        assert lib.ov_tower_backward_checkpointed(t, 0, a, a, ns, 0, a, _grads(layers), 1, Bn, L, a, nb, None) == -2
    finally:
        lib.ov_tower_destroy(t)
