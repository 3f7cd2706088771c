"""CPU: drop path's host side -- the per-block rates, the draw, the table and its inverse maps, the argument checks of the Python
surface and of the new C entry points, and the restatement's own consistency (tests/droppath_restate.py).  Nothing runs on a device."""
import ctypes

import numpy as np
import pytest
import torch

import droppath_restate as R
from openvision_amd import _lib, build as B, preset, training
from openvision_amd.model import Transformer, create_model
from test_cabi import declared_symbols

NEW = ("ov_sample_gather", "ov_sample_scatter_axpy", "ov_tower_set_drop_path", "ov_tower_drop_path_workspace_bytes")


def _tower(layers=4, rate=0.0):
    tr = Transformer(128, layers, 2, 2.0)
    tr.set_drop_path(rate)
    return tr


def test_rates_are_linspace_and_layer_zero_never_drops():
    for n in (1, 2, 3, 12, 27):
        for r in (0.0, 0.1, 0.4):
            assert np.array_equal(training.drop_path_rates(r, n), np.linspace(0, r, n))
            assert np.array_equal(training.drop_path_rates(r, n), R.rates(r, n))
    tr = _tower(6, 0.9)
    for seed in range(20):
        t = training.drop_path_table(tr, 33, generator=torch.Generator().manual_seed(seed))
        assert bool(t.keep[0].all()), "block 0 has rate 0"
    assert not bool(t.keep[-1].all())                            # rate 0.9 over 66 draws
    assert torch.allclose(t.scale, torch.from_numpy(1.0 / (1.0 - np.linspace(0, 0.9, 6))).float(), rtol=1e-6, atol=0)


def test_draw_is_floor_of_keep_plus_the_generators_rand_stream():
    tr = _tower(5, 0.4)
    t = training.drop_path_table(tr, 17, generator=torch.Generator().manual_seed(3))
    u = torch.rand(5, 2, 17, generator=torch.Generator().manual_seed(3))
    keep_p = torch.from_numpy(1.0 - np.linspace(0, 0.4, 5)).float()
    want = torch.floor(keep_p[:, None, None] + u)
    assert t.keep.dtype == torch.bool and tuple(t.keep.shape) == (5, 2, 17)
    assert torch.equal(t.keep, want >= 1.0)
    assert np.array_equal(want.numpy(), R.draw(keep_p[:, None, None].numpy(), u.numpy()))       # the reference's two lines
    again = training.drop_path_table(tr, 17, generator=torch.Generator().manual_seed(3))
    assert torch.equal(again.keep, t.keep)
    torch.manual_seed(11)
    a = training.drop_path_table(tr, 17)
    torch.manual_seed(11)
    assert torch.equal(training.drop_path_table(tr, 17).keep, a.keep)     # no generator: the default one


def test_idx_and_slot_are_inverse_and_counts_match():
    tr = _tower(4, 0.5)
    t = training.drop_path_table(tr, 9, generator=torch.Generator().manual_seed(1))
    idx, slot = t.host_tables()
    assert idx.dtype == slot.dtype == torch.int32 and tuple(idx.shape) == tuple(slot.shape) == (4, 2, 9)
    for i in range(4):
        for j in range(2):
            k = int(t.keep[i, j].sum())
            assert t.counts[i][j] == k
            assert sorted(idx[i, j].tolist()) == list(range(9))
            kept = idx[i, j, :k].tolist()
            assert kept == sorted(kept) and all(bool(t.keep[i, j, b]) for b in kept)
            for b in range(9):
                if t.keep[i, j, b]:
                    assert idx[i, j, slot[i, j, b]] == b and slot[i, j, b] < k
                else:
                    assert slot[i, j, b] == -1
    sub = t.slice(1, 3)
    assert sub.layers == 2 and torch.equal(sub.keep, t.keep[1:3]) and torch.equal(sub.scale, t.scale[1:3]) and sub.counts == t.counts[1:3]
    assert t.slice(0, 4) is t
    a, b = sub.device_tables("cpu")
    assert torch.equal(a, idx[1:3]) and torch.equal(b, slot[1:3]) and a.is_contiguous() and b.is_contiguous()


def test_explicit_keep_is_validated_and_used():
    tr = _tower(3, 0.2)
    keep = torch.ones(3, 2, 5, dtype=torch.bool)
    keep[1, 0, 2] = False
    t = training.drop_path_table(tr, 5, keep=keep)
    assert torch.equal(t.keep, keep) and t.counts == [[5, 5], [4, 5], [5, 5]]
    assert training.drop_path_table(tr, 5, keep=keep, scale=[1.0, 1.5, 2.0]).scale.tolist() == [1.0, 1.5, 2.0]
    with pytest.raises(ValueError):
        training.drop_path_table(tr, 5, keep=torch.ones(3, 2, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        training.drop_path_table(tr, 5, keep=torch.ones(2, 2, 5, dtype=torch.bool))
    with pytest.raises(ValueError):
        training.drop_path_table(tr, 5, keep=torch.ones(3, 5, dtype=torch.bool))
    with pytest.raises(TypeError):
        training.drop_path_table(tr, 5, keep=torch.ones(3, 2, 5))
    with pytest.raises(TypeError):
        training.drop_path_table(tr, 5, keep=keep.tolist())
    with pytest.raises(ValueError):
        training.drop_path_table(tr, 5, keep=keep, scale=[1.0, 2.0])
    with pytest.raises(ValueError):
        training.drop_path_table(tr, 5, keep=keep, scale=[1.0, 0.0, 2.0])
    with pytest.raises(ValueError):
        training.drop_path_table(tr, 0)


def test_rates_outside_the_half_open_interval_raise():
    tr = _tower()
    m = create_model(preset("vit-tiny-patch16-160"))
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            tr.set_drop_path(bad)
        with pytest.raises(ValueError):
            m.set_drop_path(image=bad)
        with pytest.raises(ValueError):
            m.set_drop_path(text=bad)
        with pytest.raises(ValueError):
            training.drop_path_rates(bad, 4)
    assert tr.drop_path == 0.0 and m.visual.transformer.drop_path == 0.0 and m.transformer.drop_path == 0.0
    m.set_drop_path(image=0.25, text=0.5)
    assert (m.visual.transformer.drop_path, m.transformer.drop_path) == (0.25, 0.5)
    m.set_drop_path()
    assert (m.visual.transformer.drop_path, m.transformer.drop_path) == (0.0, 0.0)


def test_no_table_at_rate_zero_or_in_eval_mode():
    tr = _tower(3, 0.0)
    assert training.drop_path_table(tr, 4) is None
    assert training._own_drop(tr.train(), 4, None) is None
    tr.set_drop_path(0.5)
    assert training._own_drop(tr.eval(), 4, None) is None
    assert isinstance(training._own_drop(tr.train(), 4, None), training.DropPathTable)
    t = training.drop_path_table(tr, 4)
    assert training._own_drop(tr.eval(), 4, t) is t                           # an explicit table is used whatever the mode
    with pytest.raises(ValueError):
        training._own_drop(tr, 5, t)
    with pytest.raises(TypeError):
        training._own_drop(tr, 4, t.keep)
    cfg = dict(preset("vit-tiny-patch16-160"))
    cfg["vision_cfg"] = dict(cfg["vision_cfg"], drop_path=0.1)
    with pytest.raises((TypeError, ValueError, KeyError)):                     # no configuration key: unknown keys stay rejected
        create_model(cfg)


def test_cpu_tensors_still_raise():
    tr = _tower(2, 0.5).train()
    x = torch.randn(2, 3, 128)
    with pytest.raises(_lib.OvhipError):
        training.tower_forward(tr, x)
    with pytest.raises(_lib.OvhipError):
        training.tower_forward(tr, x, drop=training.drop_path_table(tr, 2))


def test_new_symbols_declared_bound_exported_and_built():
    syms = declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in syms, f"{s} is not declared in include/ovhip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert hasattr(lib, s), f"{s} is not exported"
    assert "droppath.hip" in B.SOURCES and lib.ov_abi_version() == 2


def test_new_entry_points_reject_bad_arguments_and_leave_the_sizes_alone():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)      # a host address: never dereferenced, the checks come first
    assert lib.ov_sample_gather(None, None, None, 5, 2, 3, 64, 1.0, None) == -1
    assert lib.ov_sample_gather(a, a, a, 5, 6, 3, 64, 1.0, None) == -1          # k > B
    assert lib.ov_sample_gather(a, a, a, 5, 2, 3, 60, 1.0, None) == -2          # D % 8
    assert lib.ov_sample_gather(None, None, None, 5, 0, 3, 64, 1.0, None) == 0  # k == 0 launches nothing
    assert lib.ov_sample_scatter_axpy(None, None, None, None, 5, 2, 3, 64, 1.0, None) == -1
    assert lib.ov_sample_scatter_axpy(a, a, a, a, 5, -1, 3, 64, 1.0, None) == -1
    assert lib.ov_sample_scatter_axpy(a, a, a, a, 5, 2, 3, 12, 1.0, None) == -2
    assert lib.ov_tower_set_drop_path(None, None, None, None, None, 0, None, 0) == -1
    assert lib.ov_tower_drop_path_workspace_bytes(None, 4, 8) == 0
    cfg = _lib.TowerCfg(128, 2, 2, 256, 256, 0, 1e-6)
    t = lib.ov_tower_create(ctypes.byref(cfg))
    try:
        sizes = lambda: (lib.ov_tower_workspace_bytes(t, 5, 65), lib.ov_tower_saved_bytes(t, 5, 65), lib.ov_tower_slot_bytes(t, 5, 65),
                         lib.ov_tower_backward_partial_workspace_bytes(t, 5, 65), lib.ov_tower_backward_input_workspace_bytes(t, 5, 65))
        before = sizes()
        need = lib.ov_tower_drop_path_workspace_bytes(t, 5, 65)
        assert need >= 3 * 5 * 65 * 128 * 2 and lib.ov_tower_drop_path_workspace_bytes(t, 0, 65) == 0
        count, scale = (ctypes.c_int * 4)(5, 4, 0, 1), (ctypes.c_float * 2)(1.0, 2.0)
        assert lib.ov_tower_set_drop_path(t, a, a, count, scale, 5, a, need) == 0
        assert sizes() == before                                                # the existing size functions return today's values
        assert lib.ov_tower_forward(t, a, 5, 65, a, 1 << 30, None) == -2         # inference refuses a table
        assert lib.ov_tower_set_drop_path(t, None, None, None, None, 0, None, 0) == 0
        assert lib.ov_tower_set_drop_path(t, a, None, count, scale, 5, a, need) == -1
        assert lib.ov_tower_set_drop_path(t, a, a, (ctypes.c_int * 4)(5, 6, 0, 1), scale, 5, a, need) == -1      # count > B
        assert lib.ov_tower_set_drop_path(t, a, a, count, (ctypes.c_float * 2)(1.0, 0.0), 5, a, need) == -1      # scale <= 0
        assert lib.ov_tower_set_drop_path(t, a, a, count, scale, 0, a, need) == -1
        assert sizes() == before
    finally:
        lib.ov_tower_destroy(t)


def test_restatement_masks_scale_and_pass_through():
    """The restatement against itself: a dropped sample passes through and receives dy, no other sample or gradient sees it, an
    all-kept table at scale 1 is the plain stack, and the kept samples equal the plain stack run on them alone at scale 1."""
    g = torch.Generator().manual_seed(2)
    tr = Transformer(64, 2, 2, 2.0)
    params = [R.block_params(b) for b in tr.resblocks]
    x, wout = torch.randn(3, 4, 64, generator=g).double(), torch.randn(3, 4, 64, generator=g).double()
    keep = torch.ones(2, 2, 3, dtype=torch.bool)
    plain = R.tower_grads(x, params, wout, None, None, 2)
    same = R.tower_grads(x, params, wout, keep, [1.0, 1.0], 2)
    assert torch.equal(plain[0], same[0]) and torch.equal(plain[1], same[1])
    keep[:, :, 1] = False
    y, dx, gr = R.tower_grads(x, params, wout, keep, [1.0, 1.0], 2)
    assert torch.equal(y[1], x[1]) and torch.equal(dx[1], wout[1])
    sub = R.tower_grads(x[[0, 2]], params, wout[[0, 2]], None, None, 2)
    assert torch.allclose(y[[0, 2]], sub[0], rtol=0, atol=1e-12) and torch.allclose(dx[[0, 2]], sub[1], rtol=0, atol=1e-12)
    for a, b in zip(gr, sub[2]):
        for n in R.NAMES:
            assert torch.allclose(a[n], b[n], rtol=0, atol=1e-10), n
    y2 = R.tower_grads(x, params, wout, keep, [1.0, 2.0], 2)[0]
    assert not torch.allclose(y2[0], y[0])                                      # the factor of a kept branch is applied
