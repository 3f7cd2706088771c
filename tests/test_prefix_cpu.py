"""CPU: the prefix-causal mask rule, the new C entry points' argument checks, and what the forward bound can see.

No reference-generated fixture backs these tests (jax / flax were not importable where they were written): the mask is compared with a
step-by-step restatement of text_transformer.py:418-442 (tests/prefix_restate.py: reference_mask)."""
import ctypes

import pytest
import torch

import prefix_restate as PR
from hipops import err_ratio
from openvision_amd import _lib
from test_cabi import declared_symbols
from test_gpu_prefix_attention import SHAPES, inputs

NEW = ("ov_attention_prefix", "ov_attention_prefix_backward", "ov_attention_prefix_backward_workspace_bytes", "ov_tower_set_prefix",
       "ov_block_backward_prefix", "ov_softmax_xent", "ov_softmax_xent_backward", "ov_softmax_xent_workspace_bytes")


def test_rule_equals_the_reference_mask():
    for L in range(0, 41):
        for P in range(0, L + 1):
            assert torch.equal(PR.rule_mask(L, P), PR.reference_mask(L, P)), (L, P)
            if L:
                assert bool(PR.rule_mask(L, P).any(dim=1).all())             # no empty row
    assert bool(PR.rule_mask(7, 7).all()) and torch.equal(PR.rule_mask(7, 0), torch.tril(torch.ones(7, 7, dtype=torch.bool)))


def test_new_symbols_declared_bound_and_exported():
    syms = declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in syms, f"{s} is not declared in include/ovhip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert hasattr(lib, s), f"{s} is not exported"


def test_new_entry_points_reject_bad_arguments():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)       # a host address: never dereferenced, the checks come first
    L = 8
    assert lib.ov_attention_prefix(None, 192, None, 64, 1, L, 1, 64, 0.125, 0, None) == -1
    assert lib.ov_attention_prefix_backward(None, 192, None, 64, None, 64, None, 192, 1, L, 1, 64, 0.125, 0, None, 0, None) == -1
    for p in (-1, L + 1):
        assert lib.ov_attention_prefix(a, 192, a, 64, 1, L, 1, 64, 0.125, p, None) == -1
        assert lib.ov_attention_prefix_backward(a, 192, a, 64, a, 64, a, 192, 1, L, 1, 64, 0.125, p, a, 1 << 20, None) == -1
        assert lib.ov_block_backward_prefix(None, None, None, None, None, None, None, p if p > 0 else -2, 1, L, None, 0, None) == -1
    assert lib.ov_block_backward_prefix(None, None, None, None, None, None, None, 0, 1, L, None, 0, None) == -1
    assert lib.ov_attention_prefix_backward_workspace_bytes(2, 257, 16, 64) >= 2 * 2 * 16 * 257 * 4     # needed where the unmasked is resident
    assert lib.ov_attention_prefix_backward_workspace_bytes(2, 257, 16, 64) >= lib.ov_attention_backward_workspace_bytes(2, 257, 16, 80)
    assert lib.ov_softmax_xent(None, 8, None, None, 1, 8, None, None, None, 0, None) == -1
    assert lib.ov_softmax_xent_backward(None, 8, None, None, None, None, None, 8, 1, 8, None, 0, None) == -1
    assert lib.ov_softmax_xent(a, 4, a, a, 1, 8, a, a, a, 4096, None) == -1                               # row pitch below V
    assert lib.ov_softmax_xent_workspace_bytes(256 * 128) >= 256 * 128 * 4 and lib.ov_softmax_xent_workspace_bytes(0) == 0
    assert lib.ov_tower_set_prefix(None, 0) == -1
    cfg = _lib.TowerCfg(192, 1, 3, 768, 768, 1, 1e-6)
    t = lib.ov_tower_create(ctypes.byref(cfg))
    try:
        assert lib.ov_tower_set_prefix(t, -2) == -1
        assert lib.ov_tower_set_prefix(t, 5) == 0 and lib.ov_tower_set_prefix(t, -1) == 0
        saved = lib.ov_tower_saved_bytes(t, 2, 40)
        assert lib.ov_tower_set_prefix(t, 17) == 0
        assert lib.ov_tower_saved_bytes(t, 2, 40) == saved                   # the kept layout does not depend on the mask
    finally:
        lib.ov_tower_destroy(t)


def wrong_masks(L, P):
    i = torch.arange(L)[:, None]
    j = torch.arange(L)[None, :]
    no_diag = (j < P) | (j < i)
    no_diag = no_diag | (~no_diag.any(dim=1, keepdim=True) & (j == i))        # (a row left empty keeps its one key)
    out = {"diagonal dropped": no_diag, "one key too many": (j < P) | (j <= i + 1)}
    if P >= 1:
        out["prefix - 1"] = PR.rule_mask(L, P - 1)
    if P + 1 <= L:
        out["prefix + 1"] = PR.rule_mask(L, P + 1)
    return out


@pytest.mark.parametrize("B,L,Hh,hd,P", [s for s in SHAPES if s[3] == 64 or s[1] < 300])
def test_bound_sees_an_off_by_one_mask(B, L, Hh, hd, P):
    """On the GPU test's own inputs: the kernel arithmetic emulated with the right mask lies inside hipops.bound; with the diagonal
    dropped, one key too many, or the prefix off by one (wherever that is a different mask: P = 0 and P = 1 are the same one, and so
    are the variants of L = 1) it lies outside."""
    qkv = inputs(B, L, Hh, hd, P)
    right = PR.rule_mask(L, P)
    ref, pv = PR.masked_attn_ref64(qkv, B, L, Hh, hd, right)
    r = err_ratio(PR.emulate_masked(qkv, B, L, Hh, hd, right), ref, pv)
    print(f"L={L} hd={hd} P={P}: right mask {r:.3f}")
    assert r <= 1.0, r
    for name, m in wrong_masks(L, P).items():
        if torch.equal(m, right):
            continue
        rw = err_ratio(PR.emulate_masked(qkv, B, L, Hh, hd, m), ref, pv)
        print(f"    {name}: {rw:.1f}")
        assert rw > 1.0, (name, rw)
