"""CPU: the workspace sizes the inference entry points report, pinned to recorded values.

ov_tower_workspace_bytes, ov_vision_workspace_bytes, ov_vision_keep_workspace_bytes and ov_text_workspace_bytes are pure host code
(tower.hip's layout functions): they load and run without a GPU.  Every preset's two towers, with the head fields as model.py builds
them, at B in {1, 3, 256, 1024}, the keep query at K in {1, G // 2, G}; towers of width % 128 == 0 once with bf16 blocks and once with
fp8 copies set on every layer (aligned dummy pointers: the size functions read none of them).  tests/golden/workspace_sizes.json was
recorded with the library as it was before the layouts were stated once; a change that is meant to alter a layout regenerates it on
purpose:
    python tests/test_workspace_sizes_cpu.py tests/golden/workspace_sizes.json
and says so.  The two queries added with the layout functions (ov_vision_embed_workspace_bytes, ov_vision_head_workspace_bytes) are
checked against their entry points' own workspace checks further down, without a launch."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from openvision_amd import _lib, preset  # noqa: E402
from openvision_amd.config import PRESETS, mlp_width  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
BATCHES = (1, 3, 256, 1024)
A = 16                                 # an aligned non-NULL dummy pointer


def _round_up(x, m):
    return (x + m - 1) // m * m


class _Tower:
    def __init__(self, width, layers, heads, mlp_ratio, tanh):
        self.lib = _lib.load()
        mlp = mlp_width(width, mlp_ratio)
        self.cfg = _lib.TowerCfg(width, layers, heads, mlp, _round_up(mlp, 64), int(tanh), 1e-6)
        self.h = self.lib.ov_tower_create(C.byref(self.cfg))
        assert self.h

    def set_fp8(self, on):
        q = _lib.BlockFp8(*([A] * 10))
        for i in range(self.cfg.layers):
            assert self.lib.ov_tower_set_block_fp8(self.h, i, C.byref(q) if on else None) == 0

    def close(self):
        self.lib.ov_tower_destroy(self.h)


def vision_parts(name):
    """The image tower and the ov_vision_head of a preset, as VisionTransformer._head fills it."""
    cfg = preset(name)
    v, e = cfg["vision_cfg"], cfg["embed_dim"]
    t = _Tower(v["width"], v["layers"], v["width"] // v["head_width"], v["mlp_ratio"], False)
    head = _lib.VisionHead(v["image_size"], v["patch_size"], _round_up(3 * v["patch_size"] ** 2, 64), 1, 1, e, e, A, A, A, A, A, A, A)
    return t, head, (v["image_size"] // v["patch_size"]) ** 2


def text_parts(name):
    """The text tower and the ov_text_head of a preset, as CLIP._text_head fills it."""
    cfg = preset(name)
    x = cfg["text_cfg"]
    t = _Tower(x["width"], x["layers"], x["heads"], x["mlp_ratio"], True)
    head = _lib.TextHead(x["context_length"], x["vocab_size"], 1, cfg["embed_dim"], A, A, A, A, A)
    return t, head


def sizes(name):
    lib = _lib.load()
    out = {}
    t, head, G = vision_parts(name)
    try:
        for prec in ("bf16", "fp8") if t.cfg.width % 128 == 0 else ("bf16",):
            t.set_fp8(prec == "fp8")
            for B in BATCHES:
                key = f"vision.{prec}.B{B}"
                out[key + ".tower"] = lib.ov_tower_workspace_bytes(t.h, B, G + 1)
                out[key + ".encode"] = lib.ov_vision_workspace_bytes(t.h, C.byref(head), B)
                for K in (1, G // 2, G):
                    out[f"{key}.keep{K}"] = lib.ov_vision_keep_workspace_bytes(t.h, C.byref(head), B, K)
    finally:
        t.close()
    t, head = text_parts(name)
    try:
        for prec in ("bf16", "fp8") if t.cfg.width % 128 == 0 else ("bf16",):
            t.set_fp8(prec == "fp8")
            for B in BATCHES:
                key = f"text.{prec}.B{B}"
                out[key + ".tower"] = lib.ov_tower_workspace_bytes(t.h, B, head.context_length)
                out[key + ".encode"] = lib.ov_text_workspace_bytes(t.h, C.byref(head), B)
    finally:
        t.close()
    assert all(v > 0 for v in out.values()), out
    return out


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_reported_sizes_match_the_recorded_ones(name):
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    got = sizes(name)
    assert sorted(got) == sorted(want), (name, "the set of sizes changed")
    wrong = {k: (got[k], want[k]) for k in sorted(got) if got[k] != want[k]}
    assert not wrong, (name, wrong)


OV_ERR_INVALID, OV_ERR_WORKSPACE = -1, -3


def test_the_embed_and_head_queries_are_what_their_entry_points_check():
    """One byte short of the reported size is OV_ERR_WORKSPACE; the exact size passes that check and reaches the next one, made to
    fail before any launch (an image dtype that does not exist; token rows off 16 bytes): OV_ERR_INVALID."""
    lib = _lib.load()
    t, head, G = vision_parts("vit-tiny-patch16-160")
    a, odd = C.c_void_p(A), C.c_void_p(A + 8)
    hp = C.byref(head)
    try:
        B, K, D = 3, 5, t.cfg.width
        n = lib.ov_vision_embed_workspace_bytes(t.h, hp, B, 0)
        assert n == B * G * head.kpad * 2
        assert lib.ov_vision_embed(t.h, hp, a, 7, B, a, a, n - 1, None) == OV_ERR_WORKSPACE
        assert lib.ov_vision_embed(t.h, hp, a, 7, B, a, a, n, None) == OV_ERR_INVALID
        nk = lib.ov_vision_embed_workspace_bytes(t.h, hp, B, K)
        assert B * K * (head.kpad + D) * 2 <= nk < lib.ov_vision_keep_workspace_bytes(t.h, hp, B, K)
        assert lib.ov_vision_embed_keep(t.h, hp, a, 7, a, B, K, a, None, a, nk - 1, None) == OV_ERR_WORKSPACE
        assert lib.ov_vision_embed_keep(t.h, hp, a, 7, a, B, K, a, None, a, nk, None) == OV_ERR_INVALID
        assert lib.ov_vision_embed_workspace_bytes(t.h, hp, B, G + 1) == 0 and lib.ov_vision_embed_workspace_bytes(t.h, hp, B, -1) == 0
        assert lib.ov_vision_embed_workspace_bytes(t.h, hp, 0, 0) == 0 and lib.ov_vision_embed_workspace_bytes(None, hp, B, 0) == 0
        nh = lib.ov_vision_head_workspace_bytes(t.h, hp, B)
        assert B * (D * 6 + head.embed_pad * 2) <= nh < lib.ov_vision_workspace_bytes(t.h, hp, B)
        assert lib.ov_vision_head_forward_tokens(t.h, hp, odd, B, G + 1, a, 1, a, nh - 1, None) == OV_ERR_WORKSPACE
        assert lib.ov_vision_head_forward_tokens(t.h, hp, odd, B, G + 1, a, 1, a, nh, None) == OV_ERR_INVALID
        assert lib.ov_vision_head_workspace_bytes(t.h, hp, 0) == 0 and lib.ov_vision_head_workspace_bytes(t.h, None, B) == 0
    finally:
        t.close()


if __name__ == "__main__":
    table = {name: sizes(name) for name in sorted(PRESETS)}
    with open(sys.argv[1], "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", sys.argv[1], sum(len(v) for v in table.values()), "sizes")
