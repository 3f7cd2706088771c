"""GPU: the encoders' outputs, pinned to recorded results (the companion of test_gpu_block_pinned.py for the inference entry points).

ov_vision_embed[_keep], ov_encode_image[_keep], ov_vision_head_forward_tokens and ov_encode_text share tower.hip's workspace layouts
and launch sequences with ov_tower_forward.  Every output of theirs, on formula inputs (openvision_amd.synth Philox draws), is hashed
(sha256 of the raw bytes) and compared with tests/golden/encode_digests.json, recorded on an MI355X with the library as it was before
the layouts and the text tail were stated once.  The shapes are the smallest that reach every branch: the pooled last block (with and
without a peeled tail image, folded and over the module's own LayerNorms), the full block under pool 'tok' and under fp8, the text
tail on the pooled rows (folded and plain), and both fall-backs to the full block where the tail's buffers do not fit.

The text tail is bitwise the full block, so a digest cannot tell them apart: every case also asserts, from the in-situ profile, the
rows of the last block's c_proj (and out-proj and c_fc for text) -- B on a pooled tail, B L in a full block.

A change that is meant to alter the arithmetic of any of these paths regenerates the fixture on purpose:
    python tests/test_gpu_encode_pinned.py tests/golden/encode_digests.json
and says so; a host-side refactor must pass with the fixture untouched."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from openvision_amd import _lib  # noqa: E402
from openvision_amd._lib import ptr, stream_ptr, check  # noqa: E402
from test_gpu_block_pinned import _Tower, _draw, _sha, _buf, FP8_QKV, FP8_FC, FP8_ALL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(ROOT, "tests", "golden", "encode_digests.json")
D, HEADS, MLP, LAYERS = 384, 6, 1536, 2            # the width the fp8 path takes (D % 128 == 0, >= 384)
PATCH, E, KPAD = 16, 40, 768
VOCAB, TEXT_B = 300, 5
PROF_OUT, PROF_FC, PROF_PROJ, PROF_FC_TANH = 3, 4, 5, 6        # include/ovhip.h: OV_PROF_*


def _shape(tanh):
    return (D, HEADS, MLP, MLP, tanh, 0, 0, LAYERS)


def profiled_rows(fn, classes):
    """(launches, sum of their rows) per class that the in-situ profile records while fn() runs."""
    lib = _lib.load()
    check(lib.ov_profile_enable(sum(1 << c for c in classes), 256), "ov_profile_enable")
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for c in classes:
            ms, n, rows = C.c_double(0), C.c_int(0), C.c_double(0)
            check(lib.ov_profile_read(c, C.byref(ms), C.byref(n), C.byref(rows)), "ov_profile_read")
            out[c] = (n.value, int(rows.value))
    finally:
        check(lib.ov_profile_enable(0, 0), "ov_profile_enable")
    return out


def last_block_rows(classes, main_rows, last_rows):
    """What profiled_rows reports for a tower call whose last block launches `classes` on last_rows rows."""
    return {c: (LAYERS, (LAYERS - 1) * main_rows + last_rows) for c in classes}


class _VisionHead:
    def __init__(self, image, pool_avg):
        L = (image // PATCH) ** 2 + 1
        pos32 = _draw("enc.v.pos", (L, D), 0.25)
        self.keep = [t.to(DEV) for t in (
            _draw("enc.v.conv", (D, KPAD), KPAD ** -0.5).to(torch.bfloat16), _draw("enc.v.cls", (D,), 0.5), pos32.to(torch.bfloat16), pos32,
            _draw("enc.v.ln_w", (D,), 0.1, 1.0), _draw("enc.v.ln_b", (D,), 0.1), _draw("enc.v.proj", (E, D), D ** -0.5).to(torch.bfloat16))]
        self.c = _lib.VisionHead(image, PATCH, KPAD, int(pool_avg), 1, E, E, *[ptr(t) for t in self.keep])
        self.G, self.L = L - 1, L


def _keep_table(B, G, K):
    """image b keeps the first K entries of a fixed permutation of its G patches (7 is coprime with G = 16)"""
    return torch.tensor([[(7 * i + 3 * b) % G for i in range(K)] for b in range(B)], dtype=torch.int32, device=DEV)


def _vision_tower(folded, fp8=False, masks=None):
    t = _Tower("enc.v", _shape(False), folded=folded, fp8=fp8)
    if masks is not None:
        check(t.lib.ov_tower_set_fp8_mask(t.h, (C.c_ubyte * LAYERS)(*masks), LAYERS), "ov_tower_set_fp8_mask")
    return t


def _encode_image(t, head, img, B, normalize, path, tail=0, keep=None):
    """ov_encode_image[_keep] -> the digest of the features; asserts the last block's c_proj rows (path: 'pooled' or 'full')."""
    lib = _lib.load()
    hp = C.byref(head.c)
    flag = _lib.OV_F32 if img.dtype == torch.float32 else _lib.OV_BF16
    feat = torch.full((B, E), float("nan"), dtype=torch.float32, device=DEV)
    if keep is None:
        L = head.L
        nb = lib.ov_vision_workspace_bytes(t.h, hp, B)
        ws = _buf(nb)
        call = lambda: check(lib.ov_encode_image(t.h, hp, ptr(img), flag, B, ptr(feat), normalize, ptr(ws), nb, stream_ptr()), "ov_encode_image")
    else:
        K = keep.shape[1]
        L = K + 1
        nb = lib.ov_vision_keep_workspace_bytes(t.h, hp, B, K)
        ws = _buf(nb)
        call = lambda: check(lib.ov_encode_image_keep(t.h, hp, ptr(img), flag, ptr(keep), B, K, ptr(feat), normalize, None, ptr(ws), nb,
                                                      stream_ptr()), "ov_encode_image_keep")
    got = profiled_rows(call, [PROF_PROJ])
    main = (B - tail) * L                                   # the peeled images run on the side stream, which is not profiled
    assert got == last_block_rows([PROF_PROJ], main, B if path == "pooled" else main), (path, got)
    return _sha(feat)


def _vision_digests(image, B, dtype, folded, pool_avg, path, fp8_masks=None, tail=0, everything=False):
    lib = _lib.load()
    head = _VisionHead(image, pool_avg)
    hp = C.byref(head.c)
    img = _draw("enc.v.image", (B, 3, image, image), 1.0).to(dtype).to(DEV)
    t = _vision_tower(folded, fp8_masks is not None, fp8_masks)
    out = {}
    try:
        out["encode.features"] = _encode_image(t, head, img, B, 0, path, tail)
        if not everything:
            return out
        out["encode.features_normalized"] = _encode_image(t, head, img, B, 1, path, tail)
        G, L = head.G, head.L
        nb = lib.ov_vision_workspace_bytes(t.h, hp, B)
        ws = _buf(nb)
        tok = torch.full((B * L, D), float("nan"), dtype=torch.bfloat16, device=DEV)
        check(lib.ov_vision_embed(t.h, hp, ptr(img), _lib.OV_F32, B, ptr(tok), ptr(ws), nb, stream_ptr()), "ov_vision_embed")
        out["embed.tokens"] = _sha(tok)
        nbt = lib.ov_tower_workspace_bytes(t.h, B, L)
        wst = _buf(nbt)
        check(lib.ov_tower_forward(t.h, ptr(tok), B, L, ptr(wst), nbt, stream_ptr()), "ov_tower_forward")
        feat = torch.full((B, E), float("nan"), dtype=torch.float32, device=DEV)
        check(lib.ov_vision_head_forward_tokens(t.h, hp, ptr(tok), B, L, ptr(feat), 1, ptr(ws), nb, stream_ptr()), "ov_vision_head_forward_tokens")
        out["head.features_normalized"] = _sha(feat)
        for K, kpath in ((G, "pooled"), (5, "full")):        # K = G drops nothing and takes ov_encode_image's tail; dropped patches: full block
            keep = _keep_table(B, G, K)
            nbk = lib.ov_vision_keep_workspace_bytes(t.h, hp, B, K)
            wsk = _buf(nbk)
            tokk = torch.full((B * (K + 1), D), float("nan"), dtype=torch.bfloat16, device=DEV)
            check(lib.ov_vision_embed_keep(t.h, hp, ptr(img), _lib.OV_F32, ptr(keep), B, K, ptr(tokk), None, ptr(wsk), nbk, stream_ptr()),
                  "ov_vision_embed_keep")
            out[f"keep{K}.embed.tokens"] = _sha(tokk)
            out[f"keep{K}.encode.features"] = _encode_image(t, head, img, B, 0, kpath, keep=keep)
    finally:
        t.close()
    return out


def _text_digests(T, folded, pool_last, fp8, path):
    lib = _lib.load()
    B = TEXT_B
    keep = [x.to(DEV) for x in (
        _draw("enc.t.table", (VOCAB, D), 0.5).to(torch.bfloat16), _draw("enc.t.pos", (T, D), 0.25).to(torch.bfloat16),
        _draw("enc.t.ln_w", (D,), 0.1, 1.0), _draw("enc.t.ln_b", (D,), 0.1), _draw("enc.t.proj", (E, D), D ** -0.5).to(torch.bfloat16))]
    head = _lib.TextHead(T, VOCAB, int(pool_last), E, *[ptr(x) for x in keep])
    tokens = ((_draw("enc.t.tokens", (B, T), 1.0).abs() * 1e4).long() % VOCAB).to(DEV)
    t = _Tower("enc.t", _shape(True), folded=folded, fp8=fp8)
    out = {}
    try:
        nb = lib.ov_text_workspace_bytes(t.h, C.byref(head), B)
        ws = _buf(nb)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        classes = [PROF_OUT, PROF_FC_TANH, PROF_PROJ]
        for normalize in (0, 1):
            feat = torch.full((B, E), float("nan"), dtype=torch.float32, device=DEV)
            got = profiled_rows(lambda: check(lib.ov_encode_text(t.h, C.byref(head), ptr(tokens), B, ptr(feat), normalize, ptr(err), ptr(ws), nb,
                                                                 stream_ptr()), "ov_encode_text"), classes)
            assert got == last_block_rows(classes, B * T, B if path == "pooled" else B * T), (path, got)
            out["encode.features_normalized" if normalize else "encode.features"] = _sha(feat)
        assert int(err.item()) == 0
    finally:
        t.close()
    return out


F32, BF16 = torch.float32, torch.bfloat16
CASES = {
    # image, B, dtype, folded, pool_avg, the last block's path
    "V1/folded_avg": (_vision_digests, (64, 3, F32, True, True, "pooled"), dict(everything=True)),
    "V2/folded_avg_peeled_tail": (_vision_digests, (64, 964, BF16, True, True, "pooled"), dict(tail=1)),   # tail_images(964, 17) = 1
    "V3/folded_tok": (_vision_digests, (64, 3, F32, True, False, "full"), {}),
    "V4/unfolded_avg": (_vision_digests, (64, 3, F32, False, True, "pooled"), {}),
    "V5/fp8_masks_avg": (_vision_digests, (64, 3, F32, True, True, "full"), dict(fp8_masks=(FP8_QKV | FP8_FC, FP8_ALL))),
    "V6/fallback_hidden_does_not_fit": (_vision_digests, (32, 3, F32, True, True, "full"), {}),     # B F 4 = 18432 > the h region's 11520
    # T, folded, pool_last, fp8, the last block's path
    "T1/folded_last": (_text_digests, (16, True, True, False, "pooled"), {}),
    "T2/folded_first": (_text_digests, (16, True, False, False, "pooled"), {}),
    "T3/unfolded_last": (_text_digests, (16, False, True, False, "pooled"), {}),
    "T4/fp8": (_text_digests, (16, True, True, True, "full"), {}),
    "T5/fallback_tail_does_not_fit": (_text_digests, (1, True, True, False, "full"), {}),           # 23080 B > big's 16128
}


def _recorded(case):
    with open(FIXTURE) as f:
        return json.load(f)[case]


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_outputs_match_the_recorded_digests(case):
    want = _recorded(case)
    fn, args, kw = CASES[case]
    got = fn(*args, **kw)
    for k in sorted(got):
        print(case, k, got[k])
    assert sorted(got) == sorted(want), (case, "the set of outputs changed")
    wrong = [k for k in sorted(got) if got[k] != want[k]]
    assert not wrong, (case, wrong)


# ---- the embed and head size queries: a workspace of exactly the reported size, at V1's shape ------------------------------------------
SENTINEL = 256


def _exact(nbytes):
    """a buffer of exactly nbytes (a multiple of 16) followed by SENTINEL bytes of 0xA5"""
    assert nbytes > 0 and nbytes % 16 == 0
    buf = torch.full((nbytes + SENTINEL,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf


def _sentinel_intact(buf):
    torch.cuda.synchronize()
    return bool((buf[-SENTINEL:] == 0xA5).all().item())


def test_embed_in_a_workspace_of_exactly_the_reported_size():
    lib = _lib.load()
    want = _recorded("V1/folded_avg")
    B, head = 3, _VisionHead(64, True)
    hp = C.byref(head.c)
    img = _draw("enc.v.image", (B, 3, 64, 64), 1.0).to(DEV)
    t = _vision_tower(True)
    try:
        nb = lib.ov_vision_embed_workspace_bytes(t.h, hp, B, 0)
        ws = _exact(nb)
        tok = torch.full((B * head.L, D), float("nan"), dtype=torch.bfloat16, device=DEV)
        check(lib.ov_vision_embed(t.h, hp, ptr(img), _lib.OV_F32, B, ptr(tok), ptr(ws), nb, stream_ptr()), "ov_vision_embed")
        assert _sha(tok) == want["embed.tokens"] and _sentinel_intact(ws)
        K = 5
        keep = _keep_table(B, head.G, K)
        nbk = lib.ov_vision_embed_workspace_bytes(t.h, hp, B, K)
        assert nbk < lib.ov_vision_keep_workspace_bytes(t.h, hp, B, K)
        wsk = _exact(nbk)
        tokk = torch.full((B * (K + 1), D), float("nan"), dtype=torch.bfloat16, device=DEV)
        check(lib.ov_vision_embed_keep(t.h, hp, ptr(img), _lib.OV_F32, ptr(keep), B, K, ptr(tokk), None, ptr(wsk), nbk, stream_ptr()),
              "ov_vision_embed_keep")
        assert _sha(tokk) == want["keep5.embed.tokens"] and _sentinel_intact(wsk)
    finally:
        t.close()


def test_head_in_a_workspace_of_exactly_the_reported_size():
    lib = _lib.load()
    want = _recorded("V1/folded_avg")
    B, head = 3, _VisionHead(64, True)
    hp = C.byref(head.c)
    img = _draw("enc.v.image", (B, 3, 64, 64), 1.0).to(DEV)
    t = _vision_tower(True)
    try:
        nbe = lib.ov_vision_embed_workspace_bytes(t.h, hp, B, 0)
        wse = _buf(nbe)
        tok = torch.full((B * head.L, D), float("nan"), dtype=torch.bfloat16, device=DEV)
        check(lib.ov_vision_embed(t.h, hp, ptr(img), _lib.OV_F32, B, ptr(tok), ptr(wse), nbe, stream_ptr()), "ov_vision_embed")
        nbt = lib.ov_tower_workspace_bytes(t.h, B, head.L)
        wst = _buf(nbt)
        check(lib.ov_tower_forward(t.h, ptr(tok), B, head.L, ptr(wst), nbt, stream_ptr()), "ov_tower_forward")
        nb = lib.ov_vision_head_workspace_bytes(t.h, hp, B)
        ws = _exact(nb)
        feat = torch.full((B, E), float("nan"), dtype=torch.float32, device=DEV)
        check(lib.ov_vision_head_forward_tokens(t.h, hp, ptr(tok), B, head.L, ptr(feat), 1, ptr(ws), nb, stream_ptr()),
              "ov_vision_head_forward_tokens")
        assert _sha(feat) == want["head.features_normalized"] and _sentinel_intact(ws)
    finally:
        t.close()


if __name__ == "__main__":
    digests = {case: fn(*args, **kw) for case, (fn, args, kw) in CASES.items()}
    with open(sys.argv[1], "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", sys.argv[1], sum(len(v) for v in digests.values()), "digests")
