"""GPU: the launch sequences of one ResidualAttentionBlock, pinned to recorded results.

The block backward, the tower backward in its full / input-only / partial / checkpointed forms, the attention half of the feature
visualisation tap and the inference forward (bf16 LN-folded, bf16 under a prefix mask, fp8 under a per-layer mask, main part and
tail) share their host code, so comparing them with each other says little about a change to that code.  Here every output of
those entry points, on formula inputs (openvision_amd.synth Philox draws: rebuilt bit for bit anywhere), is hashed (sha256 of the
raw bytes) and compared with tests/golden/block_digests.json, recorded on an MI355X with the library as it was before the entry
points were made to share one chain.  The kernels are deterministic and the split-K plan depends on the CU count only.

A change that is meant to alter the arithmetic of any of these paths regenerates the fixture on purpose:
    python tests/test_gpu_block_pinned.py tests/golden/block_digests.json
and says so; a host-side refactor must pass with the fixture untouched."""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from openvision_amd import _lib, synth  # noqa: E402
from openvision_amd._lib import ptr, stream_ptr, check  # noqa: E402
import hipops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1609
FIXTURE = os.path.join(ROOT, "tests", "golden", "block_digests.json")
NAMES = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b")
KEYS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
        "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
FP8_QKV, FP8_OUT, FP8_FC, FP8_PROJ, FP8_ALL = 1, 2, 4, 8, 15

# (width, heads, mlp, mlp_pad, gelu_tanh, B, L, layers)
SHAPES = {
    "hd64_l257": (192, 3, 768, 768, False, 2, 257, 3),             # head_dim 64, resident attention backward over the kept lse
    "hd64_l384_tanh": (128, 2, 512, 512, True, 2, 384, 2),         # head_dim 64 streaming; tanh GELU; B * L % 64 == 0: the TN dW route
    "hd80_l257_padmlp": (320, 4, 1076, 1088, False, 2, 257, 2),    # head_dim 80; MLP width padded to the next multiple of 64
}
# inference: 69 row tiles of 256 -> remainder 5 over 64 -> tail_images(68, 257) = 5; the width the fp8 path takes (D % 128 == 0, >= 384)
INFER = (384, 6, 1536, 1536, False, 68, 257, 3)
INFER_MASKS = (0, FP8_QKV | FP8_FC, FP8_ALL)


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().reshape(-1).cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _draw(name, shape, std, mean=0.0):
    return synth._normal("pinned." + name, shape, std, SEED, mean)


def _block_weights(tag, i, D, mlp, F):
    """The module's own weights of block i in the kernels' layout (matrices bf16, vectors fp32, MLP padding zero), on the CPU."""
    sd = {}
    pre = f"pinned.{tag}.{i}."
    synth._block(sd, pre, D, mlp, SEED)
    ts = [sd[pre + k] for k in KEYS]
    fc_w, fc_b, proj_w = torch.zeros(F, D), torch.zeros(F), torch.zeros(D, F)
    fc_w[:mlp], fc_b[:mlp], proj_w[:, :mlp] = ts[8], ts[9], ts[10]
    ts[8], ts[9], ts[10] = fc_w, fc_b, proj_w
    return [t.to(torch.bfloat16).contiguous() if t.dim() == 2 else t.contiguous() for t in ts]


def _folded(tag, i, ts):
    """LN-folded operands of block i: W' = bf16(gamma * W), colsum = the exact row sums of W' (fp64 holds them exactly), and a drawn
    epilogue vector in the place of beta W^T + b (any vector is a valid operand; a draw does not depend on a host matmul's order)."""
    out = list(ts)
    cols = []
    for w_at, g_at, b_at, nm in ((2, 0, 3, "qkv"), (8, 6, 9, "fc")):
        wg = (ts[w_at].float() * ts[g_at][None, :]).to(torch.bfloat16)
        out[w_at] = wg
        out[b_at] = _draw(f"{tag}.{i}.{nm}_cvec", (wg.shape[0],), 0.1)
        cols.append(wg.double().sum(dim=1).float().contiguous())
    return out, cols


def _fp8(ts):
    """packed_block_fp8's layout: per-output-row absmax e4m3 copies of the four matrices (element-wise IEEE arithmetic only)."""
    def q8(w):
        w32 = w.float()
        scale = (w32.abs().amax(dim=1) / 448.0).clamp_min(1e-30)
        return (w32 / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).contiguous(), scale.contiguous()
    (wq, sq), (wo, so), (wf, sf), (wp, sp) = q8(ts[2]), q8(ts[4]), q8(ts[8]), q8(ts[10])
    return [wq, sq, ts[3], wo, so, wf, sf, ts[9], wp, sp]


class _Tower:
    def __init__(self, tag, shape, layers=None, first_layer=0, folded=False, fp8=False):
        D, heads, mlp, F, tanh, _, _, nl = shape
        self.layers = nl if layers is None else layers
        self.lib = _lib.load()
        self.cfg = _lib.TowerCfg(D, self.layers, heads, mlp, F, int(tanh), 1e-6)
        self.h = self.lib.ov_tower_create(C.byref(self.cfg))
        assert self.h
        self.w, self.keep = [], []
        for i in range(self.layers):
            own = _block_weights(tag, first_layer + i, D, mlp, F)
            ts, cols = _folded(tag, first_layer + i, own) if folded else (own, [None, None])
            dev = [t.to(DEV) for t in ts] + [c.to(DEV) if c is not None else None for c in cols]
            self.w.append(dev[:12])
            self.keep.append(dev)
            check(self.lib.ov_tower_set_block(self.h, i, C.byref(_lib.BlockWeights(*[ptr(t) for t in dev]))), "ov_tower_set_block")
            if fp8:
                d8 = [t.to(DEV) for t in _fp8(own)]
                self.keep.append(d8)
                check(self.lib.ov_tower_set_block_fp8(self.h, i, C.byref(_lib.BlockFp8(*[ptr(t) for t in d8]))), "ov_tower_set_block_fp8")

    def block_weights(self, i=0):
        return _lib.BlockWeights(*[ptr(t) for t in self.w[i]], None, None)

    def grads(self, pairs=None):
        """fresh gradient tensors (NaN-filled) per layer for the requested pairs (None = all) and their ov_block_grads array"""
        pairs = [set(range(6))] * self.layers if pairs is None else pairs
        gs = [[torch.full_like(p, float("nan")) if j // 2 in pairs[i] else None for j, p in enumerate(self.w[i])] for i in range(self.layers)]
        return gs

    def close(self):
        self.lib.ov_tower_destroy(self.h)


def _garr(gs):
    return (_lib.BlockGrads * len(gs))(*[_lib.BlockGrads(*[ptr(p) for p in g]) for g in gs])


def _grad_digests(out, key, gs, first=0):
    for i, g in enumerate(gs):
        for n, p in zip(NAMES, g):
            if p is not None:
                out[f"{key}.g{first + i}.{n}"] = _sha(p)


def _buf(n):
    return torch.zeros(max(int(n), 16), dtype=torch.uint8, device=DEV)


def _inputs(tag, M, D):
    x = _draw(tag + ".x", (M, D), 1.0).to(torch.bfloat16).to(DEV)
    dy = _draw(tag + ".dy", (M, D), 0.1).to(torch.bfloat16).to(DEV)
    return x, dy


def _block_digests(tag):
    """ov_block_backward (recomputing, and over a one-layer saving forward's slot), ov_block_backward_prefix, the attention half."""
    shape = SHAPES[tag]
    D, heads, mlp, F, tanh, B, L, _ = shape
    M = B * L
    lib = _lib.load()
    out = {}
    t = _Tower(tag, shape, layers=1)
    try:
        x, dy = _inputs(tag, M, D)
        wst = t.block_weights()
        nb = lib.ov_block_backward_workspace_bytes(C.byref(t.cfg), B, L)
        assert nb > 0
        ws = _buf(nb)

        def run(key, saved, prefix):
            gs = t.grads()
            dx = torch.full_like(x, float("nan"))
            g = _garr(gs)
            sv = C.byref(saved) if saved is not None else None
            if prefix is None:
                check(lib.ov_block_backward(C.byref(t.cfg), C.byref(wst), ptr(x), sv, ptr(dy), ptr(dx), g, B, L, ptr(ws), nb, stream_ptr()), key)
            else:
                check(lib.ov_block_backward_prefix(C.byref(t.cfg), C.byref(wst), ptr(x), sv, ptr(dy), ptr(dx), g, prefix, B, L, ptr(ws), nb,
                                                   stream_ptr()), key)
            out[key + ".dx"] = _sha(dx)
            _grad_digests(out, key, gs)

        run("block_recompute", None, None)
        run("block_prefix_recompute", None, L // 3)
        # a full ov_block_saved out of the one-layer saving forward: [x | qkv | o | x1 | ln_1 | ln_2 | pre | act | lse]
        saved = _buf(lib.ov_tower_saved_bytes(t.h, B, L))
        nbf = lib.ov_tower_workspace_bytes(t.h, B, L)
        wsf = _buf(nbf)
        y = x.clone()
        check(lib.ov_tower_forward_saving(t.h, ptr(y), ptr(saved), B, L, ptr(wsf), nbf, stream_ptr()), "ov_tower_forward_saving")
        out["block_saved.y"] = _sha(y)
        route = _lib.AttentionRoute()                                  # the lse is kept where the library says the backward reads it
        check(lib.ov_attention_route(B, L, heads, D // heads, 0, 0, -1, 0, 0, 0, C.addressof(route)), "ov_attention_route")
        sv = hipops.block_saved_of(hipops.saved_slots(saved, D, F, heads, B, L)[0], route.keep_lse)
        run("block_saved", sv, None)
        # the attention half alone (feature visualisation)
        qkv = torch.full((M, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
        o, x1, dx = (torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(3))
        lse_t = torch.zeros(B * heads * ((L + 31) // 32 * 32), dtype=torch.float32, device=DEV)
        check(lib.ov_block_attn_forward_saving(C.byref(t.cfg), C.byref(wst), ptr(x), ptr(qkv), ptr(o), ptr(x1), ptr(lse_t), B, L, stream_ptr()),
              "ov_block_attn_forward_saving")
        nba = lib.ov_block_attn_backward_input_workspace_bytes(C.byref(t.cfg), B, L)
        assert 0 < nba < nb
        wsa = _buf(nba)
        check(lib.ov_block_attn_backward_input(C.byref(t.cfg), C.byref(wst), ptr(x), ptr(qkv), ptr(o), ptr(lse_t), ptr(dy), ptr(dx), B, L,
                                               ptr(wsa), nba, stream_ptr()), "ov_block_attn_backward_input")
        out.update({"attn_half.qkv": _sha(qkv), "attn_half.attn_out": _sha(o), "attn_half.x1": _sha(x1), "attn_half.dx": _sha(dx)})
    finally:
        t.close()
    return out


def _tower_digests(tag, prefix=None):
    """The training walks: saving forward + full / input-only backward, saving-from + partial backward over three frozen patterns,
    the checkpointed pair.  prefix: the same full pair under ov_tower_set_prefix only."""
    shape = SHAPES[tag]
    D, heads, mlp, F, tanh, B, L, layers = shape
    M = B * L
    lib = _lib.load()
    out = {}
    t = _Tower(tag, shape)
    try:
        x, dy = _inputs(tag, M, D)
        key = "tower" if prefix is None else "tower_prefix"
        if prefix is not None:
            check(lib.ov_tower_set_prefix(t.h, prefix), "ov_tower_set_prefix")
        saved = _buf(lib.ov_tower_saved_bytes(t.h, B, L))
        nbf = lib.ov_tower_workspace_bytes(t.h, B, L)
        wsf = _buf(nbf)
        y = x.clone()
        check(lib.ov_tower_forward_saving(t.h, ptr(y), ptr(saved), B, L, ptr(wsf), nbf, stream_ptr()), "ov_tower_forward_saving")
        out[key + ".y"] = _sha(y)
        nb = lib.ov_tower_backward_workspace_bytes(t.h, B, L)
        ws = _buf(nb)
        gs = t.grads()
        dx = dy.clone()
        check(lib.ov_tower_backward(t.h, ptr(saved), ptr(dx), _garr(gs), B, L, ptr(ws), nb, stream_ptr()), "ov_tower_backward")
        out[key + ".dx"] = _sha(dx)
        _grad_digests(out, key, gs)
        nbi = lib.ov_tower_backward_input_workspace_bytes(t.h, B, L)
        assert 0 < nbi < nb
        wsi = _buf(nbi)
        dx = dy.clone()
        check(lib.ov_tower_backward_input(t.h, ptr(saved), ptr(dx), B, L, ptr(wsi), nbi, stream_ptr()), "ov_tower_backward_input")
        out[key + "_input.dx"] = _sha(dx)
        if prefix is not None:
            return out
        none = set()
        patterns = [      # (name, first, pairs per kept layer, want_dx); pairs: 0 ln_1, 1 in_proj, 2 out_proj, 3 ln_2, 4 c_fc, 5 c_proj
            ("ln2_params_only_bottom", 0, [{3, 5}] + [{0, 2}] * (layers - 1), 0),       # a trainable LayerNorm whose dx nobody reads
            ("frozen_above_trainable", 0, [{0, 4}] + [none] * (layers - 1), 0),         # ln_1 parameters only at the bottom
            ("from_1_in_proj_dx", 1, [{1}] * (layers - 1), 1),
        ]
        nbp = lib.ov_tower_backward_partial_workspace_bytes(t.h, B, L)
        wsp = _buf(nbp)
        for name, first, pairs, want_dx in patterns:
            sv = _buf(lib.ov_tower_saved_bytes_from(t.h, first, B, L))
            nbw = lib.ov_tower_forward_saving_from_workspace_bytes(t.h, first, B, L)
            wsw = _buf(nbw)
            y = x.clone()
            check(lib.ov_tower_forward_saving_from(t.h, first, ptr(y), ptr(sv), B, L, ptr(wsw), nbw, stream_ptr()), name)
            out[f"partial.{name}.y"] = _sha(y)
            gs = t.grads([none] * first + pairs)[first:]
            dx = dy.clone()
            check(lib.ov_tower_backward_partial(t.h, first, ptr(sv), ptr(dx), _garr(gs), want_dx, B, L, ptr(wsp), nbp, stream_ptr()), name)
            if want_dx:
                out[f"partial.{name}.dx"] = _sha(dx)
            _grad_digests(out, f"partial.{name}", gs, first)
        # checkpointed: block inputs only, the top layer's slot still in place for the backward
        ckpt = _buf(lib.ov_tower_checkpoint_bytes(t.h, 0, B, L))
        ns = lib.ov_tower_slot_bytes(t.h, B, L)
        slot = _buf(ns)
        y = x.clone()
        check(lib.ov_tower_forward_checkpointed(t.h, 0, ptr(y), ptr(ckpt), ptr(slot), ns, B, L, stream_ptr()), "ov_tower_forward_checkpointed")
        out["checkpointed.y"] = _sha(y)
        gs = t.grads()
        dx = dy.clone()
        check(lib.ov_tower_backward_checkpointed(t.h, 0, ptr(ckpt), ptr(slot), ns, 1, ptr(dx), _garr(gs), 1, B, L, ptr(wsp), nbp, stream_ptr()),
              "ov_tower_backward_checkpointed")
        out["checkpointed.dx"] = _sha(dx)
        _grad_digests(out, "checkpointed", gs)
    finally:
        t.close()
    return out


def _forward(t, x, B, L):
    lib = _lib.load()
    nb = lib.ov_tower_workspace_bytes(t.h, B, L)
    ws = _buf(nb)
    y = x.clone()
    check(lib.ov_tower_forward(t.h, ptr(y), B, L, ptr(ws), nb, stream_ptr()), "ov_tower_forward")
    return _sha(y)


def _infer_digests(which):
    """ov_tower_forward at a batch whose last five images run as the tail on the side stream, and at a small batch that does not split."""
    D, heads, mlp, F, tanh, B, L, layers = INFER
    lib = _lib.load()
    out = {}
    x, _ = _inputs("infer", B * L, D)
    xs = x[: 4 * L].contiguous()
    if which == "bf16":
        t = _Tower("infer", INFER, folded=True)
        try:
            out["folded.tail.y"] = _forward(t, x, B, L)
            out["folded.small.y"] = _forward(t, xs, 4, L)
        finally:
            t.close()
        t = _Tower("infer", INFER)
        try:
            out["unfolded.tail.y"] = _forward(t, x, B, L)
            check(lib.ov_tower_set_prefix(t.h, 100), "ov_tower_set_prefix")
            out["unfolded_prefix.tail.y"] = _forward(t, x, B, L)
            out["unfolded_prefix.small.y"] = _forward(t, xs, 4, L)
        finally:
            t.close()
        return out
    t = _Tower("infer", INFER, folded=True, fp8=True)
    try:
        mask = (C.c_ubyte * layers)(*INFER_MASKS)
        check(lib.ov_tower_set_fp8_mask(t.h, mask, layers), "ov_tower_set_fp8_mask")
        out["fp8_mixed.noscale.tail.y"] = _forward(t, x, B, L)
        amax = torch.zeros(4 * layers, dtype=torch.float32, device=DEV)
        check(lib.ov_tower_set_fp8_hidden_scale(t.h, ptr(amax), 1), "ov_tower_set_fp8_hidden_scale")     # record the maxima
        out["fp8_mixed.recording.tail.y"] = _forward(t, x, B, L)
        out["fp8_mixed.recording.amax"] = _sha(amax)
        check(lib.ov_tower_set_fp8_hidden_scale(t.h, ptr(amax), 3), "ov_tower_set_fp8_hidden_scale")     # frozen static scales
        out["fp8_mixed.static.tail.y"] = _forward(t, x, B, L)
        out["fp8_mixed.static.small.y"] = _forward(t, xs, 4, L)
        out["fp8_mixed.static.amax"] = _sha(amax)
    finally:
        t.close()
    return out


CASES = {}
for _tag in SHAPES:
    CASES[f"block/{_tag}"] = (_block_digests, (_tag,))
    CASES[f"tower/{_tag}"] = (_tower_digests, (_tag,))
CASES["tower_prefix/hd64_l257"] = (_tower_digests, ("hd64_l257", 41))
CASES["tower_prefix/hd80_l257_padmlp"] = (_tower_digests, ("hd80_l257_padmlp", 200))
CASES["infer/bf16"] = (_infer_digests, ("bf16",))
CASES["infer/fp8"] = (_infer_digests, ("fp8",))


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_outputs_match_the_recorded_digests(case):
    with open(FIXTURE) as f:
        want = json.load(f)[case]
    fn, args = CASES[case]
    got = fn(*args)
    for k in sorted(got):
        print(case, k, got[k])
    assert sorted(got) == sorted(want), (case, "the set of outputs changed")
    wrong = [k for k in sorted(got) if got[k] != want[k]]
    assert not wrong, (case, wrong)


if __name__ == "__main__":
    digests = {case: fn(*args) for case, (fn, args) in CASES.items()}
    with open(sys.argv[1], "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", sys.argv[1], sum(len(v) for v in digests.values()), "digests")
