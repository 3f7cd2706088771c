"""GPU: the last block of each tower computes only what the pooling head reads (ov_encode_image / ov_encode_text).

Image tower (avg pool): the last block stops after c_fc and ov_mlp_out_pooled forms mean_p(x1) + mean_p(h) W2^T + b in fp32 on B rows.
Text tower (last / first pool): past the last block's attention, out-proj .. c_proj run on the B pooled rows.
OVHIP_LAST_BLOCK_FULL=1 restores the full block in both; it is read once per process, so that side runs in ONE child process
(`full`, module scope) whose results every test below shares."""
import os
import tempfile

import numpy as np
import pytest
import torch

from openvision_amd import _lib, preset, synth
from openvision_amd._lib import ptr, stream_ptr, check
from openvision_amd.model import create_model
from ranks import run_child
from test_gpu_model import COS_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = "vit-tiny-patch16-160"
GOLDENS = (("v1", "tiny16_160.npz"), ("sharp", "tiny16_160_sharp.npz"))


def tail_images(B, L):
    """tower.hip's rule (`tail_images` in openvision_amd/csrc/tower.hip; a copy, to be kept in step with it): images peeled off onto
    the side stream so that the main part fills whole rounds of 256-row tiles.  OVHIP_NO_TAIL_SPLIT=1 turns the split off."""
    T = (B * L + 255) // 256
    r = T % 64
    if T <= 64 or r == 0 or r > 8:
        return 0
    target = T - r
    Bm = target * 256 // L
    while Bm > 0 and (Bm * L + 255) // 256 > target:
        Bm -= 1
    tail = B - Bm
    return tail if Bm > 0 and 0 < tail <= B // 8 else 0


def text_l14_cfg():
    """The tiny preset with a text tower of L/14's width (768, 12 heads); two layers keep it quick, the last one is what is tested."""
    cfg = preset(TINY)
    cfg["text_cfg"] = dict(preset("vit-large-patch14-224")["text_cfg"], layers=2)
    return cfg


def golden_npz(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


def compute_all():
    """Everything the tests compare between the default process and the OVHIP_LAST_BLOCK_FULL=1 child, on fixed inputs."""
    out = {}
    cfg = preset(TINY)
    for variant, gname in GOLDENS:
        g = golden_npz(gname)
        m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg, 0, variant))
        img = torch.from_numpy(g["images"].astype(np.float32)).to(DEV)
        out[f"image_{variant}"] = m.encode_image(img).cpu()
        if variant == "v1":
            tok = synth.make_captions(5, seed=11).to(DEV)
            out["text_tiny"] = m.encode_text(tok).cpu()
            x = m.visual._embed_tokens(img.contiguous())
            out["walk"] = m.visual.transformer(x).float().cpu()
            m.visual.output_tokens = True
            pooled, tokens = m.visual(img)
            m.visual.output_tokens = False
            out["tokens_pooled"], out["tokens"] = pooled.cpu(), tokens.float().cpu()
    cfg = text_l14_cfg()
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    out["text_l14"] = m.encode_text(synth.make_captions(5, seed=12).to(DEV)).cpu()
    return out


_CHILD = r"""
import torch
import test_gpu_last_block as T
torch.save(T.compute_all(), sys.argv[1])
"""


@pytest.fixture(scope="module")
def full():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "full.pt")
        run_child(_CHILD, path, env={"OVHIP_LAST_BLOCK_FULL": "1"}, timeout=600, gpu=True)
        return torch.load(path)


@pytest.fixture(scope="module")
def default():
    return compute_all()


def one_minus_cos(a, b):
    return (1 - torch.nn.functional.cosine_similarity(a.float().cpu(), torch.as_tensor(b).float(), dim=-1)).max().item()


# ------------------------------------------------------------------------------------------------------------------------------
# the identity, at operator level

def mlp_out_pooled(x1, h, w2, b, B, L):
    lib = _lib.load()
    D, F = x1.shape[1], w2.shape[1]
    out = torch.full((B, D), float("nan"), dtype=torch.float32, device=x1.device)
    nb = lib.ov_mlp_out_pooled_workspace_bytes(B, F)
    ws = torch.empty(nb, dtype=torch.uint8, device=x1.device)
    check(lib.ov_mlp_out_pooled(ptr(x1), x1.stride(0), ptr(h), h.stride(0), ptr(w2), w2.stride(0), ptr(b), ptr(out), B, L, D, F, 1,
                                ptr(ws), nb, stream_ptr()))
    return out


@pytest.mark.parametrize("B,L,D,F", [(3, 101, 192, 768), (2, 257, 1024, 4096)])
def test_pooled_c_proj_is_the_mean_of_the_block_output(B, L, D, F):
    """ov_mlp_out_pooled against mean_p(x1 + h W2^T + b) over the patch rows 1 .. L-1, formed in fp64 from the same bf16 inputs; the
    hidden sits under a padded pitch (F + 64, as the tower's `big` region).  Bound per element: (F + L) 2^-24 S + 1e-6 with
    S = mean|x1| + mean|h| |W2|^T + |b|: L fp32 additions per pooled value and F fp32 multiply-adds per output, worst case.  The weight
    is widened from bf16 exactly and the product runs in the fp32 MFMA, so there is no further rounding term.  Row 0 of each image (cls)
    must not enter: spiked to 1e4 in x1 and in h, the result is bitwise the same."""
    g = torch.Generator().manual_seed(B * L + D + F)
    x1 = torch.randn(B * L, D, generator=g).to(torch.bfloat16).to(DEV)
    hp = torch.randn(B * L, F + 64, generator=g).to(torch.bfloat16).to(DEV)
    h = hp[:, :F]
    w2 = (torch.randn(D, F, generator=g) / F ** 0.5).to(torch.bfloat16).to(DEV)
    b = torch.randn(D, generator=g).to(DEV)
    got = mlp_out_pooled(x1, h, w2, b, B, L).double()
    x64, h64, w64 = x1.double().view(B, L, D)[:, 1:], h.double().reshape(B, L, F)[:, 1:], w2.double()
    ref = (x64 + h64 @ w64.T + b.double()).mean(dim=1)
    S = x64.abs().mean(dim=1) + h64.abs().mean(dim=1) @ w64.abs().T + b.double().abs()
    bound = (F + L) * 2.0 ** -24 * S + 1e-6
    q = ((got - ref).abs() / bound).max().item()
    print(f"pooled c_proj {(B, L, D, F)}: max err / bound {q:.4f}, max err {(got - ref).abs().max().item():.3e}")
    assert q <= 1.0
    x1s, hs = x1.clone(), hp.clone()
    x1s.view(B, L, D)[:, 0] = 1e4
    hs.view(B, L, F + 64)[:, 0] = 1e4
    assert torch.equal(mlp_out_pooled(x1s, hs[:, :F], w2, b, B, L).double(), got)


# ------------------------------------------------------------------------------------------------------------------------------
# features, default path against the full block

def test_image_features_against_the_golden_and_the_full_block(default, full):
    """Both paths under COS_TOL of the fp32 reference's features; the pooled path no farther from them than the full block by more than
    the full block's own distance (it drops L bf16 roundings per image, so it is expected closer)."""
    for variant, gname in GOLDENS:
        ref = golden_npz(gname)["image_features"]
        c_new, c_full = one_minus_cos(default[f"image_{variant}"], ref), one_minus_cos(full[f"image_{variant}"], ref)
        print(f"{gname}: 1 - cos to the golden, pooled last block {c_new:.3e}, full last block {c_full:.3e}")
        assert c_new < COS_TOL and c_full < COS_TOL
        assert c_new - c_full <= c_full


@pytest.mark.parametrize("peel", [True, False])
def test_image_batch_invariance(peel):
    """One call on B images against a split call, bitwise: at a B where tail_images peels an image onto the side stream (the pools run
    over all B images after the join) and at B = 3 where it does not."""
    cfg = preset(TINY)
    v = cfg["vision_cfg"]
    L = (v["image_size"] // v["patch_size"]) ** 2 + 1
    B = next(b for b in range(8, 4096) if tail_images(b, L) > 0) if peel else 3
    assert (tail_images(B, L) > 0) == peel, (B, L)
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    img = synth.make_images(B, v["image_size"], seed=7).to(DEV)
    a = m.encode_image(img)
    cut = B // 2
    assert tail_images(cut, L) == 0 and tail_images(B - cut, L) == 0
    assert torch.equal(a, torch.cat([m.encode_image(img[:cut]), m.encode_image(img[cut:])]))
    assert torch.equal(a[B - 1:], m.encode_image(img[B - 1:]))


@pytest.mark.parametrize("key", ["text_tiny", "text_l14"])
def test_text_features_are_the_full_blocks(default, full, key):
    """B = 5, T = 80, the tiny preset and a text tower of L/14's width: the last block on the 5 pooled rows against the full block on all
    400.  A GEMM row is the same whichever kernel form computes it, so the features are bitwise the full block's (default settings; the
    opt-in OVHIP_ROWPARTS=1 takes its statistics from another producer in the full block and is not covered)."""
    a, b = default[key], full[key]
    d = (a.double() - b.double()).abs().max().item()
    print(f"{key}: max |pooled rows - full block| {d:.3e}")
    assert torch.equal(a, b), f"{key}: not bitwise the full block's, max difference {d:.3e}"


def profiled_rows(fn, classes):
    """Sum of the launch rows (M) the in-situ profile records per class while fn() runs."""
    import ctypes as C
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


PROF_OUT, PROF_FC, PROF_PROJ, PROF_FC_TANH = 3, 4, 5, 6        # include/ovhip.h: OV_PROF_*


def test_the_pooled_tails_are_what_runs():
    """The comparisons above would also pass on a silent return to the full block.  The in-situ profile records every launch's rows:
    in the image tower the last c_proj has B rows instead of B L, in the text tower the last out-proj, c_fc and c_proj have B rows
    instead of B T (the launch counts stay: one launch replaces one launch)."""
    cfg = preset(TINY)
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    v, t = cfg["vision_cfg"], cfg["text_cfg"]
    B, L, T = 3, (v["image_size"] // v["patch_size"]) ** 2 + 1, t["context_length"]
    img, tok = synth.make_images(B, v["image_size"], seed=7).to(DEV), synth.make_captions(B, seed=7).to(DEV)
    m.encode_image(img), m.encode_text(tok)                     # weights packed, workspaces sized
    got = profiled_rows(lambda: m.encode_image(img), [PROF_FC, PROF_PROJ])
    assert got[PROF_FC] == (v["layers"], v["layers"] * B * L), got
    assert got[PROF_PROJ] == (v["layers"], (v["layers"] - 1) * B * L + B), got
    got = profiled_rows(lambda: m.encode_text(tok), [PROF_OUT, PROF_FC_TANH, PROF_PROJ])
    for c in (PROF_OUT, PROF_FC_TANH, PROF_PROJ):
        assert got[c] == (t["layers"], (t["layers"] - 1) * B * T + B), got


def test_callers_that_want_the_token_stream_are_unchanged(default, full):
    """model.visual.transformer(x) (the exploded path) and output_tokens=True run the full block with and without the switch."""
    for key in ("walk", "tokens", "tokens_pooled"):
        assert torch.equal(default[key], full[key]), key
