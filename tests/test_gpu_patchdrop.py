"""GPU: patch dropout (PatchDropout, transformer.py:49-86,619).  The kept-patch kernels against the full path (bitwise rows, bitwise
identity-keep encodes and gradients), the model level against the reference-generated fixture and torch autograd through the oracle's
fp32 pieces, deterministic fixed-order dpos / dcls with exact zeros for positions no image kept, two attention shapes at L' = 1 + K,
patch dropout under lock_image_tower, and the device flag for a bad keep table."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openvision_amd import _lib, preset, synth, training
from openvision_amd._lib import ptr, stream_ptr
from openvision_amd.loss import ClipLoss
from openvision_amd.model import CLIP, PatchDropout, keep_to_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COS_TOL = 1e-3
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "patchdrop_tiny16_160.npz")


def one_minus_cos(a, b):
    return (1 - F.cosine_similarity(a.float().cpu(), torch.as_tensor(b).float().cpu(), dim=-1)).max().item()


def make_cfg(name, p, **vis):
    cfg = preset(name)
    return dict(cfg, vision_cfg=dict(cfg["vision_cfg"], patch_dropout=p, **vis))


def build(cfg, sd=None, train=True):
    m = CLIP(embed_dim=cfg["embed_dim"], vision_cfg=cfg["vision_cfg"], text_cfg=cfg["text_cfg"])
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    return m.train(train)


def random_keep(g, b, G, K):
    return torch.stack([torch.randperm(G, generator=g)[:K] for _ in range(b)])


# ---- 1. kernels: the kept rows are the full path's rows, bitwise ---------------------------------------------------------------------
@pytest.mark.parametrize("size", [160, 256, 384])               # G = 100, 256, 576
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_keep_rows_bitwise(size, dtype):
    torch.manual_seed(size)
    m = build(make_cfg("vit-tiny-patch16-160", 0.0, image_size=size, layers=1), train=False)
    G = (size // 16) ** 2
    g = torch.Generator().manual_seed(7)
    img = torch.randn(3, 3, size, size, generator=g).to(dtype).to(DEV)
    full = m.visual._embed_tokens(img)
    for K in (1, G // 2, G - 3, G):
        keep = random_keep(g, 3, G, K)
        kd = keep_to_device(keep, DEV)
        tok = m.visual._embed_tokens(img, kd)
        assert tok.shape == (3, 1 + K, 192)
        assert torch.equal(tok[:, 0], full[:, 0])
        want = full[:, 1:][torch.arange(3, device=DEV)[:, None], keep.to(DEV)]
        assert torch.equal(tok[:, 1:], want), (size, dtype, K)


# ---- 2. identity keep is the p = 0 path -------------------------------------------------------------------------------------------
def test_identity_keep_encode_image_bitwise():
    cfg = make_cfg("vit-tiny-patch16-160", 0.0)
    m = build(cfg, synth.make_state_dict(cfg), train=False)
    img = synth.make_images(5, 160, seed=3).to(DEV)
    kd = keep_to_device(torch.arange(100).repeat(5, 1), DEV)
    for norm in (False, True):
        a = m.visual._encode(img, norm)
        b = m.visual._encode(img, norm, keep=kd)
        assert torch.equal(a, b)


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_identity_keep_training_bitwise():
    cfg = make_cfg("vit-tiny-patch16-160", 0.0)
    m = build(cfg, synth.make_state_dict(cfg))
    g = torch.Generator().manual_seed(5)
    img0 = synth.make_images(4, 160, seed=5).to(DEV)
    r = torch.randn(4, cfg["embed_dim"], generator=g).to(DEV)
    out = {}
    for mode in ("full", "keep"):
        m.zero_grad(set_to_none=True)
        img = img0.clone().requires_grad_(True)
        keep = torch.arange(100).repeat(4, 1) if mode == "keep" else None
        f = training.encode_image(m, img, True, keep=keep)
        (f * r).sum().backward()
        out[mode] = (f.detach(), _grads(m), img.grad.detach().clone())
    (fa, ga, ia), (fb, gb, ib) = out["full"], out["keep"]
    assert torch.equal(fa, fb)
    assert torch.equal(ia, ib)
    assert sorted(ga) == sorted(gb)
    for n in ga:
        if n in ("visual.positional_embedding", "visual.class_embedding"):
            # torch's batch sum against the fixed-order kernel
            assert (ga[n] - gb[n]).abs().max() <= 1e-5 * ga[n].abs().max(), n
        else:
            assert torch.equal(ga[n], gb[n]), n


# ---- 3. model level against the reference ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def setup(gold):
    cfg = make_cfg("vit-tiny-patch16-160", float(gold["p"]))
    sd = synth.make_state_dict(cfg)
    b = gold["keep"].shape[0]
    img = synth.make_images(b, 160, seed=int(gold["img_seed"]))
    tok = synth.make_captions(b, seed=int(gold["tok_seed"]))
    return cfg, sd, img, tok


@pytest.fixture(scope="module")
def oracle_grads(gold, setup):
    """torch autograd through the oracle's fp32 pieces composed with the fixture's keep: patch_embed, gather, block_stack, pool,
    ln_post, proj (+ the text tower and the loss)."""
    from oracle import clip_ref as R
    cfg, sd, img, tok = setup
    v = cfg["vision_cfg"]
    keep = torch.from_numpy(gold["keep"])
    sdg = {k: t.clone().float().requires_grad_(True) for k, t in sd.items()}
    x = R.patch_embed(img, sdg, v["patch_size"])
    x = torch.cat([x[:, :1], x[:, 1:][torch.arange(x.shape[0])[:, None], keep]], dim=1)
    x = R.block_stack(x, sdg, "visual.transformer.", v["layers"], v["width"] // v["head_width"], False)
    pooled = R.layer_norm(x[:, 1:].mean(dim=1), sdg["visual.ln_post.weight"], sdg["visual.ln_post.bias"])
    fi = R.l2_normalize(pooled @ sdg["visual.proj"])
    ft = R.encode_text(tok, sdg, cfg, True)
    loss = R.clip_loss(fi, ft, sdg["logit_scale"].exp())
    loss.backward()
    return fi.detach(), float(loss), {k: t.grad for k, t in sdg.items() if t.grad is not None}


def _check_grads(got, ref, names=None):
    scale = max(float(r.norm()) for r in ref.values())
    checked = 0
    for n, r in ref.items():
        if names is not None and n not in names:
            continue
        r = torch.as_tensor(r).float()
        rn = float(r.norm())
        if rn < 1e-3 * scale:
            continue
        assert n in got and got[n] is not None, n
        gg = got[n].float().cpu()
        cos = float((gg * r).sum() / (gg.norm() * r.norm() + 1e-30))
        assert cos >= 0.99, (n, cos)
        assert abs(float(gg.norm()) - rn) < 0.05 * rn, (n, float(gg.norm()), rn)
        checked += 1
    return checked


def test_oracle_composition_matches_fixture(gold, oracle_grads):
    fi, loss, grads = oracle_grads
    assert one_minus_cos(fi, gold["image_features"]) < 1e-5
    assert abs(loss - float(gold["loss"])) < 1e-4
    assert _check_grads(grads, {k[5:]: torch.from_numpy(gold[k].astype(np.float32)) for k in gold.files if k.startswith("grad/")}) == 6


def test_training_step_against_reference(gold, setup, oracle_grads):
    cfg, sd, img, tok = setup
    m = build(cfg, sd)
    torch.manual_seed(int(gold["seed"]))
    fi, ft, s = training.clip_forward(m, img.to(DEV), tok.to(DEV))
    loss = ClipLoss()(fi, ft, s)
    assert one_minus_cos(fi.detach(), gold["image_features"]) < COS_TOL
    assert abs(float(loss.detach()) - float(gold["loss"])) < 2e-2
    loss.backward()
    got = {n: p.grad for n, p in m.named_parameters()}
    fixture = {k[5:]: torch.from_numpy(gold[k].astype(np.float32)) for k in gold.files if k.startswith("grad/")}
    assert _check_grads(got, fixture) == 6
    assert _check_grads(got, oracle_grads[2]) > 100
    # the inference entry points draw the same patches in training mode, and none in eval mode
    with torch.no_grad():
        torch.manual_seed(int(gold["seed"]))
        f = m.encode_image(img.to(DEV), normalize=True)
        assert one_minus_cos(f, gold["image_features"]) < COS_TOL
        torch.manual_seed(int(gold["seed"]))
        a, _, _ = m(img.to(DEV), tok.to(DEV))
        assert torch.equal(a, f)
        m.eval()
        state = torch.get_rng_state()
        e = m.encode_image(img.to(DEV), normalize=True)
        assert torch.equal(torch.get_rng_state(), state)
        m0 = build(make_cfg("vit-tiny-patch16-160", 0.0), sd, train=False)
        assert torch.equal(e, m0.encode_image(img.to(DEV), normalize=True))


def test_output_tokens_are_the_kept_tokens(gold, setup):
    cfg, sd, img, tok = setup
    cfg = dict(cfg, vision_cfg=dict(cfg["vision_cfg"], output_tokens=True))
    m = build(cfg, sd)
    torch.manual_seed(int(gold["seed"]))
    pooled, tokens = m.visual(img.to(DEV))
    assert tokens.shape == (4, 50, 192)
    torch.manual_seed(int(gold["seed"]))
    assert torch.equal(pooled, m.visual._encode(img.to(DEV), False))


# ---- 4. dpos: exact zeros where no image kept the patch, bitwise reproducible -------------------------------------------------------
def test_dpos_zero_rows_and_determinism(gold, setup):
    cfg, sd, img, tok = setup
    m = build(cfg, sd)
    keep = gold["keep"]
    unkept = sorted(set(range(100)) - set(keep.reshape(-1).tolist()))
    assert unkept
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(int(gold["seed"]))
        fi, ft, s = training.clip_forward(m, img.to(DEV), tok.to(DEV))
        ClipLoss()(fi, ft, s).backward()
        runs.append(_grads(m))
    dpos = runs[0]["visual.positional_embedding"]
    assert torch.all(dpos[[1 + p for p in unkept]] == 0)
    kept = sorted(set(keep.reshape(-1).tolist()))
    assert torch.all(dpos[[1 + p for p in kept]].abs().sum(dim=1) > 0)
    assert sorted(runs[0]) == sorted(runs[1])
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]), n


# ---- 5. forward against the oracle at the attention edge shapes ---------------------------------------------------------------------
@pytest.mark.parametrize("name,p,layers,b", [("vit-large-patch14-224", 0.5, 4, 8),      # L' = 129: the resident attention's lone key
                                            ("vit-small-patch8-384", 0.75, 2, 2)])      # L' = 577: the streaming single-key chunk
def test_forward_against_oracle(name, p, layers, b):
    from oracle import clip_ref as R
    cfg = make_cfg(name, p, layers=layers)
    v = cfg["vision_cfg"]
    sd = synth.make_state_dict(cfg, variant="sharp")
    m = build(cfg, sd)
    G = (v["image_size"] // v["patch_size"]) ** 2
    img = synth.make_images(b, v["image_size"], seed=9)
    torch.manual_seed(17)
    keep = PatchDropout(p).sample(b, G)
    assert keep.shape[1] + 1 in (129, 577)
    with torch.no_grad():
        x = R.patch_embed(img, sd, v["patch_size"])
        x = torch.cat([x[:, :1], x[:, 1:][torch.arange(b)[:, None], keep]], dim=1)
        x = R.block_stack(x, sd, "visual.transformer.", layers, v["width"] // v["head_width"], False)
        ref = R.layer_norm(x[:, 1:].mean(dim=1), sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"]
        torch.manual_seed(17)
        f = m.encode_image(img.to(DEV))
    assert one_minus_cos(f, ref) < COS_TOL
    torch.manual_seed(17)
    ft = training.encode_image(m, img.to(DEV), normalize=False)
    assert one_minus_cos(ft.detach(), ref) < COS_TOL


# ---- 6. FLIP + LiT --------------------------------------------------------------------------------------------------------------------
def test_locked_image_tower_with_dropout(gold, setup, oracle_grads):
    cfg, sd, img, tok = setup
    m = build(cfg, sd)
    m.lock_image_tower()
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(int(gold["seed"]))
    fi, ft, s = training.clip_forward(m, img.to(DEV), tok.to(DEV))
    assert not fi.requires_grad
    loss = ClipLoss()(fi, ft, s)
    assert abs(float(loss.detach()) - float(gold["loss"])) < 2e-2
    loss.backward()
    assert all(p.grad is None for p in m.visual.parameters())
    got = {n: p.grad for n, p in m.named_parameters() if not n.startswith("visual.")}
    text = {n for n in oracle_grads[2] if not n.startswith("visual.")}
    assert _check_grads(got, oracle_grads[2], text) > 40


# ---- 7. a bad keep table raises through the device flag ------------------------------------------------------------------------------
def test_bad_keep_table_sets_flag_and_raises(setup):
    cfg, sd, img, tok = setup
    m = build(cfg, sd)
    lib = _lib.load()
    good = torch.stack([torch.randperm(100)[:50] for _ in range(3)])
    for bad_value, ok in ((None, True), ("dup", False), (100, False), (-1, False)):
        keep = good.clone()
        if bad_value == "dup":
            keep[1, 7] = keep[1, 3]
        elif bad_value is not None:
            keep[2, 11] = bad_value
        kd = keep_to_device(keep, DEV)
        inv = torch.empty(3, 100, dtype=torch.int32, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.check(lib.ov_patch_keep_inverse(ptr(kd), ptr(inv), 3, 50, 100, ptr(err), stream_ptr()), "inverse")
        assert int(err.item()) == (0 if ok else 1), bad_value
        if ok:
            want = torch.full((3, 100), -1, dtype=torch.int32)
            for b in range(3):
                want[b, keep[b]] = torch.arange(50, dtype=torch.int32)
            assert torch.equal(inv.cpu(), want)
            training.encode_image(m, img[:3].to(DEV), keep=keep)
        else:
            with pytest.raises(IndexError):
                training.encode_image(m, img[:3].to(DEV), keep=keep)
