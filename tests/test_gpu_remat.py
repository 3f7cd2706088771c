"""GPU: activation recomputation (CLIP.set_grad_checkpointing).  With the flag on, the loss and every gradient are bit for bit those
with it off: at tower shapes through both attention backward forms, at every chunking, and with frozen parameters, a frozen text
tower and patch dropout at model level.  The pool keeps only the block inputs and one slot per tower, the step's peak memory drops
accordingly, and a backward after a later forward is refused as on the saving path."""
import ctypes as C

import pytest
import torch

from openvision_amd import _lib, preset, synth, training
from openvision_amd.loss import ClipLoss
from openvision_amd.model import Transformer, create_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- tower level (training.tower_forward over a bare Transformer) ---------------------------------------------------------------------
def _rand_transformer(D, layers, heads, tanh=False, seed=5):
    tr = Transformer(D, layers, heads, 4.0, {"approximate": "tanh"} if tanh else None)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in tr.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            elif n.endswith("ln_1.weight") or n.endswith("ln_2.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return tr.to(DEV)


def _tower_step(tr, x, wout, remat, chunk=0, backwards=1):
    prev = training.CHUNK_LAYERS[0]
    tr.grad_checkpointing = remat
    training.set_backward_chunk_layers(chunk)
    try:
        for p in tr.parameters():
            p.grad = None
        xx = x.clone().requires_grad_(True)
        loss = (training.tower_forward(tr, xx).float() * wout).sum()
        for i in range(backwards):
            loss.backward(retain_graph=i + 1 < backwards)
        torch.cuda.synchronize()
    finally:
        training.set_backward_chunk_layers(prev)
        tr.grad_checkpointing = False
    return loss.detach(), xx.grad.detach().clone(), {n: (p.grad.detach().clone() if p.grad is not None else None)
                                                     for n, p in tr.named_parameters()}


def _assert_same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "loss")
    assert torch.equal(a[1], b[1]), (what, "x.grad")
    assert a[2].keys() == b[2].keys()
    for n in a[2]:
        if b[2][n] is None:
            assert a[2][n] is None, (what, n)
        else:
            assert a[2][n] is not None and torch.equal(a[2][n], b[2][n]), (what, n)


# (width, layers, heads, gelu_tanh, B, L)
TOWERS = {
    "l14_4blk_b8_l257": (1024, 4, 16, False, 8, 257),      # head_dim 64, short L (the route's keep_lse): resident attention backward over the kept lse
    "hd80_b3_l257": (640, 3, 8, False, 3, 257),            # head_dim 80: streaming attention backward, no lse
    "text_b6_l80": (192, 4, 3, True, 6, 80),
}


@pytest.mark.parametrize("shape", list(TOWERS), ids=list(TOWERS))
def test_tower_gradients_bitwise(shape):
    D, layers, heads, tanh, Bn, L = TOWERS[shape]
    tr = _rand_transformer(D, layers, heads, tanh)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(Bn, L, D, generator=g).to(DEV)
    wout = (torch.randn(Bn, L, D, generator=g) * 0.1).to(DEV)
    ref = _tower_step(tr, x, wout, False)
    assert ref[1].abs().max().item() > 0
    for chunk in (0, 1, 2):
        _assert_same(_tower_step(tr, x, wout, True, chunk), ref, (shape, chunk))
    # frozen lower blocks (x needs a gradient: every block still runs its input chain)
    for p in tr.resblocks[0].parameters():
        p.requires_grad_(False)
    ref = _tower_step(tr, x, wout, False)
    got = _tower_step(tr, x, wout, True)
    _assert_same(got, ref, (shape, "block 0 frozen"))
    assert got[2]["resblocks.0.ln_1.weight"] is None and got[2]["resblocks.1.ln_1.weight"] is not None


def test_second_backward_before_and_after_a_later_forward():
    tr = _rand_transformer(192, 3, 3)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(4, 101, 192, generator=g).to(DEV)
    wout = torch.randn(4, 101, 192, generator=g).to(DEV)
    once = _tower_step(tr, x, wout, True)
    twice = _tower_step(tr, x, wout, True, backwards=2)          # the second backward recomputes the top block as well
    assert torch.equal(twice[1], 2 * once[1])
    for n in once[2]:
        assert torch.equal(twice[2][n], 2 * once[2][n]), n
    tr.grad_checkpointing = True
    try:
        xx = x.clone().requires_grad_(True)
        loss = (training.tower_forward(tr, xx).float() * wout).sum()
        loss.backward(retain_graph=True)
        training.tower_forward(tr, x.clone().requires_grad_(True))   # takes the checkpoint buffer over
        with pytest.raises(_lib.OvhipError):
            loss.backward()
    finally:
        tr.grad_checkpointing = False


def test_pool_holds_checkpoints_and_one_slot_and_peak_memory_drops():
    """An L/14-wide tower (48 blocks, so that the activations outweigh the backward workspace) at B = 16, L = 257, one autograd node
    per block: after the forward the pool holds the block inputs and the top node's slot; the step's peak falls at least 5x."""
    D, layers, heads, Bn, L = 1024, 48, 16, 16, 257
    tr = _rand_transformer(D, layers, heads)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(Bn, L, D, generator=g).to(DEV)
    wout = (torch.randn(Bn, L, D, generator=g) * 0.1).to(DEV)
    lib = _lib.load()
    cfg = _lib.TowerCfg(D, layers, heads, 4 * D, 4 * D, 0, 1e-6)
    t = lib.ov_tower_create(C.byref(cfg))
    ckpt, slot = lib.ov_tower_checkpoint_bytes(t, 0, Bn, L), lib.ov_tower_slot_bytes(t, Bn, L)
    saved_all = lib.ov_tower_saved_bytes(t, Bn, L)
    lib.ov_tower_destroy(t)
    for p in tr.parameters():                                   # .grad exists before the step: accumulated in place
        p.grad = torch.zeros_like(p)
    prev = training.CHUNK_LAYERS[0]
    training.set_backward_chunk_layers(1)
    peaks = {}
    try:
        for remat in (False, True, False, True):                # the second of each: packed weights and .grad already exist
            tr.grad_checkpointing = remat
            pool = tr._ovhip_pool = training._Pool()            # every buffer of this step is allocated within it
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            xx = x.clone().requires_grad_(True)
            loss = (training.tower_forward(tr, xx).float() * wout).sum()
            torch.cuda.synchronize()
            if remat:
                assert pool.out_bytes.get("saved", 0) == ckpt and pool.out_bytes.get("slot", 0) == slot, pool.out_bytes
                assert pool.out.get("slot", 0) == 1
            else:
                assert pool.out_bytes.get("saved", 0) == saved_all and not pool.out_bytes.get("slot")
            loss.backward()
            torch.cuda.synchronize()
            assert all(v == 0 for v in pool.out_bytes.values()), pool.out_bytes
            peaks[remat] = torch.cuda.max_memory_allocated() - base
            del xx, loss
    finally:
        training.set_backward_chunk_layers(prev)
        tr.grad_checkpointing = False
    assert peaks[True] * 5 <= peaks[False], peaks


# ---- model level ------------------------------------------------------------------------------------------------------------------------
def _tiny(cfg=None):
    cfg = cfg or preset("vit-tiny-patch16-160")
    return create_model(cfg, device=DEV, state_dict=synth.make_state_dict(preset("vit-tiny-patch16-160")))


def _clip_step(m, img, tok, remat, chunk=0, seed=None):
    prev = training.CHUNK_LAYERS[0]
    m.set_grad_checkpointing(remat)
    training.set_backward_chunk_layers(chunk)
    try:
        m.zero_grad(set_to_none=True)
        if seed is not None:
            torch.manual_seed(seed)                             # the patch-dropout draw (CPU default generator)
        loss = ClipLoss()(*training.clip_forward(m, img, tok))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        training.set_backward_chunk_layers(prev)
        m.set_grad_checkpointing(False)
    return loss.detach(), {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()}


def _assert_model_same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "loss")
    n_grad = 0
    for n in a[1]:
        if b[1][n] is None:
            assert a[1][n] is None, (what, n)
        else:
            assert a[1][n] is not None and torch.equal(a[1][n], b[1][n]), (what, n)
            n_grad += 1
    assert n_grad > 0


@pytest.fixture(scope="module")
def batch():
    return synth.make_images(6, 160, seed=51).to(DEV), synth.make_captions(6, seed=51).to(DEV)


def test_tiny_clip_step_bitwise_at_every_chunking(batch):
    img, tok = batch
    m = _tiny()
    ref = _clip_step(m, img, tok, False)
    for chunk in (0, 5, 1):
        _assert_model_same(_clip_step(m, img, tok, True, chunk), ref, chunk)


@pytest.mark.parametrize("k", [2])
def test_lock_image_tower_bitwise(batch, k):
    img, tok = batch
    m = _tiny()
    m.lock_image_tower(k)
    ref = _clip_step(m, img, tok, False)
    for chunk in (0, 5):
        _assert_model_same(_clip_step(m, img, tok, True, chunk), ref, (k, chunk))


def test_patch_dropout_bitwise(batch):
    img, tok = batch
    cfg = preset("vit-tiny-patch16-160")
    cfg = dict(cfg, vision_cfg=dict(cfg["vision_cfg"], patch_dropout=0.5))
    m = _tiny(cfg)
    m.train()
    ref = _clip_step(m, img, tok, False, seed=3)
    _assert_model_same(_clip_step(m, img, tok, True, seed=3), ref, "patch dropout")
    _assert_model_same(_clip_step(m, img, tok, True, chunk=5, seed=3), ref, "patch dropout, chunks of 5")


def test_frozen_text_soft_token_step_bitwise():
    cfg = preset("vit-tiny-patch16-160")
    V, T = cfg["text_cfg"]["vocab_size"], cfg["text_cfg"]["context_length"]
    g = torch.Generator().manual_seed(9)
    ids = synth.make_captions(3, seed=9)
    soft0 = (torch.nn.functional.one_hot(ids, V).float() * 0.9 + torch.rand(3, T, V, generator=g) * (0.1 / V)).to(DEV)
    target = torch.nn.functional.normalize(torch.randn(3, cfg["embed_dim"], generator=g), dim=-1).to(DEV)
    m = _tiny()
    m.requires_grad_(False)
    out = []
    for remat in (False, True):
        m.set_grad_checkpointing(remat)
        sp = soft0.clone().requires_grad_(True)
        loss = -(training.encode_text(m, sp, normalize=True) * target).sum(-1).mean()
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.detach(), sp.grad.detach().clone()))
        assert all(p.grad is None for p in m.parameters())
    m.set_grad_checkpointing(False)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[1][1].abs().max().item() > 0
