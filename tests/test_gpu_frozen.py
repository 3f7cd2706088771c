"""GPU: training with frozen parameters.  The partial tower entry points against the all-trainable ones (bitwise: kept slots of
ov_tower_forward_saving_from, every requested gradient of ov_tower_backward_partial), and the model level: lock_image_tower(k) and a
frozen text tower give the all-trainable gradients for what is unlocked and nothing for what is not."""
import ctypes as C

import pytest
import torch

from openvision_amd import _lib, preset, synth
from openvision_amd._lib import ptr, stream_ptr
from openvision_amd.model import create_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (width, layers, heads, mlp, gelu_tanh, B, L)
SHAPES = {
    "tiny_b4_l101": (192, 3, 3, 768, False, 4, 101),
    "l14_4blk_b8_l257": (1024, 4, 16, 4096, False, 8, 257),
    "text_b6_l80": (192, 4, 3, 768, True, 6, 80),
    "hd80_b3_l257": (640, 3, 8, 2560, False, 3, 257),         # head_dim 80: no lse is kept
    "text_b16_l80_m1280": (384, 3, 6, 1536, True, 16, 80),    # B * L a multiple of 64: the dW products take the TN route
}


def _rand_tower(lib, g, D, layers, heads, mlp, tanh):
    cfg = _lib.TowerCfg(D, layers, heads, mlp, mlp, int(tanh), 1e-6)
    t = lib.ov_tower_create(C.byref(cfg))
    assert t
    keep = []
    for i in range(layers):
        mat = lambda n, k: (torch.randn(n, k, generator=g) * k ** -0.5).to(torch.bfloat16).to(DEV)
        vec = lambda n, s=0.02, m=0.0: (torch.randn(n, generator=g) * s + m).to(DEV)
        ts = [vec(D, 0.1, 1.0), vec(D), mat(3 * D, D), vec(3 * D), mat(D, D), vec(D), vec(D, 0.1, 1.0), vec(D), mat(mlp, D), vec(mlp),
              mat(D, mlp), vec(D)]
        keep.append(ts)
        _lib.check(lib.ov_tower_set_block(t, i, C.byref(_lib.BlockWeights(*[C.c_void_p(x.data_ptr()) for x in ts], None, None))), "set")
    return t, keep


def _forward_from(lib, t, first, x, Bn, L):
    n = lib.ov_tower_saved_bytes_from(t, first, Bn, L)
    saved = torch.zeros(n, dtype=torch.uint8, device=DEV) if n else None           # zeroed: the unused lse region compares equal
    nb = lib.ov_tower_forward_saving_from_workspace_bytes(t, first, Bn, L)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV) if nb else None
    y = x.clone()
    _lib.check(lib.ov_tower_forward_saving_from(t, first, ptr(y), ptr(saved), Bn, L, ptr(ws), nb, stream_ptr()), "forward_saving_from")
    return y, saved


def _patterns(layers):
    """(name, trainable pairs per block, want_dx); pairs: 0 ln_1, 1 in_proj, 2 out_proj, 3 ln_2, 4 c_fc, 5 c_proj"""
    allp, none = set(range(6)), set()
    return [
        ("top_block", [none] * (layers - 1) + [allp], 0),
        ("top_block_dx", [none] * (layers - 1) + [allp], 1),
        ("alternating", [allp if i % 2 == 0 else none for i in range(layers)], 1),
        ("alternating_odd", [allp if i % 2 == 1 else none for i in range(layers)], 0),
        ("bottom_cproj_only", [{5}] + [none] * (layers - 2) + [allp], 0),
        ("second_ln1_only", [none, {0}] + [none] * (layers - 3) + [{3, 1}], 0),
        ("mixed_dx", [{0, 4}] + [{2}] * (layers - 1), 1),
        ("all_no_dx", [allp] * layers, 0),
        ("all_frozen_dx", [none] * layers, 1),
    ]


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_partial_forward_and_backward_bitwise(shape):
    D, layers, heads, mlp, tanh, Bn, L = SHAPES[shape]
    lib = _lib.load()
    g = torch.Generator().manual_seed(23)
    t, keep = _rand_tower(lib, g, D, layers, heads, mlp, tanh)
    try:
        M = Bn * L
        x = torch.randn(M, D, generator=g).to(torch.bfloat16).to(DEV)
        dy = (torch.randn(M, D, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
        # the all-trainable path
        full = torch.zeros(lib.ov_tower_saved_bytes(t, Bn, L), dtype=torch.uint8, device=DEV)
        nb = lib.ov_tower_workspace_bytes(t, Bn, L)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        y_full = x.clone()
        _lib.check(lib.ov_tower_forward_saving(t, ptr(y_full), ptr(full), Bn, L, ptr(ws), nb, stream_ptr()), "forward_saving")
        ref = [[torch.empty_like(p) for p in ts] for ts in keep]
        garr = (_lib.BlockGrads * layers)(*[_lib.BlockGrads(*[C.c_void_p(p.data_ptr()) for p in gs]) for gs in ref])
        dx_full = dy.clone()
        nbb = lib.ov_tower_backward_workspace_bytes(t, Bn, L)
        wsb = torch.empty(nbb, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ov_tower_backward(t, ptr(full), ptr(dx_full), garr, Bn, L, ptr(wsb), nbb, stream_ptr()), "ov_tower_backward")
        dx_in = dy.clone()
        nbi = lib.ov_tower_backward_input_workspace_bytes(t, Bn, L)
        wsi = torch.empty(nbi, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ov_tower_backward_input(t, ptr(full), ptr(dx_in), Bn, L, ptr(wsi), nbi, stream_ptr()), "ov_tower_backward_input")
        torch.cuda.synchronize()
        assert torch.isfinite(dx_full.float()).all() and dx_full.float().abs().max().item() > 0

        # forward: the kept slots and the output are ov_tower_forward_saving's
        slot = full.numel() // layers
        kept = {}
        for first in sorted({0, 1, layers - 1, layers}):
            y, saved = _forward_from(lib, t, first, x, Bn, L)
            torch.cuda.synchronize()
            assert torch.equal(y, y_full), (shape, first)
            if first < layers:
                assert saved.numel() == (layers - first) * slot
                assert torch.equal(saved, full[first * slot:]), (shape, first)
            else:
                assert saved is None
            kept[first] = saved

        # backward over several frozen patterns
        nbp = lib.ov_tower_backward_partial_workspace_bytes(t, Bn, L)
        wsp = torch.empty(nbp, dtype=torch.uint8, device=DEV)
        for name, pairs, want_dx in _patterns(layers):
            first = 0 if want_dx else next((i for i, p in enumerate(pairs) if p), layers)
            saved = kept.get(first)
            if saved is None and first < layers:
                _, saved = _forward_from(lib, t, first, x, Bn, L)
            got = [[torch.full_like(p, float("nan")) if j // 2 in pairs[i] else None for j, p in enumerate(keep[i])] for i in range(layers)]
            garr = (_lib.BlockGrads * (layers - first))(*[_lib.BlockGrads(*[ptr(p) for p in gs]) for gs in got[first:]])
            dx = dy.clone()
            _lib.check(lib.ov_tower_backward_partial(t, first, ptr(saved), ptr(dx), garr, want_dx, Bn, L, ptr(wsp), nbp, stream_ptr()),
                       f"ov_tower_backward_partial {name}")
            torch.cuda.synchronize()
            for i in range(layers):
                for j in range(12):
                    if got[i][j] is not None:
                        assert torch.equal(got[i][j], ref[i][j]), (shape, name, i, j)
            if want_dx:
                assert torch.equal(dx, dx_full), (shape, name)
            if name == "all_frozen_dx":
                assert torch.equal(dx, dx_in), shape
    finally:
        lib.ov_tower_destroy(t)


# ---- model level --------------------------------------------------------------------------------------------------------------------
def _tiny():
    cfg = preset("vit-tiny-patch16-160")
    return create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))


def _step(m, img, tok):
    from openvision_amd import training
    from openvision_amd.loss import ClipLoss
    loss = ClipLoss()(*training.clip_forward(m, img, tok))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach()


@pytest.fixture(scope="module")
def reference_step():
    img, tok = synth.make_images(6, 160, seed=41).to(DEV), synth.make_captions(6, seed=41).to(DEV)
    m = _tiny()
    for p in m.parameters():
        p.requires_grad_(True)
    loss = _step(m, img, tok)
    return img, tok, loss, {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("k", [0, 1, 2, 13])
def test_lock_image_tower_gradients_bitwise(reference_step, k):
    from openvision_amd import training
    img, tok, ref_loss, ref_grads = reference_step
    m = _tiny()
    layers = len(m.visual.transformer.resblocks)
    assert k <= layers + 1
    m.lock_image_tower(k)
    loss = _step(m, img, tok)
    assert torch.equal(loss, ref_loss), k
    n_unlocked = 0
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, ref_grads[n]), (k, n)
            n_unlocked += 1
        else:
            assert p.grad is None, (k, n)
    assert n_unlocked == sum(1 for n in ref_grads if not n.startswith("visual.")) + {0: 0, 1: 1, 2: 15, 13: 147}[k]
    pool = training._pool(m.visual.transformer)
    if k <= 1:                          # the whole tower is frozen and its input needs no gradient: nothing is kept
        assert pool.peak.get("saved", 0) == 0 and not pool.lists.get("saved"), k
    # one optimiser step (built after locking) moves only what is unlocked
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = training.FusedAdamW(m, lr=1e-3)
    opt.zero_grad()
    _step(m, img, tok)
    opt.step()
    torch.cuda.synchronize()
    moved = 0
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p.detach(), before[n]), (k, n)
        else:
            moved += int(not torch.equal(p.detach(), before[n]))
    assert moved > 0


def test_mixed_pair_keeps_the_trainable_half():
    """A pair with one frozen tensor is computed with its partner; the frozen half gets no .grad, the other one is bitwise."""
    img, tok = synth.make_images(4, 160, seed=43).to(DEV), synth.make_captions(4, seed=43).to(DEV)
    ref = _tiny()
    _step(ref, img, tok)
    m = _tiny()
    vb = m.visual.transformer.resblocks
    for p in m.visual.parameters():
        p.requires_grad_(False)
    vb[5].ln_2.weight.requires_grad_(True)                       # ln_2 bias frozen
    vb[7].attn.in_proj_bias.requires_grad_(True)                 # in_proj weight frozen
    m.transformer.resblocks[3].mlp.c_fc.weight.requires_grad_(False)
    _step(m, img, tok)
    rp = dict(ref.named_parameters())
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, rp[n].grad), n
        else:
            assert p.grad is None, n


def test_frozen_text_tower_soft_token_gradient_bitwise():
    """Gradient ascent on soft tokens (ov-gradient-ascent.py): with every parameter frozen the text backward is input-only, and the
    gradient on the soft rows is bitwise the one computed with the parameters trainable."""
    from openvision_amd import training
    cfg = preset("vit-tiny-patch16-160")
    V, T = cfg["text_cfg"]["vocab_size"], cfg["text_cfg"]["context_length"]
    g = torch.Generator().manual_seed(9)
    ids = synth.make_captions(3, seed=9)
    soft0 = (torch.nn.functional.one_hot(ids, V).float() * 0.9 + torch.rand(3, T, V, generator=g) * (0.1 / V)).to(DEV)
    target = torch.nn.functional.normalize(torch.randn(3, cfg["embed_dim"], generator=g), dim=-1).to(DEV)
    out = []
    for frozen in (False, True):
        m = _tiny()
        m.requires_grad_(not frozen)
        sp = soft0.clone().requires_grad_(True)
        loss = -(training.encode_text(m, sp, normalize=True) * target).sum(-1).mean()
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.detach(), sp.grad.detach().clone()))
        if frozen:
            assert all(p.grad is None for p in m.parameters())
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[1][1].abs().max().item() > 0
