"""GPU: the caption loss kernels (ov_softmax_xent / _backward), the prefix switch of the tower and the caption branch end to end.

Oracles are the torch restatements of tests/prefix_restate.py (fp64 for the loss, fp32 for the block): no reference-generated fixture
backs these tests (jax / flax were not importable where they were written).  Loss tolerances are those of the fp32 ov_clip_loss
tests in tests/test_gpu_ops.py -- the same arithmetic, an fp32 log-sum-exp over a row: rtol 1e-5 / atol 2e-5 for the row lse and the loss
(test_clip_loss_terms), rtol 2e-4 / atol 1e-6 for the gradient (test_clip_loss_backward_vs_oracle)."""
import ctypes as C

import pytest
import torch

import hipops as H
import prefix_restate as PR
from openvision_amd import _lib
from openvision_amd._lib import ptr, stream_ptr, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def xent_case(R, V, seed, mask_kind="mixed"):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(R, V, generator=g) * 4.0).float()
    labels = torch.randint(0, V, (R,), generator=g)
    if R >= 3:
        labels[1] = -1                                     # outside [0, V): one_hot gives a zero row, nll = 0
        labels[2] = V
    if mask_kind == "zero":
        mask = torch.zeros(R)
    elif mask_kind == "ones":
        mask = torch.ones(R)
    else:
        mask = (torch.rand(R, generator=g) < 0.7).float()
        mask[0] = 1.0
    return logits, labels, mask


@pytest.mark.parametrize("R,V", [(256, 32000), (7, 32000), (3, 1000), (1, 33)])
def test_softmax_xent_forward_backward_vs_fp64(R, V):
    logits, labels, mask = xent_case(R, V, seed=R + V)
    want_loss, want_lse, _ = PR.xent_ref64(logits, labels, mask)
    lg, lb, mk = logits.to(DEV), labels.to(DEV), mask.to(DEV)
    loss, lse = PR.softmax_xent(lg, lb, mk)
    print(f"xent R={R} V={V}: loss {float(loss):.6f} want {float(want_loss):.6f}; max |lse err| {float((lse.cpu().double() - want_lse).abs().max()):.2e}")
    torch.testing.assert_close(lse.cpu().double(), want_lse, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(loss.cpu().double()[0], want_loss, rtol=1e-5, atol=2e-5)
    # gradient with g = sum(mask) + 1e-8: dlogits = softmax - onehot on unmasked rows, exactly 0 on masked ones
    gval = float(mask.sum()) + 1e-8
    d = PR.softmax_xent_backward(lg, lb, mk, lse, gval).cpu()
    p = torch.softmax(logits.double(), dim=-1)
    inside = (labels >= 0) & (labels < V)
    want = p.clone()
    want[inside, labels[inside]] -= 1.0
    want = want * mask.double()[:, None]
    torch.testing.assert_close(d.double(), want, rtol=2e-4, atol=1e-6)
    on = mask > 0
    assert not bool(d[~on].any())
    rows = torch.nonzero(on & inside).flatten()
    torch.testing.assert_close(d[rows, labels[rows]].double(), p[rows, labels[rows]] - 1.0, rtol=2e-4, atol=1e-6)
    # dlogits aliased to logits, and a general upstream gradient
    alias = lg.clone()
    PR.softmax_xent_backward(alias, lb, mk, lse, 0.37, out=alias)
    torch.testing.assert_close(alias.cpu().double(), want * (0.37 / gval), rtol=2e-4, atol=1e-6)
    assert torch.equal(alias, PR.softmax_xent_backward(lg, lb, mk, lse, 0.37))


def test_softmax_xent_all_zero_mask():
    logits, labels, mask = xent_case(7, 32000, seed=3, mask_kind="zero")
    logits[4, 17] = float("inf")                                        # a row nobody counts may hold anything
    lg, lb, mk = logits.to(DEV), labels.to(DEV), mask.to(DEV)
    loss, lse = PR.softmax_xent(lg, lb, mk)
    assert float(loss) == 0.0
    d = PR.softmax_xent_backward(lg, lb, mk, lse, 1.0)
    assert not bool(d.any()) and bool(torch.isfinite(d).all())


def test_softmax_xent_padded_pitch():
    R, V = 5, 1000
    logits, labels, mask = xent_case(R, V, seed=9, mask_kind="ones")
    wide = torch.zeros(R, V + 24, device=DEV)
    wide[:, :V] = logits.to(DEV)
    loss, lse = PR.softmax_xent(wide[:, :V], labels.to(DEV), mask.to(DEV))
    want_loss, want_lse, _ = PR.xent_ref64(logits, labels, mask)
    torch.testing.assert_close(lse.cpu().double(), want_lse, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(loss.cpu().double()[0], want_loss, rtol=1e-5, atol=2e-5)


# ---- the prefix switch of the tower (training.tower_forward over a bare Transformer) ------------------------------------------------
from openvision_amd import preset, synth, training                       # noqa: E402
from openvision_amd.caption import CaptionLoss, TextDecoder              # noqa: E402
from openvision_amd.loss import ClipLoss                                 # noqa: E402
from openvision_amd.model import create_model                            # noqa: E402
from test_gpu_remat import _assert_same, _rand_transformer, _tower_step  # noqa: E402

# (width, layers, heads, B, L, P): head_dim 64 below and beyond the resident backward's L, and head_dim 80
MASKED_TOWERS = {"hd64_l307_p179": (192, 3, 3, 2, 307, 179), "hd64_l80_p0": (192, 3, 3, 4, 80, 0), "hd80_l207_p79": (640, 2, 8, 2, 207, 79)}


def _block_weights(blk, dtype):
    t = training._block_tensors(blk)
    return {n: v.detach().to(dtype) for n, v in zip(training._NAMES, t)}


def _restated_tower(tr, x, mask, dtype=torch.float32):
    y = x.to(dtype)
    for blk in tr.resblocks:
        y = PR.block_restated(y, _block_weights(blk, dtype), blk.attn.num_heads, mask, blk.ln_1.eps)
    return y


@pytest.mark.parametrize("shape", list(MASKED_TOWERS), ids=list(MASKED_TOWERS))
def test_masked_tower_paths_bitwise_and_error(shape):
    """With a prefix set: saving forward + backward, the checkpointed pair, a partial backward with a frozen lower block and
    set_backward_chunk_layers(1) give bitwise the same loss and gradients.  Against the restated block (fp32): the masked tower's error
    may not exceed twice the error of the same tower on the same input with prefix = L (the unmasked kernels)."""
    D, layers, heads, Bn, L, P = MASKED_TOWERS[shape]
    tr = _rand_transformer(D, layers, heads, True)
    tr.set_causal_prefix(P)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(Bn, L, D, generator=g).to(DEV)
    wout = (torch.randn(Bn, L, D, generator=g) * 0.1).to(DEV)
    ref = _tower_step(tr, x, wout, False)
    assert ref[1].abs().max().item() > 0
    for remat, chunk in ((True, 0), (False, 1), (True, 1), (True, 2)):
        _assert_same(_tower_step(tr, x, wout, remat, chunk), ref, (shape, remat, chunk))
    # the mask reaches the backward: the same tower unmasked gives other gradients
    tr.set_causal_prefix(None)
    assert not torch.equal(_tower_step(tr, x, wout, False)[1], ref[1])
    tr.set_causal_prefix(P)
    # inference (ov_tower_forward, LN folded) agrees with the training forward to bf16 accuracy, and differs from the unmasked tower
    with torch.no_grad():
        y_inf = tr(x)
        y_trn = training.tower_forward(tr, x)
        tr.set_causal_prefix(L)
        y_full = training.tower_forward(tr, x)
        tr.set_causal_prefix(P)
    want = _restated_tower(tr, x, PR.rule_mask(L, P).to(DEV))
    want_full = _restated_tower(tr, x, PR.rule_mask(L, L).to(DEV))
    e_mask = float((y_trn.float() - want).abs().max())
    e_full = float((y_full.float() - want_full).abs().max())
    e_inf = float((y_inf.float() - want).abs().max())
    print(f"masked tower {shape}: max |err| vs fp32 restated block: prefix={P}: {e_mask:.4e}, prefix=L: {e_full:.4e}, "
          f"inference (LN folded) prefix={P}: {e_inf:.4e}; max |want| {float(want.abs().max()):.3f}")
    assert e_mask <= 2.0 * e_full, (e_mask, e_full)
    assert e_inf <= 4.0 * e_full, (e_inf, e_full)
    # frozen lower block
    for p in tr.resblocks[0].parameters():
        p.requires_grad_(False)
    a, b = _tower_step(tr, x, wout, False), _tower_step(tr, x, wout, True)
    _assert_same(b, a, (shape, "block 0 frozen"))
    assert torch.equal(a[1], ref[1]) and torch.equal(a[2]["resblocks.1.attn.in_proj_weight"], ref[2]["resblocks.1.attn.in_proj_weight"])


def test_tower_prefix_rejections():
    lib = _lib.load()
    tr = _rand_transformer(192, 1, 3, True)
    x = torch.randn(2, 40, 192).to(DEV)
    with pytest.raises(ValueError):
        tr.set_causal_prefix(-1)
    tr.set_causal_prefix(41)
    with pytest.raises(ValueError):
        tr(x)
    with pytest.raises(ValueError):
        training.tower_forward(tr, x.clone().requires_grad_(True))
    # the C entry point itself: a prefix beyond L is OV_ERR_INVALID from the call
    tr.set_causal_prefix(None)
    h = tr.tower().handle
    assert lib.ov_tower_set_prefix(h, 41) == 0
    xb = x.to(torch.bfloat16).contiguous()
    nb = lib.ov_tower_workspace_bytes(h, 2, 40)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    assert lib.ov_tower_forward(h, ptr(xb), 2, 40, ptr(ws), nb, stream_ptr()) == -1
    assert lib.ov_tower_set_prefix(h, -1) == 0


# ---- end to end on the tiny preset ------------------------------------------------------------------------------------------------------
def _tiny_pair(seed=3):
    cfg = preset("vit-tiny-patch16-160")
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    torch.manual_seed(seed)
    vw, tw = m.visual.transformer.width, m.transformer.width
    dec = TextDecoder(vw, tw, 192, 2, 3, 768, m.token_embedding.weight.shape[0], num_learnable_tokens=128).to(DEV)
    return m, dec


def test_coca_step_end_to_end():
    """coca_forward + ClipLoss + 2 CaptionLoss, backward, one FusedAdamW step.  The caption logits are compared with the restated
    decoder (fp32) run on the tokens the towers produced.  Tolerance: the masked tower error measured by
    test_masked_tower_paths_bitwise_and_error at this decoder's shape (hd64_l307_p179: max |err| 6.9e-2 of the stack's bf16 output
    against the fp32 restated blocks, at max |value| 7.2; 0.07 used here), propagated through decoder_norm and the
    head: a head row has norm ~1 (std width^-0.5 over width entries) and the LayerNorm rescales by 1 / std(x) ~ 1, for which a factor 4
    is allowed; the bf16 rounding of the head GEMM's operands and output adds 2^-7 |logit|.  So |logit error| <= 4 * 0.07 + 2^-7 |logit|
    (measured: 4.4e-2 at max |logit| 4.9)."""
    m, dec = _tiny_pair()
    img, tok = synth.make_images(4, 160, seed=51).to(DEV), synth.make_captions(4, seed=51).to(DEV)
    labels = torch.randint(0, dec.vocab_size, (4, 128), generator=torch.Generator().manual_seed(1)).to(DEV)
    mask = (torch.rand(4, 128, generator=torch.Generator().manual_seed(2)) < 0.8).float().to(DEV)
    opt = training.FusedAdamW([m, dec], lr=1e-3)
    names = {id(p): n for g in opt.groups for n, p in g["params"]}
    undecayed = {n for g in opt.groups if g["wd"] == 0.0 for n, _ in g["params"]}
    assert "1.learnable_tokens" in undecayed and "1.decoder_norm.weight" in undecayed and "1.head.weight" not in undecayed
    # contrastive loss alone
    opt.zero_grad()
    ClipLoss()(*training.clip_forward(m, img, tok)).backward()
    clip_only = {n: p.grad.detach().clone() for n, p in m.visual.named_parameters()}
    opt.zero_grad()
    img_f, txt_f, scale, cap = training.coca_forward(m, dec, img, tok)
    assert cap.shape == (4, 128, dec.vocab_size) and cap.dtype == torch.float32
    loss = ClipLoss()(img_f, txt_f, scale) + 2 * CaptionLoss()(cap, labels, mask)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    for mod in (m, dec):
        for n, p in mod.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    changed = [n for n, p in m.visual.named_parameters() if not torch.equal(p.grad, clip_only[n])]
    assert any("transformer.resblocks" in n for n in changed) and "conv1.weight" in changed     # the caption gradient reaches the image tower
    # inference == training forward, bitwise; and the restated decoder
    with torch.no_grad():
        _, img_tok = training.encode_image(m, img, True, output_tokens=True)
        _, txt_tok = training.encode_text(m, tok, True, output_tokens=True)
        assert img_tok.shape[1] == 100 and txt_tok.shape[1] == tok.shape[1] - 1
        inf = dec(img_tok, txt_tok)
        trn = training.decode(dec, img_tok, txt_tok)
        assert torch.equal(inf, trn)
        assert torch.equal(trn, cap.detach())
        F = torch.nn.functional
        x = torch.cat([img_tok.float() @ dec.image_projection.weight.T, txt_tok.float() @ dec.text_projection.weight.T,
                       dec.learnable_tokens.float().expand(4, -1, -1)], dim=1)
        L, P = x.shape[1], img_tok.shape[1] + txt_tok.shape[1]
        y = _restated_tower(dec.transformer, x, PR.rule_mask(L, P).to(DEV))[:, -128:]
        want = F.layer_norm(y, (dec.width,), dec.decoder_norm.weight, dec.decoder_norm.bias, dec.decoder_norm.eps) @ dec.head.weight.T
        err = (inf - want).abs()
        print(f"caption logits vs restated decoder: max |err| {float(err.max()):.4e}, max |logit| {float(want.abs().max()):.3f}")
        assert bool((err <= 4 * 0.07 + 2.0 ** -7 * want.abs()).all())
    before = dec.learnable_tokens.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(dec.learnable_tokens.detach(), before) and bool(torch.isfinite(dec.learnable_tokens).all())
