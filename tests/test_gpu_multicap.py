"""GPU: the fused multi-caption InfoNCE (csrc/multicap.hip behind openvision_amd.loss.MultiCaptionClipLoss) against the reference's
ClipLoss run per caption set (tests/golden/multicap_grad.npz, made over gloo in float64), the float64 restatement of the JAX
function (tests/multicap_restate.py) on the device, ov_clip_loss per set, and the two-caption training step."""

import numpy as np
import pytest
import torch

from openvision_amd import _lib, preset, synth, training
from openvision_amd._lib import check, ptr, stream_ptr
from openvision_amd.caption import CaptionLoss, TextDecoder
from openvision_amd.loss import ClipLoss, MultiCaptionClipLoss
from openvision_amd.model import create_model

import hipops as H
import multicap_restate as MR
from conftest import golden
from ranks import run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_kernels(img, txt, all_img, sets, s, off, packed=False, grad=1.0, gathered=True):
    """ov_clip_loss_multi + ov_clip_loss_multi_backward.  img [b, E], txt [C b, E], all_img [N, E], sets [C, N, E] (fp32, device).
    ``packed``: the gathered operands are handed over as ONE [N, (1 + C) E] buffer read in place (ld = (1 + C) E, set stride E) and
    the gathered-side gradient comes back in a buffer of the same layout; else as separate arrays (ld = E, set stride N E).
    Returns loss, terms [4 C, b], d_img, d_txt, d_all_img [N, E] | None, d_all_txt [C, N, E] | None, d_scale."""
    lib = _lib.load()
    b, e = img.shape
    c, n = sets.shape[0], all_img.shape[0]
    if packed:
        buf = torch.cat([all_img] + list(sets), dim=1).contiguous()
        p_ai, p_at, ld, ss = ptr(buf), ptr(buf[:, e:]), (1 + c) * e, e
    else:
        sets = sets.contiguous()
        p_ai, p_at, ld, ss = ptr(all_img), ptr(sets), e, n * e
    sc = torch.full((1,), float(s), dtype=torch.float32, device=DEV)
    gr = torch.full((1,), float(grad), dtype=torch.float32, device=DEV)
    nb = lib.ov_clip_loss_multi_workspace_bytes(b, n, c)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    terms = torch.empty(4 * c, b, dtype=torch.float32, device=DEV)
    check(lib.ov_clip_loss_multi(ptr(img), ptr(txt), p_ai, p_at, ld, ss, b, n, e, c, ptr(sc), off, ptr(loss), ptr(terms), ptr(ws), nb,
                                 stream_ptr()), "ov_clip_loss_multi")
    d_img, d_txt = torch.empty_like(img), torch.empty_like(txt)
    d_s = torch.empty(1, dtype=torch.float32, device=DEV)
    if not gathered:
        gbuf, g_ai, g_at, ldg, gss = None, None, None, 0, 0
    elif packed:
        gbuf = torch.full((n, (1 + c) * e), float("nan"), dtype=torch.float32, device=DEV)
        g_ai, g_at, ldg, gss = ptr(gbuf), ptr(gbuf[:, e:]), (1 + c) * e, e
    else:
        gbuf = torch.full(((1 + c) * n, e), float("nan"), dtype=torch.float32, device=DEV)
        g_ai, g_at, ldg, gss = ptr(gbuf), ptr(gbuf[n:]), e, n * e
    nbb = lib.ov_clip_loss_multi_backward_workspace_bytes(b, n, c)
    wsb = torch.empty(nbb + 16, dtype=torch.uint8, device=DEV)
    check(lib.ov_clip_loss_multi_backward(ptr(img), ptr(txt), p_ai, p_at, ld, ss, b, n, e, c, ptr(sc), off, ptr(terms), ptr(gr),
                                          ptr(d_img), ptr(d_txt), g_ai, g_at, ldg, gss, ptr(d_s), ptr(wsb), nbb, stream_ptr()),
          "ov_clip_loss_multi_backward")
    if not gathered:
        d_ai = d_at = None
    elif packed:
        d_ai = gbuf[:, :e].contiguous()
        d_at = torch.stack([gbuf[:, (1 + k) * e:(2 + k) * e] for k in range(c)]).contiguous()
    else:
        d_ai, d_at = gbuf[:n], gbuf[n:].view(c, n, e)
    return loss[0], terms, d_img, d_txt, d_ai, d_at, d_s[0]


def close(got, ref, rel, what):
    got, ref = got.double().cpu(), torch.as_tensor(ref).double().cpu()
    err, mag = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max |err| {err:.3e} at max |ref| {mag:.3e}")
    assert got.shape == ref.shape and err <= rel * mag, (what, err, mag)


@pytest.mark.parametrize("case", MR.CASES, ids=[c[0] for c in MR.CASES])
def test_kernel_against_the_reference_fixture(case):
    """One process plays every rank: its local rows against the packed gathered set, label offset b r (or, without local_loss,
    the global rows against themselves), then the gathered side routed as the case's mode prescribes.  Loss to 1e-5 relative;
    gradients to 1e-5 of their largest entry."""
    z = golden("multicap_grad.npz")
    name, ws, b, e, c, local_loss, gwg, s, seed = case
    img64, sets64 = MR.case_inputs(ws, b, e, c, seed)
    assert abs(float(img64.sum()) - float(z[f"{name}_img_sum"])) <= 1e-9 * float(z[f"{name}_img_abs_sum"])
    assert abs(float(sets64.sum()) - float(z[f"{name}_txt_sum"])) <= 1e-9 * float(z[f"{name}_txt_abs_sum"])
    img, sets = img64.float().to(DEV), sets64.float().to(DEV)
    n = ws * b
    per = []
    for r in range(ws):
        if local_loss or ws == 1:
            x_img, x_txt, off = img[r * b:(r + 1) * b].contiguous(), MR.stack_local(sets, r, b).contiguous(), b * r
        else:
            x_img, x_txt, off = img, sets.reshape(c * n, e), 0
        per.append(run_kernels(x_img, x_txt, img, sets, s, off, packed=True))
    for r in range(ws):
        loss, _, d_img, d_txt, d_ai, d_at, d_s = per[r]
        if ws == 1:
            gi, gt = d_img + d_ai, d_txt + d_at.reshape(c * n, e)
        elif local_loss:
            gi, gt = d_img, d_txt
            if gwg:
                gi = gi + sum(p[4] for p in per)[r * b:(r + 1) * b]
                gt = gt + MR.stack_local(sum(p[5] for p in per), r, b)
        else:
            assert not gwg
            gi = (d_img + d_ai)[r * b:(r + 1) * b]
            gt = MR.stack_local(d_txt.view(c, n, e) + d_at, r, b)
        ref = float(z[f"{name}_loss"][r])
        print(f"{name} rank {r}: loss {float(loss):.8f} reference {ref:.8f} rel err {abs(float(loss) - ref) / abs(ref):.3e}")
        assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (name, r, float(loss), ref)
        close(gi, z[f"{name}_dimg"][r], 1e-5, (name, r, "dimg"))
        close(gt, z[f"{name}_dtxt"][r], 1e-5, (name, r, "dtxt"))
        close(d_s.reshape(1), [float(z[f"{name}_dscale"][r])], 1e-5, (name, r, "dscale"))


# b, N, E, C, off
SHAPES = [(13, 39, 64, 2, 13),          # ragged row tile; two e-tiles, so two of the four waves own none
          (45, 135, 96, 3, 90),         # e-tile count not a multiple of 4; last rank
          (32, 32, 1152, 1, 0),         # the backward's width limit
          (100, 700, 384, 2, 300),      # several column splits
          (1000, 3000, 768, 2, 1000)]   # ragged and large


@pytest.mark.parametrize("b,N,E,C,off", SHAPES, ids=[f"b{s[0]}_n{s[1]}_e{s[2]}_c{s[3]}" for s in SHAPES])
def test_kernel_against_float64_restatement(b, N, E, C, off):
    """Loss, terms and every gradient against the float64 restatement evaluated on the device, at the tolerances of the merged
    ov_clip_loss tests (a float64 comparand can only be closer than the fp32 one those were set against); upstream gradient 0.5.
    Then: two calls are bitwise equal, the local-side-only call gives bitwise the same local gradients, and packed and unpacked
    operands give bitwise the same results."""
    s, rank = 1 / 0.07, off // b
    img64, sets64 = MR.make_inputs(N, E, C, seed=1000 + b)
    img64, sets64 = img64.to(DEV), sets64.to(DEV)
    all_img, sets = img64.float(), sets64.float()
    x_img = all_img[off:off + b].contiguous()
    x_txt = torch.cat([sets[k, off:off + b] for k in range(C)]).contiguous()
    got = run_kernels(x_img, x_txt, all_img, sets, s, off, packed=True, grad=0.5)
    loss, terms, d_img, d_txt, d_ai, d_at, d_s = got
    a64 = (img64[off:off + b], torch.cat([sets64[k, off:off + b] for k in range(C)]), img64, sets64, s, rank, C)
    want_loss, want_terms = MR.strip_loss(*a64), MR.strip_terms(*a64)
    w_img, w_txt, w_ai, w_at, w_s = MR.strip_grads(*a64, grad=0.5)
    print(f"loss {float(loss):.7f} float64 {float(want_loss):.7f} |err| {abs(float(loss) - float(want_loss)):.3e}; "
          f"terms max |err| {float((terms.double() - want_terms).abs().max()):.3e}; "
          f"d_scale {float(d_s):.6e} float64 {float(w_s):.6e}")
    np.testing.assert_allclose(terms.cpu().numpy(), want_terms.cpu().numpy(), rtol=1e-5, atol=2e-5)
    assert abs(float(loss) - float(want_loss)) < 2e-5
    for name, g_, w in (("d_img", d_img, w_img), ("d_txt", d_txt, w_txt), ("d_all_img", d_ai, w_ai), ("d_all_txt", d_at, w_at)):
        assert g_.shape == w.shape, name
        print(f"{name}: max |err| {float((g_.double() - w).abs().max()):.3e} at max |ref| {float(w.abs().max()):.3e}")
        np.testing.assert_allclose(g_.cpu().numpy(), w.cpu().numpy(), rtol=2e-4, atol=1e-6, err_msg=name)
    assert abs(float(d_s) - float(w_s)) < 2e-6 + 2e-4 * abs(float(w_s))
    again = run_kernels(x_img, x_txt, all_img, sets, s, off, packed=True, grad=0.5)
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    local = run_kernels(x_img, x_txt, all_img, sets, s, off, packed=True, grad=0.5, gathered=False)
    assert local[4] is None and local[5] is None
    assert torch.equal(local[2], d_img) and torch.equal(local[3], d_txt) and torch.equal(local[6], d_s)
    unpacked = run_kernels(x_img, x_txt, all_img, sets, s, off, packed=False, grad=0.5)
    for x, y in zip(got, unpacked):
        assert torch.equal(x, y)


def test_two_sets_agree_with_ov_clip_loss_per_set():
    """At C = 2 the terms of each set are ov_clip_loss's on (img, txt_c), and the loss is the mean of the two."""
    b, N, E, off, s = 100, 700, 384, 300, 1 / 0.07
    img64, sets64 = MR.make_inputs(N, E, 2, seed=31)
    all_img, sets = img64.float().to(DEV), sets64.float().to(DEV).contiguous()
    x_img = all_img[off:off + b].contiguous()
    x_txt = torch.cat([sets[k, off:off + b] for k in range(2)]).contiguous()
    loss, terms = run_kernels(x_img, x_txt, all_img, sets, s, off, packed=True)[:2]
    singles = []
    for k in range(2):
        l1, t1 = H.clip_loss(x_img, x_txt[k * b:(k + 1) * b].contiguous(), all_img, sets[k], s, off)
        np.testing.assert_allclose(terms[4 * k:4 * k + 4].cpu().numpy(), t1.cpu().numpy(), rtol=1e-5, atol=2e-5)
        singles.append(float(l1))
    assert abs(float(loss) - 0.5 * (singles[0] + singles[1])) < 2e-5
    assert abs(singles[0] - singles[1]) > 1e-6                    # the sets differ


MODES = [(True, False), (True, True), (False, False)]


def _module_inputs():
    img, sets = MR.make_inputs(24, 192, 2, seed=5)
    return img, sets, 1 / 0.07


def _module_run(fn, img, sets, s):
    a = img.float().to(DEV).requires_grad_(True)
    t = torch.cat(list(sets.float())).to(DEV).requires_grad_(True)
    sc = torch.tensor(s, device=DEV, requires_grad=True)
    out = fn(a, t, sc, output_dict=True)
    assert set(out) == {"contrastive_loss"}
    out["contrastive_loss"].backward()
    with torch.no_grad():
        plain = fn(a, t, sc)
    assert torch.equal(plain, out["contrastive_loss"].detach()) and fn.last_terms.shape == (4 * sets.shape[0], img.shape[0])
    return float(plain), a.grad.cpu(), t.grad.cpu(), float(sc.grad)


def _module_check(got, img, sets, s, what):
    """World size 1 in every mode: the gradient of a feature is its local-side plus its gathered-side term."""
    (want_loss, w_img, w_txt, w_s), = MR.per_rank(img, sets, s, 1, True, False)
    loss, g_img, g_txt, g_s = got
    assert abs(loss - float(want_loss)) < 2e-5, what
    np.testing.assert_allclose(g_img.numpy(), w_img.numpy(), rtol=2e-4, atol=1e-6, err_msg=str(what))
    np.testing.assert_allclose(g_txt.numpy(), w_txt.numpy(), rtol=2e-4, atol=1e-6, err_msg=str(what))
    assert abs(g_s - float(w_s)) < 2e-6 + 2e-4 * abs(float(w_s)), what


@pytest.mark.parametrize("local_loss,gwg", MODES)
def test_module_world_size_1(local_loss, gwg):
    img, sets, s = _module_inputs()
    fn = MultiCaptionClipLoss(2, local_loss=local_loss, gather_with_grad=gwg)
    _module_check(_module_run(fn, img, sets, s), img, sets, s, (local_loss, gwg))
    one = MultiCaptionClipLoss(1)                                  # one set: the terms are ClipLoss's
    a, t = img.float().to(DEV), sets[0].float().to(DEV)
    ref = ClipLoss()
    l1, l0 = one(a, t, s), ref(a, t, s)
    assert abs(float(l1) - float(l0)) < 2e-5
    np.testing.assert_allclose(one.last_terms.cpu().numpy(), ref.last_terms.cpu().numpy(), rtol=1e-5, atol=2e-5)


def _nccl_ws1_rank(rank, ws):
    img, sets, s = _module_inputs()
    out = {}
    for local_loss, gwg in MODES:
        fn = MultiCaptionClipLoss(2, local_loss=local_loss, gather_with_grad=gwg, rank=0, world_size=1)
        fn.always_collective = True                          # all_gather_into_tensor (+ reduce_scatter_tensor) at world 1
        loss, gi, gt, gs = _module_run(fn, img, sets, s)
        out[(local_loss, gwg)] = (loss, gi.numpy(), gt.numpy(), gs)
    return out


def test_rccl_branch_of_the_module_at_world_size_1():
    """The RCCL code path (packed all-gather read in place, packed gathered-side gradient, reduce-scatter) in a world of one rank.
    A detached gather with local_loss returns the local-side gradient alone; the other two modes return the whole gradient."""
    out, = run_ranks(_nccl_ws1_rank, 1, timeout=600, backend="nccl", gpu=True)
    img, sets, s = _module_inputs()
    for (local_loss, gwg), (loss, gi, gt, gs) in out.items():
        got = (loss, torch.from_numpy(gi), torch.from_numpy(gt), gs)
        if local_loss and not gwg:
            args = (img, torch.cat(list(sets)), img, sets, s, 0, 2)
            w_img, w_txt, _, _, w_s = MR.strip_grads(*args)
            assert abs(loss - float(MR.strip_loss(*args))) < 2e-5
            np.testing.assert_allclose(gi, w_img.numpy(), rtol=2e-4, atol=1e-6)
            np.testing.assert_allclose(gt, w_txt.numpy(), rtol=2e-4, atol=1e-6)
            assert abs(gs - float(w_s)) < 2e-6 + 2e-4 * abs(float(w_s))
        else:
            _module_check(got, img, sets, s, (local_loss, gwg))


def test_two_caption_training_step_tiny():
    """vit-tiny-patch16-160, B = 4, C = 2: coca_forward on [8, T] tokens, MultiCaptionClipLoss + 2 CaptionLoss, backward, one
    FusedAdamW step.  The decoder sees the first set only (its logits are bitwise those of a call given the first 4 token rows);
    the contrastive term and the gradients arriving at the features are those of 0.5 (ClipLoss(set 1) + ClipLoss(set 2))."""
    cfg = preset("vit-tiny-patch16-160")
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    torch.manual_seed(3)
    dec = TextDecoder(m.visual.transformer.width, m.transformer.width, 192, 2, 3, 768, m.token_embedding.weight.shape[0],
                      num_learnable_tokens=128).to(DEV)
    img = synth.make_images(4, 160, seed=51).to(DEV)
    tok = torch.cat([synth.make_captions(4, seed=51), synth.make_captions(4, seed=52)]).to(DEV)
    assert tok.shape[0] == 8 and not torch.equal(tok[:4], tok[4:])
    labels = torch.randint(0, dec.vocab_size, (4, 128), generator=torch.Generator().manual_seed(1)).to(DEV)
    mask = (torch.rand(4, 128, generator=torch.Generator().manual_seed(2)) < 0.8).float().to(DEV)
    opt = training.FusedAdamW([m, dec], lr=1e-3)
    with torch.no_grad():
        cap_first = training.coca_forward(m, dec, img, tok[:4])[3]
    opt.zero_grad()
    img_f, txt_f, scale, cap = training.coca_forward(m, dec, img, tok)
    assert img_f.shape[0] == 4 and txt_f.shape[0] == 8 and cap.shape == (4, 128, dec.vocab_size)
    assert torch.equal(cap.detach(), cap_first)                   # the decoder did not see set 2
    img_f.retain_grad()
    txt_f.retain_grad()
    contrastive = MultiCaptionClipLoss()(img_f, txt_f, scale)
    loss = contrastive + 2 * CaptionLoss()(cap, labels, mask)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    # the composition on the same features
    fi, ft = img_f.detach().clone().requires_grad_(True), txt_f.detach().clone().requires_grad_(True)
    comp = 0.5 * (ClipLoss()(fi, ft[:4], scale.detach()) + ClipLoss()(fi, ft[4:], scale.detach()))
    comp.backward()
    print(f"contrastive {float(contrastive):.7f} composition {float(comp):.7f}")
    assert abs(float(contrastive) - float(comp)) < 2e-5
    np.testing.assert_allclose(txt_f.grad.cpu().numpy(), ft.grad.cpu().numpy(), rtol=2e-4, atol=1e-6)
    # img_f also feeds nothing but the contrastive term (the decoder takes the image TOKENS), so its gradient is the composition's
    np.testing.assert_allclose(img_f.grad.cpu().numpy(), fi.grad.cpu().numpy(), rtol=2e-4, atol=1e-6)
    before = {}
    for k, mod in enumerate((m, dec)):
        for n, p in mod.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
            before[(k, n)] = p.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    for k, mod in enumerate((m, dec)):
        for n, p in mod.named_parameters():
            assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[(k, n)]), n
