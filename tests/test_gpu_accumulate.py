"""GPU: gradient accumulation for the InfoNCE -- ov_clip_loss_window_backward (csrc/window.hip) against the reference-made fixture
tests/golden/multicap_grad.npz, against the float64 window restatement (tests/window_restate.py) and against the existing backward at
b = N on the device; openvision_amd.accumulate.ContrastiveAccumulator in a world of one and of two; training.accumulated_step on the
Tiny model against torch autograd through the oracle, under recomputation, a locked image tower, patch dropout and the caption
branch."""
import numpy as np
import pytest
import torch

from openvision_amd import _lib, preset, synth, training
from openvision_amd._lib import check, ptr, stream_ptr
from openvision_amd.accumulate import ContrastiveAccumulator
from openvision_amd.loss import ClipLoss, MultiCaptionClipLoss
from openvision_amd.model import create_model

import multicap_restate as MR
import window_restate as WR
from conftest import golden
from ranks import run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 1 / 0.07


def scalar(v):
    return torch.full((1,), float(v), dtype=torch.float32, device=DEV)


def bank_operands(img, sets, packed):
    """The bank img [N, E], sets [C, N, E] as the kernels address it: (keepalive, all_img ptr, all_txt ptr, ld, set_stride)."""
    c, n, e = sets.shape
    if packed:
        buf = torch.cat([img] + list(sets), dim=1).contiguous()
        return buf, ptr(buf), ptr(buf[:, e:]), (1 + c) * e, e
    buf = (img.contiguous(), sets.contiguous())
    return buf, ptr(buf[0]), ptr(buf[1]), e, n * e


def bank_forward(img, sets, s):
    """ov_clip_loss_multi at b = N over the bank: (loss, terms [4 C, N])."""
    lib = _lib.load()
    c, n, e = sets.shape
    img, txt = img.contiguous(), sets.reshape(c * n, e).contiguous()
    nb = lib.ov_clip_loss_multi_workspace_bytes(n, n, c)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)
    loss, terms, sc = torch.empty(1, device=DEV), torch.empty(4 * c, n, device=DEV), scalar(s)
    check(lib.ov_clip_loss_multi(ptr(img), ptr(txt), ptr(img), ptr(txt), e, n * e, n, n, e, c, ptr(sc), 0, ptr(loss), ptr(terms), ptr(ws),
                                 nb, stream_ptr()), "ov_clip_loss_multi")
    return loss[0], terms


def run_window(img, sets, s, terms, w0, b, norm_rows, packed=True, grad=1.0, want_scale=True):
    """ov_clip_loss_window_backward over the bank: (d_img [b, E], d_txt [C b, E], d_scale 0-d | None).  The outputs start as NaN."""
    lib = _lib.load()
    c, n, e = sets.shape
    keep, p_ai, p_at, ld, ss = bank_operands(img, sets, packed)
    sc, gr = scalar(s), scalar(grad)
    d_img = torch.full((b, e), float("nan"), device=DEV)
    d_txt = torch.full((c * b, e), float("nan"), device=DEV)
    d_s = torch.full((1,), float("nan"), device=DEV)
    nb = lib.ov_clip_loss_window_backward_workspace_bytes(b, n, c)
    assert nb > 0
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)
    check(lib.ov_clip_loss_window_backward(p_ai, p_at, ld, ss, n, e, c, ptr(sc), ptr(terms), ptr(gr), w0, b, norm_rows, ptr(d_img),
                                           ptr(d_txt), ptr(d_s) if want_scale else None, ptr(ws), nb, stream_ptr()),
          "ov_clip_loss_window_backward")
    torch.cuda.synchronize()
    return d_img, d_txt, d_s[0] if want_scale else None


def close(got, ref, rel, what):
    """test_gpu_multicap.close: to ``rel`` of the reference's largest entry."""
    got, ref = got.double().cpu(), torch.as_tensor(ref).double().cpu()
    err, mag = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max |err| {err:.3e} at max |ref| {mag:.3e}")
    assert got.shape == ref.shape and err <= rel * mag, (what, err, mag)


def allclose(got, ref, what):
    """test_gpu_multicap's gradient tolerance against float64."""
    got, ref = got.double().cpu().numpy(), torch.as_tensor(ref).double().cpu().numpy()
    print(f"{what}: max |err| {np.abs(got - ref).max():.3e} at max |ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-6, err_msg=str(what))


def scale_close(got, ref, what):
    got, ref = float(got), float(ref)
    print(f"{what}: d_scale {got:.6e} reference {ref:.6e}")
    assert abs(got - ref) < 2e-6 + 2e-4 * abs(ref), (what, got, ref)


# ---- 1. the kernel against the reference's fixture -------------------------------------------------------------------------------
GWG = [c for c in MR.CASES if c[0] in ("ws2_b16_e64_c3_local_gwg", "ws3_b13_e64_c1_local_gwg", "ws2_b13_e768_c2_local_gwg")]


@pytest.mark.parametrize("case", GWG, ids=[c[0] for c in GWG])
def test_kernel_against_the_reference_fixture(case):
    """local_loss + gather_with_grad at world size ws is the window scheme at norm_rows = b: rank r's window of the packed bank has
    the gradients the reference's ClipLoss gave that rank through its differentiable gather, to 1e-5 of the fixture's largest entry.
    A rank's d_scale share holds its image-side strips only, so the shares are compared where they must agree: their mean over the
    ranks is the mean of the fixture's per-rank logit_scale gradients (1e-5 relative)."""
    z = golden("multicap_grad.npz")
    name, ws, b, e, c, _, _, s, seed = case
    assert len(GWG) == 3
    img64, sets64 = MR.case_inputs(ws, b, e, c, seed)
    assert abs(float(img64.sum()) - float(z[f"{name}_img_sum"])) <= 1e-9 * float(z[f"{name}_img_abs_sum"])
    img, sets = img64.float().to(DEV), sets64.float().to(DEV)
    _, terms = bank_forward(img, sets, s)
    shares = []
    for r in range(ws):
        d_img, d_txt, d_s = run_window(img, sets, s, terms, r * b, b, b, packed=True)
        close(d_img, z[f"{name}_dimg"][r], 1e-5, (name, r, "dimg"))
        close(d_txt, z[f"{name}_dtxt"][r], 1e-5, (name, r, "dtxt"))
        shares.append(float(d_s))
    want = float(z[f"{name}_dscale"].astype("float64").mean())
    print(f"{name}: mean share {sum(shares) / ws:.8e} mean of the fixture's d_scale {want:.8e}")
    assert abs(sum(shares) / ws - want) <= 1e-5 * abs(want), (name, shares, want)


# ---- 2. the kernel against float64 ---------------------------------------------------------------------------------------------------
# b, N, E, C, w0
SHAPES = [(13, 39, 64, 2, 13),           # ragged tile, two waves own no e-tile
          (45, 135, 96, 3, 90),          # last window, e-tiles not a multiple of 4
          (32, 32, 1152, 1, 0),          # the window is the bank; the width limit
          (50, 150, 192, 2, 37),         # start off a tile boundary, the label diagonal crosses tiles
          (40, 131, 64, 4, 91),          # N % 32 != 0, the window ends at N, C at its limit
          (256, 2048, 768, 2, 512)]      # the workload's proportions


@pytest.mark.parametrize("b,N,E,C,w0", SHAPES, ids=[f"b{s[0]}_n{s[1]}_e{s[2]}_c{s[3]}_w{s[4]}" for s in SHAPES])
def test_kernel_against_float64_restatement(b, N, E, C, w0):
    """Gradients at rtol 2e-4, atol 1e-6 and d_scale within 2e-6 + 2e-4 |ref| of the float64 closed form evaluated on the device on
    the kernel's own terms' float64 counterpart; upstream gradient 0.5.  Then: two calls are bitwise equal, packed and separate bank
    layouts are bitwise equal, d_scale = NULL leaves the other outputs bitwise the same, and norm_rows = 2 N halves every output."""
    img64, sets64 = MR.make_inputs(N, E, C, seed=2000 + b)
    img64, sets64 = img64.to(DEV), sets64.to(DEV)
    img, sets = img64.float(), sets64.float()
    _, terms = bank_forward(img, sets, S)
    d_img, d_txt, d_s = run_window(img, sets, S, terms, w0, b, N, packed=True, grad=0.5)
    r_img, r_txt, r_s, _ = WR.window(img64, sets64, S, w0, b, N, grad=0.5)
    allclose(d_img, r_img, "d_img")
    allclose(d_txt, r_txt, "d_txt")
    scale_close(d_s, r_s, "d_scale")
    again = run_window(img, sets, S, terms, w0, b, N, packed=True, grad=0.5)
    assert all(torch.equal(x, y) for x, y in zip((d_img, d_txt, d_s), again)), "two calls differ"
    sep = run_window(img, sets, S, terms, w0, b, N, packed=False, grad=0.5)
    assert all(torch.equal(x, y) for x, y in zip((d_img, d_txt, d_s), sep)), "packed and separate layouts differ"
    nos = run_window(img, sets, S, terms, w0, b, N, packed=True, grad=0.5, want_scale=False)
    assert torch.equal(d_img, nos[0]) and torch.equal(d_txt, nos[1]) and nos[2] is None
    half = run_window(img, sets, S, terms, w0, b, 2 * N, packed=True, grad=0.5)
    for x, h in zip((d_img, d_txt, d_s), half):
        assert bool(((h - 0.5 * x).abs() <= 2.0 ** -23 * (0.5 * x).abs()).all()), "norm_rows = 2 N is not half"


# ---- 3. against the existing backward on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,C,wb", [(24, 64, 1, 8), (26, 96, 2, 13)])
def test_windows_are_the_rows_of_the_existing_backward(N, E, C, wb):
    """ov_clip_loss_multi_backward at b = N gives the one-batch gradient as local + gathered side; windows of 8 (of 13) rows give its
    rows, and their d_scale shares sum to its d_scale."""
    lib = _lib.load()
    img64, sets64 = MR.make_inputs(N, E, C, seed=77 + N)
    img, sets = img64.float().to(DEV), sets64.float().to(DEV)
    loss, terms = bank_forward(img, sets, S)
    txt = sets.reshape(C * N, E).contiguous()
    d_loc, d_gat = torch.empty((1 + C) * N, E, device=DEV), torch.empty((1 + C) * N, E, device=DEV)
    d_s, sc = torch.empty(1, device=DEV), scalar(S)
    nb = lib.ov_clip_loss_multi_backward_workspace_bytes(N, N, C)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)
    check(lib.ov_clip_loss_multi_backward(ptr(img), ptr(txt), ptr(img), ptr(txt), E, N * E, N, N, E, C, ptr(sc), 0, ptr(terms), None,
                                          ptr(d_loc), ptr(d_loc[N:]), ptr(d_gat), ptr(d_gat[N:]), E, N * E, ptr(d_s), ptr(ws), nb,
                                          stream_ptr()), "ov_clip_loss_multi_backward")
    full = d_loc + d_gat
    g_img, g_txt = full[:N], full[N:].view(C, N, E)
    assert N % wb == 0
    total = 0.0
    for w0 in range(0, N, wb):
        d_img, d_txt, share = run_window(img, sets, S, terms, w0, wb, N, packed=(w0 // wb) % 2 == 0)
        allclose(d_img, g_img[w0:w0 + wb], ("d_img", wb, w0))
        allclose(d_txt, g_txt[:, w0:w0 + wb].reshape(C * wb, E), ("d_txt", wb, w0))
        total += float(share)
    scale_close(total, d_s[0], ("d_scale", wb))


# ---- 4. the module in a world of one ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
def test_accumulator_world_of_one(C):
    a, b, e = 3, 8, 64
    n = a * b
    img64, sets64 = MR.make_inputs(n, e, C, seed=31 + C)
    mod = ClipLoss() if C == 1 else MultiCaptionClipLoss(2)
    imgs = [img64[j * b:(j + 1) * b].float().to(DEV).requires_grad_(True) for j in range(a)]
    txts = [WR.stack_window(sets64, j * b, b).float().to(DEV).requires_grad_(True) for j in range(a)]
    sc = torch.tensor(S, device=DEV, requires_grad=True)
    acc = ContrastiveAccumulator(mod)
    assert [acc.add(i, t) for i, t in zip(imgs, txts)] == [0, 1, 2]
    closed = acc.close(sc)
    assert not closed.requires_grad and acc.terms.shape == (4 * C, n)
    parts = [acc.window_loss(j, imgs[j], txts[j], sc, check=True) for j in range(a)]
    total = sum(parts)
    total.backward()
    # the one-batch module on the 24 rows, and float64
    f_img = img64.float().to(DEV).requires_grad_(True)
    f_txt = sets64.reshape(C * n, e).float().to(DEV).requires_grad_(True)
    f_sc = torch.tensor(S, device=DEV, requires_grad=True)
    ref = mod(f_img, f_txt, f_sc)
    ref.backward()
    (w_loss, w_img, w_txt, w_s), = MR.per_rank(img64, sets64, S, 1, True, False)
    print(f"C = {C}: accumulated {float(total.detach()):.7f} closed {float(closed):.7f} one batch {float(ref.detach()):.7f} float64 {float(w_loss):.7f}")
    got, one = float(total.detach()), float(ref.detach())
    assert abs(got - one) < 2e-5 and abs(float(closed) - one) < 2e-5 and abs(got - float(w_loss)) < 2e-5
    w_txt = w_txt.view(C, n, e)
    for j in range(a):
        allclose(imgs[j].grad, w_img[j * b:(j + 1) * b], ("d_img", j))
        allclose(txts[j].grad, w_txt[:, j * b:(j + 1) * b].reshape(C * b, e), ("d_txt", j))
    allclose(torch.cat([x.grad for x in imgs]), f_img.grad, "d_img against the one-batch module")
    scale_close(sc.grad, w_s, "d logit_scale")
    scale_close(sc.grad, f_sc.grad, "d logit_scale against the one-batch module")
    # check=True: one perturbed element is refused
    bad = imgs[1].detach().clone()
    bad[3, 5] = torch.nextafter(bad[3, 5], bad[3, 5] + 1)
    with pytest.raises(_lib.OvhipError):
        acc.window_loss(1, bad, txts[1], sc, check=True)
    acc.window_loss(1, bad, txts[1], sc)                              # the default looks at nothing
    acc.reset()
    assert acc.add(imgs[0], txts[0]) == 0


# ---- 5. / 6. the Tiny model ------------------------------------------------------------------------------------------------------------
CFG = preset("vit-tiny-patch16-160")
A_TINY, B_TINY = 3, 4


def tiny_model(cfg=CFG):
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(CFG))
    for p in m.parameters():
        p.requires_grad_(True)
    return m


def tiny_batches():
    img, tok = synth.make_images(12, 160, seed=21).to(DEV), synth.make_captions(12, seed=21).to(DEV)
    return img, tok, [(img[j * B_TINY:(j + 1) * B_TINY], tok[j * B_TINY:(j + 1) * B_TINY]) for j in range(A_TINY)]


def grads_of(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def tiny_step():
    """One accumulated step of 3 x 4 pairs with check=True: (loss, gradients by name).  Shared, never modified."""
    m = tiny_model()
    loss = training.accumulated_step(m, tiny_batches()[2], ClipLoss(), check=True)
    torch.cuda.synchronize()
    return float(loss), grads_of(m)


def test_accumulated_step_against_the_oracle(tiny_step):
    """test_training_step_gradients_tiny's criterion for the accumulated step of the same kind of batch, 12 pairs as 3 x 4: cosine
    > 0.99 and norm within 5 % for every parameter whose reference gradient is not negligible, more than 100 tensors, loss within
    2e-2; and the logit_scale gradient within 5 % (a scheme that adds the full gradient per window would be 3 x off)."""
    from oracle import clip_ref as R
    loss, got = tiny_step
    sd = synth.make_state_dict(CFG)
    img, tok = synth.make_images(12, 160, seed=21), synth.make_captions(12, seed=21)
    sdg = {k: v.clone().float().requires_grad_(True) for k, v in sd.items()}
    fi, ft, sc = R.clip_forward(img, tok, sdg, CFG)
    ref_loss = R.clip_loss(fi, ft, sc)
    ref_loss.backward()
    print(f"accumulated loss {loss:.6f} oracle {float(ref_loss.detach()):.6f}")
    assert abs(loss - float(ref_loss.detach())) < 2e-2
    ref_scale = max(float(v.grad.norm()) for v in sdg.values() if v.grad is not None)
    checked = 0
    for name, ref in sdg.items():
        if ref.grad is None or name not in got:
            continue
        g, r = got[name].float().cpu(), ref.grad
        rn = float(r.norm())
        if rn < 1e-3 * ref_scale:
            continue
        cos = float((g * r).sum() / (g.norm() * r.norm() + 1e-30))
        assert cos > 0.99, (name, cos)
        assert abs(float(g.norm()) - rn) < 0.05 * rn, (name, float(g.norm()), rn)
        checked += 1
    assert checked > 100
    gs, rs = float(got["logit_scale"]), float(sdg["logit_scale"].grad)
    print(f"d logit_scale: accumulated {gs:.6e} oracle {rs:.6e}")
    assert abs(gs - rs) < 0.05 * abs(rs)
    # not asserted: the accumulated gradients against the ordinary one-batch step of the same 12 pairs
    m = tiny_model()
    full_img, full_tok, _ = tiny_batches()
    ClipLoss()(*training.clip_forward(m, full_img, full_tok)).backward()
    one = grads_of(m)
    dot = sum(float((got[n].double() * one[n].double()).sum()) for n in one)
    na, nb = (sum(float(g[n].double().pow(2).sum()) for n in one) ** 0.5 for g in (got, one))
    print(f"accumulated 3 x 4 against the one-batch step of 12: cosine over all parameters {dot / (na * nb):.8f}, "
          f"norm ratio {na / nb:.6f}")


def test_accumulated_step_under_recomputation_is_bitwise(tiny_step):
    m = tiny_model()
    m.set_grad_checkpointing()
    loss = training.accumulated_step(m, tiny_batches()[2], ClipLoss(), check=True)
    got = grads_of(m)
    assert float(loss) == tiny_step[0] and got.keys() == tiny_step[1].keys()
    for n, g in tiny_step[1].items():
        assert torch.equal(got[n], g), n


def test_accumulated_step_with_a_locked_image_tower(tiny_step):
    m = tiny_model()
    m.lock_image_tower(0)
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen and all(n.startswith("visual.") for n in frozen)
    loss = training.accumulated_step(m, tiny_batches()[2], ClipLoss(), check=True)
    assert float(loss) == tiny_step[0]
    got = grads_of(m)
    assert not frozen & got.keys()
    rest = [n for n in tiny_step[1] if n not in frozen]
    assert len(rest) > 50 and "logit_scale" in rest
    for n in rest:
        assert torch.equal(got[n], tiny_step[1][n]), n


def test_accumulated_step_under_patch_dropout_uses_one_draw_for_both_passes():
    """check=True demands pass 2's features bitwise equal to pass 1's: with half the patches dropped at random that holds only if
    both passes saw the same draw."""
    cfg = dict(CFG, vision_cfg=dict(CFG["vision_cfg"], patch_dropout=0.5))
    m = tiny_model(cfg)
    m.train()
    assert m.visual.dropout_active()
    torch.manual_seed(5)
    loss = training.accumulated_step(m, tiny_batches()[2], ClipLoss(), check=True)
    got = grads_of(m)
    assert bool(torch.isfinite(loss)) and len(got) > 100 and all(bool(torch.isfinite(g).all()) for g in got.values())
    m.eval()
    full = training.accumulated_step(tiny_model(), tiny_batches()[2], ClipLoss())
    assert float(loss) != float(full)                                 # the dropout did act


def test_accumulated_step_with_the_caption_branch(monkeypatch):
    """A = 2 x b = 3 with the tiny decoder: finite loss, decoder gradients present, and the features' gradients (they come from the
    contrastive side alone) are the float64 window gradients of the bank at test 4's tolerances."""
    from openvision_amd.caption import TextDecoder
    a, b = 2, 3
    m = tiny_model()
    torch.manual_seed(3)
    dec = TextDecoder(m.visual.transformer.width, m.transformer.width, 192, 2, 3, 768, m.token_embedding.weight.shape[0],
                      num_learnable_tokens=128).to(DEV)
    img = synth.make_images(a * b, 160, seed=51).to(DEV)
    t1, t2 = synth.make_captions(a * b, seed=51).to(DEV), synth.make_captions(a * b, seed=52).to(DEV)
    batches = [(img[j * b:(j + 1) * b], torch.cat([t1[j * b:(j + 1) * b], t2[j * b:(j + 1) * b]])) for j in range(a)]
    g = torch.Generator().manual_seed(1)
    targets = [(torch.randint(0, dec.vocab_size, (b, 128), generator=g).to(DEV), (torch.rand(b, 128, generator=g) < 0.8).float().to(DEV))
               for _ in range(a)]
    seen = []
    inner = ContrastiveAccumulator.window_loss

    def spy(self, j, image_features, text_features, logit_scale, check=False):
        image_features.retain_grad()
        text_features.retain_grad()
        seen.append((self, j, image_features, text_features))
        return inner(self, j, image_features, text_features, logit_scale, check=check)

    monkeypatch.setattr(ContrastiveAccumulator, "window_loss", spy)
    loss = training.accumulated_step(m, batches, MultiCaptionClipLoss(2), decoder=dec, caption_targets=targets, check=True)
    assert bool(torch.isfinite(loss)) and len(seen) == a
    dgrads = [p.grad for p in dec.parameters()]
    assert all(gr is not None and bool(torch.isfinite(gr).all()) for gr in dgrads) and any(float(gr.abs().sum()) > 0 for gr in dgrads)
    # float64 on the bank the accumulator holds
    e = seen[0][2].shape[1]
    img64 = torch.cat([s[2].detach() for s in seen]).double().cpu()
    sets64 = torch.stack([torch.cat([s[3].detach()[k * b:(k + 1) * b] for s in seen]) for k in range(2)]).double().cpu()
    s64 = float(m.logit_scale.detach().exp())
    contrastive = 0.0
    for acc, j, f_img, f_txt in seen:
        w_img, w_txt, _, w_loss = WR.window(img64, sets64, s64, j * b, b, a * b)
        allclose(f_img.grad, w_img, ("caption branch d_img", j))
        allclose(f_txt.grad, w_txt, ("caption branch d_txt", j))
        contrastive += float(w_loss)
    assert float(loss) > contrastive > 0 and e == 192                 # the caption terms were added


# ---- 7. a world of two on the one GPU -----------------------------------------------------------------------------------------------
WS, A2, B2, E2 = 2, 2, 20, 192


def _world2_inputs():
    return {1: MR.case_inputs(WS, A2 * B2, E2, 1, 15), 2: MR.case_inputs(WS, A2 * B2, E2, 2, 16)}


def _world2_rank(rank, ws):
    torch.cuda.set_device(0)
    out = {}
    for c, (img, sets) in _world2_inputs().items():
        kw = dict(local_loss=True, gather_with_grad=True, rank=rank, world_size=ws)
        acc = ContrastiveAccumulator(ClipLoss(**kw) if c == 1 else MultiCaptionClipLoss(2, **kw))
        rows = [(rank * A2 + j) * B2 for j in range(A2)]
        imgs = [img[w0:w0 + B2].float().to(DEV).requires_grad_(True) for w0 in rows]
        txts = [WR.stack_window(sets, w0, B2).float().to(DEV).requires_grad_(True) for w0 in rows]
        sc = torch.tensor(S, device=DEV, requires_grad=True)
        for i, t in zip(imgs, txts):
            acc.add(i, t)
        closed = acc.close(sc)
        assert acc.terms.shape == (4 * c, ws * A2 * B2) and [acc.layout.start(j) for j in range(A2)] == rows
        parts = [acc.window_loss(j, imgs[j], txts[j], sc, check=True) for j in range(A2)]
        sum(parts).backward()
        out[c] = (float(closed), [float(p.detach()) for p in parts], [x.grad.cpu().numpy() for x in imgs],
                  [x.grad.cpu().numpy() for x in txts], float(sc.grad))
    return out


def test_accumulator_at_world_size_2():
    """Two ranks over gloo on the one GPU, A = 2 windows of b = 20 each: every window against the float64 restatement at norm_rows =
    A b and w0 = (r A + j) b; each rank's loss is the mean over its own rows."""
    res = run_ranks(_world2_rank, WS, timeout=300, backend="gloo", gpu=True)
    rows = A2 * B2
    for c, (img, sets) in _world2_inputs().items():
        terms = WR.bank_terms(img, sets, S)
        for r in range(WS):
            closed, parts, g_img, g_txt, g_s = res[r][c]
            want_s = want_l = 0.0
            for j in range(A2):
                w_img, w_txt, w_s, w_l = WR.window(img, sets, S, (r * A2 + j) * B2, B2, rows, terms)
                allclose(torch.as_tensor(g_img[j]), w_img, (c, r, j, "d_img"))
                allclose(torch.as_tensor(g_txt[j]), w_txt, (c, r, j, "d_txt"))
                assert abs(parts[j] - float(w_l)) < 2e-5, (c, r, j)
                want_s, want_l = want_s + float(w_s), want_l + float(w_l)
            scale_close(g_s, want_s, (c, r, "d logit_scale"))
            own = MR.strip_loss(img[r * rows:(r + 1) * rows], MR.stack_local(sets, r, rows), img, sets, S, r, c)
            print(f"C = {c} rank {r}: loss {closed:.7f} mean over its own rows in float64 {float(own):.7f}")
            assert abs(closed - float(own)) < 2e-5 and abs(want_l - float(own)) < 1e-9
