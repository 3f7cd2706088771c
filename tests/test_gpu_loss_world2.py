"""GPU: the four loss modules (openvision_amd.loss) at a world size that really is above one -- two ranks over gloo on the one GPU,
CUDA tensors -- against the float64 restatements' per_rank (tests/multicap_restate.py, distill_restate.py, siglip_restate.py), in
every (local_loss, gather_with_grad) mode.  b = 40 rows per rank: every 32-row tile is ragged and rank 1's own chunk of the N = 80
gathered rows lies across a tile boundary.  Tolerances are each loss's own module tolerances (test_gpu_multicap.py,
test_gpu_distill.py, test_gpu_siglip.py); ClipLoss takes the multi-caption loss's."""
import time

import numpy as np
import pytest
import torch

import distill_restate as DR
import multicap_restate as MR
import siglip_restate as SR
from ranks import run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS, B, E, ET = 2, 40, 192, 96
MODES = [(True, False), (True, True), (False, False), (False, True)]          # (local_loss, gather_with_grad)
S_CLIP = 1 / 0.07                           # test_gpu_multicap._module_inputs
S_DISTILL, ST_DISTILL = 5.0, 15.0           # test_gpu_distill.MOD_S, MOD_ST
S_SIGLIP, BETA_SIGLIP = 10.0, -10.0         # test_gpu_siglip._nccl_ws1_rank


def _inputs():
    """The global float64 sets of every loss; rank r owns rows [r b, (r + 1) b)."""
    return {"clip": MR.case_inputs(WS, B, E, 1, 5), "multi": MR.case_inputs(WS, B, E, 2, 6),
            "distill": DR.case_inputs(WS, B, E, ET, 7), "siglip": SR.case_inputs(WS, B, E, 8)}


def _leaf(x):
    return x.float().to(DEV).requires_grad_(True)


def _world2_rank(rank, ws):
    """Every module once on this rank's rows: name -> (loss(es), d image_features, d text_features, d scale (, d bias))."""
    from openvision_amd.loss import ClipLoss, DistillClipLoss, MultiCaptionClipLoss, SigLipLoss
    torch.cuda.set_device(0)
    own, inputs, out = slice(rank * B, (rank + 1) * B), _inputs(), {}
    for local_loss, gwg in MODES:
        kw = dict(local_loss=local_loss, gather_with_grad=gwg, rank=rank, world_size=WS)
        for name, fn in (("clip", ClipLoss(**kw)), ("multi", MultiCaptionClipLoss(2, **kw))):
            img, sets = inputs[name]
            a, t, sc = _leaf(img[own]), _leaf(MR.stack_local(sets, rank, B)), torch.tensor(S_CLIP, device=DEV, requires_grad=True)
            loss = fn(a, t, sc)
            loss.backward()
            assert fn.last_terms.shape == (4 * sets.shape[0], B if local_loss else WS * B)
            out[(name, local_loss, gwg)] = (float(loss.detach()), a.grad.cpu().numpy(), t.grad.cpu().numpy(), float(sc.grad))
        img, txt, t_img, t_txt = inputs["distill"]
        a, t, sc = _leaf(img[own]), _leaf(txt[own]), torch.tensor(S_DISTILL, device=DEV, requires_grad=True)
        c, d = DistillClipLoss(**kw)(a, t, sc, t_img[own].float().to(DEV), t_txt[own].float().to(DEV), torch.tensor(ST_DISTILL, device=DEV))
        (c + d).backward()
        out[("distill", local_loss, gwg)] = (float(c.detach()), float(d.detach()), a.grad.cpu().numpy(), t.grad.cpu().numpy(), float(sc.grad))
    img, txt = inputs["siglip"]
    a, t = _leaf(img[own]), _leaf(txt[own])
    sc, bi = torch.tensor(S_SIGLIP, device=DEV, requires_grad=True), torch.tensor(BETA_SIGLIP, device=DEV, requires_grad=True)
    loss = SigLipLoss(rank=rank, world_size=WS)(a, t, sc, bi)
    loss.backward()
    out["siglip"] = (float(loss.detach()), a.grad.cpu().numpy(), t.grad.cpu().numpy(), float(sc.grad), float(bi.grad))
    return out


@pytest.fixture(scope="module")
def world2():
    """One spawned pair of ranks runs every case; a rank that dies or raises fails the tests at once, nothing is retried."""
    t0 = time.monotonic()
    res = run_ranks(_world2_rank, WS, timeout=300, backend="gloo", gpu=True)
    print(f"two ranks, {3 * len(MODES) + 1} module runs each: {time.monotonic() - t0:.1f} s")
    return res, _inputs()


def _close(got, ref, rel, what):
    """test_gpu_distill.close / test_gpu_siglip.close: to ``rel`` of the reference's largest entry."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    err, mag = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max |err| {err:.3e} at max |ref| {mag:.3e} (ratio to the bound {err / (rel * mag):.3f})")
    assert got.shape == ref.shape and err <= rel * mag, (what, err, mag, rel)


@pytest.mark.parametrize("local_loss,gwg", MODES)
@pytest.mark.parametrize("name", ["clip", "multi"])
def test_infonce_modules_at_world_size_2(world2, name, local_loss, gwg):
    """ClipLoss (one set) and MultiCaptionClipLoss(2) at test_gpu_multicap._module_check's tolerances."""
    res, inputs = world2
    img, sets = inputs[name]
    want = MR.per_rank(img, sets, S_CLIP, WS, local_loss, gwg)
    for r in range(WS):
        what = (name, local_loss, gwg, r)
        loss, g_img, g_txt, g_s = res[r][(name, local_loss, gwg)]
        w_loss, w_img, w_txt, w_s = want[r]
        print(f"{what}: loss {loss:.7f} float64 {float(w_loss):.7f}; d_scale {g_s:.6e} float64 {float(w_s):.6e}; "
              f"max |err| d_img {np.abs(g_img - w_img.numpy()).max():.3e} d_txt {np.abs(g_txt - w_txt.numpy()).max():.3e}")
        assert abs(loss - float(w_loss)) < 2e-5, what
        np.testing.assert_allclose(g_img, w_img.numpy(), rtol=2e-4, atol=1e-6, err_msg=str(what))
        np.testing.assert_allclose(g_txt, w_txt.numpy(), rtol=2e-4, atol=1e-6, err_msg=str(what))
        assert abs(g_s - float(w_s)) < 2e-6 + 2e-4 * abs(float(w_s)), what


@pytest.mark.parametrize("local_loss,gwg", MODES)
def test_distill_module_at_world_size_2(world2, local_loss, gwg):
    """DistillClipLoss with loss = c + d at test_gpu_distill._module_check's tolerances."""
    res, inputs = world2
    want = DR.per_rank(inputs["distill"], S_DISTILL, ST_DISTILL, WS, local_loss, gwg, 1.0, 1.0)
    for r in range(WS):
        what = ("distill", local_loss, gwg, r)
        c, d, g_img, g_txt, g_s = res[r][("distill", local_loss, gwg)]
        w_c, w_d, w_img, w_txt, w_s = want[r]
        print(f"{what}: contrastive {c:.7f} float64 {float(w_c):.7f}; distill {d:.7f} float64 {float(w_d):.7f}; "
              f"d_scale {g_s:.6e} float64 {float(w_s):.6e}")
        assert abs(c - float(w_c)) <= 1e-5 * float(w_c) and abs(d - float(w_d)) <= 1e-5 * float(w_d), what
        _close(g_img, w_img, 1e-5, what + ("d_img",))
        _close(g_txt, w_txt, 1e-5, what + ("d_txt",))
        assert abs(g_s - float(w_s)) <= 1e-5 * abs(float(w_s)), (what, g_s, float(w_s))


def test_siglip_module_at_world_size_2(world2):
    """SigLipLoss with a bias at test_gpu_siglip's module tolerances: the text gradient is the gathered side summed over ranks."""
    res, inputs = world2
    img, txt = inputs["siglip"]
    want = SR.per_rank(img, txt, S_SIGLIP, BETA_SIGLIP, WS)
    for r in range(WS):
        loss, g_img, g_txt, g_s, g_b = res[r]["siglip"]
        w_loss, w_img, w_txt, w_s, w_b = want[r]
        print(f"siglip rank {r}: loss {loss:.7f} float64 {float(w_loss):.7f}")
        assert abs(loss - float(w_loss)) <= 1e-5 * abs(float(w_loss)), r
        _close(g_img, w_img, 1e-5, ("siglip", r, "d_img"))
        _close(g_txt, w_txt, 1e-5, ("siglip", r, "d_txt"))
        _close([g_s], [float(w_s)], 1e-5, ("siglip", r, "d_scale"))
        _close([g_b], [float(w_b)], 1e-5, ("siglip", r, "d_bias"))
