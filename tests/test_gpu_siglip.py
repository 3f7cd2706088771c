"""GPU: the fused SigLIP loss (csrc/siglip.hip behind openvision_amd.loss.SigLipLoss) against the reference's SigLipLoss
(tests/golden/siglip_grad.npz, made over gloo in float64) and the float64 restatement (tests/siglip_restate.py), and the SigLIP
training path: CLIP's logit_bias through training.clip_forward, FusedAdamW and two data-parallel ranks."""
import math

import numpy as np
import pytest
import torch

from openvision_amd import _lib, preset, synth
from openvision_amd._lib import check, ptr, stream_ptr
from openvision_amd.loss import SigLipLoss
from openvision_amd.model import create_model

import siglip_restate as SR
from conftest import golden
from ranks import run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def kernel_loss(x, y, s, beta, off):
    lib = _lib.load()
    b, e = x.shape
    n = y.shape[0]
    nb = lib.ov_siglip_loss_workspace_bytes(b, n)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)
    out = torch.empty(1, dtype=torch.float32, device=DEV)
    sc = torch.full((1,), float(s), dtype=torch.float32, device=DEV)
    bi = torch.full((1,), float(beta), dtype=torch.float32, device=DEV) if beta is not None else None
    check(lib.ov_siglip_loss(ptr(x), ptr(y), b, n, e, ptr(sc), ptr(bi), off, ptr(out), ptr(ws), nb, stream_ptr()), "ov_siglip_loss")
    return out[0]


def kernel_backward(x, y, s, beta, off, grad=1.0, gathered=True):
    """(d_x, d_y | None, d_s, d_beta) of ov_siglip_loss_backward."""
    lib = _lib.load()
    b, e = x.shape
    n = y.shape[0]
    dx = torch.empty_like(x)
    dy = torch.empty_like(y) if gathered else None
    dsb = torch.empty(2, dtype=torch.float32, device=DEV)
    nb = lib.ov_siglip_loss_backward_workspace_bytes(b, n)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)
    sc = torch.full((1,), float(s), dtype=torch.float32, device=DEV)
    bi = torch.full((1,), float(beta), dtype=torch.float32, device=DEV) if beta is not None else None
    gr = torch.full((1,), float(grad), dtype=torch.float32, device=DEV)
    check(lib.ov_siglip_loss_backward(ptr(x), ptr(y), b, n, e, ptr(sc), ptr(bi), off, ptr(gr), ptr(dx), ptr(dy), ptr(dsb[0:]),
                                      ptr(dsb[1:]) if beta is not None else None, ptr(ws), nb, stream_ptr()), "ov_siglip_loss_backward")
    return dx, dy, dsb[0], dsb[1]


def close(got, ref, rel, what):
    got, ref = got.double().cpu(), torch.as_tensor(ref).double()
    err, mag = float((got - ref).abs().max()), float(ref.abs().max())
    assert err <= rel * mag, (what, err, mag)


@pytest.mark.parametrize("case", SR.CASES, ids=[c[0] for c in SR.CASES])
def test_kernel_against_the_reference_fixture(case):
    """One process plays every rank r: its image rows, the gathered text set, label offset b r.  d_y is summed over the ranks and
    each rank keeps its own chunk, as the reduce-scatter does.  Loss to 1e-5 relative; gradients to 1e-5 of their largest entry."""
    z = golden("siglip_grad.npz")
    name, ws, b, e, s, beta, bidir, seed = case
    img, txt = SR.case_inputs(ws, b, e, seed)
    assert abs(float(img.sum()) - float(z[f"{name}_img_sum"])) <= 1e-9 * float(z[f"{name}_img_abs_sum"])
    x_all, y = img.float().to(DEV), txt.float().to(DEV)
    d_y = torch.zeros_like(y)
    per = []
    for r in range(ws):
        x = x_all[r * b:(r + 1) * b].contiguous()
        loss = kernel_loss(x, y, s, beta, b * r)
        dx, dy, ds, db = kernel_backward(x, y, s, beta, b * r)
        d_y += dy
        per.append((loss, dx, ds, db))
    for r, (loss, dx, ds, db) in enumerate(per):
        ref = float(z[f"{name}_loss"][r])
        assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (name, r, float(loss), ref)
        close(dx, z[f"{name}_dimg"][r], 1e-5, (name, r, "dimg"))
        close(d_y[r * b:(r + 1) * b], z[f"{name}_dtxt"][r], 1e-5, (name, r, "dtxt"))
        close(ds.reshape(1), [float(z[f"{name}_dscale"][r])], 1e-5, (name, r, "dscale"))
        close(db.reshape(1), [float(z[f"{name}_dbias"][r])], 1e-5, (name, r, "dbias"))


def _large_inputs():
    g = torch.Generator().manual_seed(17)
    n, e = 3000, 768
    y = torch.nn.functional.normalize(torch.randn(n, e, generator=g), dim=-1)
    x = torch.nn.functional.normalize(y[1000:2000] + torch.randn(1000, e, generator=g) * 0.03, dim=-1)
    return x.to(DEV), y.to(DEV)


def test_large_ragged_shape_against_float64_and_repeatable():
    """b = 1000 (ragged against the 32-row tiles), N = 3000, E = 768, rank 1 of 3 (label offset 1000): loss and every gradient
    against the float64 restatement on the device, with and without the bias; two calls are bitwise equal."""
    x, y = _large_inputs()
    for s, beta in ((10.0, -10.0), (112.0, -16.5), (10.0, None)):
        loss = kernel_loss(x, y, s, beta, 1000)
        dx, dy, ds, db = kernel_backward(x, y, s, beta, 1000, grad=0.75)
        x64, y64 = x.double(), y.double()
        rl = SR.strip_loss(x64, y64, s, beta, 1)
        rdx, rdy, rds, rdb = SR.strip_grads(x64, y64, s, beta, 1, grad=0.75)
        assert abs(float(loss) - float(rl)) <= 1e-5 * abs(float(rl)), (s, beta, float(loss), float(rl))
        close(dx, rdx.cpu(), 3e-5, ("dx", s, beta))              # 3000-term fp32 chains per output entry
        close(dy, rdy.cpu(), 3e-5, ("dy", s, beta))
        close(ds.reshape(1), [float(rds)], 1e-5, ("ds", s, beta))
        if beta is not None:
            close(db.reshape(1), [float(rdb)], 1e-5, ("dbias", s, beta))
        l2 = kernel_loss(x, y, s, beta, 1000)
        dx2, dy2, ds2, db2 = kernel_backward(x, y, s, beta, 1000, grad=0.75)
        assert torch.equal(loss, l2) and torch.equal(dx, dx2) and torch.equal(dy, dy2) and torch.equal(ds, ds2)
        if beta is not None:
            assert torch.equal(db, db2)
    # the local side alone (d_y skipped) is bitwise the same d_x
    dx3, none, _, _ = kernel_backward(x, y, 10.0, -10.0, 1000, grad=0.75, gathered=False)
    dx4, _, _, _ = kernel_backward(x, y, 10.0, -10.0, 1000, grad=0.75)
    assert none is None and torch.equal(dx3, dx4)


def test_siglip_loss_module_world_size_1():
    """SigLipLoss end to end at world size 1: the autograd node (text gradient = the gathered side, counted once), the plain
    launch under no_grad, output_dict, and logit_bias=None."""
    g = torch.Generator().manual_seed(23)
    img = torch.nn.functional.normalize(torch.randn(40, 64, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(img + torch.randn(40, 64, generator=g) * 0.1, dim=-1)
    for beta in (-10.0, None):
        a, t = img.to(DEV).requires_grad_(True), txt.to(DEV).requires_grad_(True)
        s = torch.tensor(10.0, device=DEV, requires_grad=True)
        bi = torch.tensor(beta, device=DEV, requires_grad=True) if beta is not None else None
        out = SigLipLoss()(a, t, s, bi, output_dict=True)
        assert set(out) == {"contrastive_loss"}
        out["contrastive_loss"].backward()
        with torch.no_grad():
            plain = SigLipLoss()(a, t, s, bi)
        assert torch.equal(plain, out["contrastive_loss"].detach())
        i64, t64 = img.double(), txt.double()
        rl = SR.strip_loss(i64, t64, 10.0, beta, 0)
        rdi, rdt, rds, rdb = SR.strip_grads(i64, t64, 10.0, beta, 0)
        assert abs(float(plain) - float(rl)) <= 1e-5 * abs(float(rl))
        close(a.grad, rdi, 1e-5, "d image")
        close(t.grad, rdt, 1e-5, "d text")
        close(s.grad.reshape(1), [float(rds)], 1e-5, "d scale")
        if beta is not None:
            close(bi.grad.reshape(1), [float(rdb)], 1e-5, "d bias")


def _nccl_ws1_rank(rank, ws):
    g = torch.Generator().manual_seed(5)
    img = torch.nn.functional.normalize(torch.randn(24, 192, generator=g), dim=-1).to(DEV)
    txt = torch.nn.functional.normalize(img.cpu() + torch.randn(24, 192, generator=g) * 0.1, dim=-1).to(DEV)
    out = {}
    for name, coll in (("plain", False), ("coll", True)):
        a, b, c = img.clone().requires_grad_(True), txt.clone().requires_grad_(True), torch.tensor(10.0, device=DEV, requires_grad=True)
        d = torch.tensor(-10.0, device=DEV, requires_grad=True)
        fn = SigLipLoss(rank=0, world_size=1)
        fn.always_collective = coll                          # all_gather_into_tensor + reduce_scatter_tensor at world 1
        loss = fn(a, b, c, d)
        loss.backward()
        out[name] = (float(loss.detach()), a.grad.cpu().numpy(), b.grad.cpu().numpy(), float(c.grad), float(d.grad))
    return out


def test_rccl_branch_of_siglip_loss_at_world_size_1():
    """The RCCL code path of SigLipLoss (text all-gather, reduce-scatter of the gathered-side gradient) in a world of one rank:
    loss and every gradient equal the plain single-process call."""
    out, = run_ranks(_nccl_ws1_rank, 1, timeout=600, backend="nccl", gpu=True)
    l0, gi0, gt0, gs0, gb0 = out["plain"]
    l, gi, gt, gs, gb = out["coll"]
    assert l == l0 and gs == gs0 and gb == gb0
    assert np.array_equal(gi, gi0) and np.array_equal(gt, gt0)


def _siglip_cfg_sd():
    cfg = {**preset("vit-tiny-patch16-160"), "init_logit_bias": -10.0, "init_logit_scale": math.log(10.0)}
    sd = synth.make_state_dict(preset("vit-tiny-patch16-160"))
    sd["logit_scale"] = torch.tensor(math.log(10.0))
    sd["logit_bias"] = torch.tensor(-10.0)
    return cfg, sd


def test_siglip_training_step_gradients_tiny():
    """One SigLIP training step on the Tiny model (training.clip_forward's 4-tuple + SigLipLoss + backward) against torch autograd
    through the oracle's fp32 towers and the restated loss on the CPU, with the criteria of test_training_step_gradients_tiny:
    cosine >= 0.99 and norm within 5 % for every non-negligible parameter gradient, logit_scale and logit_bias included.  Then
    eight FusedAdamW steps (logit_bias not decayed) lower the loss; get_logits adds the bias."""
    from oracle import clip_ref as R
    from openvision_amd import training
    from openvision_amd.model import logits
    cfg, sd = _siglip_cfg_sd()
    img, tok = synth.make_images(6, 160, seed=21), synth.make_captions(6, seed=21)
    sdg = {k: v.clone().float().requires_grad_(True) for k, v in sd.items()}
    fi, ft, sc = R.clip_forward(img, tok, sdg, cfg)
    ref_loss = SR.strip_loss(fi, ft, sc, sdg["logit_bias"], 0)
    ref_loss.backward()
    m = create_model(cfg, device=DEV, state_dict=sd)
    for p in m.parameters():
        p.requires_grad_(True)
    out = training.clip_forward(m, img.to(DEV), tok.to(DEV))
    assert len(out) == 4 and out[3] is m.logit_bias
    loss = SigLipLoss()(*out)
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < 2e-2 * max(1.0, abs(float(ref_loss.detach())))
    loss.backward()
    got = dict(m.named_parameters())
    ref_scale = max(float(v.grad.norm()) for v in sdg.values() if v.grad is not None)
    checked = 0
    for name, ref in sdg.items():
        if ref.grad is None:
            continue
        g, r = got[name].grad, ref.grad
        assert g is not None, name
        g = g.float().cpu()
        rn = float(r.norm())
        if rn < 1e-3 * ref_scale and name not in ("logit_scale", "logit_bias"):
            continue
        cos = float((g * r).sum() / (g.norm() * r.norm() + 1e-30))
        assert cos > 0.99, (name, cos)
        assert abs(float(g.norm()) - rn) < 0.05 * rn, (name, float(g.norm()), rn)
        checked += 1
    assert checked > 100 and got["logit_bias"].grad is not None
    # get_logits: scale * img @ txt^T + bias, on the device
    with torch.no_grad():
        li, lt = m.get_logits(img.to(DEV), tok.to(DEV))
        want = logits(m.encode_image(img.to(DEV), True), m.encode_text(tok.to(DEV), True), m.logit_scale.exp()) + m.logit_bias
    assert torch.allclose(li, want) and torch.equal(lt, li.T)
    # eight FusedAdamW steps on the fixed batch
    opt = training.FusedAdamW(m, lr=2e-3)
    assert any(n == "logit_bias" for g in opt.groups if g["wd"] == 0.0 for n, _ in g["params"])
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = SigLipLoss()(*training.clip_forward(m, img.to(DEV), tok.to(DEV)))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses
    assert max(losses[2:]) < losses[0], losses
    assert float(m.logit_bias.detach()) != -10.0


def _ddp_rank(rank, ws):
    import torch.distributed as dist
    from openvision_amd import training
    cfg, sd = _siglip_cfg_sd()
    m = create_model(cfg, device=DEV, state_dict=sd)
    img, tok = synth.make_images(8, 160, seed=41), synth.make_captions(8, seed=41)
    b = 8 // ws
    li, lt = img[rank * b:(rank + 1) * b].to(DEV), tok[rank * b:(rank + 1) * b].to(DEV)
    loss = SigLipLoss(rank=rank, world_size=ws)(*training.clip_forward(m, li, lt))
    loss.backward()
    out = {}
    for name, p in m.named_parameters():                      # what DistributedDataParallel does: average the ranks' gradients
        g = p.grad.detach().float().cpu()
        dist.all_reduce(g)
        out[name] = g / ws
    lt_ = loss.detach().float().cpu()
    dist.all_reduce(lt_)
    return rank, float(lt_ / ws), {k: v.numpy() for k, v in out.items()} if rank == 0 else None


def test_data_parallel_siglip_matches_single_process():
    """Two ranks (gloo, one GPU) on half batches, gradients averaged as DDP does, against one process on the whole batch: the
    mean of the ranks' losses is the whole-batch loss, and the gradients agree up to bf16 noise."""
    from openvision_amd import training
    res = run_ranks(_ddp_rank, 2, timeout=600, backend="gloo", gpu=True)
    dp_loss = res[0][1]
    dp_grads = next(r[2] for r in res if r[2] is not None)
    cfg, sd = _siglip_cfg_sd()
    m = create_model(cfg, device=DEV, state_dict=sd)
    img, tok = synth.make_images(8, 160, seed=41).to(DEV), synth.make_captions(8, seed=41).to(DEV)
    loss = SigLipLoss()(*training.clip_forward(m, img, tok))
    loss.backward()
    assert abs(float(loss.detach()) - dp_loss) < 2e-3 * max(1.0, abs(dp_loss))
    scale = max(float(p.grad.norm()) for p in m.parameters())
    checked = 0
    for name, p in m.named_parameters():
        g, d_ = p.grad.float().cpu(), torch.from_numpy(dp_grads[name])
        if float(g.norm()) < 1e-3 * scale:
            continue
        cos = float((g * d_).sum() / (g.norm() * d_.norm() + 1e-30))
        assert cos > 0.995, (name, cos)
        assert abs(float(d_.norm()) - float(g.norm())) < 0.03 * float(g.norm()), name
        checked += 1
    assert checked > 100
