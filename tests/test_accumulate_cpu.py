"""CPU: gradient accumulation for the InfoNCE (openvision_amd.accumulate, ov_clip_loss_window_backward) -- the float64 window
restatement against the world-of-one gradient and against the reference-made fixture tests/golden/multicap_grad.npz, the
accumulator's bookkeeping and refusals, the new entry point's status codes without a device, and FusedAdamW.zero_grad(windows=...)."""
import os
import re
import subprocess

import pytest
import torch

from openvision_amd import _lib, training
from openvision_amd import build as B
from openvision_amd.accumulate import ContrastiveAccumulator, WindowLayout
from openvision_amd.loss import ClipLoss, DistillClipLoss, MultiCaptionClipLoss, SigLipLoss

import multicap_restate as MR
import window_restate as WR
from conftest import golden

IDS = [c[0] for c in MR.CASES]
GWG = [c for c in MR.CASES if c[5] and c[6] and c[1] > 1]


def windows_of(n: int, b: int):
    """Two covers of [0, n) by disjoint windows: the ranks' own rows, and an uneven cut."""
    return [[(w0, b) for w0 in range(0, n, b)], [(0, 5), (5, n - 5)]]


@pytest.mark.parametrize("case", MR.CASES, ids=IDS)
def test_window_rows_are_the_world_of_one_gradient_and_shares_sum(case):
    """Over the case's N rows as ONE batch: every window's gradients are the matching rows of the one-batch gradient to 1e-12 of the
    largest entry, and the windows' loss and d_scale shares sum to the full values."""
    name, ws, b, e, c, _, _, s, seed = case
    img, sets = MR.case_inputs(ws, b, e, c, seed)
    n = ws * b
    (loss, g_img, g_txt, d_s), = MR.per_rank(img, sets, s, 1, True, False)
    terms = WR.bank_terms(img, sets, s)
    for cover in windows_of(n, b):
        assert sum(w[1] for w in cover) == n
        tot_s = tot_l = 0.0
        for w0, wb in cover:
            di, dt, ds, ls = WR.window(img, sets, s, w0, wb, n, terms)
            want_t = torch.cat([g_txt[k * n + w0:k * n + w0 + wb] for k in range(c)], dim=0)
            assert float((di - g_img[w0:w0 + wb]).abs().max()) <= 1e-12 * float(g_img.abs().max()), (name, w0)
            assert float((dt - want_t).abs().max()) <= 1e-12 * float(g_txt.abs().max()), (name, w0)
            tot_s, tot_l = tot_s + float(ds), tot_l + float(ls)
        assert abs(tot_s - float(d_s)) <= 1e-10 * abs(float(d_s)), name
        assert abs(tot_l - float(loss)) <= 1e-10 * abs(float(loss)), name
    # norm_rows and the upstream gradient are plain factors
    a, h = WR.window(img, sets, s, 0, b, n, terms), WR.window(img, sets, s, 0, b, 2 * n, terms, grad=0.5)
    for x, y in zip(a, h):
        assert torch.allclose(torch.as_tensor(y), 0.25 * torch.as_tensor(x), rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", GWG, ids=[c[0] for c in GWG])
def test_window_restatement_reproduces_the_references_gather_with_grad(case):
    """local_loss + gather_with_grad at world size ws is the window scheme at norm_rows = b: rank r's window [r b, (r + 1) b) has
    the gradients the reference's ClipLoss gave that rank by autograd through the differentiable gather (1e-6 relative), its loss
    share is the rank's loss, and the ranks' d_scale shares have the mean of the ranks' logit_scale gradients (a rank's share
    holds its image-side strips only, so only the sums over ranks agree: sum_r share_r = sum_r dscale_r)."""
    name, ws, b, e, c, _, _, s, seed = case
    z = golden("multicap_grad.npz")
    img, sets = MR.case_inputs(ws, b, e, c, seed)
    shares = []
    for r in range(ws):
        di, dt, ds, ls = WR.window(img, sets, s, r * b, b, b)
        for got, key in ((di, "dimg"), (dt, "dtxt")):
            want = torch.from_numpy(z[f"{name}_{key}"][r]).double()
            assert got.shape == want.shape
            assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()), (name, r, key)
        assert abs(float(ls) - float(z[f"{name}_loss"][r])) <= 1e-9 * abs(float(z[f"{name}_loss"][r]))
        shares.append(float(ds))
    want = float(z[f"{name}_dscale"].astype("float64").mean())
    assert abs(sum(shares) / ws - want) <= 1e-9 * abs(want), name


def test_window_layout_offsets_and_refusals():
    for ws, a, b in ((1, 3, 4), (2, 2, 5)):
        for rank in range(ws):
            lay = WindowLayout(2, rank, ws)
            assert [lay.admit((b, 64), (2 * b, 64)) for _ in range(a)] == list(range(a))
            lay.close()
            assert lay.local_rows == a * b and lay.bank_rows == ws * a * b
            assert [lay.start(j) for j in range(a)] == [(rank * a + j) * b for j in range(a)]
            assert [lay.start(j, rank=r) for r in range(ws) for j in range(a)] == list(range(0, ws * a * b, b))   # disjoint, in order
            with pytest.raises(IndexError):
                lay.start(a)
            with pytest.raises(RuntimeError):
                lay.admit((b, 64), (2 * b, 64))
    lay = WindowLayout(1)
    lay.admit((4, 64), (4, 64))
    for bad in (((5, 64), (5, 64)), ((4, 32), (4, 32)), ((4, 64), (8, 64)), ((4,), (4, 64))):
        with pytest.raises(ValueError):
            lay.admit(*bad)
    assert lay.windows == 1
    with pytest.raises(RuntimeError):
        WindowLayout(1).close()


def test_accumulator_refusals():
    for bad in (SigLipLoss(), DistillClipLoss()):
        with pytest.raises(TypeError):
            ContrastiveAccumulator(bad)
    with pytest.raises(ValueError):
        ContrastiveAccumulator(ClipLoss(local_loss=True, rank=0, world_size=2))
    ContrastiveAccumulator(MultiCaptionClipLoss(2, local_loss=True, gather_with_grad=True, rank=1, world_size=2))
    acc = ContrastiveAccumulator(MultiCaptionClipLoss(2))
    assert acc.layout.num_captions == 2
    with pytest.raises(ValueError):
        acc.add(torch.zeros(4, 64), torch.zeros(4, 64))               # [C b, E] wanted: the shape is judged before the device
    with pytest.raises(_lib.OvhipError):
        acc.add(torch.zeros(4, 64), torch.zeros(8, 64))               # CPU tensors
    assert acc.layout.windows == 0
    with pytest.raises(RuntimeError):
        acc.window_loss(0, torch.zeros(4, 64), torch.zeros(8, 64), 1.0)
    acc.layout.admit((4, 64), (8, 64))
    with pytest.raises(ValueError):
        acc.add(torch.zeros(6, 64), torch.zeros(12, 64))              # unequal b
    acc.layout.close()
    with pytest.raises(RuntimeError):
        acc.add(torch.zeros(4, 64), torch.zeros(8, 64))               # add after close
    acc.reset()
    assert acc.layout.windows == 0 and not acc.layout.closed


def test_window_backward_status_codes_without_a_device():
    """Every refusal is a status code returned before any HIP call (the pointers are never dereferenced)."""
    lib = _lib.load()
    wsz = lib.ov_clip_loss_window_backward_workspace_bytes
    assert wsz(256, 16384, 2) >= 8 * 4 and wsz(33, 64, 1) >= 2 * 4
    assert wsz(0, 64, 1) == 0 and wsz(16, 0, 1) == 0 and wsz(65, 64, 1) == 0 and wsz(16, 64, 0) == 0 and wsz(16, 64, 5) == 0
    fake = 1 << 20

    def call(ai=fake, at=fake, ld=192, ss=64, n=64, e=64, c=2, s=fake, terms=fake, w0=16, b=16, norm=64, di=fake, dt=fake, dsc=None,
             w=fake, wb=1 << 12):
        return lib.ov_clip_loss_window_backward(ai, at, ld, ss, n, e, c, s, terms, None, w0, b, norm, di, dt, dsc, w, wb, None)

    for k in ("ai", "at", "s", "terms", "di", "dt", "w"):
        assert call(**{k: None}) == -1, k
    assert call(w0=49) == -1 and call(w0=-1) == -1 and call(b=0) == -1 and call(norm=0) == -1 and call(w0=48, b=17) == -1
    assert call(c=0) == -1 and call(c=5) == -2
    assert call(e=1184, ld=3 * 1184, ss=1184) == -2 and call(e=48, ld=144, ss=48) == -2
    assert call(ld=60) == -1 and call(ld=194) == -1 and call(ss=66) == -1 and call(ss=-4) == -1
    for k in ("ai", "at", "terms", "di", "dt", "w"):
        assert call(**{k: fake + 4}) == -1, k
    assert call(wb=0) == -3 and call(b=64, w0=0, wb=wsz(64, 64, 2) - 1) == -3


def test_window_kernel_uses_no_scratch_and_is_exported():
    out = subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", "-",
                          os.path.join(B.CSRC, "window.hip")], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
    res = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", out)}
    assert len(res) == 2 and any("window_loss_bwd" in k for k in res) and any("scaled_sum" in k for k in res), sorted(res)
    assert all(v == 0 for v in res.values()), res
    assert "window.hip" in B.SOURCES
    import openvision_amd
    assert openvision_amd.ContrastiveAccumulator is ContrastiveAccumulator and "ContrastiveAccumulator" in openvision_amd.__all__


def test_zero_grad_windows_defers_the_exchange_to_the_last_window():
    """Under accumulation every parameter's gradient lands once per window: with zero_grad(windows=3) no bucket starts before the third
    backward, all have started when it returns; windows=1 is one backward per step."""
    model = torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.Linear(40, 8))
    opt = training.FusedAdamW(model, lr=1e-3, bucket_bytes=1 << 10)
    opt.overlap_gradient_exchange(1, always_collective=False)
    nb = len(opt._ov_buckets)
    assert nb >= 2
    x = torch.randn(5, 24)

    def backward():
        model(x).sum().backward()
        return sum(opt._ov["launched"])

    opt.zero_grad()
    assert backward() == nb
    one = [g["grad"].clone() for g in opt.groups]
    opt.zero_grad(windows=1)
    assert backward() == nb
    opt.zero_grad(windows=3)
    assert backward() == 0 and backward() == 0
    assert all(p > 0 for p in opt._ov["pending"])
    assert backward() == nb and all(p == 0 for p in opt._ov["pending"])
    for g, w in zip(opt.groups, one):
        assert torch.allclose(g["grad"], 3 * w, rtol=1e-6, atol=1e-7)
    assert opt.all_reduce_gradients(1) == 1.0
    with pytest.raises(ValueError):
        opt.zero_grad(windows=0)
    opt.zero_grad()                                                    # back to one backward per step
    assert backward() == nb
