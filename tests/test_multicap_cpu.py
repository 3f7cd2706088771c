"""CPU: the multi-caption InfoNCE (openvision_amd.loss.MultiCaptionClipLoss, reference src/losses/common.py:120-189) -- the float64
restatement against the reference's ClipLoss run per caption set (tests/golden/multicap_grad.npz), the C ABI without a device, zero
scratch in the new kernels, the refusals, the packed gather and the gradient routing over gloo, and the training entry points."""
import os
import re
import subprocess

import pytest
import torch

from openvision_amd import _lib, training
from openvision_amd import build as B
from openvision_amd import loss as L
from openvision_amd.loss import MultiCaptionClipLoss
from oracle import clip_ref as R

import multicap_restate as MR
from conftest import golden
from ranks import run_ranks

IDS = [c[0] for c in MR.CASES]


@pytest.fixture(scope="module")
def fixture():
    return golden("multicap_grad.npz")


def fixture_case(z, case):
    """The case's inputs regenerated from their seed, checked against the fixture's sums."""
    name, ws, b, e, c, local_loss, gwg, s, seed = case
    img, sets = MR.case_inputs(ws, b, e, c, seed)
    for key, x in (("img", img), ("txt", sets)):
        ref_abs = float(z[f"{name}_{key}_abs_sum"])
        assert abs(float(x.sum()) - float(z[f"{name}_{key}_sum"])) <= 1e-9 * ref_abs, (name, key)
        assert abs(float(x.abs().sum()) - ref_abs) <= 1e-9 * ref_abs, (name, key)
    return img, sets


def test_fixture_covers_the_cases(fixture):
    assert list(fixture["cases"]) == IDS
    assert {c[1] for c in MR.CASES} == {1, 2, 3}
    assert {(c[5], c[6]) for c in MR.CASES if c[1] > 1} == {(True, False), (True, True), (False, False)}
    assert {c[4] for c in MR.CASES} == {1, 2, 3} and {c[2] for c in MR.CASES} == {13, 16} and {c[3] for c in MR.CASES} == {64, 768}
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "multicap_grad.npz")) < 1 << 20


@pytest.mark.parametrize("case", MR.CASES, ids=IDS)
def test_inputs_are_matched_and_the_sets_differ(fixture, case):
    """Every caption set is correlated with the images (the loss lies well below log N) and the sets are different draws."""
    name, ws, b, e, c, local_loss, gwg, s, seed = case
    img, sets = fixture_case(fixture, case)
    assert float(torch.tensor(fixture[f"{name}_loss"]).max()) < 0.5 * float(torch.log(torch.tensor(float(ws * b))))
    assert torch.allclose(img.norm(dim=-1), torch.ones(ws * b, dtype=torch.float64), atol=1e-6)
    for k in range(c):
        assert float((img * sets[k]).sum(-1).min()) > 0.2
        for k2 in range(k):
            assert float((sets[k] - sets[k2]).abs().max()) > 1e-2


@pytest.mark.parametrize("case", MR.CASES, ids=IDS)
def test_restatement_reproduces_the_reference(fixture, case):
    """Every rank's loss and gradients from the restated JAX function equal what the reference's ClipLoss, run once per caption set
    and averaged, gave by autograd -- the text gradient after routing the gathered side as the case's mode prescribes."""
    name, ws, b, e, c, local_loss, gwg, s, seed = case
    img, sets = fixture_case(fixture, case)
    per = MR.per_rank(img, sets, s, ws, local_loss, gwg)
    for r, (loss, di, dt, ds) in enumerate(per):
        ref = float(fixture[f"{name}_loss"][r])
        assert abs(float(loss) - ref) <= 1e-9 * abs(ref), (name, r)
        for got, key in ((di, "dimg"), (dt, "dtxt")):
            want = torch.from_numpy(fixture[f"{name}_{key}"][r]).double()
            assert got.shape == want.shape, (name, key)
            assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()), (name, r, key)
        want = float(fixture[f"{name}_dscale"][r])
        assert abs(float(ds) - want) <= 1e-9 * max(abs(want), 1e-12), (name, r)


@pytest.mark.parametrize("case", MR.CASES, ids=IDS)
def test_autograd_of_the_restatement_equals_its_closed_form(case):
    name, ws, b, e, c, local_loss, gwg, s, seed = case
    img, sets = MR.case_inputs(ws, b, e, c, seed)
    rank = ws - 1
    leaves = [img[rank * b:(rank + 1) * b].clone(), MR.stack_local(sets, rank, b).clone(), img.clone(), sets.clone(),
              torch.tensor(s, dtype=torch.float64)]
    for x in leaves:
        x.requires_grad_(True)
    MR.strip_loss(*leaves, rank, c).backward()
    closed = MR.strip_grads(*[x.detach() for x in leaves], rank, c)
    for x, want in zip(leaves, closed):
        assert torch.allclose(x.grad, torch.as_tensor(want), rtol=1e-10, atol=1e-14), name
    half = MR.strip_grads(*[x.detach() for x in leaves], rank, c, grad=0.5)
    assert torch.allclose(half[0], 0.5 * closed[0], rtol=1e-12) and torch.allclose(half[3], 0.5 * closed[3], rtol=1e-12)


def test_one_set_is_the_oracles_clip_loss():
    """At C = 1 the restatement is oracle.clip_ref.clip_loss / clip_loss_grads.  The oracle computes in fp32, so the comparison is
    at fp32 accuracy, with the multiplier of the fixture's cases (a loss of order 0.5: lse - diag does not cancel)."""
    img, sets = MR.case_inputs(3, 13, 64, 1, 77)
    b, rank, s = 13, 1, 5.0
    li, lt = img[13:26], sets[0, 13:26]
    want = R.clip_loss(li.float(), lt.float(), s, img.float(), sets[0].float(), rank)
    got = MR.strip_loss(li, lt, img, sets, s, rank, 1)
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    d_img, d_txt, d_ai, d_at, d_s = MR.strip_grads(li, lt, img, sets, s, rank, 1)
    o_img, o_txt, o_ai, o_at, o_s = R.clip_loss_grads(li.float(), lt.float(), s, img.float(), sets[0].float(), rank)
    for got, want in ((d_img, o_img), (d_txt, o_txt), (d_ai, o_ai), (d_at[0], o_at)):
        assert float((got - want.double()).abs().max()) <= 1e-5 * float(want.abs().max())
    assert abs(float(d_s) - float(o_s)) <= 1e-5 * abs(float(o_s)) + 1e-9


SYMS = ("ov_clip_loss_multi_workspace_bytes", "ov_clip_loss_multi", "ov_clip_loss_multi_backward_workspace_bytes",
        "ov_clip_loss_multi_backward")


def test_new_symbols_exported_bound_and_validating():
    lib = _lib.load()
    for s in SYMS:
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert lib.ov_abi_version() == 2
    wsz = lib.ov_clip_loss_multi_workspace_bytes
    assert wsz(256, 2048, 2) > wsz(256, 2048, 1) > 0
    assert wsz(0, 2048, 2) == 0 and wsz(16, 0, 2) == 0 and wsz(16, -4, 2) == 0 and wsz(16, 64, 0) == 0 and wsz(16, 64, 5) == 0
    bsz = lib.ov_clip_loss_multi_backward_workspace_bytes
    assert bsz(4096, 32768, 2) >= 3 * 128 * 4
    assert bsz(0, 64, 2) == 0 and bsz(16, 0, 2) == 0 and bsz(-1, 64, 2) == 0 and bsz(16, 64, 0) == 0 and bsz(16, 64, 5) == 0
    fake = 1 << 20                                   # never dereferenced: every call below fails its checks first
    ws = wsz(16, 64, 2)

    def fwd(i=fake, t=fake, ai=fake, at=fake, ld=192, ss=64, b=16, n=64, e=64, c=2, s=fake, off=0, out=fake, w=fake, wb=ws):
        return lib.ov_clip_loss_multi(i, t, ai, at, ld, ss, b, n, e, c, s, off, out, None, w, wb, None)

    for k in ("i", "t", "ai", "at", "s", "out", "w"):
        assert fwd(**{k: None}) == -1, k
    assert fwd(b=0) == -1 and fwd(n=0) == -1 and fwd(b=65) == -1 and fwd(e=0) == -1 and fwd(off=-1) == -1 and fwd(off=49) == -1
    assert fwd(c=0) == -1 and fwd(c=5) == -2
    assert fwd(e=36, ld=36 * 3) == -2                # forward: E % 8
    assert fwd(ld=60) == -1 and fwd(ld=194) == -1 and fwd(ss=66) == -1 and fwd(ss=-64) == -1        # pitch / stride rules
    for k in ("i", "t", "ai", "at", "w"):
        assert fwd(**{k: fake + 4}) == -1, k         # 16-byte alignment
    assert fwd(wb=ws - 1) == -3
    wsb = bsz(16, 64, 2)

    def bwd(i=fake, t=fake, ai=fake, at=fake, ld=192, ss=64, b=16, n=64, e=64, c=2, s=fake, off=0, terms=fake, di=fake, dt=fake,
            dai=None, dat=None, ldg=0, gss=0, w=fake, wb=wsb):
        return lib.ov_clip_loss_multi_backward(i, t, ai, at, ld, ss, b, n, e, c, s, off, terms, None, di, dt, dai, dat, ldg, gss,
                                               None, w, wb, None)

    for k in ("i", "t", "ai", "at", "s", "terms", "di", "dt", "w"):
        assert bwd(**{k: None}) == -1, k
    assert bwd(b=-1) == -1 and bwd(b=65) == -1 and bwd(off=60) == -1 and bwd(c=0) == -1 and bwd(c=5) == -2
    assert bwd(e=40, ld=120) == -2 and bwd(e=1152 + 32, ld=3 * 1184) == -2          # backward: E % 32, E <= 1152
    assert bwd(ld=32) == -1 and bwd(ss=6) == -1
    assert bwd(dai=fake, dat=fake, ldg=60, gss=64) == -1 and bwd(dai=fake, dat=fake, ldg=192, gss=2) == -1
    assert bwd(dai=fake + 8, dat=fake, ldg=192, gss=64) == -1 and bwd(di=fake + 4) == -1
    assert bwd(wb=wsb - 1) == -3 and bwd(dai=fake, dat=fake, ldg=192, gss=64, wb=wsb - 1) == -3


@pytest.mark.timeout(900)
def test_multicap_kernels_use_no_scratch():
    out = subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", "-",
                          os.path.join(B.CSRC, "multicap.hip")], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
    res = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", out)}
    mine = {k: v for k, v in res.items() if "multicap_" in k or "scaled_sum" in k}
    assert len(mine) == len(res) == 5, sorted(res)   # partial, finalize, backward local / gathered, strip.h's scaled sum (d scale)
    assert all(v == 0 for v in mine.values()), mine
    assert "multicap.hip" in B.SOURCES


def test_loss_module_refusals_and_surface():
    import openvision_amd
    assert openvision_amd.MultiCaptionClipLoss is MultiCaptionClipLoss and "MultiCaptionClipLoss" in openvision_amd.__all__
    with pytest.raises(NotImplementedError):
        MultiCaptionClipLoss(use_horovod=True)
    with pytest.raises(ValueError):
        MultiCaptionClipLoss(num_captions=5)
    img = torch.nn.functional.normalize(torch.randn(4, 32), dim=-1)
    txt = torch.nn.functional.normalize(torch.randn(8, 32), dim=-1)
    with pytest.raises(_lib.OvhipError):
        MultiCaptionClipLoss()(img, txt, torch.tensor(10.0))
    with pytest.raises(_lib.OvhipError):
        MultiCaptionClipLoss()(img.clone().requires_grad_(True), txt, 10.0)
    with pytest.raises(ValueError):
        MultiCaptionClipLoss()(img, txt[:6], 10.0)              # not C * b rows
    with pytest.raises(ValueError):
        MultiCaptionClipLoss(num_captions=3)(img, txt, 10.0)
    fn = MultiCaptionClipLoss(3, local_loss=True, gather_with_grad=True, rank=1, world_size=2)
    assert (fn.num_captions, fn.local_loss, fn.gather_with_grad, fn.rank, fn.world_size, fn.always_collective) == (3, True, True, 1, 2, False)
    assert MultiCaptionClipLoss().num_captions == 2 and fn.last_terms is None


def test_forwards_refuse_a_text_batch_that_is_no_multiple(monkeypatch):
    """training.clip_forward / coca_forward take [C B, T] tokens: the text tower runs once on all rows and the decoder gets the
    first B rows' tokens.  The towers are stubbed: only the structure is under test."""
    calls = {}

    class M:
        logit_scale = torch.tensor(0.0)

    def enc_img(model, image, normalize=True, output_tokens=False):
        f, t = torch.zeros(image.shape[0], 8), torch.zeros(image.shape[0], 5, 8)
        return (f, t) if output_tokens else f

    def enc_txt(model, text, normalize=True, output_tokens=False):
        calls["text_rows"] = calls.get("text_rows", []) + [text.shape[0]]
        f = torch.arange(text.shape[0], dtype=torch.float32)[:, None].expand(-1, 8)
        t = torch.arange(text.shape[0], dtype=torch.float32)[:, None, None].expand(-1, 3, 8)
        return (f, t) if output_tokens else f

    def dec(decoder, image_tokens, text_tokens):
        calls["decoder"] = (image_tokens.shape[0], text_tokens.clone())
        return torch.zeros(image_tokens.shape[0], 3, 11)

    monkeypatch.setattr(training, "encode_image", enc_img)
    monkeypatch.setattr(training, "encode_text", enc_txt)
    monkeypatch.setattr(training, "decode", dec)
    image = torch.zeros(4, 3, 16, 16)
    for rows in (6, 3, 0):
        with pytest.raises(ValueError):
            training.clip_forward(M(), image, torch.zeros(rows, 7, dtype=torch.long))
        with pytest.raises(ValueError):
            training.coca_forward(M(), None, image, torch.zeros(rows, 7, dtype=torch.long))
    assert "text_rows" not in calls                              # refused before a tower ran
    out = training.clip_forward(M(), image, torch.zeros(8, 7, dtype=torch.long))
    assert out[0].shape[0] == 4 and out[1].shape[0] == 8 and calls["text_rows"] == [8]
    for rows in (12, 4):
        calls.clear()
        img_f, txt_f, scale, cap = training.coca_forward(M(), None, image, torch.zeros(rows, 7, dtype=torch.long))
        assert calls["text_rows"] == [rows] and txt_f.shape[0] == rows and cap.shape[0] == 4
        nb, seen = calls["decoder"]
        assert nb == 4 and seen.shape[0] == 4 and torch.equal(seen[:, 0, 0], torch.arange(4.0))     # the first set's tokens only


def _gloo_rank(rank, ws):
    b, e, c = 3, 8, 2
    log = []
    L.record_comm(log)
    img = torch.full((b, e), 100.0 * rank) + torch.arange(b)[:, None]                     # value = 100 rank + row
    txt = torch.cat([torch.full((b, e), 100.0 * rank + 10.0 * (k + 1)) + torch.arange(b)[:, None] for k in range(c)])
    packed = L.gather_caption_features(img, txt, c, ws)
    L.record_comm(None)
    # a hand-made packed gradient of the gathered rows that differs on every rank
    g = torch.Generator().manual_seed(9)
    fulls = [torch.randn(ws * b, (1 + c) * e, generator=g) for _ in range(ws)]
    summed = L.route_packed_gradient(fulls[rank].clone(), b, rank, True)
    own = L.route_packed_gradient(fulls[rank].clone(), b, rank, False)
    return packed, len(log), summed.clone(), own.clone(), fulls


def test_packed_gather_and_gradient_routing_over_gloo():
    """Two gloo ranks on CPU tensors: ONE collective gathers the packed [b, (1 + C) E] rows in rank order, the columns split into
    the image and the C sets, and a packed gathered-side gradient is routed as each mode prescribes."""
    ws, b, e, c = 2, 3, 8, 2
    res = run_ranks(_gloo_rank, ws, timeout=300, backend="gloo")
    for rank in range(ws):
        packed, ncoll, summed, own, fulls = res[rank]
        assert ncoll == 1 and packed.shape == (ws * b, (1 + c) * e)
        all_img, all_txt = L.unpack_caption_features(packed, c)
        assert all_img.shape == (ws * b, e) and all_txt.shape == (c * ws * b, e)
        for g in range(ws * b):                                                           # rank order, row order
            assert torch.all(all_img[g] == 100.0 * (g // b) + g % b)
            for k in range(c):
                assert torch.all(all_txt[k * ws * b + g] == 100.0 * (g // b) + 10.0 * (k + 1) + g % b)
                assert torch.all(packed[g, (1 + k) * e:(2 + k) * e] == all_txt[k * ws * b + g])
        assert torch.allclose(summed, sum(fulls)[rank * b:(rank + 1) * b])
        assert torch.equal(own, fulls[rank][rank * b:(rank + 1) * b])
    # pack / unpack are inverses on a local batch
    img, txt = torch.randn(b, e), torch.randn(c * b, e)
    i2, t2 = L.unpack_caption_features(L.pack_caption_features(img, txt, c), c)
    assert torch.equal(i2, img) and torch.equal(t2, txt)
