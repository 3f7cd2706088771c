"""CPU: the SigLIP loss (openvision_amd.loss.SigLipLoss, reference open_clip/loss.py:307-414) and CLIP's logit_bias -- the
all-gather restatement against the reference's ring (tests/golden/siglip_grad.npz), the C ABI without a device, zero scratch in
the new kernels, the refusals, and the model / checkpoint surface."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from openvision_amd import _lib, preset, synth
from openvision_amd import build as B
from openvision_amd import checkpoint, training
from openvision_amd.loss import SigLipLoss
from openvision_amd.model import CLIP, create_model

import siglip_restate as SR
from conftest import golden


@pytest.fixture(scope="module")
def fixture():
    return golden("siglip_grad.npz")


def fixture_case(z, case):
    """The case's inputs regenerated from their seed, checked against the fixture's sums."""
    name, ws, b, e, s, beta, bidir, seed = case
    img, txt = SR.case_inputs(ws, b, e, seed)
    for key, x in (("img", img), ("txt", txt)):
        ref_abs = float(z[f"{name}_{key}_abs_sum"])
        assert abs(float(x.sum()) - float(z[f"{name}_{key}_sum"])) <= 1e-9 * ref_abs, (name, key)
        assert abs(float(x.abs().sum()) - ref_abs) <= 1e-9 * ref_abs, (name, key)
    return img, txt


def test_fixture_covers_the_cases(fixture):
    assert list(fixture["cases"]) == [c[0] for c in SR.CASES]
    wss = {c[1] for c in SR.CASES}
    assert wss == {1, 2, 3, 4}
    assert {c[6] for c in SR.CASES if c[1] > 1} == {True, False}
    assert {c[3] for c in SR.CASES} >= {40, 768} and {c[2] % 32 for c in SR.CASES} >= {0, 13}
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "siglip_grad.npz")) < 1 << 20


@pytest.mark.parametrize("case", SR.CASES, ids=[c[0] for c in SR.CASES])
def test_restatement_reproduces_the_reference_ring(fixture, case):
    """Every rank's loss and gradients from the all-gather formulation equal what the reference's neighbour-exchange ring gave,
    the text gradient after summing the gathered side over ranks: the transport changes only the order of the sums."""
    name, ws, b, e, s, beta, bidir, seed = case
    img, txt = fixture_case(fixture, case)
    per = SR.per_rank(img, txt, torch.tensor(s, dtype=torch.float64), torch.tensor(beta, dtype=torch.float64), ws)
    for r, (loss, di, dt, ds, db) in enumerate(per):
        assert abs(float(loss) - float(fixture[f"{name}_loss"][r])) <= 1e-9 * abs(float(fixture[f"{name}_loss"][r])), (name, r)
        for got, key in ((di, "dimg"), (dt, "dtxt")):
            ref = torch.from_numpy(fixture[f"{name}_{key}"][r]).double()
            assert got.shape == ref.shape
            assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), (name, r, key)
        for got, key in ((ds, "dscale"), (db, "dbias")):
            ref = float(fixture[f"{name}_{key}"][r])
            assert abs(float(got) - ref) <= 1e-9 * max(abs(ref), 1e-12), (name, r, key)
    # the autograd of the differentiable restatement agrees with its closed form
    li = img[:b].clone().requires_grad_(True)
    at = txt.clone().requires_grad_(True)
    sc = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    bi = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    SR.strip_loss(li, at, sc, bi, 0).backward()
    di, da, ds, db = SR.strip_grads(img[:b], txt, s, beta, 0)
    assert torch.allclose(li.grad, di, rtol=1e-10, atol=1e-14) and torch.allclose(at.grad, da, rtol=1e-10, atol=1e-14)
    assert abs(float(sc.grad - ds)) < 1e-10 * max(1.0, abs(float(ds))) and abs(float(bi.grad - db)) < 1e-10 * max(1.0, abs(float(db)))


def test_new_symbols_exported_bound_and_validating():
    lib = _lib.load()
    for s in ("ov_siglip_loss_workspace_bytes", "ov_siglip_loss", "ov_siglip_loss_backward_workspace_bytes",
              "ov_siglip_loss_backward"):
        assert s in _lib.SIGNATURES
    assert lib.ov_siglip_loss_workspace_bytes(256, 2048) > 0 and lib.ov_siglip_loss_workspace_bytes(0, 2048) == 0
    assert lib.ov_siglip_loss_backward_workspace_bytes(4096, 32768) >= 2 * 128 * 4
    assert lib.ov_siglip_loss_backward_workspace_bytes(16, 0) == 0
    fake = 1 << 20                                   # never dereferenced: every call below fails its checks first
    ws = lib.ov_siglip_loss_workspace_bytes(16, 64)

    def fwd(x=fake, y=fake, b=16, n=64, e=64, s=fake, off=0, out=fake, w=fake, wb=ws):
        return lib.ov_siglip_loss(x, y, b, n, e, s, None, off, out, w, wb, None)

    assert fwd(x=None) == -1 and fwd(y=None) == -1 and fwd(s=None) == -1 and fwd(out=None) == -1 and fwd(w=None) == -1
    assert fwd(b=0) == -1 and fwd(n=0) == -1 and fwd(off=-1) == -1 and fwd(off=49) == -1 and fwd(b=65) == -1
    assert fwd(e=0) == -1 and fwd(e=36) == -2 and fwd(e=1160) == -2
    assert fwd(x=fake + 4) == -1                     # 16-byte alignment of the feature rows
    assert fwd(wb=ws - 1) == -3
    wsb = lib.ov_siglip_loss_backward_workspace_bytes(16, 64)

    def bwd(x=fake, y=fake, b=16, n=64, e=64, off=0, dx=fake, w=fake, wb=wsb):
        return lib.ov_siglip_loss_backward(x, y, b, n, e, fake, None, off, None, dx, None, None, None, w, wb, None)

    assert bwd(x=None) == -1 and bwd(dx=None) == -1 and bwd(w=None) == -1
    assert bwd(b=-1) == -1 and bwd(off=60) == -1 and bwd(e=20) == -2 and bwd(e=1152 + 8) == -2
    assert bwd(wb=wsb - 1) == -3


@pytest.mark.timeout(900)
def test_siglip_kernels_use_no_scratch():
    out = subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", "-",
                          os.path.join(B.CSRC, "siglip.hip")], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
    res = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", out)}
    mine = {k: v for k, v in res.items() if "siglip_loss" in k}
    assert len(mine) == 4, sorted(res)               # partial, finalize, backward, backward scalars
    assert all(v == 0 for v in mine.values()), mine
    assert "siglip.hip" in B.SOURCES


def test_siglip_loss_refuses_cpu_and_horovod():
    with pytest.raises(NotImplementedError):
        SigLipLoss(use_horovod=True)
    x = torch.nn.functional.normalize(torch.randn(4, 16), dim=-1)
    with pytest.raises(_lib.OvhipError):
        SigLipLoss()(x, x, torch.tensor(10.0), torch.tensor(-10.0))
    with pytest.raises(_lib.OvhipError):
        SigLipLoss()(x.requires_grad_(True), x, 10.0, None)
    fn = SigLipLoss(rank=1, world_size=2, bidir=False)                 # the reference's constructor
    assert (fn.rank, fn.world_size, fn.bidir, fn.always_collective) == (1, 2, False, False)


def _bias_model(beta=-10.0):
    cfg = preset("vit-tiny-patch16-160")
    return cfg, CLIP(embed_dim=cfg["embed_dim"], vision_cfg=cfg["vision_cfg"], text_cfg=cfg["text_cfg"], init_logit_bias=beta,
                     init_logit_scale=float(np.log(10.0)))


def test_logit_bias_parameter_and_checkpoint_round_trip(tmp_path):
    cfg, m = _bias_model(-10.0)
    sd = m.state_dict()
    assert "logit_bias" in sd and sd["logit_bias"].shape == torch.Size([]) and float(sd["logit_bias"]) == -10.0
    assert set(sd) == set(synth.make_state_dict(cfg)) | {"logit_bias"}
    assert create_model(cfg).logit_bias is None and "logit_bias" not in create_model(cfg).state_dict()
    full = {**synth.make_state_dict(cfg), "logit_bias": torch.tensor(-12.5)}
    mcfg = {**cfg, "init_logit_bias": -10.0}
    m2 = create_model(mcfg, state_dict=full)                         # strict
    checkpoint.save_pretrained(m2, mcfg, str(tmp_path))
    m3, _ = checkpoint.from_pretrained(str(tmp_path), device=None)
    assert m3.logit_bias is not None and float(m3.logit_bias.detach()) == -12.5
    for k, v in m2.state_dict().items():
        assert torch.equal(m3.state_dict()[k], v), k
    with pytest.raises(RuntimeError):                               # a bias checkpoint into a model without one: strict load fails
        create_model(cfg, state_dict=full)


def test_logit_bias_is_not_decayed():
    _, m = _bias_model()
    assert training.default_decay_filter("logit_bias", m.logit_bias) is False
    assert training.default_decay_filter("logit_scale", m.logit_scale) is False
    opt = training.FusedAdamW(m, lr=1e-3)
    nodecay = [g for g in opt.groups if g["wd"] == 0.0]
    assert len(nodecay) == 1 and any(n == "logit_bias" for n, _ in nodecay[0]["params"])


def test_forward_and_get_logits_structure(monkeypatch):
    """model.py:286-315: forward returns (img, txt, logit_scale.exp(), logit_bias) or a dict with 'logit_bias'; get_logits adds
    the bias.  Models without a bias keep the 3-tuple and dict.  The towers are stubbed: only the structure is under test."""
    from openvision_amd import model as M
    _, m = _bias_model(-3.0)
    fi, ft = torch.randn(3, 192), torch.randn(5, 192)
    monkeypatch.setattr(m, "encode_image", lambda image, normalize=False: fi)
    monkeypatch.setattr(m, "encode_text", lambda text, normalize=False: ft)
    monkeypatch.setattr(M, "logits", lambda a, b, scale=1.0: scale * a @ b.T)
    out = m(object(), object())
    assert len(out) == 4 and out[0] is fi and out[1] is ft
    assert torch.allclose(out[2], torch.tensor(10.0)) and float(out[3]) == -3.0
    m.output_dict = True
    d = m(object(), object())
    assert set(d) == {"image_features", "text_features", "logit_scale", "logit_bias"} and float(d["logit_bias"]) == -3.0
    li, lt = m.get_logits(object(), object())
    assert torch.allclose(li, 10.0 * fi @ ft.T - 3.0, atol=1e-5) and torch.equal(lt, li.T)
    cfg = preset("vit-tiny-patch16-160")
    plain = CLIP(embed_dim=cfg["embed_dim"], vision_cfg=cfg["vision_cfg"], text_cfg=cfg["text_cfg"])
    assert len(plain(None, None)) == 3
    plain.output_dict = True
    assert "logit_bias" not in plain(None, None)
