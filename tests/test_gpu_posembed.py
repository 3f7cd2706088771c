"""GPU: the towers at other resolutions than they were built at -- ``set_input_size`` and the resizing load against the
reference-generated fixture tests/golden/posembed_tiny.npz (tests/golden/make_golden_posembed.py: a tiny OpenVision model at 64, 96 and
128 px, L = 17, 37 and 65 tokens; on the reference every wrong table -- tiled, transposed, zero, bilinear -- moves the compared quantity
by at least 5 x COS_TOL), hipGraph replay across a resize, and stage-2 training with a fixed table: no gradient and no optimiser slot
for it, every other gradient bitwise."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openvision_amd import checkpoint, posembed, synth, training
from openvision_amd.loss import ClipLoss
from openvision_amd.model import create_model
from test_gpu_model import COS_TOL
from test_posembed_cpu import WIDTH, fixture_images, rand_table, state_dict_with, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_COS = 0.9998                  # what tests/test_gpu_stock.py reached for the same parameter list


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "posembed_tiny.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def images():
    return {s: fixture_images(s).to(DEV) for s in (64, 96, 128)}


def one_minus_cos(a, b):
    return float((1 - F.cosine_similarity(a.double().cpu(), torch.as_tensor(np.asarray(b, dtype=np.float32)).double(), dim=-1)).max())


def model_at_64(g, name):
    """The fixture's two models as built for stage 1: 'fixed' = pos_embed_type 'sin_cos_2d'; 'resized' = a learnable random table."""
    if name == "fixed":
        return create_model(tiny_cfg(64, "sin_cos_2d"), device=DEV, state_dict=state_dict_with(torch.from_numpy(g["mae/4"]), variant=str(g["variant"])))
    return create_model(tiny_cfg(64), device=DEV, state_dict=state_dict_with(rand_table("g4", 17), variant=str(g["variant"])))


def features_and_tokens(m, x):
    feats = m.encode_image(x)
    m.visual.output_tokens = True
    try:
        pooled, tokens = m.visual(x)
    finally:
        m.visual.output_tokens = False
    return feats, pooled, tokens


def check_against_fixture(g, name, size, m, x):
    feats, pooled, tokens = features_and_tokens(m, x)
    df, dp, dt = (one_minus_cos(feats, g[f"features/{name}/{size}"]), one_minus_cos(pooled, g[f"features/{name}/{size}"]),
                  one_minus_cos(tokens, g[f"tokens/{name}/{size}"]))
    quantity = str(g[f"quantity/{name}/{size}"])
    print(f"{name} @ {size}: 1 - cos to the reference: features {df:.3e}, visual(x) pooled {dp:.3e}, patch tokens {dt:.3e} (fixture names the {quantity})")
    assert tokens.shape == (3, (size // 16) ** 2, WIDTH)
    assert {"features": max(df, dp), "tokens": dt}[quantity] < COS_TOL
    assert df < COS_TOL and dp < COS_TOL and dt < COS_TOL
    return feats, pooled, tokens


def direct_model(m, size):
    """A model built directly at `size` from m's state dict."""
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return create_model(tiny_cfg(size, m.visual.pos_embed_type), device=DEV, state_dict=sd)


# ---- 1. inference at new sizes -----------------------------------------------------------------------------------------------------
def test_fixed_table_model_at_new_sizes(g, images):
    m = model_at_64(g, "fixed")
    m.encode_image(images[64])
    for size in (96, 128):                                                     # 64 -> 96 -> 128 on one model
        m.set_input_size(size)
        assert m.visual.positional_embedding.is_cuda and not m.visual.positional_embedding.requires_grad
        got = check_against_fixture(g, "fixed", size, m, images[size])
        want = features_and_tokens(direct_model(m, size), images[size])
        assert all(torch.equal(a, b) for a, b in zip(got, want)), size
        with pytest.raises(ValueError, match=f"3,{size},{size}"):
            m.encode_image(images[64])
        with pytest.raises(ValueError, match=f"3,{size},{size}"):
            m.visual(images[size - 32])


@pytest.mark.parametrize("size", [96, 128])
def test_learnable_table_model_at_a_new_size(g, images, size):
    m = model_at_64(g, "resized")
    m.encode_image(images[64])
    m.set_input_size(size)
    assert m.visual.positional_embedding.is_cuda and m.visual.positional_embedding.requires_grad
    d = float((m.visual.positional_embedding.detach().cpu() - torch.from_numpy(g[f"resized/4to{size // 16}"])).abs().max())
    assert d <= 256 * 2.0 ** -24 * float(np.abs(g["rand/4"]).max())
    got = check_against_fixture(g, "resized", size, m, images[size])
    want = features_and_tokens(direct_model(m, size), images[size])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match=f"3,{size},{size}"):
        m.encode_image(images[64])
    with pytest.raises(ValueError, match=f"3,{size},{size}"):
        training.encode_image(m, images[64])


# ---- 2. the load path --------------------------------------------------------------------------------------------------------------
def test_from_pretrained_at_a_new_size_is_set_input_size(g, images, tmp_path):
    for name, kind in (("resized", None), ("fixed", "sin_cos_2d")):
        m = model_at_64(g, name)
        path = str(tmp_path / name)
        checkpoint.save_pretrained(m, tiny_cfg(64), path, safetensors=False)   # the config says 'learnable', as converted ones do
        loaded, _ = checkpoint.from_pretrained(path, device=DEV, force_image_size=96, pos_embed_type=kind)
        m.set_input_size(96)
        assert loaded.visual.image_size == (96, 96) and loaded.visual.pos_embed_type == m.visual.pos_embed_type
        assert torch.equal(loaded.visual.positional_embedding, m.visual.positional_embedding)
        assert loaded.visual.positional_embedding.requires_grad == (kind is None)
        got, want = features_and_tokens(loaded, images[96]), features_and_tokens(m, images[96])
        assert all(torch.equal(a, b) for a, b in zip(got, want)), name
        assert one_minus_cos(got[2], g[f"tokens/{name}/96"]) < COS_TOL


# ---- 3. hipGraph replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixed", "resized"])
def test_graph_replay_across_a_resize(g, images, name):
    m = model_at_64(g, name)
    plain64 = m.encode_image(images[64])
    m.use_graphs(4)
    assert torch.equal(m.encode_image(images[64]), plain64)                    # captured
    assert torch.equal(m.encode_image(images[64]), plain64)                    # replayed
    assert len(m._graphs.graphs) == 1
    m.set_input_size(96)
    g96 = m.encode_image(images[96])                                           # the 64 px graph is dropped, a 96 px one captured
    assert torch.equal(m.encode_image(images[96]), g96) and len(m._graphs.graphs) == 1
    with pytest.raises(ValueError):
        m.encode_image(images[64])
    m.use_graphs(0)
    assert torch.equal(m.encode_image(images[96]), g96)                        # the plain call
    assert one_minus_cos(g96, g[f"features/{name}/96"]) < COS_TOL
    if name == "fixed":                                                        # and back: the regenerated table is the first one bitwise
        m.use_graphs(4)
        m.set_input_size(64)
        assert torch.equal(m.encode_image(images[64]), plain64) and torch.equal(m.encode_image(images[64]), plain64)
        m.use_graphs(0)


# ---- 4. training, stage 2 ----------------------------------------------------------------------------------------------------------
def _step(m, img, tok, seed=11):
    torch.manual_seed(seed)                                                    # patch dropout draws from the CPU default generator
    m.zero_grad(set_to_none=True)
    fi, ft, s = training.clip_forward(m, img, tok)
    loss = ClipLoss()(fi, ft, s)
    loss.backward()
    return fi.detach(), ft.detach(), float(loss.detach()), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_training_step_at_96_against_the_reference(g, images):
    """clip_forward + ClipLoss + backward at 96 on the model whose random grid-4 table set_input_size resampled: features under COS_TOL,
    the loss within 2e-2 (tests/test_gpu_stock.py), every stored gradient at cosine >= 0.9998."""
    tok = torch.from_numpy(g["tokens"]).to(DEV)
    m = model_at_64(g, "resized")
    m.set_input_size(96)
    m.train()
    fi, ft, loss, got = _step(m, images[96], tok)
    assert one_minus_cos(fi, g["train_image_features"]) < COS_TOL and one_minus_cos(ft, g["train_text_features"]) < COS_TOL
    print(f"loss {loss:.5f}, reference {float(g['loss']):.5f}")
    assert abs(loss - float(g["loss"])) < 2e-2
    names = [k[5:] for k in g.files if k.startswith("grad/")]
    assert len(names) == 8 and "visual.positional_embedding" in names and "visual.conv1.weight" in names
    assert got["visual.positional_embedding"].shape == (37, WIDTH)
    worst = 1.0
    for name in names:
        r = torch.from_numpy(g["grad/" + name].astype(np.float32))
        gg = got[name].float().cpu()
        cos = float((gg.double() * r.double()).sum() / (gg.double().norm() * r.double().norm() + 1e-30))
        print(f"{name}: cos {cos:.6f}, norm {float(gg.norm()):.4e} / reference {float(r.norm()):.4e}")
        worst = min(worst, cos)
    assert worst >= GRAD_COS, worst
    assert len(got) == len(list(m.parameters()))


def _pair_at_96(patch_dropout=0.0):
    """The same stage-2 model twice: with the recipe's fixed table ('sincos2d'), and with a learnable table of the same values that is
    merely frozen."""
    cfgs = [tiny_cfg(64, "sincos2d"), tiny_cfg(64)]
    for c in cfgs:
        c["vision_cfg"]["patch_dropout"] = patch_dropout
    sd = state_dict_with(posembed.sincos_2d_openvision(4, 4, WIDTH))
    fixed = create_model(cfgs[0], device=DEV, state_dict=sd)
    fixed.set_input_size(96)
    sd96 = state_dict_with(posembed.sincos_2d_openvision(6, 6, WIDTH), 96)
    learn = create_model({**cfgs[1], "vision_cfg": {**cfgs[1]["vision_cfg"], "image_size": 96}}, device=DEV, state_dict=sd96)
    learn.visual.positional_embedding.requires_grad_(False)
    assert torch.equal(fixed.visual.positional_embedding, learn.visual.positional_embedding)
    return fixed.train(), learn.train()


@pytest.mark.parametrize("mode", ["plain", "remat", "patch_dropout"])
def test_fixed_table_takes_no_gradient_and_no_update(g, images, mode):
    """With a fixed table positional_embedding.grad is None and every other gradient is bitwise that of the same model with a learnable
    table under requires_grad_(False); two FusedAdamW steps leave the table bitwise unchanged and move the other parameters.  Also
    under activation recomputation, and with patch_dropout = 0.5 (K = 18 of 36 patches)."""
    tok = torch.from_numpy(g["tokens"]).to(DEV)
    fixed, learn = _pair_at_96(0.5 if mode == "patch_dropout" else 0.0)
    if mode == "remat":
        fixed.set_grad_checkpointing()
        learn.set_grad_checkpointing()
    if mode == "patch_dropout":
        assert fixed.visual.dropout_active() and fixed.visual.patch_dropout.num_keep(fixed.visual.num_patches) == 18
    fa, ta, la, ga = _step(fixed, images[96], tok)
    fb, tb, lb, gb = _step(learn, images[96], tok)
    assert fixed.visual.positional_embedding.grad is None and "visual.positional_embedding" not in ga
    assert torch.equal(fa, fb) and torch.equal(ta, tb) and la == lb
    assert sorted(ga) == sorted(gb) and len(ga) == len(list(fixed.parameters())) - 1
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    if mode == "plain":                                                        # and the table, were it trained, WOULD get a gradient
        learn.visual.positional_embedding.requires_grad_(True)
        assert float(_step(learn, images[96], tok)[3]["visual.positional_embedding"].abs().max()) > 0
    table = fixed.visual.positional_embedding.detach().clone()
    before = {n: p.detach().clone() for n, p in fixed.named_parameters()}
    opt = training.FusedAdamW(fixed, lr=1e-3)
    assert "visual.positional_embedding" not in [n for grp in opt.groups for n, _ in grp["params"]]
    for i in range(2):
        opt.zero_grad()
        torch.manual_seed(20 + i)
        loss = ClipLoss()(*training.clip_forward(fixed, images[96], tok))
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss))
    torch.cuda.synchronize()
    assert torch.equal(fixed.visual.positional_embedding, table) and torch.equal(table, posembed.sincos_2d_openvision(6, 6, WIDTH).to(DEV))
    moved = [n for n, p in fixed.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) == len(before) - 1 and "visual.positional_embedding" not in moved


# ---- 5. two stages end to end ------------------------------------------------------------------------------------------------------
def test_two_stages_end_to_end(g, images, tmp_path):
    tok = torch.from_numpy(g["tokens"]).to(DEV)
    cfg = tiny_cfg(64, "sincos2d")
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg)).train()

    def steps(model, img):
        opt = training.FusedAdamW(model, lr=1e-3)                              # the optimiser of a stage is built after the resize
        losses = []
        for _ in range(2):
            opt.zero_grad()
            loss = ClipLoss()(*training.clip_forward(model, img, tok))
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses

    l1 = steps(m, images[64])
    path = str(tmp_path / "stage1")
    checkpoint.save_pretrained(m, tiny_cfg(64), path, safetensors=False)       # handed on with a config that says 'learnable'
    m2, _ = checkpoint.from_pretrained(path, device=DEV, force_image_size=96, pos_embed_type="sincos2d")
    want = posembed.sincos_2d_openvision(6, 6, WIDTH).to(DEV)
    assert torch.equal(m2.visual.positional_embedding, want) and not m2.visual.positional_embedding.requires_grad
    for n, p in m.named_parameters():                                          # everything else is stage 1's
        assert n == "visual.positional_embedding" or torch.equal(dict(m2.named_parameters())[n], p.detach()), n
    l2 = steps(m2.train(), images[96])
    print("stage 1 losses", l1, "stage 2 losses", l2)
    assert all(np.isfinite(l1 + l2))
    assert torch.equal(m2.visual.positional_embedding, want)
    assert m2.encode_image(images[96]).isfinite().all()
