"""CPU: multi-stage resolution on the host side -- the fixed sin-cos position tables and the resizers of ``openvision_amd.posembed``
against the reference-generated fixture tests/golden/posembed_tiny.npz (tests/golden/make_golden_posembed.py), ``pos_embed_type`` in
the config, the fixed table in the model (frozen, in the state dict, never unlocked, no optimiser slot), ``set_input_size`` and the
resizing load.  No kernel runs."""
import hashlib
import json
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openvision_amd import checkpoint, config as ovcfg, convert_jax, posembed, preset, synth, training
from openvision_amd.model import create_model

WIDTH, PATCH, T, VOCAB = 192, 16, 80, 1000


def tiny_cfg(size=64, pos_embed_type=None):
    """The fixture's model (make_golden_posembed.config): the OpenVision shape at width 192, two layers per tower."""
    v = {"image_size": size, "patch_size": PATCH, "width": WIDTH, "head_width": 64, "layers": 2, "mlp_ratio": 4.0, "pool_type": "avg",
         "final_ln_after_pool": True, "no_ln_pre": True}
    if pos_embed_type is not None:
        v["pos_embed_type"] = pos_embed_type
    return {"embed_dim": 64, "vision_cfg": v,
            "text_cfg": {"context_length": T, "vocab_size": VOCAB, "width": WIDTH, "heads": 3, "layers": 2, "mlp_ratio": 4.0,
                         "pool_type": "last", "no_causal_mask": True, "act_kwargs": {"approximate": "tanh"}}}


def rand_table(name, rows, width=WIDTH):
    """make_golden_posembed.rand_table: name-seeded N(0, 0.5^2)."""
    return synth._normal("posembed." + name, (rows, width), 0.5, 0)


def fixture_images(size):
    """make_golden_posembed.images: three structured images at 128 px rounded to fp16; smaller sizes are their top left corner."""
    return synth.make_structured_images(3, 128, seed=3).half().float()[:, :, :size, :size].contiguous()


def state_dict_with(table, size=64, variant="v1"):
    sd = synth.make_state_dict(tiny_cfg(size), 0, variant)
    sd["visual.positional_embedding"] = table.clone()
    return sd


def visual_ns(g):
    return types.SimpleNamespace(visual=types.SimpleNamespace(grid_size=(g, g)))


def resized(table, g, **kw):
    sd = {"visual.positional_embedding": table.clone()}
    posembed.resize_pos_embed(sd, visual_ns(g), **kw)
    return sd["visual.positional_embedding"]


@pytest.fixture(scope="module")
def g(gold):
    return gold("posembed_tiny.npz")


# ---- the fixture is the one this file describes ------------------------------------------------------------------------------------
def test_fixture_is_for_this_model_and_these_inputs(g):
    assert json.loads(str(g["config_json"])) == tiny_cfg()
    assert torch.equal(torch.from_numpy(g["rand/4"]), rand_table("g4", 17)) and torch.equal(torch.from_numpy(g["rand/6"]), rand_table("g6", 37))
    for size in (96, 128):
        img = fixture_images(size).double()
        np.testing.assert_allclose([float(img.sum()), float(img.abs().sum())], g[f"images_checksum/{size}"], rtol=1e-6)
        for name in ("fixed", "resized"):
            assert str(g[f"quantity/{name}/{size}"]) in ("features", "tokens")
            assert g[f"tokens/{name}/{size}"].shape == (3, (size // PATCH) ** 2, WIDTH)


# ---- the tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [4, 6, 8])
def test_mae_table_is_the_references(g, grid):
    """Both sides are float64 evaluations rounded to fp32 of values of magnitude <= 1: two libm builds differ by at most one double
    ulp, which can move the fp32 rounding by one unit, 2^-23 at most."""
    got = posembed.sincos_2d_mae(WIDTH, grid)
    want = torch.from_numpy(g[f"mae/{grid}"])
    assert got.dtype == torch.float32 and got.shape == want.shape == (1 + grid * grid, WIDTH)
    d = float((got - want).abs().max())
    print(f"grid {grid}: max |delta| {d:.3e}")
    assert d <= 2.0 ** -23
    assert not got[0].any()                                                    # class row zeros


def test_openvision_table_is_the_converters_bitwise():
    for h, w in ((4, 4), (6, 6), (3, 5)):
        got = posembed.sincos_2d_openvision(h, w, WIDTH)
        assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(convert_jax.posemb_sincos_2d(h, w, WIDTH)))
    sd = convert_jax.jax_to_open_clip({"img/cls": np.zeros((1, 1, WIDTH), np.float32)}, grid=(4, 4))
    assert torch.equal(sd["visual.positional_embedding"], posembed.sincos_2d_openvision(4, 4, WIDTH))      # what a checkpoint carries


def test_the_two_forms_are_different_tables():
    d = float((posembed.sincos_2d_mae(WIDTH, 4) - posembed.sincos_2d_openvision(4, 4, WIDTH)).abs().max())
    print(f"MAE form against MoCo-v3 form at grid 4: max |delta| {d:.4f}")
    assert d > 1e-2
    # ... while fp32 and fp64 evaluations of ONE form stay far inside the loader's 1e-3
    assert float((synth.posemb_sincos_2d(16, 16, WIDTH) - posembed.sincos_2d_openvision(16, 16, WIDTH)).abs().max()) < 1e-4
    for width in (190, 194):
        with pytest.raises(ValueError):
            posembed.sincos_2d_mae(width, 4)
        with pytest.raises(ValueError):
            posembed.sincos_2d_openvision(4, 4, width)


# ---- the resizers ------------------------------------------------------------------------------------------------------------------
def _bound(table):
    """The same fp32 sums in possibly another order: at most 8 x 8 taps at these sizes, absolute weight sum below 4."""
    return 256 * 2.0 ** -24 * float(table.abs().max())


@pytest.mark.parametrize("src,dst", [(4, 6), (4, 8), (6, 4)])
def test_resize_pos_embed_against_the_reference(g, src, dst):
    table = torch.from_numpy(g[f"rand/{src}"])
    want = torch.from_numpy(g[f"resized/{src}to{dst}"])
    got = resized(table, dst)
    d = float((got - want).abs().max())
    print(f"{src} -> {dst}: max |delta| {d:.3e}, bound {_bound(table):.3e}")
    assert got.shape == want.shape == (1 + dst * dst, WIDTH) and d <= _bound(table)
    assert torch.equal(got[0], table[0])                                       # the class row is untouched


def test_other_interpolation_kinds_lie_outside_the_bound(g):
    """Kernels that differ by design are orders above the bound: the comparison above tells them apart."""
    r4, r6 = torch.from_numpy(g["rand/4"]), torch.from_numpy(g["rand/6"])
    for table, src, dst, kw in ((r4, 4, 6, dict(antialias=False)), (r4, 4, 6, dict(interpolation="bilinear")),
                                (r6, 6, 4, dict(antialias=False))):
        want = torch.from_numpy(g[f"resized/{src}to{dst}"])
        d = float((resized(table, dst, **kw) - want).abs().max())
        print(f"{src} -> {dst} with {kw}: max |delta| {d:.3e}, bound {_bound(table):.3e}")
        assert d > 100 * _bound(table)
    # bicubic without antialias differs when enlarging too: antialias=True is not a no-op upwards in torch
    assert float((resized(r4, 8, antialias=False) - torch.from_numpy(g["resized/4to8"])).abs().max()) > 100 * _bound(r4)


@pytest.mark.parametrize("src,dst", [(80, 48), (48, 80)])
def test_resize_text_pos_embed_against_the_reference(g, src, dst):
    table = torch.from_numpy(g[f"text/{src}"])
    want = torch.from_numpy(g[f"text/{src}to{dst}"])
    sd = {"positional_embedding": table.clone()}
    posembed.resize_text_pos_embed(sd, types.SimpleNamespace(positional_embedding=torch.empty(dst, table.shape[1])))
    got = sd["positional_embedding"]
    d = float((got - want).abs().max())
    print(f"text {src} -> {dst}: max |delta| {d:.3e}, bound {_bound(table):.3e}")
    assert got.shape == want.shape and d <= _bound(table)
    nearest = table[(torch.arange(dst) * src) // dst]                          # picking rows in place of linear is another table
    assert float((nearest - want).abs().max()) > 100 * _bound(table)


def test_resizers_early_returns_and_errors():
    t = rand_table("g4", 17)
    sd = {"visual.positional_embedding": t, "positional_embedding": rand_table("t80", 80, 32)}
    before = dict(sd)
    posembed.resize_pos_embed(sd, visual_ns(4))                                # equal sizes: the dict keeps the very same objects
    posembed.resize_text_pos_embed(sd, types.SimpleNamespace(positional_embedding=torch.empty(80, 32)))
    assert all(sd[k] is before[k] for k in before) and len(sd) == 2
    empty = {}
    posembed.resize_pos_embed(empty, visual_ns(6))
    posembed.resize_text_pos_embed(empty, types.SimpleNamespace(positional_embedding=torch.empty(48, 32)))
    assert empty == {}
    posembed.resize_pos_embed(sd, types.SimpleNamespace(visual=types.SimpleNamespace()))       # a tower without a grid (timm): untouched
    assert sd["visual.positional_embedding"] is t
    for rows in (16, 19, 13):                                                  # 15, 18, 12 patch rows: no square
        with pytest.raises(ValueError, match="square"):
            posembed.resize_pos_embed({"visual.positional_embedding": torch.zeros(rows, 8)}, visual_ns(6))


# ---- config ------------------------------------------------------------------------------------------------------------------------
PRESET_DIGESTS = {"vit-tiny-patch16-160": "55c62face848fb5c", "vit-small-patch8-384": "4ef24b003261d20d",
                  "vit-base-patch16-224": "bfa7fc9bef09e81c", "vit-large-patch14-224": "2e16d572414d9499",
                  "vit-so400m-patch14-224": "411ac79cb9324bb7", "vit-huge-patch14-224": "956cf45a73bce7c2"}


def test_config_honours_pos_embed_type():
    v = tiny_cfg()["vision_cfg"]
    assert ovcfg.vision_cfg_from(v).pos_embed_type == "learnable"
    for kind in ("learnable", "sin_cos_2d", "sincos2d"):
        assert ovcfg.vision_cfg_from({**v, "pos_embed_type": kind}).pos_embed_type == kind
    for bad in ("sincos", "sin_cos_1d", "", None):
        with pytest.raises(ValueError, match="learnable.*sin_cos_2d.*sincos2d"):
            ovcfg.vision_cfg_from({**v, "pos_embed_type": bad})
    for kind in ("sin_cos_2d", "sincos2d"):                                    # width 66 = 33 * 2: a multiple of head_width 33, not of 4
        with pytest.raises(ValueError, match="multiple of 4"):
            ovcfg.vision_cfg_from({**v, "width": 66, "head_width": 33, "pos_embed_type": kind})
    assert ovcfg.vision_cfg_from({**v, "width": 66, "head_width": 33}).width == 66


def test_presets_are_as_they_were_and_the_keyword_adds_one_key():
    assert sorted(ovcfg.PRESETS) == sorted(PRESET_DIGESTS)
    for name, digest in PRESET_DIGESTS.items():
        cfg = preset(name)
        assert "pos_embed_type" not in cfg["vision_cfg"]
        assert hashlib.sha256(json.dumps(cfg, sort_keys=True).encode()).hexdigest()[:16] == digest, name
    plain = ovcfg.openvision_model_cfg("Ti", 16, 160)
    assert plain == preset("vit-tiny-patch16-160")
    for kind in ("learnable", "sin_cos_2d", "sincos2d"):
        got = ovcfg.openvision_model_cfg("Ti", 16, 160, pos_embed_type=kind)
        assert got["vision_cfg"].pop("pos_embed_type") == kind and got == plain
    with pytest.raises(ValueError):
        ovcfg.openvision_model_cfg("Ti", 16, 160, pos_embed_type="fixed")


# ---- the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sin_cos_2d", "sincos2d"])
def test_fixed_table_in_the_model(kind):
    learn = create_model(tiny_cfg())
    m = create_model(tiny_cfg(pos_embed_type=kind))
    pos = m.visual.positional_embedding
    assert isinstance(pos, torch.nn.Parameter) and not pos.requires_grad and learn.visual.positional_embedding.requires_grad
    assert torch.equal(pos, posembed.fixed_table(kind, 4, WIDTH))
    assert list(m.state_dict()) == list(learn.state_dict()) and "visual.positional_embedding" in m.state_dict()
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in learn.named_parameters()]
    # LiT locking never trains it again, however many groups are unlocked; the learnable one comes back with its group
    groups = len(m.visual._lock_groups())
    assert groups == len(learn.visual._lock_groups()) == 2 + 2
    for k in (1, groups - 1, groups, groups + 3):
        m.lock_image_tower(k)
        assert not m.visual.positional_embedding.requires_grad
    assert all(p.requires_grad for n, p in m.named_parameters() if n != "visual.positional_embedding")
    learn.lock_image_tower(groups)
    assert learn.visual.positional_embedding.requires_grad
    # the optimiser filters on requires_grad: no slot, no moments for the table
    opt = training.FusedAdamW(m, lr=1e-3)
    names = [n for grp in opt.groups for n, _ in grp["params"]]
    assert "visual.positional_embedding" not in names and len(names) == len(list(m.parameters())) - 1
    assert "visual.positional_embedding" in [n for grp in training.FusedAdamW(learn, lr=1e-3).groups for n, _ in grp["params"]]
    assert torch.equal(m.visual.positional_embedding, posembed.fixed_table(kind, 4, WIDTH)) and m.visual.positional_embedding.grad is None


def test_fixed_model_loads_a_reference_shaped_state_dict_strictly(g):
    """The reference keeps the fixed table in the state dict (a Parameter with requires_grad=False): such a dict loads strictly, and
    the table it carries is what the model then holds, as in the reference."""
    sd = state_dict_with(torch.from_numpy(g["mae/4"]))
    m = create_model(tiny_cfg(pos_embed_type="sin_cos_2d"), state_dict=sd)
    assert torch.equal(m.visual.positional_embedding, sd["visual.positional_embedding"]) and not m.visual.positional_embedding.requires_grad
    with pytest.raises(RuntimeError, match="positional_embedding"):            # another grid without the resizing load: strict as ever
        create_model(tiny_cfg(96, "sin_cos_2d"), state_dict=sd)
    sd.pop("visual.positional_embedding")
    with pytest.raises(RuntimeError, match="positional_embedding"):
        create_model(tiny_cfg(pos_embed_type="sin_cos_2d"), state_dict=sd)


@pytest.mark.parametrize("kind", ["sin_cos_2d", "sincos2d"])
def test_set_input_size_regenerates_a_fixed_table(kind):
    m = create_model(tiny_cfg(pos_embed_type=kind))
    direct = create_model(tiny_cfg(96, kind))
    old = m.visual.positional_embedding
    m.set_input_size(96)
    v = m.visual
    assert v.image_size == (96, 96) and v.grid_size == (6, 6) and v.num_patches == 36 and m.vision_cfg.image_size == 96
    assert v.positional_embedding is not old and isinstance(v.positional_embedding, torch.nn.Parameter)
    assert not v.positional_embedding.requires_grad and torch.equal(v.positional_embedding, direct.visual.positional_embedding)
    assert list(m.state_dict()) == list(direct.state_dict())
    m.set_input_size(64)
    assert torch.equal(m.visual.positional_embedding, old) and m.visual.grid_size == (4, 4)


def test_set_input_size_resamples_a_learnable_table(g):
    r4 = torch.from_numpy(g["rand/4"])
    m = create_model(tiny_cfg(), state_dict=state_dict_with(r4))
    m.visual.positional_embedding.requires_grad_(False)                        # the new Parameter inherits the flag ...
    m.set_input_size(96)
    assert torch.equal(m.visual.positional_embedding, resized(r4, 6)) and not m.visual.positional_embedding.requires_grad
    assert float((m.visual.positional_embedding - torch.from_numpy(g["resized/4to6"])).abs().max()) <= _bound(r4)
    m = create_model(tiny_cfg(), state_dict=state_dict_with(r4))
    m.set_input_size(128)
    assert torch.equal(m.visual.positional_embedding, resized(r4, 8)) and m.visual.positional_embedding.requires_grad   # ... either way
    assert m.visual.image_size == (128, 128) and m.visual.grid_size == (8, 8)
    same = m.visual.positional_embedding
    m.set_input_size(128)                                                      # nothing to do: the table stays the same object
    assert m.visual.positional_embedding is same
    for bad in (100, 0, -16, 96.0, (96, 96), True):
        with pytest.raises(ValueError, match="multiple of the patch size"):
            m.set_input_size(bad)
    assert m.visual.image_size == (128, 128)


def test_training_encode_image_names_the_size_mismatch():
    m = create_model(tiny_cfg())
    with pytest.raises(ValueError, match=r"\[B,3,64,64\].*set_input_size"):
        training.encode_image(m, torch.zeros(2, 3, 96, 96))
    m.set_input_size(96)
    with pytest.raises(ValueError, match=r"\[B,3,96,96\]"):
        training.encode_image(m, torch.zeros(2, 3, 64, 64))


# ---- the resizing load -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saved_dir(tmp_path_factory):
    """A directory written by save_pretrained at 64: synth weights, whose image table is the recipe's (MoCo-v3 form, fp64-evaluated),
    and a config that says nothing about it ('learnable'), as converted OpenVision checkpoints do."""
    path = str(tmp_path_factory.mktemp("posembed") / "tiny64")
    cfg = tiny_cfg()
    checkpoint.save_pretrained(create_model(cfg, state_dict=synth.make_state_dict(cfg)), cfg, path, safetensors=False)
    return path


def test_from_pretrained_at_another_size(saved_dir):
    sd = synth.make_state_dict(tiny_cfg())
    m, _ = checkpoint.from_pretrained(saved_dir, device=None)                  # as before
    assert m.visual.image_size == (64, 64) and torch.equal(m.visual.positional_embedding, sd["visual.positional_embedding"])
    assert m.visual.positional_embedding.requires_grad and not m.training
    m, _ = checkpoint.from_pretrained(saved_dir, device=None, force_image_size=96)
    assert m.visual.image_size == (96, 96) and m.visual.grid_size == (6, 6) and m.visual.positional_embedding.requires_grad
    assert torch.equal(m.visual.positional_embedding, resized(sd["visual.positional_embedding"], 6))
    for k, v in m.state_dict().items():
        assert k == "visual.positional_embedding" or torch.equal(v, sd[k]), k
    m, _ = checkpoint.from_pretrained(saved_dir, device=None, force_image_size=96, pos_embed_type="sincos2d")
    assert m.visual.pos_embed_type == "sincos2d" and not m.visual.positional_embedding.requires_grad
    assert torch.equal(m.visual.positional_embedding, posembed.sincos_2d_openvision(6, 6, WIDTH))           # regenerated, not resampled
    with pytest.raises(ValueError, match="another form"):
        checkpoint.from_pretrained(saved_dir, device=None, force_image_size=96, pos_embed_type="sin_cos_2d")
    m, _ = checkpoint.from_pretrained(saved_dir, device=None, pos_embed_type="sincos2d")                    # same grid: the checkpoint's table
    assert torch.equal(m.visual.positional_embedding, sd["visual.positional_embedding"]) and not m.visual.positional_embedding.requires_grad


def test_create_model_resizes_only_when_asked(saved_dir):
    sd = checkpoint.read_state_dict(saved_dir)
    with pytest.raises(RuntimeError, match="size mismatch"):
        create_model(tiny_cfg(96), state_dict=sd)
    with pytest.raises(RuntimeError, match="size mismatch"):
        create_model(tiny_cfg(96), state_dict=sd, resize_pos_embed=False)
    keep = sd["visual.positional_embedding"]
    m = create_model(tiny_cfg(96), state_dict=sd, resize_pos_embed=True)
    assert sd["visual.positional_embedding"] is keep and keep.shape[0] == 17   # the caller's dict is not changed
    assert torch.equal(m.visual.positional_embedding, resized(keep, 6))
    # a trained (here: random) table under a fixed type is refused, not silently replaced
    with pytest.raises(ValueError, match="trained one"):
        create_model(tiny_cfg(96, "sincos2d"), state_dict=state_dict_with(rand_table("g4", 17)), resize_pos_embed=True)
    # the text table: linear, to the model's context length
    cfg = tiny_cfg(96)
    cfg["text_cfg"]["context_length"] = 48
    m = create_model(cfg, state_dict=sd, resize_pos_embed=True)
    want = F.interpolate(sd["positional_embedding"].t()[None], size=48, mode="linear", align_corners=False)[0].t()
    assert m.positional_embedding.shape == (48, WIDTH) and torch.equal(m.positional_embedding, want)
