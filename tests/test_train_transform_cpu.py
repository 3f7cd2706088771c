"""CPU: the training image transform's restatement (tests/train_transform_restate.py) against Pillow live and against Pillow's
committed outputs; the host half of openvision_amd.augment (samplers, configuration, chunk planning, argument validation)."""
import ctypes
import random
import warnings

import numpy as np
import pytest
import torch

import train_transform_restate as T
from conftest import golden
from openvision_amd import _lib, augment as A
from openvision_amd.config import DEFAULT_PREPROCESS as PP
from openvision_amd.preprocess import resize_plan

FACTORS = (0.0, 0.3, 0.618, 0.68, 1.0, 1.32, 1.9)
EXTENTS = (1, 5, 31, 32, 33, 77, 333, 640)


def cases():
    g = golden("train_transform.npz")
    return g, [(str(n), str(i)) for n, i in zip(g["names"], g["interps"])]


def test_restatement_matches_committed_pillow_outputs():
    g, names = cases()
    assert len(names) >= 5
    assert any(np.float32(1.32) in g[f"{n}_factors"] for n, _ in names)
    assert list(g["contrast_last_ops"]) == [T.BRIGHTNESS, T.SATURATION, T.CONTRAST] and list(g["jitter_then_gray_ops"])[-1] == T.GRAYSCALE
    for n, interp in names:
        u8 = T.train_transform_u8(g[f"{n}_in"], g[f"{n}_box"], 32, interp, g[f"{n}_ops"], g[f"{n}_factors"])
        assert np.array_equal(u8, g[f"{n}_u8"]), n
        out = T.train_transform(g[f"{n}_in"], g[f"{n}_box"], 32, interp, g[f"{n}_ops"], g[f"{n}_factors"], PP["mean"], PP["std"])
        assert out.dtype == np.float32 and np.array_equal(out, g[f"{n}_out"]), n


def test_restatement_matches_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance
    enhance = {T.BRIGHTNESS: ImageEnhance.Brightness, T.CONTRAST: ImageEnhance.Contrast, T.SATURATION: ImageEnhance.Color}
    g, names = cases()
    for n, interp in names:
        x = g[f"{n}_in"]
        top, left, h, w = (int(v) for v in g[f"{n}_box"])
        flt = Image.BICUBIC if interp == "bicubic" else Image.BILINEAR
        pil = Image.fromarray(x).crop((left, top, left + w, top + h)).resize((32, 32), flt)
        assert np.array_equal(T.train_transform_u8(x, (top, left, h, w), 32, interp), np.asarray(pil)), n
        im = Image.fromarray(x)
        assert np.array_equal(T.luma(x), np.asarray(im.convert("L")))
        for op, cls in enhance.items():
            for f in FACTORS:
                f32 = np.float32(f)
                assert np.array_equal(T.apply_op(x, op, f32), np.asarray(cls(im).enhance(float(f32)))), (n, op, f)


def test_saturation_pairs_image_against_pillow():
    """The image of every reachable (L, channel value) pair: the restatement equals ImageEnhance.Color at 1.32, and the image holds
    pairs on which a fused multiply-add gives another byte, so the GPU test that uses it tells the two apart."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance
    img, reachable = T.saturation_pairs_image()
    f = np.float32(1.32)
    deg = np.repeat(T.luma(img)[..., None], 3, axis=-1)
    assert np.array_equal(T.apply_op(img, T.SATURATION, f), np.asarray(ImageEnhance.Color(Image.fromarray(img)).enhance(float(f))))
    d, p = np.mgrid[0:256, 0:256]
    assert reachable[d == p].all()
    sens = T.fma_sensitive(deg, img, f)
    every = T.fma_sensitive(d.astype(np.uint8), p.astype(np.uint8), f)         # over all 65 536 (degenerate, pixel) pairs
    print(f"pairs present {int(reachable.sum())} of 65536; sensitive to a fused multiply-add at 1.32: {int(every.sum())} pairs, "
          f"{int((every & reachable).sum())} of them present, {int(sens.sum())} channel values of the image")
    assert every.sum() == 309 and (every & reachable).sum() >= 1 and sens.sum() >= 1
    for other in (0.3, 0.68, 1.9):                      # the factors the issue found insensitive stay insensitive on this image
        assert not T.fma_sensitive(deg, img, np.float32(other)).any()


def test_max_taps_formula_equals_resize_plan():
    for interp in ("bilinear", "bicubic"):
        for e in EXTENTS + (9, 80, 400, 500, 481):
            assert A.max_taps(e, 32, interp) == resize_plan(e, 32, interp)[2]
            assert A.max_taps(e, 224, interp) == resize_plan(e, 224, interp)[2]


def test_crop_boxes_lie_inside_the_image():
    torch.manual_seed(5)
    shapes = [(480, 640), (5, 7), (1, 1), (333, 77), (64, 64), (10, 400), (400, 10)] * 6
    for scale in ((0.9, 1.0), (0.4, 1.0), (0.08, 1.0)):
        b = A.sample_crop_boxes(shapes, scale)
        assert b.dtype == np.int32 and b.shape == (len(shapes), 4)
        for (H, W), (top, left, h, w) in zip(shapes, b.tolist()):
            assert 0 < h <= H and 0 < w <= W and 0 <= top <= H - h and 0 <= left <= W - w


def test_crop_box_special_cases():
    torch.manual_seed(1)
    assert A.sample_crop_boxes([(64, 64)] * 4, (1.0, 1.0), (1.0, 1.0)).tolist() == [[0, 0, 64, 64]] * 4
    # 10 x 400 (H x W): every attempt at scale >= 0.9 needs h > 10, so the central crop clamped to ratio <= 4/3 is taken
    state = torch.get_rng_state()
    b = A.sample_crop_boxes([(10, 400)], (0.9, 1.0))[0].tolist()
    assert b == [0, (400 - 13) // 2, 10, 13] and b[3] / b[2] <= 4.0 / 3.0 + 0.05
    torch.set_rng_state(state)
    for _ in range(20):                                  # the fallback consumed exactly ten attempts of two uniforms each
        torch.empty(1).uniform_(0, 1)
    after = torch.get_rng_state()
    torch.set_rng_state(state)
    A.sample_crop_boxes([(10, 400)], (0.9, 1.0))
    assert torch.equal(torch.get_rng_state(), after)
    assert A.sample_crop_boxes([(400, 10)], (0.9, 1.0))[0].tolist() == [(400 - 13) // 2, 0, 13, 10]


def test_same_seed_same_draws():
    def draw():
        torch.manual_seed(11)
        random.seed(11)
        return (A.sample_crop_boxes([(480, 640), (333, 77)] * 3, (0.4, 1.0)),) + A.sample_color_ops(16, (0.4, 0.4, 0.4, 0.0), 0.8, 0.2)
    a, b = draw(), draw()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    ops, factors = a[1], a[2]
    assert ops.shape == (16, 4) and factors.dtype == np.float32
    jittered = (ops[:, :3] != 0).all(axis=1) & (ops[:, :3] != T.GRAYSCALE).all(axis=1)
    assert jittered.any() and not jittered.all()         # p = 0.8 over 16 images
    for o, f in zip(ops[jittered], factors[jittered]):
        assert sorted(o[:3].tolist()) == [T.BRIGHTNESS, T.CONTRAST, T.SATURATION] and ((f[:3] >= 0.6) & (f[:3] <= 1.4)).all()
    assert ((ops == T.GRAYSCALE).sum(axis=1) <= 1).all()


def test_zero_strength_draws_nothing_and_keeps_its_place():
    random.seed(0)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    ops, factors = A.sample_color_ops(1, (0.4, 0.0, 0.4, 0.0), 1.0, None)
    end = torch.get_rng_state()
    torch.set_rng_state(state)
    perm = torch.randperm(4).tolist()
    b = torch.empty(1).uniform_(0.6, 1.4).item()
    s = torch.empty(1).uniform_(0.6, 1.4).item()        # no draw for the contrast in between
    assert torch.equal(torch.get_rng_state(), end)
    want = [(T.BRIGHTNESS, b) if fn == 0 else (T.SATURATION, s) for fn in perm if fn in (0, 2)]
    assert ops[0].tolist() == [w[0] for w in want] + [0, 0]
    assert factors[0, :2].tolist() == [np.float32(w[1]) for w in want]
    # brightness strength above 1: the lower end is clamped at 0
    torch.manual_seed(4)
    _, f = A.sample_color_ops(32, (1.5, 0.0, 0.0), 1.0, None)
    assert (f[:, 0] >= 0).all() and (f[:, 0] <= 2.5).all()


def test_unimplemented_and_unused_configuration():
    with pytest.raises(NotImplementedError, match="hue"):
        A.sample_color_ops(1, (0.4, 0.4, 0.4, 0.1), 0.8, None)
    with pytest.raises(NotImplementedError, match="use_timm"):
        A.AugmentationCfg(use_timm=True)
    with pytest.raises(NotImplementedError, match="use_timm"):
        A.image_transform(224, True, aug_cfg={"use_timm": True})
    for kw in ({"re_prob": 0.25}, {"re_count": 2}, {"ratio": (0.5, 2.0)}):
        with pytest.warns(UserWarning, match="Unused augmentation cfg items"):
            A.AugmentationCfg(**kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cfg = A.AugmentationCfg(color_jitter=(0.32, 0.32, 0.32, 0.0), color_jitter_prob=0.8, gray_scale_prob=0.2)
    assert cfg.scale == (0.9, 1.0) and cfg.ratio is None
    assert callable(A.image_transform(224, False)) and callable(A.image_transform(224, True, aug_cfg=cfg))


def test_boxes_are_checked_on_the_host():
    shapes = np.array([[5, 7], [10, 10]], np.int32)
    A.check_boxes(shapes, np.array([[0, 0, 5, 7], [9, 9, 1, 1]]))
    for bad in ([0, 0, 6, 7], [0, 1, 5, 7], [-1, 0, 2, 2], [0, 0, 0, 3], [2, 2, 3, -1]):
        with pytest.raises(ValueError, match="box"):
            A.check_boxes(shapes, np.array([bad, [0, 0, 10, 10]]))


def test_chunks_cover_the_batch_within_the_limit():
    boxes = np.array([[0, 0, 480, 640]] * 13 + [[0, 0, 33, 20]] * 4, np.int32)
    lib = _lib.load()
    whole = A.plan_chunks(boxes, 224, "bicubic")
    assert [c[:2] for c in whole] == [(0, 17)]
    assert whole[0][2:5] == (480, A.max_taps(640, 224, "bicubic"), A.max_taps(480, 224, "bicubic"))
    assert whole[0][5] == lib.ov_train_transform_workspace_bytes(17, 224, 224, 480, whole[0][3], whole[0][4])
    assert whole[0][5] >= 17 * (480 * 224 * 3 + 224 * 224 * 3 + 4 * 8)
    limit = whole[0][5] // 3
    parts = A.plan_chunks(boxes, 224, "bicubic", limit)
    assert len(parts) > 1 and parts[0][0] == 0 and parts[-1][1] == 17
    assert all(a[1] == b[0] for a, b in zip(parts, parts[1:])) and all(c[5] <= limit for c in parts)
    assert parts[-1][2] == 33 or parts[-1][0] < 13         # a chunk of small crops alone is sized by them
    one = A.plan_chunks(boxes[:2], 224, "bicubic", 1)      # nothing fits: one image per chunk, still run
    assert [c[:2] for c in one] == [(0, 1), (1, 2)]


def test_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.ov_train_transform_workspace_bytes(0, 32, 32, 8, 5, 5) == 0
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    good = [p, 1024, p, p, p, p, p, 1, 32, 32, 8, 1, 5, 5, 0, mean, mean, p, 0, p, 1 << 30, None]
    for i in (0, 2, 3, 4, 5, 6, 15, 16, 17, 19):            # null pointers
        a = list(good)
        a[i] = None
        assert lib.ov_train_transform(*a) == -1, i
    for i, v in ((1, 0), (7, 0), (8, 0), (9, -1), (10, 0), (11, 2), (12, 0), (13, 0), (14, 5), (18, 2), (19, p + 4)):
        a = list(good)                                      # sizes, interpolation, contrast passes, dtype, workspace alignment
        a[i] = v
        assert lib.ov_train_transform(*a) == -1, i
    a = list(good)
    a[20] = 64                                              # workspace too small
    assert lib.ov_train_transform(*a) == -3
    assert lib.ov_train_transform_plan(None, 1, 32, 32, 1, 5, 5, p, p, p, p, None) == -1
    assert lib.ov_train_transform_plan(p, 1, 32, 32, 7, 5, 5, p, p, p, p, None) == -1
    with pytest.raises(_lib.OvhipError):
        A.train_transform([np.zeros((4, 4, 3), np.uint8)], 32, device="cpu")
