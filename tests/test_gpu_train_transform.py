"""GPU: openvision_amd.augment.train_transform (csrc/augment.hip) bit for bit against the host planner, the existing preprocess, the
numpy restatement (tests/train_transform_restate.py) and Pillow's committed outputs (tests/golden/train_transform.npz)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import train_transform_restate as T
from conftest import golden
from openvision_amd import _lib, augment as A
from openvision_amd.config import DEFAULT_PREPROCESS as PP
from openvision_amd.preprocess import preprocess, resize_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = PP["mean"], PP["std"]
S = 32
NO_OPS = (np.zeros(4, np.int32), np.zeros(4, np.float32))


def ops_of(*chain):
    """(op, factor) pairs -> one row of ops int32 [4] and factors float32 [4]"""
    o, f = np.zeros(4, np.int32), np.zeros(4, np.float32)
    for k, (op, factor) in enumerate(chain):
        o[k], f[k] = op, factor
    return o, f


def run(images, boxes, chains, interp="bicubic", size=S, dtype=torch.float32):
    ops = (np.stack([c[0] for c in chains]), np.stack([c[1] for c in chains]))
    return A.train_transform(images, size, MEAN, STD, interp, boxes=np.asarray(boxes), color_ops=ops, dtype=dtype, device=DEV)


def restate(images, boxes, chains, interp="bicubic", size=S):
    return np.stack([T.train_transform(im, b, size, interp, c[0], c[1], MEAN, STD) for im, b, c in zip(images, boxes, chains)])


def full(images):
    return [(0, 0, im.shape[0], im.shape[1]) for im in images]


@lru_cache(maxsize=1)
def odd_images():
    """the source shapes of test_device_preprocess_bit_exact"""
    rng = np.random.default_rng(9)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in [(5, 7, 3), (333, 77, 3), (160, 160, 3), (1, 1, 3), (640, 481, 3)]]


@lru_cache(maxsize=1)
def colour_images():
    rng = np.random.default_rng(17)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in [(40, 48, 3), (32, 32, 3), (57, 35, 3)]]


def test_planner_tables_equal_the_host_plan_bitwise():
    lib = _lib.load()
    ext = [1, 5, 31, 32, 33, 77, 333, 640]
    boxes = np.array([[0, 0, ext[i], ext[(i + 3) % 8]] for i in range(8)], np.int32)        # h and w differ: both axes, all extents
    d_boxes = torch.from_numpy(boxes).to(DEV)
    for interp in ("bilinear", "bicubic"):
        kx = ky = max(A.max_taps(e, S, interp) for e in ext)
        bx = torch.full((8, S, 2), -7, dtype=torch.int32, device=DEV)
        by = torch.full((8, S, 2), -7, dtype=torch.int32, device=DEV)
        tx = torch.full((8, S, kx), -7, dtype=torch.int32, device=DEV)
        ty = torch.full((8, S, ky), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.ov_train_transform_plan(_lib.ptr(d_boxes), 8, S, S, A.INTERPOLATION[interp], kx, ky, _lib.ptr(bx), _lib.ptr(tx),
                                               _lib.ptr(by), _lib.ptr(ty), _lib.stream_ptr()), "ov_train_transform_plan")
        bx, by, tx, ty = (t.cpu().numpy() for t in (bx, by, tx, ty))
        for n, (_, _, h, w) in enumerate(boxes.tolist()):
            for extent, b, t in ((w, bx[n], tx[n]), (h, by[n], ty[n])):
                hb, hk, ks = resize_plan(extent, S, interp)
                assert ks <= t.shape[1] and (ks < t.shape[1] or extent == 640)                # the mixed batch pads every other image
                assert np.array_equal(b, hb), (interp, extent)
                assert np.array_equal(t[:, :ks], hk), (interp, extent)
                assert not t[:, ks:].any(), (interp, extent)


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_full_frame_equals_preprocess_bitwise(interp):
    imgs = odd_images()
    got = run(imgs, full(imgs), [NO_OPS] * 5, interp)
    want = preprocess(imgs, S, MEAN, STD, "squash", interp, device=DEV)
    assert got.shape == (5, 3, S, S) and torch.equal(got, want)


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_boxes_equal_the_restatement_bitwise(interp):
    rng = np.random.default_rng(23)
    imgs = odd_images()[:3] + [odd_images()[4], rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)]
    boxes = [(2, 3, 1, 1),                  # a single pixel
             (300, 40, 33, 37),             # touches the bottom-right corner of the 333 x 77 image
             (50, 30, 9, 80),               # strip: up on one axis, down on the other
             (100, 60, 500, 400),           # large crop of the 640 x 481 image
             (0, 0, 40, 56)]                # full frame
    got = run(imgs, boxes, [NO_OPS] * 5, interp).cpu().numpy()
    want = restate(imgs, boxes, [NO_OPS] * 5, interp)
    for n in range(5):
        assert np.array_equal(got[n], want[n]), (interp, boxes[n])


def test_golden_cases_equal_pillow_bitwise():
    g = golden("train_transform.npz")
    for interp in ("bilinear", "bicubic"):                  # one batch per filter
        names = [str(n) for n, i in zip(g["names"], g["interps"]) if str(i) == interp]
        chains = [ops_of(*zip(g[f"{n}_ops"], g[f"{n}_factors"])) for n in names]
        got = run([g[f"{n}_in"] for n in names], [g[f"{n}_box"] for n in names], chains, interp).cpu().numpy()
        for n, o in zip(names, got):
            assert np.array_equal(o, g[f"{n}_out"]), n


def test_colour_operations_equal_the_restatement_bitwise():
    src = colour_images()
    chains = [ops_of((op, f)) for op in (T.BRIGHTNESS, T.CONTRAST, T.SATURATION) for f in (0.0, 0.68, 1.0, 1.32)]
    chains += [ops_of((T.SATURATION, 1.32), (T.BRIGHTNESS, 0.68), (T.CONTRAST, 1.32)),      # contrast last: the statistics pass
               ops_of((T.CONTRAST, 0.68), (T.SATURATION, 1.32), (T.BRIGHTNESS, 1.32)),      # re-applies the two before it
               ops_of((T.BRIGHTNESS, 1.2), (T.CONTRAST, 0.7), (T.SATURATION, 0.5), (T.GRAYSCALE, 0.0)),   # grayscale after jitter
               ops_of((T.GRAYSCALE, 0.0)),
               ops_of((T.CONTRAST, 1.32), (T.GRAYSCALE, 0.0), (T.CONTRAST, 0.68))]          # two contrasts: two statistics passes
    imgs = [src[n % 3] for n in range(len(chains))]
    boxes = [(1, 2, im.shape[0] - 3, im.shape[1] - 2) for im in imgs]
    got = run(imgs, boxes, chains).cpu().numpy()
    want = restate(imgs, boxes, chains)
    for n in range(len(chains)):
        assert np.array_equal(got[n], want[n]), chains[n]
    # only some images carry operations; the others pass through the colour stage unchanged
    some = [chains[12], NO_OPS, chains[5], NO_OPS, NO_OPS]
    got = run(imgs[:5], boxes[:5], some).cpu().numpy()
    assert np.array_equal(got, restate(imgs[:5], boxes[:5], some))
    # no contrast anywhere: the statistics launch is skipped
    plain = [chains[1], chains[9], NO_OPS]
    assert np.array_equal(run(imgs[:3], boxes[:3], plain).cpu().numpy(), restate(imgs[:3], boxes[:3], plain))


def test_saturation_pairs_at_1_32_separate_multiply_and_add():
    """The one case a contracted multiply-add cannot pass: 280 of the 309 (degenerate, pixel) pairs whose byte changes under a fused
    multiply-add at factor 1.32 are in this image (tests/test_train_transform_cpu.py counts them).  256 x 256 in, 256 x 256 out:
    the resize is the identity."""
    img, _ = T.saturation_pairs_image()
    chain = [ops_of((T.SATURATION, 1.32))]
    got = run([img], [(0, 0, 256, 256)], chain, size=256).cpu().numpy()
    want = T.to_tensor_normalize(T.apply_op(img, T.SATURATION, np.float32(1.32)), MEAN, STD)
    assert np.array_equal(got[0], want)


def test_bf16_output_is_the_rounded_fp32_output():
    src = colour_images()
    chains = [ops_of((T.CONTRAST, 1.32), (T.SATURATION, 0.68)), NO_OPS, ops_of((T.GRAYSCALE, 0.0))]
    f32 = run(src, full(src), chains)
    b16 = run(src, full(src), chains, dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and torch.equal(b16, f32.to(torch.bfloat16))


def test_images_are_independent_and_calls_repeat():
    imgs = odd_images()
    boxes = [(1, 2, 3, 4), (10, 5, 300, 70), (0, 0, 160, 160), (0, 0, 1, 1), (7, 9, 600, 450)]
    chains = [ops_of((T.CONTRAST, 1.32)), NO_OPS, ops_of((T.SATURATION, 1.32), (T.CONTRAST, 0.68)), NO_OPS, ops_of((T.BRIGHTNESS, 0.68))]
    batch = run(imgs, boxes, chains)
    again = run(imgs, boxes, chains)
    assert torch.equal(batch, again)
    for n in (0, 2, 4):
        alone = run([imgs[n]], [boxes[n]], [chains[n]])
        assert torch.equal(alone[0], batch[n]), n


def test_chunked_batch_equals_the_whole_batch(monkeypatch):
    imgs = odd_images()
    boxes = [(1, 2, 3, 4), (10, 5, 300, 70), (0, 0, 160, 160), (0, 0, 1, 1), (7, 9, 600, 450)]
    chains = [ops_of((T.CONTRAST, 1.32)), NO_OPS, ops_of((T.SATURATION, 1.32), (T.CONTRAST, 0.68)), NO_OPS, ops_of((T.BRIGHTNESS, 0.68))]
    whole = run(imgs, boxes, chains)
    limit = A.plan_chunks(np.asarray(boxes, np.int32), S, "bicubic")[0][5] // 2
    monkeypatch.setattr(A, "WORKSPACE_LIMIT", limit)
    assert len(A.plan_chunks(np.asarray(boxes, np.int32), S, "bicubic")) > 1
    assert torch.equal(run(imgs, boxes, chains), whole)


def test_drawn_transform_and_image_transform():
    """the drawing path end to end: same seeds, same batch; the evaluation branch is the existing preprocess"""
    import random
    imgs = odd_images()
    cfg = A.AugmentationCfg(scale=(0.4, 1.0), color_jitter=(0.32, 0.32, 0.32, 0.0), color_jitter_prob=0.8, gray_scale_prob=0.2)
    fn = A.image_transform(S, True, MEAN, STD, aug_cfg=cfg, device=DEV)

    def draw():
        torch.manual_seed(2)
        random.seed(2)
        return fn(imgs)
    a, b = draw(), draw()
    assert a.shape == (5, 3, S, S) and torch.isfinite(a).all() and torch.equal(a, b)
    ev = A.image_transform(S, False, MEAN, STD, "squash", "bilinear", device=DEV)(imgs)
    assert torch.equal(ev, preprocess(imgs, S, MEAN, STD, "squash", "bilinear", device=DEV))
