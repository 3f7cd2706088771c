"""GPU: the training entry points of the Python package, pinned to recorded results (the companion of test_gpu_block_pinned.py and
test_gpu_encode_pinned.py for openvision_amd.training and openvision_amd.visualize).

Those two files drive the C library directly; what they cannot see is the host code between a module's parameters and the library:
how a block's parameters become the device tensors a tower handle borrows, which handle an autograd node runs and which gradient comes
back under which parameter.  Here every case runs one step of a training entry point on formula inputs (openvision_amd.synth Philox
draws) and hashes (sha256 of the raw bytes) the loss, every parameter gradient by name and the input gradient where there is one; the
digests are compared with tests/golden/train_digests.json, recorded on an MI355X with the package as it was while training.py packed
its own copies of the weights and built a tower handle per node and pass.  The kernels are deterministic and the split-K
plan depends on the CU count only.

The cases are the smallest that reach each branch of the nodes: one node per tower, recomputation, a locked image tower (nothing kept;
and, unlocked further, a partial backward that stops above frozen blocks), several spans per tower, an explicit keep table, frozen
weights under an input gradient, the caption decoder under its prefix mask, the feature objective with and without a lower tower, and
a bare tower at head_dim 80 with a padded MLP.  The two loops built on these paths (visualize.FeatureVisualizer,
gradient_ascent.GradientAscent) run a few seeded iterations each, and what they leave behind is hashed.

A change that is meant to alter the arithmetic of any of these paths regenerates the fixture on purpose:
    python tests/test_gpu_train_pinned.py tests/golden/train_digests.json
and says so; a host-side refactor must pass with the fixture untouched."""
import json
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from openvision_amd import preset, synth, training, visualize  # noqa: E402
from openvision_amd.caption import CaptionLoss, TextDecoder  # noqa: E402
from openvision_amd.gradient_ascent import GradientAscent  # noqa: E402
from openvision_amd.loss import ClipLoss  # noqa: E402
from openvision_amd.model import Transformer, create_model  # noqa: E402
from test_gpu_block_pinned import _draw, _sha, SEED  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(ROOT, "tests", "golden", "train_digests.json")
PRESET = "vit-tiny-patch16-160"
B = 4


def _tiny():
    cfg = preset(PRESET)
    return create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg, seed=SEED)).train()


def _batch():
    return synth.make_images(B, 160, seed=SEED).to(DEV), synth.make_captions(B, seed=SEED).to(DEV)


def _fill(module, tag):
    """Formula weights for a module whose constructor draws from torch's generator: LayerNorm gains around 1, matrices at
    fan_in^-0.5, every other vector small."""
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() == 2:
                p.copy_(_draw(f"{tag}.{n}", tuple(p.shape), p.shape[1] ** -0.5))
            elif n.endswith(("ln_1.weight", "ln_2.weight", "norm.weight")):
                p.copy_(_draw(f"{tag}.{n}", tuple(p.shape), 0.1, 1.0))
            else:
                p.copy_(_draw(f"{tag}.{n}", tuple(p.shape), 0.1))
    return module


def _grads(modules):
    """'grad.<module>.<parameter>' -> digest of .grad ('none' where nothing left a gradient)."""
    return {f"grad.{tag}.{n}": "none" if p.grad is None else _sha(p.grad) for tag, mod in modules for n, p in mod.named_parameters()}


def _digests(loss, modules, inputs=()):
    """loss + '<module>.<parameter>' -> digest of .grad ('none' where the step left no gradient) + '<input>.grad'."""
    out = {"loss": _sha(loss.detach()), **_grads(modules)}
    for tag, t in inputs:
        out[f"grad.{tag}"] = _sha(t.grad)
    return out


def _clip_step(remat=False, unlocked=None, chunk=0, keep=False):
    m = _tiny()
    if remat:
        m.set_grad_checkpointing(True)
    if unlocked is not None:
        m.lock_image_tower(unlocked_groups=unlocked)
    img, tok = _batch()
    inputs = ()
    prev = training.CHUNK_LAYERS[0]
    training.set_backward_chunk_layers(chunk)
    try:
        if keep:                                   # image b keeps 37 of its 100 patches: a fixed permutation (37 and 7 are coprime with 100)
            table = torch.tensor([[(37 * i + 7 * b) % 100 for i in range(37)] for b in range(B)], dtype=torch.int64)
            img.requires_grad_(True)
            inputs = (("image", img),)
            feats = (training.encode_image(m, img, True, keep=table), training.encode_text(m, tok, True), m.logit_scale.exp())
        else:
            feats = training.clip_forward(m, img, tok)
        loss = ClipLoss()(*feats)
        loss.backward()
    finally:
        training.set_backward_chunk_layers(prev)
    return _digests(loss, (("clip", m),), inputs)


def _soft_tokens():
    m = _tiny()
    m.requires_grad_(False)
    vocab, ctx = m.vocab_size, m.context_length
    ids = synth.make_captions(2, seed=SEED)
    soft = torch.nn.functional.one_hot(ids, vocab).float() * 0.9 + _draw("train.soft.noise", (2, ctx, vocab), 1.0).abs() * (0.1 / vocab)
    soft = soft.to(DEV).requires_grad_(True)
    target = torch.nn.functional.normalize(_draw("train.soft.target", (2, m.embed_dim), 1.0), dim=-1).to(DEV)
    loss = -(training.encode_text(m, soft, normalize=True) * target).sum(-1).mean()
    loss.backward()
    return _digests(loss, (("clip", m),), (("soft", soft),))


def _coca():
    m = _tiny()
    dec = TextDecoder(m.visual.transformer.width, m.transformer.width, 192, 2, 3, 768, m.vocab_size, num_learnable_tokens=16)
    dec = _fill(dec, "train.dec").to(DEV)
    img, tok = _batch()
    labels = ((_draw("train.coca.labels", (B, 16), 1.0).abs() * 1e4).long() % m.vocab_size).to(DEV)
    mask = (_draw("train.coca.mask", (B, 16), 1.0) < 0.8).float().to(DEV)
    img_f, txt_f, scale, cap = training.coca_forward(m, dec, img, tok)
    loss = ClipLoss()(img_f, txt_f, scale) + 2 * CaptionLoss()(cap, labels, mask)
    loss.backward()
    return _digests(loss, (("clip", m), ("dec", dec)))


def _feature(layer):
    m = _tiny().eval()
    img = synth.make_images(2, 160, seed=SEED).to(DEV).requires_grad_(True)
    value = visualize.mlp_feature(m, img, layer, 5)
    loss = -value.sum() / 4.0
    loss.backward()
    out = _digests(loss, (("clip", m),), (("image", img),))
    out["feature"] = _sha(value.detach())
    return out


def _seed():
    """The loops draw on the host (torch's CPU generator, Python's) and, the ascent's Gumbel noise, on the device."""
    torch.manual_seed(SEED)
    random.seed(SEED)


def _viz_loop():
    """Three iterations at a batch of 6 = 3 repeats of 2 images: the packed table's step rows are not 16-byte aligned, the rows run
    b = r N + n, and layer 2 runs a lower tower under the tap block."""
    m = _tiny().eval()
    _seed()
    viz = visualize.FeatureVisualizer(m, layer=2, feature=5, steps=2, repeat=3, images=2)
    viz.begin(visualize.new_init(160, 2))
    for i in range(3):
        viz.step(i)
    return {"history": _sha(viz.history), "image": _sha(viz.image), "dcols": _sha(viz._s.dcols)}


def _ascent():
    m = _tiny()
    image = synth.make_images(1, 160, seed=4)[0]
    image = ((image - image.min()) / (image.max() - image.min())).to(DEV)
    _seed()
    loop = GradientAscent(m, batch_size=3, tokens=2, steps=2)
    loop.begin(image)
    try:
        loop.step(0)
        loop.step(1)
    finally:
        loop.end()
    return {"history": _sha(loop.history), "ids_history": _sha(loop.ids_history), "normu": _sha(loop.normu),
            "best_text_embedding": _sha(loop.best_text_embedding), **_grads((("clip", m),))}


def _bare_tower():
    """head_dim 80 (the streaming attention backward over d padded to 96) and an MLP of 1076 columns padded to 1088."""
    tr = Transformer(320, 2, 4, (1076 + 0.5) / 320)
    assert tr.resblocks[0].mlp_dim == 1076 and tr.resblocks[0].mlp_pad == 1088
    tr = _fill(tr, "train.bare").to(DEV)
    x = _draw("train.bare.x", (2, 257, 320), 1.0).to(DEV).requires_grad_(True)
    wout = _draw("train.bare.wout", (2, 257, 320), 0.1).to(DEV)
    loss = (training.tower_forward(tr, x).float() * wout).sum()
    loss.backward()
    return _digests(loss, (("tower", tr),), (("x", x),))


CASES = {
    "clip/one_node_per_tower": (_clip_step, {}),
    "clip/grad_checkpointing": (_clip_step, dict(remat=True)),
    "clip/locked_unlocked1": (_clip_step, dict(unlocked=1)),             # the whole block stack frozen: first = layers, nothing kept
    "clip/locked_unlocked3": (_clip_step, dict(unlocked=3)),             # the two top blocks train: 0 < first < layers, partial backward
    "clip/chunk_layers_1": (_clip_step, dict(chunk=1)),
    "clip/keep_table": (_clip_step, dict(keep=True)),
    "text/soft_tokens_frozen": (_soft_tokens, {}),
    "coca/two_block_decoder": (_coca, {}),
    "featviz/layer0": (_feature, dict(layer=0)),
    "featviz/layer2": (_feature, dict(layer=2)),
    "tower/hd80_l257_padmlp": (_bare_tower, {}),
    "vizloop/three_steps_n2_r3": (_viz_loop, {}),
    "ascent/two_steps_b3_k2": (_ascent, {}),
}


def _recorded(case):
    with open(FIXTURE) as f:
        return json.load(f)[case]


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_step_matches_the_recorded_digests(case):
    want = _recorded(case)
    fn, kw = CASES[case]
    got = fn(**kw)
    assert sorted(got) == sorted(want), (case, "the set of outputs changed")
    wrong = [k for k in sorted(got) if got[k] != want[k]]
    for k in wrong:
        print(case, k, got[k], "recorded", want[k])
    assert not wrong, (case, wrong)


if __name__ == "__main__":
    digests = {case: fn(**kw) for case, (fn, kw) in CASES.items()}
    with open(sys.argv[1], "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", sys.argv[1], sum(len(v) for v in digests.values()), "digests")
