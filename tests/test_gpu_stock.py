"""GPU: a stock open_clip model (causal text tower pooled at each caption's EOT token; image tower with ln_pre and 'tok' pooling) against
the reference-generated fixture tests/golden/stock_tiny.npz (tests/golden/make_golden_stock.py, whose docstring gives the inputs and
what the reference itself shows on them: under the mask the second token table gives identical features, without it every row but
the EOT-at-76 one moves by 1 - cos >= 0.031, so COS_TOL = 1e-3 separates a missing mask, a wrong pooled row and swapped rows).

Kernels first (ov_token_argmax exact, ov_gather_rows_at bitwise), then the inference entry points, causality, the pooled-rows tail
against OVHIP_LAST_BLOCK_FULL=1 (read once per process: one child, module scope), the exploded forward, hipGraph replay, training."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openvision_amd import _lib, synth, training
from openvision_amd._lib import ptr, stream_ptr, check
from openvision_amd.loss import ClipLoss
from openvision_amd.model import create_model
from ranks import run_child
from test_gpu_model import COS_TOL
from test_stock_cpu import stock_cfg, T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_LAST = 1                       # the row whose EOT sits at T - 1: both token tables agree on it
LOGIT_ATOL = 0.15                  # tests/test_gpu_model.py, tiny preset: logits = 14.29 * cosine, bf16-path budget 14.29 * ~5e-3


def golden_npz():
    return np.load(os.path.join(ROOT, "tests", "golden", "stock_tiny.npz"))


def build(train=False):
    cfg = stock_cfg()
    m = create_model(cfg, device=DEV, state_dict=synth.make_state_dict(cfg))
    return m.train(train)


def one_minus_cos_rows(a, b):
    return 1 - F.cosine_similarity(a.double().cpu(), torch.as_tensor(b).double().cpu(), dim=-1)


def one_minus_cos(a, b):
    return one_minus_cos_rows(a, b).max().item()


@pytest.fixture(scope="module")
def g():
    return golden_npz()


@pytest.fixture(scope="module")
def inputs(g):
    return (torch.from_numpy(g["images"].astype(np.float32)).to(DEV), torch.from_numpy(g["tokens"]).to(DEV),
            torch.from_numpy(g["tokens_b"]).to(DEV))


@pytest.fixture(scope="module")
def model():
    return build()


# ---- 1. ov_token_argmax ----------------------------------------------------------------------------------------------------------
def token_argmax(tok):
    idx = torch.full((tok.shape[0],), -7, dtype=torch.int32, device=tok.device)
    check(_lib.load().ov_token_argmax(ptr(tok), ptr(idx), tok.shape[0], tok.shape[1], stream_ptr()), "ov_token_argmax")
    return idx


@pytest.mark.parametrize("B,T_", [(1, 1), (3, 77), (5, 64), (2, 65), (300, 80)])
def test_token_argmax_is_torch_argmax(B, T_):
    """Exactly torch.argmax on the CPU (the first of equal maxima).  Rows: random ids with repeats (ties of the maximum among them), an
    all-equal row, ids above 2^31 that differ in the high word only or in the low word only, a negative row, the maximum at T - 1 and
    at the 64-lane boundary."""
    gen = torch.Generator().manual_seed(B * 131 + T_)
    tok = torch.randint(0, 12, (B, T_), generator=gen)                      # 12 values over T positions: the maximum repeats
    tok[0] = 5                                                              # all equal -> 0
    if B > 1:
        tok[1] = torch.randint(0, 1000, (T_,), generator=gen)
        tok[1, T_ - 1] = 49407                                              # the maximum at T - 1
    if B > 2:
        big = (1 << 31) + 5
        tok[2] = big                                                        # above 2^31 ...
        tok[2, T_ // 2] = big + (1 << 32)                                   # ... the winner differs in the high word only
        tok[2, T_ - 1] = big + (1 << 32)                                    # and ties with a later one
    if B > 3:
        tok[3] = -torch.randint(1, 1 << 40, (T_,), generator=gen)           # all negative
    if B > 4:
        tok[4] = (1 << 40) + torch.randint(0, 3, (T_,), generator=gen)      # equal high words, ties in the low word
    if B > 5 and T_ > 64:
        tok[5] = 0
        tok[5, 64] = 9                                                      # the first element of a lane's second round
        tok[6] = 3
        tok[6, 63], tok[6, 64] = 9, 9                                       # a tie across the round boundary
    want = tok.argmax(dim=-1)
    assert want[0] == 0 and (B < 2 or want[1] == T_ - 1) and (B < 3 or want[2] == T_ // 2)
    got = token_argmax(tok.to(DEV)).cpu()
    assert got.dtype == torch.int32 and torch.equal(got.long(), want), (got.tolist()[:8], want.tolist()[:8])


def test_token_argmax_on_the_fixture_tables(g, inputs):
    _, ta, tb = inputs
    want = [0, 76, 31, 32, 5, 9, 0, 20]
    assert token_argmax(ta).tolist() == want and token_argmax(tb).tolist() == want
    assert g["tokens"].argmax(axis=1).tolist() == want


# ---- 2. ov_gather_rows_at --------------------------------------------------------------------------------------------------------
def gather_rows_at(x, idx, B, L, D, out):
    check(_lib.load().ov_gather_rows_at(ptr(x), x.stride(0), ptr(idx), ptr(out), out.stride(0), B, L, D, stream_ptr()), "ov_gather_rows_at")


@pytest.mark.parametrize("D", [64, 192, 1024])
def test_gather_rows_at_bitwise(D):
    """Against torch indexing, bitwise: both pitches larger than D (the columns behind D of the output stay as they were), idx 0 and
    L - 1 among the rows, and -1 / L clamped to 0 / L - 1 (memory safety: ov_token_argmax never produces them)."""
    B, L, pad = 7, 13, 24
    gen = torch.Generator().manual_seed(D)
    xp = torch.randn(B * L, D + pad, generator=gen).to(torch.bfloat16).to(DEV)
    x = xp[:, :D]
    idx = torch.tensor([0, L - 1, 5, -1, L, 7, L - 1], dtype=torch.int32)
    outp = torch.full((B, D + 8), 3.0, dtype=torch.bfloat16, device=DEV)
    gather_rows_at(x, idx.to(DEV), B, L, D, outp[:, :D])
    want = xp.view(B, L, D + pad)[torch.arange(B), idx.clamp(0, L - 1).long()][:, :D]
    assert torch.equal(outp[:, :D], want)
    assert bool((outp[:, D:] == 3.0).all())
    # B * D / 8 beyond one block, contiguous
    B2 = 40
    x2 = torch.randn(B2 * L, D, generator=gen).to(torch.bfloat16).to(DEV)
    idx2 = torch.randint(0, L, (B2,), generator=gen).to(torch.int32)
    out2 = torch.empty(B2, D, dtype=torch.bfloat16, device=DEV)
    gather_rows_at(x2, idx2.to(DEV), B2, L, D, out2)
    assert torch.equal(out2, x2.view(B2, L, D)[torch.arange(B2), idx2.long()])


# ---- 3. the inference entry points against the fixture ---------------------------------------------------------------------------
def test_encode_forward_and_logits_against_the_reference(g, inputs, model):
    img, ta, _ = inputs
    m = model
    with torch.no_grad():
        ft_raw, fi_raw = m.encode_text(ta), m.encode_image(img)
        fi, ft, scale = m(img, ta)
        li, lt = m.get_logits(img, ta)
    ct, ci = one_minus_cos_rows(ft_raw, g["text_features_raw"]), one_minus_cos_rows(fi_raw, g["image_features_raw"])
    print("1 - cos to the reference: text rows", ct.numpy().round(6), "images", ci.numpy().round(6))
    assert ct.max().item() < COS_TOL and ci.max().item() < COS_TOL
    assert one_minus_cos(ft, g["text_features"]) < COS_TOL and one_minus_cos(fi, g["image_features"]) < COS_TOL
    np.testing.assert_allclose(ft.norm(dim=-1).cpu().numpy(), 1.0, atol=1e-5)
    np.testing.assert_allclose(fi.norm(dim=-1).cpu().numpy(), 1.0, atol=1e-5)
    assert abs(float(scale) - float(g["logit_scale"])) < 1e-3
    d = np.abs(li.cpu().numpy() - g["logits_per_image"]).max()
    print(f"max |logits - reference| {d:.4f}")
    np.testing.assert_allclose(li.cpu().numpy(), g["logits_per_image"], atol=LOGIT_ATOL)
    np.testing.assert_allclose(lt.cpu().numpy(), g["logits_per_image"].T, atol=LOGIT_ATOL)
    m.check_token_range()


# ---- 4. causality ----------------------------------------------------------------------------------------------------------------
def test_tokens_behind_the_pooled_position_do_not_matter_under_the_mask(inputs):
    _, ta, tb = inputs
    m = build()
    fa, fb = m.encode_text(ta, normalize=True), m.encode_text(tb, normalize=True)
    d = one_minus_cos_rows(fa, fb)
    print("masked: 1 - cos between the two tables per row", d.numpy(), "bitwise equal:", torch.equal(fa, fb))
    assert d.max().item() < COS_TOL
    m.transformer.set_causal_prefix(None)                       # the same weights without the mask
    ua, ub = m.encode_text(ta, normalize=True), m.encode_text(tb, normalize=True)
    d = one_minus_cos_rows(ua, ub)
    print("unmasked: 1 - cos between the two tables per row", d.numpy().round(4))
    others = [r for r in range(ta.shape[0]) if r != ROW_LAST]
    assert d[others].min().item() > 10 * COS_TOL
    assert torch.equal(ua[ROW_LAST], ub[ROW_LAST])
    m.transformer.set_causal_prefix(0)
    assert torch.equal(m.encode_text(ta, normalize=True), fa)


# ---- 5. the pooled-rows tail is the full last block ------------------------------------------------------------------------------
def compute_text(tables=("tokens", "tokens_b")):
    g = golden_npz()
    m = build()
    return {k: m.encode_text(torch.from_numpy(g[k]).to(DEV)).cpu() for k in tables}


_CHILD = r"""
import torch
import test_gpu_stock as S
torch.save(S.compute_text(), sys.argv[1])
"""


def test_pooled_tail_is_bitwise_the_full_last_block():
    """Past the last attention every row is per-token, so the last block on the B gathered EOT rows is bitwise the full block on all
    B T rows, under the causal mask as without one."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "full.pt")
        run_child(_CHILD, path, env={"OVHIP_LAST_BLOCK_FULL": "1"}, timeout=300, gpu=True)
        full = torch.load(path)
    here = compute_text()
    for k in here:
        diff = (here[k].double() - full[k].double()).abs().max().item()
        print(f"{k}: max |pooled rows - full block| {diff:.3e}")
        assert torch.equal(here[k], full[k]), k


# ---- 6. the exploded forward -----------------------------------------------------------------------------------------------------
def test_exploded_text_forward_with_the_models_own_mask(inputs, model):
    """The caller-side walk of the reference's encode_text (model.py:269-284), handing the model's attn_mask buffer to the stack."""
    _, ta, _ = inputs
    m = model
    with torch.no_grad():
        x = m.token_embedding(ta)
        x = x + m.positional_embedding
        x = m.transformer(x, attn_mask=m.attn_mask)
        x = m.ln_final(x)
        x = x[torch.arange(x.shape[0], device=x.device), ta.argmax(dim=-1)] @ m.text_projection
        want = m.encode_text(ta)
    d = one_minus_cos_rows(x, want)
    print("exploded forward against encode_text: 1 - cos per row", d.numpy())
    assert d.max().item() < COS_TOL
    xin = torch.zeros(2, T, 192, device=DEV)
    for foreign in (m.attn_mask.clone(), torch.zeros(T, T, device=DEV), m.attn_mask[:5, :5], m.attn_mask.t()):
        with pytest.raises(NotImplementedError):
            m.transformer(xin, attn_mask=foreign)
    with pytest.raises(NotImplementedError):
        m.visual.transformer(xin, attn_mask=m.attn_mask)


# ---- 7. hipGraph replay ----------------------------------------------------------------------------------------------------------
def test_graph_replay_is_the_plain_call(inputs):
    _, ta, tb = inputs
    m = build()
    plain_a, plain_b = m.encode_text(ta[:3]), m.encode_text(tb[2:5])
    m.use_graphs(8)
    assert torch.equal(m.encode_text(ta[:3]), plain_a)                      # captured
    assert torch.equal(m.encode_text(tb[2:5]), plain_b)                     # replayed on other captions: the rows are found in the graph
    assert torch.equal(m.encode_text(ta[:3]), plain_a)
    assert len(m._graphs.graphs) == 1
    m.use_graphs(0)


# ---- 8. training -----------------------------------------------------------------------------------------------------------------
def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _step(m, img, tok):
    m.zero_grad(set_to_none=True)
    fi, ft, s = training.clip_forward(m, img, tok)
    loss = ClipLoss()(fi, ft, s)
    loss.backward()
    return fi.detach(), ft.detach(), float(loss.detach()), _grads(m)


def test_training_step_against_the_reference(g, inputs):
    """clip_forward + ClipLoss + backward on the images and the first 3 captions, with the bounds of
    test_gpu_patchdrop.py::test_training_step_against_reference: features under COS_TOL, the loss within 2e-2, and EVERY stored
    gradient at cosine >= 0.99 with its norm within 5 %.  Then the same step with activation recomputation, bitwise."""
    img, ta, _ = inputs
    n = int(g["train_rows"])
    m = build(train=True)
    fi, ft, loss, got = _step(m, img, ta[:n])
    assert one_minus_cos(fi, g["image_features"]) < COS_TOL and one_minus_cos(ft, g["text_features"][:n]) < COS_TOL
    print(f"loss {loss:.5f}, reference {float(g['loss']):.5f}")
    assert abs(loss - float(g["loss"])) < 2e-2
    names = [k[5:] for k in g.files if k.startswith("grad/")]
    assert len(names) == 9 and "visual.ln_pre.weight" in names and "token_embedding.weight" in names
    for name in names:
        r = torch.from_numpy(g["grad/" + name].astype(np.float32))
        gg = got[name].float().cpu()
        cos = float((gg * r).sum() / (gg.norm() * r.norm() + 1e-30))
        print(f"{name}: cos {cos:.5f}, norm {float(gg.norm()):.4e} / reference {float(r.norm()):.4e}")
        assert cos >= 0.99, (name, cos)
        assert abs(float(gg.norm()) - float(r.norm())) < 0.05 * float(r.norm()), name
    assert len(got) == len(list(m.parameters()))                            # every parameter got one, ln_pre's among them
    m.set_grad_checkpointing()
    fi2, ft2, loss2, got2 = _step(m, img, ta[:n])
    assert torch.equal(fi, fi2) and torch.equal(ft, ft2) and loss == loss2
    assert sorted(got) == sorted(got2)
    for name in got:
        assert torch.equal(got[name], got2[name]), name


def test_soft_token_gradient_with_a_frozen_model(inputs):
    """Soft one-hot rows through the causal tower: the gradient that reaches them is bitwise the same whether or not the parameters
    take gradients (the partial backward skips their work, not the input's)."""
    _, ta, _ = inputs
    m = build(train=True)
    gen = torch.Generator().manual_seed(5)
    r = torch.randn(3, 64, generator=gen).to(DEV)
    soft0 = (F.one_hot(ta[:3], 1000).float() * 4.0 + 0.01 * torch.randn(3, T, 1000, generator=gen).to(DEV)).softmax(dim=-1)
    assert torch.equal(soft0.argmax(dim=-1).argmax(dim=-1), ta[:3].argmax(dim=-1))
    out = []
    for frozen in (False, True):
        m.requires_grad_(not frozen)
        m.zero_grad(set_to_none=True)
        soft = soft0.clone().requires_grad_(True)
        f = training.encode_text(m, soft, True)
        (f * r).sum().backward()
        out.append((f.detach(), soft.grad.detach().clone()))
        assert frozen == all(p.grad is None for p in m.parameters())
    (fa, ga), (fb, gb) = out
    assert torch.equal(fa, fb)
    assert float(ga.abs().max()) > 0 and torch.equal(ga, gb)
