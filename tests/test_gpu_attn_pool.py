"""Attentional pooling on the GPU: the ov_attn_pool / ov_attn_pool_backward kernels at their edges against the fp64 closed form of
poolops under its per-element bounds (test_attn_pool_bound.py pins what those can see), then the pooled image tower against the
reference-generated fixture tests/golden/attnpool_tiny.npz: inference, the training forward, one ClipLoss step's gradients.

Kernel shapes are the edges, not the workload: n_q of one lane, one partial tile, one full tile, one tile plus one row, all eight
tiles; L of one key, one partial tile, a full tile, a tile plus a lone key (33, 65, 257), and past 288, where K | V stream through LDS
in 256-key chunks (321: a ragged second chunk; 513: a last chunk of one key); B one past the dq reduction's chunk of images for both
chunk sizes (3 at n_q <= 64, 9 above)."""
import os

import numpy as np
import pytest
import torch

import poolops as PO
from hipops import U_BWD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, L, n_q, Hh, hd)
KERNEL_CASES = [
    # every n_q at L = 33 and L = 257
    (3, 33, 1, 2, 64), (1, 33, 5, 2, 72), (3, 33, 32, 2, 96), (1, 33, 33, 2, 64), (3, 33, 256, 2, 72),
    (1, 257, 1, 2, 96), (3, 257, 5, 2, 64), (1, 257, 32, 2, 72), (3, 257, 33, 2, 96), (3, 257, 256, 2, 64), (1, 257, 256, 2, 96),
    # every L at n_q = 5
    (3, 1, 5, 2, 64), (1, 17, 5, 2, 96), (3, 32, 5, 2, 72), (3, 65, 5, 2, 96),
    # K | V in chunks of 256 keys
    (1, 321, 33, 2, 72), (3, 513, 5, 2, 64),
    # one image past the dq chunk of 8 (n_q > 64); 3 images at n_q <= 64 are one past the chunk of 2
    (9, 33, 65, 2, 64),
]
_REFS = {}


def case(B, L, nq, Hh, hd):
    """The inputs and their fp64 reference, computed once per shape."""
    key = (B, L, nq, Hh, hd)
    if key not in _REFS:
        seed = 1000 * L + 10 * nq + hd + B
        q, kv, dout = PO.spiked_pool_case(B, L, nq, Hh, hd, seed)[:3] if L >= 2 else PO.pool_case(B, L, nq, Hh, hd, seed)
        r = PO.pool_ref64(q, kv, dout, B, L, nq, Hh, hd)
        _REFS[key] = (q, kv, dout, r, PO.bwd_bounds(r, U_BWD * r.o.abs()))
    return _REFS[key]


def test_backward_chunk_is_what_the_cases_assume():
    from openvision_amd import _lib
    lib = _lib.load()
    assert [lib.ov_attn_pool_backward_chunk(n) for n in (1, 5, 64, 65, 256)] == [2, 2, 2, 8, 8]


@pytest.mark.parametrize("B,L,nq,Hh,hd", KERNEL_CASES)
def test_kernels_inside_the_bounds_and_repeatable(B, L, nq, Hh, hd):
    q, kv, dout, r, bounds = case(B, L, nq, Hh, hd)
    qd, kvd, dd = q.to(DEV), kv.to(DEV), dout.to(DEV)
    out, lse = PO.attn_pool(qd, kvd, B, L, nq, Hh, hd)
    out2, lse2 = PO.attn_pool(qd, kvd, B, L, nq, Hh, hd)
    rf = PO.fwd_ratio(out, r)
    lse_err = float((lse[:, :nq].double().cpu() - r.lse).abs().max())
    print(f"attn_pool B={B} L={L} n_q={nq} hd={hd}: out err / bound {rf:.3f}  lse err {lse_err:.2e}")
    assert rf <= 1.0 and lse_err <= PO.LSE_ATOL, (rf, lse_err)
    assert torch.isnan(lse[:, nq:]).all()                           # nothing is written past n_q
    assert torch.equal(out, out2) and torch.equal(lse[:, :nq], lse2[:, :nq])
    # the backward is handed bf16(reference O), for which the bound's eo = U |O| holds, and the kernel's own lse
    o_ref = r.o.to(torch.bfloat16).to(DEV)
    dq, dkv = PO.attn_pool_backward(qd, kvd, o_ref, dd, lse, B, L, nq, Hh, hd)
    dq2, dkv2 = PO.attn_pool_backward(qd, kvd, o_ref, dd, lse, B, L, nq, Hh, hd)
    rb = PO.bwd_ratios(dq, dkv, r, bounds)
    print(f"  backward: err / bound dq {rb[0]:.3f} dk {rb[1]:.3f} dv {rb[2]:.3f}")
    assert max(rb) <= 1.0, rb
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)


def test_row_pitches_wider_than_the_rows():
    """ld_kv, ld_out and ld_dkv wider than their rows: the results are those of the packed call, and the padding is left alone."""
    B, L, nq, Hh, hd = 3, 33, 5, 2, 72
    q, kv, dout, r, bounds = case(B, L, nq, Hh, hd)
    E = Hh * hd
    qd, dd = q.to(DEV), dout.to(DEV)
    kvw = torch.full((B * L, 2 * E + 16), float("nan"), dtype=torch.bfloat16, device=DEV)
    kvw[:, :2 * E] = kv.to(DEV)
    outw = torch.full((B * nq, E + 8), 77.0, dtype=torch.bfloat16, device=DEV)
    dkvw = torch.full((B * L, 2 * E + 24), 77.0, dtype=torch.bfloat16, device=DEV)
    out, lse = PO.attn_pool(qd, kvw[:, :2 * E], B, L, nq, Hh, hd, out=outw[:, :E])
    ref_out, ref_lse = PO.attn_pool(qd, kv.to(DEV), B, L, nq, Hh, hd)
    assert torch.equal(out, ref_out) and torch.equal(lse[:, :nq], ref_lse[:, :nq]) and bool((outw[:, E:] == 77.0).all())
    dq, dkv = PO.attn_pool_backward(qd, kvw[:, :2 * E], outw[:, :E], dd, lse, B, L, nq, Hh, hd, dkv=dkvw[:, :2 * E])
    dq0, dkv0 = PO.attn_pool_backward(qd, kv.to(DEV), ref_out, dd, ref_lse, B, L, nq, Hh, hd)
    assert torch.equal(dq, dq0) and torch.equal(dkv, dkv0) and bool((dkvw[:, 2 * E:] == 77.0).all())


def test_bad_arguments_are_refused_before_any_launch():
    from openvision_amd import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    B, L, nq, Hh, hd = 2, 17, 5, 2, 64
    E = Hh * hd
    q = torch.zeros(nq, E, dtype=torch.bfloat16, device=DEV)
    kv = torch.zeros(B * L, 2 * E, dtype=torch.bfloat16, device=DEV)
    out = torch.full((B * nq, E), 77.0, dtype=torch.bfloat16, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()

    def fwd(q_=q, ldq=E, ldkv=2 * E, ldo=E, B_=B, L_=L, nq_=nq, hd_=hd):
        return lib.ov_attn_pool(p(q_), ldq, p(kv), ldkv, p(out), ldo, None, B_, L_, nq_, Hh, hd_, 0.125, st)

    assert fwd(hd_=60) == UNSUPPORTED and fwd(hd_=104) == UNSUPPORTED
    assert fwd(nq_=0) == UNSUPPORTED and fwd(nq_=257) == UNSUPPORTED
    assert fwd(L_=0) == INVALID and fwd(B_=0) == INVALID and fwd(q_=None) == INVALID
    assert fwd(ldq=E - 8) == INVALID and fwd(ldkv=2 * E - 8) == INVALID and fwd(ldo=E - 8) == INVALID and fwd(ldo=E + 4) == INVALID
    dq = torch.full((nq, E), 77.0, dtype=torch.float32, device=DEV)
    dkv = torch.full((B * L, 2 * E), 77.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B * Hh, 32, dtype=torch.float32, device=DEV)
    nb = lib.ov_attn_pool_backward_workspace_bytes(B, L, nq, Hh, hd)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)

    def bwd(lse_=lse, ws_=ws, nb_=nb, hd_=hd, lddq=E, nq_=nq):
        return lib.ov_attn_pool_backward(p(q), E, p(kv), 2 * E, p(out), E, p(out), E, p(lse_), p(dq), lddq, p(dkv), 2 * E, B, L, nq_, Hh, hd_,
                                         0.125, p(ws_), nb_, st)

    assert bwd(lse_=None) == INVALID and bwd(ws_=None) == INVALID and bwd(lddq=E - 4) == INVALID
    assert bwd(nb_=nb - 1) == WORKSPACE and bwd(hd_=100) == UNSUPPORTED and bwd(nq_=300) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 77.0).all()) and bool((dq == 77.0).all()) and bool((dkv == 77.0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# The pooled image tower against the reference-generated fixture (tests/golden/make_golden_attnpool.py: what it can tell apart is
# asserted there on the reference -- ln_k left out, K and V swapped, CLS excluded, uniform attention each move every image by
# 1 - cos >= 1.5e-2, while its own bf16 twin stays within 1e-4)
import tempfile                                                     # noqa: E402

import torch.nn.functional as F                                     # noqa: E402

from openvision_amd import checkpoint, training                     # noqa: E402
from openvision_amd.loss import ClipLoss                            # noqa: E402
from openvision_amd.model import create_model                       # noqa: E402
from test_attn_pool_cpu import pool_cfg, pool_state_dict            # noqa: E402
from test_gpu_model import COS_TOL                                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_ATOL = 0.15                  # tests/test_gpu_stock.py: logits = 14.29 * cosine, bf16-path budget 14.29 * ~5e-3
CONFIGS = ["a", "b"]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "attnpool_tiny.npz"))


def build(which, train=False):
    return create_model(pool_cfg(which), device=DEV, state_dict=pool_state_dict(which)).train(train)


def inputs(g, which):
    return torch.from_numpy(g[which + "/images"].astype(np.float32)).to(DEV), torch.from_numpy(g[which + "/text"]).to(DEV)


def one_minus_cos(a, b):
    return float((1 - F.cosine_similarity(a.double().cpu(), torch.as_tensor(b).double().cpu(), dim=-1)).max())


@pytest.mark.parametrize("which", CONFIGS)
def test_inference_against_the_reference(which, g):
    img, tok = inputs(g, which)
    m = build(which)
    with torch.no_grad():
        raw = m.encode_image(img)
        fi, ft, scale = m(img, tok)
        li, lt = m.get_logits(img, tok)
        m.visual.output_tokens = True
        pooled, tokens = m.visual(img)
        m.visual.output_tokens = False
        again = m.encode_image(img)                                 # the cached projected queries: the second call is the first
    c_raw, c_f, c_tok = one_minus_cos(raw, g[which + "/image_features_raw"]), one_minus_cos(fi, g[which + "/image_features"]), \
        one_minus_cos(tokens, g[which + "/tokens"])
    print(f"config {which}: 1 - cos to the reference: raw {c_raw:.2e} normalised {c_f:.2e} tokens {c_tok:.2e}")
    assert c_raw < COS_TOL and c_f < COS_TOL and c_tok < COS_TOL
    assert tuple(tokens.shape) == (3, 4, 64) and torch.equal(pooled, raw) and torch.equal(again, raw)
    assert one_minus_cos(ft, g[which + "/text_features"]) < COS_TOL
    np.testing.assert_allclose(li.cpu().numpy(), g[which + "/logits_per_image"], atol=LOGIT_ATOL)
    np.testing.assert_allclose(lt.cpu().numpy(), g[which + "/logits_per_image"].T, atol=LOGIT_ATOL)
    # the training forward agrees with the inference path, features and tokens
    tf, ttok = training.encode_image(m, img, True, output_tokens=True)
    assert one_minus_cos(tf.detach(), fi) < COS_TOL and one_minus_cos(ttok.detach(), tokens) < COS_TOL
    assert one_minus_cos(tf.detach(), g[which + "/image_features"]) < COS_TOL
    # a parameter written behind autograd's back is picked up after invalidate_packed (the cached queries among the packed copies)
    with torch.no_grad():
        m.visual.attn_pool.query.data.mul_(-1.0)
    m.invalidate_packed()
    with torch.no_grad():
        assert one_minus_cos(m.encode_image(img), raw) > 10 * COS_TOL


@pytest.mark.parametrize("which", CONFIGS)
def test_a_reference_state_dict_loads_through_a_checkpoint_directory(which, g):
    img, _ = inputs(g, which)
    m = build(which)
    with torch.no_grad():
        want = m.encode_image(img)
    with tempfile.TemporaryDirectory() as d:
        checkpoint.save_pretrained(m, pool_cfg(which), d, safetensors=False)
        sd = checkpoint.read_state_dict(d)
        assert sorted(sd) == [str(k) for k in g[which + "/keys"]]
        m2, _ = checkpoint.from_pretrained(d, device=DEV)
    with torch.no_grad():
        assert torch.equal(m2.encode_image(img), want)


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _step(m, img, tok, **kw):
    m.zero_grad(set_to_none=True)
    fi, ft, s = training.clip_forward(m, img, tok, **kw)
    loss = ClipLoss()(fi, ft, s)
    loss.backward()
    return fi.detach(), ft.detach(), float(loss.detach()), _grads(m)


@pytest.mark.parametrize("which", CONFIGS)
def test_training_step_against_the_reference(which, g):
    """One ClipLoss step by the criterion of test_gpu_stock.py: features under COS_TOL, the loss within 2e-2, every stored gradient at
    cosine >= 0.99 with its norm within 5 %.  Then: recomputation bitwise; patch dropout with an explicit keep table (the pooler sees
    1 + K keys); the pooler frozen (no gradient for it, the tower's bitwise unchanged); one FusedAdamW step moves the queries."""
    img, tok = inputs(g, which)
    m = build(which, train=True)
    fi, ft, loss, got = _step(m, img, tok)
    assert one_minus_cos(fi, g[which + "/image_features"]) < COS_TOL and one_minus_cos(ft, g[which + "/text_features"]) < COS_TOL
    print(f"config {which}: loss {loss:.5f}, reference {float(g[which + '/loss']):.5f}")
    assert abs(loss - float(g[which + "/loss"])) < 2e-2
    names = [k[len(which) + 6:] for k in g.files if k.startswith(which + "/grad/")]
    assert len(names) == 6 and "visual.attn_pool.query" in names
    for name in names:
        r = torch.from_numpy(g[f"{which}/grad/{name}"].astype(np.float32))
        gg = got[name].float().cpu()
        cos = float((gg * r).sum() / (gg.norm() * r.norm() + 1e-30))
        print(f"  {name}: cos {cos:.5f}, norm {float(gg.norm()):.4e} / reference {float(r.norm()):.4e}")
        assert cos >= 0.99, (name, cos)
        assert abs(float(gg.norm()) - float(r.norm())) < 0.05 * float(r.norm()), name
    assert len(got) == len(list(m.parameters()))                    # every parameter got one, the pooler's eleven (nine) among them
    # twice the same bits (dq is a fixed-order sum), and with activation recomputation
    fi1, _, loss1, got1 = _step(m, img, tok)
    assert torch.equal(fi, fi1) and loss == loss1 and all(torch.equal(got[n], got1[n]) for n in got)
    m.set_grad_checkpointing()
    fi2, ft2, loss2, got2 = _step(m, img, tok)
    assert torch.equal(fi, fi2) and torch.equal(ft, ft2) and loss == loss2 and sorted(got) == sorted(got2)
    for name in got:
        assert torch.equal(got[name], got2[name]), name
    m.set_grad_checkpointing(False)
    # patch dropout with an explicit keep table: 1 + K = 4 keys per image
    keep = torch.tensor([[3, 0, 9], [15, 2, 7], [8, 1, 4]])
    seen = []
    orig = training.attn_pool_forward                               # (the training path calls no module: watch its entry instead)
    training.attn_pool_forward = lambda pool, x: (seen.append(tuple(x.shape)), orig(pool, x))[1]
    try:
        fk, _, lossk, gotk = _step(m, img, tok, keep=keep)
    finally:
        training.attn_pool_forward = orig
    assert seen == [(3, 4, pool_cfg(which)["vision_cfg"]["width"])]
    assert np.isfinite(lossk) and one_minus_cos(fk, fi) > 1e-5 and "visual.attn_pool.query" in gotk
    # the pooler frozen
    for p in m.visual.attn_pool.parameters():
        p.requires_grad_(False)
    fi3, _, loss3, got3 = _step(m, img, tok)
    assert torch.equal(fi3, fi) and loss3 == loss
    assert all(p.grad is None for p in m.visual.attn_pool.parameters())
    assert sorted(got3) == sorted(n for n in got if not n.startswith("visual.attn_pool."))
    for name in got3:
        assert torch.equal(got3[name], got[name]), name
    # pooler and tower frozen: nothing below ln_post runs a backward, the head and the text side still train
    m.visual.requires_grad_(False)
    m.visual.ln_post.requires_grad_(True)
    m.visual.proj.requires_grad_(True)
    _, _, _, got4 = _step(m, img, tok)
    assert {n for n in got4 if n.startswith("visual.")} == {"visual.ln_post.weight", "visual.ln_post.bias", "visual.proj"}
    assert torch.equal(got4["visual.proj"], got["visual.proj"])
    # one optimiser step moves the queries
    m.requires_grad_(True)
    opt = training.FusedAdamW(m, lr=1e-3)
    q0 = m.visual.attn_pool.query.detach().clone()
    opt.zero_grad()
    ClipLoss()(*training.clip_forward(m, img, tok)).backward()
    opt.step()
    assert not torch.equal(m.visual.attn_pool.query.detach(), q0)
    with torch.no_grad():
        assert one_minus_cos(m.encode_image(img, True), fi) > 0     # the inference path sees the updated, re-packed pooler
