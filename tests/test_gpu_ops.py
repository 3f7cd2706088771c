"""GPU parity: each HIP operator (through the C ABI) against the oracle on the same seeded inputs.

Tolerances are stated per test.  bf16 has 8 significant bits (eps = 2^-8 = 3.9e-3 relative), so an
operator with bf16 output is compared with rtol ~ 1e-2 against the oracle evaluated in fp32 on the SAME
bf16-rounded inputs; fp32-output operators (LN stats, l2norm, logits, loss) get fp32-level tolerances."""
import os

import numpy as np
import pytest
import torch

from oracle import clip_ref as R
import hipops as H
from ranks import run_child, run_ranks
H_ = H          # the attention tests use H for the head count

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("rows,D", [(7, 192), (513, 768), (1000, 1024), (33, 1152), (5, 4096), (3, 384)])
def test_layernorm_bf16(rows, D):
    x = (rnd(rows, D, seed=1) * 2 + 0.5).to(torch.bfloat16)
    g, b = rnd(D, seed=2) * 0.1 + 1, rnd(D, seed=3) * 0.1
    y = H.layernorm(x.to(DEV), g.to(DEV), b.to(DEV)).float().cpu()
    ref = R.layer_norm(x.float(), g, b)
    # output rounded to bf16: |err| <= 2^-8 |y| + small
    np.testing.assert_allclose(y.numpy(), ref.numpy(), rtol=8e-3, atol=8e-3)


def test_layernorm_fp32_io_matches_oracle_tightly():
    x = rnd(64, 1024, seed=4) * 3 - 1
    g, b = rnd(1024, seed=5) * 0.1 + 1, rnd(1024, seed=6) * 0.1
    y = H.layernorm(x.to(DEV), g.to(DEV), b.to(DEV)).cpu()
    np.testing.assert_allclose(y.numpy(), R.layer_norm(x, g, b).numpy(), rtol=1e-5, atol=2e-5)


GEMM_SHAPES = [(256, 256, 64), (300, 200, 128), (1, 8, 64), (257 * 3, 1024, 1024), (505, 576, 192), (640, 4096, 1024),
               (512, 1024, 4096), (100, 768, 640)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_bias(M, N, K):
    a, w, bias = rnd(M, K, seed=7).to(torch.bfloat16), (rnd(N, K, seed=8) / K ** 0.5).to(torch.bfloat16), rnd(N, seed=9)
    c = H.gemm(a.to(DEV), w.to(DEV), bias.to(DEV)).float().cpu()
    ref = a.float() @ w.float().T + bias
    np.testing.assert_allclose(c.numpy(), ref.numpy(), rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("epi,tanh", [(1, False), (2, True)])
def test_gemm_gelu(epi, tanh):
    M, N, K = 333, 768, 192
    a, w, bias = rnd(M, K, seed=10).to(torch.bfloat16), (rnd(N, K, seed=11) / K ** 0.5).to(torch.bfloat16), rnd(N, seed=12)
    c = H.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), epi=epi).float().cpu()
    ref = R.gelu(a.float() @ w.float().T + bias, tanh)
    np.testing.assert_allclose(c.numpy(), ref.numpy(), rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("M,N,K,epi", [(333, 768, 192, 1), (257 * 70 + 9, 4096, 1024, 1), (4100, 4304, 1152, 2), (65792, 1024, 256, 1)])
def test_gemm_keep_pre_activation_is_the_bias_gemm_and_output_the_gelu_gemm(M, N, K, epi):
    """ov_gemm_keep (the training forward's c_fc): both outputs bitwise equal to the two single-output launches, on grids below the
    persistent kernel's threshold (second launch) and above it (one fused epilogue), with padded leading dimensions and ragged edges."""
    a, w, bias = rnd(M, K, seed=10).to(torch.bfloat16).to(DEV), (rnd(N, K, seed=11) / K ** 0.5).to(torch.bfloat16).to(DEV), rnd(N, seed=12).to(DEV)
    out, pre = H.gemm_keep(a, w, bias, epi, ldc=N + 64, ldc2=N + 8)
    assert torch.equal(out[:, :N], H.gemm(a, w, bias, epi=epi))
    assert torch.equal(pre[:, :N], H.gemm(a, w, bias, epi=0))
    assert not out[:, N:].any() and not pre[:, N:].any()


@pytest.mark.parametrize("M,N,K,tanh", [(333, 768, 192, False), (257 * 70 + 9, 4096, 1024, False), (4100, 4304, 1152, True),
                                        (65792, 1024, 256, False), (300, 512, 2048, True)])
def test_gemm_gelu_grad_epilogue(M, N, K, tanh):
    """OV_EPI_GELU_GRAD_ERF / _TANH: C = bf16(bf16(A W^T) * gelu'(R)) -- the backward through the MLP's GELU folded into dy Wproj.
    Against fp64 gelu' from autograd; the polynomial erf form is within 4.3e-4 of the exact derivative, and both kernels (small and
    persistent grids) must agree with the two-step route (plain product, then ov_gelu_backward) to that bound + one bf16 rounding."""
    a, w = rnd(M, K, seed=40).to(torch.bfloat16).to(DEV), (rnd(N, K, seed=41) / K ** 0.5).to(torch.bfloat16).to(DEV)
    pre = (rnd(M, N, seed=42) * 1.5).to(torch.bfloat16).to(DEV)
    got = H.gemm(a, w, None, epi=5 if tanh else 4, resid=pre).float()
    dh = H.gemm(a, w, None, epi=0).double()
    x = pre.double().requires_grad_(True)
    torch.nn.functional.gelu(x, approximate="tanh" if tanh else "none").sum().backward()
    want = dh * x.grad
    err = (got.double() - want).abs()
    bound = dh.abs() * (6e-4 + 1.13 * 2 ** -8) + 1e-6               # polynomial + one bf16 rounding of a product <= 1.13 |dh|
    assert bool((err <= bound).all()), float((err - bound).max())
    two_step = H.gelu_backward(pre, H.gemm(a, w, None, epi=0), tanh).float()
    assert (got - two_step).abs().max().item() <= float((dh.abs() * (6e-4 + 1.13 * 2 ** -7)).max())


@pytest.mark.parametrize("M,N,K,epi", [(771, 3072, 1024, 0), (300, 768, 192, 1), (65535, 1024, 1024, 0), (200, 2304, 768, 2)])
def test_gemm_ln_fold_matches_layernorm_then_linear(M, N, K, epi):
    """ov_rowstats + ov_gemm_ln == Linear(LayerNorm(x)) (transformer.py:263-264) without materialising LN(x)."""
    x = (rnd(M, K, seed=30) * 1.7 + 0.4).to(torch.bfloat16)
    w, bias = rnd(N, K, seed=31) / K ** 0.5, rnd(N, seed=32) * 0.1
    gamma, beta = rnd(K, seed=33) * 0.1 + 1, rnd(K, seed=34) * 0.1
    wg = (w * gamma[None, :]).to(torch.bfloat16)
    colsum = wg.float().sum(1)
    cvec = w.to(torch.bfloat16).float() @ beta + bias
    xd = x.to(DEV)
    st = H.rowstats(xd)
    ref_mean = x.float().mean(1)
    np.testing.assert_allclose(st[:, 0].cpu().numpy(), ref_mean.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(st[:, 1].cpu().numpy(), (x.float().var(1, unbiased=False) + 1e-6).rsqrt().numpy(), rtol=1e-5)
    c = H.gemm_ln(xd, wg.to(DEV), cvec.to(DEV), colsum.to(DEV), st, epi=epi).float().cpu()
    ref = torch.nn.functional.linear(R.layer_norm(x.float(), gamma, beta), w, bias)
    if epi:
        ref = R.gelu(ref, epi == 2)
    np.testing.assert_allclose(c.numpy(), ref.numpy(), rtol=1.5e-2, atol=2e-2)


def test_gemm_residual_inplace():
    M, N, K = 514, 1024, 1024
    a, w, bias = rnd(M, K, seed=13).to(torch.bfloat16), (rnd(N, K, seed=14) / K ** 0.5).to(torch.bfloat16), rnd(N, seed=15)
    x = rnd(M, N, seed=16).to(torch.bfloat16)
    xd = x.to(DEV).clone()
    H.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), epi=3, resid=xd, out=xd)
    ref = x.float() + (a.float() @ w.float().T + bias)
    np.testing.assert_allclose(xd.float().cpu().numpy(), ref.numpy(), rtol=1e-2, atol=2e-2)


@pytest.mark.parametrize("B,g2,D,K", [(3, 100, 192, 768), (700, 100, 384, 192)])
def test_gemm_patch_embed_row_maps(B, g2, D, K):
    """(the second shape: the persistent kernel with row maps, a half last n-tile and the rotated walk -- S/8's patch embedding at batch)"""
    a, w = rnd(B * g2, K, seed=17).to(torch.bfloat16), (rnd(D, K, seed=18) / K ** 0.5).to(torch.bfloat16)
    pos = rnd(g2 + 1, D, seed=19).to(torch.bfloat16)
    out = torch.zeros(B * (g2 + 1), D, dtype=torch.bfloat16, device=DEV)
    H.gemm(a.to(DEV), w.to(DEV), None, epi=3, resid=pos.to(DEV), out=out, out_group=g2, resid_mod=g2, resid_off=1)
    ref = (a.float() @ w.float().T).view(B, g2, D) + pos[1:].float()
    got = out.float().cpu().view(B, g2 + 1, D)
    np.testing.assert_allclose(got[:, 1:].numpy(), ref.numpy(), rtol=1e-2, atol=1e-2)
    assert float(got[:, 0].abs().max()) == 0.0           # cls rows untouched


@pytest.mark.parametrize("B,L,H_", [(2, 257, 16), (3, 101, 3), (2, 80, 12), (1, 32, 1), (1, 577, 2), (1, 2305, 2),
                                    # streaming kernel (hipops.attn_route: form "streaming"): head counts off the XCD round, chunk tails of 1 / 33 / 64 keys
                                    (3, 321, 3), (1, 384, 2), (1, 449, 1), (1, 481, 5), (1, 2304, 1),
                                    # L = 32 k + 1: the lone query row is shared out over the k waves (XROW)
                                    (2, 33, 1), (3, 65, 2), (1, 129, 5), (2, 225, 3), (300, 257, 16)])
def test_attention(B, L, H_):
    D = H_ * 64
    qkv = rnd(B * L, 3 * D, seed=20).to(torch.bfloat16)
    o = H.attention(qkv.to(DEV), B, L, H_).float().cpu().view(B, L, D)
    q, k, v = qkv.float().view(B, L, 3 * D).split(D, dim=-1)
    sp = lambda t: t.reshape(B, L, H_, 64).transpose(1, 2)
    p = torch.softmax(sp(q) * 0.125 @ sp(k).transpose(-1, -2), dim=-1)
    ref = (p @ sp(v)).transpose(1, 2).reshape(B, L, D)
    # P is rounded to bf16 before P.V and the output is bf16: abs err ~ 2^-8 * |v| scale
    np.testing.assert_allclose(o.numpy(), ref.numpy(), rtol=2e-2, atol=1.5e-2)


@pytest.mark.parametrize("B,L,H_,hd", [(2, 257, 3, 80), (1, 101, 2, 72), (1, 300, 1, 80), (2, 80, 4, 72)])
def test_attention_generic_head_dim(B, L, H_, hd):
    D = H_ * hd
    qkv = rnd(B * L, 3 * D, seed=24).to(torch.bfloat16)
    o = H.attention(qkv.to(DEV), B, L, H_, hd).float().cpu().view(B, L, D)
    q, k, v = qkv.float().view(B, L, 3 * D).split(D, dim=-1)
    sp = lambda t: t.reshape(B, L, H_, hd).transpose(1, 2)
    p = torch.softmax(sp(q) * hd ** -0.5 @ sp(k).transpose(-1, -2), dim=-1)
    ref = (p @ sp(v)).transpose(1, 2).reshape(B, L, D)
    np.testing.assert_allclose(o.numpy(), ref.numpy(), rtol=2e-2, atol=1.5e-2)


@pytest.mark.parametrize("L,spike", [(257, 250), (705, 700)])
def test_attention_online_softmax_rescale_branch(L, spike):
    """Force the running max to jump late (a spiked key in the LAST tile) — cdna guide rule 26.  L = 705: streaming kernel."""
    B, H_ = 1, 1
    qkv = rnd(L, 192, seed=21).to(torch.bfloat16)
    qkv[spike, 64:128] = qkv[3, 0:64] * 6.0          # that key aligned with query 3 -> huge logit in the last tile
    o = H.attention(qkv.to(DEV), B, L, H_).float().cpu()
    q, k, v = qkv.float().split(64, dim=-1)
    ref = torch.softmax(q * 0.125 @ k.T, dim=-1) @ v
    np.testing.assert_allclose(o.numpy(), ref.numpy(), rtol=2e-2, atol=1.5e-2)


@pytest.mark.parametrize("b,N,E,off", [(16, 16, 192, 0), (4, 16, 192, 8), (256, 256, 768, 0), (100, 700, 384, 300),
                                       (33, 4100, 768, 4000)])
def test_clip_loss_terms(b, N, E, off):
    ai = torch.nn.functional.normalize(rnd(N, E, seed=22), dim=-1)
    at = torch.nn.functional.normalize(ai * 0.5 + rnd(N, E, seed=23) * 0.05, dim=-1)
    img, txt = ai[off:off + b].contiguous(), at[off:off + b].contiguous()
    s = 1 / 0.07
    loss, terms = H.clip_loss(img.to(DEV), txt.to(DEV), ai.to(DEV), at.to(DEV), s, off)
    rank_loss = (torch.nn.functional.cross_entropy(s * img @ at.T, torch.arange(b) + off) +
                 torch.nn.functional.cross_entropy(s * txt @ ai.T, torch.arange(b) + off)) / 2
    li = s * img @ at.T
    np.testing.assert_allclose(terms[0].cpu().numpy(), torch.logsumexp(li, 1).numpy(), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(terms[1].cpu().numpy(), li[torch.arange(b), torch.arange(b) + off].numpy(), rtol=1e-5, atol=2e-5)
    assert abs(float(loss) - float(rank_loss)) < 2e-5


@pytest.mark.timeout(600)
def test_clip_loss_config5_shape_b4096_n32768():
    """BASELINE.json config #5's loss shape (scripts/project/openvision/train.sh:18: global batch 32 768 = 8 ranks x 4 096): this
    rank's [4096, 32768] logit strips both ways, never materialised.  The CPU oracle (fp32 torch, loss.py:102-131 arithmetic) checks
    the per-row log-sum-exp and diagonal logit of 64 sampled rows per direction; the scalar loss must equal the mean of ALL rows'
    (lse - diag) as the kernel itself reports them (so every row is tied to the sampled check by the same code path)."""
    b, N, E, rank = 4096, 32768, 768, 5
    g = torch.Generator(device="cpu").manual_seed(77)
    ai = torch.nn.functional.normalize(torch.randn(N, E, generator=g), dim=-1)
    at = torch.nn.functional.normalize(ai * 0.35 + torch.randn(N, E, generator=g) * 0.04, dim=-1)
    off = rank * b
    s = 1 / 0.07
    dai, dat = ai.to(DEV), at.to(DEV)
    img, txt = dai[off:off + b].contiguous(), dat[off:off + b].contiguous()
    loss, terms = H.clip_loss(img, txt, dai, dat, s, off)
    terms = terms.cpu()
    rows = torch.randperm(b, generator=g)[:64]
    li = s * ai[off + rows] @ at.T                                   # [64, N] on the CPU
    lt = s * at[off + rows] @ ai.T
    np.testing.assert_allclose(terms[0][rows].numpy(), torch.logsumexp(li, 1).numpy(), rtol=2e-5, atol=5e-5)
    np.testing.assert_allclose(terms[1][rows].numpy(), li[torch.arange(64), off + rows].numpy(), rtol=2e-5, atol=5e-5)
    np.testing.assert_allclose(terms[2][rows].numpy(), torch.logsumexp(lt, 1).numpy(), rtol=2e-5, atol=5e-5)
    np.testing.assert_allclose(terms[3][rows].numpy(), lt[torch.arange(64), off + rows].numpy(), rtol=2e-5, atol=5e-5)
    want = ((terms[0] - terms[1]).double().mean() + (terms[2] - terms[3]).double().mean()) / 2
    assert abs(float(loss) - float(want)) < 2e-5
    assert 0.0 < float(loss) < np.log(N)                             # informative pairs: far below the uniform-guess loss
    # backward at the same shape: local-side gradient rows of the sampled set against the closed form (P recomputed on the CPU)
    d_img, d_txt, _, _, d_s = H.clip_loss_backward(img, txt, dai, dat, s, off, terms.to(DEV), grad=1.0, gathered=False)
    pi = torch.softmax(li, 1)
    pi[torch.arange(64), off + rows] -= 1.0
    ref = (s / (2 * b)) * pi @ at
    assert (d_img.cpu()[rows] - ref).abs().max() < 2e-6 + 1e-4 * ref.abs().max()


def test_clip_loss_golden_reference_ranks():
    from conftest import golden
    g = golden("cliploss_ws.npz")
    img, txt, s = torch.from_numpy(g["img"]), torch.from_numpy(g["txt"]), float(g["scale"])
    loss, _ = H.clip_loss(img.to(DEV), txt.to(DEV), img.to(DEV), txt.to(DEV), s, 0)
    assert abs(float(loss) - float(g["loss_ws1"])) < 1e-5
    for ws in (2, 8):
        b = 16 // ws
        for r in range(ws):
            l, _ = H.clip_loss(img[r * b:(r + 1) * b].contiguous().to(DEV), txt[r * b:(r + 1) * b].contiguous().to(DEV),
                               img.to(DEV), txt.to(DEV), s, r * b)
            assert abs(float(l) - float(g[f"local_losses_ws{ws}"][r])) < 1e-5


@pytest.mark.parametrize("b,N,E,off", [(16, 16, 192, 0), (4, 16, 192, 8), (256, 256, 768, 0), (100, 700, 384, 300),
                                       (33, 2100, 1152, 2000), (24, 48, 32, 24)])
def test_clip_loss_backward_vs_oracle(b, N, E, off):
    """ov_clip_loss_backward (local-side, gathered-side and scale gradients) vs the oracle's closed form; fp32 MFMA, so the
    tolerance is a few ulps of the largest term (1e-6 absolute on gradients of magnitude <= ~0.1)."""
    from oracle import clip_ref as R
    ai = torch.nn.functional.normalize(rnd(N, E, seed=32), dim=-1)
    at = torch.nn.functional.normalize(ai * 0.5 + rnd(N, E, seed=33) * 0.05, dim=-1)
    img, txt = ai[off:off + b].contiguous(), at[off:off + b].contiguous()
    s = 1 / 0.07
    _, terms = H.clip_loss(img.to(DEV), txt.to(DEV), ai.to(DEV), at.to(DEV), s, off)
    got = H.clip_loss_backward(img.to(DEV), txt.to(DEV), ai.to(DEV), at.to(DEV), s, off, terms, grad=0.5)
    # the oracle's rank argument is off / b; keep arbitrary offsets by differentiating the shifted problem directly
    di, dt = img @ at.T, txt @ ai.T
    idx = torch.arange(b) + off
    pi, pt = torch.softmax(s * di, 1), torch.softmax(s * dt, 1)
    pi[torch.arange(b), idx] -= 1
    pt[torch.arange(b), idx] -= 1
    pi, pt = 0.5 * pi / (2 * b), 0.5 * pt / (2 * b)
    want = (s * pi @ at, s * pt @ ai, s * pt.T @ txt, s * pi.T @ img, (pi * di).sum() + (pt * dt).sum())
    if off % b == 0:                         # and the oracle itself where its labelling applies
        ref = R.clip_loss_grads(img, txt, s, ai, at, off // b)
        for w, r in zip(want, ref):
            assert (w - 0.5 * r).abs().max() < 1e-6
    for name, g_, w in zip(("d_img", "d_txt", "d_all_img", "d_all_txt"), got[:4], want[:4]):
        np.testing.assert_allclose(g_.cpu().numpy(), w.numpy(), rtol=2e-4, atol=1e-6, err_msg=name)
    assert abs(float(got[4]) - float(want[4])) < 2e-6 + 2e-4 * abs(float(want[4]))
    only_local = H.clip_loss_backward(img.to(DEV), txt.to(DEV), ai.to(DEV), at.to(DEV), s, off, terms, grad=0.5, gathered=False)
    assert only_local[2] is None and torch.equal(only_local[0], got[0]) and torch.equal(only_local[1], got[1])   # deterministic


def test_clip_loss_autograd_golden_world_size_1():
    """openvision_amd.ClipLoss as an autograd node vs autograd through the reference ClipLoss (cliploss_grad.npz)."""
    from conftest import golden
    from openvision_amd.loss import ClipLoss
    g = golden("cliploss_grad.npz")
    img = torch.from_numpy(g["img"]).to(DEV).requires_grad_(True)
    txt = torch.from_numpy(g["txt"]).to(DEV).requires_grad_(True)
    s = torch.from_numpy(g["scale"]).to(DEV).requires_grad_(True)
    loss = ClipLoss()(img, txt, s)
    assert abs(float(loss.detach()) - float(g["loss_ws1"])) < 1e-5
    (loss * 1.0).backward()
    np.testing.assert_allclose(img.grad.cpu().numpy(), g["dimg_ws1"], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(txt.grad.cpu().numpy(), g["dtxt_ws1"], rtol=2e-4, atol=1e-6)
    assert abs(float(s.grad) - float(g["dscale_ws1"])) < 2e-6
    with torch.no_grad():                                        # the forward-only path is unchanged
        assert abs(float(ClipLoss()(img, txt, s)) - float(g["loss_ws1"])) < 1e-5


def _lossgrad_rank(rank, ws):
    from conftest import golden
    from openvision_amd.loss import ClipLoss
    g = golden("cliploss_grad.npz")
    b = g["img"].shape[0] // ws
    worst = {}
    for local_loss in (True, False):
        for gwg in (False, True):
            tag = f"ws2_local{int(local_loss)}_gwg{int(gwg)}"
            img = torch.from_numpy(g["img"][rank * b:(rank + 1) * b]).to(DEV).requires_grad_(True)
            txt = torch.from_numpy(g["txt"][rank * b:(rank + 1) * b]).to(DEV).requires_grad_(True)
            s = torch.from_numpy(g["scale"]).to(DEV).requires_grad_(True)
            loss = ClipLoss(local_loss=local_loss, gather_with_grad=gwg, rank=rank, world_size=ws)(img, txt, s)
            loss.backward()
            worst[tag] = (abs(float(loss.detach()) - float(g[tag + "_loss"][rank])),
                          float((img.grad.cpu() - torch.from_numpy(g[tag + "_dimg"][rank])).abs().max()),
                          float((txt.grad.cpu() - torch.from_numpy(g[tag + "_dtxt"][rank])).abs().max()),
                          abs(float(s.grad) - float(g[tag + "_dscale"][rank])))
    return worst


def test_clip_loss_autograd_golden_world_size_2():
    """Two ranks (gloo rendezvous, both on this one GPU): loss and gradients per rank vs the reference's, for every
    local_loss x gather_with_grad routing of gather_features (loss.py:19-63)."""
    res = run_ranks(_lossgrad_rank, 2, timeout=300, backend="gloo", gpu=True)
    for rank in range(2):
        for tag, (dl, di, dt, ds) in res[rank].items():
            assert dl < 1e-5 and di < 2e-6 and dt < 2e-6 and ds < 2e-6, (rank, tag, dl, di, dt, ds)


def bf(t):
    return t.to(torch.bfloat16)


@pytest.mark.parametrize("R,C", [(1, 8), (64, 64), (257, 200), (1000, 1024), (65, 4096)])
def test_transpose_bf16_exact(R, C):
    x = bf(rnd(R, C, seed=40))
    out = H.transpose(x.to(DEV)).cpu()
    assert torch.equal(out[:, :R], x.T)                                 # a permutation of bytes: bit-exact
    assert torch.count_nonzero(out[:, R:].float()) == 0                 # zero padding up to the GEMM's K granule


@pytest.mark.parametrize("M,N,K", [(70, 192, 128), (514, 768, 192), (1285, 3072, 1024), (2056, 1024, 4096)])
def test_linear_backward_vs_oracle(M, N, K):
    """dX / dW bf16 outputs of fp32-accumulated products: one bf16 rounding (2^-9 relative) on top of the oracle evaluated on
    the same bf16 inputs; db is an fp32 sum."""
    dy, x, w = bf(rnd(M, N, seed=41)), bf(rnd(M, K, seed=42)), bf(rnd(N, K, seed=43) * K ** -0.5)
    dx, dw, db = H.linear_backward(dy.to(DEV), x.to(DEV), w.to(DEV))
    rdx, rdw, rdb = R.linear_backward(dy, x, w)
    np.testing.assert_allclose(dx.float().cpu().numpy(), rdx.numpy(), rtol=1e-2, atol=2e-2 * float(rdx.abs().mean()))
    np.testing.assert_allclose(dw.float().cpu().numpy(), rdw.numpy(), rtol=1e-2, atol=2e-2 * float(rdw.abs().mean()))
    np.testing.assert_allclose(db.cpu().numpy(), rdb.numpy(), rtol=1e-5, atol=1e-4)
    only = H.linear_backward(dy.to(DEV), x.to(DEV), w.to(DEV), want=("db",))          # stand-alone column sums (other summation order)
    assert only[0] is None and only[1] is None
    np.testing.assert_allclose(only[2].cpu().numpy(), rdb.numpy(), rtol=1e-5, atol=1e-4)
    again = H.linear_backward(dy.to(DEV), x.to(DEV), w.to(DEV))
    assert torch.equal(again[2], db) and torch.equal(again[1], dw) and torch.equal(again[0], dx)   # deterministic


@pytest.mark.parametrize("rows,D", [(37, 192), (514, 768), (1285, 1024), (9, 1152), (5, 4096)])
def test_layernorm_backward_vs_oracle(rows, D):
    x, dy = bf(rnd(rows, D, seed=44) * 1.5 + 0.2), bf(rnd(rows, D, seed=45))
    w = rnd(D, seed=46) * 0.1 + 1
    dx, dg, db = H.layernorm_backward(x.to(DEV), w.to(DEV), dy.to(DEV))
    rdx, rdg, rdb = R.layer_norm_backward(x, w, dy, 1e-6)
    np.testing.assert_allclose(dx.float().cpu().numpy(), rdx.numpy(), rtol=1e-2, atol=1e-2)      # bf16 output
    np.testing.assert_allclose(dg.cpu().numpy(), rdg.numpy(), rtol=1e-4, atol=1e-3)             # fp32 sums over rows
    np.testing.assert_allclose(db.cpu().numpy(), rdb.numpy(), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("tanh", [False, True])
def test_gelu_backward_vs_oracle_and_golden(tanh):
    from conftest import golden
    a, dh = bf(rnd(300, 1536, seed=47) * 2.0), bf(rnd(300, 1536, seed=48))
    da = H.gelu_backward(a.to(DEV), dh.to(DEV), tanh).float().cpu()
    ref = R.gelu_backward(a, dh, tanh)
    np.testing.assert_allclose(da.numpy(), ref.numpy(), rtol=1e-2, atol=1e-3)                    # bf16 output; derivative error < 1e-6
    g = golden("opgrad.npz")
    name = "tanh" if tanh else "erf"
    ga = torch.from_numpy(g[f"gelu_{name}_a"])[:384].reshape(1, 384)
    one = torch.ones(1, 384)
    d = H.gelu_backward(bf(ga).to(DEV), bf(one).to(DEV), tanh).float().cpu()
    want = R.gelu_backward(bf(ga), one, tanh)
    np.testing.assert_allclose(d.numpy(), want.numpy(), rtol=8e-3, atol=1e-3)


@pytest.mark.parametrize("B,L,H", [(2, 257, 16), (3, 65, 2), (1, 33, 1), (2, 80, 12), (1, 288, 1), (2, 5, 1), (1, 1, 1), (2, 101, 3),
                                   (1, 289, 2), (2, 513, 3), (1, 2305, 6), (1, 1000, 1)])
def test_attention_backward_vs_oracle(B, L, H):
    """dQ | dK | dV of the softmax attention vs the oracle's closed form on the same bf16 inputs.  P and dS are rounded to bf16 for
    the second products (as the forward rounds P) and the outputs are bf16: 2e-2 relative of the gradient scale."""
    qkv = bf(rnd(B * L, 3 * H * 64, seed=50))
    dout = bf(rnd(B * L, H * 64, seed=51))
    out = H_.attention(qkv.to(DEV), B, L, H)
    dqkv = H_.attention_backward(qkv.to(DEV), out, dout.to(DEV), B, L, H).float().cpu()
    q, k, v = [t.view(B, L, H, 64).transpose(1, 2) for t in qkv.float().view(B, L, 3 * H * 64).split(H * 64, dim=-1)]
    do = dout.float().view(B, L, H, 64).transpose(1, 2)
    ref = torch.cat([t.transpose(1, 2).reshape(B * L, H * 64) for t in R.attention_backward(q, k, v, do, 0.125)], dim=-1)
    for name, sl in (("dq", slice(0, H * 64)), ("dk", slice(H * 64, 2 * H * 64)), ("dv", slice(2 * H * 64, 3 * H * 64))):
        got, want = dqkv[:, sl], ref[:, sl]
        tol = 2e-2 * float(want.abs().max()) + 1e-3
        assert float((got - want).abs().max()) < tol, (name, float((got - want).abs().max()), tol)
    again = H_.attention_backward(qkv.to(DEV), out, dout.to(DEV), B, L, H).float().cpu()
    assert torch.equal(again, dqkv)                                       # deterministic


@pytest.mark.parametrize("B,L,H", [(2, 257, 4), (3, 80, 8), (1, 33, 2), (5, 288, 3), (2, 256, 16), (1, 1, 1)])
def test_attention_keeps_the_row_lse_for_the_backward(B, L, H):
    """ov_attention_lse = ov_attention plus the row log-sum-exp (log2 units) of the scaled scores; ov_attention_backward_saved with it
    skips its own score pass.  The output is bitwise ov_attention's, the lse matches fp64 logsumexp, and the gradients match the
    recomputing backward to the bf16 resolution of dS (the two lse differ in the last fp32 bits only)."""
    qkv = bf(rnd(B * L, 3 * H * 64, seed=60)).to(DEV)
    dout = bf(rnd(B * L, H * 64, seed=61)).to(DEV)
    out, lse = H_.attention_lse(qkv, B, L, H)
    assert torch.equal(out, H_.attention(qkv, B, L, H))
    q, k = [t.view(B, L, H, 64).transpose(1, 2).double() for t in qkv.view(B, L, 3 * H * 64).split(H * 64, dim=-1)[:2]]
    want = torch.logsumexp(q @ k.transpose(-1, -2) * 0.125, dim=-1) / np.log(2.0)          # [B, H, L], log2 units
    got = lse.view(B, H, -1)[:, :, :L].double()
    assert float((got - want).abs().max()) < 2e-5
    a = H_.attention_backward_saved(qkv, out, dout, lse, B, L, H).float()
    b = H_.attention_backward(qkv, out, dout, B, L, H).float()
    assert float((a - b).abs().max()) <= 2 ** -7 * float(b.abs().max()) + 1e-6
    with pytest.raises(H_._lib.OvhipError):
        H_.attention_lse(bf(rnd(2 * 300, 3 * 64, seed=1)).to(DEV), 2, 300, 1)          # beyond the resident backward's L


@pytest.mark.parametrize("B,L,H,hd", [(2, 257, 4, 72), (2, 257, 3, 80), (1, 40, 2, 72), (1, 300, 2, 80), (1, 65, 2, 32),
                                        # long sequences: three or four 256-row chunks, NDH = 3 (72, 80, 96) and NDH = 2 (48);
                                        # 769 and 513 end in a chunk of one row
                                        (1, 577, 2, 80), (1, 730, 2, 72), (1, 769, 1, 96), (2, 513, 2, 48)])
def test_attention_backward_other_head_dims(B, L, H, hd):
    """Head dims 72 (So400m) and 80 (H/14) go through the streaming kernels with the d axis zero-padded to 96 in LDS; deterministic."""
    qkv = bf(rnd(B * L, 3 * H * hd, seed=52))
    dout = bf(rnd(B * L, H * hd, seed=53))
    out = H_.attention(qkv.to(DEV), B, L, H, hd)
    dqkv = H_.attention_backward(qkv.to(DEV), out, dout.to(DEV), B, L, H, hd).float().cpu()
    q, k, v = [t.view(B, L, H, hd).transpose(1, 2) for t in qkv.float().view(B, L, 3 * H * hd).split(H * hd, dim=-1)]
    do = dout.float().view(B, L, H, hd).transpose(1, 2)
    ref = torch.cat([t.transpose(1, 2).reshape(B * L, H * hd) for t in R.attention_backward(q, k, v, do, hd ** -0.5)], dim=-1)
    for name, sl in (("dq", slice(0, H * hd)), ("dk", slice(H * hd, 2 * H * hd)), ("dv", slice(2 * H * hd, 3 * H * hd))):
        got, want = dqkv[:, sl], ref[:, sl]
        tol = 2e-2 * float(want.abs().max()) + 1e-3
        assert float((got - want).abs().max()) < tol, (name, float((got - want).abs().max()), tol)
    again = H_.attention_backward(qkv.to(DEV), out, dout.to(DEV), B, L, H, hd).float().cpu()
    assert torch.equal(again, dqkv)                                       # deterministic


def test_attention_backward_golden_reference():
    """Through the reference block's attention module (opgrad.npz): d x = dqkv W_in with an identity out-projection."""
    from conftest import golden
    g = {k: torch.from_numpy(v) for k, v in golden("opgrad.npz").items()}
    x, w, dy = g["mha_x"], g["mha_w"], g["mha_dy"]
    B, L, D = x.shape
    qkv = bf((x @ w.T).reshape(B * L, 3 * D))
    out = H_.attention(qkv.to(DEV), B, L, 2)
    dqkv = H_.attention_backward(qkv.to(DEV), out, bf(dy.reshape(B * L, D)).to(DEV), B, L, 2).float().cpu()
    dx = (dqkv @ w).view(B, L, D)
    assert float((dx - g["mha_dx"]).abs().max()) < 3e-2 * float(g["mha_dx"].abs().max()) + 2e-3


_block_case = H_.block_case          # (the chain tests draw the same blocks: hipops.block_case)


@pytest.mark.parametrize("D,heads,mlp,B,L,tanh", [(1024, 16, 4096, 72, 257, False), (768, 12, 3072, 256, 80, True), (192, 3, 768, 4, 101, False),
                                                  (1152, 16, 4304, 6, 257, False), (384, 6, 1536, 2, 700, False), (1280, 16, 5120, 3, 257, False)])
def test_kept_activation_backward_matches_the_recomputing_backward(D, heads, mlp, B, L, tanh):
    """ov_tower_forward_saving + ov_tower_backward (pre-activation from the GELU epilogue's second output, GELU derivative inside
    dy Wproj, bias gradients out of the TN kernel, attention row lse from the forward) against ov_block_backward on the block input
    alone (everything recomputed, element-wise GELU backward with the A&S erf): the same gradients up to the bf16 resolution of the
    intermediates.  The first two shapes are large enough for the PERSISTENT kernels (> 256 tiles per product), which the model-level
    gradient tests (Tiny, small batches) never reach."""
    from openvision_amd import _lib as L_
    mlp_pad = (mlp + 63) // 64 * 64            # So400m: 4304 -> 4352 (zero rows / columns); head dims 72 and 80: no kept lse; L = 700: streaming
    names, sd, dev, x, dy = _block_case(D, heads, mlp, B, L, tanh, 70, mlp_pad=mlp_pad)
    cfg = L_.TowerCfg(D, 1, heads, mlp, mlp_pad, int(tanh), 1e-6)
    xd, dyd = x.reshape(B * L, D).to(DEV), dy.reshape(B * L, D).to(DEV)
    _, dx_k, g_k = H_.tower1_forward_backward(cfg, dev, xd, dyd, B, L)
    dx_r, g_r = H_.block_backward(cfg, dev, xd, dyd, B, L)
    def close(a, b, what):
        a, b = a.float(), b.float()
        err = float((a - b).abs().max())
        rel = float((a - b).norm() / b.norm().clamp_min(1e-20))
        assert err < 2e-2 * float(b.abs().max()) + 1e-6 and rel < 1e-2, (what, err, float(b.abs().max()), rel)
    close(dx_k, dx_r, "dx")
    for k in names:
        close(g_k[k], g_r[k], k)


@pytest.mark.parametrize("D,heads,mlp,B,L,tanh", [(192, 3, 768, 2, 101, False), (1024, 16, 4096, 2, 257, False), (768, 12, 3072, 3, 80, True),
                                                  (384, 6, 1536, 1, 700, False)])
def test_block_backward_vs_oracle(D, heads, mlp, B, L, tanh):
    """ov_block_backward (recompute + chain rule through the HIP operators) vs the oracle's closed-form block backward in fp32 on the
    same bf16 weights and inputs.  Every intermediate of the HIP path is bf16, so the comparison is relative to each gradient's
    scale: 4e-2 of its maximum (weights: Frobenius-relative 2e-2).  (Every stage of the chain under its operator's per-element fp64
    bound, on the stage's own inputs: test_gpu_block_chain.py.)"""
    from openvision_amd import _lib as L_
    names, sd, dev, x, dy = _block_case(D, heads, mlp, B, L, tanh, 60)
    cfg = L_.TowerCfg(D, 1, heads, mlp, mlp, int(tanh), 1e-6)
    dx, grads = H_.block_backward(cfg, dev, x.reshape(B * L, D).to(DEV), dy.reshape(B * L, D).to(DEV), B, L)
    rdx, rg = R.resblock_backward(x, dy, sd, "b.", heads, tanh, 1e-6)
    err = float((dx.float().cpu().view(B, L, D) - rdx).abs().max())
    assert err < 4e-2 * float(rdx.abs().max()), ("dx", err, float(rdx.abs().max()))
    for k, (ref, shape, _, _) in names.items():
        got, want = grads[k].float().cpu(), rg[ref]
        if len(shape) == 2:
            rel = float((got - want).norm() / want.norm())
            assert rel < 2e-2, (k, rel)
        else:
            e = float((got - want).abs().max())
            assert e < 4e-2 * float(want.abs().max()) + 1e-3, (k, e, float(want.abs().max()))


def test_block_backward_head_dim_72_and_padded_mlp():
    """So400m-like block: head_dim 72 and an MLP width (int(D * 3.7362)) that the kernels pad to a multiple of 64.  (The padded chain
    stage by stage under per-element fp64 bounds: test_gpu_block_chain.py, shape hd80_l257_padmlp.)"""
    from openvision_amd import _lib as L_
    D, heads, mlp, B, L = 576, 8, 2152, 2, 257
    mlp_pad = 2176
    names, sd, dev, x, dy = _block_case(D, heads, mlp, B, L, False, 70, mlp_pad=mlp_pad)
    cfg = L_.TowerCfg(D, 1, heads, mlp, mlp_pad, 0, 1e-6)
    dx, grads = H_.block_backward(cfg, dev, x.reshape(B * L, D).to(DEV), dy.reshape(B * L, D).to(DEV), B, L)
    rdx, rg = R.resblock_backward(x, dy, sd, "b.", heads, False, 1e-6)
    assert float((dx.float().cpu().view(B, L, D) - rdx).abs().max()) < 4e-2 * float(rdx.abs().max())
    for k, (ref, shape, _, _) in names.items():
        got, want = grads[k].float().cpu(), rg[ref]
        if k in ("fc_w", "fc_b"):
            assert float(got[mlp:].abs().max()) == 0.0            # the padding rows receive exactly zero
            got = got[:mlp]
        if k == "proj_w":
            got = got[:, :mlp]
        if len(shape) == 2:
            assert float((got - want).norm() / want.norm()) < 2e-2, k
        else:
            assert float((got - want).abs().max()) < 4e-2 * float(want.abs().max()) + 1e-3, k


def test_block_backward_golden_reference():
    """The Tiny block 0 of the formula weights against autograd through the reference ResidualAttentionBlock (blockgrad.npz)."""
    from conftest import golden
    from openvision_amd import _lib as L_, config as ovcfg, synth
    g = golden("blockgrad.npz")
    sd = synth.make_state_dict(ovcfg.preset("vit-tiny-patch16-160"), 0)
    p = "visual.transformer.resblocks.0."
    ref_names = {"ln1_w": "ln_1.weight", "ln1_b": "ln_1.bias", "qkv_w": "attn.in_proj_weight", "qkv_b": "attn.in_proj_bias",
                 "out_w": "attn.out_proj.weight", "out_b": "attn.out_proj.bias", "ln2_w": "ln_2.weight", "ln2_b": "ln_2.bias",
                 "fc_w": "mlp.c_fc.weight", "fc_b": "mlp.c_fc.bias", "proj_w": "mlp.c_proj.weight", "proj_b": "mlp.c_proj.bias"}
    dev = {k: (bf(sd[p + r]) if sd[p + r].dim() == 2 else sd[p + r].float()).contiguous().to(DEV) for k, r in ref_names.items()}
    x, dy = torch.from_numpy(g["x"]), torch.from_numpy(g["dy"])
    cfg = L_.TowerCfg(192, 1, 3, 768, 768, 0, 1e-6)
    dx, grads = H_.block_backward(cfg, dev, bf(x).reshape(202, 192).to(DEV), bf(dy).reshape(202, 192).to(DEV), 2, 101)
    want = torch.from_numpy(g["dx"])
    assert float((dx.float().cpu().view(2, 101, 192) - want).abs().max()) < 5e-2 * float(want.abs().max())
    for k, r in ref_names.items():
        got = grads[k].float().cpu()
        if got.dim() == 2:
            norm = float(g["g." + r + ".norm"])
            assert abs(float(got.double().norm()) - norm) < 3e-2 * norm, k
            head = torch.from_numpy(g["g." + r + ".head"])
            assert float((got[:6] - head).abs().max()) < 6e-2 * float(head.abs().max()) + 1e-3, k
        else:
            w = torch.from_numpy(g["g." + r])
            assert float((got - w).abs().max()) < 5e-2 * float(w.abs().max()) + 1e-3, k


def test_operator_backward_golden_reference():
    """LayerNorm and Linear backward through the C ABI vs autograd through the reference's modules (opgrad.npz), on the
    golden's inputs rounded to bf16 (the kernels' I/O type): tolerance = bf16 input and output rounding."""
    from conftest import golden
    g = {k: torch.from_numpy(v) for k, v in golden("opgrad.npz").items()}
    dx, dg, db = H.layernorm_backward(bf(g["ln_x"]).to(DEV), g["ln_w"].to(DEV), bf(g["ln_dy"]).to(DEV))
    np.testing.assert_allclose(dx.float().cpu().numpy(), g["ln_dx"].numpy(), rtol=3e-2, atol=3e-2)
    np.testing.assert_allclose(dg.cpu().numpy(), g["ln_dw"].numpy(), rtol=3e-2, atol=8e-2)
    np.testing.assert_allclose(db.cpu().numpy(), g["ln_db"].numpy(), rtol=3e-2, atol=8e-2)
    dx, dw, db = H.linear_backward(bf(g["lin_dy"]).to(DEV), bf(g["lin_x"]).to(DEV), bf(g["lin_w"]).to(DEV))
    np.testing.assert_allclose(dx.float().cpu().numpy(), g["lin_dx"].numpy(), rtol=3e-2, atol=3e-2)
    np.testing.assert_allclose(dw.float().cpu().numpy(), g["lin_dw"].numpy(), rtol=3e-2, atol=2e-1)
    np.testing.assert_allclose(db.cpu().numpy(), g["lin_db"].numpy(), rtol=3e-2, atol=1e-1)


@pytest.mark.parametrize("M,N,K,epi", [(256, 256, 384, 0), (300, 520, 512, 0), (771, 3072, 1024, 1), (2048, 1024, 4096, 3),
                                       (65535, 1024, 1024, 0)])
def test_gemm_fp8_matches_dequantised_fp32(M, N, K, epi):
    """BASELINE.json config #5 building block: fp8 e4m3 operands on the MX-scaled MFMA (unit block scales), per-row / per-channel
    dequantisation in the epilogue.  fp8 x fp8 products are exact in fp32, so the only differences from an fp32 matmul of the
    dequantised operands are the accumulation order and the bf16 rounding of the output."""
    a = rnd(M, K, seed=40) * (rnd(M, 1, seed=41).abs() * 3 + 0.2)
    w = rnd(N, K, seed=42) / K ** 0.5
    bias = rnd(N, seed=43)
    aq, rs = H.quantize_rows_e4m3(a.to(DEV))
    wq, cs = H.quantize_rows_e4m3(w.to(DEV))
    res = rnd(M, N, seed=44).to(torch.bfloat16) if epi == 3 else None
    out = H.gemm_fp8(aq, wq, rs, cs, bias.to(DEV), epi, res.to(DEV) if res is not None else None).float().cpu()
    ad = (aq.view(torch.float8_e4m3fn).float() * rs[:, None]).cpu()
    wd = (wq.view(torch.float8_e4m3fn).float() * cs[:, None]).cpu()
    ref = ad.double() @ wd.double().T + bias.double()
    if epi == 1:
        ref = torch.nn.functional.gelu(ref)
    if epi == 3:
        ref = ref + res.double()
    np.testing.assert_allclose(out.numpy(), ref.float().numpy(), rtol=1e-2, atol=2e-2)
    # and the quantisation itself stays within e4m3 resolution (2^-4 relative) of the unquantised product at the GEMM level
    full = a.double() @ w.double().T + bias.double()
    if epi == 0:
        rel = (ref - full).norm() / full.norm()
        assert rel < 0.05, rel


def test_gemm_fp8_rejects_unsupported():
    aq = torch.zeros(256, 128, dtype=torch.uint8, device=DEV)
    s1 = torch.ones(256, device=DEV)
    with pytest.raises(Exception):
        H.gemm_fp8(aq, aq, s1, s1)                # K = 128 < 384


@pytest.mark.parametrize("rows,D", [(5, 192), (771, 1024), (300, 4096), (64, 768)])
def test_quant_rows_fp8(rows, D):
    """Row quantisation to e4m3 (bit-exact against torch's own round-to-nearest-even cast) and the fused LayerNorm variant."""
    x = (rnd(rows, D, seed=50) * (rnd(rows, 1, seed=51).abs() * 4 + 0.1)).to(torch.bfloat16)
    q, sc = H.quant_rows_fp8(x.to(DEV))
    amax = x.float().abs().amax(1)
    np.testing.assert_allclose(sc.cpu().numpy(), (amax / 448.0).numpy(), rtol=1e-6)
    scaled = x.float() * (448.0 / amax)[:, None]
    ref = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    qc = q.cpu()
    diff = qc != ref
    if diff.any():                       # v_cvt_pk_fp8_f32 against torch's CPU cast: adjacent codes only, and rarely
        gd = qc.view(torch.float8_e4m3fn).float()[diff]
        rd = ref.view(torch.float8_e4m3fn).float()[diff]
        sd = scaled[diff]
        print(f"fp8 cast differences: {int(diff.sum())} of {diff.numel()}; e.g. value {sd[0].item():.6f} -> hw {gd[0].item()} torch {rd[0].item()}")
        assert (qc.int() - ref.int()).abs()[diff].max() <= 1
        assert diff.float().mean() < 0.01
    assert ((qc.view(torch.float8_e4m3fn).float() - scaled).abs() <= scaled.abs() * 0.0625 + 2.0 ** -9).all()   # half an e4m3 step
    gamma, beta = rnd(D, seed=52) * 0.1 + 1, rnd(D, seed=53) * 0.1
    ql, scl = H.quant_rows_fp8(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6)
    y = R.layer_norm(x.float(), gamma, beta)
    deq = ql.cpu().view(torch.float8_e4m3fn).float() * scl.cpu()[:, None]
    # e4m3: 3 mantissa bits -> relative step 2^-3, half a step of rounding error relative to the row maximum's binade
    assert (deq - y).abs().max() <= (y.abs().amax(1, keepdim=True) / 448.0 * 16.0 + 1e-6).max()
    np.testing.assert_allclose(scl.cpu().numpy(), (y.abs().amax(1) / 448.0).numpy(), rtol=2e-5)


def test_gemm_fp8_static_scales():
    """c_fc -> c_proj hand-over with a static scale: the first GEMM writes e4m3 bytes (scale 2 * amax / 448), the second reads them
    with that scalar scale; both against fp32 arithmetic on the same quantised data."""
    M, D_, F_ = 1000, 1024, 4096
    a = rnd(M, D_, seed=60)
    w1, b1 = rnd(F_, D_, seed=61) / D_ ** 0.5, rnd(F_, seed=62) * 0.1
    w2, b2 = rnd(D_, F_, seed=63) / F_ ** 0.5, rnd(D_, seed=64) * 0.1
    res = rnd(M, D_, seed=65).to(torch.bfloat16)
    aq, rs = H.quantize_rows_e4m3(a.to(DEV)); w1q, c1 = H.quantize_rows_e4m3(w1.to(DEV)); w2q, c2 = H.quantize_rows_e4m3(w2.to(DEV))
    deq = lambda q, s_: q.view(torch.float8_e4m3fn).float() * s_[:, None]
    hid = torch.nn.functional.gelu(deq(aq, rs) @ deq(w1q, c1).T + b1.to(DEV))
    amax = hid.abs().max().reshape(1).contiguous()
    nxt = torch.zeros(1, device=DEV)
    h8 = H.gemm_fp8_static(aq, w1q, c1, b1.to(DEV), 1, rowscale=rs, out_amax=amax, amax_next=nxt)
    assert abs(nxt.item() - amax.item()) <= 1e-3 * amax.item() + 1e-3          # delayed scaling: the running maximum of |C|
    sc = 2.0 * amax / 448.0
    hq = h8.view(torch.float8_e4m3fn).float() * sc
    assert (hq - hid).abs().max() <= hid.abs().max() * 0.07 + 1e-3              # e4m3 step relative to the element's own magnitude
    # e4m3 half step (2^-4 relative; the hardware cast breaks near-ties downwards), one subnormal step, and the kernel's polynomial
    # erf-GELU (|err| <= 1.4e-4 |x| on the pre-activation, here |x| < 8)
    err, bound = (hq - hid).abs(), hid.abs() * 0.0725 + sc * 2.0 ** -9 * 1.01 + 1.2e-3
    worst = (err - bound).argmax()
    assert (err <= bound).all(), (hid.flatten()[worst].item(), hq.flatten()[worst].item(), sc.item())
    out = H.gemm_fp8_static(h8, w2q, c2, b2.to(DEV), 3, in_amax=amax, resid=res.to(DEV)).float()
    ref = hq @ deq(w2q, c2).T + b2.to(DEV) + res.to(DEV).float()
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=1e-2, atol=2e-2)


@pytest.mark.parametrize("B,L,H_", [(2, 257, 4), (3, 128, 2), (1, 577, 3), (2, 2305, 1)])
def test_attention_fp8_output(B, L, H_):
    """e4m3 epilogue of the persistent (9-wave and <= 8-wave) and streaming attention kernels: equal to quantising the bf16 kernel's
    own fp32 result with the static scale, up to the bf16 rounding that the bf16 path adds and the e4m3 step."""
    D = H_ * 64
    qkv = rnd(B * L, 3 * D, seed=70).to(torch.bfloat16).to(DEV)
    ref = H.attention(qkv, B, L, H_).float()
    amax = ref.abs().max().reshape(1).contiguous()
    nxt = torch.zeros(1, device=DEV)
    o8 = H.attention_fp8out(qkv, B, L, H_, amax, nxt)
    assert abs(nxt.item() - amax.item()) <= 0.01 * amax.item()                 # running maximum (ref is the bf16-rounded output)
    sc = 2.0 * amax / 448.0
    deq = o8.view(torch.float8_e4m3fn).float() * sc
    assert ((deq - ref).abs() <= ref.abs() * 0.075 + sc * 2.0 ** -9 * 1.01 + 1e-6).all()


@pytest.mark.parametrize("Mc,NI,NJ,chunk", [(256, 256, 256, 256), (640, 192, 320, 256), (8192, 1024, 1024, 2048), (4096, 3072, 768, 1024),
                                            (65792, 1024, 1024, 8256)])
def test_gemm_tn_matches_transposed_operands(Mc, NI, NJ, chunk):
    """ov_gemm_tn_batched (C = P^T Q straight from the row-major operands, transposing LDS reads) against (a) fp32 torch per split-K
    range and (b) the explicit-transpose route it replaces in ov_linear_backward (ov_transpose_bf16 + ov_gemm_batched): the same
    products accumulated in the same order, so (b) must match BIT FOR BIT."""
    g = torch.Generator().manual_seed(Mc + NI)
    p = (torch.randn(Mc, NI, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    q = (torch.randn(Mc, NJ, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    got, psum = H.gemm_tn_batched(p, q, chunk, sums=True)
    assert torch.equal(got, H.gemm_tn_batched(p, q, chunk))      # the column-sum MFMAs leave the product alone
    batch = got.shape[0]
    for z in range(batch):                                        # bias-gradient partials: fp32 sums of bf16 values, any order
        want = p[z * chunk:min(Mc, (z + 1) * chunk)].double().sum(0)
        assert (psum[z].double() - want).abs().max().item() < 1e-5 * chunk ** 0.5 * 8 + 1e-4, z
    pt, qt = H.transpose(p), H.transpose(q)                       # [NI, Mc], [NJ, Mc] (Mc % 64 == 0: no padding)
    ref2 = torch.empty_like(got)
    for z in range(batch):
        k0, k1 = z * chunk, min(Mc, (z + 1) * chunk)
        want = p[k0:k1].float().T @ q[k0:k1].float()
        err = (got[z].float() - want).abs().max().item()
        assert err < 0.02 * (k1 - k0) ** 0.5 * 0.25 + 0.05, (z, err)
        ref2[z] = H.gemm(pt[:, k0:k1], qt[:, k0:k1], None, epi=0)
    assert torch.equal(got, ref2)


@pytest.mark.parametrize("M,N,K", [(65535, 1024, 1024), (65792, 1024, 256), (257, 1024, 4096), (1500, 768, 320), (12336, 1024, 256), (300, 192, 192),
                                   (66000, 384, 256)])
def test_gemm_rowparts_are_the_row_partial_sums_of_the_output(M, N, K):
    """ov_gemm_rowparts: the residual GEMM leaves {sum, sum of squares} of every 32-column group of its OUTPUT rows -- from the
    persistent kernel's epilogue (first two shapes: whole tiles and a ragged last row tile), from the skinny kernel's (M = 257, 300,
    1500) or from the stand-alone pass behind the non-persistent kernel (M = 12336: 196 tiles) -- bitwise what ov_rowparts computes
    from the stored output (one association order everywhere: a row's statistics must not depend on the kernel that wrote it), the
    output itself bitwise the plain residual GEMM's, and ov_rowstats_finalize on them within fp32 rounding of the two-pass
    ov_rowstats (transformer.py:15-30: the LayerNorm the folded QKV / c_fc GEMMs apply)."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    r = (torch.randn(M, N, generator=g) * 3 + 0.7).to(torch.bfloat16).to(DEV)       # a mean comparable to the spread
    want = H.gemm(a, w, b, epi=3, resid=r)
    out, parts = H.gemm_rowparts(a, w, b, r)
    assert torch.equal(out, want)
    ref = H.rowparts(out)
    assert not torch.isnan(parts).any()
    assert torch.equal(parts, ref)
    x = out.float()
    np.testing.assert_allclose(ref[..., 0].cpu().numpy(), x.view(M, N // 32, 32).sum(-1).cpu().numpy(), rtol=1e-5, atol=1e-4)
    st, st2 = H.rowstats_finalize(parts), H.rowstats(out)
    assert (st[:, 0] - st2[:, 0]).abs().max().item() < 1e-5 and ((st[:, 1] - st2[:, 1]).abs() / st2[:, 1]).max().item() < 2e-5
    # in place (C aliases R, as the tower calls it): the same
    x2 = r.clone()
    _, parts2 = H.gemm_rowparts(a, w, b, x2, out=x2)
    assert torch.equal(x2, want) and torch.equal(parts2, ref)


@pytest.mark.parametrize("variant", ["2", "4"])
def test_gemm_kernel_variants_agree_bitwise_with_the_default(variant):
    """OVHIP_GEMM_VARIANT (read once per process, so each variant runs in a child process): the non-persistent ping-pong kernel (2)
    and the skinny small-M kernel forced onto every shape (4: by default it serves grids of <= 96 of the big kernels' tiles)
    accumulate the same products in the same order and share the epilogue arithmetic: every epilogue's output must equal the default
    persistent kernel's bit for bit, on ragged shapes too."""
    import tempfile
    code = r"""
import torch
import hipops as H
g = torch.Generator().manual_seed(3)
outs = []
# (the last three: a last n-tile with <= 128 valid columns -- the persistent kernel's half tiles, rotated walk at tiles_n = 2)
for (M, N, K) in ((2048, 1024, 256), (65792, 1024, 256), (1500, 776, 320), (70001, 384, 384), (66000, 1152, 192), (66100, 632, 256),
                  (70000, 128, 192), (66000, 72, 256),         # (a single n-tile that is a half tile)
                  (66000, 256, 512)):                           # (K >= 2 N: the residual epilogue walks the row tiles in descending order)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda(); w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).cuda()
    b = torch.randn(N, generator=g).cuda(); r = torch.randn(M, N, generator=g).to(torch.bfloat16).cuda()
    for epi in (0, 1, 2, 3, 4):
        outs.append(H.gemm(a, w, b, epi=epi, resid=r if epi >= 3 else None).cpu())
    if N in (384, 1152):                       # the LN-folded forms (QKV: LDS-transposed stores; c_fc: direct stores)
        st = H.rowstats(a); cs = w.float().sum(1)
        for epi in (0, 1):
            outs.append(H.gemm_ln(a, w, b, cs, st, epi=epi).cpu())
torch.save(outs, sys.argv[1])
"""
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for v in ("0", variant):
            path = os.path.join(d, f"v{v}.pt")
            run_child(code, path, env={"OVHIP_GEMM_VARIANT": v}, timeout=600, gpu=True)
            res[v] = torch.load(path)
    assert len(res["0"]) == 49
    for i, (x, y) in enumerate(zip(res["0"], res[variant])):
        assert torch.equal(x, y), (variant, i)
