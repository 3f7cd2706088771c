"""Attention forward at the edges the round-3 kernels introduced, against an fp64 reference with a per-element bound.

Every L = 32 k + 1 (patches + CLS) ends in a key tile -- or, in the streaming kernel, a 64-key chunk -- that holds ONE key; the three
forward kernels fold that key in on the VALU (its own dot product, its own lazy rescale, its own rule that the two lane halves count it
once).  The generic head_dim kernel stages 256-key chunks where the route says chunked.  A fixed absolute tolerance cannot see a
mistake in either: the output scale shrinks as L grows, and the lone key is one of L terms.  So these tests compare with

    |got - ref| <= 2^-8 |ref| + 2^-8 (P.|V|) + 1e-6          (ref = softmax(Q K^T * scale) V in fp64 on the bf16 inputs)

The first term covers the bf16 output rounding (half an ulp is <= 2^-8 relative: 8 significant bits), the second the rounding of P to
bf16 before P.V (<= 2^-8 of each term).  The reference, the bound and the spiked inputs live in hipops.py; test_attention_bound.py (CPU) pins what
the bound can see: an emulation of the kernel arithmetic stays well inside it, and the same emulation with a dropped,
double-counted or unrescaled lone key lands outside it."""
import json
import os
import tempfile

import pytest
import torch

import hipops as H
from hipops import LONE_SPIKED, attn_ref64, bound, err_ratio, rnd, spiked_qkv
from ranks import run_child

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------------------------
# B. forward coverage of every kernel and branch


def check_forward(qkv, B, L, Hh, hd, ratio_max=1.0, tag=""):
    assert H.attn_route(B, L, Hh, hd).form == FWD_FORMS[B, L, Hh, hd]         # the kernel the case is here for (a host call: no launch)
    got = H.attention(qkv.to(DEV), B, L, Hh, hd).cpu()
    ref, pv = attn_ref64(qkv, B, L, Hh, hd)
    r = err_ratio(got, ref, pv)
    print(f"attention {tag}B={B} L={L} H={Hh} hd={hd}: max err / bound {r:.3f}")
    assert r <= ratio_max, r
    return got


# shape -> what the library's route must name for it (hipops.attn_route(...).form)
GC, GR, PERS, STRM = "generic chunked", "generic resident", "persistent", "streaming"
FWD_FORMS = {
    # generic head_dim, chunked (longer sequences): 256-key chunks, 8 waves per workgroup
    (1, 321, 2, 72): GC, (3, 321, 1, 80): GC,           # first chunked L: last chunk of 65 keys (lone fold); 2nd workgroup: 3 of 8 waves
    (1, 513, 2, 80): GC, (1, 1025, 1, 72): GC,          # last chunk of ONE key: a masked tile step, not the fold (nk = 1)
    (1, 577, 3, 80): GC, (2, 737, 1, 72): GC,           # lone fold at nk = 65 / 225 (577: H/14 at 336 px)
    (2, 730, 2, 72): GC, (1, 768, 2, 80): GC,           # ragged last chunk (218 keys: So400m at 27 x 27 patches); whole chunks only
    # generic head_dim: the other multiples of 8, resident (257) and chunked (577); 96 = no zero padding of the head in LDS
    (1, 257, 2, 8): GR, (1, 257, 2, 32): GR, (1, 257, 2, 56): GR, (1, 257, 2, 88): GR, (1, 257, 2, 96): GR,
    (1, 577, 2, 8): GC, (1, 577, 2, 32): GC, (1, 577, 2, 56): GC, (1, 577, 2, 88): GC, (1, 577, 2, 96): GC,
    # head_dim 64, persistent kernel (short sequences): an odd tile count folds the lone key, an even one keeps it in a tile step
    (2, 65, 3, 64): PERS, (1, 193, 2, 64): PERS, (4, 257, 16, 64): PERS, (1, 97, 2, 64): PERS, (1, 289, 1, 64): PERS,
    # head_dim 64, streaming kernel (longer sequences): a last 64-key chunk of one key is folded in
    (1, 321, 2, 64): STRM, (1, 385, 3, 64): STRM, (1, 577, 2, 64): STRM, (1, 2305, 2, 64): STRM,
}
FWD_SHAPES = list(FWD_FORMS)
PITCH_FORMS = {(2, 257, 4, 64): "persistent", (1, 577, 2, 64): "streaming", (2, 257, 3, 80): "generic resident", (1, 577, 2, 72): "generic chunked"}


@pytest.mark.parametrize("B,L,Hh,hd", FWD_SHAPES)
def test_attention_forward_edges(B, L, Hh, hd):
    qkv = rnd(B * L, 3 * Hh * hd, seed=L * 131 + hd).to(torch.bfloat16)
    check_forward(qkv, B, L, Hh, hd)


@pytest.mark.parametrize("B,L,Hh,hd", [(2, 257, 4, 64), (1, 577, 2, 64), (2, 257, 3, 80), (1, 577, 2, 72)])
def test_attention_padded_row_pitches(B, L, Hh, hd):
    """The tower calls attention with row pitches 3D + 64 (qkv) and D + 64 (out): persistent, streaming, generic resident and
    generic chunked kernel.  The pad columns of qkv hold NaN (a read of them would show), those of out a sentinel that must survive."""
    D = Hh * hd
    assert H.attn_route(B, L, Hh, hd, ld_qkv=3 * D + 64, ld_out=D + 64).form == PITCH_FORMS[B, L, Hh, hd]
    dense = rnd(B * L, 3 * D, seed=L + hd + 7).to(torch.bfloat16)
    qkv = torch.full((B * L, 3 * D + 64), float("nan"), dtype=torch.bfloat16)
    qkv[:, :3 * D] = dense
    qkv = qkv.to(DEV)
    out = torch.full((B * L, D + 64), -1234.5, dtype=torch.bfloat16, device=DEV)
    pad0 = out[:, D:].clone()
    H.attention(qkv[:, :3 * D], B, L, Hh, hd, out=out[:, :D])
    assert qkv.stride(0) == 3 * D + 64
    assert torch.equal(out[:, D:], pad0)
    got = out[:, :D].cpu()
    ref, pv = attn_ref64(dense, B, L, Hh, hd)
    r = err_ratio(got, ref, pv)
    print(f"attention padded B={B} L={L} H={Hh} hd={hd}: max err / bound {r:.3f}")
    assert r <= 1.0, r
    assert torch.equal(got, H.attention(dense.to(DEV), B, L, Hh, hd).cpu())          # the pitch changes nothing else


def test_attention_huge_row_pitch():
    """head_dim 64, a persistent-kernel L, but the qkv image spans more than 2 GiB of rows (L * ld * 2 > 2^31, a C-API caller's pitch): the
    persistent kernel's 32-bit row offsets cannot reach it, so the generic kernel (64-bit offsets) computes it.  Pad columns hold NaN."""
    B, L, Hh, hd, ld = 2, 257, 2, 64, 1 << 22
    D = Hh * hd
    assert L * ld * 2 > 2 ** 31
    assert H.attn_route(B, L, Hh, hd).form == "persistent" and H.attn_route(B, L, Hh, hd, ld_qkv=ld).form == "generic resident"
    dense = rnd(B * L, 3 * D, seed=L + hd + 11).to(torch.bfloat16)
    qkv = torch.full((B * L, ld), float("nan"), dtype=torch.bfloat16, device=DEV)       # 4.3 GB
    qkv[:, :3 * D] = dense.to(DEV)
    got = H.attention(qkv[:, :3 * D], B, L, Hh, hd).cpu()
    del qkv
    torch.cuda.empty_cache()
    ref, pv = attn_ref64(dense, B, L, Hh, hd)
    r = err_ratio(got, ref, pv)
    print(f"attention row pitch 2^22 B={B} L={L} H={Hh} hd={hd}: max err / bound {r:.3f}")
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------------------------------------
# C. the lone key as the row maximum, with the fold (default) and with the tile step (OVHIP_ATTN_LONEKEY=0, read once per process)

LONE_FORMS = ["persistent", "streaming", "streaming", "generic chunked", "generic chunked"]          # of LONE_SPIKED, as the docstring says
_CHILD = r"""
import torch
import hipops as H
cases = torch.load(sys.argv[1])
torch.save({"outs": [H.attention(q.cuda(), B, L, Hh, hd).cpu() for (q, B, L, Hh, hd) in cases],
            "lone_valu": [H.attn_route(B, L, Hh, hd).lone_valu for (q, B, L, Hh, hd) in cases]}, sys.argv[2])
"""


def test_lone_key_as_the_row_max():
    """Spiked inputs (spiked_qkv): for one row per head the lone key is the row maximum by 4 (no rescale, p > 1) or 20 (rescale) log2
    units, at L = 257 (hd 64 persistent), 321 and 2305 (hd 64 streaming), 321 (hd 72) and 577 (hd 80, generic chunked).  The default
    fold and the tile step forced by OVHIP_ATTN_LONEKEY=0 (hd 64 kernels; the generic kernel always folds) are each within the bound,
    and within twice the bound of each other.  Each child records the lone_valu its library's route reports: 1 and 0 in the two runs
    for the hd 64 kernels."""
    cases = []
    for (B, L, Hh, hd) in LONE_SPIKED:
        qkv, _ = spiked_qkv(B, L, Hh, hd, seed=L + hd)
        cases.append((qkv, B, L, Hh, hd))
    res = {}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "cases.pt")
        torch.save(cases, src)
        for lk in ("1", "0"):
            path = os.path.join(d, f"lk{lk}.pt")
            run_child(_CHILD, src, path, env={"OVHIP_ATTN_LONEKEY": lk}, timeout=600, gpu=True)
            res[lk] = torch.load(path)
    ratios = []
    assert res["1"]["lone_valu"] == [1] * len(cases) and res["0"]["lone_valu"] == [int(hd != 64) for (_, _, _, _, hd) in cases]
    assert [H.attn_route(B, L, Hh, hd).form for (_, B, L, Hh, hd) in cases] == LONE_FORMS
    for (qkv, B, L, Hh, hd), fold, tile in zip(cases, res["1"]["outs"], res["0"]["outs"]):
        ref, pv = attn_ref64(qkv, B, L, Hh, hd)
        rf, rt = err_ratio(fold, ref, pv), err_ratio(tile, ref, pv)
        rx = float(((fold.double() - tile.double()).abs() / bound(ref, pv)).max())
        ratios.append(dict(L=L, H=Hh, hd=hd, fold=round(rf, 3), tile=round(rt, 3), fold_vs_tile=round(rx, 3)))
        assert rf <= 1.0 and rt <= 1.0 and rx <= 2.0, ratios[-1]
    print("lone key as the row max, max err / bound:", json.dumps(ratios))


# ------------------------------------------------------------------------------------------------------------------------------
# F. fused row statistics at an odd number of 32-column groups

SENTINEL = 0x7FC0BEEF                     # a NaN with a payload: no kernel writes it


@pytest.mark.parametrize("M,N,K", [(66000, 96, 256), (66000, 1120, 256),     # persistent kernel (>= 256 tiles; 1120: a half last n-tile)
                                   (12336, 1120, 256),                        # non-persistent kernel + the stand-alone pass (245 tiles)
                                   (300, 160, 192)])                          # skinny kernel
def test_gemm_rowparts_odd_group_count(M, N, K):
    """ov_gemm_rowparts with N / 32 odd.  The persistent kernel's epilogue writes two 32-column groups per 16-byte store; the last
    group of a row has no partner, and a store of both would land on the next row's group 0 -- past the buffer for the last row.
    The buffer here has 64 floats of slack behind the [M, N / 32, 2] view, filled with a sentinel that must survive."""
    G = N // 32
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    r = (torch.randn(M, N, generator=g) * 3 + 0.7).to(torch.bfloat16).to(DEV)
    want = H.gemm(a, w, b, epi=3, resid=r)
    for inplace in (False, True):
        buf = torch.full((M * G * 2 + 64,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        parts = buf[:M * G * 2].view(M, G, 2)
        if inplace:                                                   # C aliases R, as the tower calls it
            out = r.clone()
            H.gemm_rowparts(a, w, b, out, out=out, parts=parts)
        else:
            out, _ = H.gemm_rowparts(a, w, b, r, parts=parts)
        assert torch.equal(buf[M * G * 2:].view(torch.int32).cpu(), torch.full((64,), SENTINEL, dtype=torch.int32)), inplace
        assert torch.equal(out, want), inplace
        assert torch.equal(parts, H.rowparts(out)), inplace
        x = out.double().view(M, G, 32)
        s64 = torch.stack([x.sum(-1), (x * x).sum(-1)], dim=-1)
        scale = torch.stack([x.abs().sum(-1), (x * x).sum(-1)], dim=-1)             # 1e-5 relative to the sum of magnitudes
        assert float(((parts.double() - s64).abs() / (scale + 1e-30)).max()) < 1e-5, inplace
