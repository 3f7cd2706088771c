"""The fp8 path against fp64: the persistent fp8 GEMM's tile walk in all three modes, amax_next / amax_acc semantics, the row
quantiser's specialisations, the e4m3 attention epilogue and ov_amax_roll.

test_gpu_ops.py runs the fp8 GEMM with one shape that has more tiles than CUs and tolerances tuned on outputs of magnitude 1.  Here
every route of gemm_fp8.hip (odd and even K-tile counts under continuation, two and three tiles per workgroup, edge -> interior and
interior -> edge successions, e4m3 output and static input scale under continuation, the clamps at M = 1 and N = 8, padded pitches)
is compared with

    ref = (A_q.double() rs) @ (W_q.double() cs).T (+ bias) (+ GELU in fp64) (+ R)

computed by torch ON THE DEVICE from the same quantised bytes, in row chunks so that no fp64 temporary exceeds 1 GB.

The launcher restated (gemm_fp8.hip, launch_fp8 and the head of gemm_fp8_persist): tiles = ceil(M/256) ceil(N/256), n fastest;
grid = min(tiles, CUs); the tile list is cut into eight contiguous XCD runs (the first tiles % 8 runs one tile longer); workgroup
bid works for XCD bid & 7, starts at its run's tile bid >> 3 and strides by the number of workgroups of that XCD.  walk() rebuilds
that list per workgroup and every case asserts from it, before the launch, the property it is there for.

Bounds per element, derived, not tuned (REL = 2^-8 = hipops.REL: one bf16 rounding; fp8 x fp8 products are exact in fp32):

    bias:      |got - ref| <= REL |ref| + (K + 4) 2^-24 S + 1e-6,     S = rs cs (|A_q| |W_q|^T) + |bias| (+ |R|)
               (K accumulations in any order, the two scale multiplications, the bias addition, the fp32 -> bf16 input of the rounding)
    residual:  the same + REL (1 + REL) |pre|: epilogue_fp8 rounds pre = acc rs cs + bias to bf16 (pack_bf16x2 into the transposition
               image) before R is added and the sum is rounded again -- the second-rounding term test_gpu_gemm_routes.py derives.
    GELU:      1.13 x (the bias bound of the pre-activation) + REL |ref| + E,   E = max(1.4e-4, 6.6e-5 |pre|) (erf form, common.h),
               E = 1.1e-6 (tanh form) -- the constants test_gpu_gemm_routes.py states.
    e4m3 out:  |deq - hid| <= 0.0725 |hid| + sc 2^-9 1.01 + 1.2e-3,  sc = 2 amax / 448: the element bound
               test_gemm_fp8_static_scales asserts (e4m3 half step, one subnormal step, the polynomial GELU on |x| < 8).
    amax_next: no rounding precedes the maximum, so |amax_next - max |ref|| <= 1.13 ((K + 4) 2^-24 S + 1e-6) + E at the argmax
               (the mode-0 bound without its REL term, through the GELU that mode 1 always has).

Every output buffer starts as a sentinel (bf16 77; byte 0x7F for e4m3 outputs, an e4m3 NaN code the kernel never emits behind its
clamp) and carries GUARD = 256 rows behind row M - 1: pitch padding and guard rows must still hold the sentinel afterwards, and a
skipped tile fails the bound instead of passing as whatever torch.empty held.  (A whole tile of guard rows: a kernel that lost its
m < M guard then writes into memory this test owns.)  Operand padding holds e4m3 NaN bytes / bf16 NaN.

Measured on an MI355X (256 CUs), max err / bound per case: see DESIGN.md, "fp8 routes"."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import hipops as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BM = BN = 256
BKB = 128
GUARD = 256
SENT, SENT8, NAN8 = 77.0, 0x7F, 0x7F
REL = H.REL
E_TANH = 1.1e-6
CHUNK = 4096                      # rows per fp64 chunk: 4096 x 2048 x 8 B = 64 MB for the widest N here
F8 = torch.float8_e4m3fn


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def walk(M, N, K):
    """The tile list of every workgroup, as gemm_fp8_persist builds it, and what the cases assert about it."""
    ncu = cus()
    tm, tn = -(-M // BM), -(-N // BN)
    tiles = tm * tn
    grid = min(tiles, ncu)
    q8, r8 = divmod(tiles, 8)
    seqs = []
    for bid in range(grid):
        xcd, li = bid & 7, bid >> 3
        xstart = xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8
        xcnt = q8 + (1 if xcd < r8 else 0)
        nper = (grid - xcd + 7) >> 3
        seqs.append([xstart + t for t in range(li, xcnt, nper)])
    assert sorted(t for s in seqs for t in s) == list(range(tiles)), "the restated walk does not cover every tile once"
    edge = lambda t: (t // tn + 1) * BM > M or (t % tn + 1) * BN > N
    succ = {(edge(a), edge(b)) for s in seqs for a, b in zip(s, s[1:])}
    return SimpleNamespace(cus=ncu, tm=tm, tn=tn, tiles=tiles, grid=grid, nt=K // BKB, most=max(len(s) for s in seqs), succ=succ,
                           unequal=r8 != 0, rem=N % BN, last_rows=M - (tm - 1) * BM)


# case -> (tile rows on 256 CUs, rows in the last row tile, N, K, [(what the case is there for, predicate on walk())])
EDGE, INNER = True, False
CASES = {
    "a": (37, 156, 1680, 384, [("nt = 3", lambda r: r.nt == 3), ("more tiles than CUs", lambda r: r.most >= 2),
                               ("XCD runs of unequal length", lambda r: r.unequal), ("ragged M", lambda r: r.last_rows < BM),
                               ("144-column last n-tile", lambda r: r.rem == 144),
                               ("a tile after an interior tile: the counted wait", lambda r: (INNER, INNER) in r.succ)]),
    # (on 256 CUs case a continues three times, interior -> interior each time; the other successions are asserted where they occur)
    "a2": (41, 156, 1680, 384, [("nt = 3", lambda r: r.nt == 3), ("edge -> interior succession", lambda r: (EDGE, INNER) in r.succ)]),
    "b": (41, 1, 2040, 640, [("nt = 5, odd, under continuation", lambda r: r.nt == 5 and r.most >= 2),
                             ("one row in the last row tile", lambda r: r.last_rows == 1),
                             ("248-column last n-tile, N % 16 = 8", lambda r: r.rem == 248),
                             ("edge -> edge and interior -> edge successions", lambda r: {(EDGE, EDGE), (INNER, EDGE)} <= r.succ)]),
    "c": (65, 219, 2048, 512, [("three tiles for some workgroups", lambda r: r.most >= 3), ("even nt", lambda r: r.nt % 2 == 0),
                               ("interior -> edge succession", lambda r: (INNER, EDGE) in r.succ)]),
    "d": (32, 256, 2048, 1152, [("tiles = CUs: no continuation", lambda r: r.tiles == r.cus and r.most == 1), ("nt = 9", lambda r: r.nt == 9)]),
    "e1": (1, 1, 8, 384, [("one row, eight columns: every DMA row clamps", lambda r: r.tiles == 1)]),
    "e2": (1, 255, 264, 384, [("an 8-column second n-tile", lambda r: r.tn == 2 and r.rem == 8)]),
    "g": (37, 156, 1680, 640, [("continuation", lambda r: r.most >= 2), ("interior -> any succession: the counted wait of the byte output",
                                                                           lambda r: any(not a for a, _ in r.succ)),
                               ("144-column last n-tile", lambda r: r.rem == 144)]),
    "g16": (37, 156, 1552, 384, [("continuation", lambda r: r.most >= 2), ("16-column last n-tile", lambda r: r.rem == 16)]),
    "h": (37, 156, 1664, 1664, [("continuation", lambda r: r.most >= 2), ("nt = 13", lambda r: r.nt == 13)]),
}


@functools.lru_cache(maxsize=None)
def selected(case):
    """(M, N, K) of `case` on this device: the table's shape on 256 CUs, otherwise the row-tile count scaled by CUs / 256 and raised
    until every property the case is named for holds (asserted either way)."""
    tm0, last, N, K, props = CASES[case]
    ncu = cus()
    first = tm0 if ncu == 256 or tm0 == 1 else max(1, -(-tm0 * ncu // 256))
    for tm in range(first, first + (1 if ncu == 256 else 17)):
        M = (tm - 1) * BM + last
        r = walk(M, N, K)
        missing = [what for what, holds in props if not holds(r)]
        if not missing:
            return M, N, K
    raise AssertionError(f"case {case} {(M, N, K)} on {ncu} CUs no longer has: {missing}")


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def operands(M, N, K, spread=True):
    """A_q, W_q (e4m3 bytes), their row / column scales and a nonzero bias, on the device.  spread: rows of A of very different
    magnitude (per-row scales that matter); without it |pre-activation| stays below 8, what the e4m3 output bound assumes."""
    seed = 1000003 * K + 1009 * N + M
    a = rnd(M, K, seed=seed)
    if spread:
        a = a * (rnd(M, 1, seed=seed + 1).abs() * 3 + 0.2)
    w = rnd(N, K, seed=seed + 2) / K ** 0.5
    aq, rs = H.quantize_rows_e4m3(a.to(DEV))
    wq, cs = H.quantize_rows_e4m3(w.to(DEV))
    return aq, wq, rs, cs, rnd(N, seed=seed + 3).to(DEV)


@functools.lru_cache(maxsize=None)
def residual(M, N):
    return rnd(M, N, seed=7 * M + N).to(torch.bfloat16).to(DEV)


def gelu64(x, tanh):
    return torch.nn.functional.gelu(x, approximate="tanh" if tanh else "none")


def deq(q):
    return q.view(F8).float()


def reference(aq, wq, rs, cs, bias, outs, r=None):
    """outs: name -> (tensor [M, >= N], kind), kind in pre | erf | tanh | res | ("q8", sc).  Returns (name -> (max err / bound, row,
    column), amax) against fp64 on the device in row chunks; amax = (max |erf-GELU(pre)| over the M x N elements, the allowed
    difference of amax_next from it: see the module docstring)."""
    M, K = aq.shape
    N = wq.shape[0]
    wf = deq(wq) * cs[:, None]
    wd, wabs = deq(wq).double() * cs.double()[:, None], wf.abs()
    bd = bias.double() if bias is not None else torch.zeros(N, dtype=torch.float64, device=DEV)
    res, amax = {}, (-1.0, 0.0)
    for i in range(0, M, CHUNK):
        sl = slice(i, min(M, i + CHUNK))
        af = deq(aq[sl])
        pre = (af.double() * rs[sl].double()[:, None]) @ wd.T + bd
        s = ((af.abs() * rs[sl][:, None]) @ wabs.T).double() + bd.abs()
        acc = (K + 4) * 2.0 ** -24 * s + 1e-6
        b_pre = REL * pre.abs() + acc
        hid = gelu64(pre, False)
        k = int(hid.abs().argmax())
        if float(hid.abs().view(-1)[k]) > amax[0]:
            e = max(1.4e-4, 6.6e-5 * float(pre.abs().view(-1)[k]))
            amax = (float(hid.abs().view(-1)[k]), 1.13 * float(acc.view(-1)[k]) + e)
        for name, (got, kind) in outs.items():
            if kind == "pre":
                g, ref, bound = got[sl, :N].double(), pre, b_pre
            elif kind == "res":
                rr = r[sl].double()
                g, ref = got[sl, :N].double(), pre + rr
                bound = REL * ref.abs() + (K + 4) * 2.0 ** -24 * (s + rr.abs()) + 1e-6 + REL * (1 + REL) * pre.abs()
            elif kind in ("erf", "tanh"):
                g, ref = got[sl, :N].double(), gelu64(pre, kind == "tanh")
                e = E_TANH if kind == "tanh" else torch.clamp(6.6e-5 * pre.abs(), min=1.4e-4)
                bound = 1.13 * b_pre + REL * ref.abs() + e
            else:
                sc = kind[1]
                g, ref = deq(got[sl, :N]).double() * sc, hid
                bound = 0.0725 * hid.abs() + sc * 2.0 ** -9 * 1.01 + 1.2e-3
            q = (g - ref).abs() / bound
            q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)       # a NaN (an e4m3 sentinel left behind) fails
            j = int(q.argmax())
            item = (float(q.view(-1)[j]), i + j // N, j % N)
            if name not in res or item[0] > res[name][0]:
                res[name] = item
    return res, amax


def report(tag, res):
    for name, (q, row, col) in res.items():
        print(f"{tag} {name}: max err / bound {q:.3f}")
    bad = {n: (q, f"row {row} column {col} = tile ({row // BM}, {col // BN})") for n, (q, row, col) in res.items() if not q <= 1.0}
    assert not bad, (tag, bad)


def padded(t, pad, junk):
    """t as the leading columns of a buffer `pad` columns wider (its pitch), the padding holding `junk`."""
    if not pad:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + pad), junk, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def out_buffer(M, N, pad, dtype=torch.bfloat16):
    """(whole buffer, the caller's [M, N] view of it): N + pad columns, GUARD rows behind row M - 1, all of it the sentinel."""
    buf = torch.full((M + GUARD, N + pad), SENT8 if dtype == torch.uint8 else SENT, dtype=dtype, device=DEV)
    return buf, buf[:M, :N]


def sentinel_kept(buf, M, N):
    sent = SENT8 if buf.dtype == torch.uint8 else SENT
    return bool((buf[:M, N:] == sent).all()) and bool((buf[M:] == sent).all())


@functools.lru_cache(maxsize=None)
def hidden_max(case):
    """max |erf-GELU(pre)| of the mode-1 case's operands (fp64) and the allowed difference of amax_next from it."""
    aq, wq, rs, cs, bias = operands(*selected(case), spread=False)
    return reference(aq, wq, rs, cs, bias, {})[1]


@functools.lru_cache(maxsize=None)
def static_operands(M, N, K):
    """Mode 2: A as the e4m3 bytes a mode-1 GEMM leaves (a GELU output under ONE static scale 2 amax / 448), W and bias as usual."""
    hid = gelu64(rnd(M, K, seed=11 * M + K), False)
    amax = hid.abs().max().reshape(1)
    aq = (hid / (2.0 * amax / 448.0)).to(F8).view(torch.uint8).to(DEV)
    _, wq, _, cs, bias = operands(M, N, K)
    return aq, wq, amax.to(DEV), cs, bias


# run -> case, epilogue (0 bias, 1 erf-GELU, 2 tanh-GELU, 3 residual) and what else it varies.  pitched: lda = K + 16, ldw = K + 32,
# ldc = N + 8, ldr = N + 24 (case f).  inplace: C aliases R, as tower.hip calls every residual fp8 GEMM (x, D ... x, D).
RUNS = {
    "a-bias": dict(case="a", epi=0),
    "a-nobias": dict(case="a", epi=0, bias=False),
    "a2-bias": dict(case="a2", epi=0),
    "b-erf": dict(case="b", epi=1),
    "b-tanh": dict(case="b", epi=2),
    "c-residual-own-pitch": dict(case="c", epi=3, ldr=40),
    "c-residual-in-place": dict(case="c", epi=3, inplace=True),
    "d-bias": dict(case="d", epi=0),
    "e1-bias": dict(case="e1", epi=0),
    "e2-bias": dict(case="e2", epi=0),
    "f-a-bias-pitched": dict(case="a", epi=0, pitched=True),
    "f-a-residual-pitched": dict(case="a", epi=3, pitched=True),
    "f-b-erf-pitched": dict(case="b", epi=1, pitched=True),
    "g-e4m3-out": dict(case="g", epi=1, mode=1, ldc=16),
    "h-static-in-residual": dict(case="h", epi=3, mode=2, inplace=True),
}
KIND = {0: "pre", 1: "erf", 2: "tanh", 3: "res"}


def launch(run):
    """Launches `run`; returns (whole output buffer, what reference() needs to judge it)."""
    spec = RUNS[run]
    M, N, K = selected(spec["case"])
    mode, epi, pitched = spec.get("mode", 0), spec["epi"], spec.get("pitched", False)
    if mode == 2:
        aq, wq, in_amax, cs, bias = static_operands(M, N, K)
        rs = (2.0 * (1.0 / 448.0) * in_amax).expand(M).contiguous()
    else:
        aq, wq, rs, cs, bias = operands(M, N, K, spread=mode == 0)
    if not spec.get("bias", True):
        bias = None
    a_in, w_in = padded(aq, 16 if pitched else 0, NAN8), padded(wq, 32 if pitched else 0, NAN8)
    buf, out = out_buffer(M, N, spec.get("ldc", 8 if pitched else 0), torch.uint8 if mode == 1 else torch.bfloat16)
    r = r_in = None
    if epi == 3:
        r = residual(M, N)
        if spec.get("inplace"):
            out.copy_(r)
            r_in = out
        else:
            r_in = padded(r, spec.get("ldr", 24 if pitched else 0), float("nan"))
    kind = KIND[epi]
    if mode == 0:
        H.gemm_fp8(a_in, w_in, rs, cs, bias, epi, r_in, out=out)
    elif mode == 1:
        amax = torch.tensor([hidden_max(spec["case"])[0]], dtype=torch.float32, device=DEV)
        H.gemm_fp8_static(a_in, w_in, cs, bias, epi, rowscale=rs, out_amax=amax, out=out)
        kind = ("q8", 2.0 * float(amax) / 448.0)
    else:
        H.gemm_fp8_static(a_in, w_in, cs, bias, epi, in_amax=in_amax, resid=r_in, out=out)
    return buf, SimpleNamespace(M=M, N=N, K=K, args=(aq, wq, rs, cs, bias), kind=kind, r=r)


@pytest.mark.parametrize("run", list(RUNS))
def test_gemm_fp8_route_within_the_fp64_bound(run):
    buf, j = launch(run)
    res, _ = reference(*j.args, {run: (buf, j.kind)}, j.r)
    report(f"{run} {(j.M, j.N, j.K)}", res)
    assert sentinel_kept(buf, j.M, j.N), f"{run}: pitch padding or the guard rows behind row M - 1 were written"


# ---- amax_next of the e4m3-output GEMM: the maximum over the real M x N elements only ----


@functools.lru_cache(maxsize=None)
def adversarial(case):
    """Operands whose partial last n-tile would dominate amax_next if its columns past N were counted.  Those columns are W row N - 1
    (clamped DMA rows) under colscale / bias [N - 4 + e], e = column % 4 (parameter block clamped to N - 4).  W_q row N - 1 = +-448
    aligned in sign with row m* of A under a small colscale[N - 1]; rows N - 4 .. N - 2 are zero codes (their real columns are
    GELU(0) = 0) under a colscale 2^10 larger with zero bias: a counted fake is about 2^10 x element (m*, N - 1).  Everything else
    is scaled down so that the real maximum stays two orders of magnitude below."""
    M, N, K = selected(case)
    aq, wq, rs, cs, bias = operands(M, N, K, spread=False)
    wq, cs, bias = wq.clone(), cs * 2.0 ** -7, bias * 2.0 ** -7
    ms = M // 2
    arow = deq(aq[ms])
    wq[N - 1] = torch.where(arow < 0, 0xFE, 0x7E).to(torch.uint8)               # -448 / +448
    wq[N - 4:N - 1] = 0
    dot = float(rs[ms]) * 448.0 * float(arow.abs().sum())
    small = 2.0 ** round(math.log2(0.02 / dot))                                  # element (m*, N - 1) is about 0.02 before the GELU
    cs[N - 1] = small
    cs[N - 4:N - 1] = small * 2.0 ** 10
    bias[N - 4:N - 1] = 0
    # the clamp restated on the CPU: what the columns past N of the last n-tile hold
    acc = (deq(aq.cpu()).double() @ deq(wq[N - 1].cpu()).double()) * rs.double().cpu()
    fake = max(float(gelu64(acc * float(cs[N - 4 + e]) + float(bias[N - 4 + e]), False).abs().max()) for e in range(3))
    true, allowed = reference(aq, wq, rs, cs, bias, {})[1]
    assert N % BN and fake >= 100 * true, (fake, true)
    return (aq, wq, rs, cs, bias), true, allowed, fake


@pytest.mark.parametrize("case", ["g", "g16"])
def test_gemm_fp8_amax_next_is_the_maximum_over_real_elements(case):
    """N % 256 = 144 and 16 under continuation.  amax_next starts at 0 (must become the real maximum), above the real maximum (must
    stay bit for bit) and below it (must be raised to it)."""
    M, N, K = selected(case)
    args, true, allowed, fake = adversarial(case)
    aq, wq, rs, cs, bias = args
    amax = torch.tensor([true], dtype=torch.float32, device=DEV)
    for preset in (0.0, 4.0 * true, 0.25 * true):
        nxt = torch.tensor([preset], dtype=torch.float32, device=DEV)
        before = nxt.clone()
        buf, out = out_buffer(M, N, 16, torch.uint8)
        H.gemm_fp8_static(aq, wq, cs, bias, 1, rowscale=rs, out_amax=amax, amax_next=nxt, out=out)
        got = float(nxt)
        print(f"case {case} {(M, N, K)} preset {preset:.6g}: amax_next {got:.8g}, fp64 maximum {true:.8g} (+- {allowed:.3g}), "
              f"maximum of the columns past N {fake:.6g}")
        if preset > true:
            assert torch.equal(nxt.view(torch.int32), before.view(torch.int32)), (got, preset)
        else:
            assert abs(got - true) <= allowed, (got, true, allowed, fake)
        assert sentinel_kept(buf, M, N)
        assert not bool((out == SENT8).any()) and not bool((out == 0xFF).any())


# ---- ov_attention_fp8out ----


def attn_kernel(B, L, Hh, cus=0):
    """(the kernel ov_attention_fp8out takes, as the library reports it; the query rows it pads the sequence with: to whole waves of
    32 queries, in the streaming kernel to whole workgroups)."""
    r = H.attn_route(B, L, Hh, 64, out8=True, cus=cus)
    assert r.out8 and r.waves == (8 if r.kernel == "streaming" else -(-L // 32)), vars(r)
    name = r.kernel if r.kernel == "streaming" else f"{r.kernel}, {'<= 8' if r.deep else '9+'} waves"
    return name, -(-L // (32 * r.waves)) * 32 * r.waves - L


def peaked_qkv(B, L, Hh):
    """Every real query puts (almost) all its weight on key 0, whose V row is small; every other V row is the constant 8: any query
    row that is NOT a copy of a real one (zeros, garbage) would produce an output near 8.  K[0] = 0, so the top logit is exactly 0
    and every other one is below -40: the softmax shift m is then exact.  With a top logit s != 0 the shift m = fl(s c) is rounded,
    the top key's fp32 probability is 2^(s c - m) = 2^(+-2^-24 |m|) while the bf16 P that multiplies V is exactly 1, and the output
    is off by ln 2 2^-24 |m| relative (measured with K[0] = 2: 1.31e-6 = 2^-19.5 at |m| = 58, all five shapes) -- softmax accuracy,
    which test_gpu_attention_edges.py bounds, not what the 2^-20 of this test is about."""
    D = Hh * 64
    g = torch.Generator().manual_seed(L)
    x = torch.empty(B, L, 3, Hh, 64)
    x[:, :, 0] = 1.5 + torch.rand(B, L, Hh, 64, generator=g)
    x[:, :, 1] = -4.0
    x[:, 0, 1] = 0.0
    x[:, :, 2] = 8.0
    x[:, 0, 2] = (torch.rand(B, Hh, 64, generator=g) - 0.5) / 8
    qkv = x.view(B * L, 3 * D).to(torch.bfloat16)
    q, k, v = H._split(qkv, B, L, Hh, 64)
    logit = q @ k.transpose(-1, -2) * 0.125
    assert float((logit[..., :1] - logit[..., 1:]).min()) >= 40 and float(v[:, :, 0].abs().max()) <= 1 / 16
    return qkv.to(DEV)


@pytest.mark.parametrize("B,L,Hh,kernel,padded_rows", [(2, 257, 2, "persistent, 9+ waves", 31), (2, 33, 2, "persistent, <= 8 waves", 31),
                                                       (2, 65, 2, "persistent, <= 8 waves", 31), (2, 577, 2, "streaming", 191),
                                                       (1, 2305, 2, "streaming", 255)])
def test_attention_fp8out_amax_next_and_pitch(B, L, Hh, kernel, padded_rows):
    """amax_next = max |out| over the real rows (within 2^-20 relative + the softmax leak L e^-40 8), as a running maximum; the e4m3
    output within the element bound test_attention_fp8_output asserts; contiguous and with ld_out = H 64 + 16."""
    assert attn_kernel(B, L, Hh) == (kernel, padded_rows)
    D = Hh * 64
    qkv = peaked_qkv(B, L, Hh)
    ref = H.attn_ref64(qkv, B, L, Hh, 64)[0]
    true = float(ref.abs().max())
    allowed = 2.0 ** -20 * true + L * math.exp(-40) * 8
    amax = torch.tensor([true], dtype=torch.float32, device=DEV)
    sc = 2.0 * float(amax) / 448.0
    for pad, preset in ((0, 0.0), (16, 0.0), (16, 4.0 * true), (16, 0.25 * true)):
        nxt = torch.tensor([preset], dtype=torch.float32, device=DEV)
        before = nxt.clone()
        buf, out = out_buffer(B * L, D, pad, torch.uint8)
        H.attention_fp8out(qkv, B, L, Hh, amax, nxt, out=out)
        got = float(nxt)
        err = (deq(out).double() * sc - ref).abs()
        bound = ref.abs() * 0.075 + sc * 2.0 ** -9 * 1.01 + 1e-6
        q = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
        print(f"L {L} ({kernel}) pitch + {pad} preset {preset:.6g}: amax_next {got:.8g}, fp64 maximum {true:.8g} (+- {allowed:.3g}); "
              f"output max err / bound {q:.3f}")
        if preset > true:
            assert torch.equal(nxt.view(torch.int32), before.view(torch.int32)), (got, preset)
        else:
            assert abs(got - true) <= allowed, (got, true, allowed)
        assert q <= 1.0
        assert sentinel_kept(buf, B * L, D)


# ---- ov_quant_rows_fp8 / ov_layernorm_quant_fp8 ----


def quant_nch(D):
    n = (D // 8 + 63) // 64
    return next(s for s in (1, 2, 3, 4, 8, 16) if n <= s)


@pytest.mark.parametrize("rows,D,nch", [(37, 1152, 3), (37, 1280, 3), (37, 2048, 4), (21, 4304, 16), (21, 8192, 16), (37, 8, 1),
                                        (65541, 64, 1)])
def test_quant_rows_specialisations_pitches_and_amax_acc(rows, D, nch):
    """Every NCH specialisation the other tests do not reach, ldx = ldq = D + 8 with sentinels, an all-zero row, amax_acc as an exact
    running maximum, and rows = 65541 (the grid is capped at 16384 workgroups of 4 rows: a second pass of the grid-stride loop)."""
    assert quant_nch(D) == nch and (rows > 65536) == (rows == 65541)
    x = (rnd(rows, D, seed=50 + D) * (rnd(rows, 1, seed=51 + D).abs() * 4 + 0.1)).to(torch.bfloat16)
    x[3] = 0
    xin = padded(x.to(DEV), 8, float("nan"))
    rowmax = x.float().abs().amax(1)
    true = rowmax.max()
    for preset in (0.0, 2.0 * float(true), 0.5 * float(true)):
        acc = torch.tensor([preset], dtype=torch.float32, device=DEV)
        buf, out = out_buffer(rows, D, 8, torch.uint8)
        q, sc = H.quant_rows_fp8(xin, amax=acc, out=out)
        want = max(torch.tensor(preset, dtype=torch.float32), true)
        assert torch.equal(acc.cpu().view(torch.int32), want.reshape(1).view(torch.int32)), (float(acc), float(want))   # exact
        assert sentinel_kept(buf, rows, D)
    sc, qc = sc.cpu(), q.cpu()
    assert not torch.isnan(sc).any() and not torch.isnan(deq(qc)).any()
    assert float(sc[3]) == float(torch.tensor(1e-12, dtype=torch.float32) * torch.tensor(1.0 / 448.0, dtype=torch.float32))
    assert bool((qc[3] == 0).all())
    torch.testing.assert_close(sc, rowmax.clamp_min(1e-12) / 448.0, rtol=1e-6, atol=0)
    live = rowmax > 0
    scaled = (x.float() * (448.0 / rowmax.clamp_min(1e-12))[:, None])[live]
    ref = scaled.to(F8).view(torch.uint8)
    diff = qc[live] != ref
    if diff.any():                       # v_cvt_pk_fp8_f32 against torch's CPU cast: adjacent codes only, and rarely
        assert (qc[live].int() - ref.int()).abs()[diff].max() <= 1
        assert diff.float().mean() < 0.01
    assert ((deq(qc[live]) - scaled).abs() <= scaled.abs() * 0.0625 + 2.0 ** -9).all()      # half an e4m3 step
    # the LayerNorm form on the same rows (the zero row normalises to beta)
    gamma, beta = rnd(D, seed=52) * 0.1 + 1, rnd(D, seed=53) * 0.1
    buf, out = out_buffer(rows, D, 8, torch.uint8)
    ql, scl = H.quant_rows_fp8(xin, gamma.to(DEV), beta.to(DEV), 1e-6, out=out)
    assert sentinel_kept(buf, rows, D)
    y = torch.nn.functional.layer_norm(x.float(), (D,), gamma, beta, 1e-6)
    dq = deq(ql.cpu()) * scl.cpu()[:, None]
    assert not torch.isnan(dq).any()
    assert (dq - y).abs().max() <= (y.abs().amax(1, keepdim=True) / 448.0 * 16.0 + 1e-6).max()
    torch.testing.assert_close(scl.cpu(), y.abs().amax(1) / 448.0, rtol=2e-5, atol=0)


# ---- ov_amax_roll ----


@pytest.mark.parametrize("n", [1, 256, 257])
def test_amax_roll_is_the_elementwise_maximum(n):
    cur0 = rnd(n + 7, seed=n).abs()
    nxt = rnd(n + 7, seed=n + 1).abs()
    cur = cur0.to(DEV)
    H.amax_roll(cur, nxt.to(DEV)[:n])
    want = cur0.clone()
    want[:n] = torch.maximum(cur0[:n], nxt[:n])
    assert torch.equal(cur.cpu().view(torch.int32), want.view(torch.int32))
