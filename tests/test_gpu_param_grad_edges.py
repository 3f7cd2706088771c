"""The linear, LayerNorm and GELU backward of backward.hip at their edges, against fp64 closed forms with per-element bounds.

The older tests of these operators (test_gpu_ops.py) use tuned tolerances against the fp32 oracle on dense Gaussian inputs, at row
counts that never take the route every tower takes (M % 64 == 0: dW straight from the row-major operands, db from the same kernel),
never reach the two-stage rows_sum from the linear backward, the capped LayerNorm grid, a lone-lane last chunk, `dres`, `h_out` or
the in-place GELU call of the block's chain.  Here every element of every output is held to

    |dX err|     <= u |dX| + N e (|dY| |W|) + 1e-6
    |dW err|     <= u (|dW| + T) + M e (|dY|^T |X|) + 1e-6          T = sum over 64-row tiles of |the tile's share of dW|
    |db err|     <= (M + 2) e sum|dY| + 1e-7
    |LN dx err|, |dgamma err|, |dbeta err|                           hipops.ln_grads_ref64
    |da err|     <= u |da| + |dh| delta,  |h err| <= u |h| + |a| delta   (+ 2^-134: bf16 underflow)

with u = 2^-8, e = 2^-24 (hipops.linear_bounds, ln_grads_ref64, gelu_bounds, where each term is derived: nothing is tuned to what
the kernels give, and nothing depends on the split-K plan), on inputs whose edge rows are spiked (hipops.spiked_linear_case,
spiked_ln_case).  ov_linear_backward_plan is asked only to assert that a case reaches the path its comment names.
test_param_grad_bound.py (CPU) pins what the bounds can see."""
import functools
import hashlib
import os
import tempfile

import pytest
import torch

import hipops as H
from hipops import GELU_DH, LINEAR_NK, LINEAR_TN_M, LINEAR_TR_M, LN_SHAPES
from ranks import run_child

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD_SENTINEL = -1234.5
WS_SENTINEL = 0xA5
RS_DIRECT = 128                  # rows_sum sums up to this many partial rows in one launch, more in two stages


def dev(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


def padded(dense, pad, fill=float("nan")):
    """`dense` as the leading columns of a tensor `pad` columns wider whose other columns hold `fill`: (the slice, the wide tensor)."""
    wide = torch.full((dense.shape[0], dense.shape[1] + pad), fill, dtype=dense.dtype)
    wide[:, :dense.shape[1]] = dense
    wide = wide.to(DEV)
    return wide[:, :dense.shape[1]], wide


def sentinel_out(rows, cols, pad):
    """A [rows, cols] bf16 output inside a sentinel-filled tensor `pad` columns wider: (the slice, the wide tensor)."""
    wide = torch.full((rows, cols + pad), PAD_SENTINEL, dtype=torch.bfloat16, device=DEV)
    return wide[:, :cols], wide


def pads_intact(wide, cols):
    return torch.equal(wide[:, cols:].view(torch.int16), torch.full_like(wide[:, cols:], PAD_SENTINEL).view(torch.int16))


def exact_ws(nb):
    """A workspace of exactly `nb` bytes with 256 sentinel bytes behind it: (the view handed over, the whole buffer)."""
    buf = torch.full((nb + 256,), WS_SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[:nb], buf


def ws_intact(buf, nb):
    return bool((buf[nb:] == WS_SENTINEL).all())


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------------------------------
# A. linear backward


@functools.lru_cache(maxsize=None)
def linear_case(M, N, K, boost=8.0):
    """(inputs, fp64 reference, bounds), computed once per shape and shared by the tests below (never modified)."""
    dy, x, w = H.spiked_linear_case(M, N, K, seed=M * 7 + N + K, boost=boost)
    return (dy, x, w), H.linear_grads_ref64(dy, x, w), H.linear_bounds(dy, x, w)


def check_linear(tag, got, ref, bounds):
    """got: (dX | None, dW | None, db | None).  Prints max err / bound per output and asserts <= 1."""
    names = ("dX", "dW", "db")
    r = {n: float(((g.double().cpu() - want).abs() / bd).max()) for n, g, want, bd in zip(names, got, ref, bounds) if g is not None}
    print(f"linear backward {tag}: max err / bound " + " ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r           # (a NaN fails this too)
    return r


def same(a, b):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


# what each row count is here for, asserted through ov_linear_backward_plan (nz ranges of `chunk` rows; tn: the row-major route)
PLAN_CLAIMS = {
    64: lambda M, nz, chunk, tn: tn and nz == 1,                                   # db straight from the TN kernel
    512: lambda M, nz, chunk, tn: tn and nz == 1,
    1088: lambda M, nz, chunk, tn: tn and nz > 1 and nz * chunk > M,               # a ragged last range
    2048: lambda M, nz, chunk, tn: tn and nz > 1 and nz * chunk == M,              # even ranges
    16384: lambda M, nz, chunk, tn: tn and nz == 32,                               # the most ranges the plan makes
    70: lambda M, nz, chunk, tn: not tn and nz == 1,
    1100: lambda M, nz, chunk, tn: not tn and nz > 1 and nz * chunk > M,           # zeros past M inside the last range
    8200: lambda M, nz, chunk, tn: not tn and nz * chunk // 64 > RS_DIRECT,        # db: two-stage rows_sum over the tile partials
}


@pytest.mark.parametrize("N,K", LINEAR_NK)
@pytest.mark.parametrize("M", LINEAR_TN_M + LINEAR_TR_M)
def test_linear_backward_edges(M, N, K):
    nz, chunk, tn = H.linear_backward_plan(M, N, K)
    assert PLAN_CLAIMS[M](M, nz, chunk, tn), (M, N, K, nz, chunk, tn)
    (dy, x, w), ref, bounds = linear_case(M, N, K)
    dy, x, w = dev(dy, x, w)
    got = H.linear_backward(dy, x, w)
    check_linear(f"M={M} N={N} K={K} (nz={nz} chunk={chunk} {'tn' if tn else 'transposes'})", got, ref, bounds)
    assert same(got, H.linear_backward(dy, x, w))                                 # deterministic


@pytest.mark.parametrize("M", [33027, 7])
def test_linear_backward_db_alone(M):
    """colsum_partial over 256-row chunks, then rows_sum: 130 chunk partials (two stages, a last chunk of 3 rows) and a single short one.
    The db bound grows like M^2 (M terms, each against the whole column's sum|dY|): at M = 33027 it is 52 per column, so the edge rows
    are spiked 512-fold there (hipops.DB_BOOST_LARGE_M) for a dropped one to stand outside it."""
    N, K = 64, 64
    assert ((M + 255) // 256 > RS_DIRECT) == (M == 33027)
    (dy, x, w), ref, bounds = linear_case(M, N, K, boost=H.DB_BOOST_LARGE_M if M == 33027 else 8.0)
    dy, x, w = dev(dy, x, w)
    got = H.linear_backward(dy, x, w, want=("db",))
    assert got[0] is None and got[1] is None
    check_linear(f"db alone M={M} N={N}", got, ref, bounds)
    assert same(got, H.linear_backward(dy, x, w, want=("db",)))


@pytest.mark.parametrize("N,K", LINEAR_NK)
def test_linear_backward_subsets(N, K):
    """dX alone and dW + db alone at M = 1088: inside the bound, and the same launches as the full call, so bitwise its results."""
    M = 1088
    (dy, x, w), ref, bounds = linear_case(M, N, K)
    dy, x, w = dev(dy, x, w)
    full = H.linear_backward(dy, x, w)
    only_dx = H.linear_backward(dy, x, w, want=("dx",))
    only_p = H.linear_backward(dy, x, w, want=("dw", "db"))
    check_linear(f"dX alone M={M} N={N} K={K}", only_dx, ref, bounds)
    check_linear(f"dW + db alone M={M} N={N} K={K}", only_p, ref, bounds)
    assert torch.equal(only_dx[0], full[0]) and torch.equal(only_p[1], full[1]) and torch.equal(only_p[2], full[2])


_CHILD = r"""
import hashlib, torch
import hipops as H
sha = lambda t: hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
res = []
for (dy, x, w) in torch.load(sys.argv[1]):
    M, N = dy.shape
    _, dw, db = H.linear_backward(dy.cuda(), x.cuda(), w.cuda(), want=("dw", "db"))
    torch.cuda.synchronize()
    res.append(dict(plan=H.linear_backward_plan(M, N, x.shape[1]), dw=sha(dw), db_sha=sha(db), db=db.cpu()))
torch.save(res, sys.argv[2])
"""


def test_linear_backward_routes_agree_bitwise_on_dw():
    """OVHIP_DW_TRANSPOSE=1 (read once per process: a fresh child) forces the explicit transposes at M = 1088 and 512, where the
    default is the row-major route.  linear_backward's comment: "both routes accumulate the same products in the same order: bitwise
    the same dW".  db is summed per 64-row tile there and per range here: inside its bound, not necessarily the same bits."""
    N, K = 192, 320
    cases = [linear_case(M, N, K) for M in (1088, 512)]
    with tempfile.TemporaryDirectory() as d:
        src, path = os.path.join(d, "cases.pt"), os.path.join(d, "out.pt")
        torch.save([c[0] for c in cases], src)
        run_child(_CHILD, src, path, env={"OVHIP_DW_TRANSPOSE": "1"}, timeout=300, gpu=True)
        res = torch.load(path)
    for ((dy, x, w), ref, bounds), child in zip(cases, res):
        M = dy.shape[0]
        nz, chunk, tn = H.linear_backward_plan(M, N, K)
        assert tn and not child["plan"][2] and child["plan"][:2] == (nz, chunk), (M, (nz, chunk, tn), child["plan"])
        _, dw, db = H.linear_backward(*dev(dy, x, w), want=("dw", "db"))
        check_linear(f"row-major route M={M}", (None, dw, db), ref, bounds)
        check_linear(f"forced transposes M={M}", (None, None, child["db"]), ref, bounds)
        print(f"linear backward routes M={M}: dW bitwise equal {child['dw'] == digest(dw)}, db bitwise equal {child['db_sha'] == digest(db)}")
        assert child["dw"] == digest(dw), M


@pytest.mark.parametrize("M", [1088, 1100])
def test_linear_backward_pitches_and_neighbours(M):
    """Both routes with row pitches N + 8 (dY), K + 16 (X), K + 24 (W), K + 8 (dX) and K + 16 (dW): the inputs' pad columns hold NaN,
    the outputs' a sentinel that must survive; the workspace is exactly ov_linear_backward_workspace_bytes with a sentinel tail
    behind it.  Bitwise the dense run."""
    N, K = 192, 320
    (dy, x, w), ref, bounds = linear_case(M, N, K)
    want = H.linear_backward(*dev(dy, x, w))
    dy_p, _ = padded(dy, 8)
    x_p, _ = padded(x, 16)
    w_p, _ = padded(w, 24)
    assert (dy_p.stride(0), x_p.stride(0), w_p.stride(0)) == (N + 8, K + 16, K + 24)
    dx_p, dx_w = sentinel_out(M, K, 8)
    dw_p, dw_w = sentinel_out(N, K, 16)
    nb = H._lib.load().ov_linear_backward_workspace_bytes(M, N, K)
    ws, buf = exact_ws(nb)
    got = H.linear_backward(dy_p, x_p, w_p, dx=dx_p, dw=dw_p, ws=ws)
    torch.cuda.synchronize()
    assert (got[0].stride(0), got[1].stride(0)) == (K + 8, K + 16)
    assert ws_intact(buf, nb), "the workspace was overrun"
    assert pads_intact(dx_w, K) and pads_intact(dw_w, K)
    check_linear(f"padded M={M} N={N} K={K}", got, ref, bounds)
    assert same(got, want)


# ------------------------------------------------------------------------------------------------------------------------------
# B. LayerNorm backward


def check_ln(tag, got, ref):
    r = H.ln_err_ratio(*[t.cpu() for t in got], ref)
    print(f"layernorm backward {tag}: max err / bound dx {r[0]:.3f} dgamma {r[1]:.3f} dbeta {r[2]:.3f}")
    assert max(r) <= 1.0 and all(v == v for v in r), r
    return r


def run_ln(tag, rows, D, dres_on=True, mean=0.2):
    x, gamma, dy, dres = H.spiked_ln_case(rows, D, seed=rows * 3 + D, mean=mean)
    dres = dres if dres_on else None
    ref = H.ln_grads_ref64(x, gamma, dy, dres, 1e-6)
    x, gamma, dy, dres = dev(x, gamma, dy, dres)
    got = H.layernorm_backward(x, gamma, dy, dres=dres)
    check_ln(f"{tag} rows={rows} D={D}", got, ref)
    assert same(got, H.layernorm_backward(x, gamma, dy, dres=dres))               # deterministic


@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_layernorm_backward_edges(rows, D):
    """With dres.  (1, 8): one lane; D = 200: blocks of rows_sum that straddle dgamma | dbeta and a ragged last one (2 D = 400);
    129 rows: more than 128 wave partials, so rows_sum in two stages; D = 520, 1032, 1544, 2056: a last chunk group of one lane
    (2056 in the NCH = 8 form); 4096: the widest row; 4099 and 8195 rows: the capped grid, waves with two and three rows."""
    run_ln("with dres", rows, D)


@pytest.mark.parametrize("rows,D", [(129, 200), (4099, 64)])
def test_layernorm_backward_without_dres(rows, D):
    run_ln("no dres", rows, D, dres_on=False)


def test_layernorm_backward_large_mean():
    """mean 8, spread 1.5: cancellation in x - mean and in the variance."""
    run_ln("mean 8", 9, 1152, mean=8.0)


@pytest.mark.parametrize("rows,D", [(129, 200), (4099, 520)])
def test_layernorm_backward_pitches_and_neighbours(rows, D):
    """Row pitches D + 8 (x), D + 16 (dy), D + 24 (dres) with NaN pads, D + 8 (dx) with a sentinel; exact workspace with a sentinel
    tail.  Bitwise the dense run."""
    x, gamma, dy, dres = H.spiked_ln_case(rows, D, seed=rows * 3 + D + 1)
    ref = H.ln_grads_ref64(x, gamma, dy, dres, 1e-6)
    want = H.layernorm_backward(*dev(x, gamma, dy), dres=dres.to(DEV))
    x_p, _ = padded(x, 8)
    dy_p, _ = padded(dy, 16)
    dres_p, _ = padded(dres, 24)
    dx_p, dx_w = sentinel_out(rows, D, 8)
    nb = H._lib.load().ov_layernorm_backward_workspace_bytes(rows, D)
    ws, buf = exact_ws(nb)
    got = H.layernorm_backward(x_p, gamma.to(DEV), dy_p, dres=dres_p, dx=dx_p, ws=ws)
    torch.cuda.synchronize()
    assert got[0].stride(0) == D + 8
    assert ws_intact(buf, nb), "the workspace was overrun"
    assert pads_intact(dx_w, D)
    check_ln(f"padded rows={rows} D={D}", got, ref)
    assert same(got, want)


# ------------------------------------------------------------------------------------------------------------------------------
# C. GELU backward


def check_gelu(tag, da, h, a, dh, tanh):
    r = H.gelu_err_ratio(da.cpu(), h.cpu(), a, dh, tanh)
    print(f"gelu backward {'tanh' if tanh else 'erf'} {tag}: max err / bound da {r[0]:.3f} h {r[1]:.3f}")
    assert max(r) <= 1.0 and all(v == v for v in r), r
    return r


@functools.lru_cache(maxsize=None)
def gelu_case(rows, N):
    return (H.rnd(rows, N, seed=rows + N) * 2.0).to(torch.bfloat16), H.rnd(rows, N, seed=rows + N + 1).to(torch.bfloat16)


def run_gelu(tag, a, dh, tanh):
    """Out of place with h_out, twice (bitwise), then in place (da = dh, as the block's chain calls it): bitwise the same."""
    ad, dhd = dev(a, dh)
    da, h = H.gelu_backward(ad, dhd, tanh, with_h=True)
    check_gelu(tag, da, h, a, dh, tanh)
    da2, h2 = H.gelu_backward(ad, dhd, tanh, with_h=True)
    assert torch.equal(da.view(torch.int16), da2.view(torch.int16)) and torch.equal(h.view(torch.int16), h2.view(torch.int16))
    assert torch.equal(H.gelu_backward(ad, dhd, tanh).view(torch.int16), da.view(torch.int16))          # h_out changes nothing in da
    buf = dhd.clone()
    da3, h3 = H.gelu_backward(ad, buf, tanh, with_h=True, inplace=True)
    assert da3.data_ptr() == buf.data_ptr()
    assert torch.equal(da3.view(torch.int16), da.view(torch.int16)) and torch.equal(h3.view(torch.int16), h.view(torch.int16))
    assert torch.equal(ad.cpu().view(torch.int16), a.view(torch.int16))                                 # the input is left alone


@pytest.mark.parametrize("tanh", [False, True])
def test_gelu_backward_every_bf16_value(tanh):
    """Every finite bf16 a with |a| <= 2^16, -0.0 and the subnormals included, against dh = 1, -3 and 2^-20, in one launch: no NaN,
    and every element inside the bound -- the whole negative tail, where |gelu'| is below any fixed atol, included."""
    a, dh = H.gelu_all_values_case()
    assert a.shape[0] * 8 >= 3 * 36000 and set(dh[:, 0].tolist()) == set(GELU_DH)
    run_gelu("all values", a, dh, tanh)


@pytest.mark.parametrize("rows,N", [(3, 8), (300, 1544), (2049, 8200)])
@pytest.mark.parametrize("tanh", [False, True])
def test_gelu_backward_shapes(tanh, rows, N):
    """(3, 8): one thread's worth per row; (300, 1544): 193 chunks per row, the block's shape class; (2049, 8200): 2049 * 1025 chunks,
    more than the grid's 8192 * 256 threads, so the grid-stride loop turns."""
    if rows == 2049:
        assert rows * (N // 8) > 8192 * 256
    a, dh = gelu_case(rows, N)
    run_gelu(f"rows={rows} N={N}", a, dh, tanh)


@pytest.mark.parametrize("tanh", [False, True])
def test_gelu_backward_pitches_and_neighbours(tanh):
    """Row pitches N + 8 (a), N + 16 (dh) with NaN pads; N + 24 (da), N + 8 (h_out) with a sentinel.  Bitwise the dense run."""
    rows, N = 300, 1544
    a, dh = gelu_case(rows, N)
    want = H.gelu_backward(*dev(a, dh), tanh, with_h=True)
    a_p, _ = padded(a, 8)
    dh_p, _ = padded(dh, 16)
    da_p, da_w = sentinel_out(rows, N, 24)
    h_p, h_w = sentinel_out(rows, N, 8)
    da, h = H.gelu_backward(a_p, dh_p, tanh, da=da_p, h=h_p)
    torch.cuda.synchronize()
    assert (da.stride(0), h.stride(0)) == (N + 24, N + 8)
    assert pads_intact(da_w, N) and pads_intact(h_w, N)
    check_gelu(f"padded rows={rows} N={N}", da, h, a, dh, tanh)
    assert torch.equal(da.view(torch.int16), want[0].view(torch.int16)) and torch.equal(h.view(torch.int16), want[1].view(torch.int16))
