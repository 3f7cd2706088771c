"""The persistent GEMM's tile walks and store policies against an independent fp64 reference.

The other GEMM tests compare sibling launches bit for bit (persistent against plain, ov_gemm_keep against two ov_gemm calls), which
is blind to anything both get wrong alike: a tile the walk skips or visits twice, a store form that drops columns.  Here every
form the launcher selects by size (gemm.hip: gemm_route) is compared with
A.double() @ W.double().T (+ bias) (+ R) computed by torch ON THE DEVICE (rocBLAS fp64: the fp64-on-device route of the two the
plan allowed), in row chunks so that no fp64 temporary exceeds 1 GB.

Bound per element, derived, not tuned (REL = 2^-8 = hipops.REL: one bf16 rounding, half an ulp of an 8-bit significand, is at most
2^-8 of the value -- reached just above a power of two, so a correct kernel comes close to ratio 1):

    bias:      |got - ref| <= REL |ref| + K 2^-24 S + 1e-6,           S = |A| |W|^T + |bias| (+ |R|)
               (one rounding of the output; K 2^-24 S = worst-case fp32 accumulation error in any order; S from an fp32 matmul)
    residual:  the same + REL (1 + REL) |pre|,  pre = A W^T + bias.
               The residual epilogue is out = bf16(bf16(acc + bias) + R) (common.h, epi_combine: "combine(bf16(acc + bias), R)") --
               the Linear's output is rounded to bf16 before the residual is added, as the bf16 model this path replaces does
               (a bf16 nn.Linear, then x + y in bf16).  A bound with ONE rounding (the first line) therefore does not hold for a
               correct kernel wherever pre and R cancel (err up to 2^-8 |pre| where |ref| ~ 0): a torch fp32 restatement of the
               epilogue on a (300, 200, 192) problem of the same distribution gives max err / bound = 42 with it, and the residual
               tests print the ratio under it next to the asserted one.  Corrected derivation: two roundings, of pre (REL |pre|) and
               of the sum, which carries the first rounding's error (REL (|ref| + REL |pre|)).
               A tile visited twice adds pre twice (the runs are in place, C aliasing R): err = |pre|, 256 x the extra term.
    GELU:      1.13 x (the bias bound, for the pre-activation) + REL |ref| + E      (1.13 = max |gelu'|)
               E, erf form: common.h states |GELU error| <= 1.4e-4 on [-4, 4] and <= 6.6e-5 |x| beyond (gelu_erf_f2; a Python
               restatement of the polynomial on a 2^-12 grid over [-8, 8] gives 1.376e-4 and 6.61e-5 |x|): E = max(1.4e-4, 6.6e-5 |pre|).
               E, tanh form: common.h states no figure.  gelu_tanh_f2 is the closed form x / (1 + exp2(-2 log2(e) u)), algebraically
               the tanh GELU, so the restatement in fp64 differs from fp64 0.5 x (1 + tanh u) by 1.8e-15; evaluated in fp32 (numpy,
               the same operation order) on the 2^-12 grid over [-8, 8] the maximum difference is 5.2e-7 (the |x| weighting
               included: it is the error of the GELU value itself).  With the factor 2: E = 1.1e-6.
    GELU':     the GELU-gradient epilogues, out = bf16(bf16(pre) g32(R)):  |g'(R)| (the bias bound) + delta (|pre| + the bias bound)
               + REL |ref| against pre g'(R) with the exact fp64 derivative; delta = hipops.DELTA_GRAD_ERF / _TANH.
    LN fold:   x Wg - mean colsum cancels, the bounds above do not apply.  Two rules, both asserted: hipops.fold_bound, derived from
               the kernel's formula on the operands it receives (no tuned term; see there), and the older tuned rule of
               test_gemm_ln_fold_matches_layernorm_then_linear, |got - ref| <= 2e-2 + 1.5e-2 |ref| against Linear(LayerNorm(x)) in
               fp64, the same input construction (mean 0.4, spread 1.7).

The helpers (route, linear_ratios, report, ...) live in hipops.py, shared with test_gpu_gemm_small_routes.py.

Every output starts as the bf16 sentinel 77, so a skipped tile fails the bound instead of passing as zeros, and padding behind the
last valid column must still hold it.  Every case asserts, on what the library itself reports for the call (ov_gemm_route through
hipops.route: the launcher's own decision for this device's CU count), that the form it names is the one selected; what the launcher
decides at each rule's edge is pinned without a GPU by test_gemm_route_cpu.py."""
import functools
import os
import tempfile
from types import SimpleNamespace

import pytest
import torch

import hipops as H
from hipops import BM, BN, DEV, SENT, fold_ratios_bound, linear_ratios, ln_linear_ratios, padding_kept, report, route, sentinel
from ranks import run_child

pytestmark = pytest.mark.gpu


# case -> (M, N, K), the walk it must select, and what else makes it the case it is (each asserted before the launch)
CASES = {
    1: ((22100, 768, 192), "plain", [("tile count not a multiple of 8: XCD runs of unequal length", lambda r: r.nwg % 8 != 0),
                                     ("ragged last row tile", lambda r: 22100 % BM != 0)]),
    2: ((17052, 840, 192), "rotated", [("tiles_n = 4", lambda r: r.tn == 4 and r.rot == 3), ("72-column last n-tile", lambda r: r.rem == 72),
                                       ("67 row panels, pr = 3", lambda r: r.tm == 67 and r.pr == 3)]),
    3: ((8904, 1800, 192), "rotated", [("tiles_n = 8", lambda r: r.tn == 8 and r.rot == 7), ("8-column last n-tile", lambda r: r.rem == 8),
                                       ("W is 0.75 MiB", lambda r: r.wbytes == 3 << 18), ("35 panels", lambda r: r.tm == 35)]),
    4: ((8904, 2048, 832), "grouped", [("2 groups", lambda r: r.groups == 2), ("35 panels: XCDs own 5, 5, 5, 4, ...", lambda r: r.tm == 35 and r.pr == 3)]),
    5: ((8904, 1800, 832), "grouped", [("8-column last n-tile", lambda r: r.rem == 8), ("2 groups", lambda r: r.groups == 2)]),
    6: ((5688, 3072, 576), "grouped", [("3 groups", lambda r: r.groups == 3), ("23 panels, pr = 7", lambda r: r.tm == 23 and r.pr == 7)]),
    7: ((8192, 2048, 832), "grouped", [("one tile per workgroup", lambda r: r.nwg == r.cus)]),
    8: ((8904, 2048, 4096), "grouped", [("2 groups", lambda r: r.groups == 2), ("35 panels", lambda r: r.tm == 35)]),
    # rowparts only: case 2's form at the nearest N that ov_gemm_rowparts admits (N % 32 == 0; 840 is refused, see the rowparts test)
    "2r": ((17052, 832, 192), "rotated", [("tiles_n = 4", lambda r: r.tn == 4 and r.rot == 3), ("64-column last n-tile", lambda r: r.rem == 64),
                                          ("67 row panels, pr = 3", lambda r: r.tm == 67 and r.pr == 3)]),
    # the store-policy threshold itself, in a process without OVHIP_GEMM_NT_MIN_MB
    "203MB": ((24832, 4096, 192), "plain", [("output of at least 192 MB", lambda r: not r.st_plain)]),
}


def check_route(case, r, rev=False):
    """Asserts that `r`, what the library reports for a call at `case`'s shape, is the kernel form the case is in the table for."""
    (M, N, K), walk, extra = CASES[case]
    assert r.kernel == "persistent", f"case {case} {(M, N, K)}: {r.nwg} tiles on {r.cus} CUs, K = {K} selects the {r.kernel} kernel"
    got = "grouped" if r.grouped else "rotated" if r.rot else "plain"
    assert got == walk, f"case {case} {(M, N, K)}: the launcher selects the {got} walk, the case is there for the {walk} walk"
    for what, holds in extra:
        assert holds(r), f"case {case} {(M, N, K)} on {r.cus} CUs no longer has: {what}"
    assert r.rev == rev, f"case {case} {(M, N, K)}: descending row walk {r.rev}, wanted {rev}"


def selected(case, epi=0, keep=False, rev=False, **operands):
    """Asserts that `case` reaches the kernel form it is in the table for; returns its shape.  operands: fold= / rowparts= of the call."""
    M, N, K = CASES[case][0]
    check_route(case, route(M, N, K, epi, keep, **operands), rev)
    return M, N, K


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """A, W bf16, bias fp32 on the device (CPU generator: the child processes build the same)."""
    g = torch.Generator().manual_seed(1000003 * K + 1009 * N + M)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    return a, w, torch.randn(N, generator=g).to(DEV)


@functools.lru_cache(maxsize=None)
def residual(M, N):
    g = torch.Generator().manual_seed(7 * M + N)
    return torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)


@functools.lru_cache(maxsize=None)
def fold_operands(M, N, K):
    """The LN-folded operands of test_gemm_ln_fold_matches_layernorm_then_linear: x, Wg, cvec, colsum and the unfolded w, bias, gamma,
    beta (fp32) the reference uses."""
    rnd = lambda *s, seed: torch.randn(*s, generator=torch.Generator().manual_seed(seed + M + N + K))
    x = (rnd(M, K, seed=30) * 1.7 + 0.4).to(torch.bfloat16)
    w, bias = rnd(N, K, seed=31) / K ** 0.5, rnd(N, seed=32) * 0.1
    gamma, beta = rnd(K, seed=33) * 0.1 + 1, rnd(K, seed=34) * 0.1
    wg = (w * gamma[None, :]).to(torch.bfloat16)
    colsum = wg.float().sum(1)
    cvec = w.to(torch.bfloat16).float() @ beta + bias
    return tuple(t.to(DEV) for t in (x, wg, cvec, colsum, w, bias, gamma, beta))


def fold_ratios(M, N, K, outs):
    """outs: name -> (bf16 [M, >= N], epi 0 | 1 | 2) of ov_gemm_ln on fold_operands(M, N, K): max err / (atol + rtol |ref|) against
    Linear(LayerNorm(x)) (then GELU) in fp64."""
    return ln_linear_ratios(fold_operands(M, N, K), outs)


EPI_KIND = {0: "pre", 1: "erf", 2: "tanh", 3: "res", 4: "gerf", 5: "gtanh"}
EPI_NAME = {0: "bias", 1: "gelu erf", 2: "gelu tanh", 4: "gelu' erf", 5: "gelu' tanh"}


@pytest.mark.parametrize("case,epi", [(case, epi) for case in (1, 2, 3, 4, 5, 6, 7) for epi in (0, 1, 3)] + [(1, 2), (1, 4), (1, 5)])
def test_walk_epilogues_within_the_fp64_bound(case, epi):
    """Bias, erf-GELU and in-place residual epilogues over the plain, rotated and grouped walks of the case table; on case 1 the
    persistent kernel's tanh-GELU and GELU-gradient instantiations too (R = the pre-activation, out of place)."""
    M, N, K = selected(case, epi)
    a, w, bias = operands(M, N, K)
    if epi == 3:
        r = residual(M, N)
        out = r.clone()
        H.gemm(a, w, bias, epi=3, resid=out, out=out)
        res = linear_ratios(a, w, bias, {"residual": (out, "res"), "residual (one-rounding bound)": (out, "res1")}, r)
        report(f"case {case} {(M, N, K)}", res, skip=("residual (one-rounding bound)",))
    else:
        r = residual(M, N) if epi > 3 else None
        out = H.gemm(a, w, bias, epi=epi, resid=r, out=sentinel(M, N))
        report(f"case {case} {(M, N, K)}", linear_ratios(a, w, bias, {EPI_NAME[epi]: (out, EPI_KIND[epi])}, r))


def test_grouped_walk_with_descending_rows_residual():
    """Case 8: K >= 2 N, so the residual epilogue walks the row tiles of the grouped walk from the last to the first."""
    M, N, K = selected(8, 3, rev=True)
    a, w, bias = operands(M, N, K)
    r = residual(M, N)
    out = r.clone()
    H.gemm(a, w, bias, epi=3, resid=out, out=out)
    res = linear_ratios(a, w, bias, {"residual": (out, "res"), "residual (one-rounding bound)": (out, "res1")}, r)
    report(f"case 8 {(M, N, K)}", res, skip=("residual (one-rounding bound)",))


@pytest.mark.parametrize("case", [4, 6])
def test_grouped_walk_keep_both_outputs(case):
    """ov_gemm_keep over the grouped walk: the GELU output and the kept pre-activation, padded ldc / ldc2."""
    M, N, K = selected(case, 1, keep=True)
    a, w, bias = operands(M, N, K)
    out, pre = H.gemm_keep(a, w, bias, 1, ldc=N + 64, ldc2=N + 8, fill=SENT)
    report(f"case {case} {(M, N, K)} keep", linear_ratios(a, w, bias, {"gelu erf": (out, "erf"), "pre-activation": (pre, "pre")}))
    assert padding_kept(out, N) and padding_kept(pre, N)


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("case", [4, 6])
def test_grouped_walk_ln_fold(case, epi):
    M, N, K = selected(case, epi, fold=True)
    x, wg, cvec, colsum = fold_operands(M, N, K)[:4]
    st = H.rowstats(x)
    out = H.gemm_ln(x, wg, cvec, colsum, st, epi=epi, out=sentinel(M, N + 8))
    report(f"case {case} {(M, N, K)} LN fold", fold_ratios(M, N, K, {("bias", "gelu erf")[epi]: (out, epi)}))
    report(f"case {case} {(M, N, K)} LN fold, fold_bound", fold_ratios_bound(x, wg, colsum, cvec, st, {("bias", "gelu erf")[epi]: (out, epi)}))
    assert padding_kept(out, N)


@pytest.mark.parametrize("case", ["2r", 4, 8])
def test_walk_rowparts(case):
    """ov_gemm_rowparts (the residual epilogue with fused row statistics), in place as the tower calls it: the output against fp64,
    the parts against the 32-column sums and sums of squares of the stored output in fp64 (rtol 1e-5, atol 1e-4: the rule of
    test_gemm_rowparts_are_the_row_partial_sums_of_the_output).  The rotated walk runs at N = 832 instead of case 2's 840: the entry
    point needs N % 32 == 0 and refuses 840, which is asserted; 832 keeps tiles_n = 4, the 67 panels and a half last n-tile."""
    if case == "2r":
        M2, N2, K2 = CASES[2][0]
        a2, w2, b2 = operands(M2, N2, K2)
        with pytest.raises(H._lib.OvhipError):
            H.gemm_rowparts(a2, w2, b2, residual(M2, N2), parts=torch.empty(M2, N2 // 32, 2, device=DEV))
    M, N, K = selected(case, 3, rev=case == 8, rowparts=True)
    a, w, bias = operands(M, N, K)
    r = residual(M, N)
    out = r.clone()
    _, parts = H.gemm_rowparts(a, w, bias, out, out=out)
    res = linear_ratios(a, w, bias, {"residual": (out, "res"), "residual (one-rounding bound)": (out, "res1")}, r)
    report(f"case {case} {(M, N, K)} rowparts", res, skip=("residual (one-rounding bound)",))
    assert not torch.isnan(parts).any()
    x = out.double().view(M, N // 32, 32)
    for j, want in enumerate((x.sum(-1), (x * x).sum(-1))):
        err = (parts[..., j].double() - want).abs()
        assert bool((err <= 1e-4 + 1e-5 * want.abs()).all()), (case, j, float(err.max()))


def test_output_of_203_mb_is_streamed_by_the_default_threshold():
    """No environment set: a 203 MB output crosses the 192 MB rule, so the bias epilogue stores with streaming stores and the LN-folded
    GELU takes the LDS-transposed streamed form -- the production combination, selected by the threshold itself."""
    for v in ("OVHIP_GEMM_NT_MIN_MB", "OVHIP_GEMM_GELU_LDS"):
        assert v not in os.environ, f"{v} is set: this test is about the defaults"
    M, N, K = selected("203MB")
    a, w, bias = operands(M, N, K)
    out = H.gemm(a, w, bias, epi=0, out=sentinel(M, N))
    report(f"203 MB {(M, N, K)}", linear_ratios(a, w, bias, {"bias, streamed": (out, "pre")}))
    del out
    x, wg, cvec, colsum = fold_operands(M, N, K)[:4]
    out = H.gemm_ln(x, wg, cvec, colsum, H.rowstats(x), epi=1, out=sentinel(M, N))
    report(f"203 MB {(M, N, K)}", fold_ratios(M, N, K, {"LN fold + gelu erf, LDS form streamed": (out, 1)}))


# ---- store policy and the GELU-form switch: read once per process, so each setting runs in a child process of its own ----

CHILD_CASES = (1, 3, 4, 6)
LINEAR_FORMS = {"bias": "pre", "gelu erf": "erf", "gelu tanh": "tanh", "keep gelu erf": "erf", "keep pre-activation": "pre"}
FOLD_FORMS = {"fold bias": 0, "fold gelu erf": 1, "fold gelu tanh": 2}
SETTINGS = {
    "default": ({}, "all"),
    "streamed": ({"OVHIP_GEMM_NT_MIN_MB": "0"}, "all"),
    "lds form, plain stores": ({"OVHIP_GEMM_GELU_LDS": "1"}, "foldgelu"),
    "direct form, streamed": ({"OVHIP_GEMM_GELU_LDS": "0", "OVHIP_GEMM_NT_MIN_MB": "0"}, "foldgelu"),
}


ROUTE_CALLS = {"bias": dict(epi=0), "gelu erf": dict(epi=1), "gelu tanh": dict(epi=2), "keep gelu erf": dict(epi=1, keep=True),
               "fold bias": dict(epi=0, fold=True), "fold gelu erf": dict(epi=1, fold=True), "fold gelu tanh": dict(epi=2, fold=True)}


def child_main(path, which):
    """(In the child process.)  Every entry point over CHILD_CASES, outputs to `path`; which = foldgelu: the LN-folded GELUs only.
    Beside them what the library reports, under this process's switches, for every call of ROUTE_CALLS."""
    outs, routes = {}, {}
    for case in CHILD_CASES:
        M, N, K = CASES[case][0]
        for name, call in ROUTE_CALLS.items():
            routes[case, name] = vars(route(M, N, K, **call))
        if which == "all":
            a, w, bias = operands(M, N, K)
            for name, epi in (("bias", 0), ("gelu erf", 1), ("gelu tanh", 2)):
                outs[case, name] = H.gemm(a, w, bias, epi=epi, out=sentinel(M, N)).cpu()
            out, pre = H.gemm_keep(a, w, bias, 1, ldc=N + 64, ldc2=N + 8, fill=SENT)
            outs[case, "keep gelu erf"], outs[case, "keep pre-activation"] = out.cpu(), pre.cpu()
        x, wg, cvec, colsum = fold_operands(M, N, K)[:4]
        st = H.rowstats(x)
        for name, epi in FOLD_FORMS.items():
            if which == "all" or epi:
                outs[case, name] = H.gemm_ln(x, wg, cvec, colsum, st, epi=epi, out=sentinel(M, N)).cpu()
    torch.save({"outs": outs, "routes": routes}, path)


@functools.lru_cache(maxsize=None)
def child_outputs(setting):
    """Runs the child of `setting` (once per session, one child at a time) and returns what it saved: (outputs, routes)."""
    env_add, which = SETTINGS[setting]
    env = {"OVHIP_GEMM_NT_MIN_MB": None, "OVHIP_GEMM_GELU_LDS": None, **env_add}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "outs.pt")
        code = "import test_gpu_gemm_routes as T; T.child_main(sys.argv[1], sys.argv[2])"
        run_child(code, path, which, env=env, timeout=300, gpu=True)
        saved = torch.load(path)
        return saved["outs"], saved["routes"]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_store_policy_outputs_within_the_fp64_bound(setting):
    """Every output of the child under `setting` -- plain stores (default), every bias / GELU output streamed
    (OVHIP_GEMM_NT_MIN_MB=0; the folded GELU then in its LDS-transposed form: the production combination), the LDS form with plain
    stores (OVHIP_GEMM_GELU_LDS=1), the direct form streamed (GELU_LDS=0, NT_MIN_MB=0) -- within its bound.  First, on what the
    library reported IN THE CHILD for each of its calls: the case's kernel form, the store policy of the setting, and the folded
    GELU's form -- LDS-transposed under GELU_LDS=1, direct under =0, and without the switch direct exactly when stored plainly."""
    env_add, which = SETTINGS[setting]
    nt = int(env_add.get("OVHIP_GEMM_NT_MIN_MB", 192))
    outs, routes = child_outputs(setting)
    gelu_lds = env_add.get("OVHIP_GEMM_GELU_LDS")
    for case in CHILD_CASES:
        M, N, K = CASES[case][0]
        for name in ROUTE_CALLS:
            r = SimpleNamespace(**routes[case, name])
            check_route(case, r)
            assert r.st_plain == (nt != 0), (case, name, nt)
            assert (r.fold, r.keep) == (name.startswith("fold"), name.startswith("keep")), (case, name)
            if name in ("fold gelu erf", "fold gelu tanh"):
                assert r.direct == (gelu_lds == "0" if gelu_lds is not None else r.st_plain), (case, name, setting, r.direct)
        dev = {name: t.to(DEV) for (c, name), t in outs.items() if c == case}
        assert set(dev) == (set(LINEAR_FORMS) | set(FOLD_FORMS) if which == "all" else {"fold gelu erf", "fold gelu tanh"})
        tag = f"[{setting}] case {case} {(M, N, K)}"
        if which == "all":
            a, w, bias = operands(M, N, K)
            report(tag, linear_ratios(a, w, bias, {n: (dev[n], kind) for n, kind in LINEAR_FORMS.items()}))
            assert padding_kept(dev["keep gelu erf"], N) and padding_kept(dev["keep pre-activation"], N)
        report(tag, fold_ratios(M, N, K, {n: (dev[n], epi) for n, epi in FOLD_FORMS.items() if n in dev}))


def _bitwise(x, y, names):
    for case in CHILD_CASES:
        for name in names:
            assert torch.equal(x[case, name], y[case, name]), (case, name)


def test_streamed_stores_are_bitwise_the_plain_stores():
    """OVHIP_GEMM_NT_MIN_MB=0 changes only the store instruction of the forms whose instantiation it leaves alone: bias, unfolded GELU,
    KEEP (both outputs, padding included) and fold + bias equal the default process's outputs bit for bit."""
    _bitwise(child_outputs("default")[0], child_outputs("streamed")[0], list(LINEAR_FORMS) + ["fold bias"])


def test_lds_gelu_form_plain_stores_bitwise_the_streamed():
    """OVHIP_GEMM_GELU_LDS=1 under the default threshold (LDS form, plain stores) against NT_MIN_MB=0 (LDS form by default, streamed)."""
    _bitwise(child_outputs("lds form, plain stores")[0], child_outputs("streamed")[0], ["fold gelu erf", "fold gelu tanh"])


def test_direct_gelu_form_streamed_bitwise_the_default():
    """OVHIP_GEMM_GELU_LDS=0 with NT_MIN_MB=0 (direct form, streamed) against the default process (direct form, plain stores)."""
    _bitwise(child_outputs("direct form, streamed")[0], child_outputs("default")[0], ["fold gelu erf", "fold gelu tanh"])
