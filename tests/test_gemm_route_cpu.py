"""CPU: what the bf16 GEMM launcher decides, asked of the library itself (ov_gemm_route at 256 CUs; it launches nothing and needs no
device).

Part 1 pins, in a literal table, the kernel and walk of every shape the GPU route tests run (test_gpu_gemm_routes.CASES and the
tables of hipops.py): if the launcher's rules drift, this fails here, before those tests quietly cover another kernel form.
Part 2 walks each rule of gemm.hip's gemm_route at its edge, with pairs of calls that differ in the one condition named.  The
expected values are read off the rules as the code and DESIGN.md state them (96 tiles, the CU count, 3 K-tiles, 3 MiB of W, a last
n-tile of at most 128 columns, K >= 2 N, 192 MiB of output), not off what the library returns."""
import json
import os

import pytest

import hipops as H
import test_gpu_gemm_routes as RT
from hipops import route
from ranks import run_child

CUS = 256
MIB = 1 << 20


def r256(M, N, K, epi=0, **kw):
    return route(M, N, K, epi, cus=CUS, **kw)


def form(r):
    """(kernel, walk, groups, rotmask) as the table below writes it."""
    return r.kernel, "grouped" if r.grouped else "rotated" if r.rot else "plain", r.groups, r.rot


# ---- part 1: the tests' own shapes.  The walk columns are reported for every shape; only the persistent kernel reads them.

CASE_FORMS = {
    1: ((22100, 768, 192), ("persistent", "plain", 1, 0)),
    2: ((17052, 840, 192), ("persistent", "rotated", 1, 3)),
    3: ((8904, 1800, 192), ("persistent", "rotated", 1, 7)),
    4: ((8904, 2048, 832), ("persistent", "grouped", 2, 0)),
    5: ((8904, 1800, 832), ("persistent", "grouped", 2, 0)),
    6: ((5688, 3072, 576), ("persistent", "grouped", 3, 0)),
    7: ((8192, 2048, 832), ("persistent", "grouped", 2, 0)),
    8: ((8904, 2048, 4096), ("persistent", "grouped", 2, 0)),
    "2r": ((17052, 832, 192), ("persistent", "rotated", 1, 3)),
    "203MB": ((24832, 4096, 192), ("persistent", "plain", 1, 0)),
}
SMALL_FORMS = {
    (1, 8, 64): ("skinny", "plain", 1, 0),
    (65, 72, 128): ("skinny", "plain", 1, 0),
    (130, 200, 192): ("skinny", "plain", 1, 0),
    (257, 264, 256): ("skinny", "rotated", 1, 1),
    (63, 1096, 320): ("skinny", "plain", 1, 0),
    (300, 96, 576): ("skinny", "plain", 1, 0),
    (24827, 8, 64): ("plain", "plain", 1, 0),
    (1, 24584, 128): ("plain", "plain", 1, 0),
    (2500, 2568, 192): ("plain", "plain", 1, 0),
    (2305, 2816, 320): ("plain", "plain", 1, 0),
    (257, 288, 256): ("skinny", "rotated", 1, 1),
    (2500, 2592, 192): ("plain", "plain", 1, 0),
    (25000, 200, 64): ("plain", "plain", 1, 0),             # MAPPED_GELU_CASE
    (150, 200, 192): ("skinny", "plain", 1, 0),              # ROWMAP_CASE: B g^2 rows
}


def test_the_route_tests_cases_reach_the_forms_they_name():
    assert {c: s for c, (s, _) in CASE_FORMS.items()} == {c: s for c, (s, _, _) in RT.CASES.items()}, "CASES changed: extend CASE_FORMS"
    for case, (shape, want) in CASE_FORMS.items():
        for epi in (0, 1, 3):
            r = r256(*shape, epi)
            assert form(r) == want and want[1] == RT.CASES[case][1], (case, epi, form(r))
            RT.check_route(case, r, rev=(case == 8 and epi == 3))            # the GPU tests' own assertions, here at 256 CUs
    assert not r256(*CASE_FORMS["203MB"][0]).st_plain and r256(*CASE_FORMS[1][0]).st_plain


def test_the_small_route_tests_shapes_reach_the_kernels_they_name():
    B, g2, D, K = H.ROWMAP_CASE
    shapes = H.SKINNY_SHAPES + H.PLAIN_SHAPES + H.ROWPARTS_SHAPES + [H.MAPPED_GELU_CASE[:3], (B * g2, D, K)]
    assert set(shapes) == set(SMALL_FORMS), "the shape tables of hipops.py changed: extend SMALL_FORMS"
    for shape in shapes:
        for epi in (0, 1, 2, 3, 4, 5):
            assert form(r256(*shape, epi)) == SMALL_FORMS[shape], (shape, epi)
        assert r256(*shape).kernel == ("plain" if shape in H.PLAIN_SHAPES else SMALL_FORMS[shape][0])
    for shape in H.ROWPARTS_SHAPES:                            # the skinny kernel writes the parts itself, the plain one is followed
        r = r256(*shape, 3, rowparts=True)
        assert form(r) == SMALL_FORMS[shape] and not r.stats and r.rowparts_pass == (r.kernel == "plain"), shape
    for shape in H.FOLD_SHAPES + [H.FOLD_CLEAN_ONLY]:
        assert r256(*shape, 1, fold=True).kernel == ("plain" if shape in H.PLAIN_SHAPES else "skinny"), shape
    assert form(r256(*H.MAPPED_GELU_CASE[:3], 1, mapped=True)) == SMALL_FORMS[H.MAPPED_GELU_CASE[:3]]
    for epi in (0, 3):
        assert form(r256(B * g2, D, K, epi, mapped=True)) == SMALL_FORMS[B * g2, D, K]
    keep = r256(*H.PLAIN_ALL_EPI[0], 1, keep=True)
    assert keep.kernel == "plain" and keep.keep_prepass


# ---- part 2: each rule at its edge (256 CUs unless said otherwise)


def test_skinny_kernel_up_to_96_tiles():
    assert r256(96 * 256, 256, 192).kernel == "skinny" and r256(96 * 256 + 1, 256, 192).kernel == "plain"          # 96 | 97 x 1 tiles
    assert r256(256, 96 * 256, 192).kernel == "skinny" and r256(256, 96 * 256 + 8, 192).kernel == "plain"          # 1 x 96 | 97


def test_persistent_kernel_from_one_tile_per_cu():
    assert r256(255 * 256, 256, 192).kernel == "plain" and r256(256 * 256, 256, 192).kernel == "persistent"       # 255 | 256 tiles
    assert route(256 * 256, 256, 192, cus=304).kernel == "plain" and route(304 * 256, 256, 192, cus=304).kernel == "persistent"


def test_persistent_kernel_needs_three_k_tiles():
    assert r256(256 * 256, 256, 128).kernel == "plain" and r256(256 * 256, 256, 192).kernel == "persistent"
    assert r256(256, 256, 64).kernel == "skinny"               # the skinny kernel has no such minimum


def test_groups_of_four_once_w_exceeds_3_mib():
    M = 32 * 256                                               # 32 row panels: 256 tiles and more (tiles_m >= 16 is walked below)
    for N, K, groups in ((2048, 768, 1),                       # tiles_n = 8: W = 8 x 256 x 768 x 2 B = 3 MiB exactly
                         (2048, 832, 2),                       # one K-tile more
                         (3072, 512, 1),                       # tiles_n = 12: 3 MiB exactly
                         (4096, 512, 4)):                      # the next tiles_n that is a multiple of 4: 4 MiB
        r = r256(M, N, K)
        assert r.wbytes > 3 * MIB if groups > 1 else r.wbytes == 3 * MIB
        assert (r.kernel, r.groups, r.grouped) == ("persistent", groups, groups > 1), (N, K, r.groups)
    assert r256(M, 2048 + 256, 832).groups == 1                # one n-tile more than 8: 9 is no multiple of 4
    assert r256(M, 2560, 1024).groups == 1 and r256(M, 3072, 1024).groups == 3                                    # tiles_n = 10 | 12
    assert r256(64 * 256, 1024, 2048).groups == 1 and r256(64 * 256, 2048, 1024).groups == 2                      # tiles_n = 4 | 8, 4 MiB both
    assert r256(15 * 256, 5120, 512).groups == 1 and r256(16 * 256, 5120, 512).groups == 5                         # tiles_m = 15 | 16
    assert r256(15 * 256, 5120, 512).kernel == "persistent"


def test_rotated_walk_for_a_half_last_n_tile():
    M = 64 * 256
    assert r256(M, 768 + 128, 192).rot == 3 and r256(M, 768 + 136, 192).rot == 0                                 # rem = 128 | 136
    assert r256(M, 768 + 8, 192).rot == 3 and r256(M, 1024, 192).rot == 0                                        # rem = 8 | 0
    assert r256(M, 128, 192).rot == 0                          # a single n-tile has nothing to rotate
    # tiles_n a power of two or not, with the workgroup stride a multiple of tiles_n in both: 384 CUs, 48 per XCD, tiles_n = 4 | 3
    assert route(M, 768 + 128, 192, cus=384).rot == 3 and route(M, 512 + 128, 192, cus=384).rot == 0
    assert route(M, 768 + 128, 192, cus=304).rot == 0          # 38 workgroups per XCD: no multiple of 4
    assert route(M, 768 + 128, 192, cus=252).rot == 0          # a CU count that is no multiple of 8
    # the grouped walk is not rotated: tiles_n = 8, rem = 128, W of 3 MiB | one K-tile more
    assert r256(M, 1792 + 128, 768).rot == 7 and (r256(M, 1792 + 128, 832).rot, r256(M, 1792 + 128, 832).groups) == (0, 2)


def test_descending_rows_for_the_wide_k_residual():
    M = 64 * 256
    assert r256(M, 1024, 2048, 3).rev and not r256(M, 1024, 2048 - 64, 3).rev                                    # K = 2 N | 2 N - 64
    for epi in (0, 1, 2, 4, 5):
        assert not r256(M, 1024, 2048, epi).rev, epi
    assert not r256(M, 1024, 2048, 3, mapped=True).rev


def test_outputs_from_192_mib_are_streamed():
    assert r256(24576 - 1, 4096, 192).st_plain and not r256(24576, 4096, 192).st_plain                          # M N 2 B = 192 MiB - 8 KiB | 192 MiB
    assert 24576 * 4096 * 2 == 192 * MIB


def test_keep_never_takes_the_skinny_kernel():
    for epi in (1, 2):
        assert r256(256, 256, 192, epi).kernel == "skinny"
        k = r256(256, 256, 192, epi, keep=True)
        assert k.kernel == "plain" and k.keep_prepass and not k.keep          # two launches of the plain kernel
        k = r256(256 * 256, 256, 192, epi, keep=True)
        assert (k.kernel, k.keep, k.direct, k.fold, k.keep_prepass) == ("persistent", True, True, False, False)


def test_statistics_are_fused_in_the_persistent_residual_form_only():
    big, mid, small = (256 * 256, 256, 192), (255 * 256, 256, 192), (256, 256, 192)
    r = r256(*big, 3, rowparts=True)
    assert (r.kernel, r.stats, r.direct, r.rowparts_pass) == ("persistent", True, True, False)
    r = r256(*big, 3)
    assert (r.kernel, r.stats, r.direct, r.rowparts_pass) == ("persistent", False, False, False)                # LDS-transposed form
    r = r256(*mid, 3, rowparts=True)
    assert (r.kernel, r.stats, r.rowparts_pass) == ("plain", False, True)
    r = r256(*small, 3, rowparts=True)
    assert (r.kernel, r.stats, r.rowparts_pass) == ("skinny", False, False)                                     # in its own epilogue
    lib, out = H._lib.load(), H._lib.GemmRoute()
    ask = lambda *a: lib.ov_gemm_route(*a, CUS, H.C.addressof(out))
    assert ask(*big, 3, 0, 0, 1, 1) == -2                      # rowparts with row maps: refused, as by ov_gemm_rowparts
    assert ask(65536, 264, 192, 3, 0, 0, 1, 0) == -2           # N % 32
    assert ask(*big, 0, 0, 0, 1, 0) == -2                      # residual epilogue only
    assert ask(*big, 3, 1, 0, 0, 0) == -2 and ask(*big, 0, 1, 1, 0, 0) == -2 and ask(*big, 0, 0, 1, 0, 0) == -2   # what ov_gemm_ln / _keep refuse
    assert ask(*big, 6, 0, 0, 0, 0) == -1 and ask(0, 256, 192, 0, 0, 0, 0, 0) == -1 and ask(256, 256, 100, 0, 0, 0, 0, 0) == -2
    assert lib.ov_gemm_route(*big, 0, 0, 0, 0, 0, CUS, None) == -1


def test_row_maps_send_gelu_to_the_plain_kernel():
    big = (256 * 256, 256, 192)
    for epi in (1, 2):
        assert r256(*big, epi).kernel == "persistent" and r256(*big, epi, mapped=True).kernel == "plain"
    r = r256(*big, 0, mapped=True)
    assert (r.kernel, r.mapped, r.direct) == ("persistent", True, False)
    r = r256(*big, 3, mapped=True)
    assert (r.kernel, r.mapped, r.direct, r.stats) == ("persistent", True, True, False)


def test_persistent_forms_of_each_epilogue_family():
    """The instantiation flags of every remaining form: bias and GELU gradient LDS-transposed, unfolded GELU direct, the folded GELU
    direct while its output is stored plainly and LDS-transposed once it is streamed."""
    plain_out, streamed = (24576 - 1, 4096, 192), (24576, 4096, 192)
    flags = lambda r: (r.kernel, r.fold, r.direct, r.mapped, r.keep, r.stats)
    for epi in (0, 4, 5):
        assert flags(r256(*plain_out, epi)) == ("persistent", False, False, False, False, False), epi
    assert flags(r256(*plain_out, 0, fold=True)) == flags(r256(*streamed, 0, fold=True)) == ("persistent", True, False, False, False, False)
    for epi in (1, 2):
        assert flags(r256(*plain_out, epi)) == flags(r256(*streamed, epi)) == ("persistent", False, True, False, False, False)
        assert flags(r256(*plain_out, epi, fold=True)) == ("persistent", True, True, False, False, False)
        assert flags(r256(*streamed, epi, fold=True)) == ("persistent", True, False, False, False, False)


# ---- the switches: read once per process, so each setting is asked in a child process (CPU only)

CHILD = ("import ctypes, json; import hipops as H; calls = json.loads(sys.argv[1]); "
         "print(json.dumps([vars(H.route(*c[0], cus=256, **c[1])) for c in calls]))")


def ask_child(env_add, calls):
    env = {**{k: None for k in os.environ if k.startswith("OVHIP_GEMM_")}, **env_add}
    out = run_child(CHILD, json.dumps(calls), env=env, timeout=120)
    return [H.SimpleNamespace(**d) for d in json.loads(out.stdout.strip().splitlines()[-1])]


SWITCH_CALLS = [((256, 256, 192), {}), ((255 * 256, 256, 192), {}), ((256 * 256, 256, 192), {}),
                ((256, 256, 192, 1), {"keep": True}), ((256 * 256, 256, 192, 1), {"keep": True}),
                ((256 * 256, 256, 192, 3), {"rowparts": True})]


@pytest.mark.parametrize("variant,kernels", [("", ["skinny", "plain", "persistent", "plain", "persistent", "persistent"]),
                                             ("2", ["plain"] * 6),
                                             ("4", ["skinny", "skinny", "skinny", "plain", "persistent", "skinny"]),
                                             ("3", ["skinny", "plain", "persistent", "plain", "persistent", "persistent"])])
def test_variant_switch_overrides_the_kernel(variant, kernels):
    """OVHIP_GEMM_VARIANT=2: the plain kernel for every shape; =4: the skinny kernel for every shape but ov_gemm_keep's, which it never
    serves; anything else: the default."""
    got = ask_child({"OVHIP_GEMM_VARIANT": variant} if variant else {}, SWITCH_CALLS)
    assert [r.kernel for r in got] == kernels
    assert [r.keep_prepass for r in got] == [k == "plain" and "keep" in c[1] for k, c in zip(kernels, SWITCH_CALLS)]
    assert got[5].rowparts_pass == (kernels[5] == "plain") and got[5].stats == (kernels[5] == "persistent")


@pytest.mark.parametrize("env,st_plain,direct", [({"OVHIP_GEMM_NT_MIN_MB": "0"}, [False, False], [False, False]),
                                                 ({"OVHIP_GEMM_NT_MIN_MB": "64"}, [True, False], [True, False]),
                                                 ({"OVHIP_GEMM_GELU_LDS": "1"}, [True, True], [False, False]),
                                                 ({"OVHIP_GEMM_GELU_LDS": "0", "OVHIP_GEMM_NT_MIN_MB": "0"}, [False, False], [True, True])])
def test_store_policy_switches(env, st_plain, direct):
    """OVHIP_GEMM_NT_MIN_MB moves the streaming threshold (64 MiB: 8191 | 8192 rows of 4096 columns), OVHIP_GEMM_GELU_LDS forces the
    folded GELU's form whatever the store policy."""
    got = ask_child(env, [((8192 - 1, 4096, 192, 1), {"fold": True}), ((8192, 4096, 192, 1), {"fold": True})])
    assert [r.st_plain for r in got] == st_plain and [r.direct for r in got] == direct
    assert all(r.kernel == "persistent" and r.fold for r in got)
