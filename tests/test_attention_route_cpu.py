"""CPU: what the attention launchers decide, asked of the library itself (ov_attention_route at 256 CUs; it launches nothing and needs
no device).

Part 1 pins, in a literal table, the forward and backward kernel form of every attention shape the GPU tests run (the shape lists of
test_gpu_attention_edges.py, test_gpu_attention_bwd_edges.py, test_gpu_prefix_attention.py, the fp8out cases of
test_gpu_fp8_routes.py and the attention tests of test_gpu_ops.py): if the launchers' rules drift, this fails here, before those
tests quietly cover another kernel.
Part 2 walks each rule of attention_route.h at its edge, with pairs of calls that differ in the one condition named.  The expected
values are read off the rules as DESIGN.md section 4 states them (a head of up to 320 padded keys stays resident; 160 KiB of LDS and 8
or 12 waves per CU; 2 GiB of rows; the resident backward up to L = 288; 256-row backward chunks), not off what the library returns."""
import json

import pytest

import hipops as H
import test_gpu_attention_bwd_edges as BE
import test_gpu_attention_edges as FE
import test_gpu_fp8_routes as F8
import test_gpu_ops as OPS
import test_gpu_prefix_attention as PT
from hipops import attn_route
from ranks import run_child

CUS = 256
KIB = 1024


def r256(B, L, Hh, hd=64, cus=CUS, **kw):
    return attn_route(B, L, Hh, hd, cus=cus, **kw)


def refused(B, L, Hh, hd=64, prefix=-1, out8=0, lse=0, ld_qkv=0, ld_out=0, route=True):
    out = H._lib.AttentionRoute()
    return H._lib.load().ov_attention_route(B, L, Hh, hd, ld_qkv, ld_out, prefix, out8, lse, CUS, H.C.addressof(out) if route else None)


def params(test):
    return [m for m in test.pytestmark if m.name == "parametrize"][0].args[1]


# ---- part 1: the tests' own shapes.  The kernel form depends on (L, head_dim) only (B and H size the grid: part 2), so the table is
# keyed by them: (forward form, waves per workgroup, backward form), under the names hipops.attn_route gives the forms.

P, S, GR, GC = "persistent", "streaming", "generic resident", "generic chunked"
RES, S2, S3 = "resident", "stream<2>", "stream<3>"
FORMS = {
    (1, 64): (P, 1, RES), (5, 64): (P, 1, RES), (31, 64): (P, 1, RES), (32, 64): (P, 1, RES), (33, 64): (P, 2, RES), (65, 64): (P, 3, RES),
    (80, 64): (P, 3, RES), (97, 64): (P, 4, RES), (101, 64): (P, 4, RES), (128, 64): (P, 4, RES), (129, 64): (P, 5, RES),
    (193, 64): (P, 7, RES), (225, 64): (P, 8, RES), (256, 64): (P, 8, RES), (257, 64): (P, 9, RES), (288, 64): (P, 9, RES),
    (289, 64): (P, 10, S2), (321, 64): (S, 8, S2), (384, 64): (S, 8, S2), (385, 64): (S, 8, S2), (449, 64): (S, 8, S2),
    (463, 64): (S, 8, S2), (481, 64): (S, 8, S2), (513, 64): (S, 8, S2), (577, 64): (S, 8, S2), (705, 64): (S, 8, S2),
    (1000, 64): (S, 8, S2), (2304, 64): (S, 8, S2), (2305, 64): (S, 8, S2),
    (257, 8): (GR, 9, S2), (577, 8): (GC, 8, S2), (65, 32): (GR, 3, S2), (257, 32): (GR, 9, S2), (577, 32): (GC, 8, S2),
    (513, 48): (GC, 8, S2), (257, 56): (GR, 9, S2), (577, 56): (GC, 8, S2),
    (40, 72): (GR, 2, S3), (80, 72): (GR, 3, S3), (101, 72): (GR, 4, S3), (207, 72): (GR, 7, S3), (257, 72): (GR, 9, S3),
    (321, 72): (GC, 8, S3), (577, 72): (GC, 8, S3), (730, 72): (GC, 8, S3), (737, 72): (GC, 8, S3), (1025, 72): (GC, 8, S3),
    (257, 80): (GR, 9, S3), (300, 80): (GR, 10, S3), (321, 80): (GC, 8, S3), (463, 80): (GC, 8, S3), (513, 80): (GC, 8, S3),
    (577, 80): (GC, 8, S3), (768, 80): (GC, 8, S3), (257, 88): (GR, 9, S3), (577, 88): (GC, 8, S3), (257, 96): (GR, 9, S3),
    (577, 96): (GC, 8, S3), (769, 96): (GC, 8, S3),
}
# the masked calls, (L, head_dim, prefix): always the generic forward kernel's MASK form and the masked streaming pair
MASKED_FORMS = {
    (1, 64, 0): (GR, 1, S2), (33, 64, 32): (GR, 2, S2), (65, 64, 31): (GR, 3, S2), (65, 64, 33): (GR, 3, S2), (80, 64, 0): (GR, 3, S2),
    (257, 64, 1): (GR, 9, S2), (257, 64, 256): (GR, 9, S2), (307, 64, 179): (GR, 10, S2), (463, 64, 335): (GC, 8, S2),
    (513, 64, 256): (GC, 8, S2), (513, 64, 257): (GC, 8, S2), (2305, 64, 2000): (GC, 8, S2),
    (207, 72, 79): (GR, 7, S3), (463, 72, 335): (GC, 8, S3), (207, 80, 79): (GR, 7, S3), (463, 80, 335): (GC, 8, S3), (513, 80, 512): (GC, 8, S3),
}


def unmasked_shapes():
    hd64 = lambda shapes: [(B, L, Hh, 64) for (B, L, Hh, *_) in shapes]
    return (FE.FWD_SHAPES + BE.BWD_SHAPES + H.LONE_SPIKED + params(FE.test_attention_padded_row_pitches) + [(2, 257, 2, 64)]   # huge pitch
            + [s[:4] for s in params(BE.test_attention_backward_pitches_and_neighbours) if s[4] is None]
            + params(BE.test_attention_backward_saved_lse_within_bound) + params(PT.test_prefix_equal_L_is_bitwise_the_unmasked_call)
            + hd64(params(F8.test_attention_fp8out_amax_next_and_pitch)) + hd64(params(OPS.test_attention))
            + hd64(params(OPS.test_attention_backward_vs_oracle)) + hd64(params(OPS.test_attention_keeps_the_row_lse_for_the_backward))
            + hd64(params(OPS.test_attention_fp8_output)) + params(OPS.test_attention_generic_head_dim)
            + params(OPS.test_attention_backward_other_head_dims)
            + [(1, L, 1, 64) for L, _ in params(OPS.test_attention_online_softmax_rescale_branch)])


def masked_shapes():
    return (PT.SHAPES + BE.PREFIX_BWD_SHAPES + params(PT.test_invisible_keys_do_not_touch_a_row)
            + params(PT.test_backward_zero_structure_and_determinism) + [(2, 307, 2, 64, 179)])            # the padded-pitch cases


def test_the_gpu_tests_shapes_reach_the_kernels_they_name():
    shapes = unmasked_shapes()
    assert {(L, hd) for (_, L, _, hd) in shapes} == set(FORMS), "the GPU tests' attention shapes changed: extend FORMS"
    for (B, L, Hh, hd) in shapes:
        r = r256(B, L, Hh, hd)
        assert (r.form, r.waves, r.bwd_form) == FORMS[L, hd], (B, L, Hh, hd, vars(r))
        assert r.keep_lse == (FORMS[L, hd][2] == RES) and (r.bwd_workspace_bytes == 0) == r.keep_lse
    for shape, form in FE.FWD_FORMS.items():                        # the GPU tests' own expectations, here at 256 CUs
        assert r256(*shape).form == form == FORMS[shape[1], shape[3]][0]
    for shape, form in BE.BWD_FORMS.items():
        assert r256(*shape).bwd_form == form == FORMS[shape[1], shape[3]][2]
    assert [r256(*s).form for s in H.LONE_SPIKED] == FE.LONE_FORMS


def test_the_pitched_and_saved_cases_reach_the_kernels_they_name():
    for (B, L, Hh, hd), form in FE.PITCH_FORMS.items():
        D = Hh * hd
        assert r256(B, L, Hh, hd, ld_qkv=3 * D + 64, ld_out=D + 64).form == form == FORMS[L, hd][0]
    for (B, L, Hh, hd, prefix), form in BE.PITCH_FORMS.items():
        assert r256(B, L, Hh, hd, prefix=prefix).bwd_form == form
    assert r256(2, 257, 2, 64).form == P and r256(2, 257, 2, 64, ld_qkv=1 << 22).form == GR                      # the huge row pitch
    for (B, L, Hh, hd) in params(BE.test_attention_backward_saved_lse_within_bound) + [
            (B, L, Hh, 64) for (B, L, Hh) in params(OPS.test_attention_keeps_the_row_lse_for_the_backward)]:
        r = r256(B, L, Hh, hd, lse=True)
        assert (r.form, r.lse, r.bwd_form, r.keep_lse) == (P, True, "resident saved", True), (B, L, Hh, hd)
    assert refused(2, 300, 1, lse=1) == -2                         # test_attention_keeps_the_row_lse_for_the_backward's refused call


def test_the_fp8out_cases_reach_the_kernels_they_name():
    names = {"persistent, <= 8 waves": (P, True), "persistent, 9+ waves": (P, False), "streaming": (S, False)}
    for (B, L, Hh, kernel, padded_rows) in params(F8.test_attention_fp8out_amax_next_and_pitch):
        r = r256(B, L, Hh, out8=True)
        assert (r.form, r.deep) == names[kernel] and r.out8 and F8.attn_kernel(B, L, Hh, CUS) == (kernel, padded_rows)
    for (B, L, Hh) in params(OPS.test_attention_fp8_output):       # "the persistent (9-wave and <= 8-wave) and streaming kernels"
        r = r256(B, L, Hh, out8=True)
        assert (r.form, r.waves, r.out8) == FORMS[L, 64][:2] + (True,)
    assert {r256(B, L, Hh, out8=True).deep for (B, L, Hh) in params(OPS.test_attention_fp8_output) if FORMS[L, 64][0] == P} == {True, False}


def test_the_prefix_tests_shapes_reach_the_masked_forms():
    shapes = masked_shapes()
    assert {(L, hd, p) for (_, L, _, hd, p) in shapes} == set(MASKED_FORMS), "the prefix tests' shapes changed: extend MASKED_FORMS"
    for (B, L, Hh, hd, p) in shapes:
        r = PT.masked_route(B, L, Hh, hd, p, CUS)                   # the GPU tests' own assertions, here at 256 CUs
        form, waves, bwd = MASKED_FORMS[L, hd, p]
        assert (r.form, r.waves, r.bwd_form) == (form + " mask", waves, bwd + " mask"), (B, L, Hh, hd, p, vars(r))
    for (B, L, Hh, hd) in params(PT.test_prefix_equal_L_is_bitwise_the_unmasked_call):
        assert vars(r256(B, L, Hh, hd, prefix=L)) == vars(r256(B, L, Hh, hd))


# ---- part 2: each rule at its edge (256 CUs unless said otherwise)


def fwd(r):
    return r.form, r.kc, r.waves, r.grid, r.lds_bytes


def test_anchors():
    r = r256(4, 257, 16)
    assert fwd(r) == (P, 288, 9, (64, 1), 147456) and not r.deep              # 9 waves, 1 workgroup per CU, grid min(64, cus)
    r = r256(2, 65, 3)
    assert fwd(r) == (P, 96, 3, (6, 1), 49152) and r.deep                     # 2 workgroups per CU, grid B H
    assert fwd(r256(1, 321, 2)) == (S, 64, 8, (16, 1), 64 * KIB)              # one round of 8 XCDs x 2 blocks of 256 queries
    assert fwd(r256(1, 321, 2, 72)) == (GC, 256, 8, (2, 2), 98304)
    assert fwd(r256(1, 257, 2, 8)) == (GR, 288, 9, (2, 1), 110592)
    r = r256(1, 288, 1)
    assert (r.bwd_form, r.bwd_kc, r.bwd_waves, r.bwd_grid, r.bwd_lds_bytes, r.bwd_workspace_bytes) == (RES, 288, 9, 1, 149760, 0)
    r = r256(1, 289, 2)
    assert (r.bwd_form, r.ndh, r.bwd_kc, r.bwd_waves, r.bwd_grid, r.bwd_lds_bytes) == (S2, 2, 256, 8, 2 * 2, 67584)
    assert r.bwd_workspace_bytes == 2 * 2 * 512 * 4                           # lse and delta rows of 2 heads, 2 chunks of 256 rows


def test_a_head_of_up_to_320_padded_keys_stays_resident():
    a, b = r256(2, 320, 3), r256(2, 321, 3)                                   # hd 64: persistent | streaming
    assert fwd(a) == (P, 320, 10, (6, 1), 160 * KIB) and a.resident and not a.deep
    assert fwd(b) == (S, 64, 8, (8 * 2, 1), 64 * KIB) and not b.resident      # 6 heads -> one round of 8; 11 query tiles -> 2 blocks
    a, b = r256(2, 320, 3, 72), r256(2, 321, 3, 72)                           # hd 72: the generic kernel, resident | in 256-key chunks
    assert fwd(a) == (GR, 320, 10, (6, 1), 320 * 96 * 4) and a.resident and a.hdp == 96
    assert fwd(b) == (GC, 256, 8, (6, 2), 256 * 96 * 4) and not b.resident
    assert r256(2, 289, 3).form == P and r256(2, 289, 3).kc == 320            # padded L decides: 289 .. 320 are ten tiles
    a, b = r256(2, 320, 3, prefix=7), r256(2, 321, 3, prefix=7)               # the masked form, hd 64 at its own width
    assert fwd(a) == (GR + " mask", 320, 10, (6, 1), 320 * 64 * 4) and fwd(b) == (GC + " mask", 256, 8, (6, 2), 256 * 64 * 4)
    assert r256(1, 2305, 1).grid == (8 * 10, 1) and r256(1, 2305, 9).grid == (16 * 10, 1)          # 73 query tiles: 10 blocks; 9 heads: 2 rounds


def test_deep_up_to_eight_waves():
    a, b = r256(1, 256, 1), r256(1, 257, 1)
    assert (a.deep, a.waves, a.lds_bytes) == (True, 8, 128 * KIB) and (b.deep, b.waves, b.lds_bytes) == (False, 9, 144 * KIB)
    assert not r256(1, 256, 1, 72).deep and not r256(1, 2305, 1).deep         # the persistent kernel's flag only
    for kw in ({"out8": True}, {"lse": True}):                                 # all six instantiations
        assert r256(1, 256, 1, **kw).deep and not r256(1, 257, 1, **kw).deep


def test_head_dim_64_takes_the_tuned_kernels():
    assert r256(2, 100, 2, 64).form == P and r256(2, 100, 2, 56).form == GR and r256(2, 100, 2, 72).form == GR
    assert r256(2, 400, 2, 64).form == S and r256(2, 400, 2, 56).form == GC
    assert (r256(2, 100, 2, 64).hdp, r256(2, 100, 2, 56).hdp, r256(2, 100, 2, 56, prefix=5).hdp, r256(2, 100, 2, 64, prefix=5).hdp) == (0, 96, 96, 64)


def test_two_gib_of_rows_leave_the_persistent_kernel():
    """L ld 2 B < 2^31 - 1 for both pitches: at L = 256 that is ld <= 4194303, so 4194296 | 4194304 among the multiples of 8."""
    assert 256 * 4194296 * 2 < 2 ** 31 - 1 <= 256 * 4194304 * 2
    assert r256(1, 256, 2, ld_qkv=4194296).form == P and r256(1, 256, 2, ld_qkv=4194304).form == GR
    assert r256(1, 256, 2, ld_out=4194296).form == P and r256(1, 256, 2, ld_out=4194304).form == GR
    assert r256(1, 256, 2, ld_qkv=4194296, ld_out=4194296).form == P
    assert r256(1, 2305, 2, ld_qkv=4194304).form == S                         # the streaming kernel's offsets are 64-bit
    assert refused(1, 256, 2, ld_qkv=4194304, out8=1) == refused(1, 256, 2, ld_out=4194304, lse=1) == -2          # no such generic form


def test_workgroups_per_cu_by_lds_and_by_waves():
    """min(160 KiB / LDS, (8 or 12 waves) / waves), at least 1; read from the grid of 4096 heads on 256 CUs."""
    for L, lds, per_cu in ((32, 16 * KIB, 8),          # 10 by LDS, 8 by waves
                           (64, 32 * KIB, 4),          # 5, 4
                           (96, 48 * KIB, 2),          # 3, 2
                           (128, 64 * KIB, 2),         # 2, 2
                           (160, 80 * KIB, 1),         # 2, 1
                           (256, 128 * KIB, 1),        # 1, 1
                           (288, 144 * KIB, 1),        # 1, 1 (12 / 9)
                           (320, 160 * KIB, 1)):       # 1, 1
        r = r256(256, L, 16)
        assert (r.lds_bytes, r.grid) == (lds, (CUS * per_cu, 1)), (L, r.lds_bytes, r.grid)


def test_grid_capped_by_the_cus_or_by_the_heads():
    assert r256(4, 257, 16).grid == (64, 1) and r256(32, 257, 16).grid == (256, 1)
    assert r256(16, 257, 16).grid == (256, 1) and r256(16, 257, 16, cus=304).grid == (256, 1) and r256(19, 257, 16, cus=304).grid == (304, 1)
    assert r256(100, 65, 5).grid == (500, 1) and r256(103, 65, 5).grid == (512, 1)           # 2 per CU: up to 512
    assert r256(32, 257, 16, 80).grid == (512, 1) and r256(32, 577, 16, 80).grid == (512, 3)  # the generic kernel: one column per head


def test_resident_backward_and_kept_lse_up_to_288():
    a, b = r256(2, 288, 3), r256(2, 289, 3)
    assert (a.bwd_form, a.keep_lse, a.bwd_grid, a.bwd_workspace_bytes) == (RES, True, 6, 0)
    assert (b.bwd_form, b.keep_lse, b.bwd_grid, b.bwd_workspace_bytes) == (S2, False, 6 * 2, 2 * 6 * 512 * 4)
    assert r256(2, 288, 3, lse=True).bwd_form == "resident saved" and r256(2, 288, 3, lse=True).lse and refused(2, 289, 3, lse=1) == -2
    assert r256(2, 288, 3, 72).bwd_form == S3 and not r256(2, 288, 3, 72).keep_lse and refused(2, 288, 3, 72, lse=1) == -2
    a = r256(2, 33, 3)
    assert (a.bwd_kc, a.bwd_waves, a.bwd_lds_bytes) == (64, 2, 4 * 64 * 128 + 2 * 64 * 4)
    assert r256(2, 256, 3, 56).bwd_grid == 6 and r256(2, 257, 3, 56).bwd_grid == 12               # 256-row chunks
    lib = H._lib.load()
    for shape in ((2, 288, 3, 64), (2, 289, 3, 64), (2, 288, 3, 72), (3, 2305, 5, 80)):
        r = r256(*shape)
        assert lib.ov_attention_backward_workspace_bytes(*shape) == r.bwd_workspace_bytes
        assert lib.ov_attention_prefix_backward_workspace_bytes(*shape) == r256(*shape, prefix=0).bwd_workspace_bytes > 0


def test_three_d_blocks_above_head_dim_64():
    a, b = r256(1, 289, 2, 64), r256(1, 289, 2, 72)
    assert (a.ndh, a.bwd_lds_bytes) == (2, 2 * 2 * 16 * KIB + 2 * KIB) and (b.ndh, b.bwd_lds_bytes) == (3, 2 * 3 * 16 * KIB + 2 * KIB)
    assert r256(1, 100, 2, 8).ndh == 2 and r256(1, 100, 2, 96).ndh == 3 and r256(1, 100, 2, 64).ndh == 0


def test_prefix_equal_to_l_is_the_unmasked_route():
    a, b = r256(2, 100, 3, prefix=99), r256(2, 100, 3, prefix=100)
    assert fwd(a) == (GR + " mask", 128, 4, (6, 1), 128 * 64 * 4) and (a.bwd_form, a.bwd_workspace_bytes, a.keep_lse) == (S2 + " mask", 2 * 6 * 256 * 4, False)
    assert fwd(b) == (P, 128, 4, (6, 1), 64 * KIB) and (b.bwd_form, b.bwd_workspace_bytes, b.keep_lse) == (RES, 0, True)
    assert vars(b) == vars(r256(2, 100, 3)) and r256(2, 100, 3, prefix=0).form == GR + " mask"
    assert refused(2, 100, 3, prefix=101) == -1
    assert refused(2, 100, 3, prefix=99, lse=1) == refused(2, 100, 3, prefix=99, out8=1) == -2 and refused(2, 100, 3, prefix=100, lse=1) == 0
    assert refused(65536, 100, 65536, prefix=99) == -2 and refused(65536, 321, 65536) == -2       # grids beyond 2^31 - 1 workgroups


def test_what_the_entry_points_refuse():
    assert refused(2, 100, 3, out8=1, lse=1) == -2                  # a kept lse beside an e4m3 output
    assert refused(2, 100, 3, 72, out8=1) == -2 and refused(2, 100, 3, 72, lse=1) == -2 and refused(2, 100, 3, out8=1) == 0
    assert refused(2, 100, 3, 12) == refused(2, 100, 3, 104) == refused(2, 100, 3, 0) == -2
    assert refused(0, 100, 3) == refused(2, 0, 3) == refused(2, 100, 0) == refused(2, 100, 3, route=False) == -1
    assert refused(2, 100, 3, ld_qkv=3 * 192 - 8) == refused(2, 100, 3, ld_out=196) == -1


# ---- the switch: read once per process, so each setting is asked in a child process (CPU only)

CHILD = ("import json; import hipops as H; print(json.dumps([H.attn_route(*s, cus=256).lone_valu for s in json.loads(sys.argv[1])]))")


@pytest.mark.parametrize("setting,hd64", [(None, 1), ("1", 1), ("0", 0)])
def test_lone_key_switch(setting, hd64):
    """OVHIP_ATTN_LONEKEY=0 turns the hd 64 kernels' VALU fold of a lone last key into a tile step; the generic kernel always folds."""
    out = run_child(CHILD, json.dumps(H.LONE_SPIKED), env={"OVHIP_ATTN_LONEKEY": setting}, timeout=120)
    assert json.loads(out.stdout.strip().splitlines()[-1]) == [hd64 if hd == 64 else 1 for (_, _, _, hd) in H.LONE_SPIKED]
