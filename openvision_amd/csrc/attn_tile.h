// attn_tile.h — the tile steps the attention kernels share (attention.hip, attention_bwd.hip), stated once.
//
// A tile is one f32x16 accumulator of v_mfma_f32_32x32x16_bf16 holding S^T (or P^T, dS^T, ...): lane (r, h2) = (lane & 31, lane >> 5)
// owns column r and, in register i, row (i & 3) + 8 (i >> 2) + 4 h2, so a row statistic of the softmax is lane-local plus one exchange of the two lane
// halves, and the accumulator packed pairwise to bf16 IS the B operand of the next product (pack_p).
//   forward : [mask_tail] -> tile_max -> half_max -> OV_ATTN_RESCALE -> exp_rows (attention.hip) -> pack_p -> read_v / tr_wait -> pv_mma
//   lone key: lone_dot, lone_sum -> OV_ATTN_RESCALE -> lone_weight, count_once -> vrow_piece, fold4    (a last tile of one key, on the VALU)
//   backward: pack_p, tr_join, OV_ATTN_TILE_MMA, swap_halves
// A change to anything here changes every kernel that calls it: `python tools/kernel_resources.py attention.hip --against REV` (and
// attention_bwd.hip) compares each kernel's ISA with REV's.  The FORM of a helper (function, template, macro) is the one that kept
// the ISA of every caller when it was extracted, and each definition says what the other forms did.  As a rule: what a kernel had as
// a lambda or function survives as a function, what it had as inline statements on its accumulators only as a macro or a by-value
// helper -- a function that takes an accumulator or an array by reference gave a different schedule or register assignment.
#pragma once
#include "common.h"

namespace attn {

// ---- the two lane halves ------------------------------------------------------------------------------------------------------------
// (lower half's dword of a, upper half's dword of b exchanged: v_permlane32_swap)
__device__ __forceinline__ u32x2_t half_swap(unsigned a, unsigned b) { return __builtin_amdgcn_permlane32_swap(a, b, false, false); }
// a lane's row statistic joined with lane ^ 32's: the maximum, scaled to log2 units, and the sum
__device__ __forceinline__ float half_max(float mx, float scale_log2) {
    const u32x2_t sw = half_swap(__float_as_uint(mx), __float_as_uint(mx));
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * scale_log2;
}
__device__ __forceinline__ float half_sum(float x) {
    const u32x2_t sw = half_swap(__float_as_uint(x), __float_as_uint(x));
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}
// lane ^ 32's value (the backward's form: x + swap_halves(x))
__device__ __forceinline__ float swap_halves(float v) { return __shfl_xor(v, 32, 64); }

// ---- row maximum of a score tile ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float max3_asm(float x, float y, float z) {       // no canonicalising v_max in front
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(x), "v"(y), "v"(z));
    return d;
}
// tile_max reads the accumulator from inline asm (v_max3): the wait states an MFMA result needs before a VALU read (passes + 3: 11
// for the 8-pass 32x32x16) are not inserted in front of inline asm.  Where no other instruction separates the score MFMAs from this
// call -- a full tile, for which the caller's tail mask reads nothing: the single-tile step of attn_fwd_hd64_persist, every step of
// attn_fwd_generic, the last step of an even tile count in the DEEP persistent form -- the CALLER puts an `s_nop 15` (`s_nop 7` where
// one tile's maximum sits in between) naming the accumulator "+v" in front.  (In the pair loop a dozen LDS reads and the other
// tile's maximum sit in between.)  Read too early the maximum is some older value: harmless for the softmax -- any shift m gives the
// same result up to rounding -- but the output then differs in the last bit from run to run (seen in an experiment of round 2 with this
// very pattern).  tests/test_build_scratch.py scans the generated ISA for it.
__device__ __forceinline__ float tile_max(const f32x16_t& sc) {
    const float mx = max3_asm(max3_asm(sc[0], sc[1], sc[2]), max3_asm(sc[3], sc[4], sc[5]), max3_asm(sc[6], sc[7], sc[8]));
    return max3_asm(mx, max3_asm(sc[9], sc[10], sc[11]), max3_asm(max3_asm(sc[12], sc[13], sc[14]), sc[15], sc[15]));
}

// Keys at or past `limit` score -inf (P = 0): the last tile of a sequence, kt = the tile's index.  Nothing to do (wave-uniform) for a
// tile that ends below the limit.  OV_ATTN_MASK_TAIL2 takes two consecutive tiles, kt and kt + 1, under one test.
// Stated as a macro and wrapped in a function: the ISA of a caller is kept only by the form it had -- a function (then a lambda) in
// attn_fwd_hd64_persist, inline statements in the other two kernels.
#define OV_ATTN_MASK_(kt, h2, limit, NT, BODY)                                                    \
    if ((kt) * 32 + 32 * (NT) > (limit)) {                                                        \
        _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) {                                       \
            const int key = (kt) * 32 + (i_ & 3) + 8 * (i_ >> 2) + 4 * (h2);                      \
            BODY                                                                                  \
        }                                                                                         \
    }
#define OV_ATTN_MASK_TAIL(sc, kt, h2, limit) OV_ATTN_MASK_(kt, h2, limit, 1, if (key >= (limit)) (sc)[i_] = -INFINITY;)
#define OV_ATTN_MASK_TAIL2(sa, sb, kt, h2, limit) \
    OV_ATTN_MASK_(kt, h2, limit, 2, if (key >= (limit)) (sa)[i_] = -INFINITY; if (key + 32 >= (limit)) (sb)[i_] = -INFINITY;)
__device__ __forceinline__ void mask_tail(f32x16_t& sc, int kt, int h2, int limit) { OV_ATTN_MASK_TAIL(sc, kt, h2, limit) }

// ---- lazy rescale -------------------------------------------------------------------------------------------------------------------
// The running maximum m moves, and the accumulators are rescaled, only when some row's tile maximum exceeds m by more than 8 (P stays
// below 2^8: no overflow in bf16 or the fp32 sums); otherwise the tile is folded in against the old m.
// MASK (prefix-causal): each row decides by its own scores alone (alpha = 1 exactly otherwise), so that keys a row cannot see -- which
// move the maxima of the rows below it in the tile -- leave its result bitwise unchanged.
// A macro: as a forceinline function (by reference, or returning the flag) every head_dim 64 kernel came out different.
#define OV_ATTN_RESCALE_(MASK, mx, m, lsum, SCALE_O)                                       \
    if ((MASK) ? __any((mx) - (m) > 8.0f) : !__all((mx) - (m) <= 8.0f)) {                  \
        const float mn = (!(MASK) || (mx) - (m) > 8.0f) ? fmaxf(m, mx) : (m);              \
        const float alpha = __builtin_amdgcn_exp2f((m) - mn);                              \
        (m) = mn;                                                                          \
        (lsum) *= alpha;                                                                   \
        SCALE_O                                                                            \
    }
// all rows, the two d-halves of head_dim 64
#define OV_ATTN_RESCALE(mx, m, lsum, o0, o1) \
    OV_ATTN_RESCALE_(false, mx, m, lsum, _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) { (o0)[i_] *= alpha; (o1)[i_] *= alpha; })
// per row under MASK, DT accumulators o[DT]
#define OV_ATTN_RESCALE_ROWS(MASK, mx, m, lsum, o, DT) \
    OV_ATTN_RESCALE_(MASK, mx, m, lsum, _Pragma("unroll") for (int t_ = 0; t_ < (DT); ++t_) _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) (o)[t_][i_] *= alpha;)

// ---- P tile -> bf16 B operand; fragment join ----------------------------------------------------------------------------------------
// rows 16 st .. 16 st + 15 of the tile (registers 8 st .. 8 st + 7), rounded pairwise to bf16
__device__ __forceinline__ bf16x8_t pack_p(const f32x16_t& sc, int st) {
    const u32x4_t w = {pack_bf16x2(sc[8 * st + 0], sc[8 * st + 1]), pack_bf16x2(sc[8 * st + 2], sc[8 * st + 3]),
                       pack_bf16x2(sc[8 * st + 4], sc[8 * st + 5]), pack_bf16x2(sc[8 * st + 6], sc[8 * st + 7])};
    return __builtin_bit_cast(bf16x8_t, w);
}
__device__ __forceinline__ bf16x8_t tr_join(u32x2_t a, u32x2_t b) {      // two ds_read_b64_tr_b16 results = one A-operand fragment
    const u32x4_t w = {a[0], a[1], b[0], b[1]};
    return __builtin_bit_cast(bf16x8_t, w);
}

// ---- V fragments of one key tile and the P.V products -------------------------------------------------------------------------------
// Transposing LDS reads issued from inline asm: hipcc treats the ds_read_tr builtin as possibly aliasing the LDS-DMA
// (global_load_lds) writes of the NEXT head and would drain them with vmcnt(0) before every V read, serialising the
// prefetch.  The asm forms are invisible to its memory model; completion is enforced by tr_wait(), which names every
// destination "+v" (cdna guide 5.7 form ii) so no consumer can be scheduled above the lgkmcnt wait.
template <int OFF>
__device__ __forceinline__ u32x2_t tr_read_off(unsigned addr) {
    u32x2_t v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
__device__ __forceinline__ void tr_wait(u32x2_t (&t)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]));
}
// the eight reads of the key tile at byte BASE (2048 per tile) of the V image: va0 / va1 = this lane's address in d-half 0 / 1; keys
// 0-7 | 8-15 | 16-23 | 24-31 of the tile are 512 bytes apart.  v[2 k], v[2 k + 1] join to fragment k of pv_mma.
template <int BASE>
__device__ __forceinline__ void read_v(u32x2_t (&v)[8], unsigned va0, unsigned va1) {
    v[0] = tr_read_off<BASE>(va0);        v[1] = tr_read_off<BASE + 512>(va0);
    v[2] = tr_read_off<BASE>(va1);        v[3] = tr_read_off<BASE + 512>(va1);
    v[4] = tr_read_off<BASE + 1024>(va0); v[5] = tr_read_off<BASE + 1536>(va0);
    v[6] = tr_read_off<BASE + 1024>(va1); v[7] = tr_read_off<BASE + 1536>(va1);
}
// o0 / o1 (the two 32-wide d slices) += X^T . T for one 32-row tile: f0..f3 = X^T fragments (slice 0, rows 0-15), (slice 1, rows
// 0-15), (slice 0, rows 16-31), (slice 1, rows 16-31); T packed as p0 (rows 0-15) / p1 (rows 16-31).  A macro for the resident
// backward (through a function its accumulators traded registers); the forward kernels take it through pv_mma.
#define OV_ATTN_TILE_MMA(f0, f1, f2, f3, p0, p1, o0, o1)                  \
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0, p0, o0, 0, 0, 0);    \
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f1, p0, o1, 0, 0, 0);    \
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f2, p1, o0, 0, 0, 0);    \
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f3, p1, o1, 0, 0, 0);
// O^T += V^T . P^T with the fragments read_v fetched (behind their tr_wait)
__device__ __forceinline__ void pv_mma(const u32x2_t (&v)[8], bf16x8_t p0, bf16x8_t p1, f32x16_t& o0, f32x16_t& o1) {
    OV_ATTN_TILE_MMA(tr_join(v[0], v[1]), tr_join(v[2], v[3]), tr_join(v[4], v[5]), tr_join(v[6], v[7]), p0, p1, o0, o1)
}

// ---- a last key tile that holds ONE key, on the VALU --------------------------------------------------------------------------------
// q.k of this lane's query with the key, over this lane's d range: per k-step st the caller hands lone_dot the Q fragment and the
// key's row-major K fragment of that step (wherever its kernel keeps it: fetching them all ahead of the loop changed the streaming and
// generic kernels' schedule), 4 v_dot2 each into two partial sums; lone_sum adds those and the halves of d across lane ^ 32.
// Inline asm: hipcc's lowering of the fdot2 builtin on dwords extracted from the fragments picked dword 0 of every fragment for all
// four products (checked in the ISA).
template <class KF>
__device__ __forceinline__ void lone_dot(float& s0, float& s1, bf16x8_t qf, KF kf) {
    const u32x4_t kq = __builtin_bit_cast(u32x4_t, kf), qq = __builtin_bit_cast(u32x4_t, qf);
    asm("v_dot2c_f32_bf16 %0, %1, %2" : "+v"(s0) : "v"(qq[0]), "v"(kq[0]));
    asm("v_dot2c_f32_bf16 %0, %1, %2" : "+v"(s1) : "v"(qq[1]), "v"(kq[1]));
    asm("v_dot2c_f32_bf16 %0, %1, %2" : "+v"(s0) : "v"(qq[2]), "v"(kq[2]));
    asm("v_dot2c_f32_bf16 %0, %1, %2" : "+v"(s1) : "v"(qq[3]), "v"(kq[3]));
}
__device__ __forceinline__ float lone_sum(float s0, float s1) {
    asm("s_nop 2" : "+v"(s0), "+v"(s1));      // DOT result -> ordinary VALU read: 3 wait states the assembler does not insert inside inline asm
    return half_sum(s0 + s1);                 // this lane's half of d; the other half sits in lane ^ 32
}
// the key's weight against the (rescaled) running maximum, and its share of this lane's row sum: the halves' sums are added at the
// end, so the key is counted in the lower half only.  (By value: with lsum by reference the persistent kernels came out different.)
__device__ __forceinline__ float lone_weight(float mx, float m) { return __builtin_amdgcn_exp2f(mx - m); }
__device__ __forceinline__ float count_once(float pk, int h2) { return h2 ? 0.f : pk; }
// o += pk * (the key's V row, one 32-wide d slice): o[4 g + e] holds d = 8 g + 4 h2 + e, so vrow = the row's slice + 8 h2 bytes and a
// lane takes four 8-byte pieces 16 bytes apart (vrow_piece); fold4 folds piece g in.  The loops over g stay with the callers, whose
// schedules differ: the persistent kernel reads d-half 0 ahead of the rescale and d-half 1 into the same registers behind a
// sched_barrier, the streaming kernel walks both d-halves piece by piece.  (Helpers that take the accumulator and the pieces by
// reference for a whole slice changed the persistent and streaming kernels' ISA; these by-value forms keep it.)
__device__ __forceinline__ u32x2_t vrow_piece(const char* vrow, int g) { return *(const u32x2_t*)(vrow + g * 16); }
__device__ __forceinline__ void fold4(f32x16_t& o, int g, float pk, u32x2_t v) {
    o[4 * g + 0] = fmaf(pk, bf16lo_to_f32(v[0]), o[4 * g + 0]);
    o[4 * g + 1] = fmaf(pk, bf16hi_to_f32(v[0]), o[4 * g + 1]);
    o[4 * g + 2] = fmaf(pk, bf16lo_to_f32(v[1]), o[4 * g + 2]);
    o[4 * g + 3] = fmaf(pk, bf16hi_to_f32(v[1]), o[4 * g + 3]);
}

}  // namespace attn
