// gemm_tile.h — the steps the ping-pong GEMM kernels share (gemm.hip: gemm_bf16_pp, gemm_bf16_pp_tn, gemm_bf16_persist; gemm_fp8.hip:
// gemm_fp8_persist), stated once: the epilogue's element function, the tile geometry, the phase skeleton with its hazard rules, the
// persistent kernels' K-tile schedule and tile hand-over.  The skinny kernel shares the activation and the pack only.  The kernels keep what is theirs: the LDS image and stage_piece, the fragment
// reads, the MFMA type, the walk counter, stage_params, the epilogues' transposition and store tails, the diagnostics.
// A change to anything here changes every kernel that calls it: `python tools/kernel_resources.py gemm.hip --against REV` (and
// gemm_fp8.hip; gemm.hip once more with -DOVHIP_STAMPS=1) compares each kernel's ISA with REV's.  The FORM of a helper (function,
// by-value helper, lambda parameter, macro) is the one under which every caller kept the instructions it had when the step was
// extracted.
#pragma once
#include "common.h"

namespace gemm {

template <int V> struct IntC { static constexpr int value = V; };
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// ---- the epilogue's element function --------------------------------------------------------------------------------------------------
// A lane's quad: four consecutive n of one output row.  THE PROMISE THAT A ROW'S BITS DO NOT DEPEND ON WHICH KERNEL FORM COMPUTED IT
// (plain, persistent direct / LDS-transposed, skinny; tests: batch invariance, the route tests) RESTS ON THIS ONE FUNCTION: every bf16
// epilogue calls it, in packed fp32 (v_pk_*), the LN fold as two explicit FMAs -- rstd * (acc - mean * colsum) + cvec.
// (Macros: the same steps as functions -- activate<EPI>(v01, v23), pack_quad(v01, v23) -- changed the plain kernels' instructions.)
#define OV_GEMM_ACTIVATE(EPI, v01, v23)                                                           \
    do {                                                                                          \
        if (EPI == OV_EPI_BIAS_GELU_ERF) gelu_erf_f2x2(v01, v23);                                 \
        if (EPI == OV_EPI_BIAS_GELU_TANH) { v01 = gelu_tanh_f2(v01); v23 = gelu_tanh_f2(v23); }   \
    } while (0)
#define OV_GEMM_PACK_QUAD(v01, v23) u32x2_t{pack_bf16x2(v01[0], v01[1]), pack_bf16x2(v23[0], v23[1])}
// B, S: the quad's four bias values and (FOLD) column sums, indexable; MEAN, RSTD: the row's statistics (FOLD); PRE: PREOUT also takes
// the pre-activation pack (ov_gemm_keep; without PRE name OUT twice).  A macro: as a function -- quads by value, as vectors, through pointers, the result as a
// struct or through a pointer -- it changed the instructions of gemm_epilogue<GELU_ERF> or of the persistent kernels without the fold.
#define OV_GEMM_EPI_QUAD(EPI, PRE, ACC, B, FOLD, S, MEAN, RSTD, OUT, PREOUT)                      \
    do {                                                                                          \
        f32x2_t v01 = f32x2_t{(ACC)[0], (ACC)[1]};                                                \
        f32x2_t v23 = f32x2_t{(ACC)[2], (ACC)[3]};                                                \
        if (FOLD) {                                                                               \
            const f32x2_t nm = {-(MEAN), -(MEAN)}, rs = {(RSTD), (RSTD)};                         \
            v01 = __builtin_elementwise_fma(f32x2_t{(S)[0], (S)[1]}, nm, v01);                    \
            v23 = __builtin_elementwise_fma(f32x2_t{(S)[2], (S)[3]}, nm, v23);                    \
            v01 = __builtin_elementwise_fma(v01, rs, f32x2_t{(B)[0], (B)[1]});                    \
            v23 = __builtin_elementwise_fma(v23, rs, f32x2_t{(B)[2], (B)[3]});                    \
        } else {                                                                                  \
            v01 += f32x2_t{(B)[0], (B)[1]};                                                       \
            v23 += f32x2_t{(B)[2], (B)[3]};                                                       \
        }                                                                                         \
        if (PRE) PREOUT = OV_GEMM_PACK_QUAD(v01, v23);                                            \
        if (EPI == OV_EPI_BIAS_GELU_ERF) gelu_erf_f2x2(v01, v23);                                 \
        if (EPI == OV_EPI_BIAS_GELU_TANH) { v01 = gelu_tanh_f2(v01); v23 = gelu_tanh_f2(v23); }   \
        OUT = OV_GEMM_PACK_QUAD(v01, v23);                                                        \
    } while (0)

// ---- tile geometry --------------------------------------------------------------------------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs; XCD x takes the x-th of 8 consecutive runs of the linear (n fastest) tile list, so
// each XCD's L2 sees a contiguous run: the tiles resident on it share A row-panels and the whole of W.
struct Run { int start, count; };
// (The expressions are macros: the one-tile-per-workgroup kernels form their tile id `start + (bid >> 3)` from OV_GEMM_XCD_START in
// place -- through a function, xcd_run included, the sum's operands changed order.)
#define OV_GEMM_XCD_START(q8, r8, xcd) ((xcd) < (r8) ? (xcd) * ((q8) + 1) : (r8) * ((q8) + 1) + ((xcd) - (r8)) * (q8))
#define OV_GEMM_XCD_COUNT(q8, r8, xcd) ((q8) + ((xcd) < (r8) ? 1 : 0))
__host__ __device__ constexpr Run xcd_run(int nwg, int xcd) {
    const int q8 = nwg >> 3, r8 = nwg & 7;
    return Run{OV_GEMM_XCD_START(q8, r8, xcd), OV_GEMM_XCD_COUNT(q8, r8, xcd)};
}
constexpr bool xcd_runs_tile(int nwg) {         // the eight runs are consecutive and cover [0, nwg) exactly
    int next = 0;
    for (int x = 0; x < 8; ++x) {
        if (xcd_run(nwg, x).start != next || xcd_run(nwg, x).count < 0) return false;
        next += xcd_run(nwg, x).count;
    }
    return next == nwg;
}
static_assert(xcd_runs_tile(1) && xcd_runs_tile(7) && xcd_runs_tile(8) && xcd_runs_tile(9) && xcd_runs_tile(1028), "xcd_run");
constexpr int PIECE_BYTES = 256 * 64;          // bf16: one staged piece, 256 rows x 64 B = 16 KiB
// 16-B chunk c of row r of a piece is stored at chunk c ^ swz4(r) = c ^ f((r >> 2) & 3), f = {0, 2, 3, 1}: conflict-free for the
// 16x16x32 operand reads.  The DMA writes LDS lane-linearly, so the swizzle is applied to the per-lane SOURCE address.
__device__ __forceinline__ int swz4(int row) { return (0x78 >> (((row >> 2) & 3) * 2)) & 3; }

// Per-lane staging sources of a 256 x 256 bf16 tile: LDS chunk q = i*512 + tid of a piece holds row q >> 2, logical chunk
// (q & 3) ^ swz4(row); rows past M / N are clamped (they load a valid row and are never stored).  gemm_bf16_pp and gemm_bf16_persist
// each keep their statement of it: they order the same arithmetic differently (row by row / A rows, W rows, pointers), and either
// kernel changed its instructions under the other's order, as a function and as a macro.
struct TileSrc { const ov_bf16* a0; const ov_bf16* a1; const ov_bf16* w0; const ov_bf16* w1; };

// Fragment read addresses inside a K-half's piece pair [A][W]: A + i*1024 is A fragment row i, W + j*1024 W fragment column j.
// AROW / WCOL: first row / column of the wave's sub-tile inside the tile -- (wm * 128, wn * 64) for the 2 x 4 wave grid of 128 x 64
// sub-tiles, ((wave >> 1) * 64, (wave & 1) * 64) for the 4 x 2 grid of 64 x 64 of a HALF TILE (gemm_bf16_persist).  (A macro: as a
// function returning the pair it changed both callers.)
#define OV_GEMM_FRAG_LANES(A, W, LANE, AROW, WCOL)                                  \
    do {                                                                            \
        const int fr_ = (LANE) & 15, fq_ = (LANE) >> 4;                             \
        const int lsw_ = (fq_ ^ gemm::swz4(fr_)) << 4;                              \
        A = ((AROW) + fr_) * 64 + lsw_;                                             \
        W = gemm::PIECE_BYTES + ((WCOL) + fr_) * 64 + lsw_;                         \
    } while (0)

// ---- phase skeleton -------------------------------------------------------------------------------------------------------------------
// A K-tile is four phases; a phase is a LOAD segment (LDS fragment reads + one piece of a later K-tile by LDS-DMA + a COUNTED
// s_waitcnt vmcnt, never 0 in the steady state) and a COMPUTE segment (16 MFMAs at priority 1), each closed by a fence: a raw s_barrier
// the compiler may move nothing across.  Waves 4-7 (the lower 128 rows) run ONE barrier behind waves 0-3, so on every SIMD one wave is in
// its COMPUTE segment while its partner is in its LOAD segment: the matrix pipe sees back-to-back MFMA clusters instead of both waves
// stalling on LDS at once.
// Hazards (interval = span between two consecutive barriers; wave group 1 lags group 0 by one interval):
//   RAW  a piece issued in phase p of tile T is waited for (counted vmcnt) in phase 3 (p<2) or phase 1 of T+1 (p>=2),
//        and first read >= one barrier after EVERY wave has passed that wait;
//   WAR  a slot is re-staged >= 4 intervals after its last ds_read was issued (those reads are consumed by the
//        MFMAs of the reader's next COMPUTE segment, i.e. before its next barrier).
// The waits are counted because vmcnt retires in order: everything a wave has put into the vector-memory queue -- LDS-DMA, residual
// loads, stores, and a scratch reload if the compiler spills -- stands in one line, and a load issued behind stores waits for their
// write acknowledgements.  Hence also fresh_lane() (common.h): per-lane constants of a tile (staging rows, fragment addresses, the
// epilogue's columns) are rebuilt per tile from an opaque lane id; as invariants of the tile loop hipcc carried them through the main
// loop or spilled them, and a spill reload is a vector-memory operation the counts do not know about.
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void phase_fence() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
// the COMPUTE segment's bracket (the closing fence included)
template <class F>
__device__ __forceinline__ void compute_segment(F&& mfmas) {
    __builtin_amdgcn_s_setprio(1);
    mfmas();
    __builtin_amdgcn_s_setprio(0);
    phase_fence();
}
// (macros: as functions the branch round the barrier came out inverted in five of the seven kernel families)
#define OV_GEMM_STAGGER(wm) if ((wm) == 1) __builtin_amdgcn_s_barrier()      /* the lower wave group falls one interval behind */
#define OV_GEMM_REALIGN(wm) if ((wm) == 0) __builtin_amdgcn_s_barrier()      /* every wave is past its last COMPUTE segment */
// end of a kernel's prologue: the first K-tile(s) have landed for every wave
__device__ __forceinline__ void prologue_sync(int wm) {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    OV_GEMM_STAGGER(wm);
}
// the accumulator clear of the kernels that do not start a tile with FIRST products (a macro: by reference it changed them)
#define OV_GEMM_CLEAR_ACC(ACC)                                                                    \
    _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_)                                              \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)(ACC)[i_][j_] = f32x4_t{0.f, 0.f, 0.f, 0.f}
// The 16-MFMA bf16 tile product ACC[R0 + i][j] (+)= W fragment j x A fragment i (W as the MFMA A operand: a lane ends up with 4
// consecutive n of one m).  WF / AF are expressions in j_ / i_.  FIRST: a tile's first products start from a literal zero C operand --
// no 128 v_mov per tile to clear the accumulators.  (A macro: the accumulators are named in place.)
#define OV_GEMM_MMA16(ACC, R0, WF, AF, FIRST)                                                                                    \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                                             \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                                                         \
            if (FIRST) (ACC)[(R0) + i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WF, AF, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0); \
            else (ACC)[(R0) + i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WF, AF, (ACC)[(R0) + i_][j_], 0, 0, 0)

// ---- the persistent kernels' K-tile schedule and tile hand-over --------------------------------------------------------------------
// KIND selects, at compile time (the steady-state body carries no branch), what a K-tile stages into the other LDS buffer `nb` and
// which counted wait follows:
//   0: K-tile 0 of a tile -- K-tile 1 is already in flight (previous hand-over / prologue), nothing is staged; its wait at phase 3
//      leaves the previous epilogue's stores outstanding (a full drain when `strict`: first tile, or after an edge tile);
//   1: K-tile 1 -- stages K-tile 2 from `cur`, first wait at phase 3;     2: steady state -- stages the K-tile after next;
//   3: last K-tile -- stages K-tile 0 of the next tile from `nxt`, if any; otherwise it drains what is in flight.
// A piece issued in phase p is first read one (p < 2: two) K-tile phases after a counted wait that covers it (RAW above).  The table T
// carries what differs between the kernels:
//   wait_phases  bit p: phase p of a staging K-tile ends with vmcnt(4) (four pieces = 8 DMAs per K-tile, 2 per phase)
//   epi_stores   stores per wave of an epilogue: what K-tile 0's wait leaves in flight
//   any_wait     bit p: phase p can end with a wait at all
//   tail0/tail1  last K-tile of the last tile: the wait at phase 0 / 1 (-1: none)
struct KtileBf16 { static constexpr int wait_phases = 0b1010, any_wait = 0b1010, epi_stores = 16, tail0 = -1, tail1 = 0; };
template <bool BYTE_OUT>      // fp8: every MFMA needs the whole K extent -- pieces are cut by row set, piece p is first read in phase max(0, p - 1)
struct KtileFp8 { static constexpr int wait_phases = 0b1011, any_wait = 0b1111, epi_stores = BYTE_OUT ? 8 : 16, tail0 = 2, tail1 = 0; };
// The LOAD segment's tail of phase p, placed in the kernel's phase loop behind its fragment reads; stage_piece(src, buffer, piece) is
// the kernel's.  (A macro: as a function over the kernels' LOAD and COMPUTE bodies the whole K-tile changed both kernels; the outer
// any_wait test is the shape the bf16 kernel had.)
#define OV_GEMM_KTILE_STAGE_WAIT(T, KIND, p, strict, has_next, cur, nxt, nb, stage_piece)         \
    do {                                                                                          \
        if (KIND == 1 || KIND == 2) stage_piece(cur, nb, p);                                      \
        if (KIND == 3) { if (has_next) stage_piece(nxt, nb, p); }                                 \
        if ((T::any_wait >> p) & 1) {                                                             \
            if (KIND == 0) {                                                                      \
                if (p == 3) {                                                                     \
                    if (strict) gemm::wait_vmcnt<0>();                                        \
                    else gemm::wait_vmcnt<T::epi_stores>();                                       \
                }                                                                                 \
            } else if (KIND == 1) {                                                               \
                if (p == 3) gemm::wait_vmcnt<4>();                                            \
            } else if (KIND == 2) {                                                               \
                if ((T::wait_phases >> p) & 1) gemm::wait_vmcnt<4>();                         \
            } else {                                                                              \
                if (has_next) { if ((T::wait_phases >> p) & 1) gemm::wait_vmcnt<4>(); }       \
                else if (p == 0) { if (T::tail0 >= 0) gemm::wait_vmcnt<(T::tail0 < 0 ? 0 : T::tail0)>(); } \
                else if (p == 1) gemm::wait_vmcnt<T::tail1>();                                    \
            }                                                                                     \
        }                                                                                         \
    } while (0)

// Tile hand-over.  Behind the re-alignment, with the buffer `cb` of the last K-tile free: K-tile 1 of the next tile and (PARAMS) its
// parameter block go out AHEAD of the epilogue's stores -- vmcnt retires in order, so every LDS-DMA the next main loop waits for in its
// first two K-tiles is older than the stores; the vmcnt(8) in between: K-tile 0 of the next tile (issued a K-tile ago) has landed.
// advance(src) and stage_piece(src, buffer, piece) are the kernel's.  (Macros: as functions both steps changed both kernels.)
#define OV_GEMM_HANDOVER_STAGE(nxt, cb, advance, stage_piece, PARAMS)                             \
    do {                                                                                          \
        advance(nxt);                                                                             \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) stage_piece(nxt, cb, j_);                \
        advance(nxt);                                                                             \
        gemm::wait_vmcnt<8>();                                                                    \
        PARAMS;                                                                                   \
    } while (0)
// Behind the epilogue: an edge tile issued fewer stores than K-tile 0's counted wait assumes, so the next wait is strict; the barrier
// makes the next tile's K-tile 0 visible to all.  The caller re-staggers behind it, then the next tile becomes the current one.
__device__ __forceinline__ void handover_barrier(bool edge, bool& strict) {
    strict = edge;
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
}
#define OV_GEMM_HANDOVER_SWAP(cb, STAGE, pslot, cur, nxt, m0, nm0, n0, nn0)                       \
    do {                                                                                          \
        cb ^= STAGE;                                                                              \
        pslot ^= 1;                                                                               \
        cur = nxt;                                                                                \
        m0 = nm0;                                                                                 \
        n0 = nn0;                                                                                 \
    } while (0)

}  // namespace gemm
