// strip.h — the pieces the fused contrastive losses share (loss.hip, multicap.hip, distill.hip, siglip.hip), stated once.
//
// Every loss walks [b, N] logit strips in 32 x 32 tiles that are never written.  A tile is one f32x16 accumulator of the exact-fp32
// v_mfma_f32_32x32x2_f32 with the in-side (gathered) rows as the A operand: lane (j, half) holds, for out row j, the 16 in-side
// entries tile_row(i, half), so a row reduction is lane-local plus one exchange of the two lane halves.
//   forward : dot_full over the full K, then each loss's own row statistic; lse_merge joins (max, sum-exp) pairs.
//   backward: four waves split the K reduction by e-tile (dot_wave), exchange the partial tiles through LDS (put / get, summed in
//             the fixed order ((p0 + p1) + p2) + p3), form the loss's coefficient tile p in registers, and feed it back as the MFMA
//             A operand into [32 x E] accumulators (accumulate), stored once (store).
// The helpers hold no barrier: put and get sit between the caller's two __syncthreads(), so distill.hip exchanges its student and
// teacher tiles between one pair.  RAGGED (siglip.hip: E % 8, not % 32) guards the last e-tile; the others instantiate false.
#pragma once
#include "common.h"

namespace strip {

constexpr int MAXT = 9;              // backward: e-tiles per wave, E <= 4 * 9 * 32 = 1152

// the in-side row (or, in store, the out row) of accumulator register i in lane half `half`
__device__ __forceinline__ int tile_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

__device__ __forceinline__ f32x16_t zero16() {
    f32x16_t z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// eight k of the contraction, in k order
__device__ __forceinline__ f32x16_t mfma4(const float4 av, const float4 bv, f32x16_t acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
    return acc;
}

// (M, S) <- (M, S) joined with (mw, sw): running maximum and sum of exponentials relative to it.  `S * e + sw * ew` leaves the
// compiler free to round either product or both, and it chose by what surrounded the statement; the two forms it had chosen are
// written out so that an inlined call gives the same bits wherever it lands.  Inside a strip kernel (lane halves, waves) the
// newcomer's product is rounded and the running sum's is fused:
__device__ __forceinline__ void lse_merge(float& M, float& S, float mw, float sw) {
    const float mn = fmaxf(M, mw);
    if (mn > -INFINITY) S = fmaf(S, __expf(M - mn), sw * __expf(mw - mn));
    M = mn;
}

// the two lane halves of a row hold disjoint columns: join them (both halves end with the row's pair)
__device__ __forceinline__ void lse_merge_halves(float& m, float& s) {
    lse_merge(m, s, __shfl_xor(m, 32, 64), __shfl_xor(s, 32, 64));
}

// The column splits' pairs of one row, p[0], p[1] and then every split_stride floats, joined in split order.  In the finalize
// kernels both products are rounded.
__device__ __forceinline__ void lse_merge_splits(const float* p, int64_t split_stride, int nsplit, float& M, float& S) {
    M = -INFINITY; S = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) {
        const float mw = p[sp * split_stride], sw = p[sp * split_stride + 1];
        const float mn = fmaxf(M, mw);
        if (mn > -INFINITY) S = __fadd_rn(__fmul_rn(S, __expf(M - mn)), __fmul_rn(sw, __expf(mw - mn)));
        M = mn;
    }
}

// forward: acc[i] = <Y[tile_row(i, half)], X[row]> over K floats in one k-ordered chain.  yp / xp: this lane's rows, already
// offset by 4 * half.
__device__ __forceinline__ f32x16_t dot_full(const float* yp, const float* xp, int K) {
    f32x16_t acc = zero16();
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 8) acc = mfma4(*(const float4*)(yp + k0), *(const float4*)(xp + k0), acc);
    return acc;
}

// backward: this wave's share of the same dots, over its nown e-tiles wave, wave + 4, ...
template <bool RAGGED>
__device__ __forceinline__ f32x16_t dot_wave(const float* yip, const float* xop, int E, int wave, int nown) {
    f32x16_t acc = zero16();
    for (int n = 0; n < nown; ++n) {
        const int e0 = (wave + 4 * n) * 32;
        const int kend = RAGGED && E - e0 < 32 ? E - e0 : 32;
#pragma unroll
        for (int k0 = 0; k0 < 32; k0 += 8)
            if (!RAGGED || k0 < kend) acc = mfma4(*(const float4*)(yip + e0 + k0), *(const float4*)(xop + e0 + k0), acc);
    }
    return acc;
}

// the LDS exchange of the waves' partial tiles.  The caller brackets put with two __syncthreads(): the first says the previous
// tile's partials have been consumed, the second that this tile's are complete.
typedef float Exchange[4][16][64];

__device__ __forceinline__ void put(Exchange part, int wave, int lane, const f32x16_t acc) {
#pragma unroll
    for (int i = 0; i < 16; ++i) part[wave][i][lane] = acc[i];
}

__device__ __forceinline__ float get(const Exchange part, int i, int lane) {
    return ((part[0][i][lane] + part[1][i][lane]) + part[2][i][lane]) + part[3][i][lane];
}

// out[o, e] += sum_g p[o, g] * XI[g, e] over in-side tile t: contraction step s pairs g0(s) = tile_row(s, 0) (k = 0, held by the
// lower lane half as register s) with g0(s) + 4 (k = 1, upper half), so the A operand is this lane's own p[s].  Rows past ni and,
// if RAGGED, columns past E are read in range (clamped); their p is zero / they are never stored.
// KEEP_ROWS: form the 16 row offsets g * ldxi once per tile and hold them (32 registers) across the e-tiles, instead of inside
// each e-tile's branch, where the compiler recomputes some of the 64-bit products.  Measured at b = 4096 of N = 32768, E = 768:
// 4 to 6 % off the InfoNCE and SigLIP backward, but 13 % ON distillation's, which already carries a second logit tile; so
// distill.hip instantiates false (profiles/strip_refactor_time.json).
template <int NT, bool RAGGED, bool KEEP_ROWS>
__device__ __forceinline__ void accumulate(f32x16_t (&acc_o)[NT], const f32x16_t p, const float* __restrict__ XI, int64_t ldxi,
                                           int t, int ni, int E, int wave, int nown, int j, int half) {
    const auto row_offset = [&](int s) {                          // of in-side row s of this lane half, clamped into range
        const int g = t * 32 + tile_row(s, half);
        return (int64_t)(g < ni ? g : ni - 1) * ldxi;
    };
    int64_t row[16];
    if (KEEP_ROWS) {
#pragma unroll
        for (int s = 0; s < 16; ++s) row[s] = row_offset(s);
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (n < nown) {
            int e = (wave + 4 * n) * 32 + j;
            if (RAGGED) e = e < E ? e : E - 1;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float yv = XI[(KEEP_ROWS ? row[s] : row_offset(s)) + e];
                acc_o[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[s], yv, acc_o[n], 0, 0, 0);
            }
        }
    }
}

// OUT[row, e] = acc_o * coef for the rows of out tile rt below no
template <int NT, bool RAGGED>
__device__ __forceinline__ void store(const f32x16_t (&acc_o)[NT], float* __restrict__ OUT, int64_t ldout, int rt, int no, int E,
                                      int wave, int nown, int j, int half, float coef) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (n < nown) {
            const int e = (wave + 4 * n) * 32 + j;
            if (!RAGGED || e < E) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = rt * 32 + tile_row(i, half);
                    if (row < no) OUT[(int64_t)row * ldout + e] = acc_o[n][i] * coef;
                }
            }
        }
    }
}

// out[0] = c * grad * sum part[0 .. n) in a fixed order (grad NULL = 1): d loss / d scale from the per-row-tile partials.  A
// template so that only the files that launch it carry it.
template <int NT>
__global__ __launch_bounds__(NT) void scaled_sum(const float* __restrict__ part, int n, float c, const float* __restrict__ grad,
                                                 float* __restrict__ out) {
    static_assert(NT == 64, "one wave");
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += NT) v += part[i];
    v = wave_sum(v);
    if (threadIdx.x == 0) out[0] = v * c * (grad ? *grad : 1.f);
}

// The forward's split rule: nstrips strips of nrt row tiles each want ~1024 workgroups (four per CU), every column split keeps at
// least four 32-column tiles (one per wave), and no split is empty.
struct StripPlan { int bpad, nrt, ntiles, nsplit, tps; };

inline StripPlan strip_plan(int b, int N, int nstrips) {
    StripPlan p;
    p.nrt = (b + 31) / 32;
    p.bpad = p.nrt * 32;
    p.ntiles = (N + 31) / 32;
    int want = 1024 / (nstrips * p.nrt);
    if (want < 1) want = 1;
    int maxsplit = (p.ntiles + 3) / 4;
    if (maxsplit < 1) maxsplit = 1;
    p.nsplit = want < maxsplit ? want : maxsplit;
    p.tps = (p.ntiles + p.nsplit - 1) / p.nsplit;
    p.nsplit = (p.ntiles + p.tps - 1) / p.tps;
    return p;
}

}  // namespace strip
