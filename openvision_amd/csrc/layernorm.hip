// layernorm.hip — row LayerNorm with fp32 statistics (HBM-bound), gfx950.
//
// Replaces aten::native_layer_norm behind LayerNorm / LayerNormFp32.forward
// (reference open_clip/transformer.py:15-30; eps = 1e-6 from transformer.py:458,491,499,537,690,720).
// One 64-lane wave per row: each lane keeps its 16-byte chunks of the row in registers, so the row is
// read from HBM exactly once; mean and (biased) variance are two wave reductions over registers
// (two-pass, no E[x^2]-E[x]^2 cancellation); output is written once as 16-byte stores.
// Algorithmic traffic: rows * D * (sizeof(in) + sizeof(out)) bytes (+ gamma/beta, L2-resident).
#include "common.h"

namespace {

template <int NCH, bool IN_F32, bool OUT_F32>
__global__ __launch_bounds__(256) void layernorm_rows(const void* __restrict__ xv, int64_t ldx,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, void* __restrict__ yv,
                                                      int64_t ldy, int64_t rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nchunk = D >> 3;
    const float invD = 1.0f / (float)D;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        float v[NCH][8];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + c * 64;
            if (ch < nchunk) {
                if (IN_F32) {
                    const float4* p = (const float4*)((const float*)xv + row * ldx + ch * 8);
                    const float4 a = p[0], b = p[1];
                    v[c][0] = a.x; v[c][1] = a.y; v[c][2] = a.z; v[c][3] = a.w;
                    v[c][4] = b.x; v[c][5] = b.y; v[c][6] = b.z; v[c][7] = b.w;
                } else {
                    const u32x4_t w = *(const u32x4_t*)((const ov_bf16*)xv + row * ldx + ch * 8);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[c][2 * e] = bf16lo_to_f32(w[e]);
                        v[c][2 * e + 1] = bf16hi_to_f32(w[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) s += v[c][e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
            }
        }
        const float mean = wave_sum(s) * invD;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (lane + c * 64 < nchunk) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = v[c][e] - mean;
                    q += d * d;
                }
            }
        }
        const float rstd = rsqrtf(wave_sum(q) * invD + eps);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + c * 64;
            if (ch < nchunk) {
                const float4 g0 = *(const float4*)(gamma + ch * 8), g1 = *(const float4*)(gamma + ch * 8 + 4);
                const float4 b0 = *(const float4*)(beta + ch * 8), b1 = *(const float4*)(beta + ch * 8 + 4);
                float o[8];
                o[0] = (v[c][0] - mean) * rstd * g0.x + b0.x;
                o[1] = (v[c][1] - mean) * rstd * g0.y + b0.y;
                o[2] = (v[c][2] - mean) * rstd * g0.z + b0.z;
                o[3] = (v[c][3] - mean) * rstd * g0.w + b0.w;
                o[4] = (v[c][4] - mean) * rstd * g1.x + b1.x;
                o[5] = (v[c][5] - mean) * rstd * g1.y + b1.y;
                o[6] = (v[c][6] - mean) * rstd * g1.z + b1.z;
                o[7] = (v[c][7] - mean) * rstd * g1.w + b1.w;
                if (OUT_F32) {
                    float4* p = (float4*)((float*)yv + row * ldy + ch * 8);
                    p[0] = make_float4(o[0], o[1], o[2], o[3]);
                    p[1] = make_float4(o[4], o[5], o[6], o[7]);
                } else {
                    u32x4_t w = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]),
                                 pack_bf16x2(o[6], o[7])};
                    *(u32x4_t*)((ov_bf16*)yv + row * ldy + ch * 8) = w;
                }
            }
        }
    }
}

// {mean, rstd} per row only (LN folded into the next GEMM's epilogue): reads the row once, writes 8 bytes.
template <int NCH>
__global__ __launch_bounds__(256) void rowstats_rows(const ov_bf16* __restrict__ x, int64_t ldx, float* __restrict__ st,
                                                     int64_t rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nchunk = D >> 3;
    const float invD = 1.0f / (float)D;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        float v[NCH][8];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + c * 64;
            if (ch < nchunk) {
                const u32x4_t w = *(const u32x4_t*)(x + row * ldx + ch * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[c][2 * e] = bf16lo_to_f32(w[e]);
                    v[c][2 * e + 1] = bf16hi_to_f32(w[e]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) s += v[c][e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
            }
        }
        const float mean = wave_sum(s) * invD;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (lane + c * 64 < nchunk) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = v[c][e] - mean;
                    q += d * d;
                }
            }
        }
        const float rstd = rsqrtf(wave_sum(q) * invD + eps);
        if (lane == 0) *(float2*)(st + 2 * row) = make_float2(mean, rstd);
    }
}

template <int NCH>
int launch_ln(const void* x, int xd, int64_t ldx, const float* g, const float* b, void* y, int yd, int64_t ldy,
              int64_t rows, int D, float eps, hipStream_t st) {
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 16384) blocks = 16384;
    dim3 grid((unsigned)blocks), blk(256);
    if (xd == OV_BF16 && yd == OV_BF16)
        hipLaunchKernelGGL((layernorm_rows<NCH, false, false>), grid, blk, 0, st, x, ldx, g, b, y, ldy, rows, D, eps);
    else if (xd == OV_BF16 && yd == OV_F32)
        hipLaunchKernelGGL((layernorm_rows<NCH, false, true>), grid, blk, 0, st, x, ldx, g, b, y, ldy, rows, D, eps);
    else if (xd == OV_F32 && yd == OV_BF16)
        hipLaunchKernelGGL((layernorm_rows<NCH, true, false>), grid, blk, 0, st, x, ldx, g, b, y, ldy, rows, D, eps);
    else
        hipLaunchKernelGGL((layernorm_rows<NCH, true, true>), grid, blk, 0, st, x, ldx, g, b, y, ldy, rows, D, eps);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

}  // namespace

extern "C" int ov_layernorm(const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* beta,
                            void* y, int y_dtype, int64_t ldy, int64_t rows, int D, float eps,
                            ov_stream_t stream) {
    if (!x || !y || !gamma || !beta || rows <= 0 || D <= 0) return OV_ERR_INVALID;
    if ((x_dtype != OV_BF16 && x_dtype != OV_F32) || (y_dtype != OV_BF16 && y_dtype != OV_F32)) return OV_ERR_INVALID;
    if (D % 8 || D > 8192 || ldx % 8 || ldy % 8 || ldx < D || ldy < D) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 15) return OV_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int nch = (D / 8 + 63) / 64;
    if (nch <= 1) return launch_ln<1>(x, x_dtype, ldx, gamma, beta, y, y_dtype, ldy, rows, D, eps, st);
    if (nch <= 2) return launch_ln<2>(x, x_dtype, ldx, gamma, beta, y, y_dtype, ldy, rows, D, eps, st);
    if (nch <= 3) return launch_ln<3>(x, x_dtype, ldx, gamma, beta, y, y_dtype, ldy, rows, D, eps, st);
    if (nch <= 4) return launch_ln<4>(x, x_dtype, ldx, gamma, beta, y, y_dtype, ldy, rows, D, eps, st);
    if (nch <= 8) return launch_ln<8>(x, x_dtype, ldx, gamma, beta, y, y_dtype, ldy, rows, D, eps, st);
    return launch_ln<16>(x, x_dtype, ldx, gamma, beta, y, y_dtype, ldy, rows, D, eps, st);
}

namespace {
// Row statistics through partial sums (common.h): one thread per (row, 32-column group) reads 64 bytes and applies the fixed tree.
__global__ __launch_bounds__(256) void rowparts_kernel(const ov_bf16* __restrict__ x, int64_t ldx, float* __restrict__ parts, int64_t rows, int G) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * G) return;
    const int64_t row = idx / G;
    const int g = (int)(idx - row * G);
    const u32x4_t* p = (const u32x4_t*)(x + row * ldx + g * 32);
    float s[4], q[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) stat_octet(p[o], s[o], q[o]);
    const float sg = __fadd_rn(__fadd_rn(s[0], s[1]), __fadd_rn(s[2], s[3]));       // block 0 + block 1
    const float qg = __fadd_rn(__fadd_rn(q[0], q[1]), __fadd_rn(q[2], q[3]));
    *(float2*)(parts + idx * 2) = make_float2(sg, qg);
}
// {mean, rstd} of a row from its G partial sums: mean = S / D, var = Q / D - mean^2 (clamped at 0).  One pass instead of
// rowstats_rows' two: fp32 sums of D <= 8192 bf16 values carry ~1e-7 relative error, so var is good to ~1e-7 (1 + mean^2 / var)
// relative -- the LayerNorm inputs here have |mean| of the order of their standard deviation or below (the domain, as a table of
// |mean| / std against D: DESIGN.md §4, "The row passes against fp64"; tests/test_ln_rows_bound.py pins it).  Eight lanes per row (a row's
// G float2 are contiguous: coalesced 8-byte reads), each adds its groups g = k, k + 8, ... in that order, then a fixed xor tree over
// the eight lanes (the same for every row, whatever wrote the sums).
__global__ __launch_bounds__(256) void rowstats_finalize_kernel(const float* __restrict__ parts, float* __restrict__ st, int64_t rows, int G, float invD, float eps) {
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int k = threadIdx.x & 7;
    float S = 0.f, Q = 0.f;
    if (row < rows) {
        const float2* p = (const float2*)(parts + row * G * 2);
        for (int g = k; g < G; g += 8) {
            const float2 v = p[g];
            S = __fadd_rn(S, v.x);
            Q = __fadd_rn(Q, v.y);
        }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        S = __fadd_rn(S, __shfl_xor(S, o, 64));
        Q = __fadd_rn(Q, __shfl_xor(Q, o, 64));
    }
    if (row < rows && k == 0) {
        const float mean = __fmul_rn(S, invD);
        const float var = fmaxf(__fsub_rn(__fmul_rn(Q, invD), __fmul_rn(mean, mean)), 0.f);
        *(float2*)(st + 2 * row) = make_float2(mean, rsqrtf(var + eps));
    }
}
}  // namespace

extern "C" int ov_rowparts(const ov_bf16* x, int64_t ldx, float* parts, int64_t rows, int D, ov_stream_t stream) {
    if (!x || !parts || rows <= 0 || D <= 0) return OV_ERR_INVALID;
    if (D % 32 || ldx % 8 || ldx < D) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)parts & 7)) return OV_ERR_INVALID;
    const int G = D / 32;
    const int64_t n = rows * G;
    if ((n + 255) / 256 > 0x7fffffffLL) return OV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(rowparts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, parts, rows, G);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_rowstats_finalize(const float* parts, float* rowstats, int64_t rows, int D, float eps, ov_stream_t stream) {
    if (!parts || !rowstats || rows <= 0 || D <= 0) return OV_ERR_INVALID;
    if (D % 32 || D > 8192) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)parts & 7) || ((uintptr_t)rowstats & 7)) return OV_ERR_INVALID;
    hipLaunchKernelGGL(rowstats_finalize_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, parts, rowstats, rows,
                       D / 32, 1.0f / (float)D, eps);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_rowstats(const ov_bf16* x, int64_t ldx, float* rowstats, int64_t rows, int D, float eps, ov_stream_t stream) {
    if (!x || !rowstats || rows <= 0 || D <= 0) return OV_ERR_INVALID;
    if (D % 8 || D > 8192 || ldx % 8 || ldx < D) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)rowstats & 7)) return OV_ERR_INVALID;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 16384) blocks = 16384;
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const int nch = (D / 8 + 63) / 64;
    if (nch <= 1) hipLaunchKernelGGL(rowstats_rows<1>, grid, blk, 0, st, x, ldx, rowstats, rows, D, eps);
    else if (nch <= 2) hipLaunchKernelGGL(rowstats_rows<2>, grid, blk, 0, st, x, ldx, rowstats, rows, D, eps);
    else if (nch <= 3) hipLaunchKernelGGL(rowstats_rows<3>, grid, blk, 0, st, x, ldx, rowstats, rows, D, eps);
    else if (nch <= 4) hipLaunchKernelGGL(rowstats_rows<4>, grid, blk, 0, st, x, ldx, rowstats, rows, D, eps);
    else if (nch <= 8) hipLaunchKernelGGL(rowstats_rows<8>, grid, blk, 0, st, x, ldx, rowstats, rows, D, eps);
    else hipLaunchKernelGGL(rowstats_rows<16>, grid, blk, 0, st, x, ldx, rowstats, rows, D, eps);
    OV_LAUNCH_CHECK();
    return OV_OK;
}
