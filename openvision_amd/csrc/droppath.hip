// droppath.hip — the glue of stochastic depth on the sample axis (gfx950): the reference's DropPath (src/models/common.py:659-675)
// multiplies a residual branch by m[b] / keep with m[b] in {0, 1} per sample, so a dropped sample's branch contributes exactly zero to
// the forward and to every gradient.  The tower walks (tower.hip, backward.hip) therefore run a branch on its kept samples only:
//
//   ov_sample_gather        dst[j L + t, :] = bf16(scale * src[idx[j] L + t, :])  for j < k      (scale == 1.0f: a bitwise copy)
//   ov_sample_scatter_axpy  out[b] = bf16(res[b] + scale * y[slot[b]])  where slot[b] >= 0, else out[b] = res[b] bitwise
//
// Both are one memory-bound pass in plain C++: the L rows of a sample are contiguous (L D bf16, D % 8 == 0), a lane moves 16 bytes, the
// 64 lanes of a wave 1 KiB of consecutive addresses, four such pieces per thread in flight; no LDS.  grid.y is the sample, so no lane
// divides.  An index outside its range (idx[j] outside [0, B), slot[b] >= k) moves nothing for that sample: nothing is read or written
// out of bounds whatever the tables hold.
//
// The backward uses the ADDING form of the scatter: the LayerNorm backward of a compact branch runs without its residual input and
// leaves the branch's input gradient in a compact buffer; ov_sample_scatter_axpy(res = the half's incoming gradient, scale = 1) then
// forms dx for all B samples, a dropped sample's rows being the incoming gradient bitwise.  So the incoming gradient is gathered once
// (with 1 / keep, as the branch's output gradient), not twice.
#include "common.h"

namespace {
constexpr int DP_UNROLL = 4;            // 16-byte pieces per thread
constexpr int DP_BLOCK = 256;

// cps: 16-byte pieces per sample (L D / 8).  grid (ceil(cps / 1024), k)
template <bool SCALED>
__global__ __launch_bounds__(DP_BLOCK) void sample_gather(const ov_bf16* __restrict__ src, const int* __restrict__ idx, ov_bf16* __restrict__ dst,
                                                          int B, int cps, float scale) {
    const int j = blockIdx.y;
    const int s = idx[j];
    if ((unsigned)s >= (unsigned)B) return;
    const u32x4_t* in = (const u32x4_t*)src + (int64_t)s * cps;
    u32x4_t* out = (u32x4_t*)dst + (int64_t)j * cps;
    const int c0 = blockIdx.x * (DP_BLOCK * DP_UNROLL) + threadIdx.x;
    u32x4_t v[DP_UNROLL];
#pragma unroll
    for (int u = 0; u < DP_UNROLL; ++u) {
        const int c = c0 + u * DP_BLOCK;
        if (c < cps) v[u] = in[c];
    }
#pragma unroll
    for (int u = 0; u < DP_UNROLL; ++u) {
        const int c = c0 + u * DP_BLOCK;
        if (c >= cps) continue;
        if (SCALED) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = pack_bf16x2(__fmul_rn(scale, bf16lo_to_f32(v[u][e])), __fmul_rn(scale, bf16hi_to_f32(v[u][e])));
        }
        out[c] = v[u];
    }
}

// r + s y with the product rounded to fp32 before the sum (contraction into an fma is switched off for this statement block: the
// value is the one the two separate operations give)
__device__ __forceinline__ float axpy_rn(float r, float s, float y) {
#pragma clang fp contract(off)
    const float p = s * y;
    return r + p;
}

// grid (ceil(cps / 1024), B).  out may alias res (same sample, same piece, read before written by the same lane).
__global__ __launch_bounds__(DP_BLOCK) void sample_scatter_axpy(const ov_bf16* res, const ov_bf16* __restrict__ y, const int* __restrict__ slot,
                                                                ov_bf16* out, int k, int cps, float scale) {
    const int b = blockIdx.y;
    const int s = slot[b];
    const bool kept = s >= 0 && s < k;
    if (!kept && out == res) return;
    const u32x4_t* r = (const u32x4_t*)res + (int64_t)b * cps;
    const u32x4_t* yy = (const u32x4_t*)y + (int64_t)(kept ? s : 0) * cps;
    u32x4_t* o = (u32x4_t*)out + (int64_t)b * cps;
    const int c0 = blockIdx.x * (DP_BLOCK * DP_UNROLL) + threadIdx.x;
    u32x4_t rv[DP_UNROLL], yv[DP_UNROLL];
#pragma unroll
    for (int u = 0; u < DP_UNROLL; ++u) {
        const int c = c0 + u * DP_BLOCK;
        if (c < cps) {
            rv[u] = r[c];
            if (kept) yv[u] = yy[c];
        }
    }
#pragma unroll
    for (int u = 0; u < DP_UNROLL; ++u) {
        const int c = c0 + u * DP_BLOCK;
        if (c >= cps) continue;
        if (kept) {     // one rounding of the product, one of the sum, one to bf16: no contraction into an fma
#pragma unroll
            for (int e = 0; e < 4; ++e)
                rv[u][e] = pack_bf16x2(axpy_rn(bf16lo_to_f32(rv[u][e]), scale, bf16lo_to_f32(yv[u][e])),
                                       axpy_rn(bf16hi_to_f32(rv[u][e]), scale, bf16hi_to_f32(yv[u][e])));
        }
        o[c] = rv[u];
    }
}

// 16-byte pieces per sample; shape_ok: what the kernels' int indices and grid.y take
inline int64_t pieces(int L, int D) { return (int64_t)L * D / 8; }
inline bool shape_ok(int B, int k, int L, int D) {
    return B > 0 && k >= 0 && k <= B && L > 0 && D > 0 && D % 8 == 0 && B <= 65535 && pieces(L, D) <= 0x7fffffffLL;
}
}  // namespace

extern "C" int ov_sample_gather(const ov_bf16* src, const int* idx, ov_bf16* dst, int B, int k, int L, int D, float scale, ov_stream_t stream) {
    if (B <= 0 || k < 0 || k > B || L <= 0 || D <= 0) return OV_ERR_INVALID;
    if (!shape_ok(B, k, L, D)) return OV_ERR_UNSUPPORTED;
    if (k == 0) return OV_OK;
    if (!src || !idx || !dst) return OV_ERR_INVALID;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) || ((uintptr_t)idx & 3)) return OV_ERR_INVALID;
    const int cps = (int)pieces(L, D);
    const dim3 grid((unsigned)((cps + DP_BLOCK * DP_UNROLL - 1) / (DP_BLOCK * DP_UNROLL)), (unsigned)k);
    if (scale == 1.0f) hipLaunchKernelGGL(sample_gather<false>, grid, dim3(DP_BLOCK), 0, (hipStream_t)stream, src, idx, dst, B, cps, scale);
    else hipLaunchKernelGGL(sample_gather<true>, grid, dim3(DP_BLOCK), 0, (hipStream_t)stream, src, idx, dst, B, cps, scale);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_sample_scatter_axpy(const ov_bf16* res, const ov_bf16* y, const int* slot, ov_bf16* out, int B, int k, int L, int D, float scale,
                                      ov_stream_t stream) {
    if (B <= 0 || k < 0 || k > B || L <= 0 || D <= 0) return OV_ERR_INVALID;
    if (!shape_ok(B, k, L, D)) return OV_ERR_UNSUPPORTED;
    if (!res || !slot || !out || (k > 0 && !y)) return OV_ERR_INVALID;
    if ((((uintptr_t)res | (uintptr_t)y | (uintptr_t)out) & 15) || ((uintptr_t)slot & 3)) return OV_ERR_INVALID;
    const int cps = (int)pieces(L, D);
    const dim3 grid((unsigned)((cps + DP_BLOCK * DP_UNROLL - 1) / (DP_BLOCK * DP_UNROLL)), (unsigned)B);
    hipLaunchKernelGGL(sample_scatter_axpy, grid, dim3(DP_BLOCK), 0, (hipStream_t)stream, res, y, slot, out, k, cps, scale);
    OV_LAUNCH_CHECK();
    return OV_OK;
}
