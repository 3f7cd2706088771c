// ascent.hip — the inner loop of ov-gradient-ascent.py around the frozen text tower (gfx950).
//
// The script learns normu fp32 [B,K,V] (R = B K rows) for `steps` iterations of (ov-gradient-ascent.py:226-259, :380-381)
//     img_b  = Normalization(RandomAffine(degrees, translate, p)(image))                  detached
//     soft   = F.gumbel_softmax(normu, tau, hard=True)        z = (normu - log e) / tau, ys = softmax(z), forward value one_hot(argmax z)
//     tx     = text tower(cat(prompt, pad, soft) @ W + pos)   the tower's input at a learned row is W[idx]; its gradient there is dX
//     loss   = mean_j -100 mean_i cos(tx_j, img_i)
//     normu  = Adam(normu, d loss / d normu)                  d normu[r,v] = ys[r,v] (gy[r,v] - c_r) / tau, gy = dX W^T, c_r = sum_v gy ys
// Everything but the two towers is here, five entry points:
//
//   ov_ga_affine        out[b,c,y,x] = (bilinear(img[c], a0 x + a1 y + a2, a3 x + a4 y + a5) - mean_c) / std_c: the four taps around the
//                       source point, a tap outside the image zero (grid_sample 'bilinear', 'zeros', align_corners=False)
//   ov_ga_sample        per row: z itself (kept: its correctly rounded logarithm is formed once, in double), the first argmax of z, max
//                       z, sum exp(z - max z); the index into the step's history row and, as an int64 token id, into the id matrix
//                       the embedding gather reads
//   ov_ga_token_grad    gy = dX W^T on the bf16 MFMA with fp32 accumulators, stored fp32, and per 128-column slab sum_v gy ys (parts)
//   ov_ga_adam          c_r from parts in ascending order, g = ys (gy - c_r) / tau, torch.optim.Adam's single-tensor update
//   ov_ga_cosine_loss   loss1, d mean(loss1) / d tx, and the best mean so far with its step and its tx, in one launch
//
// ov_ga_token_grad is bound by its one read of W (49 MB at V = 32000, D = 768): a workgroup owns 128 rows of W and streams them from
// global memory straight into MFMA operand registers, 64 contiguous bytes per lane and 64-column block of D; dX (<= 64 rows) waits in
// LDS.  The other four stream their operands once.  No atomics: every sum runs in one fixed order, so a step is repeatable bit for
// bit.  Nothing is flushed to zero (|d normu| is of the order 1e-10, below Adam's eps).
#include "common.h"
#include <math.h>

namespace {

constexpr int GA_MAX_ROWS = 4096, GA_MAX_SIZE = 4096, GA_MAX_BATCH = 64;
constexpr int GA_SLAB = 128;                 // vocabulary rows per workgroup of ov_ga_token_grad
constexpr int GA_AHEAD = 6;                 // 64-column blocks of W a lane asks for at once in ov_ga_token_grad
constexpr int GA_LDS_PAD = 8;                // bf16 elements added to an LDS row of dX: 16-byte reads of 32 rows spread over the banks

// z = (normu - log e) / tau and ys = exp(z - zmax) / zsum: ONE sequence of fp32 operations for the three kernels that form them.
// log e is the correctly rounded fp32 logarithm, taken in double and rounded once: a float library logarithm is within an ulp of it
// but differs from one library to the next, and max z is compared bit for bit with a host restatement.
__device__ __forceinline__ float ga_z(float nu, float e, float tau) {
#pragma clang fp contract(off)
    return (nu - (float)log((double)e)) / tau;
}
__device__ __forceinline__ float ga_ys(float z, float zmax, float zsum) {
#pragma clang fp contract(off)
    return expf(z - zmax) / zsum;
}

// ---- ov_ga_affine ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tap(const float* __restrict__ plane, int y, int x, int S) {
    return (y >= 0 && y < S && x >= 0 && x < S) ? plane[(int64_t)y * S + x] : 0.f;
}

template <bool BF16>
__global__ __launch_bounds__(256) void ga_affine_kernel(const float* __restrict__ img, const float* __restrict__ mats,
                                                        const float* __restrict__ mean, const float* __restrict__ stdv, void* __restrict__ out,
                                                        int B, int S) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)B * S * S;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % S), y = (int)((i / S) % S), b = (int)(i / ((int64_t)S * S));
        const float* m = mats + b * 6;
        const float fx = (float)x, fy = (float)y;
        const float sx = (m[0] * fx + m[1] * fy) + m[2], sy = (m[3] * fx + m[4] * fy) + m[5];
        // far outside (or not finite): every tap is zero; the clamp keeps the int conversion defined
        const bool far = !(sx > -2.f && sx < (float)S + 1.f && sy > -2.f && sy < (float)S + 1.f);
        const float x0f = far ? -2.f : floorf(sx), y0f = far ? -2.f : floorf(sy);
        const int x0 = (int)x0f, y0 = (int)y0f;
        const float wx1 = far ? 0.f : sx - x0f, wy1 = far ? 0.f : sy - y0f;
        const float wx0 = (x0f + 1.f) - (far ? x0f : sx), wy0 = (y0f + 1.f) - (far ? y0f : sy);
        const float w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* plane = img + (int64_t)c * S * S;
            const float v = ((tap(plane, y0, x0, S) * w00 + tap(plane, y0, x0 + 1, S) * w01) + tap(plane, y0 + 1, x0, S) * w10) +
                            tap(plane, y0 + 1, x0 + 1, S) * w11;
            const float o = (v - mean[c]) / stdv[c];
            const int64_t at = (((int64_t)b * 3 + c) * S + y) * S + x;
            if (BF16) ((ov_bf16*)out)[at] = f32_to_bf16_bits(o);
            else ((float*)out)[at] = o;
        }
    }
}

// ---- ov_ga_sample ----------------------------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads per row.  z is formed once (the double logarithm is the cost of this kernel) and stored for the two
// kernels after it.  The maximum and its first index: per thread over v = tid, tid + 1024, ... (ascending, strict >), then across lanes
// and waves with (larger z, then smaller v).  The sum: each thread over its own stored z in the same order, wave_sum's butterfly, the
// sixteen waves in ascending order.
constexpr int GA_SAMPLE_THREADS = 1024;
__global__ __launch_bounds__(GA_SAMPLE_THREADS) void ga_sample_kernel(const float* __restrict__ normu, const float* __restrict__ e, float tau,
                                                                      int V, int K, int T, float* __restrict__ z, int* __restrict__ idx,
                                                                      float* __restrict__ zmax, float* __restrict__ zsum,
                                                                      int* __restrict__ hist_row, int64_t* __restrict__ ids) {
    constexpr int NW = GA_SAMPLE_THREADS / 64;
    __shared__ float sm[NW];
    __shared__ int si[NW];
    __shared__ float ss[NW];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* nu = normu + (int64_t)r * V;
    const float* er = e + (int64_t)r * V;
    float* zr = z + (int64_t)r * V;
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int v = tid; v < V; v += GA_SAMPLE_THREADS) {
        const float zv = ga_z(nu[v], er[v], tau);
        zr[v] = zv;
        if (zv > best || at == 0x7fffffff) { best = zv; at = v; }        // a NaN never replaces; the first element always enters
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (oa != 0x7fffffff && (at == 0x7fffffff || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    if ((tid & 63) == 0) { sm[tid >> 6] = best; si[tid >> 6] = at; }
    __syncthreads();
    best = sm[0];
    at = si[0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
        if (si[w] != 0x7fffffff && (at == 0x7fffffff || sm[w] > best || (sm[w] == best && si[w] < at))) { best = sm[w]; at = si[w]; }
    float s = 0.f;
    for (int v = tid; v < V; v += GA_SAMPLE_THREADS) s += expf(zr[v] - best);          // this thread's own stores
    s = wave_sum(s);
    if ((tid & 63) == 0) ss[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        float t = ss[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) t += ss[w];
        idx[r] = at;
        zmax[r] = best;
        zsum[r] = t;
        if (hist_row) hist_row[r] = at;
        if (ids) ids[(int64_t)(r / K) * T + (T - K) + (r % K)] = (int64_t)at;
    }
}

// ---- ov_ga_token_grad ------------------------------------------------------------------------------------------------------------------
struct GaGradArgs {
    const ov_bf16* dX; const ov_bf16* W;
    const float* z; const float* zmax; const float* zsum;
    float* gy; float* parts;
    int R, V, D, nblk;
};

// Block (x, y): vocabulary rows [128 x, 128 x + 128), rows [64 y, 64 y + 64) of dX.  Wave w owns 32 vocabulary rows; one
// v_mfma_f32_32x32x16_bf16 per 16 columns of D and 32-row tile of dX: A = dX (row on the lane), B = W (vocabulary row on the lane),
// so an accumulator register holds one row r and the lanes of a half-wave 32 consecutive v -- 128-byte stores of gy.  Within a
// 64-column block of D, lane half h holds columns [32 h, 32 h + 32): MFMA step s multiplies columns 32 h + 8 s .. + 8 of both operands
// (the sum over D does not care in which order its terms meet), and a lane's four 16-byte loads of W are 64 contiguous bytes.
template <int NT>
__global__ __launch_bounds__(256) void ga_token_grad_kernel(const GaGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ga_lds[];
    __shared__ float wp[4][64];
    ov_bf16* xs = (ov_bf16*)ga_lds;
    const int D = a.D, pitch = D + GA_LDS_PAD, tid = threadIdx.x;
    const int r0 = blockIdx.y * 64;
    const int rows = min(NT * 32, a.R - r0);
    const int lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
    const int v = blockIdx.x * GA_SLAB + wave * 32 + r32;
    const ov_bf16* wrow = a.W + (int64_t)min(v, a.V - 1) * D + h * 32;       // past V: the last row again, its column never stored
    // The stream of W is bound by latency, not by issue: a lane asks for GA_AHEAD blocks (64 bytes each) at once and for the next
    // GA_AHEAD before it multiplies these, so 2 x 6 x 64 bytes per lane -- at D = 768 its whole row -- are in flight, the first of
    // them while dX is staged.  One wave per SIMD: the registers are there.
    const int nblocks = D >> 6;
    bf16x8_t cur[GA_AHEAD][4], nxt[GA_AHEAD][4];
#pragma unroll
    for (int j = 0; j < GA_AHEAD; ++j)
        if (j < nblocks)
#pragma unroll
            for (int s = 0; s < 4; ++s) nxt[j][s] = *(const bf16x8_t*)(wrow + j * 64 + 8 * s);
    // stage dX: 16 bytes per thread and turn, rows past R zero
    // (eight loads asked for before the first is written: one load per round trip would make the staging the longest part)
    const int cpr = D >> 3, chunks = NT * 32 * cpr;
    for (int i0 = tid; i0 < chunks; i0 += 256 * 8) {
        u32x4_t x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 256, row = i / cpr, ch = i - row * cpr;
            x[u] = u32x4_t{0u, 0u, 0u, 0u};
            if (i < chunks && row < rows) x[u] = *(const u32x4_t*)(a.dX + (int64_t)(r0 + row) * D + ch * 8);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 256, row = i / cpr, ch = i - row * cpr;
            if (i < chunks) *(u32x4_t*)(xs + row * pitch + ch * 8) = x[u];
        }
    }
    __syncthreads();
    const ov_bf16* xrow = xs + r32 * pitch + h * 32;
    f32x16_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int b0 = 0; b0 < nblocks; b0 += GA_AHEAD) {
#pragma unroll
        for (int j = 0; j < GA_AHEAD; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) cur[j][s] = nxt[j][s];
#pragma unroll
        for (int j = 0; j < GA_AHEAD; ++j)
            if (b0 + GA_AHEAD + j < nblocks)
#pragma unroll
                for (int s = 0; s < 4; ++s) nxt[j][s] = *(const bf16x8_t*)(wrow + (b0 + GA_AHEAD + j) * 64 + 8 * s);
#pragma unroll
        for (int j = 0; j < GA_AHEAD; ++j)
            if (b0 + j < nblocks)
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const bf16x8_t x = *(const bf16x8_t*)(xrow + t * 32 * pitch + (b0 + j) * 64 + 8 * s);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, cur[j][s], acc[t], 0, 0, 0);
                    }
    }
    // epilogue: register i of tile t is row 32 t + (i & 3) + 8 (i >> 2) + 4 h, this lane's column v
    const bool vin = v < a.V;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        // the tile's 16 z, zmax and zsum are asked for together, then used
        float zv[16], zm[16], zs[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = r0 + t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool in = vin && r < a.R;
            zv[i] = in ? a.z[(int64_t)r * a.V + v] : 0.f;
            zm[i] = in ? a.zmax[r] : 0.f;
            zs[i] = in ? a.zsum[r] : 1.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int rl = t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const int r = r0 + rl;
            float p = 0.f;
            if (vin && r < a.R) {
#pragma clang fp contract(off)
                a.gy[(int64_t)r * a.V + v] = acc[t][i];
                p = acc[t][i] * ga_ys(zv[i], zm[i], zs[i]);
            }
            // the 32 lanes of this half-wave: one fixed butterfly
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
            if (r32 == 0) wp[wave][rl] = p;
        }
    }
    __syncthreads();
    if (tid < NT * 32 && r0 + tid < a.R)
        a.parts[(int64_t)(r0 + tid) * a.nblk + blockIdx.x] = (wp[0][tid] + wp[1][tid]) + (wp[2][tid] + wp[3][tid]);
}

// ---- ov_ga_adam ------------------------------------------------------------------------------------------------------------------------
struct GaAdamArgs {
    const float* gy; const float* parts; float* normu; const float* z; const float* zmax; const float* zsum;
    float* ea; float* es; float* g;
    float tau, w, b2, w2, bc2_sqrt, eps, step_size;          // w = 1 - b1, w2 = 1 - b2
    int V, nblk;
};

// Block (x, y): columns [2048 x, 2048 x + 2048) of row y.  c_r: thread 0 adds the row's parts in ascending order.
__global__ __launch_bounds__(256) void ga_adam_kernel(const GaAdamArgs a) {
    __shared__ float c_sh;
    const int r = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) {
        const float* p = a.parts + (int64_t)r * a.nblk;
        float c = 0.f;
        for (int k = 0; k < a.nblk; ++k) c += p[k];
        c_sh = c;
    }
    __syncthreads();
    const float c = c_sh, zmax = a.zmax[r], zsum = a.zsum[r];
    const int v1 = min(a.V, (int)(blockIdx.x + 1) * 2048);
    for (int v = blockIdx.x * 2048 + tid; v < v1; v += 256) {
#pragma clang fp contract(off)
        const int64_t at = (int64_t)r * a.V + v;
        const float ys = ga_ys(a.z[at], zmax, zsum);
        const float g = (ys * (a.gy[at] - c)) / a.tau;
        if (a.g) a.g[at] = g;
        // torch.optim.Adam, _single_tensor_adam: lerp_ (ATen's two forms), mul_ + addcmul_, sqrt / bias_correction2_sqrt + eps, addcdiv_
        float ea = a.ea[at], es = a.es[at];
        const float d = g - ea;
        ea = a.w < 0.5f ? ea + a.w * d : g - d * (1.0f - a.w);
        es = es * a.b2 + (a.w2 * g) * g;
        const float denom = sqrtf(es) / a.bc2_sqrt + a.eps;
        a.normu[at] = a.normu[at] - a.step_size * (ea / denom);
        a.ea[at] = ea;
        a.es[at] = es;
    }
}

// ---- ov_ga_cosine_loss -----------------------------------------------------------------------------------------------------------------
struct GaCosArgs {
    const float* tx; const float* img;
    float* loss1; float* dtx; float* best; int* best_step; float* best_tx;
    int B, E, step;
    float eps;
};

// sum_k x[k] y[k] by one wave: lanes over k = lane, lane + 64, ... in ascending order, then wave_sum's butterfly
__device__ __forceinline__ float wave_dot(const float* __restrict__ x, const float* __restrict__ y, int E, int lane) {
    float s = 0.f;
    for (int k = lane; k < E; k += 64) s = fmaf(x[k], y[k], s);
    return wave_sum(s);
}

// One workgroup of 1024 threads.  norms and dots by one wave each, then per pair the two denominators, loss1[j] = -100 (sum_i cos_ji, i
// ascending) / B, their mean (j ascending), and dtx[j] = -100 / B^2 sum_i (img_i / (mt_j mi_i) - [|tx_j| > eps] dot_ji tx_j / (mt_j^2
// mi_i |tx_j|)), m = max(norm, eps), i ascending.
constexpr int GA_COS_THREADS = 1024;
__global__ __launch_bounds__(GA_COS_THREADS) void ga_cosine_kernel(const GaCosArgs a) {
    __shared__ float nt[GA_MAX_BATCH], ni[GA_MAX_BATCH], dots[GA_MAX_BATCH][GA_MAX_BATCH], den[GA_MAX_BATCH][GA_MAX_BATCH], l1[GA_MAX_BATCH];
    __shared__ int better;
    constexpr int NW = GA_COS_THREADS / 64;
    const int B = a.B, E = a.E, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = wave; q < 2 * B; q += NW) {
        const float* x = q < B ? a.tx + (int64_t)q * E : a.img + (int64_t)(q - B) * E;
        const float s = sqrtf(wave_dot(x, x, E, lane));
        if (lane == 0) (q < B ? nt[q] : ni[q - B]) = s;
    }
    for (int q = wave; q < B * B; q += NW) {
        const int j = q / B, i = q - j * B;
        const float s = wave_dot(a.tx + (int64_t)j * E, a.img + (int64_t)i * E, E, lane);
        if (lane == 0) dots[j][i] = s;
    }
    __syncthreads();
    for (int q = tid; q < B * B; q += GA_COS_THREADS) {
#pragma clang fp contract(off)
        const int j = q / B, i = q - j * B;
        den[j][i] = fmaxf(nt[j], a.eps) * fmaxf(ni[i], a.eps);
    }
    __syncthreads();
    if (tid < B) {
#pragma clang fp contract(off)
        float s = 0.f;
        for (int i = 0; i < B; ++i) s += dots[tid][i] / den[tid][i];
        const float l = -100.f * (s / (float)B);
        l1[tid] = l;
        a.loss1[tid] = l;
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int j = 0; j < B; ++j) s += l1[j];
        s = s / (float)B;
        const int b = s < a.best[0];
        if (b) { a.best[0] = s; a.best_step[0] = a.step; }
        better = b;
    }
    __syncthreads();
    const float coef = -100.f / ((float)B * (float)B);
    for (int q = tid; q < B * E; q += GA_COS_THREADS) {
#pragma clang fp contract(off)
        const int j = q / E, k = q - j * E;
        const float n = nt[j], mt = fmaxf(n, a.eps), x = a.tx[q];
        const bool live = n > a.eps;                         // clamp_min's gradient: none below the clamp
        float s = 0.f;
        for (int i = 0; i < B; ++i) {
            float t = a.img[(int64_t)i * E + k] / den[j][i];
            if (live) t -= (dots[j][i] * x) / ((den[j][i] * mt) * n);
            s += t;
        }
        a.dtx[q] = coef * s;
        if (better) a.best_tx[q] = x;
    }
}

int grid_of(int64_t items) {
    const int64_t want = (items + 255) / 256;
    return (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
}

OvPerDeviceOnce ga_grad_once[2];

}  // namespace

extern "C" int ov_ga_affine(const float* img, const float* mats, const float* mean, const float* stdv, void* out, int out_dtype, int B, int S,
                            ov_stream_t stream) {
    if (!img || !mats || !mean || !stdv || !out || B <= 0 || S <= 0) return OV_ERR_INVALID;
    if (out_dtype != OV_F32 && out_dtype != OV_BF16) return OV_ERR_INVALID;
    if (((uintptr_t)img | (uintptr_t)mats | (uintptr_t)mean | (uintptr_t)stdv | (uintptr_t)out) & 3) return OV_ERR_INVALID;
    if (S > GA_MAX_SIZE || B > GA_MAX_ROWS) return OV_ERR_UNSUPPORTED;
    const int64_t total = (int64_t)B * S * S;
    if (out_dtype == OV_BF16)
        hipLaunchKernelGGL(ga_affine_kernel<true>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, img, mats, mean, stdv, out, B, S);
    else
        hipLaunchKernelGGL(ga_affine_kernel<false>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, img, mats, mean, stdv, out, B, S);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_ga_sample(const float* normu, const float* e, float tau, int R, int V, int K, int T, float* z, int* idx, float* zmax,
                            float* zsum, int* history_row, int64_t* ids, ov_stream_t stream) {
    if (!normu || !e || !z || !idx || !zmax || !zsum || R <= 0 || V <= 0 || !(tau > 0.f)) return OV_ERR_INVALID;
    if (ids && (K <= 0 || T < K || R % K)) return OV_ERR_INVALID;
    if (((uintptr_t)normu | (uintptr_t)e | (uintptr_t)z | (uintptr_t)idx | (uintptr_t)zmax | (uintptr_t)zsum | (uintptr_t)history_row) & 3)
        return OV_ERR_INVALID;
    if ((uintptr_t)ids & 7) return OV_ERR_INVALID;
    if (R > GA_MAX_ROWS) return OV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ga_sample_kernel, dim3(R), dim3(GA_SAMPLE_THREADS), 0, (hipStream_t)stream, normu, e, tau, V, ids ? K : 1, ids ? T : 1,
                       z, idx, zmax, zsum, history_row, ids);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_ga_parts_blocks(int V) { return V > 0 ? (V + GA_SLAB - 1) / GA_SLAB : 0; }

extern "C" int ov_ga_token_grad(const ov_bf16* dX, const ov_bf16* W, const float* z, const float* zmax, const float* zsum, int R, int V, int D,
                                float* gy, float* parts, ov_stream_t stream) {
    if (!dX || !W || !z || !zmax || !zsum || !gy || !parts || R <= 0 || V <= 0 || D <= 0) return OV_ERR_INVALID;
    if (((uintptr_t)dX | (uintptr_t)W) & 15) return OV_ERR_INVALID;
    if (((uintptr_t)z | (uintptr_t)zmax | (uintptr_t)zsum | (uintptr_t)gy | (uintptr_t)parts) & 3) return OV_ERR_INVALID;
    const int nt = R > 32 ? 2 : 1;
    const size_t lds = (size_t)nt * 32 * (D + GA_LDS_PAD) * sizeof(ov_bf16);
    if (D % 64 || R > GA_MAX_ROWS || lds > 156 * 1024) return OV_ERR_UNSUPPORTED;
    GaGradArgs a;
    a.dX = dX; a.W = W; a.z = z; a.zmax = zmax; a.zsum = zsum; a.gy = gy; a.parts = parts;
    a.R = R; a.V = V; a.D = D; a.nblk = ov_ga_parts_blocks(V);
    void (*kernel)(GaGradArgs) = nt == 2 ? ga_token_grad_kernel<2> : ga_token_grad_kernel<1>;
    const int dev = ov_current_device();
    if (ga_grad_once[nt - 1].need(dev)) {
        const hipError_t err = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
        if (err != hipSuccess) return ov_hip(err);
        ga_grad_once[nt - 1].mark(dev);
    }
    hipLaunchKernelGGL(kernel, dim3(a.nblk, (R + 63) / 64), dim3(256), lds, (hipStream_t)stream, a);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_ga_adam(const float* gy, const float* parts, float* normu, const float* z, const float* zmax, const float* zsum, float tau,
                          int R, int V, float* exp_avg, float* exp_avg_sq, double lr, double b1, double b2, double eps, double bias_correction1,
                          double bias_correction2, float* g, ov_stream_t stream) {
    if (!gy || !parts || !normu || !z || !zmax || !zsum || !exp_avg || !exp_avg_sq || R <= 0 || V <= 0 || !(tau > 0.f)) return OV_ERR_INVALID;
    if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps >= 0.0) || !(bias_correction1 > 0.0) || !(bias_correction2 > 0.0))
        return OV_ERR_INVALID;
    if (((uintptr_t)gy | (uintptr_t)parts | (uintptr_t)normu | (uintptr_t)z | (uintptr_t)zmax | (uintptr_t)zsum | (uintptr_t)exp_avg |
         (uintptr_t)exp_avg_sq | (uintptr_t)g) & 3)
        return OV_ERR_INVALID;
    if (R > GA_MAX_ROWS) return OV_ERR_UNSUPPORTED;
    GaAdamArgs a;
    a.gy = gy; a.parts = parts; a.normu = normu; a.z = z; a.zmax = zmax; a.zsum = zsum; a.ea = exp_avg; a.es = exp_avg_sq; a.g = g;
    a.tau = tau; a.w = (float)(1.0 - b1); a.b2 = (float)b2; a.w2 = (float)(1.0 - b2); a.bc2_sqrt = (float)sqrt(bias_correction2);
    a.eps = (float)eps; a.step_size = (float)(lr / bias_correction1);
    a.V = V; a.nblk = ov_ga_parts_blocks(V);
    hipLaunchKernelGGL(ga_adam_kernel, dim3((V + 2047) / 2048, R), dim3(256), 0, (hipStream_t)stream, a);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_ga_cosine_loss(const float* tx, const float* img, int B, int E, int step, float* loss1_row, float* dtx, float* best,
                                 int* best_step, float* best_tx, ov_stream_t stream) {
    if (!tx || !img || !loss1_row || !dtx || !best || !best_step || !best_tx || B <= 0 || E <= 0 || step < 0) return OV_ERR_INVALID;
    if (((uintptr_t)tx | (uintptr_t)img | (uintptr_t)loss1_row | (uintptr_t)dtx | (uintptr_t)best | (uintptr_t)best_step | (uintptr_t)best_tx) & 3)
        return OV_ERR_INVALID;
    if (B > GA_MAX_BATCH) return OV_ERR_UNSUPPORTED;
    GaCosArgs a;
    a.tx = tx; a.img = img; a.loss1 = loss1_row; a.dtx = dtx; a.best = best; a.best_step = best_step; a.best_tx = best_tx;
    a.B = B; a.E = E; a.step = step; a.eps = 1e-8f;
    hipLaunchKernelGGL(ga_cosine_kernel, dim3(1), dim3(GA_COS_THREADS), 0, (hipStream_t)stream, a);
    OV_LAUNCH_CHECK();
    return OV_OK;
}
