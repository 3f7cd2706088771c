// vizloop.hip — the inner loop of ov-feature-visualization.py around the MLP-feature objective (gfx950).
//
// The script optimises an image img [N,3,S,S] (fp32) for steps + 1 iterations of (ov-feature-visualization.py:120-136, :214-215)
//     aug   = Jitter(Tile(1)(GaussianNoise(ColorJitter(RepeatBatch(R)(img)))))         cliptoolsoptimized.py:1482-1580
//     loss  = c_feat * (-(1/B^2) sum_b m_b(aug)) + c_tv * TotalVariation(aug)           :719-730, :840-847
//     img   = Clip(Adamax(img, d loss / d img))                                         :1432, torch.optim.Adamax + CosineAnnealingLR
// with B = R N rows, row b = r N + n.  Everything but m_b (visualize._FeatureFn) and the patch GEMM is here, four entry points:
//
//   ov_viz_augment            aug[b,c,y,x] = ((img[n,c,(y-off1) mod S,(x-off2) mod S] - mean[b,c]) / std[b,c]) + noise[b,c], fp32 in that
//                             order with a true division, written as the conv1 operand rows (bf16, ov_im2col_patches' layout) and,
//                             on request, as fp32 [B,3,S,S]: no repeat() copies, no roll, no separate im2col
//   ov_viz_tv                 the 4 * 3B plane norms of the x / y / two diagonal difference fields of aug, and their scalar
//   ov_viz_augment_backward   dimg[n,c,y',x'] = sum_r d_aug[b,c,(y'+off1) mod S,(x'+off2) mod S] / std[b,c], r ascending, with
//                             d_aug = fp32(dcols entry) + c_tv * (TV gradient: +-diff / (norm 3B), 0 for a plane of norm 0); one
//                             row (loss, feature term, tv term) of the device history
//   ov_adamax_clip_step       torch's _single_tensor_adamax (lerp, max(b2 ei, |g| + eps), addcdiv) and the clamp, one pass
//
// All four are bandwidth- and launch-bound: one thread per 8 contiguous elements and 16-byte stores throughout.  Loads are 16 bytes
// wide in ov_viz_tv, in ov_adamax_clip_step and, when P % 8 == 0 and the column roll is a multiple of 4, in ov_viz_augment; the
// backward gathers a 3 x 3 neighbourhood of aug and single bf16 dcols entries per pixel through the roll and reads them as scalars
// (cache-resident: aug is 4.8 MB at L/14, B = 8).  No atomics -- every sum runs in one fixed order, so a step is reproducible bit for
// bit -- and no scratch.
#include "common.h"
#include <math.h>

namespace {

constexpr int VIZ_MAX_BATCH = 4096, VIZ_MAX_SIZE = 1024;

__device__ __forceinline__ int wrap_add(int a, int o, int S) {      // (a + o) mod S for 0 <= a, o < S
    const int v = a + o;
    return v >= S ? v - S : v;
}

// mean | std | noise of the step, each [3B] (row b, channel c at b * 3 + c)
struct VizTab {
    const float* t;
    int B3;
    __device__ __forceinline__ float mean(int i) const { return t[i]; }
    __device__ __forceinline__ float stdv(int i) const { return t[B3 + i]; }
    __device__ __forceinline__ float noise(int i) const { return t[2 * B3 + i]; }
};

__device__ __forceinline__ float augment_one(float v, float m, float s, float z) {
#pragma clang fp contract(off)
    return ((v - m) / s) + z;
}

// One work item per 8 operand columns of a conv1 row (ov_im2col_patches' layout: column c P^2 + ii P + jj, zero past 3 P^2).
// P8 (P % 8 == 0): the 8 columns are 8 contiguous pixels of one patch row, so channel and row are found once and the fp32 copy
// leaves as two 16-byte stores.
template <bool P8>
__global__ __launch_bounds__(256) void viz_augment_kernel(const float* __restrict__ img, const VizTab tab, ov_bf16* __restrict__ cols,
                                                          float* __restrict__ aug, int N, int S, int P, int g, int Kpad, int o1, int o2,
                                                          int64_t total) {
    const int cpr = Kpad >> 3, G = g * g, PP = P * P, K = 3 * PP;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int ch = (int)(i - row * cpr);
        const int b = (int)(row / G), pr = (int)(row - (int64_t)b * G);
        const int py = pr / g, px = pr - py * g, n = b % N;
        float v[8];
        if (P8) {
            const int k = ch * 8;
            if (k < K) {
                const int c = k / PP, rem = k - c * PP;
                const int ii = rem / P, jj = rem - ii * P;
                const int y = py * P + ii, x = px * P + jj;
                const int ys = wrap_add(y, S - o1, S);
                int xs = wrap_add(x, S - o2, S);
                const float* src = img + ((int64_t)(n * 3 + c) * S + ys) * S;
                const float m = tab.mean(b * 3 + c), s = tab.stdv(b * 3 + c), z = tab.noise(b * 3 + c);
                float in[8];
                if ((xs & 3) == 0) {              // S % 8 == 0 here: a roll by a multiple of 4 leaves two aligned quads, neither split by the seam
                    const f32x4_t lo = *(const f32x4_t*)(src + xs), hi = *(const f32x4_t*)(src + (xs + 4 == S ? 0 : xs + 4));
                    in[0] = lo[0]; in[1] = lo[1]; in[2] = lo[2]; in[3] = lo[3];
                    in[4] = hi[0]; in[5] = hi[1]; in[6] = hi[2]; in[7] = hi[3];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        in[e] = src[xs];
                        xs = xs + 1 == S ? 0 : xs + 1;
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = augment_one(in[e], m, s, z);
                if (aug) {
                    f32x4_t* dst = (f32x4_t*)(aug + ((int64_t)(b * 3 + c) * S + y) * S + x);
                    dst[0] = f32x4_t{v[0], v[1], v[2], v[3]};
                    dst[1] = f32x4_t{v[4], v[5], v[6], v[7]};
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = ch * 8 + e;
                float a = 0.f;
                if (k < K) {
                    const int c = k / PP, rem = k - c * PP;
                    const int ii = rem / P, jj = rem - ii * P;
                    const int y = py * P + ii, x = px * P + jj;
                    const int ys = wrap_add(y, S - o1, S), xs = wrap_add(x, S - o2, S);
                    a = augment_one(img[((int64_t)(n * 3 + c) * S + ys) * S + xs], tab.mean(b * 3 + c), tab.stdv(b * 3 + c),
                                    tab.noise(b * 3 + c));
                    if (aug) aug[((int64_t)(b * 3 + c) * S + y) * S + x] = a;
                }
                v[e] = a;
            }
        }
        *(u32x4_t*)(cols + row * Kpad + ch * 8) =
            u32x4_t{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
    }
}

// v[k] summed over the block's 256 threads, k = 0..3: lanes by wave_sum's butterfly, then the four waves as (0 + 1) + (2 + 3).
// The sums are in every thread afterwards; red is free again after the call.
__device__ __forceinline__ void block_sum4(float (&v)[4], float (*red)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// row[x0 .. x0 + 8] (9 values; 0 past the row's end): 16-byte loads when the rows are 16-byte aligned (S % 4 == 0, x0 % 8 == 0)
__device__ __forceinline__ void load9(const float* __restrict__ row, int x0, int S, bool vec, float (&v)[9]) {
    if (vec) {
        const f32x4_t a = *(const f32x4_t*)(row + x0);
        const f32x4_t b = x0 + 4 < S ? *(const f32x4_t*)(row + x0 + 4) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
        v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = x0 + e < S ? row[x0 + e] : 0.f;
    }
    v[8] = x0 + 8 < S ? row[x0 + 8] : 0.f;
}

// One block per plane (b, c) of aug: the sums of squares of x[y][x+1] - x[y][x], x[y+1][x] - x[y][x], x[y+1][x+1] - x[y][x] and
// x[y+1][x] - x[y][x+1] (BaseTotalVariation's four fields; nothing is differenced across the plane's border), a thread per 8
// contiguous pixels and the row below them.  norms[dir * B3 + plane] = sqrt(sum).
__global__ __launch_bounds__(256) void viz_tv_kernel(const float* __restrict__ aug, float* __restrict__ norms, int S, int B3) {
    __shared__ float red[4][4];
    const int plane = blockIdx.x, ngx = (S + 7) >> 3;
    const bool vec = (S & 3) == 0;
    const float* base = aug + (int64_t)plane * S * S;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int item = threadIdx.x; item < S * ngx; item += 256) {
        const int y = item / ngx, x0 = (item - y * ngx) << 3;
        const bool below = y + 1 < S;
        float cur[9], nxt[9];
        load9(base + (int64_t)y * S, x0, S, vec, cur);
        if (below) load9(base + (int64_t)(y + 1) * S, x0, S, vec, nxt);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool here = x0 + e < S, right = x0 + e + 1 < S;
            if (here && right) { const float d = cur[e + 1] - cur[e]; acc[0] = fmaf(d, d, acc[0]); }
            if (here && below) { const float d = nxt[e] - cur[e]; acc[1] = fmaf(d, d, acc[1]); }
            if (right && below) {
                const float d1 = nxt[e + 1] - cur[e], d2 = nxt[e] - cur[e + 1];
                acc[2] = fmaf(d1, d1, acc[2]);
                acc[3] = fmaf(d2, d2, acc[3]);
            }
        }
    }
    block_sum4(acc, red);
    if (threadIdx.x < 4) norms[(int64_t)threadIdx.x * B3 + plane] = sqrtf(acc[threadIdx.x]);
}

// tv = (mean_planes norm_x + mean_planes norm_y + mean_planes norm_d1 + mean_planes norm_d2) * scale, by one whole block
__device__ __forceinline__ float tv_total(const float* __restrict__ norms, int B3, float scale, float (*red)[4]) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = threadIdx.x; p < B3; p += 256)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += norms[(int64_t)k * B3 + p];
    block_sum4(s, red);
    const float n = (float)B3;
    return (((s[0] / n + s[1] / n) + s[2] / n) + s[3] / n) * scale;
}

__global__ __launch_bounds__(256) void viz_tv_total_kernel(const float* __restrict__ norms, int B3, float scale, float* __restrict__ tv) {
    __shared__ float red[4][4];
    const float t = tv_total(norms, B3, scale, red);
    if (threadIdx.x == 0) *tv = t;
}

struct VizBwdArgs {
    const ov_bf16* dcols; int64_t ldc;
    const float* aug; const float* norms; VizTab tab;
    const float* m; float* hist; float* dimg;
    int N, R, S, P, g, o1, o2;
    float c_feat, c_tv, tv_scale, tv_coef;         // tv_coef = c_tv * tv_scale / (3B): the factor of diff / norm in d_aug
    int64_t total;
};

// One thread per 8 contiguous pixels of dimg.  Pixel (y', x') of image n reads aug pixel (ya, xa) = ((y' + off1) mod S, (x' + off2)
// mod S) of the rows b = r N + n: the dcols entry of that pixel and the eight differences it is an end of (each formed as the
// forward formed it, so bitwise the forward's), scaled by 1 / norm of their field.
__global__ __launch_bounds__(256) void viz_augment_bwd_kernel(const VizBwdArgs a) {
    __shared__ float red[4][4];
    const int S = a.S, P = a.P, N = a.N, B = a.R * N, B3 = 3 * B, G = a.g * a.g, ngx = (S + 7) >> 3;
    if (blockIdx.x == 0 && a.hist != nullptr) {            // the history row: block-uniform branch
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int b = threadIdx.x; b < B; b += 256) s[0] += a.m[b];
        block_sum4(s, red);
        const float tv = tv_total(a.norms, B3, a.tv_scale, red);
        if (threadIdx.x == 0) {
            const float feat = a.c_feat * (-s[0] / ((float)B * (float)B)), tvt = a.c_tv * tv;
            a.hist[0] = feat + tvt;
            a.hist[1] = feat;
            a.hist[2] = tvt;
        }
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * blockDim.x) {
        const int gx = (int)(i % ngx);
        const int64_t line = i / ngx;                       // (n * 3 + c) * S + y'
        const int yp = (int)(line % S), nc = (int)(line / S);
        const int n = nc / 3, c = nc - n * 3, x0 = gx << 3;
        const int ya = wrap_add(yp, a.o1, S);
        const int py = ya / P, ii = ya - py * P;
        const bool up = ya >= 1, down = ya + 1 < S;
        // where each of the 8 pixels lands in aug and in a dcols row: the same for every r
        int xa[8];
        int64_t col[8];
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[e] = 0.f;
            xa[e] = x0 + e < S ? wrap_add(x0 + e, a.o2, S) : -1;
            const int px = xa[e] / P, jj = xa[e] - px * P;
            col[e] = (int64_t)(py * a.g + px) * a.ldc + c * P * P + ii * P + jj;
        }
        for (int r = 0; r < a.R; ++r) {                     // ascending r: the order of every pixel's sum
            const int b = r * N + n, plane = b * 3 + c;
            const float* arow = a.aug + ((int64_t)plane * S + ya) * S;
            const ov_bf16* drow = a.dcols + (int64_t)b * G * a.ldc;
            const float sd = a.tab.stdv(plane);
            float inv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float nk = a.norms[(int64_t)k * B3 + plane];
                inv[k] = nk > 0.f ? a.tv_coef / nk : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (xa[e] < 0) continue;
                const float* q = arow + xa[e];
                const bool left = xa[e] >= 1, right = xa[e] + 1 < S;
                const float v = q[0];
                float t = 0.f;
                {
#pragma clang fp contract(off)
                    if (left) t += (v - q[-1]) * inv[0];
                    if (right) t -= (q[1] - v) * inv[0];
                    if (up) t += (v - q[-S]) * inv[1];
                    if (down) t -= (q[S] - v) * inv[1];
                    if (up && left) t += (v - q[-S - 1]) * inv[2];
                    if (down && right) t -= (q[S + 1] - v) * inv[2];
                    if (up && right) t += (v - q[-S + 1]) * inv[3];
                    if (down && left) t -= (q[S - 1] - v) * inv[3];
                    acc[e] += (bf16_bits_to_f32(drow[col[e]]) + t) / sd;
                }
            }
        }
        float* dst = a.dimg + line * S + x0;
        if ((S & 3) == 0) {
            *(f32x4_t*)dst = f32x4_t{acc[0], acc[1], acc[2], acc[3]};
            if (x0 + 4 < S) *(f32x4_t*)(dst + 4) = f32x4_t{acc[4], acc[5], acc[6], acc[7]};
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (x0 + e < S) dst[e] = acc[e];
        }
    }
}

struct AdamaxArgs {
    float* p; const float* g; float* ea; float* ei;
    int64_t n;
    float w, b2, eps, clr, lo, hi;            // w = 1 - b1
};

__device__ __forceinline__ void adamax_one(float& p, float g, float& ea, float& ei, const AdamaxArgs& a) {
#pragma clang fp contract(off)
    // exp_avg.lerp_(grad, 1 - beta1) with ATen's two forms: from the start below weight 0.5, from the end at 0.5 (the default
    // beta1 = 0.5) and above
    const float d = g - ea;
    ea = a.w < 0.5f ? ea + a.w * d : g - d * (1.0f - a.w);
    ei = fmaxf(ei * a.b2, fabsf(g) + a.eps);             // torch.maximum(exp_inf.mul_(beta2), grad.abs().add_(eps))
    const float q = p - a.clr * (ea / ei);               // param.addcdiv_(exp_avg, exp_inf, value=-clr)
    p = fminf(fmaxf(q, a.lo), a.hi);                     // Clip
}

__global__ __launch_bounds__(256) void adamax_clip_kernel(const AdamaxArgs a) {
    const int64_t n4 = a.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4_t pv = ((f32x4_t*)a.p)[i], gv = ((const f32x4_t*)a.g)[i], av = ((f32x4_t*)a.ea)[i], iv = ((f32x4_t*)a.ei)[i];
        float p[4] = {pv[0], pv[1], pv[2], pv[3]}, ea[4] = {av[0], av[1], av[2], av[3]}, ei[4] = {iv[0], iv[1], iv[2], iv[3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) adamax_one(p[e], gv[e], ea[e], ei[e], a);
        ((f32x4_t*)a.p)[i] = f32x4_t{p[0], p[1], p[2], p[3]};
        ((f32x4_t*)a.ea)[i] = f32x4_t{ea[0], ea[1], ea[2], ea[3]};
        ((f32x4_t*)a.ei)[i] = f32x4_t{ei[0], ei[1], ei[2], ei[3]};
    }
    if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {
        const int64_t i = (n4 << 2) + threadIdx.x;
        adamax_one(a.p[i], a.g[i], a.ea[i], a.ei[i], a);
    }
}

int grid_of(int64_t items) {
    const int64_t want = (items + 255) / 256;
    return (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
}

// the shape checks the three image-shaped entry points share: OV_OK, or the status to return
int viz_shape_status(int N, int R, int S, int P) {
    if (N <= 0 || R <= 0 || S <= 0 || P <= 0) return OV_ERR_INVALID;
    if (S % P != 0 || S < P || S > VIZ_MAX_SIZE || (int64_t)R * N > VIZ_MAX_BATCH) return OV_ERR_UNSUPPORTED;
    return OV_OK;
}

int norm_offset(int off, int S) { return ((off % S) + S) % S; }

}  // namespace

extern "C" int ov_viz_augment(const float* img, const float* table, int N, int R, int S, int P, int Kpad, int off1, int off2, ov_bf16* cols,
                              float* aug, ov_stream_t stream) {
    if (!img || !table || !cols) return OV_ERR_INVALID;
    // the table is read one float at a time (a step's row of a packed [steps + 1, 3, 3B] table starts at any multiple of 4 bytes)
    if ((((uintptr_t)img | (uintptr_t)cols | (uintptr_t)aug) & 15) || ((uintptr_t)table & 3)) return OV_ERR_INVALID;
    const int st = viz_shape_status(N, R, S, P);
    if (st != OV_OK) return st;
    if (Kpad < 3 * P * P || Kpad % 8) return OV_ERR_INVALID;
    const int B = R * N, g = S / P;
    const int64_t total = (int64_t)B * g * g * (Kpad / 8);
    const VizTab tab{table, 3 * B};
    if (P % 8 == 0)
        hipLaunchKernelGGL(viz_augment_kernel<true>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, img, tab, cols, aug, N, S, P, g,
                           Kpad, norm_offset(off1, S), norm_offset(off2, S), total);
    else
        hipLaunchKernelGGL(viz_augment_kernel<false>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, img, tab, cols, aug, N, S, P, g,
                           Kpad, norm_offset(off1, S), norm_offset(off2, S), total);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_viz_tv(const float* aug, int B, int S, int size, float* norms, float* tv, ov_stream_t stream) {
    if (!aug || !norms || B <= 0 || S <= 0 || size <= 0) return OV_ERR_INVALID;
    if (S > VIZ_MAX_SIZE || B > VIZ_MAX_BATCH) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)aug | (uintptr_t)norms) & 15) return OV_ERR_INVALID;
    hipLaunchKernelGGL(viz_tv_kernel, dim3(3 * B), dim3(256), 0, (hipStream_t)stream, aug, norms, S, 3 * B);
    OV_LAUNCH_CHECK();
    if (tv) {
        const float scale = (float)((double)S * S / ((double)size * size));
        hipLaunchKernelGGL(viz_tv_total_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)norms, 3 * B, scale, tv);
        OV_LAUNCH_CHECK();
    }
    return OV_OK;
}

extern "C" int ov_viz_augment_backward(const ov_bf16* dcols, int64_t ldc, const float* aug, const float* norms, const float* table,
                                       const float* m, int N, int R, int S, int P, int off1, int off2, int size, float c_feat, float c_tv,
                                       float* dimg, float* history_row, ov_stream_t stream) {
    if (!dcols || !aug || !norms || !table || !dimg || size <= 0) return OV_ERR_INVALID;
    if ((history_row != nullptr) != (m != nullptr)) return OV_ERR_INVALID;
    if ((((uintptr_t)aug | (uintptr_t)norms | (uintptr_t)dimg) & 15) || (((uintptr_t)table | (uintptr_t)m | (uintptr_t)history_row) & 3))
        return OV_ERR_INVALID;
    const int st = viz_shape_status(N, R, S, P);
    if (st != OV_OK) return st;
    if (ldc < 3 * P * P) return OV_ERR_INVALID;
    const int B = R * N;
    VizBwdArgs a;
    a.dcols = dcols; a.ldc = ldc; a.aug = aug; a.norms = norms; a.tab = VizTab{table, 3 * B};
    a.m = m; a.hist = history_row; a.dimg = dimg;
    a.N = N; a.R = R; a.S = S; a.P = P; a.g = S / P; a.o1 = norm_offset(off1, S); a.o2 = norm_offset(off2, S);
    a.c_feat = c_feat; a.c_tv = c_tv;
    const double scale = (double)S * S / ((double)size * size);
    a.tv_scale = (float)scale;
    a.tv_coef = (float)((double)c_tv * scale / (3.0 * B));
    a.total = (int64_t)N * 3 * S * ((S + 7) / 8);
    hipLaunchKernelGGL(viz_augment_bwd_kernel, dim3(grid_of(a.total)), dim3(256), 0, (hipStream_t)stream, a);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_adamax_clip_step(float* img, const float* dimg, float* ea, float* ei, int64_t n, double clr, double b1, double b2,
                                   double eps, float lo, float hi, ov_stream_t stream) {
    if (!img || !dimg || !ea || !ei || n <= 0) return OV_ERR_INVALID;
    if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps >= 0.0) || !(lo <= hi)) return OV_ERR_INVALID;
    if (((uintptr_t)img | (uintptr_t)dimg | (uintptr_t)ea | (uintptr_t)ei) & 15) return OV_ERR_INVALID;
    AdamaxArgs a;
    a.p = img; a.g = dimg; a.ea = ea; a.ei = ei; a.n = n;
    a.w = (float)(1.0 - b1); a.b2 = (float)b2; a.eps = (float)eps; a.clr = (float)clr; a.lo = lo; a.hi = hi;
    hipLaunchKernelGGL(adamax_clip_kernel, dim3(grid_of((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    OV_LAUNCH_CHECK();
    return OV_OK;
}
