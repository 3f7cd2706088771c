// embed.hip — the memory-bound glue kernels either side of the block stack (gfx950).
//
//   ov_im2col_patches  operand gather for conv1 (k = s = P, no bias)      open_clip/transformer.py:469,610-612
//   ov_cls_rows        class_embedding concat + pos-emb row 0             transformer.py:615-617
//   ov_mean_pool       _global_pool 'avg' (cls excluded) / 'tok'          transformer.py:599-603
//   ov_text_embed      token_embedding(text) + positional_embedding      model.py:272-274
//   ov_gather_rows     text_global_pool 'last' / 'first'                  transformer.py:655-658
//   ov_token_argmax + ov_gather_rows_at   text_global_pool 'argmax' (the EOT row of each caption)
//   ov_convert         dtype casts (.to(cast_dtype))
//   ov_l2norm          F.normalize(x, dim=-1)                             model.py:267,284
// Patch dropout (PatchDropout, transformer.py:49-86: the image keeps K of its G patch tokens, in the order of keep[b, :]):
//   ov_im2col_patches_keep         the conv1 operand rows of the kept patches only (+ their pos-emb rows, for ov_vision_embed_keep)
//   ov_patch_keep_inverse          keep [B, K] -> inv [B, G] (j or -1), duplicate / out-of-range indices raise a device flag
//   ov_patch_keep_assemble         fp32 tokens [B, 1+K, D]: cls + pos[0], then patch rows + pos[1 + keep]
//   ov_patch_keep_assemble_backward  dpos / dcls as fixed-order sums over the batch (no atomics), dY rows of the patch GEMM
//   ov_col2im_patches_keep         pixel gradient: kept patches' rows back into the image, dropped patches 0
// All are 16-byte-per-lane streaming kernels; none re-reads its input.
#include "common.h"

namespace {

// columns ch*8 .. ch*8+7 of the conv1 operand row of patch (py, px) of image b: (c, ii, jj) order of the weight's flattening,
// zero past 3 P^2, rounded to bf16 once
template <bool IMG_F32>
__device__ __forceinline__ u32x4_t im2col_chunk(const void* __restrict__ img, int b, int py, int px, int ch, int S, int P) {
    const int PP = P * P, K = 3 * PP;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = ch * 8 + e;
        float x = 0.f;
        if (k < K) {
            const int c = k / PP, rem = k - c * PP;
            const int ii = rem / P, jj = rem - ii * P;
            const int64_t src = (((int64_t)b * 3 + c) * S + (py * P + ii)) * S + (px * P + jj);
            x = IMG_F32 ? ((const float*)img)[src] : bf16_bits_to_f32(((const ov_bf16*)img)[src]);
        }
        v[e] = x;
    }
    return u32x4_t{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
}

template <bool IMG_F32>
__global__ __launch_bounds__(256) void im2col_kernel(const void* __restrict__ img, ov_bf16* __restrict__ out,
                                                     int B, int S, int P, int g, int Kpad, int64_t total) {
    // one thread per 8 output columns
    const int cpr = Kpad >> 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int ch = (int)(i - row * cpr);
        const int b = (int)(row / (g * g));
        const int pr = (int)(row - (int64_t)b * g * g);
        const int py = pr / g, px = pr - py * g;
        *(u32x4_t*)(out + row * Kpad + ch * 8) = im2col_chunk<IMG_F32>(img, b, py, px, ch, S, P);
    }
}

// keep index of output row `row` (= b * K + j), clamped into [0, G) so that no read leaves the image; an index outside it raises *err
__device__ __forceinline__ int keep_index(const int* __restrict__ keep, int64_t row, int G, int* __restrict__ err) {
    int id = keep[row];
    if (id < 0 || id >= G) {
        if (err) *err = 1;
        id = id < 0 ? 0 : G - 1;
    }
    return id;
}

// Work items [0, ncols): one per 8 operand columns of a kept row (im2col_kernel's arithmetic); [ncols, total): one per 8 columns of the
// kept row's positional-embedding row pos[1 + keep[b, j]] (bf16, for the patch GEMM's residual epilogue), when posk is given.
template <bool IMG_F32>
__global__ __launch_bounds__(256) void im2col_keep_kernel(const void* __restrict__ img, const int* __restrict__ keep, ov_bf16* __restrict__ out,
                                                          const ov_bf16* __restrict__ pos, ov_bf16* __restrict__ posk, int S, int P, int g,
                                                          int K, int Kpad, int D, int* __restrict__ err, int64_t ncols, int64_t total) {
    const int cpr = Kpad >> 3, dpr = D >> 3, G = g * g;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ncols) {
            const int64_t row = i / cpr;
            const int ch = (int)(i - row * cpr);
            const int b = (int)(row / K);
            const int id = keep_index(keep, row, G, err);
            const int py = id / g, px = id - py * g;
            *(u32x4_t*)(out + row * Kpad + ch * 8) = im2col_chunk<IMG_F32>(img, b, py, px, ch, S, P);
        } else {
            const int64_t k = i - ncols;
            const int64_t row = k / dpr;
            const int ch = (int)(k - row * dpr);
            const int id = keep_index(keep, row, G, nullptr);
            *(u32x4_t*)(posk + row * D + ch * 8) = *(const u32x4_t*)(pos + (int64_t)(1 + id) * D + ch * 8);
        }
    }
}

// One workgroup per image: inv[b, keep[b, j]] = j, -1 where no j points.  A duplicate leaves one of its writers unconfirmed in the
// second pass; both cases raise *err.
__global__ __launch_bounds__(256) void keep_inverse_kernel(const int* __restrict__ keep, int* __restrict__ inv, int K, int G,
                                                           int* __restrict__ err) {
    extern __shared__ int sinv[];
    const int b = blockIdx.x;
    const int* kb = keep + (int64_t)b * K;
    int bad = 0;
    for (int t = threadIdx.x; t < G; t += blockDim.x) sinv[t] = -1;
    __syncthreads();
    for (int j = threadIdx.x; j < K; j += blockDim.x) {
        const int id = kb[j];
        if (id >= 0 && id < G) sinv[id] = j;
        else bad = 1;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < K; j += blockDim.x) {
        const int id = kb[j];
        if (id >= 0 && id < G && sinv[id] != j) bad = 1;
    }
    for (int t = threadIdx.x; t < G; t += blockDim.x) inv[(int64_t)b * G + t] = sinv[t];
    if (bad && err) *err = 1;
}

// x[b, 0] = cls + pos[0], x[b, 1 + j] = y[b * K + j] + pos[1 + keep[b, j]]: one fp32 add per element (what
// torch.cat([cls, y]) + pos computes); one thread per 8 columns of an output row
__global__ __launch_bounds__(256) void keep_assemble_kernel(const ov_bf16* __restrict__ y, int64_t ldy, const float* __restrict__ cls,
                                                            const float* __restrict__ pos, const int* __restrict__ keep, float* __restrict__ x,
                                                            int K, int G, int D, int64_t total) {
    const int dpr = D >> 3, L = K + 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / dpr;
        const int ch = (int)(i - row * dpr);
        const int64_t b = row / L;
        const int t = (int)(row - b * L);
        float v[8];
        if (t == 0) {
            const float4 c0 = *(const float4*)(cls + ch * 8), c1 = *(const float4*)(cls + ch * 8 + 4);
            const float4 p0 = *(const float4*)(pos + ch * 8), p1 = *(const float4*)(pos + ch * 8 + 4);
            v[0] = c0.x + p0.x; v[1] = c0.y + p0.y; v[2] = c0.z + p0.z; v[3] = c0.w + p0.w;
            v[4] = c1.x + p1.x; v[5] = c1.y + p1.y; v[6] = c1.z + p1.z; v[7] = c1.w + p1.w;
        } else {
            const int64_t r = b * K + (t - 1);
            const int id = keep_index(keep, r, G, nullptr);
            const u32x4_t w = *(const u32x4_t*)(y + r * ldy + ch * 8);
            const float* pr = pos + (int64_t)(1 + id) * D + ch * 8;
            const float4 p0 = *(const float4*)pr, p1 = *(const float4*)(pr + 4);
            v[0] = bf16lo_to_f32(w[0]) + p0.x; v[1] = bf16hi_to_f32(w[0]) + p0.y;
            v[2] = bf16lo_to_f32(w[1]) + p0.z; v[3] = bf16hi_to_f32(w[1]) + p0.w;
            v[4] = bf16lo_to_f32(w[2]) + p1.x; v[5] = bf16hi_to_f32(w[2]) + p1.y;
            v[6] = bf16lo_to_f32(w[3]) + p1.z; v[7] = bf16hi_to_f32(w[3]) + p1.w;
        }
        float4* q = (float4*)(x + row * D + ch * 8);
        q[0] = make_float4(v[0], v[1], v[2], v[3]);
        q[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
}

// Work items [0, npos): one per 4 columns of a positional row p in [0, 1 + G): dpos[p] = sum over b = 0, 1, ..., B-1 (in that order)
// of the gradient row that p fed (row 0 for p = 0, row 1 + inv[b, p - 1] when that patch was kept); exactly 0 when no image kept it.
// dcls = dpos[0].  [npos, total): one per 8 columns of a kept row: dy[b * K + j] = bf16(dx[b, 1 + j]) (the patch GEMM's output gradient).
__global__ __launch_bounds__(256) void keep_assemble_bwd_kernel(const float* __restrict__ dx, const int* __restrict__ inv, int B, int K, int G,
                                                                int D, float* __restrict__ dpos, float* __restrict__ dcls,
                                                                ov_bf16* __restrict__ dy, int64_t lddy, int64_t npos, int64_t total) {
    const int L = K + 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < npos) {
            const int qpr = D >> 2;
            const int p = (int)(i / qpr);
            const int c = (int)(i - (int64_t)p * qpr) * 4;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
            for (int b = 0; b < B; ++b) {
                const int t = p == 0 ? 0 : 1 + inv[(int64_t)b * G + p - 1];
                if (t > 0 || p == 0) {
                    const float4 g = *(const float4*)(dx + ((int64_t)b * L + t) * D + c);
                    acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
                }
            }
            if (dpos) *(float4*)(dpos + (int64_t)p * D + c) = acc;
            if (p == 0 && dcls) *(float4*)(dcls + c) = acc;
        } else {
            const int dpr = D >> 3;
            const int64_t k = i - npos;
            const int64_t r = k / dpr;
            const int ch = (int)(k - r * dpr);
            const int64_t b = r / K;
            const float* src = dx + (b * L + 1 + (r - b * K)) * D + ch * 8;
            const float4 g0 = *(const float4*)src, g1 = *(const float4*)(src + 4);
            *(u32x4_t*)(dy + r * lddy + ch * 8) =
                u32x4_t{pack_bf16x2(g0.x, g0.y), pack_bf16x2(g0.z, g0.w), pack_bf16x2(g1.x, g1.y), pack_bf16x2(g1.z, g1.w)};
        }
    }
}

// Pixel gradient of the kept-patch im2col (stride = kernel: every pixel belongs to exactly one patch, so a pure gather, no sums):
// one thread per 4 consecutive pixels of an image row, dimg [B, 3, S, S] fp32 (16-byte stores) or bf16 (8-byte stores).
template <bool OUT_F32>
__global__ __launch_bounds__(256) void col2im_keep_kernel(const ov_bf16* __restrict__ dcols, int64_t ldc, const int* __restrict__ inv,
                                                          void* __restrict__ dimg, int S, int P, int g, int K, int64_t total) {
    const int G = g * g, PP = P * P;
    const int qpr = S >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t line = i / qpr;                 // (b, c, y)
        const int x0 = (int)(i - line * qpr) * 4;
        const int y = (int)(line % S);
        const int64_t bc = line / S;
        const int c = (int)(bc % 3);
        const int64_t b = bc / 3;
        const int py = y / P, ii = y - py * P;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xx = x0 + e;
            const int px = xx / P, jj = xx - px * P;
            const int j = inv[b * G + py * g + px];
            v[e] = j >= 0 ? bf16_bits_to_f32(dcols[(b * K + j) * ldc + c * PP + ii * P + jj]) : 0.f;
        }
        if (OUT_F32) {
            *(float4*)((float*)dimg + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            *(u32x2_t*)((ov_bf16*)dimg + i * 4) = u32x2_t{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        }
    }
}

__global__ __launch_bounds__(256) void cls_rows_kernel(ov_bf16* __restrict__ x, int64_t ldx, const float* __restrict__ cls,
                                                       const float* __restrict__ pos0, int B, int L, int D) {
    const int total = B * D;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int b = i / D, d = i - b * D;
        const float v = round_bf16(cls[d]) + round_bf16(pos0[d]);
        x[(int64_t)b * L * ldx + d] = f32_to_bf16_bits(v);
    }
}

// grid (B, ceil(D/8/64)), block 256: wave w sums tokens first+w, first+w+4, ...; lanes own 16-B column chunks
__global__ __launch_bounds__(256) void mean_pool_kernel(const ov_bf16* __restrict__ x, int64_t ldx, float* __restrict__ out,
                                                        int L, int D, int first) {
    __shared__ float red[4][64][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int ch = blockIdx.y * 64 + lane;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ch * 8 < D) {
        const ov_bf16* p = x + (int64_t)b * L * ldx + ch * 8;
        for (int t = first + wave; t < L; t += 4) {
            const u32x4_t w = *(const u32x4_t*)(p + (int64_t)t * ldx);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * e] += bf16lo_to_f32(w[e]);
                acc[2 * e + 1] += bf16hi_to_f32(w[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][lane][e] = acc[e];
    __syncthreads();
    if (wave == 0 && ch * 8 < D) {
        const float inv = 1.0f / (float)(L - first);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (red[0][lane][e] + red[1][lane][e] + red[2][lane][e] + red[3][lane][e]) * inv;
        float4* q = (float4*)(out + (int64_t)b * D + ch * 8);
        q[0] = make_float4(o[0], o[1], o[2], o[3]);
        q[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
}

// out[b, n] += <A[b, :], W[n, :]> + bias[n]: fp32 rows against a bf16 weight widened exactly, in the exact-fp32 MFMA (k-ordered fmaf
// chain, as logits_kernel).  One workgroup per 32x32 tile; its four waves take a quarter of K each and are summed through LDS in wave
// order, so a row's result depends on that row alone and on nothing that varies between launches.
__global__ __launch_bounds__(256) void pooled_linear_kernel(const float* __restrict__ A, const ov_bf16* __restrict__ W, int64_t ldw,
                                                            const float* __restrict__ bias, float* __restrict__ out, int B, int N,
                                                            int K) {
    __shared__ float red[4][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const int ai = (i0 + j) < B ? (i0 + j) : B - 1;
    const int wj = (j0 + j) < N ? (j0 + j) : N - 1;
    const int kq = K >> 2;
    const float* ap = A + (int64_t)ai * K + wave * kq + 4 * half;
    const ov_bf16* wp = W + (int64_t)wj * ldw + wave * kq + 4 * half;
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 4
    for (int k0 = 0; k0 < kq; k0 += 8) {
        const u32x2_t wv = *(const u32x2_t*)(wp + k0);
        const float4 av = *(const float4*)(ap + k0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf16lo_to_f32(wv[0]), av.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf16hi_to_f32(wv[0]), av.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf16lo_to_f32(wv[1]), av.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf16hi_to_f32(wv[1]), av.w, acc, 0, 0, 0);
    }
    // acc[i] = <W[j0 + (i&3) + 8*(i>>2) + 4*half], A[i0 + j]> over this wave's quarter of K
#pragma unroll
    for (int i = 0; i < 16; ++i) red[wave][i][lane] = acc[i];
    __syncthreads();
    if (wave == 0 && i0 + j < B) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int col = j0 + (i & 3) + 8 * (i >> 2) + 4 * half;
            if (col < N) {
                const float s = ((red[0][i][lane] + red[1][i][lane]) + red[2][i][lane]) + red[3][i][lane];
                float* o = out + (int64_t)(i0 + j) * N + col;
                *o = *o + (s + bias[col]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* __restrict__ tokens, const ov_bf16* __restrict__ table,
                                                         const ov_bf16* __restrict__ pos, ov_bf16* __restrict__ x, int64_t ldx,
                                                         int T, int D, int V, int* __restrict__ err, int64_t total) {
    const int cpr = D >> 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int ch = (int)(i - row * cpr);
        const int t = (int)(row % T);
        int64_t id = tokens[row];
        if (id < 0 || id >= V) {
            if (err) *err = 1;
            id = id < 0 ? 0 : V - 1;
        }
        const u32x4_t a = *(const u32x4_t*)(table + id * D + ch * 8);
        const u32x4_t p = *(const u32x4_t*)(pos + (int64_t)t * D + ch * 8);
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            o[e] = pack_bf16x2(bf16lo_to_f32(a[e]) + bf16lo_to_f32(p[e]), bf16hi_to_f32(a[e]) + bf16hi_to_f32(p[e]));
        *(u32x4_t*)(x + row * ldx + ch * 8) = o;
    }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const ov_bf16* __restrict__ x, int64_t ldx, ov_bf16* __restrict__ out,
                                                          int64_t ldo, int B, int L, int t, int D) {
    const int cpr = D >> 3;
    const int total = B * cpr;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int b = i / cpr, ch = i - b * cpr;
        *(u32x4_t*)(out + (int64_t)b * ldo + ch * 8) = *(const u32x4_t*)(x + ((int64_t)b * L + t) * ldx + ch * 8);
    }
}

// One wave per caption: every lane keeps the (value, first position) pair of its strided share, then a butterfly over the pairs.  The
// order (larger value, then smaller position) is total, so every lane ends with the same pair whatever the order of the exchanges.
__global__ __launch_bounds__(256) void token_argmax_kernel(const int64_t* __restrict__ tokens, int* __restrict__ idx, int B, int T) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int b = blockIdx.x * wpb + (threadIdx.x >> 6); b < B; b += gridDim.x * wpb) {
        const int64_t* row = tokens + (int64_t)b * T;
        int64_t best = INT64_MIN;
        int at = T;                                           // a lane without an element: loses every comparison against a real one
        for (int t = lane; t < T; t += 64) {
            const int64_t v = row[t];
            if (at == T || v > best) { best = v; at = t; }    // ascending t: strict > keeps the first of equal values
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t ov = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(at, o, 64);
            if (oa < T && (at == T || ov > best || (ov == best && oa < at))) { best = ov; at = oa; }
        }
        if (lane == 0) idx[b] = at;
    }
}

__global__ __launch_bounds__(256) void gather_rows_at_kernel(const ov_bf16* __restrict__ x, int64_t ldx, const int* __restrict__ idx,
                                                             ov_bf16* __restrict__ out, int64_t ldo, int B, int L, int D) {
    const int cpr = D >> 3;
    const int64_t total = (int64_t)B * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / cpr), ch = (int)(i - (int64_t)b * cpr);
        int t = idx[b];
        t = t < 0 ? 0 : (t > L - 1 ? L - 1 : t);              // memory safety only: ov_token_argmax never leaves [0, L)
        *(u32x4_t*)(out + (int64_t)b * ldo + ch * 8) = *(const u32x4_t*)(x + ((int64_t)b * L + t) * ldx + ch * 8);
    }
}

template <bool SRC_F32, bool DST_F32>
__global__ __launch_bounds__(256) void convert_kernel(const void* __restrict__ src, int64_t lds, void* __restrict__ dst,
                                                      int64_t ldd, int64_t rows, int cols) {
    const int64_t total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols;
        const int c = (int)(i - r * cols);
        const float v = SRC_F32 ? ((const float*)src)[r * lds + c] : bf16_bits_to_f32(((const ov_bf16*)src)[r * lds + c]);
        if (DST_F32) ((float*)dst)[r * ldd + c] = v;
        else ((ov_bf16*)dst)[r * ldd + c] = f32_to_bf16_bits(v);
    }
}

// one wave per row
template <bool X_F32>
__global__ __launch_bounds__(256) void l2norm_kernel(const void* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy,
                                                     int64_t rows, int E) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        float ss = 0.f;
        for (int c = lane; c < E; c += 64) {
            const float v = X_F32 ? ((const float*)x)[row * ldx + c] : bf16_bits_to_f32(((const ov_bf16*)x)[row * ldx + c]);
            ss += v * v;
        }
        const float nrm = sqrtf(wave_sum(ss));
        const float inv = 1.0f / fmaxf(nrm, 1e-12f);
        for (int c = lane; c < E; c += 64) {
            const float v = X_F32 ? ((const float*)x)[row * ldx + c] : bf16_bits_to_f32(((const ov_bf16*)x)[row * ldx + c]);
            y[row * ldy + c] = v * inv;
        }
    }
}

inline unsigned grid_for(int64_t total, int block) {
    int64_t g = (total + block - 1) / block;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (unsigned)g;
}

int im2col_keep_launch(const void* image, int img_dtype, const int* keep, ov_bf16* out, int B, int S, int P, int K, int Kpad,
                       const ov_bf16* pos, ov_bf16* posk, int D, int* err_flag, hipStream_t st) {
    if (!image || !keep || !out || B <= 0 || S <= 0 || P <= 0) return OV_ERR_INVALID;
    if (S % P || Kpad % 8 || Kpad < 3 * P * P || ((uintptr_t)out & 15)) return OV_ERR_INVALID;
    const int g = S / P;
    if (K < 1 || K > g * g) return OV_ERR_INVALID;
    if (posk && (!pos || D <= 0 || D % 8 || (((uintptr_t)pos | (uintptr_t)posk) & 15))) return OV_ERR_INVALID;
    const int64_t ncols = (int64_t)B * K * (Kpad / 8);
    const int64_t total = ncols + (posk ? (int64_t)B * K * (D / 8) : 0);
    if (img_dtype == OV_F32)
        hipLaunchKernelGGL(im2col_keep_kernel<true>, dim3(grid_for(total, 256)), dim3(256), 0, st, image, keep, out, pos, posk, S, P, g, K,
                           Kpad, D, err_flag, ncols, total);
    else if (img_dtype == OV_BF16)
        hipLaunchKernelGGL(im2col_keep_kernel<false>, dim3(grid_for(total, 256)), dim3(256), 0, st, image, keep, out, pos, posk, S, P, g, K,
                           Kpad, D, err_flag, ncols, total);
    else
        return OV_ERR_INVALID;
    OV_LAUNCH_CHECK();
    return OV_OK;
}

}  // namespace

// ov_im2col_patches_keep with the kept rows' positional-embedding rows gathered in the same launch (ov_vision_embed_keep)
int ov_im2col_patches_keep_pos(const void* image, int img_dtype, const int* keep, ov_bf16* out, int B, int S, int P, int K, int Kpad,
                               const ov_bf16* pos, ov_bf16* posk, int D, int* err_flag, ov_stream_t stream) {
    if (!posk) return OV_ERR_INVALID;
    return im2col_keep_launch(image, img_dtype, keep, out, B, S, P, K, Kpad, pos, posk, D, err_flag, (hipStream_t)stream);
}

extern "C" int ov_im2col_patches(const void* image, int img_dtype, ov_bf16* out, int B, int S, int P, int Kpad,
                                 ov_stream_t stream) {
    if (!image || !out || B <= 0 || S <= 0 || P <= 0) return OV_ERR_INVALID;
    if (S % P || Kpad % 8 || Kpad < 3 * P * P || ((uintptr_t)out & 15)) return OV_ERR_INVALID;
    const int g = S / P;
    const int64_t total = (int64_t)B * g * g * (Kpad / 8);
    hipStream_t st = (hipStream_t)stream;
    if (img_dtype == OV_F32)
        hipLaunchKernelGGL(im2col_kernel<true>, dim3(grid_for(total, 256)), dim3(256), 0, st, image, out, B, S, P, g, Kpad, total);
    else if (img_dtype == OV_BF16)
        hipLaunchKernelGGL(im2col_kernel<false>, dim3(grid_for(total, 256)), dim3(256), 0, st, image, out, B, S, P, g, Kpad, total);
    else
        return OV_ERR_INVALID;
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_cls_rows(ov_bf16* x, int64_t ldx, const float* cls, const float* pos0, int B, int L, int D,
                           ov_stream_t stream) {
    if (!x || !cls || !pos0 || B <= 0 || L <= 0 || D <= 0 || ldx < D) return OV_ERR_INVALID;
    hipLaunchKernelGGL(cls_rows_kernel, dim3(grid_for((int64_t)B * D, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, cls,
                       pos0, B, L, D);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_mean_pool(const ov_bf16* x, int64_t ldx, float* out, int B, int L, int D, int first,
                            ov_stream_t stream) {
    if (!x || !out || B <= 0 || L <= 0 || D <= 0 || first < 0 || first >= L) return OV_ERR_INVALID;
    if (D % 8 || ldx % 8 || ldx < D || (((uintptr_t)x | (uintptr_t)out) & 15)) return OV_ERR_INVALID;
    hipLaunchKernelGGL(mean_pool_kernel, dim3((unsigned)B, (unsigned)((D / 8 + 63) / 64)), dim3(256), 0, (hipStream_t)stream, x,
                       ldx, out, L, D, first);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" size_t ov_mlp_out_pooled_workspace_bytes(int B, int F) {
    return B > 0 && F > 0 ? (size_t)B * F * 4 : 0;
}

// The mean commutes with c_proj: two pooling passes and a [B, F] x [D, F]^T product, all fp32 past the bf16 inputs.
extern "C" int ov_mlp_out_pooled(const ov_bf16* x1, int64_t ldx, const ov_bf16* hid, int64_t ldh, const ov_bf16* W, int64_t ldw,
                                 const float* bias, float* out, int B, int L, int D, int F, int first, void* workspace,
                                 size_t workspace_bytes, ov_stream_t stream) {
    if (!x1 || !hid || !W || !bias || !out || !workspace || B <= 0 || L <= 0 || D <= 0 || F <= 0) return OV_ERR_INVALID;
    if (F % 32 || ldw % 8 || ldw < F || (((uintptr_t)W | (uintptr_t)workspace | (uintptr_t)bias) & 15)) return OV_ERR_INVALID;
    if (workspace_bytes < ov_mlp_out_pooled_workspace_bytes(B, F)) return OV_ERR_WORKSPACE;
    float* mean_h = (float*)workspace;
    int rc;
    if ((rc = ov_mean_pool(x1, ldx, out, B, L, D, first, stream))) return rc;
    if ((rc = ov_mean_pool(hid, ldh, mean_h, B, L, F, first, stream))) return rc;
    hipLaunchKernelGGL(pooled_linear_kernel, dim3((unsigned)((D + 31) / 32), (unsigned)((B + 31) / 32)), dim3(256), 0,
                       (hipStream_t)stream, mean_h, W, ldw, bias, out, B, D, F);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_text_embed(const int64_t* tokens, const ov_bf16* table, const ov_bf16* pos, ov_bf16* x, int64_t ldx,
                             int B, int T, int D, int V, int* err_flag, ov_stream_t stream) {
    if (!tokens || !table || !pos || !x || B <= 0 || T <= 0 || D <= 0 || V <= 0) return OV_ERR_INVALID;
    if (D % 8 || ldx % 8 || ldx < D || (((uintptr_t)table | (uintptr_t)pos | (uintptr_t)x) & 15)) return OV_ERR_INVALID;
    const int64_t total = (int64_t)B * T * (D / 8);
    hipLaunchKernelGGL(text_embed_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, tokens, table, pos, x,
                       ldx, T, D, V, err_flag, total);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_gather_rows(const ov_bf16* x, int64_t ldx, ov_bf16* out, int64_t ldo, int B, int L, int t, int D,
                              ov_stream_t stream) {
    if (!x || !out || B <= 0 || L <= 0 || t < 0 || t >= L || D <= 0) return OV_ERR_INVALID;
    if (D % 8 || ldx % 8 || ldo % 8 || ldx < D || ldo < D || (((uintptr_t)x | (uintptr_t)out) & 15)) return OV_ERR_INVALID;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((int64_t)B * (D / 8), 256)), dim3(256), 0, (hipStream_t)stream, x, ldx,
                       out, ldo, B, L, t, D);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_token_argmax(const int64_t* tokens, int* idx, int B, int T, ov_stream_t stream) {
    if (!tokens || !idx || B <= 0 || T <= 0) return OV_ERR_INVALID;
    hipLaunchKernelGGL(token_argmax_kernel, dim3(grid_for(B, 4)), dim3(256), 0, (hipStream_t)stream, tokens, idx, B, T);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_gather_rows_at(const ov_bf16* x, int64_t ldx, const int* idx, ov_bf16* out, int64_t ldo, int B, int L, int D,
                                 ov_stream_t stream) {
    if (!x || !idx || !out || B <= 0 || L <= 0 || D <= 0) return OV_ERR_INVALID;
    if (D % 8 || ldx % 8 || ldo % 8 || ldx < D || ldo < D || (((uintptr_t)x | (uintptr_t)out) & 15)) return OV_ERR_INVALID;
    hipLaunchKernelGGL(gather_rows_at_kernel, dim3(grid_for((int64_t)B * (D / 8), 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, idx,
                       out, ldo, B, L, D);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_convert(const void* src, int src_dtype, int64_t lds, void* dst, int dst_dtype, int64_t ldd, int64_t rows,
                          int cols, ov_stream_t stream) {
    if (!src || !dst || rows <= 0 || cols <= 0 || lds < cols || ldd < cols) return OV_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_for(rows * cols, 256)), blk(256);
    if (src_dtype == OV_F32 && dst_dtype == OV_BF16)
        hipLaunchKernelGGL((convert_kernel<true, false>), grid, blk, 0, st, src, lds, dst, ldd, rows, cols);
    else if (src_dtype == OV_BF16 && dst_dtype == OV_F32)
        hipLaunchKernelGGL((convert_kernel<false, true>), grid, blk, 0, st, src, lds, dst, ldd, rows, cols);
    else if (src_dtype == OV_F32 && dst_dtype == OV_F32)
        hipLaunchKernelGGL((convert_kernel<true, true>), grid, blk, 0, st, src, lds, dst, ldd, rows, cols);
    else if (src_dtype == OV_BF16 && dst_dtype == OV_BF16)
        hipLaunchKernelGGL((convert_kernel<false, false>), grid, blk, 0, st, src, lds, dst, ldd, rows, cols);
    else
        return OV_ERR_INVALID;
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_l2norm(const void* x, int x_dtype, int64_t ldx, float* y, int64_t ldy, int64_t rows, int E,
                         ov_stream_t stream) {
    if (!x || !y || rows <= 0 || E <= 0 || ldx < E || ldy < E) return OV_ERR_INVALID;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == OV_F32)
        hipLaunchKernelGGL(l2norm_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, x, ldx, y, ldy, rows, E);
    else if (x_dtype == OV_BF16)
        hipLaunchKernelGGL(l2norm_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, x, ldx, y, ldy, rows, E);
    else
        return OV_ERR_INVALID;
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_im2col_patches_keep(const void* image, int img_dtype, const int* keep, ov_bf16* out, int B, int S, int P, int K, int Kpad,
                                      ov_stream_t stream) {
    return im2col_keep_launch(image, img_dtype, keep, out, B, S, P, K, Kpad, nullptr, nullptr, 0, nullptr, (hipStream_t)stream);
}

extern "C" int ov_patch_keep_inverse(const int* keep, int* inv, int B, int K, int G, int* err_flag, ov_stream_t stream) {
    if (!keep || !inv || B <= 0 || G <= 0 || K < 1 || K > G) return OV_ERR_INVALID;
    if (G > 16384) return OV_ERR_UNSUPPORTED;                 // the map of one image lives in LDS
    hipLaunchKernelGGL(keep_inverse_kernel, dim3((unsigned)B), dim3(256), (size_t)G * sizeof(int), (hipStream_t)stream, keep, inv, K, G,
                       err_flag);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_patch_keep_assemble(const ov_bf16* y, int64_t ldy, const float* cls, const float* pos, const int* keep, float* x, int B,
                                      int K, int G, int D, ov_stream_t stream) {
    if (!y || !cls || !pos || !keep || !x || B <= 0 || G <= 0 || K < 1 || K > G || D <= 0) return OV_ERR_INVALID;
    if (D % 8 || ldy % 8 || ldy < D || (((uintptr_t)y | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)x) & 15)) return OV_ERR_INVALID;
    const int64_t total = (int64_t)B * (K + 1) * (D / 8);
    hipLaunchKernelGGL(keep_assemble_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, y, ldy, cls, pos, keep, x, K, G,
                       D, total);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_patch_keep_assemble_backward(const float* dx, const int* inv, int B, int K, int G, int D, float* dpos, float* dcls,
                                               ov_bf16* dy, int64_t lddy, ov_stream_t stream) {
    if (!dx || !inv || B <= 0 || G <= 0 || K < 1 || K > G || D <= 0) return OV_ERR_INVALID;
    if (D % 8 || (((uintptr_t)dx | (uintptr_t)dpos | (uintptr_t)dcls | (uintptr_t)dy) & 15)) return OV_ERR_INVALID;
    if (dy && (lddy % 8 || lddy < D)) return OV_ERR_INVALID;
    const int64_t npos = (dpos || dcls) ? (int64_t)(1 + G) * (D / 4) : 0;
    const int64_t total = npos + (dy ? (int64_t)B * K * (D / 8) : 0);
    if (total == 0) return OV_OK;
    hipLaunchKernelGGL(keep_assemble_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, dx, inv, B, K, G, D, dpos,
                       dcls, dy, lddy, npos, total);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_col2im_patches_keep(const ov_bf16* dcols, int64_t ldc, const int* inv, void* dimg, int img_dtype, int B, int S, int P,
                                      int K, ov_stream_t stream) {
    if (!dcols || !inv || !dimg || B <= 0 || S <= 0 || P <= 0) return OV_ERR_INVALID;
    if (S % P || S % 4 || ldc < 3 * P * P) return OV_ERR_INVALID;
    const int g = S / P;
    if (K < 1 || K > g * g) return OV_ERR_INVALID;
    if (((uintptr_t)dimg & (img_dtype == OV_F32 ? 15 : 7))) return OV_ERR_INVALID;
    const int64_t total = (int64_t)B * 3 * S * (S / 4);
    hipStream_t st = (hipStream_t)stream;
    if (img_dtype == OV_F32)
        hipLaunchKernelGGL(col2im_keep_kernel<true>, dim3(grid_for(total, 256)), dim3(256), 0, st, dcols, ldc, inv, dimg, S, P, g, K, total);
    else if (img_dtype == OV_BF16)
        hipLaunchKernelGGL(col2im_keep_kernel<false>, dim3(grid_for(total, 256)), dim3(256), 0, st, dcols, ldc, inv, dimg, S, P, g, K, total);
    else
        return OV_ERR_INVALID;
    OV_LAUNCH_CHECK();
    return OV_OK;
}
