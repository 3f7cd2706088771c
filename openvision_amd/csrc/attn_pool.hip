// attn_pool.hip — attentional pooling (gfx950): cross-attention from a few learned queries, shared by every image, to the L tokens of
// each image, forward and backward.
//
// The reference is AttentionalPooler (open_clip/transformer.py:187-207): nn.MultiheadAttention(E, n_head, kdim = vdim = width) with the
// LayerNormed queries expanded over the batch.  The projections, LayerNorms and out_proj are GEMM / LayerNorm calls of the library;
// this file is the softmax(scale q k^T) v core and its backward.  Against the self-attention kernels (attention.hip, attention_bwd.hip)
// three things differ: n_q != L, the query operand q [n_q, H*hd] has no batch stride, and dq is a sum over the images.
//
// Same tile arithmetic as those kernels (attn_tile.h; v_mfma_f32_32x32x16_bf16 throughout; P and dS rounded to bf16 before the second
// products), and the LDS image of the streaming backward: [32-wide d slice][row][32 d], 64-byte rows, 16-byte chunks XOR-swizzled by
// (row >> 2) & 3.  It serves the row-major fragment reads (contraction over d) and ds_read_b64_tr_b16 (contraction over rows) alike.
// NDH = d slices: 2 for head_dim <= 64, 3 for head dims up to 96 (zero columns).  n_q <= 256, so the query side is at most 8 tiles:
//   pool_fwd     workgroup = (image, head); wave = query tile, Q fragments in registers; K | V streamed through LDS in chunks
//                of `ch` keys (the whole sequence for L <= 288): S^T, online softmax with the lazy rescale, O^T += V^T P^T.
//   pool_bwd_q   workgroup = (chunk of bc images, head); wave = query tile.  The images of the chunk are walked IN ORDER and
//                dQ^T += K^T dS^T keeps accumulating across them, so a workgroup's partial is one fixed-order sum; delta is written
//                for pool_bwd_kv.  Partials [chunk][n_q][H*hd] fp32 go to the workspace.
//   pool_bwd_kv  workgroup = (image, head, block of <= 8 key tiles); wave = key tile, K and V fragments in registers; Q and dO of
//                the head (all n_q rows) resident in LDS with lse and delta: dV^T += dO^T P, dK^T += Q^T dS.
//   pool_dq_sum  dq = scale * (partial 0 + partial 1 + ...) in chunk order.
// S and dP are computed in both backward kernels (7 tile products per tile pair, not the minimal 5) so that no accumulator is shared
// between waves: no atomics, and bc depends on n_q alone, so the result is a function of the shape and repeats bitwise.
// First version: correct and deterministic, plain staging through registers, serial LDS waits.
#include "common.h"
#include "attn_tile.h"
#include "attention_route.h"

namespace {

struct PoolArgs {
    const ov_bf16* q; int64_t ldq;            // [n_q, H*hd]
    const ov_bf16* kv; int64_t ldkv;          // [B*L, 2*H*hd]  (k | v)
    ov_bf16* out; int64_t ldo;                // [B*n_q, H*hd]  (forward: written; backward: read)
    const ov_bf16* dout; int64_t lddo;        // [B*n_q, H*hd]
    float* lse;                               // [B*H][nqp] log2 units (forward: written unless NULL; backward: read)
    float* dlt;                               // [B*H][nqp]
    float* part;                              // [nchunk][n_q][H*hd]
    ov_bf16* dkv; int64_t lddkv;              // [B*L, 2*H*hd]  (dk | dv)
    int B, L, nq, H, hd;
    int ch;                                   // rows of an LDS image
    int nqt, nqp;                             // query tiles, n_q rounded up to 32
    int bc;                                   // images per dQ partial
    int nblk, kw;                             // pool_bwd_kv: key blocks per head, key tiles (= waves) per block
    float scale, scale_log2;
};

// two A-operand fragments (contraction steps 0 and 1) of one d slice of X^T for a 32-row tile; reads and wait in ONE asm statement
// (attention_bwd.hip's tr_half)
__device__ __forceinline__ void tr_half(unsigned a0, unsigned b0, bf16x8_t& f0, bf16x8_t& f1) {
    u32x2_t v0, v1, v2, v3;
    asm volatile("ds_read_b64_tr_b16 %0, %4\n\tds_read_b64_tr_b16 %1, %5 offset:512\n\t"
                 "ds_read_b64_tr_b16 %2, %4 offset:1024\n\tds_read_b64_tr_b16 %3, %5 offset:1536\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3) : "v"(a0), "v"(b0) : "memory");
    f0 = attn::tr_join(v0, v1);
    f1 = attn::tr_join(v2, v3);
}

template <int NDH>
struct Pool {
    // stage rows [row0, row0 + nr) (clamped to `last`) of a [*, hd] column block into an image of `ch` rows; columns >= hd are zeros
    static __device__ __forceinline__ void stage(char* img, const ov_bf16* src, int64_t ld, int row0, int nr, int last, int hd, int ch,
                                                 int tid, int nthreads) {
        const int np = nr * 4;                                    // 16-byte pieces per d slice
        for (int q = tid; q < NDH * np; q += nthreads) {
            const int dh = q / np, pp = q - dh * np;
            const int pos = pp >> 2;
            int row = row0 + pos;
            row = row < last ? row : last;
            const int col = (dh * 4 + (pp & 3)) * 8;
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (col < hd) v = *(const u32x4_t*)(src + (int64_t)row * ld + col);
            *(u32x4_t*)(img + dh * ch * 64 + pos * 64 + (((pp & 3) ^ ((pos >> 2) & 3)) << 4)) = v;
        }
    }
    // this lane's B-operand fragments of row `row` of a [*, hd] column block: d = 16 st + 8 h2 .. + 8 (zeros past hd)
    static __device__ __forceinline__ void load_own(bf16x8_t (&f)[2 * NDH], const ov_bf16* base, int64_t ld, int row, int h2, int hd) {
#pragma unroll
        for (int st = 0; st < 2 * NDH; ++st) {
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (16 * st + 8 * h2 < hd) v = *(const u32x4_t*)(base + (int64_t)row * ld + 16 * st + 8 * h2);
            f[st] = __builtin_bit_cast(bf16x8_t, v);
        }
    }
    // store rows d = 32 dh + 8 g + 4 h2 + e of the accumulators (lane = output row of the tensor) scaled by `sc`
    static __device__ __forceinline__ void store(ov_bf16* op, const f32x16_t (&acc)[NDH], float sc, int h2, int hd) {
#pragma unroll
        for (int dh = 0; dh < NDH; ++dh)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int d0 = 32 * dh + 8 * gq + 4 * h2;
                if (d0 < hd) {
                    const u32x2_t w = {pack_bf16x2(acc[dh][4 * gq] * sc, acc[dh][4 * gq + 1] * sc),
                                       pack_bf16x2(acc[dh][4 * gq + 2] * sc, acc[dh][4 * gq + 3] * sc)};
                    *(u32x2_t*)(op + d0) = w;
                }
            }
    }
    static __device__ __forceinline__ void zero(f32x16_t (&acc)[NDH]) {
#pragma unroll
        for (int dh = 0; dh < NDH; ++dh)
#pragma unroll
            for (int t = 0; t < 16; ++t) acc[dh][t] = 0.f;
    }
};

// frag: row-major fragment (contraction over d) of row tile*32 + r; tr_mma: acc[dh] += X^T(d slice dh, rows of `tile`) . T with T
// packed as b0 (rows 0-15) / b1 (rows 16-31).  `ch` = rows of the image.
#define OV_POOL_HELPERS()                                                                                                             \
    auto frag = [&](const char* img, int tile, int st) {                                                                              \
        return *(const bf16x8_t*)(img + (st >> 1) * ch * 64 + (tile * 32 + r) * 64 + (((((st & 1) << 1) | h2) ^ ((r >> 2) & 3)) << 4)); \
    };                                                                                                                                \
    const int vi = lane & 15, vg = (lane >> 4) & 1;                                                                                   \
    const unsigned tr_row = (unsigned)((4 * h2 + (vi >> 2)) * 64 + 8 * (vi & 1));                                                     \
    const unsigned tr_ch = (unsigned)(2 * vg + ((vi & 3) >> 1));                                                                      \
    const unsigned tr_lane_a = tr_row + ((tr_ch ^ (unsigned)h2) << 4), tr_lane_b = tr_row + ((tr_ch ^ (unsigned)h2 ^ 2u) << 4);     \
    auto tr_mma = [&](const char* img, int tile, bf16x8_t b0, bf16x8_t b1, f32x16_t (&acc)[NDH]) {                                    \
        const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)img + (unsigned)(tile * 2048);      \
        _Pragma("unroll") for (int dh = 0; dh < NDH; ++dh) {                                                                          \
            bf16x8_t f0, f1;                                                                                                          \
            tr_half(base + (unsigned)(dh * ch * 64) + tr_lane_a, base + (unsigned)(dh * ch * 64) + tr_lane_b, f0, f1);                \
            acc[dh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0, b0, acc[dh], 0, 0, 0);                                              \
            acc[dh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f1, b1, acc[dh], 0, 0, 0);                                              \
        }                                                                                                                             \
    };

// ---- forward --------------------------------------------------------------------------------------------------------------------
// blockDim = max(nqt, 4) waves: a wave past the last query tile only helps staging.
template <int NDH>
__global__ __launch_bounds__(512) void pool_fwd(const PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef Pool<NDH> P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    const int L = a.L, hd = a.hd, HD = a.H * hd, ch = a.ch, nq = a.nq;
    const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
    char* img0 = smem;
    char* img1 = smem + NDH * ch * 64;
    OV_POOL_HELPERS()
    const bool active = wave < a.nqt;
    const int query = wave * 32 + r;
    const int qrow = query < nq ? query : nq - 1;
    const ov_bf16* kbase = a.kv + (int64_t)b * L * a.ldkv + h * hd;
    bf16x8_t qB[2 * NDH];
    P::load_own(qB, a.q + h * hd, a.ldq, qrow, h2, hd);
    float m = -INFINITY, lsum = 0.f;
    f32x16_t o[NDH];
    P::zero(o);
    for (int k0 = 0; k0 < L; k0 += ch) {
        const int nk = min(L - k0, ch), nr = (nk + 31) & ~31;
        if (k0) __syncthreads();
        P::stage(img0, kbase, a.ldkv, k0, nr, L - 1, hd, ch, tid, blockDim.x);
        P::stage(img1, kbase + HD, a.ldkv, k0, nr, L - 1, hd, ch, tid, blockDim.x);
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < (nr >> 5); ++j) {
            f32x16_t s;
#pragma unroll
            for (int t = 0; t < 16; ++t) s[t] = 0.f;
#pragma unroll
            for (int st = 0; st < 2 * NDH; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(img0, j, st), qB[st], s, 0, 0, 0);
            OV_ATTN_MASK_TAIL(s, j, h2, nk)
            asm volatile("s_nop 15" : "+v"(s));                          // a full tile: nothing else in front of attn::tile_max
            const float mx = attn::half_max(attn::tile_max(s), a.scale_log2);
            OV_ATTN_RESCALE_ROWS(false, mx, m, lsum, o, NDH)
            float ps0 = 0.f, ps1 = 0.f;
#pragma unroll
            for (int t = 0; t < 16; t += 2) {
                s[t] = __builtin_amdgcn_exp2f(fmaf(s[t], a.scale_log2, -m));
                s[t + 1] = __builtin_amdgcn_exp2f(fmaf(s[t + 1], a.scale_log2, -m));
                ps0 += s[t];
                ps1 += s[t + 1];
            }
            lsum += ps0 + ps1;
            tr_mma(img1, j, attn::pack_p(s, 0), attn::pack_p(s, 1), o);
        }
    }
    if (!active) return;
    const float l = lsum + attn::swap_halves(lsum);
    if (query < nq) {
        P::store(a.out + ((int64_t)b * nq + query) * a.ldo + h * hd, o, 1.0f / l, h2, hd);
        if (a.lse && h2 == 0) a.lse[(int64_t)bh * a.nqp + query] = m + __builtin_amdgcn_logf(l);     // v_log_f32 = log2
    }
}

// ---- backward: dQ partials and delta --------------------------------------------------------------------------------------------
template <int NDH>
__global__ __launch_bounds__(512) void pool_bwd_q(const PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef Pool<NDH> P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    const int L = a.L, hd = a.hd, HD = a.H * hd, ch = a.ch, nq = a.nq;
    const int c = blockIdx.x / a.H, h = blockIdx.x - c * a.H;
    char* img0 = smem;
    char* img1 = smem + NDH * ch * 64;
    OV_POOL_HELPERS()
    const bool active = wave < a.nqt;
    const int query = wave * 32 + r;
    const int qrow = query < nq ? query : nq - 1;
    bf16x8_t qB[2 * NDH], dB[2 * NDH];
    P::load_own(qB, a.q + h * hd, a.ldq, qrow, h2, hd);
    f32x16_t dq[NDH];
    P::zero(dq);
    const int bend = min(a.B, (c + 1) * a.bc);
    for (int b = c * a.bc; b < bend; ++b) {
        const int64_t bh = (int64_t)b * a.H + h;
        const ov_bf16* kbase = a.kv + (int64_t)b * L * a.ldkv + h * hd;
        const ov_bf16* drow = a.dout + ((int64_t)b * nq + qrow) * a.lddo + h * hd;
        float lse2 = 0.f, delta = 0.f;
        if (active) {
            P::load_own(dB, drow, 0, 0, h2, hd);
            lse2 = query < nq ? a.lse[bh * a.nqp + query] : 0.f;
            // delta = sum_d dO[q, d] O[q, d]: the two lane halves take alternate 8-element chunks
            const ov_bf16* op = a.out + ((int64_t)b * nq + qrow) * a.ldo + h * hd;
            for (int cc = h2; cc < (hd >> 3); cc += 2) {
                const u32x4_t ov = *(const u32x4_t*)(op + 8 * cc);
                const u32x4_t dv = *(const u32x4_t*)(drow + 8 * cc);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    delta = fmaf(bf16lo_to_f32(ov[e]), bf16lo_to_f32(dv[e]), delta);
                    delta = fmaf(bf16hi_to_f32(ov[e]), bf16hi_to_f32(dv[e]), delta);
                }
            }
            delta += attn::swap_halves(delta);
            if (h2 == 0) a.dlt[bh * a.nqp + query] = delta;           // every entry below nqp: pool_bwd_kv reads them all
        }
        for (int k0 = 0; k0 < L; k0 += ch) {
            const int nk = min(L - k0, ch), nr = (nk + 31) & ~31;
            __syncthreads();                                          // everybody has left the previous chunk / image
            P::stage(img0, kbase, a.ldkv, k0, nr, L - 1, hd, ch, tid, blockDim.x);
            P::stage(img1, kbase + HD, a.ldkv, k0, nr, L - 1, hd, ch, tid, blockDim.x);
            __syncthreads();
            if (!active) continue;
            for (int j = 0; j < (nr >> 5); ++j) {
                f32x16_t s, dp;
#pragma unroll
                for (int t = 0; t < 16; ++t) { s[t] = 0.f; dp[t] = 0.f; }
#pragma unroll
                for (int st = 0; st < 2 * NDH; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(img0, j, st), qB[st], s, 0, 0, 0);
#pragma unroll
                for (int st = 0; st < 2 * NDH; ++st) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(img1, j, st), dB[st], dp, 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int key = j * 32 + (t & 3) + 8 * (t >> 2) + 4 * h2;
                    const float p = (key < nk && query < nq) ? __builtin_amdgcn_exp2f(fmaf(s[t], a.scale_log2, -lse2)) : 0.f;
                    s[t] = p * (dp[t] - delta);                      // dS^T
                }
                tr_mma(img0, j, attn::pack_p(s, 0), attn::pack_p(s, 1), dq);
            }
        }
    }
    if (active && query < nq) {                                       // unscaled fp32 partial: rows d = 32 dh + 8 g + 4 h2 + e
        float* pp = a.part + ((int64_t)c * nq + query) * HD + h * hd;
#pragma unroll
        for (int dh = 0; dh < NDH; ++dh)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int d0 = 32 * dh + 8 * gq + 4 * h2;
                if (d0 < hd) *(f32x4_t*)(pp + d0) = f32x4_t{dq[dh][4 * gq], dq[dh][4 * gq + 1], dq[dh][4 * gq + 2], dq[dh][4 * gq + 3]};
            }
    }
}

// ---- backward: dK, dV -----------------------------------------------------------------------------------------------------------
template <int NDH>
__global__ __launch_bounds__(512) void pool_bwd_kv(const PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef Pool<NDH> P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    const int L = a.L, hd = a.hd, HD = a.H * hd, nq = a.nq;
    const int ch = a.nqp;                                             // the images hold the query side here
    const int bh = blockIdx.x / a.nblk, blk = blockIdx.x - bh * a.nblk;
    const int b = bh / a.H, h = bh - b * a.H;
    char* img0 = smem;
    char* img1 = smem + NDH * ch * 64;
    float* lse_s = (float*)(smem + 2 * NDH * ch * 64);
    float* dlt_s = lse_s + ch;
    OV_POOL_HELPERS()
    P::stage(img0, a.q + h * hd, a.ldq, 0, ch, nq - 1, hd, ch, tid, blockDim.x);
    P::stage(img1, a.dout + (int64_t)b * nq * a.lddo + h * hd, a.lddo, 0, ch, nq - 1, hd, ch, tid, blockDim.x);
    for (int q = tid; q < ch; q += blockDim.x) {
        lse_s[q] = q < nq ? a.lse[(int64_t)bh * ch + q] : 0.f;        // the forward writes entries [0, n_q) only
        dlt_s[q] = a.dlt[(int64_t)bh * ch + q];
    }
    __syncthreads();
    const int k0 = (blk * a.kw + wave) * 32;
    if (k0 >= L) return;                                              // (wave-uniform; no barrier follows)
    const int key = k0 + r;
    const int krow = key < L ? key : L - 1;
    const ov_bf16* kbase = a.kv + (int64_t)b * L * a.ldkv + h * hd;
    bf16x8_t kB[2 * NDH], vB[2 * NDH];
    P::load_own(kB, kbase, a.ldkv, krow, h2, hd);
    P::load_own(vB, kbase + HD, a.ldkv, krow, h2, hd);
    f32x16_t dk[NDH], dv[NDH];
    P::zero(dk);
    P::zero(dv);
    for (int i = 0; i < a.nqt; ++i) {
        f32x16_t s, dp;
#pragma unroll
        for (int t = 0; t < 16; ++t) { s[t] = 0.f; dp[t] = 0.f; }
#pragma unroll
        for (int st = 0; st < 2 * NDH; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(img0, i, st), kB[st], s, 0, 0, 0);
#pragma unroll
        for (int st = 0; st < 2 * NDH; ++st) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(img1, i, st), vB[st], dp, 0, 0, 0);
        // s[t], dp[t]: query i*32 + (t&3) + 8 (t>>2) + 4 h2 (register), key = lane column
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int ql = i * 32 + (t & 3) + 8 * (t >> 2) + 4 * h2;
            const float p = ql < nq ? __builtin_amdgcn_exp2f(fmaf(s[t], a.scale_log2, -lse_s[ql])) : 0.f;
            s[t] = p;                                                // P
            dp[t] = p * (dp[t] - dlt_s[ql]);                         // dS
        }
        tr_mma(img1, i, attn::pack_p(s, 0), attn::pack_p(s, 1), dv);
        tr_mma(img0, i, attn::pack_p(dp, 0), attn::pack_p(dp, 1), dk);
    }
    if (key < L) {
        ov_bf16* kp = a.dkv + ((int64_t)b * L + key) * a.lddkv + h * hd;
        P::store(kp, dk, a.scale, h2, hd);
        P::store(kp + HD, dv, 1.0f, h2, hd);
    }
}

// dq[query][col] = scale * (part[0] + part[1] + ...)[query][col], chunk order
__global__ __launch_bounds__(256) void pool_dq_sum(const float* part, float* dq, int64_t ld_dq, int nq, int HD, int nchunk, float scale) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= (int64_t)nq * HD) return;
    const int64_t row = i / HD, col = i - row * HD;
    f32x4_t acc = *(const f32x4_t*)(part + i);
    for (int c = 1; c < nchunk; ++c) {
        const f32x4_t v = *(const f32x4_t*)(part + (int64_t)c * nq * HD + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], v[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] *= scale;
    *(f32x4_t*)(dq + row * ld_dq + col) = acc;
}

const OvKernelForm<PoolArgs> FWD[] = {{2, pool_fwd<2>}, {3, pool_fwd<3>}};
const OvKernelForm<PoolArgs> BWD_Q[] = {{2, pool_bwd_q<2>}, {3, pool_bwd_q<3>}};
const OvKernelForm<PoolArgs> BWD_KV[] = {{2, pool_bwd_kv<2>}, {3, pool_bwd_kv<3>}};

int pool_chunk(int n_q) { return n_q > 64 ? 8 : 2; }

// The operands every entry point shares; fills the shape part of the arguments.
int pool_check(PoolArgs& p, const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const void* out, int64_t ld_out, int B, int L, int n_q,
               int H, int hd, float scale) {
    if (!q || !kv || !out || B <= 0 || L <= 0 || H <= 0) return OV_ERR_INVALID;
    if (hd <= 0 || hd % 8 || hd > 96 || n_q < 1 || n_q > 256) return OV_ERR_UNSUPPORTED;
    const int64_t HD = (int64_t)H * hd;
    if (ld_q % 8 || ld_kv % 8 || ld_out % 8 || ld_q < HD || ld_kv < 2 * HD || ld_out < HD) return OV_ERR_INVALID;
    if (((uintptr_t)q | (uintptr_t)kv | (uintptr_t)out) & 15) return OV_ERR_INVALID;
    if ((int64_t)B * H > OV_ATTN_I32 || HD > OV_ATTN_I32) return OV_ERR_UNSUPPORTED;
    p = PoolArgs{};
    p.B = B; p.L = L; p.nq = n_q; p.H = H; p.hd = hd;
    const int Lp = (L + 31) / 32 * 32;
    p.ch = Lp <= 288 ? Lp : 256;
    p.nqt = (n_q + 31) / 32;
    p.nqp = p.nqt * 32;
    p.bc = pool_chunk(n_q);
    const int nkt = Lp / 32;
    p.nblk = (nkt + 7) / 8;
    p.kw = (nkt + p.nblk - 1) / p.nblk;
    p.scale = scale;
    p.scale_log2 = scale * 1.4426950408889634f;
    return OV_OK;
}
}  // namespace

extern "C" int ov_attn_pool(const ov_bf16* q, int64_t ld_q, const ov_bf16* kv, int64_t ld_kv, ov_bf16* out, int64_t ld_out, float* lse, int B,
                            int L, int n_q, int H, int hd, float scale, ov_stream_t stream) {
    PoolArgs p;
    const int rc = pool_check(p, q, ld_q, kv, ld_kv, out, ld_out, B, L, n_q, H, hd, scale);
    if (rc != OV_OK) return rc;
    if ((uintptr_t)lse & 3) return OV_ERR_INVALID;
    p.q = q; p.ldq = ld_q; p.kv = kv; p.ldkv = ld_kv; p.out = out; p.ldo = ld_out; p.lse = lse;
    static OvPerDeviceOnce once;
    const int ndh = hd <= 64 ? 2 : 3;
    return ov_launch_form(FWD, once, OV_ATTN_LDS, ndh, dim3((unsigned)(B * H)), dim3((unsigned)(max(p.nqt, 4) * 64)),
                          (size_t)2 * ndh * p.ch * 64, (hipStream_t)stream, p);
}

extern "C" int ov_attn_pool_backward_chunk(int n_q) { return pool_chunk(n_q); }

extern "C" size_t ov_attn_pool_backward_workspace_bytes(int B, int L, int n_q, int H, int hd) {
    if (B <= 0 || L <= 0 || n_q <= 0 || H <= 0 || hd <= 0) return 0;
    const int bc = pool_chunk(n_q);
    const size_t nqp = (size_t)(n_q + 31) / 32 * 32, nchunk = (size_t)(B + bc - 1) / bc;
    return (size_t)B * H * nqp * sizeof(float) + nchunk * n_q * H * hd * sizeof(float);
}

extern "C" int ov_attn_pool_backward(const ov_bf16* q, int64_t ld_q, const ov_bf16* kv, int64_t ld_kv, const ov_bf16* out, int64_t ld_out,
                                     const ov_bf16* dout, int64_t ld_dout, const float* lse, float* dq, int64_t ld_dq, ov_bf16* dkv,
                                     int64_t ld_dkv, int B, int L, int n_q, int H, int hd, float scale, void* workspace,
                                     size_t workspace_bytes, ov_stream_t stream) {
    PoolArgs p;
    const int rc = pool_check(p, q, ld_q, kv, ld_kv, out, ld_out, B, L, n_q, H, hd, scale);
    if (rc != OV_OK) return rc;
    const int64_t HD = (int64_t)H * hd;
    if (!dout || !lse || !dq || !dkv) return OV_ERR_INVALID;
    if (ld_dout % 8 || ld_dkv % 8 || ld_dq % 4 || ld_dout < HD || ld_dkv < 2 * HD || ld_dq < HD) return OV_ERR_INVALID;
    if (((uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dkv) & 15 || ((uintptr_t)lse & 3)) return OV_ERR_INVALID;
    if ((int64_t)B * H * p.nblk > OV_ATTN_I32) return OV_ERR_UNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 15)) return OV_ERR_INVALID;
    if (workspace_bytes < ov_attn_pool_backward_workspace_bytes(B, L, n_q, H, hd)) return OV_ERR_WORKSPACE;
    p.q = q; p.ldq = ld_q; p.kv = kv; p.ldkv = ld_kv; p.out = const_cast<ov_bf16*>(out); p.ldo = ld_out; p.dout = dout; p.lddo = ld_dout;
    p.lse = const_cast<float*>(lse);
    p.dlt = (float*)workspace;
    p.part = p.dlt + (size_t)B * H * p.nqp;
    p.dkv = dkv; p.lddkv = ld_dkv;
    static OvPerDeviceOnce once[2];
    const int ndh = hd <= 64 ? 2 : 3;
    const int nchunk = (B + p.bc - 1) / p.bc;
    int r = ov_launch_form(BWD_Q, once[0], OV_ATTN_LDS, ndh, dim3((unsigned)(nchunk * H)), dim3((unsigned)(max(p.nqt, 4) * 64)),
                           (size_t)2 * ndh * p.ch * 64, (hipStream_t)stream, p);
    if (r != OV_OK) return r;
    r = ov_launch_form(BWD_KV, once[1], OV_ATTN_LDS, ndh, dim3((unsigned)((int64_t)B * H * p.nblk)), dim3((unsigned)(p.kw * 64)),
                       (size_t)2 * ndh * p.nqp * 64 + 2 * p.nqp * sizeof(float), (hipStream_t)stream, p);
    if (r != OV_OK) return r;
    const int64_t n4 = (int64_t)n_q * HD / 4;
    hipLaunchKernelGGL(pool_dq_sum, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p.part, dq, ld_dq, n_q, (int)HD,
                       nchunk, scale);
    OV_LAUNCH_CHECK();
    return OV_OK;
}
