// feature.hip — the MLP-feature objective of feature visualisation (gfx950): one hidden unit of one block's MLP, read at the
// GELU output and averaged over the patch tokens, with its gradient back to the block's mid residual x1.
//
// The reference reads the unit through a forward hook on visual.transformer.resblocks[layer].mlp.gelu
// (ov-feature-visualization.py:211, cliptoolsoptimized.py:990-999 / 1149-1164) after running the whole c_fc GEMM.  One column of
// that GEMM is all the objective needs, so both directions are per-row work:
//   forward   pre[r]  = LN_2(x1[r]) . W_fc[f] + b_fc[f]                       (fp32, kept for the backward)
//             mean[b] = sum_{t = 1 .. L-1} gelu(pre[b L + t]) / (L - 1)        (CLS excluded; fixed-order reduction, no atomics)
//   backward  g_t     = dmean[b] / (L - 1) gelu'(pre[b L + t])  (t >= 1; 0 for the CLS row)
//             dx1[r]  = LN_2-backward(x1[r], gamma_2, g_t W_fc[f])             (the dx formula of ov_layernorm_backward)
// GELU and its derivative are the exact forms here (erff / tanhf / expf): a few thousand elements per call, far from the VALU bound
// that made the GEMM epilogues take the polynomial fits of common.h.
// ov_block_attn_forward_saving is the attention half of the tap block (LN_1 -> QKV -> attention -> out_proj + residual) keeping what
// ov_block_attn_backward_input (backward.hip) reads.
#include "common.h"

namespace {

__device__ __forceinline__ float gelu_exact(float a, bool tanh_form) {
    if (tanh_form) return 0.5f * a * (1.0f + tanhf(0.7978845608028654f * (a + 0.044715f * a * a * a)));
    return 0.5f * a * (1.0f + erff(a * 0.70710678118654752440f));
}
__device__ __forceinline__ float gelu_grad_exact(float a, bool tanh_form) {
    if (tanh_form) {
        const float t = tanhf(0.7978845608028654f * (a + 0.044715f * a * a * a));
        return 0.5f * (1.0f + t) + 0.5f * a * (1.0f - t * t) * 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * a * a);
    }
    return 0.5f * (1.0f + erff(a * 0.70710678118654752440f)) + a * 0.3989422804014327f * expf(-0.5f * a * a);
}

// Loads row `row` of x (bf16) into v and returns its LayerNorm statistics (two-pass, fp32, biased variance: layernorm.hip's form).
template <int NCH>
__device__ __forceinline__ void load_row_stats(const ov_bf16* __restrict__ x, int64_t ldx, int64_t row, int D, float eps, int lane,
                                               float (&v)[NCH][8], float& mean, float& rstd) {
    const int nchunk = D >> 3;
    const float invD = 1.0f / (float)D;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
            const u32x4_t w = *(const u32x4_t*)(x + row * ldx + ch * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[c][2 * e] = bf16lo_to_f32(w[e]); v[c][2 * e + 1] = bf16hi_to_f32(w[e]); }
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[c][e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
        }
    }
    mean = wave_sum(s) * invD;
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
        if (lane + c * 64 < nchunk)
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[c][e] - mean; ss += d * d; }
    rstd = rsqrtf(wave_sum(ss) * invD + eps);
}

// pre[r] = LN(x1[r]) . wrow + bias, one wave per row (4 rows per 256-thread block, grid-stride)
template <int NCH>
__global__ __launch_bounds__(256) void mlp_feature_pre(const ov_bf16* __restrict__ x1, int64_t ldx, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const ov_bf16* __restrict__ wrow,
                                                       const float* __restrict__ bias, int64_t rows, int D, float eps,
                                                       float* __restrict__ pre) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunk = D >> 3;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        float v[NCH][8], mean, rstd;
        load_row_stats<NCH>(x1, ldx, row, D, eps, lane, v, mean, rstd);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + c * 64;
            if (ch < nchunk) {
                const float4 g0 = *(const float4*)(gamma + ch * 8), g1 = *(const float4*)(gamma + ch * 8 + 4);
                const float4 b0 = *(const float4*)(beta + ch * 8), b1 = *(const float4*)(beta + ch * 8 + 4);
                const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
                const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
                const u32x4_t w = *(const u32x4_t*)(wrow + ch * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dot = fmaf(fmaf((v[c][2 * e] - mean) * rstd, g[2 * e], b[2 * e]), bf16lo_to_f32(w[e]), dot);
                    dot = fmaf(fmaf((v[c][2 * e + 1] - mean) * rstd, g[2 * e + 1], b[2 * e + 1]), bf16hi_to_f32(w[e]), dot);
                }
            }
        }
        dot = wave_sum(dot);
        if (lane == 0) pre[row] = dot + (bias ? bias[0] : 0.f);
    }
}

// mean[b] = sum_{t=1}^{L-1} gelu(pre[b L + t]) / (L - 1): one block per image; thread i sums tokens 1 + i, 1 + i + 256, ... in order,
// then a fixed LDS tree (deterministic)
template <bool TANH>
__global__ __launch_bounds__(256) void mlp_feature_mean(const float* __restrict__ pre, int L, float* __restrict__ mean) {
    __shared__ float red[256];
    const int b = blockIdx.x, t0 = threadIdx.x;
    const float* p = pre + (int64_t)b * L;
    float s = 0.f;
    for (int t = 1 + t0; t < L; t += 256) s += gelu_exact(p[t], TANH);
    red[t0] = s;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if (t0 < h) red[t0] += red[t0 + h];
        __syncthreads();
    }
    if (t0 == 0) mean[b] = red[0] / (float)(L - 1);
}

// dx1[r] = LN-backward(x1[r], gamma, g_t wrow), g_t = dmean[b] / (L - 1) gelu'(pre[r]) for t >= 1, 0 for the CLS row
template <int NCH, bool TANH>
__global__ __launch_bounds__(256) void mlp_feature_bwd(const ov_bf16* __restrict__ x1, int64_t ldx, const float* __restrict__ gamma,
                                                       const ov_bf16* __restrict__ wrow, const float* __restrict__ pre,
                                                       const float* __restrict__ dmean, int L, int64_t rows, int D, float eps,
                                                       ov_bf16* __restrict__ dx, int64_t lddx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunk = D >> 3;
    const float invD = 1.0f / (float)D;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int64_t b = row / L;
        const int t = (int)(row - b * L);
        if (t == 0) {                                   // the CLS token does not enter the objective
            const u32x4_t z = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                if (lane + c * 64 < nchunk) *(u32x4_t*)(dx + row * lddx + (lane + c * 64) * 8) = z;
            continue;
        }
        const float gt = dmean[b] / (float)(L - 1) * gelu_grad_exact(pre[row], TANH);
        float v[NCH][8], q[NCH][8], mean, rstd;
        load_row_stats<NCH>(x1, ldx, row, D, eps, lane, v, mean, rstd);
        float sq = 0.f, sqx = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + c * 64;
            if (ch < nchunk) {
                const float4 g0 = *(const float4*)(gamma + ch * 8), g1 = *(const float4*)(gamma + ch * 8 + 4);
                const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
                const u32x4_t w = *(const u32x4_t*)(wrow + ch * 8);
                float wf[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) { wf[2 * e] = bf16lo_to_f32(w[e]); wf[2 * e + 1] = bf16hi_to_f32(w[e]); }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xh = (v[c][e] - mean) * rstd;
                    v[c][e] = xh;
                    q[c][e] = gt * wf[e] * g[e];              // q = dy * gamma, dy = g_t W_fc[f]
                    sq += q[c][e];
                    sqx = fmaf(q[c][e], xh, sqx);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) q[c][e] = 0.f;
            }
        }
        const float mq = wave_sum(sq) * invD, mqx = wave_sum(sqx) * invD;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + c * 64;
            if (ch < nchunk) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = rstd * (q[c][e] - mq - v[c][e] * mqx);
                const u32x4_t w = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
                *(u32x4_t*)(dx + row * lddx + ch * 8) = w;
            }
        }
    }
}

inline unsigned row_blocks(int64_t rows) {
    const int64_t b = (rows + 3) / 4;
    return (unsigned)(b < 16384 ? b : 16384);
}

// shape checks shared by the two tap entry points (after the null / size checks)
inline int feature_shape_ok(const void* x1, int64_t ldx, const float* gamma, const void* fc_w, int64_t ldw, int D) {
    if (D % 8 || D > 4096 || ldx % 8 || ldx < D || ldw % 8 || ldw < D) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)x1 | (uintptr_t)gamma | (uintptr_t)fc_w) & 15) return OV_ERR_INVALID;
    return OV_OK;
}

}  // namespace

extern "C" int ov_mlp_feature_forward(const ov_bf16* x1, int64_t ldx, const float* ln2_w, const float* ln2_b, const ov_bf16* fc_w,
                                      int64_t ldw, const float* fc_b, int feature, int mlp, int gelu_tanh, int B, int L, int D, float eps,
                                      float* pre, float* mean, ov_stream_t stream) {
    if (!x1 || !ln2_w || !ln2_b || !fc_w || !pre || !mean || B <= 0 || L < 2 || D <= 0 || mlp <= 0) return OV_ERR_INVALID;
    if (feature < 0 || feature >= mlp) return OV_ERR_INVALID;              // the MLP padding (So400m: 4304 .. 4351) is no feature
    int rc = feature_shape_ok(x1, ldx, ln2_w, fc_w, ldw, D);
    if (rc) return rc;
    if ((uintptr_t)ln2_b & 15) return OV_ERR_INVALID;
    const int64_t rows = (int64_t)B * L;
    hipStream_t st = (hipStream_t)stream;
    const ov_bf16* wrow = fc_w + (int64_t)feature * ldw;
    const float* bias = fc_b ? fc_b + feature : nullptr;
    const dim3 grid(row_blocks(rows)), blk(256);
    const int nch = (D / 8 + 63) / 64;
    if (nch <= 1) hipLaunchKernelGGL(mlp_feature_pre<1>, grid, blk, 0, st, x1, ldx, ln2_w, ln2_b, wrow, bias, rows, D, eps, pre);
    else if (nch <= 2) hipLaunchKernelGGL(mlp_feature_pre<2>, grid, blk, 0, st, x1, ldx, ln2_w, ln2_b, wrow, bias, rows, D, eps, pre);
    else if (nch <= 3) hipLaunchKernelGGL(mlp_feature_pre<3>, grid, blk, 0, st, x1, ldx, ln2_w, ln2_b, wrow, bias, rows, D, eps, pre);
    else if (nch <= 4) hipLaunchKernelGGL(mlp_feature_pre<4>, grid, blk, 0, st, x1, ldx, ln2_w, ln2_b, wrow, bias, rows, D, eps, pre);
    else hipLaunchKernelGGL(mlp_feature_pre<8>, grid, blk, 0, st, x1, ldx, ln2_w, ln2_b, wrow, bias, rows, D, eps, pre);
    OV_LAUNCH_CHECK();
    if (gelu_tanh) hipLaunchKernelGGL(mlp_feature_mean<true>, dim3((unsigned)B), blk, 0, st, (const float*)pre, L, mean);
    else hipLaunchKernelGGL(mlp_feature_mean<false>, dim3((unsigned)B), blk, 0, st, (const float*)pre, L, mean);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_mlp_feature_backward(const ov_bf16* x1, int64_t ldx, const float* ln2_w, const ov_bf16* fc_w, int64_t ldw, int feature,
                                       int mlp, int gelu_tanh, const float* pre, const float* dmean, ov_bf16* dx1, int64_t lddx, int B, int L,
                                       int D, float eps, ov_stream_t stream) {
    if (!x1 || !ln2_w || !fc_w || !pre || !dmean || !dx1 || B <= 0 || L < 2 || D <= 0 || mlp <= 0) return OV_ERR_INVALID;
    if (feature < 0 || feature >= mlp) return OV_ERR_INVALID;
    int rc = feature_shape_ok(x1, ldx, ln2_w, fc_w, ldw, D);
    if (rc) return rc;
    if (lddx % 8 || lddx < D) return OV_ERR_UNSUPPORTED;
    if ((uintptr_t)dx1 & 15) return OV_ERR_INVALID;
    const int64_t rows = (int64_t)B * L;
    hipStream_t st = (hipStream_t)stream;
    const ov_bf16* wrow = fc_w + (int64_t)feature * ldw;
    const dim3 grid(row_blocks(rows)), blk(256);
    const int nch = (D / 8 + 63) / 64;
#define OV_FEAT_BWD(N)                                                                                                              \
    do {                                                                                                                            \
        if (gelu_tanh) hipLaunchKernelGGL((mlp_feature_bwd<N, true>), grid, blk, 0, st, x1, ldx, ln2_w, wrow, pre, dmean, L, rows, D, eps, \
                                          dx1, lddx);                                                                               \
        else hipLaunchKernelGGL((mlp_feature_bwd<N, false>), grid, blk, 0, st, x1, ldx, ln2_w, wrow, pre, dmean, L, rows, D, eps, dx1,     \
                                lddx);                                                                                              \
    } while (0)
    if (nch <= 1) OV_FEAT_BWD(1);
    else if (nch <= 2) OV_FEAT_BWD(2);
    else if (nch <= 3) OV_FEAT_BWD(3);
    else if (nch <= 4) OV_FEAT_BWD(4);
    else OV_FEAT_BWD(8);
#undef OV_FEAT_BWD
    OV_LAUNCH_CHECK();
    return OV_OK;
}

// The attention half of one ResidualAttentionBlock (transformer.py:263): x1 = x + out_proj(attn(ln_1(x))), the operator sequence of
// ov_tower_forward_saving.  attn_out holds ln_1(x) until the attention overwrites it (no workspace).  lse (optional): the attention's
// row log-sum-exp where the resident backward uses it (head_dim 64, L <= 288), untouched otherwise.
extern "C" int ov_block_attn_forward_saving(const ov_tower_cfg* cfg, const ov_block_weights* w, const ov_bf16* x, ov_bf16* qkv,
                                            ov_bf16* attn_out, ov_bf16* x1, float* lse, int B, int L, ov_stream_t stream) {
    if (!cfg || !w || !x || !qkv || !attn_out || !x1 || B <= 0 || L <= 0) return OV_ERR_INVALID;
    if (!w->ln1_w || !w->ln1_b || !w->qkv_w || !w->qkv_b || !w->out_w || !w->out_b) return OV_ERR_INVALID;
    if (w->qkv_colsum || w->fc_colsum) return OV_ERR_UNSUPPORTED;             // the module's own (unfolded) weights
    const int D = cfg->width, H = cfg->heads;
    if (D <= 0 || H <= 0 || D % 64 || D % H || D > 4096) return OV_ERR_UNSUPPORTED;
    const int hd = D / H;
    if (hd % 8 || hd > 96) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)qkv | (uintptr_t)attn_out | (uintptr_t)x1) & 15) return OV_ERR_INVALID;
    const int64_t M = (int64_t)B * L;
    const float scale = 1.0f / sqrtf((float)hd);
    const bool keep_lse = lse != nullptr && ov_attn_bwd_resident(hd, L);
    int rc;
    if ((rc = ov_layernorm(x, OV_BF16, D, w->ln1_w, w->ln1_b, attn_out, OV_BF16, D, M, D, cfg->ln_eps, stream))) return rc;
    if ((rc = ov_gemm(attn_out, D, w->qkv_w, D, w->qkv_b, qkv, 3 * D, M, 3 * D, D, OV_EPI_BIAS, nullptr, 0, 0, 0, 0, stream))) return rc;
    rc = keep_lse ? ov_attention_lse(qkv, 3 * D, attn_out, D, lse, B, L, H, hd, scale, stream)
                  : ov_attention(qkv, 3 * D, attn_out, D, B, L, H, hd, scale, stream);
    if (rc) return rc;
    return ov_gemm(attn_out, D, w->out_w, D, w->out_b, x1, D, M, D, D, OV_EPI_BIAS_RESIDUAL, x, D, 0, 0, 0, stream);
}
