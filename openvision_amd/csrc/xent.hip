// xent.hip — the caption loss: masked softmax cross-entropy over the vocabulary (gfx950), fp32 throughout.
//
// Reference: softmax_xent(logits, labels, reduction=True, mask) of src/losses/common.py:225-251 as the trainer calls it
// (src/main_clip.py:448-465); its `smoothing` argument is unused there and here.
//     nll_r = logsumexp(logits_r) - logits_r[label_r]        (0 when label_r is outside [0, V): one_hot gives a zero row)
//     loss  = sum_r nll_r mask_r / (sum_r mask_r + 1e-8)
// Forward: one workgroup per row, ONE pass over the row (per-thread online maximum / sum over 16-byte loads, then a workgroup
// reduction of the (max, sum) pairs); the row's nll_r mask_r goes to the workspace and a single-workgroup kernel sums rows and masks in
// a fixed order -- deterministic, no atomics, no host synchronisation.
// Backward: dlogits = g mask_r / (sum mask + 1e-8) (softmax(logits_r) - onehot_r) from the kept row log-sum-exp, one pass; dlogits may
// alias logits (every element is read and written by the same thread).
#include "common.h"

namespace {
constexpr int XT = 256;                      // threads per row
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

// the workgroup's (max, sum of exp2(x log2e - max)) over a row; every thread returns the same pair
__device__ __forceinline__ void row_max_sum(const float* x, int V, bool vec, float& m_out, float& s_out) {
    __shared__ float sm[XT / 64], ss[XT / 64];
    const int tid = threadIdx.x;
    float m = -INFINITY, s = 0.f;
    auto fold4 = [&](float a, float b, float c, float d) {
        a *= LOG2E; b *= LOG2E; c *= LOG2E; d *= LOG2E;
        const float mx = fmaxf(fmaxf(a, b), fmaxf(c, d));
        if (mx > m) { s *= __builtin_amdgcn_exp2f(m - mx); m = mx; }          // (m = -inf: s = 0 stays 0)
        if (m > -INFINITY)
            s += __builtin_amdgcn_exp2f(a - m) + __builtin_amdgcn_exp2f(b - m) + __builtin_amdgcn_exp2f(c - m) + __builtin_amdgcn_exp2f(d - m);
    };
    const int nv = vec ? V >> 2 : 0;
    for (int i = tid; i < nv; i += XT) {
        const f32x4_t v = *(const f32x4_t*)(x + 4 * i);
        fold4(v[0], v[1], v[2], v[3]);
    }
    for (int i = 4 * nv + tid; i < V; i += XT) fold4(x[i], -INFINITY, -INFINITY, -INFINITY);
    // wave, then workgroup
    const float wm = wave_max(m);
    s = wm > -INFINITY ? s * __builtin_amdgcn_exp2f(m - wm) : 0.f;
    s = wave_sum(s);
    if ((tid & 63) == 0) { sm[tid >> 6] = wm; ss[tid >> 6] = s; }
    __syncthreads();
    float gm = sm[0];
#pragma unroll
    for (int w = 1; w < XT / 64; ++w) gm = fmaxf(gm, sm[w]);
    float gs = 0.f;
#pragma unroll
    for (int w = 0; w < XT / 64; ++w) gs += sm[w] > -INFINITY ? ss[w] * __builtin_amdgcn_exp2f(sm[w] - gm) : 0.f;
    m_out = gm;
    s_out = gs;
}

__global__ __launch_bounds__(XT) void xent_rows(const float* logits, int64_t ld, const int64_t* labels, const float* mask, int V, bool vec,
                                                float* row_lse, float* row_term) {
    const int64_t r = blockIdx.x;
    const float* x = logits + r * ld;
    float m, s;
    row_max_sum(x, V, vec, m, s);
    if (threadIdx.x == 0) {
        const float lse = (m + __builtin_amdgcn_logf(s)) * LN2;                // v_log_f32 = log2
        const int64_t lab = labels[r];
        const float nll = (lab >= 0 && lab < V) ? lse - x[lab] : 0.f;
        const float mk = mask[r];
        row_lse[r] = lse;
        row_term[r] = mk != 0.f ? nll * mk : 0.f;
    }
}

// One workgroup: t = sum of terms (or nothing when terms == NULL), d = sum of mask + 1e-8, both in a fixed order.
// out[0] = t / d (terms != NULL) or d (terms == NULL: the backward's denominator).
__global__ __launch_bounds__(1024) void xent_reduce(const float* terms, const float* mask, int64_t R, float* out) {
    __shared__ float st[16], sd[16];
    const int tid = threadIdx.x;
    float t = 0.f, d = 0.f;
    for (int64_t i = tid; i < R; i += 1024) {
        if (terms) t += terms[i];
        d += mask[i];
    }
    t = wave_sum(t);
    d = wave_sum(d);
    if ((tid & 63) == 0) { st[tid >> 6] = t; sd[tid >> 6] = d; }
    __syncthreads();
    if (tid == 0) {
        float tt = 0.f, dd = 0.f;
        for (int w = 0; w < 16; ++w) { tt += st[w]; dd += sd[w]; }
        dd += 1e-8f;
        out[0] = terms ? tt / dd : dd;
    }
}

__global__ __launch_bounds__(XT) void xent_bwd_rows(const float* logits, int64_t ld, const int64_t* labels, const float* mask,
                                                    const float* row_lse, const float* grad, const float* denom, float* dlogits, int64_t ldd,
                                                    int V, bool vec) {
    const int64_t r = blockIdx.x;
    const float* x = logits + r * ld;
    float* dx = dlogits + r * ldd;
    const int tid = threadIdx.x;
    const float mk = mask[r];
    const int nv = vec ? V >> 2 : 0;
    if (mk == 0.f) {                                                          // exactly zero, whatever the row holds
        const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < nv; i += XT) *(f32x4_t*)(dx + 4 * i) = z;
        for (int i = 4 * nv + tid; i < V; i += XT) dx[i] = 0.f;
        return;
    }
    const float coef = grad[0] * mk / denom[0];
    const float nl = -row_lse[r] * LOG2E;
    const int64_t lab = labels[r];
    for (int i = tid; i < nv; i += XT) {
        const f32x4_t v = *(const f32x4_t*)(x + 4 * i);
        f32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p = __builtin_amdgcn_exp2f(fmaf(v[e], LOG2E, nl));
            o[e] = coef * (4 * i + e == lab ? p - 1.0f : p);
        }
        *(f32x4_t*)(dx + 4 * i) = o;
    }
    for (int i = 4 * nv + tid; i < V; i += XT) {
        const float p = __builtin_amdgcn_exp2f(fmaf(x[i], LOG2E, nl));
        dx[i] = coef * (i == lab ? p - 1.0f : p);
    }
}

inline bool vec_ok(const void* p, int64_t ld) { return ld % 4 == 0 && ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" size_t ov_softmax_xent_workspace_bytes(int64_t R) {
    if (R <= 0) return 0;
    return ((size_t)R * sizeof(float) + 255) / 256 * 256 + 256;
}

extern "C" int ov_softmax_xent(const float* logits, int64_t ld, const int64_t* labels, const float* mask, int64_t R, int V, float* loss,
                               float* row_lse, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!logits || !labels || !mask || !loss || !row_lse || !workspace || R <= 0 || V <= 0 || ld < V) return OV_ERR_INVALID;
    if (R > 0x7fffffffLL) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)logits | (uintptr_t)mask | (uintptr_t)loss | (uintptr_t)row_lse | (uintptr_t)workspace) & 3 || ((uintptr_t)labels & 7))
        return OV_ERR_INVALID;
    if (workspace_bytes < ov_softmax_xent_workspace_bytes(R)) return OV_ERR_WORKSPACE;
    float* terms = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(xent_rows, dim3((unsigned)R), dim3(XT), 0, st, logits, ld, labels, mask, V, vec_ok(logits, ld), row_lse, terms);
    OV_LAUNCH_CHECK();
    hipLaunchKernelGGL(xent_reduce, dim3(1), dim3(1024), 0, st, (const float*)terms, mask, R, loss);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" int ov_softmax_xent_backward(const float* logits, int64_t ld, const int64_t* labels, const float* mask, const float* row_lse,
                                        const float* grad, float* dlogits, int64_t ld_dlogits, int64_t R, int V, void* workspace,
                                        size_t workspace_bytes, ov_stream_t stream) {
    if (!logits || !labels || !mask || !row_lse || !grad || !dlogits || !workspace || R <= 0 || V <= 0 || ld < V || ld_dlogits < V)
        return OV_ERR_INVALID;
    if (R > 0x7fffffffLL) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)logits | (uintptr_t)mask | (uintptr_t)row_lse | (uintptr_t)grad | (uintptr_t)dlogits | (uintptr_t)workspace) & 3 ||
        ((uintptr_t)labels & 7))
        return OV_ERR_INVALID;
    if (workspace_bytes < ov_softmax_xent_workspace_bytes(R)) return OV_ERR_WORKSPACE;
    float* denom = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(xent_reduce, dim3(1), dim3(1024), 0, st, (const float*)nullptr, mask, R, denom);
    OV_LAUNCH_CHECK();
    hipLaunchKernelGGL(xent_bwd_rows, dim3((unsigned)R), dim3(XT), 0, st, logits, ld, labels, mask, row_lse, grad, (const float*)denom, dlogits,
                       ld_dlogits, V, vec_ok(logits, ld) && vec_ok(dlogits, ld_dlogits));
    OV_LAUNCH_CHECK();
    return OV_OK;
}
