// siglip.hip — fused SigLIP pairwise sigmoid loss on a local logit strip (gfx950).
//
// Replaces SigLipLoss._loss summed over every text block (reference open_clip/loss.py:307-414; the neighbour-exchange ring
// :219-304 is replaced by one all-gather of the text features, which changes only the order of the sums):
//     z[i, j] = s * <x_i, y_j> + beta,   l[i, j] = +1 if j == i + off else -1
//     loss    = (1 / b) * sum_{i < b, j < N} softplus(-l z)            (= -logsigmoid(l z), loss.py:349-358)
// x = the local image rows [b, E], y = the gathered text rows [N, E] in rank order.  Each (i, j) term is independent (no softmax,
// no row statistic), so the forward keeps nothing for the backward.  Logit tiles live in one f32x16 MFMA accumulator
// (exact-fp32 v_mfma_f32_32x32x2_f32, strip.h); they are never written.  No atomics: every sum has a fixed order.
#include "strip.h"

namespace {

using namespace strip;

struct SigArgs {
    const float* x;         // local rows   [b, E]
    const float* y;         // gathered     [N, E]
    float* part;            // [nrt][nsplit] partial sums of softplus(-l z)
    int b, N, E, nsplit, tiles_per_split, ntiles, label_offset;
    const float* scale;     // device scalars: the logit multiplier exp(logit_scale), the bias (NULL = none)
    const float* bias;
};

__device__ __forceinline__ float softplus_stable(float u) { return fmaxf(u, 0.f) + log1pf(expf(-fabsf(u))); }

// One workgroup per (column split, 32-row tile); its four waves take the split's 32-column tiles in turn.
__global__ __launch_bounds__(256) void siglip_loss_partial(const SigArgs a) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int split = blockIdx.x, rt = blockIdx.y;
    const int row = rt * 32 + j;
    const int rowc = row < a.b ? row : a.b - 1;
    const float* xp = a.x + (int64_t)rowc * a.E + 4 * half;
    const int label = row + a.label_offset;
    const float scale = *a.scale;
    const float beta = a.bias ? *a.bias : 0.f;

    float sum = 0.f;
    const int t0 = split * a.tiles_per_split;
    int t1 = t0 + a.tiles_per_split;
    if (t1 > a.ntiles) t1 = a.ntiles;
    for (int t = t0 + wave; t < t1; t += 4) {
        int gi = t * 32 + j;
        gi = gi < a.N ? gi : a.N - 1;
        const float* yp = a.y + (int64_t)gi * a.E + 4 * half;
        const f32x16_t acc = dot_full(yp, xp, a.E);               // acc[i] = <y[t * 32 + tile_row(i, half)], x[row]>
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int g = t * 32 + tile_row(i, half);
            const float z = fmaf(acc[i], scale, beta);
            const float u = g == label ? -z : z;                   // softplus(-l z)
            if (g < a.N && row < a.b) sum += softplus_stable(u);
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) a.part[(int64_t)rt * a.nsplit + split] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void siglip_loss_finalize(const float* __restrict__ part, int n, int b,
                                                            float* __restrict__ loss_out) {
    __shared__ float red[4];
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) v += part[i];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) loss_out[0] = (((red[0] + red[1]) + red[2]) + red[3]) / (float)b;
}


// ---- backward ---------------------------------------------------------------------------------------------------------------
// g[i, j] = d loss / d z[i, j] = -l sigmoid(-l z) / b * grad_loss.  The logit tiles are recomputed with the same exact-fp32 MFMA,
// g is formed in registers, and the product g . X_in accumulates into [32 rows x E] fp32 MFMA accumulators split over the four
// waves of a workgroup by 32-column e-tile (the last e-tile may be partial: E % 8 == 0).  The logit tile's K reduction is split
// the same way and summed through LDS in a fixed order (strip.h, RAGGED = true).
//   MODE_B = false: out rows = LOCAL rows x:      d x[i] = s * sum_j g[i, j] * y[j]     (+ per-tile partials of d s, d beta)
//   MODE_B = true : out rows = GATHERED rows y:   d y[j] = s * sum_i g[i, j] * x[i]
// One launch holds both: workgroups [0, nrt_x) take local row tiles (each a sweep over all N gathered rows), the rest take
// gathered row tiles (a sweep over b local rows).  The long local sweeps are dispatched first and the short gathered ones fill
// the remaining CUs.  The in-side loop of a workgroup is not split, so every output is written once, in a fixed order.
struct SigBwdArgs {
    const float* x;         // [b, E]
    const float* y;         // [N, E]
    float* dx;              // [b, E]
    float* dy;              // [N, E]  (NULL = gathered side skipped)
    float* part;            // [2][nrt_x]: per local row tile sum g * <x, y>, sum g
    int b, N, E, label_offset, nrt_x;
    const float* scale;     // device scalars (ABI 2): logit multiplier, bias (NULL = none), upstream gradient (NULL = 1)
    const float* bias;
    const float* grad;
    float inv_b;
};

template <bool MODE_B>
__device__ __forceinline__ void siglip_bwd_tile(const SigBwdArgs& a, int rt, Exchange part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const float* __restrict__ XO = MODE_B ? a.y : a.x;
    const float* __restrict__ XI = MODE_B ? a.x : a.y;
    float* __restrict__ OUT = MODE_B ? a.dy : a.dx;
    const int no = MODE_B ? a.N : a.b, ni = MODE_B ? a.b : a.N;
    const int E = a.E, net = (E + 31) >> 5;
    const int nown = (net - wave + 3) >> 2;                       // e-tiles wave, wave + 4, ...
    const int o = rt * 32 + j;
    const int oc = o < no ? o : no - 1;
    const float* xop = XO + (int64_t)oc * E + 4 * half;
    const float scale = *a.scale;
    const float beta = a.bias ? *a.bias : 0.f;
    const float gl = (a.grad ? *a.grad : 1.f) * a.inv_b;

    f32x16_t acc_o[MAXT];
#pragma unroll
    for (int n = 0; n < MAXT; ++n) acc_o[n] = zero16();
    float dsc = 0.f, dbs = 0.f;

    const int ntiles = (ni + 31) >> 5;
    for (int t = 0; t < ntiles; ++t) {
        int gi = t * 32 + j;
        gi = gi < ni ? gi : ni - 1;
        const float* yip = XI + (int64_t)gi * E + 4 * half;
        const f32x16_t acc = dot_wave<true>(yip, xop, E, wave, nown);
        __syncthreads();                                          // the previous tile's partials have been consumed
        put(part, wave, lane, acc);
        __syncthreads();
        f32x16_t p;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float sdot = get(part, i, lane);                // <XI[g], XO[o]>
            const int g = t * 32 + tile_row(i, half);
            const bool valid = o < no && g < ni;
            const bool hit = MODE_B ? (o == g + a.label_offset) : (g == o + a.label_offset);
            const float z = fmaf(sdot, scale, beta);
            const float sg = 1.f / (1.f + expf(hit ? z : -z));    // sigmoid(-l z); expf overflow gives 0, never NaN
            const float gv = valid ? (hit ? -sg : sg) : 0.f;      // -l sigmoid(-l z)
            p[i] = gv;
            dsc = fmaf(gv, sdot, dsc);
            dbs += gv;
        }
        accumulate<MAXT, true, true>(acc_o, p, XI, E, t, ni, E, wave, nown, j, half);
    }
    store<MAXT, true>(acc_o, OUT, E, rt, no, E, wave, nown, j, half, gl * scale);
    if (!MODE_B) {                                                // every wave holds the same p: wave 0 reports
        dsc = wave_sum(dsc);
        dbs = wave_sum(dbs);
        if (wave == 0 && lane == 0) {
            a.part[rt] = dsc;
            a.part[a.nrt_x + rt] = dbs;
        }
    }
}

__global__ __launch_bounds__(256) void siglip_loss_bwd(const SigBwdArgs a) {
    __shared__ Exchange part;
    const int bid = blockIdx.x;
    if (bid < a.nrt_x) siglip_bwd_tile<false>(a, bid, part);
    else siglip_bwd_tile<true>(a, bid - a.nrt_x, part);
}

// d s = grad / b * sum g <x, y>,  d beta = grad / b * sum g: the per-row-tile partials summed in a fixed order
__global__ __launch_bounds__(64) void siglip_loss_bwd_scalars(const float* __restrict__ part, int n, float inv_b,
                                                              const float* __restrict__ grad, float* __restrict__ d_scale,
                                                              float* __restrict__ d_bias) {
    float vs = 0.f, vb = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) {
        vs += part[i];
        vb += part[n + i];
    }
    vs = wave_sum(vs);
    vb = wave_sum(vb);
    const float c = inv_b * (grad ? *grad : 1.f);
    if (threadIdx.x == 0) {
        if (d_scale) d_scale[0] = vs * c;
        if (d_bias) d_bias[0] = vb * c;
    }
}

inline int sig_check(const float* x, const float* y, const float* scale, int b, int N, int E, int label_offset) {
    if (!x || !y || !scale) return OV_ERR_INVALID;
    if (b <= 0 || N <= 0 || E <= 0 || label_offset < 0 || (int64_t)label_offset + b > N) return OV_ERR_INVALID;
    if (E % 8 || E > 4 * MAXT * 32) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)y) & 15) return OV_ERR_INVALID;
    return OV_OK;
}

}  // namespace

extern "C" size_t ov_siglip_loss_workspace_bytes(int b, int N) {
    if (b <= 0 || N <= 0) return 0;
    const StripPlan p = strip_plan(b, N, 1);                      // one strip: x rows against y
    return (size_t)p.nrt * p.nsplit * sizeof(float);
}

extern "C" int ov_siglip_loss(const float* img, const float* all_txt, int b, int N, int E, const float* logit_scale,
                              const float* logit_bias, int label_offset, float* loss_out, void* workspace, size_t workspace_bytes,
                              ov_stream_t stream) {
    const int rc = sig_check(img, all_txt, logit_scale, b, N, E, label_offset);
    if (rc != OV_OK) return rc;
    if (!loss_out || !workspace) return OV_ERR_INVALID;
    if (workspace_bytes < ov_siglip_loss_workspace_bytes(b, N)) return OV_ERR_WORKSPACE;
    const StripPlan p = strip_plan(b, N, 1);                      // one strip: x rows against y
    SigArgs a;
    a.x = img; a.y = all_txt; a.part = (float*)workspace;
    a.b = b; a.N = N; a.E = E; a.nsplit = p.nsplit; a.tiles_per_split = p.tps; a.ntiles = p.ntiles; a.label_offset = label_offset;
    a.scale = logit_scale; a.bias = logit_bias;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(siglip_loss_partial, dim3((unsigned)p.nsplit, (unsigned)p.nrt), dim3(256), 0, st, a);
    OV_LAUNCH_CHECK();
    hipLaunchKernelGGL(siglip_loss_finalize, dim3(1), dim3(256), 0, st, a.part, p.nrt * p.nsplit, b, loss_out);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" size_t ov_siglip_loss_backward_workspace_bytes(int b, int N) {
    if (b <= 0 || N <= 0) return 0;
    return (size_t)2 * ((b + 31) / 32) * sizeof(float);
}

extern "C" int ov_siglip_loss_backward(const float* img, const float* all_txt, int b, int N, int E, const float* logit_scale,
                                       const float* logit_bias, int label_offset, const float* grad_loss, float* d_img,
                                       float* d_all_txt, float* d_scale, float* d_bias, void* workspace, size_t workspace_bytes,
                                       ov_stream_t stream) {
    const int rc = sig_check(img, all_txt, logit_scale, b, N, E, label_offset);
    if (rc != OV_OK) return rc;
    if (!d_img || !workspace) return OV_ERR_INVALID;
    if (workspace_bytes < ov_siglip_loss_backward_workspace_bytes(b, N)) return OV_ERR_WORKSPACE;
    SigBwdArgs a;
    a.x = img; a.y = all_txt; a.dx = d_img; a.dy = d_all_txt; a.part = (float*)workspace;
    a.b = b; a.N = N; a.E = E; a.label_offset = label_offset; a.nrt_x = (b + 31) / 32;
    a.scale = logit_scale; a.bias = logit_bias; a.grad = grad_loss; a.inv_b = 1.0f / (float)b;
    const int nblk = a.nrt_x + (d_all_txt ? (N + 31) / 32 : 0);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(siglip_loss_bwd, dim3((unsigned)nblk), dim3(256), 0, st, a);
    OV_LAUNCH_CHECK();
    if (d_scale || d_bias) {
        hipLaunchKernelGGL(siglip_loss_bwd_scalars, dim3(1), dim3(64), 0, st, a.part, a.nrt_x, a.inv_b, grad_loss, d_scale, d_bias);
        OV_LAUNCH_CHECK();
    }
    return OV_OK;
}
