// window.hip — the InfoNCE gradient of one window of a fixed bank: gradient accumulation for the contrastive loss (gfx950).
//
// With all N rows of an accumulated batch held fixed (the bank) and the two log-sum-exp vectors of the whole bank known (terms, from
// ov_clip_loss_multi at b = N), the gradient of the full-batch loss with respect to the rows of a window [w0, w0 + b) needs only
// the b x N logit strips of those rows.  A window row appears on BOTH sides of the loss: as a row of its own strip (softmax under
// its own lse, what multicap.hip's backward forms with GATHERED = false) and as a column of every other row's strip (softmax under
// the in-side row's lse, GATHERED = true).  Both read the same logit, so one pass over the strip with both normalisers gives
//     image row i : d img_i   = coef sum_c sum_k [ exp(A_c[i,k] - lse_img,c[i]) + exp(A_c[i,k] - lse_txt,c[k]) - 2 [k = i] ] txt_c,k
//     text row j  : d txt_c,j = coef     sum_k [ exp(B_c[j,k] - lse_txt,c[j]) + exp(B_c[j,k] - lse_img,c[k]) - 2 [k = j] ] img_k
// with A_c[i,k] = s img_i . txt_c,k = B_c[k,i]: the exact rows of the full-batch gradient, no gathered-side buffer, no reduce-scatter.
// The structure is multicap.hip's backward on strip.h: one workgroup per 32-row out tile, job 0 = the image side with the loop over
// the C sets inside, job 1 + c = the text side of set c, four waves split E by e-tile, the coefficient tile is formed in registers
// and fed back as the MFMA A operand, the in-side loop is not split, no atomics.  d loss / d scale is taken from the image-side
// strips alone: there the two exponentials are the image strip's and the transposed text strip's softmax, so disjoint windows that
// cover the bank sum to the full gradient.
#include "strip.h"

namespace {

using namespace strip;

constexpr int WN_MAXC = 4;           // caption sets per image

struct WnArgs {
    const float* all_img;            // the bank: [N, .] row pitch ld
    const float* all_txt;            // set c at all_txt + c * set_stride
    int64_t ld, set_stride;
    const float* terms;              // [4C, N]
    float* d_img;                    // [b, E]
    float* d_txt;                    // [C b, E]
    float* dsc_part;                 // [nrt]: job 0 only
    int w0, b, N, E, C, nrt;
    const float* scale;              // device scalars: logit multiplier, upstream gradient of the loss (NULL = 1)
    const float* grad;
    float inv2cn;
};

__global__ __launch_bounds__(256) void window_loss_bwd(const WnArgs a) {
    __shared__ Exchange part;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int rt = blockIdx.x, job = blockIdx.y;
    const int E = a.E, b = a.b, N = a.N;
    const int c0 = job ? job - 1 : 0;                             // the set of a text job
    const int nsets = job ? 1 : a.C;
    // out side: the window's rows of the bank; in side of set s: XI0 + s * set_stride (job 0 only walks it), all N rows
    const float* __restrict__ XO = (job ? a.all_txt + (int64_t)c0 * a.set_stride : a.all_img) + (int64_t)a.w0 * a.ld;
    const float* __restrict__ XI0 = job ? a.all_img : a.all_txt;
    float* __restrict__ OUT = job ? a.d_txt + (int64_t)c0 * b * E : a.d_img;
    // lse rows of terms: image strip of set c = row 4c, text strip = row 4c + 2.  The out rows read the strip they belong to, the
    // in-side rows the other one.
    const float* __restrict__ LSEO0 = a.terms + (int64_t)(4 * c0 + (job ? 2 : 0)) * N + a.w0;
    const float* __restrict__ LSEI0 = a.terms + (int64_t)(4 * c0 + (job ? 0 : 2)) * N;
    const int net = E >> 5;
    const int nown = (net - wave + 3) >> 2;                       // e-tiles wave, wave + 4, ...
    const int o = rt * 32 + j;
    const int oc = o < b ? o : b - 1;
    const float* xop = XO + (int64_t)oc * a.ld + 4 * half;
    const float scale = *a.scale;
    const float coef = (a.grad ? *a.grad : 1.f) * a.inv2cn * scale;
    const int label = a.w0 + o;                                   // the bank column of window row o

    f32x16_t acc_o[MAXT];
#pragma unroll
    for (int n = 0; n < MAXT; ++n) acc_o[n] = zero16();
    float dsc = 0.f;

    const int ntiles = (N + 31) >> 5;
    for (int s = 0; s < nsets; ++s) {
        const float* __restrict__ XI = XI0 + (int64_t)s * a.set_stride;
        const float* __restrict__ LSEI = LSEI0 + (int64_t)s * 4 * N;
        const float lse_o = LSEO0[(int64_t)s * 4 * N + oc];
        for (int t = 0; t < ntiles; ++t) {
            int gi = t * 32 + j;
            gi = gi < N ? gi : N - 1;
            const float* yip = XI + (int64_t)gi * a.ld + 4 * half;
            const f32x16_t acc = dot_wave<false>(yip, xop, E, wave, nown);
            float lse_i[16];                                      // the in-side tile's lse, by this lane half's rows
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int g = t * 32 + tile_row(i, half);
                lse_i[i] = LSEI[g < N ? g : N - 1];
            }
            __syncthreads();                                      // the previous tile's partials have been consumed
            put(part, wave, lane, acc);
            __syncthreads();
            f32x16_t p;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float sdot = get(part, i, lane);            // <XI[g], XO[o]>
                const int g = t * 32 + tile_row(i, half);
                const bool valid = o < b && g < N;
                const float z = sdot * scale;
                const float pv = valid ? (__expf(z - lse_o) + __expf(z - lse_i[i])) - (g == label ? 2.f : 0.f) : 0.f;
                p[i] = pv;
                dsc = fmaf(pv, sdot, dsc);
            }
            accumulate<MAXT, false, true>(acc_o, p, XI, a.ld, t, N, E, wave, nown, j, half);
        }
    }
    store<MAXT, false>(acc_o, OUT, (int64_t)E, rt, b, E, wave, nown, j, half, coef);
    if (job == 0 && a.dsc_part) {                                 // every wave holds the same P; wave 0 reports
        dsc = wave_sum(dsc);
        if (wave == 0 && lane == 0) a.dsc_part[rt] = dsc;
    }
}

}  // namespace

extern "C" size_t ov_clip_loss_window_backward_workspace_bytes(int b, int N, int C) {
    if (b <= 0 || N <= 0 || b > N || C < 1 || C > WN_MAXC) return 0;
    return (size_t)((b + 31) / 32) * sizeof(float) + 64;
}

extern "C" int ov_clip_loss_window_backward(const float* all_img, const float* all_txt, int64_t ld, int64_t set_stride, int N, int E,
                                            int C, const float* logit_scale, const float* terms, const float* grad_loss, int w0, int b,
                                            int norm_rows, float* d_img, float* d_txt, float* d_scale, void* workspace,
                                            size_t workspace_bytes, ov_stream_t stream) {
    if (!all_img || !all_txt || !logit_scale || !terms || !d_img || !d_txt || !workspace) return OV_ERR_INVALID;
    if (N <= 0 || E <= 0 || w0 < 0 || b <= 0 || (int64_t)w0 + b > N || norm_rows <= 0) return OV_ERR_INVALID;
    if (C < 1) return OV_ERR_INVALID;
    if (C > WN_MAXC) return OV_ERR_UNSUPPORTED;
    if (E % 32 || E > 4 * MAXT * 32) return OV_ERR_UNSUPPORTED;
    if (ld < E || (ld & 3) || set_stride < 0 || (set_stride & 3)) return OV_ERR_INVALID;
    if (((uintptr_t)all_img | (uintptr_t)all_txt | (uintptr_t)terms | (uintptr_t)d_img | (uintptr_t)d_txt | (uintptr_t)workspace) & 15)
        return OV_ERR_INVALID;
    if (workspace_bytes < ov_clip_loss_window_backward_workspace_bytes(b, N, C)) return OV_ERR_WORKSPACE;
    WnArgs a;
    a.all_img = all_img; a.all_txt = all_txt; a.ld = ld; a.set_stride = set_stride; a.terms = terms;
    a.d_img = d_img; a.d_txt = d_txt; a.dsc_part = d_scale ? (float*)workspace : nullptr;
    a.w0 = w0; a.b = b; a.N = N; a.E = E; a.C = C; a.nrt = (b + 31) / 32;
    a.scale = logit_scale; a.grad = grad_loss;
    a.inv2cn = 1.0f / (2.0f * (float)C * (float)norm_rows);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(window_loss_bwd, dim3((unsigned)a.nrt, (unsigned)(1 + C)), dim3(256), 0, st, a);
    OV_LAUNCH_CHECK();
    if (d_scale) {
        hipLaunchKernelGGL(scaled_sum<64>, dim3(1), dim3(64), 0, st, a.dsc_part, a.nrt, a.inv2cn, grad_loss, d_scale);
        OV_LAUNCH_CHECK();
    }
    return OV_OK;
}
