// multicap.hip — fused InfoNCE over C caption sets per image (gfx950).
//
// OpenVision trains with two captions per image: bidirectional_contrastive_loss(zimg, ztxt_1, ztxt_2, t, local_loss=True)
// (src/losses/common.py:120-189) takes four log-softmax strips per rank and averages them.  With C sets stacked [C b, E]:
//     A_c = s img all_txt_c^T [b, N],   B_c = s txt_c all_img^T [b, N]
//     loss = 1 / (2 C b) sum_c sum_i [ lse(A_c[i, :]) - A_c[i, i + off] + lse(B_c[i, :]) - B_c[i, i + off] ]
// i.e. the mean over c of the InfoNCE of (img, txt_c); ov_clip_loss (loss.hip) is this file at C = 1.  The building blocks are
// strip.h's: exact-fp32 v_mfma_f32_32x32x2_f32 logit tiles that are never written, the gathered side as the MFMA A operand (row
// reductions are lane-local).  Only a running (max, sum-exp) pair per local row plus the diagonal logit leave the forward kernel.
// Two launches, no atomics, deterministic: partials per (strip, column split, row) -> finalize.  Beyond one pair of strips:
//   * the 2 C strips are the forward grid's third dimension (strip 2c: img rows x all_txt_c, strip 2c + 1: txt_c rows x all_img);
//   * the backward of the image side runs its in-side loop over the C sets INSIDE the kernel, into the same [32 x E] accumulators,
//     and stores once: no C partial gradients to add afterwards;
//   * the gathered operands and their gradients carry a row pitch and a per-set stride, so the all-gather's packed
//     [N, (1 + C) E] buffer is read in place and the gathered-side gradient is written packed for one reduce-scatter.
#include "strip.h"

namespace {

using namespace strip;

constexpr int MC_MAXC = 4;           // caption sets per image

struct McArgs {
    const float* img;       // [b, E]
    const float* txt;       // [C b, E], set c in rows c b ...
    const float* all_img;   // [N, .] row pitch ld
    const float* all_txt;   // set c at all_txt + c * set_stride, [N, .] row pitch ld
    int64_t ld, set_stride;
    float* part;            // [2C][nsplit][bpad][2]  (max, sumexp) in natural-log units
    float* diag;            // [2C][bpad]
    int b, N, E, bpad, nsplit, tiles_per_split, ntiles, label_offset;
    const float* scale;     // device scalar: the logit multiplier
};

__global__ __launch_bounds__(256) void multicap_logits_partial(const McArgs a) {
    __shared__ float red[4][32][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int split = blockIdx.x, rt = blockIdx.y, strip = blockIdx.z;
    const int c = strip >> 1, dir = strip & 1;
    const float* __restrict__ X = dir ? a.txt + (int64_t)c * a.b * a.E : a.img;
    const float* __restrict__ Y = dir ? a.all_img : a.all_txt + (int64_t)c * a.set_stride;
    const int row = rt * 32 + j;
    const int rowc = row < a.b ? row : a.b - 1;
    const float* xp = X + (int64_t)rowc * a.E + 4 * half;
    const int label = row + a.label_offset;
    const float scale = *a.scale;

    float m = -INFINITY, s = 0.f;
    const int t0 = split * a.tiles_per_split;
    int t1 = t0 + a.tiles_per_split;
    if (t1 > a.ntiles) t1 = a.ntiles;
    for (int t = t0 + wave; t < t1; t += 4) {
        int gi = t * 32 + j;
        gi = gi < a.N ? gi : a.N - 1;
        const float* yp = Y + (int64_t)gi * a.ld + 4 * half;
        f32x16_t acc = dot_full(yp, xp, a.E);                     // acc[i] = <Y[t * 32 + tile_row(i, half)], X[row]>
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int g = t * 32 + tile_row(i, half);
            float v = acc[i] * scale;
            if (g == label && row < a.b) a.diag[strip * a.bpad + row] = v;
            if (g >= a.N) v = -INFINITY;
            acc[i] = v;
            mx = fmaxf(mx, v);
        }
        if (mx > -INFINITY) {
            const float mn = fmaxf(m, mx);
            float ps = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) ps += __expf(acc[i] - mn);
            s = s * __expf(m - mn) + ps;
            m = mn;
        }
    }
    // combine the two lane halves of each row, then the four waves
    lse_merge_halves(m, s);
    if (half == 0) { red[wave][j][0] = m; red[wave][j][1] = s; }
    __syncthreads();
    if (wave == 0 && half == 0 && row < a.b) {
        float M = red[0][j][0], S = red[0][j][1];
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_merge(M, S, red[w][j][0], red[w][j][1]);
        float* p = a.part + (((int64_t)strip * a.nsplit + split) * a.bpad + row) * 2;
        p[0] = M; p[1] = S;
    }
}

// terms [4C, b]: per set lse_img, diag_img, lse_txt, diag_txt (strip 2c -> rows 4c, 4c + 1; strip 2c + 1 -> rows 4c + 2, 4c + 3)
__global__ __launch_bounds__(256) void multicap_loss_finalize(const float* __restrict__ part, const float* __restrict__ diag,
                                                              int b, int bpad, int nsplit, int nstrips,
                                                              float* __restrict__ loss_out, float* __restrict__ terms) {
    __shared__ float red[4];
    float local = 0.f;
    for (int i = threadIdx.x; i < nstrips * b; i += blockDim.x) {
        const int strip = i / b, row = i - strip * b;
        float M, S;
        lse_merge_splits(part + ((int64_t)strip * nsplit * bpad + row) * 2, (int64_t)bpad * 2, nsplit, M, S);
        const float lse = M + logf(S);
        const float d = diag[strip * bpad + row];
        if (terms) {
            terms[(int64_t)(2 * strip) * b + row] = lse;
            terms[(int64_t)(2 * strip + 1) * b + row] = d;
        }
        local += lse - d;
    }
    local = wave_sum(local);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) loss_out[0] = (red[0] + red[1] + red[2] + red[3]) / ((float)nstrips * (float)b);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// d loss / d logits = (softmax - onehot) / (2 C b) per strip.  P = exp(s S - lse) - [label] is formed in registers per recomputed
// 32 x 32 logit tile from the forward's per-row lse, and out += P . X_in accumulates in [32 x E] MFMA accumulators split over the
// four waves by e-tile (strip.h).  One workgroup per 32-row out tile; the in-side loop is not split, so the result is deterministic.
// blockIdx.y is the job: 0 = the image side, whose in-side loop runs over all C sets; 1 + c = the text side of set c.
//   GATHERED = false: out rows are LOCAL rows, lse by out row
//       job 0    : d img      = coef sum_c P_img,c . all_txt_c          job 1 + c: d txt_c     = coef P_txt,c . all_img
//   GATHERED = true : out rows are GATHERED rows, lse by in row
//       job 0    : d all_img  = coef sum_c P_txt,c^T . txt_c            job 1 + c: d all_txt_c = coef P_img,c^T . img
struct McBwdArgs {
    const float* img;
    const float* txt;
    const float* all_img;
    const float* all_txt;
    int64_t ld, set_stride;          // gathered operands
    const float* terms;              // [4C, b]
    float* o_img;                    // job 0 output:     d_img [b, E]      | d_all_img, row pitch ldo
    float* o_txt;                    // job 1 + c output: d_txt [C b, E]    | d_all_txt + c * o_set_stride, row pitch ldo
    int64_t ldo, o_set_stride;
    float* dsc_part;                 // [1 + C][nrt]  (GATHERED = false only)
    int b, N, E, C, label_offset, nrt;
    const float* scale;              // device scalars: logit multiplier, upstream gradient of the loss (NULL = 1)
    const float* grad;
    float inv2cb;
};

template <bool GATHERED>
__global__ __launch_bounds__(256) void multicap_loss_bwd(const McBwdArgs a) {
    __shared__ Exchange part;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int rt = blockIdx.x, job = blockIdx.y;
    const int E = a.E, b = a.b;
    const int c0 = job ? job - 1 : 0;                             // the set of a text job
    const int nsets = job ? 1 : a.C;
    // out side: rows [no, .] pitch ldxo; in side of set s: XI0 + s * xi_step, rows [ni, .] pitch ldxi, lse LSE0 + s * 4b
    const float* __restrict__ XO;
    const float* __restrict__ XI0;
    float* __restrict__ OUT;
    int64_t ldxo, ldxi, xi_step;
    if (!GATHERED) {
        XO = job ? a.txt + (int64_t)c0 * b * E : a.img;
        ldxo = E;
        XI0 = job ? a.all_img : a.all_txt;
        ldxi = a.ld;
        xi_step = a.set_stride;                                   // job 0 only walks it
        OUT = job ? (a.o_txt ? a.o_txt + (int64_t)c0 * a.o_set_stride : nullptr) : a.o_img;
    } else {
        XO = job ? a.all_txt + (int64_t)c0 * a.set_stride : a.all_img;
        ldxo = a.ld;
        XI0 = job ? a.img : a.txt;
        ldxi = E;
        xi_step = (int64_t)b * E;
        OUT = job ? (a.o_txt ? a.o_txt + (int64_t)c0 * a.o_set_stride : nullptr) : a.o_img;
    }
    if (OUT == nullptr) return;                                   // output not requested (workgroup-uniform)
    // lse rows of terms: image strip of set c = row 4c, text strip = row 4c + 2.  Local out rows read the strip they belong to;
    // gathered out rows read the OTHER side's strip (d all_img comes from the text strips, d all_txt_c from the image strip).
    const float* __restrict__ LSE0 = a.terms + (int64_t)(4 * c0 + ((job != 0) != GATHERED ? 2 : 0)) * b;
    const int no = GATHERED ? a.N : b, ni = GATHERED ? b : a.N;
    const int net = E >> 5;
    const int nown = (net - wave + 3) >> 2;                       // e-tiles wave, wave + 4, ...
    const int o = rt * 32 + j;
    const int oc = o < no ? o : no - 1;
    const float* xop = XO + (int64_t)oc * ldxo + 4 * half;
    const float scale = *a.scale;
    const float coef = (a.grad ? *a.grad : 1.f) * a.inv2cb * scale;

    f32x16_t acc_o[MAXT];
#pragma unroll
    for (int n = 0; n < MAXT; ++n) acc_o[n] = zero16();
    float dsc = 0.f;

    const int ntiles = (ni + 31) >> 5;
    for (int s = 0; s < nsets; ++s) {
        const float* __restrict__ XI = XI0 + (int64_t)s * xi_step;
        const float* __restrict__ LSE = LSE0 + (int64_t)s * 4 * b;
        const float lse_o = GATHERED ? 0.f : LSE[oc];
        for (int t = 0; t < ntiles; ++t) {
            int gi = t * 32 + j;
            gi = gi < ni ? gi : ni - 1;
            const float* yip = XI + (int64_t)gi * ldxi + 4 * half;
            const f32x16_t acc = dot_wave<false>(yip, xop, E, wave, nown);
            __syncthreads();                                      // the previous tile's partials have been consumed
            put(part, wave, lane, acc);
            __syncthreads();
            f32x16_t p;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float sdot = get(part, i, lane);            // <XI[g], XO[o]>
                const int g = t * 32 + tile_row(i, half);
                const bool valid = o < no && g < ni;
                const float lse_v = GATHERED ? LSE[g < ni ? g : ni - 1] : lse_o;
                const bool hit = GATHERED ? (o == g + a.label_offset) : (g == o + a.label_offset);
                const float pv = valid ? __expf(sdot * scale - lse_v) - (hit ? 1.f : 0.f) : 0.f;
                p[i] = pv;
                dsc = fmaf(pv, sdot, dsc);
            }
            accumulate<MAXT, false, true>(acc_o, p, XI, ldxi, t, ni, E, wave, nown, j, half);
        }
    }
    store<MAXT, false>(acc_o, OUT, GATHERED ? a.ldo : (int64_t)E, rt, no, E, wave, nown, j, half, coef);
    if (!GATHERED) {                                              // d loss / d scale: every wave holds the same P; wave 0 reports
        dsc = wave_sum(dsc);
        if (wave == 0 && lane == 0) a.dsc_part[job * a.nrt + rt] = dsc;
    }
}

// shared by both entry points: sizes, the pitch of the gathered operands, 16-byte alignment of every row
inline int mc_check(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld, int64_t set_stride,
                    int b, int N, int E, int C, int label_offset) {
    if (!img || !txt || !all_img || !all_txt) return OV_ERR_INVALID;
    if (b <= 0 || N < b || E <= 0 || label_offset < 0 || label_offset + b > N) return OV_ERR_INVALID;
    if (C < 1) return OV_ERR_INVALID;
    if (C > MC_MAXC) return OV_ERR_UNSUPPORTED;
    if (ld < E || (ld & 3) || set_stride < 0 || (set_stride & 3)) return OV_ERR_INVALID;
    if (((uintptr_t)img | (uintptr_t)txt | (uintptr_t)all_img | (uintptr_t)all_txt) & 15) return OV_ERR_INVALID;
    return OV_OK;
}

}  // namespace

extern "C" size_t ov_clip_loss_multi_workspace_bytes(int b, int N, int C) {
    if (b <= 0 || N <= 0 || C < 1 || C > MC_MAXC) return 0;
    const StripPlan p = strip_plan(b, N, 2 * C);
    return ((size_t)2 * C * p.nsplit * p.bpad * 2 + (size_t)2 * C * p.bpad) * sizeof(float);
}

extern "C" int ov_clip_loss_multi(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld,
                                  int64_t set_stride, int b, int N, int E, int C, const float* logit_scale, int label_offset,
                                  float* loss_out, float* terms_out, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!loss_out || !workspace || !logit_scale) return OV_ERR_INVALID;
    const int rc = mc_check(img, txt, all_img, all_txt, ld, set_stride, b, N, E, C, label_offset);
    if (rc != OV_OK) return rc;
    if (E % 8) return OV_ERR_UNSUPPORTED;
    if ((uintptr_t)workspace & 15) return OV_ERR_INVALID;
    if (workspace_bytes < ov_clip_loss_multi_workspace_bytes(b, N, C)) return OV_ERR_WORKSPACE;
    const StripPlan p = strip_plan(b, N, 2 * C);
    McArgs a;
    a.img = img; a.txt = txt; a.all_img = all_img; a.all_txt = all_txt; a.ld = ld; a.set_stride = set_stride;
    a.part = (float*)workspace;
    a.diag = a.part + (size_t)2 * C * p.nsplit * p.bpad * 2;
    a.b = b; a.N = N; a.E = E; a.bpad = p.bpad; a.nsplit = p.nsplit; a.tiles_per_split = p.tps; a.ntiles = p.ntiles;
    a.label_offset = label_offset; a.scale = logit_scale;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(multicap_logits_partial, dim3((unsigned)p.nsplit, (unsigned)p.nrt, (unsigned)(2 * C)), dim3(256), 0, st, a);
    OV_LAUNCH_CHECK();
    hipLaunchKernelGGL(multicap_loss_finalize, dim3(1), dim3(256), 0, st, a.part, a.diag, b, p.bpad, p.nsplit, 2 * C, loss_out,
                       terms_out);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" size_t ov_clip_loss_multi_backward_workspace_bytes(int b, int N, int C) {
    if (b <= 0 || N <= 0 || C < 1 || C > MC_MAXC) return 0;
    return (size_t)(1 + C) * ((b + 31) / 32) * sizeof(float) + 64;
}

extern "C" int ov_clip_loss_multi_backward(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld,
                                           int64_t set_stride, int b, int N, int E, int C, const float* logit_scale, int label_offset,
                                           const float* terms, const float* grad_loss, float* d_img, float* d_txt, float* d_all_img,
                                           float* d_all_txt, int64_t ldg, int64_t gset_stride, float* d_scale, void* workspace,
                                           size_t workspace_bytes, ov_stream_t stream) {
    if (!terms || !d_img || !d_txt || !workspace || !logit_scale) return OV_ERR_INVALID;
    const int rc = mc_check(img, txt, all_img, all_txt, ld, set_stride, b, N, E, C, label_offset);
    if (rc != OV_OK) return rc;
    if (E % 32 || E > 4 * MAXT * 32) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)d_img | (uintptr_t)d_txt | (uintptr_t)workspace) & 15) return OV_ERR_INVALID;
    if (d_all_img || d_all_txt) {
        if (ldg < E || (ldg & 3) || gset_stride < 0 || (gset_stride & 3)) return OV_ERR_INVALID;
        if (((uintptr_t)d_all_img | (uintptr_t)d_all_txt) & 15) return OV_ERR_INVALID;
    }
    if (workspace_bytes < ov_clip_loss_multi_backward_workspace_bytes(b, N, C)) return OV_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const float inv2cb = 1.0f / (2.0f * (float)C * (float)b);
    McBwdArgs a;
    a.img = img; a.txt = txt; a.all_img = all_img; a.all_txt = all_txt; a.ld = ld; a.set_stride = set_stride;
    a.terms = terms; a.b = b; a.N = N; a.E = E; a.C = C; a.label_offset = label_offset;
    a.scale = logit_scale; a.grad = grad_loss; a.inv2cb = inv2cb;
    a.dsc_part = (float*)workspace;
    // local side: d img over all sets in one pass, d txt_c per set
    a.o_img = d_img; a.o_txt = d_txt; a.ldo = E; a.o_set_stride = (int64_t)b * E;
    a.nrt = (b + 31) / 32;
    hipLaunchKernelGGL(multicap_loss_bwd<false>, dim3((unsigned)a.nrt, (unsigned)(1 + C)), dim3(256), 0, st, a);
    OV_LAUNCH_CHECK();
    if (d_scale) {
        hipLaunchKernelGGL(scaled_sum<64>, dim3(1), dim3(64), 0, st, a.dsc_part, (1 + C) * a.nrt, inv2cb, grad_loss, d_scale);
        OV_LAUNCH_CHECK();
    }
    if (d_all_img || d_all_txt) {
        // gathered side: d all_img over all sets in one pass, d all_txt_c per set
        a.o_img = d_all_img; a.o_txt = d_all_txt; a.ldo = ldg; a.o_set_stride = gset_stride;
        a.nrt = (N + 31) / 32;
        hipLaunchKernelGGL(multicap_loss_bwd<true>, dim3((unsigned)a.nrt, (unsigned)(1 + C)), dim3(256), 0, st, a);
        OV_LAUNCH_CHECK();
    }
    return OV_OK;
}
