// distill.hip — fused CLIP distillation loss from a frozen teacher (gfx950).
//
// DistillClipLoss (reference open_clip/loss.py:180-216): next to the student's InfoNCE, the cross entropy of the student's
// log-softmax under the teacher's softmax, both ways.  Per direction, with local rows x / u and gathered sets y / v:
//     A = s x y^T [b, N] (student),   T = st u v^T [b, N] (teacher),   Q = softmax(T, dim=1)
//     contrastive_i = lse(A_i) - A[i, i + off]
//     distill_i     = lse(A_i) - sum_j Q_ij A_ij                  ( = -(Q * log_softmax(A)).sum(1), sum_j Q_ij = 1 )
// and both outputs are the mean over the rows and the two directions.  The building blocks are strip.h's, as in multicap.hip:
// exact-fp32 v_mfma_f32_32x32x2_f32 logit tiles that are never written, the gathered side as the MFMA A operand (row reductions
// are lane-local), partial + finalize, no atomics, fixed summation order.  What is new here:
//   * the teacher's lse comes FIRST (one pass of the same strip kernel over the teacher operands), so q = exp(T - lse_T) is final
//     when a tile forms it and the cross term sum_j q A is a plain sum: no running-max rescale;
//   * every tile of the second pass forms two logit tiles, A over E and T over Et;
//   * the backward's tile coefficient is G = (g_c + g_d) P - g_c onehot - g_d Q with P = exp(A - lse_A), Q = exp(T - lse_T), the
//     teacher tile's K reduction split over the four waves in 8-float chunks and summed through LDS like the student's;
//   * nothing flows to the teacher operands or to st.
// Accuracy.  G cancels (P against Q, both against the label), so P and Q must each sum to one over a row as exactly as fp32 allows:
//   * a dot product is formed in ONE summation order everywhere: four k-ordered MFMA chains (the student's over the 32-float e-tiles
//     t, t + 4, ...; the teacher's over the 8-float chunks c, c + 4, ...) added as ((c0 + c1) + c2) + c3.  That is the order the
//     backward's four waves and their LDS exchange produce, so the forward's four accumulators give BITWISE the dots the backward
//     recomputes, and exp(dot * scale - lse) meets the very values its lse was summed from;
//   * the exponent is fma(dot, scale, -lse_hi) - lse_lo: the product is not rounded at the size of the logit, and the lse is kept as
//     an fp32 pair (hi = fl(M + log S), lo = (M - hi) + log S), not rounded at its own size (st = 20: 1e-6).
#include "strip.h"

namespace {

using namespace strip;

// One 32 x 32 tile of dots <Y[.], X[row]> over K floats in the summation order stated above.  yp / xp: this lane's row, already
// offset by 4 * half.  STEP = 32: chain c takes the 32-float e-tiles c, c + 4, ... (K % 32 == 0); STEP = 8: the 8-float chunks.
template <int STEP>
__device__ __forceinline__ f32x16_t dot_tile(const float* yp, const float* xp, int K) {
    f32x16_t c0 = zero16(), c1 = zero16(), c2 = zero16(), c3 = zero16();
    for (int k0 = 0; k0 < K; k0 += 4 * STEP) {
#pragma unroll
        for (int k = 0; k < STEP; k += 8) {
            c0 = mfma4(*(const float4*)(yp + k0 + k), *(const float4*)(xp + k0 + k), c0);
            if (k0 + STEP < K) c1 = mfma4(*(const float4*)(yp + k0 + STEP + k), *(const float4*)(xp + k0 + STEP + k), c1);
            if (k0 + 2 * STEP < K) c2 = mfma4(*(const float4*)(yp + k0 + 2 * STEP + k), *(const float4*)(xp + k0 + 2 * STEP + k), c2);
            if (k0 + 3 * STEP < K) c3 = mfma4(*(const float4*)(yp + k0 + 3 * STEP + k), *(const float4*)(xp + k0 + 3 * STEP + k), c3);
        }
    }
    f32x16_t r;
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = ((c0[i] + c1[i]) + c2[i]) + c3[i];
    return r;
}

struct DsArgs {
    const float* x[2];      // student local rows [b, E]    (dir 0: img, dir 1: txt)
    const float* y[2];      // student gathered, row pitch ld   (dir 0: all_txt, dir 1: all_img)
    const float* u[2];      // teacher local rows [b, Et]
    const float* v[2];      // teacher gathered, row pitch ldt
    int64_t ld, ldt;
    float* tpart;           // teacher pass:  [2][nsplit][bpad][2]  (max, sumexp)
    float* tlse;            // [2][bpad][2]   the teacher's lse per local row as an fp32 pair (hi, lo)
    float* part;            // student pass:  [2][nsplit][bpad][3]  (max, sumexp, sum q A)
    float* diag;            // [2][bpad]
    int b, N, E, Et, bpad, nsplit, tiles_per_split, ntiles, label_offset;
    const float* scale;     // device scalars: the student's and the teacher's logit multiplier
    const float* tscale;
};

// running (max, sum exp) of a row over the logits dots[i] * scale: the maximum over the rounded products, the exponentials of the
// unrounded ones (fma), as the backward forms them
__device__ __forceinline__ void online_lse(const f32x16_t dots, float scale, int g0, int half, int N, float& m, float& s) {
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int g = g0 + tile_row(i, half);
        if (g < N) mx = fmaxf(mx, dots[i] * scale);
    }
    if (mx > -INFINITY) {
        const float mn = fmaxf(m, mx);
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int g = g0 + tile_row(i, half);
            ps += g < N ? __expf(fmaf(dots[i], scale, -mn)) : 0.f;
        }
        s = s * __expf(m - mn) + ps;
        m = mn;
    }
}

// TEACHER = true: the teacher's (max, sumexp) partials alone.  TEACHER = false: the student's, the diagonal and sum q A, with the
// teacher's tile formed next to the student's and q = exp(T - lse_T) from the finished teacher lse.
template <bool TEACHER>
__global__ __launch_bounds__(256) void distill_logits_partial(const DsArgs a) {
    __shared__ float red[4][32][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int split = blockIdx.x, rt = blockIdx.y, dir = blockIdx.z;
    const float* __restrict__ Y = a.y[dir];
    const float* __restrict__ V = a.v[dir];
    const int row = rt * 32 + j;
    const int rowc = row < a.b ? row : a.b - 1;
    const float* xp = a.x[dir] + (int64_t)rowc * a.E + 4 * half;
    const float* up = a.u[dir] + (int64_t)rowc * a.Et + 4 * half;
    const int label = row + a.label_offset;
    const float scale = *a.scale, tscale = *a.tscale;
    float tl_hi = 0.f, tl_lo = 0.f;
    if (!TEACHER) {
        tl_hi = a.tlse[((int64_t)dir * a.bpad + rowc) * 2];
        tl_lo = a.tlse[((int64_t)dir * a.bpad + rowc) * 2 + 1];
    }

    float m = -INFINITY, s = 0.f, cross = 0.f;
    const int t0 = split * a.tiles_per_split;
    int t1 = t0 + a.tiles_per_split;
    if (t1 > a.ntiles) t1 = a.ntiles;
    for (int t = t0 + wave; t < t1; t += 4) {
        int gi = t * 32 + j;
        gi = gi < a.N ? gi : a.N - 1;
        // dots[i] = <V[t * 32 + tile_row(i, half)], U[row]>, and the same of Y and X
        const f32x16_t tdots = dot_tile<8>(V + (int64_t)gi * a.ldt + 4 * half, up, a.Et);
        if (TEACHER) {
            online_lse(tdots, tscale, t * 32, half, a.N, m, s);
        } else {
            const f32x16_t dots = dot_tile<32>(Y + (int64_t)gi * a.ld + 4 * half, xp, a.E);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int g = t * 32 + tile_row(i, half);
                const float v = dots[i] * scale;
                if (g == label && row < a.b) a.diag[dir * a.bpad + row] = v;
                const float q = g < a.N ? __expf(fmaf(tdots[i], tscale, -tl_hi) - tl_lo) : 0.f;
                cross = fmaf(q, v, cross);
            }
            online_lse(dots, scale, t * 32, half, a.N, m, s);
        }
    }
    // combine the two lane halves of each row, then the four waves
    lse_merge_halves(m, s);
    cross += __shfl_xor(cross, 32, 64);
    if (half == 0) { red[wave][j][0] = m; red[wave][j][1] = s; red[wave][j][2] = cross; }
    __syncthreads();
    if (wave == 0 && half == 0 && row < a.b) {
        float M = red[0][j][0], S = red[0][j][1], C = red[0][j][2];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            lse_merge(M, S, red[w][j][0], red[w][j][1]);
            C += red[w][j][2];
        }
        if (TEACHER) {
            float* p = a.tpart + (((int64_t)dir * a.nsplit + split) * a.bpad + row) * 2;
            p[0] = M; p[1] = S;
        } else {
            float* p = a.part + (((int64_t)dir * a.nsplit + split) * a.bpad + row) * 3;
            p[0] = M; p[1] = S; p[2] = C;
        }
    }
}

// the splits' (max, sumexp) of one row (p[0], p[1], then every split_stride floats) -> its lse as an fp32 pair: hi = fl(M + log S),
// lo = what that rounding lost
__device__ __forceinline__ void combine_lse(const float* p, int64_t split_stride, int nsplit, float& hi, float& lo) {
    float M, S;
    lse_merge_splits(p, split_stride, nsplit, M, S);
    const float L = logf(S);
    hi = __fadd_rn(M, L);                                         // two-sum: hi + lo == M + L exactly
    const float bb = __fsub_rn(hi, M);
    lo = __fadd_rn(__fsub_rn(M, __fsub_rn(hi, bb)), __fsub_rn(L, bb));
}

__global__ __launch_bounds__(256) void distill_teacher_lse(const float* __restrict__ tpart, int b, int bpad, int nsplit,
                                                           float* __restrict__ tlse) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * b; i += gridDim.x * blockDim.x) {
        const int dir = i / b, row = i - dir * b;
        float hi, lo;
        combine_lse(tpart + ((int64_t)dir * nsplit * bpad + row) * 2, (int64_t)bpad * 2, nsplit, hi, lo);
        tlse[((int64_t)dir * bpad + row) * 2] = hi;
        tlse[((int64_t)dir * bpad + row) * 2 + 1] = lo;
    }
}

// terms [12, b]: rows 0 ... 3 the student's lse_img, diag_img, lse_txt, diag_txt (ov_clip_loss's block), then per direction the
// teacher's lse and the cross sum (4 = tlse_img, 5 = cross_img, 6 = tlse_txt, 7 = cross_txt), then the low parts of the four lse:
// 8 = lse_img, 9 = lse_txt, 10 = tlse_img, 11 = tlse_txt (an lse is hi + lo; the rows above hold hi)
__global__ __launch_bounds__(256) void distill_loss_finalize(const float* __restrict__ part, const float* __restrict__ diag,
                                                             const float* __restrict__ tlse, int b, int bpad, int nsplit,
                                                             float* __restrict__ contrastive_out, float* __restrict__ distill_out,
                                                             float* __restrict__ terms) {
    __shared__ float red[2][4];
    float lc = 0.f, ld = 0.f;
    for (int i = threadIdx.x; i < 2 * b; i += blockDim.x) {
        const int dir = i / b, row = i - dir * b;
        const float* p = part + ((int64_t)dir * nsplit * bpad + row) * 3;
        float hi, lo, C = 0.f;
        combine_lse(p, (int64_t)bpad * 3, nsplit, hi, lo);
        for (int sp = 0; sp < nsplit; ++sp) C += p[(int64_t)sp * bpad * 3 + 2];
        const float d = diag[dir * bpad + row];
        terms[(2 * dir) * b + row] = hi;
        terms[(2 * dir + 1) * b + row] = d;
        terms[(4 + 2 * dir) * b + row] = tlse[((int64_t)dir * bpad + row) * 2];
        terms[(5 + 2 * dir) * b + row] = C;
        terms[(8 + dir) * b + row] = lo;
        terms[(10 + dir) * b + row] = tlse[((int64_t)dir * bpad + row) * 2 + 1];
        lc += (hi - d) + lo;
        ld += (hi - C) + lo;
    }
    lc = wave_sum(lc);
    ld = wave_sum(ld);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lc; red[1][threadIdx.x >> 6] = ld; }
    __syncthreads();
    if (threadIdx.x == 0) {
        contrastive_out[0] = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (2.0f * (float)b);
        distill_out[0] = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (2.0f * (float)b);
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// As multicap_loss_bwd (multicap.hip): the 32 x 32 logit tiles are recomputed, the coefficient tile is formed in registers and
// out += G . X_in accumulates in [32 x E] MFMA accumulators split over the four waves by e-tile; one workgroup per 32-row out tile
// and direction, the in-side loop not split.  Here G = (g_c + g_d) exp(A - lse_A) - g_c [label] - g_d exp(T - lse_T).
//   GATHERED = false: out rows are LOCAL rows (both lse by out row):      d x[r]  = s / (2 b) sum_g G[r, g] y[g]
//   GATHERED = true : out rows are GATHERED rows (both lse by in row):    d y[g]  = s / (2 b) sum_r G[r, g] x[r]
struct DsBwdArgs {
    const float* xo[2];     // student out-side rows, pitch ldxo
    const float* xi[2];     // student in-side rows, pitch ldxi
    const float* uo[2];     // teacher out-side rows, pitch lduo
    const float* ui[2];     // teacher in-side rows, pitch ldui
    const float* lse[2];    // per LOCAL row, the high parts: student, teacher
    const float* tlse[2];
    const float* lse_lo[2]; // and the low parts
    const float* tlse_lo[2];
    float* out[2];          // pitch ldout
    int64_t ldxo, ldxi, lduo, ldui, ldout;
    float* dsc_part;        // [2][nrt]  (GATHERED = false only)
    int no, ni, E, Et, label_offset, nrt;
    const float* scale;     // device scalars: the two multipliers, the upstream gradients of the two outputs
    const float* tscale;
    const float* gc;
    const float* gd;
    float inv2b;
};

template <bool GATHERED>
__global__ __launch_bounds__(256) void distill_loss_bwd(const DsBwdArgs a) {
    __shared__ Exchange part, tpart;                              // the student's partial tiles, the teacher's
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int rt = blockIdx.x, dir = blockIdx.y;
    const float* __restrict__ XI = a.xi[dir];
    const float* __restrict__ UI = a.ui[dir];
    const float* __restrict__ LSE = a.lse[dir];
    const float* __restrict__ TLSE = a.tlse[dir];
    const float* __restrict__ LSE_LO = a.lse_lo[dir];
    const float* __restrict__ TLSE_LO = a.tlse_lo[dir];
    float* __restrict__ OUT = a.out[dir];
    if (OUT == nullptr) return;                                   // direction not requested (workgroup-uniform)
    const int E = a.E, net = E >> 5;
    const int nown = (net - wave + 3) >> 2;                       // e-tiles wave, wave + 4, ...
    const int o = rt * 32 + j;
    const int oc = o < a.no ? o : a.no - 1;
    const float* xop = a.xo[dir] + (int64_t)oc * a.ldxo + 4 * half;
    const float* uop = a.uo[dir] + (int64_t)oc * a.lduo + 4 * half;
    const float lse_o = GATHERED ? 0.f : LSE[oc];
    const float tlse_o = GATHERED ? 0.f : TLSE[oc];
    const float lse_lo_o = GATHERED ? 0.f : LSE_LO[oc];
    const float tlse_lo_o = GATHERED ? 0.f : TLSE_LO[oc];
    const float scale = *a.scale, tscale = *a.tscale;
    const float gc = *a.gc, gd = *a.gd;
    const float gsum = gc + gd;
    const float coef = a.inv2b * scale;

    f32x16_t acc_o[MAXT];
#pragma unroll
    for (int n = 0; n < MAXT; ++n) acc_o[n] = zero16();
    float dsc = 0.f;

    const int ntiles = (a.ni + 31) >> 5;
    for (int t = 0; t < ntiles; ++t) {
        int gi = t * 32 + j;
        gi = gi < a.ni ? gi : a.ni - 1;
        const float* yip = XI + (int64_t)gi * a.ldxi + 4 * half;
        const float* uip = UI + (int64_t)gi * a.ldui + 4 * half;
        const f32x16_t acc = dot_wave<false>(yip, xop, E, wave, nown);
        f32x16_t tacc = zero16();
        for (int k0 = 8 * wave; k0 < a.Et; k0 += 32)              // the teacher's K in 8-float chunks: wave, wave + 4, ...
            tacc = mfma4(*(const float4*)(uip + k0), *(const float4*)(uop + k0), tacc);
        __syncthreads();                                          // the previous tile's partials have been consumed
        put(part, wave, lane, acc);
        put(tpart, wave, lane, tacc);
        __syncthreads();
        f32x16_t p;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float sdot = get(part, i, lane);         // <XI[g], XO[o]>; the teacher's alike
            const float tdot = get(tpart, i, lane);
            const int g = t * 32 + tile_row(i, half);
            const bool valid = o < a.no && g < a.ni;
            const int gc_ = g < a.ni ? g : a.ni - 1;
            const float lse_v = GATHERED ? LSE[gc_] : lse_o;
            const float tlse_v = GATHERED ? TLSE[gc_] : tlse_o;
            const float lse_lo_v = GATHERED ? LSE_LO[gc_] : lse_lo_o;
            const float tlse_lo_v = GATHERED ? TLSE_LO[gc_] : tlse_lo_o;
            const bool hit = GATHERED ? (o == g + a.label_offset) : (g == o + a.label_offset);
            const float pv = valid ? gsum * __expf(fmaf(sdot, scale, -lse_v) - lse_lo_v) - (hit ? gc : 0.f) -
                                         gd * __expf(fmaf(tdot, tscale, -tlse_v) - tlse_lo_v)
                                   : 0.f;
            p[i] = pv;
            dsc = fmaf(pv, sdot, dsc);
        }
        accumulate<MAXT, false, false>(acc_o, p, XI, a.ldxi, t, a.ni, E, wave, nown, j, half);
    }
    store<MAXT, false>(acc_o, OUT, a.ldout, rt, a.no, E, wave, nown, j, half, coef);
    if (!GATHERED) {                                              // d / d scale: every wave holds the same G; wave 0 reports
        dsc = wave_sum(dsc);
        if (wave == 0 && lane == 0) a.dsc_part[dir * a.nrt + rt] = dsc;
    }
}

// shared by both entry points: sizes, the pitches of the gathered operands, 16-byte alignment of every base pointer
inline int ds_check(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld, const float* t_img,
                    const float* t_txt, const float* t_all_img, const float* t_all_txt, int64_t ldt, int b, int N, int E, int Et,
                    int label_offset) {
    if (!img || !txt || !all_img || !all_txt || !t_img || !t_txt || !t_all_img || !t_all_txt) return OV_ERR_INVALID;
    if (b <= 0 || N < b || E <= 0 || Et <= 0 || label_offset < 0 || label_offset + b > N) return OV_ERR_INVALID;
    if (ld < E || (ld & 3) || ldt < Et || (ldt & 3)) return OV_ERR_INVALID;
    if (((uintptr_t)img | (uintptr_t)txt | (uintptr_t)all_img | (uintptr_t)all_txt | (uintptr_t)t_img | (uintptr_t)t_txt |
         (uintptr_t)t_all_img | (uintptr_t)t_all_txt) & 15)
        return OV_ERR_INVALID;
    if (E % 32 || E > 4 * MAXT * 32 || Et % 8) return OV_ERR_UNSUPPORTED;
    return OV_OK;
}

}  // namespace

// workspace: [teacher partials 2 nsplit bpad 2][teacher lse 2 bpad 2][student partials 2 nsplit bpad 3][diag 2 bpad]
extern "C" size_t ov_distill_loss_workspace_bytes(int b, int N) {
    if (b <= 0 || N <= 0) return 0;
    const StripPlan p = strip_plan(b, N, 2);
    return ((size_t)2 * p.nsplit * p.bpad * 5 + (size_t)2 * p.bpad * 3) * sizeof(float);
}

extern "C" int ov_distill_loss(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld,
                               const float* t_img, const float* t_txt, const float* t_all_img, const float* t_all_txt, int64_t ldt,
                               int b, int N, int E, int Et, const float* logit_scale, const float* t_logit_scale, int label_offset,
                               float* contrastive_out, float* distill_out, float* terms_out, void* workspace, size_t workspace_bytes,
                               ov_stream_t stream) {
    if (!contrastive_out || !distill_out || !terms_out || !workspace || !logit_scale || !t_logit_scale) return OV_ERR_INVALID;
    const int rc = ds_check(img, txt, all_img, all_txt, ld, t_img, t_txt, t_all_img, t_all_txt, ldt, b, N, E, Et, label_offset);
    if (rc != OV_OK) return rc;
    if ((uintptr_t)workspace & 15) return OV_ERR_INVALID;
    if (workspace_bytes < ov_distill_loss_workspace_bytes(b, N)) return OV_ERR_WORKSPACE;
    const StripPlan p = strip_plan(b, N, 2);
    DsArgs a;
    a.x[0] = img; a.y[0] = all_txt; a.u[0] = t_img; a.v[0] = t_all_txt;
    a.x[1] = txt; a.y[1] = all_img; a.u[1] = t_txt; a.v[1] = t_all_img;
    a.ld = ld; a.ldt = ldt;
    a.tpart = (float*)workspace;
    a.tlse = a.tpart + (size_t)2 * p.nsplit * p.bpad * 2;
    a.part = a.tlse + (size_t)2 * p.bpad * 2;
    a.diag = a.part + (size_t)2 * p.nsplit * p.bpad * 3;
    a.b = b; a.N = N; a.E = E; a.Et = Et; a.bpad = p.bpad; a.nsplit = p.nsplit; a.tiles_per_split = p.tps; a.ntiles = p.ntiles;
    a.label_offset = label_offset; a.scale = logit_scale; a.tscale = t_logit_scale;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nsplit, (unsigned)p.nrt, 2);
    // the teacher's lse per row and direction first, then the pass that forms both tiles
    hipLaunchKernelGGL(distill_logits_partial<true>, grid, dim3(256), 0, st, a);
    OV_LAUNCH_CHECK();
    hipLaunchKernelGGL(distill_teacher_lse, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, a.tpart, b, p.bpad, p.nsplit, a.tlse);
    OV_LAUNCH_CHECK();
    hipLaunchKernelGGL(distill_logits_partial<false>, grid, dim3(256), 0, st, a);
    OV_LAUNCH_CHECK();
    hipLaunchKernelGGL(distill_loss_finalize, dim3(1), dim3(256), 0, st, a.part, a.diag, a.tlse, b, p.bpad, p.nsplit, contrastive_out,
                       distill_out, terms_out);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

extern "C" size_t ov_distill_loss_backward_workspace_bytes(int b, int N) {
    if (b <= 0 || N <= 0) return 0;
    return (size_t)2 * ((b + 31) / 32) * sizeof(float) + 64;
}

extern "C" int ov_distill_loss_backward(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld,
                                        const float* t_img, const float* t_txt, const float* t_all_img, const float* t_all_txt,
                                        int64_t ldt, int b, int N, int E, int Et, const float* logit_scale, const float* t_logit_scale,
                                        int label_offset, const float* terms, const float* grad_contrastive, const float* grad_distill,
                                        float* d_img, float* d_txt, float* d_all_img, float* d_all_txt, int64_t ldg, float* d_scale,
                                        void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!terms || !grad_contrastive || !grad_distill || !d_img || !d_txt || !workspace || !logit_scale || !t_logit_scale)
        return OV_ERR_INVALID;
    const int rc = ds_check(img, txt, all_img, all_txt, ld, t_img, t_txt, t_all_img, t_all_txt, ldt, b, N, E, Et, label_offset);
    if (rc != OV_OK) return rc;
    if (((uintptr_t)d_img | (uintptr_t)d_txt | (uintptr_t)workspace) & 15) return OV_ERR_INVALID;
    if (d_all_img || d_all_txt) {
        if (ldg < E || (ldg & 3)) return OV_ERR_INVALID;
        if (((uintptr_t)d_all_img | (uintptr_t)d_all_txt) & 15) return OV_ERR_INVALID;
    }
    if (workspace_bytes < ov_distill_loss_backward_workspace_bytes(b, N)) return OV_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const float inv2b = 1.0f / (2.0f * (float)b);
    DsBwdArgs a;
    a.E = E; a.Et = Et; a.label_offset = label_offset; a.scale = logit_scale; a.tscale = t_logit_scale;
    a.gc = grad_contrastive; a.gd = grad_distill; a.inv2b = inv2b;
    a.lse[0] = terms; a.lse[1] = terms + (size_t)2 * b;
    a.tlse[0] = terms + (size_t)4 * b; a.tlse[1] = terms + (size_t)6 * b;
    a.lse_lo[0] = terms + (size_t)8 * b; a.lse_lo[1] = terms + (size_t)9 * b;
    a.tlse_lo[0] = terms + (size_t)10 * b; a.tlse_lo[1] = terms + (size_t)11 * b;
    a.dsc_part = (float*)workspace;
    // local side: d img = c G_i . all_txt, d txt = c G_t . all_img
    a.xo[0] = img; a.xi[0] = all_txt; a.uo[0] = t_img; a.ui[0] = t_all_txt; a.out[0] = d_img;
    a.xo[1] = txt; a.xi[1] = all_img; a.uo[1] = t_txt; a.ui[1] = t_all_img; a.out[1] = d_txt;
    a.ldxo = E; a.ldxi = ld; a.lduo = Et; a.ldui = ldt; a.ldout = E;
    a.no = b; a.ni = N; a.nrt = (b + 31) / 32;
    hipLaunchKernelGGL(distill_loss_bwd<false>, dim3((unsigned)a.nrt, 2), dim3(256), 0, st, a);
    OV_LAUNCH_CHECK();
    if (d_scale) {
        hipLaunchKernelGGL(scaled_sum<64>, dim3(1), dim3(64), 0, st, a.dsc_part, 2 * a.nrt, inv2b, nullptr, d_scale);
        OV_LAUNCH_CHECK();
    }
    if (d_all_img || d_all_txt) {
        // gathered side: d all_txt = c G_i^T . img (direction 0), d all_img = c G_t^T . txt (direction 1)
        a.xo[0] = all_txt; a.xi[0] = img; a.uo[0] = t_all_txt; a.ui[0] = t_img; a.out[0] = d_all_txt;
        a.xo[1] = all_img; a.xi[1] = txt; a.uo[1] = t_all_img; a.ui[1] = t_txt; a.out[1] = d_all_img;
        a.ldxo = ld; a.ldxi = E; a.lduo = ldt; a.ldui = Et; a.ldout = ldg;
        a.no = N; a.ni = b; a.nrt = (N + 31) / 32;
        hipLaunchKernelGGL(distill_loss_bwd<true>, dim3((unsigned)a.nrt, 2), dim3(256), 0, st, a);
        OV_LAUNCH_CHECK();
    }
    return OV_OK;
}
