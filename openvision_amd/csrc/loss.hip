// loss.hip — the CLIP InfoNCE entry points and the plain logit matrix (gfx950).
//
// ClipLoss.get_logits + F.cross_entropy both ways (reference open_clip/loss.py:102-131, local_loss branch :108-110, labels
// arange(b) + b*rank :93-94; JAX twin src/losses/common.py:120-189):
//     loss = ( CE(s * img @ all_txt^T, i + off) + CE(s * txt @ all_img^T, i + off) ) / 2
// is the multi-caption loss of multicap.hip with one caption set and dense [N, E] gathered operands: the same plan, the same
// summation order, the same [4, b] terms block.  ov_clip_loss* check their own arguments and run those kernels.
#include "strip.h"

namespace {

// out[i, j] = scale * <X[i, :], Y[j, :]>  (CLIP.get_logits, model.py:286-293; fp32-exact MFMA). One wave per 32x32 tile.
__global__ __launch_bounds__(64) void logits_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                    float* __restrict__ out, int64_t ldo, int n1, int n2, int E,
                                                    float scale, const float* __restrict__ scale_dev) {
    if (scale_dev) scale *= *scale_dev;
    const int lane = threadIdx.x & 63;
    const int j = lane & 31, half = lane >> 5;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const int xi = (i0 + j) < n1 ? (i0 + j) : n1 - 1;
    const int yj = (j0 + j) < n2 ? (j0 + j) : n2 - 1;
    const f32x16_t acc = strip::dot_full(Y + (int64_t)yj * E + 4 * half, X + (int64_t)xi * E + 4 * half, E);
    const int row = i0 + j;
    if (row < n1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int col = j0 + strip::tile_row(i, half);
            if (col < n2) out[(int64_t)row * ldo + col] = acc[i] * scale;
        }
    }
}

}  // namespace

extern "C" size_t ov_clip_loss_workspace_bytes(int b, int N) { return ov_clip_loss_multi_workspace_bytes(b, N, 1); }

extern "C" int ov_clip_loss(const float* img, const float* txt, const float* all_img, const float* all_txt, int b,
                            int N, int E, const float* logit_scale, int label_offset, float* loss_out, float* lse_out,
                            void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!img || !txt || !all_img || !all_txt || !loss_out || !workspace || !logit_scale) return OV_ERR_INVALID;
    if (b <= 0 || N < b || E <= 0 || label_offset < 0 || label_offset + b > N) return OV_ERR_INVALID;
    if (E % 8) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)img | (uintptr_t)txt | (uintptr_t)all_img | (uintptr_t)all_txt | (uintptr_t)workspace) & 15)
        return OV_ERR_INVALID;
    if (workspace_bytes < ov_clip_loss_workspace_bytes(b, N)) return OV_ERR_WORKSPACE;
    return ov_clip_loss_multi(img, txt, all_img, all_txt, E, 0, b, N, E, 1, logit_scale, label_offset, loss_out, lse_out, workspace,
                              workspace_bytes, stream);
}

extern "C" size_t ov_clip_loss_backward_workspace_bytes(int b, int N) {
    return ov_clip_loss_multi_backward_workspace_bytes(b, N, 1);
}

extern "C" int ov_clip_loss_backward(const float* img, const float* txt, const float* all_img, const float* all_txt, int b, int N,
                                     int E, const float* logit_scale, int label_offset, const float* lse_terms,
                                     const float* grad_loss, float* d_img, float* d_txt, float* d_all_img, float* d_all_txt,
                                     float* d_scale, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!img || !txt || !all_img || !all_txt || !lse_terms || !d_img || !d_txt || !workspace || !logit_scale) return OV_ERR_INVALID;
    if (b <= 0 || N < b || E <= 0 || label_offset < 0 || label_offset + b > N) return OV_ERR_INVALID;
    if (E % 32 || E > 4 * strip::MAXT * 32) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)img | (uintptr_t)txt | (uintptr_t)all_img | (uintptr_t)all_txt | (uintptr_t)workspace) & 15) return OV_ERR_INVALID;
    if (workspace_bytes < ov_clip_loss_backward_workspace_bytes(b, N)) return OV_ERR_WORKSPACE;
    return ov_clip_loss_multi_backward(img, txt, all_img, all_txt, E, 0, b, N, E, 1, logit_scale, label_offset, lse_terms, grad_loss,
                                       d_img, d_txt, d_all_img, d_all_txt, E, 0, d_scale, workspace, workspace_bytes, stream);
}

extern "C" int ov_logits(const float* X, const float* Y, float* out, int64_t ldo, int n1, int n2, int E, float scale,
                         const float* scale_dev, ov_stream_t stream) {
    if (!X || !Y || !out || n1 <= 0 || n2 <= 0 || E <= 0 || ldo < n2) return OV_ERR_INVALID;
    if (E % 8) return OV_ERR_UNSUPPORTED;
    if (((uintptr_t)X | (uintptr_t)Y) & 15) return OV_ERR_INVALID;
    hipLaunchKernelGGL(logits_kernel, dim3((unsigned)((n2 + 31) / 32), (unsigned)((n1 + 31) / 32)), dim3(64), 0,
                       (hipStream_t)stream, X, Y, out, ldo, n1, n2, E, scale, scale_dev);
    OV_LAUNCH_CHECK();
    return OV_OK;
}
