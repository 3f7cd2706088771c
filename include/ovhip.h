/* ovhip.h — C ABI of libovhip.so: the MI355X (gfx950) encode-and-contrast path of OpenVision.
 *
 * Drop-in boundary.  The reference has no FFI layer: its "operator API" for this path
 * is the Python surface of open_clip.model.CLIP / open_clip.loss.ClipLoss, whose arithmetic is
 * delegated to torch aten kernels.  Each entry point below replaces the aten work behind one piece of
 * that surface (reference paths relative to /root/reference/src/convert_upload/open_clip/):
 *
 *   ov_layernorm        LayerNorm / LayerNormFp32.forward                     transformer.py:15-30
 *   ov_gemm             nn.Linear (c_fc/c_proj/out_proj/in_proj), `@ proj`    transformer.py:225,232-236,645-646
 *   ov_rowstats+ov_gemm_ln  ln_1 -> in_proj and ln_2 -> c_fc fused (LN folded into the GEMM epilogue) transformer.py:263-264
 *   ov_attention        nn.MultiheadAttention core (softmax(qk^T/sqrt(hd)) v) transformer.py:239-252
 *   ov_im2col_patches   conv1 (stride = kernel = P) operand gather            transformer.py:469,610-612
 *   ov_cls_rows         class_embedding concat + pos-emb row 0                transformer.py:615-617
 *   ov_mean_pool        _global_pool 'avg' / 'tok'                            transformer.py:599-603
 *   ov_mlp_out_pooled   _global_pool 'avg' of the last block's output, through its c_proj   transformer.py:264,599-603
 *   ov_text_embed       token_embedding(text) + positional_embedding         model.py:272-274
 *   ov_gather_rows      text_global_pool 'last' / 'first'                     transformer.py:655-658
 *   ov_token_argmax     text.argmax(dim=-1), the EOT position of each caption transformer.py:655-658
 *   ov_gather_rows_at   text_global_pool 'argmax': one row per caption        transformer.py:655-658
 *   ov_l2norm           F.normalize(x, dim=-1)                                model.py:267,284
 *   ov_logits           CLIP.get_logits (scale * img @ txt^T)                 model.py:286-293
 *   ov_clip_loss        ClipLoss.get_logits + cross_entropy both ways         loss.py:102-131
 *   ov_clip_loss_multi  bidirectional_contrastive_loss, C caption sets        src/losses/common.py:120-189
 *   ov_distill_loss     DistillClipLoss: InfoNCE + teacher-softmax cross entropy   loss.py:180-216
 *   ov_siglip_loss      SigLipLoss._loss summed over every text block          loss.py:307-414
 *   ov_gemm_fp8         the same nn.Linear on fp8 e4m3 operands (config #5)           transformer.py:225,232-236
 *   ov_preprocess_image transforms.Resize -> ToTensor -> Normalize (Pillow-exact)  ov-zero-shot-test.py:72-77, transform.py:355-392
 *   ov_train_transform  RandomResizedCrop -> color_jitter -> gray_scale -> ToTensor -> Normalize, a batch per call   transform.py:307-358
 *   ov_class_mean_normalize / ov_topk   zero-shot classifier weights, argmax / recall@k ranking   zero_shot_classifier.py:54-57,
 *                       src/evaluators/proj/image_text/{discriminative_classifier.py:305-323, image_text_retrieval.py:24-87}
 *   ov_tower_*          Transformer.forward (the resblock loop)               transformer.py:355-366, 254-265
 *   ov_vision_* / ov_text_*   VisionTransformer.forward / CLIP.encode_text    transformer.py:609-651, model.py:269-284
 *
 * Conventions: plain pointers and sizes only (no torch types).  All pointers are DEVICE pointers owned
 * by the caller unless stated; every call enqueues on `stream` (a hipStream_t passed as void*) and
 * returns without synchronising.  Return value: 0 = OK, negative = error (see ov_error_string); nothing
 * throws across the boundary.  No call allocates device memory: workspaces are sized by
 * ov_*_workspace_bytes and provided by the caller.  Activations are bf16 row-major; LN affine params,
 * biases and final embeddings are fp32 (the reference's bf16 mode keeps LN in fp32: model.py:143).
 */
#ifndef OVHIP_H
#define OVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OV_ABI_VERSION 2       /* 2: logit scale / upstream loss gradient are device scalars (ov_clip_loss*, ov_logits) */

typedef void* ov_stream_t;            /* hipStream_t */
typedef uint16_t ov_bf16;             /* raw bfloat16 bits */

enum ov_status {
    OV_OK = 0,
    OV_ERR_INVALID = -1,              /* bad argument (null pointer, size, alignment) */
    OV_ERR_UNSUPPORTED = -2,          /* shape outside what the kernels cover */
    OV_ERR_WORKSPACE = -3,            /* workspace too small */
    OV_ERR_NO_DEVICE = -4,            /* no gfx950 device visible */
    OV_ERR_HIP = -1000                /* -(1000 + hipError_t) */
};

enum ov_dtype { OV_F32 = 0, OV_BF16 = 1 };

enum ov_epilogue {
    OV_EPI_BIAS = 0,                  /* C = bf16(acc + bias)                (bias may be NULL) */
    OV_EPI_BIAS_GELU_ERF = 1,         /* C = bf16(gelu_erf(acc + bias))      vision MLP, vit.py:202 */
    OV_EPI_BIAS_GELU_TANH = 2,        /* C = bf16(gelu_tanh(acc + bias))     text MLP, text_transformer.py:117 */
    OV_EPI_BIAS_RESIDUAL = 3,         /* C = bf16(bf16(acc + bias) + R)      x = x + f(x), transformer.py:263-264 */
    OV_EPI_GELU_GRAD_ERF = 4,         /* C = bf16(bf16(acc + bias) * gelu_erf'(R))   backward through the MLP's GELU: R = the c_fc */
    OV_EPI_GELU_GRAD_TANH = 5         /* C = bf16(bf16(acc + bias) * gelu_tanh'(R))  pre-activation (ov_gemm_keep), acc = dy Wproj */
};

int         ov_abi_version(void);
const char* ov_error_string(int status);
/* 0 if a gfx950 device is usable by this process, else OV_ERR_NO_DEVICE / OV_ERR_HIP-x. */
int         ov_device_check(void);

/* ---- granular operators ------------------------------------------------------------------------ */

/* y[r,:] = (x[r,:] - mean) * rsqrt(var + eps) * gamma + beta ; fp32 statistics (biased variance).
 * x_dtype/y_dtype: OV_BF16 or OV_F32.  D % 8 == 0, D <= 8192.  ldx/ldy in elements. */
int ov_layernorm(const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* beta,
                 void* y, int y_dtype, int64_t ldy, int64_t rows, int D, float eps, ov_stream_t stream);

/* C[M,N] = epilogue(A[M,K] * W[N,K]^T + bias[N]).  A, W, C, R bf16 row-major; bias fp32 or NULL.
 * K % 64 == 0; lda, ldw, ldc, ldr % 8 == 0; N % 8 == 0.
 * Row remapping for the patch-embed use (0 = identity):
 *   out_group  > 0 : output row = m + m / out_group + 1      (skip one cls row per image)
 *   resid_mod  > 0 : residual row = (m % resid_mod) + resid_off   (pos-emb table broadcast over batch)
 * C may alias R when the row maps are identities (in-place residual add). */
int ov_gemm(const ov_bf16* A, int64_t lda, const ov_bf16* W, int64_t ldw, const float* bias,
            ov_bf16* C, int64_t ldc, int64_t M, int N, int K, int epilogue,
            const ov_bf16* R, int64_t ldr, int out_group, int resid_mod, int resid_off,
            ov_stream_t stream);

/* `batch` independent products C_z = A_z W_z^T (bf16 out, no bias, no epilogue) in one launch; operand z = base + z * stride
 * (elements).  With A_z / W_z = column ranges of one operand pair this is split-K with bf16 partials (ov_linear_backward's dW).
 * Same shape rules as ov_gemm; strides % 8 == 0; batch <= 65535. */
int ov_gemm_batched(const ov_bf16* A, int64_t lda, int64_t stride_a, const ov_bf16* W, int64_t ldw, int64_t stride_w, ov_bf16* C,
                    int64_t ldc, int64_t stride_c, int64_t M, int N, int K, int batch, ov_stream_t stream);

/* Split-K partials of C = P^T Q with BOTH operands row-major over the contraction rows (P [Mc, NI], Q [Mc, NJ]): partial z contracts
 * rows [z * chunk, min(Mc, (z + 1) * chunk)) into C + z * stride_c (bf16 [NI, NJ], no bias).  The weight-gradient product
 * dW = dY^T X of ov_linear_backward without explicit transposes (transposing LDS reads, ds_read_b64_tr_b16).  Mc % 64 == 0,
 * chunk % 64 == 0, (batch - 1) * chunk < Mc <= batch * chunk, NI / NJ / leading dimensions % 8 == 0.
 * psum (or NULL): fp32 [batch][NI], psum[z][i] = sum of P[m, i] over the rows of partial z -- the bias gradient sum_m dY[m, i] from the
 * fragments the product already holds (one more MFMA against an all-ones operand), instead of a second pass over dY. */
int ov_gemm_tn_batched(const ov_bf16* P, int64_t ldp, const ov_bf16* Q, int64_t ldq, ov_bf16* C, int64_t ldc, int64_t stride_c, int64_t Mc,
                       int NI, int NJ, int64_t chunk, int batch, float* psum, ov_stream_t stream);

/* LayerNorm folded into the following Linear (LN(x) W^T + b without materialising LN(x)):
 *   C = epilogue( rstd[m] * (x W'^T - mean[m] * colsum[n]) + cvec[n] ),
 *   W'[n,k] = bf16(gamma[k] W[n,k]), colsum[n] = sum_k W'[n,k], cvec[n] = sum_k beta[k] W[n,k] + b[n]   (built once at pack time),
 *   rowstats[m] = {mean, rstd} of row m of x from ov_rowstats (fp32 [M,2]).  Epilogues BIAS / GELU only. */
int ov_gemm_ln(const ov_bf16* X, int64_t ldx, const ov_bf16* Wg, int64_t ldw, const float* cvec, const float* colsum,
               const float* rowstats, ov_bf16* C, int64_t ldc, int64_t M, int N, int K, int epilogue, ov_stream_t stream);

/* ov_gemm with a GELU epilogue (OV_EPI_BIAS_GELU_ERF / _TANH) that also keeps the pre-activation:
 *   C = bf16(gelu(A W^T + bias)),  C2 = bf16(A W^T + bias)   [M, N], ld = ldc2
 * -- the c_fc of the training forward, so that the backward does not run that product again (transformer.py:232-236). */
int ov_gemm_keep(const ov_bf16* A, int64_t lda, const ov_bf16* W, int64_t ldw, const float* bias, ov_bf16* C, int64_t ldc,
                 ov_bf16* C2, int64_t ldc2, int64_t M, int N, int K, int epilogue, ov_stream_t stream);

/* rowstats[r] = {mean, rsqrt(var + eps)} of x[r, 0:D] (bf16 rows, fp32 two-pass statistics, biased variance). */
int ov_rowstats(const ov_bf16* x, int64_t ldx, float* rowstats, int64_t rows, int D, float eps, ov_stream_t stream);

/* The same statistics through partial sums (the LayerNorm of transformer.py:15-30 in front of the folded QKV / c_fc GEMMs, without a
 * separate pass over the residual stream): parts[r][D / 32] = {sum, sum of squares} (fp32) of the bf16 values x[r, 32 g .. 32 g + 31], in
 * ONE fixed association order -- ov_gemm_rowparts leaves exactly these numbers for its output rows (from its epilogue where the kernel
 * can, by this pass otherwise: bitwise the same), ov_rowstats_finalize turns them into {mean, rsqrt(var + eps)} with var = E[x^2] -
 * mean^2 (one pass; fp32).  D % 32 == 0. */
int ov_rowparts(const ov_bf16* x, int64_t ldx, float* parts, int64_t rows, int D, ov_stream_t stream);
int ov_rowstats_finalize(const float* parts, float* rowstats, int64_t rows, int D, float eps, ov_stream_t stream);
/* ov_gemm(..., OV_EPI_BIAS_RESIDUAL, R, ldr, no row maps) that also writes parts[M][N / 32] of its OUTPUT rows (N % 32 == 0). */
int ov_gemm_rowparts(const ov_bf16* A, int64_t lda, const ov_bf16* W, int64_t ldw, const float* bias, ov_bf16* C, int64_t ldc,
                     int64_t M, int N, int K, const ov_bf16* R, int64_t ldr, float* parts, ov_stream_t stream);

/* What ov_gemm / ov_gemm_ln / ov_gemm_keep / ov_gemm_rowparts launch for a shape: the launcher's own decision, reported without
 * launching anything (tests and tools ask this instead of restating the rules). */
enum ov_gemm_kernel {
    OV_GEMM_SKINNY = 0,               /* 64 x 64 tiles, LDS ring: small shapes */
    OV_GEMM_PLAIN = 1,                /* 256 x 256 tiles, one workgroup per tile */
    OV_GEMM_PERSISTENT = 2            /* 256 x 256 tiles, one workgroup per CU walking the tiles */
};
typedef struct {
    int kernel;                       /* enum ov_gemm_kernel */
    /* the persistent kernel's instantiation (all 0 for the other two kernels) */
    int fold;                         /* LN-folded weights (ov_gemm_ln) */
    int direct;                       /* the register-exchange epilogue with row-per-lane stores; 0 = the LDS-transposed one */
    int mapped;                       /* row maps (out_group / resid_mod) */
    int keep;                         /* the pre-activation is kept (ov_gemm_keep), from the same launch */
    int stats;                        /* the row statistics' partial sums are fused into the epilogue (ov_gemm_rowparts) */
    /* walk and store policy: computed for every shape, MEANINGFUL FOR THE PERSISTENT KERNEL ONLY (the others never read them) */
    int ngroup;                       /* n-tiles per group of the tile walk; == the number of 256-column n-tiles: plain n-fastest walk */
    int rotmask;                      /* != 0: the rotated plain walk (half last n-tile), n index rotated under this mask */
    int rev;                          /* row tiles from the last to the first */
    int st_plain;                     /* bias / GELU outputs stored plainly; 0 = streaming stores */
    /* further launches */
    int keep_prepass;                 /* plain kernel + ov_gemm_keep: a bias-only launch writes the pre-activation first */
    int rowparts_pass;                /* ov_gemm_rowparts: the kernel does not produce the partial sums, ov_rowparts follows */
} ov_gemm_route_t;
/* fold / keep / rowparts / row_maps != 0: the call is ov_gemm_ln / ov_gemm_keep / ov_gemm_rowparts / has out_group or resid_mod set.
 * cus <= 0: the current device's CU count; > 0: used as given (no device needed).  The OVHIP_GEMM_* environment switches are those
 * the process read at its first GEMM or route call.  OV_ERR_UNSUPPORTED: a combination or shape no entry point admits. */
int ov_gemm_route(int64_t M, int N, int K, int epilogue, int fold, int keep, int rowparts, int row_maps, int cus, ov_gemm_route_t* route);

/* Non-causal, unmasked multi-head self-attention on a packed qkv activation.
 * qkv: [B*L, 3*H*hd] bf16 (q | k | v column blocks, heads contiguous inside each, ld = ld_qkv);
 * out: [B*L, H*hd] bf16 (heads merged, ld = ld_out).  scale multiplies q.k (hd^-0.5).
 * hd % 8 == 0, hd <= 96; which kernel a shape takes: ov_attention_route. */
int ov_attention(const ov_bf16* qkv, int64_t ld_qkv, ov_bf16* out, int64_t ld_out,
                 int B, int L, int H, int hd, float scale, ov_stream_t stream);
/* ov_attention that also keeps lse[B*H][Lp] (Lp = L rounded up to 32, fp32): the log-sum-exp of every query row's scaled scores in
 * log2 units, for ov_attention_backward_saved.  Only where the backward reads it (ov_attention_route_t::keep_lse);
 * OV_ERR_UNSUPPORTED otherwise. */
int ov_attention_lse(const ov_bf16* qkv, int64_t ld_qkv, ov_bf16* out, int64_t ld_out, float* lse, int B, int L, int H, int hd, float scale,
                     ov_stream_t stream);
/* Prefix-causal attention (the text decoder's prefix-LM mask, text_transformer.py:418-442 with li = prefix; make_causal_mask for
 * prefix = 0): key j is visible to query i iff j < prefix or j <= i.  An invisible key has weight exactly 0; 32 x 32 tile pairs that
 * are wholly invisible are skipped.  0 <= prefix <= L, OV_ERR_INVALID otherwise; prefix == L is ov_attention itself (bitwise).  Same
 * layouts, head dims and argument checks as ov_attention.  No e4m3-output form. */
int ov_attention_prefix(const ov_bf16* qkv, int64_t ld_qkv, ov_bf16* out, int64_t ld_out, int B, int L, int H, int hd, float scale,
                        int prefix, ov_stream_t stream);

/* What the attention entry points launch for a shape, forward (ov_attention / _lse / _fp8out / _prefix) and backward
 * (ov_attention_backward / _saved / ov_attention_prefix_backward): the launchers' own decision, reported without launching anything
 * (tests and tools ask this instead of restating the rules; DESIGN.md section 4 states them). */
enum ov_attn_fwd_kernel {
    OV_ATTN_FWD_PERSISTENT = 0,       /* head_dim 64, the head's K / V resident in LDS, workgroups walk the heads */
    OV_ATTN_FWD_STREAMING = 1,        /* head_dim 64, longer sequences: 64-key chunks streamed through LDS, 256 queries per workgroup */
    OV_ATTN_FWD_GENERIC = 2           /* every head_dim (padded to hdp in LDS), every row pitch, the prefix mask */
};
enum ov_attn_bwd_kernel {
    OV_ATTN_BWD_RESIDENT = 0,         /* head_dim 64: Q, K, V and dO of a head resident in LDS, one launch, no workspace */
    OV_ATTN_BWD_STREAMING = 1         /* the dQ and the dK / dV kernel over 256-row chunks, row lse and delta in the workspace */
};
typedef struct {
    /* ---- forward */
    int fwd_kernel;                   /* enum ov_attn_fwd_kernel */
    int deep;                         /* persistent: the instantiation for workgroups of at most 8 waves */
    int out8;                         /* persistent / streaming: e4m3 output (ov_attention_fp8out) */
    int lse;                          /* persistent: the row log-sum-exp is written (ov_attention_lse) */
    int mask;                         /* generic: the prefix mask (prefix < L) */
    int hdp;                          /* generic: the head_dim the LDS image is padded to (64 or 96); 0 for the other kernels */
    int resident;                     /* the whole (padded) sequence of a head is staged once; 0 = in chunks of kc keys */
    int kc;                           /* keys per LDS stage */
    int waves;                        /* waves per workgroup (32 queries each) */
    int grid_x, grid_y;               /* workgroups */
    int lds_bytes;                    /* dynamic LDS per workgroup */
    int lone_valu;                    /* persistent / streaming: a single-key last tile / chunk is folded in on the VALU
                                         (OVHIP_ATTN_LONEKEY=0: a tile step); the generic kernel always folds: 1 */
    /* ---- backward (saved = the call passes the forward's lse) */
    int bwd_kernel;                   /* enum ov_attn_bwd_kernel */
    int bwd_saved;                    /* resident: the row statistics are read from lse, not recomputed */
    int bwd_mask;                     /* streaming: the prefix mask */
    int ndh;                          /* streaming: 32-column d-blocks of a head in LDS (2: head_dim <= 64, 3: up to 96); 0 for resident */
    int bwd_kc;                       /* rows per LDS stage */
    int bwd_waves;
    int bwd_grid;
    int bwd_lds_bytes;
    int keep_lse;                     /* the backward reads the forward's lse: the training forward keeps it (ov_attention_lse) */
    size_t bwd_workspace_bytes;       /* what ov_attention[_prefix]_backward_workspace_bytes reports (0: none needed) */
} ov_attention_route_t;
/* ld_qkv / ld_out: the forward's row pitches in elements (0: dense, 3 H hd / H hd).  prefix < 0: no mask (ov_attention); 0 <= prefix
 * <= L: ov_attention_prefix and its backward (prefix == L is the unmasked route).  out8 / lse != 0: ov_attention_fp8out /
 * ov_attention_lse and ov_attention_backward_saved with an lse.  cus <= 0: the current device's CU count; > 0: used as given (no
 * device needed).  OVHIP_ATTN_LONEKEY is what the process read at its first attention or route call.  OV_ERR_UNSUPPORTED: a
 * combination or shape the entry points of either direction do not admit. */
int ov_attention_route(int B, int L, int H, int hd, int64_t ld_qkv, int64_t ld_out, int prefix, int out8, int lse, int cus,
                       ov_attention_route_t* route);

/* Patch gather for conv1: image [B,3,S,S] (img_dtype) -> P[B*g*g, Kpad] bf16,
 * column index c*P*P + i*P + j (the flattening of conv1.weight[D,3,P,P]); columns >= 3*P*P zeroed. */
int ov_im2col_patches(const void* image, int img_dtype, ov_bf16* out, int B, int S, int P, int Kpad,
                      ov_stream_t stream);

/* ---- patch dropout (PatchDropout, transformer.py:49-86): image b keeps the G = g*g patches keep[b, 0..K-1] (int32, in that order).
 * ov_im2col_patches on the kept patches only: out[b*K + j, :] = the operand row of patch keep[b, j] (bitwise ov_im2col_patches' row).
 * Indices are expected in [0, G) (ov_patch_keep_inverse checks them); any other index is clamped.  1 <= K <= G. */
int ov_im2col_patches_keep(const void* image, int img_dtype, const int* keep, ov_bf16* out, int B, int S, int P, int K, int Kpad,
                           ov_stream_t stream);
/* inv[b, p] = j where keep[b, j] = p, -1 for a dropped patch (int32 [B, G]).  A duplicate or an index outside [0, G) sets *err_flag
 * (device int, may be NULL) to 1.  1 <= K <= G <= 16384. */
int ov_patch_keep_inverse(const int* keep, int* inv, int B, int K, int G, int* err_flag, ov_stream_t stream);
/* The training path's token assembly, fp32 [B, 1+K, D]:  x[b, 0] = cls + pos[0],  x[b, 1+j] = y[b*K + j] + pos[1 + keep[b, j]]
 * (y bf16 rows of the patch GEMM, cls fp32 [D], pos fp32 [1+G, D]; one fp32 add per element).  D % 8 == 0. */
int ov_patch_keep_assemble(const ov_bf16* y, int64_t ldy, const float* cls, const float* pos, const int* keep, float* x, int B, int K,
                           int G, int D, ov_stream_t stream);
/* Its backward from dx fp32 [B, 1+K, D]:  dpos[p] (fp32 [1+G, D]) = sum over b = 0..B-1, in that order, of the row p fed (exactly 0 for
 * a patch no image kept), dcls = dpos[0] (fp32 [D]); dy[b*K + j] = bf16(dx[b, 1+j]).  Deterministic (no atomics).  dpos / dcls / dy
 * may be NULL (skipped). */
int ov_patch_keep_assemble_backward(const float* dx, const int* inv, int B, int K, int G, int D, float* dpos, float* dcls, ov_bf16* dy,
                                    int64_t lddy, ov_stream_t stream);
/* Pixel gradient of ov_im2col_patches_keep: dimg [B,3,S,S] (img_dtype) = the kept patches' rows of dcols [B*K, ldc] (bf16) put back,
 * 0 in dropped patches (stride = kernel: a permutation, no sums).  S % 4 == 0. */
int ov_col2im_patches_keep(const ov_bf16* dcols, int64_t ldc, const int* inv, void* dimg, int img_dtype, int B, int S, int P, int K,
                           ov_stream_t stream);

/* x[b*L + 0, :] = bf16(bf16(cls[:]) + bf16(pos[0,:]))  for every image b. cls/pos fp32. */
int ov_cls_rows(ov_bf16* x, int64_t ldx, const float* cls, const float* pos0, int B, int L, int D,
                ov_stream_t stream);

/* out[b,:] = mean over tokens first..L-1 of x[b*L + t, :]  (first = 1: skip cls; 'avg' pooling). fp32 out. */
int ov_mean_pool(const ov_bf16* x, int64_t ldx, float* out, int B, int L, int D, int first,
                 ov_stream_t stream);

/* The mean over tokens first..L-1 of a block's output x1 + hid . W^T + bias, without forming that output (the mean commutes with the
 * linear layer):  out[b, :] = mean_t x1[b*L + t, :] + (mean_t hid[b*L + t, :]) . W^T + bias,  fp32 [B, D], accumulated in fp32 from the
 * bf16 inputs (exact-fp32 MFMA) and never rounded to bf16.  x1 [B*L, D] (pitch ldx), hid [B*L, F] (pitch ldh), W [D, F] (pitch ldw) bf16,
 * bias fp32 [D].  F % 32 == 0.  Workspace: the pooled hidden, fp32 [B, F].  out is written by the pooling pass first and then
 * read-modify-written by the product, so it must not overlap the workspace (or any input). */
size_t ov_mlp_out_pooled_workspace_bytes(int B, int F);
int ov_mlp_out_pooled(const ov_bf16* x1, int64_t ldx, const ov_bf16* hid, int64_t ldh, const ov_bf16* W, int64_t ldw, const float* bias,
                      float* out, int B, int L, int D, int F, int first, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* x[b*T + t, :] = bf16(bf16(table[tokens[b,t], :]) + bf16(pos[t, :])).  tokens int64; table/pos bf16.
 * Token ids outside [0, V) set *err_flag (device int, may be NULL) and are clamped. */
int ov_text_embed(const int64_t* tokens, const ov_bf16* table, const ov_bf16* pos, ov_bf16* x,
                  int64_t ldx, int B, int T, int D, int V, int* err_flag, ov_stream_t stream);

/* out[b, :] = x[b*L + t, :] (row gather; t = L-1 for text 'last' pooling). bf16 -> bf16. */
int ov_gather_rows(const ov_bf16* x, int64_t ldx, ov_bf16* out, int64_t ldo, int B, int L, int t, int D,
                   ov_stream_t stream);

/* idx[b] = the smallest t with tokens[b, t] == max_t tokens[b, :]  (text.argmax(dim=-1) with ties going to the first position; the
 * compare runs on the full int64).  tokens int64 [B, T], idx int32 [B]. */
int ov_token_argmax(const int64_t* tokens, int* idx, int B, int T, ov_stream_t stream);

/* out[b, :] = x[b*L + clamp(idx[b], 0, L-1), :]  (row gather at a per-batch position: text 'argmax' pooling).  bf16 -> bf16, 16-byte
 * copies: D % 8 == 0, pitches % 8 == 0.  idx int32 [B] on the device; the clamp is for memory safety only. */
int ov_gather_rows_at(const ov_bf16* x, int64_t ldx, const int* idx, ov_bf16* out, int64_t ldo, int B, int L, int D,
                      ov_stream_t stream);

/* bf16 <-> fp32 row conversion helpers (strided rows). */
int ov_convert(const void* src, int src_dtype, int64_t lds, void* dst, int dst_dtype, int64_t ldd,
               int64_t rows, int cols, ov_stream_t stream);

/* y[r,:] = x[r,:] / max(||x[r,:]||_2, 1e-12)   (F.normalize).  x bf16 or fp32, y fp32. */
int ov_l2norm(const void* x, int x_dtype, int64_t ldx, float* y, int64_t ldy, int64_t rows, int E,
              ov_stream_t stream);

/* out[i, j] = scale * (*scale_dev) * <X[i,:], Y[j,:]>  fp32 in/out (CLIP.get_logits: model.py:286-293).  E % 8 == 0.
 * scale_dev: optional device scalar (NULL = 1): exp(logit_scale) stays on the device, as in the reference (model.py:288). */
int ov_logits(const float* X, const float* Y, float* out, int64_t ldo, int n1, int n2, int E, float scale, const float* scale_dev,
              ov_stream_t stream);

/* ov_attention with the output written as e4m3 bytes out8[B*L, H*64] (ld_out in bytes) under the static scale 2 * (*out_amax) / 448
 * (device scalar; fp8 path: the out-proj GEMM then reads it through ov_gemm_fp8_static).  head_dim 64; else OV_ERR_UNSUPPORTED. */
int ov_attention_fp8out(const ov_bf16* qkv, int64_t ld_qkv, unsigned char* out8, int64_t ld_out, int B, int L, int H, int hd,
                        float scale, const float* out_amax, float* out_amax_next /* optional running maximum */, ov_stream_t stream);

/* ---- fp8 GEMM (BASELINE.json config #5: fp8 weights/activations on the CDNA4 fp8 MFMA) --------------------------------------
 * C = epilogue(rowscale[m] * colscale[n] * (A . W^T) + bias):  A [M, K], W [N, K] OCP e4m3fn bytes (K contiguous, lda/ldw in
 * bytes, % 16), rowscale [M] / colscale [N] fp32 dequantisation scales (per activation row / per weight row), bias fp32 or NULL,
 * C (and R for OV_EPI_BIAS_RESIDUAL) bf16.  K % 128 == 0, K >= 384, N % 8 == 0.  Epilogues: OV_EPI_BIAS, OV_EPI_BIAS_GELU_ERF,
 * OV_EPI_BIAS_RESIDUAL.  Accumulation in fp32 on v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales). */
int ov_gemm_fp8(const unsigned char* A, int64_t lda, const unsigned char* W, int64_t ldw, const float* rowscale,
                const float* colscale, const float* bias, ov_bf16* C, int64_t ldc, int64_t M, int N, int K, int epilogue,
                const ov_bf16* R, int64_t ldr, ov_stream_t stream);

/* ov_gemm_fp8 with a STATIC activation scale on one side (scale = 2 * amax / 448, amax a calibrated device scalar):
 * out_amax != NULL: C is e4m3 bytes [M, N] (ldc in bytes, % 16; N % 16 == 0) quantised with out_amax's scale, epilogue
 *                   OV_EPI_BIAS_GELU_ERF / _TANH -- the c_fc -> c_proj hand-over without a bf16 round trip and a re-quantisation pass;
 * in_amax  != NULL: every row of A carries in_amax's scale (rowscale ignored), epilogue OV_EPI_BIAS_RESIDUAL, C / R bf16.
 * Exactly one of the two is set. */
int ov_gemm_fp8_static(const unsigned char* A, int64_t lda, const unsigned char* W, int64_t ldw, const float* rowscale,
                       const float* in_amax, const float* colscale, const float* bias, void* C, int64_t ldc, const float* out_amax,
                       float* out_amax_next /* optional: running maximum of |C| for the next call */, int64_t M, int N, int K,
                       int epilogue, const ov_bf16* R, int64_t ldr, ov_stream_t stream);
/* cur[i] = max(cur[i], next[i]), i < n (delayed scaling: roll the recorded maxima into the scales at the top of a forward). */
int ov_amax_roll(float* cur, const float* next, int n, ov_stream_t stream);

/* Activation quantisation for ov_gemm_fp8: q[r,:] = e4m3(y[r,:] / s_r), s_r = max|y[r,:]| / 448, with y = x (ov_quant_rows_fp8) or
 * y = LayerNorm(x) * gamma + beta in fp32 (ov_layernorm_quant_fp8; eps, biased variance as transformer.py:15-30).  x bf16
 * [rows, D] (ldx), q bytes [rows, D] (ldq, % 8), rowscale [rows] fp32.  D % 8 == 0, D <= 8192. */
/* amax_acc (device float, may be NULL): running maximum of |x| over every row quantised so far (calibration of static scales). */
int ov_quant_rows_fp8(const ov_bf16* x, int64_t ldx, unsigned char* q, int64_t ldq, float* rowscale, int64_t rows, int D,
                      float* amax_acc, ov_stream_t stream);
int ov_layernorm_quant_fp8(const ov_bf16* x, int64_t ldx, const float* gamma, const float* beta, unsigned char* q, int64_t ldq,
                           float* rowscale, int64_t rows, int D, float eps, ov_stream_t stream);

/* ---- image front-end: Resize [+ CenterCrop] -> ToTensor -> Normalize on the device ----------------
 * Bit-exact counterpart of PIL.Image.resize (what torchvision's Resize runs on a PIL image: reference ov-zero-shot-test.py:72-77,
 * open_clip/transform.py:355-392) followed by x / 255 and (x - mean) / std in IEEE fp32.
 * src: uint8 RGB [H, W, 3] (device).  bounds_x [Wr][2] = {first source column, tap count}, coef_x [Wr][ksize_x] = Pillow's 22-bit
 * fixed-point taps (device int32), same for y over Hr output rows; row0/nrows = the source rows the vertical pass reads
 * (Pillow's ybox); tmp: uint8 [nrows, Wr, 3] scratch (device).  The [out_h, out_w] window at (crop_x, crop_y) of the resized
 * [Hr, Wr] image is written as CHW [3, out_h, out_w] in out_dtype (OV_F32 / OV_BF16).  mean / stdv: HOST float[3]. */
int ov_preprocess_image(const unsigned char* src, int H, int W, const int* bounds_x, const int* coef_x, int ksize_x, int Wr,
                        const int* bounds_y, const int* coef_y, int ksize_y, int Hr, int row0, int nrows, unsigned char* tmp,
                        int crop_x, int crop_y, int out_h, int out_w, const float* mean, const float* stdv, void* out,
                        int out_dtype, ov_stream_t stream);

/* ---- training image transform: batched crop, resize, colour jitter, grayscale, ToTensor, Normalize ------------------------
 * The training branch of open_clip.transform.image_transform (transform.py:307-358) on PIL images, after its random numbers are
 * drawn: img.crop(box).resize((out_w, out_h)) in Pillow's fixed-point arithmetic, ImageEnhance.Brightness / Contrast / Color and
 * convert("L") in Pillow's, then x / 255 and (x - mean) / std in IEEE fp32.  One call per batch of variable-sized images, at
 * most 4 + contrast_passes launches whatever B is.
 *   pixels   uint8, the images packed back to back, pixel_bytes in all; image b is RGB [H_b, W_b, 3] at pixels + offsets[b]
 *   offsets  int64 [B]; shapes int32 [B, 2] = (H, W); boxes int32 [B, 4] = (top, left, h, w), inside the image and h, w > 0
 *            (the caller checks; an image whose box is not is never read and comes out as the normalised black image)
 *   ops      int32 [B, 4]: the colour operations in application order (enum ov_color_op); factors fp32 [B, 4]: the blend factor
 *            of a brightness / contrast / saturation operation (unused for the others)
 *   max_rows >= every box's h.  max_taps_x / max_taps_y >= ceil(fsupport * max(extent / out, 1)) * 2 + 1 over the boxes' w / h,
 *            fsupport = 1 (bilinear) or 2 (bicubic): the row length of the coefficient tables.
 *   contrast_passes  the largest number of contrast operations any one image carries (0: the statistics launch is skipped)
 *   mean / stdv  HOST float[3];  out: [B, 3, out_h, out_w] in out_dtype (OV_F32 / OV_BF16)
 *   workspace    ov_train_transform_workspace_bytes(...) bytes, 16-byte aligned: the tables, the horizontal intermediate
 *                [B, max_rows, out_w, 3], the resized uint8 image [B, out_h, out_w, 3] and the per-image sums of L.
 * ov_train_transform_plan is the first launch on its own: bounds_x int32 [B, out_w, 2] = (first source index relative to the
 * crop, tap count) and taps_x int32 [B, out_w, max_taps_x] (22-bit fixed point, zero padded) for extent w_b -> out_w, the same
 * for y over h_b -> out_h; Resample.c precompute_coeffs + normalize_coeffs_8bpc in fp64 without contraction. */
enum ov_interp { OV_INTERP_BILINEAR = 0, OV_INTERP_BICUBIC = 1 };
enum ov_color_op { OV_COLOR_NONE = 0, OV_COLOR_BRIGHTNESS = 1, OV_COLOR_CONTRAST = 2, OV_COLOR_SATURATION = 3, OV_COLOR_GRAYSCALE = 4 };
size_t ov_train_transform_workspace_bytes(int B, int out_h, int out_w, int max_rows, int max_taps_x, int max_taps_y);
int ov_train_transform_plan(const int* boxes, int B, int out_h, int out_w, int interpolation, int max_taps_x, int max_taps_y,
                            int* bounds_x, int* taps_x, int* bounds_y, int* taps_y, ov_stream_t stream);
int ov_train_transform(const unsigned char* pixels, int64_t pixel_bytes, const int64_t* offsets, const int* shapes, const int* boxes,
                       const int* ops, const float* factors, int B, int out_h, int out_w, int max_rows, int interpolation,
                       int max_taps_x, int max_taps_y, int contrast_passes, const float* mean, const float* stdv, void* out,
                       int out_dtype, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* ---- consumers of encode + logits: zero-shot classifier weights and ranking ------------
 * out[c,:] = normalize(mean_t emb[c*T + t, :])   (open_clip/zero_shot_classifier.py:54-57).  fp32 in/out. */
int ov_class_mean_normalize(const float* emb, float* out, int C, int T, int E, ov_stream_t stream);
/* Per-row top-k of x[rows, cols] (fp32): idx_out[rows, k] int64 (and val_out[rows, k], optional), best first;
 * largest != 0 ranks by value descending (logits), else ascending (distances, as image_text_retrieval.py:44,78 argsort);
 * ties go to the smaller index.  k <= cols. */
int ov_topk(const float* x, int64_t ldx, int rows, int cols, int k, int largest, int64_t* idx_out, float* val_out,
            ov_stream_t stream);

/* Local-strip InfoNCE (ClipLoss with local_loss semantics; world_size 1 = plain ClipLoss).
 *   img, txt      : this rank's L2-normalised embeddings [b, E] fp32
 *   all_img/all_txt: gathered embeddings [N, E] fp32 in rank order (== img/txt when N == b)
 *   logit_scale   : DEVICE scalar, the multiplier exp(CLIP.logit_scale) (model.py:315) -- ABI 2: it never crosses the host, so
 *                   the step enqueues without a stream drain (the reference keeps it on the device too: loss.py:120-131)
 *   labels are i + label_offset (label_offset = b * rank, loss.py:93-94)
 *   loss_out[0] = (CE(scale*img@all_txt^T) + CE(scale*txt@all_img^T)) / 2      (fp32, device)
 *   lse_out (optional, may be NULL): [4, b] fp32 = lse_img, diag_img, lse_txt, diag_txt
 * workspace: ov_clip_loss_workspace_bytes(b, N) bytes. Logits are never materialised. */
size_t ov_clip_loss_workspace_bytes(int b, int N);
int ov_clip_loss(const float* img, const float* txt, const float* all_img, const float* all_txt,
                 int b, int N, int E, const float* logit_scale, int label_offset, float* loss_out,
                 float* lse_out, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* Backward of ov_clip_loss (loss.py:102-131 differentiated; the reference gets it from autograd): with P = softmax - onehot of
 * each [b, N] strip (recomputed, never materialised; lse_terms = the [4, b] block ov_clip_loss wrote) and c = grad_loss *
 * logit_scale / (2 b) (both DEVICE scalars; grad_loss NULL = 1):   d_img = c P_i all_txt,  d_txt = c P_t all_img            (local rows, [b, E], always written)
 *                        d_all_txt = c P_i^T img, d_all_img = c P_t^T txt          (gathered rows, [N, E]; NULL = skip)
 *                        d_scale = grad_loss / (2 b) * sum P .* (x . y)            (device scalar; NULL = skip)
 * The caller routes the gathered-side terms (gather_features, loss.py:19-63: own chunk only, or reduce-scatter when
 * gather_with_grad).  E % 32 == 0, E <= 1152; OV_ERR_UNSUPPORTED otherwise.  Deterministic (no atomics). */
size_t ov_clip_loss_backward_workspace_bytes(int b, int N);
int ov_clip_loss_backward(const float* img, const float* txt, const float* all_img, const float* all_txt, int b, int N, int E,
                          const float* logit_scale, int label_offset, const float* lse_terms, const float* grad_loss, float* d_img,
                          float* d_txt, float* d_all_img, float* d_all_txt, float* d_scale, void* workspace,
                          size_t workspace_bytes, ov_stream_t stream);

/* InfoNCE over C caption sets per image (bidirectional_contrastive_loss with local_loss, src/losses/common.py:120-189, which has
 * C = 2): the mean over c of ov_clip_loss(img, txt_c), in one forward and one backward.
 *   img           : this rank's image embeddings [b, E] fp32, contiguous
 *   txt           : this rank's text embeddings, the C sets stacked [C b, E] fp32, contiguous: set c in rows c b ... c b + b - 1
 *   all_img       : gathered image embeddings, N rows of E floats, row g at all_img + g * ld
 *   all_txt       : gathered text embeddings, row g of set c at all_txt + c * set_stride + g * ld
 *                   (the all-gather's packed [N, (1 + C) E] buffer in place: all_img = buf, all_txt = buf + E, ld = (1 + C) E,
 *                    set_stride = E;  separate arrays [N, E] and [C, N, E]: ld = E, set_stride = N E;  N == b without a gather:
 *                    all_img = img, all_txt = txt, ld = E, set_stride = b E)
 *   logit_scale   : DEVICE scalar, the multiplier;  labels are i + label_offset
 *   loss_out[0] = 1 / (2 C b) sum_c sum_i [ lse(A_c[i, :]) - A_c[i, i + off] + lse(B_c[i, :]) - B_c[i, i + off] ],
 *                 A_c = scale img all_txt_c^T, B_c = scale txt_c all_img^T                     (fp32, device)
 *   terms_out (optional, may be NULL): [4 C, b] fp32; for set c rows 4c ... 4c + 3 = lse_img, diag_img, lse_txt, diag_txt
 * 1 <= C <= 4 and E % 8 == 0 (OV_ERR_UNSUPPORTED otherwise); ld >= E, ld and set_stride multiples of 4 floats, every base pointer
 * 16-byte aligned (OV_ERR_INVALID otherwise).  workspace: ov_clip_loss_multi_workspace_bytes(b, N, C) bytes (0 for sizes that are
 * not positive or C out of range).  Logits are never materialised; deterministic (no atomics). */
size_t ov_clip_loss_multi_workspace_bytes(int b, int N, int C);
int ov_clip_loss_multi(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld, int64_t set_stride,
                       int b, int N, int E, int C, const float* logit_scale, int label_offset, float* loss_out, float* terms_out,
                       void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* Backward of ov_clip_loss_multi, operands laid out as there; terms = the [4 C, b] block it wrote; coef = grad_loss * logit_scale /
 * (2 C b) (both DEVICE scalars; grad_loss NULL = 1); P = softmax - onehot of each strip, recomputed and never materialised:
 *     d_img [b, E]      = coef sum_c P_img,c all_txt_c     (ONE pass: the in-side loop runs over the C sets)     always written
 *     d_txt [C b, E]    : rows of set c = coef P_txt,c all_img                                                    always written
 *     d_all_img         = coef sum_c P_txt,c^T txt_c  (one pass), row g at d_all_img + g * ldg                    NULL = skip
 *     d_all_txt         : set c = coef P_img,c^T img, row g at d_all_txt + c * gset_stride + g * ldg               NULL = skip
 *     d_scale           = grad_loss / (2 C b) * sum over all 2 C strips of P .* (x . y)   (device scalar)          NULL = skip
 * ldg / gset_stride follow the rules of ld / set_stride, so the gathered side can be written as one packed [N, (1 + C) E] gradient
 * for one reduce-scatter (d_all_img = buf, d_all_txt = buf + E, ldg = (1 + C) E, gset_stride = E).  The caller routes the
 * gathered-side terms as for ov_clip_loss_backward.  E % 32 == 0, E <= 1152 (OV_ERR_UNSUPPORTED otherwise).  Deterministic: no
 * atomics, the d_scale partials (one per 32-row tile and job) are summed in a fixed order. */
size_t ov_clip_loss_multi_backward_workspace_bytes(int b, int N, int C);
int ov_clip_loss_multi_backward(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld,
                                int64_t set_stride, int b, int N, int E, int C, const float* logit_scale, int label_offset,
                                const float* terms, const float* grad_loss, float* d_img, float* d_txt, float* d_all_img,
                                float* d_all_txt, int64_t ldg, int64_t gset_stride, float* d_scale, void* workspace,
                                size_t workspace_bytes, ov_stream_t stream);

/* Gradient accumulation for the InfoNCE.  Gradient of the loss over a fixed bank of N rows (C caption sets) with respect to the rows
 * of one window [w0, w0 + b): the exact gradient of
 *     1 / (2 C norm_rows) sum_c sum_{i < N} [ lse(A_c[i, :]) - A_c[i, i] + lse(B_c[i, :]) - B_c[i, i] ]
 * restricted to the window's rows, which appear both as rows of their own strips and as columns of every other row's.
 *   all_img / all_txt, ld, set_stride : the bank, laid out as the gathered operands of the C-set forward above (packed
 *              [N, (1 + C) E] in place, or separate arrays)
 *   terms    : [4 C, N], what that forward wrote for b = N, label_offset = 0 (per set lse_img, diag_img, lse_txt, diag_txt)
 *   norm_rows: the number of rows the mean runs over (N in a world of one; a rank's own rows under data parallelism)
 *   d_img [b, E], d_txt [C b, E] (set c in rows c b ...): always written
 *   d_scale  : this window's share (device scalar), taken from the image-side strips only, so that disjoint windows covering the
 *              bank sum to the full gradient; NULL = skip
 * coef = grad_loss * logit_scale / (2 C norm_rows), both DEVICE scalars (grad_loss NULL = 1).  One pass over the window's b x N strips
 * with both normalisers per logit; logits are never materialised; deterministic (no atomics, the d_scale partials, one per 32-row
 * tile, are summed in a fixed order).  E % 32 == 0, E <= 1152, 1 <= C <= 4 (OV_ERR_UNSUPPORTED otherwise); NULL operands, w0 < 0,
 * b <= 0, w0 + b > N, norm_rows <= 0, ld < E, ld or set_stride not a multiple of 4 floats, a base pointer off 16 bytes:
 * OV_ERR_INVALID; a short workspace: OV_ERR_WORKSPACE; all before any launch. */
size_t ov_clip_loss_window_backward_workspace_bytes(int b, int N, int C);
int ov_clip_loss_window_backward(const float* all_img, const float* all_txt, int64_t ld, int64_t set_stride, int N, int E, int C,
                                 const float* logit_scale, const float* terms, const float* grad_loss, int w0, int b, int norm_rows,
                                 float* d_img, float* d_txt, float* d_scale, void* workspace, size_t workspace_bytes,
                                 ov_stream_t stream);

/* Distillation from a frozen teacher (DistillClipLoss, loss.py:180-216): the student's InfoNCE and, per direction, the cross
 * entropy of the student's log-softmax under the teacher's softmax, in one forward and one backward.
 *   img, txt        : the student's local embeddings [b, E] fp32, contiguous
 *   all_img/all_txt : the student's gathered embeddings, N rows of E floats, row g at base + g * ld
 *   t_img, t_txt    : the teacher's local embeddings [b, Et] fp32, contiguous (Et may differ from E)
 *   t_all_img/t_all_txt: the teacher's gathered embeddings, N rows of Et floats, row g at base + g * ldt
 *                     (the all-gather's packed [N, 2E + 2Et] buffer in place: all_img = buf, all_txt = buf + E, t_all_img = buf + 2E,
 *                      t_all_txt = buf + 2E + Et, ld = ldt = 2E + 2Et;  separate arrays: ld = E, ldt = Et;  N == b without a gather:
 *                      the gathered operands are the local ones)
 *   logit_scale, t_logit_scale: DEVICE scalars s and st, the two multipliers;  labels are i + label_offset
 *   with A = s img all_txt^T, T = st t_img t_all_txt^T, Q = softmax(T, dim=1) (and B, U, R likewise from txt, all_img, t_txt, t_all_img):
 *   contrastive_out[0] = 1 / (2 b) sum_i [ lse(A_i) - A[i, i + off] + lse(B_i) - B[i, i + off] ]        (= ov_clip_loss's value)
 *   distill_out[0]     = 1 / (2 b) sum_i [ lse(A_i) - sum_j Q_ij A_ij + lse(B_i) - sum_j R_ij B_ij ]    (fp32, device)
 *   terms_out (required): [12, b] fp32.  Rows 0 ... 3 = the student's lse_img, diag_img, lse_txt, diag_txt, as ov_clip_loss defines
 *                     them; row 4 = the teacher's lse of T, row 5 = sum_j Q_ij A_ij, row 6 = the teacher's lse of U, row 7 = sum_j R_ij B_ij;
 *                     rows 8 ... 11 = the low parts of the four lse (lse_img, lse_txt, teacher T, teacher U): each lse is kept as an
 *                     fp32 pair hi + lo, rows 0 / 2 / 4 / 6 holding hi = fl(lse), so that the backward's exp(logit - lse) is not
 *                     rounded at the size of the lse
 * The teacher's lse is taken first (one pass over the teacher operands), so the cross sums need no running-max rescale.
 * E % 32 == 0, E <= 1152 (the backward's limit), Et % 8 == 0: OV_ERR_UNSUPPORTED otherwise.  ld >= E, ldt >= Et, both multiples of
 * 4 floats, every base pointer 16-byte aligned, 0 <= label_offset, label_offset + b <= N: OV_ERR_INVALID otherwise, before any launch.
 * workspace: ov_distill_loss_workspace_bytes(b, N) bytes (0 for sizes that are not positive).  Logits are never materialised;
 * deterministic (no atomics). */
size_t ov_distill_loss_workspace_bytes(int b, int N);
int ov_distill_loss(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld, const float* t_img,
                    const float* t_txt, const float* t_all_img, const float* t_all_txt, int64_t ldt, int b, int N, int E, int Et,
                    const float* logit_scale, const float* t_logit_scale, int label_offset, float* contrastive_out,
                    float* distill_out, float* terms_out, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* Backward of ov_distill_loss, operands laid out as there; terms = the [12, b] block it wrote; grad_contrastive (g_c) and grad_distill
 * (g_d) = the upstream gradients of the two outputs, DEVICE scalars, both required.  With P = softmax(A), Q = softmax(T) recomputed per
 * tile from the saved lse and G = ((g_c + g_d) P - g_c onehot - g_d Q) / (2 b) per direction:
 *     d_img = s G_i all_txt,  d_txt = s G_t all_img                               (local rows, [b, E], always written)
 *     d_all_txt = s G_i^T img, d_all_img = s G_t^T txt                            (gathered rows, row g at base + g * ldg; NULL = skip)
 *     d_scale = sum over both directions of G .* (x . y)                          (device scalar; NULL = skip)
 * Nothing is computed for the teacher operands or t_logit_scale.  ldg follows ld's rules, so the gathered side can be written as one
 * packed [N, 2E] gradient for one reduce-scatter (d_all_img = buf, d_all_txt = buf + E, ldg = 2E).  Shape limits as the forward's.
 * Deterministic: no atomics, the d_scale partials (one per 32-row tile and direction) are summed in a fixed order. */
size_t ov_distill_loss_backward_workspace_bytes(int b, int N);
int ov_distill_loss_backward(const float* img, const float* txt, const float* all_img, const float* all_txt, int64_t ld,
                             const float* t_img, const float* t_txt, const float* t_all_img, const float* t_all_txt, int64_t ldt, int b,
                             int N, int E, int Et, const float* logit_scale, const float* t_logit_scale, int label_offset,
                             const float* terms, const float* grad_contrastive, const float* grad_distill, float* d_img, float* d_txt,
                             float* d_all_img, float* d_all_txt, int64_t ldg, float* d_scale, void* workspace, size_t workspace_bytes,
                             ov_stream_t stream);

/* SigLIP pairwise sigmoid loss on a local strip (SigLipLoss, loss.py:307-414; the neighbour-exchange ring is replaced by one
 * all-gather of the text features: only the order of the sums differs).
 *   img           : this rank's L2-normalised image embeddings [b, E] fp32
 *   all_txt       : gathered text embeddings [N, E] fp32 in rank order (== this rank's text when N == b)
 *   logit_scale   : DEVICE scalar s, the multiplier exp(CLIP.logit_scale); logit_bias: DEVICE scalar beta (NULL = no bias)
 *   with z = s img_i . all_txt_j + beta and l = +1 where j == i + label_offset (label_offset = b * rank), -1 elsewhere:
 *   loss_out[0] = (1 / b) sum_{i < b, j < N} softplus(-l z)                (fp32, device; = -logsigmoid(l z), loss.py:349-358)
 * 0 <= label_offset, label_offset + b <= N, E % 8 == 0, E <= 1152 (OV_ERR_INVALID / OV_ERR_UNSUPPORTED otherwise).
 * workspace: ov_siglip_loss_workspace_bytes(b, N) bytes.  Logits are never materialised; deterministic (no atomics). */
size_t ov_siglip_loss_workspace_bytes(int b, int N);
int ov_siglip_loss(const float* img, const float* all_txt, int b, int N, int E, const float* logit_scale, const float* logit_bias,
                   int label_offset, float* loss_out, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* Backward of ov_siglip_loss: with g = -l sigmoid(-l z) / b * grad_loss (grad_loss a DEVICE scalar, NULL = 1), recomputed tile by
 * tile and never materialised:
 *                        d_img     = s g all_txt          (local rows [b, E], always written)
 *                        d_all_txt = s g^T img            (gathered rows [N, E]; NULL = skip)
 *                        d_scale   = sum g .* (img . all_txt^T),  d_bias = sum g      (device scalars; NULL = skip)
 * The caller routes d_all_txt (sum over ranks, own chunk kept).  Same shape limits as ov_siglip_loss.  Deterministic: no atomics,
 * the scalar sums are fixed-order two-stage sums. */
size_t ov_siglip_loss_backward_workspace_bytes(int b, int N);
int ov_siglip_loss_backward(const float* img, const float* all_txt, int b, int N, int E, const float* logit_scale,
                            const float* logit_bias, int label_offset, const float* grad_loss, float* d_img, float* d_all_txt,
                            float* d_scale, float* d_bias, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* ---- caption loss: masked softmax cross-entropy over the vocabulary (softmax_xent with reduction=True and a mask,
 * src/losses/common.py:225-251; no label smoothing).  logits fp32 [R, V] (row pitch ld >= V), labels int64 [R], mask fp32 [R]:
 *     nll_r = logsumexp(logits_r) - logits_r[label_r]   (0 for a label outside [0, V));   *loss = sum nll_r mask_r / (sum mask_r + 1e-8)
 * row_lse [R] keeps every row's log-sum-exp for the backward.  fp32 throughout, one pass over a row, deterministic, device scalars in
 * and out.  Backward: dlogits = (*grad) mask_r / (sum mask + 1e-8) (softmax(logits_r) - onehot_r); rows with mask_r == 0 are exactly
 * zero; dlogits may alias logits.  Workspace for either call: ov_softmax_xent_workspace_bytes(R). */
size_t ov_softmax_xent_workspace_bytes(int64_t R);
int ov_softmax_xent(const float* logits, int64_t ld, const int64_t* labels, const float* mask, int64_t R, int V, float* loss,
                    float* row_lse, void* workspace, size_t workspace_bytes, ov_stream_t stream);
int ov_softmax_xent_backward(const float* logits, int64_t ld, const int64_t* labels, const float* mask, const float* row_lse,
                             const float* grad, float* dlogits, int64_t ld_dlogits, int64_t R, int V, void* workspace,
                             size_t workspace_bytes, ov_stream_t stream);

/* ---- operator-level backward of the block (the reference gets these from torch autograd through nn.Linear,
 * nn.LayerNorm and nn.GELU: transformer.py:15-30, 232-236).  bf16 activations and gradients, fp32 arithmetic and parameter-gradient
 * sums, deterministic (two-stage reductions in a fixed order). ---------------------------------------------------------------- */

/* out[c, r] = in[r, c]; columns rows..pad64(rows)-1 of out are written as zeros (the GEMM's K granule).  cols % 8 == 0,
 * ld_out >= pad64(rows). */
int ov_transpose_bf16(const ov_bf16* in, int64_t ld_in, int64_t rows, int cols, ov_bf16* out, int64_t ld_out, ov_stream_t stream);

/* y = x W^T + b  (x [M, K], W [N, K], dY [M, N]):  dX = dY W  [M, K],  dW = dY^T x  [N, K] (bf16),  db = column sums of dY (fp32 [N]).
 * Any of dX / dW / db may be NULL (skipped; x is only read for dW).  N % 64 == 0, K % 64 == 0.  Both products run on ov_gemm, fed by LDS-staged transposes
 * held in the workspace (ov_linear_backward_workspace_bytes). */
size_t ov_linear_backward_workspace_bytes(int64_t M, int N, int K);
/* What ov_linear_backward does for dW at this shape on the current device (for tests that assert which path they reach): *nz split-K
 * ranges of *chunk rows each (the last one shorter when nz * chunk > M), *tn_route = 1 when dW comes straight from the row-major
 * operands (M % 64 == 0 and OVHIP_DW_TRANSPOSE unset), 0 for the explicit-transpose route.  Any of the three may be NULL. */
int ov_linear_backward_plan(int64_t M, int N, int K, int* nz, int64_t* chunk, int* tn_route);
int ov_linear_backward(const ov_bf16* dY, int64_t lddy, const ov_bf16* X, int64_t ldx, const ov_bf16* W, int64_t ldw, int64_t M, int N,
                       int K, ov_bf16* dX, int64_t lddx, ov_bf16* dW, int64_t lddw, float* db, void* workspace,
                       size_t workspace_bytes, ov_stream_t stream);

/* Backward of ov_layernorm on bf16 rows: dx = rstd (q - mean(q) - xhat mean(q xhat)) with q = dy * gamma, dgamma = sum_rows dy * xhat,
 * dbeta = sum_rows dy (fp32 [D]).  D % 8 == 0, D <= 4096. */
size_t ov_layernorm_backward_workspace_bytes(int64_t rows, int D);
int ov_layernorm_backward(const ov_bf16* x, int64_t ldx, const float* gamma, const ov_bf16* dy, int64_t lddy,
                          const ov_bf16* dres /* optional: added to dx (the residual branch's gradient) */, int64_t lddres, ov_bf16* dx,
                          int64_t lddx, float* dgamma, float* dbeta, int64_t rows, int D, float eps, void* workspace,
                          size_t workspace_bytes, ov_stream_t stream);

/* Backward of ov_attention (unmasked softmax attention of nn.MultiheadAttention, transformer.py:225,239-252): from the packed
 * qkv [B*L, 3*H*hd], the forward output out [B*L, H*hd] and the upstream gradient dout, writes dqkv [B*L, 3*H*hd] = (dQ | dK | dV).
 * The row log-sum-exp is recomputed (the forward keeps none).  hd % 8 == 0, hd <= 96.  Short head_dim 64 sequences: one kernel with
 * the head resident in LDS, no workspace; otherwise (long sequences; head dims 72 / 80 of So400m / H-14, zero-padded to 96 in LDS) two
 * streaming kernels and a workspace of ov_attention_backward_workspace_bytes (row lse and delta); ov_attention_route reports which.
 * Deterministic. */
size_t ov_attention_backward_workspace_bytes(int B, int L, int H, int hd);
int ov_attention_backward(const ov_bf16* qkv, int64_t ld_qkv, const ov_bf16* out, int64_t ld_out, const ov_bf16* dout, int64_t ld_dout,
                          ov_bf16* dqkv, int64_t ld_dqkv, int B, int L, int H, int hd, float scale, void* workspace,
                          size_t workspace_bytes, ov_stream_t stream);
/* The same with the forward's row statistics kept by ov_attention_lse (lse [B*H][L rounded up to 32] fp32, or NULL): the resident
 * kernel then skips its own score pass; the streaming kernels ignore it. */
int ov_attention_backward_saved(const ov_bf16* qkv, int64_t ld_qkv, const ov_bf16* out, int64_t ld_out, const ov_bf16* dout, int64_t ld_dout,
                                ov_bf16* dqkv, int64_t ld_dqkv, const float* lse, int B, int L, int H, int hd, float scale, void* workspace,
                                size_t workspace_bytes, ov_stream_t stream);
/* Backward of ov_attention_prefix under the same visibility rule: always the two streaming kernels (every L and head dim), which skip
 * the invisible tile pairs in the dQ pass and in the dK / dV pass; deterministic.  The workspace (row lse and delta) is needed for
 * every shape: ov_attention_prefix_backward_workspace_bytes >= ov_attention_backward_workspace_bytes.  prefix == L is
 * ov_attention_backward itself (bitwise); prefix outside [0, L] is OV_ERR_INVALID. */
size_t ov_attention_prefix_backward_workspace_bytes(int B, int L, int H, int hd);
int ov_attention_prefix_backward(const ov_bf16* qkv, int64_t ld_qkv, const ov_bf16* out, int64_t ld_out, const ov_bf16* dout,
                                 int64_t ld_dout, ov_bf16* dqkv, int64_t ld_dqkv, int B, int L, int H, int hd, float scale, int prefix,
                                 void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* ---- attentional pooling (attn_pool.hip): cross-attention from n_q projected queries, shared by every image, to the L keys of each
 * image: out[b] = softmax(scale q k_b^T) v_b.  q [n_q, H*hd] has no batch stride; kv [B*L, 2*H*hd] holds the k | v column blocks with
 * heads contiguous inside each (the K/V projection GEMM's output); out [B*n_q, H*hd] has heads merged (the out-proj GEMM's operand).
 * lse (or NULL): [B*H][n_q rounded up to 32] fp32 row log-sum-exp in log2 units, entries [0, n_q) of each row written, for the
 * backward.  Same arithmetic as ov_attention (fp32 scores in log2 units, online softmax with the lazy rescale, P rounded to bf16).
 * hd % 8 == 0 and hd <= 96 (zero-padded in LDS), 1 <= n_q <= 256: OV_ERR_UNSUPPORTED otherwise.  B, L, H >= 1, every row pitch a
 * multiple of 8 and at least as wide as its row, every bf16 pointer 16-byte aligned, lse 4-byte: OV_ERR_INVALID otherwise.  Nothing
 * is launched on an error. */
int ov_attn_pool(const ov_bf16* q, int64_t ld_q, const ov_bf16* kv, int64_t ld_kv, ov_bf16* out, int64_t ld_out, float* lse, int B, int L,
                 int n_q, int H, int hd, float scale, ov_stream_t stream);
/* Backward of ov_attn_pool: from q, kv, the forward's out and lse (required) and the upstream dout [B*n_q, H*hd] it writes
 * dkv [B*L, 2*H*hd] = (dK | dV) in bf16 and dq [n_q, H*hd] in fp32 = the sum over the B images.  Three launches: the dQ pass (a
 * workgroup walks a fixed chunk of images in order and keeps their sum in its accumulators; it also writes delta), the dK / dV pass,
 * and the sum of the chunks' partials in chunk order.  No atomics; the chunk (ov_attn_pool_backward_chunk) depends on n_q alone, so
 * the result depends on the shape only and repeats bitwise.  workspace: ov_attn_pool_backward_workspace_bytes bytes (delta and the
 * partials), 16-byte aligned; OV_ERR_WORKSPACE if short.  ld_dq a multiple of 4 floats, dq 16-byte aligned.  Otherwise the checks of
 * ov_attn_pool. */
size_t ov_attn_pool_backward_workspace_bytes(int B, int L, int n_q, int H, int hd);
int ov_attn_pool_backward_chunk(int n_q);     /* images per dQ partial */
int ov_attn_pool_backward(const ov_bf16* q, int64_t ld_q, const ov_bf16* kv, int64_t ld_kv, const ov_bf16* out, int64_t ld_out,
                          const ov_bf16* dout, int64_t ld_dout, const float* lse, float* dq, int64_t ld_dq, ov_bf16* dkv, int64_t ld_dkv,
                          int B, int L, int n_q, int H, int hd, float scale, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* da = dh * gelu'(a) on the pre-activation a [rows, N] (tanh_form = 0: exact erf GELU, vision; 1: tanh form, text).  N % 8 == 0.
 * h_out (optional) receives gelu(a).  da may alias dh and h_out may alias a (element-wise, in place). */
int ov_gelu_backward(const ov_bf16* a, int64_t lda, const ov_bf16* dh, int64_t lddh, ov_bf16* da, int64_t ldda, ov_bf16* h_out,
                     int64_t ldh, int64_t rows, int N, int tanh_form, ov_stream_t stream);

/* ---- in-situ kernel timing (used by bench.py for the roofline object; off by default) ------------------
 * ov_profile_enable(mask, n): bracket every launch of the selected classes inside ov_tower_forward with a pair
 * of HIP events recorded on the launch stream (n = max launches recorded; resets earlier records; mask 0 = off).
 * ov_profile_read(cls, &ms, &count, &rows): synchronises the recorded events and returns the summed device time and
 * the summed row count M of those launches (launches on the internal tail stream are not recorded). */
enum ov_profile_class {
    OV_PROF_LN = 0, OV_PROF_GEMM_QKV = 1, OV_PROF_ATTN = 2, OV_PROF_GEMM_OUT = 3, OV_PROF_GEMM_FC = 4 /* erf-GELU c_fc (vision) */, OV_PROF_GEMM_PROJ = 5,
    OV_PROF_GEMM_FC_TANH = 6 /* tanh-GELU c_fc (text) */
};
int ov_profile_enable(unsigned class_mask, int max_records);
int ov_profile_read(int cls, double* total_ms, int* count, double* total_rows /* sum of launch M, may be NULL */);

/* Diagnostics: device buffer [workgroup][slots][8] of s_memtime stamps written by the persistent GEMM (NULL = off). */
int ov_debug_gemm_stamps(unsigned long long* buf, int slots);
/* Diagnostics: per-wave epilogue timeline [workgroup][slots][8 waves][8] (NULL = off; `slots` as given to ov_debug_gemm_stamps). */
int ov_debug_gemm_wave_stamps(unsigned long long* wbuf);

/* ---- parameter update of the training step.  The reference's trainer chains optax transforms
 * (src/optim/build_optax.py:272-278, applied at src/main_clip.py:480-483): clip_by_global_norm -> scale_by_adam(b1, b2,
 * mu_dtype=bfloat16) -> add_decayed_weights(wd) -> scale(lr) -> scale_by_schedule -> scale(-1).  One fused pass over flat fp32
 * buffers: p -= lr * ( mu_hat / (sqrt(nu_hat) + eps) + wd * p ), mu kept in bf16, nu in fp32, bias correction by `step` (>= 1).
 * grad_scale multiplies every gradient first (1 / world_size after a SUM all-reduce); gnorm_sq (device scalar from ov_sumsq over the
 * same unscaled gradients, NULL = off) enables global-norm clipping at clip_norm without a host round trip.  HBM-bound: 24 B / element. */
int ov_adamw_step(float* p, const float* g, ov_bf16* mu, float* nu, int64_t n, float lr, float b1, float b2, float eps, float wd,
                  int step, float grad_scale, const float* gnorm_sq, float clip_norm, ov_stream_t stream);
/* out[0] = (accumulate ? out[0] : 0) + sum_i g[i]^2   (two-stage fixed-order reduction: deterministic). */
size_t ov_sumsq_workspace_bytes(void);
int ov_sumsq(const float* g, int64_t n, float* out, int accumulate, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* ---- tower level (the resblock loop and the two encoders) --------------------------------------- */

typedef struct ov_tower ov_tower;     /* opaque host object holding BORROWED device weight pointers */

typedef struct {
    int width;        /* D */
    int layers;
    int heads;
    int mlp;          /* true hidden width (int(D*mlp_ratio)) */
    int mlp_pad;      /* leading dimension / padded hidden width, % 64 == 0, >= mlp */
    int gelu_tanh;    /* 0 = erf (vision), 1 = tanh (text) */
    float ln_eps;     /* 1e-6 */
} ov_tower_cfg;

typedef struct {      /* one ResidualAttentionBlock; weights bf16 [out,in] row-major, LN/bias fp32 */
    const float *ln1_w, *ln1_b;
    const ov_bf16* qkv_w;  const float* qkv_b;     /* [3D, D], [3D]   attn.in_proj_*        */
    const ov_bf16* out_w;  const float* out_b;     /* [D, D],  [D]    attn.out_proj.*       */
    const float *ln2_w, *ln2_b;
    const ov_bf16* fc_w;   const float* fc_b;      /* [mlp_pad, D], [mlp_pad] (pad rows = 0) */
    const ov_bf16* proj_w; const float* proj_b;    /* [D, mlp_pad] (pad cols = 0), [D]      */
    /* Optional LN fold (both NULL = off).  When set, qkv_w / fc_w hold gamma-scaled weights W', qkv_b / fc_b hold cvec, and
     * these are the column sums of W' (see ov_gemm_ln); ln1_* / ln2_* are then unused by the tower. */
    const float* qkv_colsum;                       /* [3D]      */
    const float* fc_colsum;                        /* [mlp_pad] */
} ov_block_weights;

typedef struct {      /* optional fp8 (OCP e4m3) copies of a block's four weight matrices for the fp8 path (config #5): bytes
                       * [out, in] row-major + one fp32 dequantisation scale per output row; qkv_b / fc_b are the module's own
                       * biases (ov_block_weights holds the LN-folded ones), out/proj biases are taken from ov_block_weights */
    const unsigned char* qkv_w8;  const float* qkv_s;  const float* qkv_b;     /* [3D, D], [3D], [3D]           */
    const unsigned char* out_w8;  const float* out_s;                         /* [D, D], [D]                   */
    const unsigned char* fc_w8;   const float* fc_s;   const float* fc_b;      /* [mlp_pad, D], [mlp_pad] x 2   */
    const unsigned char* proj_w8; const float* proj_s;                        /* [D, mlp_pad], [D]             */
} ov_block_fp8;

ov_tower* ov_tower_create(const ov_tower_cfg* cfg);
void      ov_tower_destroy(ov_tower* t);
int       ov_tower_set_block(ov_tower* t, int layer, const ov_block_weights* w);
/* Once EVERY layer has an fp8 copy (and until one is cleared with q == NULL) ov_tower_forward runs the fp8 path: LayerNorm fused
 * with row quantisation, fp8 GEMMs (ov_gemm_fp8), bf16 attention, row re-quantisation in front of out_proj / c_proj.  Needs
 * width and mlp_pad % 128 == 0 and >= 384.  ov_tower_workspace_bytes grows accordingly: query it after setting the copies. */
int       ov_tower_set_block_fp8(ov_tower* t, int layer, const ov_block_fp8* q);
/* Static (delayed) scales of the two re-quantised activations of the fp8 path.  amax: device float[4 * layers] (borrowed):
 * [layer] = MLP hidden, [layers + layer] = attention output, [2 * layers ...) = the same two sets as recorded during the
 * running forward (rolled into the first half at the top of the next one).  mode 0: off (both are written in bf16 and re-quantised row by row); 1: same, and
 * their running maxima are recorded into amax (calibration); 2: the producers (c_fc epilogue, attention epilogue for head_dim 64)
 * write e4m3 directly with the scale 2 * amax / 448 and the consumers (c_proj, out_proj) read it with that scalar scale; 3: as 2
 * but FROZEN: the recorded maxima are never rolled into the scales (bitwise repeatable, batch-composition invariant results). */
int       ov_tower_set_fp8_hidden_scale(ov_tower* t, float* amax, int mode);
/* Mixed precision of the fp8 path: mask[layer] (HOST array of n == layers bytes, copied) says which of the block's four GEMMs take e4m3
 * operands; the others run exactly as in the bf16 path (LN fold included).  NULL restores OV_FP8_ALL for every layer.  The c_fc ->
 * c_proj hand-over stays in e4m3 only where both are in the mask; a lone fp8 c_proj / out_proj re-quantises its bf16 input row by
 * row (or, out_proj with mode >= 2 and head_dim 64, reads the attention kernel's e4m3 output).  Reference: none (the reference has no
 * fp8 mode); shape source scripts/project/openvision/train.sh:18 (BASELINE.json config #5). */
#define OV_FP8_QKV 1
#define OV_FP8_OUT 2
#define OV_FP8_FC 4
#define OV_FP8_PROJ 8
#define OV_FP8_ALL 15
int       ov_tower_set_fp8_mask(ov_tower* t, const unsigned char* mask, int n);
/* Attention mask of every block of the tower (host state only): prefix = -1 (the default at creation) is unmasked; prefix >= 0 makes
 * every walk -- ov_tower_forward, ov_tower_forward_saving[_from], ov_tower_backward[_partial / _input] and the checkpointed pair --
 * run ov_attention_prefix / ov_attention_prefix_backward with that prefix.  A later call whose L is smaller than the prefix returns
 * OV_ERR_INVALID; a tower in fp8 / fp8-mixed precision with a prefix set returns OV_ERR_UNSUPPORTED from ov_tower_forward (no fp8
 * under a mask).  prefix < -1 is OV_ERR_INVALID.  The sizes ov_tower_saved_bytes* / *_workspace_bytes report hold for either state. */
int       ov_tower_set_prefix(ov_tower* t, int prefix);
/* Stochastic depth ("drop path", the reference's DropPath: src/models/common.py:659-675) on the training walks.  A table says, for
 * every block i of the tower and each of its two residual branches j (0 = attention, 1 = MLP), which of the B samples the branch
 * keeps; a kept sample's branch output is multiplied by scale[i] = 1 / keep_i, a dropped sample's branch is zero and is not computed:
 *   idx    device int32 [layers][2][B]   the kept samples' numbers first (ascending or not), then the dropped ones'
 *   slot   device int32 [layers][2][B]   the inverse: slot[b] = j where idx[j] == b and j < count, -1 for a dropped sample
 *   count  host   int   [layers][2]      kept samples of the branch, 0 .. B           (copied by the call)
 *   scale  host   float [layers]         > 0                                          (copied by the call)
 * The device arrays and `scratch` (ov_tower_drop_path_workspace_bytes(t, B, L) bytes for the walks' L, 16-byte aligned) are
 * borrowed until the table is cleared with idx == NULL.  While a table is set, ov_tower_forward_saving[_from], the checkpointed
 * pair and ov_tower_backward[_partial / _input] must be called with the table's B (OV_ERR_INVALID otherwise; OV_ERR_WORKSPACE for a
 * short scratch), and a branch whose count < B or whose scale != 1 runs
 *   ov_sample_gather -> LayerNorm -> GEMM(s) / attention on count L rows -> product with its bias -> ov_sample_scatter_axpy
 * and the mirror image in the backward (weight and bias gradients see the kept rows; count == 0: zeros); a dropped sample's rows of
 * the branch's output and input gradient are the residual's, bitwise.  A branch with count == B and scale == 1, and every walk with
 * no table, issue exactly the launches they issue without this call.  The saved slots keep their layout: a compact branch uses the
 * leading count L rows of its regions.  ov_tower_forward (inference) returns OV_ERR_UNSUPPORTED while a table is set. */
int       ov_tower_set_drop_path(ov_tower* t, const int* idx, const int* slot, const int* count, const float* scale, int B,
                                 void* scratch, size_t scratch_bytes);
size_t    ov_tower_drop_path_workspace_bytes(const ov_tower* t, int B, int L);
/* The two glue passes of a compact branch (droppath.hip).  The L rows of a sample are contiguous, L rows of D bf16, D % 8 == 0;
 * pointers 16-byte aligned; B <= 65535.
 *   ov_sample_gather        dst[j L + t, :] = bf16(scale * src[idx[j] L + t, :]) for j < k; scale == 1.0f is a bitwise copy; k == 0
 *                           launches nothing.  idx: device int32, values in [0, B) (others move nothing).
 *   ov_sample_scatter_axpy  for every b < B: out[b] = bf16(res[b] + scale * y[slot[b]]) where 0 <= slot[b] < k, else out[b] = res[b]
 *                           bitwise (nothing is written where out == res).  slot: device int32 [B].  out may alias res, not y.
 * The backward uses this adding form too: the compact LayerNorm backward runs without its residual input, and the scatter adds the
 * incoming gradient as `res`. */
int       ov_sample_gather(const ov_bf16* src, const int* idx, ov_bf16* dst, int B, int k, int L, int D, float scale, ov_stream_t stream);
int       ov_sample_scatter_axpy(const ov_bf16* res, const ov_bf16* y, const int* slot, ov_bf16* out, int B, int k, int L, int D, float scale,
                                 ov_stream_t stream);
size_t    ov_tower_workspace_bytes(const ov_tower* t, int B, int L);
/* x[B*L, D] bf16 is updated in place through all `layers` blocks. */
int       ov_tower_forward(const ov_tower* t, ov_bf16* x, int B, int L, void* workspace,
                           size_t workspace_bytes, ov_stream_t stream);

/* ---- backward of one ResidualAttentionBlock (transformer.py:254-265 differentiated by autograd in the
 * reference).  Activation recomputation: the caller keeps only the block INPUT x [B*L, D]; ln_1, qkv, attention, x1, ln_2 and the
 * c_fc pre-activation are recomputed with the forward kernels, then ov_gelu_backward / ov_linear_backward / ov_layernorm_backward /
 * ov_attention_backward run the chain rule.  `w` holds the module's own weights (no LN fold: qkv_colsum == fc_colsum == NULL,
 * qkv_b / fc_b the module biases).  Gradients: weights bf16 [out, in] (same layout as the weights), biases and LN parameters fp32;
 * all written (not accumulated; rows / columns of the MLP padding, mlp .. mlp_pad, come out as zeros when the weights' padding is
 * zero).  dx may alias dy.  width % 64 == 0, head_dim % 8 == 0 and <= 96, mlp_pad % 64 == 0; OV_ERR_UNSUPPORTED otherwise. */
typedef struct {
    float *ln1_w, *ln1_b;          /* [D] */
    ov_bf16* qkv_w; float* qkv_b;  /* [3D, D], [3D] */
    ov_bf16* out_w; float* out_b;  /* [D, D], [D] */
    float *ln2_w, *ln2_b;          /* [D] */
    ov_bf16* fc_w;  float* fc_b;   /* [mlp, D], [mlp] */
    ov_bf16* proj_w; float* proj_b;/* [D, mlp], [D] */
} ov_block_grads;
typedef struct {      /* optional forward intermediates kept for the backward (the first three together or none) */
    const ov_bf16* qkv;        /* [B*L, 3D]  packed q | k | v */
    const ov_bf16* attn_out;   /* [B*L, D]   attention output before out_proj */
    const ov_bf16* x1;         /* [B*L, D]   x + attention branch */
    const ov_bf16* fc_pre;     /* [B*L, mlp_pad]  c_fc output before GELU (ov_gemm_keep), or NULL = recomputed */
    const ov_bf16* ln1_out;    /* [B*L, D]   ln_1(x), or NULL = recomputed */
    const ov_bf16* ln2_out;    /* [B*L, D]   ln_2(x1), or NULL = recomputed */
    const ov_bf16* fc_act;     /* [B*L, mlp_pad]  gelu(fc_pre), or NULL = recomputed; with fc_pre set too, the backward folds the GELU
                                * derivative into the epilogue of dy Wproj (OV_EPI_GELU_GRAD_*) and runs no element-wise pass */
    const float* attn_lse;     /* [B*heads][L rounded up to 32]  row log-sum-exp from ov_attention_lse, or NULL = recomputed */
} ov_block_saved;
size_t ov_block_backward_workspace_bytes(const ov_tower_cfg* cfg, int B, int L);
int ov_block_backward(const ov_tower_cfg* cfg, const ov_block_weights* w, const ov_bf16* x, const ov_block_saved* saved /* or NULL */,
                      const ov_bf16* dy, ov_bf16* dx, const ov_block_grads* g, int B, int L, void* workspace, size_t workspace_bytes,
                      ov_stream_t stream);
/* The same for a block whose attention ran under ov_attention_prefix (prefix in [0, L]; -1 = unmasked = ov_block_backward);
 * saved->attn_lse is ignored when 0 <= prefix < L.  Same workspace. */
int ov_block_backward_prefix(const ov_tower_cfg* cfg, const ov_block_weights* w, const ov_bf16* x, const ov_block_saved* saved /* or NULL */,
                             const ov_bf16* dy, ov_bf16* dx, const ov_block_grads* g, int prefix, int B, int L, void* workspace,
                             size_t workspace_bytes, ov_stream_t stream);

/* Training-side tower entry points.  ov_tower_forward_saving = the tower forward on the caller's stream that keeps, per layer and
 * token, [x | qkv | attention out | x1 | ln_1 out | ln_2 out | c_fc pre-activation | c_fc activation] (8 D + 2 mlp_pad bf16, plus the
 * attention's fp32 row log-sum-exp per layer; `saved` holds ov_tower_saved_bytes: 52 GB for L/14 at batch 256; nothing of the forward
 * is run a second time by the backward -- ov_tower_forward_checkpointed below keeps the block inputs only and recomputes the rest).
 * bf16 path; the blocks must hold
 * the module's own, unfolded weights.  ov_tower_backward runs ov_block_backward over the layers in reverse: dx [B*L, D] holds
 * d loss / d (tower output) on entry and d loss / d (tower input) on return; grads[layer] receives that block's parameter gradients
 * (written, not accumulated). */
size_t ov_tower_saved_bytes(const ov_tower* t, int B, int L);
int    ov_tower_forward_saving(const ov_tower* t, ov_bf16* x, ov_bf16* saved, int B, int L, void* workspace, size_t workspace_bytes,
                               ov_stream_t stream);
size_t ov_tower_backward_workspace_bytes(const ov_tower* t, int B, int L);
int    ov_tower_backward(const ov_tower* t, const ov_bf16* saved, ov_bf16* dx, const ov_block_grads* grads, int B, int L,
                         void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* Input gradients only (frozen weights: feature visualisation, gradient ascent on the inputs): ov_tower_backward over the same saved
 * activations without any parameter-gradient work (no dW products, bias or LayerNorm parameter sums).  The block backward is one chain
 * of launches, called with every pair by ov_block_backward / ov_tower_backward, with the requested pairs by ov_tower_backward_partial
 * and with none here (its attention half alone: ov_block_attn_backward_input), so dx is bitwise the dx of ov_tower_backward.  The
 * workspace is smaller than ov_tower_backward's: no parameter-gradient staging. */
size_t ov_tower_backward_input_workspace_bytes(const ov_tower* t, int B, int L);
int    ov_tower_backward_input(const ov_tower* t, const ov_bf16* saved, ov_bf16* dx, int B, int L, void* workspace, size_t workspace_bytes,
                               ov_stream_t stream);

/* Frozen parameters (LiT: a locked image tower; gradient ascent through a frozen text tower).  ov_tower_forward_saving_from runs the
 * layers below `first` with exactly the operators of ov_tower_forward_saving, x in place and their intermediates in the workspace
 * (ov_tower_forward_saving_from_workspace_bytes, 0 when first == 0), and keeps the slots of layers [first, layers) in `saved` (slot 0 =
 * layer `first`; ov_tower_saved_bytes_from; NULL iff first == layers).  x and every kept slot are bitwise ov_tower_forward_saving's.
 * ov_tower_backward_partial walks layers layers-1 .. first over those slots: grads[layers - first] requests (weight, bias) pairs, a NULL
 * pair is frozen; a pair with one NULL pointer, or a pointer that is not 16-byte aligned, is OV_ERR_INVALID.  dx holds d(output) on
 * entry; with want_dx it holds d(input of layer `first`) on return, otherwise its contents are unspecified and nothing runs below the
 * lowest block with a requested pair.  Every gradient computed is bitwise ov_tower_backward's (all pairs NULL, first = 0, want_dx = 1:
 * ov_tower_backward_input's dx). */
size_t ov_tower_saved_bytes_from(const ov_tower* t, int first, int B, int L);
size_t ov_tower_forward_saving_from_workspace_bytes(const ov_tower* t, int first, int B, int L);
int    ov_tower_forward_saving_from(const ov_tower* t, int first, ov_bf16* x, ov_bf16* saved, int B, int L, void* workspace,
                                    size_t workspace_bytes, ov_stream_t stream);
size_t ov_tower_backward_partial_workspace_bytes(const ov_tower* t, int B, int L);
int    ov_tower_backward_partial(const ov_tower* t, int first, const ov_bf16* saved, ov_bf16* dx, const ov_block_grads* grads, int want_dx,
                                 int B, int L, void* workspace, size_t workspace_bytes, ov_stream_t stream);

/* Activation recomputation (the reference's remat='full' per block; CLIP.set_grad_checkpointing).  ov_tower_forward_checkpointed runs
 * the layers below `first` as ov_tower_forward_saving_from does (x in place, intermediates in `slot`) and keeps, for each layer
 * i >= first, only its input in ckpt[i - first] (ov_tower_checkpoint_bytes: (layers - first) B L D bf16; NULL iff first == layers):
 * layer i reads ckpt[i - first], puts its intermediates in `slot` (ov_tower_slot_bytes: one layer's slot without its x part) and
 * writes its output into ckpt[i - first + 1], the last one into x.  On return `slot` holds the top layer's slot (first < layers).
 * ov_tower_backward_checkpointed walks layers layers-1 .. first with ov_tower_backward_partial's grads / want_dx / lowest-layer rules
 * and workspace (ov_tower_backward_partial_workspace_bytes); before each block backward it recomputes that layer's slot from its
 * checkpoint with the forward's own launches (c_proj excepted: the backward never reads the block output), except the top layer's
 * when `slot_holds_top` says `slot` is untouched since the forward.  x, the loss and every gradient are bitwise those of the saving
 * path.  Same rejections as the saving entry points; a short slot is OV_ERR_WORKSPACE. */
size_t ov_tower_checkpoint_bytes(const ov_tower* t, int first, int B, int L);
size_t ov_tower_slot_bytes(const ov_tower* t, int B, int L);
int    ov_tower_forward_checkpointed(const ov_tower* t, int first, ov_bf16* x, ov_bf16* ckpt, void* slot, size_t slot_bytes, int B, int L,
                                     ov_stream_t stream);
int    ov_tower_backward_checkpointed(const ov_tower* t, int first, const ov_bf16* ckpt, void* slot, size_t slot_bytes, int slot_holds_top,
                                      ov_bf16* dx, const ov_block_grads* grads, int want_dx, int B, int L, void* workspace,
                                      size_t workspace_bytes, ov_stream_t stream);

/* ---- MLP-feature objective (feature visualisation: a forward hook on resblocks[layer].mlp.gelu, ov-feature-visualization.py:211) --
 * The attention half of one block, x1 = x + out_proj(attn(ln_1(x))) (transformer.py:263), keeping qkv [B*L, 3D], attn_out [B*L, D],
 * x1 [B*L, D] and, where the resident attention backward reads it (ov_attention_route_t::keep_lse), lse [B*heads][L rounded up to 32] fp32
 * (NULL = not kept).  `w` holds the module's own weights; only ln_1, in_proj and out_proj are read. */
int ov_block_attn_forward_saving(const ov_tower_cfg* cfg, const ov_block_weights* w, const ov_bf16* x, ov_bf16* qkv, ov_bf16* attn_out,
                                 ov_bf16* x1, float* lse, int B, int L, ov_stream_t stream);
/* Its input gradient: dx = dx1 + (out_proj, attention, in_proj, ln_1 backward of dx1); no parameter gradients. */
size_t ov_block_attn_backward_input_workspace_bytes(const ov_tower_cfg* cfg, int B, int L);
int ov_block_attn_backward_input(const ov_tower_cfg* cfg, const ov_block_weights* w, const ov_bf16* x, const ov_bf16* qkv,
                                 const ov_bf16* attn_out, const float* lse /* or NULL */, const ov_bf16* dx1, ov_bf16* dx, int B, int L,
                                 void* workspace, size_t workspace_bytes, ov_stream_t stream);
/* pre[r] = ln_2(x1[r]) . fc_w[feature] + fc_b[feature] (fp32 [B*L]; fc_b may be NULL), mean[b] = mean over tokens 1 .. L-1 of
 * gelu(pre[b*L + t]) (fp32 [B]; erf or tanh GELU, exact).  0 <= feature < mlp (the true hidden width, not the padded one); L >= 2;
 * D % 8 == 0, D <= 4096.  Deterministic (fixed-order reduction), no workspace. */
int ov_mlp_feature_forward(const ov_bf16* x1, int64_t ldx, const float* ln2_w, const float* ln2_b, const ov_bf16* fc_w, int64_t ldw,
                           const float* fc_b, int feature, int mlp, int gelu_tanh, int B, int L, int D, float eps, float* pre, float* mean,
                           ov_stream_t stream);
/* dx1[r] = ln_2-backward(x1[r], g_t * fc_w[feature]) with g_t = dmean[b] / (L-1) * gelu'(pre[r]) for t >= 1 and 0 for the CLS row:
 * d sum_b dmean[b] mean[b] / d x1, bf16 [B*L, D].  dmean: DEVICE fp32 [B]. */
int ov_mlp_feature_backward(const ov_bf16* x1, int64_t ldx, const float* ln2_w, const ov_bf16* fc_w, int64_t ldw, int feature, int mlp,
                            int gelu_tanh, const float* pre, const float* dmean, ov_bf16* dx1, int64_t lddx, int B, int L, int D, float eps,
                            ov_stream_t stream);

/* ---- the feature-visualisation loop around that objective (ov-feature-visualization.py:120-136, 214-215; csrc/vizloop.hip).  img fp32
 * [N,3,S,S]; B = R N batch rows, row b = r N + n (img.repeat(R,1,1,1)); table: the step's fp32 [3][3B] = mean | std | noise of row b,
 * channel c at b*3 + c (device); off1 / off2: the step's roll (any int, taken mod S).  All four enqueue on `stream`, allocate nothing,
 * use no atomics (fixed-order sums: bitwise repeatable).  Null pointers, non-positive sizes and misaligned buffers are OV_ERR_INVALID:
 * 16 bytes for the image-shaped buffers, cols, norms and the optimiser state, 4 bytes for table, m and history_row (a step's row of a
 * packed [steps + 1][3][3B] table or [steps + 1][3] history starts wherever it falls).  Then S % P != 0, S outside [P, 1024] and
 * R N > 4096 are OV_ERR_UNSUPPORTED. */

/* aug[b,c,y,x] = ((img[n,c,(y-off1) mod S,(x-off2) mod S] - mean) / std) + noise: fp32 in that order, a true division.  cols [B*g*g, Kpad]
 * = bf16(aug) as conv1 operand rows (ov_im2col_patches' layout, the columns past 3 P^2 zero; Kpad % 8 == 0); aug fp32 [B,3,S,S] or NULL. */
int ov_viz_augment(const float* img, const float* table, int N, int R, int S, int P, int Kpad, int off1, int off2, ov_bf16* cols,
                   float* aug, ov_stream_t stream);
/* BaseTotalVariation's four difference fields of aug fp32 [B,3,S,S] (x, y, the two diagonals; none across the plane's border):
 * norms[dir*3B + b*3 + c] = the plane's L2 norm of field dir (fp32 [4][3B]); *tv (device scalar, NULL = skipped) = sum_dir
 * mean_planes(norm) * S^2 / size^2 (TotalVariation(2, size)). */
int ov_viz_tv(const float* aug, int B, int S, int size, float* norms, float* tv, ov_stream_t stream);
/* dimg[n,c,y',x'] = sum_{r ascending} d_aug[b,c,(y'+off1) mod S,(x'+off2) mod S] / std[b,c], d_aug = fp32(dcols entry of that pixel)
 * + c_tv * d tv / d aug (+-diff / (norm 3B) * S^2 / size^2 over the up to eight differences the pixel ends; 0 where norm == 0).  dcols
 * bf16 [B*g*g, ldc] in cols' layout; aug, norms, table as above.  history_row (device fp32 [3], NULL together with m = skipped) =
 * (loss, c_feat * -(1/B^2) sum_b m[b], c_tv * tv), loss their sum; m device fp32 [B]. */
int ov_viz_augment_backward(const ov_bf16* dcols, int64_t ldc, const float* aug, const float* norms, const float* table, const float* m,
                            int N, int R, int S, int P, int off1, int off2, int size, float c_feat, float c_tv, float* dimg,
                            float* history_row, ov_stream_t stream);
/* One step of torch.optim.Adamax (torch 2.10 _single_tensor_adamax, no weight decay) followed by the script's Clip, on flat fp32 [n]:
 * ea += (g - ea) (1 - b1);  ei = max(b2 ei, |g| + eps);  img = clamp(img - clr ea / ei, lo, hi), clr = lr_t / (1 - b1^t) from the host.
 * 0 <= b1, b2 < 1, eps >= 0, lo <= hi. */
int ov_adamax_clip_step(float* img, const float* dimg, float* ea, float* ei, int64_t n, double clr, double b1, double b2, double eps,
                        float lo, float hi, ov_stream_t stream);

/* ---- the gradient-ascent loop around the frozen text tower (ov-gradient-ascent.py:226-259, 380-381; csrc/ascent.hip).  normu fp32
 * [R, V] is what is learned, R = B K rows (row r = b K + k); e fp32 [R, V] the step's Exp(1) draws; z = (normu - log e) / tau, ys =
 * softmax(z), both fp32 with true divisions, log e the correctly rounded fp32 logarithm (taken in double).  All five enqueue on `stream`, allocate nothing and use no atomics (fixed-order sums:
 * bitwise repeatable); nothing is flushed to zero.  Null pointers, non-positive sizes, tau <= 0 and misaligned buffers are
 * OV_ERR_INVALID: 16 bytes for dX and W, 8 for ids, 4 for everything else (a step's row of a packed history starts wherever it
 * falls).  R > 4096 is OV_ERR_UNSUPPORTED. */

/* out[b,c,y,x] = (bilinear(img[c]; sx, sy) - mean[c]) / stdv[c] with (sx, sy) = (a0 x + a1 y + a2, a3 x + a4 y + a5), mats[b] = a0..a5
 * the INVERSE map in pixel coordinates (destination -> source): the four taps around (sx, sy), each zero outside the image, weights
 * (x1 - sx)(y1 - sy) ... as F.grid_sample('bilinear', 'zeros', align_corners=False) forms them; fp32, a true division.  img fp32
 * [3,S,S]; mats fp32 [B,6], mean / stdv fp32 [3] (device); out [B,3,S,S] in out_dtype (OV_F32 / OV_BF16).  The identity matrix gives
 * the normalised source bit for bit.  S <= 4096. */
int ov_ga_affine(const float* img, const float* mats, const float* mean, const float* stdv, void* out, int out_dtype, int B, int S,
                 ov_stream_t stream);
/* Per row r: z[r,v] = (normu - log e) / tau (fp32 [R,V], kept for the two kernels below: the double logarithm is formed once), idx[r] =
 * the first position of max_v z, zmax[r] = that maximum, zsum[r] = sum_v exp(z - zmax) (one workgroup per row, one order).
 * history_row (int32 [R], NULL = skipped) receives idx as well; ids (int64 [R / K, T], NULL = skipped) receives idx[b K + k] at
 * [b, T - K + k]: the K learned positions close each row of the id matrix, the others are the caller's. */
int ov_ga_sample(const float* normu, const float* e, float tau, int R, int V, int K, int T, float* z, int* idx, float* zmax, float* zsum,
                 int* history_row, int64_t* ids, ov_stream_t stream);
/* ceil(V / 128): the slabs of the vocabulary, one partial sum per row and slab (parts [R, that many]); 0 for V <= 0. */
int ov_ga_parts_blocks(int V);
/* gy[r,v] = sum_d dX[r,d] W[v,d] (fp32 [R,V]; bf16 operands, fp32 accumulation on the MFMA) and parts[r, blk] = sum over slab blk of
 * gy[r,v] ys[r,v], ys = exp(z - zmax) / zsum.  dX bf16 [R,D], W bf16 [V,D], both dense; z / zmax / zsum from ov_ga_sample.  R and V of
 * any size; D % 64 == 0 and D <= 1216, OV_ERR_UNSUPPORTED otherwise.  W is read once for every 64 rows of dX. */
int ov_ga_token_grad(const ov_bf16* dX, const ov_bf16* W, const float* z, const float* zmax, const float* zsum, int R, int V, int D,
                     float* gy, float* parts, ov_stream_t stream);
/* c_r = sum_blk parts[r, blk] (ascending), g = ys (gy - c_r) / tau, then one step of torch.optim.Adam (_single_tensor_adam, no weight
 * decay, no amsgrad) on normu in its own operation order: ea += (g - ea)(1 - b1); es = b2 es + (1 - b2) g g; denom = sqrt(es) /
 * sqrt(bias_correction2) + eps; normu -= (lr / bias_correction1) ea / denom.  bias_correction{1,2} = 1 - b{1,2}^t from the host, in
 * double.  g (fp32 [R,V], NULL = skipped) receives the gradient. */
int ov_ga_adam(const float* gy, const float* parts, float* normu, const float* z, const float* zmax, const float* zsum, float tau, int R,
               int V, float* exp_avg, float* exp_avg_sq, double lr, double b1, double b2, double eps, double bias_correction1,
               double bias_correction2, float* g, ov_stream_t stream);
/* loss1_row[j] = -100 mean_i cos(tx_j, img_i), cos = x.y / (max(|x|, 1e-8) max(|y|, 1e-8)) (torch.cosine_similarity); dtx = d mean_j
 * loss1[j] / d tx.  tx, img, dtx, best_tx fp32 [B,E]; any E >= 1, B <= 64 (OV_ERR_UNSUPPORTED above).  If the mean is below best[0]
 * (device fp32; start it at +inf): best[0] = mean, best_step[0] = step, best_tx = tx.  One launch, one workgroup. */
int ov_ga_cosine_loss(const float* tx, const float* img, int B, int E, int step, float* loss1_row, float* dtx, float* best, int* best_step,
                      float* best_tx, ov_stream_t stream);

typedef struct {      /* VisionTransformer front/back ends (OpenVision: no ln_pre, no conv bias) */
    int image_size, patch_size, kpad;              /* kpad = roundup(3*P*P, 64) */
    int pool_avg;                                  /* 1 = 'avg' (skip cls), 0 = 'tok' */
    int final_ln_after_pool;                       /* 1 for OpenVision; 0 (ln_post before the pool) under 'tok' pooling only,
                                                      where it is the same arithmetic, else OV_ERR_UNSUPPORTED */
    int embed_dim, embed_pad;                      /* E, roundup(E, 8) */
    const ov_bf16* conv_w;                         /* [D, kpad] bf16, pad cols = 0 */
    const float* cls;                              /* [D] */
    const ov_bf16* pos;                            /* [L, D] bf16 */
    const float* pos_f32;                          /* [L, D] fp32 (row 0 used for the cls row) */
    const float *ln_post_w, *ln_post_b;            /* [D] */
    const ov_bf16* proj_t;                         /* [E, D] bf16 = visual.proj^T */
} ov_vision_head;

size_t ov_vision_workspace_bytes(const ov_tower* t, const ov_vision_head* h, int B);
/* The workspace of ov_vision_embed (K = 0) or of ov_vision_embed_keep with K kept patches (1 <= K <= G); 0 for bad arguments. */
size_t ov_vision_embed_workspace_bytes(const ov_tower* t, const ov_vision_head* h, int B, int K);
/* The workspace of ov_vision_head_forward[_tokens]; 0 for bad arguments. */
size_t ov_vision_head_workspace_bytes(const ov_tower* t, const ov_vision_head* h, int B);
/* image [B,3,S,S] -> tokens x[B*L, D] bf16 (patch embed + cls + pos); x caller-provided. */
int ov_vision_embed(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, int B,
                    ov_bf16* x, void* workspace, size_t workspace_bytes, ov_stream_t stream);
/* tokens x[B*L, D] -> features [B, E] fp32 (pool -> ln_post -> proj), optionally L2-normalised. */
int ov_vision_head_forward(const ov_tower* t, const ov_vision_head* h, const ov_bf16* x, int B,
                           float* features, int normalize, void* workspace, size_t workspace_bytes,
                           ov_stream_t stream);
/* VisionTransformer.forward + optional F.normalize: image -> [B, E] fp32. */
int ov_encode_image(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, int B,
                    float* features, int normalize, void* workspace, size_t workspace_bytes,
                    ov_stream_t stream);
/* ov_vision_head_forward on tokens x[B*L, D] with L given (patch dropout: L = 1 + K). */
int ov_vision_head_forward_tokens(const ov_tower* t, const ov_vision_head* h, const ov_bf16* x, int B, int L,
                                  float* features, int normalize, void* workspace, size_t workspace_bytes,
                                  ov_stream_t stream);
/* Patch dropout (transformer.py:619): the same at L' = 1 + K tokens, image b keeping the patches keep[b, 0..K-1] (int32 [B, K], in
 * that order; see ov_im2col_patches_keep).  Kept tokens are bitwise the matching tokens of ov_vision_embed.  *err_flag (device int,
 * may be NULL) is set when an index lies outside [0, G).  1 <= K <= G, else OV_ERR_INVALID. */
size_t ov_vision_keep_workspace_bytes(const ov_tower* t, const ov_vision_head* h, int B, int K);
int ov_vision_embed_keep(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, const int* keep, int B,
                         int K, ov_bf16* x, int* err_flag, void* workspace, size_t workspace_bytes, ov_stream_t stream);
int ov_encode_image_keep(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, const int* keep, int B,
                         int K, float* features, int normalize, int* err_flag, void* workspace, size_t workspace_bytes,
                         ov_stream_t stream);

enum ov_text_pool { OV_TEXT_POOL_FIRST = 0, OV_TEXT_POOL_LAST = 1, OV_TEXT_POOL_ARGMAX = 2 };   /* text_global_pool, transformer.py:655-658 */

typedef struct {      /* CLIP text front/back ends */
    int context_length, vocab_size;
    int pool_last;                                 /* enum ov_text_pool: 0 = 'first', 1 = 'last', 2 = 'argmax' (the row of the
                                                      largest token id of each caption, the first of equals: ov_token_argmax) */
    int embed_dim;
    const ov_bf16* token_embedding;                /* [V, D] bf16 */
    const ov_bf16* pos;                            /* [T, D] bf16 */
    const float *ln_final_w, *ln_final_b;          /* [D] */
    const ov_bf16* proj_t;                         /* [E, D] bf16 = text_projection^T */
} ov_text_head;

size_t ov_text_workspace_bytes(const ov_tower* t, const ov_text_head* h, int B);
/* CLIP.encode_text: tokens int64 [B, T] -> [B, E] fp32.  *err_flag (device int, may be NULL) is set
 * to 1 when a token id is outside [0, V).  'argmax' pooling finds each caption's row on the device (an int32 [B] behind the head's
 * buffers: the workspace is that much larger, and only then), so the call stays capturable; a pool mode outside ov_text_pool is
 * OV_ERR_INVALID.  A causal tower (ov_tower_set_prefix(t, 0)) is exact on the pooled-rows tail too: the rows past the last
 * attention are per-token. */
int ov_encode_text(const ov_tower* t, const ov_text_head* h, const int64_t* tokens, int B,
                   float* features, int normalize, int* err_flag, void* workspace,
                   size_t workspace_bytes, ov_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OVHIP_H */
