// attention.hip — fused multi-head self-attention, gfx950 (MI355X): non-causal (head_dim 64 tuned, generic up to 96) and, in the generic
// kernel's MASK form, prefix-causal (ov_attention_prefix, at the end of this file).
//
// Replaces the softmax(q k^T / sqrt(hd)) v core of nn.MultiheadAttention (reference
// open_clip/transformer.py:225,239-252; no mask: attn_mask=None, no dropout in eval) with a flash-style
// kernel: the [L, L] score matrix never leaves registers.  The online-softmax recurrence is the one of
// the reference's blockwise attention (src/models/bpt.py:108-124: running max, rescaled numerator and
// denominator per key block).
//
// Input is the packed qkv activation [B*L, 3*H*64] written by the QKV GEMM (q | k | v column blocks), output
// is [B*L, H*64] with heads merged -- exactly the operand layout of the out-proj GEMM, so no head
// split/merge kernels exist.
//
// A wave owns a query tile of 32 rows.  K and V of the (batch, head) are staged into LDS and shared by all waves of
// the workgroup:
//   K image  [key][64 d]   128-B rows, 16-B chunk index ^= (key >> 1) & 7  -> conflict-free ds_read_b128
//   V image  [d half][key][32 d] 64-B rows                                  -> conflict-free ds_read_b64_tr_b16
// Per 32-key tile and wave (v_mfma_f32_32x32x16_bf16 throughout):
//   S^T = K . Q^T          (K rows as the A operand, Q fragments kept in registers as B)  -> a lane holds
//                          16 of the 32 keys of ONE query, so row max / row sum are lane-local + 1 shuffle
//   P^T = exp2(S^T - m)    packed pairwise to bf16: the accumulator tile IS the next B operand
//   O^T += V^T . P^T       (V^T fragments via the transposing LDS read)
#include "common.h"
#include "attn_tile.h"
#include <stdlib.h>

namespace {

struct AttnArgs {
    const ov_bf16* qkv; int64_t ldq;
    ov_bf16* out; int64_t ldo;
    int B, L, H, nqt, KC;
    float scale_log2;
    int prefix;                   // MASK kernels: key j is visible to query i iff j < prefix or j <= i
};

typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __forceinline__ bf16x8_t tr_pair(const char* p0, const char* p1) {
    const s16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)p0);
    const s16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)p1);
    typedef short s16x8_t __attribute__((ext_vector_type(8)));
    const s16x8_t c = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8_t, c);
}

// =====================================================================================================
// Persistent kernel (head_dim 64 when two heads' K/V fit in LDS, i.e. padded L <= 320): a workgroup of nqt waves (one per
// 32-row query tile) walks heads bh = blockIdx.x, blockIdx.x + gridDim.x, ...  K/V of head j live in LDS slot j & 1.
// Per head: vmcnt(0) + ONE barrier (head j has landed for everybody, and everybody has left head j-1), then the LDS-DMA
// of head j+1 into the other slot is issued and runs under the MFMAs/softmax of head j -- HBM reads overlap compute.
// The kernel is sized for <= 168 VGPRs (3 waves on the busiest SIMD at L = 257), which leaves room to fetch all K and V
// fragments of a key tile ahead of the MFMAs that use them.
// The V fragments come by transposing LDS reads issued from inline asm (attn::read_v, completed by attn::tr_wait).

// 4 floats -> 4 e4m3 bytes (saturating)
__device__ __forceinline__ unsigned pack_fp8x4(float a, float b, float c, float d) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(a, -448.f, 448.f), __builtin_amdgcn_fmed3f(b, -448.f, 448.f), w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(c, -448.f, 448.f), __builtin_amdgcn_fmed3f(d, -448.f, 448.f), w, true);
    return (unsigned)w;
}

struct AttnPArgs {
    const ov_bf16* qkv; int64_t ldq;
    ov_bf16* out; int64_t ldo;
    int L, H, nqt, KC, nheads;
    float scale_log2;
    const float* out_amax;        // OUT8: the output is e4m3 bytes (ldo in bytes) with the static scale 2 * (*out_amax) / 448
    float* amax_next;             // OUT8, optional: running maximum of |output| (the next call's scale)
    int lone_valu;                // 1: a single-key last tile is folded in on the VALU (OVHIP_ATTN_LONEKEY=0 keeps the tile step)
    float* lse;                   // optional (training forward, bf16 output): lse[head][KC] = row log-sum-exp of scale * q.k in log2 units
};

__device__ __forceinline__ void stage_head(const AttnPArgs& a, int bh, char* slot, int wave, int lane, int nthreads) {
    const int b = bh / a.H, h = bh - b * a.H;
    const int HD = a.H * 64, KC = a.KC, L = a.L;
    // wave-uniform base + 32-bit per-lane byte offsets (L * ldq * 2 < 4 GiB: checked by the launcher): the DMA issue is on every
    // head's critical path, 64-bit per-piece address arithmetic made it ~300 cycles per 1-KiB piece
    const char* base = (const char*)(a.qkv + (int64_t)b * L * a.ldq + h * 64);
    const unsigned rowb = (unsigned)(a.ldq * 2);
    const unsigned last = (unsigned)(L - 1) * rowb;
    char* ks = slot;
    char* vs = slot + KC * 128;
    const int nchunk = KC * 8;
    // K piece q = q0c + lane: key q >> 3, source d-chunk (q & 7) ^ ((key >> 1) & 7).  V piece: d-half dh = (q0c >= 4 KC), key
    // (q - dh 4 KC) >> 2, d-chunk dh * 4 + (q & 3).  q0c is a multiple of 64, so q & 7 = lane & 7 and q & 3 = lane & 3.
    for (int q0c = wave * 64; q0c < nchunk; q0c += nthreads) {   // nothing per-lane is carried between trips (register room)
        {
            const int kkey = (q0c + lane) >> 3;
            const unsigned ro = kkey < L ? (unsigned)kkey * rowb : last;
            const int c = (lane & 7) ^ ((kkey >> 1) & 7);
            __builtin_amdgcn_global_load_lds((gptr_t)(base + (ro + (unsigned)((HD + c * 8) * 2))), (lptr_t)(ks + q0c * 16), 16, 0, 0);
        }
        {
            const int dh = q0c >= KC * 4 ? 1 : 0;                 // wave-uniform
            const int vkey = (q0c - dh * KC * 4 + lane) >> 2;
            const unsigned ro = vkey < L ? (unsigned)vkey * rowb : last;
            __builtin_amdgcn_global_load_lds((gptr_t)(base + (ro + (unsigned)((2 * HD + (dh * 4 + (lane & 3)) * 8) * 2))),
                                             (lptr_t)(vs + q0c * 16), 16, 0, 0);
        }
    }
}

typedef float f32x2_t __attribute__((ext_vector_type(2)));
// p = exp2(s * c - m) on 16 scores, two per v_pk_fma_f32 / v_pk_add_f32 (the softmax is VALU-issue bound; v_exp has no
// packed form); acc collects the two interleaved partial row sums.
__device__ __forceinline__ void exp_rows(f32x16_t& s, float c, float nm, f32x2_t& acc) {
    const f32x2_t cc = {c, c}, mm = {nm, nm};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f32x2_t v = {s[2 * i], s[2 * i + 1]};
        v = __builtin_elementwise_fma(v, cc, mm);
        v[0] = __builtin_amdgcn_exp2f(v[0]);
        v[1] = __builtin_amdgcn_exp2f(v[1]);
        acc += v;
        s[2 * i] = v[0];
        s[2 * i + 1] = v[1];
    }
}

// DEEP = workgroups of <= 8 waves (2 per SIMD, 256 VGPRs each): both K tiles of the next step are fetched behind the S MFMAs
// and all V fragments of a step are in flight from its start.
// OUT8: e4m3 output with a static scale (fp8 path: feeds the out-proj GEMM without a bf16 round trip); same 8 stores per head.
// LSE: also store every query row's log-sum-exp (a.lse; training forward).  A template parameter, not a test of the pointer: a branch
// between the stores and the vmcnt wait that names the prefetched Q registers would let hipcc copy those registers at the merge
// point BEFORE the wait (it did: nondeterministic outputs).
template <bool DEEP, bool OUT8, bool LSE = false>
__global__ __launch_bounds__(DEEP ? 512 : 640, DEEP ? 2 : 3) void attn_fwd_hd64_persist(const AttnPArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    const int L = a.L, KC = a.KC;
    const int slot_bytes = KC * 256;
    const int nk_tiles = (L + 31) >> 5;
    const bool lone_on = a.lone_valu != 0;
    const bool lone_key = lone_on && (L & 31) == 1 && (nk_tiles & 1) && nk_tiles > 1;   // an odd last key tile that holds a single key
    const int n = (a.nheads - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;     // heads of this workgroup
    if (n <= 0) return;
    // wave-uniform scalars, pinned to SGPRs (v_readfirstlane): as VGPRs they were two of the loop invariants the 9-wave variant spilled
    const float inv8 = OUT8 ? __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(448.0f / (2.0f * fmaxf(*a.out_amax, 1e-30f))))) : 1.0f;
    const float next_thr = (OUT8 && a.amax_next != nullptr)       // read once: no global load inside the head loop
                               ? __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(*a.amax_next))) : 0.f;

    // K fragment st of this lane sits at row r, 16-byte chunk (2 st + h2) ^ k_sw, k_sw = (r >> 1) & 7: byte offset
    // kb ^ (32 st) with kb = r * 128 + ((h2 ^ k_sw) << 4) (bits 5-6 of everything else are zero).  ONE register; the XOR is
    // applied to the tile's address inside load_k (4 VALU ops per tile) instead of keeping four loop-invariant offsets live.
    const int kb = r * 128 + ((h2 ^ ((r >> 1) & 7)) << 4);
    const int vi = lane & 15, vg = (lane >> 4) & 1;
    const int v_lane0 = KC * 128 + (4 * h2 + (vi >> 2)) * 64 + (16 * vg + 4 * (vi & 3)) * 2;   // d half 0
    const int v_lane1 = v_lane0 + KC * 64;                                                    // d half 1
    const int q0 = wave * 32;
    int qrow = q0 + r;
    qrow = qrow < L ? qrow : L - 1;

    auto head_base = [&](int bh) {
        const int b = bh / a.H, h = bh - b * a.H;
        return a.qkv + (int64_t)b * L * a.ldq + h * 64;
    };
    // VM-op order per head and wave: [LDS-DMA pieces of head j+1 (top of head j)] ... [4 Q loads of head j+1][NS stores of head j],
    // NS = 4 (bf16 output: dwordx4 after the half-wave swap) or 8 (e4m3 output: dword stores).
    // The wait is vmcnt(NS) at the END of head j, right behind the stores: everything but the NS youngest operations (the
    // stores) has completed, so the stores drain under the next head's MFMAs while its K/V pieces (issued a whole head
    // earlier) and Q rows are known to have landed.  The count is exact because the stores are never predicated (lanes
    // past the last query replicate query L-1 and rewrite its row with identical values) and are inline asm.
    // The Q loads are inline asm too (hipcc would drain the LDS-DMA queue at the first use of an ordinary load); the wait
    // names their registers "+v" in the same basic block, before any loop-carried copy can be made of them.
    // Per-lane parts of the Q-row and output-row addresses as 32-bit BYTE offsets from a wave-uniform (SGPR) base per head
    // (saddr form of the global instructions): two VGPRs instead of two 64-bit pointers kept live across the whole head loop.
    // The launcher guarantees L * ld * 2 < 2^31 for both pitches.
    // They are RE-derived from the lane id at each use (once per head, ~6 VALU ops) behind an opaque asm: as loop invariants hipcc
    // hoisted them out of the head loop and then spilled them in the 9-wave variant (168 VGPRs).
    auto row_offset = [&](int ld, int per_h2, unsigned bytes) {
        unsigned lf = (unsigned)lane;
        asm volatile("" : "+v"(lf));
        int qr = q0 + (int)(lf & 31u);
        qr = qr < L ? qr : L - 1;
        return (unsigned)(qr * ld + per_h2 * (int)(lf >> 5)) * bytes;
    };
    auto load_q = [&](u32x4_t (&q)[4], int bh) {
        const ov_bf16* qb = head_base(bh);                         // wave-uniform
        const unsigned qoff = row_offset((int)a.ldq, 8, 2u);
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(q[0]) : "v"(qoff), "s"(qb) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:32" : "=v"(q[1]) : "v"(qoff), "s"(qb) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:64" : "=v"(q[2]) : "v"(qoff), "s"(qb) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:96" : "=v"(q[3]) : "v"(qoff), "s"(qb) : "memory");
    };
    stage_head(a, blockIdx.x, smem, wave, lane, blockDim.x);
    u32x4_t qn[4];
    load_q(qn, blockIdx.x);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(qn[0]), "+v"(qn[1]), "+v"(qn[2]), "+v"(qn[3]) :: "memory");

    for (int j = 0; j < n; ++j) {
        const int bh = blockIdx.x + j * gridDim.x;
        bf16x8_t qf[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) qf[st] = __builtin_bit_cast(bf16x8_t, qn[st]);
        asm volatile("s_barrier" ::: "memory");   // raw barrier (a __syncthreads fence would drain vmcnt to 0, stores included);
                                                  // the memory clobber keeps every LDS read of head j below it:
                                        // everybody's pieces have landed and everybody has left head j-1
        if (j + 1 < n) stage_head(a, bh + gridDim.x, smem + ((j + 1) & 1) * slot_bytes, wave, lane, blockDim.x);
        const char* ks = smem + (j & 1) * slot_bytes;
        const unsigned ks_u = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)ks;

        float m = -INFINITY, lsum = 0.f;
        f32x16_t o0, o1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
        // Key tiles are consumed two at a time (64 keys: two independent S accumulators, one max / rescale decision,
        // 32 exps) with the K fragments of the NEXT step fetched right behind the S MFMAs, so LDS latency and the
        // MFMA->VALU->MFMA dependency chain of one tile are covered by the other's work; an odd last tile runs alone.
        bf16x8_t kfa[4], kfb[4];
        auto load_k = [&](bf16x8_t (&kf)[4], int kt) {
            const unsigned kp = (unsigned)(kt * 4096 + kb);          // slot bases are multiples of 256: the XOR stays inside the row
#pragma unroll
            for (int st = 0; st < 4; ++st) kf[st] = *(const bf16x8_t*)(ks + (kp ^ (unsigned)(st * 32)));
        };
        const int npair = nk_tiles >> 1;
        load_k(kfa, 0);
        if (DEEP && npair > 0) load_k(kfb, 1);
        for (int it = 0; it < npair; ++it) {
            const int kt = 2 * it;
            const unsigned va0 = ks_u + kt * 2048 + v_lane0, va1 = ks_u + kt * 2048 + v_lane1;
            if (!DEEP) load_k(kfb, kt + 1);                            // second tile's K: covered by the first tile's MFMAs
            u32x2_t vt[8], vu[8];
            // 9+ waves (3 per SIMD: 168 VGPRs): the first tile's V fragments are fetched behind the S MFMAs instead of in front
            // of them -- still a whole softmax ahead of their use, and 16 registers fewer while both K tiles are live (the kernel
            // spilled 10 VGPRs otherwise, which the inline-asm loads and counted waits must not meet: tests/test_build_scratch.py)
            if (DEEP) attn::read_v<0>(vt, va0, va1);
            if (DEEP) attn::read_v<2048>(vu, va0, va1);
            f32x16_t sa, sb;
#pragma unroll
            for (int i = 0; i < 16; ++i) { sa[i] = 0.f; sb[i] = 0.f; }
#pragma unroll
            for (int st = 0; st < 4; ++st) sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfa[st], qf[st], sa, 0, 0, 0);
#pragma unroll
            for (int st = 0; st < 4; ++st) sb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfb[st], qf[st], sb, 0, 0, 0);
            if (!DEEP) attn::read_v<0>(vt, va0, va1);
            if (kt + 2 < nk_tiles) load_k(kfa, kt + 2);                // next step's first tile, fetched under the softmax
            else if (DEEP) asm volatile("s_nop 7" : "+v"(sb));         // last step of an even tile count: nothing else separates the sb
                                                                       // MFMAs from tile_max's inline-asm reads (see attn::tile_max)
            if (DEEP && kt + 3 < nk_tiles) load_k(kfb, kt + 3);
            attn::mask_tail(sb, kt + 1, h2, L);
            const float mx = attn::half_max(fmaxf(attn::tile_max(sa), attn::tile_max(sb)), a.scale_log2);
            OV_ATTN_RESCALE(mx, m, lsum, o0, o1)
            const float nm = -m;
            f32x2_t ps = {0.f, 0.f};
            exp_rows(sa, a.scale_log2, nm, ps);
            exp_rows(sb, a.scale_log2, nm, ps);
            lsum += ps[0] + ps[1];
            const bf16x8_t pa0 = attn::pack_p(sa, 0), pa1 = attn::pack_p(sa, 1), pb0 = attn::pack_p(sb, 0), pb1 = attn::pack_p(sb, 1);
            attn::tr_wait(vt);
            __builtin_amdgcn_sched_barrier(0);
            if (!DEEP) attn::read_v<2048>(vu, va0, va1);   // second tile's V fragments: their LDS latency hides under the first tile's four P.V MFMAs
            attn::pv_mma(vt, pa0, pa1, o0, o1);
            attn::tr_wait(vu);
            __builtin_amdgcn_sched_barrier(0);
            attn::pv_mma(vu, pb0, pb1, o0, o1);
        }
        if (j + 1 < n) load_q(qn, bh + gridDim.x);                   // next head's Q rows, live only across the tail step
        if (lone_key) {
            // L = 32 k + 1 (ViT: patches + cls): the odd last key tile holds ONE key.  A tile step for it is a full dependent
            // chain (LDS -> 4 MFMAs -> softmax on 32 columns -> 4 MFMAs, ~2.3 k cycles per head and wave); the same update on the
            // VALU: the staged rows past L-1 are copies of row L-1, so this lane's own K fragments of the tile ARE that key
            // (its d range), 16 v_dot2 give q.k, then one exp2 and 32 FMAs with the key's V row.
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int st = 0; st < 4; ++st) attn::lone_dot(s0, s1, qf[st], kfa[st]);
            const float sd = attn::lone_sum(s0, s1);
            const char* vrow = ks + KC * 128 + (L - 1) * 64 + 8 * h2;    // the key's V row, d-half 0 (half 1: + KC * 64)
            u32x2_t v0[4];                                              // d-half 0 now, d-half 1 into the same registers afterwards
#pragma unroll
            for (int g = 0; g < 4; ++g) v0[g] = attn::vrow_piece(vrow, g);
            const float mx = sd * a.scale_log2;
            OV_ATTN_RESCALE(mx, m, lsum, o0, o1)
            const float pk = attn::lone_weight(mx, m);
            lsum += attn::count_once(pk, h2);
#pragma unroll
            for (int g = 0; g < 4; ++g) attn::fold4(o0, g, pk, v0[g]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 4; ++g) v0[g] = attn::vrow_piece(vrow + KC * 64, g);
#pragma unroll
            for (int g = 0; g < 4; ++g) attn::fold4(o1, g, pk, v0[g]);
        } else if (nk_tiles & 1) {
            const int kt = nk_tiles - 1;
            // the lane's V-image offset, re-derived behind an opaque asm (see row_offset: not a second live copy of v_lane0)
            unsigned lf = (unsigned)lane;
            asm volatile("" : "+v"(lf));
            const unsigned vif = lf & 15u, vgf = (lf >> 4) & 1u, h2f = lf >> 5;
            const unsigned vl0 = (unsigned)KC * 128u + (4u * h2f + (vif >> 2)) * 64u + (16u * vgf + 4u * (vif & 3u)) * 2u;
            const unsigned va0 = ks_u + kt * 2048 + vl0, va1 = va0 + (unsigned)KC * 64u;
            u32x2_t vt[8];
            attn::read_v<0>(vt, va0, va1);
            f32x16_t sa;
#pragma unroll
            for (int i = 0; i < 16; ++i) sa[i] = 0.f;
#pragma unroll
            for (int st = 0; st < 4; ++st) sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfa[st], qf[st], sa, 0, 0, 0);
            attn::mask_tail(sa, kt, h2, L);
            asm volatile("s_nop 15" : "+v"(sa));                         // a full tile: nothing else in front of attn::tile_max
            const float mx = attn::half_max(attn::tile_max(sa), a.scale_log2);
            OV_ATTN_RESCALE(mx, m, lsum, o0, o1)
            const float nm = -m;
            f32x2_t ps = {0.f, 0.f};
            exp_rows(sa, a.scale_log2, nm, ps);
            lsum += ps[0] + ps[1];
            const bf16x8_t pa0 = attn::pack_p(sa, 0), pa1 = attn::pack_p(sa, 1);
            attn::tr_wait(vt);
            __builtin_amdgcn_sched_barrier(0);
            attn::pv_mma(vt, pa0, pa1, o0, o1);
        }
        const float l = attn::half_sum(lsum);
        float inv = 1.0f / l;
        if (OUT8) {
            if (a.amax_next != nullptr) {          // delayed scaling; the (rare) atomic is issued AHEAD of the 8 stores the vmcnt(8) below counts
                float lm = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) lm = fmaxf(lm, fmaxf(fabsf(o0[i]), fabsf(o1[i])));
                lm *= inv;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) lm = fmaxf(lm, __shfl_xor(lm, o, 64));
                if (lane == 0 && lm > next_thr) atomicMax((unsigned*)a.amax_next, __float_as_uint(lm));
            }
            inv *= inv8;
            const unsigned char* ob = (const unsigned char*)a.out + (int64_t)(bh / a.H) * L * a.ldo + (bh % a.H) * 64;   // uniform
            const unsigned ooff = row_offset((int)a.ldo, 4, 1u);
#define OV_ST8(GQ)                                                                                                         \
            {                                                                                                              \
                const unsigned w0 = pack_fp8x4(o0[4 * GQ] * inv, o0[4 * GQ + 1] * inv, o0[4 * GQ + 2] * inv, o0[4 * GQ + 3] * inv); \
                const unsigned w1 = pack_fp8x4(o1[4 * GQ] * inv, o1[4 * GQ + 1] * inv, o1[4 * GQ + 2] * inv, o1[4 * GQ + 3] * inv); \
                asm volatile("global_store_dword %0, %1, %2 offset:%3" :: "v"(ooff), "v"(w0), "s"(ob), "n"(8 * GQ) : "memory");        \
                asm volatile("global_store_dword %0, %1, %2 offset:%3\n\ts_nop 0" :: "v"(ooff), "v"(w1), "s"(ob), "n"(32 + 8 * GQ) : "memory"); \
            }
            OV_ST8(0) OV_ST8(1) OV_ST8(2) OV_ST8(3)
#undef OV_ST8
        } else {
            // Widened store tail: after packing, a query row is split over the two half-waves (lane r: d 8g..8g+3, lane r+32:
            // d 8g+4..8g+7 of group g).  One half-wave swap (attn::half_swap) per dword and pair of groups (g, g+1) leaves 16 contiguous bytes in
            // every lane (lower half: d 8g..8g+7, upper half: d 8g+8..8g+15): FOUR global_store_dwordx4 per head instead of eight
            // dwordx2 -- the tail is store-issue bound (each row-per-lane store is 64 separate requests), so half the instructions
            // is half the time.
            const ov_bf16* ob = a.out + (int64_t)(bh / a.H) * L * a.ldo + (bh % a.H) * 64;                       // uniform
            const unsigned ooff = row_offset((int)a.ldo, 8, 2u);
#define OV_ST16(O, P, BYTE_OFF)                                                                                              \
            {                                                                                                               \
                const unsigned ax = pack_bf16x2(O[8 * P + 0] * inv, O[8 * P + 1] * inv), ay = pack_bf16x2(O[8 * P + 2] * inv, O[8 * P + 3] * inv); \
                const unsigned bx = pack_bf16x2(O[8 * P + 4] * inv, O[8 * P + 5] * inv), by = pack_bf16x2(O[8 * P + 6] * inv, O[8 * P + 7] * inv); \
                const u32x2_t sx = attn::half_swap(ax, bx);                                                                   \
                const u32x2_t sy = attn::half_swap(ay, by);                                                                   \
                const u32x4_t w = {sx[0], sy[0], sx[1], sy[1]};                                                               \
                /* s_nop 1: a store of more than 8 bytes reads its data VGPRs late -- the next VALU write of them needs 2 wait states, and */ \
                /* the assembler's hazard recogniser does not look inside inline asm */                                      \
                asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3\n\ts_nop 1" :: "v"(ooff), "v"(w), "s"(ob), "n"(BYTE_OFF) : "memory"); \
            }
            OV_ST16(o0, 0, 0) OV_ST16(o0, 1, 32) OV_ST16(o1, 0, 64) OV_ST16(o1, 1, 96)
#undef OV_ST16
        }
        if (LSE && !OUT8) {
            // kept for the backward (ov_attention_backward_saved): m and l are the same in both half-waves, rows past L repeat row
            // L - 1 (clamped Q row): duplicate stores of one value.  One more store behind the four of the output.
            const float v = m + __builtin_amdgcn_logf(l);                                                      // v_log_f32 = log2
            const float* lb = a.lse + (int64_t)bh * KC;                                                         // uniform
            const unsigned loff = row_offset(1, 0, 4u);
            asm volatile("global_store_dword %0, %1, %2" :: "v"(loff), "v"(v), "s"(lb) : "memory");
        }
        // everything but this head's stores (8 dword stores with e4m3 output, 4 dwordx4 stores otherwise, + 1 with LSE) has completed
        if (OUT8) asm volatile("s_waitcnt vmcnt(8)" : "+v"(qn[0]), "+v"(qn[1]), "+v"(qn[2]), "+v"(qn[3]) :: "memory");
        else if (LSE) asm volatile("s_waitcnt vmcnt(5)" : "+v"(qn[0]), "+v"(qn[1]), "+v"(qn[2]), "+v"(qn[3]) :: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" : "+v"(qn[0]), "+v"(qn[1]), "+v"(qn[2]), "+v"(qn[3]) :: "memory");
    }
}

// =====================================================================================================
// Streaming variant for long sequences (padded L > 320; S/8@384: 2305 tokens).  One workgroup = 8 waves = 256 queries of
// one (batch, head); K/V stream through a ring of four 16-KiB LDS slots in 64-key chunks (K image [64][128 B] +
// V image [2 d-halves][64][64 B], same swizzles as above), LDS-DMA'd three chunks ahead.  Per chunk: a counted
// vmcnt (the two younger chunks stay in flight), ONE raw barrier (the chunk has landed for everybody and everybody has
// left the slot about to be refilled), the DMA of chunk c+3, then the two-key-tile step of the persistent kernel.
// <= 128 VGPRs: two workgroups (2 x 64 KiB LDS) = 4 waves per SIMD share a CU, so one wave's softmax VALU work runs
// under another's MFMAs.  Workgroup ids are dealt to XCDs so that the q-blocks of a head share that XCD's L2.
struct AttnSArgs {
    const ov_bf16* qkv; int64_t ldq;
    ov_bf16* out; int64_t ldo;
    int L, H, nqt, nqb, nheads, nchunks;
    float scale_log2;
    const float* out_amax;        // OUT8 (see AttnPArgs)
    float* amax_next;
    int lone_valu;                // 1: a single-key last chunk (L = 64 k + 1) is folded in on the VALU (OVHIP_ATTN_LONEKEY=0: a chunk step)
};

template <bool OUT8>
__global__ __launch_bounds__(512, 4) void attn_fwd_hd64_stream(const AttnSArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    const int L = a.L;
    // XCD-aware work map: workgroup id -> (head, q-block); the q-blocks of a head run back to back on one XCD
    const int wid = blockIdx.x;
    const int xcd = wid & 7, slot_id = wid >> 3;
    const int bh = (slot_id / a.nqb) * 8 + xcd, qb = slot_id % a.nqb;
    if (bh >= a.nheads) return;
    const int b = bh / a.H, h = bh - b * a.H;
    const int HD = a.H * 64;
    const ov_bf16* base = a.qkv + (int64_t)b * L * a.ldq + h * 64;
    const int qt = qb * 8 + wave;
    const bool active = qt < a.nqt;
    int qrow = qt * 32 + r;
    qrow = qrow < L ? qrow : L - 1;

    // ---- staging: thread tid moves one 16-B piece of K and one of V per chunk (32-bit byte offsets from `base`) ----
    // K piece: key tid>>3, source d-chunk (tid&7) ^ ((key>>1)&7) (swizzle on the source side); V piece: d-half tid>>8, key
    // (tid&255)>>2, d-chunk within the half tid&3.
    char* const sdst = smem + wave * 1024;
    const int nc = a.nchunks;
    const char* const bbase = (const char*)base;
    unsigned kofs = (unsigned)(((tid >> 3) * a.ldq + HD + (((tid & 7) ^ ((tid >> 4) & 7)) * 8)) * 2);
    unsigned vofs = (unsigned)(((((tid & 255) >> 2)) * a.ldq + 2 * HD + ((tid >> 8) * 4 + (tid & 3)) * 8) * 2);
    const unsigned cstep = (unsigned)(64 * a.ldq * 2);
    auto stage = [&](int c) {                                     // chunks are staged in order 0, 1, 2, ...
        char* dst = sdst + (c & 3) * 16384;
        unsigned ko = kofs, vo = vofs;
        if (c == nc - 1) {                                        // last chunk: rows past the sequence re-read row L-1 (finite; masked)
            const int t = threadIdx.x;
            const int over_k = c * 64 + (t >> 3) - (L - 1), over_v = c * 64 + ((t & 255) >> 2) - (L - 1);
            if (over_k > 0) ko -= (unsigned)(over_k * a.ldq * 2);
            if (over_v > 0) vo -= (unsigned)(over_v * a.ldq * 2);
        }
        __builtin_amdgcn_global_load_lds((gptr_t)(bbase + ko), (lptr_t)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(bbase + vo), (lptr_t)(dst + 8192), 16, 0, 0);
        kofs += cstep;
        vofs += cstep;
    };
    // Q rows: ordinary loads, waited for by the compiler (once per workgroup).  Not the inline-asm form of the persistent
    // kernel: an asm load's destination can be spilled or copied right behind the asm statement, before the data has landed
    // (seen with a 128-VGPR ping-pong variant of this kernel: the late write then hit live address registers).
    bf16x8_t qf[4];
    {
        const ov_bf16* qp = base + (int64_t)qrow * a.ldq + 8 * h2;
#pragma unroll
        for (int st = 0; st < 4; ++st) qf[st] = *(const bf16x8_t*)(qp + 16 * st);
    }
    stage(0);
    if (nc > 1) stage(1);
    if (nc > 2) stage(2);

    const int k_lane = r * 128;
    const int k_sw = (r >> 1) & 7;
    // fragment st of a key row sits at chunk (2 st + h2) ^ k_sw = (h2 ^ k_sw) ^ 2 st: one base, st by XOR (bits 5-6)
    const int kbase = k_lane + ((h2 ^ k_sw) << 4);
    const int vi = lane & 15, vg = (lane >> 4) & 1;
    const int v_lane0 = 8192 + (4 * h2 + (vi >> 2)) * 64 + (16 * vg + 4 * (vi & 3)) * 2;    // d half 0 (half 1 = + 4096)
    const unsigned smem_u = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)smem;

    float m = -INFINITY, lsum = 0.f;
    f32x16_t o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    // L = 64 k + 1 (every ViT grid of a multiple of 8 plus the class token: 577, 1025, 2305): the last chunk holds ONE key.  It is staged
    // like any other chunk but folded in on the VALU behind the loop (its K / V rows are row 0 of its ring slot), as the persistent
    // kernel does for its single-key tile: a chunk step for it is a whole barrier + 16 MFMAs + 32 exps per lane (2.8 % of the launch at
    // L = 2305).
    const bool lone_key = a.lone_valu != 0 && (L & 63) == 1 && nc > 1;
    const int nc_mfma = lone_key ? nc - 1 : nc;
    for (int c = 0; c < nc_mfma; ++c) {
        if (c + 2 < nc) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (c + 1 < nc) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");
        if (c + 3 < nc) stage(c + 3);
        if (!active) continue;                                    // idle waves of the last q-block still stage and synchronise
        const char* ks = smem + (c & 3) * 16384;
        const unsigned va0 = smem_u + (c & 3) * 16384 + v_lane0, va1 = va0 + 4096;
        // the second tile's K fragments are fetched behind the first tile's MFMAs (register room: 128 VGPRs)
        bf16x8_t kfa[4], kfb[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) kfa[st] = *(const bf16x8_t*)(ks + (kbase ^ (st << 5)));
        f32x16_t sa, sb;
#pragma unroll
        for (int i = 0; i < 16; ++i) { sa[i] = 0.f; sb[i] = 0.f; }
#pragma unroll
        for (int st = 0; st < 4; ++st) sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfa[st], qf[st], sa, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int st = 0; st < 4; ++st) kfb[st] = *(const bf16x8_t*)(ks + 4096 + (kbase ^ (st << 5)));
#pragma unroll
        for (int st = 0; st < 4; ++st) sb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfb[st], qf[st], sb, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        u32x2_t vt[8], vu[8];
        attn::read_v<0>(vt, va0, va1);
        OV_ATTN_MASK_TAIL2(sa, sb, 2 * c, h2, L)                  // last chunk: keys past the sequence
        const float mx = attn::half_max(fmaxf(attn::tile_max(sa), attn::tile_max(sb)), a.scale_log2);
        OV_ATTN_RESCALE(mx, m, lsum, o0, o1)
        const float nm = -m;
        f32x2_t ps = {0.f, 0.f};
        exp_rows(sa, a.scale_log2, nm, ps);
        const bf16x8_t pa0 = attn::pack_p(sa, 0), pa1 = attn::pack_p(sa, 1);     // packed at once: the fp32 tile's registers retire early
        exp_rows(sb, a.scale_log2, nm, ps);
        const bf16x8_t pb0 = attn::pack_p(sb, 0), pb1 = attn::pack_p(sb, 1);
        lsum += ps[0] + ps[1];
        attn::tr_wait(vt);
        __builtin_amdgcn_sched_barrier(0);
        attn::read_v<2048>(vu, va0, va1);
        attn::pv_mma(vt, pa0, pa1, o0, o1);
        attn::tr_wait(vu);
        __builtin_amdgcn_sched_barrier(0);
        attn::pv_mma(vu, pb0, pb1, o0, o1);
    }
    if (lone_key) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the last chunk's two pieces (issued three chunks ago)
        asm volatile("s_barrier" ::: "memory");
    }
    if (!active) return;
    if (lone_key) {
        const char* ks = smem + ((nc - 1) & 3) * 16384;           // key L-1 = row 0 of the slot: K chunk c at byte 16 c, V d-half h at 8192 + 4096 h
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st) attn::lone_dot(s0, s1, qf[st], *(const u32x4_t*)(ks + (2 * st + h2) * 16));
        const float mx = attn::lone_sum(s0, s1) * a.scale_log2;
        OV_ATTN_RESCALE(mx, m, lsum, o0, o1)
        const float pk = attn::lone_weight(mx, m);
        lsum += attn::count_once(pk, h2);
        const char* vrow = ks + 8192 + 8 * h2;                    // d-half 0; half 1 = + 4096
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x2_t v0 = attn::vrow_piece(vrow, g), v1 = attn::vrow_piece(vrow + 4096, g);
            attn::fold4(o0, g, pk, v0);
            attn::fold4(o1, g, pk, v1);
        }
    }
    const float l = attn::half_sum(lsum);
    float inv = 1.0f / l;
    if (OUT8 && a.amax_next != nullptr) {                         // delayed scaling: running maximum of |output| (all lanes take part)
        float lm = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) lm = fmaxf(lm, fmaxf(fabsf(o0[i]), fabsf(o1[i])));
        lm = qt * 32 + r < L ? lm * inv : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lm = fmaxf(lm, __shfl_xor(lm, o, 64));
        if (lane == 0 && lm > *(volatile float*)a.amax_next) atomicMax((unsigned*)a.amax_next, __float_as_uint(lm));
    }
    if (qt * 32 + r < L) {
        if (OUT8) {
            inv *= 448.0f / (2.0f * fmaxf(*a.out_amax, 1e-30f));
            unsigned char* op = (unsigned char*)a.out + ((int64_t)b * L + qrow) * a.ldo + h * 64 + 4 * h2;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                *(unsigned*)(op + 8 * gq) = pack_fp8x4(o0[4 * gq] * inv, o0[4 * gq + 1] * inv, o0[4 * gq + 2] * inv, o0[4 * gq + 3] * inv);
                *(unsigned*)(op + 32 + 8 * gq) = pack_fp8x4(o1[4 * gq] * inv, o1[4 * gq + 1] * inv, o1[4 * gq + 2] * inv, o1[4 * gq + 3] * inv);
            }
        } else {
            ov_bf16* op = a.out + ((int64_t)b * L + qrow) * a.ldo + h * 64 + 4 * h2;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const u32x2_t w0 = {pack_bf16x2(o0[4 * gq] * inv, o0[4 * gq + 1] * inv),
                                    pack_bf16x2(o0[4 * gq + 2] * inv, o0[4 * gq + 3] * inv)};
                const u32x2_t w1 = {pack_bf16x2(o1[4 * gq] * inv, o1[4 * gq + 1] * inv),
                                    pack_bf16x2(o1[4 * gq + 2] * inv, o1[4 * gq + 3] * inv)};
                *(u32x2_t*)(op + 8 * gq) = w0;
                *(u32x2_t*)(op + 32 + 8 * gq) = w1;
            }
        }
    }
}

// =====================================================================================================
// Generic head_dim kernel (head_dim 72 = So400m, 80 = H/14; any multiple of 8 up to 96): same S^T / P^T / O^T scheme with
// the head padded to 96 in LDS (zero columns), 256-key chunks staged through registers, one key tile per step.  A plain,
// correctness-first variant: these model sizes are not on the benchmark configuration.
// MASK (ov_attention_prefix): prefix-causal visibility, key j is visible to query i iff j < a.prefix or j <= i.  A query tile q0 sees
// keys [0, max(prefix, q0 + 32)): key tiles wholly beyond that are never staged-for or computed by its wave, chunks beyond the
// workgroup's last tile are not staged at all; the tiles that straddle the boundary enter the online softmax with -inf scores.  Every
// tile a wave does process has its first key visible to all of its queries (it starts below prefix or at / below q0), so no row's
// running maximum stays -inf.  HDP = 64 serves head_dim 64 under a mask (K rows of 128 B, 16-byte chunks XOR-swizzled by
// (key >> 1) & 7 as in the persistent kernel: the unswizzled 128-B pitch would put the 32 rows of a ds_read_b128 on four banks).
template <int HDP, bool MASK = false>
__global__ __launch_bounds__(640) void attn_fwd_generic(const AttnArgs a, int hd) {
    constexpr bool SWZ = HDP == 64;
    constexpr int KS = HDP / 16;           // k-steps of S^T = K.Q^T
    constexpr int DT = HDP / 32;           // 32-row tiles of O^T
    constexpr int CH = HDP / 8;            // 16-byte chunks per (padded) row
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = nthreads >> 6;
    const int r = lane & 31, h2 = lane >> 5;
    const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
    const int L = a.L, KC = a.KC;
    const int HD = a.H * hd;
    char* ks = smem;                                 // K image: KC rows x HDP*2 bytes
    char* vs = smem + KC * HDP * 2;                  // V image: DT tiles x KC rows x 64 bytes
    const ov_bf16* base = a.qkv + (int64_t)b * L * a.ldq + h * hd;
    const int qt = blockIdx.y * nw + wave;
    const bool active = qt < a.nqt;
    const int q0 = qt * 32;

    bf16x8_t qf[KS];
    {
        int qrow = q0 + r;
        qrow = (active && qrow < L) ? qrow : L - 1;
        const ov_bf16* qp = base + (int64_t)qrow * a.ldq;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int d = 16 * s + 8 * h2;
            u32x4_t w = {0u, 0u, 0u, 0u};
            if (d < hd) w = *(const u32x4_t*)(qp + d);
            qf[s] = __builtin_bit_cast(bf16x8_t, w);
        }
    }
    float m = -INFINITY, lsum = 0.f;
    f32x16_t o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[t][i] = 0.f;
    const int vi = lane & 15, vg = (lane >> 4) & 1;
    const int v_lane_off = (4 * h2 + (vi >> 2)) * 64 + (16 * vg + 4 * (vi & 3)) * 2;

    // MASK: keys this workgroup's last query tile sees (a multiple of 32 or prefix, clipped) / this wave's tile sees
    const int kend_wg = MASK ? min(L, max(a.prefix, min(a.nqt, ((int)blockIdx.y + 1) * nw) * 32)) : L;
    const int kvis = MASK ? min(L, max(a.prefix, q0 + 32)) : L;
    for (int kc0 = 0; kc0 < kend_wg; kc0 += KC) {
        if (kc0) __syncthreads();
        for (int idx = tid; idx < KC * CH; idx += nthreads) {
            const int row = idx / CH, c = idx - row * CH;
            u32x4_t kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
            if (kc0 + row < L && c * 8 < hd) {
                const ov_bf16* p = base + (int64_t)(kc0 + row) * a.ldq + HD + c * 8;
                kv = *(const u32x4_t*)p;
                vv = *(const u32x4_t*)(p + HD);
            }
            *(u32x4_t*)(ks + row * (HDP * 2) + ((SWZ ? c ^ ((row >> 1) & 7) : c) << 4)) = kv;
            *(u32x4_t*)(vs + (c >> 2) * (KC * 64) + row * 64 + (c & 3) * 16) = vv;
        }
        __syncthreads();
        if (!active || kvis <= kc0) continue;
        const int nk = (kvis - kc0) < KC ? (kvis - kc0) : KC;
        // a last key tile that holds ONE key (L = 32 k + 1: 257) is folded in on the VALU behind the tile loop, as in the head_dim 64
        // kernels: a tile step for it is a ninth of the loop at L = 257
        const bool lone_key = (nk & 31) == 1 && nk > 32;
        const int ntile = ((nk + 31) >> 5) - (lone_key ? 1 : 0);
        for (int kt = 0; kt < ntile; ++kt) {
            f32x16_t s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f;
            const char* kp = ks + (kt * 32 + r) * (HDP * 2);
#pragma unroll
            for (int st = 0; st < KS; ++st) {
                const int c = 2 * st + h2;
                const bf16x8_t kf = *(const bf16x8_t*)(kp + ((SWZ ? c ^ ((r >> 1) & 7) : c) << 4));
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[st], s, 0, 0, 0);
            }
            OV_ATTN_MASK_TAIL(s, kt, h2, nk)
            if (MASK && kc0 + kt * 32 + 31 >= a.prefix && kc0 + kt * 32 + 31 > q0) {   // the tile straddles the boundary (wave-uniform)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = kc0 + kt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h2;
                    if (key >= a.prefix && key > q0 + r) s[i] = -INFINITY;
                }
            }
            asm volatile("s_nop 15" : "+v"(s));                          // a full tile: nothing else in front of attn::tile_max
            const float mx = attn::half_max(attn::tile_max(s), a.scale_log2);
            OV_ATTN_RESCALE_ROWS(MASK, mx, m, lsum, o, DT)
            const float nm = -m;
            f32x2_t ps = {0.f, 0.f};
            exp_rows(s, a.scale_log2, nm, ps);
            lsum += ps[0] + ps[1];
            bf16x8_t pf[2];
#pragma unroll
            for (int st = 0; st < 2; ++st) pf[st] = attn::pack_p(s, st);
            const char* vp = vs + kt * 32 * 64 + v_lane_off;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const char* v0 = vp + t * (KC * 64) + st * 16 * 64;
                    o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair(v0, v0 + 8 * 64), pf[st], o[t], 0, 0, 0);
                }
            }
        }
        if (lone_key) {
            const int key = nk - 1;                                   // row of the chunk
            const char* kp = ks + key * (HDP * 2);
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int st = 0; st < KS; ++st) {
                const int c = 2 * st + h2;
                attn::lone_dot(s0, s1, qf[st], *(const u32x4_t*)(kp + ((SWZ ? c ^ ((key >> 1) & 7) : c) << 4)));
            }
            const float sd = attn::lone_sum(s0, s1);
            // MASK: the lone key is visible to this lane's query like any other key (weight exactly 0 otherwise)
            const bool seen = !MASK || kc0 + key < a.prefix || kc0 + key <= q0 + r;
            const float mx = seen ? sd * a.scale_log2 : -INFINITY;
            OV_ATTN_RESCALE_ROWS(MASK, mx, m, lsum, o, DT)
            const float pk = attn::lone_weight(mx, m);
            lsum += attn::count_once(pk, h2);
#pragma unroll
            for (int t = 0; t < DT; ++t) {                            // o[t]: d = 32 t + ...
                const char* vrow = vs + t * (KC * 64) + key * 64 + 8 * h2;
#pragma unroll
                for (int g = 0; g < 4; ++g) attn::fold4(o[t], g, pk, attn::vrow_piece(vrow, g));
            }
        }
    }
    if (!active) return;
    const float l = lsum + __shfl_xor(lsum, 32, 64);      // (as written: through attn::swap_halves the HDP = 64 form came out different)
    const float inv = 1.0f / l;
    const int q = q0 + r;
    if (q < L) {
        ov_bf16* op = a.out + ((int64_t)b * L + q) * a.ldo + h * hd + 4 * h2;
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = t * 32 + 8 * g + 4 * h2;
                if (d < hd) {
                    const u32x2_t w = {pack_bf16x2(o[t][4 * g] * inv, o[t][4 * g + 1] * inv),
                                       pack_bf16x2(o[t][4 * g + 2] * inv, o[t][4 * g + 3] * inv)};
                    *(u32x2_t*)(op + t * 32 + 8 * g) = w;
                }
            }
    }
}

}  // namespace

#include "attention_route.h"

namespace {
const AttnSwitches& attn_switches() {
    static const AttnSwitches s = [] { const char* e = getenv("OVHIP_ATTN_LONEKEY"); return AttnSwitches{(e && e[0] == '0') ? 0 : 1}; }();
    return s;
}

// The instantiations each kernel has; a form = the route's flags as bits.
enum { F_DEEP = 1, F_OUT8 = 2, F_LSE = 4, F_MASK = 8, F_HDP64 = 16 };
const OvKernelForm<AttnPArgs> PERSIST[] = {{0, attn_fwd_hd64_persist<false, false>},          {F_DEEP, attn_fwd_hd64_persist<true, false>},
                                           {F_OUT8, attn_fwd_hd64_persist<false, true>},      {F_DEEP | F_OUT8, attn_fwd_hd64_persist<true, true>},
                                           {F_LSE, attn_fwd_hd64_persist<false, false, true>}, {F_DEEP | F_LSE, attn_fwd_hd64_persist<true, false, true>}};
const OvKernelForm<AttnSArgs> STREAM[] = {{0, attn_fwd_hd64_stream<false>}, {F_OUT8, attn_fwd_hd64_stream<true>}};
const OvKernelForm<AttnArgs, int> GENERIC[] = {{0, attn_fwd_generic<96>}, {F_MASK | F_HDP64, attn_fwd_generic<64, true>}, {F_MASK, attn_fwd_generic<96, true>}};

// The one way into the kernels, for ov_attention and its siblings: the entry points have checked the operands they own (lse,
// out_amax); here the common ones are checked, attn_fwd_route (attention_route.h) decides, and the route is carried out.
// prefix == L: no mask.
int attention_run(const ov_bf16* qkv, int64_t ld_qkv, ov_bf16* out, int64_t ld_out, int B, int L, int H, int hd, float scale, int prefix,
                  const float* out_amax, float* amax_next, float* lse, ov_stream_t stream) {
    if (!qkv || !out || B <= 0 || L <= 0 || H <= 0) return OV_ERR_INVALID;
    if (prefix < 0 || prefix > L) return OV_ERR_INVALID;
    if (hd <= 0 || hd % 8 || hd > 96) return OV_ERR_UNSUPPORTED;
    if (ld_qkv % 8 || ld_out % 8 || ld_qkv < 3 * H * hd || ld_out < H * hd) return OV_ERR_INVALID;
    if (((uintptr_t)qkv | (uintptr_t)out) & 15) return OV_ERR_INVALID;
    ov_attention_route_t r = {};
    const int rc = attn_fwd_route(r, B, L, H, hd, ld_qkv, ld_out, prefix, out_amax != nullptr, lse != nullptr, ov_num_cus(), attn_switches());
    if (rc != OV_OK) return rc;
    static OvPerDeviceOnce once[3];
    const int nqt = (L + 31) / 32;
    const float scale_log2 = scale * 1.4426950408889634f;
    const dim3 grid((unsigned)r.grid_x, (unsigned)r.grid_y), blk((unsigned)(r.waves * 64));
    if (r.fwd_kernel == OV_ATTN_FWD_PERSISTENT) {
        AttnPArgs p;
        p.qkv = qkv; p.ldq = ld_qkv; p.out = out; p.ldo = ld_out;
        p.L = L; p.H = H; p.nqt = nqt; p.KC = r.kc; p.nheads = B * H; p.scale_log2 = scale_log2; p.out_amax = out_amax; p.amax_next = amax_next; p.lse = lse;
        p.lone_valu = r.lone_valu;
        return ov_launch_form(PERSIST, once[0], OV_ATTN_LDS, r.deep * F_DEEP | r.out8 * F_OUT8 | r.lse * F_LSE, grid, blk, r.lds_bytes,
                              (hipStream_t)stream, p);
    }
    if (r.fwd_kernel == OV_ATTN_FWD_STREAMING) {
        AttnSArgs sa;
        sa.qkv = qkv; sa.ldq = ld_qkv; sa.out = out; sa.ldo = ld_out;
        sa.L = L; sa.H = H; sa.nqt = nqt; sa.nqb = (nqt + 7) / 8; sa.nheads = B * H; sa.nchunks = (L + 63) / 64;
        sa.scale_log2 = scale_log2;
        sa.out_amax = out_amax;
        sa.amax_next = amax_next;
        sa.lone_valu = r.lone_valu;
        return ov_launch_form(STREAM, once[1], OV_ATTN_LDS, r.out8 * F_OUT8, grid, blk, r.lds_bytes, (hipStream_t)stream, sa);
    }
    AttnArgs g;
    g.qkv = qkv; g.ldq = ld_qkv; g.out = out; g.ldo = ld_out;
    g.B = B; g.L = L; g.H = H; g.nqt = nqt; g.KC = r.kc;
    g.scale_log2 = scale_log2;
    g.prefix = prefix;
    return ov_launch_form(GENERIC, once[2], OV_ATTN_LDS, r.mask * F_MASK | (r.hdp == 64) * F_HDP64, grid, blk, r.lds_bytes,
                          (hipStream_t)stream, g, hd);
}
}  // namespace

extern "C" int ov_attention(const ov_bf16* qkv, int64_t ld_qkv, ov_bf16* out, int64_t ld_out, int B, int L,
                            int H, int hd, float scale, ov_stream_t stream) {
    return attention_run(qkv, ld_qkv, out, ld_out, B, L, H, hd, scale, L, nullptr, nullptr, nullptr, stream);
}

// ov_attention that also keeps the softmax statistics for ov_attention_backward_saved: lse[B*H][Lp] (Lp = L rounded up to 32) = the
// log-sum-exp of every query row's scaled scores, in log2 units (m + log2 l of the online softmax).  Only for the shapes the resident
// backward kernel takes (the route's keep_lse); OV_ERR_UNSUPPORTED otherwise -- call ov_attention and let the backward recompute.
extern "C" int ov_attention_lse(const ov_bf16* qkv, int64_t ld_qkv, ov_bf16* out, int64_t ld_out, float* lse, int B, int L, int H, int hd,
                                float scale, ov_stream_t stream) {
    if (!lse || ((uintptr_t)lse & 3)) return OV_ERR_INVALID;
    return attention_run(qkv, ld_qkv, out, ld_out, B, L, H, hd, scale, L, nullptr, nullptr, lse, stream);
}

// Same attention, output written as e4m3 bytes out8[B*L, H*64] (ld_out in bytes) with the static scale 2 * (*out_amax) / 448
// (fp8 path: the out-proj GEMM reads it with that scalar scale).  head_dim 64 only; OV_ERR_UNSUPPORTED otherwise.
extern "C" int ov_attention_fp8out(const ov_bf16* qkv, int64_t ld_qkv, unsigned char* out8, int64_t ld_out, int B, int L, int H,
                                   int hd, float scale, const float* out_amax, float* out_amax_next, ov_stream_t stream) {
    if (!out_amax) return OV_ERR_INVALID;
    if (hd != 64) return OV_ERR_UNSUPPORTED;
    return attention_run(qkv, ld_qkv, (ov_bf16*)out8, ld_out, B, L, H, hd, scale, L, out_amax, out_amax_next, nullptr, stream);
}

// Prefix-causal attention (the text decoder's prefix-LM mask; prefix = 0: causal, prefix = L: unmasked = ov_attention itself).
// Every head_dim takes the generic kernel's MASK form: 64 at its own width (HDP = 64), 72 / 80 / ... padded to 96.
extern "C" int ov_attention_prefix(const ov_bf16* qkv, int64_t ld_qkv, ov_bf16* out, int64_t ld_out, int B, int L, int H, int hd, float scale,
                                   int prefix, ov_stream_t stream) {
    return attention_run(qkv, ld_qkv, out, ld_out, B, L, H, hd, scale, prefix, nullptr, nullptr, nullptr, stream);
}

// What the entry points above and those of attention_bwd.hip would launch (ovhip.h); launches nothing.  cus <= 0: the current
// device's CU count.
extern "C" int ov_attention_route(int B, int L, int H, int hd, int64_t ld_qkv, int64_t ld_out, int prefix, int out8, int lse, int cus,
                                  ov_attention_route_t* route) {
    if (!route || B <= 0 || L <= 0 || H <= 0 || prefix > L) return OV_ERR_INVALID;
    if (hd <= 0 || hd % 8 || hd > 96 || (out8 && hd != 64)) return OV_ERR_UNSUPPORTED;
    if (ld_qkv == 0) ld_qkv = (int64_t)3 * H * hd;
    if (ld_out == 0) ld_out = (int64_t)H * hd;
    if (ld_qkv % 8 || ld_out % 8 || ld_qkv < (int64_t)3 * H * hd || ld_out < (int64_t)H * hd) return OV_ERR_INVALID;
    if (prefix < 0) prefix = L;
    ov_attention_route_t r = {};
    int rc = attn_fwd_route(r, B, L, H, hd, ld_qkv, ld_out, prefix, out8 != 0, lse != 0, cus > 0 ? cus : ov_num_cus(), attn_switches());
    if (rc == OV_OK) rc = attn_bwd_route(r, B, L, H, hd, prefix, lse != 0);
    if (rc == OV_OK) *route = r;
    return rc;
}
