// attention_route.h — host only: THE decision of what an attention call launches, as a value (ov_attention_route_t, ovhip.h).
// Pure functions of the shape, the forward's two row pitches, the prefix, what the output is and whether the row log-sum-exp is kept
// or given, the CU count and the process's switches: no HIP calls, no statics, no environment.  attention.hip / attention_bwd.hip
// carry the value out (attention_run / attention_bwd_run), ov_attention_route reports it, the *_workspace_bytes functions read it.
#pragma once
#include "common.h"

// The process's switch, read once (attention.hip: attn_switches; the tests drive it from child processes).
struct AttnSwitches {
    int lone_valu;         // OVHIP_ATTN_LONEKEY=0: a single-key last tile / chunk of the hd 64 kernels takes a tile step instead of the VALU fold
};

constexpr int64_t OV_ATTN_I32 = 0x7fffffffLL;        // 32-bit grids and row offsets
constexpr int OV_ATTN_LDS = 160 * 1024;              // a CU's LDS, and the limit every attention kernel's dynamic LDS is raised to
constexpr int OV_ATTN_BWD_CH = 256;                  // rows per chunk of the streaming backward (attention_bwd.hip: CH)

// Forward.  prefix: 0 .. L (L, as the unmasked entry points pass it: no mask).  Fills the forward half of r.
// OV_ERR_UNSUPPORTED: a combination the entry points do not admit, or a grid beyond 2^31 - 1 workgroups.
static inline int attn_fwd_route(ov_attention_route_t& r, int B, int L, int H, int hd, int64_t ld_qkv, int64_t ld_out, int prefix,
                                 bool out8, bool lse, int cus, const AttnSwitches& sw) {
    const int nqt = (L + 31) / 32, lp = nqt * 32;        // 32-query tiles = waves; the padded sequence
    const int64_t heads = (int64_t)B * H;
    const bool mask = prefix < L;
    // a kept lse: only where the backward reads it, never beside an e4m3 output; the masked form has neither, and a 32-bit grid.x
    if (mask ? (lse || out8 || heads > OV_ATTN_I32) : (lse && (!ov_attn_bwd_resident(hd, L) || out8))) return OV_ERR_UNSUPPORTED;
    // up to 320 (padded) keys a workgroup keeps the whole head in LDS and gives every query tile a wave of its own (<= 10): the head is
    // staged once.  (Generic kernel: 123 KB at 320 x 96; L = 257 used to take two 256-key chunks and a second workgroup for the 257th
    // query row: So400m's attention 8.0 ms per step.)
    r.resident = lp <= 320;
    // the persistent kernel's row offsets are 32-bit: an image spanning 2 GiB of rows or more (a caller's huge row pitch) goes to the
    // generic kernel
    const bool narrow = (int64_t)L * ld_qkv * 2 < OV_ATTN_I32 && (int64_t)L * ld_out * 2 < OV_ATTN_I32;
    r.out8 = out8; r.lse = lse; r.mask = mask; r.grid_y = 1;
    if (!mask && hd == 64 && r.resident && narrow) {
        r.fwd_kernel = OV_ATTN_FWD_PERSISTENT;
        r.deep = nqt <= 8;                                           // 2 waves per SIMD (launch bounds 512, 2), else 3 (640, 3)
        r.kc = lp; r.waves = nqt; r.lds_bytes = 2 * lp * 256;        // K and V of two heads in turn
        int per_cu = OV_ATTN_LDS / r.lds_bytes;                      // workgroups per CU by LDS ...
        const int by_waves = (r.deep ? 8 : 12) / nqt;                // ... and by waves
        if (per_cu > by_waves) per_cu = by_waves;
        if (per_cu < 1) per_cu = 1;
        const int64_t cap = (int64_t)cus * per_cu;
        r.grid_x = (int)(heads < cap ? heads : cap);
        r.lone_valu = sw.lone_valu;
    } else if (!mask && hd == 64 && !r.resident) {
        r.fwd_kernel = OV_ATTN_FWD_STREAMING;
        r.kc = 64; r.waves = 8; r.lds_bytes = 4 * 16384;
        const int64_t nwg = (heads + 7) / 8 * 8 * ((nqt + 7) / 8);   // whole rounds of 8 XCDs (surplus ids exit at once) x 256-query blocks
        if (nwg > OV_ATTN_I32) return OV_ERR_UNSUPPORTED;
        r.grid_x = (int)nwg;
        r.lone_valu = sw.lone_valu;
    } else {
        // Generic padded-head kernel: head_dim 72 (So400m) / 80 (H/14), head_dim 64 images beyond the persistent kernel's 2 GiB, and
        // every masked call (64 at its own width, the others padded to 96).  No kept lse, no e4m3 epilogue.  Longer sequences:
        // 256-key chunks, 8 waves
        if (lse || out8) return OV_ERR_UNSUPPORTED;
        r.fwd_kernel = OV_ATTN_FWD_GENERIC;
        r.hdp = mask && hd == 64 ? 64 : 96;
        r.kc = r.resident ? lp : 256; r.waves = r.resident ? nqt : 8;
        r.lds_bytes = r.kc * r.hdp * 4;                              // K (KC x 2 hdp B) + V (hdp / 32 x KC x 64 B)
        r.grid_x = (int)heads; r.grid_y = (nqt + r.waves - 1) / r.waves;
        r.lone_valu = 1;
    }
    return OV_OK;
}

// Backward.  saved: the call passes the forward's lse.  Fills the backward half of r, keep_lse included: the training forward keeps
// the lse exactly where this says the backward reads it.  OV_ERR_UNSUPPORTED: a grid beyond 2^31 - 1 workgroups.
static inline int attn_bwd_route(ov_attention_route_t& r, int B, int L, int H, int hd, int prefix, bool saved) {
    const int64_t heads = (int64_t)B * H;
    const bool mask = prefix < L;
    r.keep_lse = !mask && ov_attn_bwd_resident(hd, L);               // the masked backward always streams (row lse and delta in the workspace)
    if (r.keep_lse) {                                                // Q, K, V, dO of a head resident in LDS
        r.bwd_kernel = OV_ATTN_BWD_RESIDENT;
        r.bwd_saved = saved;
        r.bwd_kc = (L + 31) / 32 * 32; r.bwd_waves = r.bwd_kc / 32;
        r.bwd_lds_bytes = 4 * r.bwd_kc * 128 + 2 * r.bwd_kc * (int)sizeof(float);
        if (heads > OV_ATTN_I32) return OV_ERR_UNSUPPORTED;
        r.bwd_grid = (int)heads;
        return OV_OK;
    }
    const int64_t nblk = (L + OV_ATTN_BWD_CH - 1) / OV_ATTN_BWD_CH;
    r.bwd_kernel = OV_ATTN_BWD_STREAMING;
    r.bwd_mask = mask; r.ndh = hd <= 64 ? 2 : 3;
    r.bwd_kc = OV_ATTN_BWD_CH; r.bwd_waves = 8;
    r.bwd_lds_bytes = 2 * r.ndh * OV_ATTN_BWD_CH * 64 + 2 * OV_ATTN_BWD_CH * (int)sizeof(float);     // two chunk images + lse and delta rows
    r.bwd_workspace_bytes = (size_t)2 * heads * nblk * OV_ATTN_BWD_CH * sizeof(float);
    if (heads > OV_ATTN_I32 || heads * nblk > OV_ATTN_I32) return OV_ERR_UNSUPPORTED;
    r.bwd_grid = (int)(heads * nblk);
    return OV_OK;
}
