// tower.hip — host-side launch sequences: the resblock loop and the two encoders (no device code here).
//
//   ov_tower_forward        Transformer.forward / ResidualAttentionBlock.forward   open_clip/transformer.py:355-366, 254-265
//   ov_vision_embed         conv1 + cls + pos-emb (ln_pre = Identity)              transformer.py:610-620
//   ov_vision_head_forward  _global_pool -> ln_post -> @ proj (-> F.normalize)     transformer.py:638-646, model.py:267
//   ov_encode_image         VisionTransformer.forward                              transformer.py:609-651
//   ov_vision_embed_keep / ov_encode_image_keep   the same with patch dropout: K kept patches per image, L' = 1 + K  transformer.py:619,60-86
//   ov_encode_text          CLIP.encode_text                                       model.py:269-284
//
// Per block, seven launches on the caller's stream (all asynchronous, nothing allocated):
//   LN1 -> QKV GEMM(+bias) -> attention -> out-proj GEMM(+bias +residual, in place)
//   LN2 -> FC GEMM(+bias +GELU) -> proj GEMM(+bias +residual, in place)
// An encoder's last block computes only what its pooling head reads: the image tower (avg pool) stops after c_fc and pools in front of
// c_proj (encode_image); the text tower stops after the attention, and the text tail is run_block from past the attention on B rows.
// Workspaces, each laid out by one function below, regions in order, every region 256-byte aligned (M = B L rows):
//   tower_ws       h [M, D] | big [M, big_pitch] (qkv and the MLP hidden alias) | stats [M, 2] fp32 | parts [M, D / 32, 2] fp32 |
//                  fp8 towers only: q8 [M, max(D, mlp_pad)] e4m3 | qs [M] fp32
//   embed_ws       im2col rows [B n, kpad] | keep form only: their pos-emb rows [B K, D]
//   head_ws        pooled rows [B, D] (fp32 image, bf16 text) | ln rows [B, D] | projected rows [B, embed_pad]
//   vision_ws / text_ws   x [M, D] | tower (image: embed_ws aliases it until the blocks run) | head
//   text_tail_ws   inside the tower's big region, past the last attention: a [B, D] | n [B, D] | hid [B, mlp_pad] | stats [B, 2] fp32
#include "common.h"
#include <new>
#include <vector>
#include <mutex>
#include <stdlib.h>

// Side stream for the "tail" images of a batch (tile-quantisation fix, see ov_tower_forward): owned by the tower, created on the
// device that is current at the first forward that needs it; a forward on another device does not split.
struct TailCtx {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    int state = 0;                         // 0 = not created, 1 = ok, -1 = unavailable
    int device = -1;
    std::mutex mu;                         // held from fork to join: two host threads on one tower must not interleave them
};

struct ov_tower {
    mutable TailCtx tail;
    ov_tower_cfg cfg;
    ov_block_weights* blocks;
    unsigned char* set;
    ov_block_fp8* fp8;            // optional fp8 copies (config #5); the fp8 path runs when every layer has one
    unsigned char* set8;
    float* h_amax;                // fp8 path: [4 * layers]: scales' maxima (hidden | attention out) and the running ones (device, borrowed)
    int h_mode;
    unsigned char* mask8;         // fp8 path: per layer, which of the four GEMMs take e4m3 operands (OV_FP8_QKV | _OUT | _FC | _PROJ)
    int prefix;                   // attention mask of every block: -1 = none, >= 0 = ov_attention_prefix's prefix (ov_tower_set_prefix)
    // drop path (ov_tower_set_drop_path): device idx / slot [layers][2][drop_B] and the scratch are borrowed, count [layers][2] and
    // scale [layers] are the tower's own copies; drop_idx == NULL = no table
    const int *drop_idx, *drop_slot;
    int* drop_count;
    float* drop_scale;
    int drop_B;
    char* drop_ws;
    size_t drop_ws_bytes;
};

// Row pitch (elements) of the workspace's `big` region (qkv / MLP hidden).  max(3 D, mlp_pad) is a power-of-two number of bytes for
// the usual widths (L/14: 8 KiB), and the 256 rows of a GEMM operand piece then start 8 KiB apart: OVHIP_BIG_PAD elements (a multiple
// of 64 = one 128-byte line; default 64) are added to the pitch to spread them over the memory channels (L/14 step 45.09 -> 44.85 ms).
static inline int big_pitch(const ov_tower_cfg& c) {
    static int pad = -1;
    if (pad < 0) { const char* e = getenv("OVHIP_BIG_PAD"); pad = e ? atoi(e) : 64; if (pad < 0 || pad % 64) pad = 64; }
    return (3 * c.width > c.mlp_pad ? 3 * c.width : c.mlp_pad) + pad;
}

// OVHIP_ROWPARTS=1: LayerNorm row statistics from the residual GEMMs' epilogues (ov_gemm_rowparts + ov_rowstats_finalize) instead of a
// pass over the residual stream in front of every folded GEMM.  OFF by default: on the L/14 step the row passes shrink from 1.61 to
// 0.59 ms and the two residual GEMM classes grow by 0.57 ms, but the step moves by 0.1 ms only (44.58 against 44.66 ms, alternating
// runs) -- the memory-bound row passes were pauses in which the power-bound chip recovered clock for the next GEMM -- and the default
// keeps the two-pass statistics.
static inline bool use_rowparts() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("OVHIP_ROWPARTS"); v = (e && e[0] == '1') ? 1 : 0; }
    return v != 0;
}

namespace {
// ---- optional in-situ kernel timing (HIP events on the caller's stream; off by default) -----------------
struct ProfRec { int cls; hipEvent_t e0, e1; int64_t rows; };
struct Profiler {
    std::mutex mu;
    unsigned mask = 0;
    int device = -1;                   // the device the event pool belongs to: launches on other devices are not recorded
    std::vector<hipEvent_t> pool;      // unused events
    std::vector<ProfRec> recs;
} g_prof;

struct ProfScope {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st;
    int cls;
    int64_t rows;
    bool on = false;
    ProfScope(int c, ov_stream_t s, int64_t r) : st((hipStream_t)s), cls(c), rows(r) {
        if (!(g_prof.mask & (1u << c))) return;
        std::lock_guard<std::mutex> lk(g_prof.mu);
        if (g_prof.pool.size() < 2 || g_prof.device != ov_current_device()) return;
        e0 = g_prof.pool.back(); g_prof.pool.pop_back();
        e1 = g_prof.pool.back(); g_prof.pool.pop_back();
        on = true;
        (void)hipEventRecord(e0, st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(e1, st);
        std::lock_guard<std::mutex> lk(g_prof.mu);
        g_prof.recs.push_back({cls, e0, e1, rows});
    }
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int max_i(int a, int b) { return a > b ? a : b; }

}  // namespace

extern "C" int ov_abi_version(void) { return OV_ABI_VERSION; }

extern "C" const char* ov_error_string(int status) {
    switch (status) {
        case OV_OK: return "ok";
        case OV_ERR_INVALID: return "invalid argument";
        case OV_ERR_UNSUPPORTED: return "shape/dtype not supported by the gfx950 kernels";
        case OV_ERR_WORKSPACE: return "workspace too small";
        case OV_ERR_NO_DEVICE: return "no gfx950 (MI355X) device visible";
        default: break;
    }
    if (status <= OV_ERR_HIP) return hipGetErrorString((hipError_t)(OV_ERR_HIP - status));
    return "unknown error";
}

extern "C" int ov_device_check(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return OV_ERR_HIP - (int)e;
    if (n <= 0) return OV_ERR_NO_DEVICE;
    int dev = 0;
    e = hipGetDevice(&dev);
    if (e != hipSuccess) return OV_ERR_HIP - (int)e;
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return OV_ERR_HIP - (int)e;
    const char* arch = p.gcnArchName;
    if (!(arch[0] == 'g' && arch[1] == 'f' && arch[2] == 'x' && arch[3] == '9' && arch[4] == '5' && arch[5] == '0'))
        return OV_ERR_NO_DEVICE;
    return OV_OK;
}

extern "C" int ov_profile_enable(unsigned class_mask, int max_records) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (auto& r : g_prof.recs) { g_prof.pool.push_back(r.e0); g_prof.pool.push_back(r.e1); }
    g_prof.recs.clear();
    g_prof.mask = class_mask;
    if (max_records < 0) return OV_ERR_INVALID;
    const int dev = ov_current_device();
    if (g_prof.device != dev) {                       // events are per device: a pool made elsewhere is dropped
        for (hipEvent_t e : g_prof.pool) (void)hipEventDestroy(e);
        g_prof.pool.clear();
        g_prof.device = dev;
    }
    while ((int)g_prof.pool.size() < 2 * max_records) {
        hipEvent_t e;
        hipError_t err = hipEventCreate(&e);
        if (err != hipSuccess) return OV_ERR_HIP - (int)err;
        g_prof.pool.push_back(e);
    }
    return OV_OK;
}

extern "C" int ov_profile_read(int cls, double* total_ms, int* count, double* total_rows) {
    if (!total_ms || !count) return OV_ERR_INVALID;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    double tot = 0.0, rows = 0.0;
    int n = 0;
    for (auto& r : g_prof.recs) {
        if (r.cls != cls) continue;
        hipError_t err = hipEventSynchronize(r.e1);
        if (err != hipSuccess) return OV_ERR_HIP - (int)err;
        float ms = 0.f;
        err = hipEventElapsedTime(&ms, r.e0, r.e1);
        if (err != hipSuccess) return OV_ERR_HIP - (int)err;
        tot += ms;
        rows += (double)r.rows;
        ++n;
    }
    *total_ms = tot;
    *count = n;
    if (total_rows) *total_rows = rows;
    return OV_OK;
}

extern "C" ov_tower* ov_tower_create(const ov_tower_cfg* cfg) {
    if (!cfg || cfg->width <= 0 || cfg->layers <= 0 || cfg->heads <= 0 || cfg->mlp <= 0) return nullptr;
    if (cfg->width % cfg->heads || cfg->width % 64 || cfg->mlp_pad % 64 || cfg->mlp_pad < cfg->mlp) return nullptr;
    ov_tower* t = new (std::nothrow) ov_tower;
    if (!t) return nullptr;
    t->cfg = *cfg;
    t->h_amax = nullptr;
    t->h_mode = 0;
    t->prefix = -1;
    t->drop_idx = t->drop_slot = nullptr;
    t->drop_B = 0;
    t->drop_ws = nullptr;
    t->drop_ws_bytes = 0;
    t->drop_count = new (std::nothrow) int[2 * cfg->layers]();
    t->drop_scale = new (std::nothrow) float[cfg->layers]();
    t->blocks = new (std::nothrow) ov_block_weights[cfg->layers]();
    t->set = new (std::nothrow) unsigned char[cfg->layers]();
    t->fp8 = new (std::nothrow) ov_block_fp8[cfg->layers]();
    t->set8 = new (std::nothrow) unsigned char[cfg->layers]();
    t->mask8 = new (std::nothrow) unsigned char[cfg->layers];
    if (!t->blocks || !t->set || !t->fp8 || !t->set8 || !t->mask8 || !t->drop_count || !t->drop_scale) { ov_tower_destroy(t); return nullptr; }
    for (int i = 0; i < cfg->layers; ++i) t->mask8[i] = OV_FP8_ALL;
    return t;
}

extern "C" void ov_tower_destroy(ov_tower* t) {
    if (!t) return;
    if (t->tail.state == 1) {
        (void)hipEventDestroy(t->tail.fork);
        (void)hipEventDestroy(t->tail.join);
        (void)hipStreamDestroy(t->tail.stream);
    }
    delete[] t->blocks;
    delete[] t->set;
    delete[] t->fp8;
    delete[] t->mask8;
    delete[] t->set8;
    delete[] t->drop_count;
    delete[] t->drop_scale;
    delete t;
}

extern "C" int ov_tower_set_block(ov_tower* t, int layer, const ov_block_weights* w) {
    if (!t || !w || layer < 0 || layer >= t->cfg.layers) return OV_ERR_INVALID;
    const void* p[] = {w->ln1_w, w->ln1_b, w->qkv_w, w->qkv_b, w->out_w, w->out_b, w->ln2_w, w->ln2_b,
                       w->fc_w, w->fc_b, w->proj_w, w->proj_b};
    for (const void* q : p)
        if (!q || ((uintptr_t)q & 15)) return OV_ERR_INVALID;
    if ((w->qkv_colsum == nullptr) != (w->fc_colsum == nullptr)) return OV_ERR_INVALID;
    if (((uintptr_t)w->qkv_colsum | (uintptr_t)w->fc_colsum) & 15) return OV_ERR_INVALID;
    t->blocks[layer] = *w;
    t->set[layer] = 1;
    return OV_OK;
}

namespace {
bool tower_fp8(const ov_tower* t) {
    for (int i = 0; i < t->cfg.layers; ++i)
        if (!t->set8[i]) return false;
    return true;
}
}  // namespace

extern "C" int ov_tower_set_block_fp8(ov_tower* t, int layer, const ov_block_fp8* q) {
    if (!t || layer < 0 || layer >= t->cfg.layers) return OV_ERR_INVALID;
    if (!q) { t->set8[layer] = 0; return OV_OK; }                 // NULL clears: back to the bf16 path
    const int D = t->cfg.width, F = t->cfg.mlp_pad;
    if (D % 128 || F % 128 || D < 384 || F < 384) return OV_ERR_UNSUPPORTED;      // K-tiles of 128 fp8 elements, at least three
    const void* p[] = {q->qkv_w8, q->qkv_s, q->qkv_b, q->out_w8, q->out_s, q->fc_w8, q->fc_s, q->fc_b, q->proj_w8, q->proj_s};
    for (const void* v : p)
        if (!v || ((uintptr_t)v & 15)) return OV_ERR_INVALID;
    t->fp8[layer] = *q;
    t->set8[layer] = 1;
    return OV_OK;
}

extern "C" int ov_tower_set_fp8_hidden_scale(ov_tower* t, float* h_amax, int mode) {
    if (!t || mode < 0 || mode > 3 || (mode > 0 && !h_amax)) return OV_ERR_INVALID;
    t->h_amax = h_amax;
    t->h_mode = mode;
    return OV_OK;
}

extern "C" int ov_tower_set_fp8_mask(ov_tower* t, const unsigned char* mask, int n) {
    if (!t || (mask && n != t->cfg.layers)) return OV_ERR_INVALID;
    for (int i = 0; i < t->cfg.layers; ++i) {
        const unsigned char m = mask ? mask[i] : (unsigned char)OV_FP8_ALL;
        if (m & ~OV_FP8_ALL) return OV_ERR_INVALID;
        t->mask8[i] = m;
    }
    return OV_OK;
}

extern "C" int ov_tower_set_prefix(ov_tower* t, int prefix) {
    if (!t || prefix < -1) return OV_ERR_INVALID;
    t->prefix = prefix;
    return OV_OK;
}

extern "C" int ov_tower_set_drop_path(ov_tower* t, const int* idx, const int* slot, const int* count, const float* scale, int B,
                                      void* scratch, size_t scratch_bytes) {
    if (!t) return OV_ERR_INVALID;
    if (!idx) {                                                   // NULL clears: back to today's launches
        t->drop_idx = t->drop_slot = nullptr;
        t->drop_B = 0;
        t->drop_ws = nullptr;
        t->drop_ws_bytes = 0;
        return OV_OK;
    }
    if (!slot || !count || !scale || !scratch || B <= 0) return OV_ERR_INVALID;
    if (B > 65535) return OV_ERR_UNSUPPORTED;                     // the sample is the glue kernels' grid.y
    if ((((uintptr_t)idx | (uintptr_t)slot) & 3) || ((uintptr_t)scratch & 15)) return OV_ERR_INVALID;
    for (int i = 0; i < t->cfg.layers; ++i) {
        if (!(scale[i] > 0.0f) || !(scale[i] <= 3.0e38f)) return OV_ERR_INVALID;
        if (count[2 * i] < 0 || count[2 * i] > B || count[2 * i + 1] < 0 || count[2 * i + 1] > B) return OV_ERR_INVALID;
    }
    for (int i = 0; i < t->cfg.layers; ++i) {
        t->drop_count[2 * i] = count[2 * i];
        t->drop_count[2 * i + 1] = count[2 * i + 1];
        t->drop_scale[i] = scale[i];
    }
    t->drop_idx = idx;
    t->drop_slot = slot;
    t->drop_B = B;
    t->drop_ws = (char*)scratch;
    t->drop_ws_bytes = scratch_bytes;
    return OV_OK;
}

extern "C" size_t ov_tower_drop_path_workspace_bytes(const ov_tower* t, int B, int L) {
    if (!t || B <= 0 || L <= 0) return 0;
    return block_drop_plan(&t->cfg, B, L, nullptr, nullptr);
}

namespace {
// ---- workspace layouts (regions: see the head of the file): every inference workspace is sized and carved here, and nowhere else ------
struct Carver {                                 // hands out consecutive 256-byte aligned regions; a braced list evaluates left to right
    size_t off = 0;
    size_t take(size_t bytes) { const size_t at = off; off += align_up(bytes, 256); return at; }
};

// ldb: row pitch of big; qw: row pitch of q8.  stats: {mean, rstd} per row (LN fold); parts: ov_rowparts layout (OVHIP_ROWPARTS).
struct TowerWs { size_t h, big, stats, parts, q8, qs, total; int ldb, qw; bool fp8; };
TowerWs tower_ws(const ov_tower* t, int B, int L) {
    const size_t M = (size_t)B * L, D = t->cfg.width;
    const int ldb = big_pitch(t->cfg), qw = max_i(t->cfg.width, t->cfg.mlp_pad);
    const bool fp8 = tower_fp8(t);
    Carver c;
    return {c.take(M * D * 2), c.take(M * ldb * 2), c.take(M * 8), c.take(M * (D / 32) * 8), c.take(fp8 ? M * qw : 0), c.take(fp8 ? M * 4 : 0),
            c.off, ldb, qw, fp8};
}

// K = 0: all G patches (ov_vision_embed); K >= 1: the K kept ones and their pos-emb rows at posk (ov_vision_embed_keep)
struct EmbedWs { size_t posk, total; };
EmbedWs embed_ws(const ov_tower* t, const ov_vision_head* h, int B, int K) {
    const int g = h->image_size / h->patch_size;
    const size_t cols = (size_t)B * (K ? K : g * g) * h->kpad * 2, posk = align_up(cols, 256);
    return K ? EmbedWs{posk, posk + (size_t)B * K * t->cfg.width * 2} : EmbedWs{cols, cols};
}

struct HeadWs { size_t rows, ln, feat, total; };             // row_bytes per pooled element: 4 (fp32, image) or 2 (bf16, text)
HeadWs head_ws(int B, int D, int EP, int row_bytes) {
    Carver c;
    HeadWs w = {c.take((size_t)B * D * row_bytes), c.take((size_t)B * D * 2), c.take((size_t)B * EP * 2), 0};
    w.total = w.feat + (size_t)B * EP * 2;
    return w;
}
inline int text_embed_pad(const ov_text_head* h) { return (h->embed_dim + 7) / 8 * 8; }
HeadWs text_head_ws(const ov_tower* t, const ov_text_head* h, int B) { return head_ws(B, t->cfg.width, text_embed_pad(h), 2); }

// Image encoder, plain (K = 0, L = G + 1) or keeping K patches (L = K + 1): the embedding's buffers alias the tower region, which nothing
// uses until the blocks run.
struct EncoderWs { size_t x, tower, head, total; };
EncoderWs encoder_ws(size_t x_bytes, size_t tower_bytes, const HeadWs& head) {
    Carver c;
    return {c.take(x_bytes), c.take(tower_bytes), c.take(head.total), c.off};
}
EncoderWs vision_ws(const ov_tower* t, const ov_vision_head* h, int B, int K) {
    const int g = h->image_size / h->patch_size, L = (K ? K : g * g) + 1, D = t->cfg.width;
    const size_t tower = tower_ws(t, B, L).total, embed = embed_ws(t, h, B, K).total;
    return encoder_ws((size_t)B * L * D * 2, tower > embed ? tower : embed, head_ws(B, D, h->embed_pad, 4));
}
// 'argmax' pooling alone: the pooled position of each caption, int32 [B], behind the head's buffers (idx = the old total)
struct TextWs { size_t x, tower, head, idx, total; };
TextWs text_ws(const ov_tower* t, const ov_text_head* h, int B) {
    const int T = h->context_length;
    const EncoderWs e = encoder_ws((size_t)B * T * t->cfg.width * 2, tower_ws(t, B, T).total, text_head_ws(t, h, B));
    return {e.x, e.tower, e.head, e.total, e.total + (h->pool_last == OV_TEXT_POOL_ARGMAX ? align_up((size_t)B * sizeof(int), 256) : 0)};
}

// The text tail's buffers (ov_encode_text) in the tower's big region, free once the last attention has read qkv: a holds the gathered
// attention rows, then the LN2 rows; n is spare (counted so that the same shapes fit as when the LN2 rows had a region of their own);
// hid is the MLP hidden at pitch mlp_pad.
struct TextTailWs { size_t a, n, hid, stats, total; };
TextTailWs text_tail_ws(const ov_tower_cfg& c, int B) {
    Carver cv;
    TextTailWs w = {cv.take((size_t)B * c.width * 2), cv.take((size_t)B * c.width * 2), cv.take((size_t)B * c.mlp_pad * 2), cv.off, 0};
    w.total = w.stats + (size_t)B * 8;
    return w;
}
inline bool text_tail_fits(const TextTailWs& tail, const TowerWs& w) { return tail.total <= w.stats - w.big; }
}  // namespace

extern "C" size_t ov_tower_workspace_bytes(const ov_tower* t, int B, int L) {
    if (!t || B <= 0 || L <= 0) return 0;
    return tower_ws(t, B, L).total;
}

namespace {
// One part of the batch (the main part on the caller's stream, or the tail images on the side stream): its rows of the token stream
// and of every workspace region.  ldb: the row pitch of `big`; `parts` (or NULL): partial sums of x's row statistics (NULL under fp8);
// q8 / qs: the fp8 activation buffer and its row scales (fp8 towers, else NULL).  prof = record in-situ timings for these launches.
struct BlockPart { ov_bf16 *x, *h, *big; int ldb; float *stats, *parts; unsigned char* q8; float* qs; int B; ov_stream_t stream; bool prof; };
// B images from token row `row` on: their rows of x and of every region of the tower workspace ws laid out by w
BlockPart tower_part(const ov_tower_cfg& c, const TowerWs& w, char* ws, ov_bf16* x, int64_t row, int B, bool parts, ov_stream_t stream,
                     bool prof) {
    const int D = c.width;
    return {x + row * D, (ov_bf16*)(ws + w.h) + row * D, (ov_bf16*)(ws + w.big) + row * w.ldb, w.ldb, (float*)(ws + w.stats) + 2 * row,
            parts ? (float*)(ws + w.parts) + 2 * row * (D / 32) : nullptr, w.fp8 ? (unsigned char*)(ws + w.q8) + row * w.qw : nullptr,
            w.fp8 ? (float*)(ws + w.qs) + row : nullptr, B, stream, prof};
}
// fp8 path: one layer's scale maxima (MLP hidden | attention out), the running ones, and the tower's h_mode (0 = none set)
struct Fp8Scales { float *h_amax, *a_amax, *h_next, *a_next; int h_mode; };

// One ResidualAttentionBlock on rows [0, B*L) of p.x (in place).  parts_in: p.parts describe x on entry (left by the previous block's
// c_proj); they always describe x on exit.  Per GEMM: fp8 (e4m3) operands where `mask` names it (q != NULL; BASELINE.json config #5;
// OV_FP8_ALL = all four), else the LayerNorm folded into the QKV / c_fc epilogue where the weights carry the fold, else the plain GEMM
// -- so mask 0 is the bf16 block.  In front of an fp8 QKV / c_fc the LayerNorm is fused with the row quantisation; in front of an fp8
// out_proj / c_proj the attention output / MLP hidden is written as e4m3 by its producer where that producer has a static scale
// (h_mode >= 2: attention epilogue for head_dim 64, an fp8 c_fc's epilogue) and re-quantised row by row otherwise.
// span (anything but the whole block: bf16 blocks only, mask 0): the part of the launch sequence that runs.  It ends at the block's end,
// past the attention (its output in p.h, x untouched) or past c_fc (x = the stream after out-proj, the MLP hidden in p.big) -- a block
// whose token output nobody reads -- and starts at the block's start or past the attention (p.h holds the attention output of x's rows).
enum BlockPoint { BLOCK_START = 0, BLOCK_PAST_ATTN = 1, BLOCK_PAST_FC = 2, BLOCK_END = 3 };
struct BlockSpan { int from, to; };
constexpr BlockSpan BLOCK_FULL = {BLOCK_START, BLOCK_END};
int run_block(const ov_tower_cfg& c, const ov_block_weights& w, const ov_block_fp8* q, int mask, const Fp8Scales& sc, const BlockPart& p,
              bool parts_in, int L, int prefix, BlockSpan span = BLOCK_FULL) {
    const int D = c.width, H = c.heads, hd = D / H, F = c.mlp_pad, B = p.B;
    const int64_t M = (int64_t)B * L;
    const int ldb = p.ldb;                                      // row pitch of `big` (shared by qkv and the MLP hidden)
    const float scale = 1.0f / sqrtf((float)hd);
    const int gelu = c.gelu_tanh ? OV_EPI_BIAS_GELU_TANH : OV_EPI_BIAS_GELU_ERF;
    const int fc_cls = c.gelu_tanh ? OV_PROF_GEMM_FC_TANH : OV_PROF_GEMM_FC;
    const bool fold = w.qkv_colsum != nullptr && w.fc_colsum != nullptr;   // LN folded into the QKV / c_fc epilogues
    const bool rp = fold && p.parts != nullptr;                 // statistics ride on the residual GEMMs' epilogues
    const bool f_qkv = mask & OV_FP8_QKV, f_out = mask & OV_FP8_OUT, f_fc = mask & OV_FP8_FC, f_proj = mask & OV_FP8_PROJ;
    ov_bf16 *x = p.x, *h = p.h, *big = p.big;
    float *stats = p.stats, *parts = p.parts, *qs = p.qs;
    unsigned char* q8 = p.q8;
    ov_stream_t stream = p.stream;
    int rc;
#define OV_STEP(cls, call)                                             \
    do {                                                               \
        if (p.prof) { ProfScope ps__(cls, stream, M); rc = (call); }   \
        else rc = (call);                                              \
        if (rc) return rc;                                             \
    } while (0)
    // ---- attention half ----
    const bool from_attn = span.from == BLOCK_PAST_ATTN;        // p.h holds the attention output: nothing launches up to it
    if (from_attn) {
    } else if (f_qkv) {
        OV_STEP(OV_PROF_LN, ov_layernorm_quant_fp8(x, D, w.ln1_w, w.ln1_b, q8, D, qs, M, D, c.ln_eps, stream));
        OV_STEP(OV_PROF_GEMM_QKV, ov_gemm_fp8(q8, D, q->qkv_w8, D, qs, q->qkv_s, q->qkv_b, big, ldb, M, 3 * D, D, OV_EPI_BIAS, nullptr, 0, stream));
    } else if (fold) {
        if (rp && parts_in) OV_STEP(OV_PROF_LN, ov_rowstats_finalize(parts, stats, M, D, c.ln_eps, stream));
        else OV_STEP(OV_PROF_LN, ov_rowstats(x, D, stats, M, D, c.ln_eps, stream));
        OV_STEP(OV_PROF_GEMM_QKV, ov_gemm_ln(x, D, w.qkv_w, D, w.qkv_b, w.qkv_colsum, stats, big, ldb, M, 3 * D, D, OV_EPI_BIAS, stream));
    } else {
        OV_STEP(OV_PROF_LN, ov_layernorm(x, OV_BF16, D, w.ln1_w, w.ln1_b, h, OV_BF16, D, M, D, c.ln_eps, stream));
        OV_STEP(OV_PROF_GEMM_QKV, ov_gemm(h, D, w.qkv_w, D, w.qkv_b, big, ldb, M, 3 * D, D, OV_EPI_BIAS, nullptr, 0, 0, 0, 0, stream));
    }
    if (f_out && sc.h_mode >= 2 && hd == 64) {
        // static scale: the attention epilogue writes e4m3 itself (into the fp8 activation buffer, free at this point)
        OV_STEP(OV_PROF_ATTN, ov_attention_fp8out(big, ldb, q8, D, B, L, H, hd, scale, sc.a_amax, sc.a_next, stream));
        OV_STEP(OV_PROF_GEMM_OUT, ov_gemm_fp8_static(q8, D, q->out_w8, D, nullptr, sc.a_amax, q->out_s, w.out_b, x, D, nullptr, nullptr, M, D, D,
                                                     OV_EPI_BIAS_RESIDUAL, x, D, stream));
    } else {
        if (from_attn) {
        } else if (prefix >= 0) OV_STEP(OV_PROF_ATTN, ov_attention_prefix(big, ldb, h, D, B, L, H, hd, scale, prefix, stream));
        else OV_STEP(OV_PROF_ATTN, ov_attention(big, ldb, h, D, B, L, H, hd, scale, stream));
        if (span.to == BLOCK_PAST_ATTN) return OV_OK;
        if (f_out) {
            OV_STEP(OV_PROF_LN, ov_quant_rows_fp8(h, D, q8, D, qs, M, D, sc.h_mode == 1 ? sc.a_amax : nullptr, stream));
            OV_STEP(OV_PROF_GEMM_OUT, ov_gemm_fp8(q8, D, q->out_w8, D, qs, q->out_s, w.out_b, x, D, M, D, D, OV_EPI_BIAS_RESIDUAL, x, D, stream));
        } else if (rp) {
            OV_STEP(OV_PROF_GEMM_OUT, ov_gemm_rowparts(h, D, w.out_w, D, w.out_b, x, D, M, D, D, x, D, parts, stream));
        } else {
            OV_STEP(OV_PROF_GEMM_OUT, ov_gemm(h, D, w.out_w, D, w.out_b, x, D, M, D, D, OV_EPI_BIAS_RESIDUAL, x, D, 0, 0, 0, stream));
        }
    }
    // ---- MLP half ----
    if (f_fc) {
        OV_STEP(OV_PROF_LN, ov_layernorm_quant_fp8(x, D, w.ln2_w, w.ln2_b, q8, D, qs, M, D, c.ln_eps, stream));
    } else if (fold) {
        if (rp) OV_STEP(OV_PROF_LN, ov_rowstats_finalize(parts, stats, M, D, c.ln_eps, stream));
        else OV_STEP(OV_PROF_LN, ov_rowstats(x, D, stats, M, D, c.ln_eps, stream));
    } else {
        OV_STEP(OV_PROF_LN, ov_layernorm(x, OV_BF16, D, w.ln2_w, w.ln2_b, h, OV_BF16, D, M, D, c.ln_eps, stream));
    }
    if (f_fc && f_proj && sc.h_mode >= 2) {
        // static hidden scale: c_fc quantises its own output (e4m3 bytes, pitch F, in the `big` region), c_proj reads it as is
        unsigned char* h8 = (unsigned char*)big;
        OV_STEP(fc_cls, ov_gemm_fp8_static(q8, D, q->fc_w8, D, qs, nullptr, q->fc_s, q->fc_b, h8, F, sc.h_amax, sc.h_next, M, F, D, gelu, nullptr, 0,
                                           stream));
        OV_STEP(OV_PROF_GEMM_PROJ, ov_gemm_fp8_static(h8, F, q->proj_w8, F, nullptr, sc.h_amax, q->proj_s, w.proj_b, x, D, nullptr, nullptr, M, D, F,
                                                      OV_EPI_BIAS_RESIDUAL, x, D, stream));
    } else {
        if (f_fc) OV_STEP(fc_cls, ov_gemm_fp8(q8, D, q->fc_w8, D, qs, q->fc_s, q->fc_b, big, ldb, M, F, D, gelu, nullptr, 0, stream));
        else if (fold) OV_STEP(fc_cls, ov_gemm_ln(x, D, w.fc_w, D, w.fc_b, w.fc_colsum, stats, big, ldb, M, F, D, gelu, stream));
        else OV_STEP(fc_cls, ov_gemm(h, D, w.fc_w, D, w.fc_b, big, ldb, M, F, D, gelu, nullptr, 0, 0, 0, 0, stream));
        if (span.to == BLOCK_PAST_FC) return OV_OK;
        if (f_proj) {
            OV_STEP(OV_PROF_LN, ov_quant_rows_fp8(big, ldb, q8, F, qs, M, F, (sc.h_mode == 1 && f_fc) ? sc.h_amax : nullptr, stream));
            OV_STEP(OV_PROF_GEMM_PROJ, ov_gemm_fp8(q8, F, q->proj_w8, F, qs, q->proj_s, w.proj_b, x, D, M, D, F, OV_EPI_BIAS_RESIDUAL, x, D, stream));
        } else if (rp) {
            OV_STEP(OV_PROF_GEMM_PROJ, ov_gemm_rowparts(big, ldb, w.proj_w, F, w.proj_b, x, D, M, D, F, x, D, parts, stream));
        } else {
            OV_STEP(OV_PROF_GEMM_PROJ, ov_gemm(big, ldb, w.proj_w, F, w.proj_b, x, D, M, D, F, OV_EPI_BIAS_RESIDUAL, x, D, 0, 0, 0, stream));
        }
    }
#undef OV_STEP
    return OV_OK;
}

// The tower's tail context if it is usable on the CURRENT device (created on first use), else nullptr (= do not split).
TailCtx* tail_ctx(const ov_tower* t) {
    TailCtx& tc = t->tail;
    std::lock_guard<std::mutex> lk(tc.mu);
    if (tc.state == 0) {
        const char* e = getenv("OVHIP_NO_TAIL_SPLIT");
        if (e && e[0] == '1') { tc.state = -1; return nullptr; }
        tc.device = ov_current_device();
        if (hipStreamCreateWithFlags(&tc.stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&tc.fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&tc.join, hipEventDisableTiming) == hipSuccess)
            tc.state = 1;
        else
            tc.state = -1;
    }
    return tc.state == 1 && tc.device == ov_current_device() ? &tc : nullptr;
}

// Images to peel off so that the main part's 256-row tile count is a multiple of 64 (x 4 column tiles = whole rounds of
// 256 CUs for the N = width GEMMs).  0 = do not split.
int tail_images(int B, int L) {
    const int64_t T = ((int64_t)B * L + 255) / 256;
    const int r = (int)(T % 64);
    if (T <= 64 || r == 0 || r > 8) return 0;
    const int64_t target = T - r;                                // tiles the main part may use
    int Bm = (int)((target * 256) / L);                           // largest B' with ceil(B'*L/256) <= target
    while (Bm > 0 && ((int64_t)Bm * L + 255) / 256 > target) --Bm;
    const int tail = B - Bm;
    if (Bm <= 0 || tail <= 0 || tail > B / 8) return 0;
    return tail;
}
}  // namespace

// x[B*L, D] is updated in place through all blocks.  When B*L leaves a few 256-row tiles over a whole number of rounds
// (L/14 at B = 256: 257 tiles -> the out-proj / c_proj GEMMs need a 5th round for 4 of their 1028 tiles), the last
// image(s) are peeled off and run, layer by layer, on an internal side stream: rows are independent through LN/GEMM and
// attention never crosses images, so the split is exact; the main part then fills whole rounds and the tail's small
// kernels slot into idle CUs.  Fork/join by events; everything remains ordered with respect to the caller's stream.
// last_to: where the LAST block ends (BlockPoint; anything but BLOCK_END needs a bf16 tower, and leaves the rest of it to the caller).
static int tower_walk(const ov_tower* t, ov_bf16* x, int B, int L, void* workspace, size_t workspace_bytes, ov_stream_t stream,
                      int last_to) {
    if (!t || !x || !workspace || B <= 0 || L <= 0) return OV_ERR_INVALID;
    if (t->drop_idx) return OV_ERR_UNSUPPORTED;                    // drop path is the training walks' (ov_tower_set_drop_path)
    const TowerWs w = tower_ws(t, B, L);
    if (workspace_bytes < w.total) return OV_ERR_WORKSPACE;
    if (((uintptr_t)x | (uintptr_t)workspace) & 15) return OV_ERR_INVALID;
    const ov_tower_cfg& c = t->cfg;
    for (int i = 0; i < c.layers; ++i)
        if (!t->set[i]) return OV_ERR_INVALID;

    int nt = tail_images(B, L);
    TailCtx* tc = nt > 0 ? tail_ctx(t) : nullptr;
    if (!tc) nt = 0;
    const int Bm = B - nt;
    hipStream_t main_st = (hipStream_t)stream;
    // fork .. join under the tower's mutex: the events are this tower's own, a second host thread enqueues after the join
    std::unique_lock<std::mutex> tail_lock;
    if (nt > 0) {
        tail_lock = std::unique_lock<std::mutex>(tc->mu);
        hipError_t e = hipEventRecord(tc->fork, main_st);
        if (e == hipSuccess) e = hipStreamWaitEvent(tc->stream, tc->fork, 0);
        if (e != hipSuccess) return OV_ERR_HIP - (int)e;
    }
    const bool fp8 = w.fp8;
    if (t->prefix >= 0 && fp8) return OV_ERR_UNSUPPORTED;          // no fp8 under a mask
    if (last_to != BLOCK_END && fp8) return OV_ERR_UNSUPPORTED;
    if (t->prefix > L) return OV_ERR_INVALID;
    int rc = OV_OK;
    if (fp8 && t->h_amax && t->h_mode == 2)            // delayed scaling: last forward's maxima become this forward's scales
        rc = ov_amax_roll(t->h_amax, t->h_amax + 2 * c.layers, 2 * c.layers, stream);
    const bool parts = use_rowparts() && !fp8;
    const BlockPart main_part = tower_part(c, w, (char*)workspace, x, 0, Bm, parts, stream, true);
    const BlockPart tail_part = tower_part(c, w, (char*)workspace, x, (int64_t)Bm * L, nt, parts, (ov_stream_t)(nt > 0 ? tc->stream : nullptr), false);
    for (int i = 0; i < c.layers && rc == OV_OK; ++i) {
        Fp8Scales sc = {nullptr, nullptr, nullptr, nullptr, 0};
        if (t->h_amax) sc = {t->h_amax + i, t->h_amax + c.layers + i, t->h_amax + 2 * c.layers + i, t->h_amax + 3 * c.layers + i, t->h_mode};
        const ov_block_fp8* q = fp8 ? &t->fp8[i] : nullptr;
        const int mask = fp8 ? t->mask8[i] : 0;
        const BlockSpan span = {BLOCK_START, i == c.layers - 1 ? last_to : BLOCK_END};
        rc = run_block(c, t->blocks[i], q, mask, sc, main_part, i > 0, L, t->prefix, span);
        if (rc == OV_OK && nt > 0) rc = run_block(c, t->blocks[i], q, mask, sc, tail_part, i > 0, L, t->prefix, span);
    }
    if (nt > 0) {
        // always join, also after an error between fork and here: whatever the side stream got stays ordered before the
        // caller's next work on `stream` (and before the workspace is reused)
        hipError_t e = hipEventRecord(tc->join, tc->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(main_st, tc->join, 0);
        if (e != hipSuccess && rc == OV_OK) rc = OV_ERR_HIP - (int)e;
    }
    return rc;
}

extern "C" int ov_tower_forward(const ov_tower* t, ov_bf16* x, int B, int L, void* workspace, size_t workspace_bytes,
                                ov_stream_t stream) {
    return tower_walk(t, x, B, L, workspace, workspace_bytes, stream, BLOCK_END);
}

// ---- training-side entry points: keep every block's input, run the blocks' backward in reverse -------------
// (backward.hip's block_backward_partial / block_backward_input / block_grad_pairs: common.h)

// saved activations of one layer: [x | qkv | attention out | x1 | ln_1 out | ln_2 out | c_fc pre-activation | c_fc activation],
// 8 D + 2 mlp_pad bf16 per token (the default keeps them all; ov_tower_forward_checkpointed keeps only x and recomputes the rest
// per block in the backward)
// + per layer the attention's row log-sum-exp, fp32 [B * heads][L rounded up to 32] (ov_attention_lse; used by the backward where the
// resident kernel applies: ov_attn_bwd_resident)
static inline size_t saved_per_token(const ov_tower_cfg& c) { return (size_t)8 * c.width + 2 * (size_t)c.mlp_pad; }
static inline size_t saved_lse_elems(const ov_tower_cfg& c, int B, int L) {      // in bf16 elements, a multiple of 8 (16-byte sections)
    return ((size_t)2 * B * c.heads * ((L + 31) / 32 * 32) + 7) / 8 * 8;
}
static inline size_t saved_per_layer(const ov_tower_cfg& c, int B, int L) { return (size_t)B * L * saved_per_token(c) + saved_lse_elems(c, B, L); }
extern "C" size_t ov_tower_saved_bytes(const ov_tower* t, int B, int L) {
    if (!t || B <= 0 || L <= 0) return 0;
    return (size_t)t->cfg.layers * saved_per_layer(t->cfg, B, L) * sizeof(ov_bf16);
}

namespace {
// one layer's slot: [x | qkv | attention out | x1 | ln_1 out | ln_2 out | c_fc pre-activation | c_fc activation | lse]; `rest` = where
// the part after x starts (sx + M D in `saved`; elsewhere for the layers a Layout does not keep whole)
struct Slot { ov_bf16 *x, *qkv, *o, *x1, *n1, *n2, *pre, *act; float* lse; };
inline Slot slot_at(const ov_tower_cfg& c, ov_bf16* sx, ov_bf16* rest, int64_t M) {
    Slot s;
    s.x = sx;
    s.qkv = rest;
    s.o = s.qkv + (size_t)M * 3 * c.width;
    s.x1 = s.o + (size_t)M * c.width;
    s.n1 = s.x1 + (size_t)M * c.width;
    s.n2 = s.n1 + (size_t)M * c.width;
    s.pre = s.n2 + (size_t)M * c.width;
    s.act = s.pre + (size_t)M * c.mlp_pad;
    s.lse = (float*)(s.act + (size_t)M * c.mlp_pad);
    return s;
}
inline ov_block_saved block_saved_of(const ov_tower_cfg& c, const Slot& s, int L, int prefix) {
    ov_block_saved sv;
    sv.qkv = s.qkv; sv.attn_out = s.o; sv.x1 = s.x1; sv.ln1_out = s.n1; sv.ln2_out = s.n2; sv.fc_pre = s.pre; sv.fc_act = s.act;
    sv.attn_lse = prefix < 0 && ov_attn_bwd_resident(c.width / c.heads, L) ? s.lse : nullptr;   // (the masked forward keeps none)
    return sv;
}

// Where a kept layer i >= first has its input and the rest of its slot: x + (i - first) x_stride and rest + (i - first) rest_stride.
// Saving (ov_tower_forward_saving[_from]): a whole slot per layer in `saved`.  Checkpointed: the inputs M D apart in ckpt, and one slot
// that every layer shares (stride 0).
struct Layout { ov_bf16* x; size_t x_stride; ov_bf16* rest; size_t rest_stride; };
inline Layout saving_layout(const ov_tower_cfg& c, const ov_bf16* saved, int B, int L) {
    ov_bf16* s = const_cast<ov_bf16*>(saved);
    const size_t spl = saved_per_layer(c, B, L);
    return {s, spl, s ? s + (size_t)B * L * c.width : nullptr, spl};
}
inline Layout checkpointed_layout(const ov_tower_cfg& c, const ov_bf16* ckpt, void* slot, int B, int L) {
    return {const_cast<ov_bf16*>(ckpt), (size_t)B * L * c.width, (ov_bf16*)slot, 0};
}
inline Slot layer_slot(const ov_tower_cfg& c, const Layout& ly, int k, int64_t M) {     // k = i - first
    return slot_at(c, ly.x + (size_t)k * ly.x_stride, ly.rest + (size_t)k * ly.rest_stride, M);
}

// One block of the saving forward: the same operator sequence as run_block, with qkv / attention output / x1 / ... written where the
// backward will read them, the input read from s.x and the output written to y (y may be s.x: nothing reads the input after out_proj).
// y = NULL: the slot only (the backward's recompute), c_proj is not run.
// drop (ov_tower_set_drop_path; NULL = none): a branch that does not keep every sample at scale 1 runs compact -- its kept samples' rows
// gathered into drop->g0, the same operators on count L rows into the LEADING rows of the slot's regions, the product with its bias
// into drop->g1 (OV_EPI_BIAS: no fused residual), then res + scale * product scattered over all B samples (a dropped sample's rows are
// the residual's, bitwise).  count == 0: the branch's output is a copy of its input.
int forward_saving_layer(const ov_tower_cfg& c, const ov_block_weights& w, const Slot& s, ov_bf16* y, int B, int L, ov_stream_t stream,
                         int prefix, const ov_block_drop* drop = nullptr) {
    const int D = c.width, H = c.heads, hd = D / H;
    const int64_t M = (int64_t)B * L;
    const float scale = 1.0f / sqrtf((float)hd);
    const int gelu = c.gelu_tanh ? OV_EPI_BIAS_GELU_TANH : OV_EPI_BIAS_GELU_ERF;
    const ov_drop_branch* da = drop && ov_branch_compact(drop->attn, B) ? &drop->attn : nullptr;
    const ov_drop_branch* dm = drop && ov_branch_compact(drop->mlp, B) ? &drop->mlp : nullptr;
    const int Ba = da ? da->count : B, Bm = dm ? dm->count : B;      // samples each branch runs on
    const int64_t Ma = (int64_t)Ba * L, Mm = (int64_t)Bm * L;
    const size_t stream_bytes = (size_t)M * D * sizeof(ov_bf16);
    int rc;
    // ---- attention half ----
    const ov_bf16* xa = s.x;
    if (da && Ba > 0) {
        if ((rc = ov_sample_gather(s.x, da->idx, drop->g0, B, Ba, L, D, 1.0f, stream))) return rc;
        xa = drop->g0;
    }
    if (Ba > 0) {
        if ((rc = ov_layernorm(xa, OV_BF16, D, w.ln1_w, w.ln1_b, s.n1, OV_BF16, D, Ma, D, c.ln_eps, stream))) return rc;
        if ((rc = ov_gemm(s.n1, D, w.qkv_w, D, w.qkv_b, s.qkv, 3 * D, Ma, 3 * D, D, OV_EPI_BIAS, nullptr, 0, 0, 0, 0, stream))) return rc;
        if (prefix >= 0) rc = ov_attention_prefix(s.qkv, 3 * D, s.o, D, Ba, L, H, hd, scale, prefix, stream);
        else
            rc = ov_attn_bwd_resident(hd, L) ? ov_attention_lse(s.qkv, 3 * D, s.o, D, s.lse, Ba, L, H, hd, scale, stream)
                                             : ov_attention(s.qkv, 3 * D, s.o, D, Ba, L, H, hd, scale, stream);
        if (rc) return rc;
    }
    if (!da) {
        if ((rc = ov_gemm(s.o, D, w.out_w, D, w.out_b, s.x1, D, M, D, D, OV_EPI_BIAS_RESIDUAL, s.x, D, 0, 0, 0, stream))) return rc;
    } else if (Ba > 0) {
        if ((rc = ov_gemm(s.o, D, w.out_w, D, w.out_b, drop->g1, D, Ma, D, D, OV_EPI_BIAS, nullptr, 0, 0, 0, 0, stream))) return rc;
        if ((rc = ov_sample_scatter_axpy(s.x, drop->g1, da->slot, s.x1, B, Ba, L, D, da->scale, stream))) return rc;
    } else if ((rc = ov_hip(hipMemcpyAsync(s.x1, s.x, stream_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream)))) {
        return rc;
    }
    // ---- MLP half ----
    const ov_bf16* xm = s.x1;
    if (dm && Bm > 0) {
        if ((rc = ov_sample_gather(s.x1, dm->idx, drop->g0, B, Bm, L, D, 1.0f, stream))) return rc;
        xm = drop->g0;
    }
    if (Bm > 0) {
        if ((rc = ov_layernorm(xm, OV_BF16, D, w.ln2_w, w.ln2_b, s.n2, OV_BF16, D, Mm, D, c.ln_eps, stream))) return rc;
        if ((rc = ov_gemm_keep(s.n2, D, w.fc_w, D, w.fc_b, s.act, c.mlp_pad, s.pre, c.mlp_pad, Mm, c.mlp_pad, D, gelu, stream))) return rc;
    }
    if (!y) return OV_OK;
    if (!dm) return ov_gemm(s.act, c.mlp_pad, w.proj_w, c.mlp_pad, w.proj_b, y, D, M, D, c.mlp_pad, OV_EPI_BIAS_RESIDUAL, s.x1, D, 0, 0, 0, stream);
    if (Bm == 0) return ov_hip(hipMemcpyAsync(y, s.x1, stream_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if ((rc = ov_gemm(s.act, c.mlp_pad, w.proj_w, c.mlp_pad, w.proj_b, drop->g1, D, Mm, D, c.mlp_pad, OV_EPI_BIAS, nullptr, 0, 0, 0, 0, stream)))
        return rc;
    return ov_sample_scatter_axpy(s.x1, drop->g1, dm->slot, y, B, Bm, L, D, dm->scale, stream);
}

// The table's part for layer i of a walk over B samples, in `d` (whose scratch fields block_drop_plan filled); NULL = no table
const ov_block_drop* layer_drop(const ov_tower* t, int i, ov_block_drop& d) {
    if (!t->drop_idx) return nullptr;
    const size_t B = (size_t)t->drop_B;
    d.attn = {t->drop_idx + (2 * (size_t)i) * B, t->drop_slot + (2 * (size_t)i) * B, t->drop_count[2 * i], t->drop_scale[i]};
    d.mlp = {t->drop_idx + (2 * (size_t)i + 1) * B, t->drop_slot + (2 * (size_t)i + 1) * B, t->drop_count[2 * i + 1], t->drop_scale[i]};
    return &d;
}
// A walk under a table: its B is the table's and the scratch holds the plan for (B, L); `d` gets the carved scratch.  No table: OV_OK
int drop_walk_check(const ov_tower* t, int B, int L, ov_block_drop& d) {
    if (!t->drop_idx) return OV_OK;
    if (B != t->drop_B) return OV_ERR_INVALID;
    const size_t need = block_drop_plan(&t->cfg, B, L, t->drop_ws, &d);
    if (need == 0) return OV_ERR_UNSUPPORTED;
    return t->drop_ws_bytes >= need ? OV_OK : OV_ERR_WORKSPACE;
}

// The training forward: layers [0, first) run in place on x with their intermediates in `scratch` (the same operators on the same
// values, nothing kept); then x is copied into layer first's input, and each kept layer reads its input from its slot and writes its
// output straight into the next layer's input, the top layer into x.
int forward_walk(const ov_tower* t, int first, ov_bf16* x, ov_bf16* scratch, const Layout& ly, int B, int L, ov_stream_t stream) {
    const ov_tower_cfg& c = t->cfg;
    const int64_t M = (int64_t)B * L;
    if (t->prefix > L) return OV_ERR_INVALID;
    ov_block_drop dp = {};
    if (const int rc = drop_walk_check(t, B, L, dp)) return rc;
    for (int i = 0; i < first; ++i) {
        const int rc = forward_saving_layer(c, t->blocks[i], slot_at(c, x, scratch, M), x, B, L, stream, t->prefix, layer_drop(t, i, dp));
        if (rc) return rc;
    }
    if (first == c.layers) return OV_OK;
    const hipError_t e = hipMemcpyAsync(ly.x, x, (size_t)M * c.width * sizeof(ov_bf16), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return OV_ERR_HIP - (int)e;
    for (int i = first; i < c.layers; ++i) {
        const Slot s = layer_slot(c, ly, i - first, M);
        const int rc = forward_saving_layer(c, t->blocks[i], s, i + 1 < c.layers ? s.x + ly.x_stride : x, B, L, stream, t->prefix,
                                            layer_drop(t, i, dp));
        if (rc) return rc;
    }
    return OV_OK;
}

// The lowest layer a backward over the kept layers [first, layers) runs: `first` when d(input) is wanted, otherwise the lowest one with
// a requested pair (layers: none).  -1 when a pair of grads has one NULL pointer or a misaligned one.
int lowest_layer(const ov_tower* t, int first, const ov_block_grads* grads, bool want_dx) {
    int lo = want_dx ? first : t->cfg.layers;
    for (int i = t->cfg.layers - 1; i >= first; --i) {
        const int p = block_grad_pairs(&grads[i - first]);
        if (p < 0) return -1;
        if (p && i < lo) lo = i;
    }
    return lo;
}

// The training backward: layers layers-1 .. lo in reverse; dx holds d(block output) on entry and d(block input) on exit, and layer lo
// writes it only when want_dx.  rebuild: each layer's slot is first rebuilt from its input by the forward's own launches without c_proj
// (the backward never reads the block output), except the top layer's when top_kept.  grads[i - first] -> block_backward_partial;
// grads = NULL -> block_backward_input (input gradients only).
int backward_walk(const ov_tower* t, int first, int lo, const Layout& ly, bool rebuild, bool top_kept, ov_bf16* dx,
                  const ov_block_grads* grads, bool want_dx, int B, int L, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    const ov_tower_cfg& c = t->cfg;
    const int64_t M = (int64_t)B * L;
    if (t->prefix > L) return OV_ERR_INVALID;
    ov_block_drop dp = {};
    if (const int rc = drop_walk_check(t, B, L, dp)) return rc;
    for (int i = c.layers - 1; i >= lo; --i) {
        const Slot s = layer_slot(c, ly, i - first, M);
        const ov_block_drop* drop = layer_drop(t, i, dp);
        int rc;
        if (rebuild && !(top_kept && i == c.layers - 1) && (rc = forward_saving_layer(c, t->blocks[i], s, nullptr, B, L, stream, t->prefix, drop)))
            return rc;
        const ov_block_saved sv = block_saved_of(c, s, L, t->prefix);
        rc = grads ? block_backward_partial(&c, &t->blocks[i], s.x, &sv, dx, (i > lo || want_dx) ? dx : nullptr, &grads[i - first], t->prefix,
                                            B, L, workspace, workspace_bytes, stream, drop)
                   : block_backward_input(&c, &t->blocks[i], s.x, &sv, dx, dx, t->prefix, B, L, workspace, stream, drop);
        if (rc) return rc;
    }
    return OV_OK;
}

// The checks the training entry points share, made after their own pointer checks and reported in this order: an fp8 tower where the
// entry point runs the bf16 forward (bf16) or a block shape the backward kernels do not take (!shape_ok; backward.hip's block_cfg_ok:
// width % 64, head_dim % 8 and <= 96, mlp_pad % 64); a short workspace; a pointer in `ptrs` off 16 bytes; a block that is not set or
// holds LN-folded weights (the walks run and differentiate the module's own).
int check_walk(const ov_tower* t, bool bf16, bool shape_ok, bool ws_ok, uintptr_t ptrs) {
    if ((bf16 && tower_fp8(t)) || !shape_ok) return OV_ERR_UNSUPPORTED;
    if (!ws_ok) return OV_ERR_WORKSPACE;
    if (ptrs & 15) return OV_ERR_INVALID;
    for (int i = 0; i < t->cfg.layers; ++i)
        if (!t->set[i] || t->blocks[i].qkv_colsum || t->blocks[i].fc_colsum) return OV_ERR_INVALID;
    return OV_OK;
}
}  // namespace

// (every intermediate lands in `saved`: the workspace is checked but stays unused)
extern "C" int ov_tower_forward_saving(const ov_tower* t, ov_bf16* x, ov_bf16* saved, int B, int L, void* workspace,
                                       size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !x || !saved || !workspace || B <= 0 || L <= 0) return OV_ERR_INVALID;
    const int rc = check_walk(t, true, true, workspace_bytes >= ov_tower_workspace_bytes(t, B, L),
                              (uintptr_t)x | (uintptr_t)saved | (uintptr_t)workspace);
    return rc ? rc : forward_walk(t, 0, x, nullptr, saving_layout(t->cfg, saved, B, L), B, L, stream);
}

// ---- frozen lower layers: keep only layers [first, layers) ----------------------------------------------------------------------------
extern "C" size_t ov_tower_saved_bytes_from(const ov_tower* t, int first, int B, int L) {
    if (!t || B <= 0 || L <= 0 || first < 0 || first > t->cfg.layers) return 0;
    return (size_t)(t->cfg.layers - first) * saved_per_layer(t->cfg, B, L) * sizeof(ov_bf16);
}

// one layer's slot without its x part
static inline size_t slot_rest_bytes(const ov_tower_cfg& c, int B, int L) {
    return (saved_per_layer(c, B, L) - (size_t)B * L * c.width) * sizeof(ov_bf16);
}

// the layers below `first` run in place on x with their intermediates in one slot's worth of workspace (all but its x part); 0 = none
extern "C" size_t ov_tower_forward_saving_from_workspace_bytes(const ov_tower* t, int first, int B, int L) {
    if (!t || B <= 0 || L <= 0 || first <= 0 || first > t->cfg.layers) return 0;
    return slot_rest_bytes(t->cfg, B, L);
}

extern "C" int ov_tower_forward_saving_from(const ov_tower* t, int first, ov_bf16* x, ov_bf16* saved, int B, int L, void* workspace,
                                            size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !x || B <= 0 || L <= 0 || first < 0 || first > t->cfg.layers) return OV_ERR_INVALID;
    if (first < t->cfg.layers && !saved) return OV_ERR_INVALID;
    const size_t need = ov_tower_forward_saving_from_workspace_bytes(t, first, B, L);
    if (need > 0 && !workspace) return OV_ERR_INVALID;
    const int rc = check_walk(t, true, true, workspace_bytes >= need, (uintptr_t)x | (uintptr_t)saved | (uintptr_t)workspace);
    return rc ? rc : forward_walk(t, first, x, (ov_bf16*)workspace, saving_layout(t->cfg, saved, B, L), B, L, stream);
}

extern "C" size_t ov_tower_backward_workspace_bytes(const ov_tower* t, int B, int L) {
    if (!t) return 0;
    return ov_block_backward_workspace_bytes(&t->cfg, B, L);
}

// Every pair of every layer and dx: block_backward_partial then runs the chain as ov_block_backward does.  The checks keep the codes
// and the order in which a walk over ov_block_backward reported them (the top layer's, then the workspace and the alignment, then the
// layers below; folded weights are OV_ERR_UNSUPPORTED here), but all of them come before the first launch.
extern "C" int ov_tower_backward(const ov_tower* t, const ov_bf16* saved, ov_bf16* dx, const ov_block_grads* grads, int B, int L,
                                 void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !saved || !dx || !grads || !workspace || B <= 0 || L <= 0) return OV_ERR_INVALID;
    const ov_tower_cfg& c = t->cfg;
    for (int i = 0; i < c.layers; ++i)
        if (!t->set[i]) return OV_ERR_INVALID;
    const size_t need = ov_tower_backward_workspace_bytes(t, B, L);
    if (need == 0) return OV_ERR_UNSUPPORTED;                       // block_cfg_ok
    auto layer_rc = [&](int i) -> int {
        if (t->blocks[i].qkv_colsum || t->blocks[i].fc_colsum) return OV_ERR_UNSUPPORTED;
        return block_grad_pairs(&grads[i]) == 63 ? OV_OK : OV_ERR_INVALID;
    };
    int rc = layer_rc(c.layers - 1);
    if (rc) return rc;
    if (workspace_bytes < need) return OV_ERR_WORKSPACE;
    if (((uintptr_t)saved | (uintptr_t)dx | (uintptr_t)workspace) & 15) return OV_ERR_INVALID;
    for (int i = c.layers - 2; i >= 0; --i)
        if ((rc = layer_rc(i))) return rc;
    return backward_walk(t, 0, 0, saving_layout(c, saved, B, L), false, false, dx, grads, true, B, L, workspace, workspace_bytes, stream);
}

// Input gradients only (frozen weights): the same layers in reverse over the same saved activations, with the dX chain of each block
// and no parameter-gradient work.  dx comes out bitwise equal to ov_tower_backward's.
extern "C" size_t ov_tower_backward_input_workspace_bytes(const ov_tower* t, int B, int L) {
    if (!t) return 0;
    return block_backward_input_workspace_bytes(&t->cfg, B, L);
}

extern "C" int ov_tower_backward_input(const ov_tower* t, const ov_bf16* saved, ov_bf16* dx, int B, int L, void* workspace,
                                       size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !saved || !dx || !workspace || B <= 0 || L <= 0) return OV_ERR_INVALID;
    const size_t need = ov_tower_backward_input_workspace_bytes(t, B, L);
    const int rc = check_walk(t, false, need > 0, workspace_bytes >= need, (uintptr_t)saved | (uintptr_t)dx | (uintptr_t)workspace);
    return rc ? rc : backward_walk(t, 0, 0, saving_layout(t->cfg, saved, B, L), false, false, dx, nullptr, true, B, L, workspace,
                                   workspace_bytes, stream);
}

// Partial backward (frozen parameters): the layers [first, layers) that ov_tower_forward_saving_from kept, in reverse, with the pairs
// grads[i - first] requests.  Frozen blocks above the lowest trainable one run input-only; with want_dx = 0 nothing runs below it.
// Every gradient computed is bitwise ov_tower_backward's.
extern "C" size_t ov_tower_backward_partial_workspace_bytes(const ov_tower* t, int B, int L) {
    if (!t) return 0;
    return ov_block_backward_workspace_bytes(&t->cfg, B, L);
}

extern "C" int ov_tower_backward_partial(const ov_tower* t, int first, const ov_bf16* saved, ov_bf16* dx, const ov_block_grads* grads,
                                         int want_dx, int B, int L, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !dx || B <= 0 || L <= 0 || first < 0 || first > t->cfg.layers) return OV_ERR_INVALID;
    if (first == t->cfg.layers) return OV_OK;                     // nothing kept: d(input of layer `first`) = d(output), already in dx
    if (!saved || !grads || !workspace) return OV_ERR_INVALID;
    const int lo = lowest_layer(t, first, grads, want_dx);
    if (lo < 0) return OV_ERR_INVALID;
    const size_t need = ov_tower_backward_partial_workspace_bytes(t, B, L);
    const int rc = check_walk(t, false, need > 0, workspace_bytes >= need, (uintptr_t)saved | (uintptr_t)dx | (uintptr_t)workspace);
    return rc ? rc : backward_walk(t, first, lo, saving_layout(t->cfg, saved, B, L), false, false, dx, grads, want_dx, B, L, workspace,
                                   workspace_bytes, stream);
}

// ---- activation recomputation (the reference's remat='full' per block): keep each kept layer's input only ----------------------------
extern "C" size_t ov_tower_checkpoint_bytes(const ov_tower* t, int first, int B, int L) {
    if (!t || B <= 0 || L <= 0 || first < 0 || first > t->cfg.layers) return 0;
    return (size_t)(t->cfg.layers - first) * B * L * t->cfg.width * sizeof(ov_bf16);
}

extern "C" size_t ov_tower_slot_bytes(const ov_tower* t, int B, int L) {
    if (!t || B <= 0 || L <= 0) return 0;
    return slot_rest_bytes(t->cfg, B, L);
}

// The layers below `first` as in ov_tower_forward_saving_from with `slot` as their scratch; the kept layers read their inputs from ckpt
// and share `slot`, which ends up holding exactly the top layer's saved slot (x part: ckpt[layers-1-first]).
extern "C" int ov_tower_forward_checkpointed(const ov_tower* t, int first, ov_bf16* x, ov_bf16* ckpt, void* slot, size_t slot_bytes, int B,
                                             int L, ov_stream_t stream) {
    if (!t || !x || !slot || B <= 0 || L <= 0 || first < 0 || first > t->cfg.layers) return OV_ERR_INVALID;
    if (first < t->cfg.layers && !ckpt) return OV_ERR_INVALID;
    const int rc = check_walk(t, true, true, slot_bytes >= ov_tower_slot_bytes(t, B, L), (uintptr_t)x | (uintptr_t)ckpt | (uintptr_t)slot);
    return rc ? rc : forward_walk(t, first, x, (ov_bf16*)slot, checkpointed_layout(t->cfg, ckpt, slot, B, L), B, L, stream);
}

// ov_tower_backward_partial over checkpoints: each layer's slot is rebuilt in `slot` from ckpt[i - first] before its block backward,
// except the top layer's when the caller says `slot` still holds it from ov_tower_forward_checkpointed.  Every gradient is bitwise
// ov_tower_backward_partial's over ov_tower_forward_saving_from's slots.
extern "C" int ov_tower_backward_checkpointed(const ov_tower* t, int first, const ov_bf16* ckpt, void* slot, size_t slot_bytes,
                                              int slot_holds_top, ov_bf16* dx, const ov_block_grads* grads, int want_dx, int B, int L,
                                              void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !dx || B <= 0 || L <= 0 || first < 0 || first > t->cfg.layers) return OV_ERR_INVALID;
    if (first == t->cfg.layers) return OV_OK;                     // nothing kept: d(input of layer `first`) = d(output), already in dx
    if (!ckpt || !slot || !grads || !workspace) return OV_ERR_INVALID;
    const int lo = lowest_layer(t, first, grads, want_dx);
    if (lo < 0) return OV_ERR_INVALID;
    const size_t need = ov_tower_backward_partial_workspace_bytes(t, B, L);
    const int rc = check_walk(t, true, need > 0, workspace_bytes >= need && slot_bytes >= ov_tower_slot_bytes(t, B, L),
                              (uintptr_t)ckpt | (uintptr_t)slot | (uintptr_t)dx | (uintptr_t)workspace);
    return rc ? rc : backward_walk(t, first, lo, checkpointed_layout(t->cfg, ckpt, slot, B, L), true, slot_holds_top, dx, grads, want_dx,
                                   B, L, workspace, workspace_bytes, stream);
}

// ---- the encoders ------------------------------------------------------------------------------------------------------------------------
static inline bool grid_ok(const ov_vision_head* h, int K) {      // K = 0 (every patch) or 1 <= K <= G kept ones
    const int g = h->patch_size > 0 ? h->image_size / h->patch_size : 0;
    return h->patch_size > 0 && K >= 0 && K <= g * g;
}

extern "C" size_t ov_vision_workspace_bytes(const ov_tower* t, const ov_vision_head* h, int B) {
    if (!t || !h || B <= 0 || h->patch_size <= 0) return 0;
    return vision_ws(t, h, B, 0).total;
}

extern "C" size_t ov_vision_keep_workspace_bytes(const ov_tower* t, const ov_vision_head* h, int B, int K) {
    if (!t || !h || B <= 0 || K < 1 || !grid_ok(h, K)) return 0;
    return vision_ws(t, h, B, K).total;
}

extern "C" size_t ov_vision_embed_workspace_bytes(const ov_tower* t, const ov_vision_head* h, int B, int K) {
    if (!t || !h || B <= 0 || !grid_ok(h, K)) return 0;
    return embed_ws(t, h, B, K).total;
}

extern "C" size_t ov_vision_head_workspace_bytes(const ov_tower* t, const ov_vision_head* h, int B) {
    if (!t || !h || B <= 0) return 0;
    return head_ws(B, t->cfg.width, h->embed_pad, 4).total;
}

// The patch embedding in its workspace (embed_ws; arguments checked by the callers): im2col rows -> conv1 as a GEMM whose epilogue skips
// one cls row per image and adds the pos-emb rows (K = 0: rows 1..G, broadcast over the batch; keep form: the kept patches' rows, gathered
// into posk by the im2col launch, one to one) -> the cls rows.
static int vision_embed(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, const int* keep, int B, int K,
                        ov_bf16* x, int* err_flag, void* workspace, ov_stream_t stream) {
    const int g = h->image_size / h->patch_size, n = K ? K : g * g, D = t->cfg.width;
    ov_bf16 *patches = (ov_bf16*)workspace, *posk = (ov_bf16*)((char*)workspace + embed_ws(t, h, B, K).posk);
    int rc = K ? ov_im2col_patches_keep_pos(image, img_dtype, keep, patches, B, h->image_size, h->patch_size, K, h->kpad, h->pos, posk, D,
                                            err_flag, stream)
               : ov_im2col_patches(image, img_dtype, patches, B, h->image_size, h->patch_size, h->kpad, stream);
    if (rc) return rc;
    if ((rc = ov_gemm(patches, h->kpad, h->conv_w, h->kpad, nullptr, x, D, (int64_t)B * n, D, h->kpad, OV_EPI_BIAS_RESIDUAL, K ? posk : h->pos,
                      D, n, K ? 0 : n, K ? 0 : 1, stream)))
        return rc;
    return ov_cls_rows(x, D, h->cls, h->pos_f32, B, n + 1, D, stream);
}
static inline bool kpad_ok(const ov_vision_head* h) { return h->kpad % 64 == 0 && h->kpad >= 3 * h->patch_size * h->patch_size; }

extern "C" int ov_vision_embed(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, int B,
                               ov_bf16* x, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !h || !image || !x || !workspace || B <= 0) return OV_ERR_INVALID;
    if (workspace_bytes < embed_ws(t, h, B, 0).total) return OV_ERR_WORKSPACE;
    if (!kpad_ok(h)) return OV_ERR_INVALID;
    return vision_embed(t, h, image, img_dtype, nullptr, B, 0, x, nullptr, workspace, stream);
}

extern "C" int ov_vision_embed_keep(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, const int* keep, int B,
                                    int K, ov_bf16* x, int* err_flag, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !h || !image || !keep || !x || !workspace || B <= 0 || K < 1 || !grid_ok(h, K) || !kpad_ok(h)) return OV_ERR_INVALID;
    if (workspace_bytes < embed_ws(t, h, B, K).total) return OV_ERR_WORKSPACE;
    return vision_embed(t, h, image, img_dtype, keep, B, K, x, err_flag, workspace, stream);
}

namespace {
struct HeadBufs { void* rows; ov_bf16 *ln, *feat; };             // head_ws's regions in a workspace
inline HeadBufs head_bufs(const HeadWs& w, char* ws) { return {ws + w.rows, (ov_bf16*)(ws + w.ln), (ov_bf16*)(ws + w.feat)}; }
// the image head's buffers, after the checks of the head itself
int vision_head_bufs(const ov_tower* t, const ov_vision_head* h, int B, void* workspace, size_t workspace_bytes, HeadBufs* hb) {
    if (h->embed_pad % 8 || h->embed_pad < h->embed_dim) return OV_ERR_INVALID;
    // OpenVision: pool -> LN (transformer.py:638-640).  LN -> pool (:641-643) is the same arithmetic under 'tok' pooling, where the
    // pool picks one row and LayerNorm is per row; under 'avg' it is another function, which is not built.
    if (!h->final_ln_after_pool && h->pool_avg) return OV_ERR_UNSUPPORTED;
    const HeadWs w = head_ws(B, t->cfg.width, h->embed_pad, 4);
    if (workspace_bytes < w.total) return OV_ERR_WORKSPACE;
    *hb = head_bufs(w, (char*)workspace);
    return OV_OK;
}
// A head past its pooling, for both encoders: LayerNorm of the pooled rows hb.rows (of rows_dtype; -1: hb.ln is filled already)
// -> @ proj_t [EP, D] (-> F.normalize) -> features [B, E] fp32
int head_finish(const ov_tower_cfg& c, const float* ln_w, const float* ln_b, const ov_bf16* proj_t, int E, int EP, const HeadBufs& hb,
                int rows_dtype, int B, float* features, int normalize, ov_stream_t stream) {
    const int D = c.width;
    int rc;
    if (rows_dtype >= 0 && (rc = ov_layernorm(hb.rows, rows_dtype, D, ln_w, ln_b, hb.ln, OV_BF16, D, B, D, c.ln_eps, stream))) return rc;
    if ((rc = ov_gemm(hb.ln, D, proj_t, D, nullptr, hb.feat, EP, B, EP, D, OV_EPI_BIAS, nullptr, 0, 0, 0, 0, stream))) return rc;
    if (normalize) return ov_l2norm(hb.feat, OV_BF16, EP, features, E, B, E, stream);
    return ov_convert(hb.feat, OV_BF16, EP, features, OV_F32, E, B, E, stream);
}
inline int vision_head_finish(const ov_tower* t, const ov_vision_head* h, const HeadBufs& hb, bool pooled, int B, float* features,
                              int normalize, ov_stream_t stream) {
    return head_finish(t->cfg, h->ln_post_w, h->ln_post_b, h->proj_t, h->embed_dim, h->embed_pad, hb, pooled ? OV_F32 : -1, B, features,
                       normalize, stream);
}
}  // namespace

extern "C" int ov_vision_head_forward(const ov_tower* t, const ov_vision_head* h, const ov_bf16* x, int B, float* features,
                                      int normalize, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !h || !x || !features || !workspace || B <= 0 || h->patch_size <= 0) return OV_ERR_INVALID;
    const int g = h->image_size / h->patch_size;
    return ov_vision_head_forward_tokens(t, h, x, B, g * g + 1, features, normalize, workspace, workspace_bytes, stream);
}

extern "C" int ov_vision_head_forward_tokens(const ov_tower* t, const ov_vision_head* h, const ov_bf16* x, int B, int L, float* features,
                                             int normalize, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !h || !x || !features || !workspace || B <= 0 || L < 2) return OV_ERR_INVALID;
    const int D = t->cfg.width;
    HeadBufs hb;
    int rc;
    if ((rc = vision_head_bufs(t, h, B, workspace, workspace_bytes, &hb))) return rc;
    if (h->pool_avg) {
        if ((rc = ov_mean_pool(x, D, (float*)hb.rows, B, L, D, 1, stream))) return rc;
    } else {
        if ((rc = ov_layernorm(x, OV_BF16, (int64_t)L * D, h->ln_post_w, h->ln_post_b, hb.ln, OV_BF16, D, B, D, t->cfg.ln_eps, stream)))
            return rc;
    }
    return vision_head_finish(t, h, hb, h->pool_avg != 0, B, features, normalize, stream);
}

// OVHIP_LAST_BLOCK_FULL=1: ov_encode_image / ov_encode_text run the last block in full, as ov_tower_forward does (A/B and tests).
static inline bool last_block_full() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("OVHIP_LAST_BLOCK_FULL"); v = (e && e[0] == '1') ? 1 : 0; }
    return v != 0;
}

// The embedding, the blocks and the head of ov_encode_image (K = 0) / ov_encode_image_keep (K kept patches) in the workspace ws.
// avg pooling reads the last block's output through its mean over the patch tokens alone, and the mean commutes with c_proj: the last
// block stops after c_fc, and ov_mlp_out_pooled forms mean(x1) + mean(hidden) . W2^T + b in fp32 on B rows (the pooled hidden in the
// tower workspace's h region, free once c_fc has run) -- closer to the unrounded mean than the mean of L bf16-rounded token rows.
// bf16 towers under pool -> LN; everything else runs the full block.  So does a call that drops patches (the training-mode forward):
// its pooled output stays bitwise what the head makes of the token stream (output_tokens).  K = G drops nothing and is ov_encode_image
// on reordered patches: it takes that entry point's tail.
static int encode_image(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, const int* keep, int B, int K,
                        float* features, int normalize, int* err_flag, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    const EncoderWs w = vision_ws(t, h, B, K);
    if (workspace_bytes < w.total) return OV_ERR_WORKSPACE;
    const ov_tower_cfg& c = t->cfg;
    const int g = h->image_size / h->patch_size, L = (K ? K : g * g) + 1, D = c.width, F = c.mlp_pad;
    char *ws = (char*)workspace, *tower = ws + w.tower, *head = ws + w.head;
    const size_t tower_bytes = w.head - w.tower, head_bytes = w.total - w.head;
    ov_bf16* x = (ov_bf16*)(ws + w.x);
    int rc;
    // the embedding's buffers alias the (not yet used) tower workspace
    rc = K ? ov_vision_embed_keep(t, h, image, img_dtype, keep, B, K, x, err_flag, tower, tower_bytes, stream)
           : ov_vision_embed(t, h, image, img_dtype, B, x, tower, tower_bytes, stream);
    if (rc) return rc;
    const TowerWs tw = tower_ws(t, B, L);
    const size_t h_bytes = tw.big - tw.h;
    const bool pooled_tail = (K == 0 || K == g * g) && !last_block_full() && h->pool_avg && h->final_ln_after_pool && L >= 2 && !tw.fp8 &&
                             F % 32 == 0 && ov_mlp_out_pooled_workspace_bytes(B, F) <= h_bytes;
    if (!pooled_tail) {
        if ((rc = ov_tower_forward(t, x, B, L, tower, tower_bytes, stream))) return rc;
        return ov_vision_head_forward_tokens(t, h, x, B, L, features, normalize, head, head_bytes, stream);
    }
    HeadBufs hb;
    if ((rc = vision_head_bufs(t, h, B, head, head_bytes, &hb))) return rc;
    if ((rc = tower_walk(t, x, B, L, tower, tower_bytes, stream, BLOCK_PAST_FC))) return rc;
    const ov_block_weights& lw = t->blocks[c.layers - 1];
    {   // in-situ profile: the pooled c_proj counts as the c_proj class, with the B rows it produces
        ProfScope ps(OV_PROF_GEMM_PROJ, stream, B);
        rc = ov_mlp_out_pooled(x, D, (const ov_bf16*)(tower + tw.big), tw.ldb, lw.proj_w, F, lw.proj_b, (float*)hb.rows, B, L, D, F, 1,
                               tower + tw.h, h_bytes, stream);
    }
    if (rc) return rc;
    return vision_head_finish(t, h, hb, true, B, features, normalize, stream);
}

extern "C" int ov_encode_image(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, int B,
                               float* features, int normalize, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !h || !image || !features || !workspace || B <= 0) return OV_ERR_INVALID;
    return encode_image(t, h, image, img_dtype, nullptr, B, 0, features, normalize, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int ov_encode_image_keep(const ov_tower* t, const ov_vision_head* h, const void* image, int img_dtype, const int* keep, int B,
                                    int K, float* features, int normalize, int* err_flag, void* workspace, size_t workspace_bytes,
                                    ov_stream_t stream) {
    if (!t || !h || !image || !keep || !features || !workspace || B <= 0 || K < 1 || !grid_ok(h, K)) return OV_ERR_INVALID;
    return encode_image(t, h, image, img_dtype, keep, B, K, features, normalize, err_flag, workspace, workspace_bytes, stream);
}

extern "C" size_t ov_text_workspace_bytes(const ov_tower* t, const ov_text_head* h, int B) {
    if (!t || !h || B <= 0 || h->pool_last < OV_TEXT_POOL_FIRST || h->pool_last > OV_TEXT_POOL_ARGMAX) return 0;
    return text_ws(t, h, B).total;
}

extern "C" int ov_encode_text(const ov_tower* t, const ov_text_head* h, const int64_t* tokens, int B, float* features,
                              int normalize, int* err_flag, void* workspace, size_t workspace_bytes, ov_stream_t stream) {
    if (!t || !h || !tokens || !features || !workspace || B <= 0) return OV_ERR_INVALID;
    if (h->pool_last < OV_TEXT_POOL_FIRST || h->pool_last > OV_TEXT_POOL_ARGMAX) return OV_ERR_INVALID;
    const TextWs w = text_ws(t, h, B);
    if (workspace_bytes < w.total) return OV_ERR_WORKSPACE;
    const ov_tower_cfg& c = t->cfg;
    const int T = h->context_length, D = c.width;
    char *ws = (char*)workspace, *tower = ws + w.tower;
    const size_t tower_bytes = w.head - w.tower;
    ov_bf16* x = (ov_bf16*)(ws + w.x);
    const HeadBufs hb = head_bufs(text_head_ws(t, h, B), ws + w.head);
    ov_bf16* last = (ov_bf16*)hb.rows;                            // the pooled row of each caption
    int rc;
    if ((rc = ov_text_embed(tokens, h->token_embedding, h->pos, x, D, B, T, D, h->vocab_size, err_flag, stream))) return rc;
    // the pooled row: one fixed position, or ('argmax') each caption's own, found once on the device
    const int row = h->pool_last == OV_TEXT_POOL_LAST ? T - 1 : 0;
    const int* idx = nullptr;
    if (h->pool_last == OV_TEXT_POOL_ARGMAX) {
        if ((rc = ov_token_argmax(tokens, (int*)(ws + w.idx), B, T, stream))) return rc;
        idx = (const int*)(ws + w.idx);
    }
    const auto gather = [&](const ov_bf16* src, ov_bf16* dst) {
        return idx ? ov_gather_rows_at(src, D, idx, dst, D, B, T, D, stream) : ov_gather_rows(src, D, dst, D, B, T, row, D, stream);
    };
    const TowerWs tw = tower_ws(t, B, T);
    const TextTailWs tail = text_tail_ws(c, B);
    if (last_block_full() || tw.fp8 || !text_tail_fits(tail, tw)) {
        if ((rc = ov_tower_forward(t, x, B, T, tower, tower_bytes, stream))) return rc;
        // ln_final is per-token, so only the pooled row needs it (model.py:276-277)
        if ((rc = gather(x, last))) return rc;
    } else {
        // Past the last block's attention only the pooled row of each caption is read: the rest of that block is run_block from past the
        // attention on the B gathered rows as one "image" of L = 1 (same GEMM entry points, and a GEMM row does not depend on the kernel
        // form that computes it).  In-situ profile: each launch under its class in the full block, with its B rows.
        if ((rc = tower_walk(t, x, B, T, tower, tower_bytes, stream, BLOCK_PAST_ATTN))) return rc;
        char* big = tower + tw.big;
        ov_bf16* a = (ov_bf16*)(big + tail.a);
        if ((rc = gather((const ov_bf16*)(tower + tw.h), a))) return rc;
        if ((rc = gather(x, last))) return rc;
        const BlockPart rows = {last, a, (ov_bf16*)(big + tail.hid), c.mlp_pad, (float*)(big + tail.stats), nullptr, nullptr, nullptr, B,
                                stream, true};
        if ((rc = run_block(c, t->blocks[c.layers - 1], nullptr, 0, Fp8Scales{nullptr, nullptr, nullptr, nullptr, 0}, rows, false, 1,
                            t->prefix, {BLOCK_PAST_ATTN, BLOCK_END})))
            return rc;
    }
    return head_finish(c, h->ln_final_w, h->ln_final_b, h->proj_t, h->embed_dim, text_embed_pad(h), hb, OV_BF16, B, features, normalize,
                       stream);
}

