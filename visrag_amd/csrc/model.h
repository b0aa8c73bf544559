// The VisRAG-Ret encoder's model handle (vr_model_s) and what the translation units around it share: model.hip (weights,
// derived tables, workspace, taps, profile), encode.hip (the encode pass), chat.hip (answer generation on the same weights).
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "engine_common.h"

struct VitBlock {
    Vec n1w, n1b, n2w, n2b; Linear qkv, proj, fc1, fc2;
};
struct DecLayer {
    Vec ln1, ln2; Linear qkv, o, gu, down; int parts_qkv = 0, parts_gu = 0;
    Linear qkv_lo, o_lo, gu_lo, down_lo;     // w - bf16(w) of fp32 source weights: the split-precision text path (hp_text.hip)
};

struct GridTables {
    int gh = 0, gw = 0;
    DevBuf vit_pos;        // f32 [N][Dp]  : bicubic-antialias resample of vpm.pos_embed
    DevBuf pos_k;          // f32 [N][E]   : sincos2d(N,E) @ Wk^T (the k-side position term)
};

struct Tap { std::vector<float> data; int64_t rows = 0, cols = 0; };

struct vr_model_s {
    int device = 0;
    vr_config_t c{};
    bool finalized = false, taps_on = false;
    int pool_mode = 0;                        // VR_POOL_*
    bool borrowed = false;                    // vr_model_clone: weights belong to another handle
    // dims
    int D = 0, Dp = 0, F = 0, Fp = 0, E = 0, I = 0, Ip = 0, Kpe = 0, Kpe_p = 0, Q = 0;
    // weights
    Linear patch;
    std::vector<float> pos_embed_host;       // [G*G][D]
    std::vector<VitBlock> blocks;
    Vec vit_nw, vit_nb;
    Linear r_kvproj, r_kv, r_out, r_proj;    // r_kv = in_proj rows [E,3E) (k|v)
    Vec r_lnq_w, r_lnq_b, r_lnkv_w, r_lnkv_b, r_lnpost_w, r_lnpost_b;
    std::vector<float> r_query_host, r_wq_host, r_bq_host;   // for the one-time q projection
    bool has_query = false, has_inproj = false, has_inproj_b = false, has_pos = false;
    DevBuf r_q;                               // bf16 [64][E] projected queries
    DevBuf embed;  bool has_embed = false;    // bf16 [V][E]
    DevBuf embed_lo; bool has_embed_lo = false;   // its low half (fp32 source, split-precision text path)
    std::vector<DecLayer> layers;
    Vec final_norm;
    DevBuf rope;                              // f32 [max_pos][64]
    int rope_len = 0;
    std::map<std::pair<int, int>, GridTables> grids;
    // workspace
    int64_t Mcap = 0, Tcap = 0, Rcap = 0;     // padded rows: patches, tokens, resampler rows
    DevBuf w_hvit, w_xn, w_qkv, w_att, w_mlp, w_kv32, w_xkv, w_KV, w_ratt, w_rout, w_rln;
    DevBuf w_h, w_dxn, w_dqkv, w_datt, w_dact, w_part;   // w_part: split-K partial products [3][T][E] f32
    DevBuf w_cu, w_ids, w_seq, w_pos, w_rowmap, w_imgptr, w_pix, w_out;
    DevBuf w_hp_hi, w_hp_planes, w_hp_qkv, w_hp_att, w_hp_gu, w_seqof;   // split-precision text path (hp_text.hip)
    DevBuf w_hp_part;                                                 // its split-K planes for short batches (grown on demand)
    DevBuf w_hidden;                                                  // vr_encode_hidden: packed post-norm rows when the resampler's scratch is too small (grown on demand)
    std::map<std::string, Tap> taps;
    // HIP-event profiling of kernel classes (bench.py roofline): pairs recorded on the launch
    // stream, elapsed times summed lazily in vr_model_get_profile
    bool prof_on = false;
    int prof_level = 0;                       // 1: the seven phase classes; 2: the decoder's sub-phases instead (events between its kernels)
    struct ProfClass { std::vector<hipEvent_t> ev; size_t used = 0; double ms = 0, flops = 0; int64_t launches = 0; };
    ProfClass prof[VR_PROF_CLASSES];
    // pinned host arena for the small per-call arrays (ids, offsets, row maps, image pointers):
    // async H2D copies read it after vr_encode returned, `arena_ev` marks when they have run.
    char* arena = nullptr; size_t arena_cap = 0, arena_used = 0;
    hipEvent_t arena_ev = nullptr; bool arena_pending = false, arena_open = false;
};

static inline int arena_begin(vr_model_s* m, size_t need) {
    if (m->arena_pending) { HIPCHK(hipEventSynchronize(m->arena_ev)); m->arena_pending = false; }
    if (!m->arena_ev) HIPCHK(hipEventCreateWithFlags(&m->arena_ev, hipEventDisableTiming));
    if (m->arena_cap < need) {
        if (m->arena) (void)hipHostFree(m->arena);
        m->arena = nullptr; m->arena_cap = 0;
        const size_t cap = std::max(need, (size_t)4 << 20);
        HIPCHK(hipHostMalloc((void**)&m->arena, cap, hipHostMallocDefault));
        m->arena_cap = cap;
    }
    m->arena_used = 0;
    m->arena_open = true;        // async copies may read the arena from here on (see vr_encode)
    return VR_OK;
}
// End of an encode call: the pinned arena feeds async H2D copies, so on EVERY exit after the first of them (a failure in the
// middle of the call included) mark when they have run, or the next call would overwrite the arena under pending copies.
static inline void arena_close(vr_model_s* m, void* stream) {
    if (m->arena_open && m->arena_ev) {
        if (hipEventRecord(m->arena_ev, (hipStream_t)stream) == hipSuccess) m->arena_pending = true;
        else (void)hipStreamSynchronize((hipStream_t)stream);
    }
    m->arena_open = false;
}
static inline void* arena_take(vr_model_s* m, size_t bytes) {
    void* p = m->arena + m->arena_used;
    m->arena_used += (bytes + 63) / 64 * 64;
    return p;
}

static inline int prof_begin(vr_model_s* m, int cls, hipStream_t s) {
    if (!m->prof_on || (cls >= VR_PROF_DEC_QKV) != (m->prof_level == 2)) return VR_OK;
    auto& p = m->prof[cls];
    if (p.used + 2 > p.ev.size()) {
        for (int i = 0; i < 64; ++i) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); p.ev.push_back(e); }
    }
    HIPCHK(hipEventRecord(p.ev[p.used], s));
    return VR_OK;
}
static inline int prof_end(vr_model_s* m, int cls, double flops, hipStream_t s) {
    if (!m->prof_on || (cls >= VR_PROF_DEC_QKV) != (m->prof_level == 2)) return VR_OK;
    auto& p = m->prof[cls];
    HIPCHK(hipEventRecord(p.ev[p.used + 1], s));
    p.used += 2; p.launches += 1; p.flops += flops;
    return VR_OK;
}
static inline int prof_collect(vr_model_s* m) {
    HIPCHK(hipDeviceSynchronize());
    for (auto& p : m->prof) {
        for (size_t i = 0; i + 1 < p.used; i += 2) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]));
            p.ms += ms;
        }
        p.used = 0;
    }
    return VR_OK;
}

constexpr int DEC_KSPLIT_MAX = 3;   // decoder o / down projections: split-K factor when the tile grid is small

static inline GemmArgs gemm_args(const void* A, int lda, const Linear& L, int M, void* out, int ldo) {
    GemmArgs a{};
    a.A = A; a.lda = lda; a.W = L.w.p; a.ldw = L.k_pad; a.M = M; a.N = L.n_pad; a.K = L.k_pad;
    a.bias = L.has_b ? L.b.as<float>() : nullptr;
    a.out = out; a.ldo = ldo; a.alpha = 1.0f;
    return a;
}

// encode_impl's optional per-call extras (vr_chat_prefill): `bf16_route` keeps a token-only batch off the split-precision
// text route; `layer` (when set) runs after every decoder layer's q|k|v projection + RoPE with the layer's bf16 rows
// [T][ldqkv] (q | k | v) on the launch stream.  A null hook is the plain vr_encode pass.
// vr_chat_extend's extras (each absent when null; a hook that sets none of them launches what a hook without them launches):
// `base_pos` (host, [B]): token j of sequence b sits at position base_pos[b] + j instead of j; `rope_table` / `rope_len`: the
// RoPE table those positions index (f32 [rope_len][64]) instead of the model's; `attn` replaces the layer's launch_attention:
// it reads the q columns of qkv (and whatever `layer` stored) and writes bf16 out [T][ldo].
struct EncodeHook {
    bool bf16_route = false;
    int (*layer)(void* ctx, int l, const void* qkv, int ldqkv, int T, hipStream_t s) = nullptr;
    void* ctx = nullptr;
    const int32_t* base_pos = nullptr;
    const float* rope_table = nullptr;
    int rope_len = 0;
    int (*attn)(void* ctx, int l, const void* qkv, int ldqkv, int T, void* out, int ldo, hipStream_t s) = nullptr;
};

// ---- defined in model.hip
// RoPE table [pos][cos 32 | sin 32], fp32, `len` positions (modeling_minicpm.py:142-172)
std::vector<float> rope_table_host(float theta, int len);
// per-grid constants: resampled ViT pos-embed and the k-side position term of the resampler
int get_grid(vr_model_s* m, int gh, int gw, GridTables** out);
int tap_store(vr_model_s* m, const char* name, const void* dev, int64_t rows, int64_t cols, int64_t ld, bool is_bf16, hipStream_t s);
// ---- defined in encode.hip
int encode_impl(vr_model_t m, const uint8_t* const* slices, const int32_t* slice_hw, int32_t n_slices,
                int32_t slices_on_device, const int32_t* input_ids, const int32_t* seq_offsets, int32_t B,
                const int32_t* vision_rows, float* out_reps, int32_t out_on_device, void* stream,
                float* out_hidden = nullptr, int32_t hidden_len = 0, const EncodeHook* hook = nullptr);
