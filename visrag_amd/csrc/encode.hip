// The launch sequence of one VisRAG-Ret encode pass (vr_encode / vr_encode_hidden of include/visrag_hip.h) on the model
// handle of model.h.
// Reference call stack this replaces: SURVEY.md section 3.1 (modeling_visrag_ret.py:86-126 ->
// modeling_minicpmv.py:95-171 -> vision_transformer.py:682-692 / resampler.py:146-168 ->
// modeling_minicpm.py:1147-1304 -> dense_retrieval_model.py:180-184,222-223).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "model.h"

// -------------------------------------------------------------------------------- encode ---
// ViT + resampler for `n` same-shape slices; writes resampler rows into the decoder stream.
static int run_vision_group(vr_model_s* m, const uint8_t* const* dev_imgs_hostarray, int n, int H, int W,
                            const int32_t* rowmap_host /* [n*Q] */, bool first_group, hipStream_t s) {
    const vr_config_t& c = m->c;
    const int P = c.patch_size, gh = H / P, gw = W / P, N = gh * gw;
    const int D = m->D, Dp = m->Dp, E = m->E, Q = m->Q;
    const int M = n * N;
    GridTables* g = nullptr;
    VRCHK(get_grid(m, gh, gw, &g));

    // dev_imgs_hostarray / rowmap_host live in the pinned arena (see vr_encode)
    HIPCHK(hipMemcpyAsync(m->w_imgptr.p, dev_imgs_hostarray, (size_t)n * 8, hipMemcpyHostToDevice, s));
    int* cu = (int*)arena_take(m, (size_t)2 * (n + 1) * 4);
    for (int i = 0; i <= n; ++i) { cu[i] = i * N; cu[n + 1 + i] = i * Q; }
    HIPCHK(hipMemcpyAsync(m->w_cu.p, cu, (size_t)2 * (n + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m->w_rowmap.p, rowmap_host, (size_t)n * Q * 4, hipMemcpyHostToDevice, s));
    const int* cu_tok = m->w_cu.as<int>();
    const int* cu_qry = m->w_cu.as<int>() + (n + 1);

    float* h = m->w_hvit.as<float>();
    // K1+K2+K3: normalise + patch tiles built in LDS + conv-as-GEMM + bias + resampled pos-embed -> fp32 residual stream
    {
        GemmArgs a = gemm_args(nullptr, 0, m->patch, M, h, Dp);
        a.rowbias = g->vit_pos.as<float>(); a.rowbias_period = N; a.rowbias_ld = Dp; a.rowbias_cols = Dp;
        HIPCHK(launch_patch_embed((const uint8_t* const*)m->w_imgptr.p, n, H, W, P, a, m->Kpe, s));
    }
    if (first_group) VRCHK(tap_store(m, "vit_embed", h, N, D, Dp, false, s));
    const int ldqkv = pad128(3 * D);
    // (the plain bf16 epilogue scales whole 64-column blocks: the q section must end on one, as 16 x 72 does)
    // NOTE for any other reader of w_qkv: its q columns hold q * head_dim^-0.5 * log2(e), not q (AttnArgs::q_prescaled)
    const int vit_hd = c.vit_dim / c.vit_heads;                          // (72: checked at vr_model_create)
    const int vit_qscale_n = D % 64 == 0 ? D : 0;
    const float vit_qscale = (1.0f / sqrtf((float)vit_hd)) * 1.44269504088896340736f;
    for (int l = 0; l < c.vit_depth; ++l) {
        const VitBlock& b = m->blocks[l];
        HIPCHK(launch_layernorm(h, M, D, Dp, b.n1w.v.as<float>(), b.n1b.v.as<float>(), c.vit_ln_eps, m->w_xn.p, Dp, s));
        VRCHK(prof_begin(m, VR_PROF_VIT_QKV, s));
        {
            // the q columns leave with head_dim^-0.5 * log2(e) folded in before their one bf16 rounding (attention_w.hip starts its
            // score accumulators at -m and feeds them to v_exp_f32 as they come out)
            GemmArgs a = gemm_args(m->w_xn.p, Dp, b.qkv, M, m->w_qkv.p, ldqkv);
            a.col_scale = vit_qscale; a.col_scale_n = vit_qscale_n;
            HIPCHK(launch_gemm(a, EPI_BF16, GEMM_VARIANT_AUTO, s));
        }
        VRCHK(prof_end(m, VR_PROF_VIT_QKV, 2.0 * M * D * 3 * D, s));
        {
            AttnArgs a{};
            a.q = m->w_qkv.p; a.ldq = ldqkv;
            a.k = (const char*)m->w_qkv.p + (size_t)D * 2; a.ldk = ldqkv;
            a.v = (const char*)m->w_qkv.p + (size_t)2 * D * 2; a.ldv = ldqkv;
            a.out = m->w_att.p; a.ldo = Dp; a.cu_q = cu_tok; a.cu_kv = cu_tok; a.B = n; a.heads = c.vit_heads;
            a.head_dim = vit_hd; a.max_q = N; a.causal = 0; a.q_shared = 0; a.scale = 1.0f / sqrtf((float)vit_hd); a.q_prescaled = vit_qscale_n > 0;
            VRCHK(prof_begin(m, VR_PROF_VIT_ATTN, s));
            HIPCHK(launch_attention(a, s));
            VRCHK(prof_end(m, VR_PROF_VIT_ATTN, 4.0 * n * (double)N * N * D, s));
        }
        VRCHK(prof_begin(m, VR_PROF_VIT_PROJ, s));
        {
            GemmArgs a = gemm_args(m->w_att.p, Dp, b.proj, M, h, Dp); a.resid = h;
            HIPCHK(launch_gemm(a, EPI_RESID, GEMM_VARIANT_AUTO, s));
        }
        VRCHK(prof_end(m, VR_PROF_VIT_PROJ, 2.0 * M * D * D, s));
        HIPCHK(launch_layernorm(h, M, D, Dp, b.n2w.v.as<float>(), b.n2b.v.as<float>(), c.vit_ln_eps, m->w_xn.p, Dp, s));
        VRCHK(prof_begin(m, VR_PROF_VIT_FC1, s));
        { GemmArgs a = gemm_args(m->w_xn.p, Dp, b.fc1, M, m->w_mlp.p, m->Fp); HIPCHK(launch_gemm(a, EPI_GELU, GEMM_VARIANT_AUTO, s)); }
        VRCHK(prof_end(m, VR_PROF_VIT_FC1, 2.0 * M * D * m->F, s));
        VRCHK(prof_begin(m, VR_PROF_VIT_FC2, s));
        {
            GemmArgs a = gemm_args(m->w_mlp.p, m->Fp, b.fc2, M, h, Dp); a.resid = h;
            HIPCHK(launch_gemm(a, EPI_RESID, GEMM_VARIANT_AUTO, s));
        }
        VRCHK(prof_end(m, VR_PROF_VIT_FC2, 2.0 * M * D * m->F, s));
        if (l == 0 && first_group) VRCHK(tap_store(m, "vit_block0", h, N, D, Dp, false, s));
    }
    HIPCHK(launch_layernorm(h, M, D, Dp, m->vit_nw.v.as<float>(), m->vit_nb.v.as<float>(), c.vit_ln_eps, m->w_xn.p, Dp, s));
    if (first_group) VRCHK(tap_store(m, "vit_out", m->w_xn.p, N, D, Dp, true, s));

    // ---- resampler (resampler.py:146-168)
    VRCHK(prof_begin(m, VR_PROF_RESAMPLER, s));
    { GemmArgs a = gemm_args(m->w_xn.p, Dp, m->r_kvproj, M, m->w_kv32.p, E); HIPCHK(launch_gemm(a, EPI_F32, GEMM_VARIANT_AUTO, s)); }
    HIPCHK(launch_layernorm(m->w_kv32.as<float>(), M, E, E, m->r_lnkv_w.v.as<float>(), m->r_lnkv_b.v.as<float>(),
                            c.resampler_ln_eps, m->w_xkv.p, E, s));
    {   // fused k|v in-projection; the k half gets the per-position term pos_k[row % N]
        GemmArgs a = gemm_args(m->w_xkv.p, E, m->r_kv, M, m->w_KV.p, 2 * E);
        a.rowbias = g->pos_k.as<float>(); a.rowbias_period = N; a.rowbias_ld = E; a.rowbias_cols = E;
        HIPCHK(launch_gemm(a, EPI_BF16, GEMM_VARIANT_AUTO, s));
    }
    {
        AttnArgs a{};
        a.q = m->r_q.p; a.ldq = E; a.k = m->w_KV.p; a.ldk = 2 * E; a.v = (const char*)m->w_KV.p + (size_t)E * 2; a.ldv = 2 * E;
        a.out = m->w_ratt.p; a.ldo = E; a.cu_q = cu_qry; a.cu_kv = cu_tok; a.B = n; a.heads = E / 128; a.head_dim = 128;
        a.max_q = Q; a.causal = 0; a.q_shared = 1; a.scale = 1.0f / sqrtf(128.0f);
        HIPCHK(launch_attention(a, s));
    }
    const int R = n * Q;
    { GemmArgs a = gemm_args(m->w_ratt.p, E, m->r_out, R, m->w_rout.p, E); HIPCHK(launch_gemm(a, EPI_F32, GEMM_VARIANT_AUTO, s)); }
    HIPCHK(launch_layernorm(m->w_rout.as<float>(), R, E, E, m->r_lnpost_w.v.as<float>(), m->r_lnpost_b.v.as<float>(),
                            c.resampler_ln_eps, m->w_rln.p, E, s));
    if (first_group && m->taps_on) {   // un-scattered copy for the tap
        GemmArgs a = gemm_args(m->w_rln.p, E, m->r_proj, Q, m->w_rout.p, E);
        HIPCHK(launch_gemm(a, EPI_F32, GEMM_VARIANT_AUTO, s));
        VRCHK(tap_store(m, "resampler_out", m->w_rout.p, Q, E, E, false, s));
    }
    {   // x @ proj, scattered straight into the decoder's fp32 input rows (image_bound scatter_,
        // modeling_minicpmv.py:148-166; vision rows are NOT scaled by scale_emb)
        GemmArgs a = gemm_args(m->w_rln.p, E, m->r_proj, R, m->w_h.p, E);
        a.rowmap = m->w_rowmap.as<int>();
        HIPCHK(launch_gemm(a, EPI_F32, GEMM_VARIANT_AUTO, s));
    }
    VRCHK(prof_end(m, VR_PROF_RESAMPLER, 2.0 * M * D * E + 4.0 * M * E * (double)E + 4.0 * R * (double)N * E + 4.0 * R * E * (double)E, s));
    return VR_OK;
}

// ---- the decoder pass of a token-only batch at fp32-class precision (hp_text.hip) -----------------------------
// out (+)= alpha * A W^T with A = hi + lo (bf16 halves a_hi / a_lo, row pitch lda: w_hp_hi holds [hi rows | lo rows]) and W = L (+ Llo):
// A_hi W_hi, then A_lo W_hi and A_hi W_lo added in place by the residual epilogue of the same MFMA kernels.
static int hp_gemm_tiles(vr_model_s* m, const void* a_hi, const void* a_lo, const Linear& L, const Linear& Llo, int lda, int T, float* out,
                         int ldo, bool into_resid, float alpha, hipStream_t s) {
    // Round 4: the hi and lo halves of A are the ROWS of one GEMM — the lo rows are laid out right behind the T hi rows
    // (run_decoder_hp) — so W_hi is streamed once, M = 2 T rows fill the 256-row tiles (T = 1300 for 64 queries ran 128 x 128
    // tiles at 257 TF as two launches with a read-modify-write epilogue), and one fixed-order sum closes the planes
    // [A_hi W_hi | A_lo W_hi | A_hi W_lo].  Falls back to the three in-place launches when the planes do not fit.
    const size_t plane = (size_t)T * L.n_pad;
    const int n_planes = Llo.has_w ? 3 : 2;
    // (a Linear with a bias — none in the MiniCPM decoder — keeps the three in-place launches, whose first one adds it once: the plane
    // sum has no bias term.  ADVICE r4)
    if (!L.has_b && (const char*)a_lo == (const char*)a_hi + (size_t)T * lda * 2 && m->w_hp_planes.reserve((size_t)n_planes * plane * 4) == VR_OK) {
        float* part = m->w_hp_planes.as<float>();
        {
            GemmArgs a = gemm_args(a_hi, lda, L, 2 * T, part, L.n_pad);
            a.bias = nullptr;
            HIPCHK(launch_gemm(a, EPI_F32, GEMM_VARIANT_AUTO, s));
        }
        if (Llo.has_w) {
            GemmArgs a = gemm_args(a_hi, lda, Llo, T, part + 2 * plane, L.n_pad);
            a.bias = nullptr;
            HIPCHK(launch_gemm(a, EPI_F32, GEMM_VARIANT_AUTO, s));
        }
        HIPCHK(launch_planes_sum(part, n_planes, plane, L.n_pad, T, std::min(L.n_pad, ldo), out, ldo, into_resid ? alpha : 1.0f, into_resid, s));
        return VR_OK;
    }
    {
        GemmArgs a = gemm_args(a_hi, lda, L, T, out, ldo);
        if (into_resid) { a.resid = out; a.alpha = alpha; }
        HIPCHK(launch_gemm(a, into_resid ? EPI_RESID : EPI_F32, GEMM_VARIANT_AUTO, s));
    }
    {
        GemmArgs a = gemm_args(a_lo, lda, L, T, out, ldo);
        a.bias = nullptr;                                   // (added by the launch above)
        a.resid = out; a.alpha = into_resid ? alpha : 1.0f;
        HIPCHK(launch_gemm(a, EPI_RESID, GEMM_VARIANT_AUTO, s));
    }
    if (Llo.has_w) {
        GemmArgs a = gemm_args(a_hi, lda, Llo, T, out, ldo);
        a.bias = nullptr;
        a.resid = out; a.alpha = into_resid ? alpha : 1.0f;
        HIPCHK(launch_gemm(a, EPI_RESID, GEMM_VARIANT_AUTO, s));
    }
    return VR_OK;
}

// The same product for a SHORT batch (T <= 32 rows: one query, a few queries): the tile GEMMs above run a 128-row tile with
// a row in five real and stream a projection's weights through ~50 workgroups (0.55 TB/s: 20 ms for one query, 11 GB of
// weights).  Here every pass is ONE launch of the weight streamer (gemm_skinny.hip, 4-6 TB/s) writing fp32 split-K planes —
// A_hi W_hi | A_lo W_hi | A_hi W_lo into consecutive plane groups — and one launch sums them (fixed order) into `out`.
static int hp_gemm_stream(vr_model_s* m, const void* a_hi, const void* a_lo, const Linear& L, const Linear& Llo, int lda, int T, float* out,
                          int ldo, bool into_resid, float alpha, hipStream_t s) {
    const int ks = stream_ksplit(L.n_pad, L.k_pad);
    const size_t plane = (size_t)T * L.n_pad;
    const int n_pass = Llo.has_w ? 3 : 2;
    if ((size_t)n_pass * ks * plane * 4 > m->w_hp_part.bytes) return fail(VR_ERR_CAPACITY, "split-K planes exceed the workspace");
    float* part = m->w_hp_part.as<float>();
    for (int pass = 0; pass < n_pass; ++pass) {
        GemmArgs a = gemm_args(pass == 1 ? a_lo : a_hi, lda, pass == 2 ? Llo : L, T, part + (size_t)pass * ks * plane, L.n_pad);
        a.bias = nullptr;
        a.ksplit = ks; a.split_stride = plane;
        HIPCHK(launch_gemm_skinny(a, s));
    }
    HIPCHK(launch_planes_sum(part, n_pass * ks, plane, L.n_pad, T, std::min(L.n_pad, ldo), out, ldo, into_resid ? alpha : 1.0f, into_resid, s));
    return VR_OK;
}
static bool hp_stream_ok(const vr_model_s* m, int T) {
    if (T > 32) return false;
    for (const DecLayer& L : m->layers)
        for (const Linear* l : {&L.qkv, &L.o, &L.gu, &L.down})
            if (l->n_pad % 256 || l->k_pad % 64 || l->has_b) return false;     // 256-column tiles of the streamer; no bias in this decoder
    return true;
}

static int run_decoder_hp(vr_model_s* m, int T, int B, int max_len, hipStream_t s) {
    (void)max_len;
    const vr_config_t& c = m->c;
    const int E = m->E, I = m->I, Ip = m->Ip;
    float* h = m->w_h.as<float>();
    float* qkv = m->w_hp_qkv.as<float>();
    float* att = m->w_hp_att.as<float>();
    float* gu = m->w_hp_gu.as<float>();
    const int ld_gu = pad128(2 * I);
    HIPCHK(launch_seq_of(m->w_seq.as<int>(), B, m->w_seqof.as<int>(), s));
    const bool stream = hp_stream_ok(m, T);
    void* const hi = m->w_hp_hi.p;
    auto lo = [&](int lda) -> void* { return (char*)hi + (size_t)T * lda * 2; };     // the lo rows: right behind the T hi rows
    auto hp_gemm = [&](vr_model_s* mm, const Linear& L, const Linear& Llo, int lda, int TT, float* out, int ldo, bool into_resid,
                       float alpha, hipStream_t ss) -> int {
        return stream ? hp_gemm_stream(mm, hi, lo(lda), L, Llo, lda, TT, out, ldo, into_resid, alpha, ss)
                      : hp_gemm_tiles(mm, hi, lo(lda), L, Llo, lda, TT, out, ldo, into_resid, alpha, ss);
    };
    for (int l = 0; l < c.num_layers; ++l) {
        const DecLayer& L = m->layers[l];
        HIPCHK(launch_rmsnorm_split(h, T, E, L.ln1.v.as<float>(), c.rms_norm_eps, hi, lo(E), s));
        VRCHK(hp_gemm(m, L.qkv, L.qkv_lo, E, T, qkv, 3 * E, false, 1.0f, s));
        HIPCHK(launch_rope_f32(qkv, T, 3 * E, 2 * E, m->w_pos.as<int>(), m->rope.as<float>(), s));
        HIPCHK(launch_attn_f32(qkv, 3 * E, E, m->w_seqof.as<int>(), m->w_seq.as<int>(), T, c.num_heads, 1.0f / sqrtf(64.0f), att, s));
        HIPCHK(launch_split_bf16(att, hi, lo(E), (size_t)T * E, s));
        VRCHK(hp_gemm(m, L.o, L.o_lo, E, T, h, E, true, c.residual_scale, s));
        HIPCHK(launch_rmsnorm_split(h, T, E, L.ln2.v.as<float>(), c.rms_norm_eps, hi, lo(E), s));
        VRCHK(hp_gemm(m, L.gu, L.gu_lo, E, T, gu, ld_gu, false, 1.0f, s));
        HIPCHK(launch_swiglu_split(gu, T, ld_gu, I, Ip, hi, lo(Ip), s));
        VRCHK(hp_gemm(m, L.down, L.down_lo, Ip, T, h, E, true, c.residual_scale, s));
        if (l == 0) VRCHK(tap_store(m, "dec_layer0", h, T, E, E, false, s));
    }
    return VR_OK;
}


// How the bf16 decoder runs its o / down projections (N = E) for a batch of T rows.  With few rows the 256^2 grid is far
// smaller than the chip (T = 2176: 81 tiles on 256 CUs; the 128^2 grid of 306 tiles runs 1.2 waves at 550-700 TF), so:
//   ks > 1       split K over `ks` workgroups per tile (243 workgroups); the fp32 partial products are summed, in a fixed
//                order, by the RMSNorm that follows anyway (launch_rmsnorm_accum), which also applies the scaled residual
//                update — no reduction pass, no atomics, deterministic.  `proj_variant` is the tile of those launches.
//   proj_128w    the FULL K per workgroup on the three-stage one-wave kernel (gemm128w.hip), added into the residual stream in
//                place: no fp32 planes, the RMSNorm behind them reads 20 MB instead of moving 88 (round 6)
//   neither      the plain residual epilogue
struct DecRoute { int ks; int proj_variant; bool proj_128w; };
static DecRoute dec_route(int T, int E, int Ip, bool taps_on) {
    DecRoute r{1, GEMM_VARIANT_256W, false};
    // 256 x 192 tiles when E allows (2304 = 12 x 192): 108 tiles x 2 splits = 216 workgroups write TWO partial
    // planes instead of 81 x 3 = 243 writing three — the fp32 partials (and their re-read by the RMSNorm that
    // sums them) are what these launches spend their epilogue on, at the HBM's pace
    const long t192 = (long)((T + 255) / 256) * (E / 192);
    if (E % 192 == 0 && t192 * 2 <= 256 && t192 * 2 > 160 && E % 128 == 0 && Ip % 128 == 0) {
        r.ks = 2;
        r.proj_variant = GEMM_VARIANT_192W;
    } else {
        const long tiles = (long)((T + 255) / 256) * ((E + 255) / 256);
        for (int cand = DEC_KSPLIT_MAX; cand > 1; --cand)
            if (tiles * cand <= 256 && E % (cand * 64) == 0 && Ip % (cand * 64) == 0) { r.ks = cand; break; }
    }
    if (taps_on) r.ks = 1;          // (taps read h between the projection and the next norm)
    // when half-height tiles fill one round of the chip (T = 2176: 17 x 12 = 204 workgroups of 128 x 192)
    const long t128 = (long)((T + 127) / 128) * (E / 192);
    r.proj_128w = E % 192 == 0 && t128 > 128 && t128 <= 256;
    if (r.proj_128w) r.ks = 1;
    return r;
}

extern "C" int vr_encode(vr_model_t m, const uint8_t* const* slices, const int32_t* slice_hw, int32_t n_slices,
                         int32_t slices_on_device, const int32_t* input_ids, const int32_t* seq_offsets, int32_t B,
                         const int32_t* vision_rows, float* out_reps, int32_t out_on_device, void* stream) {
    if (!m) return fail(VR_ERR_INVALID, "NULL model");
    m->arena_open = false;
    const int rc = encode_impl(m, slices, slice_hw, n_slices, slices_on_device, input_ids, seq_offsets, B, vision_rows,
                               out_reps, out_on_device, stream);
    arena_close(m, stream);
    return rc;
}

// The HF-style forward of the second caller (visrag_scripts/demo/visrag_pipeline/utils.py:12-32 pools `last_hidden_state` itself):
// the same pass, and the post-norm hidden states as a right-padded [B][hidden_len][hidden_size] fp32 device tensor.
extern "C" int vr_encode_hidden(vr_model_t m, const uint8_t* const* slices, const int32_t* slice_hw, int32_t n_slices,
                                int32_t slices_on_device, const int32_t* input_ids, const int32_t* seq_offsets, int32_t B,
                                const int32_t* vision_rows, float* out_reps, int32_t out_on_device, float* out_hidden,
                                int32_t hidden_len, void* stream) {
    if (!m) return fail(VR_ERR_INVALID, "NULL model");
    if (!out_hidden || hidden_len <= 0) return fail(VR_ERR_INVALID, "out_hidden is NULL or hidden_len <= 0");
    m->arena_open = false;
    const int rc = encode_impl(m, slices, slice_hw, n_slices, slices_on_device, input_ids, seq_offsets, B, vision_rows,
                               out_reps, out_on_device, stream, out_hidden, hidden_len);
    arena_close(m, stream);
    return rc;
}

int encode_impl(vr_model_t m, const uint8_t* const* slices, const int32_t* slice_hw, int32_t n_slices,
                int32_t slices_on_device, const int32_t* input_ids, const int32_t* seq_offsets, int32_t B,
                const int32_t* vision_rows, float* out_reps, int32_t out_on_device, void* stream,
                float* out_hidden, int32_t hidden_len, const EncodeHook* hook) {
    if (!m->finalized) return fail(VR_ERR_STATE, "vr_model_finalize() has not succeeded");
    if (B <= 0 || !input_ids || !seq_offsets || !out_reps) return fail(VR_ERR_INVALID, "empty batch or NULL argument");
    if (n_slices > 0 && (!slices || !slice_hw || !vision_rows)) return fail(VR_ERR_INVALID, "NULL slice arguments");
    VRCHK(set_dev(m->device));
    hipStream_t s = (hipStream_t)stream;
    const vr_config_t& c = m->c;
    const int E = m->E, Q = m->Q;
    const int T = seq_offsets[B];
    if (seq_offsets[0] != 0) return fail(VR_ERR_INVALID, "seq_offsets[0] must be 0");
    if (B > c.max_seqs) return fail(VR_ERR_CAPACITY, "B=%d exceeds max_seqs=%d", B, c.max_seqs);
    if (T > c.max_tokens) return fail(VR_ERR_CAPACITY, "T=%d tokens exceed max_tokens=%d", T, c.max_tokens);
    for (int i = 0; i < B; ++i)
        if (seq_offsets[i + 1] <= seq_offsets[i]) return fail(VR_ERR_INVALID, "empty sequence %d", i);
    for (int t = 0; t < T; ++t)
        if (input_ids[t] < 0 || input_ids[t] >= c.vocab_size) return fail(VR_ERR_INVALID, "token id %d out of range at %d", input_ids[t], t);
    for (int i = 0; i < n_slices * Q; ++i)
        if (vision_rows[i] >= T) return fail(VR_ERR_INVALID, "vision row %d out of range", vision_rows[i]);

    // ---- K13: token embeddings * scale_emb into the fp32 stream
    const int32_t* base_pos = hook ? hook->base_pos : nullptr;        // (vr_chat_extend: sequences that continue a cache)
    VRCHK(arena_begin(m, (size_t)T * 4 * (base_pos ? 2 : 1) + (size_t)(B + 1) * 4 + (size_t)n_slices * (Q * 4 + 8 + 64 * 3) + 4096));
    {
        int* a_ids = (int*)arena_take(m, (size_t)T * 4);
        int* a_seq = (int*)arena_take(m, (size_t)(B + 1) * 4);
        memcpy(a_ids, input_ids, (size_t)T * 4);
        memcpy(a_seq, seq_offsets, (size_t)(B + 1) * 4);
        HIPCHK(hipMemcpyAsync(m->w_ids.p, a_ids, (size_t)T * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(m->w_seq.p, a_seq, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, s));
    }
    // token-only batches (queries, text passages) take the split-precision decoder pass (hp_text.hip).
    // text_split_precision: 0 = never, 1 = every token-only batch, N > 1 = only batches whose longest sequence has at most N
    // tokens (e.g. 512 = the reference's query length: long text passages then stay on the bf16 MFMA flash-attention path,
    // whose cost grows with L instead of L^2 waves).  NOTE the batch-composition dependence this implies: the same text item
    // is embedded at fp32-class precision in a token-only batch and at bf16 precision (inside the 1e-3 tolerance, not the
    // 1e-6 of the split pass) in a batch that also holds an image.
    int max_len = 0;
    for (int i = 0; i < B; ++i) max_len = std::max(max_len, seq_offsets[i + 1] - seq_offsets[i]);
    const bool hp = n_slices == 0 && c.text_split_precision != 0 && (c.text_split_precision == 1 || max_len <= c.text_split_precision) &&
                    !(hook && hook->bf16_route);
    if (hp && m->has_embed_lo)
        HIPCHK(launch_embed_gather_hp(m->w_ids.as<int>(), T, m->embed.p, m->embed_lo.p, E, c.scale_emb, m->w_h.as<float>(), s));
    else
        HIPCHK(launch_embed_gather(m->w_ids.as<int>(), T, m->embed.p, E, c.scale_emb, m->w_h.as<float>(), s));
    if (base_pos) {                      // positions that do not start at 0: built here, uploaded like the ids
        int* a_pos = (int*)arena_take(m, (size_t)T * 4);
        for (int i = 0; i < B; ++i)
            for (int t = seq_offsets[i]; t < seq_offsets[i + 1]; ++t) a_pos[t] = base_pos[i] + (t - seq_offsets[i]);
        HIPCHK(hipMemcpyAsync(m->w_pos.p, a_pos, (size_t)T * 4, hipMemcpyHostToDevice, s));
    } else {
        HIPCHK(launch_iota_pos(m->w_seq.as<int>(), B, m->w_pos.as<int>(), s));
    }

    // ---- vision: group slices by shape, chunk to the workspace
    if (n_slices > 0) {
        size_t pix_total = 0;
        std::vector<size_t> pix_off(n_slices);
        for (int i = 0; i < n_slices; ++i) {
            const int H = slice_hw[2 * i], W = slice_hw[2 * i + 1];
            if (H <= 0 || W <= 0 || H % c.patch_size || W % c.patch_size)
                return fail(VR_ERR_INVALID, "slice %d: %dx%d is not a multiple of the patch size", i, H, W);
            if ((H / c.patch_size) * (W / c.patch_size) > c.max_patches)
                return fail(VR_ERR_CAPACITY, "slice %d has more than max_patches=%d patches", i, c.max_patches);
            pix_off[i] = pix_total;
            pix_total += ((size_t)H * W * 3 + 15) / 16 * 16;
        }
        std::vector<const uint8_t*> dev_ptr(n_slices);
        if (slices_on_device) {
            for (int i = 0; i < n_slices; ++i) dev_ptr[i] = slices[i];
        } else {
            if (m->w_pix.bytes < pix_total) VRCHK(m->w_pix.alloc(pix_total));
            for (int i = 0; i < n_slices; ++i) {
                const size_t nb = (size_t)slice_hw[2 * i] * slice_hw[2 * i + 1] * 3;
                HIPCHK(hipMemcpyAsync((char*)m->w_pix.p + pix_off[i], slices[i], nb, hipMemcpyHostToDevice, s));
                dev_ptr[i] = (const uint8_t*)m->w_pix.p + pix_off[i];
            }
        }
        std::vector<char> done(n_slices, 0);
        bool first = true;
        for (int i = 0; i < n_slices; ++i) {
            if (done[i]) continue;
            const int H = slice_hw[2 * i], W = slice_hw[2 * i + 1];
            const int N = (H / c.patch_size) * (W / c.patch_size);
            std::vector<int> idx;
            for (int j = i; j < n_slices; ++j)
                if (!done[j] && slice_hw[2 * j] == H && slice_hw[2 * j + 1] == W) { idx.push_back(j); done[j] = 1; }
            const int per_pass = std::max(1, (int)std::min<int64_t>(c.max_images, ((int64_t)c.max_images * c.max_patches) / N));
            for (size_t lo = 0; lo < idx.size(); lo += per_pass) {
                const int n = (int)std::min<size_t>(per_pass, idx.size() - lo);
                const uint8_t** ptrs = (const uint8_t**)arena_take(m, (size_t)n * 8);
                int32_t* rowmap = (int32_t*)arena_take(m, (size_t)n * Q * 4);
                for (int k = 0; k < n; ++k) {
                    ptrs[k] = dev_ptr[idx[lo + k]];
                    memcpy(rowmap + (size_t)k * Q, vision_rows + (size_t)idx[lo + k] * Q, (size_t)Q * 4);
                }
                VRCHK(run_vision_group(m, ptrs, n, H, W, rowmap, first, s));
                first = false;
            }
        }
    }
    VRCHK(tap_store(m, "inputs_embeds", m->w_h.p, T, E, E, false, s));

    // ---- decoder (modeling_minicpm.py:939-1004, 1147-1304), packed ragged sequences
    float* h = m->w_h.as<float>();
    const int* seq = m->w_seq.as<int>();
    const float* rope_table = hook && hook->rope_table ? hook->rope_table : m->rope.as<float>();
    {
        const int rope_len = hook && hook->rope_table ? hook->rope_len : m->rope_len;
        int last = max_len;              // one past the largest position of the batch
        if (base_pos) {
            last = 0;
            for (int i = 0; i < B; ++i) last = std::max(last, base_pos[i] + seq_offsets[i + 1] - seq_offsets[i]);
        }
        if (last > rope_len) return fail(VR_ERR_CAPACITY, "sequence of %d tokens exceeds the RoPE table", last);
    }
    VRCHK(prof_begin(m, VR_PROF_DECODER, s));
    if (hp) {
        VRCHK(run_decoder_hp(m, T, B, max_len, s));
    } else {
    const DecRoute route = dec_route(T, E, m->Ip, m->taps_on);
    const int ks = route.ks;
    const size_t pstride = (size_t)T * E;
    float* part = m->w_part.as<float>();
    bool pend = false;                   // h still lacks residual_scale * sum(partials)
    auto proj = [&](const void* A, int lda, const Linear& L) -> int {
        if (route.proj_128w) {
            GemmArgs a = gemm_args(A, lda, L, T, h, E); a.resid = h; a.alpha = c.residual_scale;
            if (gemm128w_fits(a, 192)) { HIPCHK(launch_gemm(a, EPI_RESID, GEMM_VARIANT_128W_192, s)); return VR_OK; }
        }
        if (ks > 1) {
            GemmArgs a = gemm_args(A, lda, L, T, part, E);
            a.ksplit = ks; a.split_stride = pstride;
            HIPCHK(launch_gemm(a, EPI_F32, gemm256w_fits(a, route.proj_variant == GEMM_VARIANT_192W ? 192 : 256) ? route.proj_variant : GEMM_VARIANT_256IL, s));
            pend = true;
        } else {
            GemmArgs a = gemm_args(A, lda, L, T, h, E); a.resid = h; a.alpha = c.residual_scale;
            HIPCHK(launch_gemm(a, EPI_RESID, GEMM_VARIANT_AUTO, s));
        }
        return VR_OK;
    };
    auto norm = [&](const float* w) -> int {
        VRCHK(prof_begin(m, VR_PROF_DEC_NORM, s));
        struct End { vr_model_s* m; hipStream_t s; ~End() { (void)prof_end(m, VR_PROF_DEC_NORM, 0.0, s); } } end_{m, s};
        if (pend) {
            HIPCHK(launch_rmsnorm_accum(h, T, E, E, part, ks, pstride, E, c.residual_scale, w, c.rms_norm_eps, m->w_dxn.p, E, s));
            pend = false;
        } else {
            HIPCHK(launch_rmsnorm(h, T, E, E, w, c.rms_norm_eps, m->w_dxn.p, E, s));
        }
        return VR_OK;
    };
    // The half-height projections wait on every K-step for weight lines that come from HBM (the 4.9 GB of decoder weights never
    // survive a step in any cache; gemm128w.hip has the arithmetic).  The MFMA-bound launch IN FRONT of each — q|k|v + RoPE in front
    // of o, gate|up + SwiGLU in front of down — requests the projection's (padded) matrix while it runs (GemmArgs::warm): the bytes
    // are the ones the projection fetches anyway, asked for some tens of microseconds earlier, and wait for it in the memory-side cache.
    // (not under a hook: a chat prefill puts a launch of its own between q|k|v and o.)
    auto warm_for = [&](GemmArgs& a, int epi, const Linear& next) {
        const size_t bytes = (size_t)next.n_pad * next.k_pad * 2;
        if (route.proj_128w && !hook && bytes < WARM_MAX_BYTES && gemm_auto_variant(a, epi) == GEMM_VARIANT_256W) { a.warm = next.w.p; a.warm_bytes = bytes; }
    };
    double attn_flops = 0;
    for (int i = 0; i < B; ++i) { const double Li = seq_offsets[i + 1] - seq_offsets[i]; attn_flops += 4.0 * Li * Li * E; }
    for (int l = 0; l < c.num_layers; ++l) {
        const DecLayer& L = m->layers[l];
        VRCHK(norm(L.ln1.v.as<float>()));
        {
            GemmArgs a = gemm_args(m->w_dxn.p, E, L.qkv, T, m->w_dqkv.p, 3 * E);
            a.rope_pos = m->w_pos.as<int>(); a.rope_table = rope_table; a.rope_cols = 2 * E;
            warm_for(a, EPI_ROPE, L.o);
            VRCHK(prof_begin(m, VR_PROF_DEC_QKV, s));
            HIPCHK(launch_gemm(a, EPI_ROPE, GEMM_VARIANT_AUTO, s));
            VRCHK(prof_end(m, VR_PROF_DEC_QKV, 6.0 * T * (double)E * E, s));
        }
        if (hook && hook->layer) VRCHK(hook->layer(hook->ctx, l, m->w_dqkv.p, 3 * E, T, s));
        if (hook && hook->attn) {
            VRCHK(prof_begin(m, VR_PROF_DEC_ATTN, s));
            VRCHK(hook->attn(hook->ctx, l, m->w_dqkv.p, 3 * E, T, m->w_datt.p, E, s));
            VRCHK(prof_end(m, VR_PROF_DEC_ATTN, 0.0, s));     // (its keys are the hook's business: time is booked, FLOPs are not)
        } else {
            VRCHK(prof_begin(m, VR_PROF_DEC_ATTN, s));
            AttnArgs a{};
            a.q = m->w_dqkv.p; a.ldq = 3 * E; a.k = (const char*)m->w_dqkv.p + (size_t)E * 2; a.ldk = 3 * E;
            a.v = (const char*)m->w_dqkv.p + (size_t)2 * E * 2; a.ldv = 3 * E;
            a.out = m->w_datt.p; a.ldo = E; a.cu_q = seq; a.cu_kv = seq; a.B = B; a.heads = c.num_heads; a.head_dim = 64;
            a.max_q = max_len; a.causal = 1; a.q_shared = 0; a.scale = 1.0f / sqrtf(64.0f);
            HIPCHK(launch_attention(a, s));
            VRCHK(prof_end(m, VR_PROF_DEC_ATTN, attn_flops, s));
        }
        VRCHK(prof_begin(m, VR_PROF_DEC_O, s));
        VRCHK(proj(m->w_datt.p, E, L.o));
        VRCHK(prof_end(m, VR_PROF_DEC_O, 2.0 * T * (double)E * E, s));
        VRCHK(norm(L.ln2.v.as<float>()));
        VRCHK(prof_begin(m, VR_PROF_DEC_GU, s));
        {
            GemmArgs a = gemm_args(m->w_dxn.p, E, L.gu, T, m->w_dact.p, m->Ip);
            warm_for(a, EPI_SWIGLU, L.down);
            HIPCHK(launch_gemm(a, EPI_SWIGLU, GEMM_VARIANT_AUTO, s));
        }
        VRCHK(prof_end(m, VR_PROF_DEC_GU, 4.0 * T * (double)E * m->I, s));
        VRCHK(prof_begin(m, VR_PROF_DEC_DOWN, s));
        VRCHK(proj(m->w_dact.p, m->Ip, L.down));
        VRCHK(prof_end(m, VR_PROF_DEC_DOWN, 2.0 * T * (double)E * m->I, s));
        if (l == 0) VRCHK(tap_store(m, "dec_layer0", h, T, E, E, false, s));
    }
    if (pend) {                          // last down projection: residual update only
        HIPCHK(launch_rmsnorm_accum(h, T, E, E, part, ks, pstride, E, c.residual_scale, nullptr, c.rms_norm_eps, nullptr, 0, s));
        pend = false;
    }
    }
    {
        double fl = 0;
        for (int i = 0; i < B; ++i) { const double Li = seq_offsets[i + 1] - seq_offsets[i]; fl += 4.0 * Li * Li * E; }
        fl = c.num_layers * (fl + (double)T * (8.0 * E * E + 6.0 * (double)E * m->I));
        VRCHK(prof_end(m, VR_PROF_DECODER, fl, s));
    }
    // ---- K19+K20: final norm + wmean pool + L2 normalise
    float* tap_hidden = nullptr;   // scratch f32 [T][E] for the post-norm hidden states
    if (m->taps_on && (size_t)T * E * 4 <= m->w_kv32.bytes) tap_hidden = m->w_kv32.as<float>();
    if (out_hidden) {              // vr_encode_hidden: the packed rows first (the resampler's scratch when it is large enough)
        if (max_len > hidden_len) return fail(VR_ERR_INVALID, "hidden_len=%d is shorter than the longest sequence (%d)", hidden_len, max_len);
        if (!tap_hidden) {
            if ((size_t)T * E * 4 <= m->w_kv32.bytes) tap_hidden = m->w_kv32.as<float>();
            else { VRCHK(m->w_hidden.reserve((size_t)T * E * 4)); tap_hidden = m->w_hidden.as<float>(); }
        }
    }
    float* dst = out_on_device ? out_reps : m->w_out.as<float>();
    HIPCHK(launch_pool(h, seq, B, E, m->final_norm.v.as<float>(), c.rms_norm_eps, dst, tap_hidden, s, m->pool_mode));
    if (tap_hidden && m->taps_on) VRCHK(tap_store(m, "last_hidden", tap_hidden, T, E, E, false, s));
    if (out_hidden) {              // right padding (modeling_minicpmv.py:440-479 `pad`): item i -> rows [i * hidden_len, + len_i), zeros behind
        HIPCHK(hipMemsetAsync(out_hidden, 0, (size_t)B * hidden_len * E * 4, s));
        for (int i = 0; i < B; ++i)
            HIPCHK(hipMemcpyAsync(out_hidden + (size_t)i * hidden_len * E, tap_hidden + (size_t)seq_offsets[i] * E,
                                  (size_t)(seq_offsets[i + 1] - seq_offsets[i]) * E * 4, hipMemcpyDeviceToDevice, s));
    }
    if (!out_on_device) HIPCHK(hipMemcpyAsync(out_reps, dst, (size_t)B * E * 4, hipMemcpyDeviceToHost, s));
    if (!out_on_device || (n_slices > 0 && !slices_on_device)) HIPCHK(hipStreamSynchronize(s));   // host buffers consumed
    return VR_OK;
}
