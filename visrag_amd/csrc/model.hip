// The encoder's model handle of libvisrag_hip.so (the C ABI of include/visrag_hip.h): device weight store, derived tables,
// workspace, per-grid tables, taps, clones and the event profile.  The launch sequence of an encode pass: encode.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "model.h"

extern "C" const char* vr_version(void) { return "visrag_hip 0.1.0 (gfx950)"; }
extern "C" const char* vr_last_error(void) { return g_err.c_str(); }
extern "C" int vr_device_count(int* count) {
    if (!count) return fail(VR_ERR_INVALID, "count is NULL");
    HIPCHK(hipGetDeviceCount(count));
    return VR_OK;
}

// ------------------------------------------------------------------------------ create ---
extern "C" int vr_model_create(int device_id, const vr_config_t* cfg, vr_model_t* out) {
    if (!cfg || !out) return fail(VR_ERR_INVALID, "cfg/out is NULL");
    const vr_config_t& c = *cfg;
    if (c.vit_dim % c.vit_heads || c.vit_dim / c.vit_heads != 72)
        return fail(VR_ERR_INVALID, "ViT head_dim must be 72 (vit_dim %d / heads %d)", c.vit_dim, c.vit_heads);
    if (c.hidden_size % 128) return fail(VR_ERR_INVALID, "hidden_size %d must be a multiple of 128", c.hidden_size);
    if (c.hidden_size % c.num_heads || c.hidden_size / c.num_heads != 64)
        return fail(VR_ERR_INVALID, "decoder head_dim must be 64");
    if (c.intermediate_size % 64) return fail(VR_ERR_INVALID, "intermediate_size must be a multiple of 64");
    if (c.query_num != 64) return fail(VR_ERR_INVALID, "query_num must be 64");
    if (c.vit_dim % 4 || c.hidden_size > 2560 || c.vit_dim > 2560) return fail(VR_ERR_INVALID, "dims out of range");
    if (c.max_images <= 0 || c.max_patches <= 0 || c.max_tokens <= 0 || c.max_seqs <= 0)
        return fail(VR_ERR_INVALID, "workspace limits must be positive");
    VRCHK(set_dev(device_id));
    vr_model_s* m = new vr_model_s();
    m->device = device_id;
    m->c = c;
    m->D = c.vit_dim; m->Dp = pad128(c.vit_dim);
    m->F = c.vit_hidden; m->Fp = pad128(c.vit_hidden);
    m->E = c.hidden_size; m->I = c.intermediate_size; m->Ip = pad128(c.intermediate_size);
    m->Kpe = 3 * c.patch_size * c.patch_size; m->Kpe_p = pad128(m->Kpe);
    m->Q = c.query_num;
    m->blocks.resize(c.vit_depth);
    m->layers.resize(c.num_layers);
    *out = m;
    return VR_OK;
}

extern "C" int vr_model_destroy(vr_model_t m) {
    if (!m) return VR_OK;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    if (!m->borrowed) {
        auto fl = [](Linear& l) { l.w.free(); l.b.free(); };
        fl(m->patch); fl(m->r_kvproj); fl(m->r_kv); fl(m->r_out); fl(m->r_proj);
        for (auto& b : m->blocks) {
            fl(b.qkv); fl(b.proj); fl(b.fc1); fl(b.fc2); b.n1w.v.free(); b.n1b.v.free(); b.n2w.v.free(); b.n2b.v.free();
        }
        for (auto& l : m->layers) { fl(l.qkv); fl(l.o); fl(l.gu); fl(l.down); fl(l.qkv_lo); fl(l.o_lo); fl(l.gu_lo); fl(l.down_lo); l.ln1.v.free(); l.ln2.v.free(); }
        for (Vec* v : {&m->vit_nw, &m->vit_nb, &m->r_lnq_w, &m->r_lnq_b, &m->r_lnkv_w, &m->r_lnkv_b, &m->r_lnpost_w, &m->r_lnpost_b, &m->final_norm}) v->v.free();
        for (DevBuf* b : {&m->r_q, &m->embed, &m->embed_lo, &m->rope}) b->free();
    }
    for (auto& g : m->grids) { g.second.vit_pos.free(); g.second.pos_k.free(); }
    for (auto& pc : m->prof) for (hipEvent_t e : pc.ev) (void)hipEventDestroy(e);
    if (m->arena) (void)hipHostFree(m->arena);
    if (m->arena_ev) (void)hipEventDestroy(m->arena_ev);
    for (DevBuf* b : {&m->w_hvit, &m->w_xn, &m->w_qkv, &m->w_att, &m->w_mlp,
                      &m->w_kv32, &m->w_xkv, &m->w_KV, &m->w_ratt, &m->w_rout, &m->w_rln, &m->w_h, &m->w_dxn, &m->w_part, &m->w_dqkv,
                      &m->w_datt, &m->w_dact, &m->w_cu, &m->w_ids, &m->w_seq, &m->w_pos, &m->w_rowmap, &m->w_imgptr,
                      &m->w_pix, &m->w_out, &m->w_hp_hi, &m->w_hp_planes, &m->w_hp_qkv, &m->w_hp_att, &m->w_hp_gu, &m->w_seqof, &m->w_hp_part, &m->w_hidden})
        b->free();
    delete m;
    return VR_OK;
}

extern "C" int vr_model_load_weight(vr_model_t m, const char* name_c, const void* data, const int64_t* shape,
                                    int32_t ndim, int32_t dtype, int32_t on_device) {
    if (!m || !name_c || !data || !shape) return fail(VR_ERR_INVALID, "NULL argument");
    if (dtype != VR_DTYPE_F32 && dtype != VR_DTYPE_BF16) return fail(VR_ERR_INVALID, "bad dtype %d", dtype);
    VRCHK(set_dev(m->device));
    const std::string name(name_c);
    const int bf = dtype == VR_DTYPE_BF16;
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    const vr_config_t& c = m->c;
    const int D = m->D, F = m->F, E = m->E, I = m->I;
    auto bad_shape = [&]() { return fail(VR_ERR_INVALID, "unexpected shape for %s", name_c); };

    // keys the embedding path does not use
    if (name.rfind("llm.lm_head.", 0) == 0 || name.rfind("vpm.attn_pool.", 0) == 0 ||
        name == "resampler.pos_embed" || name.find("rotary_emb") != std::string::npos)
        return VR_OK;

    Staged st;
    VRCHK(stage(data, numel * (bf ? 2 : 4), on_device, st));
    const void* src = st.dev;
    m->finalized = false;

    if (name == "vpm.patch_embed.proj.weight") {
        if (!shape_is(shape, ndim, {D, 3, c.patch_size, c.patch_size})) return bad_shape();
        Linear& L = m->patch;      // columns permuted to the image's byte order inside a patch (patch_embed.hip)
        if (!L.w.p) { L.n = D; L.k = m->Kpe; L.n_pad = pad128(D); L.k_pad = pad128(m->Kpe); VRCHK(L.w.alloc((size_t)pad256(D) * L.k_pad * 2)); }
        HIPCHK(launch_pack_patch_weight(src, bf, D, c.patch_size, L.w.p, L.k_pad, 0));
        HIPCHK(hipDeviceSynchronize());
        L.has_w = true;
        return VR_OK;
    }
    if (name == "vpm.patch_embed.proj.bias") { if (numel != (size_t)D) return bad_shape(); return load_bias_part(m->patch, D, src, bf, D, 0); }
    if (name == "vpm.pos_embed") {
        if (numel != (size_t)c.vit_pos_grid * c.vit_pos_grid * D) return bad_shape();
        m->has_pos = true;
        m->grids.clear();
        return to_host_f32(src, bf, numel, m->pos_embed_host);
    }
    if (name == "vpm.norm.weight") { if (numel != (size_t)D) return bad_shape(); return load_vec(m->vit_nw, src, bf, D, m->Dp); }
    if (name == "vpm.norm.bias") { if (numel != (size_t)D) return bad_shape(); return load_vec(m->vit_nb, src, bf, D, m->Dp); }
    if (name.rfind("vpm.blocks.", 0) == 0) {
        int n = -1, off = 0;
        if (sscanf(name.c_str(), "vpm.blocks.%d.%n", &n, &off) < 1) return fail(VR_ERR_INVALID, "bad key %s", name_c);
        if (n >= c.vit_depth) return VR_OK;     // dropped last block (modeling_minicpmv.py:70-71)
        const std::string sub = name.substr(off);
        VitBlock& b = m->blocks[n];
        if (sub == "norm1.weight") { if (numel != (size_t)D) return bad_shape(); return load_vec(b.n1w, src, bf, D, m->Dp); }
        if (sub == "norm1.bias") { if (numel != (size_t)D) return bad_shape(); return load_vec(b.n1b, src, bf, D, m->Dp); }
        if (sub == "norm2.weight") { if (numel != (size_t)D) return bad_shape(); return load_vec(b.n2w, src, bf, D, m->Dp); }
        if (sub == "norm2.bias") { if (numel != (size_t)D) return bad_shape(); return load_vec(b.n2b, src, bf, D, m->Dp); }
        if (sub == "attn.qkv.weight") { if (!shape_is(shape, ndim, {3 * D, D})) return bad_shape(); return load_linear_part(b.qkv, 3 * D, D, src, bf, 3 * D, D, 0, 3 * D, 0, 0); }
        if (sub == "attn.qkv.bias") { if (numel != (size_t)3 * D) return bad_shape(); return load_bias_part(b.qkv, 3 * D, src, bf, 3 * D, 0); }
        if (sub == "attn.proj.weight") { if (!shape_is(shape, ndim, {D, D})) return bad_shape(); return load_linear_part(b.proj, D, D, src, bf, D, D, 0, D, 0, 0); }
        if (sub == "attn.proj.bias") { if (numel != (size_t)D) return bad_shape(); return load_bias_part(b.proj, D, src, bf, D, 0); }
        if (sub == "mlp.fc1.weight") { if (!shape_is(shape, ndim, {F, D})) return bad_shape(); return load_linear_part(b.fc1, F, D, src, bf, F, D, 0, F, 0, 0); }
        if (sub == "mlp.fc1.bias") { if (numel != (size_t)F) return bad_shape(); return load_bias_part(b.fc1, F, src, bf, F, 0); }
        if (sub == "mlp.fc2.weight") { if (!shape_is(shape, ndim, {D, F})) return bad_shape(); return load_linear_part(b.fc2, D, F, src, bf, D, F, 0, D, 0, 0); }
        if (sub == "mlp.fc2.bias") { if (numel != (size_t)D) return bad_shape(); return load_bias_part(b.fc2, D, src, bf, D, 0); }
        return fail(VR_ERR_INVALID, "unknown ViT key %s", name_c);
    }
    if (name.rfind("resampler.", 0) == 0) {
        const std::string sub = name.substr(10);
        if (sub == "query") { if (!shape_is(shape, ndim, {m->Q, E})) return bad_shape(); m->has_query = true; return to_host_f32(src, bf, numel, m->r_query_host); }
        if (sub == "kv_proj.weight") { if (!shape_is(shape, ndim, {E, D})) return bad_shape(); return load_linear_part(m->r_kvproj, E, D, src, bf, E, D, 0, E, 0, 0); }
        if (sub == "attn.in_proj_weight") {
            if (!shape_is(shape, ndim, {3 * E, E})) return bad_shape();
            std::vector<float> all;
            VRCHK(to_host_f32(src, bf, (size_t)E * E, all));      // q rows only
            m->r_wq_host.swap(all);
            m->has_inproj = true;
            const char* kv_src = (const char*)src + (size_t)E * E * (bf ? 2 : 4);
            return load_linear_part(m->r_kv, 2 * E, E, kv_src, bf, 2 * E, E, 0, 2 * E, 0, 0);
        }
        if (sub == "attn.in_proj_bias") {
            if (numel != (size_t)3 * E) return bad_shape();
            VRCHK(to_host_f32(src, bf, (size_t)E, m->r_bq_host));
            m->has_inproj_b = true;
            const char* kv_src = (const char*)src + (size_t)E * (bf ? 2 : 4);
            return load_bias_part(m->r_kv, 2 * E, kv_src, bf, 2 * E, 0);
        }
        if (sub == "attn.out_proj.weight") { if (!shape_is(shape, ndim, {E, E})) return bad_shape(); return load_linear_part(m->r_out, E, E, src, bf, E, E, 0, E, 0, 0); }
        if (sub == "attn.out_proj.bias") { if (numel != (size_t)E) return bad_shape(); return load_bias_part(m->r_out, E, src, bf, E, 0); }
        if (sub == "proj") { if (!shape_is(shape, ndim, {E, E})) return bad_shape(); return load_linear_part(m->r_proj, E, E, src, bf, E, E, 1, E, 0, 0); }
        Vec* v = nullptr;
        if (sub == "ln_q.weight") v = &m->r_lnq_w; else if (sub == "ln_q.bias") v = &m->r_lnq_b;
        else if (sub == "ln_kv.weight") v = &m->r_lnkv_w; else if (sub == "ln_kv.bias") v = &m->r_lnkv_b;
        else if (sub == "ln_post.weight") v = &m->r_lnpost_w; else if (sub == "ln_post.bias") v = &m->r_lnpost_b;
        if (!v) return fail(VR_ERR_INVALID, "unknown resampler key %s", name_c);
        if (numel != (size_t)E) return bad_shape();
        return load_vec(*v, src, bf, E, E);
    }
    if (name == "llm.model.embed_tokens.weight") {
        if (!shape_is(shape, ndim, {c.vocab_size, E})) return bad_shape();
        VRCHK(m->embed.alloc(numel * 2));
        HIPCHK(launch_pack_weight(src, bf, c.vocab_size, E, E, 0, m->embed.p, E, c.vocab_size, 0, 0, 0));
        m->has_embed_lo = false;
        if (!bf && c.text_split_precision) {
            VRCHK(m->embed_lo.alloc(numel * 2));
            HIPCHK(launch_pack_weight(src, bf, c.vocab_size, E, E, 0, m->embed_lo.p, E, c.vocab_size, 0, 0, 0, 1));
            m->has_embed_lo = true;
        }
        HIPCHK(hipDeviceSynchronize());
        m->has_embed = true;
        return VR_OK;
    }
    if (name == "llm.model.norm.weight") { if (numel != (size_t)E) return bad_shape(); return load_vec(m->final_norm, src, bf, E, E); }
    if (name.rfind("llm.model.layers.", 0) == 0) {
        int n = -1, off = 0;
        if (sscanf(name.c_str(), "llm.model.layers.%d.%n", &n, &off) < 1) return fail(VR_ERR_INVALID, "bad key %s", name_c);
        if (n >= c.num_layers) return fail(VR_ERR_INVALID, "layer index %d out of range", n);
        const std::string sub = name.substr(off);
        DecLayer& l = m->layers[n];
        if (sub == "input_layernorm.weight") { if (numel != (size_t)E) return bad_shape(); return load_vec(l.ln1, src, bf, E, E); }
        if (sub == "post_attention_layernorm.weight") { if (numel != (size_t)E) return bad_shape(); return load_vec(l.ln2, src, bf, E, E); }
        // fp32 source weights also leave their low halves (w - bf16(w)) for the split-precision text path; a bf16
        // checkpoint has none (the two activation halves against the one weight are then the whole product)
        const bool lo = !bf && c.text_split_precision;
        for (int part = 0; part < 3; ++part) {
            static const char* nm[3] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"};
            if (sub == nm[part]) {
                if (!shape_is(shape, ndim, {E, E})) return bad_shape();
                l.parts_qkv |= 1 << part;
                if (lo) VRCHK(load_linear_part(l.qkv_lo, 3 * E, E, src, bf, E, E, 0, E, 0, part * E, 1));
                return load_linear_part(l.qkv, 3 * E, E, src, bf, E, E, 0, E, 0, part * E);
            }
        }
        if (sub == "self_attn.o_proj.weight") {
            if (!shape_is(shape, ndim, {E, E})) return bad_shape();
            if (lo) VRCHK(load_linear_part(l.o_lo, E, E, src, bf, E, E, 0, E, 0, 0, 1));
            return load_linear_part(l.o, E, E, src, bf, E, E, 0, E, 0, 0);
        }
        if (sub == "mlp.gate_proj.weight" || sub == "mlp.up_proj.weight") {
            if (!shape_is(shape, ndim, {I, E})) return bad_shape();
            const int up = sub == "mlp.up_proj.weight";
            l.parts_gu |= 1 << up;
            // 16-row interleave: [16 gate | 16 up | ...] (EPI_SWIGLU)
            if (lo) VRCHK(load_linear_part(l.gu_lo, 2 * I, E, src, bf, I, E, 0, 16, 32, up * 16, 1));
            return load_linear_part(l.gu, 2 * I, E, src, bf, I, E, 0, 16, 32, up * 16);
        }
        if (sub == "mlp.down_proj.weight") {
            if (!shape_is(shape, ndim, {E, I})) return bad_shape();
            if (lo) VRCHK(load_linear_part(l.down_lo, E, I, src, bf, E, I, 0, E, 0, 0, 1));
            return load_linear_part(l.down, E, I, src, bf, E, I, 0, E, 0, 0);
        }
        return fail(VR_ERR_INVALID, "unknown decoder key %s", name_c);
    }
    return fail(VR_ERR_INVALID, "unknown weight key %s", name_c);
}

// ---------------------------------------------------------------------- derived tables ---
// fp32 sincos table of resampler.py:38-90 (numpy float32 arithmetic restated)
static void sincos_2d_host(int E, int gh, int gw, std::vector<float>& out) {
    const int half = E / 2, quarter = half / 2;
    out.assign((size_t)gh * gw * E, 0.f);
    std::vector<float> omega(quarter);
    for (int i = 0; i < quarter; ++i) {
        float o = (float)i / ((float)half / 2.0f);
        omega[i] = 1.0f / powf(10000.0f, o);
    }
    for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x) {
            float* row = out.data() + ((size_t)y * gw + x) * E;
            // first half <- grid[0] = column index (meshgrid(w, h), "w goes first"); second <- row index
            for (int i = 0; i < quarter; ++i) {
                const float a = (float)x * omega[i], b = (float)y * omega[i];
                row[i] = sinf(a); row[quarter + i] = cosf(a);
                row[half + i] = sinf(b); row[half + quarter + i] = cosf(b);
            }
        }
}

// bicubic (a = -0.5) anti-aliased separable resample, align_corners=False: the algorithm of
// F.interpolate(mode="bicubic", antialias=True) used by timm's resample_abs_pos_embed
// (timm/layers/pos_embed.py:46).  in [gi][gi][D] -> out [gh][gw][D].
static inline float cubic_aa(float x) {
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
    return 0.0f;
}
static void aa_weights(int in, int out, std::vector<int>& xmin, std::vector<int>& xsize, std::vector<float>& w, int& maxk) {
    const float scale = (float)in / (float)out;
    const float support = (scale >= 1.0f) ? 2.0f * scale : 2.0f;
    const float invscale = (scale >= 1.0f) ? 1.0f / scale : 1.0f;
    maxk = (int)ceilf(support) * 2 + 1;
    xmin.resize(out); xsize.resize(out); w.assign((size_t)out * maxk, 0.f);
    for (int i = 0; i < out; ++i) {
        const float center = scale * ((float)i + 0.5f);
        int lo = std::max(0, (int)(center - support + 0.5f));
        int hi = std::min(in, (int)(center + support + 0.5f));
        xmin[i] = lo; xsize[i] = hi - lo;
        float tot = 0.f;
        for (int j = 0; j < xsize[i]; ++j) {
            const float ww = cubic_aa(((float)(j + lo) - center + 0.5f) * invscale);
            w[(size_t)i * maxk + j] = ww; tot += ww;
        }
        for (int j = 0; j < xsize[i]; ++j) w[(size_t)i * maxk + j] /= tot;
    }
}
static void resample_pos_host(const std::vector<float>& pe, int gi, int D, int gh, int gw, std::vector<float>& out) {
    out.assign((size_t)gh * gw * D, 0.f);
    if (gh == gi && gw == gi) { out = pe; return; }
    std::vector<int> xm, xs, ym, ys; std::vector<float> xw, yw; int xk, yk;
    aa_weights(gi, gw, xm, xs, xw, xk);
    aa_weights(gi, gh, ym, ys, yw, yk);
    std::vector<float> tmp((size_t)gi * gw * D, 0.f);      // horizontal pass
    for (int y = 0; y < gi; ++y)
        for (int x = 0; x < gw; ++x) {
            float* o = tmp.data() + ((size_t)y * gw + x) * D;
            for (int j = 0; j < xs[x]; ++j) {
                const float ww = xw[(size_t)x * xk + j];
                const float* s = pe.data() + ((size_t)y * gi + xm[x] + j) * D;
                for (int d = 0; d < D; ++d) o[d] += ww * s[d];
            }
        }
    for (int y = 0; y < gh; ++y)                             // vertical pass
        for (int x = 0; x < gw; ++x) {
            float* o = out.data() + ((size_t)y * gw + x) * D;
            for (int j = 0; j < ys[y]; ++j) {
                const float ww = yw[(size_t)y * yk + j];
                const float* s = tmp.data() + ((size_t)(ym[y] + j) * gw + x) * D;
                for (int d = 0; d < D; ++d) o[d] += ww * s[d];
            }
        }
}

std::vector<float> rope_table_host(float theta, int len) {
    std::vector<float> tab((size_t)len * 64);
    float inv[32];
    for (int i = 0; i < 32; ++i) inv[i] = 1.0f / powf(theta, (float)(2 * i) / 64.0f);
    for (int p = 0; p < len; ++p)
        for (int i = 0; i < 32; ++i) {
            const float a = (float)p * inv[i];
            tab[(size_t)p * 64 + i] = cosf(a);
            tab[(size_t)p * 64 + 32 + i] = sinf(a);
        }
    return tab;
}

static int alloc_workspace(vr_model_s* m) {
    const vr_config_t& c = m->c;
    const int64_t M = pad256l((int64_t)c.max_images * c.max_patches);
    const int64_t T = pad256l(c.max_tokens);
    const int64_t R = pad256l((int64_t)c.max_images * m->Q);
    m->Mcap = M; m->Tcap = T; m->Rcap = R;
    const int E = m->E, Dp = m->Dp;
    VRCHK(m->w_hvit.alloc((size_t)M * Dp * 4));
    VRCHK(m->w_xn.alloc((size_t)M * Dp * 2));
    VRCHK(m->w_qkv.alloc((size_t)M * pad128(3 * m->D) * 2));
    VRCHK(m->w_att.alloc((size_t)M * Dp * 2));
    VRCHK(m->w_mlp.alloc((size_t)M * m->Fp * 2));
    VRCHK(m->w_kv32.alloc((size_t)M * E * 4));
    VRCHK(m->w_xkv.alloc((size_t)M * E * 2));
    VRCHK(m->w_KV.alloc((size_t)M * 2 * E * 2));
    VRCHK(m->w_ratt.alloc((size_t)R * E * 2));
    VRCHK(m->w_rout.alloc((size_t)R * E * 4));
    VRCHK(m->w_rln.alloc((size_t)R * E * 2));
    VRCHK(m->w_h.alloc((size_t)T * E * 4));
    VRCHK(m->w_dxn.alloc((size_t)T * E * 2));
    VRCHK(m->w_part.alloc((size_t)DEC_KSPLIT_MAX * T * E * 4));
    VRCHK(m->w_dqkv.alloc((size_t)T * 3 * E * 2));
    VRCHK(m->w_datt.alloc((size_t)T * E * 2));
    VRCHK(m->w_dact.alloc((size_t)T * m->Ip * 2));
    VRCHK(m->w_cu.alloc((size_t)(c.max_images + c.max_seqs + 8) * 2 * 4));
    VRCHK(m->w_ids.alloc((size_t)T * 4));
    VRCHK(m->w_seq.alloc((size_t)(c.max_seqs + 1) * 4));
    VRCHK(m->w_pos.alloc((size_t)T * 4));
    VRCHK(m->w_rowmap.alloc((size_t)R * 4));
    VRCHK(m->w_imgptr.alloc((size_t)c.max_images * 8));
    VRCHK(m->w_out.alloc((size_t)c.max_seqs * E * 4));
    if (c.text_split_precision) {
        const int Kmax = std::max(E, m->Ip);
        VRCHK(m->w_hp_hi.alloc((size_t)2 * T * Kmax * 2));       // [hi rows | lo rows]: the lo half starts right behind the batch's T hi rows
        VRCHK(m->w_hp_qkv.alloc((size_t)T * 3 * E * 4));
        VRCHK(m->w_hp_att.alloc((size_t)T * E * 4));
        VRCHK(m->w_hp_gu.alloc((size_t)T * pad128(2 * m->I) * 4));
        VRCHK(m->w_seqof.alloc((size_t)T * 4));
        // split-K planes of the weight-streaming path of short batches: 3 passes x 32 rows x (ksplit * n_pad <= 256 tiles of 256)
        VRCHK(m->w_hp_part.alloc((size_t)3 * 32 * 65536 * 4));
    }
    return VR_OK;
}

extern "C" int vr_model_finalize(vr_model_t m) {
    if (!m) return fail(VR_ERR_INVALID, "NULL model");
    VRCHK(set_dev(m->device));
    const vr_config_t& c = m->c;
    const int E = m->E;
    // ---- completeness
    auto need = [&](bool ok, const char* what) { return ok ? VR_OK : fail(VR_ERR_STATE, "missing weight: %s", what); };
    VRCHK(need(m->patch.has_w && m->patch.has_b, "vpm.patch_embed.proj"));
    VRCHK(need(m->has_pos, "vpm.pos_embed"));
    VRCHK(need(m->vit_nw.ok && m->vit_nb.ok, "vpm.norm"));
    for (int n = 0; n < c.vit_depth; ++n) {
        const VitBlock& b = m->blocks[n];
        const bool ok = b.n1w.ok && b.n1b.ok && b.n2w.ok && b.n2b.ok && b.qkv.has_w && b.qkv.has_b && b.proj.has_w &&
                        b.proj.has_b && b.fc1.has_w && b.fc1.has_b && b.fc2.has_w && b.fc2.has_b;
        if (!ok) return fail(VR_ERR_STATE, "missing weight in vpm.blocks.%d", n);
    }
    VRCHK(need(m->has_query && m->has_inproj && m->has_inproj_b, "resampler.query / attn.in_proj"));
    VRCHK(need(m->r_kvproj.has_w && m->r_kv.has_w && m->r_kv.has_b && m->r_out.has_w && m->r_out.has_b && m->r_proj.has_w,
               "resampler linear weights"));
    VRCHK(need(m->r_lnq_w.ok && m->r_lnq_b.ok && m->r_lnkv_w.ok && m->r_lnkv_b.ok && m->r_lnpost_w.ok && m->r_lnpost_b.ok,
               "resampler layer norms"));
    VRCHK(need(m->has_embed && m->final_norm.ok, "llm.model.embed_tokens / norm"));
    for (int n = 0; n < c.num_layers; ++n) {
        const DecLayer& l = m->layers[n];
        const bool ok = l.ln1.ok && l.ln2.ok && l.parts_qkv == 7 && l.parts_gu == 3 && l.o.has_w && l.down.has_w;
        if (!ok) return fail(VR_ERR_STATE, "missing weight in llm.model.layers.%d", n);
    }
    // ---- resampler query projection (batch-invariant, computed once in fp32 on the host):
    //      q = (ln_q(query) + sincos(8x8)) @ Wq^T + bq          resampler.py:157-160
    {
        const int Q = m->Q;
        std::vector<float> lw(E), lb(E), pq;
        HIPCHK(hipMemcpy(lw.data(), m->r_lnq_w.v.p, (size_t)E * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(lb.data(), m->r_lnq_b.v.p, (size_t)E * 4, hipMemcpyDeviceToHost));
        const int g = (int)lround(sqrt((double)Q));
        sincos_2d_host(E, g, g, pq);
        std::vector<float> x((size_t)Q * E), out((size_t)Q * E);
        for (int q = 0; q < Q; ++q) {
            const float* s = m->r_query_host.data() + (size_t)q * E;
            double mu = 0; for (int i = 0; i < E; ++i) mu += s[i]; mu /= E;
            double var = 0; for (int i = 0; i < E; ++i) { const double d = s[i] - mu; var += d * d; } var /= E;
            const float rstd = (float)(1.0 / sqrt(var + (double)c.resampler_ln_eps));
            for (int i = 0; i < E; ++i) x[(size_t)q * E + i] = ((float)(s[i] - mu)) * rstd * lw[i] + lb[i] + pq[(size_t)q * E + i];
        }
        for (int q = 0; q < Q; ++q)
            for (int n = 0; n < E; ++n) {
                const float* wr = m->r_wq_host.data() + (size_t)n * E;
                const float* xr = x.data() + (size_t)q * E;
                float acc = 0.f;
                for (int i = 0; i < E; ++i) acc += xr[i] * wr[i];
                out[(size_t)q * E + n] = acc + m->r_bq_host[n];
            }
        DevBuf t;
        VRCHK(t.alloc(out.size() * 4));
        HIPCHK(hipMemcpy(t.p, out.data(), out.size() * 4, hipMemcpyHostToDevice));
        VRCHK(m->r_q.alloc((size_t)pad128(Q) * E * 2));
        HIPCHK(launch_f32_to_bf16(t.as<float>(), m->r_q.p, out.size(), 0));
        HIPCHK(hipDeviceSynchronize());
        t.free();
    }
    // ---- RoPE table [pos][cos 32 | sin 32], fp32 (modeling_minicpm.py:142-172)
    {
        m->rope_len = std::max(c.max_tokens, 16);
        const std::vector<float> tab = rope_table_host(c.rope_theta, m->rope_len);
        VRCHK(m->rope.alloc(tab.size() * 4));
        HIPCHK(hipMemcpy(m->rope.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    }
    // ---- split-precision text path: a checkpoint whose fp32 weights are bf16-exact (or that came as bf16) has no
    //      low halves — drop the all-zero buffers, the passes over them would add nothing but weight reads
    if (c.text_split_precision) {
        DevBuf flag;
        VRCHK(flag.alloc(4));
        for (auto& l : m->layers)
            for (Linear* L : {&l.qkv_lo, &l.o_lo, &l.gu_lo, &l.down_lo})
                if (L->has_w) HIPCHK(launch_any_nonzero16(L->w.p, L->w.bytes / 2, flag.as<int>(), 0));
        int any = 0;
        HIPCHK(hipMemcpy(&any, flag.p, 4, hipMemcpyDeviceToHost));
        if (!any)
            for (auto& l : m->layers)
                for (Linear* L : {&l.qkv_lo, &l.o_lo, &l.gu_lo, &l.down_lo}) { L->w.free(); L->has_w = false; }
        if (m->has_embed_lo) {
            HIPCHK(hipMemset(flag.p, 0, 4));
            HIPCHK(launch_any_nonzero16(m->embed_lo.p, m->embed_lo.bytes / 2, flag.as<int>(), 0));
            HIPCHK(hipMemcpy(&any, flag.p, 4, hipMemcpyDeviceToHost));
            if (!any) { m->embed_lo.free(); m->has_embed_lo = false; }
        }
    }
    if (!m->w_h.p) VRCHK(alloc_workspace(m));
    m->finalized = true;
    return VR_OK;
}


int get_grid(vr_model_s* m, int gh, int gw, GridTables** out) {
    auto key = std::make_pair(gh, gw);
    auto it = m->grids.find(key);
    if (it != m->grids.end()) { *out = &it->second; return VR_OK; }
    const int N = gh * gw, D = m->D, Dp = m->Dp, E = m->E;
    GridTables g;
    g.gh = gh; g.gw = gw;
    {   // K3: timm resample_abs_pos_embed, once per grid instead of once per forward
        std::vector<float> rs, padded((size_t)N * Dp, 0.f);
        resample_pos_host(m->pos_embed_host, m->c.vit_pos_grid, D, gh, gw, rs);
        for (int r = 0; r < N; ++r) memcpy(padded.data() + (size_t)r * Dp, rs.data() + (size_t)r * D, (size_t)D * 4);
        VRCHK(g.vit_pos.alloc(padded.size() * 4));
        HIPCHK(hipMemcpy(g.vit_pos.p, padded.data(), padded.size() * 4, hipMemcpyHostToDevice));
    }
    {   // K10/K11: k = (x + pos) Wk^T + bk = x Wk^T + bk + (pos Wk^T); the last term is a
        // per-position bias computed once per grid with two bf16 passes (hi + lo split of the
        // fp32 sincos table keeps ~16 mantissa bits).
        std::vector<float> sc;
        sincos_2d_host(E, gh, gw, sc);
        const int Np = pad128(N);
        DevBuf f32, hi, lo, tmp;
        VRCHK(f32.alloc((size_t)Np * E * 4));
        VRCHK(hi.alloc((size_t)Np * E * 2));
        VRCHK(lo.alloc((size_t)Np * E * 2));
        VRCHK(tmp.alloc((size_t)Np * E * 4));
        VRCHK(g.pos_k.alloc((size_t)Np * E * 4));
        HIPCHK(hipMemcpy(f32.p, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(launch_split_bf16(f32.as<float>(), hi.p, lo.p, (size_t)N * E, 0));
        GemmArgs a{};
        a.A = hi.p; a.lda = E; a.W = m->r_kv.w.p; a.ldw = m->r_kv.k_pad; a.M = N; a.N = E; a.K = E;
        a.out = tmp.p; a.ldo = E; a.alpha = 1.f;
        HIPCHK(launch_gemm(a, EPI_F32, GEMM_VARIANT_GLDS, 0));
        a.A = lo.p; a.resid = tmp.as<float>(); a.out = g.pos_k.p;
        HIPCHK(launch_gemm(a, EPI_RESID, GEMM_VARIANT_GLDS, 0));
        HIPCHK(hipDeviceSynchronize());
        f32.free(); hi.free(); lo.free(); tmp.free();
    }
    auto ins = m->grids.emplace(key, std::move(g));
    *out = &ins.first->second;
    return VR_OK;
}

// ---------------------------------------------------------------------------------- taps ---
int tap_store(vr_model_s* m, const char* name, const void* dev, int64_t rows, int64_t cols, int64_t ld, bool is_bf16, hipStream_t s) {
    if (!m->taps_on) return VR_OK;
    HIPCHK(hipStreamSynchronize(s));
    Tap& t = m->taps[name];
    t.rows = rows; t.cols = cols;
    t.data.resize((size_t)rows * cols);
    const size_t esz = is_bf16 ? 2 : 4;
    std::vector<char> raw((size_t)rows * ld * esz);
    HIPCHK(hipMemcpy(raw.data(), dev, raw.size(), hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t cc = 0; cc < cols; ++cc) {
            if (is_bf16) {
                uint16_t b; memcpy(&b, raw.data() + ((size_t)r * ld + cc) * 2, 2);
                uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4);
                t.data[(size_t)r * cols + cc] = f;
            } else {
                float f; memcpy(&f, raw.data() + ((size_t)r * ld + cc) * 4, 4);
                t.data[(size_t)r * cols + cc] = f;
            }
        }
    return VR_OK;
}

extern "C" int vr_model_set_pooling(vr_model_t m, int32_t mode) {
    if (!m) return fail(VR_ERR_INVALID, "NULL model");
    if (mode < VR_POOL_WMEAN || mode > VR_POOL_CLS) return fail(VR_ERR_INVALID, "pooling mode %d: 0 wmean, 1 mean, 2 lasttoken, 3 cls", mode);
    m->pool_mode = mode;
    return VR_OK;
}

extern "C" int vr_model_set_taps(vr_model_t m, int32_t enable) {
    if (!m) return fail(VR_ERR_INVALID, "NULL model");
    m->taps_on = enable != 0;
    if (!enable) m->taps.clear();
    return VR_OK;
}

extern "C" int vr_model_tap(vr_model_t m, const char* name, float* out, int64_t rows, int64_t cols) {
    if (!m || !name || !out) return fail(VR_ERR_INVALID, "NULL argument");
    auto it = m->taps.find(name);
    if (it == m->taps.end()) return fail(VR_ERR_STATE, "tap %s not recorded (enable taps, then encode)", name);
    const Tap& t = it->second;
    if (rows > t.rows || cols != t.cols) return fail(VR_ERR_INVALID, "tap %s is [%lld][%lld]", name, (long long)t.rows, (long long)t.cols);
    memcpy(out, t.data.data(), (size_t)rows * cols * 4);
    return VR_OK;
}

// A second handle on the SAME weights with its own workspace, per-grid tables, pinned arena and
// profiling state: two batches can then be in flight on two HIP streams (the tails and the
// LayerNorm/epilogue phases of one batch's kernels overlap the other's GEMMs).  The source handle
// must outlive its clones.
extern "C" int vr_model_clone(vr_model_t src, vr_model_t* out) {
    if (!src || !out) return fail(VR_ERR_INVALID, "src/out is NULL");
    if (!src->finalized) return fail(VR_ERR_STATE, "vr_model_clone before vr_model_finalize");
    VRCHK(set_dev(src->device));
    vr_model_s* m = new vr_model_s(*src);          // shallow: the weight buffers are aliased, never freed by the clone
    m->borrowed = true;
    for (DevBuf* b : {&m->w_hvit, &m->w_xn, &m->w_qkv, &m->w_att, &m->w_mlp, &m->w_kv32, &m->w_xkv, &m->w_KV,
                      &m->w_ratt, &m->w_rout, &m->w_rln, &m->w_h, &m->w_dxn, &m->w_part, &m->w_dqkv, &m->w_datt, &m->w_dact,
                      &m->w_cu, &m->w_ids, &m->w_seq, &m->w_pos, &m->w_rowmap, &m->w_imgptr, &m->w_pix, &m->w_out,
                      &m->w_hp_hi, &m->w_hp_planes, &m->w_hp_qkv, &m->w_hp_att, &m->w_hp_gu, &m->w_seqof, &m->w_hp_part, &m->w_hidden}) {
        b->free();                                 // (a non-owning alias after the copy: just forget it)
    }
    m->grids.clear();                              // (entries alias the source's tables; the clone builds its own)
    m->taps.clear(); m->taps_on = false;
    m->prof_on = false;
    for (auto& pc : m->prof) { pc.ev.clear(); pc.used = 0; pc.ms = 0; pc.flops = 0; pc.launches = 0; }
    m->arena = nullptr; m->arena_cap = 0; m->arena_used = 0; m->arena_ev = nullptr; m->arena_pending = false; m->arena_open = false;
    const int r = alloc_workspace(m);
    if (r != VR_OK) { (void)vr_model_destroy(m); return r; }
    *out = m;
    return VR_OK;
}

extern "C" int vr_model_set_profile(vr_model_t m, int32_t enable) {
    if (!m) return fail(VR_ERR_INVALID, "NULL model");
    VRCHK(set_dev(m->device));
    VRCHK(prof_collect(m));
    m->prof_on = enable != 0;
    m->prof_level = enable == 2 ? 2 : (enable ? 1 : 0);
    for (auto& p : m->prof) { p.ms = 0; p.flops = 0; p.launches = 0; p.used = 0; }
    return VR_OK;
}

extern "C" int vr_model_get_profile(vr_model_t m, int32_t cls, double* total_ms, int64_t* launches, double* total_flops) {
    if (!m || cls < 0 || cls >= VR_PROF_CLASSES || !total_ms || !launches || !total_flops)
        return fail(VR_ERR_INVALID, "bad profile arguments");
    VRCHK(set_dev(m->device));
    VRCHK(prof_collect(m));
    *total_ms = m->prof[cls].ms; *launches = m->prof[cls].launches; *total_flops = m->prof[cls].flops;
    return VR_OK;
}
