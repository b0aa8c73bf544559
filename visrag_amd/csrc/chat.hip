// MiniCPM-V 2.0 answer generation on the model's weights (MiniCPMV.generate / chat, modeling_minicpmv.py:218-237, 276-400;
// the decoder + head of modeling_minicpm.py:1147-1304, 1411-1412).  The prefill is the encode pass itself (bf16 route) with a
// per-layer hook that keeps the rope'd K / V rows; a decode step streams every weight once for all its rows (gemm_skinny.hip).
// Cache: prompt planes per prompt SLOT [layer][K|V][max_slots][max_len][E], tail planes (generated tokens) per ROW
// [layer][K|V][max_rows][max_new][E], bf16.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "model.h"

struct vr_chat_s {
    vr_model_s* model = nullptr;
    vr_model_t work = nullptr;            // vr_model_clone of `model`: the prefill pass's workspace
    vr_chat_config_t c{};
    int E = 0, H = 0, L = 0, V = 0, Vpad = 0, Ip = 0, words = 0;
    Linear head;
    DevBuf norm_w;                        // final norm weight * dim_model_base / hidden (the /scale of the head's input, :1411)
    DevBuf rope;                          // f32 [max_len][64], the table of vr_model_finalize extended to max_len
    DevBuf prompt, tails, seen;           // caches; seen-id bit sets [max_rows][words]
    DevBuf w_h, w_xn, w_q, w_att, w_act, w_part, w_po, w_pml, w_logits, w_lse, w_sel, w_out, w_reps, w_move, w_move_seen;
    DevBuf w_pxn;                         // bf16 [2 * CHAT_MAX_ROWS][E]: the normed last rows of a batched prefill (the head reads 16 rows from any of the first 16)
    // vr_chat_score (allocated at its first call): bf16 [pad256(max_tokens)][k_pad] normed rows, the head's partials,
    // targets int32 [max_tokens], results 4 x [max_tokens] words, pooled reps of the pass f32 [max_seqs][E] (unused)
    DevBuf s_xn, s_part, s_tgt, s_out, s_reps;
    std::vector<int> plen;                // per slot: prompt tokens (0 = none)
    std::vector<int> row_slot, row_len;   // per row: its prompt slot (-1 = unbound), generated tokens in its tail
    std::vector<int> lpos;                // per row: its logits row in w_logits (-1 = none)
    // per slot: the line of w_logits that still holds the logits of the prompt's LAST position (-1 = gone).  A prefill writes
    // them to line max_rows + row; decode steps write the lower half only, so the line survives a generation and is lost
    // when a prefill or an extend writes that line again
    std::vector<int> slot_lrow;
    std::vector<int> slot_gen;            // per slot: prefills so far (a caller that keeps a slot asks whether it is still its own)
};

static size_t chat_prompt_off(const vr_chat_s* ch, int l, int kv, int slot) {      // bytes
    return ((((size_t)l * 2 + kv) * ch->c.max_slots + slot) * (size_t)ch->c.max_len * ch->E) * 2;
}

// logits line `line` is about to be rewritten: no slot's prompt logits live there any more
static void chat_release_line(vr_chat_s* ch, int line) {
    for (int& l : ch->slot_lrow)
        if (l == line) l = -1;
}

extern "C" int vr_chat_create(vr_model_t m, const vr_chat_config_t* cfg, vr_chat_t* out) {
    if (!m || !cfg || !out) return fail(VR_ERR_INVALID, "NULL argument");
    if (!m->finalized) return fail(VR_ERR_STATE, "vr_chat_create before vr_model_finalize");
    if (cfg->max_rows < 1 || cfg->max_rows > CHAT_MAX_ROWS) return fail(VR_ERR_INVALID, "max_rows must be 1..%d", CHAT_MAX_ROWS);
    if (cfg->max_len < 2) return fail(VR_ERR_INVALID, "max_len must be at least 2");
    if (cfg->max_slots < 1 || cfg->max_slots > cfg->max_rows) return fail(VR_ERR_INVALID, "max_slots must be 1..max_rows");
    if (cfg->max_new < 1 || cfg->max_new >= cfg->max_len) return fail(VR_ERR_INVALID, "max_new must be 1..max_len - 1");
    if (!(cfg->dim_model_base > 0.f)) return fail(VR_ERR_INVALID, "dim_model_base must be positive");
    VRCHK(set_dev(m->device));
    vr_chat_s* ch = new vr_chat_s();
    auto bail = [&](int rc) { if (ch->work) vr_model_destroy(ch->work); delete ch; return rc; };
    ch->model = m;
    ch->c = *cfg;
    ch->E = m->E; ch->H = m->c.num_heads; ch->L = m->c.num_layers; ch->V = m->c.vocab_size; ch->Vpad = pad128(ch->V); ch->Ip = m->Ip;
    ch->words = (ch->V + 31) / 32;
    const int E = ch->E, R = cfg->max_rows, ML = cfg->max_len;
    int rc = vr_model_clone(m, &ch->work);
    if (rc) return bail(rc);
    {   // final norm weight with the head's input scale folded in
        std::vector<float> w(E);
        if (hipMemcpy(w.data(), m->final_norm.v.p, (size_t)E * 4, hipMemcpyDeviceToHost) != hipSuccess) return bail(fail(VR_ERR_HIP, "norm copy"));
        const float sc = cfg->dim_model_base / (float)E;
        for (float& x : w) x *= sc;
        if ((rc = ch->norm_w.alloc((size_t)E * 4))) return bail(rc);
        if (hipMemcpy(ch->norm_w.p, w.data(), (size_t)E * 4, hipMemcpyHostToDevice) != hipSuccess) return bail(fail(VR_ERR_HIP, "norm upload"));
    }
    {   // RoPE table of the model (vr_model_finalize), max_len positions
        const std::vector<float> tab = rope_table_host(m->c.rope_theta, ML);
        if ((rc = ch->rope.alloc(tab.size() * 4))) return bail(rc);
        if (hipMemcpy(ch->rope.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return bail(fail(VR_ERR_HIP, "rope upload"));
    }
    const size_t pcache = (size_t)ch->L * 2 * cfg->max_slots * ML * E * 2, tcache = (size_t)ch->L * 2 * R * cfg->max_new * E * 2;
    size_t part = 0;
    for (const DecLayer& l : m->layers)
        for (const Linear* w : {&l.qkv, &l.o, &l.gu, &l.down})
            part = std::max(part, (size_t)stream_ksplit(w->n_pad, w->k_pad) * CHAT_MAX_ROWS * w->n_pad);
    const size_t H = ch->H;
    if ((rc = ch->prompt.alloc(pcache)) || (rc = ch->tails.alloc(tcache)) || (rc = ch->seen.alloc((size_t)R * ch->words * 4)) ||
        (rc = ch->w_h.alloc((size_t)CHAT_MAX_ROWS * E * 4)) || (rc = ch->w_xn.alloc((size_t)CHAT_MAX_ROWS * E * 2)) ||
        (rc = ch->w_q.alloc((size_t)CHAT_MAX_ROWS * E * 2)) || (rc = ch->w_att.alloc((size_t)CHAT_MAX_ROWS * E * 2)) ||
        (rc = ch->w_act.alloc((size_t)CHAT_MAX_ROWS * ch->Ip * 2)) || (rc = ch->w_part.alloc(part * 4)) ||
        (rc = ch->w_po.alloc((size_t)CHAT_MAX_ROWS * H * CHAT_ATT_SPLITS * 64 * 4)) ||
        (rc = ch->w_pml.alloc((size_t)CHAT_MAX_ROWS * H * CHAT_ATT_SPLITS * 2 * 4)) ||
        (rc = ch->w_logits.alloc((size_t)2 * R * ch->Vpad * 4)) || (rc = ch->w_lse.alloc(CHAT_MAX_ROWS * 4)) ||
        (rc = ch->w_sel.alloc((size_t)CHAT_MAX_ROWS * CHAT_SEL_WGS * CHAT_TOPK_MAX * 8)) ||
        (rc = ch->w_out.alloc((size_t)CHAT_MAX_ROWS * CHAT_TOPK_MAX * 12)) || (rc = ch->w_reps.alloc((size_t)CHAT_MAX_ROWS * E * 4)) ||
        (rc = ch->w_pxn.alloc((size_t)2 * CHAT_MAX_ROWS * E * 2)) ||
        (rc = ch->w_move_seen.alloc((size_t)CHAT_MAX_ROWS * ch->words * 4)))
        return bail(rc);
    ch->plen.assign(cfg->max_slots, 0);
    ch->row_slot.assign(R, -1);
    ch->row_len.assign(R, 0);
    ch->lpos.assign(R, -1);
    ch->slot_lrow.assign(cfg->max_slots, -1);
    ch->slot_gen.assign(cfg->max_slots, 0);
    *out = ch;
    return VR_OK;
}

extern "C" int vr_chat_destroy(vr_chat_t ch) {
    if (!ch) return VR_OK;
    (void)hipSetDevice(ch->model->device);
    (void)hipDeviceSynchronize();
    if (ch->work) vr_model_destroy(ch->work);
    delete ch;
    return VR_OK;
}

extern "C" int vr_chat_load_head(vr_chat_t ch, const void* data, const int64_t* shape, int32_t ndim, int32_t dtype, int32_t on_device) {
    if (!ch || !data || !shape) return fail(VR_ERR_INVALID, "NULL argument");
    if (dtype != VR_DTYPE_F32 && dtype != VR_DTYPE_BF16) return fail(VR_ERR_INVALID, "bad dtype %d", dtype);
    if (!shape_is(shape, ndim, {ch->V, ch->E})) return fail(VR_ERR_INVALID, "lm_head must be [vocab_size][hidden_size]");
    VRCHK(set_dev(ch->model->device));
    const int bf = dtype == VR_DTYPE_BF16;
    Staged st;
    VRCHK(stage(data, (size_t)ch->V * ch->E * (bf ? 2 : 4), on_device, st));
    return load_linear_part(ch->head, ch->V, ch->E, st.dev, bf, ch->V, ch->E, 0, ch->V, 0, 0);
}

// logits f32 of the step rows xn [n][E] (already normed and scaled) -> w_logits rows [lrow0, lrow0 + n)
static int chat_head(vr_chat_s* ch, int n, int lrow0, hipStream_t s) {
    GemmArgs a = gemm_args(ch->w_xn.p, ch->E, ch->head, n, ch->w_logits.as<float>() + (size_t)lrow0 * ch->Vpad, ch->Vpad);
    HIPCHK(launch_gemm_skinny(a, s));
    return VR_OK;
}

struct ChatPrefillCtx { vr_chat_s* ch; int slot; };
static int chat_prefill_layer(void* ctx, int l, const void* qkv, int ldqkv, int T, hipStream_t s) {
    const ChatPrefillCtx* p = (const ChatPrefillCtx*)ctx;
    vr_chat_s* ch = p->ch;
    HIPCHK(launch_chat_prompt_kv(qkv, ldqkv, T, ch->E, (char*)ch->prompt.p + chat_prompt_off(ch, l, 0, p->slot),
                                 (char*)ch->prompt.p + chat_prompt_off(ch, l, 1, p->slot), s));
    return VR_OK;
}

extern "C" int vr_chat_prefill(vr_chat_t ch, int32_t slot, int32_t row, const uint8_t* const* slices, const int32_t* slice_hw,
                               int32_t n_slices, int32_t slices_on_device, const int32_t* input_ids, int32_t T,
                               const int32_t* vision_rows, void* stream) {
    if (!ch || !input_ids) return fail(VR_ERR_INVALID, "NULL argument");
    if (!ch->head.has_w) return fail(VR_ERR_STATE, "vr_chat_load_head has not run");
    if (slot < 0 || slot >= ch->c.max_slots || row < 0 || row >= ch->c.max_rows) return fail(VR_ERR_INVALID, "slot / row out of range");
    if (T < 1) return fail(VR_ERR_INVALID, "empty prompt");
    if (T > ch->c.max_len - 1) return fail(VR_ERR_CAPACITY, "prompt of %d tokens leaves no room below max_len=%d", T, ch->c.max_len);
    if (T > ch->work->c.max_tokens) return fail(VR_ERR_CAPACITY, "prompt of %d tokens exceeds the model's max_tokens=%d", T, ch->work->c.max_tokens);
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    vr_model_s* w = ch->work;
    ch->plen[slot] = 0;                                  // the slot's cache is rewritten from here on
    ch->slot_lrow[slot] = -1;
    ch->slot_gen[slot]++;
    for (int r = 0; r < ch->c.max_rows; ++r)
        if (ch->row_slot[r] == slot) { ch->row_slot[r] = -1; ch->row_len[r] = 0; ch->lpos[r] = -1; }
    ChatPrefillCtx ctx{ch, slot};
    EncodeHook hook;
    hook.bf16_route = true;                              // the reference generator runs in bf16 (generate.py: torch_dtype=bfloat16)
    hook.layer = chat_prefill_layer;
    hook.ctx = &ctx;
    const int32_t seq[2] = {0, T};
    w->arena_open = false;
    int rc = encode_impl(w, slices, slice_hw, n_slices, slices_on_device, input_ids, seq, 1, vision_rows, ch->w_reps.as<float>(), 1,
                         stream, nullptr, 0, &hook);
    arena_close(w, stream);
    if (rc) return rc;
    // last prompt token: final RMSNorm (scaled weight) -> head, modeling_minicpm.py:1411-1412
    const vr_config_t& c = w->c;
    HIPCHK(launch_rmsnorm(w->w_h.as<float>() + (size_t)(T - 1) * ch->E, 1, ch->E, ch->E, ch->norm_w.as<float>(), c.rms_norm_eps, ch->w_xn.p,
                          ch->E, s));
    const int lrow = ch->c.max_rows + row;               // prefill logits live in the upper half of w_logits
    chat_release_line(ch, lrow);
    VRCHK(chat_head(ch, 1, lrow, s));
    HIPCHK(hipMemsetAsync((unsigned*)ch->seen.p + (size_t)row * ch->words, 0, (size_t)ch->words * 4, s));
    ch->plen[slot] = T;
    ch->row_slot[row] = slot;
    ch->row_len[row] = 0;
    ch->lpos[row] = lrow;
    ch->slot_lrow[slot] = lrow;
    return VR_OK;
}

// ---- batched prefill: B prompts in ONE packed encode pass (the pass is ragged already; this is the cache and logits side)
struct ChatPrefillBatchCtx { vr_chat_s* ch; ChatBatch bt; };
static int chat_prefill_batch_layer(void* ctx, int l, const void* qkv, int ldqkv, int T, hipStream_t s) {
    const ChatPrefillBatchCtx* p = (const ChatPrefillBatchCtx*)ctx;
    vr_chat_s* ch = p->ch;
    if (T != p->bt.off[p->bt.n]) return fail(VR_ERR_STATE, "prefill hook: %d rows, expected %d", T, p->bt.off[p->bt.n]);
    HIPCHK(launch_chat_prompt_scatter(p->bt, qkv, ldqkv, ch->E, ch->c.max_len, (char*)ch->prompt.p + chat_prompt_off(ch, l, 0, 0),
                                      (char*)ch->prompt.p + chat_prompt_off(ch, l, 1, 0), s));
    return VR_OK;
}

extern "C" int vr_chat_prefill_batch(vr_chat_t ch, int32_t B, const int32_t* slots, const int32_t* rows, const uint8_t* const* slices,
                                     const int32_t* slice_hw, int32_t n_slices, int32_t slices_on_device, const int32_t* input_ids,
                                     const int32_t* seq_offsets, const int32_t* vision_rows, void* stream) {
    if (!ch || !slots || !rows || !input_ids || !seq_offsets) return fail(VR_ERR_INVALID, "NULL argument");
    if (!ch->head.has_w) return fail(VR_ERR_STATE, "vr_chat_load_head has not run");
    if (B < 1) return fail(VR_ERR_INVALID, "B must be positive");
    const int R = ch->c.max_rows;
    vr_model_s* w = ch->work;
    // ---- every check before any state changes
    if (B > ch->c.max_slots || B > R) return fail(VR_ERR_INVALID, "%d prompts exceed max_slots=%d / max_rows=%d", B, ch->c.max_slots, R);
    if (seq_offsets[0] != 0) return fail(VR_ERR_INVALID, "seq_offsets[0] must be 0");
    std::vector<char> slot_used(ch->c.max_slots, 0), row_used(R, 0);
    for (int b = 0; b < B; ++b) {
        const int sl = slots[b], r = rows[b], T = seq_offsets[b + 1] - seq_offsets[b];
        if (sl < 0 || sl >= ch->c.max_slots || slot_used[sl]) return fail(VR_ERR_INVALID, "prompt %d: slot %d out of range or repeated", b, sl);
        if (r < 0 || r >= R || row_used[r]) return fail(VR_ERR_INVALID, "prompt %d: row %d out of range or repeated", b, r);
        slot_used[sl] = 1; row_used[r] = 1;
        if (T < 1) return fail(VR_ERR_INVALID, "empty prompt %d", b);
        if (T > ch->c.max_len - 1) return fail(VR_ERR_CAPACITY, "prompt %d of %d tokens leaves no room below max_len=%d", b, T, ch->c.max_len);
    }
    const int Ttot = seq_offsets[B];
    if (Ttot > w->c.max_tokens) return fail(VR_ERR_CAPACITY, "%d prompt tokens exceed the model's max_tokens=%d", Ttot, w->c.max_tokens);
    if (B > w->c.max_seqs) return fail(VR_ERR_CAPACITY, "%d prompts exceed the model's max_seqs=%d", B, w->c.max_seqs);
    for (int t = 0; t < Ttot; ++t)
        if (input_ids[t] < 0 || input_ids[t] >= ch->V) return fail(VR_ERR_INVALID, "token id %d out of range at %d", input_ids[t], t);
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    // the slots' caches are rewritten from here on: rows that continued them lose their tails
    auto unbind = [&]() {
        for (int b = 0; b < B; ++b) { ch->plen[slots[b]] = 0; ch->slot_lrow[slots[b]] = -1; ch->slot_gen[slots[b]]++; }
        for (int r = 0; r < R; ++r)
            if (ch->row_slot[r] >= 0 && slot_used[ch->row_slot[r]]) { ch->row_slot[r] = -1; ch->row_len[r] = 0; ch->lpos[r] = -1; }
    };
    unbind();
    ChatPrefillBatchCtx ctx{ch, {}};
    ctx.bt.n = B;
    for (int b = 0; b < B; ++b) { ctx.bt.off[b] = seq_offsets[b]; ctx.bt.idx[b] = slots[b]; }
    ctx.bt.off[B] = Ttot;
    EncodeHook hook;
    hook.bf16_route = true;
    hook.layer = chat_prefill_batch_layer;
    hook.ctx = &ctx;
    w->arena_open = false;
    int rc = encode_impl(w, slices, slice_hw, n_slices, slices_on_device, input_ids, seq_offsets, B, vision_rows, ch->w_reps.as<float>(), 1,
                         stream, nullptr, 0, &hook);
    arena_close(w, stream);
    if (rc) return rc;
    // last prompt tokens -> final RMSNorm (scaled weight), the rows in the order of their logits rows: a run of adjacent logits
    // rows is one pass of the head over its weights
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return rows[a] < rows[b]; });
    ChatBatch lr = ctx.bt;
    for (int j = 0; j < B; ++j) lr.idx[order[j]] = j;
    HIPCHK(launch_chat_last_rows(lr, w->w_h.as<float>(), ch->E, ch->norm_w.as<float>(), w->c.rms_norm_eps, ch->w_pxn.p, s));
    for (int j = 0; j < B;) {
        int n = 1;
        while (j + n < B && rows[order[j + n]] == rows[order[j]] + n) ++n;
        GemmArgs a = gemm_args((const char*)ch->w_pxn.p + (size_t)j * ch->E * 2, ch->E, ch->head, n,
                               ch->w_logits.as<float>() + (size_t)(R + rows[order[j]]) * ch->Vpad, ch->Vpad);
        HIPCHK(launch_gemm_skinny(a, s));
        j += n;
    }
    for (int b = 0; b < B; ++b) chat_release_line(ch, R + rows[b]);
    for (int b = 0; b < B; ++b) {
        const int r = rows[b];
        HIPCHK(hipMemsetAsync((unsigned*)ch->seen.p + (size_t)r * ch->words, 0, (size_t)ch->words * 4, s));
        ch->slot_lrow[slots[b]] = R + r;
        ch->plen[slots[b]] = seq_offsets[b + 1] - seq_offsets[b];
        ch->row_slot[r] = slots[b];
        ch->row_len[r] = 0;
        ch->lpos[r] = R + r;
    }
    return VR_OK;
}

extern "C" int vr_chat_step(vr_chat_t ch, int32_t n, const int32_t* slots, const int32_t* rows, const int32_t* tokens, void* stream) {
    if (!ch || !slots || !rows || !tokens) return fail(VR_ERR_INVALID, "NULL argument");
    if (!ch->head.has_w) return fail(VR_ERR_STATE, "vr_chat_load_head has not run");
    const int R = ch->c.max_rows;
    if (n < 1) return fail(VR_ERR_INVALID, "n must be positive");
    if (n > R) return fail(VR_ERR_CAPACITY, "%d rows exceed max_rows=%d", n, R);
    // ---- every check before any state changes
    ChatStep st{};
    st.n = n;
    std::vector<char> used(R, 0);
    for (int i = 0; i < n; ++i) {
        const int sl = slots[i], r = rows[i], t = tokens[i];
        if (sl < 0 || sl >= ch->c.max_slots || ch->plen[sl] <= 0) return fail(VR_ERR_INVALID, "step row %d: slot %d holds no prompt", i, sl);
        if (r < 0 || r >= R || used[r]) return fail(VR_ERR_INVALID, "step row %d: row %d out of range or repeated", i, r);
        if (t < 0 || t >= ch->V) return fail(VR_ERR_INVALID, "token id %d out of range", t);
        used[r] = 1;
        if (ch->row_slot[r] != sl && ch->row_len[r] > 0) return fail(VR_ERR_INVALID, "row %d continues slot %d, not %d", r, ch->row_slot[r], sl);
        const int len = ch->row_slot[r] == sl ? ch->row_len[r] : 0;
        if (ch->plen[sl] + len + 1 > ch->c.max_len || len + 1 > ch->c.max_new)
            return fail(VR_ERR_CAPACITY, "row %d would exceed max_len=%d / max_new=%d", r, ch->c.max_len, ch->c.max_new);
        st.row[i] = r; st.slot[i] = sl; st.tail[i] = len; st.pos[i] = ch->plen[sl] + len; st.token[i] = t;
    }
    const int S = chat_step_groups(st, ch->plen.data(), ch->c.max_slots);      // groups and their prompt-key ranges
    if (!S) return fail(VR_ERR_INVALID, "the rows of a slot must be adjacent");
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    vr_model_s* m = ch->model;
    const vr_config_t& c = m->c;
    const int E = ch->E;
    for (int i = 0; i < n; ++i)                          // a row that starts on a slot starts with an empty seen set
        if (ch->row_slot[rows[i]] != slots[i])
            HIPCHK(hipMemsetAsync((unsigned*)ch->seen.p + (size_t)rows[i] * ch->words, 0, (size_t)ch->words * 4, s));
    float* h = ch->w_h.as<float>();
    float* part = ch->w_part.as<float>();
    HIPCHK(launch_chat_embed(st, m->embed.p, E, c.scale_emb, h, ch->seen.as<unsigned>(), ch->words, s));
    const ChatCaps caps{ch->c.max_slots, ch->c.max_len, R, ch->c.max_new};
    int pend_ks = 0;                                     // > 0: h still lacks residual_scale * (the last projection's planes)
    auto norm = [&](const float* wn) -> int {
        if (pend_ks) HIPCHK(launch_rmsnorm_accum(h, n, E, E, part, pend_ks, (size_t)n * E, E, c.residual_scale, wn, c.rms_norm_eps, ch->w_xn.p, E, s));
        else HIPCHK(launch_rmsnorm(h, n, E, E, wn, c.rms_norm_eps, ch->w_xn.p, E, s));
        pend_ks = 0;
        return VR_OK;
    };
    for (int l = 0; l < ch->L; ++l) {
        const DecLayer& Ly = m->layers[l];
        VRCHK(norm(Ly.ln1.v.as<float>()));
        {
            GemmArgs a = gemm_args(ch->w_xn.p, E, Ly.qkv, n, part, Ly.qkv.n_pad);
            a.ksplit = stream_ksplit(Ly.qkv.n_pad, Ly.qkv.k_pad); a.split_stride = (size_t)n * Ly.qkv.n_pad;
            HIPCHK(launch_gemm_skinny(a, s));
            HIPCHK(launch_chat_qkv(st, part, a.ksplit, a.split_stride, Ly.qkv.n_pad, ch->rope.as<float>(), E, ch->H, ch->w_q.p, ch->tails.p, l,
                                   ch->c.max_rows, ch->c.max_new, s));
        }
        HIPCHK(launch_chat_attn(st, ch->w_q.p, ch->prompt.p, ch->tails.p, l, E, ch->H, caps, S, ch->w_po.as<float>(),
                                ch->w_pml.as<float>(), ch->w_att.p, s));
        {
            GemmArgs a = gemm_args(ch->w_att.p, E, Ly.o, n, part, E);
            a.ksplit = stream_ksplit(Ly.o.n_pad, Ly.o.k_pad); a.split_stride = (size_t)n * E;
            HIPCHK(launch_gemm_skinny(a, s));
            pend_ks = a.ksplit;
        }
        VRCHK(norm(Ly.ln2.v.as<float>()));
        {
            const int N2 = Ly.gu.n_pad;
            GemmArgs g = gemm_args(ch->w_xn.p, E, Ly.gu, n, ch->w_act.p, ch->Ip);
            g.ksplit = stream_ksplit(N2, Ly.gu.k_pad);
            if (g.ksplit == 1) {
                HIPCHK(launch_gemm_skinny(g, s, true));
            } else {
                g.out = part; g.ldo = N2; g.split_stride = (size_t)n * N2;
                HIPCHK(launch_gemm_skinny(g, s));
                HIPCHK(launch_swiglu_sum(part, g.ksplit, (size_t)n * N2, N2, n, m->I, ch->w_act.p, ch->Ip, s));
            }
        }
        {
            GemmArgs a = gemm_args(ch->w_act.p, ch->Ip, Ly.down, n, part, E);
            a.ksplit = stream_ksplit(Ly.down.n_pad, Ly.down.k_pad); a.split_stride = (size_t)n * E;
            HIPCHK(launch_gemm_skinny(a, s));
            pend_ks = a.ksplit;
        }
    }
    VRCHK(norm(ch->norm_w.as<float>()));
    VRCHK(chat_head(ch, n, 0, s));
    for (int r = 0; r < R; ++r)
        if (ch->lpos[r] >= 0 && ch->lpos[r] < R) ch->lpos[r] = -1;        // step logits rows are overwritten
    for (int i = 0; i < n; ++i) {
        ch->row_slot[rows[i]] = slots[i];
        ch->row_len[rows[i]] = st.tail[i] + 1;
        ch->lpos[rows[i]] = i;
    }
    return VR_OK;
}

extern "C" int vr_chat_select(vr_chat_t ch, int32_t mode, int32_t n_groups, const int32_t* group_offsets, const int32_t* rows,
                              const float* beam_scores, int32_t k, float repetition_penalty, float temperature, int32_t top_k,
                              uint64_t seed, int32_t step, float* out_scores, int32_t* out_tokens, int32_t* out_parents, void* stream) {
    if (!ch || !group_offsets || !rows || !out_scores || !out_tokens || !out_parents) return fail(VR_ERR_INVALID, "NULL argument");
    if (mode < VR_CHAT_GREEDY || mode > VR_CHAT_SAMPLE) return fail(VR_ERR_INVALID, "mode %d", mode);
    if (n_groups < 1 || group_offsets[0] != 0) return fail(VR_ERR_INVALID, "bad groups");
    const int n = group_offsets[n_groups];
    if (n > CHAT_MAX_ROWS || n > ch->c.max_rows) return fail(VR_ERR_CAPACITY, "%d rows exceed max_rows", n);
    if (!(repetition_penalty > 0.f)) return fail(VR_ERR_INVALID, "repetition_penalty must be positive");
    ChatSel sel{};
    sel.n = n; sel.groups = n_groups;
    for (int g = 0; g <= n_groups; ++g) sel.g_lo[g] = group_offsets[g];
    for (int g = 0; g < n_groups; ++g) {
        const int nb = group_offsets[g + 1] - group_offsets[g];
        if (nb < 1) return fail(VR_ERR_INVALID, "empty group %d", g);
        if (mode != VR_CHAT_BEAM && nb != 1) return fail(VR_ERR_INVALID, "greedy / sampling groups hold one row");
    }
    for (int i = 0; i < n; ++i) {
        const int r = rows[i];
        if (r < 0 || r >= ch->c.max_rows || ch->lpos[r] < 0) return fail(VR_ERR_STATE, "row %d has no logits", r);
        sel.lrow[i] = ch->lpos[r]; sel.srow[i] = r;
        sel.bscore[i] = mode == VR_CHAT_BEAM && beam_scores ? beam_scores[i] : 0.f;
    }
    int K = k;
    if (mode == VR_CHAT_SAMPLE) {
        if (k != 1 || !(temperature > 0.f)) return fail(VR_ERR_INVALID, "sampling: k must be 1 and temperature positive");
        K = top_k;
    }
    if (K < 1 || K > CHAT_TOPK_MAX || k < 1 || k > CHAT_TOPK_MAX) return fail(VR_ERR_INVALID, "k / top_k must be 1..%d", CHAT_TOPK_MAX);
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    float* o_score = ch->w_out.as<float>();
    int* o_tok = (int*)(o_score + CHAT_MAX_ROWS * CHAT_TOPK_MAX);
    int* o_par = o_tok + CHAT_MAX_ROWS * CHAT_TOPK_MAX;
    const int cm = mode == VR_CHAT_BEAM ? CHAT_SEL_BEAM : mode == VR_CHAT_SAMPLE ? CHAT_SEL_SAMPLE : CHAT_SEL_GREEDY;
    HIPCHK(launch_chat_select(sel, cm, ch->w_logits.as<float>(), ch->Vpad, ch->V, ch->seen.as<unsigned>(), ch->words, repetition_penalty,
                              temperature, K, k, (unsigned long long)seed, (unsigned)step, ch->w_lse.as<float>(),
                              ch->w_sel.as<unsigned long long>(), o_score, o_tok, o_par, s));
    const size_t cnt = (size_t)n_groups * k;
    HIPCHK(hipMemcpyAsync(out_scores, o_score, cnt * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_tokens, o_tok, cnt * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_parents, o_par, cnt * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_chat_sample(vr_chat_t ch, int32_t n, const int32_t* rows, float repetition_penalty, float temperature, int32_t top_k,
                              double top_p, uint64_t seed, int32_t step, float* out_scores, int32_t* out_tokens, int32_t* out_kept,
                              int32_t* out_cut, void* stream) {
    if (!ch || !rows || !out_scores || !out_tokens || !out_kept || !out_cut) return fail(VR_ERR_INVALID, "NULL argument");
    if (n < 1) return fail(VR_ERR_INVALID, "n must be positive");
    if (n > CHAT_MAX_ROWS || n > ch->c.max_rows) return fail(VR_ERR_CAPACITY, "%d rows exceed max_rows", n);
    if (!(repetition_penalty > 0.f)) return fail(VR_ERR_INVALID, "repetition_penalty must be positive");
    if (!(temperature > 0.f)) return fail(VR_ERR_INVALID, "temperature must be positive");
    if (top_k < 0) return fail(VR_ERR_INVALID, "top_k must be 0 (off) or positive");
    if (!(top_p > 0.0 && top_p <= 1.0)) return fail(VR_ERR_INVALID, "top_p must be in (0, 1]");
    ChatSel sel{};
    sel.n = n; sel.groups = n;
    for (int i = 0; i < n; ++i) {
        const int r = rows[i];
        if (r < 0 || r >= ch->c.max_rows || ch->lpos[r] < 0) return fail(VR_ERR_STATE, "row %d has no logits", r);
        sel.lrow[i] = ch->lpos[r]; sel.srow[i] = r; sel.g_lo[i] = i;
    }
    sel.g_lo[n] = n;
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    float* o_score = ch->w_out.as<float>();                   // (w_out holds 3 x 16 x 64 words: four runs of 16 fit)
    int* o_tok = (int*)(o_score + CHAT_MAX_ROWS);
    int* o_kept = o_tok + CHAT_MAX_ROWS;
    int* o_cut = o_kept + CHAT_MAX_ROWS;
    HIPCHK(launch_chat_sample(sel, ch->w_logits.as<float>(), ch->Vpad, ch->V, ch->seen.as<unsigned>(), ch->words, repetition_penalty,
                              temperature, top_k, top_p, (unsigned long long)seed, (unsigned)step, o_score, o_tok, o_kept, o_cut, s));
    int32_t host[4 * CHAT_MAX_ROWS];                          // one copy for the four runs
    HIPCHK(hipMemcpyAsync(host, o_score, sizeof(host), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(out_scores, host, (size_t)n * 4);
    memcpy(out_tokens, host + CHAT_MAX_ROWS, (size_t)n * 4);
    memcpy(out_kept, host + 2 * CHAT_MAX_ROWS, (size_t)n * 4);
    memcpy(out_cut, host + 3 * CHAT_MAX_ROWS, (size_t)n * 4);
    return VR_OK;
}

extern "C" int vr_chat_reorder(vr_chat_t ch, int32_t n, const int32_t* rows, const int32_t* parents, void* stream) {
    if (!ch || !rows || !parents) return fail(VR_ERR_INVALID, "NULL argument");
    const int R = ch->c.max_rows;
    if (n < 1) return fail(VR_ERR_INVALID, "n must be positive");
    if (n > R) return fail(VR_ERR_CAPACITY, "%d rows exceed max_rows=%d", n, R);
    std::vector<char> used(R, 0);
    ChatMove mv{};
    int max_tail = 0;
    for (int i = 0; i < n; ++i) {
        const int r = rows[i], p = parents[i];
        if (r < 0 || r >= R || used[r] || p < 0 || p >= R) return fail(VR_ERR_INVALID, "reorder %d: row %d / parent %d", i, r, p);
        used[r] = 1;
        if (p == r) continue;
        mv.src[mv.n] = p; mv.dst[mv.n] = r; mv.len[mv.n] = ch->row_len[p];
        max_tail = std::max(max_tail, ch->row_len[p]);
        mv.n++;
    }
    if (!mv.n) return VR_OK;
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t need = (size_t)mv.n * 2 * ch->L * std::max(max_tail, 1) * ch->E * 2;
    if (ch->w_move.bytes < need) {
        HIPCHK(hipStreamSynchronize(s));                 // (the old scratch may still be read by an earlier reorder)
        VRCHK(ch->w_move.reserve(need));
    }
    HIPCHK(launch_chat_move(mv, ch->tails.p, ch->w_move.p, ch->L, R, ch->c.max_new, ch->E, max_tail, ch->seen.as<unsigned>(),
                            ch->w_move_seen.as<unsigned>(), ch->words, s));
    const std::vector<int> old_slot = ch->row_slot, old_len = ch->row_len;
    for (int i = 0; i < mv.n; ++i) {
        ch->row_slot[mv.dst[i]] = old_slot[mv.src[i]];
        ch->row_len[mv.dst[i]] = old_len[mv.src[i]];
        ch->lpos[mv.dst[i]] = -1;
    }
    return VR_OK;
}

extern "C" int vr_chat_logits(vr_chat_t ch, int32_t row, float* out, void* stream) {
    if (!ch || !out) return fail(VR_ERR_INVALID, "NULL argument");
    if (row < 0 || row >= ch->c.max_rows || ch->lpos[row] < 0) return fail(VR_ERR_STATE, "row %d has no logits", row);
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(out, ch->w_logits.as<float>() + (size_t)ch->lpos[row] * ch->Vpad, (size_t)ch->V * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// the scoring head's buffers (s_*), allocated at the first call that scores
static int chat_score_scratch(vr_chat_s* ch) {
    if (ch->s_xn.p) return VR_OK;
    const int cap = ch->work->c.max_tokens;
    int rc;
    if ((rc = ch->s_xn.alloc((size_t)pad256(cap) * ch->head.k_pad * 2)) || (rc = ch->s_part.alloc(head_score_part_words(cap, ch->V) * 4)) ||
        (rc = ch->s_tgt.alloc((size_t)cap * 4)) || (rc = ch->s_out.alloc((size_t)4 * cap * 4)) ||
        (rc = ch->s_reps.alloc((size_t)ch->work->c.max_seqs * ch->E * 4))) {
        ch->s_xn.free();
        return rc;
    }
    return VR_OK;
}

// ---- teacher-forced scoring: the packed pass of a prefill without its cache side, every continuation position through the
// fused head (head_score.hip).  Touches none of the generation state: its rows, targets and results live in buffers of its own.
extern "C" int vr_chat_score(vr_chat_t ch, int32_t B, const uint8_t* const* slices, const int32_t* slice_hw, int32_t n_slices,
                             int32_t slices_on_device, const int32_t* input_ids, const int32_t* seq_offsets,
                             const int32_t* vision_rows, const int32_t* cont_len, float* out_logit, float* out_lse,
                             float* out_top_logit, int32_t* out_top_token, void* stream) {
    if (!ch || !input_ids || !seq_offsets || !cont_len || !out_logit || !out_lse || !out_top_logit || !out_top_token)
        return fail(VR_ERR_INVALID, "NULL argument");
    if (n_slices > 0 && (!slices || !slice_hw || !vision_rows)) return fail(VR_ERR_INVALID, "NULL slice arguments");
    if (!ch->head.has_w) return fail(VR_ERR_STATE, "vr_chat_load_head has not run");
    if (B < 1) return fail(VR_ERR_INVALID, "B must be positive");
    vr_model_s* w = ch->work;
    // ---- every check before any launch
    if (B > w->c.max_seqs) return fail(VR_ERR_CAPACITY, "%d sequences exceed the model's max_seqs=%d", B, w->c.max_seqs);
    if (seq_offsets[0] != 0) return fail(VR_ERR_INVALID, "seq_offsets[0] must be 0");
    for (int b = 0; b < B; ++b)
        if (seq_offsets[b + 1] <= seq_offsets[b]) return fail(VR_ERR_INVALID, "empty sequence %d", b);
    const int Ttot = seq_offsets[B];
    if (Ttot > w->c.max_tokens) return fail(VR_ERR_CAPACITY, "%d packed tokens exceed the model's max_tokens=%d", Ttot, w->c.max_tokens);
    int M = 0;
    for (int b = 0; b < B; ++b) {
        const int T = seq_offsets[b + 1] - seq_offsets[b];
        if (cont_len[b] < 1 || cont_len[b] >= T) return fail(VR_ERR_INVALID, "sequence %d: cont_len %d outside 1..%d", b, cont_len[b], T - 1);
        M += cont_len[b];
    }
    for (int t = 0; t < Ttot; ++t)
        if (input_ids[t] < 0 || input_ids[t] >= ch->V) return fail(VR_ERR_INVALID, "token id %d out of range at %d", input_ids[t], t);
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    const int E = ch->E, Kp = ch->head.k_pad, cap = w->c.max_tokens;
    VRCHK(chat_score_scratch(ch));
    EncodeHook hook;
    hook.bf16_route = true;                              // the route of the prefill; no layer hook: nothing is cached
    w->arena_open = false;
    int rc = encode_impl(w, slices, slice_hw, n_slices, slices_on_device, input_ids, seq_offsets, B, vision_rows, ch->s_reps.as<float>(), 1,
                         stream, nullptr, 0, &hook);
    arena_close(w, stream);
    if (rc) return rc;
    // continuation token at position p: the hidden state of p - 1 -> final RMSNorm (scaled weight); a sequence's rows are adjacent
    std::vector<int32_t> tgt(M);
    for (int b = 0, m = 0; b < B; ++b) {
        const int first = seq_offsets[b + 1] - cont_len[b];          // packed position of the first continuation token
        HIPCHK(launch_rmsnorm(w->w_h.as<float>() + (size_t)(first - 1) * E, cont_len[b], E, E, ch->norm_w.as<float>(), w->c.rms_norm_eps,
                              ch->s_xn.as<char>() + (size_t)m * Kp * 2, Kp, s));
        for (int j = 0; j < cont_len[b]; ++j) tgt[m + j] = input_ids[first + j];
        m += cont_len[b];
    }
    HIPCHK(hipMemcpyAsync(ch->s_tgt.p, tgt.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
    float* o = ch->s_out.as<float>();
    HIPCHK(launch_head_score(ch->s_xn.p, Kp, ch->head.w.p, Kp, M, ch->V, Kp, ch->s_tgt.as<int>(), ch->s_part.p, o, o + cap, o + 2 * (size_t)cap,
                             (int*)(o + 3 * (size_t)cap), s));
    std::vector<int32_t> host((size_t)4 * M);
    for (int a = 0; a < 4; ++a) HIPCHK(hipMemcpyAsync(host.data() + (size_t)a * M, o + (size_t)a * cap, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(out_logit, host.data(), (size_t)M * 4);
    memcpy(out_lse, host.data() + M, (size_t)M * 4);
    memcpy(out_top_logit, host.data() + 2 * (size_t)M, (size_t)M * 4);
    memcpy(out_top_token, host.data() + 3 * (size_t)M, (size_t)M * 4);
    return VR_OK;
}

extern "C" int vr_chat_row_len(vr_chat_t ch, int32_t row, int32_t* slot, int32_t* generated) {
    if (!ch || !slot || !generated) return fail(VR_ERR_INVALID, "NULL argument");
    if (row < 0 || row >= ch->c.max_rows) return fail(VR_ERR_INVALID, "row %d out of range", row);
    *slot = ch->row_slot[row];
    *generated = ch->row_len[row];
    return VR_OK;
}

// ---- several given tokens appended to rows whose prompts are cached: ONE packed decoder pass (the encode pass on the bf16
// route) whose positions continue the rows, whose per-layer hook stores the rope'd K / V rows in the rows' tails and whose
// attention reads "prompt plane, then tail plane" (chat_extend.hip)
struct ChatExtendCtx { vr_chat_s* ch; ChatExtend ex; };
static int chat_extend_layer(void* ctx, int l, const void* qkv, int ldqkv, int T, hipStream_t s) {
    const ChatExtendCtx* p = (const ChatExtendCtx*)ctx;
    vr_chat_s* ch = p->ch;
    if (T != p->ex.off[p->ex.n]) return fail(VR_ERR_STATE, "extend hook: %d rows, expected %d", T, p->ex.off[p->ex.n]);
    const size_t plane = (size_t)ch->c.max_rows * ch->c.max_new * ch->E * 2;      // bytes of one (layer, K|V) tail plane
    HIPCHK(launch_chat_tail_scatter(p->ex, qkv, ldqkv, ch->E, ch->c.max_new, (char*)ch->tails.p + ((size_t)l * 2) * plane,
                                    (char*)ch->tails.p + ((size_t)l * 2 + 1) * plane, s));
    return VR_OK;
}
static int chat_extend_attn(void* ctx, int l, const void* qkv, int ldqkv, int T, void* out, int ldo, hipStream_t s) {
    const ChatExtendCtx* p = (const ChatExtendCtx*)ctx;
    vr_chat_s* ch = p->ch;
    (void)T;
    const ChatCaps caps{ch->c.max_slots, ch->c.max_len, ch->c.max_rows, ch->c.max_new};
    HIPCHK(launch_chat_extend_attn(p->ex, qkv, ldqkv, ch->prompt.p, ch->tails.p, l, ch->E, ch->H, caps, out, ldo, s));
    return VR_OK;
}

extern "C" int vr_chat_extend(vr_chat_t ch, int32_t B, const int32_t* slots, const int32_t* rows, const int32_t* tok_offsets,
                              const int32_t* tokens, const int32_t* targets, int32_t seen_mode, float* out_logit, float* out_lse,
                              float* out_top_logit, int32_t* out_top_token, void* stream) {
    if (!ch || !slots || !rows || !tok_offsets || !tokens) return fail(VR_ERR_INVALID, "NULL argument");
    if (targets && (!out_logit || !out_lse || !out_top_logit || !out_top_token)) return fail(VR_ERR_INVALID, "targets without outputs");
    if (!ch->head.has_w) return fail(VR_ERR_STATE, "vr_chat_load_head has not run");
    if (seen_mode < 0 || seen_mode > 2) return fail(VR_ERR_INVALID, "seen_mode %d: 0 (keep), 1 (join), 2 (clear)", seen_mode);
    if (B < 1) return fail(VR_ERR_INVALID, "B must be positive");
    const int R = ch->c.max_rows;
    vr_model_s* w = ch->work;
    // ---- every check before any state changes
    if (B > R) return fail(VR_ERR_CAPACITY, "%d rows exceed max_rows=%d", B, R);
    if (B > w->c.max_seqs) return fail(VR_ERR_CAPACITY, "%d rows exceed the model's max_seqs=%d", B, w->c.max_seqs);
    if (tok_offsets[0] != 0) return fail(VR_ERR_INVALID, "tok_offsets[0] must be 0");
    ChatExtendCtx ctx{ch, {}};
    ChatExtend& ex = ctx.ex;
    ex.n = B;
    std::vector<char> used(R, 0);
    int32_t base_pos[CHAT_MAX_ROWS];
    for (int b = 0; b < B; ++b) {
        const int sl = slots[b], r = rows[b], n = tok_offsets[b + 1] - tok_offsets[b];
        if (n < 1) return fail(VR_ERR_INVALID, "extend row %d: empty token list", b);
        if (sl < 0 || sl >= ch->c.max_slots || ch->plen[sl] <= 0) return fail(VR_ERR_INVALID, "extend row %d: slot %d holds no prompt", b, sl);
        if (r < 0 || r >= R || used[r]) return fail(VR_ERR_INVALID, "extend row %d: row %d out of range or repeated", b, r);
        used[r] = 1;
        if (ch->row_slot[r] != sl && ch->row_len[r] > 0) return fail(VR_ERR_INVALID, "row %d continues slot %d, not %d", r, ch->row_slot[r], sl);
        const int t0 = ch->row_slot[r] == sl ? ch->row_len[r] : 0;
        if (t0 + n > ch->c.max_new || ch->plen[sl] + t0 + n > ch->c.max_len)
            return fail(VR_ERR_CAPACITY, "row %d would exceed max_len=%d / max_new=%d", r, ch->c.max_len, ch->c.max_new);
        ex.row[b] = r; ex.slot[b] = sl; ex.plen[b] = ch->plen[sl]; ex.t0[b] = t0; ex.off[b] = tok_offsets[b];
        base_pos[b] = ch->plen[sl] + t0;
    }
    const int T = tok_offsets[B];
    ex.off[B] = T;
    if (T > w->c.max_tokens) return fail(VR_ERR_CAPACITY, "%d appended tokens exceed the model's max_tokens=%d", T, w->c.max_tokens);
    for (int t = 0; t < T; ++t) {
        if (tokens[t] < 0 || tokens[t] >= ch->V) return fail(VR_ERR_INVALID, "token id %d out of range at %d", tokens[t], t);
        if (targets && (targets[t] < -1 || targets[t] >= ch->V)) return fail(VR_ERR_INVALID, "target id %d out of range at %d", targets[t], t);
    }
    VRCHK(set_dev(ch->model->device));
    if (targets) VRCHK(chat_score_scratch(ch));
    hipStream_t s = (hipStream_t)stream;
    const int E = ch->E;
    EncodeHook hook;
    hook.bf16_route = true;
    hook.layer = chat_extend_layer;
    hook.attn = chat_extend_attn;
    hook.ctx = &ctx;
    hook.base_pos = base_pos;
    hook.rope_table = ch->rope.as<float>();              // max_len positions (the work model's table stops at max_tokens)
    hook.rope_len = ch->c.max_len;
    w->arena_open = false;
    int rc = encode_impl(w, nullptr, nullptr, 0, 0, tokens, tok_offsets, B, nullptr, ch->w_reps.as<float>(), 1, stream, nullptr, 0, &hook);
    arena_close(w, stream);
    if (rc) return rc;
    // the rows' last tokens -> final RMSNorm (scaled weight) -> the head, one pass per run of adjacent logits rows (as the
    // batched prefill): the logits of rows this call does not name stay where they are
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return rows[a] < rows[b]; });
    // the head rewrites the rows' logits lines from here on: whatever they held (a row's logits, a prompt's) is gone even if a
    // launch below fails
    for (int b = 0; b < B; ++b) { chat_release_line(ch, R + rows[b]); ch->lpos[rows[b]] = -1; }
    ChatBatch lr{};
    lr.n = B;
    for (int b = 0; b <= B; ++b) lr.off[b] = tok_offsets[b];
    for (int j = 0; j < B; ++j) lr.idx[order[j]] = j;
    HIPCHK(launch_chat_last_rows(lr, w->w_h.as<float>(), E, ch->norm_w.as<float>(), w->c.rms_norm_eps, ch->w_pxn.p, s));
    for (int j = 0; j < B;) {
        int n = 1;
        while (j + n < B && rows[order[j + n]] == rows[order[j]] + n) ++n;
        GemmArgs a = gemm_args((const char*)ch->w_pxn.p + (size_t)j * E * 2, E, ch->head, n,
                               ch->w_logits.as<float>() + (size_t)(R + rows[order[j]]) * ch->Vpad, ch->Vpad);
        HIPCHK(launch_gemm_skinny(a, s));
        j += n;
    }
    for (int b = 0; b < B; ++b) {
        unsigned* seen = (unsigned*)ch->seen.p + (size_t)rows[b] * ch->words;
        // (a row that starts on a slot starts with an empty seen set, as in vr_chat_step)
        if (seen_mode == 2 || ch->row_slot[rows[b]] != slots[b]) HIPCHK(hipMemsetAsync(seen, 0, (size_t)ch->words * 4, s));
        if (seen_mode == 1) HIPCHK(launch_mark_seen(w->w_ids.as<int>() + tok_offsets[b], tok_offsets[b + 1] - tok_offsets[b], seen, ch->V, s));
    }
    if (targets) {
        // entry t: the distribution after packed token t = its hidden row through the final norm and the fused head
        const int Kp = ch->head.k_pad, cap = w->c.max_tokens;
        HIPCHK(launch_rmsnorm(w->w_h.as<float>(), T, E, E, ch->norm_w.as<float>(), w->c.rms_norm_eps, ch->s_xn.p, Kp, s));
        HIPCHK(hipMemcpyAsync(ch->s_tgt.p, targets, (size_t)T * 4, hipMemcpyHostToDevice, s));
        float* o = ch->s_out.as<float>();
        HIPCHK(launch_head_score(ch->s_xn.p, Kp, ch->head.w.p, Kp, T, ch->V, Kp, ch->s_tgt.as<int>(), ch->s_part.p, o, o + cap, o + 2 * (size_t)cap,
                                 (int*)(o + 3 * (size_t)cap), s));
        std::vector<int32_t> host((size_t)4 * T);
        for (int a = 0; a < 4; ++a) HIPCHK(hipMemcpyAsync(host.data() + (size_t)a * T, o + (size_t)a * cap, (size_t)T * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int t = 0; t < T; ++t) {
            if (targets[t] < 0) continue;
            memcpy(out_logit + t, &host[t], 4);
            memcpy(out_lse + t, &host[(size_t)T + t], 4);
            memcpy(out_top_logit + t, &host[2 * (size_t)T + t], 4);
            out_top_token[t] = host[3 * (size_t)T + t];
        }
    }
    for (int b = 0; b < B; ++b) {
        const int r = rows[b];
        ch->row_slot[r] = slots[b];
        ch->row_len[r] = ex.t0[b] + (tok_offsets[b + 1] - tok_offsets[b]);
        ch->lpos[r] = R + r;
    }
    return VR_OK;
}

// the four numbers of the scoring head from finished logits lines (chat_row_score_kernel), CHAT_ROW_SCORE_MAX entries per launch
static int chat_score_lines(vr_chat_s* ch, int n, const std::vector<int>& lines, const int32_t* targets, float* out_logit, float* out_lse,
                            float* out_top_logit, int32_t* out_top_token, void* stream) {
    VRCHK(set_dev(ch->model->device));
    hipStream_t s = (hipStream_t)stream;
    float* o = ch->w_out.as<float>();                         // (w_out holds 3072 words: four runs of CHAT_ROW_SCORE_MAX fit)
    static_assert(4 * CHAT_ROW_SCORE_MAX <= CHAT_MAX_ROWS * CHAT_TOPK_MAX * 3, "w_out holds the four runs");
    for (int i0 = 0; i0 < n; i0 += CHAT_ROW_SCORE_MAX) {
        ChatRowScore sc{};
        sc.n = std::min(CHAT_ROW_SCORE_MAX, n - i0);
        for (int i = 0; i < sc.n; ++i) { sc.lrow[i] = lines[i0 + i]; sc.target[i] = targets[i0 + i]; }
        HIPCHK(launch_chat_row_score(sc, ch->w_logits.as<float>(), ch->Vpad, ch->V, o, o + CHAT_ROW_SCORE_MAX, o + 2 * CHAT_ROW_SCORE_MAX,
                                     (int*)(o + 3 * CHAT_ROW_SCORE_MAX), s));
        int32_t host[4 * CHAT_ROW_SCORE_MAX];
        HIPCHK(hipMemcpyAsync(host, o, sizeof(host), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        memcpy(out_logit + i0, host, (size_t)sc.n * 4);
        memcpy(out_lse + i0, host + CHAT_ROW_SCORE_MAX, (size_t)sc.n * 4);
        memcpy(out_top_logit + i0, host + 2 * CHAT_ROW_SCORE_MAX, (size_t)sc.n * 4);
        memcpy(out_top_token + i0, host + 3 * CHAT_ROW_SCORE_MAX, (size_t)sc.n * 4);
    }
    return VR_OK;
}

extern "C" int vr_chat_row_score(vr_chat_t ch, int32_t n, const int32_t* rows, const int32_t* targets, float* out_logit, float* out_lse,
                                 float* out_top_logit, int32_t* out_top_token, void* stream) {
    if (!ch || !rows || !targets || !out_logit || !out_lse || !out_top_logit || !out_top_token) return fail(VR_ERR_INVALID, "NULL argument");
    if (n < 1) return fail(VR_ERR_INVALID, "n must be positive");
    std::vector<int> lines(n);
    for (int i = 0; i < n; ++i) {
        if (rows[i] < 0 || rows[i] >= ch->c.max_rows) return fail(VR_ERR_INVALID, "entry %d: row %d out of range", i, rows[i]);
        if (targets[i] < 0 || targets[i] >= ch->V) return fail(VR_ERR_INVALID, "entry %d: target id %d out of range", i, targets[i]);
        if (ch->lpos[rows[i]] < 0) return fail(VR_ERR_STATE, "row %d has no logits", rows[i]);
        lines[i] = ch->lpos[rows[i]];
    }
    return chat_score_lines(ch, n, lines, targets, out_logit, out_lse, out_top_logit, out_top_token, stream);
}

extern "C" int vr_chat_slot_score(vr_chat_t ch, int32_t n, const int32_t* slots, const int32_t* targets, float* out_logit, float* out_lse,
                                  float* out_top_logit, int32_t* out_top_token, void* stream) {
    if (!ch || !slots || !targets || !out_logit || !out_lse || !out_top_logit || !out_top_token) return fail(VR_ERR_INVALID, "NULL argument");
    if (n < 1) return fail(VR_ERR_INVALID, "n must be positive");
    std::vector<int> lines(n);
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= ch->c.max_slots) return fail(VR_ERR_INVALID, "entry %d: slot %d out of range", i, slots[i]);
        if (targets[i] < 0 || targets[i] >= ch->V) return fail(VR_ERR_INVALID, "entry %d: target id %d out of range", i, targets[i]);
        if (ch->plen[slots[i]] <= 0 || ch->slot_lrow[slots[i]] < 0) return fail(VR_ERR_STATE, "slot %d: the prompt's logits are gone", slots[i]);
        lines[i] = ch->slot_lrow[slots[i]];
    }
    return chat_score_lines(ch, n, lines, targets, out_logit, out_lse, out_top_logit, out_top_token, stream);
}

extern "C" int vr_chat_slot_state(vr_chat_t ch, int32_t slot, int32_t* prompt_len, int32_t* has_prompt_logits, int32_t* generation) {
    if (!ch || !prompt_len || !has_prompt_logits || !generation) return fail(VR_ERR_INVALID, "NULL argument");
    if (slot < 0 || slot >= ch->c.max_slots) return fail(VR_ERR_INVALID, "slot %d out of range", slot);
    *prompt_len = ch->plen[slot];
    *has_prompt_logits = ch->plen[slot] > 0 && ch->slot_lrow[slot] >= 0;
    *generation = ch->slot_gen[slot];
    return VR_OK;
}

extern "C" int vr_chat_row_truncate(vr_chat_t ch, int32_t row, int32_t length) {
    if (!ch) return fail(VR_ERR_INVALID, "NULL argument");
    if (row < 0 || row >= ch->c.max_rows) return fail(VR_ERR_INVALID, "row %d out of range", row);
    if (length < 0 || length > ch->row_len[row]) return fail(VR_ERR_INVALID, "length %d outside 0..%d", length, ch->row_len[row]);
    ch->row_len[row] = length;                           // host state only: the tail's rows stay, the next append overwrites them
    ch->lpos[row] = -1;
    return VR_OK;
}
