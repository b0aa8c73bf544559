// Launcher prototypes of the gfx950 kernels (host side of libvisrag_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_warm.h"

namespace vr {

// ---- GEMM (gemm.hip) ---------------------------------------------------------------------
enum GemmEpilogue { EPI_BF16 = 0, EPI_GELU = 1, EPI_F32 = 2, EPI_RESID = 3, EPI_SWIGLU = 4, EPI_ROPE = 5 };
// GLDS: 128x128 4-wave tile; 256IL: 256x256 8-wave tile (needs W and A readable up to the next
// multiple of 256 rows); 192: 256x192 tile for N % 192 == 0; AUTO picks by shape.  (The gaps in the ids are
// retired round-1 experiment variants: DESIGN.md ledger row 5.)
// 128W_192 / 128W_256: the half-height one-wave tiles of gemm128w.hip (few rows: the decoder's o / down projections).
// 288W: the 256x288 form of the one-wave tile (N % 288 == 0, the lookup-free residual epilogue only).
enum GemmVariant { GEMM_VARIANT_GLDS = 0, GEMM_VARIANT_AUTO = 3, GEMM_VARIANT_192 = 7, GEMM_VARIANT_256IL = 9, GEMM_VARIANT_256W = 12,
                   GEMM_VARIANT_192W = 13, GEMM_VARIANT_128W_192 = 14, GEMM_VARIANT_128W_256 = 15, GEMM_VARIANT_288W = 16 };

struct GemmArgs {
    const void* A; int lda;          // bf16 [M_pad][lda]
    const void* W; int ldw;          // bf16 [N][ldw]   (nn.Linear layout: [out][in])
    int M, N, K;                     // N % 128 == 0, K % 64 == 0
    const float* bias;               // f32 [N] or null
    const float* resid;              // f32 [M][ldo] (EPI_RESID)
    float alpha;                     // EPI_RESID scale
    void* out; int ldo;
    const int* rowmap;               // optional: output row of input row m (-1 = drop)
    const float* rowbias;            // optional: f32 [period][rowbias_ld], added for n < rowbias_cols (EPI_BF16 / GELU / F32; refused with the others)
    int rowbias_period, rowbias_ld, rowbias_cols;
    const int* rope_pos;             // EPI_ROPE: position of row m
    const float* rope_table;         // f32 [max_pos][64] = cos[32] | sin[32]
    int rope_cols;                   // columns < rope_cols are rotated (q and k), rest copied (v)
    int raster_gm;                   // 256-tile kernels: m-tiles per raster group (0 = choose by W size)
    int ksplit;                      // 256-tile kernels, EPI_F32 only: split K over ksplit workgroups per tile;
    size_t split_stride;             //   split s writes its partial product to out + s * split_stride (elements)
    float col_scale; int col_scale_n;   // optional, EPI_BF16 only (the general forms scale per column under a row map / row bias): columns n < col_scale_n
                                     // (a multiple of 64) leave as bf16((acc + bias) * col_scale) — the ViT's q columns carry
                                     // head_dim^-0.5 * log2(e) into the attention kernel with ONE rounding (attention_w.hip)
    const int* m_dev; int m_sub;     // optional, GEMM_VARIANT_256IL only (refused elsewhere): rows < *m_dev - m_sub exist (a row count known on the
                                     // device only: tiles at or past it leave at once — the search's band pass)
    const void* warm; size_t warm_bytes;   // optional, GEMM_VARIANT_256W only (refused elsewhere): "while you run, request every 128-byte line of
                                     // this region once" — the bytes are not used, only brought into the memory-side cache for the launch
                                     // behind this one (the decoder's o / down weights ride the q|k|v and gate|up launches); null or 0
                                     // bytes: absent.  Each workgroup requests its share (gemm_warm.h) between its K-loop and its epilogue
};
hipError_t launch_gemm(const GemmArgs& a, int epilogue, int variant, hipStream_t s);
// The rule of the optional fields: each is HONOURED by the kernel a launch reaches or the launch is REFUSED (hipErrorInvalidValue)
// before anything runs — never silently ignored.  `variant` is a concrete one (AUTO resolved); true = refuse.  Every variant
// launcher below asks this itself, so a direct caller gets the same answer as launch_gemm's.  (include/visrag_hip.h,
// vr_op_gemm_ex, has the table.)
bool gemm_args_refused(const GemmArgs& a, int epilogue, int variant);
// the concrete variant GEMM_VARIANT_AUTO resolves to for this launch (a caller that sets a field only one variant honours asks first)
int gemm_auto_variant(const GemmArgs& a, int epilogue);
// the concrete variant launch_gemm reaches with these arguments (it dispatches on this), or GEMM_ROUTE_REFUSED where the launch
// is refused by a test of the host's; integer and null tests only, no pointer is dereferenced
constexpr int GEMM_ROUTE_REFUSED = -1;
int gemm_route(const GemmArgs& a, int epilogue, int variant);
// 256x192 tile (gemm192.hip): N % 192 == 0, epilogues BF16 / GELU / F32 / RESID only
hipError_t launch_gemm192(const GemmArgs& a, int epilogue, hipStream_t s);
// 256x256 tile, one wave per SIMD (gemm256w.hip): same contract as the 256-tile path of launch_gemm
hipError_t launch_gemm256w(const GemmArgs& a, int epilogue, hipStream_t s);
bool gemm256w_fits(const GemmArgs& a, int tile_cols);   // its 32-bit LDS-DMA offsets cover both operands
// its 256x192 form: N % 192 == 0, EPI_RESID and EPI_F32 (incl. ksplit)
hipError_t launch_gemm192w(const GemmArgs& a, int epilogue, hipStream_t s);
// its 256x288 form: N % 288 == 0, EPI_RESID without a row map (every other optional field is refused)
hipError_t launch_gemm288w(const GemmArgs& a, int epilogue, hipStream_t s);
// 128 x 192 / 128 x 256 tile, one wave per SIMD, three LDS stages (gemm128w.hip): N % tile_cols == 0, no row map / row bias /
// split K; tile_cols 192: EPI_RESID, 256: EPI_RESID / BF16 / GELU / SWIGLU
hipError_t launch_gemm128w(const GemmArgs& a, int epilogue, int tile_cols, hipStream_t s);
bool gemm128w_fits(const GemmArgs& a, int tile_cols);

// M <= 16 rows (gemm_skinny.hip): the decode step's weight streamer; fp32 planes out[split][M][ldo] (+ bias with split 0)
// swiglu (ksplit 1, 16-row [gate | up] interleaved W): out = bf16 act [M][ldo] = silu(gate) * up instead of a plane
// combine (M = 1, K = heads * 128): the A row is merged on the fly from the decode step's partial attention rows
// (bf16 part[S][ldp], lse f32 [S][heads]: see launch_attn_combine) — no separate merge launch
// part / lse come from the decode attention with the `group` query heads of a KV head as ROWS: range t, query head hq =
// hkv * group + g  ->  part[((t * group + g) * (heads / group) + hkv) * 128 + d],  lse[(t * group + g) * (heads / group) + hkv]
struct SkinnyCombine { const void* part; const float* lse; int S; int heads; int group; const int* S_dev; };
hipError_t launch_gemm_skinny(const GemmArgs& a, hipStream_t s, bool swiglu = false, const struct SkinnyCombine* combine = nullptr);
// act = silu(gate) * up from the fp32 planes of a gate/up GEMM over 16-row interleaved weights
hipError_t launch_swiglu_sum(const float* parts, int n_parts, size_t plane_stride, int ldp, int M, int I, void* act, int lda,
                             hipStream_t s);

// ---- fused LM head for scoring (head_score.hip) ------------------------------------------
// x = A [M][lda] . W [V][ldw]^T over K (bf16, fp32 accumulation; A readable up to pad256(M) rows, W up to pad256(V) rows) is
// reduced per row without being written: x_t = x[m][target[m]], lse = log sum_{v < V} exp x, top_x / top_id = the largest logit
// and its token (lowest id among ties).  part: head_score_part_words(M, V) 4-byte words of scratch.  A target outside [0, V)
// leaves its x_t entry unwritten.  Every pointer is a device pointer.
size_t head_score_part_words(int M, int V);
hipError_t launch_head_score(const void* A, int lda, const void* W, int ldw, int M, int V, int K, const int* target, void* part,
                             float* x_t, float* lse, float* top_x, int* top_id, hipStream_t s);

// ---- norms (norm.hip) --------------------------------------------------------------------
// x f32 [rows][ldx] (dim used) -> bf16 [rows][ldo]; columns [dim, ldo) are written as zero.
hipError_t launch_layernorm(const float* x, int rows, int dim, int ldx, const float* w, const float* b,
                            float eps, void* out, int ldo, hipStream_t s);
// x += alpha * sum_s partial[s] (fp32, fixed order: deterministic), written back; then RMSNorm -> out
// (out == null: accumulate only).  Closes a split-K GEMM (GemmArgs::ksplit) without a reduction pass.
hipError_t launch_rmsnorm_accum(float* x, int rows, int dim, int ldx, const float* partial, int nsplit,
                                size_t split_stride, int ldp, float alpha, const float* w, float eps, void* out,
                                int ldo, hipStream_t s);
hipError_t launch_rmsnorm(const float* x, int rows, int dim, int ldx, const float* w, float eps,
                          void* out, int ldo, hipStream_t s);

// ---- attention (attention.hip) -----------------------------------------------------------
struct AttnArgs {
    const void* q; int ldq;          // bf16, row stride in elements; head h at column h*head_dim
    const void* k; int ldk;
    const void* v; int ldv;
    void* out; int ldo;              // bf16 [rows_q][ldo], head h at column h*head_dim
    const int* cu_q;                 // [B+1] row ranges of q/out (ignored for q when q_shared)
    const int* cu_kv;                // [B+1] row ranges of k/v
    int B, heads, head_dim, max_q;
    int causal, q_shared;            // q_shared: q rows [0,max_q) are the same for every batch item
    float scale;
    int kv_group;                    // grouped-query attention: query head h reads K/V head h / kv_group (0 or 1: one each)
    const int* kv_end;               // optional [B]: item b's K/V rows are [cu_kv[b], kv_end[b]) instead of [cu_kv[b], cu_kv[b+1])
                                     // (ranges of DIFFERENT caches: batched decode)
    const int* q_in_rows;            // optional [B]: first q row of item b (overrides cu_q / q_shared for READING q; out rows stay cu_q)
    int q_head_stride;               // elements between the heads of a q row (0: head_dim) — lets the query HEADS of a
                                     // grouped-query group be handed in as the ROWS of one tile (decode: K/V read once per group)
    int q_prescaled;                 // the q rows already carry scale * log2(e) (GemmArgs::col_scale): the kernels apply no scale
    float* lse;                      // optional f32 [rows_q][heads]: log2 of the row's softmax denominator (with the running
                                     // max folded in) — lets a caller merge attention over separately processed KV ranges
};
hipError_t launch_attention(const AttnArgs& a, hipStream_t s);
// the kernel launch_attention reaches with these arguments (it dispatches on this): attention_small.hip, attention_w.hip, or
// attention.hip's attention_kernel<head_dim, qf, pipe>
enum AttnRouteKind { ATTN_ROUTE_REFUSED = -1, ATTN_ROUTE_NONE = 0, ATTN_ROUTE_SMALL = 1, ATTN_ROUTE_72W = 2, ATTN_ROUTE_TILED = 3 };
struct AttnRoute { int kind, head_dim, qf, pipe; };       // qf, pipe: the tiled form's template arguments (0 otherwise)
AttnRoute attention_route(const AttnArgs& a);

// ---- MiniCPM-V 2.0 answer generation (chat_kernels.hip; host side vr_chat_* in chat.hip) ------
constexpr int CHAT_MAX_ROWS = 16;   // rows (prompts x beams) of one decode step
constexpr int CHAT_ATT_SPLITS = 8;  // most prompt-key ranges of one (prompt, head) in the decode attention
constexpr int CHAT_KEYS = 256;      // keys per chunk of the decode attention (one per thread)
constexpr int CHAT_SEL_WGS = 64;    // workgroups of the candidate pass per group
constexpr int CHAT_TOPK_MAX = 64;   // most candidates per group
enum ChatSelMode { CHAT_SEL_GREEDY = 0, CHAT_SEL_BEAM = 1, CHAT_SEL_SAMPLE = 2 };
// one decode step, passed by value: step row i appends `token[i]` to tail row `row[i]` (at tail index tail[i], position
// pos[i]); rows [g_lo[g], g_lo[g + 1]) share prompt slot slot[g_lo[g]] of plen[g] tokens
struct ChatStep {
    int n, groups;
    int row[CHAT_MAX_ROWS], slot[CHAT_MAX_ROWS], tail[CHAT_MAX_ROWS], pos[CHAT_MAX_ROWS], token[CHAT_MAX_ROWS];
    int g_lo[CHAT_MAX_ROWS + 1], plen[CHAT_MAX_ROWS];
    int gsplit[CHAT_MAX_ROWS], rsplit[CHAT_MAX_ROWS];   // prompt-key ranges of the attention per group / per row (its group's)
};
// cache geometry: prompt planes [slots][len][E], tail planes [rows][tail][E] per (layer, K|V)
struct ChatCaps { int slots, len, rows, tail; };
// beam reordering: row dst[i] receives the first len[i] tail rows and the seen set of row src[i]
struct ChatMove { int n; int src[CHAT_MAX_ROWS], dst[CHAT_MAX_ROWS], len[CHAT_MAX_ROWS]; };
// selection: selected row i reads logits row lrow[i] and seen set srow[i]; rows [g_lo[g], g_lo[g + 1]) form group g
struct ChatSel {
    int n, groups;
    int lrow[CHAT_MAX_ROWS], srow[CHAT_MAX_ROWS], g_lo[CHAT_MAX_ROWS + 1];
    float bscore[CHAT_MAX_ROWS];
};
// The attention's view of a step whose n, slot[] are set: groups of adjacent rows with one slot (g_lo, groups, plen[g] =
// slot_plen[slot]) and their prompt-key ranges (gsplit / rsplit: ~CHAT_KEYS keys each, at most CHAT_ATT_SPLITS).  Returns the
// largest gsplit (launch_chat_attn's S_max), or 0 when the rows of a slot are not adjacent.  force_splits in
// 1..CHAT_ATT_SPLITS overrides the policy for every group (op-level tests: ranges that hold no key).
int chat_step_groups(ChatStep& st, const int* slot_plen, int max_slots, int force_splits = 0);
hipError_t launch_chat_embed(const ChatStep& st, const void* table, int E, float scale, float* h, unsigned* seen, int words, hipStream_t s);
hipError_t launch_chat_qkv(const ChatStep& st, const float* parts, int n_parts, size_t plane, int ldp, const float* rope, int E, int heads,
                           void* q_out, void* tails, int l, int max_rows, int max_new, hipStream_t s);
hipError_t launch_chat_attn(const ChatStep& st, const void* q, const void* prompt, const void* tails, int l, int E, int heads,
                            const ChatCaps& cap, int S_max, float* po, float* pml, void* att, hipStream_t s);
hipError_t launch_chat_prompt_kv(const void* qkv, int ld, int T, int E, void* kdst, void* vdst, hipStream_t s);
// a batched prefill, passed by value: prompt b owns the packed rows [off[b], off[b + 1]); idx[b] = its prompt slot (the
// scatter) or its output row (the last-rows norm)
struct ChatBatch { int n; int off[CHAT_MAX_ROWS + 1], idx[CHAT_MAX_ROWS]; };
// one layer's rope'd K / V rows of the packed q | k | v rows [off[n]][ld] -> position t - off[b] of slot idx[b] in the layer's
// K / V planes [slots][max_len][E]; the caller has checked idx[b] < slots and off[b + 1] - off[b] <= max_len
hipError_t launch_chat_prompt_scatter(const ChatBatch& bt, const void* qkv, int ld, int E, int max_len, void* kplane, void* vplane,
                                      hipStream_t s);
// out[idx[b]][E] = bf16 RMSNorm(h[off[b + 1] - 1]) * w: the last token of every packed prompt, ready for the head
hipError_t launch_chat_last_rows(const ChatBatch& bt, const float* h, int E, const float* w, float eps, void* out, hipStream_t s);
hipError_t launch_chat_move(const ChatMove& mv, void* tails, void* scratch, int layers, int max_rows, int max_new, int E, int max_tail,
                            unsigned* seen, unsigned* seen_scratch, int words, hipStream_t s);
hipError_t launch_chat_select(const ChatSel& sel, int mode, const float* logits, int ld, int V, const unsigned* seen, int words, float pen,
                              float temperature, int K, int kout, unsigned long long seed, unsigned step, float* lse,
                              unsigned long long* part, float* o_score, int* o_tok, int* o_par, hipStream_t s);
// The nucleus sampler (chat_sample.hip; definition at vr_chat_sample in include/visrag_hip.h): one draw per selected row i
// (sel.n rows; groups are not used) among the kept candidates of logits row lrow[i] under seen set srow[i].  top_k 0 = off,
// 0 < top_p <= 1.  o_* [sel.n] on the device: penalised logit, token, kept candidates, last kept token; a row without
// candidates gives (-inf, -1, 0, -1).  One workgroup per row; reads logits and seen, writes the four outputs, nothing else.
hipError_t launch_chat_sample(const ChatSel& sel, const float* logits, int ld, int V, const unsigned* seen, int words, float pen,
                              float temperature, int top_k, double top_p, unsigned long long seed, unsigned step, float* o_score,
                              int* o_tok, int* o_kept, int* o_cut, hipStream_t s);
// ---- several given tokens appended to cached prompts in one packed pass (chat_extend.hip; host side vr_chat_extend) ----
// passed by value: sequence b appends the packed rows [off[b], off[b + 1]) to tail row row[b] at tail index t0[b]; its prompt
// is the first plen[b] keys of slot slot[b]
struct ChatExtend { int n; int row[CHAT_MAX_ROWS], slot[CHAT_MAX_ROWS], plen[CHAT_MAX_ROWS], t0[CHAT_MAX_ROWS], off[CHAT_MAX_ROWS + 1]; };
constexpr int CHAT_EXT_QT = 64;     // query rows per workgroup of the two-segment attention
// one layer's rope'd K / V rows of the packed q | k | v rows [off[n]][ld] -> tail index t0[b] + t - off[b] of row[b] in the
// layer's K / V tail planes [rows][max_new][E]; the caller has checked row[b] < rows and t0[b] + n_b <= max_new
hipError_t launch_chat_tail_scatter(const ChatExtend& ex, const void* qkv, int ld, int E, int max_new, void* kplane, void* vplane,
                                    hipStream_t s);
// Two-segment causal attention, head_dim 64, scale 1/8: query j of sequence b (packed row off[b] + j of q [rows][ldq], head h at
// column h * 64) sees keys [0, plen[b]) of its slot's prompt planes and keys [0, t0[b] + j] of its row's tail planes (layer l of
// prompt [layers][K|V][slots][len][E] / tails [layers][K|V][rows][tail][E]); out bf16 [rows][ldo].  One workgroup per (64-query
// tile, head, sequence); reads no plane row outside [0, plen) / [0, t0 + n), writes its own output rows only.  The caller has
// checked every index against `cap`; q and the planes 16-byte aligned, ldq % 8 == 0, E % 8 == 0, ldo % 4 == 0.
hipError_t launch_chat_extend_attn(const ChatExtend& ex, const void* q, int ldq, const void* prompt, const void* tails, int l, int E,
                                   int heads, const ChatCaps& cap, void* out, int ldo, hipStream_t s);
// the four numbers of launch_head_score from fp32 logits rows already computed: entry i < sc.n reads logits row lrow[i] at
// target[i] (outside [0, V): its x_t entry is left unwritten); one workgroup per entry, lowest id among tied maxima
constexpr int CHAT_ROW_SCORE_MAX = 64;
struct ChatRowScore { int n; int lrow[CHAT_ROW_SCORE_MAX], target[CHAT_ROW_SCORE_MAX]; };
hipError_t launch_chat_row_score(const ChatRowScore& sc, const float* logits, int ld, int V, float* x_t, float* lse, float* top_x,
                                 int* top_id, hipStream_t s);

// ---- EVisRAG generator (gen_kernels.hip) ---------------------------------------------------
constexpr int GEN_ATT_SPLITS = 16;  // most KV ranges one decode step's attention is cut into
// What a decode step needs beyond the caches, resident on the device so that consecutive steps need no host round trip
// (gen.hip: host-driven steps upload the first five words; free-running steps advance them on the device).  The op-level
// entries take it as 42 i32 words: the layout is tabled in include/visrag_hip.h and asserted next to vr_op_gen_sample (ops.hip).
struct GenState {
    int token;                      // the token this step appends
    int pos[3];                     // its temporal / height / width position
    int len;                        // KV-cache rows in use before this step
    int step;                       // index of the next sampled token (selects the sampling noise)
    int splits;                     // KV ranges of this step's attention (decode_begin_kernel)
    int pad;
    int cu_q[GEN_ATT_SPLITS + 1], cu_kv[GEN_ATT_SPLITS + 1];
};
// KV ranges of a decode row's attention over its L = len + 1 cache rows: up to GEN_ATT_SPLITS ranges of `chunk` rows (a multiple
// of the attention kernel's 64-key tile, ~128 keys or more each); range t is rows [min(L, t * chunk), min(L, (t + 1) * chunk)).
// One rule for the device (decode_begin_kernel) and the host (vg_decode_batch).
struct KvSplit { int splits, chunk; };
__host__ __device__ inline KvSplit gen_kv_split(int L) {
    int splits = min(GEN_ATT_SPLITS, max(1, (L + 127) / 128));
    const int chunk = ((L + splits - 1) / splits + 63) / 64 * 64;
    splits = (L + chunk - 1) / chunk;
    return KvSplit{splits, chunk};
}
// one vg_decode_batch step (up to 16 sequences): built on the host, uploaded once per step
struct GenBatch {
    int token[16];
    int pos[3][16];                                  // [component][row]
    int cache_row[16];                               // cache row the row's new token goes to: slot * max_len + len
    int splits[16];                                  // KV ranges of the row's attention
    int cu_q[16 * GEN_ATT_SPLITS + 1];               // output rows of item (row, range): (row * SPLITS + range) * group
    int kv_lo[16 * GEN_ATT_SPLITS], kv_hi[16 * GEN_ATT_SPLITS];   // the item's cache rows [lo, hi)
    int q_in[16 * GEN_ATT_SPLITS];                   // the item's first q row (128-wide rows: row * heads)
    int sampled[16];                                 // vg_sample_batch: the sampled tokens
};
hipError_t launch_decode_begin(GenState* st, int q_rows, hipStream_t s);   // q_rows: query rows per KV range (the GQA group size)
// multimodal RoPE on q (in place into q_out) and k (into the K cache at rows cache_row0 + t), v copied into the V
// cache; head_dim 128; pos3 = [3][pos_stride] ints (temporal, height, width); inv_freq f32 [64]; source = bf16 qkv rows
// or (parts != null) fp32 split-K planes + bias; cu_kv (optional) receives {0, cache_row0 + T}
hipError_t launch_mrope_cache(const void* src_bf16, const float* parts, int n_parts, size_t plane_stride, const float* bias,
                              int ld, int T, int H, int KV, const int* pos3, int pos_stride, int sec_t, int sec_h,
                              const float* inv_freq, void* q_out, int ldq, void* k_cache, void* v_cache, int ld_cache,
                              int cache_row0, int* cu_kv, hipStream_t s, const int* row0_dev = nullptr,   // row0_dev: cache_row0 read on the device
                              const int* cache_rows = nullptr);  // cache_rows [T] (device): row t goes to cache row cache_rows[t] (batched decode)
// vision tower: cs f32 [T][64][2] = (cos, sin)((p < sec_h ? pos_h : pos_w)[t] * freq[p]); then q / k head slots (2 * hh
// wide, pairs (p, p + hh), hh <= 64) of bf16 qkv rows rotated in place, slots [0, n_slots) at columns slot * 2 * hh
hipError_t launch_rope2d_table(const int* pos_h, const int* pos_w, int T, int sec_h, const float* freq, void* cs, hipStream_t s);
hipError_t launch_rope2d_inplace(void* qkv, int ld, int T, int n_slots, int hh, const void* cs, hipStream_t s);
hipError_t launch_mark_seen(const int* ids, int n, unsigned* seen, int vocab, hipStream_t s);
// repetition penalty over the seen ids, temperature sampling (Gumbel-max; 0 = argmax), marks the chosen token seen.
// st (optional): the token also goes to st->token; step_from_state: the noise index is st->step; advance: the step's
// bookkeeping (len, step, positions + 1) happens here, on the device
hipError_t launch_sample(const float* logits, int vocab, unsigned* seen, float penalty, float temperature,
                         unsigned long long seed, unsigned step, int* token_out, unsigned long long* scratch64, hipStream_t s,
                         GenState* st = nullptr, int step_from_state = 0, int advance = 0);
hipError_t launch_scatter_rows(const float* src, const int* row_idx, int n, int dim, float* dst, int ld, hipStream_t s);
// dst[i][:] = bf16(src[row_idx[i]][0..dim)), zero up to ld (src rows are dense: stride dim)
hipError_t launch_gather_rows_bf16(const float* src, const int* row_idx, int n, int dim, void* dst, int ld, hipStream_t s);
// dst[i][:] = bf16 patch row (c, t, y, x) of patch (ph[i], pw[i]) of u8 HWC page img[i], (u8 / 255 - mean) / std; zero up to ld
hipError_t launch_patch_rows_u8(const uint8_t* const* pages, const int* page_w, const int* img, const int* ph, const int* pw, int n,
                                int P, int tp, const float* mean3, const float* std3, void* dst, int ld, hipStream_t s);
// out[h*128 + d] = sum_s 2^(lse[s][h] - max) * part[s][h*128 + d] / sum_s 2^(lse[s][h] - max): merges the S partial
// attention rows (bf16 [S][ldp], each normalised over its own KV range) of one decode step
hipError_t launch_attn_combine(const void* part, const float* lse, int S, int heads, int group, void* out, hipStream_t s,
                               const int* S_dev = nullptr,       // S_dev: S read on the device; layout: see SkinnyCombine
                               int n_rows = 1, int ld_out = 0);  // batched decode: row r's ranges start at range r * GEN_ATT_SPLITS,
                                                                 // its count is S_dev[r], its output row is out + r * ld_out

// ---- elementwise / gather / pooling (misc.hip) ---------------------------------------------
// Fused ToTensor/Normalize + patch-embed conv (patch_embed.hip): g carries the PERMUTED weight (k = ky*3P + kx*3 + c),
// bias, the resampled pos-embed as rowbias (period = patches per image), out fp32 [M][ldo], M = n_imgs * patches.
hipError_t launch_patch_embed(const uint8_t* const* imgs, int n_imgs, int H, int W, int P, const GemmArgs& g, int Kreal,
                              hipStream_t s);
// h[t][:] = table[ids[t]][:] * scale   (bf16 table -> f32 rows)
hipError_t launch_embed_gather(const int* ids, int T, const void* table, int dim, float scale,
                               float* out, hipStream_t s);
// final RMSNorm + position-weighted mean pool + L2 normalise: one embedding per sequence.
hipError_t launch_pool(const float* h, const int* seq_offsets, int B, int dim, const float* norm_w,
                       float eps, float* out, float* tap_hidden, hipStream_t s, int mode = 0);   // mode: VR_POOL_*
hipError_t launch_f32_to_bf16(const float* in, void* out, size_t n, hipStream_t s);
hipError_t launch_f32_to_bf16_pad(const float* in, void* out, size_t n, size_t n_total, hipStream_t s,
                                  int* zero_word = nullptr);   // + zero tail (+ TWO ints cleared)
// split x (f32) into hi + lo bf16 parts (x ~= hi + lo to ~16 bits of mantissa)
hipError_t launch_split_bf16(const float* in, void* hi, void* lo, size_t n, hipStream_t s);
hipError_t launch_iota_pos(const int* seq_offsets, int B, int* pos, hipStream_t s);
hipError_t launch_any_nonzero16(const void* p, size_t n, int* flag, hipStream_t s);   // *flag |= any bf16 word != +-0

// ---- split-precision text path (hp_text.hip): fp32 glue between hi + lo bf16 GEMMs ---------------
hipError_t launch_rmsnorm_split(const float* x, int rows, int dim, const float* w, float eps, void* hi, void* lo, hipStream_t s);
hipError_t launch_rope_f32(float* qkv, int T, int ld, int rope_cols, const int* pos, const float* table, hipStream_t s);
hipError_t launch_attn_f32(const float* qkv, int ld, int E, const int* seq_of, const int* seq_offsets, int T, int heads,
                           float scale, float* out, hipStream_t s);
hipError_t launch_swiglu_split(const float* gu, int T, int ld_gu, int I, int ld_act, void* hi, void* lo, hipStream_t s);
hipError_t launch_embed_gather_hp(const int* ids, int T, const void* table_hi, const void* table_lo, int dim, float scale,
                                  float* out, hipStream_t s);
hipError_t launch_seq_of(const int* seq_offsets, int B, int* seq_of, hipStream_t s);
// out = (accumulate ? out : 0) + alpha * sum of n_parts fp32 planes [T][ldp] (columns < N), fixed order
hipError_t launch_planes_sum(const float* parts, int n_parts, size_t stride, int ldp, int T, int N, float* out, int ldo, float alpha,
                             bool accumulate, hipStream_t s);

// ---- synthetic page images (synth.hip; bench / test support): pages first .. first + n - 1 of visrag_amd/synth.py's corpus
hipError_t launch_synth_pages(uint8_t* out, int n, int size, long long seed, long long first, hipStream_t s);

// ---- PIL-exact bicubic resize (resize.hip) ------------------------------------------------------
} // namespace vr
#include <vector>
namespace vr {
int resize_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk);   // returns ksize
hipError_t launch_resize_h(const uint8_t* in, int in_w, int rows, uint8_t* out, int out_w, const int* bounds,
                           const int* kk, int ksize, hipStream_t s);
hipError_t launch_resize_v(const uint8_t* in, int w, uint8_t* out, int out_h, const int* bounds, const int* kk,
                           int ksize, hipStream_t s);

// ---- search (search.hip) -------------------------------------------------------------------
struct SearchArgs {
    const void* index_bf16;          // [n_docs_pad][dim] bf16
    const float* index_f32;          // [n_docs][dim] f32
    int64_t n_docs;
    int dim;
    const void* q_bf16;              // [nq_pad][dim] bf16
    int convert_q;                   // streaming kernel only: q_bf16 has NOT been filled — every workgroup converts the queries
                                     // from q_f32 itself, workgroup 0 writes q_bf16 rows [0, nq) and clears the two flag counters
    const float* q_f32;              // [nq][dim]
    int nq, k;
    float* cand_scores; int* cand_ids; int n_chunks;   // workspace [nq_pad][n_chunks][KP]
    float* out_scores; int64_t* out_ids;               // [nq][k]
    float* thr_init;                                   // workspace [nq_pad] or null (no pre-pass)
    int pre_own_chunks;                                // 0, or the number of list chunks at the END of n_chunks that belong to the threshold
                                                       // pre-pass (search_prepass_owned): its sampled 256-row tiles are scored ONCE — the pre-pass
                                                       // keeps every score, appends the rows >= the threshold to those lists itself, and the
                                                       // sweep (n_chunks - pre_own_chunks workgroup chunks) skips the sampled tiles
    float* thr_cert;                                   // workspace [nq_pad] (pre_own_chunks > 0): what the lists are complete down to — the
                                                       // threshold, or +inf for a query whose pre-pass list overflowed (exact ties)
    unsigned long long* cand_keys;                     // 256-tile sweep scratch [nq_pad256][n_chunks][2][64] or null
    float* score_rows; size_t ld_scores;               // streaming search (nq <= 16) only: the sweep writes EVERY bf16-MFMA score,
                                                       // [16][ld_scores] (ld_scores % 256 == 0, >= n_docs), and a query its merge cannot
                                                       // certify is redone in place by its own merge workgroup (search_band.h)
    int exact_follows;               // streaming search with score_rows: 1 = the exact fp32 pass IS launched behind this merge — a query whose band
                                     // exceeds search_band_max() rows goes on the flag2 list instead of being walked by its one workgroup
    int* huge_seen;                  // host-visible word (or null): set when a merge workgroup had to walk such a band itself (exact_follows == 0);
                                     // the engine launches the exact pass behind the index's streaming searches from then on
    // ---- certification of the candidate selection (search_common.h: certify_tail)
    const float* thr_used;           // thresholds the sweep STARTED from (set by the launcher; null: none)
    float eps_rel;                   // >= 0: |bf16-MFMA score - fp32 score| <= eps_rel * |q| * dmax (the caller's model);
                                     // < 0: no certification; eps_data set: ignored, the bound is search_common.h's query_eps
    int eps_data;                    // 1: the default, data-dependent rigorous bound (needs dmax[1] and acc_rel)
    float acc_rel;                   // its accumulation term: (2 dim + 128) 2^-24
    const float* dmax;               // device floats: [0] largest row norm |d|, [1] largest bf16 rounding residual |d - bf16(d)|
    int* flag_count; int* flag_list; // queries whose top-k could not be certified: the band pass (search_band.hip) redoes them
    float* flag_tau;                 // [slot] the flagged query's tau = s_k - eps (-inf: unknown)
    void* flag_q;                    // bf16 [slots][dim]: the flagged queries' bf16 rows, compacted (the band pass's GEMM operand)
    int* flag2_count; int* flag2_list;   // flagged queries whose band holds too many rows: the exact fp32 pass redoes them
    unsigned* stats;                 // [0] certified at once [1] after extended re-scoring [2] flagged [3] uncertified mode
                                     // [4] candidates gathered a second time [5] of the flagged: redone by the exact fp32 pass
    // ---- packed output (multi-GPU exchange format): key = orderable(score) << 32 | ~(row + id_offset); 0 = none
    unsigned long long* out_keys; int64_t id_offset;   // when set, out_scores / out_ids are not written
    hipEvent_t* prof_ev;             // optional [SEARCH_PROF_EVENTS] stage marks recorded on the launch stream
};
constexpr int SEARCH_PROF_EVENTS = 6;   // start | queries converted | thresholds | sweep | merge | exact pass
int search_kprime(int k);            // candidates kept per (query, chunk); 0 if k unsupported
int search_num_chunks(int64_t n_docs, int nq);         // workgroup chunks of the sweep (over the rows it sweeps: see search_prepass_owned)
// 8 when the threshold pre-pass OWNS its sample (the 256-tile sweep on the one-wave kernel, >= 128 index tiles), else 0: the caller
// adds it to n_chunks (list chunks) and sets SearchArgs::pre_own_chunks / thr_cert
int search_prepass_owned(int64_t n_docs, int nq, int dim);
constexpr int SEARCH_PRE_SPOTS = 16;    // sampled 256-row tiles of the owning pre-pass: tile k * S + S - 1, S = index tiles / 16
int search_prepass_floats();         // floats of cand_scores per (padded) query the threshold pre-pass needs
hipError_t launch_search(const SearchArgs& a, hipStream_t s);
bool search_uses_stream(int nq, int dim);   // nq <= 16: index streamed through registers (search_small.hip)
int search_stream_chunks();
hipError_t launch_search_stream(const SearchArgs& a, int kp, hipStream_t s);   // sweep only; merge: search_merge_wg_kernel
bool search_uses_256(int nq);         // more than 128 queries: main sweep on the 256^2 tile (search256.hip)
hipError_t launch_sweep256(const SearchArgs& a, int kp, const float* thr, hipStream_t s);
// the same sweep on the one-wave-per-SIMD tile (search256w.hip; dim % 128 == 0): sweep only, launch_sweep256 merges
bool sweep256w_ok(const SearchArgs& a);
hipError_t launch_sweep256w(const SearchArgs& a, int kp, const float* thr, hipStream_t s);   // (honours pre_own_chunks)
// k > 26 (search_bigk.hip): radix select over the block's score rows S + exact re-score; k <= search_bigk_max()
int search_bigk_max();
hipError_t launch_search_bigk(const SearchArgs& a, const float* S, size_t ldS, int nq_block, hipStream_t s);
hipError_t launch_topk_merge_big(const float* scores, const int64_t* ids, int n_parts, int nq, int k,
                                 float* out_scores, int64_t* out_ids, hipStream_t s);   // n_parts * k <= 8192
hipError_t launch_topk_merge(const float* scores, const int64_t* ids, int n_parts, int nq, int k,
                             float* out_scores, int64_t* out_ids, hipStream_t s);
// the same merge over packed keys [n_parts][nq][k] (SearchArgs::out_keys format; ids are global already)
hipError_t launch_topk_merge_keys(const unsigned long long* keys, int n_parts, int nq, int k, float* out_scores,
                                  int64_t* out_ids, hipStream_t s);      // n_parts * k <= 8192
// ---- exact fp32 pass for the flagged queries (search_exact.hip)
// S[slot][doc] = fp32 dot(query flag_list[slot], row doc) for slot < *flag_count, in the summation order of the
// re-scoring (search_common.h: dot_lane) — every workgroup leaves at once when nothing is flagged
// entries [sub, sub + max_slots) of the list are this launch's slots 0.. (a pass over a bounded score buffer)
hipError_t launch_exact_scores(const float* index_f32, int64_t n_docs, int dim, const float* q_f32, const int* flag_list,
                               const int* flag_count, int sub, int max_slots, float* S, size_t ldS, hipStream_t s);
// top-k of the flagged queries from their exact score rows (radix select + re-score + sort): overwrites their outputs
// (a.flag_count / a.flag_list: the list the scores were made for)
hipError_t launch_exact_select(const SearchArgs& a, const float* S, size_t ldS, int sub, int max_slots, hipStream_t s);
// ---- band pass for the flagged queries (search_band.hip): S[slot][doc] = bf16-MFMA scores of flagged query
// flag_list[sub + slot] (GEMM over a.flag_q); every row with a score >= its tau re-scored in fp32, top k emitted; a band of
// more than search_band_max() rows goes on the flag2 list (exact fp32 pass)
int search_band_max();
hipError_t launch_band_select(const SearchArgs& a, const float* S, size_t ldS, int sub, int max_slots, hipStream_t s);
// dmax[0] = max(dmax[0], |row|), dmax[1] = max(dmax[1], |row - bf16(row)|) over n rows (vr_index_add)
hipError_t launch_row_norm_max(const float* rows, int64_t n, int dim, float* dmax, hipStream_t s);
float search_default_eps_rel(int dim);      // worst-case relative bound (a caller's yardstick; the default bound is data-dependent)
float search_acc_rel(int dim);
// ---- grouped search (search_group.hip): the k best groups of adjacent rows per query, each with its best row
struct GroupSearchArgs {
    SearchArgs a;                    // the block's view, as for launch_search_bigk: index, queries, k, out_scores / out_ids, the error
                                     // model (eps_data / eps_rel / acc_rel / dmax: ALWAYS a valid model, it also bounds the rows re-scored
                                     // inside a group), flag_count / flag_list (the grouped search's own); everything else unused
    const int* goff;                 // [n_groups + 1] first row of every group; goff[n_groups] = n_docs
    int n_groups;
    float* B; size_t ldB;            // group maxima [slot][ldB] of the score rows at hand
    int64_t* out_groups;             // [nq][k] group of every result (-1: none)
    unsigned* stats;                 // [0] certified from the first candidate set [1] after widening it [2] flagged: redone exactly
    int certify;                     // 0: the first candidate set re-scored, no guarantee
};
int search_groups_kmax();
// B[slot][g] = max of S[slot][rows of group g] for n_slots score rows; slot_count set: only the first *slot_count - sub of them
hipError_t launch_group_max(const float* S, size_t ldS, const int* goff, int n_groups, float* B, size_t ldB, int n_slots,
                            const int* slot_count, int sub, hipStream_t s);
hipError_t launch_group_select(const GroupSearchArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s);
// the flagged queries from EXACT score rows / group maxima (slot i = query flag_list[sub + i]): overwrites their outputs
hipError_t launch_group_select_exact(const GroupSearchArgs& p, const float* S, size_t ldS, int sub, int max_slots, hipStream_t s);
// ---- filtered search (search_filter.hip): the k best rows per query among the rows its filter allows
struct FilterSearchArgs {
    SearchArgs a;                    // the block's view, as for launch_search_bigk: index, queries, k, out_scores / out_ids, the error
                                     // model, flag_count / flag_list (the filtered search's own); everything else unused
    const uint32_t* bits;            // [n_filters][words] the library's copy: bit r & 31 of word r >> 5 = row r allowed, bits >= n_docs clear
    size_t words;                    // (n_docs + 31) / 32
    int n_filters;
    const int* allowed;              // [n_filters] allowed rows of every filter
    const int* filter_of_query;      // [nq] device: the filter of every query of the block, -1 = all rows; an entry outside
                                     // [-1, n_filters) allows nothing
    unsigned* stats;                 // [0] certified from the first candidate set [1] after widening it [2] flagged: redone exactly
    int certify;                     // 0: the first candidate set re-scored, no guarantee, nothing counted
};
// the library's copy of the filters as the caller's words arrived: spare bits of the last word cleared, allowed[f] = popcount
hipError_t launch_filter_prepare(uint32_t* bits, size_t words, int n_filters, int64_t n_rows, int* allowed, hipStream_t s);
// what the mask reads: the first three as FilterSearchArgs', filter_of_query [nq] device, the rows of the index
struct MaskArgs {
    const uint32_t* bits;
    size_t words;
    int n_filters;
    const int* filter_of_query;
    int64_t n_docs;
};
// disallowed columns of score rows [0, n_slots) of S -> -inf (row i = query i of the block; slot_count set: the first
// *slot_count - sub rows only, row i = query flag_list[sub + i])
hipError_t launch_filter_mask(const MaskArgs& m, float* S, size_t ldS, int n_slots, const int* flag_list, const int* slot_count,
                              int sub, hipStream_t s);
hipError_t launch_filter_select(const FilterSearchArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s);
// the flagged queries from masked EXACT score rows (slot i = query flag_list[sub + i]): overwrites their outputs
hipError_t launch_filter_select_exact(const FilterSearchArgs& p, const float* S, size_t ldS, int sub, int max_slots, hipStream_t s);
// ---- range search (search_range.hip): every row whose fp32 score reaches the query's threshold, CSR, ascending row id
struct RangeSearchArgs {
    SearchArgs a;                    // the block's view, as for launch_search_bigk: index_f32, n_docs, dim, q_f32, nq and the error
                                     // model (ALWAYS a valid one, as for GroupSearchArgs); everything else unused
    const float* thresholds;         // [nq] device: the threshold of every query of the block; not finite: an empty segment
    const int* filter_of_query;      // [nq] device or null (no filter for any query): as FilterSearchArgs'; the score rows have been
    int n_filters;                   //   masked by launch_filter_mask; an entry outside [-1, n_filters): an empty segment
    float* out_scores; int64_t* out_ids;   // the result arrays of the whole call (the pack writes at lims[q] + scanned offset)
    unsigned long long* stats;       // [0] queries [1] candidate rows re-scored in fp32 [2] rows kept
};
bool range_dim_ok(int dim);          // the dim limits of the fp32 re-scoring (search_common.h: dot_lane)
int64_t range_scan_slots(int64_t n_docs);   // counts / offsets per query: one per 1024 columns
// S rows [0, nq_block): the band b >= t - eps re-scored in place (e where e >= t, else -inf); counts [nq_block][slots] = rows kept
hipError_t launch_range_rescore(const RangeSearchArgs& p, float* S, size_t ldS, int nq_block, int* counts, hipStream_t s);
// offs [nq_block][slots] = exclusive scan of a query's counts; lims[q + 1] = base + entries of the block's queries <= q (lims: the
// block's first query's entry of the call's lims; first: lims[0] = 0); *block_total = entries of the block
hipError_t launch_range_scan(const int* counts, int* offs, int64_t n_docs, int nq_block, int64_t base, int first, int64_t* lims,
                             int64_t* block_total, hipStream_t s);
// (score, id) of every column with S >= t -> p.out_scores / p.out_ids [lims[q] + offs ...], in column order
hipError_t launch_range_pack(const RangeSearchArgs& p, const float* S, size_t ldS, int nq_block, const int* counts, const int* offs,
                             const int64_t* lims, hipStream_t s);
// ---- rank search (search_rank.hip): the exact rank and score of named rows, exact counts against thresholds; a pair = (query, bar)
struct RankSearchArgs {
    SearchArgs a;                    // the block's view, as RangeSearchArgs': index_f32, n_docs, dim, q_f32, nq and a valid error model
    const int* pair_query;           // [pairs] device: the pair's query inside the block, 0 .. nq - 1
    const int* pair_id;              // [pairs] device: the target row of a rank, in [0, n_docs) ... (exactly one of the two is set)
    const float* pair_thr;           // [pairs] device: ... or the threshold of a count, finite
    int strict;                      // counts: 0 = rows with e >= t, 1 = rows with e > t
    const int* filter_of_query;      // [nq] device or null, as RangeSearchArgs': the score rows have been masked; an entry outside
    int n_filters;                   //   [-1, n_filters): the pair's count is 0
    unsigned long long* bars;        // [pairs] scratch: make_key(target's fp32 score, id), or the threshold's bits
    float* bar_eps;                  // [pairs] scratch: query_eps of the pair's query (NaN: nothing to count)
    float* out_scores;               // [pairs] ranks: the target's fp32 score; counts: unused
    unsigned long long* out_counts;  // [pairs] rows ahead of the bar
    unsigned long long* stats;       // [0] pairs [1] band candidates re-scored in fp32 [2] rows counted
};
// the bars (and the scores of the targets) of the block's pairs; their counts start at 0
hipError_t launch_rank_bars(const RankSearchArgs& p, size_t ldS, int nq_block, int64_t n_pairs, hipStream_t s);
// out_counts[pair] += rows of S row pair_query[pair] ahead of the pair's bar, the band around it decided by fp32 re-scoring; S is only read
hipError_t launch_rank_count(const RankSearchArgs& p, const float* S, size_t ldS, int nq_block, int64_t n_pairs, hipStream_t s);
// ---- windowed search (search_window.hip): the rows at ranks [offset, offset + k) of a query's fp32 ranking, any offset
struct WindowSearchArgs {
    SearchArgs a;                    // the block's view, as RangeSearchArgs': index_f32, n_docs, dim, q_f32, nq and a valid error model;
                                     // k, out_scores / out_ids [nq][k]: the block's part of the result (no out_keys)
    const int64_t* offsets;          // [nq] device: the first rank of every query's window, >= 0
    const int* filter_of_query;      // [nq] device or null, as RangeSearchArgs': the score rows have been masked; an entry outside
    int n_filters;                   //   [-1, n_filters): a row of tails
    const int* allowed;              // [n_filters] device (filter_of_query set): the rows every filter allows
    float* edges;                    // [nq][2] scratch: the band {lo, hi} of bf16 scores the window's rows lie in (NaN: an empty window)
    unsigned long long* stats;       // [0] queries [1] band candidates re-scored in fp32 [2] rows certainly ahead of their window
};
// edges[q] from two radix selects over S row q (masked bf16-MFMA scores); S is only read
hipError_t launch_window_edges(const WindowSearchArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s);
// S rows [0, nq_block) rewritten in place: +inf certainly ahead, -inf certainly behind or masked, the fp32 score inside the band
hipError_t launch_window_rescore(const WindowSearchArgs& p, float* S, size_t ldS, int nq_block, hipStream_t s);
// ranks [offset, offset + k) of the rewritten rows -> a.out_scores / a.out_ids, (-inf, -1) past the allowed rows
hipError_t launch_window_select(const WindowSearchArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s);
// ---- document window search (search_group_window.hip): the groups at ranks [offset, offset + k) of a query's document ranking
struct GroupWindowArgs {
    SearchArgs a;                    // the block's view, as WindowSearchArgs': index_f32, n_docs, dim, q_f32, nq and a valid error model;
                                     // k, out_scores / out_ids [nq][k]: the block's part of the result (no out_keys)
    const int* goff;                 // [n_groups + 1] first row of every group; goff[n_groups] = n_docs
    int n_groups;
    float* B; size_t ldB;            // [nq][ldB] group maxima of the (masked) score rows: launch_group_max; rewritten in place
    int* R;                          // [nq][ldB] scratch: the best row of every band group
    const int64_t* offsets;          // [nq] device: the first rank of every query's window, >= 0
    const int* filter_of_query;      // [nq] device or null, as WindowSearchArgs': the score rows have been masked; an entry outside
    int n_filters;                   //   [-1, n_filters): a row of tails
    float* edges;                    // [nq][2] scratch: the band {lo, hi} of group maxima the window's groups lie in (NaN: an empty window)
    int* present;                    // [nq] scratch: groups with an allowed row
    int64_t* out_groups;             // [nq][k] the block's part: the group of every result (-1: a tail)
    unsigned long long* stats;       // [0] queries [1] band groups re-scored [2] fp32 row dots
};
// edges[q] / present[q] from p.B row q (group maxima of masked bf16-MFMA scores); B is only read
hipError_t launch_group_window_edges(const GroupWindowArgs& p, int nq_block, hipStream_t s);
// B rows [0, nq_block) rewritten in place: +inf certainly ahead, -inf certainly behind or absent, E_g inside the band (R: its best
// row); S (the masked score rows the maxima came from) is only read
hipError_t launch_group_window_rescore(const GroupWindowArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s);
// ranks [offset, offset + k) of the rewritten rows -> a.out_scores / a.out_ids / out_groups, (-inf, -1, -1) past the present groups
hipError_t launch_group_window_select(const GroupWindowArgs& p, int nq_block, hipStream_t s);
// ---- document rank search (search_group_rank.hip): the exact rank, score and best row of named groups, exact counts of groups
// against thresholds, under filters; a pair = (query, bar)
struct GroupRankArgs {
    SearchArgs a;                    // the block's view, as RankSearchArgs': index_f32, n_docs, dim, q_f32, nq and a valid error model
    const int* goff;                 // [n_groups + 1] first row of every group; goff[n_groups] = n_docs
    int n_groups;
    const float* B; size_t ldB;      // [nq][ldB] group maxima of the (masked) score rows: launch_group_max; only read
    const int* pair_query;           // [pairs] device: the pair's query inside the block, 0 .. nq - 1
    const int* pair_group;           // [pairs] device: the target group of a rank, in [0, n_groups) ... (exactly one of the two is set)
    const float* pair_thr;           // [pairs] device: ... or the threshold of a count, finite
    int strict;                      // counts: 0 = groups with E >= t, 1 = groups with E > t
    const int* filter_of_query;      // [nq] device or null, as RankSearchArgs': the score rows have been masked; an entry outside
    int n_filters;                   //   [-1, n_filters): a rank's tail triple, a count of 0
    unsigned long long* bars;        // [pairs] scratch: make_key(target's E_g, g), or the threshold's bits
    float* bar_eps;                  // [pairs] scratch: query_eps of the pair's query (NaN: a dead pair, its outputs are final)
    float* out_scores;               // [pairs] ranks: E_g of the target (-inf: absent); counts: unused
    long long* out_rows;             // [pairs] ranks: the target's best row (-1: absent); counts: unused
    unsigned long long* out_counts;  // [pairs] groups ahead of the bar (a rank's absent target: -1)
    unsigned long long* stats;       // [0] pairs [1] band groups re-scored (a rank's target among them) [2] fp32 row dots
};
// the bars (and score / best row of the targets) of the block's pairs from p.B and S; their counts start at 0, or stay at -1
hipError_t launch_group_rank_bars(const GroupRankArgs& p, const float* S, size_t ldS, int nq_block, int64_t n_pairs, hipStream_t s);
// out_counts[pair] += groups of B row pair_query[pair] ahead of the pair's bar, the band around it decided by fp32 re-scoring of
// the band groups' rows; B and S are only read
hipError_t launch_group_rank_count(const GroupRankArgs& p, const float* S, size_t ldS, int nq_block, int64_t n_pairs, hipStream_t s);
// ---- document range search (search_group_range.hip): every group whose score reaches the query's threshold, under filters, CSR,
// ascending group
struct GroupRangeArgs {
    SearchArgs a;                    // the block's view, as RangeSearchArgs': index_f32, n_docs, dim, q_f32, nq and a valid error model
    const int* goff;                 // [n_groups + 1] first row of every group; goff[n_groups] = n_docs
    int n_groups;
    float* B; size_t ldB;            // [nq][ldB] group maxima of the (masked) score rows: launch_group_max; rewritten in place
    int* R;                          // [nq][ldB] scratch: the best row of every band group
    const float* thresholds;         // [nq] device: the threshold of every query of the block; not finite: an empty segment
    const int* filter_of_query;      // [nq] device or null, as RangeSearchArgs': the score rows have been masked; an entry outside
    int n_filters;                   //   [-1, n_filters): an empty segment
    float* out_scores; int64_t* out_rows; int64_t* out_groups;   // the result arrays of the whole call (the pack writes at lims[q] +
                                     // scanned offset)
    unsigned long long* stats;       // [0] queries [1] band groups re-scored [2] fp32 row dots
};
// B rows [0, nq_block): the band B >= t - eps re-scored in place (E_g where E_g >= t, else -inf; R: its best row); counts
// [nq_block][range_scan_slots(n_groups)] = groups kept per 1024; S (the masked score rows the maxima came from) is only read.
// The scan between the two launches is launch_range_scan with n_groups in the place of n_docs
hipError_t launch_group_range_rescore(const GroupRangeArgs& p, const float* S, size_t ldS, int nq_block, int* counts, hipStream_t s);
// (B[g], R[g], g) of every group with B >= t -> p.out_scores / p.out_rows / p.out_groups [lims[q] + offs ...], in group order
hipError_t launch_group_range_pack(const GroupRangeArgs& p, int nq_block, const int* counts, const int* offs, const int64_t* lims,
                                   hipStream_t s);
// ---- fused search (search_multi.hip): the k rows of largest max (or min) fp32 score over a group of sub-queries
struct MultiSearchArgs {
    SearchArgs a;                    // the block's view, as WindowSearchArgs': q_f32 and nq are the block's SUB-QUERIES (whole groups, <= 256),
                                     // k, out_scores / out_ids [groups][k]: the block's part of the result (no out_keys), a valid error model
    const int* lims;                 // [groups + 1] device: the block's entries of the call's lims; group g = sub-queries lims[g] .. lims[g + 1] - 1
    int sub_base;                    // the call's index of the block's first sub-query (= lims[0]): score row of sub-query s is s - sub_base
    int fuse;                        // 0: max over the group, 1: min
    const int* filter_of_group;      // [groups] device or null, as WindowSearchArgs' filter_of_query: the score rows have been masked
    int n_filters;                   //   with the group's filter in every sub-row; an entry outside [-1, n_filters): a row of tails
    const int* allowed;              // [n_filters] device (filter_of_group set): the rows every filter allows
    float* edges;                    // [groups] scratch: the band's lower edge lo of fused bf16 scores (NaN: nothing allowed)
    int* out_which;                  // [groups][k] the block's part: the in-group sub-query that decided every row (-1: a tail)
    unsigned long long* stats;       // [0] groups [1] band columns re-scored in fp32 [2] fp32 row dots (columns x group size)
};
// filter_of_sub[s] = filter_of_group[g] for lims[g] <= s < lims[g + 1]: the mask's filter of every score row
hipError_t launch_multi_expand(const int* lims, const int* filter_of_group, int n_groups, int* filter_of_sub, hipStream_t s);
// the group's first score row becomes the column-wise max / min over its rows (masked bf16-MFMA scores)
hipError_t launch_multi_fuse(const MultiSearchArgs& p, float* S, size_t ldS, int n_groups, hipStream_t s);
// edges[g] from a radix select over group g's fused row; S is only read
hipError_t launch_multi_edges(const MultiSearchArgs& p, const float* S, size_t ldS, int n_groups, hipStream_t s);
// the fused rows rewritten in place: -inf certainly behind or masked, the fp32 fused score at or above the edge
hipError_t launch_multi_rescore(const MultiSearchArgs& p, float* S, size_t ldS, int n_groups, hipStream_t s);
// the k best of the rewritten fused rows -> a.out_scores / a.out_ids / out_which, (-inf, -1, -1) past the allowed rows
hipError_t launch_multi_select(const MultiSearchArgs& p, const float* S, size_t ldS, int n_groups, hipStream_t s);
// ---- fused document search (search_multi_group.hip): the k groups of rows (documents) of largest max (or min) over a question's
// sub-queries of the document's best allowed page, with the best page per sub-query (the evidence)
struct MultiGroupArgs {
    SearchArgs a;                    // the block's view, as MultiSearchArgs': q_f32 and nq are the block's SUB-QUERIES (whole questions, <= 256),
                                     // k, out_scores / out_ids (best rows) [questions][k]: the block's part (no out_keys), a valid error model
    const int* lims;                 // [questions + 1] device: the block's entries of the call's lims (the call's own numbering)
    int sub_base;                    // the call's index of the block's first sub-query (= lims[0]): score row of sub-query s is s - sub_base
    int fuse;                        // 0: max over the question, 1: min
    const int* goff;                 // [n_groups + 1] first row of every document; goff[n_groups] = n_docs
    int n_groups;
    const float* B; size_t ldB;      // [nq][ldB] document maxima of the (masked) score rows: launch_group_max; only read
    float* F;                        // [questions][ldB] the fused rows: written by the fusion, rewritten in place by the re-scoring
    float* eps_sub;                  // [nq] scratch: query_eps of every sub-query of a non-empty question
    const int* filter_of_group;      // [questions] device or null: the score rows have been masked with the question's filter in every
    int n_filters;                   //   sub-row; an entry outside [-1, n_filters): a row of tails
    float* edges;                    // [questions] scratch: the band's lower edge lo of fused bf16 values (NaN: no document present)
    int* present;                    // [questions] scratch: documents with an allowed page
    int64_t* out_docs;               // [questions][k] the block's part: the document of every result (-1: a tail)
    int* out_which;                  // [questions][k] the block's part: the in-question sub-query that decided it (-1: a tail)
    float* out_ev_scores; int64_t* out_ev_rows;   // both null, or the CALL's evidence arrays [n_sub * k]: question g's block starts at
                                     // k * lims[g] and reads [k][m_g] = (E_j(D), row_j(D)); (-inf, -1) in a tail
    unsigned long long* stats;       // [0] questions [1] band documents re-scored [2] fp32 page dots
};
// F rows [0, n_questions) = column-wise max / min of the questions' B rows
hipError_t launch_multi_group_fuse(const MultiGroupArgs& p, int n_questions, hipStream_t s);
// edges / present / eps_sub from the F rows; F is only read
hipError_t launch_multi_group_edges(const MultiGroupArgs& p, int n_questions, hipStream_t s);
// the F rows rewritten in place: -inf certainly behind or absent, F(D) at or above the edge; S and B are only read
hipError_t launch_multi_group_rescore(const MultiGroupArgs& p, const float* S, size_t ldS, int n_questions, hipStream_t s);
// the k best of the rewritten F rows -> out_scores / out_ids / out_docs / out_which (/ the evidence), tails past the present documents
hipError_t launch_multi_group_select(const MultiGroupArgs& p, const float* S, size_t ldS, int n_questions, hipStream_t s);
// ---- diversified search (search_diverse.hip): k rows per query picked by maximal marginal relevance from a pool of its best rows
struct MmrArgs {
    const float* index_f32;          // [n_docs][dim] f32
    int64_t n_docs;
    int dim;
    const float* pool_scores;        // [nq][pool] a search's result for k = pool: fp32 scores, best first ...
    const int64_t* pool_ids;         // ... and row ids; the (-inf, -1) tail of a query with fewer rows is not part of its pool
    int nq, pool, k;                 // 1 <= k <= pool <= 1000
    float lambda;                    // 0..1: weight of the relevance; 1 - lambda weighs the largest dot with a picked row
    float* out_scores; int64_t* out_ids;               // [nq][k] the picks in pick order, their pool scores; tail (-inf, -1)
};
bool mmr_dim_ok(int dim);            // the dim limits of the fp32 re-scoring (search_common.h: dot_lane)
hipError_t launch_mmr_select(const MmrArgs& p, hipStream_t s);
// ---- rank fusion (search_rrf.hip): the k ids of largest reciprocal-rank-fusion score over the lists of a group's sub-queries
struct RrfArgs {
    const int64_t* ids;              // [n_lists][depth] device: slot r of list j; an id outside [0, 2^31 - 2] is an empty slot
    const int* lims;                 // [groups + 1] device: group g = lists lims[g] .. lims[g + 1] - 1 (1..256 of them, m * depth <= rrf_max_entries())
    const float* weights;            // [n_lists] device or null (every weight 1)
    int depth, k;                    // slots per list; result slots per group
    float c;                         // the term of entry (j, r) is (double)w_j / ((double)c + (double)(r + 1)); finite, >= 0
    float* out_scores; int64_t* out_ids; int* out_hits;   // [groups][k]; (-inf, -1, 0) past the distinct ids
    unsigned long long* stats;       // null, or [0] groups [1] non-empty entries [2] distinct ids
};
int rrf_max_entries();               // the largest m * depth of one group
// max_entries: the largest m * depth among the groups (sizes the dynamic LDS)
hipError_t launch_rrf_fuse(const RrfArgs& p, int n_groups, int max_entries, hipStream_t s);
// ---- editing in place (index_edit.hip): whole rows of `row_bytes` (a multiple of 16) moved by whole waves.  rem: the removed rows,
// sorted and distinct (device, nr ints); src(j) = j + #{i : rem[i] - i <= j} = the old row that becomes row j
// out rows [0, n_rows) = store rows src(j0) .. src(j0 + n_rows - 1).  `out` may lie inside `store` if the rows written (all below
// j0 + n_rows) and the rows read (all >= src(j0)) are apart: workgroups are not ordered, only launches are
hipError_t launch_rows_compact(const void* store, size_t row_bytes, const int* rem, int nr, int64_t j0, int64_t n_rows, void* out,
                               hipStream_t s);
// out row i = store row ids[i] (device ints, in range — the caller has checked them; duplicates allowed)
hipError_t launch_rows_gather(const void* store, size_t row_bytes, const int* ids, int64_t n_rows, void* out, hipStream_t s);
// f32 row ids[i] = reps row i and bf16 row ids[i] = its conversion (as launch_f32_to_bf16); ids distinct and in range, dim % 8 == 0
hipError_t launch_rows_update(const float* reps, const int* ids, int64_t n, int dim, float* f32, void* bf16, hipStream_t s);
// out [n_filters][ceil(new_n / 32)]: bit j of a filter = bit src(j) of bits [n_filters][words] (words = ceil((new_n + nr) / 32)),
// bits at or beyond new_n clear; out is another buffer
hipError_t launch_filter_compact(const uint32_t* bits, size_t words, int n_filters, const int* rem, int nr, int64_t new_n,
                                 uint32_t* out, hipStream_t s);

}  // namespace vr
