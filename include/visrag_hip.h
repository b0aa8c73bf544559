/*
 * visrag_hip.h — C ABI of libvisrag_hip.so: the MI355X (gfx950) native VisRAG-Ret
 * corpus-embedding + retrieval hot path.
 *
 * The reference (OpenBMB/VisRAG) has NO FFI for this path — it is pure Python over
 * PyTorch ops — so this header is new surface.  Each entry point states the reference
 * interface (file:line under /root/reference) whose device math it replaces; the Python
 * adapter in visrag_amd/ keeps the reference's operator API on top of it
 * (INTEGRATION.md shows the ctypes binding a maintainer would add).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; vr_last_error() gives text
 *     (reference convention is Python exceptions: dense_retriever.py:70-71,
 *      inference.py:105-108 — the adapter raises RuntimeError from the status).
 *   - plain pointers and sizes only; no torch types.  "dev" pointers are HIP device
 *     pointers (e.g. tensor.data_ptr() of a torch-ROCm tensor used as a container).
 *   - the library owns device weights, workspace and the HBM-resident index; the caller
 *     owns every input and output buffer.  No cross-boundary frees.
 *   - a handle is NOT thread-safe: one handle per process / GPU (the reference runs one
 *     process per GPU under torchrun, eval.sh:48).  `stream` is a hipStream_t (NULL = the
 *     default stream) so torch containers stay ordered with the kernels.
 */
#ifndef VISRAG_HIP_H
#define VISRAG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_OK 0
#define VR_ERR_INVALID 1   /* bad argument / shape / missing weight */
#define VR_ERR_HIP 2       /* HIP runtime failure */
#define VR_ERR_STATE 3     /* call order (e.g. encode before weights are finalised) */
#define VR_ERR_CAPACITY 4  /* workspace / index capacity exceeded */

#define VR_DTYPE_F32 0
#define VR_DTYPE_BF16 1

typedef struct vr_model_s* vr_model_t;
typedef struct vr_index_s* vr_index_t;

/* Model dimensions (visrag_amd/config.py; SURVEY.md section 8 "dimension provenance"). */
typedef struct vr_config {
    int32_t patch_size;        /* 14 */
    int32_t vit_dim;           /* 1152 */
    int32_t vit_depth;         /* 26 (27 in the checkpoint, last dropped: modeling_minicpmv.py:70-71) */
    int32_t vit_heads;         /* 16  -> head_dim must be 72 */
    int32_t vit_hidden;        /* 4304 = int(1152*3.7362) */
    int32_t vit_pos_grid;      /* 27  (learned pos-embed is 27x27) */
    float   vit_ln_eps;        /* 1e-6 */
    int32_t query_num;         /* 64 */
    float   resampler_ln_eps;  /* 1e-6 */
    int32_t hidden_size;       /* 2304 -> resampler heads = hidden/128, head_dim 128 */
    int32_t num_layers;        /* 40 */
    int32_t num_heads;         /* 36  -> head_dim must be 64 */
    int32_t intermediate_size; /* 5760 */
    int32_t vocab_size;        /* 122753 */
    float   rms_norm_eps;      /* 1e-5 */
    float   rope_theta;        /* 1e4 */
    float   scale_emb;         /* 12 */
    float   residual_scale;    /* scale_depth / sqrt(num_layers) = 1.4/sqrt(40) */
    int32_t max_images;        /* workspace: image slices per ViT pass (chunk size) */
    int32_t max_patches;       /* workspace: patches per image slice (1024 for 448x448; <=1064 sliced) */
    int32_t max_tokens;        /* workspace: packed decoder tokens per vr_encode call */
    int32_t max_seqs;          /* workspace: sequences per vr_encode call */
    int32_t text_split_precision; /* 1: token-only batches (queries, text passages) run the decoder on hi + lo bf16
                                   * splits of activations and fp32 source weights with fp32 glue (fp32-class accuracy:
                                   * the 1e-3 score bar for ~20-token queries); 0: the bf16 path for everything;
                                   * N > 1: only token-only batches whose longest sequence has <= N tokens (512 = the
                                   * reference's query length): longer text passages stay on the bf16 MFMA attention path.
                                   * The route is per vr_encode CALL (a call with image slices runs the bf16 pass for all its
                                   * items); the host adapter (visrag_amd/modeling.py: encode_prepared) therefore groups the
                                   * token-only items of a batch into calls of their own, so that an item's embedding does not
                                   * depend on its batch mates. */
} vr_config_t;

/* ---- library ------------------------------------------------------------------------ */
const char* vr_version(void);
/* Last error text of this thread's most recent failing call. */
const char* vr_last_error(void);
int vr_device_count(int* count);

/* ---- model: replaces VisRAG_Ret.forward + pooling ----------------------------------- */
/* Reference: DRModelForInference.build / from_pretrained
 * (src/openmatch/modeling/dense_retrieval_model.py:233-364). */
int vr_model_create(int device_id, const vr_config_t* cfg, vr_model_t* out);
int vr_model_destroy(vr_model_t m);

/* Load one tensor of the HF state dict by its key (e.g.
 * "vpm.blocks.3.attn.qkv.weight", "resampler.proj", "llm.model.layers.7.mlp.up_proj.weight").
 * `data` is row-major with `shape[ndim]`; dtype VR_DTYPE_F32 or VR_DTYPE_BF16; on_device
 * tells whether `data` is a device pointer.  Unused keys (llm.lm_head.*, vpm.attn_pool.*,
 * vpm.blocks.<depth>.*, resampler.pos_embed, rotary buffers) are accepted and ignored.
 * Reference: PreTrainedModel.from_pretrained via dense_retrieval_model.py:292-318. */
int vr_model_load_weight(vr_model_t m, const char* name, const void* data,
                         const int64_t* shape, int32_t ndim, int32_t dtype, int32_t on_device);
/* Check that every required weight arrived and build derived tables (packed / padded
 * bf16 weights, resampler query projection, RoPE table). */
int vr_model_finalize(vr_model_t m);
/* A second handle on the same (finalised) weights with its own workspace: lets a caller keep two
 * batches in flight on two HIP streams (each vr_encode call is still ordered on the stream it is
 * given).  `src` must outlive the clone; the clone is destroyed with vr_model_destroy. */
int vr_model_clone(vr_model_t src, vr_model_t* out);

/* Encode a batch of items (pages and/or text queries) to unit-norm embeddings.
 *   slices      n_slices pointers to uint8 HWC (RGB) images, all on host or all on device
 *   slice_hw    [n_slices][2] = (H, W), multiples of patch_size
 *   input_ids   [T] packed token ids of all B items (already truncated to max_inp_length)
 *   seq_offsets [B+1] token offsets of the items in `input_ids` (seq_offsets[B] == T)
 *   vision_rows [n_slices*query_num] packed-token row that receives resampler output
 *               (slice s, query j), or -1 to drop it (the reference's scatter_ of image_bound)
 *   out_reps    [B][hidden_size] float32, device or host
 * Replaces: VisRAG_Ret.forward (modeling_visrag_ret.py:86-126) incl. ToTensor/Normalize
 * (modeling_minicpmv.py:84-92), get_vllm_embedding / get_vision_embedding (:95-171),
 * timm forward_features (vision_transformer.py:682-692), Resampler.forward
 * (resampler.py:146-168), MiniCPMModel.forward (modeling_minicpm.py:1147-1304), and the
 * wmean pooling + F.normalize of DRModel.encode (dense_retrieval_model.py:180-184,222-223). */
int vr_encode(vr_model_t m,
              const uint8_t* const* slices, const int32_t* slice_hw, int32_t n_slices,
              int32_t slices_on_device,
              const int32_t* input_ids, const int32_t* seq_offsets, int32_t B,
              const int32_t* vision_rows,
              float* out_reps, int32_t out_on_device, void* stream);

/* vr_encode, and ALSO the last hidden states the pooling reads — the HF-style forward of the reference's second caller:
 * `outputs = model(text=..., image=..., tokenizer=...)` returns `last_hidden_state` [B, L, hidden] + `attention_mask` and the
 * caller pools them itself (visrag_scripts/demo/visrag_pipeline/utils.py:12-32, demo/retriever/demo.py:14-36;
 * BaseModelOutputWithAttentionMask, modeling_visrag_ret.py:123-126).
 *   out_hidden  [B][hidden_len][hidden_size] float32 on the DEVICE: item i's post-norm rows, right-padded with zeros like the
 *               reference's `pad` (modeling_minicpmv.py:440-479); hidden_len >= the longest item. */
int vr_encode_hidden(vr_model_t m,
                     const uint8_t* const* slices, const int32_t* slice_hw, int32_t n_slices,
                     int32_t slices_on_device,
                     const int32_t* input_ids, const int32_t* seq_offsets, int32_t B,
                     const int32_t* vision_rows,
                     float* out_reps, int32_t out_on_device,
                     float* out_hidden, int32_t hidden_len, void* stream);

/* Pooling of the last hidden states (DRModel.encode, dense_retrieval_model.py:172-220), applied after the
 * final RMSNorm and followed by the L2 normalisation (:222-223).  VisRAG-Ret's published setting is wmean
 * (the default).  The reference's drop_wmean / drop_mean / lasttoken_simcse apply dropout in training mode
 * even at inference (a fresh nn.Dropout1d, :187,196; F.dropout(training=True), :215): stochastic there,
 * not offered here. */
#define VR_POOL_WMEAN 0      /* sum_t (t+1) h_t / sum_t (t+1)        :180-184 */
#define VR_POOL_MEAN 1       /* mean over the item's tokens           :204-207 */
#define VR_POOL_LASTTOKEN 2  /* last_token_pool, right padding        :26-34,172-177 */
#define VR_POOL_CLS 3        /* hidden[:, 0]                          :217-218 */
int vr_model_set_pooling(vr_model_t m, int32_t mode);

/* Debug taps for parity tests: copy an internal activation of the LAST vr_encode call to
 * host float32.  name in {"vit_embed","vit_block0","vit_out","resampler_out",
 * "inputs_embeds","dec_layer0","last_hidden"}; rows/cols describe `out`. */
int vr_model_tap(vr_model_t m, const char* name, float* out, int64_t rows, int64_t cols);
/* Enable/disable recording of taps (off by default; costs device copies). */
int vr_model_set_taps(vr_model_t m, int32_t enable);

/* Per-kernel-class HIP-event timing on the launch stream (bench.py roofline fields).
 * Enabling resets the counters.  total_flops is the ALGORITHMIC work of the launches
 * (SURVEY.md section 8d formulas), total_ms the sum of their event-bracketed durations. */
#define VR_PROF_VIT_QKV 0    /* gemm_bf16_kernel<EPI_BF16>  : qkv projection            */
#define VR_PROF_VIT_ATTN 1   /* attention_kernel<72,2>      : ViT self-attention        */
#define VR_PROF_VIT_PROJ 2   /* gemm_bf16_kernel<EPI_RESID> : attn out-projection       */
#define VR_PROF_VIT_FC1 3    /* gemm_bf16_kernel<EPI_GELU>  : MLP fc1 + erf-GELU        */
#define VR_PROF_VIT_FC2 4    /* gemm_bf16_kernel<EPI_RESID> : MLP fc2 + residual        */
#define VR_PROF_RESAMPLER 5  /* whole resampler phase (several kernels)                 */
#define VR_PROF_DECODER 6    /* whole 40-layer decoder phase (several kernels)          */
/* the decoder phase again, split (events between its kernels: read these for shares, VR_PROF_DECODER for the total) */
#define VR_PROF_DEC_QKV 7    /* q|k|v projection + RoPE epilogue                        */
#define VR_PROF_DEC_ATTN 8   /* causal attention over the packed sequences              */
#define VR_PROF_DEC_O 9      /* o projection (split-K planes or residual epilogue)      */
#define VR_PROF_DEC_GU 10    /* gate|up projection + SwiGLU epilogue                    */
#define VR_PROF_DEC_DOWN 11  /* down projection                                         */
#define VR_PROF_DEC_NORM 12  /* RMSNorm passes (incl. the split-K accumulate)           */
#define VR_PROF_CLASSES 13
/* enable: 0 off, 1 the phase classes 0..6, 2 the decoder's sub-phases 7..12 instead (their events sit between the decoder's
 * kernels and would lengthen VR_PROF_DECODER if both were taken in one pass) */
int vr_model_set_profile(vr_model_t m, int32_t enable);
int vr_model_get_profile(vr_model_t m, int32_t cls, double* total_ms, int64_t* launches,
                         double* total_flops);

/* ---- chat: MiniCPM-V 2.0 answer generation on the model's weights ------------------- */
/* Reference: MiniCPMV.generate / chat (src/openmatch/modeling/modeling_minicpmv/modeling_minicpmv.py:218-237, 276-400) over
 * MiniCPMForCausalLM (modeling_minicpm.py:1411-1412: logits = lm_head(h / (hidden_size / dim_model_base))), driven by HF
 * generate; visrag_amd/generation.py holds the decoding loop.  A chat handle shares the weights of a finalised model (like
 * vr_model_clone: the model must outlive it) and owns its KV cache and workspace; the model's own vr_encode is unaffected.
 * Cache: a prompt SLOT keeps the rope'd K / V of one prompt, a ROW keeps the K / V of the tokens it generated (its tail)
 * and its seen-id set; the beams of a prompt are rows that share the slot.  Device memory: the caches, layers x 2 x
 * (max_slots x max_len + max_rows x max_new) x hidden_size bf16, the logits (2 max_rows x vocab f32), and a second
 * encode workspace for the prefill (a vr_model_clone of the model, sized by the model's vr_config_t). */
typedef struct vr_chat_s* vr_chat_t;
typedef struct vr_chat_config {
    int32_t max_len;        /* positions of a sequence: prompt + generated tokens (a prompt has at most max_len - 1) */
    int32_t max_rows;       /* rows of one step (prompts x beams), 1..16 */
    float   dim_model_base; /* 256 for MiniCPM-V 2.0 (config.json) */
    int32_t max_slots;      /* prompts held at once, 1..max_rows (one per prompt of a step: max_rows / num_beams) */
    int32_t max_new;        /* generated tokens a row can hold, 1..max_len - 1 (max_new_tokens) */
} vr_chat_config_t;
#define VR_CHAT_GREEDY 0    /* repetition penalty on the raw logits, then argmax (ties: lowest id) */
#define VR_CHAT_BEAM 1      /* log_softmax, penalty, + beam score; top-k over the group's rows x vocab */
#define VR_CHAT_SAMPLE 2    /* penalty, / temperature, top_k filter, softmax, one draw from counter noise */
int vr_chat_create(vr_model_t m, const vr_chat_config_t* cfg, vr_chat_t* out);
int vr_chat_destroy(vr_chat_t ch);
/* llm.lm_head.weight [vocab_size][hidden_size] (tied embeddings: pass llm.model.embed_tokens.weight); dtype / on_device as
 * in vr_model_load_weight.  Stored as padded bf16 for the decode step's weight streamer. */
int vr_chat_load_head(vr_chat_t ch, const void* data, const int64_t* shape, int32_t ndim, int32_t dtype, int32_t on_device);
/* Run ONE prompt (the arguments of vr_encode for a single item: T tokens) through tower, resampler and decoder on the bf16
 * route, keep every layer's K / V in `slot`, and leave the last token's logits on row `row`, which becomes the slot's first
 * row with an empty tail and an empty seen set (generation starts from inputs_embeds: only generated ids are penalised).
 * Rows that continued the slot before lose their tails.  T >= max_len: VR_ERR_CAPACITY. */
int vr_chat_prefill(vr_chat_t ch, int32_t slot, int32_t row, const uint8_t* const* slices, const int32_t* slice_hw,
                    int32_t n_slices, int32_t slices_on_device, const int32_t* input_ids, int32_t T,
                    const int32_t* vision_rows, void* stream);
/* The same for B prompts in ONE packed pass (the arguments of vr_encode for B items: seq_offsets [B + 1], vision_rows index the
 * packed rows): every layer's K / V rows of prompt b go to slot slots[b], its last token's logits to row rows[b], which is
 * bound to the slot as vr_chat_prefill binds it; rows that continued one of the slots lose their tails; the logits of rows
 * the call does not name stay readable.  The head streams its weights once per run of adjacent rows[] values.  The tile
 * and split-K choices of the decoder pass follow the packed token count, so a prompt's logits equal those of a lone
 * vr_chat_prefill to bf16 accuracy, not bit for bit.  Checked before anything changes: slots distinct and in range, rows
 * distinct and in range (VR_ERR_INVALID); a prompt of max_len tokens or more, more than the model's max_tokens tokens or
 * max_seqs prompts in all (VR_ERR_CAPACITY). */
int vr_chat_prefill_batch(vr_chat_t ch, int32_t B, const int32_t* slots, const int32_t* rows, const uint8_t* const* slices,
                          const int32_t* slice_hw, int32_t n_slices, int32_t slices_on_device, const int32_t* input_ids,
                          const int32_t* seq_offsets, const int32_t* vision_rows, void* stream);
/* Append tokens[i] to row rows[i] of prompt slot slots[i] (the rows of one slot adjacent) and compute each row's logits:
 * one pass over the weights for all n rows.  The token joins the row's seen set.  A row with an empty tail may start on any
 * slot.  n > max_rows, or a row past max_len or max_new: VR_ERR_CAPACITY, nothing changed. */
int vr_chat_step(vr_chat_t ch, int32_t n, const int32_t* slots, const int32_t* rows, const int32_t* tokens, void* stream);
/* Next-token candidates from the current logits of rows[] grouped by group_offsets [n_groups + 1] (beam search: one group
 * per prompt; greedy / sampling: one row per group).  Host outputs [n_groups][k]: score, token, parent (row index within the
 * group), best first; missing candidates are (-inf, -1, -1); a token whose score is -inf (a masked logit) is no candidate.
 *   VR_CHAT_GREEDY: score = penalised logit;  VR_CHAT_BEAM: score = penalised log-prob + beam_scores[i];
 *   VR_CHAT_SAMPLE: k = 1, top_k candidates (1..64), temperature > 0, noise selected by (seed, step, token). */
int vr_chat_select(vr_chat_t ch, int32_t mode, int32_t n_groups, const int32_t* group_offsets, const int32_t* rows,
                   const float* beam_scores, int32_t k, float repetition_penalty, float temperature, int32_t top_k,
                   uint64_t seed, int32_t step, float* out_scores, int32_t* out_tokens, int32_t* out_parents, void* stream);
/* The nucleus sampler: one draw per row from the current logits of rows[0..n), with ANY top_k (0 = off) and top_p, by a radix
 * select over the row (csrc/chat_sample.hip) — its cost does not grow with top_k.  vr_chat_select(VR_CHAT_SAMPLE) stays as it is.
 * Definition, per row: logits x[0..V) fp32, the row's seen set, repetition_penalty > 0, temperature > 0, top_k >= 0, 0 < top_p <= 1.
 *   1. s_t = the penalised logit VR_CHAT_SAMPLE scores with (x_t * penalty if x_t < 0 else x_t / penalty on seen ids);
 *      z_t = s_t * (1 / temperature), the rounded fp32 product — the value VR_CHAT_SAMPLE adds its noise to.
 *   2. A token whose z_t is -inf or NaN is no candidate.  Candidates are ordered by z descending, then token ascending.
 *   3. C = the number of candidates; K = C when top_k = 0, else min(top_k, C).
 *   4. m = the first candidate's z; w_t = the mass exp(z_t - m) as an unsigned 64-bit fixed-point integer of scale 2^40 (fp32
 *      exponential, truncated); Z = the integer sum of w over the first K candidates; A_j = the integer sum over the
 *      candidates ahead of position j.  Integer sums do not depend on the order of addition: the kept set is a function of
 *      the row alone.
 *   5. The candidate at position j is KEPT iff j < K and (top_p == 1 or A_j < top_p * Z, the product and the comparison in
 *      fp64).  Position 0 is always kept; top_p == 1 applies no mass filter at all (HF builds no TopPLogitsWarper then).
 *   6. The draw is the kept token of largest fma(s_t, 1 / temperature, noise(seed, step, t)) — the Gumbel-max and the noise
 *      of VR_CHAT_SAMPLE, bit for bit; among equal values the better-ranked candidate wins.
 * This is transformers 4.40.2's chain in order (repetition penalty, TemperatureLogitsWarper, TopKLogitsWarper,
 * TopPLogitsWarper with min_tokens_to_keep = 1, softmax, one multinomial draw) with two stated differences: where the k-th
 * value is exactly tied HF keeps every tied token and this keeps the lower ids (the library's tie rule everywhere); the noise
 * is counter-based, so a seed reproduces a run.
 * Host outputs [n]: out_scores = s of the drawn token, out_tokens, out_kept = the number of kept candidates, out_cut = the
 * last kept token in the order; a row without candidates gives (-inf, -1, 0, -1).  Every check comes before any launch and an
 * error leaves the outputs untouched: NULL pointers, n < 1, a penalty or temperature that is not positive, top_k < 0, top_p
 * outside (0, 1] or NaN are VR_ERR_INVALID; n > 16 or n > max_rows is VR_ERR_CAPACITY; a row without logits is VR_ERR_STATE. */
int vr_chat_sample(vr_chat_t ch, int32_t n, const int32_t* rows, float repetition_penalty, float temperature, int32_t top_k,
                   double top_p, uint64_t seed, int32_t step, float* out_scores, int32_t* out_tokens, int32_t* out_kept,
                   int32_t* out_cut, void* stream);
/* Row rows[i] becomes a copy of row parents[i] (slot, tail, seen set), all read before any is written; the prompt's K / V
 * are never copied. */
int vr_chat_reorder(vr_chat_t ch, int32_t n, const int32_t* rows, const int32_t* parents, void* stream);
/* The current logits of `row` (f32 [vocab_size]) to the host — tests. */
int vr_chat_logits(vr_chat_t ch, int32_t row, float* out, void* stream);
/* The prompt slot of `row` (-1: none) and the number of tokens in its tail. */
int vr_chat_row_len(vr_chat_t ch, int32_t row, int32_t* slot, int32_t* generated);
/* Teacher-forced scoring: how likely are GIVEN continuations?  B sequences (prompt + continuation each, the arguments of
 * vr_chat_prefill_batch) run in ONE packed causal pass on the bf16 route; the last cont_len[b] tokens of sequence b are its
 * continuation, 1 <= cont_len[b] < T_b.  For the continuation token at position p the hidden state of position p - 1 goes
 * through the final RMSNorm (the chat's scaled weight, as in vr_chat_prefill) and the fused head (csrc/head_score.hip), which
 * reduces each row's logits x without writing them:
 *   out_logit      x[token]                         (bf16 x bf16 products, fp32 accumulation)
 *   out_lse        log sum_{v < vocab_size} exp x[v]    (so log p(token) = out_logit - out_lse, before any penalty)
 *   out_top_logit  max_v x[v],  out_top_token its id (lowest id among exact ties)
 * Host arrays, flat [sum_b cont_len[b]], sequence after sequence.  Synchronises the stream.
 *   Stateless with respect to generation: no slot, row, tail, seen set or logits row is touched; vr_chat_row_len and
 * vr_chat_logits of every row return what they returned before, a generation in progress continues with the same tokens.
 * The row and partial buffers are allocated at the first call.
 *   Checked before any launch, the outputs untouched: a NULL pointer, B < 1, an empty sequence, cont_len out of range, a token
 * id outside [0, vocab_size): VR_ERR_INVALID; more than the model's max_seqs sequences or max_tokens packed tokens:
 * VR_ERR_CAPACITY; no head loaded: VR_ERR_STATE. */
int vr_chat_score(vr_chat_t ch, int32_t B, const uint8_t* const* slices, const int32_t* slice_hw, int32_t n_slices,
                  int32_t slices_on_device, const int32_t* input_ids, const int32_t* seq_offsets, const int32_t* vision_rows,
                  const int32_t* cont_len, float* out_logit, float* out_lse, float* out_top_logit, int32_t* out_top_token,
                  void* stream);
/* Several GIVEN tokens appended to prompts that are already cached, in ONE packed decoder pass on the bf16 route: tokens
 * [tok_offsets[b], tok_offsets[b + 1]) go to row rows[b] of slot slots[b].  Binding as in vr_chat_step: a row with an empty
 * tail may start on any slot that holds a prompt, a row with a tail continues its slot; several rows may share a slot and
 * need not be adjacent.  Token j of a row whose tail holds t0 tokens sits at tail index t0 + j and position plen + t0 + j (the
 * chat's own RoPE table); every layer's rope'd K / V rows go to the row's tail, and the attention reads the slot's prompt
 * keys, then the row's tail keys up to the token's own (csrc/chat_extend.hip).  Afterwards the row's tail holds t0 + n
 * tokens, its current logits are those after its last appended token (vr_chat_select / vr_chat_sample / vr_chat_step /
 * vr_chat_row_score continue from there); the logits of rows the call does not name stay readable.
 *   seen_mode 0 leaves the row's seen set alone, 1 adds the appended ids (forced tokens that count as generated), 2 clears
 * it (a new turn); a row that starts on a slot starts with an empty set in every mode.
 *   targets NULL: nothing is scored, the stream is not synchronised.  Otherwise targets [sum n] (-1 = none): entry t is the
 * distribution AFTER packed token t evaluated at targets[t], the four numbers of vr_chat_score; entries whose target is -1
 * are left untouched.  Synchronises the stream.
 *   Checked before any state changes, state and outputs untouched: a NULL pointer, B < 1, an empty token list, a token or
 * target id out of range, a slot without a prompt, a repeated row, a row that continues another slot: VR_ERR_INVALID;
 * B > max_rows, t0 + n > max_new, plen + t0 + n > max_len, sum n > the model's max_tokens, B > its max_seqs:
 * VR_ERR_CAPACITY; no head loaded: VR_ERR_STATE. */
int vr_chat_extend(vr_chat_t ch, int32_t B, const int32_t* slots, const int32_t* rows, const int32_t* tok_offsets,
                   const int32_t* tokens, const int32_t* targets, int32_t seen_mode, float* out_logit, float* out_lse,
                   float* out_top_logit, int32_t* out_top_token, void* stream);
/* The four numbers of vr_chat_score from the CURRENT logits of rows[i] at targets[i] (host arrays [n]; rows may repeat: the
 * first tokens of several continuations of one prefilled row are one call).  One workgroup per entry over the fp32 logits
 * row; the lowest id wins among tied maxima.  An id or row out of range: VR_ERR_INVALID; a row without logits:
 * VR_ERR_STATE.  Synchronises the stream. */
int vr_chat_row_score(vr_chat_t ch, int32_t n, const int32_t* rows, const int32_t* targets, float* out_logit, float* out_lse,
                      float* out_top_logit, int32_t* out_top_token, void* stream);
/* vr_chat_row_score from the logits of a slot's PROMPT, its last position (what a prefill leaves on its row): they outlive the
 * decode steps of a generation on that slot (steps write other lines) and are lost when a prefill or a vr_chat_extend writes
 * the logits of the row the prefill named.  slots may repeat.  A slot without a prompt or whose prompt logits are gone:
 * VR_ERR_STATE; otherwise as vr_chat_row_score.  This is how the first token of a continuation is scored on a prompt that a
 * finished generation left resident. */
int vr_chat_slot_score(vr_chat_t ch, int32_t n, const int32_t* slots, const int32_t* targets, float* out_logit, float* out_lse,
                       float* out_top_logit, int32_t* out_top_token, void* stream);
/* The prompt tokens `slot` holds (0: none), whether vr_chat_slot_score can still read the prompt's logits, and how often the
 * slot has been prefilled (vr_chat_prefill / vr_chat_prefill_batch, whoever called them): a caller that keeps a prompt in a slot
 * compares the count with the one it saw after its own prefill. */
int vr_chat_slot_state(vr_chat_t ch, int32_t slot, int32_t* prompt_len, int32_t* has_prompt_logits, int32_t* generation);
/* Shortens the tail of `row` to `length` tokens (0 <= length <= its current length, else VR_ERR_INVALID).  The row loses its
 * logits, its seen set stays; host state only. */
int vr_chat_row_truncate(vr_chat_t ch, int32_t row, int32_t length);

/* ---- index: replaces torch.matmul + torch.topk over pickle shards -------------------- */
/* Reference: _retrieve_one_shard / distributed_parallel_retrieve
 * (src/openmatch/retriever/dense_retriever.py:13-97); demo answer.py:26-35. */
int vr_index_create(int device_id, int32_t dim, int64_t capacity, vr_index_t* out);
int vr_index_destroy(vr_index_t ix);
int vr_index_reset(vr_index_t ix);
/* Append n rows of float32 [n][dim] (host or device); rows keep their insertion order,
 * the global id of a row is its position. */
int vr_index_add(vr_index_t ix, const float* reps, int64_t n, int32_t on_device, void* stream);
int vr_index_size(vr_index_t ix, int64_t* n);
/* For every query the k best rows by inner product: higher score first, lower row id first
 * among equal scores — the ranking torch.topk sees over the fp32 matmul of
 * dense_retriever.py:28-30.  Scores are fp32 dot products of the fp32 rows.  A bf16 MFMA
 * sweep selects candidates, the survivors are re-scored in fp32, and the selection is
 * CERTIFIED per query: with |bf16 score - fp32 score| <= eps (below) every row whose bf16 score
 * could still reach the fp32 top-k is re-scored too; a query whose candidate lists cannot prove
 * completeness (more near-ties at the k-th score than they hold, or a cluster of near-duplicate
 * pages that overran them) is redone by the band pass — bf16 scores of that query against every
 * row, ALL rows inside the error band re-scored in fp32 — and, if its band holds more than 8192
 * rows, by an exact fp32 pass over the whole index.  The ids are the fp32 ranking's.
 *   queries [nq][dim] float32;  out_scores [nq][k] float32;  out_ids [nq][k] int64
 * (all host or all device per `on_device`).  If the index holds fewer than k rows the
 * tail is filled with score -inf, id -1.  k = 1..1000: up to 26 on the fused sweep (the
 * throughput path; --retrieve_depth 10 in eval.sh), deeper runs on GEMM + radix select.
 * NaN, the same on every route (sweeps, merges, deep path, band pass, exact pass): a row whose
 * fp32 score against a query is NaN never ranks for that query — a row with a NaN component is
 * returned for no query, the other rows rank as if it were not there.  A query with a NaN
 * component gets (-inf, -1) in every slot, and key 0 in every slot from vr_index_search_keys;
 * the other queries of the batch are unaffected.  Both are counted by vr_index_search_stats
 * like any other query.  Infinite components, and finite ones whose fp32 or bf16 products or
 * sums overflow, are outside this contract: their scores may be inf or NaN on one route and
 * not on another. */
int vr_index_search(vr_index_t ix, const float* queries, int32_t nq, int32_t k,
                    float* out_scores, int64_t* out_ids, int32_t on_device, void* stream);
/* The error model of the certification.  Default (NaN restores it): the rigorous bound for the
 * data at hand — with dq = q - bf16(q), dd = d - bf16(d) (round to nearest even: bf16 keeps 8
 * significand bits, unit roundoff 2^-8) and fp32 accumulation,
 *   |bf16 score - fp32 score| <= |dq| max|d| + |q| max|dd| + |dq| max|dd|
 *                                + (2 dim + 128) 2^-24 (|q| + |dq|) (max|d| + max|dd|)
 * by Cauchy-Schwarz; |dq| is measured per query, max|d| and max|dd| over the index rows by
 * vr_index_add (~3.4e-3 for unit vectors at dim 2304; the worst case over all data would be
 * 2^-7 + 2^-16 + ... = 8.1e-3).  eps_rel >= 0: the caller's model eps_rel * |q| * max|d| instead;
 * eps_rel < 0: certification off (the bf16 top-(k+6) re-scored, as in rounds 1-2: tolerance-exact). */
int vr_index_set_search_eps(vr_index_t ix, float eps_rel);
/* out4 = {max|d|, max|d - bf16(d)| over the rows added so far, the accumulation term
 * (2 dim + 128) 2^-24, the worst-case relative bound 2^-7 + 2^-16 + accumulation}. */
int vr_index_error_model(vr_index_t ix, float* out4);
/* Queries counted since the last reset: out6[0..5] = {certified at once, certified after extended
 * re-scoring, flagged (redone by the band pass), searched with certification off, of the second
 * group: those whose candidates had to be gathered a second time, of the flagged: those whose band
 * exceeded 8192 rows — redone by the exact fp32 pass, or (the first such queries of an index: the exact
 * pass is only launched behind an index that has shown one) walked by one workgroup}. */
int vr_index_search_stats(vr_index_t ix, int64_t* out6, int32_t reset);
/* How a search of `nq` queries (k <= 26) over the rows added so far would be laid out: out5 = {list chunks per query,
 * of them the chunks that belong to the threshold pre-pass (0, or 8 when the pre-pass OWNS its sample: its 16 sampled 256-row
 * tiles are scored once, their survivors kept in lists of their own, and the sweep skips them), workgroup chunks of the
 * sweep, index tiles (256 rows) per workgroup chunk, whether the exact fp32 pass is launched behind the search (1 once the
 * index has met a band beyond 8192 rows; vr_index_reset clears it)}.  Introspection only (tests, bench.py's `search.plan`). */
int vr_index_search_plan(vr_index_t ix, int32_t nq, int32_t* out5);
/* Per-stage HIP-event times of vr_index_search (k <= 26), summed over calls since enabling:
 * ms5 = {query conversion, threshold pre-pass, sweep, merge + re-scoring, band + exact pass}.
 * While enabled every call ends with an event synchronisation. */
int vr_index_set_search_profile(vr_index_t ix, int32_t enable);
int vr_index_get_search_profile(vr_index_t ix, double* ms5, int64_t* calls);
/* The same search with the result packed for the multi-GPU exchange: out_keys [nq][k] uint64,
 * key = orderable(score) << 32 | ~(row id + id_offset) — larger key = better (higher score,
 * then lower global id); 0 = no entry.  One 8-byte word per result is what the ranks
 * all-gather (dense_retriever.py:48-69 exchanges through the file system instead).
 * id_offset + rows must stay below 2^32 - 1. */
int vr_index_search_keys(vr_index_t ix, const float* queries, int32_t nq, int32_t k, int64_t id_offset,
                         uint64_t* out_keys, int32_t on_device, void* stream);
/* ---- document-level search: the best row per group of adjacent rows, the k best groups ---- */
/* Partition the rows present into n_groups groups (documents) of ADJACENT rows: group g holds rows
 * group_offsets[g] .. group_offsets[g + 1] - 1.  group_offsets (host, n_groups + 1 entries) starts at 0, is
 * strictly increasing and ends at the row count; a NULL pointer, n_groups < 1 or offsets that break one
 * of these rules: VR_ERR_INVALID, and the index keeps the grouping it had.  A later vr_index_add that
 * appends rows, or vr_index_reset, drops the grouping. */
int vr_index_set_groups(vr_index_t ix, const int64_t* group_offsets, int64_t n_groups);
/* For every query the k best groups.  The score of a group, E_g, is the largest fp32 dot product of the
 * query with a row of the group — the score vr_index_search returns for that row — and the group's best
 * row is the row that attains it, the lowest row id among equal scores.  Results: larger E_g first, the
 * lower best row id first among equal E_g.
 *   out_scores [nq][k] float32 = E_g;  out_ids [nq][k] int64 = best row;  out_groups [nq][k] int64 = g
 * (all host or all device per `on_device`); with fewer than k groups the tail is (-inf, -1, -1).
 * The ids are the fp32 ranking's, as for vr_index_search, and by the same argument applied to groups: the
 * bf16 MFMA scores b_i of all rows (|b_i - e_i| <= eps, the error model of vr_index_set_search_eps) give
 * group maxima B_g with |B_g - E_g| <= eps; the k + 24 groups of largest B_g are candidates; in a
 * candidate every row with b_i >= B_g - 2 eps (only such a row can attain E_g) is re-scored in fp32; the
 * result is certified if the best B_g outside the candidates lies below E_(k) - eps, else every group with
 * B_g >= E_(k) - eps is re-scored (up to 1024), else the query is redone from exact fp32 scores of all
 * rows.  With certification off (eps_rel < 0) the first candidate set is re-scored (rows within the
 * default error model of their group's B_g) and returned with no guarantee.
 * k = 1..1000 and the dim limits of the deep path of vr_index_search: anything else is VR_ERR_INVALID
 * before any launch; no grouping set for the rows present: VR_ERR_STATE.  Grouped searches are not counted
 * by vr_index_search_stats and leave every state the other searches read alone. */
int vr_index_search_groups(vr_index_t ix, const float* queries, int32_t nq, int32_t k,
                           float* out_scores, int64_t* out_ids, int64_t* out_groups,
                           int32_t on_device, void* stream);
/* Grouped-search queries since the last reset: out3 = {certified from the first candidate set,
 * certified after widening it, redone exactly}. */
int vr_index_group_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- filtered search: the top k among the rows a query's filter allows ---- */
/* Set n_filters row filters over the rows present.  bits (host or device per `on_device`) is [n_filters][words] uint32,
 * words = ceil(rows / 32): filter f allows row r iff bit r & 31 of word r >> 5 of filter f is set.  Bits at or beyond
 * the row count are ignored (cleared in the library's copy).  The library copies the filters into memory it owns and
 * counts every filter's allowed rows once, here.  NULL, n_filters < 1 or an empty index: VR_ERR_INVALID, and the index
 * keeps the filters it had.  A later vr_index_add that appends rows, or vr_index_reset, drops the filters.  Filters and
 * groups are independent. */
int vr_index_set_filters(vr_index_t ix, const uint32_t* bits, int32_t n_filters, int32_t on_device, void* stream);
/* For every query the k ALLOWED rows of largest fp32 dot product, larger score first and the lower row id first among
 * equal scores: what vr_index_search returns on an index that holds only the allowed rows, with the original row ids.
 * filter_of_query [nq] int32 (host or device as `queries`): the filter of query q, -1 = no filter (all rows).
 *   out_scores [nq][k] float32;  out_ids [nq][k] int64;  fewer than k allowed rows (none included): the tail is (-inf, -1).
 * The allowed rows are a sub-index for which the error model of vr_index_set_search_eps holds as it does for the whole
 * index (the index-wide max |d| and max |d - bf16(d)| can only be looser), so the certification of the deep path
 * applies with na = the filter's allowed rows in the place of the row count: the bf16 MFMA scores of all rows are
 * computed, the disallowed ones set to -inf, the min(na, k + 24) best are re-scored in fp32; the result is certified if
 * every allowed row was re-scored or the best bf16 score outside the candidates lies below E_(k) - eps, else every
 * allowed row with a bf16 score >= E_(k) - eps is re-scored (up to 1024), else the query is redone from exact fp32 scores
 * of all rows, masked the same way.  With certification off (eps_rel < 0) the first candidate set is re-scored and
 * returned with no guarantee, and nothing is counted.
 * k = 1..1000 and the dim limits of the deep path of vr_index_search; a HOST filter_of_query entry outside
 * [-1, n_filters): VR_ERR_INVALID before any launch.  On the device such an entry cannot be seen before the launch: it
 * allows nothing (an all-empty result row) and nothing outside the filter store is read.  No filters set for the rows
 * present: VR_ERR_STATE.  Filtered searches are not counted by vr_index_search_stats or vr_index_group_search_stats and
 * leave every state the other searches read alone. */
int vr_index_search_filtered(vr_index_t ix, const float* queries, int32_t nq, int32_t k,
                             const int32_t* filter_of_query,
                             float* out_scores, int64_t* out_ids, int32_t on_device, void* stream);
/* Filtered-search queries since the last reset: out3 = {certified from the first candidate set (a query with no
 * allowed row included), certified after widening it, redone exactly}. */
int vr_index_filter_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- diversified search: k rows picked by maximal marginal relevance (MMR) from a pool of the best rows ---- */
/* For every query, k rows that are relevant AND unlike each other — what a caller wants who hands the k pages to a
 * generator, where near-duplicate pages (one slide template across many decks) spend its context on one page.
 *   1. The pool is the first `pool` rows of the fp32 ranking: exactly what vr_index_search(k = pool) returns, or with
 *      filter_of_query (as for vr_index_search_filtered; NULL = no filter for any query) exactly what
 *      vr_index_search_filtered(k = pool) returns — produced by those code paths as they stand, and so certified as they
 *      are.  The (-inf, -1) tail entries are not members; P' = the number of members.  Pool position = rank in that
 *      result: higher fp32 score first, lower row id among equal scores.
 *   2. Pick 0 is pool position 0.
 *   3. Pick t >= 1 is the unselected member i that maximises
 *          v_i = lambda r_i - (1 - lambda) max_{j selected} <d_i, d_j>
 *      with r_i the member's fp32 score as the search returned it and <d_i, d_j> the fp32 dot product of the index's fp32
 *      rows (unit rows: their cosine, the measure the index ranks by), computed like every score the library returns and
 *      never in bf16.  Among equal v the lower pool position wins; bit-identical rows have bit-identical v.
 *   4. out_ids [nq][k] int64 = the picks in pick order, out_scores [nq][k] float32 = their r_i — the relevance, not
 *      monotone in general (all host or all device per `on_device`).  With P' < k the tail is (-inf, -1).
 * lambda = 1 gives the first k of the pool; lambda = 0 only avoids what was picked.
 * 1 <= k <= pool <= 1000, 0 <= lambda <= 1 (NaN refused) and the dim limits of the deep path of vr_index_search: anything
 * else is VR_ERR_INVALID before any launch, the outputs untouched.  A HOST filter_of_query entry outside [-1, n_filters):
 * VR_ERR_INVALID likewise; filter_of_query given while no filters are set for the rows present: VR_ERR_STATE.
 * The pool stage IS the plain or the filtered search and counts in that search's statistics; the MMR stage keeps no
 * counters and leaves every state the other searches read alone.  Work: (k - 1) P' fp32 row dots per query. */
int vr_index_search_diverse(vr_index_t ix, const float* queries, int32_t nq, int32_t k, int32_t pool, float lambda,
                            const int32_t* filter_of_query /* NULL: no filter for any query */,
                            float* out_scores, int64_t* out_ids, int32_t on_device, void* stream);
/* ---- range search: every row at or above a score threshold, exact ---- */
/* For query q the result is the SET of rows i with e_i >= thresholds[q] — with filter_of_query (as for
 * vr_index_search_filtered; NULL = no filter for any query) only rows the query's filter allows.  e_i is the fp32 dot product
 * of the fp32 rows, computed by the library's one re-scoring dot product: a row returned both here and by vr_index_search
 * for the same query carries the same score bits, and the comparison with the threshold is an fp32 compare of that value.
 * The size of the answer is the answer: nothing is cut at a k.
 *   Layout: CSR.  out_lims [nq + 1] int64: entries out_lims[q] .. out_lims[q + 1] - 1 are query q's, out_lims[0] = 0,
 * out_lims[nq] = *total; inside a query the entries are in ASCENDING ROW ID (deterministic, no sort).  queries [nq][dim]
 * float32, thresholds [nq] float32, filter_of_query [nq] int32 and out_lims are all host or all device per `on_device`;
 * `total` is always a host pointer.
 *   Ownership: scores and ids are written to device buffers the library owns; they stay valid until the next range search,
 * vr_index_reset or vr_index_destroy.  vr_index_range_results copies the first n entries (n <= the last total) to the
 * caller's arrays (out_scores [n] float32, out_ids [n] int64, host or device per `on_device`); n larger than the last total,
 * or no range search since the last reset: VR_ERR_STATE.
 *   Exactness: with b_i the bf16 MFMA score and |b_i - e_i| <= eps (the error model of vr_index_set_search_eps) every row
 * with e_i >= t has b_i >= t - eps.  The bf16 scores of all rows are computed, disallowed ones set to -inf, exactly the rows
 * with b_i >= t - eps (the bound lowered by one ulp) are re-scored in fp32 and those with e_i >= t kept: the fp32 answer, with
 * no candidate margin, no widening and no flagged query; a query costs what its band holds.  A range search always uses a
 * valid model: with certification off (eps_rel < 0) the default data-dependent bound, so the result is exact in every
 * setting.  Columns at or past the row count are never looked at.
 *   Checks, all before any launch, the outputs and the previous result untouched: NULL pointers, nq < 1, max_total < 1 or a
 * dim outside the limits of the deep path of vr_index_search: VR_ERR_INVALID; a HOST threshold that is NaN or +-inf:
 * VR_ERR_INVALID (a caller that wants every row passes a finite threshold below every score); a HOST filter_of_query entry
 * outside [-1, n_filters): VR_ERR_INVALID; filter_of_query given while no filters are set for the rows present:
 * VR_ERR_STATE.  On the device such values cannot be seen before the launch: a non-finite threshold or an out-of-range
 * filter yields an empty segment, and nothing outside the library's buffers is read.  An empty index: all-zero lims and
 * total 0 without a launch.
 *   Capacity: if the running total would exceed max_total the call returns VR_ERR_CAPACITY (the text names the first block of
 * 256 queries that overran); the previous result is gone — vr_index_range_results then returns VR_ERR_STATE — and nothing
 * else of the index changes but the range search's own counters, which have counted the blocks that ran.
 *   The call synchronises the stream, because the sizes of its result are host values: once per block of 256 queries and
 * once at the end.  It leaves every state the other searches read alone and counts in none of their statistics.
 * Not offered: sorted output (sort a segment by score on the caller's side: the Python wrapper does), corpus-sharded ranks
 * (a range result over shards is the union of the shards' results).  An exact count without the rows: vr_index_count_range
 * below; documents in the place of rows: vr_index_search_groups_range. */
int vr_index_search_range(vr_index_t ix, const float* queries, int32_t nq,
                          const float* thresholds,          /* [nq] */
                          const int32_t* filter_of_query,   /* NULL: no filter for any query */
                          int64_t max_total,
                          int64_t* out_lims,                /* [nq + 1] */
                          int64_t* total,                   /* host */
                          int32_t on_device, void* stream);
int vr_index_range_results(vr_index_t ix, float* out_scores, int64_t* out_ids, int64_t n,
                           int32_t on_device, void* stream);
/* Range searches since the last reset: out3 = {queries, candidate rows re-scored in fp32, rows returned} — 64-bit counters
 * in device memory. */
int vr_index_range_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- rank search: the exact rank and score of named rows, exact counts against thresholds ---- */
/* vr_index_rank_rows: for query q and target row i, out_scores = e_i, the fp32 score of the library's one re-scoring dot product
 * (the bits vr_index_search returns for that (query, row)), and out_ranks = the number of rows j — allowed by the query's filter
 * if filter_of_query is given — whose key is greater than the target's: score descending, then lower id first.  A target of
 * rank r is therefore at position r of vr_index_search for every k > r (of vr_index_search_filtered under the filter), rows
 * with identical bits get consecutive ranks in id order, and duplicate targets are allowed.  The rank is defined whether or
 * not the filter allows the target itself: it is then the position the row WOULD take among the allowed rows.
 *   vr_index_count_range: for query q and threshold t the number of (allowed) rows with e >= t, or with e > t when strict:
 * the non-strict count is exactly the size of vr_index_search_range's segment for the same threshold.  -0.0 counts as +0.0.
 *   Layout: targets / thresholds in CSR form: query q's are entries lims[q] .. lims[q + 1] - 1.  lims [nq + 1] int64, ids int64
 * and thresholds float32 are always HOST arrays (as the ids of vr_index_remove are); queries [nq][dim] float32, filter_of_query
 * [nq] int32 and the outputs (lims[nq] entries each) are all host or all device per `on_device`.
 *   Exactness: as for the range search.  With |b_j - e_j| <= eps a row with b_j > t + eps is certainly ahead of a bar t (t = e_i
 * for a rank) and one with b_j < t - eps certainly behind it; exactly the rows of the band between are re-scored in fp32 and
 * compared — by key for a rank, by the fp32 compare for a count.  No candidate margin, no widening, no flagged query; a pair
 * costs what its band holds.  With certification off the default error model defines the band.  Counts are additive over
 * shards of a corpus, which no top-k result is.
 *   Checks, all before any launch and with the outputs untouched: NULL pointers, nq < 0, lims[0] != 0 or decreasing lims, an
 * id outside [0, rows), a threshold that is NaN or +-inf, an unsupported dim (as vr_index_search_range): VR_ERR_INVALID; the
 * filter checks are those of vr_index_search_range (on the device an out-of-range filter index gives a count of 0).  Zero
 * pairs: VR_OK, nothing is launched.  An empty index: vr_index_count_range writes zeros, vr_index_rank_rows with pairs is
 * VR_ERR_INVALID (no id is in range).  Nothing is stored: a later vr_index_remove / update / add has nothing to invalidate.
 * A host caller's call synchronises the stream.  Not offered: corpus-sharded ranks inside the library (add per-shard counts),
 * ranks under MMR.  Ranks of groups: vr_index_rank_groups below. */
int vr_index_rank_rows(vr_index_t ix, const float* queries, int32_t nq,
                       const int64_t* lims,              /* host [nq + 1] */
                       const int64_t* ids,               /* host [lims[nq]] */
                       const int32_t* filter_of_query,   /* NULL: no filter for any query */
                       float* out_scores, int64_t* out_ranks,   /* [lims[nq]] */
                       int32_t on_device, void* stream);
int vr_index_count_range(vr_index_t ix, const float* queries, int32_t nq,
                         const int64_t* lims,            /* host [nq + 1] */
                         const float* thresholds,        /* host [lims[nq]] */
                         int32_t strict,                 /* 0: e >= t, 1: e > t */
                         const int32_t* filter_of_query, /* NULL: no filter for any query */
                         int64_t* out_counts,            /* [lims[nq]] */
                         int32_t on_device, void* stream);
/* Rank searches since the last reset: out3 = {pairs, band candidates re-scored in fp32, rows counted} — 64-bit counters in
 * device memory. */
int vr_index_rank_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- windowed search: the rows at ranks [offset, offset + k) of a query's ranking, any offset ---- */
/* vr_index_search_window: entry j of query q is the row at rank offsets[q] + j of q's fp32 ranking — fp32 score descending, then
 * lower id first, over the rows q's filter allows (filter_of_query NULL or an entry of -1: all rows) — with e, the fp32 score of
 * the library's one re-scoring dot product (the bits every other search returns for that (query, row)).  Slots at or past the
 * number of allowed rows are (-inf, -1); an offset at or past that number gives a row of them.  In every setting of
 * vr_index_set_search_eps the result equals entries offsets[q] .. offsets[q] + k - 1 of vr_index_search / _search_filtered for
 * k' = offsets[q] + k wherever that search reaches, the same entries of the sorted segment of vr_index_search_range for a
 * threshold below every score, and vr_index_rank_rows of the ids returned is offsets[q] + j: the inverse of the rank search.
 *   Layout: offsets [nq] int64 is always a HOST array (as the ids and lims of vr_index_rank_rows are), each >= 0, with no upper
 * limit; 1 <= k <= 1000 (page for more); queries [nq][dim] float32, filter_of_query [nq] int32 and the outputs [nq][k] are all
 * host or all device per `on_device`.
 *   Exactness: as for the range and the rank search.  With |b_j - e_j| <= eps the r-th largest bf16 score lies within eps of
 * the r-th largest fp32 score, so the window's rows have b within 2 eps of the bf16 scores at ranks offset + 1 and offset + k:
 * rows above that band are certainly ahead of the window, rows below it certainly behind; exactly the band is re-scored in
 * fp32 and ranked by key.  No candidate margin, no widening, no flagged query; a query costs what its band holds.  With
 * certification off the default error model defines the band.
 *   Checks, all before any launch and with the outputs untouched: NULL pointers with nq > 0, nq < 0, k outside 1..1000, a
 * negative offset, an unsupported dim (as vr_index_search_range): VR_ERR_INVALID; the filter checks are those of
 * vr_index_search_range (on the device an out-of-range filter index gives a row of tails).  nq == 0: VR_OK, nothing is
 * launched.  An empty index: tails, nothing is launched.  Nothing is stored: a later vr_index_remove / update / add has nothing
 * to invalidate.  A host caller's call synchronises the stream.  Not offered: corpus-sharded ranks inside the library (merge
 * per-shard pages on the host), windows under MMR, k > 1000 in one call, a k per query.  Windows of groups:
 * vr_index_search_groups_window below. */
int vr_index_search_window(vr_index_t ix, const float* queries, int32_t nq,
                           const int64_t* offsets,           /* host [nq] */
                           int32_t k,
                           const int32_t* filter_of_query,   /* NULL: no filter for any query */
                           float* out_scores, int64_t* out_ids,   /* [nq][k] */
                           int32_t on_device, void* stream);
/* Windowed searches since the last reset: out3 = {queries, band candidates re-scored in fp32, rows certainly ahead of their
 * window} — 64-bit counters in device memory. */
int vr_index_window_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- document window search: the groups at ranks [offset, offset + k) of a query's document ranking, under filters ---- */
/* vr_index_search_groups_window: the document-level search with a filter and a window.  For query q with filter f
 * (filter_of_query NULL or an entry of -1: every row) a group g (vr_index_set_groups) is PRESENT if f allows at least one of
 * its rows; its score is E_g = the largest e_i over its ALLOWED rows — e_i the library's one fp32 dot product, the bits
 * vr_index_search returns for that pair — and its best row the lowest allowed row id that attains E_g.  Present groups rank by
 * E_g descending, then lower best row first (groups are runs of adjacent rows: lower group first).  Entry j of query q is the
 * group at rank offsets[q] + j:
 *   out_scores [nq][k] float32 = E_g;  out_ids [nq][k] int64 = best row;  out_groups [nq][k] int64 = g.
 * Slots at or past the number of present groups are (-inf, -1, -1); an offset at or past that number gives a row of them.
 * With offset 0 and no filter the result equals vr_index_search_groups bit for bit; with
 * groups of one row it equals vr_index_search_window with out_groups == out_ids.
 *   Layout: offsets [nq] int64 is always a HOST array, each >= 0, with no upper limit; 1 <= k <= 1000 (page for more); queries
 * [nq][dim] float32, filter_of_query [nq] int32 and the outputs [nq][k] are all host or all device per `on_device`.
 *   Exactness: the windowed search's argument composed with the grouped search's.  With |b_i - e_i| <= eps over the allowed
 * rows, the masked group maximum B_g lies within eps of E_g (max is 1-Lipschitz) and the r-th largest B within eps of the r-th
 * largest E (so are order statistics); groups whose B lies more than 2 eps above the B at rank offset + 1 are certainly ahead of
 * the window, groups more than 2 eps below the B at rank offset + k certainly behind it; inside a group of the band between,
 * exactly the rows with b_i >= B_g - 2 eps — only such a row can attain E_g — are re-scored in fp32, and the groups are ranked
 * by key.  Every edge is rounded outward by one ulp.  No candidate margin, no widening, no flagged query; a query costs what
 * its band holds; with certification off the default error model defines the band, so the result is exact in every setting of
 * vr_index_set_search_eps.
 *   Checks, all before any launch and with the outputs untouched: NULL pointers with nq > 0, nq < 0, k outside 1..1000, a
 * negative offset, an unsupported dim (as vr_index_search_range), a HOST filter_of_query entry outside [-1, n_filters):
 * VR_ERR_INVALID; no grouping set for the rows present, or filter_of_query given while no filters are set for them:
 * VR_ERR_STATE.  On the device an out-of-range filter index allows nothing: a row of tails.  nq == 0: VR_OK, nothing is
 * launched.  Nothing is stored between calls.  A host caller's call synchronises the stream.  The call counts in no other
 * search's statistics and leaves every state the other searches read alone; vr_index_search_groups is untouched by it.
 * Ranks of named documents: vr_index_rank_groups below; every document above a threshold: vr_index_search_groups_range.
 * Not offered: documents under the fused search or MMR, corpus-sharded ranks (merge per-shard pages on the host), k > 1000 in one call, a k per query. */
int vr_index_search_groups_window(vr_index_t ix, const float* queries, int32_t nq,
                                  const int64_t* offsets,           /* host [nq] */
                                  int32_t k,
                                  const int32_t* filter_of_query,   /* NULL: no filter for any query */
                                  float* out_scores, int64_t* out_ids, int64_t* out_groups,   /* [nq][k] */
                                  int32_t on_device, void* stream);
/* Document window searches since the last reset: out3 = {queries, band groups re-scored, fp32 row dot products} — 64-bit
 * counters in device memory. */
int vr_index_group_window_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- document rank search: the exact rank of named groups, exact counts of groups against thresholds, under filters ---- */
/* vr_index_rank_groups: WHERE a named document stands.  The semantics are those of vr_index_search_groups_window: for query q
 * with filter f (filter_of_query NULL or an entry of -1: every row) a group g (vr_index_set_groups) is PRESENT if f allows at
 * least one of its rows; its score is E_g = the largest e_i over its ALLOWED rows — e_i the library's one fp32 dot product, the
 * bits vr_index_search returns for that pair — its best row the lowest allowed row id that attains E_g; present groups rank by
 * E_g descending, then lower group first.  For a present target g
 *   out_scores = E_g;  out_rows = best row;  out_ranks = the number of present groups h whose key (E_h, h) is greater.
 * A group of rank r is therefore entry r - o of vr_index_search_groups_window for every offset o <= r < o + k, with the same
 * score bits and the same best row; groups with identical bits get consecutive ranks in group order; duplicate targets are
 * allowed.  A target the filter leaves no row of is NOT in the ranking: it gets (-inf, -1, -1).  This differs from
 * vr_index_rank_rows, where a forbidden row gets the position it WOULD take: a row has a score whether or not it is allowed, a
 * group's score is defined over its allowed rows, and an absent group has none.
 *   vr_index_count_groups_range: for query q and threshold t the number of present groups with E_g >= t, or with E_g > t when
 * strict.  -0.0 counts as +0.0, as in vr_index_count_range.
 *   Layout: targets / thresholds in CSR form: query q's are entries lims[q] .. lims[q + 1] - 1.  lims [nq + 1] int64, groups
 * int64 and thresholds float32 are always HOST arrays (as the ids of vr_index_rank_rows are); queries [nq][dim] float32,
 * filter_of_query [nq] int32 and the outputs (lims[nq] entries each) are all host or all device per `on_device`.
 *   Exactness: the rank search's argument composed with the grouped search's.  With |b_i - e_i| <= eps over the allowed rows
 * the masked group maximum B_h lies within eps of E_h (max is 1-Lipschitz): a group with B_h > t + eps is certainly ahead of a
 * bar t (t = E_g for a rank), one with B_h < t - eps certainly behind it or absent; inside a group of the band between exactly
 * the rows with b_i >= B_h - 2 eps — only such a row can attain E_h — are re-scored in fp32, and the group is compared by key
 * for a rank, by the fp32 compare for a count.  The target is found the same way and never counts itself.  Every edge is rounded
 * outward by one ulp.  No candidate margin, no widening, no flagged query; a pair costs what its band holds; with certification
 * off the default error model defines the band, so the result is exact in every setting of vr_index_set_search_eps.
 *   Checks, all before any launch and with the outputs untouched: NULL pointers, nq < 0, lims[0] != 0 or decreasing lims,
 * 2^31 pairs or more, an unsupported dim (as vr_index_search_range): VR_ERR_INVALID; no grouping set for the rows present
 * (vr_index_add / vr_index_remove drop it): VR_ERR_STATE; a group outside [0, n_groups), a threshold that is NaN or +-inf, a
 * HOST filter_of_query entry outside [-1, n_filters): VR_ERR_INVALID; filter_of_query given while no filters are set:
 * VR_ERR_STATE.  On the device an out-of-range filter index allows nothing: ranks (-inf, -1, -1), counts 0.  Zero pairs: VR_OK,
 * nothing is launched; a block of 256 queries without pairs is skipped.  Nothing is stored between calls.  A host caller's call
 * synchronises the stream.  The calls count in no other search's statistics and leave every state the other searches read
 * alone.  Not offered: document ranks under the fused search or MMR, corpus-sharded
 * ranks inside the library (add per-shard counts), several bars of one query per read of its group maxima. */
int vr_index_rank_groups(vr_index_t ix, const float* queries, int32_t nq,
                         const int64_t* lims,              /* host [nq + 1] */
                         const int64_t* groups,            /* host [lims[nq]] */
                         const int32_t* filter_of_query,   /* NULL: no filter for any query */
                         float* out_scores, int64_t* out_rows, int64_t* out_ranks,   /* [lims[nq]] */
                         int32_t on_device, void* stream);
int vr_index_count_groups_range(vr_index_t ix, const float* queries, int32_t nq,
                                const int64_t* lims,            /* host [nq + 1] */
                                const float* thresholds,        /* host [lims[nq]] */
                                int32_t strict,                 /* 0: E >= t, 1: E > t */
                                const int32_t* filter_of_query, /* NULL: no filter for any query */
                                int64_t* out_counts,            /* [lims[nq]] */
                                int32_t on_device, void* stream);
/* Document rank searches and counts since the last reset: out3 = {pairs, band groups re-scored (a rank's own target among
 * them), fp32 row dot products} — 64-bit counters in device memory. */
int vr_index_group_rank_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- document range search: every group at or above a score threshold, under filters, exact ---- */
/* vr_index_search_groups_range: WHICH documents reach a threshold.  The semantics are those of vr_index_search_groups_window and
 * vr_index_count_groups_range: for query q with filter f (filter_of_query NULL or an entry of -1: every row) a group g
 * (vr_index_set_groups) is PRESENT if f allows at least one of its rows; its score is E_g = the largest e_i over its ALLOWED rows
 * — e_i the library's one fp32 dot product, the bits vr_index_search returns for that pair — its best row the lowest allowed row
 * id that attains E_g.  The result of query q is the SET of present groups with E_g >= thresholds[q], an fp32 compare: -0.0 counts
 * as +0.0.  Its size is exactly vr_index_count_groups_range's non-strict count for the same threshold and filter, its entries
 * carry the score bits and best rows of vr_index_search_groups_window / vr_index_rank_groups.  Nothing is cut at a k.
 *   Layout: CSR, as vr_index_search_range's.  out_lims [nq + 1] int64: entries out_lims[q] .. out_lims[q + 1] - 1 are query q's,
 * out_lims[0] = 0, out_lims[nq] = *total; inside a query the entries are in ASCENDING GROUP (deterministic, no sort).  queries
 * [nq][dim] float32, thresholds [nq] float32, filter_of_query [nq] int32 and out_lims are all host or all device per `on_device`;
 * `total` is always a host pointer.
 *   Ownership: scores, best rows and groups are written to device buffers the library owns — the document range search's own,
 * not vr_index_search_range's: either result survives the other search.  They stay valid until the next document range search,
 * vr_index_reset, vr_index_add, vr_index_set_groups, vr_index_remove, vr_index_update or vr_index_destroy.
 * vr_index_group_range_results copies the first n entries (n <= the last total) to the caller's arrays (out_scores [n] float32,
 * out_rows [n] int64, out_groups [n] int64, host or device per `on_device`); n larger than the last total, or no stored result:
 * VR_ERR_STATE.
 *   Exactness: with |b_i - e_i| <= eps over the allowed rows (the error model of vr_index_set_search_eps) the masked group
 * maximum B_g of the bf16 MFMA scores lies within eps of E_g, because max is 1-Lipschitz: E_g >= t implies B_g >= t - eps.  Inside
 * such a group only a row with b_i >= B_g - 2 eps can attain E_g.  Exactly those rows of exactly those groups are re-scored in
 * fp32 and the groups with E_g >= t kept; every edge is rounded outward by one ulp.  No candidate margin, no widening, no flagged
 * query; a query costs what its band holds; with certification off the default error model defines the band, so the result is
 * exact in every setting of vr_index_set_search_eps.
 *   Checks, all before any launch, the outputs and the previous result untouched: NULL pointers, nq < 1, max_total < 1, an
 * unsupported dim (as vr_index_search_range), a HOST threshold that is NaN or +-inf, a HOST filter_of_query entry outside
 * [-1, n_filters): VR_ERR_INVALID; no grouping set for the rows present (vr_index_add / vr_index_remove drop it), or
 * filter_of_query given while no filters are set: VR_ERR_STATE.  On the device a non-finite threshold or an out-of-range filter
 * index yields an empty segment, and nothing is read for that query.  An empty index: all-zero lims and total 0 without a launch.
 *   Capacity: if the running total would exceed max_total the call returns VR_ERR_CAPACITY (the text names the first block of
 * 256 queries that overran); the previous result is gone and nothing else of the index changes but this search's own counters,
 * which have counted the blocks that ran.
 *   The call synchronises the stream, because the sizes of its result are host values: once per block of 256 queries and once
 * at the end.  It counts in no other search's statistics and leaves every state the other searches read alone.
 * Not offered: sorted output (the Python wrapper sorts a segment by score, then group), corpus-sharded ranks (a result over
 * shards of whole documents is the union of the shards' results), documents under the fused search or MMR. */
int vr_index_search_groups_range(vr_index_t ix, const float* queries, int32_t nq,
                                 const float* thresholds,          /* [nq] */
                                 const int32_t* filter_of_query,   /* NULL: no filter for any query */
                                 int64_t max_total,
                                 int64_t* out_lims,                /* [nq + 1] */
                                 int64_t* total,                   /* host */
                                 int32_t on_device, void* stream);
int vr_index_group_range_results(vr_index_t ix, float* out_scores, int64_t* out_rows, int64_t* out_groups, int64_t n,
                                 int32_t on_device, void* stream);
/* Document range searches since the last reset: out3 = {queries, band groups re-scored, fp32 row dot products} — 64-bit counters
 * in device memory. */
int vr_index_group_range_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- fused search: the top-k rows by max or min over a group of sub-queries ---- */
/* vr_index_search_multi: one question, several vectors (reformulations, the last turns of a chat, the sub-questions of a
 * multi-hop question).  The sub-queries are a flat [n_sub][dim] float32 array; group g holds sub-queries lims[g] ..
 * lims[g + 1] - 1 (CSR).  For group g, its sub-queries j and row i the FUSED score is
 *     E_g(i) = max_j e_j(i)   (fuse = 0, "any-of": a row scores as its best sub-query does)
 *     E_g(i) = min_j e_j(i)   (fuse = 1, "all-of": a row scores as its worst sub-query does)
 * with e_j(i) the library's one fp32 dot product (the bits vr_index_search returns for that pair); max and min are taken in the
 * ranking's own order of floats, in which -0.0 < +0.0.  The result of group g is the k rows of largest E_g among the rows the
 * group's filter allows (filter_of_group NULL or an entry of -1: all rows), score descending, then lower id first; slots past
 * the allowed rows hold (-inf, -1, -1).  out_which names, for every returned row, the lowest in-group index j (0-based inside
 * the group) whose e_j(i) has exactly the fused score's bits.  A group of one equals vr_index_search / _search_filtered bit for
 * bit, with which == 0.
 *   Layout: lims [n_groups + 1] int64 is always a HOST array (as the offsets of vr_index_search_window are); queries, filter_of_group
 * [n_groups] int32 and the outputs [n_groups][k] are all host or all device per `on_device`.
 *   Exactness: with |b_j - e_j| <= eps_j for the bf16 MFMA scores b_j, the fused bf16 value B_g = max_j b_j (or min) lies within
 * eps_g = max_j eps_j of E_g for every row, because max and min over a fixed set are 1-Lipschitz in the sup norm.  From there it
 * is the windowed search's argument at offset 0: a row whose B_g lies more than 2 eps_g below the min(k, allowed)-th largest B_g
 * is certainly behind the whole result; every other row is re-scored in fp32 against every sub-query of the group and ranked by
 * key.  No candidate margin, no widening, no flagged group; the result is exact in every setting of vr_index_set_search_eps
 * (with certification off the default error model defines the band).
 *   Checks, all before any launch and with the outputs untouched: NULL pointers with n_groups > 0, n_groups < 0, n_sub < 0,
 * k outside 1..1000, fuse outside {0, 1}, an unsupported dim (as vr_index_search_window), lims[0] != 0, a decreasing lims, an
 * empty group, a group of more than 256 sub-queries, lims[n_groups] != n_sub: VR_ERR_INVALID; the filter checks are those of
 * vr_index_search_window (on the device an out-of-range filter index gives a row of tails).  n_groups == 0 (then n_sub == 0):
 * VR_OK, nothing is launched.  An empty index: tails, nothing is launched.  Nothing is stored between calls.  A host caller's
 * call synchronises the stream.  Not offered: weighted-sum fusion (linear: sum the queries into one), a window offset, MMR over
 * a fused pool, corpus-sharded ranks, groups of more than 256 sub-queries; groups of documents are vr_index_search_multi_groups
 * below.  Reciprocal-rank fusion, which fuses positions and not scores, is vr_index_search_rrf below. */
int vr_index_search_multi(vr_index_t ix, const float* queries, int32_t n_sub,
                          const int64_t* lims,              /* host [n_groups + 1] */
                          int32_t n_groups, int32_t k,
                          int32_t fuse,                     /* 0: max, 1: min */
                          const int32_t* filter_of_group,   /* NULL: no filter for any group */
                          float* out_scores, int64_t* out_ids, int32_t* out_which,   /* [n_groups][k] */
                          int32_t on_device, void* stream);
/* Fused searches since the last reset: out3 = {groups, band columns re-scored in fp32, fp32 row dot products (columns x group
 * size)} — 64-bit counters in device memory. */
int vr_index_multi_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- fused document search: the top-k documents by max or min over a question's sub-queries, with the evidence ---- */
/* vr_index_search_multi_groups: vr_index_search_multi with DOCUMENTS (the groups of adjacent rows of vr_index_set_groups) in the
 * place of rows.  A multi-hop question decomposes into sub-questions that different pages of one document answer; the document
 * wanted is the one whose best page per sub-question is good for every sub-question.  A question is a group of 1..256 sub-queries,
 * given through lims exactly as vr_index_search_multi takes it.  For question g with filter f (-1 or none: every row),
 * sub-queries j = 0 .. m - 1 and document D:
 *     D is PRESENT if f allows at least one of its pages;
 *     E_j(D)  = max e_j(i) over the ALLOWED pages i of D, row_j(D) the lowest allowed row attaining it;
 *     F(D)    = max_j E_j(D) (fuse = 0, "any-of")  or  min_j E_j(D) (fuse = 1, "all-of");
 *     which(D) = the lowest j whose E_j(D) has exactly F(D)'s bits, best_row(D) = row_which(D)
 * with e_j(i) the library's one fp32 dot product (the bits vr_index_search returns for that pair) and every max and min taken in
 * the ranking's order of floats (-0.0 < +0.0).  Present documents rank by F descending, then lower document first: out_scores /
 * out_rows / out_docs / out_which [n_groups][k] hold (F, best_row, D, which), slots at or past the number of present documents
 * (-inf, -1, -1, -1).  The EVIDENCE (out_ev_scores / out_ev_rows, both NULL or both set; one of each: VR_ERR_INVALID) is what
 * goes to a generator: flat [n_sub * k] arrays, question g's block starts at k * lims[g] and reads as [k][m_g] — slot-major,
 * then sub-query — holding (E_j(D), row_j(D)) of the slot's document, (-inf, -1) in a tail slot.
 *   Layout: lims is a HOST array; queries, filter_of_group [n_groups] int32 and every output are all host or all device per
 * `on_device`.
 *   Exactness: |b_j(i) - e_j(i)| <= eps_j for the bf16 MFMA scores; the masked document maximum B_j(D) lies within eps_j of
 * E_j(D), the fused value BF(D) within eps_g = max_j eps_j of F(D), the r-th largest BF within eps_g of the r-th largest F.  With
 * v_z the min(k, present)-th largest BF, a document with BF < v_z - 2 eps_g is strictly behind the whole result; every other
 * document is re-scored: per sub-query every page with b_j(i) >= B_j(D) - 2 eps_j — only such a page can attain E_j(D) — gets
 * one fp32 dot.  No candidate margin, no widening, no flagged question; exact in every setting of vr_index_set_search_eps (with
 * certification off the default error model defines eps).
 *   Checks: every check of vr_index_search_multi, with the same codes, before any launch; no grouping set, or a filter named
 * while none is set: VR_ERR_STATE.  Errors leave every output untouched.  n_groups == 0 launches nothing; an empty index
 * returns tails; a device filter id out of range allows nothing.  Nothing is stored, and no other search's state or counters
 * are touched.  A host caller's call synchronises the stream.  Not offered: a window offset, documents under MMR,
 * corpus-sharded ranks, questions of more than 256 sub-queries. */
int vr_index_search_multi_groups(vr_index_t ix, const float* queries, int32_t n_sub,
                                 const int64_t* lims,              /* host [n_groups + 1] */
                                 int32_t n_groups, int32_t k,
                                 int32_t fuse,                     /* 0: max, 1: min */
                                 const int32_t* filter_of_group,   /* NULL: no filter for any question */
                                 float* out_scores, int64_t* out_rows, int64_t* out_docs, int32_t* out_which,   /* [n_groups][k] */
                                 float* out_ev_scores, int64_t* out_ev_rows,   /* NULL, or [n_sub * k] */
                                 int32_t on_device, void* stream);
/* Fused document searches since the last reset: out3 = {questions, band documents re-scored, fp32 page dot products} — 64-bit
 * counters in device memory. */
int vr_index_multi_group_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- rank-fusion search: the top-k of reciprocal-rank fusion (RRF) over the lists of a group's sub-queries ---- */
/* RRF fuses POSITIONS, not scores: it needs no comparable score scales, so a paraphrase with a flat score profile and one with a
 * peaked profile count the same, and lists under different filters, of pages and of documents, or from different indexes can be
 * fused.  Definition (normative; a numpy statement of it reproduces every bit): group g has lists L_0 .. L_{m-1} of `depth`
 * slots each; slot r of list j holds an id >= 0, or -1 for an empty slot.  For an id i
 *     F(i)    = fp32( sum over the entries (j, r) with L_j[r] == i of  (double)w_j / ((double)c + (double)(r + 1)) )
 *     hits(i) = the number of such entries
 * — an fp64 sum that starts at 0.0 and runs in ascending (j, r), every term that ONE division, rounded to fp32 once; c a float32
 * (60 is customary), w_j a float32 weight per list (weights NULL: every weight 1).  A duplicate id inside one list counts at
 * both positions.  The result is the k ids of largest F in the ranking's own order of floats, then lower id first;
 * slots past the distinct ids hold (-inf, -1, 0).  A row below position `depth` of a list contributes nothing.
 *   vr_rrf_fuse fuses lists from anywhere: ids [n_lists][depth] int64 and the three outputs [n_groups][k] are all host or all
 * device per `on_device`; lims [n_groups + 1] int64 (group g = lists lims[g] .. lims[g + 1] - 1) and weights [n_lists] are always
 * HOST arrays.  Host ids must lie in [-1, 2^31 - 2]; a device id outside [0, 2^31 - 2] is an empty slot, as -1 is.  The call
 * synchronises the stream.
 *   vr_index_search_rrf runs the lists itself: list j is what vr_index_search(k = depth) returns for sub-query j; with
 * filter_of_group (one entry per group, expanded to its sub-queries as by vr_index_search_multi; -1: no filter) what
 * vr_index_search_filtered(k = depth) returns; with by_groups != 0 the GROUPS vr_index_search_groups_window(offset 0,
 * k = depth) returns under the same filters, and the ids are then documents.  The lists are produced by those code paths as they
 * stand, into buffers the library owns (as the pool of vr_index_search_diverse is), and are therefore exact in every setting
 * of vr_index_set_search_eps; they count in that search's own statistics.  queries [n_sub][dim], filter_of_group
 * [n_groups] int32 and the outputs are all host or all device per `on_device`; lims and weights [n_sub] are HOST arrays.
 *   One launch of one kernel (one workgroup per group, none waits for another) holds the whole definition for both calls.
 *   Checks, all before any launch and with the outputs untouched: NULL pointers with n_groups > 0, negative counts, k outside
 * 1..1000, depth outside 1..1000, lims[0] != 0, a decreasing lims, an empty group, a group of more than 256 lists, a group with
 * m * depth above the value of vr_rrf_max_entries (16384), lims[n_groups] != the number of lists, c not finite or negative, a
 * weight not finite, a host id out of range: VR_ERR_INVALID; by_groups without a grouping, or filter_of_group while no
 * filters are set for the rows present: VR_ERR_STATE; a HOST filter_of_group entry outside [-1, n_filters): VR_ERR_INVALID.
 * n_groups == 0 (then no lists): VR_OK, nothing is launched.  An empty index: tails, nothing is launched.  Nothing is stored
 * between calls, and no other search's state or counters change beyond the statistics of the search that made the lists.
 * Not offered: RRF over full rankings, a window offset or MMR over a fused list, corpus-sharded ranks (merge every
 * sub-query's per-shard lists into its global list first: retriever.retrieve_rrf does), groups of more than 256 lists, the
 * best rows of fused documents. */
int vr_rrf_fuse(int device_id, const int64_t* ids, int32_t n_lists, int32_t depth,
                const int64_t* lims,                /* host [n_groups + 1] */
                int32_t n_groups, int32_t k, float c,
                const float* weights,               /* host [n_lists], NULL: every weight 1 */
                float* out_scores, int64_t* out_ids, int32_t* out_hits,      /* [n_groups][k] */
                int32_t on_device, void* stream);
/* The largest m * depth of one group. */
int vr_rrf_max_entries(void);
int vr_index_search_rrf(vr_index_t ix, const float* queries, int32_t n_sub,
                        const int64_t* lims,              /* host [n_groups + 1] */
                        int32_t n_groups, int32_t k, int32_t depth, float c,
                        const float* weights,             /* host [n_sub], NULL: every weight 1 */
                        const int32_t* filter_of_group,   /* NULL: no filter for any group */
                        int32_t by_groups,                /* != 0: fuse documents (vr_index_set_groups) */
                        float* out_scores, int64_t* out_ids, int32_t* out_hits,    /* [n_groups][k] */
                        int32_t on_device, void* stream);
/* Rank-fusion searches since the last reset: out3 = {groups, non-empty list entries, distinct ids} — 64-bit counters in device
 * memory. */
int vr_index_rrf_search_stats(vr_index_t ix, int64_t* out3, int32_t reset);
/* ---- editing in place: remove rows, overwrite rows, read rows back ---- */
/* After any of the calls below every search behaves exactly — score bits, ids, groups, lims — as on an index freshly built
 * (vr_index_create, vr_index_add, vr_index_set_filters / vr_index_set_groups) from the rows that remain.  Ids are positions, as
 * everywhere in this ABI.  `ids` is always a HOST array: the list is small, and everything is checked before anything changes.
 *   Checks, all before any launch and with the index unchanged: a NULL ix, NULL ids with n > 0, n < 0 or an id outside
 * [0, rows): VR_ERR_INVALID; vr_index_update: NULL reps with n > 0 or an id named twice: VR_ERR_INVALID; vr_index_get_rows: both
 * outputs NULL: VR_ERR_INVALID.  n == 0: VR_OK and nothing is touched — not the grouping, the filters or the range result.
 *   All three calls synchronise the stream before they return (the id list is the caller's host memory); vr_index_remove also
 * waits for the device first, as vr_index_reset does, because a search in flight on another stream reads the rows it moves. */
/* Remove the rows ids[0..n) (host int64, any order, duplicates count once).  The remaining rows keep their relative order and
 * close up: a surviving row's new id = old id - (removed ids below it).  *removed (host, may be NULL) = distinct rows removed.
 * What is left is the state of vr_index_reset + vr_index_add of the surviving rows: both stores hold survivor j at row j; the row
 * count drops, so capacity comes back; max|d| and max|d - bf16(d)| of the error model are RECOMPUTED over the survivors (a stale
 * larger maximum would still bound the error, but would leave the certification looser than a fresh index's for ever); the
 * exact-pass hint of vr_index_search_plan is cleared.  The FILTERS ARE CARRIED: bit j of every filter becomes the old bit of the
 * row now at j, and the allowed rows are recounted (a filter may end up allowing nothing: legal).  The GROUPING IS DROPPED, as by
 * vr_index_add: a removal can empty a group, and the offsets are the host's to rebuild.  The range result is gone
 * (vr_index_range_results: VR_ERR_STATE).  The searches' counters stay.
 *   Rows below the first removed id are not touched.  The rest move in ascending windows, each either straight into place (when
 * the rows removed so far make the window's source lie wholly behind it) or through a scratch of at most 64 MiB: never a second
 * copy of the store, and no kernel waits for another workgroup — stream order between launches is the only ordering. */
int vr_index_remove(vr_index_t ix, const int64_t* ids, int64_t n, int64_t* removed, void* stream);
/* Row ids[i] becomes reps[i] (float32 [n][dim], host or device per on_device); ids host, distinct.  The bf16 rows are converted
 * as vr_index_add converts them and the two maxima of the error model are recomputed over all rows (an overwritten row may have
 * been the largest).  No row moves: grouping and filters stay.  The range result is gone and the exact-pass hint is cleared. */
int vr_index_update(vr_index_t ix, const int64_t* ids, const float* reps, int64_t n, int32_t on_device, void* stream);
/* Rows by id: out_f32 [n][dim] float32 and / or out_bf16 [n][dim] uint16 (the MFMA copy; tests), either may be NULL, not both;
 * host or device per on_device; ids host, duplicates allowed.  Changes nothing. */
int vr_index_get_rows(vr_index_t ix, const int64_t* ids, int64_t n, float* out_f32, uint16_t* out_bf16, int32_t on_device,
                      void* stream);
/* Merge per-shard results (e.g. after an RCCL all-gather): in [n_parts][nq][k] scores and
 * global ids -> out [nq][k], same ordering rule.  Device pointers. */
int vr_topk_merge(int device_id, const float* scores, const int64_t* ids, int32_t n_parts,
                  int32_t nq, int32_t k, float* out_scores, int64_t* out_ids, void* stream);
/* The same merge over the packed keys of vr_index_search_keys ([n_parts][nq][k], e.g. the
 * all-gather's output buffer as it is) -> scores and global ids. */
int vr_topk_merge_keys(int device_id, const uint64_t* keys, int32_t n_parts, int32_t nq, int32_t k,
                       float* out_scores, int64_t* out_ids, void* stream);

/* ---- synthetic corpus (bench / test support; no reference counterpart) --------------------- */
/* Pages first .. first + n - 1 of the deterministic synthetic corpus of visrag_amd/synth.py::synth_pages,
 * bit-identical to the host generator, written as uint8 [n][size][size][3] to DEVICE memory.  BASELINE
 * config 3 needs 100 000 distinct pages; there is no dataset on the box (BASELINE.json: "data": synthetic). */
int vr_synth_pages(int device_id, uint8_t* out, int32_t n, int32_t size, int64_t seed, int64_t first, void* stream);

/* ---- streams (caller support; no reference counterpart) ------------------------------------ */
/* *overlap = 1 when kernels on the two streams run SIDE BY SIDE, 0 when the runtime put the streams on one hardware
 * queue (kernels of one wait for the other's).  Probed with two 400 us one-thread kernels, three rounds (~2.5 ms);
 * both streams are synchronised.  A caller that keeps two vr_model_clone workspaces in flight picks its stream pair
 * with this (visrag_amd/engine.py::overlapping_streams): a pair on one queue runs at the single-stream rate. */
int vr_streams_overlap(int device_id, void* stream_a, void* stream_b, int32_t* overlap);

/* ---- host pre-processing moved to the GPU ------------------- */
/* Bicubic resize of an 8-bit RGB (HWC) image, bit-exact with Pillow's
 * Image.resize((out_w, out_h), Image.Resampling.BICUBIC) — the resize of slice_image /
 * find_best_resize (modeling_minicpmv.py:482-537).  src on host or device, dst on device. */
int vr_resize_bicubic(int device_id, const uint8_t* src, int32_t src_on_device, int32_t H, int32_t W,
                      uint8_t* dst, int32_t out_h, int32_t out_w, void* stream);

/* ---- single kernels (parity tests and micro-benchmarks call these through the ABI) ---- */
/* out[M][N] = epilogue(A[M][K] * W[N][K]^T).  A, W bf16 row-major, K % 64 == 0,
 * N % 128 == 0, buffers padded to a multiple of 128 rows.  epilogue:
 *   0 bf16 out = acc + bias            3 f32 out = resid + alpha*(acc + bias)
 *   1 bf16 out = gelu_erf(acc + bias)  4 bf16 out[N/2] = silu(gate)*up (16-row interleaved W)
 *   2 f32  out = acc + bias            5 bf16 out = rope(acc) for col < rope_cols (head 64)
 * bias (f32[N]) and resid (f32[M][ldo]) may be NULL.  variant: 3 = the engine's own choice,
 * 0 = 128x128 tile, 7 = 256x192 tile (N % 192 == 0), 9 = 256x256 tile (8 waves), 12 = 256x256 tile with one
 * wave per SIMD (what the engine uses for its big GEMMs), 13 = its 256x192 form (N % 192 == 0; epilogues 2, 3),
 * 16 = its 256x288 form (N % 288 == 0; epilogue 3 and none of vr_op_gemm_ex's fields but raster_gm: anything else is
 * VR_ERR_INVALID here).
 * Buffers padded to a multiple of 256 rows for the 256-row tiles. */
int vr_op_gemm(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw,
               int32_t M, int32_t N, int32_t K, int32_t epilogue, const float* bias,
               const float* resid, float alpha, void* out, int32_t ldo,
               const int32_t* rope_pos, const float* rope_table, int32_t rope_cols,
               int32_t variant, void* stream);
/* vr_op_gemm with the rest of the launch arguments (GemmArgs, csrc/kernels.h); extras NULL: all zero, i.e. vr_op_gemm.
 * Nothing is checked here beyond what vr_op_gemm checks: every field is either HONOURED by the variant it reaches or the
 * launchers REFUSE the call (VR_ERR_HIP, hipErrorInvalidValue) before anything is launched — for every variant and for 3
 * (the rule applies to the variant the engine's choice lands on):
 *   rowmap (i32 [M], device: output row of input row m, -1 = drop; EPI_RESID reads the residual at the mapped row)
 *                   honoured by 0, 7, 9, 12, 13 for each epilogue the variant has; refused by 14 / 15 / 16
 *   rowbias (f32 [rowbias_period][rowbias_ld], device: row m % rowbias_period is added to the columns n < rowbias_cols)
 *                   honoured with epilogues 0, 1, 2 on 0, 7, 9, 12 and with epilogue 2 on 13; refused with epilogues 3, 4, 5,
 *                   with rowbias_period < 1, and by 14 / 15 / 16
 *   ksplit > 1      (split s covers the K columns [s, s + 1) * K / ksplit and writes its fp32 plane to out + s * split_stride
 *                   floats; the bias rides with plane 0) honoured by 9, 12, 13 with epilogue 2 and K % (ksplit * 64) == 0;
 *                   refused everywhere else (0, 7, 14, 15, 16, any other epilogue) and together with rowmap / rowbias
 *   m_dev, m_sub    (i32 on the device: only the rows m < *m_dev - m_sub exist; 256-row tiles at or past that count are not
 *                   computed, rows between the count and the next multiple of 256 are unspecified) honoured by 9; refused
 *                   everywhere else
 *   col_scale, col_scale_n   (columns n < col_scale_n leave as bf16((acc + bias + rowbias) * col_scale)) honoured with epilogue 0
 *                   and col_scale_n a non-negative multiple of 64 on 0, 7, 9, 12; refused otherwise (any other epilogue, any
 *                   other col_scale_n) and, whatever the epilogue, by 14 / 15 / 16
 *   raster_gm       (m-tiles per rasterisation group, 0 = the launcher's choice) honoured everywhere: the order of the tiles
 *                   never changes a result bit */
typedef struct vr_gemm_extras {
    const int32_t* rowmap;
    const float* rowbias;
    int32_t rowbias_period, rowbias_ld, rowbias_cols;
    float col_scale;
    int32_t col_scale_n;
    int32_t ksplit;
    int64_t split_stride;
    const int32_t* m_dev;
    int32_t m_sub;
    int32_t raster_gm;
} vr_gemm_extras_t;
int vr_op_gemm_ex(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw,
                  int32_t M, int32_t N, int32_t K, int32_t epilogue, const float* bias,
                  const float* resid, float alpha, void* out, int32_t ldo,
                  const int32_t* rope_pos, const float* rope_table, int32_t rope_cols,
                  int32_t variant, const vr_gemm_extras_t* extras, void* stream);
/* vr_op_gemm_ex with one more launch argument, under the same rule:
 *   warm, warm_bytes   (a device region the launch only REQUESTS while it runs: one dword of each of its 128-byte lines, counted from
 *                   its first byte, each line once, so that the launch behind this one finds the region in the memory-side cache —
 *                   nothing is computed from it, nothing outside it is read, no output bit depends on it) honoured by 12 for
 *                   every epilogue; refused by 0, 7, 9, 13, 14, 15, 16 (and by 3 where the engine's choice lands on one of them) and for a region of
 *                   2 GiB or more; warm NULL or
 *                   warm_bytes 0: absent, i.e. vr_op_gemm_ex */
int vr_op_gemm_warm(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw,
                    int32_t M, int32_t N, int32_t K, int32_t epilogue, const float* bias,
                    const float* resid, float alpha, void* out, int32_t ldo,
                    const int32_t* rope_pos, const float* rope_table, int32_t rope_cols,
                    int32_t variant, const vr_gemm_extras_t* extras, const void* warm, uint64_t warm_bytes, void* stream);
/* The variant a vr_op_gemm_warm call with these arguments reaches: `variant` itself, what 3 (the engine's choice) resolves to
 * for this shape, or VR_GEMM_ROUTE_REFUSED where the entry or the launchers refuse the call (a variant that does not exist, a
 * shape off its tile, a field the variant does not honour).  The launch dispatches on the same function.  Host arithmetic only:
 * no device is selected, nothing is launched, the pointers of `extras` are compared with NULL and never dereferenced
 * (extras NULL: all zero); warm_bytes != 0 stands for a region to warm. */
#define VR_GEMM_ROUTE_REFUSED (-1)
int vr_op_gemm_route(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant, int32_t lda, int32_t ldw, int32_t ldo,
                     const vr_gemm_extras_t* extras, uint64_t warm_bytes);
/* y = LN(x) (kind 0, affine, eps) or RMSNorm(x) (kind 1): x f32 [rows][dim] -> bf16 [rows][ldo]. */
int vr_op_norm(int device_id, int32_t kind, const float* x, int32_t rows, int32_t dim,
               const float* weight, const float* bias, float eps, void* out, int32_t ldo,
               void* stream);
/* vr_op_norm with the row pitch of x (ldx >= dim floats; the pitch columns are not read): the ViT's LayerNorms read rows of
 * the padded width. */
int vr_op_norm_ex(int device_id, int32_t kind, const float* x, int32_t rows, int32_t dim, int32_t ldx, const float* weight,
                  const float* bias, float eps, void* out, int32_t ldo, void* stream);

/* ---- the fp32 text path (csrc/hp_text.hip) and the encode glue kernels (csrc/misc.hip, csrc/patch_embed.hip) ----
 * Thin forwards to the launchers the encode path calls.  The entries check NULL pointers only (VR_ERR_INVALID); a shape a
 * launcher cannot run is refused THERE, before anything is launched, and comes back as VR_ERR_HIP.  All buffers are the
 * caller's, on the device, 16-byte aligned unless stated otherwise.
 *
 *   entry                      launcher(s)                                  kernel file
 *   vr_op_text_rmsnorm_split   launch_rmsnorm_split                         hp_text.hip
 *   vr_op_text_rope            launch_rope_f32                              hp_text.hip
 *   vr_op_text_attention       launch_seq_of + launch_attn_f32              hp_text.hip
 *   vr_op_text_swiglu_split    launch_swiglu_split                          hp_text.hip
 *   vr_op_embed_gather         launch_embed_gather / launch_embed_gather_hp misc.hip / hp_text.hip
 *   vr_op_pool                 launch_pool                                  misc.hip
 *   vr_op_convert              launch_f32_to_bf16 / _pad / launch_split_bf16 / launch_any_nonzero16 / launch_iota_pos /
 *                              launch_seq_of                                misc.hip / hp_text.hip
 *   vr_op_planes_sum           launch_planes_sum                            hp_text.hip
 *   vr_op_patch_embed          launch_pack_patch_weight + launch_patch_embed  pack.hip / patch_embed.hip
 *   vr_op_norm_ex              launch_layernorm / launch_rmsnorm            norm.hip */
/* y = x * rsqrt(mean(x^2) + eps) * weight of f32 rows [rows][dim], written as hi + lo bf16 rows [rows][dim] each (y ~= hi + lo
 * to 16 mantissa bits).  hi and lo are separate pointers: the encode path puts lo right behind the `rows` hi rows.
 * dim % 4 == 0, dim <= 2560. */
int vr_op_text_rmsnorm_split(int device_id, const float* x, int32_t rows, int32_t dim, const float* weight, float eps, void* hi,
                             void* lo, void* stream);
/* Rotates, in place, the heads (64 columns, pairs (c, c + 32)) of the first rope_cols columns of the f32 rows qkv [T][ld] by
 * table [pos[t]][32 cos | 32 sin]; pos i32 [T].  rope_cols % 64 == 0. */
int vr_op_text_rope(int device_id, float* qkv, int32_t T, int32_t ld, int32_t rope_cols, const int32_t* pos, const float* table,
                    void* stream);
/* Causal fp32 attention over packed ragged sequences, head_dim 64: qkv f32 [T][ld] holds q | k | v at columns 0, E, 2 E;
 * seq_offsets i32 [B + 1] on the device (seq_offsets[B] == T); out f32 [T][E].  E == 64 heads.  Synchronises the stream. */
int vr_op_text_attention(int device_id, const float* qkv, int32_t ld, int32_t E, const int32_t* seq_offsets, int32_t B, int32_t T,
                         int32_t heads, float scale, float* out, void* stream);
/* act = silu(gate) * up of gu f32 [T][ld_gu] (gate of column i at (i / 16) * 32 + i % 16, up 16 further), written as hi + lo
 * bf16 rows [T][ld_act], columns [I, ld_act) zero.  I % 16 == 0, ld_act % 4 == 0, ld_act >= I. */
int vr_op_text_swiglu_split(int device_id, const float* gu, int32_t T, int32_t ld_gu, int32_t I, int32_t ld_act, void* hi, void* lo,
                            void* stream);
/* out f32 [T][dim] = table[ids[t]] * scale (table_lo NULL) or (table[ids[t]] + table_lo[ids[t]]) * scale; tables bf16
 * [rows][dim], ids i32 [T] on the device.  dim % 4 == 0. */
int vr_op_embed_gather(int device_id, const int32_t* ids, int32_t T, const void* table, const void* table_lo, int32_t dim,
                       float scale, float* out, void* stream);
/* Final RMSNorm, pooling (mode 0 wmean, 1 mean, 2 last token, 3 first token) and L2 normalisation of the packed f32 rows
 * h [seq_offsets[B]][dim]: out f32 [B][dim]; tap (or NULL) f32 [seq_offsets[B]][dim] receives the normed rows.  Every
 * sequence holds at least one row.  dim % 4 == 0, dim <= 2560. */
int vr_op_pool(int device_id, const float* h, const int32_t* seq_offsets, int32_t B, int32_t dim, const float* norm_w, float eps,
               float* out, float* tap, int32_t mode, void* stream);
/* The conversions and index fills:
 *   kind 0: out bf16 [n] = round-to-nearest-even of in f32 [n]
 *   kind 1: the same for the first n elements, zeros up to n_total (n, n_total % 4 == 0); aux (or NULL): two i32 cleared
 *   kind 2: out / out2 bf16 [n] = hi / lo parts of in f32 [n], hi = bf16(v), lo = bf16(v - hi)
 *   kind 3: *aux |= 1 if any of the n 16-bit words of `in` is neither +0 nor -0
 *   kind 4: in = seq_offsets i32 [n + 1]: out i32 [t] = t - seq_offsets[b] for every token t of sequence b
 *   kind 5: in = seq_offsets i32 [n + 1]: out i32 [t] = b */
int vr_op_convert(int device_id, int32_t kind, const void* in, void* out, void* out2, int64_t n, int64_t n_total, int32_t* aux,
                  void* stream);
/* out[t][c] = (accumulate ? out[t][c] : 0) + alpha * (parts[0][t][c] + parts[1][t][c] + ...), c < N: n_parts f32 planes
 * [T][ldp], plane p at parts + p * stride floats, summed in plane order; out f32 [T][ldo], columns >= N not written.
 * N, ldp, ldo % 4 == 0. */
int vr_op_planes_sum(int device_id, const float* parts, int32_t n_parts, int64_t stride, int32_t ldp, int32_t T, int32_t N,
                     float* out, int32_t ldo, float alpha, int32_t accumulate, void* stream);
/* ToTensor + Normalize(0.5, 0.5) + Conv2d(3, D, kernel = stride = P) + bias + position embedding of n HWC u8 images of H x W:
 * imgs is a HOST array of n device pointers; weight f32 [D][3][P][P] (packed into a temporary as vr_model_load_weight packs
 * it, K columns per row, K % 64 == 0, K >= 3 P^2); bias f32 [D]; pos f32 [(H / P)(W / P)][ld_pos]; out f32
 * [n (H / P)(W / P)][ldo], row (img, py, px).  D % 128 == 0, H % P == 0, W % P == 0.  Synchronises the stream. */
int vr_op_patch_embed(int device_id, const void* const* imgs, int32_t n, int32_t H, int32_t W, int32_t P, const float* weight,
                      int32_t D, int32_t K, const float* bias, const float* pos, int32_t ld_pos, float* out, int32_t ldo,
                      void* stream);
/* Flash attention over bf16 q/k/v with row strides ld*, per-batch row ranges cu_q/cu_kv
 * ([B+1], device), head_dim in {64,72,80,128}; causal uses absolute positions within the
 * sequence.  q_batch_stride==0 shares q across the batch (resampler). out bf16 [rows_q][ldo].
 *
 * What a launch may touch (every kernel behind it; tests/test_gpu_attention_isolation.py holds them to it on a buffer whose
 * every other cell is NaN).  Item b has the q / out rows [cu_q[b], cu_q[b+1]) and the key rows [cu_kv[b], cu_kv[b+1]) (or
 * [cu_kv[b], kv_end[b]), vr_op_attention_ex); H = heads * head_dim (K / V: H / kv_group).
 *   READ    q: columns [0, H) of the q rows of items that have keys (q_shared: of rows [0, cu_q[b+1] - cu_q[b]) of q itself;
 *              q_in_rows / q_head_stride: of the rows and head offsets they name), nothing else of q.
 *           k, v: columns [0, H) of the key rows of items that have q rows, nothing else — not the row behind a range (in a
 *              cache: stale rows), not the pitch columns [H, ld), not a neighbouring allocation.  The kernels walk keys in
 *              tiles of 64 that run past a range's last row; what lies there never reaches a result: the loads are bounded by
 *              the range's last row or their values are replaced (never multiplied by zero) before they are used.
 *           cu_q, cu_kv [B+1], kv_end / q_in_rows [B].
 *   WRITTEN out rows [cu_q[b], cu_q[b+1]) x columns [0, H), and the same rows of lse, of items that HAVE keys — every one of
 *           those cells, and no other: not the row behind an item, not out's pitch columns [H, ldo), nothing of an item
 *           without keys.  No input is written.
 *   The ONE exception is a precondition of the head_dim 72 route VR_ATTN_ROUTE_72W (attention_w.hip; the ViT): it stages a
 *   head's 72 columns as 80, so in every key row of an item it also reads the 8 elements BEHIND a head's 72 of k and of v — the next head's
 *   first 8 columns or, for the last head, k[row][H .. H+8) and v[row][H .. H+8) — and multiplies them by zero.  Those
 *   16 bytes must be readable and hold FINITE bf16 values (any finite value: no output bit depends on them; a NaN or an
 *   infinity there would reach the outputs as 0 * NaN).  The route is only taken when k and v are columns of the same rows
 *   (v - k inside one row, ldk == ldv), so the cells lie in the caller's own row buffer: in the engine (encode.hip, the only
 *   caller on this route) the v columns behind k and, behind v, what the qkv GEMM wrote there — the row's pad columns or the
 *   next row's q columns. */
int vr_op_attention(int device_id, const void* q, int32_t ldq, const void* k, int32_t ldk,
                    const void* v, int32_t ldv, void* out, int32_t ldo,
                    const int32_t* cu_q, const int32_t* cu_kv, int32_t B, int32_t heads,
                    int32_t head_dim, int32_t max_q, int32_t causal, int32_t q_shared,
                    float scale, void* stream);
/* vr_op_attention with the rest of the launch arguments (AttnArgs, csrc/kernels.h); extras NULL: all zero.
 *   kv_group       grouped-query attention: query head h reads K / V head h / kv_group (0 or 1: one each)
 *   kv_end         i32 [B] (device) or NULL: item b's K / V rows are [cu_kv[b], kv_end[b]) — ranges of different caches
 *   q_in_rows      i32 [B] (device) or NULL: first q row of item b (reading q only; the out rows stay cu_q)
 *   q_head_stride  elements between the heads of a q row (0: head_dim): the query heads of a group as the ROWS of a tile
 *   q_prescaled    the q rows already carry scale * log2(e) (vr_gemm_extras_t::col_scale): no kernel scales again
 *   lse            f32 [rows_q][heads] (device) or NULL: log2(sum_k exp(scale * s_k)) of every row that has keys
 * An item without keys writes neither its out rows nor its lse. */
typedef struct vr_attn_extras {
    int32_t kv_group;
    const int32_t* kv_end;
    const int32_t* q_in_rows;
    int32_t q_head_stride;
    int32_t q_prescaled;
    float* lse;
} vr_attn_extras_t;
int vr_op_attention_ex(int device_id, const void* q, int32_t ldq, const void* k, int32_t ldk,
                       const void* v, int32_t ldv, void* out, int32_t ldo,
                       const int32_t* cu_q, const int32_t* cu_kv, int32_t B, int32_t heads,
                       int32_t head_dim, int32_t max_q, int32_t causal, int32_t q_shared,
                       float scale, const vr_attn_extras_t* extras, void* stream);
/* The kernel vr_op_attention_ex reaches with the same arguments — the launch dispatches on the very function behind this, so
 * the answer cannot drift from it.  Host arithmetic only: nothing is launched, no device is selected and no pointer is
 * dereferenced (pointers and strides are compared with each other, so a test may pass made-up addresses).  Returns
 *   VR_ATTN_ROUTE_NONE      nothing to do (B <= 0 or max_q <= 0): the launch succeeds without a kernel
 *   VR_ATTN_ROUTE_REFUSED   the launch fails before anything runs (a NULL pointer, a stride off its alignment, a head_dim
 *                           nobody implements)
 *   VR_ATTN_ROUTE_SMALL     attention_small.hip: head_dim 64, max_q <= 80, cu_q and cu_kv the SAME buffer, no extras
 *   VR_ATTN_ROUTE_72W       attention_w.hip: head_dim 72, non-causal, no extras, k and v columns of the same rows (0 < v - k <
 *                           one row, heads * 72 elements apart at least, ldk == ldv), max_q >= 192 and at most 1/8 of its 256-row
 *                           query tiles wasted (which is the stricter of the two: 224..256, 448..512, 672..768, ...)
 *   VR_ATTN_ROUTE_TILED(head_dim, qf, pipe)   attention.hip's attention_kernel<head_dim, qf, pipe>: 64 qf query rows per
 *                           workgroup; head_dim 64 / 72 / 80: <1, 0> up to max_q 64, <2, 0> up to 128, <2, 3> beyond; 128: <1, 0> */
#define VR_ATTN_ROUTE_REFUSED (-1)
#define VR_ATTN_ROUTE_NONE 0
#define VR_ATTN_ROUTE_SMALL 1
#define VR_ATTN_ROUTE_72W 2
#define VR_ATTN_ROUTE_TILED(head_dim, qf, pipe) (100000 + (head_dim) * 100 + (qf) * 10 + (pipe))
int vr_op_attention_route(int device_id, const void* q, int32_t ldq, const void* k, int32_t ldk,
                          const void* v, int32_t ldv, void* out, int32_t ldo,
                          const int32_t* cu_q, const int32_t* cu_kv, int32_t B, int32_t heads,
                          int32_t head_dim, int32_t max_q, int32_t causal, int32_t q_shared,
                          float scale, const vr_attn_extras_t* extras);
/* Merge of the KV ranges of a decode step's attention (head_dim 128): part bf16 / lse f32 are the out / lse of
 * vr_op_attention_ex run with the `group` query heads of a KV head as rows — the layout is SkinnyCombine's in
 * csrc/kernels.h; row r of n_rows owns the 16 ranges from 16 r on, the first S (or S_dev[r], i32 on the device, when S_dev is
 * not NULL) of which are merged.
 *   W NULL: out bf16, row r at out + r * ld_out elements, out[h * 128 + d] for the `heads` query heads.
 *   W bf16 [N][ldw] (rows readable up to the next multiple of 256): the merged row (rounded to bf16) times W^T as fp32
 *           planes out[ksplit][M][ldo], plane s at out + s * split_stride floats, `planes` of them allocated (ksplit <= planes)
 *           — the decode step's o projection, merged inside gemm_skinny.hip.  M = 1, K = heads * 128 and at most four
 *           K-steps per split are the LAUNCHER's limits: anything else is refused there (VR_ERR_HIP) before a launch. */
int vr_op_attn_combine(int device_id, const void* part, const float* lse, int32_t S, const int32_t* S_dev, int32_t heads,
                       int32_t group, int32_t n_rows, void* out, int32_t ld_out, const void* W, int32_t ldw, int32_t M,
                       int32_t N, int32_t K, int32_t ksplit, int32_t planes, int32_t ldo, int64_t split_stride, void* stream);
/* The decode step's weight streamer (gemm_skinny.hip): A bf16 [M <= 32][lda], W bf16 [N][ldw] (nn.Linear layout), K % 64 == 0,
 * N % 4 == 0.  The CALLER pads: A readable up to 16 rows (32 when M > 16), W up to the next multiple of 256 rows.
 *   swiglu 0: fp32 planes out[ksplit][M][ldo] (plane s at out + s * split_stride floats); split s covers the K-steps
 *             [s * ceil(steps / ksplit), ...), a split past the end writes zeros; bias (f32 [N] or NULL) rides with split 0.
 *   swiglu 1: ksplit 1, M <= 16, N % 32 == 0, W rows (and bias) interleaved [16 gate | 16 up]: out = bf16 act [M][ldo],
 *             act[m][i] = silu(gate) * up, N / 2 columns.
 * Rows >= M and columns >= N of out are not written. */
int vr_op_gemm_skinny(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw, int32_t M, int32_t N,
                      int32_t K, int32_t ksplit, const float* bias, int32_t swiglu, void* out, int32_t ldo,
                      int64_t split_stride, void* stream);
/* The consumers of those planes (parts f32 [nsplit][rows][ldp], plane s at parts + s * split_stride), summed in plane order.
 *   kind 0: x[rows][ldx] += alpha * sum_s parts[s] in place (dim columns), then out = bf16 RMSNorm(x) * weight [rows][ldo],
 *           columns [dim, ldo) zero; out NULL: the update only.  dim <= 3584.
 *   kind 1: out = bf16 [rows][ldo], out[m][i] = silu(gate) * up of the summed planes, i < dim, gate of column i at
 *           (i / 16) * 32 + i % 16 and up 16 further (x, alpha, weight, eps unused). */
int vr_op_plane_sum(int device_id, int32_t kind, const float* parts, int32_t nsplit, int64_t split_stride, int32_t ldp,
                    int32_t rows, int32_t dim, float* x, int32_t ldx, float alpha, const float* weight, float eps,
                    void* out, int32_t ldo, void* stream);
/* Decode attention of one step (chat_kernels.hip), head_dim 64, E / 64 heads, scale 64^-0.5: q bf16 [n][E]; prompt cache bf16
 * [layers][K|V][slots][max_len][E]; tail cache bf16 [layers][K|V][rows][max_new][E]; layer l.  Step row i attends to the
 * slot_plen[step_slot[i]] prompt keys of its slot and to the tail keys 0..step_tail[i] of cache row step_row[i]; the rows of a
 * slot are adjacent and form one group.  The key ranges come from the policy vr_chat_step uses; force_splits 1..8 sets the
 * number of ranges of every group instead (0: the policy).  step_* and slot_plen are host arrays; att bf16 [n][E].
 * Synchronises the stream. */
int vr_op_chat_attention(int device_id, const void* q, const void* prompt, const void* tails, int32_t layers, int32_t l,
                         int32_t E, int32_t slots, int32_t max_len, int32_t rows, int32_t max_new, int32_t n,
                         const int32_t* step_row, const int32_t* step_slot, const int32_t* step_tail,
                         const int32_t* slot_plen, int32_t force_splits, void* att, void* stream);
/* vr_chat_extend's two-segment attention (chat_extend.hip) on the caller's buffers, head_dim 64, scale 1/8, `heads` heads
 * (heads * 64 <= E): q bf16 [seq_off[B]][ldq], head h at column h * 64; caches as vr_op_chat_attention's; layer l.  Sequence b
 * owns the packed rows [seq_off[b], seq_off[b + 1]) (n_b >= 1 of them): query j sees the prompt keys [0, seq_plen[b]) of slot
 * seq_slot[b] and the tail keys [0, seq_t0[b] + j] of cache row seq_row[b], which already hold the new tokens' K / V.  out bf16
 * [seq_off[B]][ldo].  No plane row outside [0, plen) / [0, t0 + n) is read, nothing but the sequence's own out rows is
 * written.  seq_* are host arrays; 1 <= B <= 16, rows distinct, 1 <= plen <= max_len, t0 >= 0, t0 + n <= max_new, ldq a
 * multiple of 8, ldo of 4, both >= heads * 64, pointers 16-byte aligned — every check comes before the launch
 * (VR_ERR_INVALID; B > 16, plen > max_len or t0 + n > max_new: VR_ERR_CAPACITY).  Synchronises the stream. */
int vr_op_chat_extend_attention(int device_id, const void* q, int32_t ldq, const void* prompt, const void* tails, int32_t layers,
                                int32_t l, int32_t E, int32_t heads, int32_t slots, int32_t max_len, int32_t rows, int32_t max_new,
                                int32_t B, const int32_t* seq_row, const int32_t* seq_slot, const int32_t* seq_plen,
                                const int32_t* seq_t0, const int32_t* seq_off, void* out, int32_t ldo, void* stream);
/* vr_chat_select's kernels on the caller's logits: logits f32 [n][ld] and seen bit sets u32 [n][words] on the device (row i of
 * both belongs to selected row i), group_offsets [n_groups + 1] and beam_scores [n] (or NULL) on the host.  mode VR_CHAT_*;
 * K candidates are ranked (the sampler draws among them), kout are returned per group: out_* [n_groups][kout] on the host,
 * outputs past the candidates are (-inf, -1, -1).  Ties: the lower flat index parent * V + token first. */
int vr_op_chat_select(int device_id, int32_t mode, const float* logits, int32_t ld, int32_t V, const uint32_t* seen,
                      int32_t words, int32_t n_groups, const int32_t* group_offsets, const float* beam_scores, int32_t K,
                      int32_t kout, float repetition_penalty, float temperature, uint64_t seed, int32_t step,
                      float* out_scores, int32_t* out_tokens, int32_t* out_parents, void* stream);
/* vr_chat_sample's kernel on the caller's buffers: logits f32 [n][ld] and seen bit sets u32 [n][words] on the device, one draw
 * per row, n <= 16; the definition, the outputs (host arrays [n]) and the error codes are vr_chat_sample's, plus V >= 1,
 * ld >= V, words >= ceil(V / 32) (VR_ERR_INVALID).  Synchronises the stream. */
int vr_op_chat_sample(int device_id, const float* logits, int32_t ld, int32_t V, const uint32_t* seen, int32_t words, int32_t n,
                      float repetition_penalty, float temperature, int32_t top_k, double top_p, uint64_t seed, int32_t step,
                      float* out_scores, int32_t* out_tokens, int32_t* out_kept, int32_t* out_cut, void* stream);
/* The batched prefill's per-layer K / V scatter (chat_kernels.hip) on the caller's buffers, ONE layer's planes: qkv bf16
 * [seq_offsets[B]][ld], row t = q | k | v of a packed token (k at column E, v at 2 E; ld >= 3 E; E, ld multiples of 8);
 * kplane / vplane bf16 [n_slots][max_len][E].  Token t of prompt b (seq_offsets[b] <= t < seq_offsets[b + 1]) goes to
 * row t - seq_offsets[b] of slot slots[b]; nothing else of the planes is written.  slots are distinct, every prompt holds
 * 1..max_len rows, B <= 16; seq_offsets and slots are host arrays, all pointers 16-byte aligned.  Synchronises the stream. */
int vr_op_chat_prompt_scatter(int device_id, const void* qkv, int32_t ld, int32_t E, int32_t B, const int32_t* seq_offsets,
                              const int32_t* slots, int32_t n_slots, int32_t max_len, void* kplane, void* vplane, void* stream);
/* vr_chat_score's head (csrc/head_score.hip) on the caller's buffers, all on the device: A bf16 [pad256(M)][lda] (rows >= M
 * are read, never counted or written), W bf16 [pad256(V)][ldw] (columns >= V never count, whatever they hold), K a multiple
 * of 64, lda / ldw >= K and multiples of 8, A and W 16-byte aligned; targets int32 [M].  Outputs [M] each as vr_chat_score's;
 * a target outside [0, V) leaves its out_logit entry unwritten.  No M x V buffer is allocated: the scratch is
 * 3 * ceil(V / 256) * M words.  M < 1, V < 1 or a NULL pointer: VR_ERR_INVALID; a shape the launcher refuses: VR_ERR_HIP.
 * Synchronises the stream. */
int vr_op_head_score(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw, int32_t M, int32_t V, int32_t K,
                     const int32_t* targets, float* out_logit, float* out_lse, float* out_top_logit, int32_t* out_top_token,
                     void* stream);

/* ---- the EVisRAG generator's small kernels (csrc/gen_kernels.hip; the model calls them through vg_*, include/visrag_gen.h) ----
 * Thin forwards to the launchers gen.hip / gen_vision.hip call.  The entries check NULL pointers and counts (VR_ERR_INVALID); a
 * shape a launcher cannot run is refused THERE, before its kernel is launched, and comes back as VR_ERR_HIP.  Buffers are the
 * caller's, on the device, unless stated otherwise.
 *
 *   entry                    launcher(s)
 *   vr_op_gen_mrope_cache    launch_mrope_cache
 *   vr_op_gen_rope2d         launch_rope2d_table + launch_rope2d_inplace
 *   vr_op_gen_sample         launch_sample
 *   vr_op_gen_mark_seen      launch_mark_seen
 *   vr_op_gen_decode_begin   launch_decode_begin
 *   vr_op_gen_rows           launch_scatter_rows / launch_gather_rows_bf16 / launch_patch_rows_u8
 *
 * `state` below is the decode state that lives on the device, 42 i32 words:
 *   0 token | 1..3 temporal / height / width position | 4 len (KV-cache rows in use before the step) | 5 step (index of the next
 *   sampled token: selects the sampling noise) | 6 splits | 7 unused | 8..24 cu_q[17] | 25..41 cu_kv[17] */
/* Multimodal RoPE + KV-cache append, head_dim 128: T rows of H query, KV key and KV value heads ((H + 2 KV) * 128 columns).
 * Source: parts NULL: bf16 rows src_bf16 [T][ld]; else fp32 planes parts [n_parts][plane_stride] of rows [T][ld], summed in
 * float32 in the order bias (f32 [(H + 2 KV) * 128] or NULL: 0) + plane 0 + plane 1 + ...  Pair p of a head is columns
 * (p, p + 64), its angle float(pos3[c][t]) * inv_freq[p] (f32 [64]) with c = 0 for p < sec_t, 1 for p < sec_t + sec_h, else 2;
 * pos3 i32 [3][pos_stride].  Rotated q -> q_out bf16 [T][ldq]; rotated k and the unrotated v -> row r(t) of k_cache / v_cache
 * bf16 [rows][ld_cache], r(t) = cache_rows[t] (i32 [T] on the device) if given, else row0 + t with row0 = *row0_dev (i32 on the
 * device) if given, else cache_row0.  cu_kv (i32 [2] on the device, or NULL) receives {0, row0 + T}.  Nothing else is written. */
int vr_op_gen_mrope_cache(int device_id, const void* src_bf16, const float* parts, int32_t n_parts, int64_t plane_stride,
                          const float* bias, int32_t ld, int32_t T, int32_t H, int32_t KV, const int32_t* pos3, int32_t pos_stride,
                          int32_t sec_t, int32_t sec_h, const float* inv_freq, void* q_out, int32_t ldq, void* k_cache, void* v_cache,
                          int32_t ld_cache, int32_t cache_row0, const int32_t* row0_dev, const int32_t* cache_rows, int32_t* cu_kv,
                          void* stream);
/* The vision tower's 2-D rotary embedding, in place: head slot j < n_slots of row t is columns [2 hh j, 2 hh (j + 1)) of qkv bf16
 * [T][ld], its pair p < hh the columns (p, p + hh), the pair's angle float(p < sec_h ? pos_h[t] : pos_w[t]) * freq[p]; pos_h,
 * pos_w i32 [T], freq f32 [64].  Columns from 2 hh n_slots on (v, padding) are not touched.  hh <= 64.  Synchronises the stream. */
int vr_op_gen_rope2d(int device_id, void* qkv, int32_t ld, int32_t T, int32_t n_slots, int32_t hh, const int32_t* pos_h,
                     const int32_t* pos_w, int32_t sec_h, const float* freq, void* stream);
/* Next token of one row of logits f32 [vocab]: repetition penalty on the ids of the bit set seen u32 [ceil(vocab / 32)] (logit > 0:
 * / penalty, else * penalty), then temperature 0: the argmax, ties to the lowest id; temperature > 0: the argmax of
 * logit / temperature + Gumbel noise of (seed, step, id).  The pick's bit is set in `seen` and it is copied to *out_token (host).
 * state (or NULL): word 0 receives the pick; step_from_state: the noise index is word 5, not `step`; advance: words 1..5 grow by
 * one.  The 64 partial keys are the entry's own scratch.  Synchronises the stream. */
int vr_op_gen_sample(int device_id, const float* logits, int32_t vocab, uint32_t* seen, float repetition_penalty, float temperature,
                     uint64_t seed, int32_t step, int32_t* state, int32_t step_from_state, int32_t advance, int32_t* out_token,
                     void* stream);
/* seen[id / 32] |= 1 << (id % 32) for the n ids (i32, device); ids outside [0, vocab) are ignored. */
int vr_op_gen_mark_seen(int device_id, const int32_t* ids, int32_t n, uint32_t* seen, int32_t vocab, void* stream);
/* The KV ranges of a decode step's attention from word 4 of `state`: L = len + 1 cache rows in at most 16 ranges of `chunk` rows, a
 * multiple of 64; splits = the ranges that hold a row, cu_kv[i] = min(L, i chunk), cu_q[i] = i q_rows, i = 0..16. */
int vr_op_gen_decode_begin(int device_id, int32_t* state, int32_t q_rows, void* stream);
/* The row movers.  kind 0: dst f32 [.][ld], dst[row_idx[i]][0..dim) = src[i][0..dim), src f32 [n][dim].
 *   kind 1: dst bf16 [n][ld], dst[i] = bf16(src[row_idx[i]][0..dim)), columns [dim, ld) zero; src rows are dense ([.][dim]).
 *   kind 2: dst bf16 [n][ld], dst[i] = patch (ph[i], pw[i]) of page img[i], P x P pixels, element (c, t, y, x) =
 *           (u8 / 255 - mean3[c]) / std3[c] in float32, the same for each of the tp temporal copies, columns [3 tp P^2, ld) zero.
 *           pages: HOST array of n_pages device pointers to u8 HWC pages, page_w their widths (host), both uploaded by the entry;
 *           img, ph, pw i32 [n] on the device; mean3, std3 on the host.  Synchronises the stream. */
int vr_op_gen_rows(int device_id, int32_t kind, const float* src, const int32_t* row_idx, int32_t n, int32_t dim, void* dst,
                   int32_t ld, const void* const* pages, const int32_t* page_w, int32_t n_pages, const int32_t* img, const int32_t* ph,
                   const int32_t* pw, int32_t P, int32_t tp, const float* mean3, const float* std3, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VISRAG_HIP_H */
