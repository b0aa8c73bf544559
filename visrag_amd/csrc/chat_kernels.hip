// Kernels of MiniCPM-V 2.0 answer generation on the VisRAG-Ret weights (vr_chat_*, chat.hip): the decode step's token
// embedding, q|k|v plane sum + RoPE + KV-tail append, decode attention for head_dim 64 (full multi-head), and the logits
// processing of HF generate (repetition penalty, log_softmax + beam scores, top-k candidates, sampling).
// The decode step's GEMMs are the weight streamer of gemm_skinny.hip; everything here is small and HBM / latency bound.
#include <algorithm>
#include <vector>

#include "chat_score.h"
#include "common.h"
#include "gen_math.h"
#include "kernels.h"

namespace vr {

namespace {

// element offset of cache plane (layer l, kind kv: 0 = K, 1 = V, index idx of count: a prompt slot or a tail row): [cap][E] bf16
__device__ __forceinline__ size_t cache_off(int l, int kv, int idx, int count, int cap, int E) {
    return (((size_t)l * 2 + kv) * count + idx) * (size_t)cap * E;
}

__device__ __forceinline__ unsigned long long key_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// max of a 64-bit key over the block (blockDim.x = 256); every thread gets the result
__device__ __forceinline__ unsigned long long block_key_max(unsigned long long k, unsigned long long* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) k = key_max(k, __shfl_xor(k, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
    __syncthreads();
    k = key_max(key_max(red[0], red[1]), key_max(red[2], red[3]));
    __syncthreads();
    return k;
}

}  // namespace

// h[i] = embed[token_i] * scale_emb (modeling_minicpm.py:1212: inputs_embeds * scale_emb); the token joins row i's seen set
__global__ __launch_bounds__(256) void chat_embed_kernel(ChatStep st, const bf16_t* __restrict__ table, int E, float scale,
                                                         float* __restrict__ h, unsigned* __restrict__ seen, int words) {
    const int i = blockIdx.x, tok = st.token[i];
    const bf16_t* src = table + (size_t)tok * E;
    for (int c = threadIdx.x; c < E; c += 256) h[(size_t)i * E + c] = bf2f(src[c]) * scale;
    if (threadIdx.x == 0) seen[(size_t)st.row[i] * words + (tok >> 5)] |= 1u << (tok & 31);
}

// One workgroup per (step row i, head): threads [0, 32) rotate the q pairs (p, p + 32), [32, 64) the k pairs, [64, 96) copy
// the v pairs; the split-K planes of the q|k|v projection are summed in a fixed order first.  q -> bf16 q_out [n][E];
// k, v -> the row's tail at index st.tail[i] (the cache row of position st.pos[i]).
__global__ __launch_bounds__(96) void chat_qkv_kernel(ChatStep st, const float* __restrict__ parts, int n_parts, size_t plane,
                                                      int ldp, const float* __restrict__ rope, int E, bf16_t* __restrict__ q_out,
                                                      bf16_t* __restrict__ tails, int l, int max_rows, int max_new) {
    const int i = blockIdx.x, h = blockIdx.y, part = threadIdx.x >> 5, p = threadIdx.x & 31;
    const float* src = parts + (size_t)i * ldp + part * E + h * 64 + p;
    float x1 = 0.f, x2 = 0.f;
    for (int s = 0; s < n_parts; ++s) { x1 += src[(size_t)s * plane]; x2 += src[(size_t)s * plane + 32]; }
    if (part < 2) {
        const float* tab = rope + (size_t)st.pos[i] * 64;                 // [pos][32 cos | 32 sin]
        rope_rotate(x1, x2, tab[p], tab[32 + p]);
    }
    bf16_t* dst = part == 0 ? q_out + (size_t)i * E + h * 64
                            : tails + cache_off(l, part - 1, st.row[i], max_rows, max_new, E) + (size_t)st.tail[i] * E + h * 64;
    dst[p] = f2bf(x1);
    dst[p + 32] = f2bf(x2);
}

// Decode attention, head_dim 64, one query row per beam.  Grid (heads, groups, splits): group g = the step rows
// [g_lo[g], g_lo[g + 1]) — the beams of ONE prompt — whose prompt K/V are stored once per prompt slot.  Split s takes a range
// of the prompt's keys with ALL the group's rows as the rows of its tile: every prompt K / V row is read once for all beams.
// The last split also walks every row's own tail (the generated tokens, this step's row included).  Per (row, head, split)
// the unnormalised output, the running max and the denominator (exp2 domain) go to po / pml; chat_attn_combine merges.
__global__ __launch_bounds__(256) void chat_attn_kernel(ChatStep st, const bf16_t* __restrict__ q, const bf16_t* __restrict__ prompt,
                                                        const bf16_t* __restrict__ tails, int l, int E, ChatCaps cap, int S,
                                                        float* __restrict__ po, float* __restrict__ pml) {
    __shared__ float qs[CHAT_MAX_ROWS][64];
    __shared__ float sc[CHAT_MAX_ROWS][CHAT_KEYS];
    __shared__ float rm[CHAT_MAX_ROWS], rl[CHAT_MAX_ROWS], ra[CHAT_MAX_ROWS];
    const int h = blockIdx.x, g = blockIdx.y, sp = blockIdx.z, H = gridDim.x;
    S = st.gsplit[g];                                             // (per prompt: a row's sums do not depend on its batch mates)
    if (sp >= S) return;
    const int r0 = st.g_lo[g], nb = st.g_lo[g + 1] - r0;
    const int slot = st.slot[r0], P = st.plen[g];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float qscale = 0.125f * 1.44269504088896340736f;       // head_dim^-0.5 * log2(e): scores in the exp2 domain
    for (int e = tid; e < nb * 64; e += 256) qs[e >> 6][e & 63] = bf2f(q[(size_t)(r0 + (e >> 6)) * E + h * 64 + (e & 63)]) * qscale;
    if (tid < CHAT_MAX_ROWS) { rm[tid] = -INFINITY; rl[tid] = 0.f; ra[tid] = 1.f; }
    __syncthreads();
    float acc[CHAT_MAX_ROWS / 4] = {0.f, 0.f, 0.f, 0.f};          // channel `lane` of rows wave, wave + 4, ...
    // one chunk of <= CHAT_KEYS keys [j0, j0 + cnt) of planes kb / vb; owner < 0: keys of every row (the prompt), else of row owner only
    auto chunk = [&](const bf16_t* kb, const bf16_t* vb, int j0, int cnt, int owner) {
        if (tid < cnt) {
            const bf16_t* kr = kb + (size_t)(j0 + tid) * E;
            float kv[64];
#pragma unroll
            for (int c = 0; c < 64; c += 8) {
                const bf16x8 v8 = *reinterpret_cast<const bf16x8*>(kr + c);
#pragma unroll
                for (int u = 0; u < 8; ++u) kv[c + u] = bf2f(v8[u]);
            }
            for (int r = 0; r < nb; ++r) {
                float s = -INFINITY;
                if (owner < 0 || owner == r) {
                    s = 0.f;
#pragma unroll
                    for (int c = 0; c < 64; ++c) s = fmaf(qs[r][c], kv[c], s);
                }
                sc[r][tid] = s;
            }
        }
        __syncthreads();
        for (int r = wave; r < nb; r += 4) {                       // online softmax, one wave per row
            float mx = -INFINITY;
            for (int j = lane; j < cnt; j += 64) mx = fmaxf(mx, sc[r][j]);
            mx = wave_max(mx);
            const float mo = rm[r], mn = fmaxf(mo, mx);
            float sum = 0.f;
            for (int j = lane; j < cnt; j += 64) {
                const float e = mn == -INFINITY ? 0.f : exp2f(sc[r][j] - mn);
                sc[r][j] = e;
                sum += e;
            }
            sum = wave_sum(sum);
            if (lane == 0) {
                const float a = mn == -INFINITY ? 1.f : exp2f(mo - mn);
                ra[r] = a; rl[r] = rl[r] * a + sum; rm[r] = mn;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CHAT_MAX_ROWS / 4; ++k) {
            const int r = wave + 4 * k;
            if (r < nb && (owner < 0 || owner == r)) {
                float a = acc[k] * ra[r];
                const bf16_t* vr = vb + (size_t)j0 * E + lane;
#pragma unroll 8
                for (int j = 0; j < cnt; ++j) a = fmaf(sc[r][j], bf2f(vr[(size_t)j * E]), a);
                acc[k] = a;
            }
        }
        __syncthreads();
    };
    const int per = (P + S - 1) / S, k_lo = min(P, sp * per), k_hi = min(P, k_lo + per);
    {
        const bf16_t* pk = prompt + cache_off(l, 0, slot, cap.slots, cap.len, E) + h * 64;
        const bf16_t* pv = prompt + cache_off(l, 1, slot, cap.slots, cap.len, E) + h * 64;
        for (int j0 = k_lo; j0 < k_hi; j0 += CHAT_KEYS) chunk(pk, pv, j0, min(CHAT_KEYS, k_hi - j0), -1);
    }
    if (sp == S - 1) {
        for (int r = 0; r < nb; ++r) {
            const int row = st.row[r0 + r], len = st.tail[r0 + r] + 1;
            const bf16_t* tk = tails + cache_off(l, 0, row, cap.rows, cap.tail, E) + h * 64;
            const bf16_t* tv = tails + cache_off(l, 1, row, cap.rows, cap.tail, E) + h * 64;
            for (int j0 = 0; j0 < len; j0 += CHAT_KEYS) chunk(tk, tv, j0, min(CHAT_KEYS, len - j0), r);
        }
    }
#pragma unroll
    for (int k = 0; k < CHAT_MAX_ROWS / 4; ++k) {
        const int r = wave + 4 * k;
        if (r < nb) po[(((size_t)(r0 + r) * H + h) * CHAT_ATT_SPLITS + sp) * 64 + lane] = acc[k];
    }
    if (tid < nb) {
        float* d = pml + (((size_t)(r0 + tid) * H + h) * CHAT_ATT_SPLITS + sp) * 2;
        d[0] = rm[tid];
        d[1] = rl[tid];
    }
}

// att[i][h * 64 + d] = sum_s 2^(m_s - M) po_s[d] / sum_s 2^(m_s - M) l_s   (grid (n, heads), 64 threads)
__global__ __launch_bounds__(64) void chat_attn_combine_kernel(ChatStep st, const float* __restrict__ po, const float* __restrict__ pml, int E,
                                                               bf16_t* __restrict__ att) {
    const int i = blockIdx.x, h = blockIdx.y, d = threadIdx.x, S = st.rsplit[i];
    const size_t b = ((size_t)i * gridDim.y + h) * CHAT_ATT_SPLITS;
    float M = -INFINITY;
    for (int s = 0; s < S; ++s) M = fmaxf(M, pml[(b + s) * 2]);
    float num = 0.f, den = 0.f;
    for (int s = 0; s < S; ++s) {
        const float w = exp2f(pml[(b + s) * 2] - M);
        num = fmaf(w, po[(b + s) * 64 + d], num);
        den = fmaf(w, pml[(b + s) * 2 + 1], den);
    }
    att[(size_t)i * E + h * 64 + d] = f2bf(num / den);
}

// the prefill's rope'd K and V rows of one layer (q | k | v bf16 rows of the encode pass) -> the prompt slot's cache planes
__global__ __launch_bounds__(256) void chat_prompt_kv_kernel(const bf16_t* __restrict__ qkv, int ld, int E, bf16_t* __restrict__ kdst,
                                                             bf16_t* __restrict__ vdst) {
    const int t = blockIdx.x;
    const bf16_t* src = qkv + (size_t)t * ld;
    for (int c = threadIdx.x * 8; c < E; c += 256 * 8) {
        *reinterpret_cast<bf16x8*>(kdst + (size_t)t * E + c) = *reinterpret_cast<const bf16x8*>(src + E + c);
        *reinterpret_cast<bf16x8*>(vdst + (size_t)t * E + c) = *reinterpret_cast<const bf16x8*>(src + 2 * E + c);
    }
}

// The batched prefill's form of the copy above: the packed rows hold several prompts, token t of prompt b (bt.off[b] <= t <
// bt.off[b + 1]) is position t - off[b] of prompt slot bt.idx[b].  kplane / vplane: the layer's [slots][max_len][E] planes.
// One workgroup per token, 16 bytes per thread and copy.
__global__ __launch_bounds__(256) void chat_prompt_scatter_kernel(ChatBatch bt, const bf16_t* __restrict__ qkv, int ld, int E, int max_len,
                                                                  bf16_t* __restrict__ kplane, bf16_t* __restrict__ vplane) {
    const int t = blockIdx.x;
    int b = 0;
    while (b + 1 < bt.n && t >= bt.off[b + 1]) ++b;
    const bf16_t* src = qkv + (size_t)t * ld;
    const size_t dst = ((size_t)bt.idx[b] * max_len + (t - bt.off[b])) * E;
    for (int c = threadIdx.x * 8; c < E; c += 256 * 8) {
        *reinterpret_cast<bf16x8*>(kplane + dst + c) = *reinterpret_cast<const bf16x8*>(src + E + c);
        *reinterpret_cast<bf16x8*>(vplane + dst + c) = *reinterpret_cast<const bf16x8*>(src + 2 * E + c);
    }
}

// The last token of every packed prompt: out[bt.idx[b]] = bf16(h[off[b + 1] - 1] * rsqrt(mean(h^2) + eps) * w), w = the final
// norm's weight with the head's input scale folded in.  One workgroup per prompt.
__global__ __launch_bounds__(256) void chat_last_rows_kernel(ChatBatch bt, const float* __restrict__ h, int E, const float* __restrict__ w,
                                                             float eps, bf16_t* __restrict__ out) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* x = h + (size_t)(bt.off[b + 1] - 1) * E;
    float q = 0.f;
    for (int c = tid * 4; c < E; c += 256 * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + c);
        q += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    q = wave_sum(q);
    if ((tid & 63) == 0) red[tid >> 6] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / E + eps);
    bf16_t* dst = out + (size_t)bt.idx[b] * E;
    for (int c = tid * 4; c < E; c += 256 * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + c), ww = *reinterpret_cast<const f32x4*>(w + c);
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e] * rstd * ww[e]);
        *reinterpret_cast<bf16x4*>(dst + c) = o;
    }
}

// beam reordering: dir 0 copies the first len_i rows of every (layer, K|V) tail plane of row src_i to scratch slot i, dir 1
// copies scratch slot i to row dst_i (two passes: a row may be both a source and a destination).  Grid (2 * layers, n).
__global__ __launch_bounds__(256) void chat_tail_move_kernel(ChatMove mv, bf16_t* __restrict__ tails, bf16_t* __restrict__ scratch,
                                                             int max_rows, int max_new, int E, int max_tail, int dir) {
    const int lk = blockIdx.x, i = blockIdx.y;
    bf16_t* t = tails + cache_off(lk >> 1, lk & 1, dir == 0 ? mv.src[i] : mv.dst[i], max_rows, max_new, E);
    bf16_t* sc = scratch + ((size_t)i * gridDim.x + lk) * (size_t)max_tail * E;
    const size_t cnt = (size_t)mv.len[i] * E;
    for (size_t e = (size_t)threadIdx.x * 8; e < cnt; e += 256 * 8) {
        if (dir == 0) *reinterpret_cast<bf16x8*>(sc + e) = *reinterpret_cast<const bf16x8*>(t + e);
        else *reinterpret_cast<bf16x8*>(t + e) = *reinterpret_cast<const bf16x8*>(sc + e);
    }
}
__global__ __launch_bounds__(256) void chat_seen_move_kernel(ChatMove mv, unsigned* __restrict__ seen, unsigned* __restrict__ scratch,
                                                             int words, int dir) {
    const int i = blockIdx.x;
    unsigned* s = seen + (size_t)(dir == 0 ? mv.src[i] : mv.dst[i]) * words;
    unsigned* c = scratch + (size_t)i * words;
    for (int w = threadIdx.x; w < words; w += 256) {
        if (dir == 0) c[w] = s[w];
        else s[w] = c[w];
    }
}

// log-sum-exp of every selected row's logits (beam search: log_softmax = logit - lse), one workgroup per row
__global__ __launch_bounds__(256) void chat_lse_kernel(ChatSel sel, const float* __restrict__ logits, int ld, int V, float* __restrict__ lse) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const float* x = logits + (size_t)sel.lrow[blockIdx.x] * ld;
    float m = -INFINITY;
    for (int c = tid; c < V; c += 256) m = fmaxf(m, x[c]);
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int c = tid; c < V; c += 256) s += expf(x[c] - m);
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) lse[blockIdx.x] = m + logf((red[0] + red[1]) + (red[2] + red[3]));
}

// Top-K keys (score, -flat index) of group g's candidates: flat index f = r * V + tok over the group's rows.  Grid
// (CHAT_SEL_WGS, groups): workgroup w takes a slice of the flat range and finds its K best by K rounds of a max below the
// previous round's key (keys are distinct: the index is part of them).  Key 0 = no candidate; a score of -inf is none either.
__global__ __launch_bounds__(256) void chat_topk_partial_kernel(ChatSel sel, int mode, const float* __restrict__ logits, int ld, int V,
                                                                const unsigned* __restrict__ seen, int words, const float* __restrict__ lse,
                                                                float pen, int K, unsigned long long* __restrict__ part) {
    __shared__ unsigned long long red[4];
    const int g = blockIdx.y, w = blockIdx.x, tid = threadIdx.x;
    const int r0 = sel.g_lo[g], nb = sel.g_lo[g + 1] - r0;
    const unsigned total = (unsigned)nb * (unsigned)V, per = (total + CHAT_SEL_WGS - 1) / CHAT_SEL_WGS;
    const unsigned lo = min(total, w * per), hi = min(total, lo + per);
    unsigned long long* out = part + ((size_t)g * CHAT_SEL_WGS + w) * K;
    unsigned long long prev = ~0ull;
    for (int k = 0; k < K; ++k) {
        unsigned long long best = 0ull;
        for (unsigned f = lo + tid; f < hi; f += 256) {
            const int r = (int)(f / (unsigned)V), tok = (int)(f - (unsigned)r * V), i = r0 + r;
            const float x = logits[(size_t)sel.lrow[i] * ld + tok];
            const bool sn = (seen[(size_t)sel.srow[i] * words + (tok >> 5)] >> (tok & 31)) & 1u;
            const float s = chat_score(mode, x, sn, pen, mode == CHAT_SEL_BEAM ? lse[i] : 0.f, sel.bscore[i]);
            // (a score of -inf — a masked logit — is no candidate: key 0, like the end of the range)
            const unsigned long long key = s > -INFINITY ? ((unsigned long long)f2ord(s) << 32) | (unsigned)(~f) : 0ull;
            if (key < prev && key > best) best = key;
        }
        best = block_key_max(best, red);
        if (tid == 0) out[k] = best;
        prev = best;
    }
}

// The K best of the CHAT_SEL_WGS * K partial keys of group g, best first -> (score, token, parent row within the group).
// Sampling: one draw among those K (HF's top-k filter) from softmax(score / temperature) — Gumbel-max with counter noise.
__global__ __launch_bounds__(256) void chat_topk_final_kernel(const unsigned long long* __restrict__ part, int K, int mode, float inv_t,
                                                              unsigned long long seed, unsigned step, int V, int kout,
                                                              float* __restrict__ o_score, int* __restrict__ o_tok, int* __restrict__ o_par) {
    __shared__ unsigned long long red[4];
    __shared__ unsigned long long top[CHAT_TOPK_MAX];
    const int g = blockIdx.x, tid = threadIdx.x;
    const unsigned long long* src = part + (size_t)g * CHAT_SEL_WGS * K;
    const int n = CHAT_SEL_WGS * K;
    unsigned long long prev = ~0ull;
    for (int k = 0; k < K; ++k) {
        unsigned long long best = 0ull;
        for (int i = tid; i < n; i += 256) {
            const unsigned long long key = src[i];
            if (key < prev && key > best) best = key;
        }
        best = block_key_max(best, red);
        if (tid == 0) top[k] = best;
        prev = best;
    }
    __syncthreads();
    auto decode = [&](unsigned long long key, float& s, int& tok, int& par) {
        if (!key) { s = -INFINITY; tok = -1; par = -1; return; }
        const unsigned f = ~(unsigned)(key & 0xFFFFFFFFull);
        s = ord2f((unsigned)(key >> 32));
        par = (int)(f / (unsigned)V);
        tok = (int)(f - (unsigned)par * V);
    };
    if (mode != CHAT_SEL_SAMPLE) {
        if (tid < kout) {
            float s; int tok, par;
            decode(tid < K ? top[tid] : 0ull, s, tok, par);
            o_score[(size_t)g * kout + tid] = s; o_tok[(size_t)g * kout + tid] = tok; o_par[(size_t)g * kout + tid] = par;
        }
        return;
    }
    if (tid >= 64) return;
    float s = -INFINITY, v = -INFINITY;
    int tok = -1, par = -1;
    if (tid < K) {
        decode(top[tid], s, tok, par);
        if (tok >= 0) v = chat_noisy(s, inv_t, gumbel_noise(seed, step, (unsigned)tok));
    }
    // argmax over the lanes (ties: the lower lane = the better-ranked candidate)
    unsigned long long key = tok >= 0 ? ((unsigned long long)f2ord(v) << 32) | (unsigned)(~(unsigned)tid) : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) key = key_max(key, __shfl_xor(key, off, 64));
    // (no candidate at all — every score of the row -inf or NaN: lane 0 reports "none", its s / tok / par are then -inf, -1, -1)
    const int win = key ? (int)(~(unsigned)(key & 0xFFFFFFFFull)) : 0;
    if (tid == win) {
        for (int j = 0; j < kout; ++j) {
            o_score[(size_t)g * kout + j] = j == 0 ? s : -INFINITY;
            o_tok[(size_t)g * kout + j] = j == 0 ? tok : -1;
            o_par[(size_t)g * kout + j] = j == 0 ? par : -1;
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
hipError_t launch_chat_embed(const ChatStep& st, const void* table, int E, float scale, float* h, unsigned* seen, int words, hipStream_t s) {
    hipLaunchKernelGGL(chat_embed_kernel, dim3(st.n), dim3(256), 0, s, st, (const bf16_t*)table, E, scale, h, seen, words);
    return hipGetLastError();
}
hipError_t launch_chat_qkv(const ChatStep& st, const float* parts, int n_parts, size_t plane, int ldp, const float* rope, int E, int heads,
                           void* q_out, void* tails, int l, int max_rows, int max_new, hipStream_t s) {
    hipLaunchKernelGGL(chat_qkv_kernel, dim3(st.n, heads), dim3(96), 0, s, st, parts, n_parts, plane, ldp, rope, E, (bf16_t*)q_out,
                       (bf16_t*)tails, l, max_rows, max_new);
    return hipGetLastError();
}
int chat_step_groups(ChatStep& st, const int* slot_plen, int max_slots, int force_splits) {
    std::vector<char> slot_done(max_slots, 0);
    st.groups = 0;
    for (int i = 0; i < st.n; ++i) {
        const int sl = st.slot[i];
        if (i == 0 || st.slot[i - 1] != sl) {
            if (slot_done[sl]) return 0;
            slot_done[sl] = 1;
            st.g_lo[st.groups] = i;
            st.plen[st.groups] = slot_plen[sl];
            st.groups++;
        }
    }
    st.g_lo[st.groups] = st.n;
    int S = 1;                                           // prompt-key ranges of the attention: ~CHAT_KEYS keys each, per prompt
    for (int g = 0; g < st.groups; ++g) {
        st.gsplit[g] = force_splits > 0 ? std::min(CHAT_ATT_SPLITS, force_splits)
                                        : std::min(CHAT_ATT_SPLITS, std::max(1, (st.plen[g] + CHAT_KEYS - 1) / CHAT_KEYS));
        S = std::max(S, st.gsplit[g]);
        for (int i = st.g_lo[g]; i < st.g_lo[g + 1]; ++i) st.rsplit[i] = st.gsplit[g];
    }
    return S;
}
hipError_t launch_chat_attn(const ChatStep& st, const void* q, const void* prompt, const void* tails, int l, int E, int heads,
                            const ChatCaps& cap, int S_max, float* po, float* pml, void* att, hipStream_t s) {
    if (S_max < 1 || S_max > CHAT_ATT_SPLITS || st.groups < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chat_attn_kernel, dim3(heads, st.groups, S_max), dim3(256), 0, s, st, (const bf16_t*)q, (const bf16_t*)prompt,
                       (const bf16_t*)tails, l, E, cap, S_max, po, pml);
    hipLaunchKernelGGL(chat_attn_combine_kernel, dim3(st.n, heads), dim3(64), 0, s, st, (const float*)po, (const float*)pml, E, (bf16_t*)att);
    return hipGetLastError();
}
hipError_t launch_chat_prompt_kv(const void* qkv, int ld, int T, int E, void* kdst, void* vdst, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    if (E % 8 || ld % 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chat_prompt_kv_kernel, dim3(T), dim3(256), 0, s, (const bf16_t*)qkv, ld, E, (bf16_t*)kdst, (bf16_t*)vdst);
    return hipGetLastError();
}
hipError_t launch_chat_prompt_scatter(const ChatBatch& bt, const void* qkv, int ld, int E, int max_len, void* kplane, void* vplane,
                                      hipStream_t s) {
    if (bt.n < 1 || bt.n > CHAT_MAX_ROWS || bt.off[0] != 0 || E % 8 || ld % 8 || ld < 3 * E) return hipErrorInvalidValue;
    for (int b = 0; b < bt.n; ++b)
        if (bt.off[b + 1] <= bt.off[b] || bt.off[b + 1] - bt.off[b] > max_len || bt.idx[b] < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chat_prompt_scatter_kernel, dim3(bt.off[bt.n]), dim3(256), 0, s, bt, (const bf16_t*)qkv, ld, E, max_len,
                       (bf16_t*)kplane, (bf16_t*)vplane);
    return hipGetLastError();
}
hipError_t launch_chat_last_rows(const ChatBatch& bt, const float* h, int E, const float* w, float eps, void* out, hipStream_t s) {
    if (bt.n < 1 || bt.n > CHAT_MAX_ROWS || E % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chat_last_rows_kernel, dim3(bt.n), dim3(256), 0, s, bt, h, E, w, eps, (bf16_t*)out);
    return hipGetLastError();
}
hipError_t launch_chat_move(const ChatMove& mv, void* tails, void* scratch, int layers, int max_rows, int max_new, int E, int max_tail,
                            unsigned* seen, unsigned* seen_scratch, int words, hipStream_t s) {
    if (mv.n <= 0) return hipSuccess;
    for (int dir = 0; dir < 2; ++dir) {
        if (max_tail > 0)
            hipLaunchKernelGGL(chat_tail_move_kernel, dim3(2 * layers, mv.n), dim3(256), 0, s, mv, (bf16_t*)tails, (bf16_t*)scratch, max_rows,
                               max_new, E, max_tail, dir);
        hipLaunchKernelGGL(chat_seen_move_kernel, dim3(mv.n), dim3(256), 0, s, mv, seen, seen_scratch, words, dir);
    }
    return hipGetLastError();
}
hipError_t launch_chat_select(const ChatSel& sel, int mode, const float* logits, int ld, int V, const unsigned* seen, int words, float pen,
                              float temperature, int K, int kout, unsigned long long seed, unsigned step, float* lse,
                              unsigned long long* part, float* o_score, int* o_tok, int* o_par, hipStream_t s) {
    if (K < 1 || K > CHAT_TOPK_MAX || kout < 1 || kout > CHAT_TOPK_MAX || sel.groups < 1) return hipErrorInvalidValue;
    if (mode == CHAT_SEL_BEAM)
        hipLaunchKernelGGL(chat_lse_kernel, dim3(sel.n), dim3(256), 0, s, sel, logits, ld, V, lse);
    hipLaunchKernelGGL(chat_topk_partial_kernel, dim3(CHAT_SEL_WGS, sel.groups), dim3(256), 0, s, sel, mode, logits, ld, V, seen, words,
                       (const float*)lse, pen, K, part);
    const float inv_t = temperature > 0.f ? 1.0f / temperature : 1.0f;
    hipLaunchKernelGGL(chat_topk_final_kernel, dim3(sel.groups), dim3(256), 0, s, (const unsigned long long*)part, K, mode, inv_t, seed, step,
                       V, kout, o_score, o_tok, o_par);
    return hipGetLastError();
}

}  // namespace vr
