// Several given tokens appended to cached prompts in ONE packed pass (vr_chat_extend, chat.hip): the attention whose keys are
// "the slot's prompt plane, then the row's tail plane, causal inside the tail", the tail-plane twin of the prompt scatter, and
// the reduction of a finished logits row to the four numbers of the fused scoring head.
//
// The attention (DESIGN.md section 4 has the choices): bf16 MFMA flash form of attention_body.h — S^T = K Q^T on 16x16x32
// MFMAs, online softmax in the exp2 domain, P rounded to bf16 for O^T += V^T P^T, fp32 accumulators — with 16 query rows per
// wave, 64 per workgroup, 64 keys per LDS tile staged through registers one tile ahead.  A workgroup walks the prompt tiles,
// then the tail tiles up to its last query's own key.  Masked scores are SELECTED to -inf (a masked tail row may hold any
// finite K); this file is built without -fno-honor-nans, so the selects and the fmaxf / exp2 of -inf stay as written.
#include <algorithm>

#include "attention_body.h"

namespace vr {

namespace {

constexpr int EXT_PITCH = AttnCfg<64>::PITCH;   // bytes per key row in LDS (128 of data + 32 of padding: conflict-free fragment reads)

__device__ __forceinline__ size_t ext_cache_off(int l, int kv, int idx, int count, int cap, int E) {
    return (((size_t)l * 2 + kv) * count + idx) * (size_t)cap * E;
}

}  // namespace

__global__ __launch_bounds__(256) void chat_extend_attn_kernel(ChatExtend sq, const bf16_t* __restrict__ q, int ldq,
                                                               const bf16_t* __restrict__ prompt, const bf16_t* __restrict__ tails, int l,
                                                               int E, ChatCaps cap, bf16_t* __restrict__ out, int ldo) {
    __shared__ __attribute__((aligned(16))) char Ks[ATT_KV * EXT_PITCH];
    __shared__ __attribute__((aligned(16))) char Vs[ATT_KV * EXT_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, qs = blockIdx.x * CHAT_EXT_QT;
    const int row0 = sq.off[b], n = sq.off[b + 1] - row0;
    if (qs >= n) return;                                   // (uniform over the workgroup)
    const int plen = sq.plen[b], t0 = sq.t0[b];
    const int tail_end = t0 + min(n, qs + CHAT_EXT_QT);    // tail keys any query of this tile may see: [0, tail_end)
    const bf16_t* pk = prompt + ext_cache_off(l, 0, sq.slot[b], cap.slots, cap.len, E) + h * 64;
    const bf16_t* pv = prompt + ext_cache_off(l, 1, sq.slot[b], cap.slots, cap.len, E) + h * 64;
    const bf16_t* tk = tails + ext_cache_off(l, 0, sq.row[b], cap.rows, cap.tail, E) + h * 64;
    const bf16_t* tv = tails + ext_cache_off(l, 1, sq.row[b], cap.rows, cap.tail, E) + h * 64;
    const int np = (plen + ATT_KV - 1) / ATT_KV, nt = (tail_end + ATT_KV - 1) / ATT_KV;

    // ---- Q fragments (B operand of S^T): lane holds Q[q = fr][d = ks * 32 + fq * 8 .. + 7]; rows past n are zero
    const int qrow = qs + wave * 16 + fr;                  // this lane's query (sequence-relative)
    bf16x8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        u32x4 raw = {0, 0, 0, 0};
        if (qrow < n) raw = *reinterpret_cast<const u32x4*>(q + (size_t)(row0 + qrow) * ldq + h * 64 + ks * 32 + fq * 8);
        qf[ks] = __builtin_bit_cast(bf16x8, raw);
    }

    // ---- staging: tile t < np is prompt keys [t * 64, + 64), the others tail keys; every thread moves two 16-byte chunks of K
    //      and of V; a key at or past the segment's end is not read: its LDS row is zero
    u32x4 rk[2], rv[2];
    auto fetch = [&](int t) {
        const bool in_prompt = t < np;
        const bf16_t* kb = in_prompt ? pk : tk;
        const bf16_t* vb = in_prompt ? pv : tv;
        const int key0 = (in_prompt ? t : t - np) * ATT_KV, end = in_prompt ? plen : tail_end;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + i * 256, key = key0 + (c >> 3), ch = c & 7;
            rk[i] = u32x4{0, 0, 0, 0}; rv[i] = u32x4{0, 0, 0, 0};
            if (key < end) {
                rk[i] = *reinterpret_cast<const u32x4*>(kb + (size_t)key * E + ch * 8);
                rv[i] = *reinterpret_cast<const u32x4*>(vb + (size_t)key * E + ch * 8);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + i * 256;
            *reinterpret_cast<u32x4*>(Ks + (c >> 3) * EXT_PITCH + (c & 7) * 16) = rk[i];
            *reinterpret_cast<u32x4*>(Vs + (c >> 3) * EXT_PITCH + (c & 7) * 16) = rv[i];
        }
    };

    f32x4 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const float sc = 0.125f * 1.44269504088896340736f;     // scale 1/8, exp2 domain
    const int k_off = fr * EXT_PITCH + fq * 16;
    const int v_off = (fq * 4 + (fr >> 2)) * EXT_PITCH + (fr & 3) * 8;

    fetch(0);
    for (int t = 0; t < np + nt; ++t) {
        if (t) __syncthreads();                            // the previous tile is consumed
        stage();
        __syncthreads();
        if (t + 1 < np + nt) fetch(t + 1);                 // in flight during the MFMAs below

        // S^T = K Q^T: lane holds s[kf][r] = score(key kf * 16 + fq * 4 + r, query fr)
        f32x4 s[4];
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) {
            s[kf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 ka = *reinterpret_cast<const bf16x8*>(Ks + kf * 16 * EXT_PITCH + k_off + ks * 64);
                s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[ks], s[kf], 0, 0, 0);
            }
        }
        // mask by selection: a prompt key exists below plen; tail key k is visible to query j when k <= t0 + j
        const bool in_prompt = t < np;
        const int key0 = (in_prompt ? t : t - np) * ATT_KV;
        const int lim = in_prompt ? plen - 1 : t0 + qrow;  // last visible key of this segment
        float mx = -INFINITY;
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kf][r] = key0 + kf * 16 + fq * 4 + r <= lim ? s[kf][r] : -INFINITY;
                mx = fmaxf(mx, s[kf][r]);
            }
        mx = col4_max(mx);
        // online softmax; key 0 of the prompt is visible to every query, so m_new is finite from the first tile on
        const float m_new = fmaxf(m_run, mx * sc);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);      // (first tile: exp2(-inf) = 0 on zeros)
        m_run = m_new;
        float rs = 0.f;
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kf][r] = __builtin_amdgcn_exp2f(fmaf(s[kf][r], sc, -m_new));
                rs += s[kf][r];
            }
        l_run = l_run * alpha + col4_sum(rs);
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] *= alpha;
        // O^T += V^T P^T: B operand k-slot fq * 8 + i = key (2 ks) * 16 + fq * 4 + i (i < 4), (2 ks + 1) * 16 + fq * 4 + i - 4
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 pb;
#pragma unroll
            for (int r = 0; r < 4; ++r) { pb[r] = f2bf(s[2 * ks][r]); pb[4 + r] = f2bf(s[2 * ks + 1][r]); }
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const char* vr = Vs + v_off + ks * 32 * EXT_PITCH + d * 32;
                const bf16x8 va = __builtin_shufflevector(lds_tr_read(vr), lds_tr_read(vr + 16 * EXT_PITCH), 0, 1, 2, 3, 4, 5, 6, 7);
                o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, o[d], 0, 0, 0);
            }
        }
    }

    // ---- normalise and store: lane owns out[query fr][h * 64 + d * 16 + fq * 4 .. + 3]
    if (qrow < n) {
        const float inv = 1.0f / l_run;
        bf16_t* orow = out + (size_t)(row0 + qrow) * ldo + h * 64;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            bf16x4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = f2bf(o[d][r] * inv);
            *reinterpret_cast<bf16x4*>(orow + d * 16 + fq * 4) = ov;
        }
    }
}

// The tail-plane twin of chat_prompt_scatter_kernel: packed token t of sequence b goes to tail index t0[b] + t - off[b] of tail
// row row[b].  kplane / vplane: the layer's [rows][max_new][E] planes.  One workgroup per token, 16 bytes per thread and copy.
__global__ __launch_bounds__(256) void chat_tail_scatter_kernel(ChatExtend ex, const bf16_t* __restrict__ qkv, int ld, int E, int max_new,
                                                                bf16_t* __restrict__ kplane, bf16_t* __restrict__ vplane) {
    const int t = blockIdx.x;
    int b = 0;
    while (b + 1 < ex.n && t >= ex.off[b + 1]) ++b;
    const bf16_t* src = qkv + (size_t)t * ld;
    const size_t dst = ((size_t)ex.row[b] * max_new + (ex.t0[b] + t - ex.off[b])) * E;
    for (int c = threadIdx.x * 8; c < E; c += 256 * 8) {
        *reinterpret_cast<bf16x8*>(kplane + dst + c) = *reinterpret_cast<const bf16x8*>(src + E + c);
        *reinterpret_cast<bf16x8*>(vplane + dst + c) = *reinterpret_cast<const bf16x8*>(src + 2 * E + c);
    }
}

// One workgroup per entry over an fp32 logits row: the largest logit and its lowest id, log sum exp, the logit of the target.
__global__ __launch_bounds__(256) void chat_row_score_kernel(ChatRowScore sc, const float* __restrict__ logits, int ld, int V,
                                                             float* __restrict__ x_t, float* __restrict__ lse, float* __restrict__ top_x,
                                                             int* __restrict__ top_id) {
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ float red_s[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (size_t)sc.lrow[i] * ld;
    float best = -INFINITY;
    int id = 0x7fffffff;
    for (int c = tid; c < V; c += 256) {                   // ascending ids: a strict test keeps the thread's lowest
        const float v = x[c];
        if (v > best || id == 0x7fffffff) { best = v; id = c; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(id, off, 64);
        if (ov > best || (ov == best && oi < id)) { best = ov; id = oi; }
    }
    if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_i[tid >> 6] = id; }
    __syncthreads();
    best = red_v[0]; id = red_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (red_v[w] > best || (red_v[w] == best && red_i[w] < id)) { best = red_v[w]; id = red_i[w]; }
    float sum = 0.f;
    for (int c = tid; c < V; c += 256) sum += expf(x[c] - best);
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red_s[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        lse[i] = best + logf((red_s[0] + red_s[1]) + (red_s[2] + red_s[3]));
        top_x[i] = best;
        top_id[i] = id;
        const int tg = sc.target[i];
        if (tg >= 0 && tg < V) x_t[i] = x[tg];
    }
}

hipError_t launch_chat_extend_attn(const ChatExtend& ex, const void* q, int ldq, const void* prompt, const void* tails, int l, int E,
                                   int heads, const ChatCaps& cap, void* out, int ldo, hipStream_t s) {
    if (ex.n < 1 || ex.n > CHAT_MAX_ROWS || heads < 1 || heads * 64 > E || ldq % 8 || E % 8 || ldo % 4) return hipErrorInvalidValue;
    int max_n = 0;
    for (int b = 0; b < ex.n; ++b) max_n = std::max(max_n, ex.off[b + 1] - ex.off[b]);
    if (max_n < 1) return hipErrorInvalidValue;
    const dim3 grid((max_n + CHAT_EXT_QT - 1) / CHAT_EXT_QT, heads, ex.n);
    hipLaunchKernelGGL(chat_extend_attn_kernel, grid, dim3(256), 0, s, ex, (const bf16_t*)q, ldq, (const bf16_t*)prompt,
                       (const bf16_t*)tails, l, E, cap, (bf16_t*)out, ldo);
    return hipGetLastError();
}

hipError_t launch_chat_tail_scatter(const ChatExtend& ex, const void* qkv, int ld, int E, int max_new, void* kplane, void* vplane,
                                    hipStream_t s) {
    if (ex.n < 1 || ex.n > CHAT_MAX_ROWS || ex.off[ex.n] < 1 || E % 8 || ld % 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chat_tail_scatter_kernel, dim3(ex.off[ex.n]), dim3(256), 0, s, ex, (const bf16_t*)qkv, ld, E, max_new,
                       (bf16_t*)kplane, (bf16_t*)vplane);
    return hipGetLastError();
}

hipError_t launch_chat_row_score(const ChatRowScore& sc, const float* logits, int ld, int V, float* x_t, float* lse, float* top_x,
                                 int* top_id, hipStream_t s) {
    if (sc.n < 1 || sc.n > CHAT_ROW_SCORE_MAX || V < 1 || ld < V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chat_row_score_kernel, dim3(sc.n), dim3(256), 0, s, sc, logits, ld, V, x_t, lse, top_x, top_id);
    return hipGetLastError();
}

}  // namespace vr
