// vr_index_search for k > 26 (the reference's --retrieve_depth is free: eval.sh uses 10, TREC runs
// are commonly 100 or 1000 deep) and the matching multi-GPU merge for k > 64.
//
// The fused sweeps keep one wave-wide candidate list per (query, chunk), which bounds k at 26.
// Deep retrieval is not the throughput case, so it takes the plain route, exact all the same:
//   1. scores S[q][doc] of a block of <= 256 queries against the whole index with the bf16 MFMA
//      GEMM (EPI_F32), the same arithmetic the sweeps use;
//   2. per query (one workgroup): the K' = k + 24 best bf16 scores in row order (search_select.h: radix select of the
//      K'-th largest, then every key above it and the lowest ids among its ties) — the margin keeps a true top-k row
//      inside the candidate set although S carries bf16 rounding;
//   3. re-score the candidates against the fp32 index (exact fp32 dots: dot_lane), bitonic-sort the keys (score desc,
//      id asc) in LDS;
//   4. certify as the fused path does (search_common.h): if the K'-th bf16 score is not below
//      tau = s_k - eps, gather and re-score EVERY row with a bf16 score >= tau (<= 1024), else
//      flag the query for the exact fp32 pass; emit the top k.
#include <algorithm>

#include "kernels.h"
#include "search_select.h"

namespace vr {

int search_bigk_max() { return SEL_CAND - SEL_MARGIN; }

// exact == 0: S rows are bf16-MFMA scores of queries blockIdx.x; the result is certified like the fused path's
//   (search_common.h): tau = s_k - eps; if the radix threshold T does not lie below tau, every row with a bf16 score
//   >= tau is gathered and re-scored instead (up to SEL_CAND of them), else the query is flagged.
// exact == 1: S row i holds EXACT fp32 scores of flagged query flag_list[i] (search_exact.hip); plain top-k of it.
__global__ __launch_bounds__(256) void bigk_select_kernel(SearchArgs p, const float* __restrict__ S, size_t ldS, int kp_want,
                                                          int exact, int sub, int max_slots) {
    __shared__ SelectLds L;
    const int tid = threadIdx.x, lane = tid & 63;
    // exact: a fixed grid walks entries [sub, sub + max_slots) of the flag list
    const int n_slots = exact ? flag_slots(p.flag_count, sub, max_slots) : (int)gridDim.x;
    for (int slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
    const int q = exact ? p.flag_list[sub + slot] : slot;
    const float* row = S + (size_t)slot * ldS;
    const int n_docs = (int)p.n_docs, k = p.k, dim = p.dim;
    __syncthreads();                                                    // (LDS of the previous slot is free)

    // ---- 2.-4. candidates, exact fp32 re-scoring, certification (search_select.h: certified_select; rows outside the re-scored
    // set have a bf16 score <= the K'-th).  A NaN score sorts last: never a candidate before a number, and never ranks.
    int kp = min(n_docs, kp_want);
    const KthKey kth = top_positions<true>(row, n_docs, kp, L);
    const int nv = dim >> 2;
    f32x4 qv[MERGE_MAXV];
    load_query_regs(qv, p.q_f32 + (size_t)q * dim, nv, lane);
    const bool certify = !exact && (p.eps_data || p.eps_rel >= 0.f);
    int what;
    float tau;
    kp = certified_select<true, false>(
        row, n_docs, n_docs, kp, kth.T, k, certify,
        [&](int id) { return make_key_ranked(wave_sum(dot_lane(qv, p.index_f32 + (size_t)id * dim, nv, lane)), (uint32_t)id); },
        [&] { return query_eps(p, qv); }, L, &what, &tau);
    if (certify) {
        if (tid == 0 && p.stats) atomicAdd(&p.stats[what], 1u);
        __syncthreads();
        flag_query(p, q, what == 2, tau, &L.rank);
    } else if (!exact && tid == 0 && p.stats) {
        atomicAdd(&p.stats[3], 1u);
    }
    for (int c = tid; c < k; c += 256) emit_slot(p, q, c, c < kp ? L.keys[c] : KEY_NONE);
    }
}

// a block of nq_block queries of the call: S holds their bf16-MFMA scores, one row of ldS floats each.
// `a` is the BLOCK's view (q_f32 / outputs / flag lists start at the block's first query).
hipError_t launch_search_bigk(const SearchArgs& a, const float* S, size_t ldS, int nq_block, hipStream_t s) {
    if (nq_block <= 0) return hipSuccess;
    if (a.k > search_bigk_max() || a.dim % 4 || a.dim > 64 * 4 * MERGE_MAXV) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bigk_select_kernel, dim3(nq_block), dim3(256), 0, s, a, S, ldS, a.k + SEL_MARGIN, 0, 0, 0);
    return hipGetLastError();
}

// exact top-k of the flagged queries from their exact score rows (slot i of S = query flag_list[i])
hipError_t launch_exact_select(const SearchArgs& a, const float* S, size_t ldS, int sub, int max_slots, hipStream_t s) {
    if (max_slots <= 0) return hipSuccess;
    if (a.k > SEL_CAND || a.dim % 4 || a.dim > 64 * 4 * MERGE_MAXV || !a.flag_count || !a.flag_list) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bigk_select_kernel, dim3(max_slots < 128 ? max_slots : 128), dim3(256), 0, s, a, S, ldS, a.k, 1, sub, max_slots);
    return hipGetLastError();
}

// ---- multi-GPU merge for k > 64: one workgroup per query, all n_parts * k keys sorted in LDS --------
constexpr int MERGE_BIG_MAX = 8192;

__global__ __launch_bounds__(256) void topk_merge_big_kernel(const float* __restrict__ scores,
                                                             const int64_t* __restrict__ ids,
                                                             const unsigned long long* __restrict__ pk, int n_parts,
                                                             int nq, int k, int n2, float* __restrict__ out_scores,
                                                             int64_t* __restrict__ out_ids) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem_raw);
    const int q = blockIdx.x, tid = threadIdx.x;
    const int total = n_parts * k;
    for (int e = tid; e < n2; e += 256) {
        uint64_t key = KEY_NONE;
        if (e < total) {
            const int part = e / k, sidx = e % k;
            const size_t o = ((size_t)part * nq + q) * k + sidx;
            if (pk) key = pk[o];
            else if (ids[o] >= 0) key = make_key(scores[o], (uint32_t)ids[o]);
        }
        keys[e] = key;
    }
    __syncthreads();
    block_bitonic_desc(keys, n2, tid, 256);
    for (int c = tid; c < k; c += 256) {
        const uint64_t key = keys[c];
        const bool ok = key != KEY_NONE;
        out_scores[(size_t)q * k + c] = ok ? orderable_f32((uint32_t)(key >> 32)) : -INFINITY;
        out_ids[(size_t)q * k + c] = ok ? (int64_t)(~(uint32_t)key) : (int64_t)-1;
    }
}

hipError_t launch_topk_merge_any(const float* scores, const int64_t* ids, const unsigned long long* pk, int n_parts, int nq,
                                 int k, float* out_scores, int64_t* out_ids, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    const long total = (long)n_parts * k;
    if (k <= 0 || total > MERGE_BIG_MAX) return hipErrorInvalidValue;
    int n2 = 64;
    while (n2 < total) n2 <<= 1;
    static unsigned long long attr = 0;     // bit d: set on device d
    set_max_dynamic_lds((const void*)topk_merge_big_kernel, MERGE_BIG_MAX * 8, attr);
    hipLaunchKernelGGL(topk_merge_big_kernel, dim3(nq), dim3(256), (size_t)n2 * 8, s, scores, ids, pk, n_parts, nq, k, n2,
                       out_scores, out_ids);
    return hipGetLastError();
}

hipError_t launch_topk_merge_big(const float* scores, const int64_t* ids, int n_parts, int nq, int k, float* out_scores,
                                 int64_t* out_ids, hipStream_t s) {
    return launch_topk_merge_any(scores, ids, nullptr, n_parts, nq, k, out_scores, out_ids, s);
}

}  // namespace vr
