// vr_index_rank_rows / vr_index_count_range: WHERE a named row stands in a query's fp32 ranking, and HOW MANY rows reach a
// threshold — exact counts, no row lists.  A pair is (query, bar): the bar of a rank is the 64-bit key make_key(e, id) of the
// target row (e its fp32 score: dot_lane + wave_sum, the bits vr_index_search returns for that (query, row)), the bar of a count
// is the threshold t.  With b_j the bf16-MFMA score of row j, e_j its fp32 score and |b_j - e_j| <= eps (search_common.h:
// query_eps), a row with b_j > t + eps lies certainly ahead of the bar and one with b_j < t - eps certainly behind it (t = e for
// a rank): only the rows of the band between need their fp32 dot product.  No candidate margin, no widening, no flagged queries;
// exact under the conditions of the range search (search_range.hip).  Per block of <= 256 queries (index_searches.hip):
//   1. score rows S[q][row] on the bf16 MFMA GEMM (the deep path's launch); with filters launch_filter_mask turns the columns a
//      query may not see into -inf: below every finite bar, never counted;
//   2. rank_bar_kernel, one wave per pair: eps of the pair's query; for a rank the target's fp32 score from the fp32 store ->
//      out_scores and the bar key; for a count the bar is the threshold (-0.0 taken as +0.0); the pair's count starts at 0.  A
//      filter index outside [-1, n_filters) (a device caller's: it cannot be seen before the launch) leaves the count at 0;
//   3. rank_count_kernel, one workgroup per (column chunk of 4096, pair): lo = one_ulp_down(t - eps), hi = the next float above
//      t + eps.  b > hi: counted from the bf16 score alone; b < lo: skipped; the columns in [lo, hi] are compacted into an LDS
//      list (search_rescore.h: chunk_scan) and re-scored one candidate per wave, the row's loads issued in front of the fma
//      chain (search_common.h: exact_row_score; profiles/diverse_search_bench.txt): a rank compares keys (score descending, then lower id
//      first), a count compares floats (>= t, or > t when strict).  The target lies in its own band and compares equal: it never
//      counts itself.  S is only read — several pairs share a score row.  The workgroup's total is added to the pair's 64-bit
//      count: integer adds commute, the result does not depend on the order; no workgroup waits for another.
// Pairs are laid along the grid's x dimension (chunk fastest), a launch holds at most 2^22 workgroups: no pair count is assumed
// to fit a grid's y or z.  No kernel looks at or past column n_docs of a score row: the padded columns hold zeros.
#include "kernels.h"
#include "search_rescore.h"

namespace vr {

constexpr int64_t RANK_MAX_WGS = (int64_t)1 << 22;   // workgroups per launch of the counting kernel

__global__ __launch_bounds__(256) void rank_bar_kernel(RankSearchArgs p, int n_pairs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SearchArgs& a = p.a;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&p.stats[0], (unsigned long long)n_pairs);
    const int pair = blockIdx.x * 4 + wave;
    if (pair >= n_pairs) return;                                           // (wave-uniform; no barrier below)
    const int q = p.pair_query[pair], nv = a.dim >> 2;
    f32x4 qv[MERGE_MAXV];
    load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
    float eps = query_eps(a, qv);
    // a filter index out of range: nothing is allowed, the count stays 0
    if (!filter_index_ok(p.filter_of_query ? p.filter_of_query[q] : -1, p.n_filters)) eps = __builtin_nanf("");
    unsigned long long bar;
    if (p.pair_id) {
        const uint32_t id = (uint32_t)p.pair_id[pair];                     // (in [0, n_docs): the host checked it)
        const float e = wave_sum(dot_lane(qv, a.index_f32 + (size_t)id * a.dim, nv, lane));
        bar = make_key(e, id);
        if (lane == 0) p.out_scores[pair] = e;
    } else {
        const float t = p.pair_thr[pair];
        bar = (unsigned long long)__float_as_uint(t == 0.f ? 0.f : t);     // -0.0 counts as +0.0
    }
    if (lane == 0) {
        p.bars[pair] = bar;
        p.bar_eps[pair] = eps;
        p.out_counts[pair] = 0ull;
    }
}

__global__ __launch_bounds__(256) void rank_count_kernel(RankSearchArgs p, const float* __restrict__ S, size_t ldS, int pair0,
                                                         int chunks) {
    __shared__ ChunkLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int pair = pair0 + (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    const float eps = p.bar_eps[pair];
    if (eps != eps) return;                                                // (workgroup-uniform) a filter index out of range
    const int q = p.pair_query[pair], n_docs = (int)a.n_docs, nv = a.dim >> 2;
    const int c0 = chunk * RESCORE_CHUNK, c1 = min(c0 + RESCORE_CHUNK, n_docs);
    const unsigned long long bar = p.bars[pair];
    const bool by_key = p.pair_id != nullptr;
    const float t = by_key ? key_score(bar) : __uint_as_float((uint32_t)bar);
    const float lo = one_ulp_down(t - eps), hi = one_ulp_up(t + eps);
    // ---- certainly ahead: b > hi; the band: lo <= b <= hi (a masked column is -inf, lo is finite)
    unsigned mine = chunk_scan<4, false>(S + (size_t)q * ldS, c0, c1, lo, hi, L);   // rows ahead of the bar this wave found
    __syncthreads();
    // ---- fp32 re-scoring of the band, one candidate per wave
    const int m = L.n_cand;
    if (m > 0) {                                                           // (workgroup-uniform)
        f32x4 qv[MERGE_MAXV];
        load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
        for (int c = wave; c < m; c += 4) {
            const int id = L.cand[c];
            const float s = exact_row_score(a, qv, id, nv, lane);
            const bool ahead = by_key ? make_key(s, (uint32_t)id) > bar : (p.strict ? s > t : s >= t);
            mine += ahead ? 1u : 0u;                                       // (every lane holds the same s)
        }
    }
    if (lane == 0 && mine) atomicAdd(&L.ahead, mine);
    __syncthreads();
    if (tid == 0) {
        if (m > 0) atomicAdd(&p.stats[1], (unsigned long long)m);
        const unsigned n = L.ahead;
        if (n > 0) {
            atomicAdd(&p.out_counts[pair], (unsigned long long)n);
            atomicAdd(&p.stats[2], (unsigned long long)n);
        }
    }
}

static bool rank_args_ok(const RankSearchArgs& p, size_t ldS, int nq_block, int64_t n_pairs) {
    return rescore_args_ok(p.a, nq_block) && n_pairs >= 1 && n_pairs < ((int64_t)1 << 31) && p.pair_query &&
           ((p.pair_id != nullptr) != (p.pair_thr != nullptr)) && (!p.pair_id || p.out_scores) && p.bars && p.bar_eps &&
           p.out_counts && p.stats && ldS % 4 == 0 && (int64_t)ldS >= p.a.n_docs && (!p.filter_of_query || p.n_filters >= 1);
}

hipError_t launch_rank_bars(const RankSearchArgs& p, size_t ldS, int nq_block, int64_t n_pairs, hipStream_t s) {
    if (!rank_args_ok(p, ldS, nq_block, n_pairs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rank_bar_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0, s, p, (int)n_pairs);
    return hipGetLastError();
}

hipError_t launch_rank_count(const RankSearchArgs& p, const float* S, size_t ldS, int nq_block, int64_t n_pairs, hipStream_t s) {
    if (!rank_args_ok(p, ldS, nq_block, n_pairs) || !S) return hipErrorInvalidValue;
    const int64_t chunks = (p.a.n_docs + RESCORE_CHUNK - 1) / RESCORE_CHUNK;
    const int64_t per_launch = RANK_MAX_WGS / chunks;                      // (chunks < 2^19: at least 8 pairs)
    for (int64_t p0 = 0; p0 < n_pairs; p0 += per_launch) {
        const int64_t np = n_pairs - p0 < per_launch ? n_pairs - p0 : per_launch;
        hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)(np * chunks)), dim3(256), 0, s, p, S, ldS, (int)p0, (int)chunks);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace vr
