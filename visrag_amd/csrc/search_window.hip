// vr_index_search_window: WHICH rows stand at ranks [o, o + k) of a query's fp32 ranking (fp32 score descending, then lower id
// first, over the rows the query's filter allows) — the inverse of vr_index_rank_rows, any offset o, k <= search_bigk_max().
// Let b_j be row j's bf16-MFMA score, e_j its fp32 score (dot_lane + wave_sum, the bits vr_index_search returns for that pair)
// and |b_j - e_j| <= eps for every allowed j (search_common.h: query_eps).  Order statistics are 1-Lipschitz under a sup-norm
// perturbation: with b_(r) the r-th largest bf16 score and e_(r) the r-th largest fp32 score, |b_(r) - e_(r)| <= eps for every
// rank r.  With na the allowed rows, v_a = b_(o + 1) and v_z = b_(min(o + k, na)):
//   - every row of the window has e in [v_z - eps, v_a + eps], hence b in [v_z - 2 eps, v_a + 2 eps]: the BAND;
//   - a row with b > v_a + 2 eps has e > v_a + eps >= e_(o + 1): strictly ahead of the whole window, whatever its id;
//   - a row with b < v_z - 2 eps is strictly behind the whole window.
// With A the rows certainly ahead (A <= o always: fewer than o + 1 rows have b > b_(o + 1)), the window is positions
// o - A .. o - A + k - 1 of the band rows sorted by make_key(e, id).  Both bounds are rounded outward by one ulp (the rounded
// subtraction / addition cannot have narrowed the band).  No candidate margin, no widening, no flagged queries; with
// certification off the default error model defines the band.  Per block of <= 256 queries (index_searches.hip):
//   1. score rows S[q][row] on the bf16 MFMA GEMM (the deep path's launch); with filters launch_filter_mask turns the columns a
//      query may not see into -inf;
//   2. window_edge_kernel, one workgroup per query: eps, na; o >= na (or a filter index outside [-1, n_filters), which a device
//      caller's cannot be checked for before the launch): the query is empty (lo = NaN).  Otherwise two radix selects over the
//      row give v_a and v_z (both ranks <= na: neither is a masked -inf) and lo = one_ulp_down(v_z - 2 eps), hi = the next
//      float above v_a + 2 eps;
//   3. window_rescore_kernel, grid (column chunk of 4096, query): the row is REWRITTEN in place so that it alone defines the
//      answer: +inf for b > hi (certainly ahead), -inf for b < lo (certainly behind, or masked), and for the columns in
//      [lo, hi] — compacted into an LDS list (search_rescore.h: chunk_scan), re-scored one candidate per wave with the row's loads
//      issued in front of the fma chain (exact_row_score; profiles/diverse_search_bench.txt) — their fp32 score e.  The A rows of +inf then occupy
//      ranks 0 .. A - 1 of the rewritten row (id order), every band row stands where its key puts it, and the window is ranks
//      o .. o + k - 1 of the rewritten row: no per-query counter to subtract.  A column is written by one thread only;
//   4. window_select_kernel, one workgroup per query: radix selects for rank o (when o > 0) and rank min(o + k, na) of the
//      rewritten row, then gather_window: the positions NOT among the first o and among the first o + k, "lowest ids first
//      among equals" being the tie rule at both edges (T_a == T_z: both edges inside one tie tier, equal-positions
//      [need_a, need_z)).  At most k <= 1000 positions: keys make_key(S[i], i), block_bitonic_desc, k slots emitted,
//      (-inf, -1) past the allowed rows.
// No kernel waits for another workgroup; stream order between the launches is the only ordering.  No kernel reads a column at
// or past n_docs as a value or writes one: the padded columns hold zeros.
#include "kernels.h"
#include "search_rescore.h"

namespace vr {

__global__ __launch_bounds__(256) void window_edge_kernel(WindowSearchArgs p, const float* __restrict__ S, size_t ldS) {
    __shared__ SelectLds L;
    const int tid = threadIdx.x, lane = tid & 63;
    const SearchArgs& a = p.a;
    const int q = blockIdx.x, n_docs = (int)a.n_docs, nv = a.dim >> 2;
    if (q == 0 && tid == 0) atomicAdd(&p.stats[0], (unsigned long long)gridDim.x);
    const int na = rows_allowed(a.n_docs, p.n_filters, p.allowed, p.filter_of_query ? p.filter_of_query[q] : -1);
    const int64_t o = p.offsets[q];
    if (o >= (int64_t)na) {                                                // (workgroup-uniform) an empty window: a row of tails
        if (tid == 0) { p.edges[2 * q] = __builtin_nanf(""); p.edges[2 * q + 1] = __builtin_nanf(""); }
        return;
    }
    f32x4 qv[MERGE_MAXV];
    load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
    const float eps = query_eps(a, qv);                                    // (every wave computes the same value)
    const float* row = S + (size_t)q * ldS;
    const int kz = (int)min(o + (int64_t)a.k, (int64_t)na);                // 1 <= o + 1 <= kz <= na
    const BandEdges e = window_edges(row, n_docs, (int)o, kz, eps, L);
    if (tid == 0) { p.edges[2 * q] = e.lo; p.edges[2 * q + 1] = e.hi; }
}

__global__ __launch_bounds__(256) void window_rescore_kernel(WindowSearchArgs p, float* __restrict__ S, size_t ldS) {
    __shared__ ChunkLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int q = blockIdx.y, n_docs = (int)a.n_docs, nv = a.dim >> 2;
    const float lo = p.edges[2 * q], hi = p.edges[2 * q + 1];
    if (lo != lo) return;                                                  // (workgroup-uniform) an empty window
    const int c0 = blockIdx.x * RESCORE_CHUNK, c1 = min(c0 + RESCORE_CHUNK, n_docs);
    // ---- certainly ahead: b > hi -> +inf; certainly behind or masked: b < lo -> -inf; the band lo <= b <= hi: listed
    float* row = S + (size_t)q * ldS;
    const unsigned mine = chunk_scan<4, true>(row, c0, c1, lo, hi, L);     // rows certainly ahead this wave found
    if (lane == 0 && mine) atomicAdd(&L.ahead, mine);
    __syncthreads();
    // ---- fp32 re-scoring of the band, one candidate per wave
    const int m = L.n_cand;
    if (m > 0) {                                                           // (workgroup-uniform)
        f32x4 qv[MERGE_MAXV];
        load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
        for (int c = wave; c < m; c += 4) {
            const int id = L.cand[c];
            const float s = exact_row_score(a, qv, id, nv, lane);
            if (lane == 0) row[id] = s;
        }
    }
    if (tid == 0) {
        if (m > 0) atomicAdd(&p.stats[1], (unsigned long long)m);
        const unsigned n = L.ahead;
        if (n > 0) atomicAdd(&p.stats[2], (unsigned long long)n);
    }
}

__global__ __launch_bounds__(256) void window_select_kernel(WindowSearchArgs p, const float* __restrict__ S, size_t ldS, int n_sort) {
    __shared__ WindowSelectLds L;
    const int tid = threadIdx.x;
    const SearchArgs& a = p.a;
    const int q = blockIdx.x, n_docs = (int)a.n_docs, k = a.k;
    const float lo = p.edges[2 * q];
    if (lo != lo) {                                                        // (workgroup-uniform) an empty window: k tails
        for (int c = tid; c < k; c += 256) emit_slot(a, q, c, KEY_NONE);
        return;
    }
    const int na = rows_allowed(a.n_docs, p.n_filters, p.allowed, p.filter_of_query ? p.filter_of_query[q] : -1);
    const int o = (int)p.offsets[q];                                       // (< na: the edge kernel saw it)
    const int kz = (int)min((int64_t)o + k, (int64_t)na);
    const float* row = S + (size_t)q * ldS;
    sort_gathered(row, window_positions(row, n_docs, o, kz, L), n_sort, L.s);
    for (int c = tid; c < k; c += 256) emit_slot(a, q, c, L.s.keys[c]);
}

static bool window_args_ok(const WindowSearchArgs& p, size_t ldS, int nq_block) {
    return rescore_args_ok(p.a, nq_block) && topk_out_ok(p.a) && p.offsets && p.edges && p.stats && ldS % 4 == 0 &&
           (int64_t)ldS >= p.a.n_docs && (!p.filter_of_query || (p.n_filters >= 1 && p.allowed));
}

hipError_t launch_window_edges(const WindowSearchArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s) {
    if (!window_args_ok(p, ldS, nq_block) || !S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_edge_kernel, dim3((unsigned)nq_block), dim3(256), 0, s, p, S, ldS);
    return hipGetLastError();
}

hipError_t launch_window_rescore(const WindowSearchArgs& p, float* S, size_t ldS, int nq_block, hipStream_t s) {
    if (!window_args_ok(p, ldS, nq_block) || !S) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.a.n_docs + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
    hipLaunchKernelGGL(window_rescore_kernel, dim3(chunks, (unsigned)nq_block), dim3(256), 0, s, p, S, ldS);
    return hipGetLastError();
}

hipError_t launch_window_select(const WindowSearchArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s) {
    if (!window_args_ok(p, ldS, nq_block) || !S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_select_kernel, dim3((unsigned)nq_block), dim3(256), 0, s, p, S, ldS, sort_width(p.a.k));
    return hipGetLastError();
}

}  // namespace vr
