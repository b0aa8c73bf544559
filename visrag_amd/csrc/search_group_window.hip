// vr_index_search_groups_window: WHICH groups (documents: runs of adjacent rows, group g = rows [goff[g], goff[g + 1])) stand at
// ranks [o, o + k) of a query's document ranking, under the query's filter — the windowed search (search_window.hip) with groups
// in the place of rows, any offset o, k <= search_bigk_max().  A group is PRESENT if the filter allows at least one of its rows;
// its score is E_g = max e_i over its ALLOWED rows, its best row the lowest allowed row that attains E_g; present groups rank by
// E_g descending, then lower best row first — groups are runs of adjacent rows, so that is lower group first.
// Let b_i be row i's bf16-MFMA score, e_i its fp32 score (dot_regs + wave_sum, the bits vr_index_search returns for that pair) and
// |b_i - e_i| <= eps for every allowed i (search_common.h: query_eps).
//   1. max is 1-Lipschitz under a sup-norm perturbation: the masked group maximum B_g = max b_i over the allowed rows lies within
//      eps of E_g (search_group.hip's argument);
//   2. so are order statistics: the r-th largest B lies within eps of the r-th largest E (search_window.hip's argument);
//   3. with nd the present groups, v_a the (o + 1)-th largest B and v_z the min(o + k, nd)-th largest B: every group of the window
//      has E in [v_z - eps, v_a + eps], hence B in [v_z - 2 eps, v_a + 2 eps]: the BAND.  A group with B_g > v_a + 2 eps has
//      E_g > v_a + eps >= the (o + 1)-th largest E: strictly ahead of the whole window, whatever its number; a group with
//      B_g < v_z - 2 eps is strictly behind it;
//   4. inside a band group only a row with b_i >= B_g - 2 eps can attain E_g, ties included: e_i = E_g >= B_g - eps gives
//      b_i >= e_i - eps >= B_g - 2 eps.  Re-scoring exactly those rows in fp32 and taking the largest make_key(e, row) gives
//      (E_g, best row); a row the filter forbids carries b = -inf and is never one of them;
//   5. every edge is rounded outward by one ulp (the rounded subtraction / addition cannot have narrowed a band);
//   6. with certification off the default error model defines eps, as in search_window.hip.
// With A the groups certainly ahead (A <= o always: fewer than o + 1 groups have B > v_a), the window is positions o - A ..
// o - A + k - 1 of the band groups sorted by make_key(E_g, g).  No candidate margin, no widening, no flagged queries: exact in
// every setting of vr_index_set_search_eps.  Per block of <= 256 queries (index_searches.hip):
//   1. score rows S[q][row] on the bf16 MFMA GEMM; with filters launch_filter_mask turns the columns a query may not see into
//      -inf; group_max_kernel (search_group.hip, as it is) gives B[q][g], -inf for a group without an allowed row;
//   2. group_window_edge_kernel, one workgroup per query: eps; nd = the group count without a filter, a workgroup count of
//      B_g > -inf with one, 0 for a filter index outside [-1, n_filters) (which a device caller's cannot be checked for before
//      the launch; the mask leaves such a row alone, and from here on nobody reads it); o >= nd: the query is empty (lo = NaN).
//      Otherwise two radix selects over the B row give v_a and v_z (both ranks <= nd: neither is an absent group's -inf) and
//      lo = one_ulp_down(v_z - 2 eps), hi = one_ulp_up(v_a + 2 eps);
//   3. group_window_rescore_kernel, grid (chunk of 4096 groups, query): the B row is REWRITTEN in place so that it alone defines
//      the answer: +inf for B_g > hi (certainly ahead), -inf for B_g < lo (certainly behind, or absent), and for the groups in
//      [lo, hi] — compacted into an LDS list (search_rescore.h: chunk_scan), one wave per group — E_g, with the best row in the
//      int32 side row R[q][g]: group_best_row gives every row with b_i >= one_ulp_down(B_g - 2 eps) one fp32 dot and keeps the
//      largest key.  A group longer than a chunk of rows — the whole index may be one group — is still one wave's loop, as in
//      group_select_kernel.  A column is written by one thread only: a group outside the band by the thread that classified it,
//      a band group by lane 0 of its wave;
//   4. group_window_select_kernel, one workgroup per query: radix selects for rank o (when o > 0) and rank min(o + k, nd) of the
//      rewritten row, gather_window (search_select.h), keys make_key(B[g], g), block_bitonic_desc, k slots (B[g], R[g], g)
//      emitted, (-inf, -1, -1) past the present groups.  The A groups of +inf hold ranks 0 .. A - 1 of the rewritten row, so
//      there is no per-query counter to subtract: the windowed search's trick unchanged.
// No kernel waits for another workgroup; stream order between the launches is the only ordering.  No kernel reads a B or R
// column at or past n_groups, or an S column at or past n_docs, as a value or writes one.
#include "kernels.h"
#include "search_rescore.h"

namespace vr {

__global__ __launch_bounds__(256) void group_window_edge_kernel(GroupWindowArgs p) {
    __shared__ SelectLds L;
    __shared__ int s_present;
    const int tid = threadIdx.x, lane = tid & 63;
    const SearchArgs& a = p.a;
    const int q = blockIdx.x, ng = p.n_groups, nv = a.dim >> 2;
    if (q == 0 && tid == 0) atomicAdd(&p.stats[0], (unsigned long long)gridDim.x);
    const float* brow = p.B + (size_t)q * p.ldB;
    // nd = the groups with an allowed row (workgroup-uniform)
    const int nd = present_count(brow, ng, p.filter_of_query ? p.filter_of_query[q] : -1, p.n_filters, &s_present);
    if (tid == 0) p.present[q] = nd;
    const int64_t o = p.offsets[q];
    if (o >= (int64_t)nd) {                                                // (workgroup-uniform) an empty window: a row of tails
        if (tid == 0) { p.edges[2 * q] = __builtin_nanf(""); p.edges[2 * q + 1] = __builtin_nanf(""); }
        return;
    }
    f32x4 qv[MERGE_MAXV];
    load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
    const float eps = query_eps(a, qv);                                    // (every wave computes the same value)
    const int kz = (int)min(o + (int64_t)a.k, (int64_t)nd);                // 1 <= o + 1 <= kz <= nd
    const BandEdges e = window_edges(brow, ng, (int)o, kz, eps, L);
    if (tid == 0) { p.edges[2 * q] = e.lo; p.edges[2 * q + 1] = e.hi; }
}

__global__ __launch_bounds__(256) void group_window_rescore_kernel(GroupWindowArgs p, const float* __restrict__ S, size_t ldS) {
    __shared__ ChunkLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int q = blockIdx.y, ng = p.n_groups, nv = a.dim >> 2;
    const float lo = p.edges[2 * q], hi = p.edges[2 * q + 1];
    if (lo != lo) return;                                                  // (workgroup-uniform) an empty window
    const int c0 = blockIdx.x * RESCORE_CHUNK, c1 = min(c0 + RESCORE_CHUNK, ng);
    // ---- certainly ahead: B > hi -> +inf; certainly behind or absent: B < lo -> -inf; the band lo <= B <= hi: listed
    float* brow = p.B + (size_t)q * p.ldB;
    chunk_scan<1, true>(brow, c0, c1, lo, hi, L);
    __syncthreads();
    // ---- the band: one wave per group, one fp32 dot for every row that can attain E_g
    const int m = L.n_cand;
    if (m > 0) {                                                           // (workgroup-uniform)
        f32x4 qv[MERGE_MAXV];
        load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
        const float eps = query_eps(a, qv);                                // (the edge kernel's value)
        const float* srow = S + (size_t)q * ldS;
        int* rrow = p.R + (size_t)q * p.ldB;
        unsigned dots = 0;
        for (int c = wave; c < m; c += 4) {
            const int g = L.cand[c];
            const uint64_t best = group_best_row(a, qv, srow, p.goff[g], p.goff[g + 1], band_lo(brow[g], eps), nv, lane, &dots);
            if (lane == 0) { brow[g] = key_score(best); rrow[g] = (int)(~(uint32_t)best); }
        }
        if (lane == 0 && dots) atomicAdd(&L.dots, (unsigned long long)dots);
    }
    __syncthreads();
    if (tid == 0 && m > 0) {
        atomicAdd(&p.stats[1], (unsigned long long)m);
        atomicAdd(&p.stats[2], L.dots);
    }
}

__global__ __launch_bounds__(256) void group_window_select_kernel(GroupWindowArgs p, int n_sort) {
    __shared__ WindowSelectLds L;
    const int tid = threadIdx.x;
    const SearchArgs& a = p.a;
    const int q = blockIdx.x, ng = p.n_groups, k = a.k;
    const float* brow = p.B + (size_t)q * p.ldB;
    const int* rrow = p.R + (size_t)q * p.ldB;
    auto emit = [&](int slot, uint64_t key) {                              // (score, best row, group) or a tail
        const size_t o = (size_t)q * k + slot;
        float score = -INFINITY;
        int64_t row = -1, group = -1;
        if (key != KEY_NONE) {
            const int g = (int)(~(uint32_t)key);
            score = key_score(key); row = (int64_t)rrow[g]; group = (int64_t)g;
        }
        a.out_scores[o] = score;
        a.out_ids[o] = row;
        p.out_groups[o] = group;
    };
    const float lo = p.edges[2 * q];
    if (lo != lo) {                                                        // (workgroup-uniform) an empty window: k tails
        for (int c = tid; c < k; c += 256) emit(c, KEY_NONE);
        return;
    }
    const int nd = p.present[q];
    const int o = (int)p.offsets[q];                                       // (< nd: the edge kernel saw it)
    const int kz = (int)min((int64_t)o + k, (int64_t)nd);
    sort_gathered(brow, window_positions(brow, ng, o, kz, L), n_sort, L.s);
    for (int c = tid; c < k; c += 256) emit(c, L.s.keys[c]);
}

static bool group_window_args_ok(const GroupWindowArgs& p, int nq_block) {
    return rescore_args_ok(p.a, nq_block) && topk_out_ok(p.a) && p.n_groups >= 1 && p.a.n_docs >= p.n_groups && p.out_groups &&
           p.goff && p.B && p.R && (int64_t)p.ldB >= p.n_groups && p.offsets && p.edges && p.present && p.stats;
}

hipError_t launch_group_window_edges(const GroupWindowArgs& p, int nq_block, hipStream_t s) {
    if (!group_window_args_ok(p, nq_block)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_window_edge_kernel, dim3((unsigned)nq_block), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_group_window_rescore(const GroupWindowArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s) {
    if (!group_window_args_ok(p, nq_block) || !S || (int64_t)ldS < p.a.n_docs) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.n_groups + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
    hipLaunchKernelGGL(group_window_rescore_kernel, dim3(chunks, (unsigned)nq_block), dim3(256), 0, s, p, S, ldS);
    return hipGetLastError();
}

hipError_t launch_group_window_select(const GroupWindowArgs& p, int nq_block, hipStream_t s) {
    if (!group_window_args_ok(p, nq_block)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_window_select_kernel, dim3((unsigned)nq_block), dim3(256), 0, s, p, sort_width(p.a.k));
    return hipGetLastError();
}

}  // namespace vr
