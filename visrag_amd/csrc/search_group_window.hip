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
//      [lo, hi] — compacted into an LDS list by ballot + popcount, one wave per group — E_g, with the best row in the int32 side
//      row R[q][g].  The wave walks the group's rows 64 at a time, ballots b_i >= one_ulp_down(B_g - 2 eps) and gives each such
//      row one fp32 dot, the row's loads issued in front of the fma chain; it keeps the largest key.  A group longer than a chunk
//      of rows — the whole index may be one group — is still one wave's loop, as in group_select_kernel.  A column is written
//      by one thread only: a group outside the band by the thread that classified it, a band group by lane 0 of its wave;
//   4. group_window_select_kernel, one workgroup per query: radix selects for rank o (when o > 0) and rank min(o + k, nd) of the
//      rewritten row, gather_window (search_select.h), keys make_key(B[g], g), block_bitonic_desc, k slots (B[g], R[g], g)
//      emitted, (-inf, -1, -1) past the present groups.  The A groups of +inf hold ranks 0 .. A - 1 of the rewritten row, so
//      there is no per-query counter to subtract: the windowed search's trick unchanged.
// No kernel waits for another workgroup; stream order between the launches is the only ordering.  No kernel reads a B or R
// column at or past n_groups, or an S column at or past n_docs, as a value or writes one.
#include "kernels.h"
#include "search_select.h"

namespace vr {

constexpr int GWIN_CHUNK = 4096;            // groups per workgroup of the re-scoring (the windowed search's chunk)

struct GroupWindowLds {
    int cand[GWIN_CHUNK];                   // groups inside the band, any order
    int n_cand;
    unsigned long long dots;                // fp32 row dots of this workgroup
};

__global__ __launch_bounds__(256) void group_window_edge_kernel(GroupWindowArgs p) {
    __shared__ SelectLds L;
    __shared__ int s_present;
    const int tid = threadIdx.x, lane = tid & 63;
    const SearchArgs& a = p.a;
    const int q = blockIdx.x, ng = p.n_groups, nv = a.dim >> 2;
    if (q == 0 && tid == 0) atomicAdd(&p.stats[0], (unsigned long long)gridDim.x);
    const float* brow = p.B + (size_t)q * p.ldB;
    const int f = p.filter_of_query ? p.filter_of_query[q] : -1;
    int nd = ng;
    if (f != -1 && (unsigned)f >= (unsigned)p.n_filters) {                 // (workgroup-uniform) no such filter: nothing is allowed, and
        nd = 0;                                                            // the mask left the row alone — nobody reads it
    } else if (f != -1) {                                                  // (workgroup-uniform) the groups with an allowed row
        if (tid == 0) s_present = 0;
        __syncthreads();
        int mine = 0;                       // (complete in lane 0: every lane of a wave holds the wave's count)
        for (int g0 = 0; g0 < ng; g0 += 256) {
            const int g = g0 + tid;
            mine += __popcll(__ballot(g < ng && brow[g] > -INFINITY));
        }
        if (lane == 0 && mine) atomicAdd(&s_present, mine);
        __syncthreads();
        nd = s_present;
    }
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
    const KthKey ka = select_kth(brow, ng, (int)o + 1, L);
    __syncthreads();
    const KthKey kz_key = select_kth(brow, ng, kz, L);
    if (tid == 0) {
        const float va = orderable_f32(ka.T), vz = orderable_f32(kz_key.T);
        p.edges[2 * q] = one_ulp_down(vz - 2.f * eps);
        p.edges[2 * q + 1] = one_ulp_up(va + 2.f * eps);
    }
}

__global__ __launch_bounds__(256) void group_window_rescore_kernel(GroupWindowArgs p, const float* __restrict__ S, size_t ldS) {
    __shared__ GroupWindowLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int q = blockIdx.y, ng = p.n_groups, nv = a.dim >> 2;
    const float lo = p.edges[2 * q], hi = p.edges[2 * q + 1];
    if (lo != lo) return;                                                  // (workgroup-uniform) an empty window
    const int c0 = blockIdx.x * GWIN_CHUNK, c1 = min(c0 + GWIN_CHUNK, ng);
    if (tid == 0) { L.n_cand = 0; L.dots = 0ull; }
    __syncthreads();
    // ---- certainly ahead: B > hi -> +inf; certainly behind or absent: B < lo -> -inf; the band lo <= B <= hi: listed
    float* brow = p.B + (size_t)q * p.ldB;
    for (int g0 = c0; g0 < c1; g0 += 256) {
        const int g = g0 + tid;
        const bool valid = g < c1;
        const float b = valid ? brow[g] : 0.f;
        const bool in = valid && b >= lo && b <= hi;
        if (valid && !in) brow[g] = b > hi ? INFINITY : -INFINITY;         // (a band column is written by the wave that re-scores it)
        band_append(in, g, L.cand, &L.n_cand);                             // (< GWIN_CHUNK: one slot per group)
    }
    __syncthreads();
    // ---- the band: one wave per group, one fp32 dot for every row that can attain E_g
    const int m = L.n_cand;
    if (m > 0) {                                                           // (workgroup-uniform)
        f32x4 qv[MERGE_MAXV];
        load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
        const float band = 2.f * query_eps(a, qv);                         // (the edge kernel's value)
        const float* srow = S + (size_t)q * ldS;
        int* rrow = p.R + (size_t)q * p.ldB;
        unsigned dots = 0;
        for (int c = wave; c < m; c += 4) {
            const int g = L.cand[c];
            const int glo = p.goff[g], ghi = p.goff[g + 1];
            const float lim = one_ulp_down(brow[g] - band);                // (the subtraction may have rounded up)
            uint64_t best = KEY_NONE;
            for (int i0 = glo; i0 < ghi; i0 += 64) {
                const int i = i0 + lane;
                unsigned long long in = __ballot(i < ghi && srow[i] >= lim);
                dots += (unsigned)__popcll(in);
                while (in) {                                               // (wave-uniform)
                    const int id = i0 + __ffsll((long long)in) - 1;
                    in &= in - 1ull;
                    f32x4 dv[MERGE_MAXV];
                    load_row_regs(dv, a.index_f32 + (size_t)id * a.dim, nv, lane);
                    const float s = wave_sum(dot_regs(qv, dv, nv, lane));
                    const uint64_t key = make_key(s, (uint32_t)id);
                    best = key > best ? key : best;
                }
            }
            // (the row that attains B_g passes lim: best is a key)
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
    KthKey ka{0xFFFFFFFFu, 0};
    if (o > 0) {
        ka = select_kth(brow, ng, o, L.s);
        __syncthreads();
    }
    const KthKey kzk = select_kth(brow, ng, kz, L.s);
    __syncthreads();
    const int n_sel = min(gather_window(brow, ng, ka, o > 0, kzk, L), SEL_CAND);
    for (int c = tid; c < n_sort; c += 256) {
        uint64_t key = KEY_NONE;
        if (c < n_sel) { const int g = L.s.cand[c]; key = make_key(brow[g], (uint32_t)g); }
        L.s.keys[c] = key;
    }
    __syncthreads();
    block_bitonic_desc(L.s.keys, n_sort, tid, 256);
    for (int c = tid; c < k; c += 256) emit(c, L.s.keys[c]);
}

static bool group_window_args_ok(const GroupWindowArgs& p, int nq_block) {
    const SearchArgs& a = p.a;
    return nq_block >= 1 && nq_block <= 256 && p.n_groups >= 1 && a.n_docs >= p.n_groups && a.n_docs < ((int64_t)1 << 31) &&
           range_dim_ok(a.dim) && a.index_f32 && a.q_f32 && a.dmax && (a.eps_data || a.eps_rel >= 0.f) && a.k >= 1 &&
           a.k <= SEL_CAND - SEL_MARGIN && a.out_scores && a.out_ids && !a.out_keys && p.out_groups && p.goff && p.B && p.R &&
           (int64_t)p.ldB >= p.n_groups && p.offsets && p.edges && p.present && p.stats;
}

hipError_t launch_group_window_edges(const GroupWindowArgs& p, int nq_block, hipStream_t s) {
    if (!group_window_args_ok(p, nq_block)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_window_edge_kernel, dim3((unsigned)nq_block), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_group_window_rescore(const GroupWindowArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s) {
    if (!group_window_args_ok(p, nq_block) || !S || (int64_t)ldS < p.a.n_docs) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.n_groups + GWIN_CHUNK - 1) / GWIN_CHUNK);
    hipLaunchKernelGGL(group_window_rescore_kernel, dim3(chunks, (unsigned)nq_block), dim3(256), 0, s, p, S, ldS);
    return hipGetLastError();
}

hipError_t launch_group_window_select(const GroupWindowArgs& p, int nq_block, hipStream_t s) {
    if (!group_window_args_ok(p, nq_block)) return hipErrorInvalidValue;
    int n_sort = 64;                                                       // the power of two that holds k keys
    while (n_sort < p.a.k) n_sort <<= 1;
    hipLaunchKernelGGL(group_window_select_kernel, dim3((unsigned)nq_block), dim3(256), 0, s, p, n_sort);
    return hipGetLastError();
}

}  // namespace vr
