// vr_index_search_groups_range: EVERY group (document: a run of adjacent rows, group g = rows [goff[g], goff[g + 1])) whose score
// reaches a query's threshold t, under the query's filter — the range search (search_range.hip) with groups in the place of rows:
// a result whose size is the answer, in CSR form (lims, scores, best rows, groups), ascending group inside a query.  The semantics
// are those of search_group_window.hip and search_group_rank.hip: a group is PRESENT if the filter allows at least one of its
// rows; its score is E_g = max e_i over its ALLOWED rows, its best row the lowest allowed row that attains E_g; the result of a
// query is every present group with E_g >= t (a float compare: -0.0 counts as +0.0).
// Let b_i be row i's bf16-MFMA score, e_i its fp32 score (dot_regs + wave_sum, the bits vr_index_search returns for that pair)
// and |b_i - e_i| <= eps for every allowed i (search_common.h: query_eps).
//   1. max is 1-Lipschitz under a sup-norm perturbation: the masked group maximum B_g = max b_i over the allowed rows lies within
//      eps of E_g (search_group.hip's argument);
//   2. so E_g >= t implies B_g >= t - eps: a group with B_g < t - eps is not in the result — or it is absent (B_g = -inf, below
//      every finite bound);
//   3. inside a group of the band B_g >= t - eps only a row with b_i >= B_g - 2 eps can attain E_g, ties included: e_i = E_g >=
//      B_g - eps gives b_i >= e_i - eps >= B_g - 2 eps (step 4 of search_group_window.hip).  Re-scoring exactly those rows in fp32
//      and taking the largest make_key(e, row) gives (E_g, best row); a row the filter forbids carries b = -inf and is never one
//      of them;
//   4. the groups kept are those with E_g >= t: the fp32 answer;
//   5. every edge is rounded outward by one ulp (one_ulp_down: the rounded subtraction cannot have narrowed a band);
//   6. with certification off the default error model defines eps: the result is exact in every setting of
//      vr_index_set_search_eps.
// No candidate margin, no widening, no flagged queries; a query costs what its band holds.  Per block of <= 256 queries
// (index_searches.hip):
//   1. score rows S[q][row] on the bf16 MFMA GEMM; with filters launch_filter_mask turns the columns a query may not see into
//      -inf; group_max_kernel (search_group.hip, as it is) gives B[q][g] in a buffer of this search's own, -inf for a group
//      without an allowed row;
//   2. group_range_rescore_kernel, grid (chunk of 4096 groups, query): eps from the query in registers, bound = one_ulp_down(t -
//      eps).  The groups with B_g >= bound are compacted into an LDS list (search_rescore.h: chunk_scan) and re-scored one
//      group per wave by group_best_row: the wave walks the group's rows 64 at a time, ballots b_i >= one_ulp_down(B_g - 2 eps)
//      and gives each such row one fp32 dot, the row's loads in front of the fma chain.
//      The result goes back IN PLACE: B[g] = E_g where E_g >= t, -inf where not, the best row into the int32 side row R[q][g].  A
//      group below the bound keeps its B < t, an absent group its -inf: from here on "B[q][g] >= t" is exactly membership and the
//      stored value is the score to return.  Kept groups are counted per 1024 groups (a wave's share of the pack).  A band column
//      is read and written by the one wave that re-scores it.  A group longer than a chunk of rows — the whole index may be one
//      group — is still one wave's loop;
//   3. range_scan_kernel (search_range.hip, as it is, the group count in the place of the row count): exclusive scan of a query's
//      (1024 groups) counts -> the offsets of the pack inside the query's segment; scan of the queries' totals -> the block's part
//      of lims and the block's total, which the host reads (capacity check, growth of the result buffers);
//   4. group_range_pack_kernel, same grid: wave w of a workgroup compacts (B[g], R[g], g) of its 1024 groups with B >= t to the
//      three result arrays at lims[q] + its scanned offset, in group order — no barrier, no sort.
// A threshold that is not finite, or a filter index outside [-1, n_filters) (on the device neither can be seen before the
// launch): an empty segment, nothing of S, B, R, of the index or of the grouping is read for that query.
// No kernel waits for another workgroup; stream order between the launches is the only ordering.  No kernel reads a B or R
// column at or past n_groups, or an S column at or past n_docs.  S is only read.
#include "kernels.h"
#include "search_rescore.h"

namespace vr {

__global__ __launch_bounds__(256) void group_range_rescore_kernel(GroupRangeArgs p, const float* __restrict__ S, size_t ldS,
                                                                  int* __restrict__ counts) {
    __shared__ ChunkLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int q = blockIdx.y, ng = p.n_groups, nv = a.dim >> 2;
    const int c0 = blockIdx.x * RESCORE_CHUNK, c1 = min(c0 + RESCORE_CHUNK, ng);
    const int64_t nsub = ((int64_t)ng + RESCORE_SUB - 1) / RESCORE_SUB;
    int* cnt = counts + (size_t)q * nsub + (size_t)blockIdx.x * RESCORE_SUBS;
    const int my_subs = (c1 - c0 + RESCORE_SUB - 1) / RESCORE_SUB;         // 1..4 counts belong to this workgroup
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&p.stats[0], 1ull);
    const float t = range_threshold(p.thresholds, p.filter_of_query, p.n_filters, q);
    if (t != t) {                                                          // (workgroup-uniform) an empty segment
        if (tid < my_subs) cnt[tid] = 0;
        return;
    }
    f32x4 qv[MERGE_MAXV];
    load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
    const float eps = query_eps(a, qv);                                    // (every wave computes the same value)
    const float bound = one_ulp_down(t - eps);                             // (the subtraction may have rounded up)
    // ---- the band: groups with B >= bound (an absent group is -inf, the bound is finite)
    float* brow = p.B + (size_t)q * p.ldB;
    chunk_scan<1, false>(brow, c0, c1, bound, INFINITY, L);
    __syncthreads();
    // ---- the band: one wave per group, one fp32 dot for every row that can attain E_g
    const int m = L.n_cand;
    if (m > 0) {                                                           // (workgroup-uniform)
        const float* srow = S + (size_t)q * ldS;
        int* rrow = p.R + (size_t)q * p.ldB;
        unsigned dots = 0;
        for (int c = wave; c < m; c += 4) {
            const int g = L.cand[c];
            const uint64_t best = group_best_row(a, qv, srow, p.goff[g], p.goff[g + 1], band_lo(brow[g], eps), nv, lane, &dots);
            if (lane == 0) {                                               // (the row that attains B_g passed lim: best is a key)
                const float e = key_score(best);
                const bool keep = e >= t;
                brow[g] = keep ? e : -INFINITY;
                rrow[g] = (int)(~(uint32_t)best);
                if (keep) atomicAdd(&L.kept[(g - c0) / RESCORE_SUB], 1);
            }
        }
        if (lane == 0 && dots) atomicAdd(&L.dots, (unsigned long long)dots);
    }
    __syncthreads();
    if (tid < my_subs) cnt[tid] = L.kept[tid];
    if (tid == 0 && m > 0) {
        atomicAdd(&p.stats[1], (unsigned long long)m);
        atomicAdd(&p.stats[2], L.dots);
    }
}

__global__ __launch_bounds__(256) void group_range_pack_kernel(GroupRangeArgs p, const int* __restrict__ counts,
                                                               const int* __restrict__ offs, const int64_t* __restrict__ lims) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y, ng = p.n_groups;
    const int s0 = blockIdx.x * RESCORE_CHUNK + wave * RESCORE_SUB, s1 = min(s0 + RESCORE_SUB, ng);
    if (s0 >= ng) return;                                                  // (wave-uniform, no barrier below)
    const int64_t nsub = ((int64_t)ng + RESCORE_SUB - 1) / RESCORE_SUB;
    const size_t slot = (size_t)q * nsub + (size_t)blockIdx.x * RESCORE_SUBS + wave;
    if (counts[slot] == 0) return;                                         // (also: every query with an empty segment)
    const float t = p.thresholds[q];
    int64_t run = lims[q] + offs[slot];                                    // (lims: the block's first query's entry, as the scan got it)
    const float* brow = p.B + (size_t)q * p.ldB;
    const int* rrow = p.R + (size_t)q * p.ldB;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int g0 = s0; g0 < s1; g0 += 64) {                                 // (wave-uniform trip count: the ballot needs every lane)
        const int g = g0 + lane;
        const float v = g < s1 ? brow[g] : -INFINITY;
        const bool in = g < s1 && v >= t;
        const unsigned long long bm = __ballot(in);
        if (in) {
            const int64_t o = run + __popcll(bm & below);                  // (< lims[nq_block] <= the buffers' entries)
            p.out_scores[o] = v;
            p.out_rows[o] = (int64_t)rrow[g];                              // (a kept group went through the re-scoring: R[g] is set)
            p.out_groups[o] = (int64_t)g;
        }
        run += __popcll(bm);
    }
}

static bool group_range_args_ok(const GroupRangeArgs& p, int nq_block) {
    return rescore_args_ok(p.a, nq_block) && p.n_groups >= 1 && p.a.n_docs >= p.n_groups && p.goff && p.B && p.R &&
           (int64_t)p.ldB >= p.n_groups && p.thresholds && p.stats && (!p.filter_of_query || p.n_filters >= 1);
}

hipError_t launch_group_range_rescore(const GroupRangeArgs& p, const float* S, size_t ldS, int nq_block, int* counts, hipStream_t s) {
    if (!group_range_args_ok(p, nq_block) || !S || (int64_t)ldS < p.a.n_docs || !counts) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.n_groups + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
    hipLaunchKernelGGL(group_range_rescore_kernel, dim3(chunks, (unsigned)nq_block), dim3(256), 0, s, p, S, ldS, counts);
    return hipGetLastError();
}

hipError_t launch_group_range_pack(const GroupRangeArgs& p, int nq_block, const int* counts, const int* offs, const int64_t* lims,
                                   hipStream_t s) {
    if (!group_range_args_ok(p, nq_block) || !counts || !offs || !lims || !p.out_scores || !p.out_rows || !p.out_groups)
        return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.n_groups + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
    hipLaunchKernelGGL(group_range_pack_kernel, dim3(chunks, (unsigned)nq_block), dim3(256), 0, s, p, counts, offs, lims);
    return hipGetLastError();
}

}  // namespace vr
