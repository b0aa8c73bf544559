// vr_index_rank_groups / vr_index_count_groups_range: WHERE a named group (document: a run of adjacent rows, group g = rows
// [goff[g], goff[g + 1])) stands in a query's document ranking under the query's filter, and HOW MANY documents reach a
// threshold — exact counts, no lists.  The semantics are those of search_group_window.hip: a group is PRESENT if the filter
// allows at least one of its rows; its score is E_g = max e_i over its ALLOWED rows, its best row the lowest allowed row that
// attains E_g; present groups rank by E_g descending, then lower group first.  A pair is (query, bar): the bar of a rank is the
// 64-bit key make_key(E_g, g) of the target group, the bar of a count is the threshold t.
// Let b_i be row i's bf16-MFMA score, e_i its fp32 score (dot_regs + wave_sum, the bits vr_index_search returns for that pair)
// and |b_i - e_i| <= eps for every allowed i (search_common.h: query_eps).
//   1. max is 1-Lipschitz under a sup-norm perturbation: the masked group maximum B_g = max b_i over the allowed rows lies within
//      eps of E_g (search_group.hip's argument);
//   2. so for a bar t (t = E_g for a rank) a group with B_h > t + eps has E_h > t: certainly ahead of the bar; a group with
//      B_h < t - eps has E_h < t: certainly behind it — or it is absent (B_h = -inf, below every finite edge);
//   3. only the groups of the band between need E_h;
//   4. inside a band group only a row with b_i >= B_h - 2 eps can attain E_h, ties included: e_i = E_h >= B_h - eps gives
//      b_i >= e_i - eps >= B_h - 2 eps (step 4 of search_group_window.hip).  Re-scoring exactly those rows in fp32 and taking the
//      largest make_key(e, row) gives (E_h, best row); a row the filter forbids carries b = -inf and is never one of them;
//   5. every edge is rounded outward by one ulp (the rounded subtraction / addition cannot have narrowed a band);
//   6. with certification off the default error model defines eps: the result is exact in every setting of
//      vr_index_set_search_eps;
//   7. the target lies in its own band and compares equal to its own key: it never counts itself.
// A target the filter leaves no row of is NOT in the ranking — its score is defined over its allowed rows, and it has none: it
// gets (-inf, -1, -1).  (vr_index_rank_rows differs: a forbidden row has a score, and gets the position it would take.)
// No candidate margin, no widening, no flagged queries.  Per block of <= 256 queries (index_searches.hip):
//   1. score rows S[q][row] on the bf16 MFMA GEMM; with filters launch_filter_mask turns the columns a query may not see into
//      -inf; group_max_kernel (search_group.hip, as it is) gives B[q][g], -inf for a group without an allowed row;
//   2. group_rank_bar_kernel, one wave per pair: eps of the pair's query.  For a rank the wave walks the target's rows 64 at a
//      time, ballots b_i >= one_ulp_down(B_g - 2 eps) and gives each such row one fp32 dot, the row's loads issued in front of
//      the fma chain; the largest key is (E_g, best row) -> out_scores / out_rows, the bar is make_key(E_g, g), the count
//      starts at 0.  An absent target (B_g = -inf), or any target under a filter index outside [-1, n_filters) (a device
//      caller's: it cannot be seen before the launch; the mask left that row alone, nobody reads it), gets the tail triple and
//      the pair is dead: eps = NaN.  For a count the bar is the threshold (-0.0 taken as +0.0), the count starts at 0, and a
//      filter index out of range leaves it there (dead as well);
//   3. group_rank_count_kernel, one workgroup per (chunk of 4096 groups, pair): lo = one_ulp_down(t - eps), hi = one_ulp_up(t +
//      eps).  B_h > hi: counted from B alone; B_h < lo: skipped; the groups in [lo, hi] are compacted into an LDS list
//      (search_rescore.h: chunk_scan) and re-scored one group per wave by the same group_best_row: a rank compares
//      make_key(E_h, h) with the bar, a count compares floats (>= t, or > t when strict).  B and S are only read — several pairs
//      share a query's rows.  The workgroup's total is one 64-bit integer add into the pair's count: integer adds commute, the
//      result does not depend on the order.  A group longer than a chunk of rows — the whole index may be one group — is still
//      one wave's loop.
// Pairs are laid along the grid's x dimension (chunk fastest), a launch holds at most 2^22 workgroups, as launch_rank_count
// splits.  No kernel waits for another workgroup; stream order between the launches is the only ordering.  No kernel reads a B
// column at or past n_groups, or an S column at or past n_docs.
#include "kernels.h"
#include "search_rescore.h"

namespace vr {

constexpr int64_t GRNK_MAX_WGS = (int64_t)1 << 22;   // workgroups per launch of the counting kernel

__global__ __launch_bounds__(256) void group_rank_bar_kernel(GroupRankArgs p, const float* __restrict__ S, size_t ldS, int n_pairs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SearchArgs& a = p.a;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&p.stats[0], (unsigned long long)n_pairs);
    const int pair = blockIdx.x * 4 + wave;
    if (pair >= n_pairs) return;                                           // (wave-uniform; no barrier below)
    const int q = p.pair_query[pair], nv = a.dim >> 2;
    f32x4 qv[MERGE_MAXV];
    load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
    float eps = query_eps(a, qv);
    const bool no_filter = !filter_index_ok(p.filter_of_query ? p.filter_of_query[q] : -1, p.n_filters);   // nothing allowed
    if (no_filter) eps = __builtin_nanf("");
    unsigned long long bar;
    long long count = 0;
    if (p.pair_group) {
        const int g = p.pair_group[pair];                                  // (in [0, n_groups): the host checked it)
        const float bg = no_filter ? -INFINITY : p.B[(size_t)q * p.ldB + g];
        float score = -INFINITY;
        long long row = -1;
        bar = KEY_NONE;
        if (bg > -INFINITY) {                                              // (wave-uniform) a present target
            unsigned dots = 0;
            const uint64_t best = group_best_row(a, qv, S + (size_t)q * ldS, p.goff[g], p.goff[g + 1], band_lo(bg, eps), nv, lane, &dots);
            score = key_score(best); row = (long long)(~(uint32_t)best);
            bar = make_key(score, (uint32_t)g);
            if (lane == 0) {
                atomicAdd(&p.stats[1], 1ull);
                atomicAdd(&p.stats[2], (unsigned long long)dots);
            }
        } else {                                                           // absent: not in the ranking
            eps = __builtin_nanf("");
            count = -1;
        }
        if (lane == 0) { p.out_scores[pair] = score; p.out_rows[pair] = row; }
    } else {
        const float t = p.pair_thr[pair];
        bar = (unsigned long long)__float_as_uint(t == 0.f ? 0.f : t);     // -0.0 counts as +0.0
    }
    if (lane == 0) {
        p.bars[pair] = bar;
        p.bar_eps[pair] = eps;
        p.out_counts[pair] = (unsigned long long)count;
    }
}

__global__ __launch_bounds__(256) void group_rank_count_kernel(GroupRankArgs p, const float* __restrict__ S, size_t ldS, int pair0,
                                                               int chunks) {
    __shared__ ChunkLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int pair = pair0 + (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    const float eps = p.bar_eps[pair];
    if (eps != eps) return;                                                // (workgroup-uniform) a dead pair: its slot is final
    const int q = p.pair_query[pair], ng = p.n_groups, nv = a.dim >> 2;
    const int c0 = chunk * RESCORE_CHUNK, c1 = min(c0 + RESCORE_CHUNK, ng);
    const unsigned long long bar = p.bars[pair];
    const bool by_key = p.pair_group != nullptr;
    const float t = by_key ? key_score(bar) : __uint_as_float((uint32_t)bar);
    const float lo = one_ulp_down(t - eps), hi = one_ulp_up(t + eps);
    // ---- certainly ahead: B > hi; the band: lo <= B <= hi (an absent group is -inf, lo is finite)
    const float* brow = p.B + (size_t)q * p.ldB;
    unsigned mine = chunk_scan<1, false>(brow, c0, c1, lo, hi, L);         // groups ahead of the bar this wave found
    __syncthreads();
    // ---- the band: one wave per group, one fp32 dot for every row that can attain E_h
    const int m = L.n_cand;
    if (m > 0) {                                                           // (workgroup-uniform)
        f32x4 qv[MERGE_MAXV];
        load_query_regs(qv, a.q_f32 + (size_t)q * a.dim, nv, lane);
        const float* srow = S + (size_t)q * ldS;
        unsigned dots = 0;
        for (int c = wave; c < m; c += 4) {
            const int h = L.cand[c];
            const uint64_t best = group_best_row(a, qv, srow, p.goff[h], p.goff[h + 1], band_lo(brow[h], eps), nv, lane, &dots);
            const float e = key_score(best);
            const bool ahead = by_key ? make_key(e, (uint32_t)h) > bar : (p.strict ? e > t : e >= t);
            mine += ahead ? 1u : 0u;                                       // (every lane holds the same e)
        }
        if (lane == 0 && dots) atomicAdd(&L.dots, (unsigned long long)dots);
    }
    if (lane == 0 && mine) atomicAdd(&L.ahead, mine);
    __syncthreads();
    if (tid == 0) {
        if (m > 0) {
            atomicAdd(&p.stats[1], (unsigned long long)m);
            atomicAdd(&p.stats[2], L.dots);
        }
        const unsigned n = L.ahead;
        if (n > 0) atomicAdd(&p.out_counts[pair], (unsigned long long)n);
    }
}

static bool group_rank_args_ok(const GroupRankArgs& p, const float* S, size_t ldS, int nq_block, int64_t n_pairs) {
    return rescore_args_ok(p.a, nq_block) && n_pairs >= 1 && n_pairs < ((int64_t)1 << 31) && p.n_groups >= 1 &&
           p.a.n_docs >= p.n_groups && p.goff && p.B && (int64_t)p.ldB >= p.n_groups && p.pair_query &&
           ((p.pair_group != nullptr) != (p.pair_thr != nullptr)) && (!p.pair_group || (p.out_scores && p.out_rows)) && p.bars &&
           p.bar_eps && p.out_counts && p.stats && S && (int64_t)ldS >= p.a.n_docs && (!p.filter_of_query || p.n_filters >= 1);
}

hipError_t launch_group_rank_bars(const GroupRankArgs& p, const float* S, size_t ldS, int nq_block, int64_t n_pairs, hipStream_t s) {
    if (!group_rank_args_ok(p, S, ldS, nq_block, n_pairs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_rank_bar_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0, s, p, S, ldS, (int)n_pairs);
    return hipGetLastError();
}

hipError_t launch_group_rank_count(const GroupRankArgs& p, const float* S, size_t ldS, int nq_block, int64_t n_pairs, hipStream_t s) {
    if (!group_rank_args_ok(p, S, ldS, nq_block, n_pairs)) return hipErrorInvalidValue;
    const int64_t chunks = ((int64_t)p.n_groups + RESCORE_CHUNK - 1) / RESCORE_CHUNK;
    const int64_t per_launch = GRNK_MAX_WGS / chunks;                      // (chunks < 2^19: at least 8 pairs)
    for (int64_t p0 = 0; p0 < n_pairs; p0 += per_launch) {
        const int64_t np = n_pairs - p0 < per_launch ? n_pairs - p0 : per_launch;
        hipLaunchKernelGGL(group_rank_count_kernel, dim3((unsigned)(np * chunks)), dim3(256), 0, s, p, S, ldS, (int)p0, (int)chunks);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace vr
