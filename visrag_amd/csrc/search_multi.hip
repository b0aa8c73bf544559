// vr_index_search_multi: the k rows of largest FUSED score per group of sub-queries.  For group g with sub-queries j and row i,
// E_g(i) = max_j e_j(i) (fuse = max, "any-of") or min_j e_j(i) (fuse = min, "all-of"), e_j(i) the library's one fp32 score
// (dot_lane + wave_sum, the bits vr_index_search returns for that pair), max and min taken on f32_orderable keys (-0.0 < +0.0).
// The result is ranked by E_g descending, then lower id first, over the rows the group's filter allows; `which` names the lowest
// in-group j whose e_j(i) has exactly the fused score's bits.  Why it is exact:
//   1. let b_j(i) be the bf16-MFMA score, |b_j(i) - e_j(i)| <= eps_j (search_common.h: query_eps), and B_g = max_j b_j (or min);
//   2. max and min over a fixed set are 1-Lipschitz in the sup norm: |B_g(i) - E_g(i)| <= eps_g := max_j eps_j for every row;
//   3. from here on it is search_window.hip's argument at offset 0 with eps_g in the place of eps.  Order statistics are
//      1-Lipschitz too: with v_a the largest fused bf16 value and v_z the min(k, allowed)-th largest, every row of the result has
//      E in [v_z - eps_g, v_a + eps_g], hence B in the BAND [v_z - 2 eps_g, v_a + 2 eps_g].  A row with B below the band is
//      strictly behind the whole result; at offset 0 nothing can be ahead of it, and v_a is the row's maximum, so no fused value
//      lies above the band's upper edge: only the lower edge lo = one_ulp_down(v_z - 2 eps_g) is ever tested, one radix select
//      finds it, and exactly the rows with B >= lo are re-scored in fp32;
//   4. no candidate margin, no widening, no flagged groups; with certification off the default error model defines the band.
// The host (index_searches.hip) packs whole groups greedily into blocks of <= 256 sub-queries.  Per block:
//   1. score rows S[sub-query][row] on the bf16 MFMA GEMM (the deep path's launch); under filters launch_filter_mask runs with the
//      group's filter expanded to its sub-queries (multi_expand_kernel), so a masked column is -inf in every sub-row and stays
//      -inf under either fusion;
//   2. multi_fuse_kernel, grid (column chunk, group): the column-wise max or min over the group's rows, written into the group's
//      FIRST row (a group of one: nothing to do).  16-byte loads and stores, a thread reads and writes its own four columns only;
//   3. multi_edge_kernel, one workgroup per group: eps_g (query_eps of every sub-query, a wave each, then the max), the allowed
//      count na; na == 0 (an empty filter, or a device caller's filter index outside [-1, n_filters)): the group is empty
//      (lo = NaN).  Otherwise a radix select over the fused row gives v_z (rank <= na: not a masked -inf) and lo;
//   4. multi_rescore_kernel, grid (column chunk of 4096, group): the fused row is REWRITTEN in place: -inf below lo, and for the
//      columns at or above it — compacted into an LDS list (search_rescore.h: chunk_scan), one candidate per wave, the row's loads issued
//      in front of the fma chains and held in registers while the kernel loops over the group's sub-queries — the fp32 fused
//      score.  Every dot product keeps dot_lane's summation order.  A column is written by one thread only;
//   5. multi_select_kernel, one workgroup per group: radix select at rank min(k, na) of the rewritten row, gather_ordered
//      (lowest ids first inside the last tie tier), keys make_key(E, id), block_bitonic_desc, k slots emitted, (-inf, -1, -1)
//      past the allowed rows; `which` is recomputed for the winners (k * m dot products: no side buffer).
// No kernel waits for another workgroup; stream order between the launches is the only ordering.  No kernel reads a column at
// or past n_docs as a value or writes one.
#include "kernels.h"
#include "search_rescore.h"

namespace vr {

struct MultiEdgeLds {
    SelectLds s;
    float eps[4];                           // group_eps: the largest query_eps every wave met
};

// rows group g may see (search_common.h: rows_allowed); no filter array: every group is on -1
__device__ __forceinline__ int group_rows(const MultiSearchArgs& p, int g) {
    return rows_allowed(p.a.n_docs, p.n_filters, p.allowed, p.filter_of_group ? p.filter_of_group[g] : -1);
}

// filter_of_sub[s] = filter_of_group[g] for the sub-queries s of group g: what launch_filter_mask reads, one entry per score row
__global__ __launch_bounds__(256) void multi_expand_kernel(const int* __restrict__ lims, const int* __restrict__ filter_of_group,
                                                           int* __restrict__ filter_of_sub) {
    const int g = blockIdx.x, f = filter_of_group[g];
    for (int s = lims[g] + threadIdx.x; s < lims[g + 1]; s += 256) filter_of_sub[s] = f;
}

__global__ __launch_bounds__(256) void multi_fuse_kernel(MultiSearchArgs p, float* __restrict__ S, size_t ldS) {
    const int g = blockIdx.y, n_docs = (int)p.a.n_docs;
    const int s0 = p.lims[g] - p.sub_base, m = p.lims[g + 1] - p.lims[g];
    if (m < 2) return;                                                     // a group of one: its row is its own fusion
    float* row = S + (size_t)s0 * ldS;
    fuse_columns(row, ldS, m, row, n_docs, p.fuse);
}

__global__ __launch_bounds__(256) void multi_edge_kernel(MultiSearchArgs p, const float* __restrict__ S, size_t ldS) {
    __shared__ MultiEdgeLds L;
    const int tid = threadIdx.x;
    const SearchArgs& a = p.a;
    const int g = blockIdx.x, n_docs = (int)a.n_docs;
    if (g == 0 && tid == 0) atomicAdd(&p.stats[0], (unsigned long long)gridDim.x);
    const int na = group_rows(p, g);
    if (na <= 0) {                                                         // (workgroup-uniform) nothing allowed: a row of tails
        if (tid == 0) p.edges[g] = __builtin_nanf("");
        return;
    }
    const int s0 = p.lims[g] - p.sub_base, m = p.lims[g + 1] - p.lims[g];
    const float eps_g = group_eps(a, s0, m, nullptr, L.eps);
    const KthKey kz = select_kth(S + (size_t)s0 * ldS, n_docs, min(a.k, na), L.s);
    if (tid == 0) p.edges[g] = band_lo(orderable_f32(kz.T), eps_g);
}

// the fused fp32 score of row `id` for the group's m sub-queries (first: qrow), and — want_which — the lowest j whose score has
// exactly the bits `target`; called by a whole wave, the result is wave-uniform
__device__ __forceinline__ float multi_fused_score(const SearchArgs& a, const float* qrow, int m, int fuse, int id, int nv, int lane,
                                                   bool want_which, float target, int* which) {
    f32x4 dv[MERGE_MAXV];
    load_row_regs(dv, a.index_f32 + (size_t)id * a.dim, nv, lane);
    float best = 0.f;
    int w = -1;
    for (int j = 0; j < m; ++j) {
        const f32x4* qr = reinterpret_cast<const f32x4*>(qrow + (size_t)j * a.dim);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MERGE_MAXV; ++i) {
            const int cc = lane + i * 64;
            if (cc < nv) s = dot_chunk(qr[cc], dv[i], s);                  // the chain of dot_lane(query, row)
        }
        s = wave_sum(s);
        best = j == 0 ? s : multi_pick(best, s, fuse);
        if (want_which && w < 0 && __float_as_uint(s) == __float_as_uint(target)) w = j;
    }
    if (want_which) *which = w;
    return best;
}

__global__ __launch_bounds__(256) void multi_rescore_kernel(MultiSearchArgs p, float* __restrict__ S, size_t ldS) {
    __shared__ ChunkLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int g = blockIdx.y, n_docs = (int)a.n_docs, nv = a.dim >> 2;
    const float lo = p.edges[g];
    if (lo != lo) return;                                                  // (workgroup-uniform) an empty group
    const int s0 = p.lims[g] - p.sub_base, m = p.lims[g + 1] - p.lims[g];
    const int c0 = blockIdx.x * RESCORE_CHUNK, c1 = min(c0 + RESCORE_CHUNK, n_docs);
    // ---- certainly behind or masked: B < lo -> -inf; the band B >= lo: listed
    float* row = S + (size_t)s0 * ldS;
    chunk_scan<4, true>(row, c0, c1, lo, INFINITY, L);
    __syncthreads();
    // ---- fp32 re-scoring of the band, one candidate per wave, every sub-query of the group against the row in registers
    const int n = L.n_cand;
    const float* qrow = a.q_f32 + (size_t)s0 * a.dim;
    for (int c = wave; c < n; c += 4) {
        const int id = L.cand[c];
        const float s = multi_fused_score(a, qrow, m, p.fuse, id, nv, lane, false, 0.f, nullptr);
        if (lane == 0) row[id] = s;
    }
    if (tid == 0 && n > 0) {
        atomicAdd(&p.stats[1], (unsigned long long)n);
        atomicAdd(&p.stats[2], (unsigned long long)n * (unsigned long long)m);
    }
}

__global__ __launch_bounds__(256) void multi_select_kernel(MultiSearchArgs p, const float* __restrict__ S, size_t ldS, int n_sort) {
    __shared__ SelectLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int g = blockIdx.x, n_docs = (int)a.n_docs, k = a.k, nv = a.dim >> 2;
    int* which = p.out_which + (size_t)g * k;
    const float lo = p.edges[g];
    if (lo != lo) {                                                        // (workgroup-uniform) an empty group: k tails
        for (int c = tid; c < k; c += 256) { emit_slot(a, g, c, KEY_NONE); which[c] = -1; }
        return;
    }
    const int s0 = p.lims[g] - p.sub_base, m = p.lims[g + 1] - p.lims[g];
    const int kz = min(k, group_rows(p, g));                               // >= 1: at least kz columns hold a finite fp32 score
    const float* row = S + (size_t)s0 * ldS;
    top_positions(row, n_docs, kz, L);
    sort_gathered(row, kz, n_sort, L);
    for (int c = tid; c < k; c += 256) {
        emit_slot(a, g, c, L.keys[c]);
        if (c >= kz) which[c] = -1;
    }
    // ---- which sub-query decided every winner: the lowest j whose fp32 score has the fused score's bits
    const float* qrow = a.q_f32 + (size_t)s0 * a.dim;
    for (int c = wave; c < kz; c += 4) {
        const uint64_t key = L.keys[c];
        int w = -1;
        multi_fused_score(a, qrow, m, p.fuse, (int)(~(uint32_t)key), nv, lane, true, key_score(key), &w);
        if (lane == 0) which[c] = w;
    }
}

static bool multi_args_ok(const MultiSearchArgs& p, size_t ldS, int n_groups) {
    const SearchArgs& a = p.a;
    return rescore_args_ok(a, n_groups) && topk_out_ok(a) && a.nq >= n_groups && a.nq <= 256 && p.out_which && p.lims &&
           p.sub_base >= 0 && (p.fuse == 0 || p.fuse == 1) && p.edges && p.stats && ldS % 4 == 0 && (int64_t)ldS >= a.n_docs &&
           (!p.filter_of_group || (p.n_filters >= 1 && p.allowed));
}

hipError_t launch_multi_expand(const int* lims, const int* filter_of_group, int n_groups, int* filter_of_sub, hipStream_t s) {
    if (n_groups <= 0) return hipSuccess;
    if (!lims || !filter_of_group || !filter_of_sub) return hipErrorInvalidValue;
    hipLaunchKernelGGL(multi_expand_kernel, dim3((unsigned)n_groups), dim3(256), 0, s, lims, filter_of_group, filter_of_sub);
    return hipGetLastError();
}

hipError_t launch_multi_fuse(const MultiSearchArgs& p, float* S, size_t ldS, int n_groups, hipStream_t s) {
    if (!multi_args_ok(p, ldS, n_groups) || !S) return hipErrorInvalidValue;
    if (p.a.nq == n_groups) return hipSuccess;                             // groups of one: every row is its own fusion
    const unsigned chunks = (unsigned)((p.a.n_docs + FUSE_COLS - 1) / FUSE_COLS);
    hipLaunchKernelGGL(multi_fuse_kernel, dim3(chunks, (unsigned)n_groups), dim3(256), 0, s, p, S, ldS);
    return hipGetLastError();
}

hipError_t launch_multi_edges(const MultiSearchArgs& p, const float* S, size_t ldS, int n_groups, hipStream_t s) {
    if (!multi_args_ok(p, ldS, n_groups) || !S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(multi_edge_kernel, dim3((unsigned)n_groups), dim3(256), 0, s, p, S, ldS);
    return hipGetLastError();
}

hipError_t launch_multi_rescore(const MultiSearchArgs& p, float* S, size_t ldS, int n_groups, hipStream_t s) {
    if (!multi_args_ok(p, ldS, n_groups) || !S) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.a.n_docs + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
    hipLaunchKernelGGL(multi_rescore_kernel, dim3(chunks, (unsigned)n_groups), dim3(256), 0, s, p, S, ldS);
    return hipGetLastError();
}

hipError_t launch_multi_select(const MultiSearchArgs& p, const float* S, size_t ldS, int n_groups, hipStream_t s) {
    if (!multi_args_ok(p, ldS, n_groups) || !S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(multi_select_kernel, dim3((unsigned)n_groups), dim3(256), 0, s, p, S, ldS, sort_width(p.a.k));
    return hipGetLastError();
}

}  // namespace vr
