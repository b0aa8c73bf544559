// vr_index_search_multi_groups: the k DOCUMENTS (groups of adjacent rows, vr_index_set_groups) of largest fused score per question
// (a group of sub-queries, as vr_index_search_multi takes it), with the evidence: the best page per sub-question.  For question g
// with sub-queries j, filter f and document D:
//   D is PRESENT if f allows one of its pages;  E_j(D) = max e_j(i) over its ALLOWED pages i, row_j(D) the lowest allowed row that
//   attains it;  F(D) = max_j E_j(D) (fuse = max, "any-of") or min_j E_j(D) (fuse = min, "all-of");  which(D) the lowest j whose
//   E_j(D) has exactly F(D)'s bits, best_row(D) = row_which(D).
// e_j(i) is the library's one fp32 score (dot_regs + wave_sum, the bits vr_index_search returns for that pair); every max and min
// is taken on f32_orderable keys (-0.0 < +0.0).  Present documents rank by F descending, then lower document first.
// Why it is exact:
//   1. within the allowed rows |b_j(i) - e_j(i)| <= eps_j for the bf16-MFMA score b_j (search_common.h: query_eps);
//   2. max over a fixed set is 1-Lipschitz in the sup norm: the masked document maximum B_j(D) = max b_j(i) over the allowed pages
//      lies within eps_j of E_j(D) (search_group.hip's argument);
//   3. so are max and min over the question's sub-queries: the fused bf16 value BF(D) = max_j B_j(D) (or min) lies within
//      eps_g := max_j eps_j of F(D) (search_multi.hip's argument);
//   4. so are order statistics: the r-th largest BF lies within eps_g of the r-th largest F (search_window.hip's argument);
//   5. let v_z be the min(k, present)-th largest BF.  Every document of the result has F >= v_z - eps_g, hence BF >= v_z - 2 eps_g;
//      a document with BF(D) < v_z - 2 eps_g is strictly behind the whole result, and at offset 0 nothing is ahead of it.  So exactly
//      the documents with BF >= lo = one_ulp_down(v_z - 2 eps_g) form the BAND (the rounded subtraction cannot have narrowed it);
//   6. inside a band document, for sub-query j, only a page with b_j(i) >= B_j(D) - 2 eps_j can attain E_j(D), ties included:
//      e_j(i) = E_j(D) >= B_j(D) - eps_j gives b_j(i) >= e_j(i) - eps_j >= B_j(D) - 2 eps_j.  Exactly those pages get one fp32 dot
//      each; the largest make_key(e, row) is (E_j(D), row_j(D)).  A page the filter forbids carries b = -inf and is never one;
//   7. no candidate margin, no widening, no flagged questions: exact in every setting of vr_index_set_search_eps; with
//      certification off the default error model defines eps.
// The host (index_searches.hip) packs whole questions greedily into blocks of <= 256 sub-queries.  Per block:
//   1. score rows S[sub-query][row] on the bf16 MFMA GEMM, the question's filter expanded to its sub-queries and masked to -inf
//      (multi_expand_kernel, launch_filter_mask), group_max_kernel (search_group.hip, as it is) into B[sub-query][document]: a
//      document without an allowed page is -inf in every sub-row.  S and B are only read from here on;
//   2. multi_group_fuse_kernel, grid (chunk of 1024 documents, question): BF = the column-wise max or min of the question's B rows,
//      into the question's row of the SEPARATE array F;
//   3. multi_group_edge_kernel, one workgroup per question: eps_j of every sub-query (kept in eps_sub for the kernels behind it)
//      and their max eps_g; the present count — the document count without a filter, a workgroup count of BF > -inf with one, 0
//      for a filter index outside [-1, n_filters) (a device caller's cannot be checked before the launch; the mask left such rows
//      alone and from here on nobody reads them); none present: the question is empty (lo = NaN).  Otherwise a radix select over
//      the F row gives v_z (rank <= present: not an absent document's -inf) and lo;
//   4. multi_group_rescore_kernel, grid (chunk of 4096 documents, question): the F row is REWRITTEN in place: -inf below lo (or
//      absent), and for the band — compacted into an LDS list (search_rescore.h: chunk_scan), one wave per document — F(D).  The
//      wave loops over the question's sub-queries; for each, group_best_row gives every page of the document with
//      b_j(i) >= one_ulp_down(B_j(D) - 2 eps_j) one fp32 dot, the row's loads issued in front of the fma chain.  A document longer than a chunk of pages — the whole index may be one — is still one wave's loop.  A column is
//      written by one thread only: below the band by the thread that classified it, inside by lane 0 of its wave;
//   5. multi_group_select_kernel, one workgroup per question: radix select at rank min(k, present) of the rewritten row,
//      gather_ordered (lowest documents first inside the last tie tier), keys make_key(F, document), block_bitonic_desc, k slots;
//      which, best_row and the evidence are recomputed for the winners only, a wave per slot over the question's sub-queries (the
//      same walk as in 4: the same bits) — no side buffer proportional to documents x sub-queries.
// No kernel waits for another workgroup; stream order between the launches is the only ordering.  No kernel reads as a value, or
// writes, an S column at or past n_docs or a B / F column at or past n_groups.
#include "kernels.h"
#include "search_rescore.h"

namespace vr {

struct MultiGroupEdgeLds {
    SelectLds s;
    float eps[4];                           // group_eps: the largest query_eps every wave met
    int present;
};

__global__ __launch_bounds__(256) void multi_group_fuse_kernel(MultiGroupArgs p) {
    const int g = blockIdx.y, ng = p.n_groups;
    const int s0 = p.lims[g] - p.sub_base, m = p.lims[g + 1] - p.lims[g];
    fuse_columns(p.B + (size_t)s0 * p.ldB, p.ldB, m, p.F + (size_t)g * p.ldB, ng, p.fuse);
}

__global__ __launch_bounds__(256) void multi_group_edge_kernel(MultiGroupArgs p) {
    __shared__ MultiGroupEdgeLds L;
    const int tid = threadIdx.x;
    const SearchArgs& a = p.a;
    const int g = blockIdx.x, ng = p.n_groups;
    if (g == 0 && tid == 0) atomicAdd(&p.stats[0], (unsigned long long)gridDim.x);
    const float* frow = p.F + (size_t)g * p.ldB;
    // nd = the documents with an allowed page (workgroup-uniform)
    const int nd = present_count(frow, ng, p.filter_of_group ? p.filter_of_group[g] : -1, p.n_filters, &L.present);
    if (tid == 0) p.present[g] = nd;
    if (nd <= 0) {                                                         // (workgroup-uniform) nothing present: a row of tails
        if (tid == 0) p.edges[g] = __builtin_nanf("");
        return;
    }
    const int s0 = p.lims[g] - p.sub_base, m = p.lims[g + 1] - p.lims[g];
    const float eps_g = group_eps(a, s0, m, p.eps_sub, L.eps);
    const KthKey kz = select_kth(frow, ng, min(a.k, nd), L.s);
    if (tid == 0) p.edges[g] = band_lo(orderable_f32(kz.T), eps_g);
}

__global__ __launch_bounds__(256) void multi_group_rescore_kernel(MultiGroupArgs p, const float* __restrict__ S, size_t ldS) {
    __shared__ ChunkLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int g = blockIdx.y, ng = p.n_groups, nv = a.dim >> 2;
    const float lo = p.edges[g];
    if (lo != lo) return;                                                  // (workgroup-uniform) an empty question
    const int s0 = p.lims[g] - p.sub_base, m = p.lims[g + 1] - p.lims[g];
    const int c0 = blockIdx.x * RESCORE_CHUNK, c1 = min(c0 + RESCORE_CHUNK, ng);
    // ---- certainly behind or absent: BF < lo -> -inf; the band BF >= lo: listed
    float* frow = p.F + (size_t)g * p.ldB;
    chunk_scan<1, true>(frow, c0, c1, lo, INFINITY, L);
    __syncthreads();
    // ---- the band: one wave per document, every sub-query of the question, one fp32 dot for every page that can attain E_j(D)
    const int n = L.n_cand;
    unsigned dots = 0;
    for (int c = wave; c < n; c += 4) {
        const int d = L.cand[c];
        const int glo = p.goff[d], ghi = p.goff[d + 1];
        float fused = 0.f;
        for (int j = 0; j < m; ++j) {
            f32x4 qv[MERGE_MAXV];
            load_query_regs(qv, a.q_f32 + (size_t)(s0 + j) * a.dim, nv, lane);
            const float lim = band_lo(p.B[(size_t)(s0 + j) * p.ldB + d], p.eps_sub[s0 + j]);
            const float e = key_score(group_best_row(a, qv, S + (size_t)(s0 + j) * ldS, glo, ghi, lim, nv, lane, &dots));
            fused = j == 0 ? e : multi_pick(fused, e, p.fuse);
        }
        if (lane == 0) frow[d] = fused;
    }
    if (lane == 0 && dots) atomicAdd(&L.dots, (unsigned long long)dots);
    __syncthreads();
    if (tid == 0 && n > 0) {
        atomicAdd(&p.stats[1], (unsigned long long)n);
        atomicAdd(&p.stats[2], L.dots);
    }
}

__global__ __launch_bounds__(256) void multi_group_select_kernel(MultiGroupArgs p, const float* __restrict__ S, size_t ldS, int n_sort) {
    __shared__ SelectLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int g = blockIdx.x, ng = p.n_groups, k = a.k, nv = a.dim >> 2;
    const int m = p.lims[g + 1] - p.lims[g];
    const size_t o0 = (size_t)g * k;
    const size_t ev0 = (size_t)k * (size_t)p.lims[g];                      // the question's evidence block [k][m]
    const bool ev = p.out_ev_scores != nullptr;
    const float lo = p.edges[g];
    const int kz = lo != lo ? 0 : min(k, p.present[g]);                    // (workgroup-uniform) an empty question: k tails
    // ---- the tails: slots at or past the present documents
    for (int c = kz + tid; c < k; c += 256) {
        a.out_scores[o0 + c] = -INFINITY; a.out_ids[o0 + c] = -1; p.out_docs[o0 + c] = -1; p.out_which[o0 + c] = -1;
    }
    if (ev)
        for (size_t t = (size_t)kz * m + tid; t < (size_t)k * m; t += 256) { p.out_ev_scores[ev0 + t] = -INFINITY; p.out_ev_rows[ev0 + t] = -1; }
    if (kz == 0) return;
    const int s0 = p.lims[g] - p.sub_base;
    const float* frow = p.F + (size_t)g * p.ldB;
    top_positions(frow, ng, kz, L);                                        // (>= kz columns hold a fp32 fused score)
    sort_gathered(frow, kz, n_sort, L);
    // ---- the winners: which sub-query decided, its page, and the evidence — a wave per slot, the re-scoring's walk again
    unsigned dots = 0;
    for (int c = wave; c < kz; c += 4) {
        const uint64_t key = L.keys[c];
        const int d = (int)(~(uint32_t)key);
        const uint32_t fbits = __float_as_uint(key_score(key));
        const int glo = p.goff[d], ghi = p.goff[d + 1];
        int w = -1;
        long long wrow = -1;
        for (int j = 0; j < m; ++j) {
            f32x4 qv[MERGE_MAXV];
            load_query_regs(qv, a.q_f32 + (size_t)(s0 + j) * a.dim, nv, lane);
            const float lim = band_lo(p.B[(size_t)(s0 + j) * p.ldB + d], p.eps_sub[s0 + j]);
            const uint64_t best = group_best_row(a, qv, S + (size_t)(s0 + j) * ldS, glo, ghi, lim, nv, lane, &dots);
            const float e = key_score(best);
            const long long row = (long long)(~(uint32_t)best);
            if (w < 0 && __float_as_uint(e) == fbits) { w = j; wrow = row; }
            if (ev && lane == 0) { p.out_ev_scores[ev0 + (size_t)c * m + j] = e; p.out_ev_rows[ev0 + (size_t)c * m + j] = row; }
        }
        if (lane == 0) {
            a.out_scores[o0 + c] = key_score(key); a.out_ids[o0 + c] = wrow; p.out_docs[o0 + c] = d; p.out_which[o0 + c] = w;
        }
    }
}

static bool multi_group_args_ok(const MultiGroupArgs& p, int n_questions) {
    const SearchArgs& a = p.a;
    return rescore_args_ok(a, n_questions) && topk_out_ok(a) && a.nq >= n_questions && a.nq <= 256 && p.n_groups >= 1 &&
           a.n_docs >= p.n_groups && p.out_docs && p.out_which && (p.out_ev_scores != nullptr) == (p.out_ev_rows != nullptr) &&
           p.lims && p.sub_base >= 0 && (p.fuse == 0 || p.fuse == 1) && p.goff && p.B && p.F && p.ldB % 4 == 0 &&
           (int64_t)p.ldB >= p.n_groups && p.eps_sub && p.edges && p.present && p.stats && (!p.filter_of_group || p.n_filters >= 1);
}

hipError_t launch_multi_group_fuse(const MultiGroupArgs& p, int n_questions, hipStream_t s) {
    if (!multi_group_args_ok(p, n_questions)) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.n_groups + FUSE_COLS - 1) / FUSE_COLS);
    hipLaunchKernelGGL(multi_group_fuse_kernel, dim3(chunks, (unsigned)n_questions), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_multi_group_edges(const MultiGroupArgs& p, int n_questions, hipStream_t s) {
    if (!multi_group_args_ok(p, n_questions)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(multi_group_edge_kernel, dim3((unsigned)n_questions), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_multi_group_rescore(const MultiGroupArgs& p, const float* S, size_t ldS, int n_questions, hipStream_t s) {
    if (!multi_group_args_ok(p, n_questions) || !S || (int64_t)ldS < p.a.n_docs) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.n_groups + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
    hipLaunchKernelGGL(multi_group_rescore_kernel, dim3(chunks, (unsigned)n_questions), dim3(256), 0, s, p, S, ldS);
    return hipGetLastError();
}

hipError_t launch_multi_group_select(const MultiGroupArgs& p, const float* S, size_t ldS, int n_questions, hipStream_t s) {
    if (!multi_group_args_ok(p, n_questions) || !S || (int64_t)ldS < p.a.n_docs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(multi_group_select_kernel, dim3((unsigned)n_questions), dim3(256), 0, s, p, S, ldS, sort_width(p.a.k));
    return hipGetLastError();
}

}  // namespace vr
