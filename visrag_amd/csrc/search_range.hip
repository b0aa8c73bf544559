// vr_index_search_range: EVERY row whose fp32 score reaches a query's threshold t — a result whose size is the answer, in CSR
// form (lims, scores, ids), ascending row id inside a query.  With b_i the bf16-MFMA score of row i, e_i its fp32 score and
// |b_i - e_i| <= eps (search_common.h: query_eps), every row with e_i >= t has b_i >= t - eps: re-scoring exactly the rows of
// that band in fp32 and keeping those with e_i >= t IS the fp32 answer.  No candidate margin, no widening, no flagged queries;
// a query costs what its band holds.  Per block of <= 256 queries (index_searches.hip):
//   1. score rows S[q][row] on the bf16 MFMA GEMM (the deep path's launch); with filters launch_filter_mask turns the columns a
//      query may not see into -inf in place, so that they can never be candidates;
//   2. range_rescore_kernel, grid (column chunk of 4096, query): the columns with b >= one_ulp_down(t - eps) are compacted into
//      an LDS list (search_rescore.h: chunk_scan), re-scored one candidate per wave with the query in registers (dot_lane + wave_sum: the
//      library's one fp32 dot product, so a row carries the score bits vr_index_search returns for it) and written back into S:
//      e where e >= t, -inf where not.  A non-candidate keeps its b < t - eps <= t.  From here on "S[q][row] >= t" is exactly
//      membership and the stored value is the score to return.  Kept rows are counted per 1024 columns (a wave's share of the
//      pack); queries, candidates and kept rows go to the 64-bit counters;
//   3. range_scan_kernel, one workgroup: exclusive scan of a query's (1024 columns) counts -> the offsets of the pack inside the
//      query's segment; scan of the queries' totals -> the block's part of lims and the block's total, which the host reads
//      (capacity check, growth of the result buffers);
//   4. range_pack_kernel, same grid: wave w of a workgroup compacts (score, id) of its 1024 columns with S >= t to the result
//      arrays at lims[q] + its scanned offset, in column order — no barrier, no sort.
// No kernel looks at or past column n_docs of a score row: the padded columns hold zeros and would pass any threshold <= 0.
// A threshold that is not finite, or a filter index outside [-1, n_filters) (on the device neither can be seen before the
// launch): an empty segment, nothing of S, of the index or of the filter store is read for that query.
#include "kernels.h"
#include "search_rescore.h"

namespace vr {

__device__ __forceinline__ int64_t range_subs(int64_t n_docs) { return (n_docs + RESCORE_SUB - 1) / RESCORE_SUB; }

__global__ __launch_bounds__(256) void range_rescore_kernel(RangeSearchArgs p, float* __restrict__ S, size_t ldS,
                                                            int* __restrict__ counts) {
    __shared__ ChunkLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchArgs& a = p.a;
    const int q = blockIdx.y, n_docs = (int)a.n_docs, nv = a.dim >> 2;
    const int c0 = blockIdx.x * RESCORE_CHUNK, c1 = min(c0 + RESCORE_CHUNK, n_docs);
    const int64_t nsub = range_subs(a.n_docs);
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
    const float bound = one_ulp_down(t - query_eps(a, qv));
    // ---- the band: columns with b >= bound (a masked column is -inf, the bound is finite)
    float* row = S + (size_t)q * ldS;
    chunk_scan<4, false>(row, c0, c1, bound, INFINITY, L);
    __syncthreads();
    // ---- fp32 re-scoring, one candidate per wave
    const int m = L.n_cand;
    for (int c = wave; c < m; c += 4) {
        const int id = L.cand[c];
        const float s = wave_sum(dot_lane(qv, a.index_f32 + (size_t)id * a.dim, nv, lane));
        if (lane == 0) {
            const bool keep = s >= t;
            row[id] = keep ? s : -INFINITY;
            if (keep) atomicAdd(&L.kept[(id - c0) / RESCORE_SUB], 1);
        }
    }
    __syncthreads();
    if (tid < my_subs) cnt[tid] = L.kept[tid];
    if (tid == 0 && m > 0) {
        atomicAdd(&p.stats[1], (unsigned long long)m);
        const int kept = L.kept[0] + L.kept[1] + L.kept[2] + L.kept[3];
        if (kept > 0) atomicAdd(&p.stats[2], (unsigned long long)kept);
    }
}

// One workgroup of 16 waves.  Wave w takes queries w, w + 16, ...: offs = exclusive scan of the query's counts in column order
// (64 counts per step, relative to the query's first entry).  Then thread q: lims[q + 1] = base + entries of the block's queries
// <= q (lims points at the block's first query, so lims[q] is where query q starts; the block that starts the call also writes
// lims[0] = 0: base == 0 there); *block_total = entries of the block.
__global__ __launch_bounds__(1024) void range_scan_kernel(const int* __restrict__ counts, int* __restrict__ offs, int64_t nsub, int nb,
                                                          int64_t base, int first, int64_t* __restrict__ lims,
                                                          int64_t* __restrict__ block_total) {
    __shared__ int qtot[256];
    __shared__ int64_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = wave; q < nb; q += 16) {
        int run = 0;                                                       // (a query's entries are rows: they fit an int)
        for (int64_t j0 = 0; j0 < nsub; j0 += 64) {
            const int64_t j = j0 + lane;
            const int c = j < nsub ? counts[(size_t)q * nsub + j] : 0;
            int incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            if (j < nsub) offs[(size_t)q * nsub + j] = run + incl - c;
            run += __shfl(incl, 63, 64);
        }
        if (lane == 0) qtot[q] = run;
    }
    __syncthreads();
    int64_t incl = tid < nb ? qtot[tid] : 0;                               // inclusive scan over the queries (waves 0..3 hold them)
    if (wave < 4) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up((long long)incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
    }
    __syncthreads();
    if (wave >= 4) return;
    for (int w = 0; w < wave; ++w) incl += wsum[w];
    if (tid < nb) lims[tid + 1] = base + incl;
    if (tid == 0 && first) lims[0] = 0;
    if (tid == nb - 1) *block_total = incl;
}

__global__ __launch_bounds__(256) void range_pack_kernel(RangeSearchArgs p, const float* __restrict__ S, size_t ldS,
                                                         const int* __restrict__ counts, const int* __restrict__ offs,
                                                         const int64_t* __restrict__ lims) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y, n_docs = (int)p.a.n_docs;
    const int s0 = blockIdx.x * RESCORE_CHUNK + wave * RESCORE_SUB, s1 = min(s0 + RESCORE_SUB, n_docs);
    if (s0 >= n_docs) return;                                              // (wave-uniform, no barrier below)
    const int64_t nsub = range_subs(p.a.n_docs);
    const size_t slot = (size_t)q * nsub + (size_t)blockIdx.x * RESCORE_SUBS + wave;
    if (counts[slot] == 0) return;                                         // (also: every query with an empty segment)
    const float t = p.thresholds[q];
    int64_t run = lims[q] + offs[slot];                                    // (lims: the block's first query's entry, as the scan got it)
    const float* row = S + (size_t)q * ldS;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i0 = s0 + lane * 4; i0 - lane * 4 < s1; i0 += 64 * 4) {       // (wave-uniform trip count: the ballots need every lane)
        f32x4 v = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (i0 < s1) v = *reinterpret_cast<const f32x4*>(row + i0);
        bool in[4];
        unsigned long long bm[4];
        int before = 0;                                                    // kept columns of the lower lanes
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            in[e] = i0 + e < s1 && v[e] >= t;
            bm[e] = __ballot(in[e]);
            before += __popcll(bm[e] & below);
        }
        int own = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (in[e]) {
                const int64_t o = run + before + own++;                    // (< lims[nq_block] <= the buffers' entries)
                p.out_scores[o] = v[e];
                p.out_ids[o] = (int64_t)(i0 + e);
            }
        run += __popcll(bm[0]) + __popcll(bm[1]) + __popcll(bm[2]) + __popcll(bm[3]);
    }
}

bool range_dim_ok(int dim) { return dim >= 4 && dim % 4 == 0 && dim <= 64 * 4 * MERGE_MAXV; }
int64_t range_scan_slots(int64_t n_docs) { return (n_docs + RESCORE_SUB - 1) / RESCORE_SUB; }

static bool range_args_ok(const RangeSearchArgs& p, size_t ldS, int nq_block) {
    return rescore_args_ok(p.a, nq_block) && p.thresholds && p.stats && ldS % 4 == 0 && (int64_t)ldS >= p.a.n_docs &&
           (!p.filter_of_query || p.n_filters >= 1);
}

hipError_t launch_range_rescore(const RangeSearchArgs& p, float* S, size_t ldS, int nq_block, int* counts, hipStream_t s) {
    if (!range_args_ok(p, ldS, nq_block) || !S || !counts) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.a.n_docs + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
    hipLaunchKernelGGL(range_rescore_kernel, dim3(chunks, (unsigned)nq_block), dim3(256), 0, s, p, S, ldS, counts);
    return hipGetLastError();
}

hipError_t launch_range_scan(const int* counts, int* offs, int64_t n_docs, int nq_block, int64_t base, int first, int64_t* lims,
                             int64_t* block_total, hipStream_t s) {
    if (!counts || !offs || !lims || !block_total || n_docs < 1 || nq_block < 1 || nq_block > 256 || base < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(1024), 0, s, counts, offs, range_scan_slots(n_docs), nq_block, base, first, lims,
                       block_total);
    return hipGetLastError();
}

hipError_t launch_range_pack(const RangeSearchArgs& p, const float* S, size_t ldS, int nq_block, const int* counts, const int* offs,
                             const int64_t* lims, hipStream_t s) {
    if (!range_args_ok(p, ldS, nq_block) || !S || !counts || !offs || !p.out_scores || !p.out_ids || !lims) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((p.a.n_docs + RESCORE_CHUNK - 1) / RESCORE_CHUNK);
    hipLaunchKernelGGL(range_pack_kernel, dim3(chunks, (unsigned)nq_block), dim3(256), 0, s, p, S, ldS, counts, offs, lims);
    return hipGetLastError();
}

}  // namespace vr
