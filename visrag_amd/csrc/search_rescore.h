// The steps the band searches share (search_range / rank / window .hip, their document forms search_group_*.hip, and the fused
// searches search_multi*.hip): each scores rows on the bf16 GEMM, finds the band of columns the fp32 answer can depend on,
// re-scores exactly that band in fp32 and selects.  One definition of each step; why a step is exact is argued in the header of
// the search that needs it.
//   chunk_scan      a workgroup's chunk of a row classified against [lo, hi]: ahead / in the band (listed in LDS) / behind;
//   group_best_row  (E_g, best row) of a document: the rows that can attain its maximum, one fp32 dot each;
//   present_count, group_eps, window_edges            what the edge kernels compute before the band is known;
//   fuse_columns    the column-wise max or min over a question's rows;
//   range_threshold, rescore_args_ok, topk_out_ok     the argument rules the searches share.
// The fp32 score itself is search_common.h's (exact_row_score), the selection search_select.h's.
#pragma once
#include "kernels.h"
#include "search_select.h"

namespace vr {

constexpr int RESCORE_CHUNK = 4096;         // columns per workgroup of a re-scoring kernel: 100 000 rows x 256 queries = 6 400 workgroups
constexpr int RESCORE_SUB = 1024;           // columns per wave of a range pack = granularity of its counts and scan (range_scan_slots)
constexpr int RESCORE_SUBS = RESCORE_CHUNK / RESCORE_SUB;

struct ChunkLds {                           // static LDS of a re-scoring kernel
    int cand[RESCORE_CHUNK];                // columns inside the band, any order (one slot per column of the chunk)
    int n_cand;
    unsigned ahead;                         // columns of this chunk ahead of the band (rank, window)
    int kept[RESCORE_SUBS];                 // band columns kept, per wave of the pack (range)
    unsigned long long dots;                // fp32 row dots of this workgroup (the document forms)
};

// Columns [c0, c1) of `row` by the whole workgroup, COLS per thread (4: a score row, c0 and its leading dimension multiples of
// 4, one 16-byte load; 1: a row of group maxima).  b > hi: certainly ahead, counted; lo <= b <= hi: the band, appended to
// L.cand; else (NaN included) behind.  A search without an upper edge passes hi = +inf: nothing is ahead, b <= hi holds for
// every number.  REWRITE: the row is rewritten so that it alone defines the answer — +inf ahead, -inf behind; a band column is
// written by the wave that re-scores it, a column at or past c1 by nobody, so every column has one writer.
// Zeroes L's counters first; the caller's barrier publishes the list.  Returns the wave's ahead count, complete in lane 0 (it
// leaves the loop last).
template <int COLS, bool REWRITE, typename F>
__device__ __forceinline__ unsigned chunk_scan(F* __restrict__ row, int c0, int c1, float lo, float hi, ChunkLds& L) {
    static_assert(COLS == 1 || COLS == 4, "one column or one 16-byte load per thread");
    const int tid = threadIdx.x;
    if (tid == 0) { L.n_cand = 0; L.ahead = 0u; L.dots = 0ull; }
    if (tid < RESCORE_SUBS) L.kept[tid] = 0;
    __syncthreads();
    unsigned ahead = 0;
    for (int i0 = c0 + tid * COLS; i0 < c1; i0 += 256 * COLS) {
        float b[COLS], w[COLS];
        if constexpr (COLS == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + i0);     // (aligned; < the leading dimension)
#pragma unroll
            for (int e = 0; e < 4; ++e) b[e] = v[e];
        } else {
            b[0] = row[i0];
        }
        bool in[COLS], any_band = false;
#pragma unroll
        for (int e = 0; e < COLS; ++e) {
            const bool valid = i0 + e < c1;
            const bool up = valid && b[e] > hi;
            in[e] = valid && b[e] >= lo && b[e] <= hi;
            w[e] = up ? INFINITY : -INFINITY;
            any_band |= in[e];
            ahead += (unsigned)__popcll(__ballot(up));
            band_append(in[e], i0 + e, L.cand, &L.n_cand);
        }
        if constexpr (REWRITE) {
            if constexpr (COLS == 4) {
                if (i0 + 4 <= c1 && !any_band) {
                    *reinterpret_cast<f32x4*>(row + i0) = f32x4{w[0], w[1], w[2], w[3]};
                    continue;
                }
            }
#pragma unroll
            for (int e = 0; e < COLS; ++e)
                if (i0 + e < c1 && !in[e]) row[i0 + e] = w[e];
        }
    }
    return ahead;
}

// (E_g, best row) of group rows [glo, ghi) as a key: every row whose bf16 score in srow reaches `lim` is re-scored in fp32 by
// the whole wave, the largest make_key(e, row) kept; *dots += rows re-scored.  The row that attains B_g passes
// lim = band_lo(B_g, eps): the result is a key.  Called by a whole wave with the query in qv; wave-uniform.
__device__ __forceinline__ uint64_t group_best_row(const SearchArgs& a, const f32x4 (&qv)[MERGE_MAXV], const float* __restrict__ srow,
                                                   int glo, int ghi, float lim, int nv, int lane, unsigned* dots) {
    uint64_t best = KEY_NONE;
    for (int i0 = glo; i0 < ghi; i0 += 64) {
        const int i = i0 + lane;
        unsigned long long in = __ballot(i < ghi && srow[i] >= lim);
        *dots += (unsigned)__popcll(in);
        while (in) {                                                       // (wave-uniform)
            const int id = i0 + __ffsll((long long)in) - 1;
            in &= in - 1ull;
            const uint64_t key = make_key(exact_row_score(a, qv, id, nv, lane), (uint32_t)id);
            best = key > best ? key : best;
        }
    }
    return best;
}

// how many of row[0, n) are present (> -inf: a group with a row that filter f allows): all n without a filter, none for an
// index outside [-1, n_filters) — the mask left such a row alone, and nobody reads it.  Whole workgroup, f uniform; sh: LDS.
__device__ __forceinline__ int present_count(const float* __restrict__ row, int n, int f, int n_filters, int* sh) {
    if (f == -1) return n;
    if (!filter_index_ok(f, n_filters)) return 0;
    const int tid = threadIdx.x;
    if (tid == 0) *sh = 0;
    __syncthreads();
    int mine = 0;                           // (every lane of a wave holds the wave's count)
    for (int g0 = 0; g0 < n; g0 += 256) {
        const int g = g0 + tid;
        mine += __popcll(__ballot(g < n && row[g] > -INFINITY));
    }
    if ((tid & 63) == 0 && mine) atomicAdd(sh, mine);
    __syncthreads();
    return *sh;
}

// eps_g = the largest query_eps of sub-queries [s0, s0 + m), a wave each; eps_sub (or null) gets every one.  Whole workgroup;
// sh: LDS[4].
__device__ __forceinline__ float group_eps(const SearchArgs& a, int s0, int m, float* __restrict__ eps_sub, float* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float eps = 0.f;
    for (int j = wave; j < m; j += 4) {                                    // (wave-uniform)
        f32x4 qv[MERGE_MAXV];
        load_query_regs(qv, a.q_f32 + (size_t)(s0 + j) * a.dim, a.dim >> 2, lane);
        const float e = query_eps(a, qv);
        if (eps_sub && lane == 0) eps_sub[s0 + j] = e;
        eps = fmaxf(eps, e);
    }
    if (lane == 0) sh[wave] = eps;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

struct BandEdges { float lo, hi; };

// the band of the window at ranks [o, kz) of vals[0, n): two radix selects give v_a (rank o + 1) and v_z (rank kz), both
// edges 2 eps outside them and rounded outward.  Whole workgroup, the LDS free.
__device__ __forceinline__ BandEdges window_edges(const float* __restrict__ vals, int n, int o, int kz, float eps, SelectLds& L) {
    const KthKey ka = select_kth(vals, n, o + 1, L);
    __syncthreads();
    const KthKey kzk = select_kth(vals, n, kz, L);
    return BandEdges{band_lo(orderable_f32(kzk.T), eps), band_hi(orderable_f32(ka.T), eps)};
}

// dst[i] = multi_pick over rows j < m of src[j * ld_src + i] for the thread's four columns i of [0, n) (grid x: 1024 columns;
// src, dst and ld_src multiples of 4 floats: 16-byte loads, also over the last columns — < ld_src — which are never stored).
// dst == src: in place, into the first row.
__device__ __forceinline__ void fuse_columns(const float* src, size_t ld_src, int m, float* dst, int n, int fuse) {
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    f32x4 v = *reinterpret_cast<const f32x4*>(src + i0);
    for (int j = 1; j < m; ++j) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(src + (size_t)j * ld_src + i0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = multi_pick(v[e], w[e], fuse);
    }
    if (i0 + 4 <= n) {
        *reinterpret_cast<f32x4*>(dst + i0) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < n) dst[i0 + e] = v[e];
    }
}
constexpr int FUSE_COLS = 256 * 4;          // columns per workgroup of fuse_columns

// the threshold of query q, or NaN for a query that gets an empty segment: a threshold that is not finite, or a filter index
// outside [-1, n_filters) (workgroup-uniform)
__device__ __forceinline__ float range_threshold(const float* __restrict__ thresholds, const int* __restrict__ filter_of_query,
                                                 int n_filters, int q) {
    const float t = thresholds[q];
    const bool ok = t == t && fabsf(t) != INFINITY && filter_index_ok(filter_of_query ? filter_of_query[q] : -1, n_filters);
    return ok ? t : __builtin_nanf("");
}

// ---- host: what every launcher of these searches asks of its SearchArgs and its block of n_block (sub-)queries
inline bool rescore_args_ok(const SearchArgs& a, int n_block) {
    return n_block >= 1 && n_block <= 256 && a.n_docs >= 1 && a.n_docs < ((int64_t)1 << 31) && range_dim_ok(a.dim) && a.index_f32 &&
           a.q_f32 && a.dmax && (a.eps_data || a.eps_rel >= 0.f);
}
// ... and of the k result slots per query, where it emits them
inline bool topk_out_ok(const SearchArgs& a) {
    return a.k >= 1 && a.k <= SEL_CAND - SEL_MARGIN && a.out_scores && a.out_ids && !a.out_keys;
}

}  // namespace vr
