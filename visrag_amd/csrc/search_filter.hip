// vr_index_search_filtered: the k best rows per query AMONG THE ROWS ITS FILTER ALLOWS — ranked by the fp32 score like
// vr_index_search, never by the bf16 one.  A filter is a bit set over the rows (bit r & 31 of word r >> 5; vr_index_set_filters
// keeps the library's own copy with the bits at or beyond the row count cleared, and every filter's number of allowed rows);
// filter_of_query[q] names the filter of query q, -1 = all rows.
//
// The allowed rows of a query form a sub-index, and the result is what vr_index_search returns on that sub-index with the
// original row ids.  With b_i the bf16-MFMA score of row i, e_i its fp32 score and |b_i - e_i| <= eps (search_common.h:
// query_eps — the index-wide max |d| and max |d - bf16(d)| bound those of any subset of the rows, so the eps of the whole
// index holds for the sub-index, only looser), the certification of the deep path (search_bigk.hip) applies verbatim with
// na = the number of allowed rows in the place of n_docs:
//   1. score rows S[q][row] of a block of <= 256 queries on the bf16 MFMA GEMM (the deep path's launch, index.h: score_block);
//   2. filter_mask_kernel: the disallowed columns of S become -inf in place (S is scratch), the filter words read once per 32
//      columns — from here on a disallowed row cannot be selected, gathered or re-scored, and search_select.h stays as it is;
//      the select never looks past column n_docs, so the zero scores of the index's padded columns never win either;
//   3. filter_select_kernel, one workgroup per query: K' = min(na, k + 24) rows of largest b_i in row order (radix select and
//      ordered gather over the masked row: K' <= na, so the threshold is a finite score and no -inf column is gathered),
//      re-scored in fp32 (dot_lane) and sorted.  K' = na: every allowed row was re-scored, certified at once.  Otherwise
//      tau = E_(k) - eps; an allowed row outside the candidates has b_i <= the K'-th b, so if that lies below tau none of them
//      can reach the top k; else EVERY allowed row with b_i >= tau is gathered (<= 1024) and re-scored, else the query is flagged;
//   4. flagged queries: exact fp32 score rows (search_exact.hip, as it is), masked the same way — slot i belongs to query
//      flag_list[sub + i], whose filter masks it — and the same select with eps = 0 and K' = min(na, k).
// na = 0 (an empty filter, or — filter_of_query on the device cannot be checked before the launch — an entry outside
// [-1, n_filters)): k empty slots, nothing of S or of the filter store is read.
// One route whatever the filter's density: the GEMM over 100 000 rows costs ~137 us per 256 queries; gathering and scoring a few
// thousand allowed fp32 rows per query on the VALU is not cheaper.
#include <algorithm>

#include "kernels.h"
#include "search_select.h"

namespace vr {

constexpr int FILT_COLS = 4;                // columns per thread of the mask kernel (one 16-byte store)

// The library's copy of filter blockIdx.x: bits at or beyond n_rows cleared, allowed[f] = its population count.
__global__ __launch_bounds__(256) void filter_prepare_kernel(uint32_t* __restrict__ bits, size_t words, int64_t n_rows,
                                                             int* __restrict__ allowed) {
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* w = bits + (size_t)blockIdx.x * words;
    const int spare = (int)(words * 32 - (size_t)n_rows);                  // 0..31 bits of the last word
    int c = 0;
    for (size_t i = tid; i < words; i += 256) {
        uint32_t v = w[i];
        if (i == words - 1 && spare > 0) { v &= 0xFFFFFFFFu >> spare; w[i] = v; }
        c += __popc(v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) red[wave] = c;
    __syncthreads();
    if (tid == 0) allowed[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Score row blockIdx.y (query blockIdx.y of the block, or with a flag list the query flag_list[sub + blockIdx.y]): columns the
// query's filter does not allow become -inf.  Thread t of workgroup x owns columns (x * 256 + t) * 4 .. + 3 (< words * 32 <= ldS).
__global__ __launch_bounds__(256) void filter_mask_kernel(float* __restrict__ S, size_t ldS, const uint32_t* __restrict__ bits,
                                                          size_t words, int n_filters, const int* __restrict__ filter_of_query,
                                                          const int* __restrict__ flag_list, const int* __restrict__ slot_count,
                                                          int sub) {
    const int slot = blockIdx.y;
    if (slot >= flag_slots(slot_count, sub, (int)gridDim.y)) return;       // (workgroup-uniform)
    const int q = flag_list ? flag_list[sub + slot] : slot;
    const int f = filter_of_query[q];
    if ((unsigned)f >= (unsigned)n_filters) return;                        // -1: all rows; out of range: the select reads no score
    const size_t c0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * FILT_COLS;
    if ((c0 >> 5) >= words) return;
    const uint32_t nib = (bits[(size_t)f * words + (c0 >> 5)] >> (c0 & 31)) & 0xFu;
    if (nib == 0xFu) return;
    float* dst = S + (size_t)slot * ldS + c0;
    if (nib == 0u) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    } else {
#pragma unroll
        for (int e = 0; e < FILT_COLS; ++e)
            if (!((nib >> e) & 1u)) dst[e] = -INFINITY;
    }
}

// exact == 0: S rows hold the MASKED bf16-MFMA scores of queries blockIdx.x; the result is certified as described on top.
// exact == 1: S row i holds the MASKED exact fp32 scores of flagged query flag_list[sub + i]: eps = 0, plain top-k of it.
__global__ __launch_bounds__(256) void filter_select_kernel(FilterSearchArgs p, const float* __restrict__ S, size_t ldS,
                                                            int kp_want, int exact, int sub, int max_slots) {
    __shared__ SelectLds L;
    const int tid = threadIdx.x, lane = tid & 63;
    const SearchArgs& a = p.a;
    const int n_slots = exact ? flag_slots(a.flag_count, sub, max_slots) : (int)gridDim.x;
    for (int slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
    const int q = exact ? a.flag_list[sub + slot] : slot;
    const float* row = S + (size_t)slot * ldS;
    const int n_docs = (int)a.n_docs, k = a.k, dim = a.dim;
    const int na = rows_allowed(a.n_docs, p.n_filters, p.allowed, p.filter_of_query[q]);    // (workgroup-uniform)
    __syncthreads();                                                    // (LDS of the previous slot is free)
    if (na == 0) {                                                      // nothing allowed: k empty slots, certified
        for (int c = tid; c < k; c += 256) emit_slot(a, q, c, KEY_NONE);
        if (!exact && p.certify && tid == 0) atomicAdd(&p.stats[0], 1u);
        continue;
    }

    // ---- 3. candidates among the masked row (K' <= na, so the K'-th is a finite score and no masked column is gathered),
    // exact fp32 re-scoring, certification (search_select.h: certified_select with na in the place of the row count; an allowed
    // row outside the re-scored set has a bf16 score <= the K'-th; K' == na: there is none)
    int kp = min(na, kp_want);
    const KthKey kth = top_positions(row, n_docs, kp, L);
    const int nv = dim >> 2;
    f32x4 qv[MERGE_MAXV];
    load_query_regs(qv, a.q_f32 + (size_t)q * dim, nv, lane);
    const bool certify = !exact && p.certify;
    int what;
    float tau;
    kp = certified_select<false, true>(
        row, n_docs, na, kp, kth.T, k, certify,
        [&](int id) { return make_key(wave_sum(dot_lane(qv, a.index_f32 + (size_t)id * dim, nv, lane)), (uint32_t)id); },
        [&] { return query_eps(a, qv); }, L, &what, &tau);
    if (certify) {
        if (tid == 0) atomicAdd(&p.stats[what], 1u);
        __syncthreads();
        flag_query(a, q, what == 2, 0.f, &L.rank);
    }
    for (int c = tid; c < k; c += 256) emit_slot(a, q, c, c < kp ? L.keys[c] : KEY_NONE);
    }
}

static bool filter_args_ok(const FilterSearchArgs& p) {
    const SearchArgs& a = p.a;
    return a.k >= 1 && a.k <= SEL_CAND - SEL_MARGIN && a.dim % 4 == 0 && a.dim <= 64 * 4 * MERGE_MAXV && a.n_docs >= 1 &&
           p.n_filters >= 1 && p.words == (size_t)((a.n_docs + 31) / 32) && p.bits && p.allowed && p.filter_of_query &&
           a.out_scores && a.out_ids && !a.out_keys && a.flag_count && a.flag_list && p.stats;
}

hipError_t launch_filter_prepare(uint32_t* bits, size_t words, int n_filters, int64_t n_rows, int* allowed, hipStream_t s) {
    if (!bits || !allowed || n_filters < 1 || n_rows < 1 || words != (size_t)((n_rows + 31) / 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_prepare_kernel, dim3((unsigned)n_filters), dim3(256), 0, s, bits, words, n_rows, allowed);
    return hipGetLastError();
}

// score rows [0, n_slots) of S (slot_count set: only the first *slot_count - sub of them, slot i = query flag_list[sub + i])
hipError_t launch_filter_mask(const MaskArgs& m, float* S, size_t ldS, int n_slots, const int* flag_list, const int* slot_count,
                              int sub, hipStream_t s) {
    if (n_slots <= 0) return hipSuccess;
    if (!m.bits || !m.filter_of_query || m.n_filters < 1 || m.n_docs < 1 || m.words != (size_t)((m.n_docs + 31) / 32) ||
        (slot_count && !flag_list) || !S || n_slots > 65535 || m.words * 32 > ldS || ldS % FILT_COLS)
        return hipErrorInvalidValue;
    const size_t per_wg = 256 * FILT_COLS / 32;                            // filter words per workgroup
    hipLaunchKernelGGL(filter_mask_kernel, dim3((unsigned)((m.words + per_wg - 1) / per_wg), (unsigned)n_slots), dim3(256), 0, s, S,
                       ldS, m.bits, m.words, m.n_filters, m.filter_of_query, slot_count ? flag_list : nullptr, slot_count, sub);
    return hipGetLastError();
}

// queries [0, nq_block) of the block view `p`: S holds their masked bf16-MFMA score rows
hipError_t launch_filter_select(const FilterSearchArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s) {
    if (nq_block <= 0) return hipSuccess;
    if (!filter_args_ok(p) || !S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_select_kernel, dim3(nq_block), dim3(256), 0, s, p, S, ldS, p.a.k + SEL_MARGIN, 0, 0, 0);
    return hipGetLastError();
}

// the flagged queries from their masked exact score rows (slot i = query flag_list[sub + i])
hipError_t launch_filter_select_exact(const FilterSearchArgs& p, const float* S, size_t ldS, int sub, int max_slots, hipStream_t s) {
    if (max_slots <= 0) return hipSuccess;
    if (!filter_args_ok(p) || !S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_select_kernel, dim3(max_slots < 128 ? max_slots : 128), dim3(256), 0, s, p, S, ldS, p.a.k, 1, sub,
                       max_slots);
    return hipGetLastError();
}

}  // namespace vr
