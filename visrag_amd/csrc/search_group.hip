// vr_index_search_groups: the k best GROUPS (documents: runs of adjacent rows, group g = rows [goff[g], goff[g + 1])) of the
// index per query, each with its best row — ranked by the fp32 score like vr_index_search, never by the bf16 one.
//
// With b_i the bf16-MFMA score of row i, e_i its fp32 score and |b_i - e_i| <= eps (search_common.h: query_eps), the group
// maxima B_g = max b_i and E_g = max e_i obey |B_g - E_g| <= eps too (max is 1-Lipschitz), so the certification of the deep
// path (search_bigk.hip) carries over with groups in the place of rows:
//   1. score rows S[q][row] of a block of <= 256 queries on the bf16 MFMA GEMM (the deep path's launch, index.h: score_block);
//   2. group_max_kernel: B[q][g] = max of S[q] over the group's rows (columns < n_docs only: the padding never wins);
//   3. group_select_kernel, one workgroup per query: the K' = k + 24 largest B_g in group order (search_select.h: the deep
//      path's radix select and ordered gather, over B in the place of S); inside every candidate group
//      each row with b_i >= B_g - 2 eps — only such a row can attain E_g, ties included — is re-scored in fp32 (dot_lane), the
//      largest key (score, then LOWER row id) is the group's (E_g, best row); the keys are sorted and certified:
//      tau = E_(k) - eps; a group outside the candidates has B_g <= the K'-th B, so if that lies below tau none of them can
//      reach the top k; otherwise EVERY group with B_g >= tau is gathered (<= 1024) and re-scored, else the query is flagged;
//   4. flagged queries: exact fp32 score rows (search_exact.hip, as it is), the same two kernels with eps = 0.
// Groups are runs of adjacent rows in row order, so "lower best row id first" among equal E_g is "lower group first".
#include <algorithm>

#include "kernels.h"
#include "search_rescore.h"

namespace vr {

constexpr int GRP_SHORT = 64;               // a group of up to this many rows is reduced by its own thread

// B[slot][g] = max over rows [goff[g], goff[g + 1]) of S[slot][row].  Thread t of a workgroup owns group blockIdx.x * 256 + t;
// a group longer than GRP_SHORT rows is reduced by the whole workgroup instead (a group may be the whole index).
__global__ __launch_bounds__(256) void group_max_kernel(const float* __restrict__ S, size_t ldS, const int* __restrict__ goff,
                                                        int n_groups, float* __restrict__ B, size_t ldB,
                                                        const int* __restrict__ slot_count, int sub) {
    __shared__ int s_lo[256], s_hi[256];
    __shared__ float red[4];
    const int slot = blockIdx.y;
    if (slot >= flag_slots(slot_count, sub, (int)gridDim.y)) return;       // (workgroup-uniform)
    const float* row = S + (size_t)slot * ldS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x * 256 + tid;
    const int lo = g < n_groups ? goff[g] : 0, hi = g < n_groups ? goff[g + 1] : 0;
    const bool is_long = hi - lo > GRP_SHORT;
    float m = -INFINITY;
    if (!is_long)
        for (int i = lo; i < hi; ++i) m = fmaxf(m, row[i]);
    if (__syncthreads_or(is_long)) {
        s_lo[tid] = lo; s_hi[tid] = hi;
        __syncthreads();
        for (int j = 0; j < 256; ++j) {
            const int jl = s_lo[j], jh = s_hi[j];
            if (jh - jl <= GRP_SHORT) continue;                             // (workgroup-uniform)
            float v = -INFINITY;
            for (int i = jl + tid; i < jh; i += 256) v = fmaxf(v, row[i]);
            v = wave_max(v);
            __syncthreads();                                                // (red of the previous long group has been read)
            if (lane == 0) red[wave] = v;
            __syncthreads();
            if (tid == j) m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        }
    }
    if (g < n_groups) B[(size_t)slot * ldB + g] = m;
}

// exact == 0: S / B rows of query blockIdx.x hold bf16-MFMA scores; the result is certified as described on top.
// exact == 1: S / B row i hold EXACT fp32 scores of flagged query flag_list[sub + i] (search_exact.hip): eps = 0, plain top-k.
__global__ __launch_bounds__(256) void group_select_kernel(GroupSearchArgs p, const float* __restrict__ S, size_t ldS,
                                                           int kp_want, int exact, int sub, int max_slots) {
    __shared__ SelectLds L;
    const int tid = threadIdx.x, lane = tid & 63;
    const SearchArgs& a = p.a;
    const int n_slots = exact ? flag_slots(a.flag_count, sub, max_slots) : (int)gridDim.x;
    for (int slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
    const int q = exact ? a.flag_list[sub + slot] : slot;
    const float* srow = S + (size_t)slot * ldS;
    const float* brow = p.B + (size_t)slot * p.ldB;
    const int n_groups = p.n_groups, k = a.k, dim = a.dim;
    __syncthreads();                                                    // (LDS of the previous slot is free)

    // ---- 3. candidate groups by B, per candidate the exact fp32 score of every row that can be the group's best, certification
    // (search_select.h: certified_select with groups in the place of rows; a group outside the re-scored set has B <= the K'-th)
    int kp = min(n_groups, kp_want);
    const KthKey kth = top_positions(brow, n_groups, kp, L);
    const int nv = dim >> 2;
    f32x4 qv[MERGE_MAXV];
    load_query_regs(qv, a.q_f32 + (size_t)q * dim, nv, lane);
    const float eps = exact ? 0.f : query_eps(a, qv);
    const bool certify = !exact && p.certify;
    unsigned dots = 0;                                                  // (not counted here)
    int what;
    float tau;
    kp = certified_select<false, true>(
        brow, n_groups, n_groups, kp, kth.T, k, certify,
        [&](int g) { return group_best_row(a, qv, srow, p.goff[g], p.goff[g + 1], band_lo(brow[g], eps), nv, lane, &dots); },
        [&] { return eps; }, L, &what, &tau);
    if (certify) {
        if (tid == 0) atomicAdd(&p.stats[what], 1u);
        __syncthreads();
        flag_query(a, q, what == 2, 0.f, &L.rank);
    }
    for (int c = tid; c < k; c += 256) {
        const uint64_t key = c < kp ? L.keys[c] : KEY_NONE;
        emit_slot(a, q, c, key);
        int g = -1;
        if (key != KEY_NONE) {                                           // the group of the row: last g with goff[g] <= row
            const int id = (int)(~(uint32_t)key);
            int l = 0, r = n_groups - 1;
            while (l < r) {
                const int mid = (l + r + 1) >> 1;
                if (p.goff[mid] <= id) l = mid; else r = mid - 1;
            }
            g = l;
        }
        p.out_groups[(size_t)q * k + c] = (int64_t)g;
    }
    }
}

int search_groups_kmax() { return SEL_CAND - SEL_MARGIN; }

static bool group_args_ok(const GroupSearchArgs& p) {
    const SearchArgs& a = p.a;
    return a.k >= 1 && a.k <= search_groups_kmax() && a.dim % 4 == 0 && a.dim <= 64 * 4 * MERGE_MAXV && p.n_groups >= 1 &&
           a.n_docs >= p.n_groups && p.goff && p.B && p.out_groups && a.out_scores && a.out_ids && !a.out_keys && a.flag_count &&
           a.flag_list && p.stats;
}

hipError_t launch_group_max(const float* S, size_t ldS, const int* goff, int n_groups, float* B, size_t ldB, int n_slots,
                            const int* slot_count, int sub, hipStream_t s) {
    if (n_slots <= 0) return hipSuccess;
    if (!S || !goff || !B || n_groups < 1 || n_slots > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_max_kernel, dim3((unsigned)((n_groups + 255) / 256), (unsigned)n_slots), dim3(256), 0, s, S, ldS,
                       goff, n_groups, B, ldB, slot_count, sub);
    return hipGetLastError();
}

// queries [0, nq_block) of the block view `p`: S / p.B hold their bf16-MFMA score rows and group maxima
hipError_t launch_group_select(const GroupSearchArgs& p, const float* S, size_t ldS, int nq_block, hipStream_t s) {
    if (nq_block <= 0) return hipSuccess;
    if (!group_args_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_select_kernel, dim3(nq_block), dim3(256), 0, s, p, S, ldS, p.a.k + SEL_MARGIN, 0, 0, 0);
    return hipGetLastError();
}

// the flagged queries from their exact score rows and group maxima (slot i = query flag_list[sub + i])
hipError_t launch_group_select_exact(const GroupSearchArgs& p, const float* S, size_t ldS, int sub, int max_slots, hipStream_t s) {
    if (max_slots <= 0) return hipSuccess;
    if (!group_args_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_select_kernel, dim3(max_slots < 128 ? max_slots : 128), dim3(256), 0, s, p, S, ldS, p.a.k, 1, sub,
                       max_slots);
    return hipGetLastError();
}

}  // namespace vr
