// vr_index_search_diverse: k rows per query picked from a POOL of its best rows by maximal marginal relevance (MMR), so that
// near-duplicate rows do not fill the result.  The pool is what vr_index_search / vr_index_search_filtered return for k = pool
// (index_searches.hip calls them as they stand: certified, fp32 scores r_c, (-inf, -1) tail where fewer rows exist); this file holds the
// selection over it.
//
// mmr_select_kernel, one workgroup of 256 threads per query:
//   pick 0  = pool position 0;
//   pick t  = the unselected member c of largest  v_c = lambda r_c - (1 - lambda) m_c,  m_c = max over the picked rows j of
//             <d_c, d_j>, the lower pool position among equal v.
// m_c is a running maximum in LDS: after a pick its fp32 row goes into registers (load_query_regs) and every unselected member
// is scored against it with the library's ONE fp32 dot product (search_common.h: dot_lane's chain + wave_sum, wave w takes
// members w, w + 4, ...) — the re-scoring loop of search_filter.hip with a row in the place of the query.  (k - 1) P' dots per query,
// rows L2-resident after the first pick.  Every member's dot takes the same lane assignment and summation order whichever wave
// computes it, so bit-identical rows carry bit-identical m, r and v and the tie rule (lower position) decides between them.
// The argmax is a workgroup maximum over packed keys: orderable bits of v in the high word, ~position in the low word.
// No bf16 anywhere: v is decided by fp32 dots of fp32 rows.  No counters: the pool stage counts in its search's statistics.
#include "kernels.h"
#include "search_common.h"

namespace vr {

constexpr int MMR_POOL = 1000;              // members per query held in LDS (= search_bigk_max())

struct MmrLds {
    int id[MMR_POOL];                       // row of pool position c
    float r[MMR_POOL];                      // its fp32 score as the search returned it
    float m[MMR_POOL];                      // largest dot with a picked row so far
    int taken[MMR_POOL];
    uint64_t red[4];                        // the waves' best keys of the pick at hand
    int np;                                 // members: the positions in front of the first entry that is no row
};

__global__ __launch_bounds__(256) void mmr_select_kernel(MmrArgs p) {
    __shared__ MmrLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pool = p.pool, k = p.k, dim = p.dim, nv = dim >> 2;
    const float lam = p.lambda, oml = 1.0f - p.lambda;
    for (int q = blockIdx.x; q < p.nq; q += gridDim.x) {
        __syncthreads();                                                // (LDS of the previous query is free)
        // ---- the pool: its members are a prefix of the search's result, the (-inf, -1) tail behind them is not part of it
        if (tid == 0) L.np = pool;
        __syncthreads();
        for (int c = tid; c < pool; c += 256) {
            const int64_t id = p.pool_ids[(size_t)q * pool + c];
            const bool member = id >= 0 && id < p.n_docs;
            L.id[c] = member ? (int)id : -1;
            L.r[c] = p.pool_scores[(size_t)q * pool + c];
            L.m[c] = -INFINITY;
            L.taken[c] = 0;
            if (!member) atomicMin(&L.np, c);
        }
        __syncthreads();
        const int np = L.np;                                            // every position below it holds a row of the index
        const int n_pick = min(k, np);
        float* os = p.out_scores + (size_t)q * k;
        int64_t* oi = p.out_ids + (size_t)q * k;
        for (int c = n_pick + tid; c < k; c += 256) { os[c] = -INFINITY; oi[c] = -1; }
        if (n_pick == 0) continue;
        int b = 0;                                                      // pick 0: the best row of the pool
        if (tid == 0) { L.taken[0] = 1; os[0] = L.r[0]; oi[0] = L.id[0]; }
        __syncthreads();
        for (int t = 1; t < n_pick; ++t) {
            // ---- m_c = max(m_c, <d_c, picked row>) for every unselected member
            f32x4 pv[MERGE_MAXV];
            load_query_regs(pv, p.index_f32 + (size_t)L.id[b] * dim, nv, lane);
            // (a row is nine 1 KiB loads: all of them issued before dot_lane's own chain starts, one memory round trip per
            // row — with the loads inside the chain, as dot_lane has them, a row is nine round trips and the stage up to three times
            // slower: profiles/diverse_search_bench.txt)
            for (int c = wave; c < np; c += 4) {
                if (L.taken[c]) continue;                               // (wave-uniform)
                const f32x4* dr = reinterpret_cast<const f32x4*>(p.index_f32 + (size_t)L.id[c] * dim);
                f32x4 dv[MERGE_MAXV];
#pragma unroll
                for (int i = 0; i < MERGE_MAXV; ++i) {
                    const int cc = lane + i * 64;
                    dv[i] = (cc < nv) ? dr[cc] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
                float a = 0.f;
#pragma unroll
                for (int i = 0; i < MERGE_MAXV; ++i) {
                    const int cc = lane + i * 64;
                    if (cc < nv) a = dot_chunk(pv[i], dv[i], a);        // the chain of dot_lane(picked row, row)
                }
                a = wave_sum(a);
                if (lane == 0) L.m[c] = fmaxf(L.m[c], a);
            }
            __syncthreads();
            // ---- argmax of v over the unselected members, the lower position among equal v
            uint64_t best = 0;
            for (int c = tid; c < np; c += 256) {
                if (L.taken[c]) continue;
                const float v = __builtin_fmaf(lam, L.r[c], -(oml * L.m[c]));
                const uint64_t key = ((uint64_t)f32_orderable(v) << 32) | (uint32_t)(~(uint32_t)c);
                best = key > best ? key : best;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const uint64_t x = shfl_xor_u64(best, o); best = x > best ? x : best; }
            if (lane == 0) L.red[wave] = best;
            __syncthreads();
            best = L.red[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) best = L.red[w] > best ? L.red[w] : best;
            b = (int)min(~(uint32_t)best, (uint32_t)(np - 1));                  // (t < n_pick <= np: an unselected member exists, best != 0)
            if (tid == 0) { L.taken[b] = 1; os[t] = L.r[b]; oi[t] = L.id[b]; }
            __syncthreads();
        }
    }
}

bool mmr_dim_ok(int dim) { return dim > 0 && dim % 4 == 0 && dim <= 64 * 4 * MERGE_MAXV; }

hipError_t launch_mmr_select(const MmrArgs& p, hipStream_t s) {
    if (p.nq <= 0) return hipSuccess;
    if (!p.index_f32 || !p.pool_scores || !p.pool_ids || !p.out_scores || !p.out_ids || !mmr_dim_ok(p.dim) || p.n_docs < 0 ||
        p.k < 1 || p.k > p.pool || p.pool > MMR_POOL || !(p.lambda >= 0.f && p.lambda <= 1.f))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mmr_select_kernel, dim3(p.nq < 4096 ? p.nq : 4096), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace vr
