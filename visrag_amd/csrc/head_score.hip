// Fused LM head for teacher-forced scoring (vr_chat_score, vr_op_head_score): per row m of A
//     x[m][v] = A[m, :K] . W[v, :K]       (bf16 x bf16 products, fp32 accumulation)
// reduced on the fly to  x_t[m] = x[m][target[m]],  lse[m] = log sum_{v < V} exp(x[m][v]),  top_x[m] = max_v x[m][v] and
// top_id[m] = its token (lowest id among exact ties) — the M x V logits are never written (2 048 rows x 122 753 columns
// would be a 1 GB write and re-read).  The precedent is the search sweep (search256.hip): a bf16 MFMA GEMM whose scores
// are consumed in registers.
//
//   head_score_kernel          one workgroup per (256-column vocab tile, 256-row tile) on the 256 x 256 x 64 main loop of
//                              gemm256_bf16_kernel (gemm_core_il.h).  Epilogue: a lane holds 4 x 4 columns of each of its 8
//                              rows (acc[i][j][r]: row wm*128 + i*16 + fr, column wn*64 + j*16 + fq*4 + r); it reduces them to
//                              (max, sum exp(x - max), argmax), merges with the three other lanes of the row (shuffles), the
//                              four column slabs of the waves meet in LDS (the stages are free after the K-loop), and the
//                              tile's partial goes to part[...][vocab tile][M].  The lane that holds column target[m] writes x_t[m].
//   head_score_combine_kernel  one wave per row merges the row's <= 480 partials by the usual (max, sum) rescale.
//
// A column counts iff its INDEX is < V: the padded weight rows are zero and would contribute logit 0.  Rows >= M are computed
// (A is readable up to the next multiple of 256 rows) and never written.  No workgroup waits for another, no atomics; every
// merge runs in a fixed order, so two runs agree bit for bit.  Sums are hierarchical: 16 terms per lane, 4 lanes, 4 waves,
// then ceil(tiles / 64) partials per lane and a 64-lane tree.
#include <climits>

#include "gemm_core.h"
#include "gemm_core_il.h"
#include "kernels.h"

namespace vr {

struct HeadScoreArgs {
    const void* A; int lda;
    const void* W; int ldw;
    int M, V, K;
    const int* target;
    float* pmax; float* psum; int* parg;      // [vocab tiles][M] each
    float* x_t;
};

// (m, s, a) <- merge with (om, os, oa): s is the sum of exp(x - m) over the columns seen, a the lowest column that holds m.
// A side that has seen no column is (-inf, 0, INT_MAX); commutative bit for bit (fp32 addition and max are).
__device__ __forceinline__ void hs_merge(float& m, float& s, int& a, float om, float os, int oa) {
    const float nm = fmaxf(m, om);
    const float ea = m == nm ? 1.f : __expf(m - nm), eb = om == nm ? 1.f : __expf(om - nm);
    s = s * ea + os * eb;
    a = (om > m || (om == m && oa < a)) ? oa : a;
    m = nm;
}

__global__ __launch_bounds__(512, 2) void head_score_kernel(HeadScoreArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tiles_m = (p.M + G256_BM - 1) / G256_BM, tiles_v = (p.V + G256_BN - 1) / G256_BN;
    // row tiles fastest: the row tiles of one vocab tile run side by side on one XCD, so a weight tile leaves HBM once
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_v);
    const int vt = t / tiles_m, mt = t - vt * tiles_m;
    const int m0 = mt * G256_BM, n0 = vt * G256_BN;

    gemm256_acc_t acc;
    gemm256_zero(acc);
    gemm256_mainloop_il(acc, (const bf16_t*)p.A, p.lda, (const bf16_t*)p.W, p.ldw, m0, n0, p.K, smem);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 2, wn = wave & 3, fr = lane & 15, fq = lane >> 4;
    float* l_max = reinterpret_cast<float*>(smem);           // [4 slabs][256 rows]
    float* l_sum = l_max + 4 * G256_BM;
    int* l_arg = reinterpret_cast<int*>(l_sum + 4 * G256_BM);
    const int cbase = n0 + wn * 64 + fq * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row_l = wm * 128 + i * 16 + fr, row = m0 + row_l;
        const int tgt = row < p.M ? p.target[row] : -1;
        float mx = -INFINITY, xt = 0.f;
        int am = INT_MAX;
        bool hit = false;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {                     // ascending columns: the first of equal maxima stays
                const int col = cbase + j * 16 + r;
                const float x = acc[i][j][r];
                if (col < p.V && x > mx) { mx = x; am = col; }
                if (col == tgt) { xt = x; hit = true; }
            }
        float sm = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (cbase + j * 16 + r < p.V) sm += __expf(acc[i][j][r] - mx);
        if (hit) p.x_t[row] = xt;                             // (tgt >= 0 only for rows < M; one lane of the grid holds the column)
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sm, o, 64);
            const int oa = __shfl_xor(am, o, 64);
            hs_merge(mx, sm, am, om, os, oa);
        }
        if (fq == 0) { l_max[wn * G256_BM + row_l] = mx; l_sum[wn * G256_BM + row_l] = sm; l_arg[wn * G256_BM + row_l] = am; }
    }
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < G256_BM && m0 + tid < p.M) {
        float mx = l_max[tid], sm = l_sum[tid];
        int am = l_arg[tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) hs_merge(mx, sm, am, l_max[w * G256_BM + tid], l_sum[w * G256_BM + tid], l_arg[w * G256_BM + tid]);
        const size_t o = (size_t)vt * p.M + m0 + tid;
        p.pmax[o] = mx; p.psum[o] = sm; p.parg[o] = am;
    }
}

__global__ __launch_bounds__(256) void head_score_combine_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                                 const int* __restrict__ parg, int tiles_v, int M,
                                                                 float* __restrict__ lse, float* __restrict__ top_x,
                                                                 int* __restrict__ top_id) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float mx = -INFINITY, sm = 0.f;
    int am = INT_MAX;
    for (int vt = lane; vt < tiles_v; vt += 64) {
        const size_t o = (size_t)vt * M + row;
        hs_merge(mx, sm, am, pmax[o], psum[o], parg[o]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sm, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        hs_merge(mx, sm, am, om, os, oa);
    }
    if (lane == 0) { lse[row] = mx + logf(sm); top_x[row] = mx; top_id[row] = am; }
}

size_t head_score_part_words(int M, int V) { return (size_t)3 * ((V + G256_BN - 1) / G256_BN) * (size_t)M; }

hipError_t launch_head_score(const void* A, int lda, const void* W, int ldw, int M, int V, int K, const int* target, void* part,
                             float* x_t, float* lse, float* top_x, int* top_id, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (!A || !W || !target || !part || !x_t || !lse || !top_x || !top_id) return hipErrorInvalidValue;
    if (V < 1 || K < GEMM_BK || K % GEMM_BK || lda < K || ldw < K || lda % 8 || ldw % 8) return hipErrorInvalidValue;
    if ((((uintptr_t)A | (uintptr_t)W) & 15) || ((uintptr_t)part & 3)) return hipErrorInvalidValue;
    const int tiles_m = (M + G256_BM - 1) / G256_BM, tiles_v = (V + G256_BN - 1) / G256_BN;
    if ((long)tiles_m * tiles_v > INT_MAX) return hipErrorInvalidValue;
    const size_t plane = (size_t)tiles_v * M;
    HeadScoreArgs p{A, lda, W, ldw, M, V, K, target, (float*)part, (float*)part + plane, (int*)part + 2 * plane, x_t};
    auto k = head_score_kernel;
    static unsigned long long attr = 0;     // bit d: set on device d
    set_max_dynamic_lds((const void*)k, G256_SMEM_BYTES, attr);
    hipLaunchKernelGGL(k, dim3(tiles_m * tiles_v), dim3(512), G256_SMEM_BYTES, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head_score_combine_kernel, dim3((M + 3) / 4), dim3(256), 0, s, p.pmax, p.psum, p.parg, tiles_v, M, lse, top_x,
                       top_id);
    return hipGetLastError();
}

}  // namespace vr
