// Editing the index in place (vr_index_remove / vr_index_update / vr_index_get_rows, index_rows.hip): whole rows moved by whole waves,
// 16 bytes per lane and access.  A row of the fp32 store is dim * 4 bytes (a multiple of 256), a row of the bf16 store dim * 2
// (a multiple of 128): both are counted here in 16-byte units, and one kernel serves both stores.
//
// Removal closes the store up in row order: with rem[0..nr) the removed rows, sorted and distinct, new row j is old row
//   src(j) = j + #{i : rem[i] - i <= j}          (rem[i] - i = the NEW position the first survivor behind rem[i] takes)
// — monotone, src(j) >= j, found by a binary search over nr ints.  In place this is a hazard: new row j is also the source of
// some earlier new row (remove row 0 alone: src(j) = j + 1 everywhere), and the workgroups of one launch run in no order.  No
// kernel here looks at another workgroup: every LAUNCH reads a set of rows and writes a set of rows that are disjoint by
// construction, and stream order between launches is the only ordering (index_rows.hip: compact_store picks the launches).
#include "common.h"
#include "kernels.h"

namespace vr {

constexpr int EDIT_MAX_BLOCKS = 8192;       // grid-stride beyond: 4 rows (waves) per workgroup

__device__ __forceinline__ int compact_src(const int* __restrict__ rem, int nr, int j) {
    int lo = 0, hi = nr;                    // -> the first i with rem[i] - i > j
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rem[mid] - mid <= j) lo = mid + 1;
        else hi = mid;
    }
    return j + lo;
}

// one row of `units` 16-byte words by one wave: up to four loads in flight per lane, then their stores
__device__ __forceinline__ void copy_row(const u32x4* s, u32x4* d, int units, int lane) {
    for (int c = lane; c < units; c += 256) {
        u32x4 v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e * 64 < units) v[e] = s[c + e * 64];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e * 64 < units) d[c + e * 64] = v[e];
    }
}

// out row i = store row (COMPACT ? src(j0 + i) : list[i]) for i < n_rows.  `out` may lie inside `store` (the wide windows of a
// removal): the launcher's caller keeps the rows read and the rows written apart, so neither pointer is __restrict__.
template <bool COMPACT>
__global__ __launch_bounds__(256) void rows_gather_kernel(const u32x4* store, int units, const int* __restrict__ list, int nlist,
                                                          int j0, int64_t n_rows, u32x4* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_rows; i += (int64_t)gridDim.x * 4) {
        const int r = COMPACT ? compact_src(list, nlist, j0 + (int)i) : list[i];
        copy_row(store + (size_t)r * units, out + (size_t)i * units, units, lane);
    }
}

static unsigned edit_blocks(int64_t n_rows) {
    const int64_t b = (n_rows + 3) / 4;
    return (unsigned)(b < EDIT_MAX_BLOCKS ? b : EDIT_MAX_BLOCKS);
}

hipError_t launch_rows_compact(const void* store, size_t row_bytes, const int* rem, int nr, int64_t j0, int64_t n_rows, void* out,
                               hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    if (!store || !rem || !out || nr < 1 || j0 < 0 || row_bytes == 0 || row_bytes % 16 || row_bytes / 16 > 0x7fffffff ||
        j0 + n_rows + nr > 0x7fffffff)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rows_gather_kernel<true>, dim3(edit_blocks(n_rows)), dim3(256), 0, s, (const u32x4*)store,
                       (int)(row_bytes / 16), rem, nr, (int)j0, n_rows, (u32x4*)out);
    return hipGetLastError();
}

hipError_t launch_rows_gather(const void* store, size_t row_bytes, const int* ids, int64_t n_rows, void* out, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    if (!store || !ids || !out || row_bytes == 0 || row_bytes % 16 || row_bytes / 16 > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rows_gather_kernel<false>, dim3(edit_blocks(n_rows)), dim3(256), 0, s, (const u32x4*)store,
                       (int)(row_bytes / 16), ids, 0, 0, n_rows, (u32x4*)out);
    return hipGetLastError();
}

// fp32 row ids[i] = reps row i, and its bf16 row with it (the conversion of launch_f32_to_bf16): a lane takes 8 floats — 32 bytes
// in, 32 bytes to the fp32 store, 16 bytes to the bf16 store.  ids are distinct: no two waves write one row.
__global__ __launch_bounds__(256) void rows_update_kernel(const float* __restrict__ reps, const int* __restrict__ ids, int64_t n,
                                                          int dim, float* __restrict__ f32, bf16_t* __restrict__ bf16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n; i += (int64_t)gridDim.x * 4) {
        const size_t r = (size_t)ids[i];
        const float* x = reps + (size_t)i * dim;
        for (int c = lane * 8; c < dim; c += 64 * 8) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(x + c), b = *reinterpret_cast<const f32x4*>(x + c + 4);
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) { o[e] = f2bf(a[e]); o[4 + e] = f2bf(b[e]); }
            *reinterpret_cast<f32x4*>(f32 + r * dim + c) = a;
            *reinterpret_cast<f32x4*>(f32 + r * dim + c + 4) = b;
            *reinterpret_cast<bf16x8*>(bf16 + r * dim + c) = o;
        }
    }
}

hipError_t launch_rows_update(const float* reps, const int* ids, int64_t n, int dim, float* f32, void* bf16, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!reps || !ids || !f32 || !bf16 || dim < 8 || dim % 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rows_update_kernel, dim3(edit_blocks(n)), dim3(256), 0, s, reps, ids, n, dim, f32, (bf16_t*)bf16);
    return hipGetLastError();
}

// New word w (thread) of every filter: bit b = the old bit of row src(32 w + b), clear at or beyond new_n.  The 32 sources are found
// once — a binary search for the first, a walk along rem for the rest — and serve all filters.  Out of place: `out` is another buffer.
__global__ __launch_bounds__(256) void filter_compact_kernel(const uint32_t* __restrict__ bits, size_t words, uint32_t* __restrict__ out,
                                                             size_t new_words, int n_filters, const int* __restrict__ rem, int nr,
                                                             int64_t new_n) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= new_words) return;
    const int j = (int)(w * 32);
    int p = compact_src(rem, nr, j) - j;    // removed rows in front of src(j)
    int src[32];
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        while (p < nr && rem[p] - p <= j + b) ++p;
        src[b] = j + b < new_n ? j + b + p : -1;
    }
    for (int f = 0; f < n_filters; ++f) {
        const uint32_t* old = bits + (size_t)f * words;
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 32; ++b)
            if (src[b] >= 0) v |= ((old[src[b] >> 5] >> (src[b] & 31)) & 1u) << b;
        out[(size_t)f * new_words + w] = v;
    }
}

hipError_t launch_filter_compact(const uint32_t* bits, size_t words, int n_filters, const int* rem, int nr, int64_t new_n,
                                 uint32_t* out, hipStream_t s) {
    if (!bits || !out || !rem || bits == out || n_filters < 1 || nr < 1 || new_n < 1 || new_n + nr > 0x7fffffff - 32 ||
        words != (size_t)((new_n + nr + 31) / 32))
        return hipErrorInvalidValue;
    const size_t new_words = (size_t)((new_n + 31) / 32);
    hipLaunchKernelGGL(filter_compact_kernel, dim3((unsigned)((new_words + 255) / 256)), dim3(256), 0, s, bits, words, out, new_words,
                       n_filters, rem, nr, new_n);
    return hipGetLastError();
}

}  // namespace vr
