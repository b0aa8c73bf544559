// vr_rrf_fuse / vr_index_search_rrf: reciprocal-rank fusion (RRF) of the lists of a group's sub-queries.  Group g has lists
// L_0 .. L_{m-1} of `depth` slots each; slot r of list j holds an id in [0, 2^31 - 2], anything else is an empty slot.  For id i
//     F(i) = fp32( sum over the entries (j, r) with L_j[r] == i, in ascending (j, r), of  (double)w_j / ((double)c + (double)(r + 1)) )
// — an fp64 sum that starts at 0.0, every term ONE division (no reciprocal, nothing to contract), rounded to fp32 once —
// and hits(i) = the number of such entries.  The result of the group is the k ids of largest make_key(F, id): F descending in the
// ranking's own order of floats, then lower id first; slots past the distinct ids hold (-inf, -1, 0).  Scores depend on
// positions only, so the result is a function of the lists: a numpy statement of the above reproduces it bit for bit.
//
// rrf_fuse_kernel, one workgroup of 256 threads per group, the whole definition in this one kernel:
//   1. every non-empty entry becomes one 64-bit word in dynamic LDS: id + 1 in the high word (31 bits, 0 = empty, bit 31 clear),
//      ~(j << 16 | r) in the low word; the array is padded with zeros to the next power of two of m * depth;
//   2. block_bitonic_desc: equal ids are adjacent, a segment's entries stand in ASCENDING (j, r), the empty words at the end;
//   3. the head of a segment (the entry whose predecessor has another id) walks it in that order, sums in fp64, and replaces
//      its own low word by the bits of F and sets bit 31 of its own high word.  The words are accessed as 32-bit halves: a
//      head writes its own two halves only, a walker reads the high halves of later entries under a mask that ignores bit
//      31 and the low halves of its own segment's entries, which nobody writes — no barrier is needed inside the step;
//   4. every slot, reading itself alone, becomes make_key(F, id) (heads) or KEY_NONE; block_bitonic_desc again; k slots are
//      emitted;
//   5. hits of the winners are recounted from the group's lists, a wave per winner (k * m * depth compares against lists
//      that are cache-resident: cheaper than carrying a count through the second sort, whose keys have no room for it).
// No workgroup waits for another; the launch is the only ordering.  LDS: 8 bytes per entry of the padded array, at most
// RRF_MAX_ENTRIES * 8 = 128 KiB, plus two counters.  Reads of the lists stay inside [lims[g] * depth, lims[g + 1] * depth);
// a group whose padded size exceeds the LDS the launch reserved (never, from this file's launcher) emits tails.
#include "kernels.h"
#include "search_common.h"

namespace vr {

constexpr int RRF_MAX_ENTRIES = 16384;      // m * depth of one group: 128 KiB of words
constexpr int64_t RRF_ID_MAX = ((int64_t)1 << 31) - 2;

int rrf_max_entries() { return RRF_MAX_ENTRIES; }

__global__ __launch_bounds__(256) void rrf_fuse_kernel(RrfArgs p, int lds_words) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int cnt[2];                                              // non-empty entries, distinct ids
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem_raw);
    typedef uint32_t __attribute__((may_alias)) half_t;                 // (the same bytes as `keys`)
    half_t* half = reinterpret_cast<half_t*>(smem_raw);                 // word e: low half at 2e, high half at 2e + 1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x, depth = p.depth, k = p.k;
    const int l0 = p.lims[g], m = p.lims[g + 1] - l0;
    const int n_ent = m * depth;
    int n_sort = 64;
    while (n_sort < n_ent) n_sort <<= 1;
    float* os = p.out_scores + (size_t)g * k;
    int64_t* oi = p.out_ids + (size_t)g * k;
    int* oh = p.out_hits + (size_t)g * k;
    if (m <= 0 || n_sort > lds_words) {                                 // (workgroup-uniform)
        for (int c = tid; c < k; c += 256) { os[c] = -INFINITY; oi[c] = -1; oh[c] = 0; }
        return;
    }
    if (tid < 2) cnt[tid] = 0;
    const int64_t* L = p.ids + (size_t)l0 * depth;
    // ---- 1. the entries
    int filled = 0;
    for (int e = tid; e < n_sort; e += 256) {
        uint64_t w = 0;
        if (e < n_ent) {
            const int64_t id = L[e];
            if (id >= 0 && id <= RRF_ID_MAX) {
                const int j = e / depth, r = e - j * depth;
                w = ((uint64_t)(uint32_t)(id + 1) << 32) | (uint32_t)(~(((uint32_t)j << 16) | (uint32_t)r));
                ++filled;
            }
        }
        keys[e] = w;
    }
    __syncthreads();
    // ---- 2. equal ids adjacent, ascending (j, r) inside a segment
    block_bitonic_desc(keys, n_sort, tid, 256);
    // ---- 3. segment heads sum their segment
    const double c64 = (double)p.c;
    int heads = 0;
    for (int e = tid; e < n_sort; e += 256) {
        const uint32_t hi = half[2 * e + 1];                           // (its own high half: not yet flagged)
        if (hi == 0u) continue;
        if (e > 0 && (half[2 * e - 1] & 0x7FFFFFFFu) == hi) continue;
        double acc = 0.0;
        int q = e;
        do {
            const uint32_t x = ~half[2 * q];
            const int j = (int)(x >> 16), r = (int)(x & 0xFFFFu);
            const float wj = p.weights ? p.weights[l0 + j] : 1.0f;
            acc += (double)wj / (c64 + (double)(r + 1));
            ++q;
        } while (q < n_sort && (half[2 * q + 1] & 0x7FFFFFFFu) == hi);
        half[2 * e] = __float_as_uint((float)acc);
        half[2 * e + 1] = hi | 0x80000000u;
        ++heads;
    }
    __syncthreads();
    // ---- 4. ranking keys, every slot from itself alone
    for (int e = tid; e < n_sort; e += 256) {
        const uint32_t hi = half[2 * e + 1], lo = half[2 * e];
        const uint64_t key = (hi & 0x80000000u) ? make_key(__uint_as_float(lo), (hi & 0x7FFFFFFFu) - 1u) : KEY_NONE;
        half[2 * e] = (uint32_t)key;
        half[2 * e + 1] = (uint32_t)(key >> 32);
    }
    __syncthreads();
    block_bitonic_desc(keys, n_sort, tid, 256);
    for (int c = tid; c < k; c += 256) {
        const uint64_t key = c < n_sort ? keys[c] : KEY_NONE;
        const bool ok = key != KEY_NONE;
        os[c] = ok ? key_score(key) : -INFINITY;
        oi[c] = ok ? (int64_t)(~(uint32_t)key) : (int64_t)-1;
        if (!ok) oh[c] = 0;
    }
    // ---- 5. hits of the winners, a wave per winner
    const int kz = min(k, n_sort);
    for (int c = wave; c < kz; c += 4) {
        const uint64_t key = keys[c];
        if (key == KEY_NONE) break;                                     // (wave-uniform; sorted: nothing behind it either)
        const int64_t id = (int64_t)(~(uint32_t)key);
        int h = 0;
        for (int e = lane; e - lane < n_ent; e += 64) h += __popcll(__ballot(e < n_ent && L[e] == id));
        if (lane == 0) oh[c] = h;
    }
    if (p.stats) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { filled += __shfl_xor(filled, o, 64); heads += __shfl_xor(heads, o, 64); }
        if (lane == 0) { atomicAdd(&cnt[0], filled); atomicAdd(&cnt[1], heads); }
        __syncthreads();
        if (tid == 0) {
            atomicAdd(&p.stats[0], 1ull);
            atomicAdd(&p.stats[1], (unsigned long long)cnt[0]);
            atomicAdd(&p.stats[2], (unsigned long long)cnt[1]);
        }
    }
}

hipError_t launch_rrf_fuse(const RrfArgs& p, int n_groups, int max_entries, hipStream_t s) {
    if (n_groups <= 0) return hipSuccess;
    if (!p.ids || !p.lims || !p.out_scores || !p.out_ids || !p.out_hits || p.depth < 1 || p.depth > 65535 || p.k < 1 ||
        max_entries < 1 || max_entries > RRF_MAX_ENTRIES || !(p.c >= 0.f))
        return hipErrorInvalidValue;
    int n_sort = 64;                                                    // the padded size of the largest group
    while (n_sort < max_entries) n_sort <<= 1;
    static unsigned long long attr = 0;     // bit d: set on device d
    set_max_dynamic_lds((const void*)rrf_fuse_kernel, RRF_MAX_ENTRIES * 8, attr);
    hipLaunchKernelGGL(rrf_fuse_kernel, dim3((unsigned)n_groups), dim3(256), (size_t)n_sort * 8, s, p, n_sort);
    return hipGetLastError();
}

}  // namespace vr
