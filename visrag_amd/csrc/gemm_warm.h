// GemmArgs::warm — the share arithmetic: which lines (128 bytes) of the region a workgroup, a wave and a wave-instruction request.
// Host and device use the same function; gemm256w.hip pins it with static_asserts.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace vr {

#ifndef VR_WARM_LINE                                    // (tagged builds of tools/warm_probe.py only: one request per 64 bytes)
#define VR_WARM_LINE 128
#endif
constexpr unsigned WARM_LINE = VR_WARM_LINE;            // bytes one request is meant to bring into the memory-side cache
constexpr unsigned WARM_WAVES = 4;                      // waves of the carrying workgroup
constexpr size_t WARM_MAX_BYTES = (size_t)1 << 31;      // a buffer descriptor's num_records and 32-bit lane offsets cover the region

struct WarmShare { unsigned first, end; };              // lines [first, end) of the region

// lines are counted from the region's first byte: line i = bytes [WARM_LINE i, WARM_LINE (i + 1)) of it
__host__ __device__ constexpr unsigned warm_lines(size_t bytes) { return (unsigned)((bytes + WARM_LINE - 1) / WARM_LINE); }

// part `w` of `total` of the lines [lo, hi): contiguous, ordered by w, disjoint, and together every line exactly once
__host__ __device__ constexpr unsigned warm_cut(unsigned n, unsigned w, unsigned total) {     // floor(n w / total), w <= total
    // n w / total = (n / total) w + (n % total) w / total exactly; the second product stays in 32 bits for every grid below 2^16
    // workgroups (a 64-bit division by a run-time divisor is a loop on the GPU)
    if (total < 65536u) return n / total * w + n % total * w / total;
    return (unsigned)((unsigned long long)n * w / total);
}
__host__ __device__ constexpr WarmShare warm_part(unsigned lo, unsigned hi, unsigned w, unsigned total) {
    return WarmShare{lo + warm_cut(hi - lo, w, total), lo + warm_cut(hi - lo, w + 1, total)};
}
// workgroup w of `total`, then wave `wave` of WARM_WAVES inside it
__host__ __device__ constexpr WarmShare warm_share(size_t bytes, unsigned w, unsigned total, unsigned wave) {
    const WarmShare g = warm_part(0, warm_lines(bytes), w, total);
    return warm_part(g.first, g.end, wave, WARM_WAVES);
}
// wave-instructions a wave issues for its share: instruction i, lane l requests line first + 64 i + l (if below end)
__host__ __device__ constexpr unsigned warm_instructions(WarmShare s) { return (s.end - s.first + 63) / 64; }

}  // namespace vr
