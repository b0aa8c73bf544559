// What the two samplers of the answer generation (chat_kernels.hip: top-k by repeated max; chat_sample.hip: nucleus / any top-k
// by radix select) must compute with the same bits: the penalised score, the order-preserving key, the tempered value and the
// value the Gumbel noise is added to.
#pragma once
#include "common.h"
#include "kernels.h"

namespace vr {

// order-preserving map of a float to 32 bits, and back
__device__ __forceinline__ unsigned f2ord(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

// Candidate score of token `tok` of selected row r (HF order: log_softmax first for beams, then the repetition penalty on the
// row's generated ids, then the running beam score)
__device__ __forceinline__ float chat_score(int mode, float x, bool seen, float pen, float lse, float bs) {
    if (mode == CHAT_SEL_BEAM) x = x - lse;
    if (seen) x = x < 0.f ? x * pen : x / pen;
    if (mode == CHAT_SEL_BEAM) x = x + bs;
    return x;
}

// z = s / temperature as the samplers order and weigh it: the rounded fp32 product
__device__ __forceinline__ float chat_tempered(float s, float inv_t) {
#pragma clang fp contract(off)
    return s * inv_t;
}

// The value a sampler takes the argmax of: s * inv_t + noise in ONE rounding.  hipcc contracts that expression into an fma in
// chat_topk_final_kernel; spelled as the fma here, so that every sampler draws with those bits whatever surrounds the call.
__device__ __forceinline__ float chat_noisy(float s, float inv_t, float noise) { return __builtin_fmaf(s, inv_t, noise); }

}  // namespace vr
