// Small arithmetic of the decode steps that more than one kernel performs and that must give the same bits wherever it runs
// (the range merge: fused into gemm_skinny.hip's o projection and on its own in attn_combine_kernel): spelled out operation by operation, because left to
// -ffp-contract=fast hipcc fuses `a * b + c * d` one way in one kernel and the other way in the next (seen: a rotated q / k
// element one ulp apart, a bf16 rounding flipped, logits 2e-3 of their scale apart at one decode step in a few hundred).
#pragma once
#include "common.h"

namespace vr {

// rotate-half pair (x1, x2) by the angle whose cosine / sine are cs / sn: x * cos + rotate_half(x) * sin
__device__ __forceinline__ void rope_rotate(float& x1, float& x2, float cs, float sn) {
#pragma clang fp contract(off)
    const float a = x2 * sn, b = x1 * sn;
    const float r1 = __builtin_fmaf(x1, cs, -a), r2 = __builtin_fmaf(x2, cs, b);
    x1 = r1; x2 = r2;
}

// sum of the squares of a float4 (one lane's share of a row's sum of squares)
__device__ __forceinline__ float sumsq4(f32x4 v) {
#pragma clang fp contract(off)
    return __builtin_fmaf(v[3], v[3], __builtin_fmaf(v[2], v[2], __builtin_fmaf(v[1], v[1], v[0] * v[0])));
}

// The samplers' noise (gen_kernels.hip, chat_kernels.hip): 64-bit counter hash of (seed, step, token id) -> a 24-bit draw ->
// u = (draw + 0.5) 2^-24 -> standard Gumbel noise -log(-log(u)).  draw + 0.5 is rounded to float32 (from 2^23 on it is a tie, to
// even), and for the draw 0xFFFFFF that rounding gives 2^24, i.e. u = 1 and infinite noise — the token was then drawn whatever
// its logit, once in 2^24 (token, step) pairs.  That one draw is held at the largest float below 1; every other draw keeps its bits.
__device__ __forceinline__ float gumbel_noise(unsigned long long seed, unsigned step, unsigned idx) {
    unsigned long long x = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)step << 32 | idx);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    const float u = fminf(((float)(x >> 40) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
    return -__logf(-__logf(u));
}

// one KV range's contribution to the merge of partial attention rows: weight e = 2^(lse - max)
__device__ __forceinline__ void merge_range(float& num, float& den, float e, float pv) {
#pragma clang fp contract(off)
    num = __builtin_fmaf(e, pv, num);
    den = den + e;
}

}  // namespace vr
