// Split-precision decoder pieces for TOKEN-ONLY batches (text queries, text passages).
//
// north_star's parity bar is "cosine scores within 1e-3" of the reference's fp32 CPU path.  A page
// pools 68+ tokens and averages the bf16 rounding of the MFMA operands away (max score error 3.9e-4
// on the config-1 fixture); a ~20-token query does not (9.7e-4: no margin).  Queries are ~0.1 % of
// the path's work, so their decoder pass runs at fp32-class precision instead:
//   * every GEMM operand is split into hi + lo bf16 parts (x = hi + lo to ~16 mantissa bits) and the
//     product is accumulated from A_hi W_hi + A_lo W_hi + A_hi W_lo on the SAME MFMA kernels
//     (encode.hip issues them as an EPI_F32 launch followed by in-place EPI_RESID launches);
//   * everything between the GEMMs stays fp32: the kernels below (RMSNorm -> split, RoPE, causal
//     attention, SwiGLU -> split, embedding gather from a hi + lo table).
// Reference arithmetic: modeling_minicpm.py:119-136 (RMSNorm), :259-290 (rotary), :816-910 (SDPA,
// causal), :293-335 (MLP), modeling_minicpmv.py:139-141 (embed * scale_emb).
// Roofline: none of these is on the throughput path (weights are streamed for a few hundred rows:
// HBM-bound by the weight reads of the GEMMs around them).
#include "common.h"
#include "kernels.h"

namespace vr {

constexpr int HP_MAXV = 10;      // float4 per lane: rows up to 2560 columns (the encoder's hidden size limit)

__device__ __forceinline__ void split_store4(const f32x4 y, bf16_t* hi, bf16_t* lo) {
    bf16x4 h, l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        h[r] = f2bf(y[r]);
        l[r] = f2bf(y[r] - bf2f(h[r]));
    }
    *reinterpret_cast<bf16x4*>(hi) = h;
    *reinterpret_cast<bf16x4*>(lo) = l;
}

// y = x * rsqrt(mean(x^2) + eps) * w, written as hi + lo bf16 rows (one wave per row)
__global__ __launch_bounds__(256) void rmsnorm_split_kernel(const float* __restrict__ x, int rows, int dim,
                                                            const float* __restrict__ w, float eps,
                                                            bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nv = dim >> 2;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * dim);
    f32x4 v[HP_MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < HP_MAXV; ++i) {
        const int c = lane + i * 64;
        v[i] = (c < nv) ? xr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        s += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    }
    s = wave_sum(s);
    const float rstd = rsqrtf(s / dim + eps);
#pragma unroll
    for (int i = 0; i < HP_MAXV; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            const f32x4 y = v[i] * rstd * reinterpret_cast<const f32x4*>(w)[c];
            split_store4(y, hi + (size_t)row * dim + c * 4, lo + (size_t)row * dim + c * 4);
        }
    }
}

hipError_t launch_rmsnorm_split(const float* x, int rows, int dim, const float* w, float eps, void* hi, void* lo, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (dim % 4 || dim > 64 * 4 * HP_MAXV) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rmsnorm_split_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, dim, w, eps, (bf16_t*)hi, (bf16_t*)lo);
    return hipGetLastError();
}

// rotate the q and k heads (head_dim 64, pairs (c, c + 32)) of fp32 qkv rows in place; table = [pos][32 cos | 32 sin]
__global__ __launch_bounds__(256) void rope_f32_kernel(float* __restrict__ qkv, int T, int ld, int rope_cols,
                                                       const int* __restrict__ pos, const float* __restrict__ table) {
    const int t = blockIdx.x;
    const float* tab = table + (size_t)pos[t] * 64;
    float* row = qkv + (size_t)t * ld;
    for (int i = threadIdx.x; i < rope_cols / 2; i += 256) {
        const int head = i >> 5, c = i & 31;
        float* p = row + head * 64 + c;
        const float x1 = p[0], x2 = p[32], cs = tab[c], sn = tab[32 + c];
        p[0] = x1 * cs - x2 * sn;
        p[32] = x2 * cs + x1 * sn;
    }
}

hipError_t launch_rope_f32(float* qkv, int T, int ld, int rope_cols, const int* pos, const float* table, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    if (rope_cols % 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rope_f32_kernel, dim3(T), dim3(256), 0, s, qkv, T, ld, rope_cols, pos, table);
    return hipGetLastError();
}

// Causal attention in fp32, head_dim 64, packed ragged sequences: one wave per (token, head).
// Scores: lane = key (64 keys per round), each lane dots its key row with the query row; online softmax over the
// rounds; PV: lane = output column, p_j broadcast from lane j.  q/k/v at columns [0,E) / [E,2E) / [2E,3E) of `qkv`.
__global__ __launch_bounds__(256) void attn_f32_kernel(const float* __restrict__ qkv, int ld, int E,
                                                       const int* __restrict__ seq_of, const int* __restrict__ seq_offsets,
                                                       int T, int heads, float scale, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= T * heads) return;
    const int t = w / heads, h = w % heads;
    const int t0 = seq_offsets[seq_of[t]];
    const int n_keys = t - t0 + 1;                         // causal: keys t0 .. t
    const float* qrow = qkv + (size_t)t * ld + h * 64;
    f32x4 q[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) q[i] = reinterpret_cast<const f32x4*>(qrow)[i];
    float m = -INFINITY, l = 0.f, acc = 0.f;               // running max, denominator, output column `lane`
    for (int j0 = 0; j0 < n_keys; j0 += 64) {
        const int j = j0 + lane;
        float sc = -INFINITY;
        if (j < n_keys) {
            const f32x4* kr = reinterpret_cast<const f32x4*>(qkv + (size_t)(t0 + j) * ld + E + h * 64);
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const f32x4 kv = kr[i];
                a += q[i][0] * kv[0] + q[i][1] * kv[1] + q[i][2] * kv[2] + q[i][3] * kv[3];
            }
            sc = a * scale;
        }
        const float mn = fmaxf(m, wave_max(sc));
        const float p = (j < n_keys) ? expf(sc - mn) : 0.f;
        const float corr = expf(m - mn);                   // (m = -inf on the first round: 0)
        l = l * corr + wave_sum(p);
        acc *= corr;
        const int nj = min(64, n_keys - j0);
        const float* vbase = qkv + (size_t)(t0 + j0) * ld + 2 * E + h * 64 + lane;
        for (int jj = 0; jj < nj; ++jj) acc += __shfl(p, jj, 64) * vbase[(size_t)jj * ld];
        m = mn;
    }
    out[(size_t)t * E + h * 64 + lane] = acc / l;
}

hipError_t launch_attn_f32(const float* qkv, int ld, int E, const int* seq_of, const int* seq_offsets, int T, int heads,
                           float scale, float* out, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    if (E != heads * 64) return hipErrorInvalidValue;
    const long waves = (long)T * heads;
    hipLaunchKernelGGL(attn_f32_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, qkv, ld, E, seq_of, seq_offsets, T,
                       heads, scale, out);
    return hipGetLastError();
}

// act = silu(gate) * up in fp32 from the fp32 output of the gate/up GEMM over 16-row interleaved weights
// ([16 gate | 16 up] per 32 columns), written as hi + lo bf16 rows [T][ld_act] (columns >= I: zero)
__global__ __launch_bounds__(256) void swiglu_split_kernel(const float* __restrict__ gu, int ld_gu, int I, int ld_act,
                                                           bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
    const int t = blockIdx.x;
    const float* row = gu + (size_t)t * ld_gu;
    for (int c4 = threadIdx.x; c4 < ld_act / 4; c4 += 256) {
        const int c = c4 * 4;
        f32x4 y = {0.f, 0.f, 0.f, 0.f};
        if (c < I) {
            const int blk = c >> 4, o = c & 15;
            const f32x4 g = *reinterpret_cast<const f32x4*>(row + blk * 32 + o);
            const f32x4 u = *reinterpret_cast<const f32x4*>(row + blk * 32 + 16 + o);
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = g[r] / (1.0f + expf(-g[r])) * u[r];
        }
        split_store4(y, hi + (size_t)t * ld_act + c, lo + (size_t)t * ld_act + c);
    }
}

hipError_t launch_swiglu_split(const float* gu, int T, int ld_gu, int I, int ld_act, void* hi, void* lo, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    if (I % 16 || ld_act % 4 || ld_act < I) return hipErrorInvalidValue;
    hipLaunchKernelGGL(swiglu_split_kernel, dim3(T), dim3(256), 0, s, gu, ld_gu, I, ld_act, (bf16_t*)hi, (bf16_t*)lo);
    return hipGetLastError();
}

// h[t][:] = (table_hi[ids[t]][:] + table_lo[ids[t]][:]) * scale
__global__ __launch_bounds__(256) void embed_gather_hp_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ table_hi,
                                                              const bf16_t* __restrict__ table_lo, int dim, float scale,
                                                              float* __restrict__ out) {
    const int t = blockIdx.x;
    const size_t off = (size_t)ids[t] * dim;
    float* dst = out + (size_t)t * dim;
    for (int c = threadIdx.x * 4; c < dim; c += 1024) {
        const bf16x4 a = *reinterpret_cast<const bf16x4*>(table_hi + off + c);
        const bf16x4 b = *reinterpret_cast<const bf16x4*>(table_lo + off + c);
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf2f(a[r]) + bf2f(b[r])) * scale;
        *reinterpret_cast<f32x4*>(dst + c) = o;
    }
}

hipError_t launch_embed_gather_hp(const int* ids, int T, const void* table_hi, const void* table_lo, int dim, float scale,
                                  float* out, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    if (dim % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(embed_gather_hp_kernel, dim3(T), dim3(256), 0, s, ids, (const bf16_t*)table_hi, (const bf16_t*)table_lo,
                       dim, scale, out);
    return hipGetLastError();
}

// sequence index of every packed token
__global__ void seq_of_kernel(const int* __restrict__ seq_offsets, int* __restrict__ seq_of) {
    const int b = blockIdx.x;
    for (int t = seq_offsets[b] + threadIdx.x; t < seq_offsets[b + 1]; t += blockDim.x) seq_of[t] = b;
}

hipError_t launch_seq_of(const int* seq_offsets, int B, int* seq_of, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(seq_of_kernel, dim3(B), dim3(256), 0, s, seq_offsets, seq_of);
    return hipGetLastError();
}

// out[t][n] = (accumulate ? out[t][n] : 0) + alpha * sum_p parts[p][t][n]: closes the fp32 partial planes of the weight-streaming
// GEMMs (gemm_skinny.hip) of a short token-only batch — the K splits of the A_hi W_hi, A_lo W_hi (and A_hi W_lo) passes — in
// a fixed order
__global__ __launch_bounds__(256) void planes_sum_kernel(const float* __restrict__ parts, int n_parts, size_t stride, int ldp, int N,
                                                         float* __restrict__ out, int ldo, float alpha, int accumulate) {
    const int t = blockIdx.y;
    const int n = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (n >= N) return;
    const float* p0 = parts + (size_t)t * ldp + n;
    f32x4 a = *reinterpret_cast<const f32x4*>(p0);
    for (int p = 1; p < n_parts; ++p) a += *reinterpret_cast<const f32x4*>(p0 + (size_t)p * stride);
    float* o = out + (size_t)t * ldo + n;
    f32x4 r = a * alpha;
    if (accumulate) r += *reinterpret_cast<const f32x4*>(o);
    *reinterpret_cast<f32x4*>(o) = r;
}

hipError_t launch_planes_sum(const float* parts, int n_parts, size_t stride, int ldp, int T, int N, float* out, int ldo, float alpha,
                             bool accumulate, hipStream_t s) {
    if (T <= 0 || n_parts <= 0) return hipSuccess;
    if (N % 4 || ldp % 4 || ldo % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(planes_sum_kernel, dim3((N / 4 + 255) / 256, T), dim3(256), 0, s, parts, n_parts, stride, ldp, N, out, ldo, alpha,
                       accumulate ? 1 : 0);
    return hipGetLastError();
}

}  // namespace vr
