// The nucleus sampler of the answer generation (vr_chat_sample / vr_op_chat_sample; definition in include/visrag_hip.h): any
// top-k (0 = off) and top-p over the whole row, by a radix select instead of chat_kernels.hip's K rounds of a max.
//
// One workgroup of 1024 lanes per row, one launch, no global scratch: the row (V fp32 logits, just written by the head GEMM)
// is read once per pass (SampleRow::each: float4 loads, several in flight per lane), and every pass recomputes
// z = penalised logit * (1 / temperature) from the logit and the seen bit.  Seven passes at (top_k 100, top_p 0.8), five when
// only one of the two cuts.
//   1. m = the largest z.
//   2. histogram of the top 11 bits of f2ord(z): candidates (u32) and mass (u64 fixed point, exp(z - m) * 2^40) per bin.
//   3. count cut (when top_k cuts at all): descend 11 / 11 / 10 bits to the key that holds the K-th candidate -> Z.
//   4. mass cut (top_p < 1): the same descent to the key that holds the nucleus edge, on the SAME top histogram.
//   5. the tier of keys equal to the edge key keeps its lowest token ids; how many is a closed form (one w for all of them),
//      which ones is an ordered count over the lanes — two more passes, run only when the tier is split.
//   6. argmax of fma(s, 1 / T, gumbel noise) over the kept tokens.
// The sums are integers, so the kept set does not depend on the order the lanes add in.
#include "chat_score.h"
#include "common.h"
#include "gen_math.h"
#include "kernels.h"

namespace vr {

namespace {

constexpr int SMP_THREADS = 1024, SMP_WAVES = SMP_THREADS / 64;
constexpr int SMP_UNROLL = 4;                        // 16-byte loads a lane has in flight in a pass
constexpr int SMP_BINS = 2048;                       // 11-bit digits (the last digit has 10: half the bins)
constexpr float SMP_ONE = 1099511627776.0f;          // 2^40: the mass of the best candidate

typedef unsigned long long u64;

struct SampleRow {
    const float* x;
    const unsigned* seen;
    float pen, inv_t;
    int V;
    // token c with logit xv and seen word `word` -> penalised logit s and tempered z; false: no candidate (z is -inf or NaN)
    __device__ __forceinline__ bool score(int c, float xv, unsigned word, float& s, float& z) const {
        s = chat_score(CHAT_SEL_SAMPLE, xv, (word >> (c & 31)) & 1u, pen, 0.f, 0.f);
        z = chat_tempered(s, inv_t);
        return z > -INFINITY;
    }
    __device__ __forceinline__ bool eval(int c, float& s, float& z) const { return score(c, x[c], seen[c >> 5], s, z); }
    // f(token, s, z) for every candidate of the row, each token once, spread over the lanes.  The passes live on loads in
    // flight (one CU against L2 / HBM latency): a 16-byte aligned row is read as float4, SMP_UNROLL of them issued per lane
    // before the first is used (four consecutive tokens share a seen word); any other row token by token, 2 SMP_UNROLL ahead.
    template <typename F>
    __device__ __forceinline__ void each(F&& f) const {
        if (((size_t)x & 15) == 0) {
            const f32x4* x4 = (const f32x4*)x;
            const long long V4 = V >> 2;
            long long q = threadIdx.x;                        // (64 bits: the look-ahead may pass 2^31 when V is close to it)
            for (; q + (SMP_UNROLL - 1) * SMP_THREADS < V4; q += SMP_UNROLL * SMP_THREADS) {
                f32x4 xv[SMP_UNROLL];
                unsigned wd[SMP_UNROLL];
#pragma unroll
                for (int j = 0; j < SMP_UNROLL; ++j) { xv[j] = x4[q + j * SMP_THREADS]; wd[j] = seen[(q + j * SMP_THREADS) >> 3]; }
#pragma unroll
                for (int j = 0; j < SMP_UNROLL; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float s, z;
                        const int t = (int)(4 * (q + j * SMP_THREADS)) + k;
                        if (score(t, xv[j][k], wd[j], s, z)) f(t, s, z);
                    }
            }
            for (; q < V4; q += SMP_THREADS) {
                const f32x4 xv = x4[q];
                const unsigned wd = seen[q >> 3];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float s, z;
                    const int t = (int)(4 * q) + k;
                    if (score(t, xv[k], wd, s, z)) f(t, s, z);
                }
            }
            const long long c = 4 * V4 + threadIdx.x;         // the last V % 4 tokens
            float s, z;
            if (c < V && eval((int)c, s, z)) f((int)c, s, z);
            return;
        }
        long long c = threadIdx.x;
        for (; c + (2 * SMP_UNROLL - 1) * SMP_THREADS < V; c += 2 * SMP_UNROLL * SMP_THREADS) {
            float xv[2 * SMP_UNROLL];
            unsigned wd[2 * SMP_UNROLL];
#pragma unroll
            for (int j = 0; j < 2 * SMP_UNROLL; ++j) { xv[j] = x[c + j * SMP_THREADS]; wd[j] = seen[(c + j * SMP_THREADS) >> 5]; }
#pragma unroll
            for (int j = 0; j < 2 * SMP_UNROLL; ++j) {
                float s, z;
                const int t = (int)(c + j * SMP_THREADS);
                if (score(t, xv[j], wd[j], s, z)) f(t, s, z);
            }
        }
        for (; c < V; c += SMP_THREADS) {
            float s, z;
            if (eval((int)c, s, z)) f((int)c, s, z);
        }
    }
};

__device__ __forceinline__ u64 sample_mass(float z, float m) { return z == m ? (u64)SMP_ONE : (u64)(expf(z - m) * SMP_ONE); }

struct SampleCut { unsigned bin, c_before; u64 m_before; };

struct SampleShared {
    unsigned h1c[SMP_BINS], h2c[SMP_BINS];
    u64 h1m[SMP_BINS], h2m[SMP_BINS];
    unsigned wc[SMP_WAVES];
    u64 wm[SMP_WAVES], wk[SMP_WAVES];
    unsigned wk2[SMP_WAVES];
    SampleCut cut;
    int tier_tok;
};

// (c, m): a thread's own sums -> the sums of the threads below it; tot_*: the block's
__device__ __forceinline__ void block_scan(unsigned& c, u64& m, SampleShared& sh, unsigned& tot_c, u64& tot_m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned ci = c;
    u64 mi = m;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned tc = __shfl_up(ci, off, 64);
        const u64 tm = __shfl_up(mi, off, 64);
        if (lane >= off) { ci += tc; mi += tm; }
    }
    if (lane == 63) { sh.wc[wave] = ci; sh.wm[wave] = mi; }
    __syncthreads();
    unsigned bc = 0;
    u64 bm = 0;
    tot_c = 0; tot_m = 0;
    for (int w = 0; w < SMP_WAVES; ++w) {
        if (w == wave) { bc = tot_c; bm = tot_m; }
        tot_c += sh.wc[w]; tot_m += sh.wm[w];
    }
    __syncthreads();
    c = bc + ci - c;
    m = bm + mi - m;
}

// Walk the bins [0, 1024 * per) of a histogram from the top.  BY_MASS false: the bin that holds the need-th candidate
// (1-based).  BY_MASS true: the first bin behind which the mass ahead, m_base + everything down to and including the bin, is no
// longer below pz — the caller guarantees that m_base itself is.  The bin, and the count and mass above it, land in sh.cut;
// tot_*: the histogram's sums.
template <bool BY_MASS>
__device__ __forceinline__ void cut_search(const unsigned* hc, const u64* hm, int per, unsigned need, u64 m_base, double pz,
                                           SampleShared& sh, unsigned& tot_c, u64& tot_m) {
    const int nb = SMP_THREADS * per;
    unsigned c[2] = {0u, 0u}, ec = 0;
    u64 mm[2] = {0ull, 0ull}, em = 0;
    for (int j = 0; j < per; ++j) {
        const int b = nb - 1 - (per * (int)threadIdx.x + j);
        c[j] = hc[b]; mm[j] = hm[b];
        ec += c[j]; em += mm[j];
    }
    block_scan(ec, em, sh, tot_c, tot_m);
    for (int j = 0; j < per; ++j) {
        const unsigned ic = ec + c[j];
        const u64 im = em + mm[j];
        const bool hit = BY_MASS ? ((double)(m_base + em) < pz && !((double)(m_base + im) < pz)) : (ec < need && need <= ic);
        if (hit) { sh.cut.bin = (unsigned)(nb - 1 - (per * (int)threadIdx.x + j)); sh.cut.c_before = ec; sh.cut.m_before = em; }
        ec = ic; em = im;
    }
    __syncthreads();
}

// The two lower digits of a cut whose top digit is in sh.cut: one pass over the row per digit, into the second histogram.
// -> the edge key e, the candidates (c_above) and the mass (m_above) of the keys above it, the tier's size n_tier and the mass
// w_tier of each of its members.
template <bool BY_MASS>
__device__ __forceinline__ void cut_descend(const SampleRow& row, float m, unsigned need, double pz, SampleShared& sh, unsigned& e,
                                            unsigned& c_above, u64& m_above, unsigned& n_tier, u64& w_tier) {
    const int tid = threadIdx.x;
    unsigned prefix = sh.cut.bin, tc;
    u64 tm;
    c_above = sh.cut.c_before; m_above = sh.cut.m_before;
    __syncthreads();                                          // sh.cut is read: the searches below write it again
    for (int level = 0; level < 2; ++level) {
        const int shift = level == 0 ? 21 : 10, dshift = level == 0 ? 10 : 0;
        const unsigned dmask = level == 0 ? 2047u : 1023u;
        for (int b = tid; b < SMP_BINS; b += SMP_THREADS) { sh.h2c[b] = 0u; sh.h2m[b] = 0ull; }
        __syncthreads();
        row.each([&](int, float, float z) {
            const unsigned o = f2ord(z);
            if ((o >> shift) != prefix) return;
            const unsigned d = (o >> dshift) & dmask;
            atomicAdd(&sh.h2c[d], 1u);
            atomicAdd(&sh.h2m[d], sample_mass(z, m));
        });
        __syncthreads();
        cut_search<BY_MASS>(sh.h2c, sh.h2m, level == 0 ? 2 : 1, need - c_above, m_above, pz, sh, tc, tm);
        const unsigned bin = sh.cut.bin;
        c_above += sh.cut.c_before; m_above += sh.cut.m_before;
        prefix = (prefix << (level == 0 ? 11 : 10)) | bin;
        if (level == 1) { n_tier = sh.h2c[bin]; w_tier = sh.h2m[bin] / n_tier; }
        __syncthreads();
    }
    e = prefix;
}

}  // namespace

// Row i of the grid: logits row sel.lrow[i], seen set sel.srow[i] -> (score, token, n_kept, cut_token) at index i.
__global__ __launch_bounds__(SMP_THREADS) void chat_sample_kernel(ChatSel sel, const float* __restrict__ logits, int ld, int V,
                                                                  const unsigned* __restrict__ seen, int words, float pen, float inv_t,
                                                                  int top_k, double top_p, unsigned long long seed, unsigned step,
                                                                  float* __restrict__ o_score, int* __restrict__ o_tok,
                                                                  int* __restrict__ o_kept, int* __restrict__ o_cut) {
    __shared__ SampleShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x;
    const SampleRow row{logits + (size_t)sel.lrow[i] * ld, seen + (size_t)sel.srow[i] * words, pen, inv_t, V};

    for (int b = tid; b < SMP_BINS; b += SMP_THREADS) { sh.h1c[b] = 0u; sh.h1m[b] = 0ull; }
    if (tid == 0) sh.tier_tok = -1;
    // ---- 1. the best candidate's key
    unsigned mo = 0u;
    row.each([&](int, float, float z) { mo = max(mo, f2ord(z)); });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mo = max(mo, (unsigned)__shfl_xor(mo, off, 64));
    if (lane == 0) sh.wc[wave] = mo;
    __syncthreads();
    mo = 0u;
    for (int w = 0; w < SMP_WAVES; ++w) mo = max(mo, sh.wc[w]);
    __syncthreads();
    if (mo == 0u) {                                           // no candidate at all
        if (tid == 0) { o_score[i] = -INFINITY; o_tok[i] = -1; o_kept[i] = 0; o_cut[i] = -1; }
        return;
    }
    const float m = ord2f(mo);
    // ---- 2. the top digit's histogram: it serves both cuts
    row.each([&](int, float, float z) {
        const unsigned d = f2ord(z) >> 21;
        atomicAdd(&sh.h1c[d], 1u);
        atomicAdd(&sh.h1m[d], sample_mass(z, m));
    });
    __syncthreads();
    unsigned C;
    u64 total;
    {   // the sums of the row (a search for the first candidate; its result is not used)
        cut_search<false>(sh.h1c, sh.h1m, 2, 1u, 0ull, 0.0, sh, C, total);
    }
    const unsigned K = top_k == 0 ? C : min((unsigned)top_k, C);
    const bool by_mass = top_p < 1.0, by_count = !by_mass || K < C;
    // ---- 3. the count cut: the key of the K-th candidate, and Z
    unsigned eK = 0u, rK = 0u, nK = 0u;
    u64 Z = total;
    if (by_count) {
        unsigned tc, c_above;
        u64 tm, m_above, w;
        cut_search<false>(sh.h1c, sh.h1m, 2, K, 0ull, 0.0, sh, tc, tm);
        cut_descend<false>(row, m, K, 0.0, sh, eK, c_above, m_above, nK, w);
        rK = K - c_above;
        Z = m_above + (u64)rK * w;
    }
    // ---- 4. the mass cut: candidate j is kept iff the mass ahead of it is below top_p * Z (fp64)
    unsigned e = eK, r = rK, n_tier = nK, n_kept = K;
    if (by_mass) {
        const double pz = top_p * (double)Z;
        unsigned tc, eM, c_above, nM;
        u64 tm, m_above, w;
        cut_search<true>(sh.h1c, sh.h1m, 2, 0u, 0ull, pz, sh, tc, tm);
        cut_descend<true>(row, m, 0u, pz, sh, eM, c_above, m_above, nM, w);
        // members 0 .. rM - 1 of the tier have m_above + index * w below pz: member 0 has, member nM would not
        unsigned lo = 0u, hi = nM;
        while (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            if ((double)(m_above + (u64)mid * w) < pz) lo = mid + 1; else hi = mid;
        }
        if (!by_count || c_above + lo <= K) { e = eM; r = lo; n_tier = nM; n_kept = c_above + lo; }
    }
    // ---- 5. a split tier keeps its r lowest token ids: the r-th of them, counted wave by wave over contiguous ranges
    const bool whole = r == n_tier;
    if (!whole) {
        const long long seg = (((long long)V + SMP_WAVES - 1) / SMP_WAVES + 63) & ~63ll;
        const long long lo = min((long long)V, wave * seg), hi = min((long long)V, lo + seg);
        unsigned cnt = 0u;
        for (long long base = lo; base < hi; base += 64) {
            const long long c = base + lane;
            float s, z;
            const bool hit = c < hi && row.eval((int)c, s, z) && f2ord(z) == e;
            cnt += (unsigned)__popcll(__ballot(hit));
        }
        if (lane == 0) sh.wc[wave] = cnt;
        __syncthreads();
        unsigned before = 0u;
        for (int w = 0; w < wave; ++w) before += sh.wc[w];
        if (before < r && r <= before + cnt) {                // this wave holds the r-th (wave-uniform)
            unsigned run = before;
            for (long long base = lo; base < hi; base += 64) {
                const long long c = base + lane;
                float s, z;
                const bool hit = c < hi && row.eval((int)c, s, z) && f2ord(z) == e;
                const u64 bal = __ballot(hit);
                const unsigned n = (unsigned)__popcll(bal);
                if (run + n >= r) {
                    const unsigned rank = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
                    if (hit && run + rank + 1u == r) sh.tier_tok = (int)c;
                    break;
                }
                run += n;
            }
        }
        __syncthreads();
    }
    const int cut_tok = sh.tier_tok;                          // (-1 while the tier is whole: found in the pass below)
    // ---- 6. the draw: the kept token of largest z + noise; among equals the better-ranked (higher z, then lower id)
    u64 k1 = 0ull;
    unsigned k2 = 0u;
    row.each([&](int c, float s, float z) {
        const unsigned o = f2ord(z);
        if (o < e || (o == e && !whole && c > cut_tok)) return;
        if (whole && o == e) atomicMax(&sh.tier_tok, c);
        const float v = chat_noisy(s, inv_t, gumbel_noise(seed, step, (unsigned)c));
        const u64 a1 = ((u64)f2ord(v) << 32) | o;
        const unsigned a2 = ~(unsigned)c;
        if (a1 > k1 || (a1 == k1 && a2 > k2)) { k1 = a1; k2 = a2; }
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 b1 = __shfl_xor(k1, off, 64);
        const unsigned b2 = __shfl_xor(k2, off, 64);
        if (b1 > k1 || (b1 == k1 && b2 > k2)) { k1 = b1; k2 = b2; }
    }
    if (lane == 0) { sh.wk[wave] = k1; sh.wk2[wave] = k2; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < SMP_WAVES; ++w)
            if (sh.wk[w] > k1 || (sh.wk[w] == k1 && sh.wk2[w] > k2)) { k1 = sh.wk[w]; k2 = sh.wk2[w]; }
        const int tok = k1 ? (int)~k2 : -1;                   // (position 0 is always kept: k1 is never 0 here)
        float s = -INFINITY, z;
        if (tok >= 0) row.eval(tok, s, z);
        o_score[i] = s; o_tok[i] = tok; o_kept[i] = tok >= 0 ? (int)n_kept : 0; o_cut[i] = tok >= 0 ? sh.tier_tok : -1;
    }
}

hipError_t launch_chat_sample(const ChatSel& sel, const float* logits, int ld, int V, const unsigned* seen, int words, float pen,
                              float temperature, int top_k, double top_p, unsigned long long seed, unsigned step, float* o_score,
                              int* o_tok, int* o_kept, int* o_cut, hipStream_t s) {
    if (sel.n < 1 || sel.n > CHAT_MAX_ROWS || V < 1 || ld < V || words < (V + 31) / 32 || top_k < 0 || !(temperature > 0.f) ||
        !(top_p > 0.0 && top_p <= 1.0))
        return hipErrorInvalidValue;
    const float inv_t = 1.0f / temperature;
    hipLaunchKernelGGL(chat_sample_kernel, dim3(sel.n), dim3(SMP_THREADS), 0, s, sel, logits, ld, V, seen, words, pen, inv_t, top_k, top_p,
                       seed, step, o_score, o_tok, o_kept, o_cut);
    return hipGetLastError();
}

}  // namespace vr
