// Selection of the K' best of a row of n fp32 values by ONE workgroup of 256 threads, shared by the deep path
// (search_bigk.hip: values = a query's score row) and the grouped search (search_group.hip: values = its group maxima):
//   select_kth      3-pass radix select (11 + 11 + 10 bits of the order-preserving key, histograms in LDS) of the key of
//                   the kp-th largest value, and how many of its ties belong to the kp best;
//   gather_ordered  the positions of the candidates in ascending order: every key above a threshold, then the LOWEST positions
//                   among the keys equal to it — the one place where "lowest ids first at the threshold" is decided;
//   gather_window   the positions at ranks [o, kz) between two such keys, the same tie rule at both edges (search_window.hip:
//                   values = a rewritten score row; search_group_window.hip: values = rewritten group maxima).
//   top_positions / window_positions / sort_gathered   the select-and-gather fronts and the sorting tail of the kernels that
//                   select from a row of final fp32 scores;
//   certified_select  the deep path's flow over a row of bf16 scores: K' best, re-score, tau, gather again or flag.
// What a candidate's exact key is, and the output, are the kernels' own.
// Also here: flag_slots, the part of a flag list that one launch of a fallback kernel walks.
#pragma once
#include "kernels.h"
#include "search_common.h"

namespace vr {

constexpr int SEL_CAND = 1024;              // K' = k + margin <= SEL_CAND; cap of a widened candidate set
constexpr int SEL_MARGIN = 24;              // keeps a true top-k entry inside the candidate set although the values carry bf16 rounding

struct SelectLds {                          // static LDS of a selecting kernel: declared once, __shared__
    unsigned hist[2048];
    int cand[SEL_CAND];                     // gathered positions
    uint64_t keys[SEL_CAND];                // their exact keys (the kernels' re-scoring)
    unsigned prefix;                        // radix select: the key bits fixed so far (those above the pass's own)
    int rank;                               // ... and the rank wanted among the keys that share them (also flag_query's scratch)
    int wc[4][2], run[2];                   // gather_ordered: per-wave and running counts {above, equal}
};

// slots this launch works on: all max_slots, or (count set) entries [sub, sub + max_slots) of a flag list of count[0] queries
__device__ __forceinline__ int flag_slots(const int* count, int sub, int max_slots) {
    return count ? min(max(count[0] - sub, 0), max_slots) : max_slots;
}

// the order-preserving key of a value to select by.  NAN_LOW (the plain search, search_bigk.hip): a NaN sorts below every
// number, -inf included — key 0, which no number has — so that the kp best are numbers as long as there are kp of them
template <bool NAN_LOW>
__device__ __forceinline__ unsigned select_key(float v) {
    return NAN_LOW && !(v == v) ? 0u : f32_orderable(v);
}

struct KthKey {
    unsigned T;                             // key of the kp-th largest value
    int need_eq;                            // how many keys == T belong to the kp best (lowest positions first); kp - need_eq keys are > T
};

// Called by the whole workgroup, 1 <= kp <= n; the LDS must be free (barrier) when it is entered.
template <bool NAN_LOW = false>
__device__ __forceinline__ KthKey select_kth(const float* __restrict__ vals, int n, int kp, SelectLds& L) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { L.prefix = 0u; L.rank = kp; }
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        const int nb = pass < 2 ? 2048 : 1024;
        for (int i = tid; i < 2048; i += 256) L.hist[i] = 0u;
        __syncthreads();
        const int top = shift + (pass < 2 ? 11 : 10);                // the pass's digit: key bits [shift, top)
        const unsigned prefix = L.prefix, mask = top < 32 ? ~0u << top : 0u;    // ... the bits above it: fixed by the passes before
        for (int i = tid; i < n; i += 256) {
            const unsigned key = select_key<NAN_LOW>(vals[i]);
            if ((key & mask) == prefix) atomicAdd(&L.hist[(key >> shift) & (nb - 1)], 1u);
        }
        __syncthreads();
        if (wave == 0) {
            // bins from the top in strides of 64: lane 0 owns the highest bin of the stride
            int rank = L.rank, sel = -1;
            for (int b0 = nb - 64; b0 >= 0 && sel < 0; b0 -= 64) {
                const unsigned h = L.hist[b0 + 63 - lane];
                unsigned incl = h;                                   // inclusive prefix over lanes (from the top)
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                const unsigned total = __shfl(incl, 63, 64);
                if ((int)total >= rank) {
                    const unsigned long long hit = __ballot((int)incl >= rank);
                    const int l = __ffsll((long long)hit) - 1;
                    const unsigned before = __shfl(incl, l, 64) - __shfl(h, l, 64);
                    sel = b0 + 63 - l;
                    rank -= (int)before;
                } else {
                    rank -= (int)total;
                }
            }
            if (lane == 0) {
                L.prefix = prefix | ((unsigned)sel << shift);
                L.rank = rank;
            }
        }
        __syncthreads();
    }
    return KthKey{L.prefix, L.rank};
}

// Positions i of vals[0, n) in ascending order into L.cand: those with key > hi_T from slot 0, then the first `eq_take` with
// key == hi_T from slot n_gt (n_gt = how many are above); nothing is written at or beyond slot `cap`.  Returns the number of
// keys > hi_T (may exceed cap).  Called by the whole workgroup.
template <bool NAN_LOW = false>
__device__ __forceinline__ int gather_ordered(const float* __restrict__ vals, int n, unsigned hi_T, int n_gt, int eq_take, int cap,
                                              SelectLds& L) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 2) L.run[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const unsigned key = i < n ? select_key<NAN_LOW>(vals[i]) : 0u;
        const bool gt = i < n && key > hi_T, eq = i < n && key == hi_T && eq_take > 0;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        if (!__syncthreads_or(gt || eq)) continue;                   // (barrier; most blocks hold no candidate)
        if (lane == 0) { L.wc[wave][0] = __popcll(bg); L.wc[wave][1] = __popcll(be); }
        __syncthreads();
        int og = L.run[0], oe = L.run[1], tg = 0, te = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) { og += L.wc[w][0]; oe += L.wc[w][1]; }
            tg += L.wc[w][0]; te += L.wc[w][1];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (gt) { const int g = og + __popcll(bg & below); if (g < cap) L.cand[g] = i; }
        if (eq) { const int e = oe + __popcll(be & below); if (e < eq_take && n_gt + e < cap) L.cand[n_gt + e] = i; }
        __syncthreads();
        if (tid == 0) { L.run[0] += tg; L.run[1] += te; }
        __syncthreads();
    }
    return L.run[0];
}

struct WindowSelectLds {
    SelectLds s;
    int wc[4][3], run[3];                   // gather_window: per-wave and running counts {== T_a, == T_z, selected}
};

// Positions i of vals[0, n) that are NOT among the first o of the ranking (value descending, then lower position) and ARE among
// its first kz, into L.s.cand in ascending order; returns how many (kz - o when both keys come from select_kth over vals).
//   first o:  key > a.T, or key == a.T at equal-position < a.need_eq      (skip_a == false: o == 0, nothing is excluded)
//   first kz: key > z.T, or key == z.T at equal-position < z.need_eq
// Nothing is written at or beyond slot SEL_CAND.  Called by the whole workgroup; the LDS must be free (barrier).
__device__ __forceinline__ int gather_window(const float* __restrict__ vals, int n, KthKey a, bool skip_a, KthKey z, WindowSelectLds& L) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 3) L.run[tid] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const unsigned key = i < n ? f32_orderable(vals[i]) : 0u;
        const bool eqa = i < n && skip_a && key == a.T, eqz = i < n && key == z.T;
        const bool span = i < n && key >= z.T && (!skip_a || key <= a.T);  // every selected position, and every tie of an edge
        if (!__syncthreads_or(span)) continue;                             // (barrier; most blocks hold none)
        const unsigned long long ba = __ballot(eqa), bz = __ballot(eqz);
        if (lane == 0) { L.wc[wave][0] = __popcll(ba); L.wc[wave][1] = __popcll(bz); }
        __syncthreads();
        int pa = L.run[0] + __popcll(ba & below), pz = L.run[1] + __popcll(bz & below), ta = 0, tz = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) { pa += L.wc[w][0]; pz += L.wc[w][1]; }
            ta += L.wc[w][0]; tz += L.wc[w][1];
        }
        const bool past_o = !skip_a || key < a.T || (eqa && pa >= a.need_eq);
        const bool in_kz = key > z.T || (eqz && pz < z.need_eq);
        const bool sel = span && past_o && in_kz;
        const unsigned long long bs = __ballot(sel);
        if (lane == 0) L.wc[wave][2] = __popcll(bs);
        __syncthreads();
        int ps = L.run[2] + __popcll(bs & below), ts = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) ps += L.wc[w][2];
            ts += L.wc[w][2];
        }
        if (sel && ps < SEL_CAND) L.s.cand[ps] = i;
        __syncthreads();
        if (tid == 0) { L.run[0] += ta; L.run[1] += tz; L.run[2] += ts; }
        __syncthreads();
    }
    return L.run[2];
}

// ---- what the selecting kernels do with the two gathers: each is called by the whole workgroup, the LDS free (barrier) ----
// the positions at ranks [0, kz) of vals[0, n) into L.cand, ascending (1 <= kz <= n); returns the kz-th largest key
template <bool NAN_LOW = false>
__device__ __forceinline__ KthKey top_positions(const float* __restrict__ vals, int n, int kz, SelectLds& L) {
    const KthKey kth = select_kth<NAN_LOW>(vals, n, kz, L);
    gather_ordered<NAN_LOW>(vals, n, kth.T, kz - kth.need_eq, kth.need_eq, SEL_CAND, L);
    return kth;
}

// the positions at ranks [o, kz) of vals[0, n) into L.s.cand, ascending (0 <= o < kz <= n); returns how many were stored
__device__ __forceinline__ int window_positions(const float* __restrict__ vals, int n, int o, int kz, WindowSelectLds& L) {
    KthKey ka{0xFFFFFFFFu, 0};
    if (o > 0) {
        ka = select_kth(vals, n, o, L.s);
        __syncthreads();
    }
    const KthKey kzk = select_kth(vals, n, kz, L.s);
    __syncthreads();
    return min(gather_window(vals, n, ka, o > 0, kzk, L), SEL_CAND);
}

// keys make_key(vals[i], i) of the n_sel gathered positions, padded to n_sort (a power of two) and sorted: L.keys[0, n_sort)
__device__ __forceinline__ void sort_gathered(const float* __restrict__ vals, int n_sel, int n_sort, SelectLds& L) {
    const int tid = threadIdx.x;
    for (int c = tid; c < n_sort; c += 256) {
        uint64_t key = KEY_NONE;
        if (c < n_sel) { const int i = L.cand[c]; key = make_key(vals[i], (uint32_t)i); }
        L.keys[c] = key;
    }
    __syncthreads();
    block_bitonic_desc(L.keys, n_sort, tid, 256);
}

// n_sort of a launch: the power of two (>= 64) that holds k keys
inline int sort_width(int k) {
    int n_sort = 64;
    while (n_sort < k) n_sort <<= 1;
    return n_sort;
}

// ---- the certifying select (search_bigk.hip has the why; search_filter.hip and search_group.hip run it on their own rows) ----
// The kp best of vals[0, n), gathered by top_positions<NAN_LOW> (T: the key it returned; the kernel loads its query between the
// two, so that the select runs without it), are re-scored (key_of(c): the exact key of candidate position c, called by a whole
// wave, wave-uniform) and sorted into L.keys.  universe = how many positions can rank at all.  With `certify`, and candidates
// left outside (kp < universe): tau = (k-th exact score) - eps_of(), lowered by one ulp with TAU_DOWN; a candidate
// outside has a value <= the kp-th; if that does not lie below tau, EVERY position with a value >= tau is gathered and
// re-scored instead (up to SEL_CAND), else the query is to be flagged.  Returns how many keys of L.keys stand; *what: 0 certified
// as it stood, 1 after the second gather, 2 to be flagged; *tau: -inf where none was taken.
// NAN_LOW (the plain search: ranked keys): a NaN value is selected last, and with fewer than k numbers among the re-scored —
// the candidates then hold EVERY position that ranks: a NaN query, or fewer than k rows free of NaN — the result stands as it is.
// Called by the whole workgroup, the LDS free (barrier).
template <bool NAN_LOW, bool TAU_DOWN, typename KeyOf, typename EpsOf>
__device__ __forceinline__ int certified_select(const float* __restrict__ vals, int n, int universe, int kp, unsigned T, int k,
                                                bool certify, KeyOf key_of, EpsOf eps_of, SelectLds& L, int* what, float* tau) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto rescore_sort = [&](int m) {
        int n2 = 1;
        while (n2 < m) n2 <<= 1;
        for (int c = m + tid; c < n2; c += 256) L.keys[c] = KEY_NONE;
        for (int c = wave; c < m; c += 4) {
            const uint64_t key = key_of(L.cand[c]);
            if (lane == 0) L.keys[c] = key;
        }
        __syncthreads();
        block_bitonic_desc(L.keys, n2, tid, 256);
    };
    rescore_sort(kp);
    *what = 0;
    *tau = -INFINITY;
    if (certify && kp < universe && (!NAN_LOW || L.keys[k - 1] != KEY_NONE)) {      // kp >= k here (kp < universe => kp = k + margin)
        const float t = key_score(L.keys[k - 1]) - eps_of();
        *tau = TAU_DOWN ? one_ulp_down(t) : t;
        if (!(orderable_f32(T) < *tau)) {
            // every position whose value is >= tau (strictly above the key just below tau's)
            __syncthreads();
            const unsigned tk = f32_orderable(*tau);
            const int m = gather_ordered<NAN_LOW>(vals, n, tk ? tk - 1u : 0u, 0, 0, SEL_CAND, L);
            __syncthreads();
            if (m <= SEL_CAND && m >= kp) { rescore_sort(m); kp = m; *what = 1; }
            else *what = 2;
        }
    }
    return kp;
}

}  // namespace vr
