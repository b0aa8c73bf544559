// The search index's handle and the host helpers its three files share: index.hip (life cycle, vr_index_search*),
// index_searches.hip (the score-row searches) and index_rows.hip (editing in place).  A row-level search and its document-level
// sibling (range, rank, window, fused) keep their state in two members of ONE type and run through one body; what every such
// body is made of stands below: the argument checks, the staging of pairs and of sub-query groups, the call frame (staged
// queries and filter ids, score rows, group maxima) and the growing result store of the range searches.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "engine_common.h"

constexpr int CERT_WORDS = 32, CERT_FLAG = 2, CERT_FLAG2 = 3, CERT_STATS = 4, CERT_NSTATS = 6;   // (the two flag counters are consecutive: cleared together)
constexpr int GRP_STATS = 2, GRP_LIST = 8, GRP_WORDS = GRP_LIST + 256;
constexpr int FLT_STATS = 2, FLT_LIST = 8, FLT_WORDS = FLT_LIST + 256;
constexpr int STAT_WORDS = 3, RANGE_TOTAL = STAT_WORDS, RANGE_WORDS = RANGE_TOTAL + 1;   // u64 words of the searches below: 0..2 the counters of
                                  // the search's *_search_stats; the range searches: then a block's total
constexpr int64_t QBLK = 256;     // queries (sub-queries) of a block: one fp32 score row each, as on the deep path

// ---- the state of a row-level search and of its document-level sibling: one type, a member each ---------------------------------
// (what only the document-level search uses — group maxima B, best rows R, a third array — the row-level one never reserves)
struct RangeState {                   // range / document range search: the result and what makes it
    DevBuf scores, rows, groups;      // the result: f32 scores [cap] | int64 (best) rows [cap] | int64 groups [cap], valid entries [0, total)
    int64_t cap = 0, total = -1;      // -1: no result (none yet, dropped with what it names, or the last search failed)
    DevBuf thr, lims, cnt, off, B, R, state;   // staged thresholds / lims of a host caller | int entries kept [256][slots] | int their
                                      // exclusive scan per query | group maxima [256][ldB], rewritten in place | int best rows [256][ldB]
                                      // | u64 words: [0..2] the counters, [RANGE_TOTAL] a block's total
    int64_t* host_total = nullptr;    // pinned host word: the block total as the host reads it
};
struct RankState {                    // rank / document rank search (and the counts): no stored result
    DevBuf q, v, bar, eps, B, out, state;   // int query of every pair | int targets or f32 thresholds | u64 bars | f32 eps per pair |
                                      // group maxima [256][ldB], only read | staged counts (document level) | u64 words: the counters
};
struct WindowState {                  // windowed / document window search: no stored result
    DevBuf off, edge, B, R, out, state;   // int64 offsets of the call's queries | f32 band edges {lo, hi} [256][2] (document level:
                                      // then int present groups [256]) of a block's queries | group maxima [256][ldB], rewritten in
                                      // place | int best rows [256][ldB] | staged out_groups | u64 words: the counters
};
struct MultiState {                   // fused / fused document search: no stored result
    DevBuf lims, fsub, B, F, eps, edge, docs, which, evs, evr, state;   // int lims of the call's groups | int filter of every
                                      // sub-query | document maxima [256][ldB], only read | fused rows [256][ldB], rewritten in place |
                                      // f32 eps of a block's sub-queries | f32 band edge [256] (document level: then int present
                                      // documents [256]) of a block's groups | staged out_docs | out_which | out_ev_scores |
                                      // out_ev_rows | u64 words: the counters
};

struct vr_index_s {
    int device = 0, dim = 0;
    int64_t cap = 0, n = 0;
    DevBuf f32, bf16;                 // [cap_pad][dim]
    DevBuf q32, qbf, cs, ci, ck, os, oi, ok, thr, sbuf;  // query staging / candidates / outputs / thresholds / score rows
    int64_t qcap = 0, ccap = 0, kcap = 0;
    // certification state (search_common.h), 32 words: f32 [0] largest row norm, [1] largest bf16 rounding residual of a row;
    // int [2] flag count, [3] second-level flag count (exact fp32 pass); u32 [4..9] query counters {certified at once, after
    // extended re-scoring, flagged, uncertified mode, candidates gathered a second time, of the flagged: exact fp32 pass}
    DevBuf cert, flags, flagq;        // flags: int flag_list[fcap] | int flag2_list[fcap] | f32 flag_tau[fcap]; flagq: bf16 [fcap][dim]
    int64_t fcap = 0;
    int* huge_seen = nullptr;         // pinned host word: a streaming search met a band beyond search_band_max() rows (SearchArgs::huge_seen)
    float eps_rel = -2.f;             // -2: the rigorous data-dependent default; >= 0: the caller's eps_rel |q| max|d|; else off
    // Every search below has state of its own in a member of its own: no other search reads any of it (the filters excepted:
    // range, rank, windowed, fused and diversified search read flt.bits / flt.count and stage their filter ids in flt.ids; the
    // document-level searches do too, and read grp.off / grp.n_groups: the grouping is the index's, not a search's).
    struct {                          // grouped search (vr_index_search_groups, search_group.hip)
        int64_t n_groups = 0;         // 0: no grouping set (vr_index_add / vr_index_reset drop it)
        DevBuf off, B, out, state;    // int first rows [n_groups + 1] | group maxima [256][ldB] | staged out_groups | int words: [0] flag
                                      // count, [1] unused (cleared with it), u32 [2..4] the three counters of vr_index_group_search_stats,
                                      // [GRP_LIST..] flag list of a block of <= 256 queries
    } grp;
    struct {                          // filtered search (vr_index_search_filtered, search_filter.hip), independent of the grouping
        int64_t n_filters = 0;        // 0: no filters set (vr_index_add / vr_index_reset drop them)
        DevBuf bits, count, ids, state;   // u32 [n_filters][ceil(n / 32)] the library's copy | int allowed rows [n_filters] | staged
                                      // filter_of_query (filter_of_group) of a host caller | int words laid out as grp.state's: [0] flag count,
                                      // [1] unused, u32 [2..4] the counters of vr_index_filter_search_stats, [FLT_LIST..] flag list of a block
    } flt;
    // diversified search (vr_index_search_diverse, search_diverse.hip): its pool — the result of the plain or the filtered search for
    // k = pool — in buffers of its own, because that very search overwrites the shared scratch
    struct { DevBuf scores, ids; } div;   // f32 pool scores [nq][pool] | int64 pool ids [nq][pool]
    RangeState rng, grng;             // vr_index_search_range (search_range.hip) | vr_index_search_groups_range (search_group_range.hip);
                                      // total = -1 also after vr_index_reset / _remove / _update, grng's after _add / _set_groups
    RankState rnk, grnk;              // vr_index_rank_rows / _count_range (search_rank.hip) | vr_index_rank_groups /
                                      // _count_groups_range (search_group_rank.hip)
    WindowState win, gwin;            // vr_index_search_window (search_window.hip) | vr_index_search_groups_window (search_group_window.hip)
    MultiState mul, mgrp;             // vr_index_search_multi (search_multi.hip) | vr_index_search_multi_groups (search_multi_group.hip)
    struct {                          // rank-fusion search (vr_index_search_rrf, search_rrf.hip): no stored result
        DevBuf scores, ids, groups;   // the pool — the plain, the filtered or the document window search's result for k = depth, by
                                      // that search as it stands — f32 [n_sub][depth] | int64 rows | int64 groups (by_groups: the lists)
        DevBuf lims, fsub, w, hits, state;   // int lims of the call's groups | int filter of every sub-query | f32 weights | staged
                                      // out_hits | u64 words: [0..2] the counters of vr_index_rrf_search_stats
    } rrf;
    struct {                          // editing in place (vr_index_remove / vr_index_update / vr_index_get_rows, index_edit.hip)
        DevBuf ids, rows, bits2;      // int row ids of the call | rows of a host caller, staged (<= EDIT_SCRATCH bytes for get_rows) |
                                      // the filters compacted out of place: swapped with flt.bits
    } edit;
    // per-stage HIP events (vr_index_set_search_profile): convert | thresholds | sweep | merge | exact pass
    bool prof_on = false;
    hipEvent_t prof_ev[SEARCH_PROF_EVENTS] = {};
    double prof_ms[SEARCH_PROF_EVENTS - 1] = {};
    int64_t prof_calls = 0;
};

// queries [nq][dim] -> top k per query, as (scores, ids) or as packed keys with `id_offset` added to the row ids (index.hip)
int search_impl(vr_index_t ix, const float* queries, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids,
                unsigned long long* out_keys, int64_t id_offset, int32_t on_device, void* stream);

// ---- staging: what a host caller's arrays go through -------------------------------------------------------------------------
// Query staging for passes of up to `nqp` (padded) queries: capacity of the bf16 rows and thresholds, host queries to the
// device.  *q32: the fp32 queries on the device.
static inline int stage_queries(vr_index_t ix, const float* queries, int32_t nq, int64_t nqp, int32_t on_device, hipStream_t s,
                                const float** q32) {
    if (ix->qcap < nqp) {
        VRCHK(ix->qbf.alloc((size_t)nqp * ix->dim * 2));
        VRCHK(ix->thr.alloc((size_t)nqp * 8));            // thresholds | what the lists are complete down to (thr_cert)
        ix->qcap = nqp;
    }
    *q32 = queries;
    if (!on_device) {
        VRCHK(ix->q32.reserve((size_t)nq * ix->dim * 4));
        HIPCHK(hipMemcpyAsync(ix->q32.p, queries, (size_t)nq * ix->dim * 4, hipMemcpyHostToDevice, s));
        *q32 = ix->q32.as<float>();
    }
    return VR_OK;
}

// One input array of n elements: the kernels read *dev — the caller's own array, or a host array's copy in `buf` (the copy is
// asynchronous: a caller whose source dies before the call's last synchronisation synchronises itself)
template <typename T>
static inline int stage_input(DevBuf& buf, const T* in, size_t n, int32_t on_device, hipStream_t s, const T** dev) {
    *dev = in;
    if (!on_device) {
        VRCHK(buf.reserve(n * sizeof(T)));
        HIPCHK(hipMemcpyAsync(buf.p, in, n * sizeof(T), hipMemcpyHostToDevice, s));
        *dev = buf.as<T>();
    }
    return VR_OK;
}

// One output array of n elements: the kernels write *dev — the caller's own array, or for a host caller the staging buffer
// that return_output copies back (the caller synchronises the stream after the last one)
template <typename T>
static inline int stage_output(DevBuf& buf, T* out, size_t n, int32_t on_device, T** dev) {
    *dev = out;
    if (!on_device) { VRCHK(buf.reserve(n * sizeof(T))); *dev = buf.as<T>(); }
    return VR_OK;
}
template <typename T>
static inline int return_output(T* out, const T* dev, size_t n, int32_t on_device, hipStream_t s) {
    if (!on_device) HIPCHK(hipMemcpyAsync(out, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
    return VR_OK;
}

// n result slots of a search over no row: (-inf, -1) and, for the fused search, which = -1
static inline int fill_tails(float* out_scores, int64_t* out_ids, int32_t* out_which, size_t n, int32_t on_device, hipStream_t s) {
    if (on_device) {
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)out_scores, (int)0xFF800000u, n, s));     // -inf
        HIPCHK(hipMemsetAsync(out_ids, 0xFF, n * 8, s));                                   // -1
        if (out_which) HIPCHK(hipMemsetAsync(out_which, 0xFF, n * 4, s));
    } else {
        std::fill(out_scores, out_scores + n, -INFINITY);
        std::fill(out_ids, out_ids + n, (int64_t)-1);
        if (out_which) std::fill(out_which, out_which + n, (int32_t)-1);
    }
    return VR_OK;
}

// ---- argument checks that more than one search makes ------------------------------------------------------------------------------
// a host array of n floats (`what`: the argument's name): every entry finite
static inline int check_finite(const float* v, int64_t n, const char* what) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return fail(VR_ERR_INVALID, "%s[%lld] = %g is not finite", what, (long long)i, (double)v[i]);
    return VR_OK;
}

// the lims of the (query, target) pairs of nq queries: lims[0] == 0, non-decreasing, *np = lims[nq] < 2^31 pairs
static inline int check_pair_lims(const int64_t* lims, int32_t nq, int64_t* np) {
    if (lims[0] != 0) return fail(VR_ERR_INVALID, "lims[0] = %lld must be 0", (long long)lims[0]);
    for (int32_t q = 0; q < nq; ++q)
        if (lims[q + 1] < lims[q]) return fail(VR_ERR_INVALID, "lims[%d] = %lld decreases", (int)q + 1, (long long)lims[q + 1]);
    *np = lims[nq];
    if (*np >= ((int64_t)1 << 31)) return fail(VR_ERR_INVALID, "%lld pairs: too many for one call", (long long)*np);
    return VR_OK;
}

// the lims of n_groups >= 1 groups (`noun`: "group", "question") of n_members members (`members`: "sub-queries", "lists"):
// lims[0] == 0, every group holds 1..256, lims[n_groups] == n_members.  depth > 0: the rank fusion's rule as well, a group's
// members x depth within rrf_max_entries().  *most (if set) = the most members of a group.
static inline int check_group_lims(const int64_t* lims, int32_t n_groups, int32_t n_members, const char* noun, const char* members,
                                   int32_t depth, int64_t* most) {
    if (lims[0] != 0) return fail(VR_ERR_INVALID, "lims[0] = %lld, not 0", (long long)lims[0]);
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t m = lims[g + 1] - lims[g];
        if (m < 0) return fail(VR_ERR_INVALID, "lims[%d] = %lld decreases", (int)g + 1, (long long)lims[g + 1]);
        if (m == 0) return fail(VR_ERR_INVALID, "%s %d is empty", noun, (int)g);
        if (m > 256) return fail(VR_ERR_INVALID, "%s %d holds %lld %s (1..256)", noun, (int)g, (long long)m, members);
        if (depth > 0 && m * depth > rrf_max_entries())
            return fail(VR_ERR_INVALID, "%s %d holds %lld %s x depth %d = %lld entries (at most %d)", noun, (int)g, (long long)m, members,
                        (int)depth, (long long)(m * depth), rrf_max_entries());
        if (most) *most = std::max(*most, m);
    }
    if (lims[n_groups] != n_members)
        return fail(VR_ERR_INVALID, "lims[%d] = %lld, not the %d %s", (int)n_groups, (long long)lims[n_groups], (int)n_members, members);
    return VR_OK;
}

static inline int check_grouping(vr_index_t ix) {
    if (ix->grp.n_groups <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no grouping set for the rows of the index (vr_index_set_groups)");
    return VR_OK;
}

// ---- rank fusion: what vr_rrf_fuse and vr_index_search_rrf check of n_groups >= 1 groups of lists before anything else --------
// *max_entries = the largest m * depth of a group
static inline int rrf_check(const int64_t* lims, int32_t n_lists, int32_t n_groups, int32_t k, int32_t depth, float c,
                            const float* weights, int* max_entries) {
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (depth <= 0 || depth > search_bigk_max()) return fail(VR_ERR_INVALID, "depth=%d unsupported (1..%d)", depth, search_bigk_max());
    if (!std::isfinite(c) || c < 0.f) return fail(VR_ERR_INVALID, "c=%g must be finite and >= 0", (double)c);
    int64_t most = 0;
    VRCHK(check_group_lims(lims, n_groups, n_lists, "group", "lists", depth, &most));
    if (weights) VRCHK(check_finite(weights, n_lists, "weights"));
    *max_entries = (int)(most * depth);
    return VR_OK;
}

// n result slots of a rank fusion over no list entry: (-inf, -1, 0)
static inline int rrf_fill_tails(float* out_scores, int64_t* out_ids, int32_t* out_hits, size_t n, int32_t on_device, hipStream_t s) {
    VRCHK(fill_tails(out_scores, out_ids, nullptr, n, on_device, s));
    if (on_device) HIPCHK(hipMemsetAsync(out_hits, 0, n * 4, s));
    else std::fill(out_hits, out_hits + n, (int32_t)0);
    return VR_OK;
}

// ---- a block of <= 256 queries on the score-row route: S[q][row] in ix->sbuf, one fp32 row per query ---------------------------
static inline bool certifies(vr_index_t ix) { return ix->eps_rel == -2.f || ix->eps_rel >= 0.f; }

// The block's view for the kernels: index, queries [q0, q0 + nb), k and the error model of the certification (search_common.h:
// query_eps) as vr_index_set_search_eps left it.  always_model: the model also defines what is re-scored (a band, the rows of
// a group) — with certification off, the default one does that.
static inline SearchArgs block_view(vr_index_t ix, const float* q32, int64_t q0, int nb, int k, bool always_model) {
    SearchArgs a{};
    a.index_bf16 = ix->bf16.p; a.index_f32 = ix->f32.as<float>(); a.n_docs = ix->n; a.dim = ix->dim;
    a.q_bf16 = ix->qbf.p; a.q_f32 = q32 + (size_t)q0 * ix->dim; a.nq = nb; a.k = k;
    a.eps_data = (ix->eps_rel == -2.f || (always_model && !certifies(ix))) ? 1 : 0;
    a.eps_rel = a.eps_data ? 0.f : ix->eps_rel;
    a.acc_rel = search_acc_rel(ix->dim);
    a.dmax = ix->cert.as<float>();
    return a;
}

// S[r][row] = bf16 rows A[0, M) x index^T on the bf16 MFMA GEMM, fp32 out (m_dev set: the row count is read on the device)
static inline int score_rows(vr_index_t ix, const void* A_bf16, int M, const int* m_dev, int m_sub, int variant, int64_t ldS, hipStream_t s) {
    GemmArgs g{};
    g.A = A_bf16; g.lda = ix->dim;
    g.W = ix->bf16.p; g.ldw = ix->dim; g.M = M; g.N = (int)pad128l(ix->n); g.K = ix->dim;
    g.out = ix->sbuf.p; g.ldo = (int)ldS; g.alpha = 1.0f;
    g.m_dev = m_dev; g.m_sub = m_sub;
    HIPCHK(launch_gemm(g, EPI_F32, variant, s));
    return VR_OK;
}

// The block's queries to bf16 (rows >= nb of the padded tile: zeros; clear_words set: those two ints cleared along, a search's
// flag counter), then their score rows: the deep path's GEMM launch
static inline int score_block(vr_index_t ix, const float* q32, int64_t q0, int nb, int64_t ldS, int* clear_words, hipStream_t s) {
    HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)q0 * ix->dim, ix->qbf.p, (size_t)nb * ix->dim, (size_t)pad256l(nb) * ix->dim, s, clear_words));
    return score_rows(ix, ix->qbf.p, nb, nullptr, 0, GEMM_VARIANT_AUTO, ldS, s);
}

// ---- filters as the searches other than the filtered one use them ---------------------------------------------------------------
// filter ids (`what`: the argument's name) before any launch: filters must be set; a host array is range-checked (a device
// array cannot be read here: an entry outside [-1, n_filters) allows nothing)
static inline int check_filter_ids(vr_index_t ix, const int32_t* ids, int32_t n, int32_t on_device, const char* what) {
    if (ix->flt.n_filters <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no filters set for the rows of the index (vr_index_set_filters)");
    if (!on_device)
        for (int32_t i = 0; i < n; ++i)
            if (ids[i] < -1 || ids[i] >= ix->flt.n_filters)
                return fail(VR_ERR_INVALID, "%s[%d] = %d outside [-1, %lld)", what, (int)i, (int)ids[i], (long long)ix->flt.n_filters);
    return VR_OK;
}

// disallowed columns of the block's score rows -> -inf: row i is masked by filter foq_block[i] (slot_count set: the first
// *slot_count - sub rows only, row i by the filter of query flag_list[sub + i])
static inline int mask_block(vr_index_t ix, const int* foq_block, int nb, int64_t ldS, const int* flag_list, const int* slot_count, int sub,
                             hipStream_t s) {
    const MaskArgs m{ix->flt.bits.as<uint32_t>(), (size_t)((ix->n + 31) / 32), (int)ix->flt.n_filters, foq_block, ix->n};
    HIPCHK(launch_filter_mask(m, ix->sbuf.as<float>(), (size_t)ldS, nb, flag_list, slot_count, sub, s));
    return VR_OK;
}

// ---- the call frame: what every score-row search sets up once its arguments are checked -----------------------------------------
struct Frame {
    hipStream_t s;
    const float* q32;                 // the call's fp32 queries on the device
    const int* foq;                   // the call's filter ids on the device, or null
    float* S; int64_t ldS;            // a block's score rows [QBLK][ldS]
    const int* goff; int ng; int64_t ldB;   // with a grouping: first rows, groups, the pitch of a block's group maxima [QBLK][ldB]
};

// queries staged, filter ids (n_ids of them, if set) staged in flt.ids, score rows reserved; B set: the grouping's view and the
// reserve of the search's own group maxima.  A nested call (on_device) stages nothing: flt.ids and the staged queries stay the outer call's.
static inline int open_frame(vr_index_t ix, const float* queries, int32_t nq, const int32_t* filter_ids, int32_t n_ids, int32_t on_device,
                             hipStream_t s, DevBuf* B, Frame* f) {
    *f = Frame{};
    f->s = s; f->ldS = pad256l(ix->n);
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, QBLK)), on_device, s, &f->q32));
    if (filter_ids) VRCHK(stage_input(ix->flt.ids, filter_ids, (size_t)n_ids, on_device, s, &f->foq));
    VRCHK(ix->sbuf.reserve((size_t)QBLK * f->ldS * 4));
    f->S = ix->sbuf.as<float>();
    if (B) {
        f->goff = ix->grp.off.as<int>(); f->ng = (int)ix->grp.n_groups; f->ldB = (ix->grp.n_groups + 63) / 64 * 64;
        VRCHK(B->reserve((size_t)QBLK * f->ldB * 4));
    }
    return VR_OK;
}

// a block's score rows of queries [q0, q0 + nb) (clear_words: as score_block's), masked row by row with mask_ids (if set), and
// with B set their group maxima
static inline int frame_block(vr_index_t ix, const Frame& f, int64_t q0, int nb, const int* mask_ids, int* clear_words, DevBuf* B) {
    VRCHK(score_block(ix, f.q32, q0, nb, f.ldS, clear_words, f.s));
    if (mask_ids) VRCHK(mask_block(ix, mask_ids, nb, f.ldS, nullptr, nullptr, 0, f.s));
    if (B) HIPCHK(launch_group_max(f.S, (size_t)f.ldS, f.goff, f.ng, B->as<float>(), (size_t)f.ldB, nb, nullptr, 0, f.s));
    return VR_OK;
}

// a search's counters, allocated (and cleared) the first time it launches
static inline int open_state(DevBuf& state, int words) { return state.p ? VR_OK : state.alloc((size_t)words * 8); }

// ---- staging of (query, target) pairs and of groups of sub-queries ----------------------------------------------------------------
// The np pairs of the rank searches, 4 bytes each: st.q = the pair's query inside its block, st.v = its target (`targets` set) or
// its threshold; bars and eps reserved.  Synchronises: the host arrays are free afterwards.
static inline int stage_pairs(RankState& st, const int64_t* lims, int32_t nq, int64_t np, const int64_t* targets, const float* thresholds,
                              hipStream_t s) {
    std::vector<int> pq((size_t)np), pv(targets ? (size_t)np : 0);
    for (int32_t q = 0; q < nq; ++q)
        for (int64_t i = lims[q]; i < lims[q + 1]; ++i) pq[(size_t)i] = (int)(q % QBLK);
    if (targets) for (int64_t i = 0; i < np; ++i) pv[(size_t)i] = (int)targets[i];
    VRCHK(st.q.reserve((size_t)np * 4));
    VRCHK(st.v.reserve((size_t)np * 4));
    VRCHK(st.bar.reserve((size_t)np * 8));
    VRCHK(st.eps.reserve((size_t)np * 4));
    HIPCHK(hipMemcpyAsync(st.q.p, pq.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(st.v.p, targets ? (const void*)pv.data() : (const void*)thresholds, (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// The groups of sub-queries of the fused searches and the rank fusion: *glims = the lims as ints in lims_buf; with filter_of_group
// its staged copy *fog (flt.ids) and *fsub = the group's filter for every one of its n_sub sub-queries, in fsub_buf: what the
// mask reads.  Synchronises: the host arrays (the caller's own staged ones too) are free afterwards.
static inline int stage_groups(vr_index_t ix, DevBuf& lims_buf, DevBuf& fsub_buf, const int64_t* lims, int32_t n_groups, int32_t n_sub,
                               const int32_t* filter_of_group, int32_t on_device, hipStream_t s, const int** glims, const int** fog,
                               const int** fsub) {
    std::vector<int> lims32((size_t)n_groups + 1);
    for (int32_t g = 0; g <= n_groups; ++g) lims32[(size_t)g] = (int)lims[g];
    VRCHK(stage_input(lims_buf, (const int*)lims32.data(), lims32.size(), 0, s, glims));
    *fog = *fsub = nullptr;
    if (filter_of_group) {
        VRCHK(stage_input(ix->flt.ids, filter_of_group, (size_t)n_groups, on_device, s, fog));
        VRCHK(fsub_buf.reserve((size_t)n_sub * 4));
        HIPCHK(launch_multi_expand(*glims, *fog, n_groups, fsub_buf.as<int>(), s));
        *fsub = fsub_buf.as<int>();
    }
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- the growing result store of the range searches: scores | rows | with `grouped` groups -----------------------------------------
// counters and the pinned word, the first time
static inline int range_store_open(RangeState& st) {
    VRCHK(open_state(st.state, RANGE_WORDS));
    if (!st.host_total && hipHostMalloc((void**)&st.host_total, 64, hipHostMallocDefault) != hipSuccess) {
        st.host_total = nullptr;
        return fail(VR_ERR_HIP, "hipHostMalloc");
    }
    return VR_OK;
}

// room for `need` entries, the first `keep` of which are kept (what earlier blocks of the call packed)
static inline int range_store_reserve(RangeState& st, bool grouped, int64_t need, int64_t keep, int64_t max_total, hipStream_t s) {
    DevBuf* const arr[3] = {&st.scores, &st.rows, &st.groups};
    const size_t width[3] = {4, 8, 8};
    const int na = grouped ? 3 : 2;
    bool have = need <= st.cap;
    for (int i = 0; i < na; ++i) have = have && arr[i]->p;
    if (have) return VR_OK;
    const int64_t cap = std::max<int64_t>(std::min(max_total, std::max(need, 2 * st.cap)), std::max<int64_t>(need, 1));
    DevBuf grown[3];
    for (int i = 0; i < na; ++i) VRCHK(grown[i].reserve((size_t)cap * width[i]));
    if (keep > 0) {
        for (int i = 0; i < na; ++i) HIPCHK(hipMemcpyAsync(grown[i].p, arr[i]->p, (size_t)keep * width[i], hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    for (int i = 0; i < na; ++i) *arr[i] = std::move(grown[i]);
    st.cap = cap;
    return VR_OK;
}

// *bt = the block's total (the scan left it in the state's word) as the host reads it: one copy, one synchronisation
static inline int range_store_block_total(RangeState& st, hipStream_t s, int64_t* bt) {
    HIPCHK(hipMemcpyAsync(st.host_total, st.state.as<int64_t>() + RANGE_TOTAL, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *bt = *st.host_total;
    return VR_OK;
}

// the first n entries of the stored result (`noun`: "range" / "document range", `fn`: the search that makes it)
static inline int range_store_results(vr_index_t ix, RangeState& st, bool grouped, float* out_scores, int64_t* out_rows, int64_t* out_groups,
                                      int64_t n, int32_t on_device, void* stream) {
    const char* noun = grouped ? "document range" : "range";
    if (st.total < 0) return fail(VR_ERR_STATE, "no %s result (%s)", noun, grouped ? "vr_index_search_groups_range" : "vr_index_search_range");
    if (n > st.total) return fail(VR_ERR_STATE, "%lld entries asked for, the last %s search found %lld", (long long)n, noun, (long long)st.total);
    if (n == 0) return VR_OK;
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(out_scores, st.scores.p, (size_t)n * 4, kind, s));
    HIPCHK(hipMemcpyAsync(out_rows, st.rows.p, (size_t)n * 8, kind, s));
    if (grouped) HIPCHK(hipMemcpyAsync(out_groups, st.groups.p, (size_t)n * 8, kind, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- counters ---------------------------------------------------------------------------------------------------------------------
// out[0, N) = words [first_word, first_word + N) of a search's state buffer (W: their width), then cleared with `reset`; a
// buffer that was never allocated counted nothing: zeros, no device call
template <typename W, int N>
static inline int read_counters(vr_index_t ix, const DevBuf& state, int first_word, int64_t* out, int32_t reset) {
    std::fill(out, out + N, (int64_t)0);
    if (!state.p) return VR_OK;
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    W w[N];
    HIPCHK(hipMemcpy(w, state.as<W>() + first_word, sizeof(w), hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i) out[i] = (int64_t)w[i];
    if (reset) HIPCHK(hipMemset(state.as<W>() + first_word, 0, sizeof(w)));
    return VR_OK;
}
