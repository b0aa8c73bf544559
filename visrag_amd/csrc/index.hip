// The search index of libvisrag_hip.so (vr_index_* / vr_topk_merge* of include/visrag_hip.h): fp32 + bf16 row store,
// the certified top-k search over it and its fallback passes (search*.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "engine_common.h"

constexpr int GRP_STATS = 2, GRP_LIST = 8, GRP_WORDS = GRP_LIST + 256;
constexpr int FLT_STATS = 2, FLT_LIST = 8, FLT_WORDS = FLT_LIST + 256;
constexpr int CERT_WORDS = 32, CERT_FLAG = 2, CERT_FLAG2 = 3, CERT_STATS = 4, CERT_NSTATS = 6;   // (the two flag counters are consecutive: cleared together)
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
    // grouped search (vr_index_search_groups, search_group.hip): state of its own — the plain searches read none of it
    int64_t n_groups = 0;             // 0: no grouping set (vr_index_add / vr_index_reset drop it)
    DevBuf goff, gB, og, gstate;      // int first rows [n_groups + 1] | group maxima [256][ldB] | staged out_groups |
                                      // int words: [0] flag count, [1] unused (cleared with it), u32 [2..4] the three counters of
                                      // vr_index_group_search_stats, [GRP_LIST..] flag list of a block of <= 256 queries
    // filtered search (vr_index_search_filtered, search_filter.hip): state of its own, independent of the grouping
    int64_t n_filters = 0;            // 0: no filters set (vr_index_add / vr_index_reset drop them)
    DevBuf fbits, fcount, ffq, fstate;   // u32 [n_filters][ceil(n / 32)] the library's copy | int allowed rows [n_filters] | staged
                                      // filter_of_query of a host caller | int words laid out as gstate's: [0] flag count, [1] unused,
                                      // u32 [2..4] the counters of vr_index_filter_search_stats, [FLT_LIST..] flag list of a block
    // diversified search (vr_index_search_diverse, search_diverse.hip): its pool — the result of the plain or the filtered search for
    // k = pool — in buffers of its own, because that very search overwrites the shared scratch
    DevBuf dps, dpi;                  // f32 pool scores [nq][pool] | int64 pool ids [nq][pool]
    // range search (vr_index_search_range, search_range.hip): its result and state of its own — no other search reads any of it
    DevBuf rs, ri;                    // the result: f32 scores [rcap] | int64 row ids [rcap], valid entries [0, range_total)
    int64_t rcap = 0, range_total = -1;   // -1: no result (none yet, vr_index_reset, or the last range search failed)
    DevBuf rthr, rlims, rcnt, roff, rstate;   // staged thresholds / lims of a host caller | int rows kept [256][slots] | int their
                                      // exclusive scan per query | u64 words: [0..2] the counters of vr_index_range_search_stats, [3] a block's
                                      // total, [4..] never written: the flag words launch_filter_mask's argument check wants to see
    int64_t* range_host = nullptr;    // pinned host word: the block total as the host reads it
    // rank search (vr_index_rank_rows / vr_index_count_range, search_rank.hip): scratch and counters of its own, no stored result
    DevBuf kq, kv, kbar, keps, kstate;   // int query of every pair | int target rows or f32 thresholds | u64 bars | f32 eps per pair | u64
                                      // words: [0..2] the counters of vr_index_rank_search_stats, [4..] never written (as rstate's)
    // windowed search (vr_index_search_window, search_window.hip): scratch and counters of its own, no stored result
    DevBuf woff, wedge, wstate;       // int64 offsets of the call's queries | f32 band edges {lo, hi} of a block's queries | u64 words:
                                      // [0..2] the counters of vr_index_window_search_stats, [4..] never written (as rstate's)
    // fused search (vr_index_search_multi, search_multi.hip): scratch and counters of its own, no stored result
    DevBuf mlims, mfsub, medge, mwhich, mstate;   // int lims of the call's groups | int filter of every sub-query | f32 band edge of a
                                      // block's groups | staged out_which | u64 words: [0..2] the counters of vr_index_multi_search_stats,
                                      // [4..] never written (as rstate's)
    // editing in place (vr_index_remove / vr_index_update / vr_index_get_rows, index_edit.hip)
    DevBuf eids, erows, fbits2;       // int row ids of the call | rows of a host caller, staged (<= EDIT_SCRATCH bytes for get_rows) |
                                      // the filters compacted out of place: swapped with fbits
    // per-stage HIP events (vr_index_set_search_profile): convert | thresholds | sweep | merge | exact pass
    bool prof_on = false;
    hipEvent_t prof_ev[SEARCH_PROF_EVENTS] = {};
    double prof_ms[SEARCH_PROF_EVENTS - 1] = {};
    int64_t prof_calls = 0;
};

extern "C" int vr_index_create(int device_id, int32_t dim, int64_t capacity, vr_index_t* out) {
    if (!out || dim <= 0 || capacity <= 0) return fail(VR_ERR_INVALID, "bad index arguments");
    if (dim % 64 || dim > 2560) return fail(VR_ERR_INVALID, "dim %d must be a multiple of 64 and <= 2560", dim);
    if (capacity >= ((int64_t)1 << 31) - 256) return fail(VR_ERR_INVALID, "capacity too large for 32-bit row ids");
    VRCHK(set_dev(device_id));
    vr_index_s* ix = new vr_index_s();
    ix->device = device_id; ix->dim = dim; ix->cap = capacity;
    const int64_t cp = pad256l(capacity);
    int r = ix->f32.alloc((size_t)cp * dim * 4);
    if (r == VR_OK) r = ix->bf16.alloc((size_t)cp * dim * 2);
    if (r == VR_OK) r = ix->cert.alloc(CERT_WORDS * 4);
    if (r == VR_OK && hipHostMalloc((void**)&ix->huge_seen, 64, hipHostMallocDefault) != hipSuccess) r = fail(VR_ERR_HIP, "hipHostMalloc");
    if (r != VR_OK) { ix->f32.free(); ix->bf16.free(); ix->cert.free(); delete ix; return r; }
    *ix->huge_seen = 0;
    *out = ix;
    return VR_OK;
}

extern "C" int vr_index_destroy(vr_index_t ix) {
    if (!ix) return VR_OK;
    (void)hipSetDevice(ix->device);
    (void)hipDeviceSynchronize();
    for (DevBuf* b : {&ix->f32, &ix->bf16, &ix->q32, &ix->qbf, &ix->cs, &ix->ci, &ix->ck, &ix->os, &ix->oi, &ix->ok, &ix->thr,
                      &ix->sbuf, &ix->cert, &ix->flags, &ix->flagq, &ix->goff, &ix->gB, &ix->og, &ix->gstate,
                      &ix->fbits, &ix->fcount, &ix->ffq, &ix->fstate, &ix->dps, &ix->dpi, &ix->rs, &ix->ri, &ix->rthr, &ix->rlims,
                      &ix->rcnt, &ix->roff, &ix->rstate, &ix->kq, &ix->kv, &ix->kbar, &ix->keps, &ix->kstate, &ix->woff, &ix->wedge, &ix->wstate,
                      &ix->mlims, &ix->mfsub, &ix->medge, &ix->mwhich, &ix->mstate,
                      &ix->eids, &ix->erows, &ix->fbits2})
        b->free();
    if (ix->range_host) (void)hipHostFree(ix->range_host);
    for (hipEvent_t e : ix->prof_ev) if (e) (void)hipEventDestroy(e);
    if (ix->huge_seen) (void)hipHostFree(ix->huge_seen);
    delete ix;
    return VR_OK;
}

extern "C" int vr_index_reset(vr_index_t ix) {
    if (!ix) return fail(VR_ERR_INVALID, "NULL index");
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(ix->cert.p, 0, 8));          // largest row norm, largest rounding residual
    ix->n = 0;
    ix->n_groups = 0;
    ix->n_filters = 0;
    ix->range_total = -1;
    if (ix->huge_seen) *ix->huge_seen = 0;
    return VR_OK;
}

extern "C" int vr_index_size(vr_index_t ix, int64_t* n) {
    if (!ix || !n) return fail(VR_ERR_INVALID, "NULL argument");
    *n = ix->n;
    return VR_OK;
}

extern "C" int vr_index_add(vr_index_t ix, const float* reps, int64_t n, int32_t on_device, void* stream) {
    if (!ix || (!reps && n > 0) || n < 0) return fail(VR_ERR_INVALID, "bad arguments");
    if (n == 0) return VR_OK;
    if (ix->n + n > ix->cap) return fail(VR_ERR_CAPACITY, "index capacity %lld exceeded", (long long)ix->cap);
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    float* dst = ix->f32.as<float>() + (size_t)ix->n * ix->dim;
    HIPCHK(hipMemcpyAsync(dst, reps, (size_t)n * ix->dim * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIPCHK(launch_f32_to_bf16(dst, (char*)ix->bf16.p + (size_t)ix->n * ix->dim * 2, (size_t)n * ix->dim, s));
    HIPCHK(launch_row_norm_max(dst, n, ix->dim, ix->cert.as<float>(), s));      // max |d|, max |d - bf16(d)|: the search's error bound
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    ix->n += n;
    ix->n_groups = 0;                 // the grouping described the rows that were there
    ix->n_filters = 0;                // ... and so did the filters
    return VR_OK;
}

extern "C" int vr_index_set_search_eps(vr_index_t ix, float eps_rel) {
    if (!ix) return fail(VR_ERR_INVALID, "NULL index");
    if (eps_rel != eps_rel) ix->eps_rel = -2.f;    // NaN: back to the default bound
    else ix->eps_rel = eps_rel < 0.f ? -1.f : eps_rel;
    return VR_OK;
}

extern "C" int vr_index_search_stats(vr_index_t ix, int64_t* out6, int32_t reset) {     // out6: SIX words, see the header
    if (!ix || !out6) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned w[CERT_NSTATS];
    HIPCHK(hipMemcpy(w, ix->cert.as<unsigned>() + CERT_STATS, CERT_NSTATS * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < CERT_NSTATS; ++i) out6[i] = w[i];
    if (reset) HIPCHK(hipMemset(ix->cert.as<unsigned>() + CERT_STATS, 0, CERT_NSTATS * 4));
    return VR_OK;
}

// The list chunks of one search pass over `nq` queries (the fused path, k <= 26): the streaming kernel of a handful of
// queries has its own fixed count; otherwise the threshold pre-pass may own its 16 sampled tiles — scored once, its survivors
// in `own` list chunks of their own behind the sweep's — and the sweep walks the rest in `sweep` chunks (search.hip).
struct SearchPlan { bool stream; int own, sweep, n_chunks, tiles_per_chunk; };
static SearchPlan search_plan(int64_t n_docs, int nq, int dim) {
    SearchPlan p{};
    p.stream = search_uses_stream(nq, dim);
    p.own = p.stream ? 0 : search_prepass_owned(n_docs, nq, dim);
    p.sweep = p.stream ? search_stream_chunks() : search_num_chunks(n_docs - (p.own ? (int64_t)SEARCH_PRE_SPOTS * 256 : 0), nq);
    p.n_chunks = p.sweep + p.own;
    const int64_t tile = search_uses_256(nq) ? 256 : 128;
    const int64_t tiles = (n_docs + tile - 1) / tile - (p.own ? SEARCH_PRE_SPOTS : 0);
    p.tiles_per_chunk = p.stream ? 0 : (int)((tiles + p.sweep - 1) / p.sweep);
    return p;
}

extern "C" int vr_index_search_plan(vr_index_t ix, int32_t nq, int32_t* out5) {
    if (!ix || !out5 || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    const SearchPlan p = search_plan(ix->n, nq, ix->dim);
    out5[0] = p.n_chunks; out5[1] = p.own; out5[2] = p.sweep; out5[3] = p.tiles_per_chunk;
    out5[4] = (ix->huge_seen && __atomic_load_n(ix->huge_seen, __ATOMIC_RELAXED) != 0) ? 1 : 0;
    return VR_OK;
}

extern "C" int vr_index_error_model(vr_index_t ix, float* out4) {
    if (!ix || !out4) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out4, ix->cert.p, 8, hipMemcpyDeviceToHost));
    out4[2] = search_acc_rel(ix->dim);
    out4[3] = search_default_eps_rel(ix->dim);
    return VR_OK;
}

extern "C" int vr_index_set_search_profile(vr_index_t ix, int32_t enable) {
    if (!ix) return fail(VR_ERR_INVALID, "NULL index");
    VRCHK(set_dev(ix->device));
    if (enable)
        for (hipEvent_t& e : ix->prof_ev) if (!e) HIPCHK(hipEventCreate(&e));
    ix->prof_on = enable != 0;
    for (double& m : ix->prof_ms) m = 0;
    ix->prof_calls = 0;
    return VR_OK;
}

extern "C" int vr_index_get_search_profile(vr_index_t ix, double* ms5, int64_t* calls) {
    if (!ix || !ms5 || !calls) return fail(VR_ERR_INVALID, "NULL argument");
    for (int i = 0; i < SEARCH_PROF_EVENTS - 1; ++i) ms5[i] = ix->prof_ms[i];
    *calls = ix->prof_calls;
    return VR_OK;
}

// ---- what vr_index_search* and vr_index_search_groups share -----------------------------------------------------------------
// Query staging for passes of up to `nqp` (padded) queries: capacity of the bf16 rows and thresholds, host queries to the
// device.  *q32: the fp32 queries on the device.
static int stage_queries(vr_index_t ix, const float* queries, int32_t nq, int64_t nqp, int32_t on_device, hipStream_t s,
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

// One output array of n elements: the kernels write *dev — the caller's own array, or for a host caller the staging buffer
// that return_output copies back (the caller synchronises the stream after the last one)
template <typename T>
static int stage_output(DevBuf& buf, T* out, size_t n, int32_t on_device, T** dev) {
    *dev = out;
    if (!on_device) { VRCHK(buf.reserve(n * sizeof(T))); *dev = buf.as<T>(); }
    return VR_OK;
}
template <typename T>
static int return_output(T* out, const T* dev, size_t n, int32_t on_device, hipStream_t s) {
    if (!on_device) HIPCHK(hipMemcpyAsync(out, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
    return VR_OK;
}

// S[r][row] = bf16 rows A[0, M) x index^T on the bf16 MFMA GEMM, fp32 out (m_dev set: the row count is read on the device)
static int score_rows(vr_index_t ix, const void* A_bf16, int M, const int* m_dev, int m_sub, int variant, int64_t ldS, hipStream_t s) {
    GemmArgs g{};
    g.A = A_bf16; g.lda = ix->dim;
    g.W = ix->bf16.p; g.ldw = ix->dim; g.M = M; g.N = (int)pad128l(ix->n); g.K = ix->dim;
    g.out = ix->sbuf.p; g.ldo = (int)ldS; g.alpha = 1.0f;
    g.m_dev = m_dev; g.m_sub = m_sub;
    HIPCHK(launch_gemm(g, EPI_F32, variant, s));
    return VR_OK;
}

// the error model of the certification (search_common.h: query_eps) as vr_index_set_search_eps left it
static void fill_error_model(vr_index_t ix, SearchArgs& a) {
    a.eps_data = ix->eps_rel == -2.f ? 1 : 0;
    a.eps_rel = a.eps_data ? 0.f : ix->eps_rel;
    a.acc_rel = search_acc_rel(ix->dim);
    a.dmax = ix->cert.as<float>();
}

// entries [f0, f0 + ns) of a's flag list through the exact fp32 pass: score rows over the whole index, plain top-k of each
static int exact_pass(vr_index_t ix, const SearchArgs& a, int f0, int ns, int64_t ldS, hipStream_t s) {
    HIPCHK(launch_exact_scores(a.index_f32, a.n_docs, a.dim, a.q_f32, a.flag_list, a.flag_count, f0, ns, ix->sbuf.as<float>(),
                               (size_t)ldS, s));
    HIPCHK(launch_exact_select(a, ix->sbuf.as<float>(), (size_t)ldS, f0, ns, s));
    return VR_OK;
}

// queries [nq][dim] -> top k per query, as (scores, ids) or as packed keys with `id_offset` added to the row ids
static int search_impl(vr_index_t ix, const float* queries, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids,
                       unsigned long long* out_keys, int64_t id_offset, int32_t on_device, void* stream) {
    const bool keys_out = out_keys != nullptr;
    if (!ix || !queries || nq <= 0 || (!keys_out && (!out_scores || !out_ids))) return fail(VR_ERR_INVALID, "bad arguments");
    const bool bigk = k > 26;             // deep retrieval: GEMM + radix select (search_bigk.hip)
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (keys_out && (id_offset < 0 || id_offset + ix->n >= ((int64_t)1 << 32) - 1))
        return fail(VR_ERR_INVALID, "id_offset %lld + %lld rows do not fit 32-bit global ids", (long long)id_offset, (long long)ix->n);
    const int kp = bigk ? 0 : search_kprime(k);
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const int dim = ix->dim;
    const int64_t ldS = pad256l(std::max<int64_t>(ix->n, 1));
    // queries per pass: the deep path's GEMM writes one fp32 score row per query; the fused path's candidate scratch grows
    // with the pass (128 KiB of half-lists per query at 100k rows)
    int64_t qblk = bigk ? 256 : 4096;
    const int64_t nqp = pad256l(std::min<int64_t>(nq, qblk));
    // score rows of the fallback passes (band pass / exact pass over the FLAGGED queries, search_band.hip): a bounded buffer
    // — at most 512 MiB of fp32 score rows (never fewer than 16 rows) — walked in passes of `slots` flagged queries
    const int64_t slots = bigk ? 256 : std::min<int64_t>(nqp, std::max<int64_t>(16, (((int64_t)1 << 27) / ldS) / 16 * 16));
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, nqp, on_device, s, &q32));
    const size_t n_out = (size_t)nq * k;
    float* os = nullptr; int64_t* oi = nullptr; unsigned long long* ok = nullptr;
    if (keys_out) VRCHK(stage_output(ix->ok, out_keys, n_out, on_device, &ok));
    else {
        VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
        VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    }
    if (ix->n == 0) {
        if (keys_out) HIPCHK(hipMemsetAsync(ok, 0, (size_t)nq * k * 8, s));
        else {
            std::vector<float> sc((size_t)nq * k, -INFINITY);
            std::vector<int64_t> id((size_t)nq * k, -1);
            HIPCHK(hipMemcpyAsync(os, sc.data(), sc.size() * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(oi, id.data(), id.size() * 8, hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    } else {
        if (ix->fcap < nqp) {
            VRCHK(ix->flags.alloc((size_t)nqp * 12));
            VRCHK(ix->flagq.alloc((size_t)(nqp + 256) * dim * 2));     // (+ one tile: the GEMM's last row tile may start anywhere)
            ix->fcap = nqp;
        }
        VRCHK(ix->sbuf.reserve((size_t)slots * ldS * 4));
        for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
            const int nb = (int)std::min<int64_t>(qblk, nq - q0);
            const int64_t nbp = pad256l(nb);
            const bool prof = ix->prof_on && !bigk;
            if (prof) HIPCHK(hipEventRecord(ix->prof_ev[0], s));
            // rows >= nb: zeros; also clears the flag counters.  A handful of queries (streaming kernel): converted inside it.
            const bool conv_in_kernel = !bigk && search_uses_stream(nb, dim);
            if (!conv_in_kernel)
                HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)q0 * dim, ix->qbf.p, (size_t)nb * dim, (size_t)nbp * dim, s,
                                              ix->cert.as<int>() + CERT_FLAG));   // (clears both flag counters)
            if (prof) HIPCHK(hipEventRecord(ix->prof_ev[1], s));
            SearchArgs a{};
            a.index_bf16 = ix->bf16.p; a.index_f32 = ix->f32.as<float>(); a.n_docs = ix->n; a.dim = dim;
            a.q_bf16 = ix->qbf.p; a.q_f32 = q32 + (size_t)q0 * dim; a.nq = nb; a.k = k;
            a.convert_q = conv_in_kernel ? 1 : 0;
            // (a handful of queries: the streaming sweep leaves every bf16 score behind — a query its merge cannot certify is
            // redone by that merge workgroup itself, and none of the fallback launches below is issued)
            if (conv_in_kernel) { a.score_rows = ix->sbuf.as<float>(); a.ld_scores = (size_t)ldS; }
            // (... unless the band is beyond search_band_max() rows: the first such query is walked by its one workgroup and sets
            // the host-visible word; from then on the exact pass is launched behind this index's streaming searches)
            const bool huge_seen = ix->huge_seen && __atomic_load_n(ix->huge_seen, __ATOMIC_RELAXED) != 0;
            const bool exact_small = conv_in_kernel && huge_seen;
            // (the sweeps behind a pre-pass likewise: band_select_kernel walks the first band beyond search_band_max() rows itself;
            // deep retrieval, k > 26, keeps the exact pass — its select handles any k)
            const bool exact_big = !conv_in_kernel && (bigk || huge_seen || !ix->huge_seen);
            a.exact_follows = (exact_small || exact_big) ? 1 : 0;
            a.huge_seen = ix->huge_seen;
            fill_error_model(ix, a);
            a.flag_count = ix->cert.as<int>() + CERT_FLAG; a.flag_list = ix->flags.as<int>();
            a.flag2_count = ix->cert.as<int>() + CERT_FLAG2; a.flag2_list = ix->flags.as<int>() + ix->fcap;
            a.flag_tau = ix->flags.as<float>() + 2 * ix->fcap; a.flag_q = ix->flagq.p;
            a.stats = ix->cert.as<unsigned>() + CERT_STATS;
            if (keys_out) { a.out_keys = ok + (size_t)q0 * k; a.id_offset = id_offset; }
            else { a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k; }
            a.prof_ev = prof ? ix->prof_ev : nullptr;
            if (bigk) {
                // score rows of <= 256 queries at a time: S[q][doc] = queries x index^T on the bf16 MFMA GEMM
                VRCHK(score_rows(ix, ix->qbf.p, nb, nullptr, 0, GEMM_VARIANT_AUTO, ldS, s));
                HIPCHK(launch_search_bigk(a, ix->sbuf.as<float>(), (size_t)ldS, nb, s));
            } else {
                const SearchPlan plan = search_plan(ix->n, nb, dim);
                a.pre_own_chunks = plan.own;
                a.n_chunks = plan.n_chunks;
                a.thr_init = ix->thr.as<float>();
                a.thr_cert = ix->thr.as<float>() + ix->qcap;
                const int64_t need = std::max<int64_t>(nbp * a.n_chunks * kp, nbp * search_prepass_floats());
                if (ix->ccap < need) {
                    VRCHK(ix->cs.alloc((size_t)need * 4));
                    VRCHK(ix->ci.alloc((size_t)need * 4));
                    ix->ccap = need;
                }
                a.cand_scores = ix->cs.as<float>(); a.cand_ids = ix->ci.as<int>();
                if (search_uses_256(nb)) {
                    const int64_t kneed = nbp * a.n_chunks * 128;      // [q][chunk][2 halves][64]
                    if (ix->kcap < kneed) { VRCHK(ix->ck.alloc((size_t)kneed * 8)); ix->kcap = kneed; }
                    a.cand_keys = ix->ck.as<unsigned long long>();
                }
                HIPCHK(launch_search(a, s));
            }
            if (prof) HIPCHK(hipEventRecord(ix->prof_ev[4], s));
            if ((a.eps_data || a.eps_rel >= 0.f) && !a.score_rows) {
                // whatever the merge flagged (nothing, normally: every kernel below leaves at once), `slots` queries per pass:
                // bf16 score rows of the flagged queries (GEMM over their compacted bf16 rows, row count on the device) ->
                // every row inside a query's error band re-scored in fp32 (search_band.hip) -> what is left (bands beyond
                // search_band_max() rows) through the exact fp32 pass over the whole index (search_exact.hip)
                for (int64_t f0 = 0; f0 < nb; f0 += slots) {
                    const int ns = (int)std::min<int64_t>(slots, nb - f0);
                    VRCHK(score_rows(ix, (const char*)ix->flagq.p + (size_t)f0 * dim * 2, ns, a.flag_count, (int)f0, GEMM_VARIANT_256IL, ldS, s));
                    HIPCHK(launch_band_select(a, ix->sbuf.as<float>(), (size_t)ldS, (int)f0, ns, s));
                }
                SearchArgs ax = a;
                ax.flag_count = a.flag2_count; ax.flag_list = a.flag2_list;
                for (int64_t f0 = 0; exact_big && f0 < nb; f0 += slots) {
                    const int ns = (int)std::min<int64_t>(slots, nb - f0);
                    VRCHK(exact_pass(ix, ax, (int)f0, ns, ldS, s));
                }
            }
            if ((a.eps_data || a.eps_rel >= 0.f) && a.score_rows && exact_small) {
                SearchArgs ax = a;
                ax.flag_count = a.flag2_count; ax.flag_list = a.flag2_list;
                VRCHK(exact_pass(ix, ax, 0, nb, ldS, s));
            }
            if (prof) {
                HIPCHK(hipEventRecord(ix->prof_ev[5], s));
                HIPCHK(hipEventSynchronize(ix->prof_ev[5]));
                for (int i = 0; i + 1 < SEARCH_PROF_EVENTS; ++i) {
                    float ms = 0.f;
                    HIPCHK(hipEventElapsedTime(&ms, ix->prof_ev[i], ix->prof_ev[i + 1]));
                    ix->prof_ms[i] += ms;
                }
                ix->prof_calls += 1;
            }
        }
    }
    if (keys_out) VRCHK(return_output(out_keys, ok, n_out, on_device, s));
    else {
        VRCHK(return_output(out_scores, os, n_out, on_device, s));
        VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    }
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_index_search(vr_index_t ix, const float* queries, int32_t nq, int32_t k, float* out_scores,
                               int64_t* out_ids, int32_t on_device, void* stream) {
    return search_impl(ix, queries, nq, k, out_scores, out_ids, nullptr, 0, on_device, stream);
}

extern "C" int vr_index_search_keys(vr_index_t ix, const float* queries, int32_t nq, int32_t k, int64_t id_offset,
                                    uint64_t* out_keys, int32_t on_device, void* stream) {
    if (!out_keys) return fail(VR_ERR_INVALID, "out_keys is NULL");
    return search_impl(ix, queries, nq, k, nullptr, nullptr, (unsigned long long*)out_keys, id_offset, on_device, stream);
}

extern "C" int vr_index_set_groups(vr_index_t ix, const int64_t* group_offsets, int64_t n_groups) {
    if (!ix || !group_offsets) return fail(VR_ERR_INVALID, "NULL argument");
    if (n_groups < 1 || n_groups > ix->n) return fail(VR_ERR_INVALID, "%lld groups over %lld rows", (long long)n_groups, (long long)ix->n);
    if (group_offsets[0] != 0) return fail(VR_ERR_INVALID, "group_offsets[0] must be 0");
    for (int64_t g = 0; g < n_groups; ++g)
        if (group_offsets[g + 1] <= group_offsets[g]) return fail(VR_ERR_INVALID, "group_offsets must be strictly increasing (entry %lld)", (long long)(g + 1));
    if (group_offsets[n_groups] != ix->n)
        return fail(VR_ERR_INVALID, "last group offset %lld is not the row count %lld", (long long)group_offsets[n_groups], (long long)ix->n);
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());               // (a grouped search in flight reads the offsets)
    ix->n_groups = 0;
    std::vector<int> off((size_t)n_groups + 1);   // rows are 32-bit (vr_index_create)
    for (int64_t g = 0; g <= n_groups; ++g) off[(size_t)g] = (int)group_offsets[g];
    VRCHK(ix->goff.reserve(off.size() * 4));
    HIPCHK(hipMemcpy(ix->goff.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (!ix->gstate.p) VRCHK(ix->gstate.alloc(GRP_WORDS * 4));
    ix->n_groups = n_groups;
    return VR_OK;
}

extern "C" int vr_index_group_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    out3[0] = out3[1] = out3[2] = 0;
    if (!ix->gstate.p) return VR_OK;              // no grouping was ever set: nothing counted
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned w[3];
    HIPCHK(hipMemcpy(w, ix->gstate.as<unsigned>() + GRP_STATS, sizeof(w), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) out3[i] = w[i];
    if (reset) HIPCHK(hipMemset(ix->gstate.as<unsigned>() + GRP_STATS, 0, sizeof(w)));
    return VR_OK;
}

// The k best groups per query (search_group.hip).  Scratch (query staging, score rows, staged outputs) is shared with the plain
// searches; flag list, counters and group maxima are the grouped search's own.
extern "C" int vr_index_search_groups(vr_index_t ix, const float* queries, int32_t nq, int32_t k, float* out_scores,
                                      int64_t* out_ids, int64_t* out_groups, int32_t on_device, void* stream) {
    if (!ix || !queries || !out_scores || !out_ids || !out_groups || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_groups_kmax() || k > search_bigk_max())
        return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, std::min(search_groups_kmax(), search_bigk_max()));
    if (ix->n_groups <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no grouping set for the rows of the index (vr_index_set_groups)");
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const int dim = ix->dim, ng = (int)ix->n_groups;
    const int64_t ldS = pad256l(ix->n), ldB = (ix->n_groups + 63) / 64 * 64;
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const int64_t nqp = pad256l(std::min<int64_t>(nq, qblk));
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, nqp, on_device, s, &q32));
    const size_t n_out = (size_t)nq * k;
    float* os = nullptr; int64_t* oi = nullptr; int64_t* og = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(stage_output(ix->og, out_groups, n_out, on_device, &og));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    VRCHK(ix->gB.reserve((size_t)qblk * ldB * 4));
    const bool certify = ix->eps_rel == -2.f || ix->eps_rel >= 0.f;
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        const int64_t nbp = pad256l(nb);
        // rows >= nb: zeros; also clears the grouped search's flag counter
        HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)q0 * dim, ix->qbf.p, (size_t)nb * dim, (size_t)nbp * dim, s, ix->gstate.as<int>()));
        GroupSearchArgs p{};
        SearchArgs& a = p.a;
        a.index_bf16 = ix->bf16.p; a.index_f32 = ix->f32.as<float>(); a.n_docs = ix->n; a.dim = dim;
        a.q_bf16 = ix->qbf.p; a.q_f32 = q32 + (size_t)q0 * dim; a.nq = nb; a.k = k;
        // the error model also bounds which rows of a group are re-scored: with certification off, the default one does that
        fill_error_model(ix, a);
        if (!certify) { a.eps_data = 1; a.eps_rel = 0.f; }
        a.flag_count = ix->gstate.as<int>(); a.flag_list = ix->gstate.as<int>() + GRP_LIST;
        a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k;
        p.goff = ix->goff.as<int>(); p.n_groups = ng;
        p.B = ix->gB.as<float>(); p.ldB = (size_t)ldB;
        p.out_groups = og + (size_t)q0 * k;
        p.stats = ix->gstate.as<unsigned>() + GRP_STATS;
        p.certify = certify ? 1 : 0;
        // S[q][row] = queries x index^T on the bf16 MFMA GEMM, the deep path's launch
        VRCHK(score_rows(ix, ix->qbf.p, nb, nullptr, 0, GEMM_VARIANT_AUTO, ldS, s));
        HIPCHK(launch_group_max(ix->sbuf.as<float>(), (size_t)ldS, p.goff, ng, p.B, p.ldB, nb, nullptr, 0, s));
        HIPCHK(launch_group_select(p, ix->sbuf.as<float>(), (size_t)ldS, nb, s));
        if (certify) {
            // whatever the select flagged (nothing, normally: the three kernels leave at once): exact fp32 score rows
            HIPCHK(launch_exact_scores(a.index_f32, a.n_docs, dim, a.q_f32, a.flag_list, a.flag_count, 0, nb, ix->sbuf.as<float>(), (size_t)ldS, s));
            HIPCHK(launch_group_max(ix->sbuf.as<float>(), (size_t)ldS, p.goff, ng, p.B, p.ldB, nb, a.flag_count, 0, s));
            HIPCHK(launch_group_select_exact(p, ix->sbuf.as<float>(), (size_t)ldS, 0, nb, s));
        }
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    VRCHK(return_output(out_groups, og, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_index_set_filters(vr_index_t ix, const uint32_t* bits, int32_t n_filters, int32_t on_device, void* stream) {
    if (!ix || !bits) return fail(VR_ERR_INVALID, "NULL argument");
    if (n_filters < 1) return fail(VR_ERR_INVALID, "%d filters", (int)n_filters);
    if (ix->n <= 0) return fail(VR_ERR_INVALID, "filters over an empty index");
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());               // (a filtered search in flight reads the filters)
    hipStream_t s = (hipStream_t)stream;
    const size_t words = (size_t)((ix->n + 31) / 32), total = words * (size_t)n_filters;
    ix->n_filters = 0;
    VRCHK(ix->fbits.reserve(total * 4));
    VRCHK(ix->fcount.reserve((size_t)n_filters * 4));
    if (!ix->fstate.p) VRCHK(ix->fstate.alloc(FLT_WORDS * 4));
    HIPCHK(hipMemcpyAsync(ix->fbits.p, bits, total * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    // the caller's bits at or beyond the row count are garbage: cleared in the copy; allowed rows per filter counted once, here
    HIPCHK(launch_filter_prepare(ix->fbits.as<uint32_t>(), words, n_filters, ix->n, ix->fcount.as<int>(), s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    ix->n_filters = n_filters;
    return VR_OK;
}

extern "C" int vr_index_filter_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    out3[0] = out3[1] = out3[2] = 0;
    if (!ix->fstate.p) return VR_OK;              // no filters were ever set: nothing counted
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned w[3];
    HIPCHK(hipMemcpy(w, ix->fstate.as<unsigned>() + FLT_STATS, sizeof(w), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) out3[i] = w[i];
    if (reset) HIPCHK(hipMemset(ix->fstate.as<unsigned>() + FLT_STATS, 0, sizeof(w)));
    return VR_OK;
}

// The k best rows per query among the rows its filter allows (search_filter.hip).  Scratch (query staging, score rows, staged
// outputs) is shared with the other searches; filters, flag list and counters are the filtered search's own.
extern "C" int vr_index_search_filtered(vr_index_t ix, const float* queries, int32_t nq, int32_t k, const int32_t* filter_of_query,
                                        float* out_scores, int64_t* out_ids, int32_t on_device, void* stream) {
    if (!ix || !queries || !filter_of_query || !out_scores || !out_ids || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (ix->n_filters <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no filters set for the rows of the index (vr_index_set_filters)");
    if (!on_device)
        for (int32_t q = 0; q < nq; ++q)
            if (filter_of_query[q] < -1 || filter_of_query[q] >= ix->n_filters)
                return fail(VR_ERR_INVALID, "filter_of_query[%d] = %d outside [-1, %lld)", (int)q, (int)filter_of_query[q], (long long)ix->n_filters);
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const int dim = ix->dim;
    const int64_t ldS = pad256l(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const int64_t nqp = pad256l(std::min<int64_t>(nq, qblk));
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, nqp, on_device, s, &q32));
    const int* foq = filter_of_query;
    if (!on_device) {
        VRCHK(ix->ffq.reserve((size_t)nq * 4));
        HIPCHK(hipMemcpyAsync(ix->ffq.p, filter_of_query, (size_t)nq * 4, hipMemcpyHostToDevice, s));
        foq = ix->ffq.as<int>();
    }
    const size_t n_out = (size_t)nq * k;
    float* os = nullptr; int64_t* oi = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    const bool certify = ix->eps_rel == -2.f || ix->eps_rel >= 0.f;
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        const int64_t nbp = pad256l(nb);
        // rows >= nb: zeros; also clears the filtered search's flag counter
        HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)q0 * dim, ix->qbf.p, (size_t)nb * dim, (size_t)nbp * dim, s, ix->fstate.as<int>()));
        FilterSearchArgs p{};
        SearchArgs& a = p.a;
        a.index_bf16 = ix->bf16.p; a.index_f32 = ix->f32.as<float>(); a.n_docs = ix->n; a.dim = dim;
        a.q_bf16 = ix->qbf.p; a.q_f32 = q32 + (size_t)q0 * dim; a.nq = nb; a.k = k;
        fill_error_model(ix, a);
        a.flag_count = ix->fstate.as<int>(); a.flag_list = ix->fstate.as<int>() + FLT_LIST;
        a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k;
        p.bits = ix->fbits.as<uint32_t>(); p.words = (size_t)((ix->n + 31) / 32); p.n_filters = (int)ix->n_filters;
        p.allowed = ix->fcount.as<int>();
        p.filter_of_query = foq + q0;
        p.stats = ix->fstate.as<unsigned>() + FLT_STATS;
        p.certify = certify ? 1 : 0;
        // S[q][row] = queries x index^T on the bf16 MFMA GEMM, the deep path's launch; disallowed columns -> -inf
        VRCHK(score_rows(ix, ix->qbf.p, nb, nullptr, 0, GEMM_VARIANT_AUTO, ldS, s));
        HIPCHK(launch_filter_mask(p, ix->sbuf.as<float>(), (size_t)ldS, nb, nullptr, 0, s));
        HIPCHK(launch_filter_select(p, ix->sbuf.as<float>(), (size_t)ldS, nb, s));
        if (certify) {
            // whatever the select flagged (nothing, normally: the three kernels leave at once): exact fp32 score rows, masked
            HIPCHK(launch_exact_scores(a.index_f32, a.n_docs, dim, a.q_f32, a.flag_list, a.flag_count, 0, nb, ix->sbuf.as<float>(), (size_t)ldS, s));
            HIPCHK(launch_filter_mask(p, ix->sbuf.as<float>(), (size_t)ldS, nb, a.flag_count, 0, s));
            HIPCHK(launch_filter_select_exact(p, ix->sbuf.as<float>(), (size_t)ldS, 0, nb, s));
        }
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

constexpr int RNG_TOTAL = 3, RNG_SPARE = 4, RNG_WORDS = 16;

extern "C" int vr_index_range_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    out3[0] = out3[1] = out3[2] = 0;
    if (!ix->rstate.p) return VR_OK;              // no range search ever ran: nothing counted
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long w[3];
    HIPCHK(hipMemcpy(w, ix->rstate.p, sizeof(w), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) out3[i] = (int64_t)w[i];
    if (reset) HIPCHK(hipMemset(ix->rstate.p, 0, sizeof(w)));
    return VR_OK;
}

// room for `need` entries of the range result, the first `keep` of which are kept (what earlier blocks of the call packed)
static int range_reserve(vr_index_t ix, int64_t need, int64_t keep, int64_t max_total, hipStream_t s) {
    if (need <= ix->rcap && ix->rs.p && ix->ri.p) return VR_OK;
    const int64_t cap = std::max<int64_t>(std::min(max_total, std::max(need, 2 * ix->rcap)), std::max<int64_t>(need, 1));
    DevBuf ns, ni;
    VRCHK(ns.reserve((size_t)cap * 4));
    VRCHK(ni.reserve((size_t)cap * 8));
    if (keep > 0) {
        HIPCHK(hipMemcpyAsync(ns.p, ix->rs.p, (size_t)keep * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ni.p, ix->ri.p, (size_t)keep * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    ix->rs = std::move(ns);
    ix->ri = std::move(ni);
    ix->rcap = cap;
    return VR_OK;
}

// Every row at or above a query's threshold (search_range.hip).  Scratch (query staging, score rows, the staged filter_of_query)
// is shared with the other searches; result, counts, offsets and counters are the range search's own.
extern "C" int vr_index_search_range(vr_index_t ix, const float* queries, int32_t nq, const float* thresholds,
                                     const int32_t* filter_of_query, int64_t max_total, int64_t* out_lims, int64_t* total,
                                     int32_t on_device, void* stream) {
    if (!ix || !queries || !thresholds || !out_lims || !total || nq < 1) return fail(VR_ERR_INVALID, "bad arguments");
    if (max_total < 1) return fail(VR_ERR_INVALID, "max_total=%lld must be at least 1", (long long)max_total);
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (!on_device)
        for (int32_t q = 0; q < nq; ++q)
            if (!std::isfinite(thresholds[q])) return fail(VR_ERR_INVALID, "thresholds[%d] = %g is not finite", (int)q, (double)thresholds[q]);
    if (filter_of_query) {
        if (ix->n_filters <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no filters set for the rows of the index (vr_index_set_filters)");
        if (!on_device)
            for (int32_t q = 0; q < nq; ++q)
                if (filter_of_query[q] < -1 || filter_of_query[q] >= ix->n_filters)
                    return fail(VR_ERR_INVALID, "filter_of_query[%d] = %d outside [-1, %lld)", (int)q, (int)filter_of_query[q], (long long)ix->n_filters);
    }
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    if (ix->n == 0) {                             // no row: no launch
        if (on_device) {
            HIPCHK(hipMemsetAsync(out_lims, 0, ((size_t)nq + 1) * 8, s));
            HIPCHK(hipStreamSynchronize(s));
        } else {
            std::fill(out_lims, out_lims + nq + 1, (int64_t)0);
        }
        *total = 0;
        ix->range_total = 0;
        return VR_OK;
    }
    if (!ix->rstate.p) VRCHK(ix->rstate.alloc(RNG_WORDS * 8));
    if (!ix->range_host && hipHostMalloc((void**)&ix->range_host, 64, hipHostMallocDefault) != hipSuccess) {
        ix->range_host = nullptr;
        return fail(VR_ERR_HIP, "hipHostMalloc");
    }
    ix->range_total = -1;                         // from here on the previous result is gone
    const int dim = ix->dim;
    const int64_t ldS = pad256l(ix->n), slots = range_scan_slots(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const float* thr = thresholds;
    const int* foq = filter_of_query;
    int64_t* lims = out_lims;
    if (!on_device) {
        VRCHK(ix->rthr.reserve((size_t)nq * 4));
        HIPCHK(hipMemcpyAsync(ix->rthr.p, thresholds, (size_t)nq * 4, hipMemcpyHostToDevice, s));
        thr = ix->rthr.as<float>();
        if (foq) {
            VRCHK(ix->ffq.reserve((size_t)nq * 4));
            HIPCHK(hipMemcpyAsync(ix->ffq.p, filter_of_query, (size_t)nq * 4, hipMemcpyHostToDevice, s));
            foq = ix->ffq.as<int>();
        }
        VRCHK(ix->rlims.reserve(((size_t)nq + 1) * 8));
        lims = ix->rlims.as<int64_t>();
    }
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    VRCHK(ix->rcnt.reserve((size_t)qblk * slots * 4));
    VRCHK(ix->roff.reserve((size_t)qblk * slots * 4));
    VRCHK(range_reserve(ix, std::min<int64_t>(max_total, 65536), 0, max_total, s));
    unsigned long long* words = ix->rstate.as<unsigned long long>();
    const bool certify = ix->eps_rel == -2.f || ix->eps_rel >= 0.f;
    int64_t base = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        const int64_t nbp = pad256l(nb);
        HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)q0 * dim, ix->qbf.p, (size_t)nb * dim, (size_t)nbp * dim, s));   // rows >= nb: zeros
        RangeSearchArgs p{};
        SearchArgs& a = p.a;
        a.index_bf16 = ix->bf16.p; a.index_f32 = ix->f32.as<float>(); a.n_docs = ix->n; a.dim = dim;
        a.q_bf16 = ix->qbf.p; a.q_f32 = q32 + (size_t)q0 * dim; a.nq = nb; a.k = 1;
        // the band is defined by the error model: with certification off, the default one defines it
        fill_error_model(ix, a);
        if (!certify) { a.eps_data = 1; a.eps_rel = 0.f; }
        p.thresholds = thr + q0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->n_filters;
        p.stats = words;
        // S[q][row] = queries x index^T on the bf16 MFMA GEMM, the deep path's launch; disallowed columns -> -inf
        VRCHK(score_rows(ix, ix->qbf.p, nb, nullptr, 0, GEMM_VARIANT_AUTO, ldS, s));
        if (foq) {
            FilterSearchArgs f{};                 // the mask reads bits, words, n_filters and filter_of_query; the rest passes its argument check
            f.a = a;
            f.a.out_scores = ix->rs.as<float>(); f.a.out_ids = ix->ri.as<int64_t>();
            f.a.flag_count = reinterpret_cast<int*>(words + RNG_SPARE); f.a.flag_list = f.a.flag_count + 2;
            f.bits = ix->fbits.as<uint32_t>(); f.words = (size_t)((ix->n + 31) / 32); f.n_filters = (int)ix->n_filters;
            f.allowed = ix->fcount.as<int>();
            f.filter_of_query = p.filter_of_query;
            f.stats = reinterpret_cast<unsigned*>(words + RNG_SPARE) + 4;
            HIPCHK(launch_filter_mask(f, ix->sbuf.as<float>(), (size_t)ldS, nb, nullptr, 0, s));
        }
        HIPCHK(launch_range_rescore(p, ix->sbuf.as<float>(), (size_t)ldS, nb, ix->rcnt.as<int>(), s));
        HIPCHK(launch_range_scan(ix->rcnt.as<int>(), ix->roff.as<int>(), ix->n, nb, base, q0 == 0 ? 1 : 0, lims + q0,
                                 reinterpret_cast<int64_t*>(words + RNG_TOTAL), s));
        // the size of the block's result is a host value: capacity check, growth of the result arrays
        HIPCHK(hipMemcpyAsync(ix->range_host, words + RNG_TOTAL, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int64_t bt = *ix->range_host;
        if (bt < 0 || base + bt > max_total)
            return fail(VR_ERR_CAPACITY, "range result exceeds max_total=%lld in query block %lld (queries %lld..%lld): %lld entries by then",
                        (long long)max_total, (long long)(q0 / qblk), (long long)q0, (long long)(q0 + nb - 1), (long long)(base + bt));
        VRCHK(range_reserve(ix, base + bt, base, max_total, s));
        p.out_scores = ix->rs.as<float>(); p.out_ids = ix->ri.as<int64_t>();
        if (bt > 0)
            HIPCHK(launch_range_pack(p, ix->sbuf.as<float>(), (size_t)ldS, nb, ix->rcnt.as<int>(), ix->roff.as<int>(), lims + q0, s));
        base += bt;
    }
    if (!on_device) HIPCHK(hipMemcpyAsync(out_lims, lims, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *total = base;
    ix->range_total = base;
    return VR_OK;
}

extern "C" int vr_index_range_results(vr_index_t ix, float* out_scores, int64_t* out_ids, int64_t n, int32_t on_device, void* stream) {
    if (!ix || n < 0 || (n > 0 && (!out_scores || !out_ids))) return fail(VR_ERR_INVALID, "bad arguments");
    if (ix->range_total < 0) return fail(VR_ERR_STATE, "no range result (vr_index_search_range)");
    if (n > ix->range_total) return fail(VR_ERR_STATE, "%lld entries asked for, the last range search found %lld", (long long)n, (long long)ix->range_total);
    if (n == 0) return VR_OK;
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(out_scores, ix->rs.p, (size_t)n * 4, kind, s));
    HIPCHK(hipMemcpyAsync(out_ids, ix->ri.p, (size_t)n * 8, kind, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

constexpr int RNK_SPARE = 4, RNK_WORDS = 16;

extern "C" int vr_index_rank_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    out3[0] = out3[1] = out3[2] = 0;
    if (!ix->kstate.p) return VR_OK;              // no rank search ever ran: nothing counted
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long w[3];
    HIPCHK(hipMemcpy(w, ix->kstate.p, sizeof(w), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) out3[i] = (int64_t)w[i];
    if (reset) HIPCHK(hipMemset(ix->kstate.p, 0, sizeof(w)));
    return VR_OK;
}

// What vr_index_rank_rows (ids set) and vr_index_count_range (thresholds set) share: every check first, then per block of <= 256
// queries the score rows, the mask, the bars of the block's pairs and their counts (search_rank.hip).  Scratch (query staging,
// score rows, the staged filter_of_query and outputs) is shared with the other searches; nothing is stored.
static int rank_impl(vr_index_t ix, bool ranks, const float* queries, int32_t nq, const int64_t* lims, const int64_t* ids,
                     const float* thresholds, int32_t strict, const int32_t* filter_of_query, float* out_scores, int64_t* out_counts, int32_t on_device,
                     void* stream) {
    if (!ix || !lims || nq < 0 || (nq > 0 && !queries)) return fail(VR_ERR_INVALID, "bad arguments");
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (lims[0] != 0) return fail(VR_ERR_INVALID, "lims[0] = %lld must be 0", (long long)lims[0]);
    for (int32_t q = 0; q < nq; ++q)
        if (lims[q + 1] < lims[q]) return fail(VR_ERR_INVALID, "lims[%d] = %lld decreases", (int)q + 1, (long long)lims[q + 1]);
    const int64_t np = lims[nq];
    if (np >= ((int64_t)1 << 31)) return fail(VR_ERR_INVALID, "%lld pairs: too many for one call", (long long)np);
    if (np > 0 && (!out_counts || (ranks ? !ids || !out_scores : !thresholds))) return fail(VR_ERR_INVALID, "bad arguments");
    if (ranks) {
        for (int64_t i = 0; i < np; ++i)
            if (ids[i] < 0 || ids[i] >= ix->n)
                return fail(VR_ERR_INVALID, "ids[%lld] = %lld outside [0, %lld)", (long long)i, (long long)ids[i], (long long)ix->n);
    } else {
        for (int64_t i = 0; i < np; ++i)
            if (!std::isfinite(thresholds[i])) return fail(VR_ERR_INVALID, "thresholds[%lld] = %g is not finite", (long long)i, (double)thresholds[i]);
    }
    if (filter_of_query) {
        if (ix->n_filters <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no filters set for the rows of the index (vr_index_set_filters)");
        if (!on_device)
            for (int32_t q = 0; q < nq; ++q)
                if (filter_of_query[q] < -1 || filter_of_query[q] >= ix->n_filters)
                    return fail(VR_ERR_INVALID, "filter_of_query[%d] = %d outside [-1, %lld)", (int)q, (int)filter_of_query[q], (long long)ix->n_filters);
    }
    if (np == 0) return VR_OK;                    // no pair: no launch
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    if (ix->n == 0) {                             // (counts only: a target row would have been out of range) no row: no launch
        if (on_device) HIPCHK(hipMemsetAsync(out_counts, 0, (size_t)np * 8, s));
        else std::fill(out_counts, out_counts + np, (int64_t)0);
        return VR_OK;
    }
    if (!ix->kstate.p) VRCHK(ix->kstate.alloc(RNK_WORDS * 8));
    const int dim = ix->dim;
    const int64_t ldS = pad256l(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const int* foq = filter_of_query;
    if (foq && !on_device) {
        VRCHK(ix->ffq.reserve((size_t)nq * 4));
        HIPCHK(hipMemcpyAsync(ix->ffq.p, filter_of_query, (size_t)nq * 4, hipMemcpyHostToDevice, s));
        foq = ix->ffq.as<int>();
    }
    // the pairs: their query inside its block and their target row or threshold, 4 bytes each
    std::vector<int> pq((size_t)np), pv(ids ? (size_t)np : 0);
    for (int32_t q = 0; q < nq; ++q)
        for (int64_t i = lims[q]; i < lims[q + 1]; ++i) pq[(size_t)i] = (int)(q % qblk);
    if (ids) for (int64_t i = 0; i < np; ++i) pv[(size_t)i] = (int)ids[i];
    VRCHK(ix->kq.reserve((size_t)np * 4));
    VRCHK(ix->kv.reserve((size_t)np * 4));
    VRCHK(ix->kbar.reserve((size_t)np * 8));
    VRCHK(ix->keps.reserve((size_t)np * 4));
    HIPCHK(hipMemcpyAsync(ix->kq.p, pq.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ix->kv.p, ids ? (const void*)pv.data() : (const void*)thresholds, (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));              // (the host arrays are free from here on)
    float* os = nullptr; int64_t* oc = nullptr;
    if (ids) VRCHK(stage_output(ix->os, out_scores, (size_t)np, on_device, &os));
    VRCHK(stage_output(ix->oi, out_counts, (size_t)np, on_device, &oc));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    unsigned long long* words = ix->kstate.as<unsigned long long>();
    const bool certify = ix->eps_rel == -2.f || ix->eps_rel >= 0.f;
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        const int64_t p0 = lims[q0], pn = lims[q0 + nb] - p0;
        if (pn == 0) continue;                    // a block without pairs: no launch
        const int64_t nbp = pad256l(nb);
        HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)q0 * dim, ix->qbf.p, (size_t)nb * dim, (size_t)nbp * dim, s));   // rows >= nb: zeros
        RankSearchArgs p{};
        SearchArgs& a = p.a;
        a.index_bf16 = ix->bf16.p; a.index_f32 = ix->f32.as<float>(); a.n_docs = ix->n; a.dim = dim;
        a.q_bf16 = ix->qbf.p; a.q_f32 = q32 + (size_t)q0 * dim; a.nq = nb; a.k = 1;
        // the band is defined by the error model: with certification off, the default one defines it
        fill_error_model(ix, a);
        if (!certify) { a.eps_data = 1; a.eps_rel = 0.f; }
        p.pair_query = ix->kq.as<int>() + p0;
        p.pair_id = ids ? ix->kv.as<int>() + p0 : nullptr;
        p.pair_thr = ids ? nullptr : ix->kv.as<float>() + p0;
        p.strict = strict ? 1 : 0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->n_filters;
        p.bars = ix->kbar.as<unsigned long long>() + p0;
        p.bar_eps = ix->keps.as<float>() + p0;
        p.out_scores = ids ? os + p0 : nullptr;
        p.out_counts = reinterpret_cast<unsigned long long*>(oc) + p0;
        p.stats = words;
        // S[q][row] = queries x index^T on the bf16 MFMA GEMM, the deep path's launch; disallowed columns -> -inf
        VRCHK(score_rows(ix, ix->qbf.p, nb, nullptr, 0, GEMM_VARIANT_AUTO, ldS, s));
        if (foq) {
            FilterSearchArgs f{};                 // the mask reads bits, words, n_filters and filter_of_query; the rest passes its argument check
            f.a = a;
            f.a.out_scores = ix->keps.as<float>(); f.a.out_ids = oc;
            f.a.flag_count = reinterpret_cast<int*>(words + RNK_SPARE); f.a.flag_list = f.a.flag_count + 2;
            f.bits = ix->fbits.as<uint32_t>(); f.words = (size_t)((ix->n + 31) / 32); f.n_filters = (int)ix->n_filters;
            f.allowed = ix->fcount.as<int>();
            f.filter_of_query = p.filter_of_query;
            f.stats = reinterpret_cast<unsigned*>(words + RNK_SPARE) + 4;
            HIPCHK(launch_filter_mask(f, ix->sbuf.as<float>(), (size_t)ldS, nb, nullptr, 0, s));
        }
        HIPCHK(launch_rank_bars(p, (size_t)ldS, nb, pn, s));
        HIPCHK(launch_rank_count(p, ix->sbuf.as<float>(), (size_t)ldS, nb, pn, s));
    }
    if (ids) VRCHK(return_output(out_scores, os, (size_t)np, on_device, s));
    VRCHK(return_output(out_counts, oc, (size_t)np, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_index_rank_rows(vr_index_t ix, const float* queries, int32_t nq, const int64_t* lims, const int64_t* ids,
                                  const int32_t* filter_of_query, float* out_scores, int64_t* out_ranks, int32_t on_device, void* stream) {
    return rank_impl(ix, true, queries, nq, lims, ids, nullptr, 0, filter_of_query, out_scores, out_ranks, on_device, stream);
}

extern "C" int vr_index_count_range(vr_index_t ix, const float* queries, int32_t nq, const int64_t* lims, const float* thresholds,
                                    int32_t strict, const int32_t* filter_of_query, int64_t* out_counts, int32_t on_device, void* stream) {
    return rank_impl(ix, false, queries, nq, lims, nullptr, thresholds, strict, filter_of_query, nullptr, out_counts,
                     on_device, stream);
}

constexpr int WIN_SPARE = 4, WIN_WORDS = 16;

extern "C" int vr_index_window_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    out3[0] = out3[1] = out3[2] = 0;
    if (!ix->wstate.p) return VR_OK;              // no windowed search ever ran: nothing counted
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long w[3];
    HIPCHK(hipMemcpy(w, ix->wstate.p, sizeof(w), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) out3[i] = (int64_t)w[i];
    if (reset) HIPCHK(hipMemset(ix->wstate.p, 0, sizeof(w)));
    return VR_OK;
}

// The rows at ranks [offsets[q], offsets[q] + k) of every query's fp32 ranking (search_window.hip): every check first, then per
// block of <= 256 queries the score rows, the mask, the band edges, the rewritten rows and the select.  Scratch (query staging,
// score rows, the staged filter_of_query and outputs) is shared with the other searches; nothing is stored.
extern "C" int vr_index_search_window(vr_index_t ix, const float* queries, int32_t nq, const int64_t* offsets, int32_t k,
                                      const int32_t* filter_of_query, float* out_scores, int64_t* out_ids, int32_t on_device,
                                      void* stream) {
    if (!ix || nq < 0 || (nq > 0 && (!queries || !offsets || !out_scores || !out_ids))) return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    for (int32_t q = 0; q < nq; ++q)
        if (offsets[q] < 0) return fail(VR_ERR_INVALID, "offsets[%d] = %lld is negative", (int)q, (long long)offsets[q]);
    if (filter_of_query) {
        if (ix->n_filters <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no filters set for the rows of the index (vr_index_set_filters)");
        if (!on_device)
            for (int32_t q = 0; q < nq; ++q)
                if (filter_of_query[q] < -1 || filter_of_query[q] >= ix->n_filters)
                    return fail(VR_ERR_INVALID, "filter_of_query[%d] = %d outside [-1, %lld)", (int)q, (int)filter_of_query[q], (long long)ix->n_filters);
    }
    if (nq == 0) return VR_OK;                    // no query: no launch
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)nq * k;
    if (ix->n == 0) {                             // no row: tails, no launch
        if (on_device) {
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)out_scores, (int)0xFF800000u, n_out, s));     // -inf
            HIPCHK(hipMemsetAsync(out_ids, 0xFF, n_out * 8, s));                                   // -1
        } else {
            std::fill(out_scores, out_scores + n_out, -INFINITY);
            std::fill(out_ids, out_ids + n_out, (int64_t)-1);
        }
        return VR_OK;
    }
    if (!ix->wstate.p) VRCHK(ix->wstate.alloc(WIN_WORDS * 8));
    const int dim = ix->dim;
    const int64_t ldS = pad256l(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const int* foq = filter_of_query;
    if (foq && !on_device) {
        VRCHK(ix->ffq.reserve((size_t)nq * 4));
        HIPCHK(hipMemcpyAsync(ix->ffq.p, filter_of_query, (size_t)nq * 4, hipMemcpyHostToDevice, s));
        foq = ix->ffq.as<int>();
    }
    VRCHK(ix->woff.reserve((size_t)nq * 8));
    VRCHK(ix->wedge.reserve((size_t)qblk * 8));
    HIPCHK(hipMemcpyAsync(ix->woff.p, offsets, (size_t)nq * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));              // (the host array is free from here on)
    float* os = nullptr; int64_t* oi = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    unsigned long long* words = ix->wstate.as<unsigned long long>();
    const bool certify = ix->eps_rel == -2.f || ix->eps_rel >= 0.f;
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        const int64_t nbp = pad256l(nb);
        HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)q0 * dim, ix->qbf.p, (size_t)nb * dim, (size_t)nbp * dim, s));   // rows >= nb: zeros
        WindowSearchArgs p{};
        SearchArgs& a = p.a;
        a.index_bf16 = ix->bf16.p; a.index_f32 = ix->f32.as<float>(); a.n_docs = ix->n; a.dim = dim;
        a.q_bf16 = ix->qbf.p; a.q_f32 = q32 + (size_t)q0 * dim; a.nq = nb; a.k = k;
        // the band is defined by the error model: with certification off, the default one defines it
        fill_error_model(ix, a);
        if (!certify) { a.eps_data = 1; a.eps_rel = 0.f; }
        a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k;
        p.offsets = ix->woff.as<int64_t>() + q0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->n_filters;
        p.allowed = foq ? ix->fcount.as<int>() : nullptr;
        p.edges = ix->wedge.as<float>();
        p.stats = words;
        // S[q][row] = queries x index^T on the bf16 MFMA GEMM, the deep path's launch; disallowed columns -> -inf
        VRCHK(score_rows(ix, ix->qbf.p, nb, nullptr, 0, GEMM_VARIANT_AUTO, ldS, s));
        if (foq) {
            FilterSearchArgs f{};                 // the mask reads bits, words, n_filters and filter_of_query; the rest passes its argument check
            f.a = a;
            f.a.flag_count = reinterpret_cast<int*>(words + WIN_SPARE); f.a.flag_list = f.a.flag_count + 2;
            f.bits = ix->fbits.as<uint32_t>(); f.words = (size_t)((ix->n + 31) / 32); f.n_filters = (int)ix->n_filters;
            f.allowed = ix->fcount.as<int>();
            f.filter_of_query = p.filter_of_query;
            f.stats = reinterpret_cast<unsigned*>(words + WIN_SPARE) + 4;
            HIPCHK(launch_filter_mask(f, ix->sbuf.as<float>(), (size_t)ldS, nb, nullptr, 0, s));
        }
        HIPCHK(launch_window_edges(p, ix->sbuf.as<float>(), (size_t)ldS, nb, s));
        HIPCHK(launch_window_rescore(p, ix->sbuf.as<float>(), (size_t)ldS, nb, s));
        HIPCHK(launch_window_select(p, ix->sbuf.as<float>(), (size_t)ldS, nb, s));
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_index_multi_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    out3[0] = out3[1] = out3[2] = 0;
    if (!ix->mstate.p) return VR_OK;              // no fused search ever ran: nothing counted
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long w[3];
    HIPCHK(hipMemcpy(w, ix->mstate.p, sizeof(w), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) out3[i] = (int64_t)w[i];
    if (reset) HIPCHK(hipMemset(ix->mstate.p, 0, sizeof(w)));
    return VR_OK;
}

// The k rows of largest fused score of every group of sub-queries (search_multi.hip): every check first, then whole groups packed
// greedily into blocks of <= 256 sub-queries, and per block the score rows, the mask, the fusion, the band edges, the rewritten
// fused rows and the select.  Scratch (query staging, score rows, the staged filter_of_group and outputs) is shared with the
// other searches; nothing is stored.
extern "C" int vr_index_search_multi(vr_index_t ix, const float* queries, int32_t n_sub, const int64_t* lims, int32_t n_groups,
                                     int32_t k, int32_t fuse, const int32_t* filter_of_group, float* out_scores, int64_t* out_ids,
                                     int32_t* out_which, int32_t on_device, void* stream) {
    if (!ix || n_groups < 0 || n_sub < 0 || (n_groups > 0 && (!queries || !lims || !out_scores || !out_ids || !out_which)))
        return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (fuse != 0 && fuse != 1) return fail(VR_ERR_INVALID, "fuse=%d unsupported (0: max, 1: min)", (int)fuse);
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (n_groups == 0) {
        if (n_sub != 0) return fail(VR_ERR_INVALID, "%d sub-queries in no group", (int)n_sub);
        return VR_OK;                             // no group: no launch
    }
    if (lims[0] != 0) return fail(VR_ERR_INVALID, "lims[0] = %lld, not 0", (long long)lims[0]);
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t m = lims[g + 1] - lims[g];
        if (m < 0) return fail(VR_ERR_INVALID, "lims[%d] = %lld decreases", (int)g + 1, (long long)lims[g + 1]);
        if (m == 0) return fail(VR_ERR_INVALID, "group %d is empty", (int)g);
        if (m > 256) return fail(VR_ERR_INVALID, "group %d holds %lld sub-queries (1..256)", (int)g, (long long)m);
    }
    if (lims[n_groups] != n_sub)
        return fail(VR_ERR_INVALID, "lims[%d] = %lld, not the %d sub-queries", (int)n_groups, (long long)lims[n_groups], (int)n_sub);
    if (filter_of_group) {
        if (ix->n_filters <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no filters set for the rows of the index (vr_index_set_filters)");
        if (!on_device)
            for (int32_t g = 0; g < n_groups; ++g)
                if (filter_of_group[g] < -1 || filter_of_group[g] >= ix->n_filters)
                    return fail(VR_ERR_INVALID, "filter_of_group[%d] = %d outside [-1, %lld)", (int)g, (int)filter_of_group[g], (long long)ix->n_filters);
    }
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)n_groups * k;
    if (ix->n == 0) {                             // no row: tails, no launch
        if (on_device) {
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)out_scores, (int)0xFF800000u, n_out, s));     // -inf
            HIPCHK(hipMemsetAsync(out_ids, 0xFF, n_out * 8, s));                                   // -1
            HIPCHK(hipMemsetAsync(out_which, 0xFF, n_out * 4, s));
        } else {
            std::fill(out_scores, out_scores + n_out, -INFINITY);
            std::fill(out_ids, out_ids + n_out, (int64_t)-1);
            std::fill(out_which, out_which + n_out, (int32_t)-1);
        }
        return VR_OK;
    }
    if (!ix->mstate.p) VRCHK(ix->mstate.alloc(WIN_WORDS * 8));
    const int dim = ix->dim;
    const int64_t ldS = pad256l(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per sub-query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, n_sub, pad256l(std::min<int64_t>(n_sub, qblk)), on_device, s, &q32));
    std::vector<int> lims32((size_t)n_groups + 1);
    for (int32_t g = 0; g <= n_groups; ++g) lims32[g] = (int)lims[g];
    VRCHK(ix->mlims.reserve(lims32.size() * 4));
    VRCHK(ix->medge.reserve((size_t)qblk * 4));
    HIPCHK(hipMemcpyAsync(ix->mlims.p, lims32.data(), lims32.size() * 4, hipMemcpyHostToDevice, s));
    const int* fog = filter_of_group;
    if (fog) {                                    // the group's filter for every one of its score rows: what the mask reads
        if (!on_device) {
            VRCHK(ix->ffq.reserve((size_t)n_groups * 4));
            HIPCHK(hipMemcpyAsync(ix->ffq.p, filter_of_group, (size_t)n_groups * 4, hipMemcpyHostToDevice, s));
            fog = ix->ffq.as<int>();
        }
        VRCHK(ix->mfsub.reserve((size_t)n_sub * 4));
        HIPCHK(launch_multi_expand(ix->mlims.as<int>(), fog, n_groups, ix->mfsub.as<int>(), s));
    }
    HIPCHK(hipStreamSynchronize(s));              // (the host arrays are free from here on)
    float* os = nullptr; int64_t* oi = nullptr; int32_t* ow = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(stage_output(ix->mwhich, out_which, n_out, on_device, &ow));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    unsigned long long* words = ix->mstate.as<unsigned long long>();
    const bool certify = ix->eps_rel == -2.f || ix->eps_rel >= 0.f;
    for (int32_t g0 = 0; g0 < n_groups;) {
        int32_t g1 = g0 + 1;                      // whole groups while the block holds <= 256 sub-queries
        while (g1 < n_groups && lims[g1 + 1] - lims[g0] <= qblk) ++g1;
        const int64_t s0 = lims[g0];
        const int nb = (int)(lims[g1] - s0), ng = g1 - g0;
        const int64_t nbp = pad256l(nb);
        HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)s0 * dim, ix->qbf.p, (size_t)nb * dim, (size_t)nbp * dim, s));   // rows >= nb: zeros
        MultiSearchArgs p{};
        SearchArgs& a = p.a;
        a.index_bf16 = ix->bf16.p; a.index_f32 = ix->f32.as<float>(); a.n_docs = ix->n; a.dim = dim;
        a.q_bf16 = ix->qbf.p; a.q_f32 = q32 + (size_t)s0 * dim; a.nq = nb; a.k = k;
        // the band is defined by the error model: with certification off, the default one defines it
        fill_error_model(ix, a);
        if (!certify) { a.eps_data = 1; a.eps_rel = 0.f; }
        a.out_scores = os + (size_t)g0 * k; a.out_ids = oi + (size_t)g0 * k;
        p.out_which = ow + (size_t)g0 * k;
        p.lims = ix->mlims.as<int>() + g0;
        p.sub_base = (int)s0;
        p.fuse = fuse;
        p.filter_of_group = fog ? fog + g0 : nullptr;
        p.n_filters = (int)ix->n_filters;
        p.allowed = fog ? ix->fcount.as<int>() : nullptr;
        p.edges = ix->medge.as<float>();
        p.stats = words;
        // S[sub-query][row] = sub-queries x index^T on the bf16 MFMA GEMM, the deep path's launch; disallowed columns -> -inf
        VRCHK(score_rows(ix, ix->qbf.p, nb, nullptr, 0, GEMM_VARIANT_AUTO, ldS, s));
        if (fog) {
            FilterSearchArgs f{};                 // the mask reads bits, words, n_filters and filter_of_query; the rest passes its argument check
            f.a = a;
            f.a.flag_count = reinterpret_cast<int*>(words + WIN_SPARE); f.a.flag_list = f.a.flag_count + 2;
            f.bits = ix->fbits.as<uint32_t>(); f.words = (size_t)((ix->n + 31) / 32); f.n_filters = (int)ix->n_filters;
            f.allowed = ix->fcount.as<int>();
            f.filter_of_query = ix->mfsub.as<int>() + s0;
            f.stats = reinterpret_cast<unsigned*>(words + WIN_SPARE) + 4;
            HIPCHK(launch_filter_mask(f, ix->sbuf.as<float>(), (size_t)ldS, nb, nullptr, 0, s));
        }
        HIPCHK(launch_multi_fuse(p, ix->sbuf.as<float>(), (size_t)ldS, ng, s));
        HIPCHK(launch_multi_edges(p, ix->sbuf.as<float>(), (size_t)ldS, ng, s));
        HIPCHK(launch_multi_rescore(p, ix->sbuf.as<float>(), (size_t)ldS, ng, s));
        HIPCHK(launch_multi_select(p, ix->sbuf.as<float>(), (size_t)ldS, ng, s));
        g0 = g1;
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    VRCHK(return_output(out_which, ow, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// k rows per query picked by maximal marginal relevance from the pool of its `pool` best rows (search_diverse.hip).  The pool
// is the plain or the filtered search's own result, produced by that search as it stands on the staged queries with device
// outputs of the diverse search's own; the selection kernel writes the (staged) outputs.  No state of its own but the pool.
extern "C" int vr_index_search_diverse(vr_index_t ix, const float* queries, int32_t nq, int32_t k, int32_t pool, float lambda,
                                       const int32_t* filter_of_query, float* out_scores, int64_t* out_ids, int32_t on_device,
                                       void* stream) {
    if (!ix || !queries || !out_scores || !out_ids || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    if (k < 1 || k > pool || pool > search_bigk_max())
        return fail(VR_ERR_INVALID, "k=%d pool=%d unsupported (1 <= k <= pool <= %d)", k, pool, search_bigk_max());
    if (!(lambda >= 0.f && lambda <= 1.f)) return fail(VR_ERR_INVALID, "lambda=%g outside [0, 1]", (double)lambda);
    if (!mmr_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (filter_of_query) {
        if (ix->n_filters <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no filters set for the rows of the index (vr_index_set_filters)");
        if (!on_device)
            for (int32_t q = 0; q < nq; ++q)
                if (filter_of_query[q] < -1 || filter_of_query[q] >= ix->n_filters)
                    return fail(VR_ERR_INVALID, "filter_of_query[%d] = %d outside [-1, %lld)", (int)q, (int)filter_of_query[q], (long long)ix->n_filters);
    }
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, 256)), on_device, s, &q32));
    const int* foq = filter_of_query;
    if (foq && !on_device) {
        VRCHK(ix->ffq.reserve((size_t)nq * 4));
        HIPCHK(hipMemcpyAsync(ix->ffq.p, filter_of_query, (size_t)nq * 4, hipMemcpyHostToDevice, s));
        foq = ix->ffq.as<int>();
    }
    // ---- the pool: the staged queries are device queries to the search, which then stages nothing and writes the pool buffers
    const size_t n_pool = (size_t)nq * pool, n_out = (size_t)nq * k;
    VRCHK(ix->dps.reserve(n_pool * 4));
    VRCHK(ix->dpi.reserve(n_pool * 8));
    if (foq) VRCHK(vr_index_search_filtered(ix, q32, nq, pool, foq, ix->dps.as<float>(), ix->dpi.as<int64_t>(), 1, stream));
    else VRCHK(search_impl(ix, q32, nq, pool, ix->dps.as<float>(), ix->dpi.as<int64_t>(), nullptr, 0, 1, stream));
    // ---- the picks
    float* os = nullptr; int64_t* oi = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    MmrArgs m{};
    m.index_f32 = ix->f32.as<float>(); m.n_docs = ix->n; m.dim = ix->dim;
    m.pool_scores = ix->dps.as<float>(); m.pool_ids = ix->dpi.as<int64_t>();
    m.nq = nq; m.pool = pool; m.k = k; m.lambda = lambda;
    m.out_scores = os; m.out_ids = oi;
    HIPCHK(launch_mmr_select(m, s));
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- editing in place (index_edit.hip) ----------------------------------------------------------------------------------------
constexpr size_t EDIT_SCRATCH = (size_t)64 << 20;        // rows in flight between two launches of a removal; the staging of get_rows
constexpr size_t EDIT_WINDOW_MIN = (size_t)16 << 20;     // a removal's window that wide is moved without scratch

// the ids of an editing call, checked against the rows present, as 32-bit rows (vr_index_create: rows fit)
static int edit_ids(vr_index_t ix, const int64_t* ids, int64_t n, std::vector<int>& out) {
    out.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= ix->n)
            return fail(VR_ERR_INVALID, "ids[%lld] = %lld outside [0, %lld)", (long long)i, (long long)ids[i], (long long)ix->n);
        out[(size_t)i] = (int)ids[i];
    }
    return VR_OK;
}

// The list is a host vector that dies with the call: every editing call ends with a stream synchronisation.
static int upload_ids(vr_index_t ix, const std::vector<int>& ids, hipStream_t s) {
    VRCHK(ix->eids.reserve(ids.size() * 4));
    HIPCHK(hipMemcpyAsync(ix->eids.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, s));
    return VR_OK;
}

// the largest row norm and rounding residual over the rows present, from scratch (vr_index_add only ever raises them)
static int recompute_error_model(vr_index_t ix, hipStream_t s) {
    HIPCHK(hipMemsetAsync(ix->cert.p, 0, 8, s));
    HIPCHK(launch_row_norm_max(ix->f32.as<float>(), ix->n, ix->dim, ix->cert.as<float>(), s));
    return VR_OK;
}

// the old row that becomes row j once the sorted distinct rows `rem` are gone (index_edit.hip: compact_src)
static int64_t compact_src_host(const std::vector<int>& rem, int64_t j) {
    size_t lo = 0, hi = rem.size();
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if ((int64_t)rem[mid] - (int64_t)mid <= j) lo = mid + 1;
        else hi = mid;
    }
    return j + (int64_t)lo;
}

// Rows [rem[0], new_n) of one store closed up in place, in ascending windows [c0, c1).  A launch never reads a row that it (or a
// launch still to come) writes: windows before this one wrote rows < c0 only, and this one reads rows >= src(c0) >= c0.
//   src(c0) >= c1 (the rows removed so far make the window at least EDIT_WINDOW_MIN wide): gathered straight into place — the
//     launch reads rows >= c1 and writes rows < c1;
//   else: gathered into the scratch, then copied to [c0, c1) — each launch reads one buffer and writes the other.
static int compact_store(vr_index_t ix, void* store, size_t row_bytes, const std::vector<int>& rem, int64_t new_n, hipStream_t s) {
    const int* rem_dev = ix->eids.as<int>();
    const int nr = (int)rem.size();
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(EDIT_SCRATCH / row_bytes));
    const int64_t window_min = std::max<int64_t>(1, (int64_t)(EDIT_WINDOW_MIN / row_bytes));
    for (int64_t c0 = rem[0]; c0 < new_n;) {
        const int64_t shift = compact_src_host(rem, c0) - c0;
        char* dst = (char*)store + (size_t)c0 * row_bytes;
        int64_t c1;
        if (shift >= window_min) {
            c1 = std::min(new_n, c0 + shift);
            HIPCHK(launch_rows_compact(store, row_bytes, rem_dev, nr, c0, c1 - c0, dst, s));
        } else {
            c1 = std::min(new_n, c0 + chunk);
            HIPCHK(launch_rows_compact(store, row_bytes, rem_dev, nr, c0, c1 - c0, ix->sbuf.p, s));
            HIPCHK(hipMemcpyAsync(dst, ix->sbuf.p, (size_t)(c1 - c0) * row_bytes, hipMemcpyDeviceToDevice, s));
        }
        c0 = c1;
    }
    return VR_OK;
}

extern "C" int vr_index_remove(vr_index_t ix, const int64_t* ids, int64_t n, int64_t* removed, void* stream) {
    if (!ix || (!ids && n > 0) || n < 0) return fail(VR_ERR_INVALID, "bad arguments");
    std::vector<int> rem;
    VRCHK(edit_ids(ix, ids, n, rem));
    if (removed) *removed = 0;
    if (n == 0) return VR_OK;
    std::sort(rem.begin(), rem.end());
    rem.erase(std::unique(rem.begin(), rem.end()), rem.end());
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());               // (a search in flight reads the rows)
    hipStream_t s = (hipStream_t)stream;
    const int64_t old_n = ix->n, new_n = old_n - (int64_t)rem.size();
    const size_t rb32 = (size_t)ix->dim * 4, rb16 = (size_t)ix->dim * 2;
    const bool moves = rem[0] < new_n, filters = ix->n_filters > 0 && new_n > 0;
    if (moves || filters) VRCHK(upload_ids(ix, rem, s));
    if (moves) {
        VRCHK(ix->sbuf.reserve(std::min(EDIT_SCRATCH, (size_t)(new_n - rem[0]) * rb32)));
        VRCHK(compact_store(ix, ix->f32.p, rb32, rem, new_n, s));
        VRCHK(compact_store(ix, ix->bf16.p, rb16, rem, new_n, s));
    }
    // what a 256-row tile of the new last rows can still touch reads as in an index that never held more
    const int64_t tail = std::min(old_n, pad256l(new_n)) - new_n;
    if (tail > 0) {
        HIPCHK(hipMemsetAsync((char*)ix->f32.p + (size_t)new_n * rb32, 0, (size_t)tail * rb32, s));
        HIPCHK(hipMemsetAsync((char*)ix->bf16.p + (size_t)new_n * rb16, 0, (size_t)tail * rb16, s));
    }
    if (filters) {
        const size_t words = (size_t)((old_n + 31) / 32), new_words = (size_t)((new_n + 31) / 32);
        VRCHK(ix->fbits2.reserve(new_words * (size_t)ix->n_filters * 4));
        HIPCHK(launch_filter_compact(ix->fbits.as<uint32_t>(), words, (int)ix->n_filters, ix->eids.as<int>(), (int)rem.size(), new_n,
                                     ix->fbits2.as<uint32_t>(), s));
        std::swap(ix->fbits, ix->fbits2);
        HIPCHK(launch_filter_prepare(ix->fbits.as<uint32_t>(), new_words, (int)ix->n_filters, new_n, ix->fcount.as<int>(), s));
    }
    ix->n = new_n;
    ix->n_groups = 0;                 // a removal can empty a group: the caller sets the offsets of the rows that remain
    ix->range_total = -1;             // its ids name rows as they were
    if (ix->huge_seen) *ix->huge_seen = 0;
    VRCHK(recompute_error_model(ix, s));
    HIPCHK(hipStreamSynchronize(s));
    if (removed) *removed = (int64_t)rem.size();
    return VR_OK;
}

extern "C" int vr_index_update(vr_index_t ix, const int64_t* ids, const float* reps, int64_t n, int32_t on_device, void* stream) {
    if (!ix || ((!ids || !reps) && n > 0) || n < 0) return fail(VR_ERR_INVALID, "bad arguments");
    std::vector<int> rows;
    VRCHK(edit_ids(ix, ids, n, rows));
    if (n == 0) return VR_OK;
    {
        std::vector<int> sorted(rows);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) return fail(VR_ERR_INVALID, "row %d is named more than once", *dup);
    }
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    VRCHK(upload_ids(ix, rows, s));
    const float* src = reps;
    if (!on_device) {
        VRCHK(ix->erows.reserve((size_t)n * ix->dim * 4));
        HIPCHK(hipMemcpyAsync(ix->erows.p, reps, (size_t)n * ix->dim * 4, hipMemcpyHostToDevice, s));
        src = ix->erows.as<float>();
    }
    HIPCHK(launch_rows_update(src, ix->eids.as<int>(), n, ix->dim, ix->f32.as<float>(), ix->bf16.p, s));
    VRCHK(recompute_error_model(ix, s));          // (an overwritten row may have been the largest)
    ix->range_total = -1;
    if (ix->huge_seen) *ix->huge_seen = 0;
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// rows ids[0..n) of one store to `out`: gathered straight into a device array, or through the bounded staging to a host array
static int get_rows(vr_index_t ix, const void* store, size_t row_bytes, int64_t n, void* out, int32_t on_device, hipStream_t s) {
    if (on_device) {
        HIPCHK(launch_rows_gather(store, row_bytes, ix->eids.as<int>(), n, out, s));
        return VR_OK;
    }
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(EDIT_SCRATCH / row_bytes));
    VRCHK(ix->erows.reserve((size_t)std::min(n, chunk) * row_bytes));
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t cn = std::min(chunk, n - c0);
        HIPCHK(launch_rows_gather(store, row_bytes, ix->eids.as<int>() + c0, cn, ix->erows.p, s));
        HIPCHK(hipMemcpyAsync((char*)out + (size_t)c0 * row_bytes, ix->erows.p, (size_t)cn * row_bytes, hipMemcpyDeviceToHost, s));
    }
    return VR_OK;
}

extern "C" int vr_index_get_rows(vr_index_t ix, const int64_t* ids, int64_t n, float* out_f32, uint16_t* out_bf16, int32_t on_device,
                                 void* stream) {
    if (!ix || (!ids && n > 0) || n < 0 || (!out_f32 && !out_bf16)) return fail(VR_ERR_INVALID, "bad arguments");
    std::vector<int> rows;
    VRCHK(edit_ids(ix, ids, n, rows));
    if (n == 0) return VR_OK;
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    VRCHK(upload_ids(ix, rows, s));
    if (out_f32) VRCHK(get_rows(ix, ix->f32.p, (size_t)ix->dim * 4, n, out_f32, on_device, s));
    if (out_bf16) VRCHK(get_rows(ix, ix->bf16.p, (size_t)ix->dim * 2, n, out_bf16, on_device, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_topk_merge(int device_id, const float* scores, const int64_t* ids, int32_t n_parts, int32_t nq,
                             int32_t k, float* out_scores, int64_t* out_ids, void* stream) {
    if (!scores || !ids || !out_scores || !out_ids || n_parts <= 0 || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_topk_merge(scores, ids, n_parts, nq, k, out_scores, out_ids, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_topk_merge_keys(int device_id, const uint64_t* keys, int32_t n_parts, int32_t nq, int32_t k,
                                  float* out_scores, int64_t* out_ids, void* stream) {
    if (!keys || !out_scores || !out_ids || n_parts <= 0 || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_topk_merge_keys((const unsigned long long*)keys, n_parts, nq, k, out_scores, out_ids, (hipStream_t)stream));
    return VR_OK;
}
