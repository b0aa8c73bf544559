// The searches of the index that work on score rows (vr_index_search_groups / _filtered / _range / _rank_rows / _count_range /
// _window / _groups_window / _rank_groups / _count_groups_range / _groups_range / _multi / _diverse / _rrf of include/visrag_hip.h, with what sets them up and their counters).  Each of them: every argument
// check first, then per block of <= 256 queries the block's score rows S[q][row] (index.h: score_block, the deep path's bf16
// MFMA GEMM), with filters the mask (mask_block: disallowed columns -> -inf), then the search's own kernels.  Scratch (query
// staging, score rows, staged outputs, the staged filter ids) is shared between the searches; what a search keeps is its member
// of the handle (index.h).
#include "index.h"

// ---- grouped search (search_group.hip) ----------------------------------------------------------------------------------------
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
    ix->grp.n_groups = 0;
    ix->grng.total = -1;              // the document range result names groups of the grouping that was
    std::vector<int> off((size_t)n_groups + 1);   // rows are 32-bit (vr_index_create)
    for (int64_t g = 0; g <= n_groups; ++g) off[(size_t)g] = (int)group_offsets[g];
    VRCHK(ix->grp.off.reserve(off.size() * 4));
    HIPCHK(hipMemcpy(ix->grp.off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (!ix->grp.state.p) VRCHK(ix->grp.state.alloc(GRP_WORDS * 4));
    ix->grp.n_groups = n_groups;
    return VR_OK;
}

extern "C" int vr_index_group_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned, 3>(ix, ix->grp.state, GRP_STATS, out3, reset);
}

// The k best groups per query: flag list, counters and group maxima are the grouped search's own.
extern "C" int vr_index_search_groups(vr_index_t ix, const float* queries, int32_t nq, int32_t k, float* out_scores,
                                      int64_t* out_ids, int64_t* out_groups, int32_t on_device, void* stream) {
    if (!ix || !queries || !out_scores || !out_ids || !out_groups || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_groups_kmax() || k > search_bigk_max())
        return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, std::min(search_groups_kmax(), search_bigk_max()));
    if (ix->grp.n_groups <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no grouping set for the rows of the index (vr_index_set_groups)");
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const int ng = (int)ix->grp.n_groups;
    const int64_t ldS = pad256l(ix->n), ldB = (ix->grp.n_groups + 63) / 64 * 64;
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const size_t n_out = (size_t)nq * k;
    float* os = nullptr; int64_t* oi = nullptr; int64_t* og = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(stage_output(ix->grp.out, out_groups, n_out, on_device, &og));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    VRCHK(ix->grp.B.reserve((size_t)qblk * ldB * 4));
    float* S = ix->sbuf.as<float>();
    const bool certify = certifies(ix);
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        GroupSearchArgs p{};
        // (the error model also bounds which rows of a group are re-scored)
        SearchArgs& a = p.a = block_view(ix, q32, q0, nb, k, true);
        a.flag_count = ix->grp.state.as<int>(); a.flag_list = ix->grp.state.as<int>() + GRP_LIST;
        a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k;
        p.goff = ix->grp.off.as<int>(); p.n_groups = ng;
        p.B = ix->grp.B.as<float>(); p.ldB = (size_t)ldB;
        p.out_groups = og + (size_t)q0 * k;
        p.stats = ix->grp.state.as<unsigned>() + GRP_STATS;
        p.certify = certify ? 1 : 0;
        VRCHK(score_block(ix, q32, q0, nb, ldS, a.flag_count, s));         // (also clears the grouped search's flag counter)
        HIPCHK(launch_group_max(S, (size_t)ldS, p.goff, ng, p.B, p.ldB, nb, nullptr, 0, s));
        HIPCHK(launch_group_select(p, S, (size_t)ldS, nb, s));
        if (certify) {
            // whatever the select flagged (nothing, normally: the three kernels leave at once): exact fp32 score rows
            HIPCHK(launch_exact_scores(a.index_f32, a.n_docs, a.dim, a.q_f32, a.flag_list, a.flag_count, 0, nb, S, (size_t)ldS, s));
            HIPCHK(launch_group_max(S, (size_t)ldS, p.goff, ng, p.B, p.ldB, nb, a.flag_count, 0, s));
            HIPCHK(launch_group_select_exact(p, S, (size_t)ldS, 0, nb, s));
        }
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    VRCHK(return_output(out_groups, og, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- filtered search (search_filter.hip) --------------------------------------------------------------------------------------
extern "C" int vr_index_set_filters(vr_index_t ix, const uint32_t* bits, int32_t n_filters, int32_t on_device, void* stream) {
    if (!ix || !bits) return fail(VR_ERR_INVALID, "NULL argument");
    if (n_filters < 1) return fail(VR_ERR_INVALID, "%d filters", (int)n_filters);
    if (ix->n <= 0) return fail(VR_ERR_INVALID, "filters over an empty index");
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());               // (a filtered search in flight reads the filters)
    hipStream_t s = (hipStream_t)stream;
    const size_t words = (size_t)((ix->n + 31) / 32), total = words * (size_t)n_filters;
    ix->flt.n_filters = 0;
    VRCHK(ix->flt.bits.reserve(total * 4));
    VRCHK(ix->flt.count.reserve((size_t)n_filters * 4));
    if (!ix->flt.state.p) VRCHK(ix->flt.state.alloc(FLT_WORDS * 4));
    HIPCHK(hipMemcpyAsync(ix->flt.bits.p, bits, total * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    // the caller's bits at or beyond the row count are garbage: cleared in the copy; allowed rows per filter counted once, here
    HIPCHK(launch_filter_prepare(ix->flt.bits.as<uint32_t>(), words, n_filters, ix->n, ix->flt.count.as<int>(), s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    ix->flt.n_filters = n_filters;
    return VR_OK;
}

extern "C" int vr_index_filter_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned, 3>(ix, ix->flt.state, FLT_STATS, out3, reset);
}

// The k best rows per query among the rows its filter allows: filters, flag list and counters are the filtered search's own.
extern "C" int vr_index_search_filtered(vr_index_t ix, const float* queries, int32_t nq, int32_t k, const int32_t* filter_of_query,
                                        float* out_scores, int64_t* out_ids, int32_t on_device, void* stream) {
    if (!ix || !queries || !filter_of_query || !out_scores || !out_ids || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t ldS = pad256l(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const int* foq = nullptr;
    VRCHK(stage_input(ix->flt.ids, filter_of_query, (size_t)nq, on_device, s, &foq));
    const size_t n_out = (size_t)nq * k;
    float* os = nullptr; int64_t* oi = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    float* S = ix->sbuf.as<float>();
    const bool certify = certifies(ix);
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        FilterSearchArgs p{};
        SearchArgs& a = p.a = block_view(ix, q32, q0, nb, k, false);
        a.flag_count = ix->flt.state.as<int>(); a.flag_list = ix->flt.state.as<int>() + FLT_LIST;
        a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k;
        p.bits = ix->flt.bits.as<uint32_t>(); p.words = (size_t)((ix->n + 31) / 32); p.n_filters = (int)ix->flt.n_filters;
        p.allowed = ix->flt.count.as<int>();
        p.filter_of_query = foq + q0;
        p.stats = ix->flt.state.as<unsigned>() + FLT_STATS;
        p.certify = certify ? 1 : 0;
        VRCHK(score_block(ix, q32, q0, nb, ldS, a.flag_count, s));         // (also clears the filtered search's flag counter)
        VRCHK(mask_block(ix, foq + q0, nb, ldS, nullptr, nullptr, 0, s));
        HIPCHK(launch_filter_select(p, S, (size_t)ldS, nb, s));
        if (certify) {
            // whatever the select flagged (nothing, normally: the three kernels leave at once): exact fp32 score rows, masked
            HIPCHK(launch_exact_scores(a.index_f32, a.n_docs, a.dim, a.q_f32, a.flag_list, a.flag_count, 0, nb, S, (size_t)ldS, s));
            VRCHK(mask_block(ix, foq + q0, nb, ldS, a.flag_list, a.flag_count, 0, s));
            HIPCHK(launch_filter_select_exact(p, S, (size_t)ldS, 0, nb, s));
        }
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- range search (search_range.hip) ------------------------------------------------------------------------------------------
extern "C" int vr_index_range_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->rng.state, 0, out3, reset);
}

// room for `need` entries of the range result, the first `keep` of which are kept (what earlier blocks of the call packed)
static int range_reserve(vr_index_t ix, int64_t need, int64_t keep, int64_t max_total, hipStream_t s) {
    if (need <= ix->rng.cap && ix->rng.scores.p && ix->rng.ids.p) return VR_OK;
    const int64_t cap = std::max<int64_t>(std::min(max_total, std::max(need, 2 * ix->rng.cap)), std::max<int64_t>(need, 1));
    DevBuf ns, ni;
    VRCHK(ns.reserve((size_t)cap * 4));
    VRCHK(ni.reserve((size_t)cap * 8));
    if (keep > 0) {
        HIPCHK(hipMemcpyAsync(ns.p, ix->rng.scores.p, (size_t)keep * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ni.p, ix->rng.ids.p, (size_t)keep * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    ix->rng.scores = std::move(ns);
    ix->rng.ids = std::move(ni);
    ix->rng.cap = cap;
    return VR_OK;
}

// Every row at or above a query's threshold: result, counts, offsets and counters are the range search's own.
extern "C" int vr_index_search_range(vr_index_t ix, const float* queries, int32_t nq, const float* thresholds,
                                     const int32_t* filter_of_query, int64_t max_total, int64_t* out_lims, int64_t* total,
                                     int32_t on_device, void* stream) {
    if (!ix || !queries || !thresholds || !out_lims || !total || nq < 1) return fail(VR_ERR_INVALID, "bad arguments");
    if (max_total < 1) return fail(VR_ERR_INVALID, "max_total=%lld must be at least 1", (long long)max_total);
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (!on_device)
        for (int32_t q = 0; q < nq; ++q)
            if (!std::isfinite(thresholds[q])) return fail(VR_ERR_INVALID, "thresholds[%d] = %g is not finite", (int)q, (double)thresholds[q]);
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
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
        ix->rng.total = 0;
        return VR_OK;
    }
    if (!ix->rng.state.p) VRCHK(ix->rng.state.alloc(RNG_WORDS * 8));
    if (!ix->rng.host_total && hipHostMalloc((void**)&ix->rng.host_total, 64, hipHostMallocDefault) != hipSuccess) {
        ix->rng.host_total = nullptr;
        return fail(VR_ERR_HIP, "hipHostMalloc");
    }
    ix->rng.total = -1;                           // from here on the previous result is gone
    const int64_t ldS = pad256l(ix->n), slots = range_scan_slots(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const float* thr = nullptr;
    const int* foq = nullptr;
    int64_t* lims = nullptr;
    VRCHK(stage_input(ix->rng.thr, thresholds, (size_t)nq, on_device, s, &thr));
    if (filter_of_query) VRCHK(stage_input(ix->flt.ids, filter_of_query, (size_t)nq, on_device, s, &foq));
    VRCHK(stage_output(ix->rng.lims, out_lims, (size_t)nq + 1, on_device, &lims));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    VRCHK(ix->rng.cnt.reserve((size_t)qblk * slots * 4));
    VRCHK(ix->rng.off.reserve((size_t)qblk * slots * 4));
    VRCHK(range_reserve(ix, std::min<int64_t>(max_total, 65536), 0, max_total, s));
    float* S = ix->sbuf.as<float>();
    int64_t* block_total = ix->rng.state.as<int64_t>() + RNG_TOTAL;
    int64_t base = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        RangeSearchArgs p{};
        p.a = block_view(ix, q32, q0, nb, 1, true);                        // (the band is defined by the error model)
        p.thresholds = thr + q0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->flt.n_filters;
        p.stats = ix->rng.state.as<unsigned long long>();
        VRCHK(score_block(ix, q32, q0, nb, ldS, nullptr, s));
        if (foq) VRCHK(mask_block(ix, foq + q0, nb, ldS, nullptr, nullptr, 0, s));
        HIPCHK(launch_range_rescore(p, S, (size_t)ldS, nb, ix->rng.cnt.as<int>(), s));
        HIPCHK(launch_range_scan(ix->rng.cnt.as<int>(), ix->rng.off.as<int>(), ix->n, nb, base, q0 == 0 ? 1 : 0, lims + q0, block_total, s));
        // the size of the block's result is a host value: capacity check, growth of the result arrays
        HIPCHK(hipMemcpyAsync(ix->rng.host_total, block_total, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int64_t bt = *ix->rng.host_total;
        if (bt < 0 || base + bt > max_total)
            return fail(VR_ERR_CAPACITY, "range result exceeds max_total=%lld in query block %lld (queries %lld..%lld): %lld entries by then",
                        (long long)max_total, (long long)(q0 / qblk), (long long)q0, (long long)(q0 + nb - 1), (long long)(base + bt));
        VRCHK(range_reserve(ix, base + bt, base, max_total, s));
        p.out_scores = ix->rng.scores.as<float>(); p.out_ids = ix->rng.ids.as<int64_t>();
        if (bt > 0)
            HIPCHK(launch_range_pack(p, S, (size_t)ldS, nb, ix->rng.cnt.as<int>(), ix->rng.off.as<int>(), lims + q0, s));
        base += bt;
    }
    VRCHK(return_output(out_lims, lims, (size_t)nq + 1, on_device, s));
    HIPCHK(hipStreamSynchronize(s));
    *total = base;
    ix->rng.total = base;
    return VR_OK;
}

extern "C" int vr_index_range_results(vr_index_t ix, float* out_scores, int64_t* out_ids, int64_t n, int32_t on_device, void* stream) {
    if (!ix || n < 0 || (n > 0 && (!out_scores || !out_ids))) return fail(VR_ERR_INVALID, "bad arguments");
    if (ix->rng.total < 0) return fail(VR_ERR_STATE, "no range result (vr_index_search_range)");
    if (n > ix->rng.total) return fail(VR_ERR_STATE, "%lld entries asked for, the last range search found %lld", (long long)n, (long long)ix->rng.total);
    if (n == 0) return VR_OK;
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(out_scores, ix->rng.scores.p, (size_t)n * 4, kind, s));
    HIPCHK(hipMemcpyAsync(out_ids, ix->rng.ids.p, (size_t)n * 8, kind, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- rank search (search_rank.hip) --------------------------------------------------------------------------------------------
extern "C" int vr_index_rank_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->rnk.state, 0, out3, reset);
}

// What vr_index_rank_rows (ids set) and vr_index_count_range (thresholds set) share: per block the bars of the block's pairs
// and their counts; a block without pairs is skipped.  Nothing is stored.
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
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    if (np == 0) return VR_OK;                    // no pair: no launch
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    if (ix->n == 0) {                             // (counts only: a target row would have been out of range) no row: no launch
        if (on_device) HIPCHK(hipMemsetAsync(out_counts, 0, (size_t)np * 8, s));
        else std::fill(out_counts, out_counts + np, (int64_t)0);
        return VR_OK;
    }
    if (!ix->rnk.state.p) VRCHK(ix->rnk.state.alloc(RNK_WORDS * 8));
    const int64_t ldS = pad256l(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const int* foq = nullptr;
    if (filter_of_query) VRCHK(stage_input(ix->flt.ids, filter_of_query, (size_t)nq, on_device, s, &foq));
    // the pairs: their query inside its block and their target row or threshold, 4 bytes each
    std::vector<int> pq((size_t)np), pv(ids ? (size_t)np : 0);
    for (int32_t q = 0; q < nq; ++q)
        for (int64_t i = lims[q]; i < lims[q + 1]; ++i) pq[(size_t)i] = (int)(q % qblk);
    if (ids) for (int64_t i = 0; i < np; ++i) pv[(size_t)i] = (int)ids[i];
    VRCHK(ix->rnk.q.reserve((size_t)np * 4));
    VRCHK(ix->rnk.v.reserve((size_t)np * 4));
    VRCHK(ix->rnk.bar.reserve((size_t)np * 8));
    VRCHK(ix->rnk.eps.reserve((size_t)np * 4));
    HIPCHK(hipMemcpyAsync(ix->rnk.q.p, pq.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ix->rnk.v.p, ids ? (const void*)pv.data() : (const void*)thresholds, (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));              // (the host arrays are free from here on)
    float* os = nullptr; int64_t* oc = nullptr;
    if (ids) VRCHK(stage_output(ix->os, out_scores, (size_t)np, on_device, &os));
    VRCHK(stage_output(ix->oi, out_counts, (size_t)np, on_device, &oc));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        const int64_t p0 = lims[q0], pn = lims[q0 + nb] - p0;
        if (pn == 0) continue;                    // a block without pairs: no launch
        RankSearchArgs p{};
        p.a = block_view(ix, q32, q0, nb, 1, true);                        // (the band is defined by the error model)
        p.pair_query = ix->rnk.q.as<int>() + p0;
        p.pair_id = ids ? ix->rnk.v.as<int>() + p0 : nullptr;
        p.pair_thr = ids ? nullptr : ix->rnk.v.as<float>() + p0;
        p.strict = strict ? 1 : 0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->flt.n_filters;
        p.bars = ix->rnk.bar.as<unsigned long long>() + p0;
        p.bar_eps = ix->rnk.eps.as<float>() + p0;
        p.out_scores = ids ? os + p0 : nullptr;
        p.out_counts = reinterpret_cast<unsigned long long*>(oc) + p0;
        p.stats = ix->rnk.state.as<unsigned long long>();
        VRCHK(score_block(ix, q32, q0, nb, ldS, nullptr, s));
        if (foq) VRCHK(mask_block(ix, foq + q0, nb, ldS, nullptr, nullptr, 0, s));
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

// ---- document rank search (search_group_rank.hip) -----------------------------------------------------------------------------
extern "C" int vr_index_group_rank_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->grnk.state, 0, out3, reset);
}

// What vr_index_rank_groups (groups set) and vr_index_count_groups_range (thresholds set) share: per block with pairs the
// (masked) score rows, their group maxima, the bars of the block's pairs and their counts.  Pairs, bars, group maxima and
// counters are the search's own; the grouping and the filters are read.  Nothing is stored.
static int group_rank_impl(vr_index_t ix, bool ranks, const float* queries, int32_t nq, const int64_t* lims, const int64_t* groups,
                           const float* thresholds, int32_t strict, const int32_t* filter_of_query, float* out_scores,
                           int64_t* out_rows, int64_t* out_counts, int32_t on_device, void* stream) {
    if (!ix || !lims || nq < 0 || (nq > 0 && !queries)) return fail(VR_ERR_INVALID, "bad arguments");
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (lims[0] != 0) return fail(VR_ERR_INVALID, "lims[0] = %lld must be 0", (long long)lims[0]);
    for (int32_t q = 0; q < nq; ++q)
        if (lims[q + 1] < lims[q]) return fail(VR_ERR_INVALID, "lims[%d] = %lld decreases", (int)q + 1, (long long)lims[q + 1]);
    const int64_t np = lims[nq];
    if (np >= ((int64_t)1 << 31)) return fail(VR_ERR_INVALID, "%lld pairs: too many for one call", (long long)np);
    if (np > 0 && (!out_counts || (ranks ? !groups || !out_scores || !out_rows : !thresholds))) return fail(VR_ERR_INVALID, "bad arguments");
    if (ix->grp.n_groups <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no grouping set for the rows of the index (vr_index_set_groups)");
    if (ranks) {
        for (int64_t i = 0; i < np; ++i)
            if (groups[i] < 0 || groups[i] >= ix->grp.n_groups)
                return fail(VR_ERR_INVALID, "groups[%lld] = %lld outside [0, %lld)", (long long)i, (long long)groups[i], (long long)ix->grp.n_groups);
    } else {
        for (int64_t i = 0; i < np; ++i)
            if (!std::isfinite(thresholds[i])) return fail(VR_ERR_INVALID, "thresholds[%lld] = %g is not finite", (long long)i, (double)thresholds[i]);
    }
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    if (np == 0) return VR_OK;                    // no pair: no launch
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    if (!ix->grnk.state.p) VRCHK(ix->grnk.state.alloc(GRNK_WORDS * 8));
    const int ng = (int)ix->grp.n_groups;
    const int64_t ldS = pad256l(ix->n), ldB = (ix->grp.n_groups + 63) / 64 * 64;
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const int* foq = nullptr;
    if (filter_of_query) VRCHK(stage_input(ix->flt.ids, filter_of_query, (size_t)nq, on_device, s, &foq));
    // the pairs: their query inside its block and their target group or threshold, 4 bytes each
    std::vector<int> pq((size_t)np), pv(ranks ? (size_t)np : 0);
    for (int32_t q = 0; q < nq; ++q)
        for (int64_t i = lims[q]; i < lims[q + 1]; ++i) pq[(size_t)i] = (int)(q % qblk);
    if (ranks) for (int64_t i = 0; i < np; ++i) pv[(size_t)i] = (int)groups[i];
    VRCHK(ix->grnk.q.reserve((size_t)np * 4));
    VRCHK(ix->grnk.v.reserve((size_t)np * 4));
    VRCHK(ix->grnk.bar.reserve((size_t)np * 8));
    VRCHK(ix->grnk.eps.reserve((size_t)np * 4));
    HIPCHK(hipMemcpyAsync(ix->grnk.q.p, pq.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ix->grnk.v.p, ranks ? (const void*)pv.data() : (const void*)thresholds, (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));              // (the host arrays are free from here on)
    float* os = nullptr; int64_t* orow = nullptr; int64_t* oc = nullptr;
    if (ranks) {
        VRCHK(stage_output(ix->os, out_scores, (size_t)np, on_device, &os));
        VRCHK(stage_output(ix->oi, out_rows, (size_t)np, on_device, &orow));
    }
    VRCHK(stage_output(ix->grnk.out, out_counts, (size_t)np, on_device, &oc));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    VRCHK(ix->grnk.B.reserve((size_t)qblk * ldB * 4));
    float* S = ix->sbuf.as<float>();
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        const int64_t p0 = lims[q0], pn = lims[q0 + nb] - p0;
        if (pn == 0) continue;                    // a block without pairs: no launch
        GroupRankArgs p{};
        p.a = block_view(ix, q32, q0, nb, 1, true);                        // (the band is defined by the error model)
        p.goff = ix->grp.off.as<int>(); p.n_groups = ng;
        p.B = ix->grnk.B.as<float>(); p.ldB = (size_t)ldB;
        p.pair_query = ix->grnk.q.as<int>() + p0;
        p.pair_group = ranks ? ix->grnk.v.as<int>() + p0 : nullptr;
        p.pair_thr = ranks ? nullptr : ix->grnk.v.as<float>() + p0;
        p.strict = strict ? 1 : 0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->flt.n_filters;
        p.bars = ix->grnk.bar.as<unsigned long long>() + p0;
        p.bar_eps = ix->grnk.eps.as<float>() + p0;
        p.out_scores = ranks ? os + p0 : nullptr;
        p.out_rows = ranks ? reinterpret_cast<long long*>(orow) + p0 : nullptr;
        p.out_counts = reinterpret_cast<unsigned long long*>(oc) + p0;
        p.stats = ix->grnk.state.as<unsigned long long>();
        VRCHK(score_block(ix, q32, q0, nb, ldS, nullptr, s));
        if (foq) VRCHK(mask_block(ix, foq + q0, nb, ldS, nullptr, nullptr, 0, s));
        HIPCHK(launch_group_max(S, (size_t)ldS, p.goff, ng, ix->grnk.B.as<float>(), p.ldB, nb, nullptr, 0, s));
        HIPCHK(launch_group_rank_bars(p, S, (size_t)ldS, nb, pn, s));
        HIPCHK(launch_group_rank_count(p, S, (size_t)ldS, nb, pn, s));
    }
    if (ranks) {
        VRCHK(return_output(out_scores, os, (size_t)np, on_device, s));
        VRCHK(return_output(out_rows, orow, (size_t)np, on_device, s));
    }
    VRCHK(return_output(out_counts, oc, (size_t)np, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_index_rank_groups(vr_index_t ix, const float* queries, int32_t nq, const int64_t* lims, const int64_t* groups,
                                    const int32_t* filter_of_query, float* out_scores, int64_t* out_rows, int64_t* out_ranks,
                                    int32_t on_device, void* stream) {
    return group_rank_impl(ix, true, queries, nq, lims, groups, nullptr, 0, filter_of_query, out_scores, out_rows, out_ranks, on_device, stream);
}

extern "C" int vr_index_count_groups_range(vr_index_t ix, const float* queries, int32_t nq, const int64_t* lims,
                                           const float* thresholds, int32_t strict, const int32_t* filter_of_query,
                                           int64_t* out_counts, int32_t on_device, void* stream) {
    return group_rank_impl(ix, false, queries, nq, lims, nullptr, thresholds, strict, filter_of_query, nullptr, nullptr, out_counts, on_device,
                           stream);
}

// ---- document range search (search_group_range.hip) ---------------------------------------------------------------------------
extern "C" int vr_index_group_range_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->grng.state, 0, out3, reset);
}

// room for `need` entries of the document range result, the first `keep` of which are kept (what earlier blocks of the call packed)
static int group_range_reserve(vr_index_t ix, int64_t need, int64_t keep, int64_t max_total, hipStream_t s) {
    if (need <= ix->grng.cap && ix->grng.scores.p && ix->grng.rows.p && ix->grng.groups.p) return VR_OK;
    const int64_t cap = std::max<int64_t>(std::min(max_total, std::max(need, 2 * ix->grng.cap)), std::max<int64_t>(need, 1));
    DevBuf ns, nr, ng;
    VRCHK(ns.reserve((size_t)cap * 4));
    VRCHK(nr.reserve((size_t)cap * 8));
    VRCHK(ng.reserve((size_t)cap * 8));
    if (keep > 0) {
        HIPCHK(hipMemcpyAsync(ns.p, ix->grng.scores.p, (size_t)keep * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(nr.p, ix->grng.rows.p, (size_t)keep * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ng.p, ix->grng.groups.p, (size_t)keep * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    ix->grng.scores = std::move(ns);
    ix->grng.rows = std::move(nr);
    ix->grng.groups = std::move(ng);
    ix->grng.cap = cap;
    return VR_OK;
}

// Every document at or above a query's threshold, under its filter: result, group maxima, best rows, counts, offsets and counters
// are the document range search's own; the grouping and the filters are read.
extern "C" int vr_index_search_groups_range(vr_index_t ix, const float* queries, int32_t nq, const float* thresholds,
                                            const int32_t* filter_of_query, int64_t max_total, int64_t* out_lims, int64_t* total,
                                            int32_t on_device, void* stream) {
    if (!ix || !queries || !thresholds || !out_lims || !total || nq < 1) return fail(VR_ERR_INVALID, "bad arguments");
    if (max_total < 1) return fail(VR_ERR_INVALID, "max_total=%lld must be at least 1", (long long)max_total);
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (!on_device)
        for (int32_t q = 0; q < nq; ++q)
            if (!std::isfinite(thresholds[q])) return fail(VR_ERR_INVALID, "thresholds[%d] = %g is not finite", (int)q, (double)thresholds[q]);
    if (ix->n > 0 && ix->grp.n_groups <= 0) return fail(VR_ERR_STATE, "no grouping set for the rows of the index (vr_index_set_groups)");
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    if (ix->n == 0) {                             // no row, no document: no launch
        if (on_device) {
            HIPCHK(hipMemsetAsync(out_lims, 0, ((size_t)nq + 1) * 8, s));
            HIPCHK(hipStreamSynchronize(s));
        } else {
            std::fill(out_lims, out_lims + nq + 1, (int64_t)0);
        }
        *total = 0;
        ix->grng.total = 0;
        return VR_OK;
    }
    if (!ix->grng.state.p) VRCHK(ix->grng.state.alloc(GRNG_WORDS * 8));
    if (!ix->grng.host_total && hipHostMalloc((void**)&ix->grng.host_total, 64, hipHostMallocDefault) != hipSuccess) {
        ix->grng.host_total = nullptr;
        return fail(VR_ERR_HIP, "hipHostMalloc");
    }
    ix->grng.total = -1;                          // from here on the previous result is gone
    const int ng = (int)ix->grp.n_groups;
    const int64_t ldS = pad256l(ix->n), ldB = (ix->grp.n_groups + 63) / 64 * 64, slots = range_scan_slots(ix->grp.n_groups);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const float* thr = nullptr;
    const int* foq = nullptr;
    int64_t* lims = nullptr;
    VRCHK(stage_input(ix->grng.thr, thresholds, (size_t)nq, on_device, s, &thr));
    if (filter_of_query) VRCHK(stage_input(ix->flt.ids, filter_of_query, (size_t)nq, on_device, s, &foq));
    VRCHK(stage_output(ix->grng.lims, out_lims, (size_t)nq + 1, on_device, &lims));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    VRCHK(ix->grng.B.reserve((size_t)qblk * ldB * 4));
    VRCHK(ix->grng.R.reserve((size_t)qblk * ldB * 4));
    VRCHK(ix->grng.cnt.reserve((size_t)qblk * slots * 4));
    VRCHK(ix->grng.off.reserve((size_t)qblk * slots * 4));
    VRCHK(group_range_reserve(ix, std::min<int64_t>(max_total, 65536), 0, max_total, s));
    float* S = ix->sbuf.as<float>();
    int64_t* block_total = ix->grng.state.as<int64_t>() + GRNG_TOTAL;
    int64_t base = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        GroupRangeArgs p{};
        p.a = block_view(ix, q32, q0, nb, 1, true);                        // (the band is defined by the error model)
        p.goff = ix->grp.off.as<int>(); p.n_groups = ng;
        p.B = ix->grng.B.as<float>(); p.ldB = (size_t)ldB;
        p.R = ix->grng.R.as<int>();
        p.thresholds = thr + q0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->flt.n_filters;
        p.stats = ix->grng.state.as<unsigned long long>();
        VRCHK(score_block(ix, q32, q0, nb, ldS, nullptr, s));
        if (foq) VRCHK(mask_block(ix, foq + q0, nb, ldS, nullptr, nullptr, 0, s));
        HIPCHK(launch_group_max(S, (size_t)ldS, p.goff, ng, p.B, p.ldB, nb, nullptr, 0, s));
        HIPCHK(launch_group_range_rescore(p, S, (size_t)ldS, nb, ix->grng.cnt.as<int>(), s));
        HIPCHK(launch_range_scan(ix->grng.cnt.as<int>(), ix->grng.off.as<int>(), ix->grp.n_groups, nb, base, q0 == 0 ? 1 : 0, lims + q0,
                                 block_total, s));
        // the size of the block's result is a host value: capacity check, growth of the result arrays
        HIPCHK(hipMemcpyAsync(ix->grng.host_total, block_total, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int64_t bt = *ix->grng.host_total;
        if (bt < 0 || base + bt > max_total)
            return fail(VR_ERR_CAPACITY,
                        "document range result exceeds max_total=%lld in query block %lld (queries %lld..%lld): %lld entries by then",
                        (long long)max_total, (long long)(q0 / qblk), (long long)q0, (long long)(q0 + nb - 1), (long long)(base + bt));
        VRCHK(group_range_reserve(ix, base + bt, base, max_total, s));
        p.out_scores = ix->grng.scores.as<float>(); p.out_rows = ix->grng.rows.as<int64_t>(); p.out_groups = ix->grng.groups.as<int64_t>();
        if (bt > 0)
            HIPCHK(launch_group_range_pack(p, nb, ix->grng.cnt.as<int>(), ix->grng.off.as<int>(), lims + q0, s));
        base += bt;
    }
    VRCHK(return_output(out_lims, lims, (size_t)nq + 1, on_device, s));
    HIPCHK(hipStreamSynchronize(s));
    *total = base;
    ix->grng.total = base;
    return VR_OK;
}

extern "C" int vr_index_group_range_results(vr_index_t ix, float* out_scores, int64_t* out_rows, int64_t* out_groups, int64_t n,
                                            int32_t on_device, void* stream) {
    if (!ix || n < 0 || (n > 0 && (!out_scores || !out_rows || !out_groups))) return fail(VR_ERR_INVALID, "bad arguments");
    if (ix->grng.total < 0) return fail(VR_ERR_STATE, "no document range result (vr_index_search_groups_range)");
    if (n > ix->grng.total)
        return fail(VR_ERR_STATE, "%lld entries asked for, the last document range search found %lld", (long long)n, (long long)ix->grng.total);
    if (n == 0) return VR_OK;
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(out_scores, ix->grng.scores.p, (size_t)n * 4, kind, s));
    HIPCHK(hipMemcpyAsync(out_rows, ix->grng.rows.p, (size_t)n * 8, kind, s));
    HIPCHK(hipMemcpyAsync(out_groups, ix->grng.groups.p, (size_t)n * 8, kind, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- windowed search (search_window.hip) --------------------------------------------------------------------------------------
extern "C" int vr_index_window_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->win.state, 0, out3, reset);
}

// The rows at ranks [offsets[q], offsets[q] + k) of every query's fp32 ranking: per block the band edges, the rewritten rows
// and the select.  Nothing is stored.
extern "C" int vr_index_search_window(vr_index_t ix, const float* queries, int32_t nq, const int64_t* offsets, int32_t k,
                                      const int32_t* filter_of_query, float* out_scores, int64_t* out_ids, int32_t on_device,
                                      void* stream) {
    if (!ix || nq < 0 || (nq > 0 && (!queries || !offsets || !out_scores || !out_ids))) return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    for (int32_t q = 0; q < nq; ++q)
        if (offsets[q] < 0) return fail(VR_ERR_INVALID, "offsets[%d] = %lld is negative", (int)q, (long long)offsets[q]);
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    if (nq == 0) return VR_OK;                    // no query: no launch
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)nq * k;
    if (ix->n == 0) return fill_tails(out_scores, out_ids, nullptr, n_out, on_device, s);      // no row: tails, no launch
    if (!ix->win.state.p) VRCHK(ix->win.state.alloc(WIN_WORDS * 8));
    const int64_t ldS = pad256l(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const int* foq = nullptr;
    if (filter_of_query) VRCHK(stage_input(ix->flt.ids, filter_of_query, (size_t)nq, on_device, s, &foq));
    const int64_t* off = nullptr;                 // (a host array whoever calls)
    VRCHK(stage_input(ix->win.off, offsets, (size_t)nq, 0, s, &off));
    VRCHK(ix->win.edge.reserve((size_t)qblk * 8));
    HIPCHK(hipStreamSynchronize(s));              // (the host array is free from here on)
    float* os = nullptr; int64_t* oi = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    float* S = ix->sbuf.as<float>();
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        WindowSearchArgs p{};
        p.a = block_view(ix, q32, q0, nb, k, true);                        // (the band is defined by the error model)
        p.a.out_scores = os + (size_t)q0 * k; p.a.out_ids = oi + (size_t)q0 * k;
        p.offsets = off + q0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->flt.n_filters;
        p.allowed = foq ? ix->flt.count.as<int>() : nullptr;
        p.edges = ix->win.edge.as<float>();
        p.stats = ix->win.state.as<unsigned long long>();
        VRCHK(score_block(ix, q32, q0, nb, ldS, nullptr, s));
        if (foq) VRCHK(mask_block(ix, foq + q0, nb, ldS, nullptr, nullptr, 0, s));
        HIPCHK(launch_window_edges(p, S, (size_t)ldS, nb, s));
        HIPCHK(launch_window_rescore(p, S, (size_t)ldS, nb, s));
        HIPCHK(launch_window_select(p, S, (size_t)ldS, nb, s));
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- document window search (search_group_window.hip) -------------------------------------------------------------------------
extern "C" int vr_index_group_window_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->gwin.state, 0, out3, reset);
}

// The groups at ranks [offsets[q], offsets[q] + k) of every query's document ranking under its filter: per block the (masked)
// score rows, their group maxima, the band edges, the rewritten maxima and the select.  Group maxima, best rows and counters are
// the search's own; the grouping and the filters are read.  Nothing is stored.
extern "C" int vr_index_search_groups_window(vr_index_t ix, const float* queries, int32_t nq, const int64_t* offsets, int32_t k,
                                             const int32_t* filter_of_query, float* out_scores, int64_t* out_ids,
                                             int64_t* out_groups, int32_t on_device, void* stream) {
    if (!ix || nq < 0 || (nq > 0 && (!queries || !offsets || !out_scores || !out_ids || !out_groups)))
        return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    for (int32_t q = 0; q < nq; ++q)
        if (offsets[q] < 0) return fail(VR_ERR_INVALID, "offsets[%d] = %lld is negative", (int)q, (long long)offsets[q]);
    if (ix->grp.n_groups <= 0 || ix->n <= 0) return fail(VR_ERR_STATE, "no grouping set for the rows of the index (vr_index_set_groups)");
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    if (nq == 0) return VR_OK;                    // no query: no launch
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)nq * k;
    if (!ix->gwin.state.p) VRCHK(ix->gwin.state.alloc(GWIN_WORDS * 8));
    const int ng = (int)ix->grp.n_groups;
    const int64_t ldS = pad256l(ix->n), ldB = (ix->grp.n_groups + 63) / 64 * 64;
    const int64_t qblk = 256;                     // one fp32 score row per query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, qblk)), on_device, s, &q32));
    const int* foq = nullptr;
    if (filter_of_query) VRCHK(stage_input(ix->flt.ids, filter_of_query, (size_t)nq, on_device, s, &foq));
    const int64_t* off = nullptr;                 // (a host array whoever calls)
    VRCHK(stage_input(ix->gwin.off, offsets, (size_t)nq, 0, s, &off));
    VRCHK(ix->gwin.edge.reserve((size_t)qblk * 12));
    HIPCHK(hipStreamSynchronize(s));              // (the host array is free from here on)
    float* os = nullptr; int64_t* oi = nullptr; int64_t* og = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(stage_output(ix->gwin.out, out_groups, n_out, on_device, &og));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    VRCHK(ix->gwin.B.reserve((size_t)qblk * ldB * 4));
    VRCHK(ix->gwin.R.reserve((size_t)qblk * ldB * 4));
    float* S = ix->sbuf.as<float>();
    for (int64_t q0 = 0; q0 < nq; q0 += qblk) {
        const int nb = (int)std::min<int64_t>(qblk, nq - q0);
        GroupWindowArgs p{};
        p.a = block_view(ix, q32, q0, nb, k, true);                        // (the band is defined by the error model)
        p.a.out_scores = os + (size_t)q0 * k; p.a.out_ids = oi + (size_t)q0 * k;
        p.out_groups = og + (size_t)q0 * k;
        p.goff = ix->grp.off.as<int>(); p.n_groups = ng;
        p.B = ix->gwin.B.as<float>(); p.ldB = (size_t)ldB;
        p.R = ix->gwin.R.as<int>();
        p.offsets = off + q0;
        p.filter_of_query = foq ? foq + q0 : nullptr;
        p.n_filters = (int)ix->flt.n_filters;
        p.edges = ix->gwin.edge.as<float>();
        p.present = ix->gwin.edge.as<int>() + 2 * qblk;
        p.stats = ix->gwin.state.as<unsigned long long>();
        VRCHK(score_block(ix, q32, q0, nb, ldS, nullptr, s));
        if (foq) VRCHK(mask_block(ix, foq + q0, nb, ldS, nullptr, nullptr, 0, s));
        HIPCHK(launch_group_max(S, (size_t)ldS, p.goff, ng, p.B, p.ldB, nb, nullptr, 0, s));
        HIPCHK(launch_group_window_edges(p, nb, s));
        HIPCHK(launch_group_window_rescore(p, S, (size_t)ldS, nb, s));
        HIPCHK(launch_group_window_select(p, nb, s));
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    VRCHK(return_output(out_groups, og, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- fused search (search_multi.hip) ------------------------------------------------------------------------------------------
extern "C" int vr_index_multi_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->mul.state, 0, out3, reset);
}

// The k rows of largest fused score of every group of sub-queries: whole groups packed greedily into blocks of <= 256
// sub-queries, and per block the fusion, the band edges, the rewritten fused rows and the select.  Nothing is stored.
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
    if (filter_of_group) VRCHK(check_filter_ids(ix, filter_of_group, n_groups, on_device, "filter_of_group"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)n_groups * k;
    if (ix->n == 0) return fill_tails(out_scores, out_ids, out_which, n_out, on_device, s);    // no row: tails, no launch
    if (!ix->mul.state.p) VRCHK(ix->mul.state.alloc(MUL_WORDS * 8));
    const int64_t ldS = pad256l(ix->n);
    const int64_t qblk = 256;                     // one fp32 score row per sub-query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, n_sub, pad256l(std::min<int64_t>(n_sub, qblk)), on_device, s, &q32));
    std::vector<int> lims32((size_t)n_groups + 1);
    for (int32_t g = 0; g <= n_groups; ++g) lims32[g] = (int)lims[g];
    const int* glims = nullptr;
    VRCHK(stage_input(ix->mul.lims, lims32.data(), lims32.size(), 0, s, &glims));
    VRCHK(ix->mul.edge.reserve((size_t)qblk * 4));
    const int* fog = nullptr;
    if (filter_of_group) {                        // the group's filter for every one of its score rows: what the mask reads
        VRCHK(stage_input(ix->flt.ids, filter_of_group, (size_t)n_groups, on_device, s, &fog));
        VRCHK(ix->mul.fsub.reserve((size_t)n_sub * 4));
        HIPCHK(launch_multi_expand(glims, fog, n_groups, ix->mul.fsub.as<int>(), s));
    }
    HIPCHK(hipStreamSynchronize(s));              // (the host arrays are free from here on)
    float* os = nullptr; int64_t* oi = nullptr; int32_t* ow = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(stage_output(ix->mul.which, out_which, n_out, on_device, &ow));
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    float* S = ix->sbuf.as<float>();
    for (int32_t g0 = 0; g0 < n_groups;) {
        int32_t g1 = g0 + 1;                      // whole groups while the block holds <= 256 sub-queries
        while (g1 < n_groups && lims[g1 + 1] - lims[g0] <= qblk) ++g1;
        const int64_t s0 = lims[g0];
        const int nb = (int)(lims[g1] - s0), ng = g1 - g0;
        MultiSearchArgs p{};
        p.a = block_view(ix, q32, s0, nb, k, true);                        // (the band is defined by the error model)
        p.a.out_scores = os + (size_t)g0 * k; p.a.out_ids = oi + (size_t)g0 * k;
        p.out_which = ow + (size_t)g0 * k;
        p.lims = glims + g0;
        p.sub_base = (int)s0;
        p.fuse = fuse;
        p.filter_of_group = fog ? fog + g0 : nullptr;
        p.n_filters = (int)ix->flt.n_filters;
        p.allowed = fog ? ix->flt.count.as<int>() : nullptr;
        p.edges = ix->mul.edge.as<float>();
        p.stats = ix->mul.state.as<unsigned long long>();
        VRCHK(score_block(ix, q32, s0, nb, ldS, nullptr, s));
        if (fog) VRCHK(mask_block(ix, ix->mul.fsub.as<int>() + s0, nb, ldS, nullptr, nullptr, 0, s));
        HIPCHK(launch_multi_fuse(p, S, (size_t)ldS, ng, s));
        HIPCHK(launch_multi_edges(p, S, (size_t)ldS, ng, s));
        HIPCHK(launch_multi_rescore(p, S, (size_t)ldS, ng, s));
        HIPCHK(launch_multi_select(p, S, (size_t)ldS, ng, s));
        g0 = g1;
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    VRCHK(return_output(out_which, ow, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- fused document search (search_multi_group.hip) ---------------------------------------------------------------------------
extern "C" int vr_index_multi_group_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->mgrp.state, 0, out3, reset);
}

// The k documents of largest fused score of every question, with the best page per sub-query: whole questions packed greedily into
// blocks of <= 256 sub-queries, and per block the (masked) score rows, their document maxima, the fusion, the band edges, the
// rewritten fused rows and the select.  Maxima, fused rows and counters are the search's own; the grouping and the filters are
// read.  Nothing is stored.
extern "C" int vr_index_search_multi_groups(vr_index_t ix, const float* queries, int32_t n_sub, const int64_t* lims, int32_t n_groups,
                                            int32_t k, int32_t fuse, const int32_t* filter_of_group, float* out_scores,
                                            int64_t* out_rows, int64_t* out_docs, int32_t* out_which, float* out_ev_scores,
                                            int64_t* out_ev_rows, int32_t on_device, void* stream) {
    if (!ix || n_groups < 0 || n_sub < 0 ||
        (n_groups > 0 && (!queries || !lims || !out_scores || !out_rows || !out_docs || !out_which)))
        return fail(VR_ERR_INVALID, "bad arguments");
    if ((out_ev_scores != nullptr) != (out_ev_rows != nullptr))
        return fail(VR_ERR_INVALID, "the evidence outputs are both NULL or both set");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (fuse != 0 && fuse != 1) return fail(VR_ERR_INVALID, "fuse=%d unsupported (0: max, 1: min)", (int)fuse);
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (n_groups == 0) {
        if (n_sub != 0) return fail(VR_ERR_INVALID, "%d sub-queries in no question", (int)n_sub);
        return VR_OK;                             // no question: no launch
    }
    if (lims[0] != 0) return fail(VR_ERR_INVALID, "lims[0] = %lld, not 0", (long long)lims[0]);
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t m = lims[g + 1] - lims[g];
        if (m < 0) return fail(VR_ERR_INVALID, "lims[%d] = %lld decreases", (int)g + 1, (long long)lims[g + 1]);
        if (m == 0) return fail(VR_ERR_INVALID, "question %d is empty", (int)g);
        if (m > 256) return fail(VR_ERR_INVALID, "question %d holds %lld sub-queries (1..256)", (int)g, (long long)m);
    }
    if (lims[n_groups] != n_sub)
        return fail(VR_ERR_INVALID, "lims[%d] = %lld, not the %d sub-queries", (int)n_groups, (long long)lims[n_groups], (int)n_sub);
    if (filter_of_group) VRCHK(check_filter_ids(ix, filter_of_group, n_groups, on_device, "filter_of_group"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)n_groups * k, n_ev = out_ev_scores ? (size_t)n_sub * k : 0;
    if (ix->n == 0) {                             // no row: tails, no launch
        VRCHK(fill_tails(out_scores, out_rows, out_which, n_out, on_device, s));
        VRCHK(fill_tails(out_scores, out_docs, nullptr, n_out, on_device, s));
        if (n_ev) VRCHK(fill_tails(out_ev_scores, out_ev_rows, nullptr, n_ev, on_device, s));
        return VR_OK;
    }
    if (ix->grp.n_groups <= 0) return fail(VR_ERR_STATE, "no grouping set for the rows of the index (vr_index_set_groups)");
    if (!ix->mgrp.state.p) VRCHK(ix->mgrp.state.alloc(MGRP_WORDS * 8));
    const int nd = (int)ix->grp.n_groups;
    const int64_t ldS = pad256l(ix->n), ldB = (ix->grp.n_groups + 63) / 64 * 64;
    const int64_t qblk = 256;                     // one fp32 score row per sub-query, as on the deep path
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, n_sub, pad256l(std::min<int64_t>(n_sub, qblk)), on_device, s, &q32));
    std::vector<int> lims32((size_t)n_groups + 1);
    for (int32_t g = 0; g <= n_groups; ++g) lims32[g] = (int)lims[g];
    const int* glims = nullptr;
    VRCHK(stage_input(ix->mgrp.lims, lims32.data(), lims32.size(), 0, s, &glims));
    VRCHK(ix->mgrp.edge.reserve((size_t)qblk * 8));
    VRCHK(ix->mgrp.eps.reserve((size_t)qblk * 4));
    const int* fog = nullptr;
    if (filter_of_group) {                        // the question's filter for every one of its score rows: what the mask reads
        VRCHK(stage_input(ix->flt.ids, filter_of_group, (size_t)n_groups, on_device, s, &fog));
        VRCHK(ix->mgrp.fsub.reserve((size_t)n_sub * 4));
        HIPCHK(launch_multi_expand(glims, fog, n_groups, ix->mgrp.fsub.as<int>(), s));
    }
    HIPCHK(hipStreamSynchronize(s));              // (the host arrays are free from here on)
    float* os = nullptr; int64_t* oi = nullptr; int64_t* od = nullptr; int32_t* ow = nullptr; float* es = nullptr; int64_t* er = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_rows, n_out, on_device, &oi));
    VRCHK(stage_output(ix->mgrp.docs, out_docs, n_out, on_device, &od));
    VRCHK(stage_output(ix->mgrp.which, out_which, n_out, on_device, &ow));
    if (n_ev) {
        VRCHK(stage_output(ix->mgrp.evs, out_ev_scores, n_ev, on_device, &es));
        VRCHK(stage_output(ix->mgrp.evr, out_ev_rows, n_ev, on_device, &er));
    }
    VRCHK(ix->sbuf.reserve((size_t)qblk * ldS * 4));
    VRCHK(ix->mgrp.B.reserve((size_t)qblk * ldB * 4));
    VRCHK(ix->mgrp.F.reserve((size_t)qblk * ldB * 4));
    float* S = ix->sbuf.as<float>();
    for (int32_t g0 = 0; g0 < n_groups;) {
        int32_t g1 = g0 + 1;                      // whole questions while the block holds <= 256 sub-queries
        while (g1 < n_groups && lims[g1 + 1] - lims[g0] <= qblk) ++g1;
        const int64_t s0 = lims[g0];
        const int nb = (int)(lims[g1] - s0), nqs = g1 - g0;
        MultiGroupArgs p{};
        p.a = block_view(ix, q32, s0, nb, k, true);                        // (the band is defined by the error model)
        p.a.out_scores = os + (size_t)g0 * k; p.a.out_ids = oi + (size_t)g0 * k;
        p.out_docs = od + (size_t)g0 * k; p.out_which = ow + (size_t)g0 * k;
        p.out_ev_scores = es; p.out_ev_rows = er;                          // (the call's arrays: indexed by the call's lims)
        p.lims = glims + g0;
        p.sub_base = (int)s0;
        p.fuse = fuse;
        p.goff = ix->grp.off.as<int>(); p.n_groups = nd;
        p.B = ix->mgrp.B.as<float>(); p.ldB = (size_t)ldB;
        p.F = ix->mgrp.F.as<float>();
        p.eps_sub = ix->mgrp.eps.as<float>();
        p.filter_of_group = fog ? fog + g0 : nullptr;
        p.n_filters = (int)ix->flt.n_filters;
        p.edges = ix->mgrp.edge.as<float>();
        p.present = ix->mgrp.edge.as<int>() + qblk;
        p.stats = ix->mgrp.state.as<unsigned long long>();
        VRCHK(score_block(ix, q32, s0, nb, ldS, nullptr, s));
        if (fog) VRCHK(mask_block(ix, ix->mgrp.fsub.as<int>() + s0, nb, ldS, nullptr, nullptr, 0, s));
        HIPCHK(launch_group_max(S, (size_t)ldS, p.goff, nd, ix->mgrp.B.as<float>(), p.ldB, nb, nullptr, 0, s));
        HIPCHK(launch_multi_group_fuse(p, nqs, s));
        HIPCHK(launch_multi_group_edges(p, nqs, s));
        HIPCHK(launch_multi_group_rescore(p, S, (size_t)ldS, nqs, s));
        HIPCHK(launch_multi_group_select(p, S, (size_t)ldS, nqs, s));
        g0 = g1;
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_rows, oi, n_out, on_device, s));
    VRCHK(return_output(out_docs, od, n_out, on_device, s));
    VRCHK(return_output(out_which, ow, n_out, on_device, s));
    if (n_ev) {
        VRCHK(return_output(out_ev_scores, es, n_ev, on_device, s));
        VRCHK(return_output(out_ev_rows, er, n_ev, on_device, s));
    }
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- diversified search (search_diverse.hip) ----------------------------------------------------------------------------------
// k rows per query picked by maximal marginal relevance from the pool of its `pool` best rows.  The pool is the plain or the
// filtered search's own result, produced by that search as it stands on the staged queries with device outputs of the diverse
// search's own; the selection kernel writes the (staged) outputs.  No state of its own but the pool.
extern "C" int vr_index_search_diverse(vr_index_t ix, const float* queries, int32_t nq, int32_t k, int32_t pool, float lambda,
                                       const int32_t* filter_of_query, float* out_scores, int64_t* out_ids, int32_t on_device,
                                       void* stream) {
    if (!ix || !queries || !out_scores || !out_ids || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    if (k < 1 || k > pool || pool > search_bigk_max())
        return fail(VR_ERR_INVALID, "k=%d pool=%d unsupported (1 <= k <= pool <= %d)", k, pool, search_bigk_max());
    if (!(lambda >= 0.f && lambda <= 1.f)) return fail(VR_ERR_INVALID, "lambda=%g outside [0, 1]", (double)lambda);
    if (!mmr_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, nq, pad256l(std::min<int64_t>(nq, 256)), on_device, s, &q32));
    const int* foq = nullptr;
    if (filter_of_query) VRCHK(stage_input(ix->flt.ids, filter_of_query, (size_t)nq, on_device, s, &foq));
    // ---- the pool: the staged queries are device queries to the search, which then stages nothing and writes the pool buffers
    const size_t n_pool = (size_t)nq * pool, n_out = (size_t)nq * k;
    VRCHK(ix->div.scores.reserve(n_pool * 4));
    VRCHK(ix->div.ids.reserve(n_pool * 8));
    if (foq) VRCHK(vr_index_search_filtered(ix, q32, nq, pool, foq, ix->div.scores.as<float>(), ix->div.ids.as<int64_t>(), 1, stream));
    else VRCHK(search_impl(ix, q32, nq, pool, ix->div.scores.as<float>(), ix->div.ids.as<int64_t>(), nullptr, 0, 1, stream));
    // ---- the picks
    float* os = nullptr; int64_t* oi = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    MmrArgs m{};
    m.index_f32 = ix->f32.as<float>(); m.n_docs = ix->n; m.dim = ix->dim;
    m.pool_scores = ix->div.scores.as<float>(); m.pool_ids = ix->div.ids.as<int64_t>();
    m.nq = nq; m.pool = pool; m.k = k; m.lambda = lambda;
    m.out_scores = os; m.out_ids = oi;
    HIPCHK(launch_mmr_select(m, s));
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- rank-fusion search (search_rrf.hip) --------------------------------------------------------------------------------------
extern "C" int vr_index_rrf_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, ix->rrf.state, 0, out3, reset);
}

// The k ids of largest reciprocal-rank-fusion score of every group of sub-queries.  The lists are the plain, the filtered or the
// document window search's own result for k = depth, produced by that search as it stands on the staged queries into buffers of
// the rank fusion's own (as the diversified search's pool is); one launch of the fusion kernel writes the (staged) outputs.
// No state of its own but the pool and three counters.
extern "C" int vr_index_search_rrf(vr_index_t ix, const float* queries, int32_t n_sub, const int64_t* lims, int32_t n_groups, int32_t k,
                                   int32_t depth, float c, const float* weights, const int32_t* filter_of_group, int32_t by_groups,
                                   float* out_scores, int64_t* out_ids, int32_t* out_hits, int32_t on_device, void* stream) {
    if (!ix || n_groups < 0 || n_sub < 0 || (n_groups > 0 && (!queries || !lims || !out_scores || !out_ids || !out_hits)))
        return fail(VR_ERR_INVALID, "bad arguments");
    if (n_groups == 0) {
        if (n_sub != 0) return fail(VR_ERR_INVALID, "%d sub-queries in no group", (int)n_sub);
        return VR_OK;                             // no group: no launch
    }
    int max_entries = 0;
    VRCHK(rrf_check(lims, n_sub, n_groups, k, depth, c, weights, &max_entries));
    if (!range_dim_ok(ix->dim) || !mmr_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (by_groups && (ix->grp.n_groups <= 0 || ix->n <= 0))
        return fail(VR_ERR_STATE, "no grouping set for the rows of the index (vr_index_set_groups)");
    if (filter_of_group) VRCHK(check_filter_ids(ix, filter_of_group, n_groups, on_device, "filter_of_group"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)n_groups * k;
    if (ix->n == 0) return rrf_fill_tails(out_scores, out_ids, out_hits, n_out, on_device, s);   // no row: tails, no launch
    if (!ix->rrf.state.p) VRCHK(ix->rrf.state.alloc(3 * 8));
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, n_sub, pad256l(std::min<int64_t>(n_sub, 256)), on_device, s, &q32));
    std::vector<int> lims32((size_t)n_groups + 1);
    for (int32_t g = 0; g <= n_groups; ++g) lims32[(size_t)g] = (int)lims[g];
    const int* glims = nullptr;
    const float* w = nullptr;
    VRCHK(stage_input(ix->rrf.lims, (const int*)lims32.data(), lims32.size(), 0, s, &glims));
    if (weights) VRCHK(stage_input(ix->rrf.w, weights, (size_t)n_sub, 0, s, &w));
    const int* fsub = nullptr;
    if (filter_of_group) {                        // the group's filter for every one of its sub-queries, as the fused search expands it
        const int* fog = nullptr;
        VRCHK(stage_input(ix->flt.ids, filter_of_group, (size_t)n_groups, on_device, s, &fog));
        VRCHK(ix->rrf.fsub.reserve((size_t)n_sub * 4));
        HIPCHK(launch_multi_expand(glims, fog, n_groups, ix->rrf.fsub.as<int>(), s));
        fsub = ix->rrf.fsub.as<int>();
    }
    HIPCHK(hipStreamSynchronize(s));              // (the host arrays are free from here on)
    // ---- the pool: the staged queries are device queries to the search, which then stages nothing and writes the pool buffers
    const size_t n_pool = (size_t)n_sub * depth;
    VRCHK(ix->rrf.scores.reserve(n_pool * 4));
    VRCHK(ix->rrf.ids.reserve(n_pool * 8));
    if (by_groups) {
        VRCHK(ix->rrf.groups.reserve(n_pool * 8));
        const std::vector<int64_t> zero((size_t)n_sub, 0);
        VRCHK(vr_index_search_groups_window(ix, q32, n_sub, zero.data(), depth, fsub, ix->rrf.scores.as<float>(), ix->rrf.ids.as<int64_t>(),
                                            ix->rrf.groups.as<int64_t>(), 1, stream));      // (synchronises before `zero` dies)
    } else if (fsub) {
        VRCHK(vr_index_search_filtered(ix, q32, n_sub, depth, fsub, ix->rrf.scores.as<float>(), ix->rrf.ids.as<int64_t>(), 1, stream));
    } else {
        VRCHK(search_impl(ix, q32, n_sub, depth, ix->rrf.scores.as<float>(), ix->rrf.ids.as<int64_t>(), nullptr, 0, 1, stream));
    }
    // ---- the fusion
    RrfArgs p{};
    p.ids = by_groups ? ix->rrf.groups.as<int64_t>() : ix->rrf.ids.as<int64_t>();
    p.lims = glims; p.weights = w; p.depth = depth; p.k = k; p.c = c;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &p.out_scores));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &p.out_ids));
    VRCHK(stage_output(ix->rrf.hits, out_hits, n_out, on_device, &p.out_hits));
    p.stats = ix->rrf.state.as<unsigned long long>();
    HIPCHK(launch_rrf_fuse(p, n_groups, max_entries, s));
    VRCHK(return_output(out_scores, p.out_scores, n_out, on_device, s));
    VRCHK(return_output(out_ids, p.out_ids, n_out, on_device, s));
    VRCHK(return_output(out_hits, p.out_hits, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}
