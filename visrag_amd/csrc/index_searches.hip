// The searches of the index that work on score rows (vr_index_search_groups / _filtered / _range / _rank_rows / _count_range /
// _window / _groups_window / _rank_groups / _count_groups_range / _groups_range / _multi / _multi_groups / _diverse / _rrf of
// include/visrag_hip.h, with what sets them up and their counters).  Each of them: every argument check first, then the call frame
// (index.h: open_frame — staged queries and filter ids, the score rows, with a grouping the group maxima), then per block of <= 256
// queries frame_block (the deep path's bf16 MFMA GEMM, the mask, the group maxima) and the search's own kernels.  A row-level
// search and its document-level sibling are ONE body over two members of the handle (range_impl, rank_impl, window_impl,
// multi_impl): `grouped` picks the member, the grouping check, the kernels and the outputs that differ.  Scratch (query staging,
// score rows, staged outputs, the staged filter ids) is shared between the searches; what a search keeps is its member of the
// handle (index.h).
#include "index.h"

// the three counters of a search whose state words are u64 (all but the grouped and the filtered search); state: null with ix
static int stats3(vr_index_t ix, const DevBuf* state, int64_t* out3, int32_t reset) {
    if (!ix || !out3) return fail(VR_ERR_INVALID, "NULL argument");
    return read_counters<unsigned long long, 3>(ix, *state, 0, out3, reset);
}

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
    VRCHK(check_grouping(ix));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    Frame f;
    VRCHK(open_frame(ix, queries, nq, nullptr, 0, on_device, s, &ix->grp.B, &f));
    const size_t n_out = (size_t)nq * k;
    float* os = nullptr; int64_t* oi = nullptr; int64_t* og = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    VRCHK(stage_output(ix->grp.out, out_groups, n_out, on_device, &og));
    const bool certify = certifies(ix);
    for (int64_t q0 = 0; q0 < nq; q0 += QBLK) {
        const int nb = (int)std::min<int64_t>(QBLK, nq - q0);
        GroupSearchArgs p{};
        // (the error model also bounds which rows of a group are re-scored)
        SearchArgs& a = p.a = block_view(ix, f.q32, q0, nb, k, true);
        a.flag_count = ix->grp.state.as<int>(); a.flag_list = ix->grp.state.as<int>() + GRP_LIST;
        a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k;
        p.goff = f.goff; p.n_groups = f.ng;
        p.B = ix->grp.B.as<float>(); p.ldB = (size_t)f.ldB;
        p.out_groups = og + (size_t)q0 * k;
        p.stats = ix->grp.state.as<unsigned>() + GRP_STATS;
        p.certify = certify ? 1 : 0;
        VRCHK(frame_block(ix, f, q0, nb, nullptr, a.flag_count, &ix->grp.B));   // (also clears the grouped search's flag counter)
        HIPCHK(launch_group_select(p, f.S, (size_t)f.ldS, nb, s));
        if (certify) {
            // whatever the select flagged (nothing, normally: the three kernels leave at once): exact fp32 score rows
            HIPCHK(launch_exact_scores(a.index_f32, a.n_docs, a.dim, a.q_f32, a.flag_list, a.flag_count, 0, nb, f.S, (size_t)f.ldS, s));
            HIPCHK(launch_group_max(f.S, (size_t)f.ldS, p.goff, f.ng, p.B, p.ldB, nb, a.flag_count, 0, s));
            HIPCHK(launch_group_select_exact(p, f.S, (size_t)f.ldS, 0, nb, s));
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
    Frame f;
    VRCHK(open_frame(ix, queries, nq, filter_of_query, nq, on_device, s, nullptr, &f));
    const size_t n_out = (size_t)nq * k;
    float* os = nullptr; int64_t* oi = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    const bool certify = certifies(ix);
    for (int64_t q0 = 0; q0 < nq; q0 += QBLK) {
        const int nb = (int)std::min<int64_t>(QBLK, nq - q0);
        FilterSearchArgs p{};
        SearchArgs& a = p.a = block_view(ix, f.q32, q0, nb, k, false);
        a.flag_count = ix->flt.state.as<int>(); a.flag_list = ix->flt.state.as<int>() + FLT_LIST;
        a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k;
        p.bits = ix->flt.bits.as<uint32_t>(); p.words = (size_t)((ix->n + 31) / 32); p.n_filters = (int)ix->flt.n_filters;
        p.allowed = ix->flt.count.as<int>();
        p.filter_of_query = f.foq + q0;
        p.stats = ix->flt.state.as<unsigned>() + FLT_STATS;
        p.certify = certify ? 1 : 0;
        VRCHK(frame_block(ix, f, q0, nb, f.foq + q0, a.flag_count, nullptr));   // (also clears the filtered search's flag counter)
        HIPCHK(launch_filter_select(p, f.S, (size_t)f.ldS, nb, s));
        if (certify) {
            // whatever the select flagged (nothing, normally: the three kernels leave at once): exact fp32 score rows, masked
            HIPCHK(launch_exact_scores(a.index_f32, a.n_docs, a.dim, a.q_f32, a.flag_list, a.flag_count, 0, nb, f.S, (size_t)f.ldS, s));
            VRCHK(mask_block(ix, f.foq + q0, nb, f.ldS, a.flag_list, a.flag_count, 0, s));
            HIPCHK(launch_filter_select_exact(p, f.S, (size_t)f.ldS, 0, nb, s));
        }
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- range search (search_range.hip) and document range search (search_group_range.hip) -----------------------------------------
// Every row (grouped: every document, under the query's filter) at or above a query's threshold.  Result, counts, offsets and
// counters — grouped: group maxima and best rows too — are the search's own (rng / grng); the grouping and the filters are read.
static int range_impl(vr_index_t ix, bool grouped, const float* queries, int32_t nq, const float* thresholds, const int32_t* filter_of_query,
                      int64_t max_total, int64_t* out_lims, int64_t* total, int32_t on_device, void* stream) {
    if (!ix || !queries || !thresholds || !out_lims || !total || nq < 1) return fail(VR_ERR_INVALID, "bad arguments");
    if (max_total < 1) return fail(VR_ERR_INVALID, "max_total=%lld must be at least 1", (long long)max_total);
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (!on_device) VRCHK(check_finite(thresholds, nq, "thresholds"));
    if (grouped && ix->n > 0) VRCHK(check_grouping(ix));
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    RangeState& st = grouped ? ix->grng : ix->rng;
    if (ix->n == 0) {                             // no row, no document: no launch
        if (on_device) {
            HIPCHK(hipMemsetAsync(out_lims, 0, ((size_t)nq + 1) * 8, s));
            HIPCHK(hipStreamSynchronize(s));
        } else {
            std::fill(out_lims, out_lims + nq + 1, (int64_t)0);
        }
        *total = 0;
        st.total = 0;
        return VR_OK;
    }
    VRCHK(range_store_open(st));
    st.total = -1;                                // from here on the previous result is gone
    const int64_t universe = grouped ? ix->grp.n_groups : ix->n, slots = range_scan_slots(universe);   // what the scan counts
    Frame f;
    VRCHK(open_frame(ix, queries, nq, filter_of_query, nq, on_device, s, grouped ? &st.B : nullptr, &f));
    const float* thr = nullptr;
    int64_t* lims = nullptr;
    VRCHK(stage_input(st.thr, thresholds, (size_t)nq, on_device, s, &thr));
    VRCHK(stage_output(st.lims, out_lims, (size_t)nq + 1, on_device, &lims));
    if (grouped) VRCHK(st.R.reserve((size_t)QBLK * f.ldB * 4));
    VRCHK(st.cnt.reserve((size_t)QBLK * slots * 4));
    VRCHK(st.off.reserve((size_t)QBLK * slots * 4));
    VRCHK(range_store_reserve(st, grouped, std::min<int64_t>(max_total, 65536), 0, max_total, s));
    int* cnt = st.cnt.as<int>(); int* off = st.off.as<int>();
    int64_t base = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += QBLK) {
        const int nb = (int)std::min<int64_t>(QBLK, nq - q0);
        RangeSearchArgs p{}; GroupRangeArgs g{};
        auto fill = [&](auto& a) {
            a.a = block_view(ix, f.q32, q0, nb, 1, true);                  // (the band is defined by the error model)
            a.thresholds = thr + q0;
            a.filter_of_query = f.foq ? f.foq + q0 : nullptr;
            a.n_filters = (int)ix->flt.n_filters;
            a.stats = st.state.as<unsigned long long>();
        };
        if (grouped) {
            fill(g);
            g.goff = f.goff; g.n_groups = f.ng; g.B = st.B.as<float>(); g.ldB = (size_t)f.ldB; g.R = st.R.as<int>();
        } else {
            fill(p);
        }
        VRCHK(frame_block(ix, f, q0, nb, f.foq ? f.foq + q0 : nullptr, nullptr, grouped ? &st.B : nullptr));
        if (grouped) HIPCHK(launch_group_range_rescore(g, f.S, (size_t)f.ldS, nb, cnt, s));
        else HIPCHK(launch_range_rescore(p, f.S, (size_t)f.ldS, nb, cnt, s));
        HIPCHK(launch_range_scan(cnt, off, universe, nb, base, q0 == 0 ? 1 : 0, lims + q0, st.state.as<int64_t>() + RANGE_TOTAL, s));
        // the size of the block's result is a host value: capacity check, growth of the result arrays
        int64_t bt = 0;
        VRCHK(range_store_block_total(st, s, &bt));
        if (bt < 0 || base + bt > max_total)
            return fail(VR_ERR_CAPACITY, "%s result exceeds max_total=%lld in query block %lld (queries %lld..%lld): %lld entries by then",
                        grouped ? "document range" : "range", (long long)max_total, (long long)(q0 / QBLK), (long long)q0,
                        (long long)(q0 + nb - 1), (long long)(base + bt));
        VRCHK(range_store_reserve(st, grouped, base + bt, base, max_total, s));
        p.out_scores = g.out_scores = st.scores.as<float>();
        p.out_ids = g.out_rows = st.rows.as<int64_t>();
        g.out_groups = st.groups.as<int64_t>();
        if (bt > 0) {
            if (grouped) HIPCHK(launch_group_range_pack(g, nb, cnt, off, lims + q0, s));
            else HIPCHK(launch_range_pack(p, f.S, (size_t)f.ldS, nb, cnt, off, lims + q0, s));
        }
        base += bt;
    }
    VRCHK(return_output(out_lims, lims, (size_t)nq + 1, on_device, s));
    HIPCHK(hipStreamSynchronize(s));
    *total = base;
    st.total = base;
    return VR_OK;
}

extern "C" int vr_index_range_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) { return stats3(ix, ix ? &ix->rng.state : nullptr, out3, reset); }
extern "C" int vr_index_group_range_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    return stats3(ix, ix ? &ix->grng.state : nullptr, out3, reset);
}

extern "C" int vr_index_search_range(vr_index_t ix, const float* queries, int32_t nq, const float* thresholds,
                                     const int32_t* filter_of_query, int64_t max_total, int64_t* out_lims, int64_t* total,
                                     int32_t on_device, void* stream) {
    return range_impl(ix, false, queries, nq, thresholds, filter_of_query, max_total, out_lims, total, on_device, stream);
}

extern "C" int vr_index_search_groups_range(vr_index_t ix, const float* queries, int32_t nq, const float* thresholds,
                                            const int32_t* filter_of_query, int64_t max_total, int64_t* out_lims, int64_t* total,
                                            int32_t on_device, void* stream) {
    return range_impl(ix, true, queries, nq, thresholds, filter_of_query, max_total, out_lims, total, on_device, stream);
}

extern "C" int vr_index_range_results(vr_index_t ix, float* out_scores, int64_t* out_ids, int64_t n, int32_t on_device, void* stream) {
    if (!ix || n < 0 || (n > 0 && (!out_scores || !out_ids))) return fail(VR_ERR_INVALID, "bad arguments");
    return range_store_results(ix, ix->rng, false, out_scores, out_ids, nullptr, n, on_device, stream);
}

extern "C" int vr_index_group_range_results(vr_index_t ix, float* out_scores, int64_t* out_rows, int64_t* out_groups, int64_t n,
                                            int32_t on_device, void* stream) {
    if (!ix || n < 0 || (n > 0 && (!out_scores || !out_rows || !out_groups))) return fail(VR_ERR_INVALID, "bad arguments");
    return range_store_results(ix, ix->grng, true, out_scores, out_rows, out_groups, n, on_device, stream);
}

// ---- rank search (search_rank.hip) and document rank search (search_group_rank.hip) ---------------------------------------------
// What vr_index_rank_rows / vr_index_rank_groups (ranks: targets set) and vr_index_count_range / vr_index_count_groups_range
// (thresholds set) share: per block with pairs the (masked) score rows, grouped their group maxima, the bars of the block's pairs
// and their counts.  Pairs, bars, group maxima and counters are the search's own (rnk / grnk); the grouping and the filters are
// read.  Nothing is stored.
static int rank_impl(vr_index_t ix, bool grouped, bool ranks, const float* queries, int32_t nq, const int64_t* lims, const int64_t* targets,
                     const float* thresholds, int32_t strict, const int32_t* filter_of_query, float* out_scores, int64_t* out_rows,
                     int64_t* out_counts, int32_t on_device, void* stream) {
    if (!ix || !lims || nq < 0 || (nq > 0 && !queries)) return fail(VR_ERR_INVALID, "bad arguments");
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    int64_t np = 0;
    VRCHK(check_pair_lims(lims, nq, &np));
    if (np > 0 && (!out_counts || (ranks ? !targets || !out_scores || (grouped && !out_rows) : !thresholds)))
        return fail(VR_ERR_INVALID, "bad arguments");
    if (grouped) VRCHK(check_grouping(ix));
    if (ranks) {
        const int64_t bound = grouped ? ix->grp.n_groups : ix->n;
        for (int64_t i = 0; i < np; ++i)
            if (targets[i] < 0 || targets[i] >= bound)
                return fail(VR_ERR_INVALID, "%s[%lld] = %lld outside [0, %lld)", grouped ? "groups" : "ids", (long long)i, (long long)targets[i],
                            (long long)bound);
    } else {
        VRCHK(check_finite(thresholds, np, "thresholds"));
    }
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    if (np == 0) return VR_OK;                    // no pair: no launch
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    if (ix->n == 0) {                             // (row counts only: a target would have been out of range, a grouping unset) no row: no launch
        if (on_device) HIPCHK(hipMemsetAsync(out_counts, 0, (size_t)np * 8, s));
        else std::fill(out_counts, out_counts + np, (int64_t)0);
        return VR_OK;
    }
    RankState& st = grouped ? ix->grnk : ix->rnk;
    VRCHK(open_state(st.state, STAT_WORDS));
    Frame f;
    VRCHK(open_frame(ix, queries, nq, filter_of_query, nq, on_device, s, grouped ? &st.B : nullptr, &f));
    VRCHK(stage_pairs(st, lims, nq, np, ranks ? targets : nullptr, thresholds, s));     // (the host arrays are free from here on)
    // the staged outputs: scores in os; the row search's counts in oi, the document search's best rows there and its counts in its own
    float* os = nullptr; int64_t* orow = nullptr; int64_t* oc = nullptr;
    if (ranks) VRCHK(stage_output(ix->os, out_scores, (size_t)np, on_device, &os));
    if (ranks && grouped) VRCHK(stage_output(ix->oi, out_rows, (size_t)np, on_device, &orow));
    VRCHK(stage_output(grouped ? st.out : ix->oi, out_counts, (size_t)np, on_device, &oc));
    for (int64_t q0 = 0; q0 < nq; q0 += QBLK) {
        const int nb = (int)std::min<int64_t>(QBLK, nq - q0);
        const int64_t p0 = lims[q0], pn = lims[q0 + nb] - p0;
        if (pn == 0) continue;                    // a block without pairs: no launch
        RankSearchArgs p{}; GroupRankArgs g{};
        auto fill = [&](auto& a) {
            a.a = block_view(ix, f.q32, q0, nb, 1, true);                  // (the band is defined by the error model)
            a.pair_query = st.q.as<int>() + p0;
            a.pair_thr = ranks ? nullptr : st.v.as<float>() + p0;
            a.strict = strict ? 1 : 0;
            a.filter_of_query = f.foq ? f.foq + q0 : nullptr;
            a.n_filters = (int)ix->flt.n_filters;
            a.bars = st.bar.as<unsigned long long>() + p0;
            a.bar_eps = st.eps.as<float>() + p0;
            a.out_scores = ranks ? os + p0 : nullptr;
            a.out_counts = reinterpret_cast<unsigned long long*>(oc) + p0;
            a.stats = st.state.as<unsigned long long>();
        };
        VRCHK(frame_block(ix, f, q0, nb, f.foq ? f.foq + q0 : nullptr, nullptr, grouped ? &st.B : nullptr));
        if (grouped) {
            fill(g);
            g.goff = f.goff; g.n_groups = f.ng; g.B = st.B.as<float>(); g.ldB = (size_t)f.ldB;
            g.pair_group = ranks ? st.v.as<int>() + p0 : nullptr;
            g.out_rows = ranks ? reinterpret_cast<long long*>(orow) + p0 : nullptr;
            HIPCHK(launch_group_rank_bars(g, f.S, (size_t)f.ldS, nb, pn, s));
            HIPCHK(launch_group_rank_count(g, f.S, (size_t)f.ldS, nb, pn, s));
        } else {
            fill(p);
            p.pair_id = ranks ? st.v.as<int>() + p0 : nullptr;
            HIPCHK(launch_rank_bars(p, (size_t)f.ldS, nb, pn, s));
            HIPCHK(launch_rank_count(p, f.S, (size_t)f.ldS, nb, pn, s));
        }
    }
    if (ranks) VRCHK(return_output(out_scores, os, (size_t)np, on_device, s));
    if (ranks && grouped) VRCHK(return_output(out_rows, orow, (size_t)np, on_device, s));
    VRCHK(return_output(out_counts, oc, (size_t)np, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_index_rank_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) { return stats3(ix, ix ? &ix->rnk.state : nullptr, out3, reset); }
extern "C" int vr_index_group_rank_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    return stats3(ix, ix ? &ix->grnk.state : nullptr, out3, reset);
}

extern "C" int vr_index_rank_rows(vr_index_t ix, const float* queries, int32_t nq, const int64_t* lims, const int64_t* ids,
                                  const int32_t* filter_of_query, float* out_scores, int64_t* out_ranks, int32_t on_device, void* stream) {
    return rank_impl(ix, false, true, queries, nq, lims, ids, nullptr, 0, filter_of_query, out_scores, nullptr, out_ranks, on_device, stream);
}

extern "C" int vr_index_count_range(vr_index_t ix, const float* queries, int32_t nq, const int64_t* lims, const float* thresholds,
                                    int32_t strict, const int32_t* filter_of_query, int64_t* out_counts, int32_t on_device, void* stream) {
    return rank_impl(ix, false, false, queries, nq, lims, nullptr, thresholds, strict, filter_of_query, nullptr, nullptr, out_counts,
                     on_device, stream);
}

extern "C" int vr_index_rank_groups(vr_index_t ix, const float* queries, int32_t nq, const int64_t* lims, const int64_t* groups,
                                    const int32_t* filter_of_query, float* out_scores, int64_t* out_rows, int64_t* out_ranks,
                                    int32_t on_device, void* stream) {
    return rank_impl(ix, true, true, queries, nq, lims, groups, nullptr, 0, filter_of_query, out_scores, out_rows, out_ranks, on_device,
                     stream);
}

extern "C" int vr_index_count_groups_range(vr_index_t ix, const float* queries, int32_t nq, const int64_t* lims,
                                           const float* thresholds, int32_t strict, const int32_t* filter_of_query,
                                           int64_t* out_counts, int32_t on_device, void* stream) {
    return rank_impl(ix, true, false, queries, nq, lims, nullptr, thresholds, strict, filter_of_query, nullptr, nullptr, out_counts,
                     on_device, stream);
}

// ---- windowed search (search_window.hip) and document window search (search_group_window.hip) -----------------------------------
// The rows (grouped: the groups, under the query's filter) at ranks [offsets[q], offsets[q] + k) of every query's ranking: per
// block the (masked) score rows, grouped their group maxima, the band edges, the rewritten rows (maxima) and the select.  Edges,
// counters, group maxima and best rows are the search's own (win / gwin); the grouping and the filters are read.  Nothing is stored.
static int window_impl(vr_index_t ix, bool grouped, const float* queries, int32_t nq, const int64_t* offsets, int32_t k,
                       const int32_t* filter_of_query, float* out_scores, int64_t* out_ids, int64_t* out_groups, int32_t on_device,
                       void* stream) {
    if (!ix || nq < 0 || (nq > 0 && (!queries || !offsets || !out_scores || !out_ids || (grouped && !out_groups))))
        return fail(VR_ERR_INVALID, "bad arguments");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    for (int32_t q = 0; q < nq; ++q)
        if (offsets[q] < 0) return fail(VR_ERR_INVALID, "offsets[%d] = %lld is negative", (int)q, (long long)offsets[q]);
    if (grouped) VRCHK(check_grouping(ix));       // (so the document search has no empty-index answer)
    if (filter_of_query) VRCHK(check_filter_ids(ix, filter_of_query, nq, on_device, "filter_of_query"));
    if (nq == 0) return VR_OK;                    // no query: no launch
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)nq * k;
    if (ix->n == 0) return fill_tails(out_scores, out_ids, nullptr, n_out, on_device, s);      // no row: tails, no launch
    WindowState& st = grouped ? ix->gwin : ix->win;
    VRCHK(open_state(st.state, STAT_WORDS));
    Frame f;
    VRCHK(open_frame(ix, queries, nq, filter_of_query, nq, on_device, s, grouped ? &st.B : nullptr, &f));
    const int64_t* off = nullptr;                 // (a host array whoever calls)
    VRCHK(stage_input(st.off, offsets, (size_t)nq, 0, s, &off));
    VRCHK(st.edge.reserve((size_t)QBLK * (grouped ? 12 : 8)));
    HIPCHK(hipStreamSynchronize(s));              // (the host array is free from here on)
    float* os = nullptr; int64_t* oi = nullptr; int64_t* og = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    if (grouped) {
        VRCHK(stage_output(st.out, out_groups, n_out, on_device, &og));
        VRCHK(st.R.reserve((size_t)QBLK * f.ldB * 4));
    }
    for (int64_t q0 = 0; q0 < nq; q0 += QBLK) {
        const int nb = (int)std::min<int64_t>(QBLK, nq - q0);
        WindowSearchArgs p{}; GroupWindowArgs g{};
        auto fill = [&](auto& a) {
            a.a = block_view(ix, f.q32, q0, nb, k, true);                  // (the band is defined by the error model)
            a.a.out_scores = os + (size_t)q0 * k; a.a.out_ids = oi + (size_t)q0 * k;
            a.offsets = off + q0;
            a.filter_of_query = f.foq ? f.foq + q0 : nullptr;
            a.n_filters = (int)ix->flt.n_filters;
            a.edges = st.edge.as<float>();
            a.stats = st.state.as<unsigned long long>();
        };
        VRCHK(frame_block(ix, f, q0, nb, f.foq ? f.foq + q0 : nullptr, nullptr, grouped ? &st.B : nullptr));
        if (grouped) {
            fill(g);
            g.out_groups = og + (size_t)q0 * k;
            g.goff = f.goff; g.n_groups = f.ng; g.B = st.B.as<float>(); g.ldB = (size_t)f.ldB; g.R = st.R.as<int>();
            g.present = st.edge.as<int>() + 2 * QBLK;
            HIPCHK(launch_group_window_edges(g, nb, s));
            HIPCHK(launch_group_window_rescore(g, f.S, (size_t)f.ldS, nb, s));
            HIPCHK(launch_group_window_select(g, nb, s));
        } else {
            fill(p);
            p.allowed = f.foq ? ix->flt.count.as<int>() : nullptr;
            HIPCHK(launch_window_edges(p, f.S, (size_t)f.ldS, nb, s));
            HIPCHK(launch_window_rescore(p, f.S, (size_t)f.ldS, nb, s));
            HIPCHK(launch_window_select(p, f.S, (size_t)f.ldS, nb, s));
        }
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (grouped) VRCHK(return_output(out_groups, og, n_out, on_device, s));
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_index_window_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) { return stats3(ix, ix ? &ix->win.state : nullptr, out3, reset); }
extern "C" int vr_index_group_window_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    return stats3(ix, ix ? &ix->gwin.state : nullptr, out3, reset);
}

extern "C" int vr_index_search_window(vr_index_t ix, const float* queries, int32_t nq, const int64_t* offsets, int32_t k,
                                      const int32_t* filter_of_query, float* out_scores, int64_t* out_ids, int32_t on_device,
                                      void* stream) {
    return window_impl(ix, false, queries, nq, offsets, k, filter_of_query, out_scores, out_ids, nullptr, on_device, stream);
}

extern "C" int vr_index_search_groups_window(vr_index_t ix, const float* queries, int32_t nq, const int64_t* offsets, int32_t k,
                                             const int32_t* filter_of_query, float* out_scores, int64_t* out_ids,
                                             int64_t* out_groups, int32_t on_device, void* stream) {
    return window_impl(ix, true, queries, nq, offsets, k, filter_of_query, out_scores, out_ids, out_groups, on_device, stream);
}

// ---- fused search (search_multi.hip) and fused document search (search_multi_group.hip) -----------------------------------------
// The k rows (grouped: documents, with the best page per sub-query) of largest fused score of every group of sub-queries (there: a
// question): whole groups packed greedily into blocks of <= 256 sub-queries, and per block the (masked) score rows, grouped their
// document maxima, the fusion, the band edges, the rewritten fused rows and the select.  Edges and counters, grouped maxima and
// fused rows, are the search's own (mul / mgrp); the grouping and the filters are read.  Nothing is stored.
static int multi_impl(vr_index_t ix, bool grouped, const float* queries, int32_t n_sub, const int64_t* lims, int32_t n_groups, int32_t k,
                      int32_t fuse, const int32_t* filter_of_group, float* out_scores, int64_t* out_ids, int64_t* out_docs,
                      int32_t* out_which, float* out_ev_scores, int64_t* out_ev_rows, int32_t on_device, void* stream) {
    const char* noun = grouped ? "question" : "group";
    if (!ix || n_groups < 0 || n_sub < 0 ||
        (n_groups > 0 && (!queries || !lims || !out_scores || !out_ids || (grouped && !out_docs) || !out_which)))
        return fail(VR_ERR_INVALID, "bad arguments");
    if ((out_ev_scores != nullptr) != (out_ev_rows != nullptr))
        return fail(VR_ERR_INVALID, "the evidence outputs are both NULL or both set");
    if (k <= 0 || k > search_bigk_max()) return fail(VR_ERR_INVALID, "k=%d unsupported (1..%d)", k, search_bigk_max());
    if (fuse != 0 && fuse != 1) return fail(VR_ERR_INVALID, "fuse=%d unsupported (0: max, 1: min)", (int)fuse);
    if (!range_dim_ok(ix->dim)) return fail(VR_ERR_INVALID, "dim %d unsupported", ix->dim);
    if (n_groups == 0) {
        if (n_sub != 0) return fail(VR_ERR_INVALID, "%d sub-queries in no %s", (int)n_sub, noun);
        return VR_OK;                             // no group: no launch
    }
    VRCHK(check_group_lims(lims, n_groups, n_sub, noun, "sub-queries", 0, nullptr));
    if (filter_of_group) VRCHK(check_filter_ids(ix, filter_of_group, n_groups, on_device, "filter_of_group"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)n_groups * k, n_ev = out_ev_scores ? (size_t)n_sub * k : 0;
    if (ix->n == 0) {                             // no row: tails, no launch (and no look at the grouping)
        VRCHK(fill_tails(out_scores, out_ids, out_which, n_out, on_device, s));
        if (grouped) VRCHK(fill_tails(out_scores, out_docs, nullptr, n_out, on_device, s));
        if (n_ev) VRCHK(fill_tails(out_ev_scores, out_ev_rows, nullptr, n_ev, on_device, s));
        return VR_OK;
    }
    if (grouped) VRCHK(check_grouping(ix));
    MultiState& st = grouped ? ix->mgrp : ix->mul;
    VRCHK(open_state(st.state, STAT_WORDS));
    Frame f;
    VRCHK(open_frame(ix, queries, n_sub, nullptr, 0, on_device, s, grouped ? &st.B : nullptr, &f));
    VRCHK(st.edge.reserve((size_t)QBLK * (grouped ? 8 : 4)));
    if (grouped) {
        VRCHK(st.eps.reserve((size_t)QBLK * 4));
        VRCHK(st.F.reserve((size_t)QBLK * f.ldB * 4));
    }
    const int* glims = nullptr; const int* fog = nullptr; const int* fsub = nullptr;
    VRCHK(stage_groups(ix, st.lims, st.fsub, lims, n_groups, n_sub, filter_of_group, on_device, s, &glims, &fog, &fsub));
    float* os = nullptr; int64_t* oi = nullptr; int64_t* od = nullptr; int32_t* ow = nullptr; float* es = nullptr; int64_t* er = nullptr;
    VRCHK(stage_output(ix->os, out_scores, n_out, on_device, &os));
    VRCHK(stage_output(ix->oi, out_ids, n_out, on_device, &oi));
    if (grouped) VRCHK(stage_output(st.docs, out_docs, n_out, on_device, &od));
    VRCHK(stage_output(st.which, out_which, n_out, on_device, &ow));
    if (n_ev) {
        VRCHK(stage_output(st.evs, out_ev_scores, n_ev, on_device, &es));
        VRCHK(stage_output(st.evr, out_ev_rows, n_ev, on_device, &er));
    }
    for (int32_t g0 = 0; g0 < n_groups;) {
        int32_t g1 = g0 + 1;                      // whole groups while the block holds <= 256 sub-queries
        while (g1 < n_groups && lims[g1 + 1] - lims[g0] <= QBLK) ++g1;
        const int64_t s0 = lims[g0];
        const int nb = (int)(lims[g1] - s0), ng = g1 - g0;
        MultiSearchArgs p{}; MultiGroupArgs g{};
        auto fill = [&](auto& a) {
            a.a = block_view(ix, f.q32, s0, nb, k, true);                  // (the band is defined by the error model)
            a.a.out_scores = os + (size_t)g0 * k; a.a.out_ids = oi + (size_t)g0 * k;
            a.out_which = ow + (size_t)g0 * k;
            a.lims = glims + g0;
            a.sub_base = (int)s0;
            a.fuse = fuse;
            a.filter_of_group = fog ? fog + g0 : nullptr;
            a.n_filters = (int)ix->flt.n_filters;
            a.edges = st.edge.as<float>();
            a.stats = st.state.as<unsigned long long>();
        };
        VRCHK(frame_block(ix, f, s0, nb, fsub ? fsub + s0 : nullptr, nullptr, grouped ? &st.B : nullptr));
        if (grouped) {
            fill(g);
            g.out_docs = od + (size_t)g0 * k;
            g.out_ev_scores = es; g.out_ev_rows = er;                      // (the call's arrays: indexed by the call's lims)
            g.goff = f.goff; g.n_groups = f.ng; g.B = st.B.as<float>(); g.ldB = (size_t)f.ldB;
            g.F = st.F.as<float>();
            g.eps_sub = st.eps.as<float>();
            g.present = st.edge.as<int>() + QBLK;
            HIPCHK(launch_multi_group_fuse(g, ng, s));
            HIPCHK(launch_multi_group_edges(g, ng, s));
            HIPCHK(launch_multi_group_rescore(g, f.S, (size_t)f.ldS, ng, s));
            HIPCHK(launch_multi_group_select(g, f.S, (size_t)f.ldS, ng, s));
        } else {
            fill(p);
            p.allowed = fog ? ix->flt.count.as<int>() : nullptr;
            HIPCHK(launch_multi_fuse(p, f.S, (size_t)f.ldS, ng, s));
            HIPCHK(launch_multi_edges(p, f.S, (size_t)f.ldS, ng, s));
            HIPCHK(launch_multi_rescore(p, f.S, (size_t)f.ldS, ng, s));
            HIPCHK(launch_multi_select(p, f.S, (size_t)f.ldS, ng, s));
        }
        g0 = g1;
    }
    VRCHK(return_output(out_scores, os, n_out, on_device, s));
    VRCHK(return_output(out_ids, oi, n_out, on_device, s));
    if (grouped) VRCHK(return_output(out_docs, od, n_out, on_device, s));
    VRCHK(return_output(out_which, ow, n_out, on_device, s));
    if (n_ev) {
        VRCHK(return_output(out_ev_scores, es, n_ev, on_device, s));
        VRCHK(return_output(out_ev_rows, er, n_ev, on_device, s));
    }
    if (!on_device) HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_index_multi_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) { return stats3(ix, ix ? &ix->mul.state : nullptr, out3, reset); }
extern "C" int vr_index_multi_group_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) {
    return stats3(ix, ix ? &ix->mgrp.state : nullptr, out3, reset);
}

extern "C" int vr_index_search_multi(vr_index_t ix, const float* queries, int32_t n_sub, const int64_t* lims, int32_t n_groups,
                                     int32_t k, int32_t fuse, const int32_t* filter_of_group, float* out_scores, int64_t* out_ids,
                                     int32_t* out_which, int32_t on_device, void* stream) {
    return multi_impl(ix, false, queries, n_sub, lims, n_groups, k, fuse, filter_of_group, out_scores, out_ids, nullptr, out_which, nullptr,
                      nullptr, on_device, stream);
}

extern "C" int vr_index_search_multi_groups(vr_index_t ix, const float* queries, int32_t n_sub, const int64_t* lims, int32_t n_groups,
                                            int32_t k, int32_t fuse, const int32_t* filter_of_group, float* out_scores,
                                            int64_t* out_rows, int64_t* out_docs, int32_t* out_which, float* out_ev_scores,
                                            int64_t* out_ev_rows, int32_t on_device, void* stream) {
    return multi_impl(ix, true, queries, n_sub, lims, n_groups, k, fuse, filter_of_group, out_scores, out_rows, out_docs, out_which,
                      out_ev_scores, out_ev_rows, on_device, stream);
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
extern "C" int vr_index_rrf_search_stats(vr_index_t ix, int64_t* out3, int32_t reset) { return stats3(ix, ix ? &ix->rrf.state : nullptr, out3, reset); }

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
    if (by_groups) VRCHK(check_grouping(ix));
    if (filter_of_group) VRCHK(check_filter_ids(ix, filter_of_group, n_groups, on_device, "filter_of_group"));
    VRCHK(set_dev(ix->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = (size_t)n_groups * k;
    if (ix->n == 0) return rrf_fill_tails(out_scores, out_ids, out_hits, n_out, on_device, s);   // no row: tails, no launch
    VRCHK(open_state(ix->rrf.state, STAT_WORDS));
    const float* q32 = nullptr;
    VRCHK(stage_queries(ix, queries, n_sub, pad256l(std::min<int64_t>(n_sub, QBLK)), on_device, s, &q32));
    const float* w = nullptr;
    if (weights) VRCHK(stage_input(ix->rrf.w, weights, (size_t)n_sub, 0, s, &w));
    // the group's filter for every one of its sub-queries, as the fused search expands it
    const int* glims = nullptr; const int* fog = nullptr; const int* fsub = nullptr;
    VRCHK(stage_groups(ix, ix->rrf.lims, ix->rrf.fsub, lims, n_groups, n_sub, filter_of_group, on_device, s, &glims, &fog, &fsub));
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
