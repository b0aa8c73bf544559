// The search index of libvisrag_hip.so (vr_index_* / vr_topk_merge* / vr_rrf_* of include/visrag_hip.h): fp32 + bf16 row store, its life
// cycle, and the certified top-k search over it with its fallback passes (search*.hip).  The searches over score rows are in
// index_searches.hip, editing in place in index_rows.hip, the handle and what the three share in index.h.
#include "index.h"

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
    if (r != VR_OK) { delete ix; return r; }      // (the buffers free themselves)
    *ix->huge_seen = 0;
    *out = ix;
    return VR_OK;
}

extern "C" int vr_index_destroy(vr_index_t ix) {
    if (!ix) return VR_OK;
    (void)hipSetDevice(ix->device);
    (void)hipDeviceSynchronize();
    if (ix->rng.host_total) (void)hipHostFree(ix->rng.host_total);
    if (ix->grng.host_total) (void)hipHostFree(ix->grng.host_total);
    for (hipEvent_t e : ix->prof_ev) if (e) (void)hipEventDestroy(e);
    if (ix->huge_seen) (void)hipHostFree(ix->huge_seen);
    delete ix;                                    // every DevBuf frees what it owns
    return VR_OK;
}

extern "C" int vr_index_reset(vr_index_t ix) {
    if (!ix) return fail(VR_ERR_INVALID, "NULL index");
    VRCHK(set_dev(ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(ix->cert.p, 0, 8));          // largest row norm, largest rounding residual
    ix->n = 0;
    ix->grp.n_groups = 0;
    ix->flt.n_filters = 0;
    ix->rng.total = -1;
    ix->grng.total = -1;
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
    ix->grp.n_groups = 0;             // the grouping described the rows that were there
    ix->flt.n_filters = 0;            // ... and so did the filters
    ix->grng.total = -1;              // ... and the document range result names groups of that grouping
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
    return read_counters<unsigned, CERT_NSTATS>(ix, ix->cert, CERT_STATS, out6, reset);
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

// entries [f0, f0 + ns) of a's flag list through the exact fp32 pass: score rows over the whole index, plain top-k of each
static int exact_pass(vr_index_t ix, const SearchArgs& a, int f0, int ns, int64_t ldS, hipStream_t s) {
    HIPCHK(launch_exact_scores(a.index_f32, a.n_docs, a.dim, a.q_f32, a.flag_list, a.flag_count, f0, ns, ix->sbuf.as<float>(),
                               (size_t)ldS, s));
    HIPCHK(launch_exact_select(a, ix->sbuf.as<float>(), (size_t)ldS, f0, ns, s));
    return VR_OK;
}

int search_impl(vr_index_t ix, const float* queries, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids,
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
        else VRCHK(fill_tails(os, oi, nullptr, n_out, 1, s));            // (the staged arrays: on the device either way)
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
            // Deep retrieval: score rows of <= 256 queries at a time behind it, S[q][doc] = queries x index^T on the bf16 MFMA GEMM.
            const bool conv_in_kernel = !bigk && search_uses_stream(nb, dim);
            if (bigk) VRCHK(score_block(ix, q32, q0, nb, ldS, ix->cert.as<int>() + CERT_FLAG, s));
            else if (!conv_in_kernel)
                HIPCHK(launch_f32_to_bf16_pad(q32 + (size_t)q0 * dim, ix->qbf.p, (size_t)nb * dim, (size_t)nbp * dim, s,
                                              ix->cert.as<int>() + CERT_FLAG));   // (clears both flag counters)
            if (prof) HIPCHK(hipEventRecord(ix->prof_ev[1], s));
            SearchArgs a = block_view(ix, q32, q0, nb, k, false);
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
            a.flag_count = ix->cert.as<int>() + CERT_FLAG; a.flag_list = ix->flags.as<int>();
            a.flag2_count = ix->cert.as<int>() + CERT_FLAG2; a.flag2_list = ix->flags.as<int>() + ix->fcap;
            a.flag_tau = ix->flags.as<float>() + 2 * ix->fcap; a.flag_q = ix->flagq.p;
            a.stats = ix->cert.as<unsigned>() + CERT_STATS;
            if (keys_out) { a.out_keys = ok + (size_t)q0 * k; a.id_offset = id_offset; }
            else { a.out_scores = os + (size_t)q0 * k; a.out_ids = oi + (size_t)q0 * k; }
            a.prof_ev = prof ? ix->prof_ev : nullptr;
            if (bigk) {
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

extern "C" int vr_topk_merge(int device_id, const float* scores, const int64_t* ids, int32_t n_parts, int32_t nq,
                             int32_t k, float* out_scores, int64_t* out_ids, void* stream) {
    if (!scores || !ids || !out_scores || !out_ids || n_parts <= 0 || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_topk_merge(scores, ids, n_parts, nq, k, out_scores, out_ids, (hipStream_t)stream));
    return VR_OK;
}

// ---- rank fusion of lists from anywhere (search_rrf.hip); the index's own is vr_index_search_rrf (index_searches.hip) ----------
extern "C" int vr_rrf_max_entries(void) { return rrf_max_entries(); }

extern "C" int vr_rrf_fuse(int device_id, const int64_t* ids, int32_t n_lists, int32_t depth, const int64_t* lims, int32_t n_groups,
                           int32_t k, float c, const float* weights, float* out_scores, int64_t* out_ids, int32_t* out_hits,
                           int32_t on_device, void* stream) {
    if (n_groups < 0 || n_lists < 0 || (n_groups > 0 && (!ids || !lims || !out_scores || !out_ids || !out_hits)))
        return fail(VR_ERR_INVALID, "bad arguments");
    if (n_groups == 0) {
        if (n_lists != 0) return fail(VR_ERR_INVALID, "%d lists in no group", (int)n_lists);
        return VR_OK;                             // no group: no launch
    }
    int max_entries = 0;
    VRCHK(rrf_check(lims, n_lists, n_groups, k, depth, c, weights, &max_entries));
    const size_t n_in = (size_t)n_lists * depth, n_out = (size_t)n_groups * k;
    if (!on_device)
        for (size_t e = 0; e < n_in; ++e)
            if (ids[e] < -1 || ids[e] > ((int64_t)1 << 31) - 2)
                return fail(VR_ERR_INVALID, "ids[%lld] = %lld outside [-1, 2^31 - 2]", (long long)e, (long long)ids[e]);
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    // no handle to keep scratch in: the call's own buffers, released when it returns (the stream is synchronised first)
    DevBuf b_ids, b_lims, b_w, b_os, b_oi, b_oh;
    std::vector<int> lims32((size_t)n_groups + 1);
    for (int32_t g = 0; g <= n_groups; ++g) lims32[(size_t)g] = (int)lims[g];
    RrfArgs p{};
    const int* glims = nullptr;
    VRCHK(stage_input(b_ids, ids, n_in, on_device, s, &p.ids));
    VRCHK(stage_input(b_lims, (const int*)lims32.data(), lims32.size(), 0, s, &glims));
    if (weights) VRCHK(stage_input(b_w, weights, (size_t)n_lists, 0, s, &p.weights));
    VRCHK(stage_output(b_os, out_scores, n_out, on_device, &p.out_scores));
    VRCHK(stage_output(b_oi, out_ids, n_out, on_device, &p.out_ids));
    VRCHK(stage_output(b_oh, out_hits, n_out, on_device, &p.out_hits));
    p.lims = glims; p.depth = depth; p.k = k; p.c = c;
    HIPCHK(launch_rrf_fuse(p, n_groups, max_entries, s));
    VRCHK(return_output(out_scores, p.out_scores, n_out, on_device, s));
    VRCHK(return_output(out_ids, p.out_ids, n_out, on_device, s));
    VRCHK(return_output(out_hits, p.out_hits, n_out, on_device, s));
    HIPCHK(hipStreamSynchronize(s));              // (lims and weights are the caller's host memory, the scratch is the call's)
    return VR_OK;
}

extern "C" int vr_topk_merge_keys(int device_id, const uint64_t* keys, int32_t n_parts, int32_t nq, int32_t k,
                                  float* out_scores, int64_t* out_ids, void* stream) {
    if (!keys || !out_scores || !out_ids || n_parts <= 0 || nq <= 0) return fail(VR_ERR_INVALID, "bad arguments");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_topk_merge_keys((const unsigned long long*)keys, n_parts, nq, k, out_scores, out_ids, (hipStream_t)stream));
    return VR_OK;
}
