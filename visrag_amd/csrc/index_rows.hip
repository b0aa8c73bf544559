// Editing the index in place, host side (vr_index_remove / vr_index_update / vr_index_get_rows of include/visrag_hip.h): the checks,
// the staging and the choice of launches; index_edit.hip has the kernels and why no launch reads what it writes.
#include "index.h"

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
    VRCHK(ix->edit.ids.reserve(ids.size() * 4));
    HIPCHK(hipMemcpyAsync(ix->edit.ids.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, s));
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
    const int* rem_dev = ix->edit.ids.as<int>();
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
    const bool moves = rem[0] < new_n, filters = ix->flt.n_filters > 0 && new_n > 0;
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
        VRCHK(ix->edit.bits2.reserve(new_words * (size_t)ix->flt.n_filters * 4));
        HIPCHK(launch_filter_compact(ix->flt.bits.as<uint32_t>(), words, (int)ix->flt.n_filters, ix->edit.ids.as<int>(), (int)rem.size(), new_n,
                                     ix->edit.bits2.as<uint32_t>(), s));
        std::swap(ix->flt.bits, ix->edit.bits2);
        HIPCHK(launch_filter_prepare(ix->flt.bits.as<uint32_t>(), new_words, (int)ix->flt.n_filters, new_n, ix->flt.count.as<int>(), s));
    }
    ix->n = new_n;
    ix->grp.n_groups = 0;             // a removal can empty a group: the caller sets the offsets of the rows that remain
    ix->rng.total = -1;               // its ids name rows as they were
    ix->grng.total = -1;              // ... and so do the document range result's
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
    const float* src = nullptr;
    VRCHK(stage_input(ix->edit.rows, reps, (size_t)n * ix->dim, on_device, s, &src));
    HIPCHK(launch_rows_update(src, ix->edit.ids.as<int>(), n, ix->dim, ix->f32.as<float>(), ix->bf16.p, s));
    VRCHK(recompute_error_model(ix, s));          // (an overwritten row may have been the largest)
    ix->rng.total = -1;
    ix->grng.total = -1;
    if (ix->huge_seen) *ix->huge_seen = 0;
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// rows ids[0..n) of one store to `out`: gathered straight into a device array, or through the bounded staging to a host array
static int get_rows(vr_index_t ix, const void* store, size_t row_bytes, int64_t n, void* out, int32_t on_device, hipStream_t s) {
    if (on_device) {
        HIPCHK(launch_rows_gather(store, row_bytes, ix->edit.ids.as<int>(), n, out, s));
        return VR_OK;
    }
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(EDIT_SCRATCH / row_bytes));
    VRCHK(ix->edit.rows.reserve((size_t)std::min(n, chunk) * row_bytes));
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t cn = std::min(chunk, n - c0);
        HIPCHK(launch_rows_gather(store, row_bytes, ix->edit.ids.as<int>() + c0, cn, ix->edit.rows.p, s));
        HIPCHK(hipMemcpyAsync((char*)out + (size_t)c0 * row_bytes, ix->edit.rows.p, (size_t)cn * row_bytes, hipMemcpyDeviceToHost, s));
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
