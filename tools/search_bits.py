"""Every tensor and every stats counter the band searches return on one small seeded index, for comparing two builds bit for bit.

    python tools/search_bits.py --out A.npz                              # this tree's library
    VISRAG_HIP_LIB=/path/to/libvisrag_hip.so python tools/search_bits.py --out B.npz
    python tools/search_bits.py --compare A.npz B.npz                    # exit status 1 on any difference

The entry points: search (k > 26), search_filtered, search_groups; search_range, search_groups_range; rank_rows, count_range,
rank_groups, count_groups_range; search_window, search_groups_window; search_multi, search_multi_groups (evidence, both fusions)
— under the default error model, under a caller's eps_rel and, for the first three, with certification off.  The counters of
the matching *_search_stats are saved next to the tensors: they show a changed path even where the answer survives.

The index is the smallest at which these kernels take every path: 8 195 rows (two chunks of 4 096 and a tail of 3), 4 099
documents of unequal length (1, 2, 65 and 300 pages: past one ballot step, two chunks of documents), dim 320 (an index takes
multiples of 64; 80 float4 chunks: lanes 0..15 alone hold a second one) and 2 304; exact duplicates of one row across document
and chunk borders (both window edges and the k-th place fall inside a tie tier); 40 and 2 100 near-duplicates of two queries'
best rows (the second gather, and a flagged query); filters of density 0.5 and 0.01, an empty one, -1, and — on the device,
where the host cannot see it — an index out of range; offsets 0, 7, 4 000 and 9 000; k = 10, 100 and once 1 000; sub-query groups of 1, 3 and 5; thresholds that keep nothing,
about 50 rows, NaN and +inf; a zero row (a score's sign: a fp32 score here is never -0.0, its chain starts from +0.0).
Queries live on the device, so that thresholds and filter indices reach the kernels unchecked."""
import argparse
import os
import sys

import numpy as np

ROWS, NQ, DUPS = 8195, 24, (10, 11, 64, 65, 300, 4094, 4095, 4096, 4097, 8192, 8193, 8194)
GROUP_SIZES = [2] * 2000 + [65] + [2] * 1733 + [300] + [1] * 364
SUB_LIMS = np.cumsum([0, 1, 3, 5, 1, 3, 5, 1, 3, 2])
OFFSETS = [0, 7, 4000, 9000]


def make_data(dim, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((ROWS, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = g.standard_normal((NQ, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for r in DUPS[1:]:                                               # exact duplicates: one tie tier of 12 rows
        x[r] = x[DUPS[0]]
    q[0] = x[DUPS[0]]
    x[100:140] = x[100] + 1e-4 * g.standard_normal((40, dim)).astype(np.float32)          # inside the error band of q[1]
    q[1] = x[100] / np.linalg.norm(x[100])
    # ... and more than a select can hold, as rows (2 100) and as documents (1 050 of two pages): the query is flagged
    x[1000:3100] = x[1000] + 1e-4 * g.standard_normal((2100, dim)).astype(np.float32)
    q[2] = x[1000] / np.linalg.norm(x[1000])
    x[7000] = 0.0
    q[3, : dim // 2] = 0.0
    masks = np.stack([g.random(ROWS) < 0.5, g.random(ROWS) < 0.01, np.zeros(ROWS, dtype=bool)])
    return x, q, masks


def run(dim, seed, out):
    import torch
    from visrag_amd.engine import HipIndex

    x, q, masks = make_data(dim, seed)
    assert sum(GROUP_SIZES) == ROWS and len(GROUP_SIZES) == 4099
    ix = HipIndex(dim, ROWS)
    ix.add(x)
    ix.set_groups(np.concatenate([[0], np.cumsum(GROUP_SIZES)]))
    ix.set_filters(masks)
    Q = torch.from_numpy(q).cuda()
    S = q.astype(np.float64) @ x.astype(np.float64).T
    thr50 = np.sort(S, axis=1)[:, -50].astype(np.float32)
    thr = thr50.copy()
    thr[4], thr[5], thr[6] = 2.0, np.nan, np.inf                     # nothing, and the two that are not finite
    fq = np.array([0, 1, 2, -1] * 6, dtype=np.int64)
    fq[2] = -1                                                       # (the query of the 2 100 near-duplicates sees them all)
    fq_bad = fq.copy()
    fq_bad[8] = 7                                                    # no such filter: an empty result (device callers only)
    fg, fg_bad = fq[:9], fq_bad[:9].copy()
    fg_bad[4] = 7
    off = np.array(OFFSETS * 6, dtype=np.int64)
    targets = np.stack([np.argsort(-S, axis=1)[:, 5], np.full(NQ, DUPS[4]), np.full(NQ, 1500)], axis=1)
    goff = np.concatenate([[0], np.cumsum(GROUP_SIZES)])
    tgroups = np.searchsorted(goff, targets, side="right") - 1
    cthr = np.stack([thr50, np.full(NQ, 2.0, dtype=np.float32), np.zeros(NQ, dtype=np.float32)], axis=1)

    def keep(name, res):
        for i, t in enumerate(res if isinstance(res, tuple) else (res,)):
            out[f"{name}.{i}"] = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    def stats(name, d):
        out[f"{name}.stats"] = np.array([d[k] for k in sorted(d)], dtype=np.int64)

    class unchecked:                                                 # the binding checks filter indices; the device path cannot
        def __enter__(self):
            self.n, ix.n_filters = ix.n_filters, 0

        def __exit__(self, *a):
            ix.n_filters = self.n

    for mode, eps in (("default", None), ("eps_rel", 0.01), ("off", -1.0)):
        ix.set_search_eps(eps)
        for st in ("search_stats", "filter_search_stats", "group_search_stats", "range_search_stats", "group_range_search_stats",
                   "rank_search_stats", "group_rank_search_stats", "window_search_stats", "group_window_search_stats",
                   "multi_search_stats", "multi_group_search_stats"):
            getattr(ix, st)(reset=True)
        t = f"d{dim}.{mode}"
        for k in (100, 1000) if mode == "default" else (100,):
            keep(f"{t}.search.k{k}", ix.search(Q, k))
        for k in (10, 100):
            keep(f"{t}.filtered.k{k}", ix.search_filtered(Q, k, fq))
            keep(f"{t}.groups.k{k}", ix.search_groups(Q, k))
        with unchecked():
            keep(f"{t}.filtered.bad", ix.search_filtered(Q, 10, fq_bad))
        stats(f"{t}.search", ix.search_stats())
        stats(f"{t}.filtered", ix.filter_search_stats())
        stats(f"{t}.groups", ix.group_search_stats())
        if mode == "off":
            continue
        for name, f in (("nofilter", None), ("filter", fq), ("bad", fq_bad)):
            with unchecked():
                keep(f"{t}.range.{name}", ix.search_range(Q, thr, f, sort=False))
                keep(f"{t}.groups_range.{name}", ix.search_groups_range(Q, thr, f, sort=False))
                keep(f"{t}.rank_rows.{name}", ix.rank_rows(Q, targets, filter_of_query=f))
                keep(f"{t}.rank_groups.{name}", ix.rank_groups(Q, tgroups, filter_of_query=f))
                for strict in (False, True):
                    keep(f"{t}.count_range.{name}.{int(strict)}", ix.count_range(Q, cthr, filter_of_query=f, strict=strict))
                    keep(f"{t}.count_groups.{name}.{int(strict)}", ix.count_groups_range(Q, cthr, filter_of_query=f, strict=strict))
                for k in (10, 100):
                    keep(f"{t}.window.{name}.k{k}", ix.search_window(Q, off, k, f))
                    keep(f"{t}.groups_window.{name}.k{k}", ix.search_groups_window(Q, off, k, f))
        for name, f in (("nofilter", None), ("filter", fg), ("bad", fg_bad)):
            for fuse in ("max", "min"):
                for k in (10, 100):
                    with unchecked():
                        keep(f"{t}.multi.{name}.{fuse}.k{k}", ix.search_multi(Q, SUB_LIMS, k, fuse, f))
                        keep(f"{t}.multi_groups.{name}.{fuse}.k{k}", ix.search_multi_groups(Q, SUB_LIMS, k, fuse, f, evidence=True))
        if mode == "default":
            keep(f"{t}.window.k1000", ix.search_window(Q, off, 1000))
            keep(f"{t}.groups_window.k1000", ix.search_groups_window(Q, off, 1000))
            keep(f"{t}.multi.k1000", ix.search_multi(Q, SUB_LIMS, 1000))
            keep(f"{t}.multi_groups.k1000", ix.search_multi_groups(Q, SUB_LIMS, 1000, evidence=True))
        for st in ("range", "group_range", "rank", "group_rank", "window", "group_window", "multi", "multi_group"):
            stats(f"{t}.{st}", getattr(ix, f"{st}_search_stats")())
    ix.close()


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for name in sorted(set(A.files) & set(B.files)):
        x, y = A[name], B[name]
        if x.dtype == np.float32 and y.dtype == np.float32:
            x, y = x.view(np.int32), y.view(np.int32)
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y):
            bad.append(name)
    print(f"{len(A.files)} arrays in {a}, {len(B.files)} in {b}: " + (f"{len(bad)} DIFFER: {bad[:20]}" if bad else "all equal"))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    run(320, 1, out)
    run(2304, 2, out)
    np.savez(args.out, **out)
    flagged = {k: out[k].tolist() for k in out if k.endswith(".stats") and ".default." in k and k.startswith("d320")}
    print(f"{len(out)} arrays -> {args.out}; d320 default counters: {flagged}")


if __name__ == "__main__":
    main()
