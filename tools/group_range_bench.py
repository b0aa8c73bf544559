"""Document range search next to the document count and the document window search of the same build, on one GPU, alternating in
one process:

  range10, range100, range1000   HipIndex.search_groups_range(Q, t) at per-query thresholds that about 10 / 100 / 1 000 documents
                                 reach (the scores at ranks 9, 99 and 999 of the query's document ranking), next to
                                 count_groups_range(Q, t) at the same thresholds (the same band, no output) and
                                 search_groups_window(Q, 0, k) at the matching k

The three return different things — the documents, how many there are, the k best whatever they score: no figure is a bar for
another.  The one checkable relation is asserted on all queries: np.diff(lims) equals count_groups_range's counts.

    python tools/group_range_bench.py [--docs 10000 --pages 10 --nq 1000 --dim 2304 --reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/group_range_bench.py --reps 3 --only range100   # one case

Unit rows and queries (seeded), documents of `pages` adjacent rows.  Every timed call is one call between two device events
(cuda queries: the range call's own synchronisations, once per block of 256 queries, are inside).  Band documents re-scored and
fp32 page dots per document returned come from group_range_search_stats; 32 queries per case are checked against an fp64 brute
force under the bar of tests/test_gpu_group_range_search.py: membership as in fp64 but for documents within 3e-7 of the
threshold, scores within 1e-5 of the fp64 document score, the best row's fp64 score within 6e-7 of it.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visrag_amd.engine import HipIndex  # noqa: E402

TOL, NEAR, ATOL = 6e-7, 3e-7, 1e-5


def unit(n, dim, g):
    x = torch.randn((n, dim), generator=g, device="cuda")
    return x / x.norm(dim=1, keepdim=True)


def alternate(todo, reps):
    for _, fn in todo:                                                # warm-up: code objects, scratch buffers
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in todo}
    for _ in range(reps):
        for name, fn in todo:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    out = {}
    for name, v in ms.items():
        v = sorted(v)
        out[name + "_ms"] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
    return out


def check_range(ix, Q, E, S, pages, thr, tag):
    """one call: counters, lims against the counts on ALL queries, and the first 32 queries against the fp64 document scores E
    [32][docs] (S [32][rows]: the pages')"""
    ix.group_range_search_stats(reset=True)
    lims, sc, rows, gr = ix.search_groups_range(Q, thr, sort=False)
    st = ix.group_range_search_stats()
    cnt = ix.count_groups_range(Q, thr)
    per = lims[1:] - lims[:-1]
    assert torch.equal(per, cnt), "np.diff(lims) is count_groups_range"
    total = int(lims[-1])
    n, docs = E.shape
    t = torch.as_tensor(thr[:n], device=E.device).double()[:, None]
    want = E >= t
    got = torch.zeros_like(want)
    seg = torch.repeat_interleave(torch.arange(n, device=E.device), per[:n])
    m = int(lims[n])
    got[seg, gr[:m]] = True
    differ = got != want
    ok = bool(((E - t).abs()[differ] <= NEAR).all())
    s = E[seg, gr[:m]]
    ok = ok and bool(((sc[:m].double() - s).abs() <= ATOL).all()) and bool(((S[seg, rows[:m]] - s).abs() <= TOL).all())
    ok = ok and bool((rows[:m] // pages == gr[:m]).all())
    return {f"{tag}_returned_per_query": {"min": int(per.min()), "median": int(per.median()), "max": int(per.max())},
            f"{tag}_band_documents_per_document_returned": round(st["documents"] / max(total, 1), 3),
            f"{tag}_page_dots_per_document_returned": round(st["page_dots"] / max(total, 1), 3),
            f"{tag}_excused_on_32_queries": int(differ.sum()), f"{tag}_lims_equal_counts": True, f"{tag}_ok": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10000)
    ap.add_argument("--pages", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated cases to run: range10, range100, range1000; default: all")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_range_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = a.docs * a.pages
    res = {"docs": a.docs, "pages": a.pages, "rows": rows, "nq": a.nq, "dim": a.dim, "reps": a.reps}
    C, Q = unit(rows, a.dim, g), unit(a.nq, a.dim, g)
    S = Q[:32].double() @ C.double().T
    E = S.view(32, -1, a.pages).max(dim=2).values                     # fp64 document scores
    ix = HipIndex(a.dim, rows)
    ix.add(C)
    ix.set_groups(np.arange(a.docs + 1, dtype=np.int64) * a.pages)
    only = [c for c in a.only.split(",") if c]
    depth = {f"range{d}": min(d, a.docs) for d in (10, 100, 1000)}
    todo, checks = [], []
    for case, d in depth.items():
        if only and case not in only:
            continue
        thr = ix.search_groups_window(Q, d - 1, 1)[0][:, 0].cpu().numpy()
        todo.append((case, (lambda t: (lambda: ix.search_groups_range(Q, t, sort=False)))(thr)))
        todo.append((f"{case}_sorted", (lambda t: (lambda: ix.search_groups_range(Q, t)))(thr)))
        todo.append((f"count_next_to_{case}", (lambda t: (lambda: ix.count_groups_range(Q, t)))(thr)))
        todo.append((f"window_k{d}_next_to_{case}", (lambda k: (lambda: ix.search_groups_window(Q, 0, k)))(d)))
        checks.append((lambda t, c: (lambda: check_range(ix, Q, E, S, a.pages, t, c)))(thr, case))
    res.update(alternate(todo, a.reps))
    for fn in checks:
        res.update(fn())
    res["error_model"] = ix.error_model()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
