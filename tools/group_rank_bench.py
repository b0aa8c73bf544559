"""Document rank search next to the document window search of the same build, on one GPU, alternating in one process:

  (a) own        HipIndex.rank_groups(Q, g): one target per query taken from the query's own search_groups(k = 10) (entry q % 10),
                 next to search_groups_window(Q, 0, 10)
  (b) random     rank_groups(Q, g): one uniformly random document per query (ranks spread over the whole ranking), next to
                 search_groups_window(Q, docs / 2, 10)
  (c) count10,   count_groups_range(Q, t) at per-query thresholds that about 10 / about 1 000 documents reach (the scores at
      count1000  ranks 9 and 999), next to search_groups_window(Q, 10, 10) / (Q, 1 000, 10)

The window search at the matching depth returns something else — WHICH documents stand there, not where a named one stands: no
figure is a bar for another.

    python tools/group_rank_bench.py [--docs 10000 --pages 10 --nq 1000 --dim 2304 --reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/group_rank_bench.py --reps 3 --only random   # one case

Unit rows and queries (seeded), documents of `pages` adjacent rows.  Every timed call is one call between two device events.
Band documents re-scored and fp32 page dots per pair come from group_rank_search_stats; 32 queries per case are checked against
an fp64 brute force under the interval bar of tests/test_gpu_group_rank_search.py: the rank of a document of fp64 score s lies in
[#(E > s + 6e-7), #(E >= s - 6e-7) - 1], its score within 1e-5 of s, its best row's fp64 score within 6e-7 of s; a count at
threshold t lies in [#(E >= t + 6e-7), #(E >= t - 6e-7)].  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visrag_amd.engine import HipIndex  # noqa: E402

TOL = 6e-7


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


def counters(ix, fn, tag):
    ix.group_rank_search_stats(reset=True)
    out = fn()
    st = ix.group_rank_search_stats()
    return out, {f"{tag}_band_documents_per_pair": round(st["documents"] / max(st["pairs"], 1), 2),
                 f"{tag}_page_dots_per_pair": round(st["page_dots"] / max(st["pairs"], 1), 2)}


def check_ranks(ix, Q, E, S, pages, groups, tag):
    """one call: counters, and the first 32 queries against the fp64 document scores E [32][docs] (S [32][rows]: the pages')"""
    (sc, rows, rk), res = counters(ix, lambda: ix.rank_groups(Q, groups), tag)
    n, docs = E.shape
    g = torch.as_tensor(groups[:n], device=E.device)[:, None]
    s = torch.gather(E, 1, g)
    asc = E.sort(dim=1).values
    lo = docs - torch.searchsorted(asc, (s + TOL).contiguous(), right=True)
    hi = docs - torch.searchsorted(asc, (s - TOL).contiguous(), right=False) - 1
    r, row = rk[:n, None], rows[:n, None]
    ok = bool(((r >= lo) & (r <= hi)).all()) and bool(((sc[:n, None].double() - s).abs() <= 1e-5).all())
    ok = ok and bool(((torch.gather(S, 1, row) - s).abs() <= TOL).all()) and bool((row // pages == g).all())
    res.update({f"{tag}_median_rank": int(rk.median()), f"{tag}_max_rank": int(rk.max()),
                f"{tag}_widened_intervals_on_32_queries": int((hi > lo).sum()), f"{tag}_ok": ok})
    return res


def check_counts(ix, Q, E, thr, tag):
    cnt, res = counters(ix, lambda: ix.count_groups_range(Q, thr), tag)
    n = E.shape[0]
    t = torch.as_tensor(thr[:n], device=E.device).double()[:, None]
    lo, hi = (E >= t + TOL).sum(1), (E >= t - TOL).sum(1)
    ok = bool(((cnt[:n] >= lo) & (cnt[:n] <= hi)).all())
    res.update({f"{tag}_median_count": int(cnt.median()), f"{tag}_widened_intervals_on_32_queries": int((hi > lo).sum()), f"{tag}_ok": ok})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10000)
    ap.add_argument("--pages", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated cases to run: own, random, count10, count1000; default: all")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_rank_bench needs a GPU: there is no CPU fallback")
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
    want = lambda c: not only or c in only                            # noqa: E731
    own = ix.search_groups(Q, 10)[2][torch.arange(a.nq), torch.arange(a.nq) % 10].cpu().numpy().astype(np.int64)
    rnd = np.random.default_rng(1).integers(0, a.docs, a.nq).astype(np.int64)
    depth = {"count10": min(10, a.docs), "count1000": min(1000, a.docs)}
    thr = {c: ix.search_groups_window(Q, d - 1, 1)[0][:, 0].cpu().numpy() for c, d in depth.items()}
    todo, checks = [], []
    for case, groups, o in (("own", own, 0), ("random", rnd, a.docs // 2)):
        if want(case):
            todo.append((f"rank_{case}", (lambda t: (lambda: ix.rank_groups(Q, t)))(groups)))
            todo.append((f"window_o{o}_next_to_{case}", (lambda o: (lambda: ix.search_groups_window(Q, o, 10)))(o)))
            checks.append((lambda t, c: (lambda: check_ranks(ix, Q, E, S, a.pages, t, f"rank_{c}")))(groups, case))
    for case, d in depth.items():
        if want(case):
            todo.append((case, (lambda t: (lambda: ix.count_groups_range(Q, t)))(thr[case])))
            todo.append((f"window_o{d}_next_to_{case}", (lambda o: (lambda: ix.search_groups_window(Q, min(o, a.docs - 1), 10)))(d)))
            checks.append((lambda t, c: (lambda: check_counts(ix, Q, E, t, c)))(thr[case], case))
    res.update(alternate(todo, a.reps))
    for fn in checks:
        res.update(fn())
    res["error_model"] = ix.error_model()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
