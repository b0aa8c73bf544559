"""Document-level search against the row search it replaces, on one GPU, alternating the two in one process:

  A  HipIndex.search_groups(Q, k)                       exact: the k best documents, each by its best page
  B  HipIndex.search(Q, k * pages) + a collapse on the device (best page per document of the k * pages rows, top k):
     what a caller could do before — NOT exact: a document whose best page ranks below the cut is lost

    python tools/group_search_bench.py [--docs 10000 --pages 10 --nq 1000 --dim 2304 --k 10 --reps 10 --noise 0.05]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/group_search_bench.py --reps 3 --only groups     # kernel split

The corpus is decks: page = its document's unit vector + noise * N(0, 1), renormalised (seeded).  Each timed window ends in a
device synchronise.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visrag_amd.engine import HipIndex  # noqa: E402


def collapse(sc, ids, pages, k):
    """best row per document among the returned rows (they come best first), then the k best documents"""
    doc = ids // pages
    first = torch.ones_like(doc, dtype=torch.bool)
    order = torch.argsort(doc, dim=1, stable=True)                    # stable: inside a document the best row stays first
    d_sorted = torch.gather(doc, 1, order)
    first_sorted = torch.ones_like(first)
    first_sorted[:, 1:] = d_sorted[:, 1:] != d_sorted[:, :-1]
    first.scatter_(1, order, first_sorted)
    s = torch.where(first, sc, torch.full_like(sc, float("-inf")))
    top, pos = torch.topk(s, k, dim=1)
    return top, torch.gather(ids, 1, pos), torch.gather(doc, 1, pos)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10000)
    ap.add_argument("--pages", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--only", choices=["both", "groups", "rows"], default="both")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    n = a.docs * a.pages
    base = torch.randn((a.docs, a.dim), generator=g, device="cuda")
    base = base / base.norm(dim=1, keepdim=True)
    C = base.repeat_interleave(a.pages, dim=0) + a.noise * torch.randn((n, a.dim), generator=g, device="cuda")
    C = C / C.norm(dim=1, keepdim=True)
    Q = torch.randn((a.nq, a.dim), generator=g, device="cuda")
    Q = Q / Q.norm(dim=1, keepdim=True)
    ix = HipIndex(a.dim, n)
    ix.add(C)
    ix.set_groups(torch.arange(a.docs + 1).numpy() * a.pages)
    deep = a.k * a.pages

    def run_groups():
        return ix.search_groups(Q, a.k)

    def run_rows():
        return collapse(*ix.search(Q, deep), a.pages, a.k)

    todo = [("search_groups", run_groups)] * (a.only != "rows") + [("search_deep_collapse", run_rows)] * (a.only != "groups")
    for _, fn in todo:                                                # warm-up: code objects, scratch buffers
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in todo}
    for _ in range(a.reps):                                           # alternate the two
        for name, fn in todo:
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    res = {"docs": a.docs, "pages": a.pages, "nq": a.nq, "dim": a.dim, "k": a.k, "reps": a.reps, "noise": a.noise}
    for name, v in ms.items():
        v = sorted(v)
        res[name + "_ms"] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
    if a.only == "both":
        gs, gi, gg = run_groups()
        rs, ri, rg = run_rows()
        res["queries_where_the_collapse_differs"] = int((gg != rg).any(dim=1).sum())
        ref = (Q[:32].double() @ C.double().T).view(32, a.docs, a.pages).amax(dim=2).topk(a.k, dim=1).indices
        res["groups_match_fp64_on_32_queries"] = bool(torch.equal(ref, gg[:32]))
    res["group_search_stats"] = ix.group_search_stats()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
