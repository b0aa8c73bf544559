"""Document window search next to the grouped search of the same build, on one GPU, alternating in one process:

  (a) o0            HipIndex.search_groups_window(Q, 0, k = 10) next to search_groups(Q, 10): the one comparison where both sides
                    return the same thing (checked bit for bit)
  (b) o100 .. o5000 search_groups_window(Q, o, 10) at o = 100, 1 000 and 5 000 — nothing else answers these
  (c) f0.5, f0.01   search_groups_window(Q, 0, 10, filter) under one shared filter of density 0.5 / 0.01 — nothing else answers these

No figure of (b) or (c) is a bar for another.

    python tools/group_window_bench.py [--docs 10000 --pages 10 --nq 1000 --dim 2304 --reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/group_window_bench.py --reps 3 --only o0   # one case

Unit rows and queries (seeded), documents of `pages` adjacent rows.  Every timed call is one call between two device events.
Band documents re-scored and fp32 page dots per document returned come from group_window_search_stats; 32 queries per case are
checked against an fp64 brute force under the interval bar of tests/test_gpu_group_window_search.py: the document of fp64 score s
at position j has o + j in [#(E > s + 6e-7), #(E >= s - 6e-7) - 1] over the present documents, its score lies within 1e-5 of s
and its best row's fp64 score within 6e-7 of s.  Prints one JSON line."""
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


def check(ix, Q, S, pages, mask, o, k, f, tag):
    """one call: band documents and page dots per document returned, and the windows of the first 32 queries against the fp64
    scores S [32][rows] (mask: bool [rows] or None)"""
    ix.group_window_search_stats(reset=True)
    sc, ids, gr = ix.search_groups_window(Q, o, k, f)
    st = ix.group_window_search_stats()
    n = S.shape[0]
    Sm = S if mask is None else S.masked_fill(~mask[None, :], float("-inf"))
    E = Sm.view(n, -1, pages).max(dim=2).values                       # fp64 document scores, -inf where absent
    present = int((E[0] > float("-inf")).sum())
    live = gr[:n] >= 0
    s = torch.gather(E, 1, gr[:n].clamp(min=0))
    asc = E.sort(dim=1).values                                        # (absent documents sort first: they never count)
    docs = E.shape[1]
    lo = docs - torch.searchsorted(asc, (s + TOL).contiguous(), right=True)
    hi = docs - torch.searchsorted(asc, (s - TOL).contiguous(), right=False) - 1
    pos = o + torch.arange(k, device=S.device)[None, :]
    best = torch.gather(Sm, 1, ids[:n].clamp(min=0))
    ok = bool((((pos >= lo) & (pos <= hi)) | ~live).all()) and bool((((sc[:n].double() - s).abs() <= 1e-5) | ~live).all())
    ok = ok and bool((((best - s).abs() <= TOL) | ~live).all()) and bool(((ids[:n] // pages == gr[:n]) | ~live).all())
    ok = ok and bool((live.sum(1) == max(0, min(k, present - o))).all())
    returned = int((gr >= 0).sum())
    return {f"{tag}_band_documents_per_document_returned": round(st["documents"] / max(returned, 1), 2),
            f"{tag}_page_dots_per_document_returned": round(st["page_dots"] / max(returned, 1), 2),
            f"{tag}_band_documents_per_query": round(st["documents"] / max(st["queries"], 1), 1),
            f"{tag}_present_documents": present,
            f"{tag}_widened_intervals_on_32_queries": int(((hi > lo) & live).sum()), f"{tag}_ok": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10000)
    ap.add_argument("--pages", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated cases to run: o0, o100, o1000, o5000, f0.5, f0.01; default: all")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_window_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows, k = a.docs * a.pages, a.k
    res = {"docs": a.docs, "pages": a.pages, "rows": rows, "nq": a.nq, "dim": a.dim, "k": k, "reps": a.reps}
    C, Q = unit(rows, a.dim, g), unit(a.nq, a.dim, g)
    S = Q[:32].double() @ C.double().T
    masks = torch.stack([torch.rand(rows, generator=g, device="cuda") < d for d in (0.5, 0.01)])
    ix = HipIndex(a.dim, rows)
    ix.add(C)
    ix.set_groups(np.arange(a.docs + 1, dtype=np.int64) * a.pages)
    ix.set_filters(masks)
    only = [c for c in a.only.split(",") if c]
    want = lambda c: not only or c in only                            # noqa: E731
    offsets = [o for o in (0, 100, 1000, 5000) if o < a.docs and want(f"o{o}")]
    filters = [(i, d) for i, d in enumerate((0.5, 0.01)) if want(f"f{d}")]
    todo = []
    for o in offsets:
        todo.append((f"window_o{o}", (lambda o: (lambda: ix.search_groups_window(Q, o, k)))(o)))
        if o == 0:
            todo.append(("search_groups_next_to_o0", lambda: ix.search_groups(Q, k)))
    for i, d in filters:
        todo.append((f"window_o0_f{d}", (lambda i: (lambda: ix.search_groups_window(Q, 0, k, i)))(i)))
    res.update(alternate(todo, a.reps))
    for o in offsets:
        res.update(check(ix, Q, S, a.pages, None, o, k, None, f"window_o{o}"))
    for i, d in filters:
        res.update(check(ix, Q, S, a.pages, masks[i], 0, k, i, f"window_o0_f{d}"))
    if 0 in offsets:
        w, s = ix.search_groups_window(Q, 0, k), ix.search_groups(Q, k)
        res["window_o0_equals_search_groups"] = all(bool((x == y).all()) for x, y in zip((w[0].view(torch.int32), w[1], w[2]),
                                                                                           (s[0].view(torch.int32), s[1], s[2])))
        res["search_groups_stats"] = ix.group_search_stats()
    res["error_model"] = ix.error_model()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
