"""Windowed search next to the top-k search of the same k, on one GPU, alternating in one process:

  (a) window_o      HipIndex.search_window(Q, o, k = 100) at o = 0, 1 000, 10 000 and 50 000 — each next to search(Q, 100),
                    which answers o = 0 only
  (b) window_k1000  HipIndex.search_window(Q, 0, k = 1000) — next to search(Q, 1000)

The sides of each comparison return different things (but at o = 0): no figure is a bar for another.

    python tools/window_search_bench.py [--rows 100000 --nq 1000 --dim 2304 --reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/window_search_bench.py --reps 3 --only 50000   # one case

Unit rows and queries (seeded).  Every timed window is one call between two device events.  Band candidates re-scored per row
returned and rows certainly ahead come from window_search_stats; 32 queries per case are checked against an fp64 brute force under
the interval bar of tests/test_gpu_window_search.py: the row of fp64 score s at position j has o + j in [#(S > s + 6e-7),
#(S >= s - 6e-7) - 1], and its score lies within 1e-5 of s.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def check(ix, Q, S, o, k, tag):
    """one call: candidates per row returned, and the windows of the first 32 queries against the fp64 scores S [32][rows]"""
    ix.window_search_stats(reset=True)
    sc, ids = ix.search_window(Q, o, k)
    st = ix.window_search_stats()
    n = S.shape[0]
    live = ids[:n] >= 0
    s = torch.gather(S, 1, ids[:n].clamp(min=0))
    asc = S.sort(dim=1).values
    rows = S.shape[1]
    lo = rows - torch.searchsorted(asc, (s + TOL).contiguous(), right=True)
    hi = rows - torch.searchsorted(asc, (s - TOL).contiguous(), right=False) - 1
    pos = o + torch.arange(k, device=S.device)[None, :]
    ok = bool((((pos >= lo) & (pos <= hi)) | ~live).all()) and bool((((sc[:n].double() - s).abs() <= 1e-5) | ~live).all())
    ok = ok and bool((live.sum(1) == max(0, min(k, rows - o))).all())
    returned = int((ids >= 0).sum())
    return {f"{tag}_candidates_per_row_returned": round(st["candidates"] / max(returned, 1), 1),
            f"{tag}_candidates_per_query": round(st["candidates"] / max(st["queries"], 1), 1),
            f"{tag}_rows_certainly_ahead_per_query": round(st["ahead"] / max(st["queries"], 1), 1),
            f"{tag}_widened_intervals_on_32_queries": int(((hi > lo) & live).sum()), f"{tag}_ok": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated cases to run: offsets of (a), or k1000; default: all")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"rows": a.rows, "nq": a.nq, "dim": a.dim, "reps": a.reps}
    C, Q = unit(a.rows, a.dim, g), unit(a.nq, a.dim, g)
    S = Q[:32].double() @ C.double().T
    ix = HipIndex(a.dim, a.rows)
    ix.add(C)
    only = [c for c in a.only.split(",") if c]
    offsets = [o for o in (0, 1000, 10000, 50000) if o < a.rows and (not only or str(o) in only)]
    todo = []
    for o in offsets:
        todo += [(f"window_o{o}_k100", (lambda o: (lambda: ix.search_window(Q, o, 100)))(o)), (f"search_k100_next_to_o{o}", lambda: ix.search(Q, 100))]
    k1000 = not only or "k1000" in only
    if k1000:
        todo += [("window_o0_k1000", lambda: ix.search_window(Q, 0, 1000)), ("search_k1000", lambda: ix.search(Q, 1000))]
    res.update(alternate(todo, a.reps))
    for o in offsets:
        res.update(check(ix, Q, S, o, 100, f"window_o{o}_k100"))
    if k1000:
        res.update(check(ix, Q, S, 0, 1000, "window_o0_k1000"))
        w, s = ix.search_window(Q, 0, 1000), ix.search(Q, 1000)
        res["window_o0_k1000_equals_search"] = bool((w[1] == s[1]).all()) and bool((w[0].view(torch.int32) == s[0].view(torch.int32)).all())
    res["error_model"] = ix.error_model()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
