"""Rank search next to the searches a caller would use instead, on one GPU, alternating in one process:

  (a) rank_top      HipIndex.rank_rows(Q, one target per query taken from the query's search(k = 10) result): the evaluation case,
                    a positive near the top — next to search(Q, 10)
  (b) rank_random   HipIndex.rank_rows(Q, one uniformly random target per query): the expensive corner, the band around a
                    mid-ranked score holds a good part of the index — next to search(Q, 1000), which cannot answer the question
  (c) count_c       HipIndex.count_range(Q, t_c) at the thresholds of tools/range_search_bench.py that return about c = 10 and
                    c = 1000 rows per query — next to search_range(Q, t_c, sort=False)

The sides of each comparison return different things: no figure is a bar for another.

    python tools/rank_search_bench.py [--rows 100000 --nq 1000 --dim 2304 --reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rank_search_bench.py --reps 3 --only b   # one case

Unit rows and queries (seeded).  Every timed window is one call between two device events.  Band candidates re-scored per pair
come from rank_search_stats; 32 queries per case are checked against an fp64 brute force under the interval bar of
tests/test_gpu_rank_search.py: the rank (count) lies in [#(S > s + 6e-7), #(S >= s - 6e-7) - 1] ([#(S >= t + 6e-7), #(S >= t - 6e-7)]).
Prints one JSON line."""
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


def check_ranks(ix, Q, S, targets, tag):
    """one call: candidates per pair, and the ranks of the first 32 queries against the fp64 scores S [32][rows]"""
    ix.rank_search_stats(reset=True)
    sc, rk = ix.rank_rows(Q, targets)
    st = ix.rank_search_stats()
    n = S.shape[0]
    s = S[torch.arange(n, device=S.device), targets[:n]]
    lo = (S > (s + TOL)[:, None]).sum(1)
    hi = (S >= (s - TOL)[:, None]).sum(1) - 1
    ok = bool(((rk[:n] >= lo) & (rk[:n] <= hi)).all()) and bool(((sc[:n].double() - s).abs() <= 1e-5).all())
    return {f"{tag}_candidates_per_pair": round(st["candidates"] / max(st["pairs"], 1), 1),
            f"{tag}_rank": {"median": int(rk.median()), "min": int(rk.min()), "max": int(rk.max())},
            f"{tag}_widened_intervals_on_32_queries": int((hi > lo).sum()), f"{tag}_ok": ok}


def check_counts(ix, Q, S, t, tag):
    ix.rank_search_stats(reset=True)
    cnt = ix.count_range(Q, t)
    st = ix.rank_search_stats()
    same = bool((cnt == (lambda l: l[1:] - l[:-1])(ix.search_range(Q, t, sort=False)[0])).all())
    n = S.shape[0]
    t32 = float(torch.tensor(t, dtype=torch.float32))
    lo, hi = (S >= t32 + TOL).sum(1), (S >= t32 - TOL).sum(1)
    ok = same and bool(((cnt[:n] >= lo) & (cnt[:n] <= hi)).all())
    return {f"{tag}_threshold": round(float(t), 6), f"{tag}_rows_per_query": round(float(cnt.double().mean()), 1),
            f"{tag}_candidates_per_pair": round(st["candidates"] / max(st["pairs"], 1), 1),
            f"{tag}_equals_the_range_search": same, f"{tag}_ok": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="abc", help="the cases to run: any of a, b, c")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"rows": a.rows, "nq": a.nq, "dim": a.dim, "reps": a.reps}
    C, Q = unit(a.rows, a.dim, g), unit(a.nq, a.dim, g)
    S = Q[:32].double() @ C.double().T
    sample = S.flatten().sort(descending=True).values
    thr = {c: float(sample[32 * c - 1].float()) for c in (10, 1000) if c < a.rows}
    ix = HipIndex(a.dim, a.rows)
    ix.add(C)
    top = ix.search(Q, 10)[1]
    pick = torch.randint(0, 10, (a.nq,), generator=g, device="cuda")
    near_top = top[torch.arange(a.nq, device="cuda"), pick].contiguous()
    anywhere = torch.randint(0, a.rows, (a.nq,), generator=g, device="cuda")
    todo = []
    if "a" in a.only:
        todo += [("rank_top", lambda: ix.rank_rows(Q, near_top)), ("search_k10", lambda: ix.search(Q, 10))]
    if "b" in a.only:
        todo += [("rank_random", lambda: ix.rank_rows(Q, anywhere)), ("search_k1000", lambda: ix.search(Q, 1000))]
    if "c" not in a.only:
        thr = {}
    for c, t in thr.items():
        todo.append((f"count_{c}", (lambda t: (lambda: ix.count_range(Q, t)))(t)))
        todo.append((f"range_{c}", (lambda t: (lambda: ix.search_range(Q, t, sort=False)))(t)))
    res.update(alternate(todo, a.reps))
    if "a" in a.only:
        res.update(check_ranks(ix, Q, S, near_top, "rank_top"))
        res["rank_top_equals_search_position"] = bool((ix.rank_rows(Q, near_top)[1] == pick).all())
    if "b" in a.only:
        res.update(check_ranks(ix, Q, S, anywhere, "rank_random"))
    for c, t in thr.items():
        res.update(check_counts(ix, Q, S, t, f"count_{c}"))
    res["error_model"] = ix.error_model()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
