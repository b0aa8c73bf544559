"""Rank-fusion search next to the search that makes its lists and next to the host workaround, on one GPU, alternating in one
process:

  (a) search_rrf     HipIndex.search_rrf(sub-queries, lims, k = 10, depth = 100)
  (b) pool           HipIndex.search(sub-queries, k = 100) — the very call that produces search_rrf's lists, so (a) - (b) is the
                     fusion stage (its kernel alone: a `rocprofv3 --kernel-trace --stats` run of this tool, rrf_fuse_kernel)
  (c) workaround     the same search, the lists copied to the host, documents.rrf_runs: wall-clock time

    python tools/rrf_search_bench.py [--rows 100000 --groups 1000 --m 4 --dim 2304 --k 10 --depth 100 --reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rrf_search_bench.py --reps 3 --no-workaround

Rows and sub-queries are unit vectors (seeded).  (a) and (b) are one call between two device events each; (c) is timed on the
host clock.  The device result must equal the workaround's on every group — score bits, ids, hits — or the tool fails.  Prints
one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visrag_amd.documents import rrf_runs  # noqa: E402
from visrag_amd.engine import HipIndex  # noqa: E402


def unit(n, dim, g):
    x = torch.randn((n, dim), generator=g, device="cuda")
    return x / x.norm(dim=1, keepdim=True)


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-workaround", action="store_true", help="time the two device calls only (profiling runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrf_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"rows": a.rows, "groups": a.groups, "m": a.m, "dim": a.dim, "k": a.k, "depth": a.depth, "reps": a.reps}
    C = unit(a.rows, a.dim, g)
    Q = unit(a.groups * a.m, a.dim, g)
    lims = np.arange(a.groups + 1, dtype=np.int64) * a.m
    ix = HipIndex(a.dim, a.rows)
    ix.add(C)

    def wall():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ids = ix.search(Q, a.depth)
        out = rrf_runs(ids.cpu().numpy(), lims, a.k)
        return (time.perf_counter() - t0) * 1e3, out

    todo = [("search_rrf", lambda: ix.search_rrf(Q, lims, a.k, a.depth)), ("pool_search", lambda: ix.search(Q, a.depth))]
    for _, fn in todo:                                                # warm-up: code objects, scratch buffers
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in todo}
    walls = []
    for _ in range(a.reps):
        for name, fn in todo:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
        if not a.no_workaround:
            walls.append(wall()[0])
    for name, v in ms.items():
        res[name + "_ms"] = spread(v)
    res["fusion_stage_ms_by_difference"] = round(res["search_rrf_ms"]["median"] - res["pool_search_ms"]["median"], 3)
    ix.rrf_search_stats(reset=True)
    sc, ids, hits = ix.search_rrf(Q, lims, a.k, a.depth)
    res["stats_of_one_call"] = ix.rrf_search_stats()
    if not a.no_workaround:
        res["workaround_wall_ms"] = spread(walls)
        w_sc, w_ids, w_hits = wall()[1]
        same = ((w_ids == ids.cpu().numpy()).all(1) & (w_hits == hits.cpu().numpy()).all(1)
                & (w_sc.view(np.uint32) == sc.cpu().numpy().view(np.uint32)).all(1))
        res["groups_equal_to_the_workaround"] = int(same.sum())
        if not same.all():
            print(json.dumps(res))
            raise SystemExit(f"{int((~same).sum())} groups differ from the host workaround")
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
