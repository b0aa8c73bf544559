"""Filtered search against the unfiltered deep path, on one GPU, alternating in one process:

  F(d)  HipIndex.search_filtered(Q, k, 0) under a filter of density d shared by all queries, d = 1.0, 0.5, 0.01
  B     HipIndex.search(Q, 27): the deep path without a filter — the same GEMM and the same select, so F - B is the mask pass
        and the narrower (or equal) candidate work

    python tools/filter_search_bench.py [--rows 100000 --nq 1000 --dim 2304 --k 10 --reps 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/filter_search_bench.py --reps 3      # kernel split

Unit rows and queries (seeded).  Every timed window is one call between two device events.  The ids of 32 queries per density
are checked against an fp64 brute force.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visrag_amd.engine import HipIndex  # noqa: E402

DENSITIES = (1.0, 0.5, 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    C = torch.randn((a.rows, a.dim), generator=g, device="cuda")
    C = C / C.norm(dim=1, keepdim=True)
    Q = torch.randn((a.nq, a.dim), generator=g, device="cuda")
    Q = Q / Q.norm(dim=1, keepdim=True)
    M = torch.stack([torch.rand(a.rows, generator=g, device="cuda") < d for d in DENSITIES])
    ix = HipIndex(a.dim, a.rows)
    ix.add(C)
    ix.set_filters(M)
    todo = [(f"filtered_density_{d}", (lambda f: (lambda: ix.search_filtered(Q, a.k, f)))(f)) for f, d in enumerate(DENSITIES)]
    todo.append(("search_k27", lambda: ix.search(Q, 27)))
    for _, fn in todo:                                                # warm-up: code objects, scratch buffers
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in todo}
    for _ in range(a.reps):                                           # alternate
        for name, fn in todo:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    res = {"rows": a.rows, "nq": a.nq, "dim": a.dim, "k": a.k, "reps": a.reps, "allowed_rows": [int(m.sum()) for m in M]}
    for name, v in ms.items():
        v = sorted(v)
        res[name + "_ms"] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
    S = Q[:32].double() @ C.double().T
    for f, d in enumerate(DENSITIES):
        ref = torch.where(M[f][None, :], S, torch.full_like(S, float("-inf"))).topk(a.k, dim=1).indices
        res[f"ids_match_fp64_on_32_queries_density_{d}"] = bool(torch.equal(ref, ix.search_filtered(Q[:32], a.k, f)[1]))
    res["filter_search_stats"] = ix.filter_search_stats()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
