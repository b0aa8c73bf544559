"""Fused search next to the plain top-k search of the same sub-queries and next to the host workaround, on one GPU, alternating in
one process, for two kinds of groups:

  paraphrase   every group is a unit base vector plus --noise * N(0, 1) per component, renormalised (the reformulations of one question)
  unrelated    every sub-query is an independent unit vector (the parts of a multi-hop question)

  (a) multi_max / multi_min   HipIndex.search_multi(sub-queries, lims, k = 10, "max" / "min") — each next to search(sub-queries, 10),
                              which shares the GEMM but returns a list per sub-query: neither figure is a bar for the other
  (b) workaround              search(sub-queries, 100), the lists copied to the host, documents.fuse_runs: wall-clock time, and in
                              how many groups the lists do not determine its "all-of" answer

    python tools/multi_search_bench.py [--rows 100000 --groups 1000 --m 4 --dim 2304 --k 10 --reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/multi_search_bench.py --reps 3 --only unrelated:min   # one case

Rows are unit vectors (seeded).  Every timed fused search is one call between two device events.  Band columns re-scored and fp32
row dots per row returned come from multi_search_stats; 32 groups per case are checked against an fp64 brute force under the bar of
tests/test_gpu_multi_search.py: the row of fp64 fused score s at position j has j in [#(F > s + 6e-7), #(F >= s - 6e-7) - 1], its
score lies within 1e-5 of s, and the sub-query named by `which` has an fp64 score within 6e-7 of s.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visrag_amd.documents import fuse_runs  # noqa: E402
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


def check(ix, Q, lims, S, m, k, fuse, tag):
    """one call: counters per row returned, and the first 32 groups against the fp64 scores S [32 * m][rows]"""
    ix.multi_search_stats(reset=True)
    sc, ids, which = ix.search_multi(Q, lims, k, fuse)
    st = ix.multi_search_stats()
    n = S.shape[0] // m
    F = S.view(n, m, -1).max(1).values if fuse == "max" else S.view(n, m, -1).min(1).values
    rows = F.shape[1]
    s = torch.gather(F, 1, ids[:n])
    asc = F.sort(dim=1).values
    lo = rows - torch.searchsorted(asc, (s + TOL).contiguous(), right=True)
    hi = rows - torch.searchsorted(asc, (s - TOL).contiguous(), right=False) - 1
    pos = torch.arange(k, device=S.device)[None, :]
    named = S.view(n, m, -1)[torch.arange(n, device=S.device)[:, None], which[:n].long(), ids[:n]]
    ok = bool(((pos >= lo) & (pos <= hi)).all()) and bool(((sc[:n].double() - s).abs() <= 1e-5).all())
    ok = ok and bool(((named - s).abs() <= TOL).all()) and bool((ids >= 0).all())
    returned = int((ids >= 0).sum())
    return {f"{tag}_band_columns_per_row_returned": round(st["candidates"] / max(returned, 1), 1),
            f"{tag}_row_dots_per_row_returned": round(st["dots"] / max(returned, 1), 1),
            f"{tag}_band_columns_per_group": round(st["candidates"] / max(st["groups"], 1), 1),
            f"{tag}_widened_intervals_on_32_groups": int((hi > lo).sum()), f"{tag}_ok": ok}


def workaround(ix, Q, lims, k, depth, fused, reps, tag):
    """search(depth) per sub-query + documents.fuse_runs on the host: wall-clock ms, undetermined groups, agreement with the fused search"""
    lims = np.asarray(lims)
    ms, out = [], {}
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc, ids = ix.search(Q, depth)
        sc, ids = sc.cpu().numpy(), ids.cpu().numpy()
        res = {fuse: fuse_runs(sc, ids, lims, k, fuse) for fuse in ("max", "min")}
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms)
    out[f"{tag}_workaround_depth{depth}_both_fusions_wall_ms"] = {"median": round(ms[len(ms) // 2], 1), "min": round(ms[0], 1), "max": round(ms[-1], 1)}
    for fuse in ("max", "min"):
        _, w_ids, det = res[fuse]
        same = (w_ids == fused[fuse][1].cpu().numpy()).all(1)
        out[f"{tag}_workaround_{fuse}_undetermined_groups"] = int((~det).sum())
        out[f"{tag}_workaround_{fuse}_groups_with_fewer_than_k_rows"] = int(((w_ids >= 0).sum(1) < k).sum())
        out[f"{tag}_workaround_{fuse}_groups_that_differ_from_the_fused_search"] = int((~same).sum())
        out[f"{tag}_workaround_{fuse}_determined_groups_that_differ"] = int((~same & det).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated cases regime:fuse (paraphrase:max ... unrelated:min); default: all, and the workaround")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"rows": a.rows, "groups": a.groups, "m": a.m, "dim": a.dim, "k": a.k, "noise": a.noise, "reps": a.reps}
    C = unit(a.rows, a.dim, g)
    n_sub = a.groups * a.m
    base = unit(a.groups, a.dim, g).repeat_interleave(a.m, dim=0)
    para = base + a.noise * torch.randn((n_sub, a.dim), generator=g, device="cuda")
    regimes = {"paraphrase": (para / para.norm(dim=1, keepdim=True)).contiguous(), "unrelated": unit(n_sub, a.dim, g)}
    lims = np.arange(a.groups + 1, dtype=np.int64) * a.m
    ix = HipIndex(a.dim, a.rows)
    ix.add(C)
    only = [c for c in a.only.split(",") if c]
    for regime, Q in regimes.items():
        cube = Q.view(a.groups, a.m, a.dim)
        res[f"{regime}_mean_cosine_inside_a_group"] = round(float(((cube @ cube.transpose(1, 2)).sum((1, 2)) - a.m).mean() / (a.m * (a.m - 1))), 3)
        fuses = [f for f in ("max", "min") if not only or f"{regime}:{f}" in only]
        if not fuses:
            continue
        todo = []
        for fuse in fuses:
            todo += [(f"{regime}_multi_{fuse}", (lambda f: (lambda: ix.search_multi(Q, lims, a.k, f)))(fuse)),
                     (f"{regime}_search_next_to_{fuse}", lambda: ix.search(Q, a.k))]
        res.update(alternate(todo, a.reps))
        S = Q[:32 * a.m].double() @ C.double().T
        for fuse in fuses:
            res.update(check(ix, Q, lims, S, a.m, a.k, fuse, f"{regime}_multi_{fuse}"))
        del S
        if not only:
            fused = {fuse: ix.search_multi(Q, lims, a.k, fuse) for fuse in ("max", "min")}
            res.update(workaround(ix, Q, lims, a.k, 100, fused, 3, regime))
    res["error_model"] = ix.error_model()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
