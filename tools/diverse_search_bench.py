"""Diversified search against the pool search it starts from, on one GPU, alternating in one process:

  D  HipIndex.search_diverse(Q, k, pool, lambda_): the pool search, then the MMR selection over the pool
  B  HipIndex.search(Q, pool): the existing deep path — the very call that produces D's pool, so D - B is the MMR stage

    python tools/diverse_search_bench.py [--rows 100000 --nq 1000 --dim 2304 --k 10 --pool 100 --lam 0.5 --reps 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/diverse_search_bench.py --reps 3      # kernel split

Two corpora (seeded): i.i.d. unit rows, and decks of 10 near-identical pages (a document's unit vector + 3e-4 N(0, 1) per
page, renormalised: tests/group_search_ref.py::decks, made on the device).  Every timed window is one call between two device
events.  On 32 queries per corpus the picks are re-walked in fp64 on the device: every pick's objective within 1e-6 of the best
unselected pool member's, given the picks before it.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visrag_amd.engine import HipIndex  # noqa: E402


def worst_deficit(Q, C, ids, pool_ids, lam):
    """fp64 on the device: the largest (best unselected pool member's v) - (the returned row's v) over queries and picks t >= 1"""
    worst = 0.0
    for q in range(len(Q)):
        D = C[pool_ids[q]].double()
        r = D @ Q[q].double()
        pos = {int(i): c for c, i in enumerate(pool_ids[q].tolist())}
        m = torch.full_like(r, float("-inf"))
        free = torch.ones_like(r, dtype=torch.bool)
        for t, row in enumerate(ids[q].tolist()):
            c = pos[row]                                               # (a pick outside the pool search's result raises)
            if t > 0:
                v = torch.where(free, lam * r - (1.0 - lam) * m, torch.full_like(r, float("-inf")))
                worst = max(worst, float(v.max() - v[c]))
            free[c] = False
            m = torch.maximum(m, D @ D[c])
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diverse_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    Q = torch.randn((a.nq, a.dim), generator=g, device="cuda")
    Q = Q / Q.norm(dim=1, keepdim=True)
    res = {"rows": a.rows, "nq": a.nq, "dim": a.dim, "k": a.k, "pool": a.pool, "lambda": a.lam, "reps": a.reps}
    for corpus in ("iid", "decks"):
        if corpus == "iid":
            C = torch.randn((a.rows, a.dim), generator=g, device="cuda")
        else:
            base = torch.randn((a.rows // 10, a.dim), generator=g, device="cuda")
            base = base / base.norm(dim=1, keepdim=True)
            C = base.repeat_interleave(10, dim=0) + 3e-4 * torch.randn((a.rows // 10 * 10, a.dim), generator=g, device="cuda")
            del base
        C = C / C.norm(dim=1, keepdim=True)
        ix = HipIndex(a.dim, len(C))
        ix.add(C)
        todo = [("diverse", lambda: ix.search_diverse(Q, a.k, a.pool, a.lam)), (f"search_k{a.pool}", lambda: ix.search(Q, a.pool))]
        for _, fn in todo:                                            # warm-up: code objects, scratch buffers
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in todo}
        for _ in range(a.reps):                                       # alternate
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
        out["mmr_stage_ms_median_difference"] = round(out["diverse_ms"]["median"] - out[f"search_k{a.pool}_ms"]["median"], 3)
        ids = ix.search_diverse(Q[:32], a.k, a.pool, a.lam)[1]
        pool_ids = ix.search(Q[:32], a.pool)[1]
        out["worst_fp64_deficit_on_32_queries"] = worst_deficit(Q[:32], C, ids, pool_ids, a.lam)
        out["picks_eps_optimal_1e-6_on_32_queries"] = bool(out["worst_fp64_deficit_on_32_queries"] <= 1e-6)
        if corpus == "decks":
            docs = lambda x: sorted({len(set(r)) for r in (x // 10).tolist()})                       # noqa: E731
            out["documents_per_query_diverse"] = docs(ix.search_diverse(Q, a.k, a.pool, a.lam)[1])
            out["documents_per_query_search"] = docs(ix.search(Q, a.k)[1])
        res[corpus] = out
        ix.close()
        del C
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
