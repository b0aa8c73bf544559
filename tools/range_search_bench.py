"""Range search next to the top-k search of the same depth, on one GPU, alternating in one process:

  R(c)  HipIndex.search_range(Q, t_c, sort=False): the threshold t_c chosen by quantile on a 32-query fp64 sample so that a query
        returns about c rows, c = 10, 100, 1000;  Rs(c): the same with sort=True (segments in ranking order, sorted on the device)
  K(c)  HipIndex.search(Q, c): the partner — it returns exactly c rows per query whatever they score, so the two figures answer
        different questions and neither is a bar for the other
  T     the templated corpus (100 families x 1 000 near-duplicate rows, laid out contiguously; queries near a family's centre) with
        a threshold between family and rest, next to search(k = 1000)

    python tools/range_search_bench.py [--rows 100000 --nq 1000 --dim 2304 --reps 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/range_search_bench.py --reps 3      # kernel split

Unit rows and queries (seeded).  Every timed window is one call between two device events.  Candidates re-scored per row returned
come from range_search_stats; the membership of 32 queries per configuration is checked against an fp64 brute force (a pair
within 3e-7 of the threshold may differ: fp32 summation order).  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visrag_amd.engine import HipIndex  # noqa: E402

COUNTS = (10, 100, 1000)


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


def measure(ix, Q, C, t, tag):
    """one threshold: what a call returns, candidates per row returned, membership of 32 queries against fp64"""
    ix.range_search_stats(reset=True)
    lims, _, ids = ix.search_range(Q, t, sort=False)
    st = ix.range_search_stats()
    per = (lims[1:] - lims[:-1]).double()
    n = min(32, len(Q))
    t32 = float(torch.tensor(t, dtype=torch.float32))
    S = Q[:n].double() @ C.double().T
    want = S >= t32
    have = torch.zeros_like(want)
    seg = torch.repeat_interleave(torch.arange(n, device=Q.device), lims[1:n + 1] - lims[:n])
    have[seg, ids[:int(lims[n])]] = True
    diff = have != want
    near = bool(((S[diff] - t32).abs() < 3e-7).all())
    return {f"{tag}_threshold": round(float(t), 6), f"{tag}_rows_per_query": {"mean": round(float(per.mean()), 1), "min": int(per.min()),
                                                                             "max": int(per.max())},
            f"{tag}_candidates_per_row_returned": round(st["candidates"] / max(st["returned"], 1), 3),
            f"{tag}_membership_differs_from_fp64_on_32_queries": int(diff.sum()), f"{tag}_ok": near}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("range_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"rows": a.rows, "nq": a.nq, "dim": a.dim, "reps": a.reps}
    # ---- unit rows: thresholds by quantile
    C, Q = unit(a.rows, a.dim, g), unit(a.nq, a.dim, g)
    sample = (Q[:32].double() @ C.double().T).flatten().sort(descending=True).values
    thr = {c: float(sample[32 * c - 1].float()) for c in COUNTS if c < a.rows}
    ix = HipIndex(a.dim, a.rows)
    ix.add(C)
    todo = []
    for c, t in thr.items():
        todo.append((f"range_{c}", (lambda t: (lambda: ix.search_range(Q, t, sort=False)))(t)))
        todo.append((f"range_{c}_sorted", (lambda t: (lambda: ix.search_range(Q, t)))(t)))
        todo.append((f"search_k{c}", (lambda c: (lambda: ix.search(Q, c)))(c)))
    res.update(alternate(todo, a.reps))
    for c, t in thr.items():
        res.update(measure(ix, Q, C, t, f"range_{c}"))
    ix.close()
    del C, ix
    # ---- the templated corpus: 100 families x 1 000 near-duplicates (tools/search_templated.py's rows), queries near a centre
    n_fam, per = 100, 1000
    centers = unit(n_fam, a.dim, g)
    spread = torch.logspace(-0.7545, -1.5, n_fam, device="cuda")     # pairwise cosine 0.97 .. 0.999 inside a family
    rows = torch.empty((n_fam * per, a.dim), device="cuda")
    for f in range(n_fam):
        r = centers[f][None, :] + spread[f] * torch.randn((per, a.dim), generator=g, device="cuda") / a.dim ** 0.5
        rows[f * per:(f + 1) * per] = r / r.norm(dim=1, keepdim=True)
    fam_q = torch.randint(0, n_fam, (a.nq,), generator=g, device="cuda")
    Qt = centers[fam_q] + 0.5 * torch.randn((a.nq, a.dim), generator=g, device="cuda") / a.dim ** 0.5
    Qt = Qt / Qt.norm(dim=1, keepdim=True)                             # ~0.88 with its family's rows, ~N(0, 0.02) with the rest
    ix = HipIndex(a.dim, n_fam * per)
    ix.add(rows)
    t = 0.5
    res.update(alternate([("templated_range", lambda: ix.search_range(Qt, t, sort=False)),
                          ("templated_range_sorted", lambda: ix.search_range(Qt, t)),
                          ("templated_search_k1000", lambda: ix.search(Qt, 1000))], a.reps))
    res.update(measure(ix, Qt, rows, t, "templated_range"))
    res["range_search_stats_templated_one_call"] = ix.range_search_stats()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
