"""Fused document search next to the searches a caller would otherwise combine, on one GPU, alternating in one process, for two
kinds of questions:

  paraphrase   every question is a unit base vector plus --noise * N(0, 1) per component, renormalised (the reformulations of one question)
  unrelated    every sub-query is an independent unit vector (the parts of a multi-hop question)

  (a) docs_max / docs_min   HipIndex.search_multi_groups(sub-queries, lims, k = 10, "max" / "min", evidence=True) — each next to
                            search_multi on the same sub-queries (which ranks PAGES) and next to search_groups over the sub-queries
                            one by one (a list per sub-query): both return something else, neither figure is a bar for the other
  (b) workaround            search_groups(sub-queries, 1000), the lists copied to the host and intersected per question: wall-clock
                            time, and in how many questions the lists determine the "all-of" answer

    python tools/multi_group_search_bench.py [--docs 10000 --pages 10 --questions 1000 --m 4 --dim 2304 --k 10 --reps 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/multi_group_search_bench.py --reps 3 --only unrelated:min

Rows are unit vectors (seeded), --pages adjacent rows a document.  Every timed search is one call between two device events.  Band
documents and fp32 page dots per document returned come from multi_group_search_stats; 32 questions per case are checked against
an fp64 brute force under the bar of tests/test_gpu_multi_group_search.py: the document of fp64 score s at position j has j in
[#(F > s + 6e-7), #(F >= s - 6e-7) - 1], its score lies within 1e-5 of s, the sub-query named by `which` has an fp64 E_j(D) within
6e-7 of s, and every evidence row's fp64 score lies within 6e-7 of its sub-query's E_j(D).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

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


def check(ix, Q, lims, S, m, pages, k, fuse, tag):
    """one call: counters per document returned, and the first 32 questions against the fp64 scores S [32 * m][rows]"""
    ix.multi_group_search_stats(reset=True)
    sc, rows, docs, which, evs, evr = ix.search_multi_groups(Q, lims, k, fuse, evidence=True)
    st = ix.multi_group_search_stats()
    n = S.shape[0] // m
    E = S.view(n, m, -1, pages).max(3).values                        # [n][m][docs]
    F = E.max(1).values if fuse == "max" else E.min(1).values
    nd = F.shape[1]
    s = torch.gather(F, 1, docs[:n])
    asc = F.sort(dim=1).values
    lo = nd - torch.searchsorted(asc, (s + TOL).contiguous(), right=True)
    hi = nd - torch.searchsorted(asc, (s - TOL).contiguous(), right=False) - 1
    pos = torch.arange(k, device=S.device)[None, :]
    q_ix = torch.arange(n, device=S.device)[:, None]
    named = E[q_ix, which[:n].long(), docs[:n]]
    ev_rows = evr.view(-1, k, m)[:n]                                  # [n][k][m]
    ev64 = S.view(n, m, -1)[q_ix[:, :, None], torch.arange(m, device=S.device)[None, None, :], ev_rows]
    e_of = E.permute(0, 2, 1)[q_ix, docs[:n]]                        # [n][k][m]
    ok = bool(((pos >= lo) & (pos <= hi)).all()) and bool(((sc[:n].double() - s).abs() <= 1e-5).all())
    ok = ok and bool(((named - s).abs() <= TOL).all()) and bool((docs >= 0).all()) and bool(((ev64 - e_of).abs() <= TOL).all())
    ok = ok and bool((torch.div(ev_rows, pages, rounding_mode="floor") == docs[:n, :, None]).all())
    returned = int((docs >= 0).sum())
    return {f"{tag}_band_documents_per_document_returned": round(st["documents"] / max(returned, 1), 2),
            f"{tag}_page_dots_per_document_returned": round(st["page_dots"] / max(returned, 1), 2),
            f"{tag}_band_documents_per_question": round(st["documents"] / max(st["questions"], 1), 1),
            f"{tag}_max_score_error_on_32_questions": float((sc[:n].double() - s).abs().max()),
            f"{tag}_widened_intervals_on_32_questions": int((hi > lo).sum()), f"{tag}_ok": ok}


def workaround(ix, Q, lims, k, depth, fused_docs, reps, tag):
    """search_groups(depth) per sub-query, the lists to the host, intersected per question ("all-of"): wall-clock ms, the
    questions whose answer the lists determine, agreement with the fused document search"""
    lims = np.asarray(lims)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc, _, gr = ix.search_groups(Q, depth)
        sc, gr = sc.cpu().numpy(), gr.cpu().numpy()
        determined = np.zeros(len(lims) - 1, dtype=bool)
        answer = np.full((len(lims) - 1, k), -1, dtype=np.int64)
        for g in range(len(lims) - 1):
            a, b = int(lims[g]), int(lims[g + 1])
            seen: dict = {}
            for j in range(a, b):
                for d, v in zip(gr[j].tolist(), sc[j].tolist()):
                    if d >= 0:
                        e = seen.get(d)
                        seen[d] = [v, 1] if e is None else [min(e[0], v), e[1] + 1]
            known = sorted(((v, d) for d, (v, c) in seen.items() if c == b - a), key=lambda t: (-t[0], t[1]))[:k]
            full = [j for j in range(a, b) if gr[j][-1] >= 0]          # a document missing from a full list may score up to its last entry
            bound = max((float(sc[j][-1]) for j in full), default=-np.inf)
            answer[g, :len(known)] = [d for _, d in known]
            determined[g] = not full or (len(known) == k and known[-1][0] > bound)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms)
    same = (answer == fused_docs.cpu().numpy()).all(1)
    return {f"{tag}_workaround_depth{depth}_all_of_wall_ms": {"median": round(ms[len(ms) // 2], 1), "min": round(ms[0], 1), "max": round(ms[-1], 1)},
            f"{tag}_workaround_all_of_determined_questions": int(determined.sum()),
            f"{tag}_workaround_all_of_questions_with_fewer_than_k_documents": int(((answer >= 0).sum(1) < k).sum()),
            f"{tag}_workaround_all_of_questions_that_differ_from_the_fused_document_search": int((~same).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10000)
    ap.add_argument("--pages", type=int, default=10)
    ap.add_argument("--questions", type=int, default=1000)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated cases regime:fuse (paraphrase:max ... unrelated:min); default: all, and the workaround")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_group_search_bench needs a GPU: there is no CPU fallback")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = a.docs * a.pages
    res = {"rows": rows, "docs": a.docs, "pages": a.pages, "questions": a.questions, "m": a.m, "dim": a.dim, "k": a.k, "noise": a.noise,
           "reps": a.reps}
    C = unit(rows, a.dim, g)
    n_sub = a.questions * a.m
    base = unit(a.questions, a.dim, g).repeat_interleave(a.m, dim=0)
    para = base + a.noise * torch.randn((n_sub, a.dim), generator=g, device="cuda")
    regimes = {"paraphrase": (para / para.norm(dim=1, keepdim=True)).contiguous(), "unrelated": unit(n_sub, a.dim, g)}
    lims = np.arange(a.questions + 1, dtype=np.int64) * a.m
    ix = HipIndex(a.dim, rows)
    ix.add(C)
    ix.set_groups(np.arange(a.docs + 1, dtype=np.int64) * a.pages)
    only = [c for c in a.only.split(",") if c]
    for regime, Q in regimes.items():
        fuses = [f for f in ("max", "min") if not only or f"{regime}:{f}" in only]
        if not fuses:
            continue
        todo = []
        for fuse in fuses:
            todo += [(f"{regime}_docs_{fuse}", (lambda f: (lambda: ix.search_multi_groups(Q, lims, a.k, f, evidence=True)))(fuse)),
                     (f"{regime}_search_multi_next_to_{fuse}", (lambda f: (lambda: ix.search_multi(Q, lims, a.k, f)))(fuse)),
                     (f"{regime}_search_groups_next_to_{fuse}", lambda: ix.search_groups(Q, a.k))]
        res.update(alternate(todo, a.reps))
        S = Q[:32 * a.m].double() @ C.double().T
        for fuse in fuses:
            res.update(check(ix, Q, lims, S, a.m, a.pages, a.k, fuse, f"{regime}_docs_{fuse}"))
        del S
        if not only:
            res.update(workaround(ix, Q, lims, a.k, 1000, ix.search_multi_groups(Q, lims, a.k, "min")[2], 3, regime))
    res["error_model"] = ix.error_model()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
