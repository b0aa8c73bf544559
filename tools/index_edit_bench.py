"""Editing the index in place against the only alternative there was — emptying it and adding the surviving rows again — on one
GPU, alternating in one process:

  E    HipIndex.remove(ids) / HipIndex.update(ids, rows) on the resident index
  Rd   HipIndex.reset() + HipIndex.add(survivors) from a DEVICE tensor: needs a second copy of the corpus in HBM
  Rh   the same from HOST memory (numpy): the upload crosses PCIe

    python tools/index_edit_bench.py [--rows 100000 --dim 2304 --reps 10] [--out FILE]

Cases: remove row 0 alone (every row moves), remove one document of 10 pages in the middle, remove 1 % and 50 % of the rows at
random, update 32 rows.  Unit rows (seeded).  Every timed window is one call (or reset + add) between two device events; before
each window of E the index is restored to the full corpus, untimed.  The two sides keep different things resident — E keeps the
filters and needs no copy of the corpus anywhere — so the figures are not a race, they are the price list.
"Must move": the rows at or behind the first removed one that survive, read and written once in both stores (dim * 6 bytes each
way), plus one read of the fp32 rows that remain for the maxima of the error model; for an update the rows written and the same
read.  For the rebuild: every surviving row copied, converted and read for the maxima (dim * 18 bytes).  GB/s = must move / time.
Prints a table and one JSON line; --out writes both to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visrag_amd.engine import HipIndex  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("index_edit_bench needs a GPU: there is no CPU fallback")
    n, dim = a.rows, a.dim
    g = torch.Generator(device="cuda").manual_seed(0)
    C = torch.randn((n, dim), generator=g, device="cuda")
    C = C / C.norm(dim=1, keepdim=True)
    rng = np.random.default_rng(0)
    cases = [("remove_row_0", np.array([0])),
             ("remove_10_pages_mid", np.arange(n // 2, n // 2 + 10)),
             ("remove_1pct_random", np.sort(rng.choice(n, size=n // 100, replace=False))),
             ("remove_50pct_random", np.sort(rng.choice(n, size=n // 2, replace=False)))]
    upd_ids = np.sort(rng.choice(n, size=32, replace=False))
    upd_rows = torch.randn((32, dim), generator=g, device="cuda")
    upd_rows = upd_rows / upd_rows.norm(dim=1, keepdim=True)
    E = HipIndex(dim, n)
    R = HipIndex(dim, n)

    def restore():
        E.reset()
        E.add(C)
        torch.cuda.synchronize()

    res = {"device": torch.cuda.get_device_name(0), "rows": n, "dim": dim, "reps": a.reps, "cases": {}}
    for name, ids in cases + [("update_32_rows", upd_ids)]:
        update = name.startswith("update")
        if update:
            left_dev = C.clone()
            left_dev[torch.from_numpy(upd_ids).cuda()] = upd_rows
            edit = lambda: E.update(upd_ids, upd_rows)                       # noqa: E731
            must_edit = len(ids) * dim * (4 + 6) + n * dim * 4
        else:
            keep = np.ones(n, dtype=bool)
            keep[ids] = False
            left_dev = C[torch.from_numpy(keep).cuda()].contiguous()
            edit = lambda: E.remove(ids)                                     # noqa: E731
            new_n = int(keep.sum())
            must_edit = max(new_n - int(ids[0]), 0) * dim * 6 * 2 + new_n * dim * 4
        left_host = left_dev.cpu().numpy()
        must_rebuild = len(left_host) * dim * 18
        rebuild_dev = lambda: (R.reset(), R.add(left_dev))                   # noqa: E731
        rebuild_host = lambda: (R.reset(), R.add(left_host))                 # noqa: E731
        restore(); edit(); rebuild_dev(); rebuild_host()                     # warm-up: code objects, scratch buffers
        ms = {"edit": [], "rebuild_device": [], "rebuild_host": []}
        for _ in range(a.reps):                                              # alternate
            restore()
            ms["edit"].append(timed(edit))
            ms["rebuild_device"].append(timed(rebuild_dev))
            ms["rebuild_host"].append(timed(rebuild_host))
        assert len(E) == len(R) == len(left_host)
        probe = np.linspace(0, len(left_host) - 1, 64).astype(np.int64)
        assert np.array_equal(E.rows(probe).view(np.uint32), left_host[probe].view(np.uint32))
        assert E.error_model() == R.error_model()
        out = {"rows_named": int(len(ids)), "rows_left": int(len(left_host))}
        for k, v in ms.items():
            v = sorted(v)
            must = must_edit if k == "edit" else must_rebuild
            out[k] = {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3),
                      "must_move_MB": round(must / 1e6, 1), "GB_per_s": round(must / 1e6 / v[len(v) // 2], 1)}
        res["cases"][name] = out
        del left_dev, left_host
    lines = [f"{res['device']}: {n} x {dim}, {a.reps} alternations, median ms (min-max) | must move MB | GB/s",
             f"{'case':24s} {'edit in place':>40s} {'reset + add, device rows':>40s} {'reset + add, host rows':>40s}"]
    for name, o in res["cases"].items():
        cell = lambda d: f"{d['median_ms']:9.3f} ({d['min_ms']:.3f}-{d['max_ms']:.3f}) | {d['must_move_MB']:7.1f} | {d['GB_per_s']:7.1f}"  # noqa: E731
        lines.append(f"{name:24s} {cell(o['edit']):>40s} {cell(o['rebuild_device']):>40s} {cell(o['rebuild_host']):>40s}")
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
