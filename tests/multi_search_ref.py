"""Plain numpy statement of the fused search (include/visrag_hip.h: vr_index_search_multi), the reference of
tests/test_gpu_multi_search.py.  Scores are fp64 dot products of the fp32 data (group_search_ref.scores64).  Group g holds
sub-queries lims[g] .. lims[g + 1] - 1; the fused score of row i is the max ("any-of") or the min ("all-of") of its scores over
them; the result is the k rows of largest fused score — score descending, then lower id first — among the rows of the group's
mask, slots past them (-inf, -1); `which` is the lowest in-group sub-query whose score is the fused score.

The library ranks by its fp32 scores, the reference by fp64: a row of fp64 fused score s that the library returns at position j
must have j in `rank_search_ref.interval(F, s)` = [#(F > s + TOL), #(F >= s - TOL) - 1] with TOL = 6e-7 — the rank search's
interval bar, on the same grounds: a fused fp32 score is ONE fp32 dot product (the deciding sub-query's), so it lies inside the
project's NEAR_TIE = 3e-7 of its fp64 value, and two such scores are compared.  For the same reason the sub-query the library
names must have an fp64 score within TOL of the fp64 fused score.  tests/test_cpu_multi_search_ref.py pins how wide these
intervals are on the corpora the GPU test uses.  Nothing here needs a GPU or the built library."""
import numpy as np

from tests.rank_search_ref import TOL, case, interval, ranking  # noqa: F401  (the corpora, the order and the bar are the rank search's)


def layout(n_sub, cycle):
    """lims int64 of groups whose sizes cycle through `cycle` until the n_sub sub-queries are used up (the last group takes what
    is left)"""
    lims, j = [0], 0
    while lims[-1] < n_sub:
        lims.append(min(n_sub, lims[-1] + int(cycle[j % len(cycle)])))
        j += 1
    return np.asarray(lims, dtype=np.int64)


def fuse_ref(S, lims, fuse):
    """S [n_sub][rows] -> F [n_groups][rows]: the max / min over every group's sub-queries"""
    S = np.asarray(S)
    op = {"max": np.max, "min": np.min}[fuse]
    return np.stack([op(S[lims[g]:lims[g + 1]], axis=0) for g in range(len(lims) - 1)])


def which_ref(S, lims, g, ids, fuse):
    """the lowest in-group sub-query whose score of row ids[j] is group g's fused score of it; -1 for a tail"""
    sub = np.asarray(S)[lims[g]:lims[g + 1]]
    pick = np.argmax if fuse == "max" else np.argmin           # (both return the first of equals)
    ids = np.asarray(ids, dtype=np.int64)
    return np.where(ids >= 0, pick(sub[:, np.maximum(ids, 0)], axis=0), -1).astype(np.int32)


def multi_ref(S, lims, k, fuse, mask=None):
    """-> (scores f64 [n_groups][k], ids i64 [n_groups][k], which i32 [n_groups][k]); `mask`: None, or per group a bool row
    mask or None"""
    F = fuse_ref(S, lims, fuse)
    ng = len(F)
    sc, ids = np.full((ng, k), -np.inf, dtype=np.float64), np.full((ng, k), -1, dtype=np.int64)
    which = np.full((ng, k), -1, dtype=np.int32)
    for g in range(ng):
        order = ranking(F[g])
        m = None if mask is None else mask[g]
        if m is not None:
            order = order[np.asarray(m, dtype=bool)[order]]
        part = order[:k]
        ids[g, :len(part)], sc[g, :len(part)] = part, F[g][part]
        which[g] = which_ref(S, lims, g, ids[g], fuse)
    return sc, ids, which


def runner_up_gap(S, lims, g, ids, fuse):
    """for rows ids of group g: how far the second-closest sub-query's score lies from the fused score (inf for a group of one)"""
    sub = np.asarray(S)[lims[g]:lims[g + 1]][:, ids]
    if len(sub) < 2:
        return np.full(len(ids), np.inf)
    srt = np.sort(sub, axis=0)
    return srt[-1] - srt[-2] if fuse == "max" else srt[1] - srt[0]


def interval_table(S, lims, k, fuse, tol=TOL):
    """-> (positions, widened intervals, max width, smallest runner-up gap) over the reference's own top-k of every group;
    width = hi - lo, and the reference's own position always lies inside"""
    _, ids, _ = multi_ref(S, lims, k, fuse)
    F = fuse_ref(S, lims, fuse)
    positions = widened = widest = 0
    gap = np.inf
    for g in range(len(F)):
        live = ids[g][ids[g] >= 0]
        for j, i in enumerate(live):
            lo, hi = interval(F[g], F[g, i], tol)
            assert lo <= j <= hi
            positions += 1; widened += int(hi > lo); widest = max(widest, hi - lo)
        gap = min(gap, float(runner_up_gap(S, lims, g, live, fuse).min()))
    return positions, widened, widest, gap


def check_group(S, lims, g, fuse, ids, which, tol=TOL):
    """the bar of the fp64 test for one group: ids / which [k] as the library returned them -> (entries, positions that differ
    from the reference's ranking, first violation or None)"""
    F = fuse_ref(S, lims, fuse)[g]
    ids, which = np.asarray(ids, dtype=np.int64), np.asarray(which, dtype=np.int64)
    live = ids >= 0
    assert live.sum() == min(len(ids), len(F)) and live[:live.sum()].all(), "the result's length is exact"
    assert (which[~live] == -1).all()
    got, w = ids[live], which[live]
    assert len(set(got.tolist())) == len(got), "a row is returned once"
    want = ranking(F)[:len(got)]
    bad = None
    for j, i in enumerate(got):
        lo, hi = interval(F, F[i], tol)
        named = S[lims[g] + w[j], i] if 0 <= w[j] < lims[g + 1] - lims[g] else np.inf
        if not (lo <= j <= hi) or abs(named - F[i]) > tol:
            bad = (j, int(i), lo, hi, int(w[j]), float(named - F[i]))
            break
    return len(got), int((got != want).sum()), bad


K_FP64 = 100
# the layouts of the fp64 test (k = 100) and what the reference alone says about them at TOL = 6e-7:
#   name -> (size cycle, groups, {fuse: (positions, widened intervals, max width)})
TABLE = {
    "unit-5000x37x256": ((1, 2, 3, 4, 5, 6, 7, 9), 8, {"max": (800, 2, 1), "min": (800, 1, 1)}),
    "unit-3001x300x128": ((1, 3, 8, 2, 64, 5), 23, {"max": (2300, 2, 1), "min": (2300, 4, 1)}),
    "unit-20000x64x2304": ((4, 1, 7, 2, 16, 3), 12, {"max": (1200, 18, 1), "min": (1200, 14, 1)}),
    "families-2304": ((2, 3), 4, {"max": (400, 60, 2), "min": (400, 33, 2)}),
    "norms-4000x20x256": ((1, 4, 2, 5), 8, {"max": (800, 0, 0), "min": (800, 0, 0)}),
}
