"""Plain-loop statement of reciprocal-rank fusion (include/visrag_hip.h: vr_rrf_fuse / vr_index_search_rrf), the oracle of
tests/test_gpu_rrf_search.py.  A group has lists of `depth` slots; slot r of list j holds an id in [0, 2^31 - 2], anything else
is an empty slot.  An id scores F = float32(sum over its entries (j, r), in ascending (j, r), of float64(float32(w_j)) /
(float64(float32(c)) + float64(r + 1))) — a float64 sum that starts at 0.0, one division per term — and hits counts the entries.
The result is ranked F descending in the library's order of floats (-0.0 < +0.0), then lower id first; tails (-inf, -1, 0).
tests/test_cpu_rrf_search_ref.py pins it on hand-worked cases.  Nothing here needs a GPU or the built library."""
import numpy as np

ID_MAX = 2 ** 31 - 2


def orderable(x):
    """search_common.h: f32_orderable of one float32 -> int"""
    u = int(np.float32(x).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u >> 31 else (u | 0x80000000)


def rrf_ref(ids, lims, k, c=60.0, weights=None):
    """-> (scores f32 [n_groups][k], ids i64 [n_groups][k], hits i32 [n_groups][k])"""
    ids = np.asarray(ids, dtype=np.int64)
    lims = [int(x) for x in np.asarray(lims).reshape(-1)]
    ng = len(lims) - 1
    c64 = np.float64(np.float32(c))
    out_s = np.full((ng, k), -np.inf, dtype=np.float32)
    out_i = np.full((ng, k), -1, dtype=np.int64)
    out_h = np.zeros((ng, k), dtype=np.int32)
    for g in range(ng):
        acc, hits = {}, {}
        for j in range(lims[g], lims[g + 1]):
            w = np.float64(np.float32(1.0 if weights is None else weights[j]))
            for r, i in enumerate(ids[j].tolist()):
                if 0 <= i <= ID_MAX:
                    acc[i] = acc.get(i, np.float64(0.0)) + w / (c64 + np.float64(r + 1))
                    hits[i] = hits.get(i, 0) + 1
        with np.errstate(over="ignore"):
            F = {i: np.float32(v) for i, v in acc.items()}
        top = sorted(F, key=lambda i: (-orderable(F[i]), i))[:k]
        for slot, i in enumerate(top):
            out_s[g, slot], out_i[g, slot], out_h[g, slot] = F[i], i, hits[i]
    return out_s, out_i, out_h


def random_lists(n_lists, depth, universe, holes, seed, distinct=True):
    """[n_lists][depth] int64 lists over ids [0, universe): without repeats inside a list when `distinct` (and the universe is
    large enough), a fraction `holes` of the slots emptied (-1)"""
    rng = np.random.default_rng(seed)
    out = np.empty((n_lists, depth), dtype=np.int64)
    for j in range(n_lists):
        if distinct and universe >= depth:
            out[j] = rng.choice(universe, depth, replace=False) if universe <= 1 << 20 else rng.integers(0, universe, depth)
        else:
            out[j] = rng.integers(0, universe, depth)
    if holes > 0:
        out[rng.random(out.shape) < holes] = -1
    return out
