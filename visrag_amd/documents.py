"""Documents over pages: the host side of the document-level search (HipIndex.set_groups / search_groups).

The index ranks rows (pages); a corpus is usually documents embedded page after page.  `search_groups` wants every document
to be ONE run of adjacent rows.  `group_rows` turns per-row labels into that layout, `doc_of_page` is the label rule of the demo's
knowledge base (`<pdf>_<idx>.png`).

The filtered search (HipIndex.set_filters / search_filtered) ranks inside a subset of the rows: `pack_filters` is the bit layout
the library takes, `group_filter` allows the rows of some groups, `label_filters` the rows whose label is in a wanted set.

The range search (HipIndex.search_range) returns a CSR result (lims, scores, ids): `split_ranges` cuts it into per-query pairs,
`duplicate_groups` reads it — the index's own rows as queries — as a graph and returns its components.

Editing in place (HipIndex.remove / update): `rows_of_documents` names the rows of documents to withdraw, `new_id_of_old` is the
map a removal applies to the row ids, `remap_rows` carries ids a caller holds across it, and `compact_filters` states what the
library does to the filters it keeps.

The rank search (HipIndex.rank_rows) returns the rank of every qrel positive, in CSR form (query q's positives are entries
lims[q] .. lims[q + 1] - 1): `reciprocal_ranks` / `mrr_from_ranks` and `recall_at` turn them into the metrics a run of fixed
depth cannot give — MRR without a cut-off, recall at any k.

The windowed search (HipIndex.search_window) returns the rows at ranks [offset, offset + k): `window_negatives` takes such a
window and a query's positives and leaves the hard negatives a trainer wants ("ranks 30-200 minus the positives").

The document window search (HipIndex.search_groups_window) ranks documents under a row filter: `collection_filters` builds such
filters from a label per DOCUMENT ("the ten best documents of this collection").

The document rank search (HipIndex.rank_groups) returns the rank of named documents, -1 for one the filter leaves no page of:
`never_retrieved` turns that into a rank the three metrics above count as a miss.

The document range search (HipIndex.search_groups_range) returns every document at or above a threshold as a CSR result (lims,
scores, best rows, groups): `split_document_ranges` cuts it into per-query triples.

The fused search (HipIndex.search_multi) ranks rows by the max or the min of their scores over a group of sub-queries:
`group_rows` of the sub-queries' labels gives its `lims`, and `fuse_runs` states what per-sub-query top-k lists can and cannot
say about that ranking — the workaround the fused search replaces.

The rank-fusion search (HipIndex.search_rrf, engine.rrf_fuse) fuses the POSITIONS of the sub-queries' lists by reciprocal-rank
fusion: `rrf_runs` is its definition in numpy, bit for bit, and the host workaround it replaces.
Pure numpy: nothing here touches the GPU.
"""
from __future__ import annotations

from typing import Hashable, Iterable, List, Optional, Sequence, Tuple

import numpy as np


def group_rows(labels: Sequence[Hashable]) -> Tuple[np.ndarray, np.ndarray, List[Hashable]]:
    """-> (order, offsets, names).

    `order` (int64 [n]) is a stable permutation of the rows that makes equal labels adjacent: row `order[j]` of the input is row
    j of the grouped layout; groups come in the order their label first appears and rows keep their order inside a group, so
    labels that are contiguous already give the identity.  `offsets` (int64 [n_groups + 1]) are the groups' first rows in the
    grouped layout — what `HipIndex.set_groups` takes — and `names[g]` is the label of group g.  A row id `i` returned by a
    search over the grouped layout is row `order[i]` of the input.

    The same call groups SUB-QUERIES for `HipIndex.search_multi`: with `labels[s]` the question sub-query s belongs to,
    `queries[order]` is the flat layout it takes, `offsets` its `lims` and `names[g]` the question of group g; `which` of a
    result counts inside the group, so the deciding sub-query of the input is `order[offsets[g] + which]`."""
    first: dict = {}
    gid = np.empty(len(labels), dtype=np.int64)
    names: List[Hashable] = []
    for i, lab in enumerate(labels):
        g = first.get(lab)
        if g is None:
            g = first[lab] = len(names)
            names.append(lab)
        gid[i] = g
    order = np.argsort(gid, kind="stable").astype(np.int64)
    counts = np.bincount(gid, minlength=len(names)).astype(np.int64)
    offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts)]).astype(np.int64)
    return order, offsets, names


def doc_of_page(name: str) -> str:
    """The document of a page file name of the demo's knowledge base: `<pdf>_<idx>.png` -> `<pdf>`.  The split is on the LAST
    underscore (`my_report.pdf_12.png` -> `my_report.pdf`); a name without an underscore is its own document."""
    head, sep, _ = name.rpartition("_")
    return head if sep else name


def pack_filters(masks) -> np.ndarray:
    """bool [n_filters][rows] (or [rows]: one filter) -> uint32 [n_filters][ceil(rows / 32)]: row r is bit r & 31 of word r >> 5,
    the spare bits of the last word are 0 — what `HipIndex.set_filters` hands to the library."""
    m = np.atleast_2d(np.asarray(masks, dtype=bool))
    nf, n = m.shape
    words = (n + 31) // 32
    padded = np.zeros((nf, words * 32), dtype=bool)
    padded[:, :n] = m
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32).reshape(nf, words)


def group_filter(offsets, groups: Iterable[int]) -> np.ndarray:
    """bool [rows]: exactly the rows of the listed groups of `offsets` (group g = rows offsets[g] .. offsets[g + 1] - 1)."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    out = np.zeros(int(off[-1]), dtype=bool)
    for g in groups:
        g = int(g)
        if not 0 <= g < len(off) - 1:
            raise ValueError(f"group {g} outside [0, {len(off) - 1})")
        out[off[g]:off[g + 1]] = True
    return out


def label_filters(labels: Sequence[Hashable], wanted_sets: Sequence[Optional[Iterable[Hashable]]]) -> np.ndarray:
    """bool [len(wanted_sets)][rows]: filter j allows the rows whose label is in wanted_sets[j] (None: every row).  A wanted
    label that no row carries allows nothing."""
    out = np.zeros((len(wanted_sets), len(labels)), dtype=bool)
    for j, wanted in enumerate(wanted_sets):
        if wanted is None:
            out[j] = True
            continue
        w = set(wanted)
        out[j] = [lab in w for lab in labels]
    return out


def collection_filters(offsets, collection_of_group: Sequence[Hashable],
                       wanted_sets: Sequence[Optional[Iterable[Hashable]]]) -> np.ndarray:
    """bool [len(wanted_sets)][rows]: filter j allows every row of the groups of `offsets` whose label `collection_of_group[g]` is in
    wanted_sets[j] (None: every row) — `label_filters` with a label per document, not per row; what `HipIndex.set_filters` takes
    for `search_groups_window`.  A wanted label that no group carries allows nothing."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if len(collection_of_group) != len(off) - 1:
        raise ValueError(f"{len(collection_of_group)} labels for {len(off) - 1} groups")
    out = np.zeros((len(wanted_sets), int(off[-1])), dtype=bool)
    for j, wanted in enumerate(wanted_sets):
        if wanted is None:
            out[j] = True
            continue
        w = set(wanted)
        out[j] = group_filter(off, [g for g, lab in enumerate(collection_of_group) if lab in w])
    return out


def split_ranges(lims, scores, ids) -> List[Tuple[np.ndarray, np.ndarray]]:
    """A range result (HipIndex.search_range) -> [(scores, ids)] per query: views of entries lims[q] .. lims[q + 1] - 1."""
    lims = np.asarray(lims, dtype=np.int64).reshape(-1)
    scores, ids = np.asarray(scores), np.asarray(ids)
    if len(lims) < 1 or lims[0] != 0 or (np.diff(lims) < 0).any() or lims[-1] != len(ids) or len(scores) != len(ids):
        raise ValueError("lims must start at 0, be non-decreasing and end at the number of entries")
    return [(scores[lims[q]:lims[q + 1]], ids[lims[q]:lims[q + 1]]) for q in range(len(lims) - 1)]


def split_document_ranges(lims, scores, rows, groups) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """A document range result (HipIndex.search_groups_range) -> [(scores, best rows, groups)] per query: views of entries
    lims[q] .. lims[q + 1] - 1."""
    lims = np.asarray(lims, dtype=np.int64).reshape(-1)
    scores, rows, groups = np.asarray(scores), np.asarray(rows), np.asarray(groups)
    if len(lims) < 1 or lims[0] != 0 or (np.diff(lims) < 0).any() or lims[-1] != len(groups) or len(scores) != len(groups) or len(rows) != len(groups):
        raise ValueError("lims must start at 0, be non-decreasing and end at the number of entries")
    return [(scores[lims[q]:lims[q + 1]], rows[lims[q]:lims[q + 1]], groups[lims[q]:lims[q + 1]]) for q in range(len(lims) - 1)]


def duplicate_groups(lims, ids, n_rows: int) -> List[List[int]]:
    """The connected components with more than one row of the graph "row q - row ids[j]" for every entry j of query q's segment
    (lims[q] <= j < lims[q + 1]): the rows of an index chained by a score at or above the threshold of a range search whose
    queries were the index's own rows 0, 1, ...  A row's match with itself joins nothing.  -> sorted lists of rows, ordered by
    their first row.  Union-find over n_rows rows, pure host code."""
    lims = np.asarray(lims, dtype=np.int64).reshape(-1)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    parent = np.arange(int(n_rows), dtype=np.int64)

    def find(x: int) -> int:
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:                       # path compression
            parent[x], x = root, parent[x]
        return int(root)

    for q in range(len(lims) - 1):
        row = q
        if row >= n_rows:
            raise ValueError(f"query {q} is no row of [0, {n_rows})")
        for j in ids[lims[q]:lims[q + 1]]:
            j = int(j)
            if not 0 <= j < n_rows:
                raise ValueError(f"row id {j} outside [0, {n_rows})")
            a, b = find(row), find(j)
            if a != b:                                 # the smaller row is the root: a component is named by its first row
                parent[max(a, b)] = min(a, b)
    members: dict = {}
    for r in range(int(n_rows)):
        members.setdefault(find(r), []).append(r)
    return [m for _, m in sorted(members.items()) if len(m) > 1]


def rows_of_documents(names: Sequence[str], documents: Iterable[str]) -> np.ndarray:
    """int64, ascending: the rows (pages `names[i]` of the demo's knowledge base) whose `doc_of_page` is one of `documents` — what
    `HipIndex.remove` takes to withdraw those documents.  A document that no page belongs to names no row."""
    wanted = set(documents)
    return np.asarray([i for i, nm in enumerate(names) if doc_of_page(nm) in wanted], dtype=np.int64)


def new_id_of_old(n_rows: int, removed) -> np.ndarray:
    """int64 [n_rows]: where every row of an index of `n_rows` rows is after `HipIndex.remove(removed)` — the survivors keep their
    order and close up (new id = old id - removed ids below it), a removed row maps to -1.  `removed`: any order, duplicates count
    once; an id outside [0, n_rows) raises ValueError."""
    rem = np.asarray(removed, dtype=np.int64).reshape(-1)
    if len(rem) and (rem.min() < 0 or rem.max() >= n_rows):
        raise ValueError(f"row ids must lie in [0, {n_rows})")
    keep = np.ones(int(n_rows), dtype=bool)
    keep[rem] = False
    out = np.cumsum(keep, dtype=np.int64) - 1
    out[~keep] = -1
    return out


def remap_rows(new_id_of_old, ids) -> np.ndarray:
    """Row ids a caller holds from before a removal -> their ids after it, in the same order; ids of removed rows are dropped."""
    m = np.asarray(new_id_of_old, dtype=np.int64)[np.asarray(ids, dtype=np.int64).reshape(-1)]
    return m[m >= 0]


def compact_filters(masks, new_id_of_old) -> np.ndarray:
    """bool [n_filters][old rows] -> bool [n_filters][rows left]: the filters an index keeps across `HipIndex.remove` — entry j of
    a filter is its old entry for the row now at j.  A filter may end up allowing nothing."""
    m = np.atleast_2d(np.asarray(masks, dtype=bool))
    nid = np.asarray(new_id_of_old, dtype=np.int64).reshape(-1)
    if m.shape[1] != len(nid):
        raise ValueError(f"masks over {m.shape[1]} rows, a map over {len(nid)}")
    return np.ascontiguousarray(m[:, nid >= 0])


def _ranks_csr(ranks, lims) -> Tuple[np.ndarray, np.ndarray]:
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    lims = np.asarray(lims, dtype=np.int64).reshape(-1)
    if len(lims) < 1 or lims[0] != 0 or (np.diff(lims) < 0).any() or lims[-1] != len(ranks):
        raise ValueError("lims must start at 0, be non-decreasing and end at the number of ranks")
    if len(ranks) and ranks.min() < 0:
        raise ValueError("ranks are positions: 0 is the best row")
    return ranks, lims


def reciprocal_ranks(ranks, lims, cutoff: Optional[int] = None) -> np.ndarray:
    """float64 [nq]: 1 / (1 + the best rank among query q's positives `ranks[lims[q]:lims[q + 1]]`) (HipIndex.rank_rows: rank 0 is
    the best row); 0 for a query without positives, and with `cutoff` for one whose best positive has a rank >= cutoff."""
    ranks, lims = _ranks_csr(ranks, lims)
    out = np.zeros(len(lims) - 1, dtype=np.float64)
    for q in range(len(out)):
        if lims[q + 1] > lims[q]:
            best = int(ranks[lims[q]:lims[q + 1]].min())
            if cutoff is None or best < cutoff:
                out[q] = 1.0 / (best + 1)
    return out


def mrr_from_ranks(ranks, lims, cutoff: Optional[int] = None) -> float:
    """Mean reciprocal rank over all queries of `lims` from the ranks of their positives: with `cutoff=k` what `utils.eval_mrr`
    computes from a run of depth k, with `cutoff=None` the MRR no run of fixed depth can give."""
    rr = reciprocal_ranks(ranks, lims, cutoff)
    return float(rr.mean()) if len(rr) else 0.0


def recall_at(ranks, lims, ks) -> np.ndarray:
    """float64 [len(ks)]: recall@k for every k of `ks` — the share of a query's positives with a rank < k, averaged over the queries
    that have a positive (trec_eval's convention; 0 if none has)."""
    ranks, lims = _ranks_csr(ranks, lims)
    ks = np.asarray(ks, dtype=np.int64).reshape(-1)
    out = np.zeros(len(ks), dtype=np.float64)
    n = 0
    for q in range(len(lims) - 1):
        r = ranks[lims[q]:lims[q + 1]]
        if len(r):
            n += 1
            out += (r[None, :] < ks[:, None]).sum(1) / len(r)
    return out / n if n else out


NEVER_RETRIEVED = 1 << 62       # a rank no cut-off reaches


def never_retrieved(ranks) -> np.ndarray:
    """int64, shaped as `ranks`: the ranks of HipIndex.rank_groups with every -1 — a document the query's filter leaves no page
    of, which is not in the ranking — replaced by NEVER_RETRIEVED (2^62).  `reciprocal_ranks` / `mrr_from_ranks` / `recall_at`
    refuse negative ranks; with this they treat an absent positive as not retrieved: it misses every recall@k, falls outside
    every `cutoff`, and without a cut-off adds a reciprocal rank below 1e-18."""
    r = np.array(ranks, dtype=np.int64)
    if r.size and r.min() < -1:
        raise ValueError("ranks are positions, or -1 for a document that is not in the ranking")
    return np.where(r < 0, np.int64(NEVER_RETRIEVED), r)


def window_negatives(ids, positives_of_query, count: int) -> np.ndarray:
    """int64 [nq][count]: for every query the first `count` ids of its window `ids[q]` (HipIndex.search_window: rows in ranking
    order, -1 where the ranking has ended) that are not among `positives_of_query[q]` (a sequence of row ids per query, or a
    callable q -> row ids) — the window's order kept, padded with -1."""
    ids = np.asarray(ids, dtype=np.int64)
    if ids.ndim != 2:
        raise ValueError("ids must be [nq][k]")
    count = int(count)
    if count < 0:
        raise ValueError("count must be >= 0")
    get = positives_of_query if callable(positives_of_query) else (lambda q: positives_of_query[q])
    if not callable(positives_of_query) and len(positives_of_query) != len(ids):
        raise ValueError(f"{len(positives_of_query)} positive lists for {len(ids)} queries")
    out = np.full((len(ids), count), -1, dtype=np.int64)
    for q in range(len(ids)):
        pos = np.asarray(list(get(q)), dtype=np.int64).reshape(-1)
        row = ids[q]
        keep = row[(row >= 0) & ~np.isin(row, pos)][:count]
        out[q, :len(keep)] = keep
    return out


def fuse_runs(scores, ids, lims, k: int, fuse: str = "max") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """What per-sub-query top lists say about the fused ranking of `HipIndex.search_multi` -> (scores f32 [n_groups][k], ids i64
    [n_groups][k], determined bool [n_groups]).  `scores` / `ids` [n_sub][depth] are the lists of `search(depth)` for every
    sub-query (best first, tails (-inf, -1)); group g holds sub-queries lims[g] .. lims[g + 1] - 1.  The result is ranked score
    descending, then lower id first, padded with (-inf, -1).

    fuse="max" ("any-of"): a listed row scores as the best of its listed scores.  A row of the true top-k stands in the top-k
    of the sub-query that decides it, so with depth >= k (or lists that ended: every row is listed) the answer is the true
    one: determined.  fuse="min" ("all-of"): only a row that appears in EVERY list of its group has a known score, and a row
    missing from a full list j may still score up to that list's last entry.  The rows returned are those of every list;
    `determined[g]` says whether k of them (or, when every list ended, all of them) lie strictly above that bound — otherwise
    a row at rank 5 000 for one part and rank 3 for the other may belong in front, and no top-k list shows it."""
    if fuse not in ("max", "min"):
        raise ValueError("fuse must be 'max' or 'min'")
    scores, ids = np.asarray(scores, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    lims = np.asarray(lims, dtype=np.int64).reshape(-1)
    k = int(k)
    if scores.ndim != 2 or scores.shape != ids.shape:
        raise ValueError("scores and ids must both be [n_sub][depth]")
    if len(lims) < 1 or lims[0] != 0 or (np.diff(lims) < 1).any() or lims[-1] != len(ids):
        raise ValueError("lims must start at 0, increase and end at the number of sub-queries")
    if k < 1:
        raise ValueError("k must be >= 1")
    ng, depth = len(lims) - 1, scores.shape[1]
    out_s = np.full((ng, k), -np.inf, dtype=np.float32)
    out_i = np.full((ng, k), -1, dtype=np.int64)
    determined = np.zeros(ng, dtype=bool)
    for g in range(ng):
        rows: dict = {}                                # row -> [fused score so far, lists it appears in]
        ended, bound = True, -np.inf                   # every list ended | the largest last entry of a full list
        m = int(lims[g + 1] - lims[g])
        for s in range(int(lims[g]), int(lims[g + 1])):
            live = ids[s] >= 0
            if live.all() and depth > 0:
                ended, bound = False, max(bound, float(scores[s, -1]))
            for i, v in zip(ids[s][live].tolist(), scores[s][live].tolist()):
                e = rows.get(i)
                if e is None:
                    rows[i] = [v, 1]
                else:
                    e[0], e[1] = (max(e[0], v) if fuse == "max" else min(e[0], v)), e[1] + 1
        known = [(v, i) for i, (v, c) in rows.items() if fuse == "max" or c == m]
        known.sort(key=lambda t: (-t[0], t[1]))
        top = known[:k]
        out_s[g, :len(top)] = [v for v, _ in top]
        out_i[g, :len(top)] = [i for _, i in top]
        if fuse == "max" or m == 1:                    # (a group of one: the list itself, under either fusion)
            determined[g] = ended or depth >= k
        else:
            determined[g] = ended or (len(top) == k and top[-1][0] > bound)
    return out_s, out_i, determined


def evidence_pages(ev_rows, ev_scores, limit: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The page list a generator gets from ONE question's evidence of `HipIndex.search_multi_groups(evidence=True)`:
    `ev_rows` / `ev_scores` [k][m] hold, per returned document (slot) and sub-question, the document's best page and its score.
    -> (rows i64, scores f32): the DISTINCT evidence rows in (slot, sub-question) order — the best document's pages first —
    each with the best score seen for it (one page may serve several sub-questions), tail entries (-1) skipped, cut at `limit`
    pages."""
    rows = np.asarray(ev_rows, dtype=np.int64)
    scores = np.asarray(ev_scores, dtype=np.float32)
    if rows.shape != scores.shape:
        raise ValueError("ev_rows and ev_scores must have one shape")
    if limit is not None and limit < 0:
        raise ValueError("limit must be >= 0")
    best: dict = {}                                    # row -> best score; dicts keep the order of first appearance
    for r, v in zip(rows.reshape(-1).tolist(), scores.reshape(-1).tolist()):
        if r < 0:
            continue
        if r not in best:
            if limit is not None and len(best) >= limit:
                continue
            best[r] = v
        elif v > best[r]:
            best[r] = v
    return np.asarray(list(best.keys()), dtype=np.int64), np.asarray(list(best.values()), dtype=np.float32)


RRF_ID_MAX = 2 ** 31 - 2        # ids of a rank fusion lie in [0, RRF_ID_MAX]; anything else is an empty slot


def _f32_orderable(x: np.ndarray) -> np.ndarray:
    """the ranking's order of float32 values as uint32 keys (-0.0 < +0.0), as the library's make_key has it"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def rrf_runs(ids, lims, k: int, c: float = 60.0, weights=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Reciprocal-rank fusion of top lists, the definition of `HipIndex.search_rrf` / `engine.rrf_fuse` (include/visrag_hip.h:
    vr_rrf_fuse) in vectorised numpy, bit for bit -> (scores f32 [n_groups][k], ids i64 [n_groups][k], hits i32 [n_groups][k]).
    `ids` [n_lists][depth]: slot r of list j holds an id in [0, 2^31 - 2] (anything else: an empty slot); group g holds lists
    lims[g] .. lims[g + 1] - 1.  An id scores F = float32(sum of float64(w_j) / (float64(float32(c)) + float64(r + 1)) over
    its entries (j, r)), the float64 sum started at 0.0 and taken in ascending (j, r); `hits` counts the entries.  The result
    is ranked F descending (in the ranking's order of floats), then lower id first, and padded with (-inf, -1, 0).  This is
    also the host workaround the device call replaces: `search(k=depth)` per sub-query, the lists pulled to the host, this."""
    ids = np.asarray(ids, dtype=np.int64)
    lims = np.asarray(lims, dtype=np.int64).reshape(-1)
    k = int(k)
    if ids.ndim != 2:
        raise ValueError("ids must be [n_lists][depth]")
    if len(lims) < 1 or lims[0] != 0 or (np.diff(lims) < 1).any() or lims[-1] != len(ids):
        raise ValueError("lims must start at 0, increase and end at the number of lists")
    if k < 1:
        raise ValueError("k must be >= 1")
    c32 = np.float32(c)
    if not np.isfinite(c32) or c32 < 0:
        raise ValueError("c must be finite and >= 0")
    n_lists, ng = len(ids), len(lims) - 1
    w = np.ones(n_lists, dtype=np.float32) if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
    if len(w) != n_lists or not np.isfinite(w).all():
        raise ValueError("weights must be one finite value per list")
    out_s = np.full((ng, k), -np.inf, dtype=np.float32)
    out_i = np.full((ng, k), -1, dtype=np.int64)
    out_h = np.zeros((ng, k), dtype=np.int32)
    jj, rr = np.nonzero((ids >= 0) & (ids <= RRF_ID_MAX))             # row-major: ascending (j, r)
    if len(jj) == 0:
        return out_s, out_i, out_h
    e_id = ids[jj, rr]
    e_g = np.repeat(np.arange(ng, dtype=np.int64), np.diff(lims))[jj]
    term = w[jj].astype(np.float64) / (np.float64(c32) + (rr + 1).astype(np.float64))
    order = np.lexsort((e_id, e_g))                                   # stable: (j, r) stays ascending inside an (group, id) segment
    e_id, e_g, term = e_id[order], e_g[order], term[order]
    head = np.ones(len(e_id), dtype=bool)
    head[1:] = (e_id[1:] != e_id[:-1]) | (e_g[1:] != e_g[:-1])
    starts = np.flatnonzero(head)
    seg = np.cumsum(head) - 1
    t = np.arange(len(e_id)) - starts[seg]                            # an entry's place inside its segment
    hits = np.bincount(seg, minlength=len(starts))
    by_t = np.argsort(t, kind="stable")
    cut = np.concatenate([[0], np.cumsum(np.bincount(t))])
    acc = np.zeros(len(starts), dtype=np.float64)
    for step in range(len(cut) - 1):                                  # the t-th entry of every segment that has one: the sum's order
        sel = by_t[cut[step]:cut[step + 1]]
        acc[seg[sel]] += term[sel]                                    # (distinct segments: a plain vector add)
    with np.errstate(over="ignore"):
        F = acc.astype(np.float32)
    sg, sid = e_g[starts], e_id[starts]
    rank = np.lexsort((sid, -_f32_orderable(F).astype(np.int64), sg))
    sg, sid, F, hits = sg[rank], sid[rank], F[rank], hits[rank]
    first = np.concatenate([[0], np.cumsum(np.bincount(sg, minlength=ng))])
    place = np.arange(len(sg)) - first[sg]
    keep = place < k
    out_s[sg[keep], place[keep]] = F[keep]
    out_i[sg[keep], place[keep]] = sid[keep]
    out_h[sg[keep], place[keep]] = hits[keep]
    return out_s, out_i, out_h
