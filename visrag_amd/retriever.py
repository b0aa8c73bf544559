"""Retrieval with the reference's signature (src/openmatch/retriever/dense_retriever.py:37-97):
`distributed_parallel_retrieve(args, topk) -> {qid: {docid: score}}` over the pickle shards in
`args.output_dir`, this rank's query shard(s) against ALL corpus shards.

The per-shard `torch.matmul` + `torch.topk` (dense_retriever.py:13-34) is replaced by the
HBM-resident HipIndex: corpus shards are appended to one device index and searched with the
fused bf16-MFMA similarity + bitonic top-k kernel, fp32 re-scored.  Like the reference, the
default result is the UNION of the per-shard top-k lists (up to k * n_shards docs per query,
dense_retriever.py:79-92 — `save_as_trec` writes all of them); `global_topk=True` keeps only the
global top-k (one search over the concatenated index: the fast path when only depth k is
evaluated).

Two ways to run it under torchrun (one process per GPU), same result, byte for byte in the TREC file:
  * replicated (the reference's: dense_retriever.py:48-69): every rank loads ALL corpus shards into its own GPU
    and searches its own queries — N copies of the index, no exchange;
  * corpus-sharded (`sharded=True`, `args.sharded_corpus`, or VISRAG_SHARDED_RETRIEVE=1; BASELINE.json north_star):
    rank r loads only the corpus shards rank r wrote (`embeddings.corpus.rank.{r}*`: the rows it embedded),
    every rank searches ALL queries against its shard, ONE all-gather of the packed per-shard top-k keys,
    and each rank returns the entries of ITS queries — so the caller (driver/eval.py:210-232: save_as_trec per
    rank, rank-0 merge) is unchanged.

`sharded_search` is the data path of the second form for one local index: local top-k emitted as packed 64-bit
(score, global id) keys by the search's own merge kernel, ONE RCCL all-gather of those [nq, k] words, on-device
merge of the gathered buffer."""
from __future__ import annotations

import logging
import os
import warnings
from typing import Callable, Dict, Hashable, List, Optional, Tuple

import numpy as np
import torch

from .documents import collection_filters, group_rows, label_filters, window_negatives
from .engine import HipIndex, rrf_fuse, topk_merge_keys
from .utils import list_shards, read_shard, shard_rank as _shard_rank

logger = logging.getLogger(__name__)


def _device_index(args) -> int:
    """args.device (reference: dense_retriever.py:23, `.to(args.device)`) -> cuda index; a bare
    'cuda' / missing device means this process's own GPU (LOCAL_RANK, else the current device)."""
    from .modeling import _device_index as _idx, default_device
    dev = getattr(args, "device", None)
    if dev is None:
        lr = getattr(args, "local_rank", None)
        return int(lr) if lr is not None and int(lr) >= 0 else default_device()
    i = _idx(dev)
    return default_device() if i is None else i


def _load_queries(args, rank="own") -> Tuple[np.ndarray, List[str], List[bool]]:
    """-> (reps, ids, mine): the query shards of this process (`rank="own"`: dense_retriever.py:40-46) or of every
    process (`rank=None`), in sorted file order; mine[i] = query i belongs to this process's own shards."""
    parts = list_shards(args.output_dir, "query", args.process_index if rank == "own" else None)
    own = set(list_shards(args.output_dir, "query", args.process_index))
    if rank != "own":
        # corpus-sharded form: a query file belongs to the process its rank field maps to — the same rule as the corpus files
        # (rank % world), so a retrieval world smaller than the encoding world drops nothing
        dist = torch.distributed
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        own = {p for p in parts if _shard_rank(p) % world == int(args.process_index) % world}
    logger.info("query_all_partitions = %s", parts)
    reps, ids, mine = [], [], []
    for p in parts:
        r, i = read_shard(p)
        if len(i) == 0:
            continue
        reps.append(r)
        ids.extend(i)
        mine.extend([p in own] * len(i))
    if not reps:
        raise ValueError("No pre-computed query embeddings found")
    return np.concatenate(reps), ids, mine


def _sharded_requested(args, sharded: Optional[bool]) -> bool:
    if sharded is None:
        sharded = getattr(args, "sharded_corpus", None)
    if sharded is None:
        sharded = os.environ.get("VISRAG_SHARDED_RETRIEVE", "0") not in ("", "0")
    return bool(sharded) and _collective_wanted()


def _collective_wanted(group=None) -> bool:
    """A process group of two or more ranks exchanges; a group of ONE rank returns its own result without touching the
    backend (a single-rank run that happens to have initialised torch.distributed needs no working all-gather) unless
    VISRAG_SHARDED_RETRIEVE=force asks for the transport anyway (the one-GPU RCCL test)."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size(group) > 1 or os.environ.get("VISRAG_SHARDED_RETRIEVE", "") == "force"


def _corpus(args) -> Tuple[np.ndarray, List[str], List[str]]:
    """-> (queries, qids, corpus_parts): this rank's queries and the files of ALL corpus shards; missing queries are reported
    before missing documents"""
    queries, qids, _ = _load_queries(args)
    corpus_parts = list_shards(args.output_dir, "corpus")
    if len(corpus_parts) == 0:
        raise ValueError("No pre-computed document embeddings found")
    logger.info("corpus_all_partitions = %s", corpus_parts)
    return queries, qids, corpus_parts


def _whole_corpus(corpus_parts) -> Tuple[List[np.ndarray], List[str]]:
    """-> (the float32 rows of every shard that has some, their ids in one list): what ONE index over all shards holds"""
    reps, ids = [], []
    for p in corpus_parts:
        r, i = read_shard(p)
        if len(i):
            reps.append(np.asarray(r, dtype=np.float32))
            ids.extend(i)
    return reps, ids


def _filter_index(keys, labels_of: Callable) -> Tuple[List[Optional[frozenset]], np.ndarray]:
    """-> (the DISTINCT label sets `labels_of(key)` in the order they first appear, None = everything; int32 [len(keys)]: the set
    of each key): one filter is built per distinct set"""
    sets: List[Optional[frozenset]] = []
    which: Dict[Optional[frozenset], int] = {}
    filter_of = np.empty(len(keys), dtype=np.int32)
    for i, key in enumerate(keys):
        wanted = labels_of(key)
        labels = None if wanted is None else frozenset(wanted)
        if labels not in which:
            which[labels] = len(sets)
            sets.append(labels)
        filter_of[i] = which[labels]
    return sets, filter_of


def _document_index(make_index, dim, reps, page_ids, doc_of, dev, keys=(), label_of_doc=None, labels_of=None, grouping=None):
    """ONE index over the pages of all shards, reordered so that every document's pages are adjacent (documents.group_rows of
    `doc_of`, or `grouping` if the caller has it already), the documents set as its groups; with `label_of_doc` and `labels_of`
    one filter per distinct label set of `keys`.  -> (ix, order, docs, filter_of): row r of the index is page `page_ids[order[r]]`,
    `filter_of` the filter of each key, None without labels.  The caller closes the index."""
    order, offsets, docs = grouping or group_rows([doc_of(i) for i in page_ids])
    ix = make_index(dim, len(page_ids), dev)
    ix.add(np.concatenate(reps)[order])
    ix.set_groups(offsets)
    filter_of = None
    if label_of_doc is not None and labels_of is not None:
        sets, filter_of = _filter_index(keys, labels_of)
        ix.set_filters(collection_filters(offsets, [label_of_doc(d) for d in docs], sets))
    return ix, order, docs, filter_of


def _each_shard(shards, make_index, dim, dev, as_float32: bool = True):
    """`shards`: (reps, ids) pairs, read as they are asked for -> yields (ix, ids) per shard that has rows, the index filled with
    that shard alone and closed when the consumer moves on (or stops): the index never holds more than one shard"""
    for reps, ids in shards:
        if len(ids) == 0:
            continue
        ix = make_index(dim, len(ids), dev)
        try:
            ix.add(np.asarray(reps, dtype=np.float32) if as_float32 else reps)
            yield ix, ids
        finally:
            ix.close()


def _shard_lists(shards, make_index, dim, dev, search: Callable) -> Tuple[List[np.ndarray], List[np.ndarray], List[str]]:
    """`search(ix, ids) -> (scores [n][d], rows [n][d], ...)` over one shard at a time -> (the scores of every shard, its rows as
    GLOBAL positions — shifted by the rows of the shards before, -1 kept — and the ids of all shards): what merge_pages_host takes"""
    all_ids: List[str] = []
    lists_s, lists_p = [], []
    for ix, ids in _each_shard(shards, make_index, dim, dev):
        sc, rows = search(ix, ids)[:2]
        rows = np.asarray(rows, dtype=np.int64)
        lists_s.append(np.asarray(sc, dtype=np.float32))
        lists_p.append(np.where(rows >= 0, rows + len(all_ids), -1))
        all_ids.extend(ids)
    return lists_s, lists_p, all_ids


def _fill(result: Dict, keys, scores, ids, names) -> Dict:
    """result[key][names[id]] = score for the taken slots (id >= 0) of every key's list, in list order"""
    for row, key in enumerate(keys):
        for s, j in zip(scores[row], ids[row]):
            if j >= 0:
                result[key][names[int(j)]] = float(s)
    return result


def _fill_documents(scores: Dict, pages: Dict, key, sc, rows, groups, docs, page_ids, order) -> None:
    """one key's document list: scores[key][doc] = score, pages[key][doc] = the id of its best page, for the taken slots"""
    for s, r, g in zip(sc, rows, groups):
        if r >= 0:
            scores[key][docs[int(g)]] = float(s)
            pages[key][docs[int(g)]] = page_ids[int(order[int(r)])]


def distributed_parallel_retrieve(args, topk: int, global_topk: bool = False, sharded: Optional[bool] = None,
                                  index_factory: Optional[Callable] = None, merge_keys: Optional[Callable] = None
                                  ) -> Dict[str, Dict[str, float]]:
    """`index_factory(dim, capacity, device)` / `merge_keys` default to HipIndex / vr_topk_merge_keys; the CPU (gloo)
    tests inject host stand-ins so that THIS function is what runs under world_size 2."""
    make_index = index_factory or HipIndex
    if _sharded_requested(args, sharded):
        return _retrieve_corpus_sharded(args, topk, global_topk, make_index, merge_keys)
    queries, qids, corpus_parts = _corpus(args)
    dev = _device_index(args)
    result: Dict[str, Dict[str, float]] = {q: {} for q in qids}
    dim = queries.shape[1]
    if not global_topk:
        for ix, ids in _each_shard(map(read_shard, corpus_parts), make_index, dim, dev, as_float32=False):
            sc, idx = ix.search(queries, topk)
            _fill(result, qids, sc, idx, ids)
        return result
    shards = [read_shard(p) for p in corpus_parts]
    total = sum(len(i) for _, i in shards)
    ix = make_index(dim, max(total, 1), dev)
    all_ids: List[str] = []
    for reps, ids in shards:
        if len(ids):
            ix.add(reps)
            all_ids.extend(ids)
    sc, idx = ix.search(queries, topk)
    ix.close()
    return _fill(result, qids, sc, idx, all_ids)


def retrieve_documents(args, topk: int, doc_of: Callable[[str], str], index_factory: Optional[Callable] = None
                       ) -> Tuple[Dict[str, Dict[str, float]], Dict[str, Dict[str, str]]]:
    """Document-level retrieval over the same pickle shards: this rank's query shard(s) against ALL corpus shards, the corpus
    rows being PAGES and `doc_of(page_id)` the document a page belongs to.  -> ({qid: {doc: score}}, {qid: {doc: best_page_id}}):
    the `topk` best documents per query, a document scoring as its best page does (HipIndex.search_groups: the fp32 ranking);
    the first dict goes to `save_as_trec` as it is.  Pages of a document need not be adjacent or in one shard: all shards are
    loaded into ONE index, reordered so that they are (documents.group_rows).

    Replicated form only: every rank holds the whole corpus.  Corpus-sharded multi-GPU grouped search is out of scope — a
    document may straddle the shards of two ranks, and a per-rank best page is not a document's best page."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    reps, page_ids = _whole_corpus(corpus_parts)
    scores: Dict[str, Dict[str, float]] = {q: {} for q in qids}
    pages: Dict[str, Dict[str, str]] = {q: {} for q in qids}
    if not page_ids or topk <= 0:
        return scores, pages
    ix, order, docs, _ = _document_index(make_index, queries.shape[1], reps, page_ids, doc_of, _device_index(args))
    sc, rows, groups = ix.search_groups(queries, min(topk, len(docs)))
    ix.close()
    for qi, q in enumerate(qids):
        _fill_documents(scores, pages, q, sc[qi], rows[qi], groups[qi], docs, page_ids, order)
    return scores, pages


def retrieve_filtered(args, topk: int, label_of: Callable[[str], object], labels_of_query: Callable[[str], Optional[set]],
                      index_factory: Optional[Callable] = None) -> Dict[str, Dict[str, float]]:
    """Retrieval inside a subset of the corpus, over the same pickle shards: this rank's query shard(s) against ALL corpus
    shards in ONE index, query `qid` ranked only against the rows whose `label_of(docid)` is in `labels_of_query(qid)` (None =
    every row) — a dataset, a tenant, a few documents.  -> {qid: {docid: score}}: the `topk` best ALLOWED rows per query
    (HipIndex.search_filtered: the fp32 ranking inside the subset, fewer entries when fewer rows are allowed); it goes to
    `save_as_trec` as it is.  One filter is built per distinct label set.

    Replicated form only, like retrieve_documents: every rank holds the whole corpus."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    reps, doc_ids = _whole_corpus(corpus_parts)
    result: Dict[str, Dict[str, float]] = {q: {} for q in qids}
    if not doc_ids or topk <= 0:
        return result
    sets, filter_of_query = _filter_index(qids, labels_of_query)
    ix = make_index(queries.shape[1], len(doc_ids), _device_index(args))
    ix.add(np.concatenate(reps))
    ix.set_filters(label_filters([label_of(i) for i in doc_ids], sets))
    sc, rows = ix.search_filtered(queries, min(topk, len(doc_ids)), filter_of_query)
    ix.close()
    return _fill(result, qids, sc, rows, doc_ids)


def retrieve_documents_filtered(args, topk: int, doc_of: Callable[[str], str], label_of_doc: Callable[[str], object],
                                labels_of_query: Callable[[str], Optional[set]], offset: int = 0,
                                index_factory: Optional[Callable] = None
                                ) -> Tuple[Dict[str, Dict[str, float]], Dict[str, Dict[str, str]]]:
    """Document-level retrieval inside a subset of the documents, over the same pickle shards: retrieve_documents plus
    retrieve_filtered.  The corpus rows are PAGES, `doc_of(page_id)` the document of a page, `label_of_doc(doc)` the collection of
    a document; query `qid` ranks only the documents whose label is in `labels_of_query(qid)` (None = every document).
    -> ({qid: {doc: score}}, {qid: {doc: best_page_id}}): the documents at ranks offset .. offset + topk - 1 of that ranking, a
    document scoring as its best page does (HipIndex.search_groups_window: the fp32 ranking, exact however deep the offset, fewer
    entries where the ranking ends); the first dict goes to `save_as_trec` as it is.  One filter is built per distinct label set.

    Replicated form only, like retrieve_documents: every rank holds the whole corpus."""
    if offset < 0:
        raise ValueError("offset must be >= 0")
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    reps, page_ids = _whole_corpus(corpus_parts)
    scores: Dict[str, Dict[str, float]] = {q: {} for q in qids}
    pages: Dict[str, Dict[str, str]] = {q: {} for q in qids}
    if not page_ids or topk <= 0:
        return scores, pages
    ix, order, docs, filter_of_query = _document_index(make_index, queries.shape[1], reps, page_ids, doc_of, _device_index(args),
                                                       qids, label_of_doc, labels_of_query)
    for o in range(int(offset), min(int(offset) + topk, len(docs)), WINDOW_PAGE):     # a list longer than one window: paged
        sc, rows, groups = ix.search_groups_window(queries, o, min(WINDOW_PAGE, int(offset) + topk - o, len(docs) - o), filter_of_query)
        for qi, q in enumerate(qids):
            _fill_documents(scores, pages, q, sc[qi], rows[qi], groups[qi], docs, page_ids, order)
    ix.close()
    return scores, pages


def rank_documents(args, docs_of_query, doc_of: Callable[[str], str], label_of_doc: Optional[Callable[[str], object]] = None,
                   labels_of_query: Optional[Callable[[str], Optional[set]]] = None, index_factory: Optional[Callable] = None
                   ) -> Dict[str, Dict[str, Tuple[float, Optional[str], int]]]:
    """Where named DOCUMENTS stand, over the same pickle shards: `docs_of_query` is {qid: [doc, ...]} (qrels that name a PDF, not a
    page) or a callable qid -> docs; -> {qid: {doc: (score, best_page_id, rank)}}.  The corpus rows are PAGES, `doc_of(page_id)`
    the document of a page; a document scores as its best page does and `rank` is its position (0 = the best) in the ranking of
    ALL documents, however deep it lies (HipIndex.rank_groups: exact counts, no run of fixed depth) — the ranking
    `retrieve_documents` / `retrieve_documents_filtered` cut at a k.  With `label_of_doc` and `labels_of_query` given, query `qid`
    ranks only the documents whose label is in `labels_of_query(qid)` (None = every document), one filter per distinct label
    set; a named document outside them is not in that ranking: (-inf, None, -1) — `documents.never_retrieved` turns such ranks
    into what `mrr_from_ranks` / `recall_at` count as a miss.  Without labels there is no filter.  A document no page belongs to
    raises ValueError; a query without documents gets {}.

    Replicated form only, like retrieve_documents: every rank holds the whole corpus, all shards in ONE index."""
    if (label_of_doc is None) != (labels_of_query is None):
        raise ValueError("label_of_doc and labels_of_query go together")
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    reps, page_ids = _whole_corpus(corpus_parts)
    get = docs_of_query if callable(docs_of_query) else (lambda q: docs_of_query.get(q, ()))
    wanted = [list(dict.fromkeys(get(q))) for q in qids]                  # a document named twice counts once
    lims = np.concatenate([np.zeros(1, np.int64), np.cumsum([len(w) for w in wanted])]).astype(np.int64)
    flat = [d for w in wanted for d in w]
    if not flat:
        return {q: {} for q in qids}
    grouping = group_rows([doc_of(i) for i in page_ids])
    group_of = {d: g for g, d in enumerate(grouping[2])}
    missing = [d for d in flat if d not in group_of]
    if missing:
        raise ValueError(f"no such document in the corpus shards: {missing[0]}")
    ix, order, _, filter_of_query = _document_index(make_index, queries.shape[1], reps, page_ids, doc_of, _device_index(args),
                                                    qids, label_of_doc, labels_of_query, grouping)
    sc, rows, rk = ix.rank_groups(queries, np.asarray([group_of[d] for d in flat], dtype=np.int64), lims, filter_of_query)
    ix.close()
    return {q: {d: (float(sc[j]), page_ids[int(order[int(rows[j])])] if rows[j] >= 0 else None, int(rk[j]))
                for j, d in zip(range(lims[qi], lims[qi + 1]), wanted[qi])}
            for qi, q in enumerate(qids)}


def retrieve_documents_range(args, threshold: float, doc_of: Callable[[str], str], label_of_doc: Optional[Callable[[str], object]] = None,
                             labels_of_query: Optional[Callable[[str], Optional[set]]] = None, max_per_query: Optional[int] = None,
                             index_factory: Optional[Callable] = None
                             ) -> Tuple[Dict[str, Dict[str, float]], Dict[str, Dict[str, str]]]:
    """A run of variable depth over DOCUMENTS, over the same pickle shards: retrieve_range one level up.  The corpus rows are
    PAGES, `doc_of(page_id)` the document of a page; a document scores as its best page does, and query `qid` gets every document
    whose score is at least `threshold` (HipIndex.search_groups_range: the exact fp32 answer, not cut at a k).
    -> ({qid: {doc: score}}, {qid: {doc: best_page_id}}), a query's entries best first (score descending, then the order the
    documents first appear in the shards); the first dict goes to `save_as_trec` as it is.  With `label_of_doc` and
    `labels_of_query` given, query `qid` sees only the documents whose label is in `labels_of_query(qid)` (None = every document),
    one filter per distinct label set, as in retrieve_documents_filtered; without them there is no filter.  `max_per_query`, if
    given, keeps a query's best entries only.

    Replicated form only, like retrieve_documents: every rank holds the whole corpus, all shards in ONE index — a document's
    pages may straddle the shards."""
    if (label_of_doc is None) != (labels_of_query is None):
        raise ValueError("label_of_doc and labels_of_query go together")
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    reps, page_ids = _whole_corpus(corpus_parts)
    scores: Dict[str, Dict[str, float]] = {q: {} for q in qids}
    pages: Dict[str, Dict[str, str]] = {q: {} for q in qids}
    if not page_ids or (max_per_query is not None and max_per_query <= 0):
        return scores, pages
    ix, order, docs, filter_of_query = _document_index(make_index, queries.shape[1], reps, page_ids, doc_of, _device_index(args),
                                                       qids, label_of_doc, labels_of_query)
    lims, sc, rows, groups = ix.search_groups_range(queries, float(threshold), filter_of_query)
    ix.close()
    for qi, q in enumerate(qids):
        a, b = int(lims[qi]), int(lims[qi + 1])
        if max_per_query is not None:
            b = min(b, a + int(max_per_query))
        _fill_documents(scores, pages, q, sc[a:b], rows[a:b], groups[a:b], docs, page_ids, order)
    return scores, pages


def retrieve_range(args, threshold: float, max_per_query: Optional[int] = None, index_factory: Optional[Callable] = None
                   ) -> Dict[str, Dict[str, float]]:
    """A run of variable depth over the same pickle shards: this rank's query shard(s) against ALL corpus shards, every row
    whose score is at least `threshold` (HipIndex.search_range: the exact fp32 answer, not cut at a k).  -> {qid: {docid:
    score}}, a query's entries best first; it goes to `save_as_trec` as it is.  The corpus is taken shard by shard: a range
    result is the union of the shard results, so no merge kernel is involved and the index never holds more than one shard.
    `max_per_query`, if given, keeps a query's best entries only (score descending, then shard and row order).

    Replicated form only, like retrieve_documents: every rank sees the whole corpus."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    found: List[List[Tuple[float, str]]] = [[] for _ in qids]
    for ix, ids in _each_shard(map(read_shard, corpus_parts), make_index, queries.shape[1], _device_index(args)):
        lims, sc, rows = ix.search_range(queries, float(threshold))
        for qi in range(len(qids)):
            found[qi].extend((float(s), ids[int(r)]) for s, r in zip(sc[lims[qi]:lims[qi + 1]], rows[lims[qi]:lims[qi + 1]]))
    result: Dict[str, Dict[str, float]] = {}
    for q, entries in zip(qids, found):
        entries.sort(key=lambda e: -e[0])                # stable: equal scores keep shard and row order
        if max_per_query is not None:
            entries = entries[:max(int(max_per_query), 0)]
        result[q] = {d: s for s, d in entries}
    return result


def rank_rows(args, targets_of_query, index_factory: Optional[Callable] = None) -> Dict[str, Dict[str, Tuple[float, int]]]:
    """Where named rows stand, over the same pickle shards: `targets_of_query` is {qid: [docid, ...]} (the qrel positives, say) or
    a callable qid -> docids; -> {qid: {docid: (score, rank)}} with `score` the row's fp32 score and `rank` its position (0 = the
    best) in the ranking of the WHOLE corpus — score descending, then shard and row order — however deep it lies
    (HipIndex.rank_rows / count_range: exact counts, no run of fixed depth).  `documents.mrr_from_ranks` / `recall_at` take the
    ranks.  The corpus is taken shard by shard, twice, and the index never holds more than one shard: the shard that holds a
    target gives its score and its rank inside the shard; every EARLIER shard adds its rows with a score >= that score (on equal
    scores the earlier position is ahead), every LATER shard its rows with a score > it.  Counts add up over shards, which no
    top-k list does: the sum is the global rank.  A docid in no shard raises ValueError; a query without targets gets {}.

    Replicated form only, like retrieve_documents: every rank sees the whole corpus."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    dev = _device_index(args)
    get = targets_of_query if callable(targets_of_query) else (lambda q: targets_of_query.get(q, ()))
    wanted = [list(dict.fromkeys(get(q))) for q in qids]                  # a docid named twice counts once
    lims = np.concatenate([np.zeros(1, np.int64), np.cumsum([len(w) for w in wanted])]).astype(np.int64)
    query_of = np.repeat(np.arange(len(qids)), np.diff(lims))
    flat = [d for w in wanted for d in w]
    n = len(flat)
    shard_of, scores, ranks = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int64)
    if n:
        # pass 1: a target's own shard: its score and the rows of that shard ahead of it
        for si, p in enumerate(corpus_parts):
            reps, ids = read_shard(p)
            row_of: Dict[str, int] = {}
            for r, d in enumerate(ids):
                row_of.setdefault(d, r)
            here = np.asarray([j for j in range(n) if shard_of[j] < 0 and flat[j] in row_of], dtype=np.int64)
            if len(here) == 0:
                continue
            ix = make_index(queries.shape[1], len(ids), dev)
            ix.add(np.asarray(reps, dtype=np.float32))
            sub = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.bincount(query_of[here], minlength=len(qids)))]).astype(np.int64)
            sc, rk = ix.rank_rows(queries, np.asarray([row_of[flat[j]] for j in here], dtype=np.int64), sub)
            ix.close()
            shard_of[here], scores[here], ranks[here] = si, sc, rk
        if (shard_of < 0).any():
            raise ValueError(f"no such document in the corpus shards: {flat[int(np.argmax(shard_of < 0))]}")
        # pass 2: every other shard: its rows at or above (earlier shard) / above (later shard) the target's score
        for si, p in enumerate(corpus_parts):
            ix = None
            for strict in (False, True):
                there = np.flatnonzero(shard_of < si) if strict else np.flatnonzero(shard_of > si)
                if len(there) == 0:
                    continue
                if ix is None:
                    reps, ids = read_shard(p)
                    if len(ids) == 0:
                        break
                    ix = make_index(queries.shape[1], len(ids), dev)
                    ix.add(np.asarray(reps, dtype=np.float32))
                sub = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.bincount(query_of[there], minlength=len(qids)))]).astype(np.int64)
                ranks[there] += ix.count_range(queries, scores[there], sub, strict=strict)
            if ix is not None:
                ix.close()
    return {q: {d: (float(scores[j]), int(ranks[j])) for j, d in zip(range(lims[qi], lims[qi + 1]), wanted[qi])}
            for qi, q in enumerate(qids)}


WINDOW_PAGE = 1000          # rows per HipIndex.search_window call (its k limit)


def _shard_pages(ix, queries, first: int, count: int, page: int = WINDOW_PAGE) -> Tuple[np.ndarray, np.ndarray]:
    """ranks [first, first + count) of every query over one index, paged in windows of <= `page` -> (scores [nq][count] f32,
    rows [nq][count] i64), tails (-inf, -1)"""
    if count <= 0:
        return np.zeros((len(queries), 0), dtype=np.float32), np.zeros((len(queries), 0), dtype=np.int64)
    sc, rows = [], []
    for o in range(first, first + count, page):
        s, r = ix.search_window(queries, o, min(page, first + count - o))
        sc.append(np.asarray(s, dtype=np.float32)); rows.append(np.asarray(r, dtype=np.int64))
    return np.concatenate(sc, axis=1), np.concatenate(rows, axis=1)


def merge_pages_host(scores: List[np.ndarray], positions: List[np.ndarray], depth: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per-shard lists (scores [nq][d_s] f32, GLOBAL positions [nq][d_s] i64 with -1 for an empty slot) -> the best `depth`
    entries per query (scores [nq][depth], positions [nq][depth]), by score descending, then global position ascending; tails
    (-inf, -1).  The global top `depth` is contained in the union of the shards' top `depth`."""
    sc = np.concatenate([np.asarray(s, dtype=np.float32) for s in scores], axis=1)
    pos = np.concatenate([np.asarray(p, dtype=np.int64) for p in positions], axis=1)
    nq = sc.shape[0]
    out_s = np.full((nq, depth), -np.inf, dtype=np.float32)
    out_p = np.full((nq, depth), -1, dtype=np.int64)
    for q in range(nq):
        live = np.flatnonzero(pos[q] >= 0)
        order = live[np.lexsort((pos[q][live], -sc[q][live].astype(np.float64)))][:depth]
        out_s[q, :len(order)], out_p[q, :len(order)] = sc[q][order], pos[q][order]
    return out_s, out_p


def retrieve_deep(args, depth: int, index_factory: Optional[Callable] = None) -> Dict[str, Dict[str, float]]:
    """A run of any depth over the same pickle shards: this rank's query shard(s) against ALL corpus shards, the `depth` best
    rows of the WHOLE corpus per query — score descending, then shard and row order — with `depth` beyond the 1 000 rows one
    `search` returns.  -> {qid: {docid: score}}, a query's entries best first; it goes to `save_as_trec` as it is, and at
    depth <= 1000 it is the run of `distributed_parallel_retrieve(args, depth, global_topk=True)`.  The corpus is taken shard
    by shard and the index never holds more than one shard: every shard is paged in windows of <= 1 000 rows down to `depth`
    (HipIndex.search_window: exact at every offset), the per-shard lists are merged on the host.

    Replicated form only, like retrieve_documents: every rank sees the whole corpus."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    depth = int(depth)
    result: Dict[str, Dict[str, float]] = {q: {} for q in qids}
    if depth <= 0:
        return result
    lists_s, lists_p, all_ids = _shard_lists(map(read_shard, corpus_parts), make_index, queries.shape[1], _device_index(args),
                                             lambda ix, ids: _shard_pages(ix, queries, 0, min(depth, len(ids))))
    if not lists_s:
        return result
    sc, pos = merge_pages_host(lists_s, lists_p, depth)
    return _fill(result, qids, sc, pos, all_ids)


def retrieve_fused(args, group_of_query: Callable, topk: int, fuse: str = "max", index_factory: Optional[Callable] = None
                   ) -> Dict[Hashable, Dict[str, float]]:
    """One run per QUESTION over the same pickle shards, where a question is several queries (reformulations, the turns of a
    chat, sub-questions): the queries are grouped by `group_of_query(qid)` and every group gets the `topk` rows of the whole
    corpus of largest fused score — the max (`fuse="max"`, "any-of") or the min (`fuse="min"`, "all-of") of a row's scores
    over the group's queries (HipIndex.search_multi: exact).  -> {group: {docid: score}}, groups in the order their first
    query appears, a group's entries best first — score descending, then shard and row order; it goes to `save_as_trec` as it
    is.  A row's fused score depends on that row only, so the global top-k lies in the union of the shards' top-k: the corpus
    is taken shard by shard and the per-shard lists are merged on the host (merge_pages_host).  1 <= topk <= 1000, groups of
    at most 256 queries.

    Replicated form only, like retrieve_deep: every rank sees the whole corpus."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    topk = int(topk)
    order, lims, groups = group_rows([group_of_query(q) for q in qids])
    result: Dict[Hashable, Dict[str, float]] = {g: {} for g in groups}
    if len(groups) == 0 or topk <= 0:
        return result
    grouped = np.ascontiguousarray(np.asarray(queries, dtype=np.float32)[order])
    lists_s, lists_p, all_ids = _shard_lists(map(read_shard, corpus_parts), make_index, queries.shape[1], _device_index(args),
                                             lambda ix, ids: ix.search_multi(grouped, lims, topk, fuse))
    if not lists_s:
        return result
    sc, pos = merge_pages_host(lists_s, lists_p, topk)
    return _fill(result, groups, sc, pos, all_ids)


def retrieve_documents_fused(args, group_of_query: Callable, topk: int, doc_of: Callable[[str], str], fuse: str = "max",
                             label_of_doc: Optional[Callable[[str], object]] = None,
                             labels_of_group: Optional[Callable[[Hashable], Optional[set]]] = None,
                             index_factory: Optional[Callable] = None
                             ) -> Tuple[Dict[Hashable, Dict[str, float]], Dict[Hashable, Dict[str, List[str]]]]:
    """retrieve_fused with DOCUMENTS in the place of rows, over the same pickle shards: the queries are grouped into questions by
    `group_of_query(qid)`, the corpus rows are pages, `doc_of(page_id)` the document of a page.  Per sub-query a document scores
    as its best page does, and a question ranks the documents by the max (`fuse="max"`) or the min (`fuse="min"`) of that over its
    sub-queries — the sub-questions of a multi-hop question may be answered by different pages of one document
    (HipIndex.search_multi_groups: exact).  With `label_of_doc` and `labels_of_group` question g ranks only the documents whose
    label is in `labels_of_group(g)` (None = every document), one filter per distinct label set.
    -> ({group: {doc: score}}, {group: {doc: [page id per sub-query]}}): the `topk` best documents, best first, and for each the
    evidence — its best page for every sub-query of the question, in the order the question's queries appear; the first dict goes
    to `save_as_trec` as it is.  1 <= topk <= 1000, questions of at most 256 queries.

    Replicated form only: the shards go into one index reordered so that every document's pages are adjacent, as
    retrieve_documents_filtered builds it."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    topk = int(topk)
    q_order, lims, groups = group_rows([group_of_query(q) for q in qids])
    scores: Dict[Hashable, Dict[str, float]] = {g: {} for g in groups}
    pages: Dict[Hashable, Dict[str, List[str]]] = {g: {} for g in groups}
    reps, page_ids = _whole_corpus(corpus_parts)
    if not page_ids or len(groups) == 0 or topk <= 0:
        return scores, pages
    grouped = np.ascontiguousarray(np.asarray(queries, dtype=np.float32)[q_order])
    ix, order, docs, filter_of_group = _document_index(make_index, queries.shape[1], reps, page_ids, doc_of, _device_index(args),
                                                       groups, label_of_doc, labels_of_group)      # a lone label argument: no filter
    k = min(topk, len(docs))
    sc, _, dd, _, _, ev_r = ix.search_multi_groups(grouped, lims, k, fuse, filter_of_group, evidence=True)
    ix.close()
    for gi, g in enumerate(groups):
        a, b = int(lims[gi]), int(lims[gi + 1])
        ev = np.asarray(ev_r[k * a:k * b]).reshape(k, b - a)
        for slot, (s_, d) in enumerate(zip(sc[gi], dd[gi])):
            if d >= 0:
                scores[g][docs[int(d)]] = float(s_)
                pages[g][docs[int(d)]] = [page_ids[int(order[int(r)])] for r in ev[slot]]
    return scores, pages


def retrieve_rrf(args, group_of_query: Callable, topk: int, depth: int = 100, c: float = 60.0,
                 weight_of_query: Optional[Callable] = None, index_factory: Optional[Callable] = None,
                 fuse_lists: Optional[Callable] = None) -> Dict[Hashable, Dict[str, float]]:
    """One run per QUESTION by reciprocal-rank fusion over the same pickle shards: the queries are grouped by
    `group_of_query(qid)`, every query's list is its `depth` best rows of the WHOLE corpus, and a group gets the `topk` rows of
    largest sum of weight / (c + position) over its queries' lists, positions from 1 (HipIndex.search_rrf's definition:
    documents.rrf_runs).  `weight_of_query(qid)`: a float per query, None = 1.  -> {group: {docid: score}}, groups in the order
    their first query appears, a group's entries best first — score descending, then shard and row order; it goes to
    `save_as_trec` as it is.  A position is a property of the whole corpus, so per shard only `search(k=depth)` runs; every
    query's shard lists are merged into its global top `depth` on the host (merge_pages_host) and ONE `rrf_fuse` over those
    global positions fuses all groups.  1 <= topk, depth <= 1000, groups of at most 256 queries and rrf_max_entries() list slots.
    `fuse_lists(ids, lims, k, c, weights, device)` defaults to engine.rrf_fuse.

    Replicated form only, like retrieve_deep: every rank sees the whole corpus."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    topk, depth = int(topk), int(depth)
    order, lims, groups = group_rows([group_of_query(q) for q in qids])
    result: Dict[Hashable, Dict[str, float]] = {g: {} for g in groups}
    if len(groups) == 0 or topk <= 0:
        return result
    grouped = np.ascontiguousarray(np.asarray(queries, dtype=np.float32)[order])
    weights = None if weight_of_query is None else np.asarray([weight_of_query(qids[i]) for i in order], dtype=np.float32)
    dev = _device_index(args)
    lists_s, lists_p, all_ids = _shard_lists(map(read_shard, corpus_parts), make_index, queries.shape[1], dev,
                                             lambda ix, ids: ix.search(grouped, depth))
    if not lists_s:
        return result
    _, pos = merge_pages_host(lists_s, lists_p, depth)                # every query's global list, best first
    sc, ids, _ = (fuse_lists or rrf_fuse)(pos, lims, topk, c, weights, dev)
    return _fill(result, groups, np.asarray(sc), np.asarray(ids), all_ids)


def mine_negatives(args, positives_of_query, start: int, count: int, index_factory: Optional[Callable] = None
                   ) -> Dict[str, List[str]]:
    """Hard negatives for a trainer that takes one positive and a list of negatives per query (the reference's train_dataset):
    for every query the first `count` docids of the rank window that starts at rank `start` (skipping the top: "ranks 30-200
    minus the positives") which are not among its positives.  `positives_of_query`: {qid: [docid, ...]} or a callable qid ->
    docids.  The window taken is [start, start + count + the largest number of positives of a query), so that `count`
    negatives are left wherever the corpus has that many rows (a window wider than 1 000 rows is paged); -> {qid: [docid,
    ...]} in ranking order, fewer than `count` where the ranking ends.  Ranks are those of the whole corpus (retrieve_deep's
    order), over a single shard or several: the rows of ranks below start + count + positives of every shard are merged.

    Replicated form only, like retrieve_documents: every rank sees the whole corpus."""
    make_index = index_factory or HipIndex
    queries, qids, corpus_parts = _corpus(args)
    start, count = int(start), int(count)
    if start < 0 or count < 0:
        raise ValueError("start and count must be >= 0")
    get = positives_of_query if callable(positives_of_query) else (lambda q: positives_of_query.get(q, ()))
    positives = [list(dict.fromkeys(get(q))) for q in qids]
    width = count + max((len(p) for p in positives), default=0)
    shards = [s for s in map(read_shard, corpus_parts) if len(s[1])]
    if len(shards) == 1:                          # the window itself
        search = lambda ix, ids: _shard_pages(ix, queries, start, width)      # noqa: E731
    else:                                         # every row that can stand above the window's end
        search = lambda ix, ids: _shard_pages(ix, queries, 0, min(start + width, len(ids)))      # noqa: E731
    lists_s, lists_p, all_ids = _shard_lists(shards, make_index, queries.shape[1], _device_index(args), search)
    if not lists_s or width == 0:
        return {q: [] for q in qids}
    if len(shards) == 1:
        pos = lists_p[0]
    else:
        pos = merge_pages_host(lists_s, lists_p, start + width)[1][:, start:]
    row_of: Dict[str, int] = {}
    for r, d in enumerate(all_ids):
        row_of.setdefault(d, r)
    pos_rows = [[row_of[d] for d in p if d in row_of] for p in positives]
    neg = window_negatives(pos, pos_rows, count)
    return {q: [all_ids[int(j)] for j in neg[qi] if j >= 0] for qi, q in enumerate(qids)}


def _retrieve_corpus_sharded(args, topk: int, global_topk: bool, make_index: Callable, merge_keys: Optional[Callable]
                             ) -> Dict[str, Dict[str, float]]:
    """The corpus-sharded form (module docstring).  Row ids are global: files in sorted order (the order the
    replicated form walks them), a file's rows in place.  Exchange steps: one all_gather_object of the files' doc-id
    lists (control plane: strings), ONE all_gather_into_tensor of the packed keys (data path)."""
    dist = torch.distributed
    rank, world = dist.get_rank(), dist.get_world_size()
    queries, qids, mine = _load_queries(args, rank=None)                  # every rank searches all queries
    files = list_shards(args.output_dir, "corpus")
    if len(files) == 0:
        raise ValueError("No pre-computed document embeddings found")
    my_files = [p for p in files if _shard_rank(p) % world == rank]
    logger.info("corpus partitions of rank %d = %s", rank, my_files)
    dev = _device_index(args)
    on_gpu = make_index is HipIndex
    local = {os.path.basename(p): read_shard(p) for p in my_files}
    metas: List[Dict[str, List[str]]] = [None] * world
    dist.all_gather_object(metas, {name: list(ids) for name, (_, ids) in local.items()})
    doc_ids: Dict[str, List[str]] = {}
    for m in metas:
        doc_ids.update(m)
    offsets, table, off = {}, [], 0
    for p in files:                                                        # global ids: sorted file order
        name = os.path.basename(p)
        offsets[name] = off
        table.extend(doc_ids[name])
        off += len(doc_ids[name])
    dim, nq = queries.shape[1], queries.shape[0]
    q = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32))
    if on_gpu:
        q = q.to(f"cuda:{dev}")
    # slot f of the exchange buffer = the f-th file of the sorted list owned by this rank; ranks own different numbers
    # of files: pad with empty keys
    f_max = max(sum(1 for p in files if _shard_rank(p) % world == r) for r in range(world))
    keys = torch.zeros((f_max, nq, topk), dtype=torch.int64, device=q.device)
    for f, p in enumerate(my_files):
        reps, ids = local[os.path.basename(p)]
        if len(ids) == 0:
            continue
        ix = make_index(dim, len(ids), dev)
        ix.add(reps)
        keys[f] = ix.search_keys(q, topk, offsets[os.path.basename(p)])
        ix.close()
    gathered = exchange_keys(keys)                                         # [world, f_max, nq, k]: the one data-path collective
    result: Dict[str, Dict[str, float]] = {qid: {} for qid, m in zip(qids, mine) if m}
    if global_topk:
        sc, gid = (merge_keys or topk_merge_keys)(gathered.view(world * f_max, nq, topk))
        sc, gid = sc.cpu().numpy(), gid.cpu().numpy()
        for qi, qid in enumerate(qids):
            if mine[qi]:
                for s, j in zip(sc[qi], gid[qi]):
                    if j >= 0:
                        result[qid][table[int(j)]] = float(s)
        return result
    # the reference's union of the per-file top-k lists, files in sorted order like the replicated form
    sc, gid = unpack_keys_host(gathered.cpu().numpy())
    owners = [r for r in range(world)]
    slot_of = {}
    for r in owners:
        for f, p in enumerate([p for p in files if _shard_rank(p) % world == r]):
            slot_of[os.path.basename(p)] = (r, f)
    for p in files:
        r, f = slot_of[os.path.basename(p)]
        for qi, qid in enumerate(qids):
            if mine[qi]:
                for s, j in zip(sc[r, f, qi], gid[r, f, qi]):
                    if j >= 0:
                        result[qid][table[int(j)]] = float(s)
    return result


def exchange_keys(keys: torch.Tensor, group=None) -> torch.Tensor:
    """ONE all_gather_into_tensor of this rank's packed keys (same shape on every rank) -> [world, *keys.shape] on the
    keys' device.  RCCL over xGMI when the group's backend is nccl; a gloo group (CPU tests, two ranks sharing one
    GPU) exchanges on the host."""
    dist = torch.distributed
    world = dist.get_world_size(group)
    dev = keys.device
    mine = keys.contiguous()
    if mine.is_cuda and dist.get_backend(group) == "gloo":
        mine = mine.cpu()
    gathered = torch.empty((world * mine.shape[0],) + tuple(mine.shape[1:]), dtype=torch.int64, device=mine.device)
    dist.all_gather_into_tensor(gathered, mine, group=group)
    return gathered.to(dev).view((world,) + tuple(keys.shape))


def sharded_search(index, queries, k: int, id_offset: int = 0, group=None,
                   local_search_keys: Optional[Callable] = None, merge_keys: Optional[Callable] = None,
                   local_search: Optional[Callable] = None, merge: Optional[Callable] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Every rank holds `index` = its corpus shard (row j has global id id_offset + j) and the
    same `queries` [nq, dim] (a cuda tensor; a cpu tensor or numpy array is moved to the index's device).
    Returns the global (scores, ids) [nq, k] on every rank.

    A world of one rank (no process group, or a group of one) with the library's own calls is ONE call, `index.search`.
    Otherwise the data path is three library calls and one collective, no tensor arithmetic in between:
      1. `index.search_keys(queries, k, id_offset)` — the local fused search, whose merge kernel writes
         each result as ONE 64-bit word, orderable(score) << 32 | ~global_id (vr_index_search_keys);
      2. ONE `all_gather_into_tensor` of those [nq, k] words (80 KB per rank at nq = 1000, k = 10;
         RCCL over xGMI when the group's backend is nccl) — the only exchange step of the path;
      3. `vr_topk_merge_keys` over the gathered buffer as it is.
    `local_search_keys(queries, k, id_offset)` / `merge_keys(keys[world, nq, k])` default to those calls;
    the CPU (gloo) test injects the host statements below so that THIS function runs under world_size 2.
    (`local_search(queries, k) -> (scores, local ids)` / `merge(all_scores, all_ids)` are the round-2 names of the
    two hooks, still accepted: their results are converted through the host statements of the key format.)"""
    n_local = len(index) if index is not None else 0
    if id_offset < 0 or id_offset + n_local >= 2 ** 32 - 1:
        raise ValueError("global row ids must stay below 2^32 - 1 for the packed exchange")
    if local_search is not None and local_search_keys is None:
        warnings.warn("sharded_search(local_search=...) is deprecated: pass local_search_keys", DeprecationWarning, stacklevel=2)

        def local_search_keys(q_, k_, off_):
            s_, i_ = local_search(q_, k_)
            s_ = s_.cpu().numpy() if isinstance(s_, torch.Tensor) else s_
            i_ = i_.cpu().numpy() if isinstance(i_, torch.Tensor) else i_
            return pack_keys_host(s_, i_, off_)
    if merge is not None and merge_keys is None:
        warnings.warn("sharded_search(merge=...) is deprecated: pass merge_keys", DeprecationWarning, stacklevel=2)

        def merge_keys(keys_):
            s_, i_ = unpack_keys_host(keys_.cpu().numpy())
            return merge(torch.from_numpy(s_), torch.from_numpy(i_))
    if local_search_keys is None and index is not None and not (isinstance(queries, torch.Tensor) and queries.is_cuda):
        queries = torch.as_tensor(np.ascontiguousarray(queries, dtype=np.float32) if not isinstance(queries, torch.Tensor)
                                  else queries).to(f"cuda:{index.device}")      # host queries: the exchange buffer lives in HBM
    if local_search_keys is None and merge_keys is None and index is not None and not _collective_wanted(group):
        # a world of ONE rank with the library's own calls: nothing to exchange, so no exchange format either — the local search
        # writes (scores, ids) itself (one launch and two allocations less per search than pack -> merge of a single part)
        sc, ids = index.search(queries, k)
        if id_offset:
            ids += int(id_offset) * (ids >= 0)
        return sc, ids
    keys = (local_search_keys or index.search_keys)(queries, k, id_offset)
    if not isinstance(keys, torch.Tensor):
        keys = torch.from_numpy(np.ascontiguousarray(keys))
    merge_fn = merge_keys or topk_merge_keys
    if not _collective_wanted(group):
        return merge_fn(keys.view((1,) + tuple(keys.shape)))
    return merge_fn(exchange_keys(keys, group))                              # the one collective of the path


# ---- host statements of the exchange format (tests; the product path above never calls them) ----
def pack_keys_host(scores: np.ndarray, ids: np.ndarray, id_offset: int = 0) -> np.ndarray:
    """(fp32 score, local row id or -1) -> the packed key of include/visrag_hip.h as int64 bit patterns."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    ordr = np.where(u >> np.uint64(31), u ^ np.uint64(0xFFFFFFFF), u ^ np.uint64(0x80000000))
    gid = (np.asarray(ids, dtype=np.int64) + id_offset).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    keys = (ordr << np.uint64(32)) | (gid ^ np.uint64(0xFFFFFFFF))
    return np.where(np.asarray(ids) >= 0, keys, np.uint64(0)).view(np.int64)


def unpack_keys_host(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    k = np.ascontiguousarray(keys).view(np.uint64)
    o = (k >> np.uint64(32)).astype(np.uint32)
    u = np.where(o >> np.uint32(31), o ^ np.uint32(0x80000000), o ^ np.uint32(0xFFFFFFFF)).astype(np.uint32)
    sc = u.view(np.float32)
    ids = ((k & np.uint64(0xFFFFFFFF)) ^ np.uint64(0xFFFFFFFF)).astype(np.int64)
    none = k == 0
    return np.where(none, -np.inf, sc).astype(np.float32), np.where(none, -1, ids)


def merge_keys_host(keys: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """[world, nq, kk] packed keys -> (scores, global ids) [nq, k]: larger key first — the merge rule
    (score desc, id asc) is the integer order of the keys."""
    P, nq, kk = keys.shape
    u = np.transpose(np.ascontiguousarray(keys).view(np.uint64), (1, 0, 2)).reshape(nq, P * kk)
    order = np.argsort(~u, axis=1, kind="stable")[:, :k]
    return unpack_keys_host(np.take_along_axis(u, order, 1).view(np.int64))


def merge_topk_host(all_sc: np.ndarray, all_ids: np.ndarray, k: int):
    """Host-side statement of the merge rule (score desc, id asc) used by the gloo CPU tests."""
    P, nq, kk = all_sc.shape
    sc = np.transpose(all_sc, (1, 0, 2)).reshape(nq, P * kk)
    ids = np.transpose(all_ids, (1, 0, 2)).reshape(nq, P * kk)
    sc = np.where(ids >= 0, sc, -np.inf)
    order = np.lexsort((ids, -sc), axis=1)[:, :k]
    return np.take_along_axis(sc, order, 1), np.take_along_axis(ids, order, 1)


def pack_topk(scores: torch.Tensor, ids: torch.Tensor, id_offset: int = 0) -> torch.Tensor:
    """Deprecated name (round 2) of the exchange packing — the product path packs inside the search's merge kernel
    (HipIndex.search_keys).  Host statement of the CURRENT key format (include/visrag_hip.h), torch in / torch out."""
    warnings.warn("pack_topk is deprecated: HipIndex.search_keys emits packed keys", DeprecationWarning, stacklevel=2)
    return torch.from_numpy(pack_keys_host(scores.cpu().numpy(), ids.cpu().numpy(), id_offset)).to(scores.device)


def unpack_topk(packed: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Deprecated name (round 2): host statement of the key format's inverse (see unpack_keys_host)."""
    warnings.warn("unpack_topk is deprecated: vr_topk_merge_keys consumes packed keys", DeprecationWarning, stacklevel=2)
    s_, i_ = unpack_keys_host(packed.cpu().numpy())
    return torch.from_numpy(s_).to(packed.device), torch.from_numpy(i_).to(packed.device)
