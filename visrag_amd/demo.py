"""Drop-in for the demo pipeline of the reference (visrag_scripts/demo/visrag_pipeline/):

  * `encode(model, tokenizer, text_or_image_list)`            utils.py:12-32   (re-exported from modeling)
  * `add_pages(...)` / `add_pdfs(...)`  -> `reps.npy`, `index2img_filename.txt`, cached page PNGs
                                                               build_index.py:14-58
  * `retrieve(knowledge_base_path, query, topk, ...)` -> paths of the top-k page images
                                                               answer.py:14-40
    (`documents=[...]`: only the pages of those documents are ranked — HipIndex.search_filtered)
  * `retrieve_any(knowledge_base_path, questions, topk, ...)` -> the top-k pages for a question asked in several ways, by the
                                                               best ("any-of") or the worst ("all-of") of their scores
                                                               (HipIndex.search_multi; no reference counterpart)
  * `retrieve_documents_any(knowledge_base_path, questions, topk, ...)` -> the top-k DOCUMENTS for a question asked in several
                                                               parts, each part answered by the document's best page for it, and
                                                               with `return_evidence` those pages (HipIndex.search_multi_groups;
                                                               no reference counterpart)
  * `retrieve_documents(knowledge_base_path, query, topk, ...)` -> the best page of each of the top-k DOCUMENTS
                                                               (no reference counterpart: its top-k is pages)
    (`documents=[...]`: only those documents are ranked; `offset=n`: the next page of documents — HipIndex.search_groups_window)
  * `retrieve_above(knowledge_base_path, query, min_score, ...)` -> EVERY page at or above a score, best first
  * `retrieve_documents_above(knowledge_base_path, query, min_score, ...)` -> the best page of EVERY document at or above a
                                                               score, best document first (HipIndex.search_groups_range)
  * `duplicate_pages(knowledge_base_path, threshold, ...)` -> groups of near-duplicate pages
                                                               (HipIndex.search_range; no reference counterpart either)
  * `explain(knowledge_base_path, query, pages, ...)` -> the score and the rank of named pages for a question: "why was my page
                                                               not retrieved?" (HipIndex.rank_rows)
  * `remove_documents(knowledge_base_path, documents, ...)` / `update_pages(...)`: withdraw documents, re-embed pages — on disk
                                                               and in a resident index, in place (HipIndex.remove / update)

Same on-disk knowledge base (`reps.npy` float32 [n_pages, 2304], `index2img_filename.txt` one file name per
row, `<pdf>_<idx>.png`), so a base built by either side can be queried by the other.  Differences that do
not change results: pages are embedded in batches (the reference encodes one page per forward,
build_index.py:40-41) and the query x corpus matmul + topk (answer.py:31-33) runs on the HBM-resident
HipIndex.  The generation step of answer.py (MiniCPM-V-2.6 chat) is outside this path.
"""
from __future__ import annotations

import contextlib
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from .documents import doc_of_page, duplicate_groups, group_rows, label_filters, rows_of_documents
from .engine import HipIndex
from .modeling import encode  # noqa: F401  (demo/visrag_pipeline/utils.py:12-32)

# answer.py:27 (singular "document": the demo's own instruction string, kept verbatim)
QUERY_INSTRUCTION = "Represent this query for retrieving relevant document: "


@torch.no_grad()
def add_pages(model, tokenizer, pages: Sequence, knowledge_base_path: str, names: Optional[Sequence[str]] = None,
              batch_size: int = 32, save_images: bool = True, append: bool = False) -> np.ndarray:
    """Embed PIL page images into `knowledge_base_path` (build_index.py:37-55 without the PDF rasteriser).
    `names[i]` is the cache file name of page i (default `page_<i>.png`).  Returns the [n, D] float32 reps."""
    os.makedirs(knowledge_base_path, exist_ok=True)
    names = list(names) if names is not None else [f"page_{i}.png" for i in range(len(pages))]
    if len(names) != len(pages):
        raise ValueError("names and pages must have the same length")
    reps: List[np.ndarray] = []
    for lo in range(0, len(pages), batch_size):
        reps.append(encode(model, tokenizer, list(pages[lo:lo + batch_size])))
    out = np.concatenate(reps).astype(np.float32) if reps else np.zeros((0, model.cfg.hidden_size), np.float32)
    rp, ip = os.path.join(knowledge_base_path, "reps.npy"), os.path.join(knowledge_base_path, "index2img_filename.txt")
    if append and os.path.exists(rp):
        out = np.concatenate([np.load(rp), out])
        with open(ip) as f:
            names = [n for n in f.read().split("\n") if n] + names
    if save_images:
        for img, name in zip(pages, names[-len(pages):] if len(pages) else []):
            img.save(os.path.join(knowledge_base_path, name))
    np.save(rp, out)
    with open(ip, "w") as f:
        f.write("\n".join(names))
    return out


def add_pdfs(model, tokenizer, pdf_dir: str, knowledge_base_path: str, dpi: int = 200, batch_size: int = 32) -> np.ndarray:
    """build_index.py:14-58: rasterise every PDF under `pdf_dir` at 200 dpi (PyMuPDF, like the reference) and
    embed the pages.  PyMuPDF is an optional dependency of the demo, not of the library."""
    try:
        import fitz  # PyMuPDF
    except ImportError as e:  # pragma: no cover - not installed in the build image
        raise ImportError("add_pdfs needs PyMuPDF (`fitz`), as the reference demo does; "
                          "rasterise the pages yourself and call add_pages()") from e
    from PIL import Image
    pages, names = [], []
    for fn in sorted(f for f in os.listdir(pdf_dir) if f.endswith(".pdf")):
        doc = fitz.open(os.path.join(pdf_dir, fn))
        for idx, page in enumerate(doc):
            pix = page.get_pixmap(dpi=dpi)
            pages.append(Image.frombytes("RGB", [pix.width, pix.height], pix.samples))
            names.append(f"{fn}_{idx}.png")
    return add_pages(model, tokenizer, pages, knowledge_base_path, names, batch_size)


def load_knowledge_base(knowledge_base_path: str, device: Optional[int] = None):
    """-> (HipIndex holding reps.npy in HBM, list of image file names)."""
    with open(os.path.join(knowledge_base_path, "index2img_filename.txt")) as f:
        names = f.read().split("\n")
    reps = np.load(os.path.join(knowledge_base_path, "reps.npy")).astype(np.float32)
    from .modeling import default_device
    ix = HipIndex(reps.shape[1], max(len(reps), 1), default_device() if device is None else device)
    if len(reps):
        ix.add(reps)
    return ix, names


@contextlib.contextmanager
def _base(knowledge_base_path: str, index, names, model, documents: bool = False, groups: Optional[str] = None):
    """-> (index, names) for the length of one call.  `index is None`: the base on disk, loaded (`documents`: as a document base,
    load_document_base) and closed again however the call ends.  A caller's index stays open; `documents` and no groups set on
    it: they are set from the names — `groups="always"`: whenever it has none, `groups="rows"`: only if it holds rows, None:
    left to the caller — and rows that are not adjacent per document raise ValueError."""
    if index is None:
        load = load_document_base if documents else load_knowledge_base
        index, names = load(knowledge_base_path, model.encoder.device if model is not None else None)
        try:
            yield index, names
        finally:
            index.close()
        return
    if documents and groups and not index.n_groups and (groups == "always" or len(index)):
        order, offsets, _ = group_rows([doc_of_page(n) for n in names])
        if not np.array_equal(order, np.arange(len(order))):
            raise ValueError("the pages of a document are not adjacent in this index: load it with load_document_base()")
        index.set_groups(offsets)
    yield index, names


def _query_rows(query, model, tokenizer, dim: Optional[int] = None):
    """One question — a string, or its embedding ([dim] or [1, dim]) — -> [1, dim]; with `dim` SEVERAL questions — a list of
    strings, or their embeddings [m, dim] — -> contiguous float32 [m, dim].  Strings are encoded behind QUERY_INSTRUCTION."""
    if dim is None and isinstance(query, str):
        return encode(model, tokenizer, [QUERY_INSTRUCTION + query])
    if dim is not None and isinstance(query, (list, tuple)) and all(isinstance(x, str) for x in query):
        q = encode(model, tokenizer, [QUERY_INSTRUCTION + x for x in query])
    else:
        q = np.asarray(query.detach().cpu() if isinstance(query, torch.Tensor) else query, dtype=np.float32)
    return q.reshape(1, -1) if dim is None else np.ascontiguousarray(np.asarray(q, dtype=np.float32).reshape(-1, dim))


def _documents_mask(names, n: int, documents, strict: bool):
    """`documents` (None: no filter, -> None) -> the one filter of a question, bool [n]: the pages of those documents.  A name no
    page carries allows nothing; with `strict` (the document-level functions) it raises ValueError."""
    if documents is None:
        return None
    docs = [doc_of_page(nm) for nm in names[:n]]
    wanted = set(documents)
    unknown = sorted(wanted - set(docs)) if strict else []
    if unknown:
        raise ValueError(f"no page of the base belongs to {unknown[0]!r}" + (f" (and {len(unknown) - 1} more)" if len(unknown) > 1 else ""))
    return label_filters(docs, [wanted])


def _paths(knowledge_base_path: str, names, ids, scores):
    """one question's row ids and scores -> (paths of the taken slots (id >= 0), their scores)"""
    ids, scores = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (ids, scores))
    keep = [int(i) for i in ids if i >= 0]
    return [os.path.join(knowledge_base_path, names[i]) for i in keep], [float(s) for s in scores[: len(keep)]]


@torch.no_grad()
def retrieve(knowledge_base_path: str, query: str, topk: int, model, tokenizer, index=None, names=None,
             return_scores: bool = False, documents=None, diverse=None, pool=None, offset: int = 0):
    """answer.py:14-40: paths of the `topk` most similar page images (None if the base does not exist).
    Pass `index, names = load_knowledge_base(path)` to keep the index resident between questions.
    `documents`: an iterable of document names (the `doc_of_page` of the page names) — only their pages are ranked
    (HipIndex.search_filtered: the true top-k of those pages, however few they are); a name no page carries contributes
    nothing, and with no page allowed the result is [].  Works on a `load_knowledge_base` index and on a `load_document_base`
    one; `query` may then also be the query's embedding ([dim] or [1, dim]).
    `diverse`: a lambda in [0, 1] — the pages are picked by maximal marginal relevance from the `pool` best ones
    (HipIndex.search_diverse; `pool=None`: its default) and come in PICK order with their relevance scores, so near-duplicate
    pages do not fill the generator's context; with `documents` the pool holds only their pages.  `query` may be an embedding.
    `offset`: the "next page" of a result list — the pages at ranks offset .. offset + topk - 1 of the same ranking
    (HipIndex.search_window: exact however deep, page 101 costs what page 2 costs), also among the pages of `documents`;
    fewer than `topk` paths where the ranking ends.  Not together with `diverse`: ValueError."""
    if not os.path.exists(knowledge_base_path):
        return None
    if offset < 0:
        raise ValueError("offset must be >= 0")
    if offset > 0 and diverse is not None:
        raise ValueError("offset and diverse exclude each other: MMR picks have no ranks to page through")
    offset = int(offset)
    with _base(knowledge_base_path, index, names, model) as (index, names):
        n = len(index)
        if documents is None and diverse is None and offset == 0:         # the reference's call: a string, the plain search
            sc, ids = index.search(encode(model, tokenizer, [QUERY_INSTRUCTION + query]), min(topk, max(n, 1)))
            paths, scores = _paths(knowledge_base_path, names, ids[0], sc[0])
            return (paths, scores) if return_scores else paths
        q = _query_rows(query, model, tokenizer)
        mask = _documents_mask(names, n, documents, strict=False)        # one filter, set for this question (it replaces the index's)
        rows, f = (n, None) if mask is None else (int(mask.sum()), 0)
        paths, scores = [], []
        if topk > 0 and offset < rows:
            if mask is not None:
                index.set_filters(mask)
            if diverse is not None:                                       # MMR picks, in pick order
                k = min(topk, rows)
                sc, ids = index.search_diverse(q, k, None if pool is None else max(int(pool), k), float(diverse), f)
                paths, scores = _paths(knowledge_base_path, names, ids[0], sc[0])
            elif offset > 0:                                              # ranks [offset, offset + topk)
                for o in range(offset, min(offset + topk, rows), 1000):   # a list longer than one window: paged
                    sc, ids = index.search_window(q, o, min(1000, offset + topk - o, rows - o), f)
                    page = _paths(knowledge_base_path, names, ids[0], sc[0])
                    paths += page[0]
                    scores += page[1]
            else:
                sc, ids = index.search_filtered(q, min(topk, rows), 0)
                paths, scores = _paths(knowledge_base_path, names, ids[0], sc[0])
    return (paths, scores) if return_scores else paths


@torch.no_grad()
def retrieve_any(knowledge_base_path: str, questions, topk: int, model, tokenizer, index=None, names=None, fuse: str = "max",
                 documents=None, return_scores: bool = False):
    """Paths of the `topk` pages that serve a question asked in SEVERAL ways (None if the base does not exist): `questions` is
    a list of strings — reformulations, the last turns of a chat, the sub-questions of a multi-hop question — or their
    embeddings [m, dim].  `fuse="max"` ("any-of") scores a page as its best question does, `fuse="min"` ("all-of") as its worst
    does, so a page has to serve every part (HipIndex.search_multi: the exact top-k of the fused score, no duplicates to
    collapse, never fewer than `topk` pages while the base has them).  `documents`: only the pages of those documents, as in
    `retrieve` (one filter, set for this question).  With `return_scores` -> (paths, scores, deciding): `deciding[i]` is the
    index into `questions` of the question whose score is page i's fused score.  Pass `index, names = load_knowledge_base(path)`
    to keep the index resident."""
    if not os.path.exists(knowledge_base_path):
        return None
    with _base(knowledge_base_path, index, names, model) as (index, names):
        n = len(index)
        q = _query_rows(questions, model, tokenizer, index.dim)
        mask = _documents_mask(names, n, documents, strict=False)
        k = min(topk, n if mask is None else int(mask.sum()), 1000)
        paths, scores, deciding = [], [], []
        if k > 0 and len(q) > 0:
            if mask is not None:
                index.set_filters(mask)
            sc, ids, which = index.search_multi(q, [0, len(q)], k, fuse, None if mask is None else 0)
            paths, scores = _paths(knowledge_base_path, names, ids[0], sc[0])
            deciding = [int(w) for w in which[0][: len(paths)]]
    return (paths, scores, deciding) if return_scores else paths


@torch.no_grad()
def retrieve_rrf(knowledge_base_path: str, questions, topk: int, model, tokenizer, index=None, names=None, depth: int = 100,
                 c: float = 60.0, weights=None, documents=None, return_scores: bool = False):
    """Paths of the `topk` pages that serve a question asked in SEVERAL ways, by reciprocal-rank fusion (None if the base does
    not exist): every question's `depth` best pages form a list, and a page scores the sum of weight / (c + position) over the
    lists that hold it, positions from 1 (HipIndex.search_rrf) — positions only, so a reformulation with a flat score profile
    counts as much as one with a peaked profile.  `questions` as in `retrieve_any`: strings or their embeddings [m, dim];
    `weights`: one float per question, None = 1.  `documents`: only the pages of those documents, as in `retrieve` (one
    filter, set for this question).  Fewer than `topk` paths where the lists hold fewer distinct pages.  With `return_scores`
    -> (paths, scores, hits): `hits[i]` is the number of lists page i stands in.  Pass `index, names =
    load_knowledge_base(path)` to keep the index resident."""
    if not os.path.exists(knowledge_base_path):
        return None
    with _base(knowledge_base_path, index, names, model) as (index, names):
        n = len(index)
        q = _query_rows(questions, model, tokenizer, index.dim)
        mask = _documents_mask(names, n, documents, strict=False)
        k = min(topk, n if mask is None else int(mask.sum()), 1000)
        paths, scores, hits = [], [], []
        if k > 0 and len(q) > 0:
            if mask is not None:
                index.set_filters(mask)
            sc, ids, h = index.search_rrf(q, [0, len(q)], k, depth, c, weights, None if mask is None else 0)
            paths, scores = _paths(knowledge_base_path, names, ids[0], sc[0])
            hits = [int(x) for x in h[0][: len(paths)]]
    return (paths, scores, hits) if return_scores else paths


def load_document_base(knowledge_base_path: str, device: Optional[int] = None):
    """-> (HipIndex holding reps.npy with every document's pages adjacent and the documents set as its groups, the image file
    names in the index's row order).  The document of a page is `doc_of_page(name)`; a base whose pages are not contiguous per
    document is reordered on load (documents in the order of their first page, pages in their order), and because the names
    are reordered with the rows, `names[row id]` is the page whatever the order on disk."""
    with open(os.path.join(knowledge_base_path, "index2img_filename.txt")) as f:
        names = [n for n in f.read().split("\n") if n]
    reps = np.load(os.path.join(knowledge_base_path, "reps.npy")).astype(np.float32)
    if len(names) != len(reps):
        raise ValueError(f"{len(reps)} rows but {len(names)} page names in {knowledge_base_path}")
    order, offsets, _ = group_rows([doc_of_page(n) for n in names])
    from .modeling import default_device
    ix = HipIndex(reps.shape[1], max(len(reps), 1), default_device() if device is None else device)
    if len(reps):
        ix.add(reps[order])
        ix.set_groups(offsets)
    return ix, [names[i] for i in order]


@torch.no_grad()
def retrieve_documents(knowledge_base_path: str, query, topk: int, model, tokenizer, index=None, names=None,
                       return_scores: bool = False, documents=None, offset: int = 0):
    """Paths of the best page of each of the `topk` most similar DOCUMENTS, best document first (None if the base does not
    exist): a document scores as its best page does, so ten results are ten documents, not ten pages of one.  Documents are
    the `doc_of_page` of the page names.  Pass `index, names = load_document_base(path)` to keep the index resident between
    questions; an index of your own must hold every document's pages adjacently, `names` in its row order.  `query` is the
    question, or its embedding ([dim] or [1, dim]) if it has been encoded already.
    `documents`: an iterable of document names — only those documents are ranked, each by its best page (one filter, set for this
    question as in `retrieve`; HipIndex.search_groups_window); a name no page carries raises ValueError.  `offset`: the "next
    page" of the document list — the documents at ranks offset .. offset + topk - 1 of the same ranking, exact however deep;
    fewer than `topk` paths where the ranking ends.  With both at their defaults the call is HipIndex.search_groups."""
    if not os.path.exists(knowledge_base_path):
        return None
    if offset < 0:
        raise ValueError("offset must be >= 0")
    with _base(knowledge_base_path, index, names, model, documents=True, groups="always") as (index, names):
        q = _query_rows(query, model, tokenizer)
        if documents is not None or offset > 0:
            paths, scores = _document_window(knowledge_base_path, q, topk, index, names, documents, int(offset))
        elif len(index) == 0:
            paths, scores = [], []
        else:
            sc, ids, _ = index.search_groups(q, max(1, min(topk, index.n_groups)))
            paths, scores = _paths(knowledge_base_path, names, ids[0][:topk], sc[0])
    return (paths, scores) if return_scores else paths


@torch.no_grad()
def retrieve_documents_any(knowledge_base_path: str, questions, topk: int, model, tokenizer, index=None, names=None,
                           fuse: str = "max", documents=None, return_evidence: bool = False):
    """Paths of the deciding page of each of the `topk` DOCUMENTS that serve a question asked in several parts (None if the base
    does not exist): `questions` as in `retrieve_any` — strings or their embeddings [m, dim] — form one group.  Per question a
    document scores as its best page does; `fuse="max"` ("any-of") ranks it by its best question, `fuse="min"` ("all-of") by its
    worst, so the sub-questions of a multi-hop question may be answered by DIFFERENT pages of the document
    (HipIndex.search_multi_groups: exact).  The index is a document base (`load_document_base`), as in `retrieve_documents`.
    `documents`: only those documents are ranked (one filter, set for this question); a name no page carries raises ValueError.
    With `return_evidence` -> (paths, scores, evidence): `evidence[i]` lists, for document i and every question in order, (path of
    the document's best page for that question, its score) — the pages to hand to the generator."""
    if not os.path.exists(knowledge_base_path):
        return None
    with _base(knowledge_base_path, index, names, model, documents=True, groups="always") as (index, names):
        n = len(index)
        q = _query_rows(questions, model, tokenizer, index.dim)
        wanted = None if documents is None else set(documents)
        mask = _documents_mask(names, n, wanted, strict=True)
        present = (int(index.n_groups) if n else 0) if mask is None else len(wanted)
        k = min(topk, present, 1000)
        paths, scores, evidence = [], [], []
        if k > 0 and len(q) > 0:
            if mask is not None:
                index.set_filters(mask)
            sc, rows, _, _, ev_s, ev_r = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in
                                          index.search_multi_groups(q, [0, len(q)], k, fuse, None if mask is None else 0, evidence=True))
            paths, scores = _paths(knowledge_base_path, names, rows[0], sc[0])
            ev_s, ev_r = ev_s.reshape(k, len(q)), ev_r.reshape(k, len(q))
            evidence = [[(os.path.join(knowledge_base_path, names[int(r)]), float(s)) for r, s in zip(ev_r[i], ev_s[i])] for i in range(len(paths))]
    return (paths, scores, evidence) if return_evidence else paths


def _document_window(knowledge_base_path, q, topk, index, names, documents, offset):
    """retrieve_documents() at ranks [offset, offset + topk); `documents` given: among them, through one filter set for this question"""
    n = len(index)
    wanted = None if documents is None else set(documents)
    mask = _documents_mask(names, n, wanted, strict=True)
    present = (int(index.n_groups) if n else 0) if mask is None else len(wanted)
    paths, scores = [], []
    if topk > 0 and offset < present:
        if mask is not None:
            index.set_filters(mask)
        for o in range(offset, min(offset + topk, present), 1000):        # a list longer than one window: paged
            sc, ids, _ = index.search_groups_window(q, o, min(1000, offset + topk - o, present - o), None if mask is None else 0)
            page = _paths(knowledge_base_path, names, ids[0], sc[0])
            paths += page[0]
            scores += page[1]
    return paths, scores


@torch.no_grad()
def retrieve_above(knowledge_base_path: str, query, min_score: float, model, tokenizer, index=None, names=None, documents=None,
                   max_pages: Optional[int] = None, return_scores: bool = False):
    """Paths of EVERY page whose score is at least `min_score`, best first (None if the base does not exist): the similarity
    threshold of a RAG stack — a question with one relevant page gets one page, and a family of a thousand near-duplicates comes
    back whole (HipIndex.search_range: the exact fp32 answer, no cap at a k).  `documents`: only the pages of those documents,
    as in `retrieve` (one filter, set for this question).  `max_pages`, if given, cuts the sorted result.  `query` is the
    question, or its embedding ([dim] or [1, dim]).  Pass `index, names = load_knowledge_base(path)` to keep the index resident."""
    if not os.path.exists(knowledge_base_path):
        return None
    with _base(knowledge_base_path, index, names, model) as (index, names):
        n = len(index)
        q = _query_rows(query, model, tokenizer)
        mask = _documents_mask(names, n, documents, strict=False)
        paths, scores = [], []
        if n and (mask is None or mask.any()) and (max_pages is None or max_pages > 0):
            if mask is not None:
                index.set_filters(mask)
            _, sc, ids = index.search_range(q, float(min_score), None if mask is None else 0)
            paths, scores = _paths(knowledge_base_path, names, ids[:max_pages], sc[:max_pages])
    return (paths, scores) if return_scores else paths


@torch.no_grad()
def retrieve_documents_above(knowledge_base_path: str, query, min_score: float, model, tokenizer, index=None, names=None,
                             documents=None, max_documents: Optional[int] = None, return_scores: bool = False):
    """Paths of the best page of EVERY document whose score is at least `min_score`, best document first (None if the base does
    not exist): `retrieve_above` one level up — a document scores as its best page does, so a relevant 300-page report is one
    entry, and an irrelevant one is none (HipIndex.search_groups_range: the exact fp32 answer, no cap at a k).  Documents are the
    `doc_of_page` of the page names; pass `index, names = load_document_base(path)` to keep the index resident, as in
    `retrieve_documents`.  `documents`: only those documents, each by its best page (one filter, set for this question); a name
    no page carries raises ValueError.  `max_documents`, if given, cuts the sorted result.  `query` is the question, or its
    embedding ([dim] or [1, dim])."""
    if not os.path.exists(knowledge_base_path):
        return None
    with _base(knowledge_base_path, index, names, model, documents=True, groups="rows") as (index, names):
        n = len(index)
        q = _query_rows(query, model, tokenizer)
        mask = _documents_mask(names, n, documents, strict=True)
        paths, scores = [], []
        if n and (mask is None or mask.any()) and (max_documents is None or max_documents > 0):
            if mask is not None:
                index.set_filters(mask)
            _, sc, rows, _ = index.search_groups_range(q, float(min_score), None if mask is None else 0)
            paths, scores = _paths(knowledge_base_path, names, rows[:max_documents], sc[:max_documents])
    return (paths, scores) if return_scores else paths


@torch.no_grad()
def explain(knowledge_base_path: str, query, pages, documents=None, index=None, names=None, model=None, tokenizer=None):
    """Where named pages stand for a question: -> [(score, rank)] for the page names `pages` (one name: one pair; None if the base
    does not exist).  `score` is the page's fp32 score as `retrieve` reports it, `rank` its position in the ranking of ALL
    pages (0 = the best; HipIndex.rank_rows: exact, however deep) — `retrieve(topk)` returns the page iff rank < topk.  With
    `documents=[...]` the rank is among the pages of those documents, as `retrieve(documents=...)` ranks them (one filter, set
    for this question); for a page outside them it is the position the page would take.  A name the base does not hold raises
    ValueError.  `query` is the question (`model`, `tokenizer` encode it) or its embedding ([dim] or [1, dim]).  Pass `index,
    names = load_knowledge_base(path)` to keep the index resident."""
    if not os.path.exists(knowledge_base_path):
        return None
    with _base(knowledge_base_path, index, names, model) as (index, names):
        n = len(index)
        one = isinstance(pages, str)
        wanted = [pages] if one else list(pages)
        row_of = {nm: i for i, nm in enumerate(names[:n])}
        missing = [nm for nm in wanted if nm not in row_of]
        if missing:
            raise ValueError(f"no such page in {knowledge_base_path}: {missing[0]}")
        q = _query_rows(query, model, tokenizer)
        if not wanted:
            return []
        foq = None
        if documents is not None:
            index.set_filters(_documents_mask(names, n, documents, strict=False))
            foq = 0
        sc, rk = index.rank_rows(q, np.asarray([[row_of[nm] for nm in wanted]], dtype=np.int64), filter_of_query=foq)
        out = [(float(s), int(r)) for s, r in zip(sc[0], rk[0])]
        return out[0] if one else out


@torch.no_grad()
def explain_documents(knowledge_base_path: str, query, wanted, documents=None, index=None, names=None, model=None, tokenizer=None):
    """Where named DOCUMENTS stand for a question: -> [(score, best page name, rank)] for the document names `wanted` (one name:
    one triple; None if the base does not exist).  The ranking is `retrieve_documents`': a document scores as its best page
    does, `rank` is its position among the documents (0 = the best; HipIndex.rank_groups: exact, however deep) —
    `retrieve_documents(topk)` returns the document iff rank < topk, through the same page.  With `documents=[...]` the rank is
    among those documents, as `retrieve_documents(documents=...)` ranks them (one filter, set for this question); a wanted
    document outside them is not in that ranking and gives (-inf, None, -1).  A name no page belongs to raises ValueError.
    `query` is the question (`model`, `tokenizer` encode it) or its embedding ([dim] or [1, dim]).  Pass `index, names =
    load_document_base(path)` to keep the index resident; an index of your own must hold every document's pages adjacently."""
    if not os.path.exists(knowledge_base_path):
        return None
    with _base(knowledge_base_path, index, names, model, documents=True) as (index, names):
        n = len(index)
        one = isinstance(wanted, str)
        want = [wanted] if one else list(wanted)
        docs = [doc_of_page(nm) for nm in names[:n]]
        order, offsets, doc_names = group_rows(docs)
        if not np.array_equal(order, np.arange(len(order))):
            raise ValueError("the pages of a document are not adjacent in this index: load it with load_document_base()")
        group_of = {d: g for g, d in enumerate(doc_names)}
        unknown = [d for d in list(want) + list(documents or ()) if d not in group_of]
        if unknown:
            raise ValueError(f"no page of the base belongs to {unknown[0]!r}")
        if not index.n_groups and n:                                      # after the names are known to be the base's
            index.set_groups(offsets)
        q = _query_rows(query, model, tokenizer)
        if not want:
            return []
        foq = None
        if documents is not None:
            index.set_filters(label_filters(docs, [set(documents)]))
            foq = 0
        sc, rows, rk = index.rank_groups(q, np.asarray([[group_of[d] for d in want]], dtype=np.int64), filter_of_query=foq)
        sc, rows, rk = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (sc, rows, rk))
        out = [(float(s), names[int(r)] if r >= 0 else None, int(k)) for s, r, k in zip(sc[0], rows[0], rk[0])]
        return out[0] if one else out


def duplicate_pages(knowledge_base_path: str, threshold: float, index=None, names=None, batch: int = 256) -> Optional[List[List[str]]]:
    """Groups of page names whose embeddings are chained by a dot product >= `threshold` (None if the base does not exist): the
    near-duplicate pages of a knowledge base, found before they reach the generator.  The base's own rows are the queries of a
    range search, `batch` of them per call; page a and page c land in one group when a-b and b-c match, even if a-c does not.
    Groups come ordered by their first page, pages in row order; a page that matches only itself is in no group.  An index
    passed in must hold the rows of reps.npy in their order on disk (`load_knowledge_base`)."""
    if not os.path.exists(knowledge_base_path):
        return None
    with _base(knowledge_base_path, index, names, None) as (index, names):
        n_disk = len(np.load(os.path.join(knowledge_base_path, "reps.npy"), mmap_mode="r"))
        n = len(index)
        if n_disk != n:
            raise ValueError(f"{n_disk} rows in {knowledge_base_path} but {n} in the index")
        lims, ids = [np.zeros(1, np.int64)], []
        batch = max(int(batch), 1)
        for lo in range(0, n, batch):              # the queries are the index's own fp32 rows, read back: no host copy of the base
            l, _, i = index.search_range(index.rows(np.arange(lo, min(lo + batch, n))), float(threshold), sort=False)
            lims.append(l[1:] + lims[-1][-1])
            ids.append(i)
    groups = duplicate_groups(np.concatenate(lims), np.concatenate(ids) if ids else np.zeros(0, np.int64), n)
    return [[names[r] for r in g] for g in groups]


def _read_names(knowledge_base_path: str) -> List[str]:
    with open(os.path.join(knowledge_base_path, "index2img_filename.txt")) as f:
        return [n for n in f.read().split("\n") if n]


def _write_base(knowledge_base_path: str, reps: np.ndarray, names: Sequence[str]) -> None:
    np.save(os.path.join(knowledge_base_path, "reps.npy"), reps)
    with open(os.path.join(knowledge_base_path, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))


def remove_documents(knowledge_base_path: str, documents, index=None, names=None, delete_images: bool = True) -> Optional[List[str]]:
    """Withdraw the documents `documents` (the `doc_of_page` of the page names) from the base: their rows leave `reps.npy` and
    `index2img_filename.txt`, and with `delete_images` their cached PNGs are deleted — files inside the base directory only.
    With a resident `index` / `names` (`load_knowledge_base`, rows in the order on disk) the rows are removed from the index in
    place (HipIndex.remove: no rebuild, no upload) and `names` is edited in place, so the next `retrieve(..., index=, names=)`
    sees the edited base; a grouping is dropped with the rows (`retrieve_documents` sets it again).  -> the removed file names
    (None if the base does not exist); a document no page belongs to removes nothing."""
    if not os.path.exists(knowledge_base_path):
        return None
    disk_names = _read_names(knowledge_base_path)
    if names is not None and [n for n in names if n] != disk_names:
        raise ValueError("`names` is not the page list of the base on disk: withdraw documents from an index in the disk's row order")
    ids = rows_of_documents(disk_names, documents)
    gone = [disk_names[i] for i in ids]
    if not len(ids):
        return gone
    keep = np.ones(len(disk_names), dtype=bool)
    keep[ids] = False
    reps = np.load(os.path.join(knowledge_base_path, "reps.npy"))
    if len(reps) != len(disk_names):
        raise ValueError(f"{len(reps)} rows but {len(disk_names)} page names in {knowledge_base_path}")
    left = [n for n, k in zip(disk_names, keep) if k]
    _write_base(knowledge_base_path, np.ascontiguousarray(reps[keep]), left)
    if index is not None:
        index.remove(ids)
    if names is not None:
        names[:] = left
    if delete_images:
        base = os.path.realpath(knowledge_base_path)
        for nm in gone:
            path = os.path.realpath(os.path.join(base, nm))
            if os.path.dirname(path) == base and os.path.isfile(path):
                os.remove(path)
    return gone


@torch.no_grad()
def update_pages(model, tokenizer, pages: Sequence, knowledge_base_path: str, names: Sequence[str], index=None,
                 batch_size: int = 32) -> np.ndarray:
    """Re-embed pages that are in the base already (a re-scanned page): `names[i]` is the file name of PIL image `pages[i]`.
    Their rows are replaced in `reps.npy` and, with a resident `index` (rows in the order on disk), overwritten in place
    (HipIndex.update); their PNGs are overwritten.  A name the base does not hold, or one given twice, raises ValueError
    before anything changes.  -> the new [n, D] float32 reps."""
    names = list(names)
    if len(names) != len(pages):
        raise ValueError("names and pages must have the same length")
    disk_names = _read_names(knowledge_base_path)
    row_of = {n: i for i, n in enumerate(disk_names)}
    unknown = [n for n in names if n not in row_of]
    if unknown:
        raise ValueError(f"not in the knowledge base: {unknown[:5]}")
    if len(set(names)) != len(names):
        raise ValueError("a page is named more than once")
    reps = np.load(os.path.join(knowledge_base_path, "reps.npy")).astype(np.float32)
    if not names:
        return np.zeros((0, reps.shape[1]), np.float32)
    new = np.concatenate([encode(model, tokenizer, list(pages[lo:lo + batch_size]))
                          for lo in range(0, len(pages), batch_size)]).astype(np.float32)
    ids = np.asarray([row_of[n] for n in names], dtype=np.int64)
    reps[ids] = new
    _write_base(knowledge_base_path, reps, disk_names)
    if index is not None:
        index.update(ids, new)
    for img, nm in zip(pages, names):
        img.save(os.path.join(knowledge_base_path, nm))
    return new
