"""The numpy reference of the document window search (tests/group_window_search_ref.py) on hand-worked cases, the number of fp64
intervals wider than one position on the corpora of tests/test_gpu_group_window_search.py, the host helpers (documents.
collection_filters, demo.retrieve_documents with `documents` / `offset`, retriever.retrieve_documents_filtered over a host stand-in
for the index) and the declarations of the two ABI symbols.  No GPU, no library."""
import os
import types

import numpy as np
import pytest

from tests import group_search_ref as R
from tests import group_window_search_ref as G
from visrag_amd import demo, retriever
from visrag_amd.documents import collection_filters, group_filter, label_filters
from visrag_amd.utils import write_shard

# one query, nine pages in four documents
#   document 0 = rows 0-2 (.5, .75, .75)   document 1 = row 3 (.25)   document 2 = rows 4-6 (.75, .9, .1)   document 3 = rows 7-8 (.75, .2)
S = np.array([[0.5, 0.75, 0.75, 0.25, 0.75, 0.9, 0.1, 0.75, 0.2]])
OFF = np.array([0, 3, 4, 7, 9])


def _ref(mask, o, k):
    sc, ids, gr = G.group_window_ref(S, OFF, None if mask is None else np.asarray(mask, dtype=bool), o, k)
    return sc[0].tolist(), ids[0].tolist(), gr[0].tolist()


def test_no_mask_is_the_grouped_ranking_with_a_window():
    assert _ref(None, 0, 4) == ([0.9, 0.75, 0.75, 0.25], [5, 1, 7, 3], [2, 0, 3, 1])
    assert _ref(None, 1, 2) == ([0.75, 0.75], [1, 7], [0, 3])
    assert _ref(None, 3, 3) == ([0.25, -np.inf, -np.inf], [3, -1, -1], [1, -1, -1])
    # offset 0 without a mask is the grouped search's reference, tails included
    C_, Q = R.unit(60, 16, 1), R.unit(3, 16, 2)
    off = R.random_offsets(60, 4)
    for k in (5, len(off) + 2):
        for a, b in zip(G.group_window_ref(R.scores64(Q, C_), off, None, 0, k), R.group_topk_ref(Q, C_, off, k)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_a_document_with_no_allowed_page_is_absent():
    mask = [1, 1, 1, 0, 1, 1, 1, 1, 1]                                    # document 1 has no allowed page
    assert _ref(mask, 0, 4) == ([0.9, 0.75, 0.75, -np.inf], [5, 1, 7, -1], [2, 0, 3, -1])
    assert _ref(np.zeros(9), 0, 2) == ([-np.inf, -np.inf], [-1, -1], [-1, -1])
    E, best, present = G.present_best(S, OFF, np.asarray(mask, dtype=bool))
    assert present[0].tolist() == [True, False, True, True] and best[0].tolist() == [1, -1, 5, 7] and np.isneginf(E[0, 1])


def test_the_best_row_is_the_lowest_allowed_tied_row_and_a_forbidden_best_page_lowers_the_document():
    mask = [1, 0, 1, 1, 1, 0, 1, 1, 1]                                    # row 1 (tied best of document 0) and row 5 (best of 2) forbidden
    # document 0 keeps .75 through row 2; document 2 drops to .75 (row 4): three documents tie, in group order
    assert _ref(mask, 0, 4) == ([0.75, 0.75, 0.75, 0.25], [2, 4, 7, 3], [0, 2, 3, 1])
    mask = [1, 1, 1, 1, 0, 0, 1, 1, 1]                                    # document 2 drops to .1: last, and the order changes
    assert _ref(mask, 0, 4) == ([0.75, 0.75, 0.25, 0.1], [1, 7, 3, 6], [0, 3, 1, 2])


def test_both_window_edges_inside_one_tie_tier_of_documents():
    s = np.full((1, 12), 0.5)
    s[0, 0] = 0.9; s[0, 11] = 0.1                                         # six documents of two rows: one above, four tied, one below
    off = np.arange(0, 13, 2)
    sc, ids, gr = G.group_window_ref(s, off, None, 2, 2)
    assert gr[0].tolist() == [2, 3] and ids[0].tolist() == [4, 6] and sc[0].tolist() == [0.5, 0.5]
    assert G.group_window_ref(s, off, None, 1, 5)[2][0].tolist() == [1, 2, 3, 4, 5]
    mask = np.ones(12, dtype=bool); mask[4] = False                       # the tied document 2 answers with its other row
    assert G.group_window_ref(s, off, mask, 2, 2)[1][0].tolist() == [5, 6]


def test_an_offset_past_the_present_documents_gives_tails_and_offsets_may_differ_per_query():
    assert _ref(None, 4, 2) == ([-np.inf, -np.inf], [-1, -1], [-1, -1])
    assert _ref(None, 1 << 40, 1) == ([-np.inf], [-1], [-1])
    mask = [1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert _ref(mask, 3, 1) == ([-np.inf], [-1], [-1])
    two = np.concatenate([S, S])
    gr = G.group_window_ref(two, OFF, np.stack([np.ones(9, dtype=bool), np.asarray(mask, dtype=bool)]), [3, 2], 2)[2]
    assert gr.tolist() == [[1, -1], [3, -1]]


def test_fp32_scores_rank_on_their_orderable_bits():
    s32 = S.astype(np.float32)
    a, b = G.group_window_ref(s32, OFF, None, 0, 4), G.group_window_ref(S, OFF, None, 0, 4)
    assert a[0].dtype == np.float32 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert G.ordered(np.array([-0.0, 0.0, -1.0, 1.0], dtype=np.float32)).argsort().tolist() == [2, 0, 1, 3]


def test_check_docs_accepts_a_near_tie_swap_and_nothing_else():
    s = np.array([0.9, 0.1, 0.5, 0.2, 0.5 + 4e-7, 0.0, 0.3, 0.1])       # four documents of two rows: .9, .5, .5 + 4e-7, .3
    off = np.arange(0, 9, 2)
    f32 = lambda *x: np.asarray(x, dtype=np.float32)                     # noqa: E731
    assert G.check_docs(s, off, None, f32(.5, .5, .3), [4, 2, 6], [2, 1, 3], 1)[1:] == (0, pytest.approx(4e-7, abs=1e-7), None)
    assert G.check_docs(s, off, None, f32(.5, .5, .3), [2, 4, 6], [1, 2, 3], 1)[1::2] == (2, None)      # 4e-7 apart: may trade places
    assert G.check_docs(s, off, None, f32(.5, .3, .5), [4, 6, 2], [2, 3, 1], 1)[3] is not None          # ... 0.2 apart: may not
    assert G.check_docs(s, off, None, f32(.5, .5, .3), [4, 3, 6], [2, 1, 3], 1)[3] is not None          # a best row that is not the best
    assert G.check_docs(s, off, None, f32(.5, .5001, .3), [4, 2, 6], [2, 1, 3], 1)[3] is not None       # a score 1e-4 off
    with pytest.raises(AssertionError):
        G.check_docs(s, off, None, f32(.3, -np.inf), [6, -1], [3, -1], 2)                               # a window that ends early


@pytest.mark.parametrize("name", list(G.TABLE))
def test_widened_intervals_of_the_reference_windows(name):
    """the 6e-7 table of the GPU test: (entries, intervals wider than one position) per (offset, filter) at k = 100"""
    C, Q, off, S_ = G.case(name)
    for o, density, want in G.TABLE[name]:
        assert G.widened(S_, off, G.case_mask(name, density), o, G.K_FP64) == want, (o, density)
    assert len(R.random_offsets(5000, 7)) - 1 == 723


# ------------------------------------------------------------------------------------------------ host helpers ---
def test_collection_filters():
    off = [0, 3, 4, 7, 9]
    coll = ["a", "b", "a", "c"]
    m = collection_filters(off, coll, [{"a"}, None, {"c", "b"}, {"zzz"}, set()])
    assert m.dtype == np.bool_ and m.shape == (5, 9)
    assert m[0].tolist() == [1, 1, 1, 0, 1, 1, 1, 0, 0] and m[1].all() and m[2].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 1]
    assert not m[3].any() and not m[4].any()
    assert np.array_equal(m[0], group_filter(off, [0, 2]))
    # a label per document is label_filters with that label on each of its rows
    per_row = np.repeat(coll, np.diff(off))
    assert np.array_equal(m[:3], label_filters(list(per_row), [{"a"}, None, {"c", "b"}]))
    with pytest.raises(ValueError):
        collection_filters(off, coll[:3], [None])


class HostIndex:
    """stands in for HipIndex: the reference's ranking rule over fp32-rounded fp64 scores, on the host"""
    calls = []

    def __init__(self, dim, capacity, device=0):
        self.dim = dim
        self.C = np.zeros((0, dim), dtype=np.float32)
        self.n_groups = self.n_filters = 0

    def add(self, reps):
        self.C = np.concatenate([self.C, np.asarray(reps, dtype=np.float32)])
        self.n_groups = self.n_filters = 0

    def __len__(self):
        return len(self.C)

    def set_groups(self, offsets):
        self.off = np.asarray(offsets, dtype=np.int64)
        assert self.off[0] == 0 and self.off[-1] == len(self.C) and (np.diff(self.off) > 0).all()
        self.n_groups = len(self.off) - 1

    def set_filters(self, masks):
        self.masks = np.atleast_2d(np.asarray(masks, dtype=bool))
        assert self.masks.shape[1] == len(self.C)
        self.n_filters = len(self.masks)

    def search_groups_window(self, Q, offset, k, filter_of_query=None):
        assert 1 <= k <= 1000 and self.n_groups
        HostIndex.calls.append(("window", int(np.max(offset)), int(k), filter_of_query is not None))
        S_ = R.scores64(Q, self.C).astype(np.float32)
        mask = None
        if filter_of_query is not None:
            f = np.broadcast_to(np.asarray(filter_of_query, dtype=np.int64), (len(S_),))
            assert self.n_filters and ((f >= -1) & (f < self.n_filters)).all()
            mask = np.stack([np.ones(len(self.C), dtype=bool) if i < 0 else self.masks[i] for i in f])
        return G.group_window_ref(S_, self.off, mask, offset, k)

    def search_groups(self, Q, k):
        assert 1 <= k <= 1000 and self.n_groups
        HostIndex.calls.append(("groups", 0, int(k), False))
        return G.group_window_ref(R.scores64(Q, self.C).astype(np.float32), self.off, None, 0, k)

    def close(self):
        pass


def _base(tmp_path):
    """six decks of five near-identical pages and forty one-page documents, interleaved on disk"""
    D, _ = R.decks(6, 5, 64, 0.05)
    C = np.concatenate([D, R.unit(40, 64, 9)])
    names = [f"deck_{d}.pdf_{i}.png" for d in range(6) for i in range(5)] + [f"other_{j}.pdf_0.png" for j in range(40)]
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    return kb, C, names


def test_demo_retrieve_documents_with_documents_and_offset(tmp_path):
    kb, C, names = _base(tmp_path)
    ix = HostIndex(64, len(C)); ix.add(C)
    qvec = R.unit(6, 64, 5)[2:3]
    HostIndex.calls = []
    p46, s46 = demo.retrieve_documents(kb, qvec, 46, None, None, index=ix, names=names, return_scores=True)
    assert HostIndex.calls == [("groups", 0, 46, False)] and ix.n_groups == 46      # both at their defaults: today's path
    assert len(p46) == 46 and len({demo.doc_of_page(os.path.basename(p)) for p in p46}) == 46
    HostIndex.calls = []
    p, s = demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=names, return_scores=True, offset=10)
    assert HostIndex.calls == [("window", 10, 10, False)]
    assert p == p46[10:20] and s == s46[10:20]
    assert demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=names, offset=40) == p46[40:]      # the ranking ends
    assert demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=names, offset=46) == []
    docs = ["deck_2.pdf", "other_7.pdf", "deck_4.pdf"]
    HostIndex.calls = []
    only, so = demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=names, documents=docs, return_scores=True)
    assert HostIndex.calls == [("window", 0, 3, True)] and ix.n_filters == 1
    assert [demo.doc_of_page(os.path.basename(x)) for x in only] == [d for d in (demo.doc_of_page(os.path.basename(x)) for x in p46) if d in docs]
    assert so == [v for x, v in zip(p46, s46) if demo.doc_of_page(os.path.basename(x)) in docs]
    assert demo.retrieve_documents(kb, qvec, 5, None, None, index=ix, names=names, documents=docs, offset=1) == only[1:]
    assert demo.retrieve_documents(kb, qvec, 5, None, None, index=ix, names=names, documents=docs, offset=3) == []
    assert demo.retrieve_documents(kb, qvec, 0, None, None, index=ix, names=names, documents=docs) == []
    with pytest.raises(ValueError, match="nowhere.pdf"):
        demo.retrieve_documents(kb, qvec, 5, None, None, index=ix, names=names, documents=["deck_2.pdf", "nowhere.pdf"])
    with pytest.raises(ValueError):
        demo.retrieve_documents(kb, qvec, 5, None, None, index=ix, names=names, offset=-1)
    assert demo.retrieve_documents(str(tmp_path / "missing"), qvec, 5, None, None, documents=docs) is None


def test_retrieve_documents_filtered_over_pickle_shards(tmp_path):
    """three shards, the pages of a deck spread over them; collections by document; per-query label sets, None = every document"""
    _, C, names = _base(tmp_path)
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(C))                                        # pages of a document are neither adjacent nor in one shard
    Cp, pids = C[perm], [names[i] for i in perm]
    bounds = (0, 20, 55, 70)
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), Cp[bounds[s]:bounds[s + 1]], pids[bounds[s]:bounds[s + 1]])
    Q = R.unit(5, 64, 42)
    qids = [f"q{q}" for q in range(5)]
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    label_of_doc = lambda d: "decks" if d.startswith("deck") else ("odd" if int(d.split("_")[1].split(".")[0]) % 2 else "even")      # noqa: E731
    wanted = {"q0": None, "q1": {"decks"}, "q2": {"odd", "decks"}, "q3": {"none-such"}, "q4": {"decks"}}
    everything, best_page = retriever.retrieve_documents(args, 46, demo.doc_of_page, index_factory=HostIndex)
    for offset, topk in ((0, 46), (0, 4), (2, 3), (5, 10)):
        HostIndex.calls = []
        sc, pg = retriever.retrieve_documents_filtered(args, topk, demo.doc_of_page, label_of_doc, lambda q: wanted[q], offset=offset,
                                                       index_factory=HostIndex)
        assert [c[0] for c in HostIndex.calls] == ["window"] and HostIndex.calls[0][3]
        for q in qids:
            allowed = [d for d in everything[q] if wanted[q] is None or label_of_doc(d) in wanted[q]]
            want = allowed[offset:offset + topk]
            assert list(sc[q]) == want and list(pg[q]) == want, (q, offset, topk)
            assert [sc[q][d] for d in want] == [everything[q][d] for d in want]
            assert [pg[q][d] for d in want] == [best_page[q][d] for d in want]
            assert all(demo.doc_of_page(pg[q][d]) == d for d in want)
    assert sc["q3"] == {} and len(sc["q1"]) == 1 and len(sc["q0"]) == 10
    with pytest.raises(ValueError):
        retriever.retrieve_documents_filtered(args, 5, demo.doc_of_page, label_of_doc, lambda q: None, offset=-1, index_factory=HostIndex)
    assert retriever.retrieve_documents_filtered(args, 0, demo.doc_of_page, label_of_doc, lambda q: None, index_factory=HostIndex)[0] == \
        {q: {} for q in qids}


# ------------------------------------------------------------------------------------------------ declarations ---
def test_the_two_symbols_are_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from visrag_amd import _lib, build
    from visrag_amd.engine import HipIndex
    header = open(os.path.join(root, "include", "visrag_hip.h")).read()
    for name in ("vr_index_search_groups_window", "vr_index_group_window_search_stats"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vr_index_search_groups_window"][1]) == 11
    assert "search_group_window.hip" in build.SOURCES
    assert build.SOURCES.index("search_group_window.hip") < build.SOURCES.index("index.hip")
    assert callable(HipIndex.search_groups_window) and callable(HipIndex.group_window_search_stats)
