"""The numpy reference of the fused document search (tests/multi_group_search_ref.py) on hand-worked cases, what the reference
alone says about the fp64 test's intervals, `documents.evidence_pages`, and the demo / retriever additions over a host stand-in
for the index.  No GPU, no built library."""
import os
import types

import numpy as np
import pytest

from tests import multi_group_search_ref as M
from tests import rank_search_ref as K
from tests.group_search_ref import scores64, unit
from visrag_amd import retriever
from visrag_amd.documents import evidence_pages
from visrag_amd.utils import write_shard

NEG = -np.inf


# ------------------------------------------------------------------------------------------- hand-worked cases ---
def test_all_of_wins_through_two_different_pages():
    """document 1 answers sub-query 0 on its first page and sub-query 1 on its second; no single page of it scores above the
    runner-up's pages, so page-level all-of prefers document 0, document-level all-of document 1"""
    off = [0, 2, 4, 5]
    S = np.array([[0.5, 0.1, 0.9, 0.0, 0.3],
                  [0.5, 0.2, 0.0, 0.8, 0.3]])
    sc, rows, docs, which, evs, evr = M.multi_group_ref(S, [0, 2], off, 3, "min")
    assert docs.tolist() == [[1, 0, 2]] and sc.tolist() == [[0.8, 0.5, 0.3]]
    assert which.tolist() == [[1, 0, 0]] and rows.tolist() == [[3, 0, 4]]          # which on equal values: the lowest sub-query
    assert evr.reshape(3, 2).tolist() == [[2, 3], [0, 0], [4, 4]]
    assert evs.reshape(3, 2).tolist() == [[0.9, 0.8], [0.5, 0.5], [0.3, 0.3]]
    page_min = S.min(axis=0)
    assert page_min.argmax() == 0 and page_min[2:4].max() < page_min[0]           # over pages: a page of document 0
    sc, rows, docs, which, evs, evr = M.multi_group_ref(S, [0, 2], off, 3, "max")
    assert docs.tolist() == [[1, 0, 2]] and sc.tolist() == [[0.9, 0.5, 0.3]] and which.tolist() == [[0, 0, 0]] and rows.tolist() == [[2, 0, 4]]


def test_absent_documents_allowed_ties_and_k_beyond_the_present():
    off = [0, 3, 5, 6, 8]
    S = np.array([[0.7, 0.7, 0.7, 0.2, 0.6, 0.9, 0.6, 0.6],
                  [0.1, 0.4, 0.4, 0.6, 0.2, 0.9, 0.3, 0.6]])
    mask = np.array([False, True, True, True, True, False, True, True])           # document 2 has no allowed page: absent
    sc, rows, docs, which, evs, evr = M.multi_group_ref(S, [0, 2], off, 5, "max", mask)
    assert docs.tolist() == [[0, 1, 3, -1, -1]] and sc.tolist() == [[0.7, 0.6, 0.6, NEG, NEG]]      # exactly tied: the lower document first
    assert rows.tolist() == [[1, 4, 6, -1, -1]] and which.tolist() == [[0, 0, 0, -1, -1]]          # the lowest ALLOWED tied row; equal E: j = 0
    assert evr.reshape(5, 2).tolist() == [[1, 1], [4, 3], [6, 7], [-1, -1], [-1, -1]]
    assert evs.reshape(5, 2).tolist() == [[0.7, 0.4], [0.6, 0.6], [0.6, 0.6], [NEG, NEG], [NEG, NEG]]
    sc, rows, docs, which, _, _ = M.multi_group_ref(S, [0, 2], off, 2, "min", mask)
    assert docs.tolist() == [[1, 3]] and sc.tolist() == [[0.6, 0.6]] and which.tolist() == [[0, 0]] and rows.tolist() == [[4, 6]]
    # per-question masks, questions of different sizes, the evidence blocks at k * lims[g]
    sc, rows, docs, which, evs, evr = M.multi_group_ref(S, [0, 1, 2], off, 2, "max", [None, mask])
    assert docs.tolist() == [[2, 0], [1, 3]] and rows.tolist() == [[5, 0], [3, 7]]
    assert M.evidence_of(evr, [0, 1, 2], 1, 2).tolist() == [[3], [7]] and len(evr) == 4
    none = M.multi_group_ref(S, [0, 2], off, 2, "max", np.zeros(8, dtype=bool))
    assert (none[2] == -1).all() and np.isneginf(none[0]).all() and (none[5] == -1).all()


def test_float32_scores_rank_on_their_bits():
    off = [0, 1, 2]
    S = np.array([[-0.0, 0.0]], dtype=np.float32)
    sc, rows, docs, which, _, _ = M.multi_group_ref(S, [0, 1], off, 2, "max")
    assert docs.tolist() == [[1, 0]] and np.signbit(sc[0, 1]) and not np.signbit(sc[0, 0])         # -0.0 < +0.0
    S2 = np.array([[0.0], [-0.0]], dtype=np.float32)
    assert M.multi_group_ref(S2, [0, 2], [0, 1], 1, "min")[3].tolist() == [[1]]
    assert M.multi_group_ref(S2, [0, 2], [0, 1], 1, "max")[3].tolist() == [[0]]


@pytest.mark.parametrize("name", list(M.TABLE))
def test_what_the_reference_alone_widens(name):
    C, Q, off, S = M.case(name)
    for cycle, density, table in M.TABLE[name]:
        lims = M.layout(len(Q), cycle)
        for fuse in ("max", "min"):
            assert M.widened(S, lims, off, M.K_FP64, fuse, M.case_mask(name, density)) == table[fuse]


def test_check_question_accepts_the_reference_and_rejects_a_swap():
    C, Q, off, S = M.case("unit-5000x37x256-mean7")
    lims = M.layout(len(Q), (1, 2, 3, 4, 5, 6, 7, 9))
    out = M.multi_group_ref(S, lims, off, 20, "min")
    g = 4
    args = [out[i][g] for i in range(4)] + [M.evidence_of(out[4], lims, g, 20), M.evidence_of(out[5], lims, g, 20)]
    n, moved, err, bad = M.check_question(S, lims, off, g, "min", None, *args)
    assert (n, moved, err, bad) == (20, 0, 0.0, None)
    swapped = [a.copy() for a in args]
    for a in swapped:
        a[[0, 19]] = a[[19, 0]]
    assert M.check_question(S, lims, off, g, "min", None, *swapped)[3] is not None


# --------------------------------------------------------------------------------------------- evidence_pages ---
def test_evidence_pages():
    rows = np.array([[7, 3], [3, 9], [-1, -1]])
    scores = np.array([[0.9, 0.4], [0.6, 0.5], [NEG, NEG]], dtype=np.float32)
    r, s = evidence_pages(rows, scores)
    assert r.tolist() == [7, 3, 9] and r.dtype == np.int64 and s.dtype == np.float32
    assert np.array_equal(s, np.array([0.9, 0.6, 0.5], dtype=np.float32))          # the best score seen for a page
    r, s = evidence_pages(rows, scores, limit=2)
    assert r.tolist() == [7, 3] and np.array_equal(s, np.array([0.9, 0.6], dtype=np.float32))
    assert evidence_pages(rows, scores, limit=0)[0].tolist() == [] and evidence_pages(rows[2:], scores[2:])[0].tolist() == []
    with pytest.raises(ValueError):
        evidence_pages(rows, scores[:2])
    with pytest.raises(ValueError):
        evidence_pages(rows, scores, limit=-1)


# ------------------------------------------------------------------------------------------- host consumers ---
class HostIndex:
    """stands in for HipIndex: the fused document ranking over fp32-rounded fp64 scores, on the host"""
    calls = []

    def __init__(self, dim, capacity, device=0):
        self.dim = dim
        self.C = np.zeros((0, dim), dtype=np.float32)
        self.off, self.masks, self.n_groups = None, None, 0

    def add(self, reps):
        self.C = np.concatenate([self.C, np.asarray(reps, dtype=np.float32)])

    def __len__(self):
        return len(self.C)

    def set_groups(self, offsets):
        self.off = np.asarray(offsets, dtype=np.int64)
        self.n_groups = len(self.off) - 1

    def set_filters(self, masks):
        self.masks = np.asarray(masks, dtype=bool)

    def search_multi_groups(self, Q, lims, k, fuse="max", filter_of_group=None, evidence=False):
        assert 1 <= k <= 1000 and np.diff(lims).max() <= 256 and self.off is not None
        nq = len(lims) - 1
        HostIndex.calls.append((len(self.C), len(Q), nq, int(k), fuse, filter_of_group is not None))
        mask = None
        if filter_of_group is not None:
            f = np.broadcast_to(np.asarray(filter_of_group), (nq,))
            mask = [None if x < 0 else self.masks[x] for x in f]
        out = M.multi_group_ref(scores64(Q, self.C).astype(np.float32), lims, self.off, k, fuse, mask)
        return out if evidence else out[:4]

    def close(self):
        pass


def test_retrieve_documents_fused_builds_one_reordered_index(tmp_path):
    C, Q, bounds = K.shards_case()                                        # shards of 1 000, 3 001 and 1 999 rows, 9 queries
    names = [f"page_{i}" for i in range(len(C))]
    doc_of = lambda page: f"doc_{int(page.split('_')[1]) % 50}"          # noqa: E731  (the pages of a document are NOT adjacent)
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"t{q % 4}-part{q}" for q in range(len(Q))]                   # topics t0 (3 queries), t1, t2, t3 (2 each), interleaved
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    topic = lambda qid: qid.split("-")[0]                                 # noqa: E731
    topics = ["t0", "t1", "t2", "t3"]
    S_ = scores64(Q, C)
    for fuse in ("max", "min"):
        HostIndex.calls = []
        sc, pg = retriever.retrieve_documents_fused(args, topic, 7, doc_of, fuse, index_factory=HostIndex)
        assert HostIndex.calls == [(6000, 9, 4, 7, fuse, False)] and list(sc) == topics == list(pg)
        for t in topics:
            sub = [q for q in range(len(Q)) if q % 4 == int(t[1])]
            E = np.array([[S_[q, d::50].astype(np.float32).max() for d in range(50)] for q in sub])         # [m][50]
            Fd = E.max(axis=0) if fuse == "max" else E.min(axis=0)
            best = np.lexsort((np.arange(50), -Fd.astype(np.float64)))[:7]
            assert list(sc[t]) == [f"doc_{d}" for d in best] == list(pg[t])
            assert list(sc[t].values()) == [float(Fd[d]) for d in best]
            for d in best:
                assert pg[t][f"doc_{d}"] == [names[d + 50 * int(np.argmax(S_[q, d::50].astype(np.float32)))] for q in sub]
    lab = lambda d: int(d.split("_")[1]) % 2                              # noqa: E731
    sc, pg = retriever.retrieve_documents_fused(args, topic, 30, doc_of, "max", lab, lambda g: {1} if g == "t1" else None, index_factory=HostIndex)
    assert HostIndex.calls[-1] == (6000, 9, 4, 30, "max", True)
    assert len(sc["t0"]) == 30 and len(sc["t1"]) == 25 and all(int(d.split("_")[1]) % 2 == 1 for d in sc["t1"])
    assert retriever.retrieve_documents_fused(args, topic, 0, doc_of, index_factory=HostIndex) == ({t: {} for t in topics}, {t: {} for t in topics})


def test_demo_retrieve_documents_any_over_the_host_index(tmp_path, monkeypatch):
    from visrag_amd import demo
    monkeypatch.setattr(demo, "HipIndex", HostIndex)
    monkeypatch.setattr("visrag_amd.modeling.default_device", lambda: 0)
    C = unit(12, 32, 3)
    names = [f"{'ab'[i % 2]}.pdf_{i // 2}.png" for i in range(12)]         # two documents, pages interleaved on disk
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    np.save(os.path.join(kb, "reps.npy"), C)
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))
    qv = np.stack([C[2], C[6]])                                           # pages 1 and 3 of a.pdf
    paths, scores, ev = demo.retrieve_documents_any(kb, qv, 5, None, None, fuse="min", return_evidence=True)
    assert [os.path.basename(p) for p in paths][0] in ("a.pdf_1.png", "a.pdf_3.png") and len(paths) == 2
    assert [os.path.basename(p) for p, _ in ev[0]] == ["a.pdf_1.png", "a.pdf_3.png"]
    assert all(os.path.basename(p).startswith("b.pdf") for p, _ in ev[1]) and scores[0] > scores[1]
    only = demo.retrieve_documents_any(kb, qv, 5, None, None, documents=["b.pdf"])
    assert len(only) == 1 and os.path.basename(only[0]).startswith("b.pdf")
    with pytest.raises(ValueError):
        demo.retrieve_documents_any(kb, qv, 5, None, None, documents=["c.pdf"])
    assert demo.retrieve_documents_any(str(tmp_path / "nowhere"), qv, 5, None, None) is None


# ------------------------------------------------------------------------------------------------ declarations ---
def test_the_two_symbols_are_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from visrag_amd import _lib, build, demo, documents
    from visrag_amd.engine import HipIndex
    header = open(os.path.join(root, "include", "visrag_hip.h")).read()
    for name in ("vr_index_search_multi_groups", "vr_index_multi_group_search_stats"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vr_index_search_multi_groups"][1]) == 16 and len(_lib.SIGNATURES["vr_index_multi_group_search_stats"][1]) == 3
    assert "search_multi_group.hip" in build.SOURCES and build.SOURCES.index("search_multi_group.hip") < build.SOURCES.index("index.hip")
    assert callable(HipIndex.search_multi_groups) and callable(HipIndex.multi_group_search_stats)
    assert callable(retriever.retrieve_documents_fused) and callable(demo.retrieve_documents_any) and callable(documents.evidence_pages)
