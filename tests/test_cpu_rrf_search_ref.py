"""The plain-loop oracle of reciprocal-rank fusion (tests/rrf_search_ref.py) on hand-worked cases, documents.rrf_runs (the
definition in vectorised numpy, the host workaround stated exactly) against it on random lists with heavy overlap, the host
consumers (retriever.retrieve_rrf, demo.retrieve_rrf) over a host stand-in for the index, and the declarations of the four ABI
symbols.  No GPU, no library."""
import os
import types

import numpy as np
import pytest

from tests import rank_search_ref as K
from tests import rrf_search_ref as RR
from tests.group_search_ref import scores64, unit
from visrag_amd import retriever
from visrag_amd.documents import group_rows, rrf_runs
from visrag_amd.utils import write_shard

f32 = np.float32


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(_u32(got[0]), _u32(want[0]))


# ------------------------------------------------------------------------------------------------ hand-worked ---
def test_two_lists_tie_exactly_and_the_lower_id_leads():
    sc, ids, hits = RR.rrf_ref([[3, 7, 9], [7, 3, 5]], [0, 2], 4)
    both = f32(np.float64(1) / np.float64(61) + np.float64(1) / np.float64(62))
    third = f32(np.float64(1) / np.float64(63))
    assert ids.tolist() == [[3, 7, 5, 9]] and hits.tolist() == [[2, 2, 1, 1]]
    assert sc.tolist() == [[both, both, third, third]]            # 1/61 + 1/62 == 1/62 + 1/61: rows 3 and 7 tie, 3 first
    # c = 0 is plain reciprocal rank; c is a float32 before it is a float64
    sc, ids, _ = RR.rrf_ref([[3, 7, 9], [7, 3, 5]], [0, 2], 2, c=0.0)
    assert ids.tolist() == [[3, 7]] and sc.tolist() == [[f32(1.5), f32(1.5)]]
    sc, _, _ = RR.rrf_ref([[4]], [0, 1], 1, c=0.1)
    assert sc[0, 0] == f32(np.float64(1) / (np.float64(f32(0.1)) + np.float64(1)))
    # positions (1, 4) beat positions (2, 3) in fp64 (1/x is convex); at c = 1e6 the two sums round to ONE float32 and the id decides
    lists = [[9, 2, -1, -1], [-1, -1, 2, 9]]
    assert RR.rrf_ref(lists, [0, 2], 2, c=60.0)[1].tolist() == [[9, 2]]
    sc, ids, _ = RR.rrf_ref(lists, [0, 2], 2, c=1e6)
    assert ids.tolist() == [[2, 9]] and sc[0, 0] == sc[0, 1]
    # two groups: the same lists apart
    sc, ids, hits = RR.rrf_ref([[3, 7, 9], [7, 3, 5]], [0, 1, 2], 3)
    assert ids.tolist() == [[3, 7, 9], [7, 3, 5]] and (hits == 1).all()
    assert sc[0].tolist() == [f32(1 / 61), f32(1 / 62), f32(1 / 63)] and np.array_equal(sc[0], sc[1])


def test_zero_and_negative_weights():
    lists = [[1, 2, 3], [2, 4, 1], [5, 2, 6]]
    sc, ids, hits = RR.rrf_ref(lists, [0, 3], 6, weights=[1.0, 0.0, -0.5])
    # list 1 counts in hits but adds 0.0; list 2 subtracts
    F = {1: 1 / 61 + 0.0 / 63, 2: 1 / 62 + 0.0 / 61 - 0.5 / 62, 3: 1 / 63, 4: 0.0 / 62, 5: -0.5 / 61, 6: -0.5 / 63}
    assert ids.tolist() == [[1, 3, 2, 4, 6, 5]] and hits.tolist() == [[2, 1, 3, 1, 1, 1]]
    assert sc.tolist() == [[f32(F[i]) for i in (1, 3, 2, 4, 6, 5)]]
    assert sc[0, 3] == 0.0 and not np.signbit(sc[0, 3])           # 0.0 + 0.0 / 62: +0.0, ahead of the negative scores
    # a weight of -0.0: the sum starts at +0.0, so the score is +0.0 and id order decides among the zeros
    sc, ids, _ = RR.rrf_ref([[9, 8]], [0, 1], 2, weights=[-0.0])
    assert ids.tolist() == [[8, 9]] and not np.signbit(sc).any()


def test_holes_duplicates_and_tails():
    # holes keep their position: id 7 stands at position 3 of list 0
    sc, ids, hits = RR.rrf_ref([[-1, 4, 7, -1], [-1, -1, -1, -1]], [0, 2], 3)
    assert ids.tolist() == [[4, 7, -1]] and hits.tolist() == [[1, 1, 0]]
    assert sc[0, :2].tolist() == [f32(1 / 62), f32(1 / 63)] and np.isneginf(sc[0, 2])
    # a duplicate inside one list counts at both positions
    sc, ids, hits = RR.rrf_ref([[5, 6, 5]], [0, 1], 2)
    assert ids.tolist() == [[5, 6]] and hits.tolist() == [[2, 1]]
    assert sc.tolist() == [[f32(np.float64(1) / 61 + np.float64(1) / 63), f32(1 / 62)]]
    # k beyond the distinct ids; a group of empty lists; ids out of range are holes
    sc, ids, hits = RR.rrf_ref([[1, 2], [2, 1], [-1, -1], [2 ** 31 - 1, -5]], [0, 2, 3, 4], 5)
    assert ids.tolist() == [[1, 2, -1, -1, -1], [-1] * 5, [-1] * 5] and hits.tolist() == [[2, 2, 0, 0, 0], [0] * 5, [0] * 5]
    assert np.isneginf(sc[0, 2:]).all() and np.isneginf(sc[1:]).all()
    sc, ids, _ = RR.rrf_ref([[0, 2 ** 31 - 2]], [0, 1], 2)
    assert ids.tolist() == [[0, 2 ** 31 - 2]]


# ------------------------------------------------------------------------------------------------ rrf_runs ---
@pytest.mark.parametrize("universe,holes,c,seed", [(50, 0.0, 60.0, 1), (50, 0.3, 0.0, 2), (12, 0.3, 1e6, 3), (2 ** 31 - 1, 0.1, 60.0, 4),
                                                  (7, 0.0, 60.0, 5)])
def test_rrf_runs_is_the_oracle(universe, holes, c, seed):
    from tests.multi_search_ref import layout
    lims = layout(37, (1, 2, 3, 4, 5, 6, 7, 9))
    ids = RR.random_lists(37, 10, universe, holes, seed, distinct=universe > 12)     # (universe 7 and 12: repeats inside a list)
    if universe > 1 << 20:
        ids[0, 0], ids[3, 4] = 0, 2 ** 31 - 2
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(37).astype(np.float32)
    w[5], w[11] = 0.0, -abs(w[11]) - 1
    for weights in (None, w):
        for k in (1, 10, 100):
            _same(rrf_runs(ids, lims, k, c, weights), RR.rrf_ref(ids, lims, k, c, weights))


def test_rrf_runs_checks_its_arguments():
    ids = np.array([[1, 2], [2, 3]])
    for bad in ([1, 2], [0, 0, 2], [0, 1], [0, 2, 1]):
        with pytest.raises(ValueError):
            rrf_runs(ids, bad, 1)
    for kw in (dict(k=0), dict(k=1, c=-1.0), dict(k=1, c=float("nan")), dict(k=1, weights=[1.0]), dict(k=1, weights=[1.0, float("inf")])):
        with pytest.raises(ValueError):
            rrf_runs(ids, [0, 2], **kw)
    with pytest.raises(ValueError):
        rrf_runs(np.array([1, 2]), [0, 1], 1)
    sc, ids_, hits = rrf_runs(np.zeros((0, 4), dtype=np.int64), [0], 3)
    assert sc.shape == ids_.shape == hits.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ host consumers ---
class HostIndex:
    """stands in for HipIndex: rankings of fp32-rounded fp64 scores, the rank fusion by the oracle"""
    calls = []

    def __init__(self, dim, capacity, device=0):
        self.dim = dim
        self.C = np.zeros((0, dim), dtype=np.float32)
        self.mask = None

    def add(self, reps):
        self.C = np.concatenate([self.C, np.asarray(reps, dtype=np.float32)])

    def __len__(self):
        return len(self.C)

    def set_filters(self, masks):
        self.mask = np.asarray(masks, dtype=bool)

    def search(self, Q, k, mask=None):
        HostIndex.calls.append((len(self.C), len(Q), int(k)))
        S = scores64(Q, self.C).astype(np.float32)
        sc = np.full((len(Q), k), -np.inf, dtype=np.float32)
        ids = np.full((len(Q), k), -1, dtype=np.int64)
        for q in range(len(Q)):
            order = K.ranking(S[q])
            order = (order if mask is None else order[mask[order]])[:k]
            sc[q, :len(order)], ids[q, :len(order)] = S[q][order], order
        return sc, ids

    def search_rrf(self, Q, lims, k, depth=100, c=60.0, weights=None, filter_of_group=None, documents=False):
        assert not documents and filter_of_group in (None, 0)
        _, ids = self.search(Q, depth, None if filter_of_group is None else self.mask[0])
        return RR.rrf_ref(ids, lims, k, c, weights)

    def close(self):
        pass


def _host_fuse(ids, lims, k, c, weights, device):
    return rrf_runs(ids, lims, k, c, weights)


def test_retrieve_rrf_fuses_global_positions(tmp_path):
    C, Q, bounds = K.shards_case()                                        # shards of 1 000, 3 001 and 1 999 rows, 9 queries
    names = [f"page_{i}" for i in range(len(C))]
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"t{q % 4}-part{q}" for q in range(len(Q))]                   # topics t0 (3 queries), t1, t2, t3 (2 each), interleaved
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    topic = lambda qid: qid.split("-")[0]
    order, lims, topics = group_rows([topic(q) for q in qids])
    whole = HostIndex(256, len(C))
    whole.add(C)
    weight = lambda qid: 0.5 + int(qid.split("part")[1]) / 4
    for depth, k, wfn in ((40, 30, None), (120, 1000, weight), (1, 3, None)):
        HostIndex.calls = []
        run = retriever.retrieve_rrf(args, topic, k, depth, 10.0, wfn, index_factory=HostIndex, fuse_lists=_host_fuse)
        assert HostIndex.calls == [(1000, 9, depth), (3001, 9, depth), (1999, 9, depth)]
        w = None if wfn is None else [wfn(qids[i]) for i in order]
        sc, ids, _ = whole.search_rrf(Q[order], lims, k, depth, 10.0, w)
        assert list(run) == topics
        for g, t in enumerate(topics):
            live = ids[g] >= 0
            assert list(run[t]) == [names[i] for i in ids[g][live]]
            assert list(run[t].values()) == [float(s) for s in sc[g][live]]
    assert retriever.retrieve_rrf(args, topic, 0, index_factory=HostIndex, fuse_lists=_host_fuse) == {t: {} for t in topics}
    one = retriever.retrieve_rrf(args, lambda qid: qid, 5, 5, index_factory=HostIndex, fuse_lists=_host_fuse)   # groups of one
    assert list(one) == qids and list(one[qids[3]]) == [names[i] for i in whole.search(Q[3:4], 5)[1][0]]
    assert list(one[qids[3]].values()) == [float(f32(1 / (f32(60.0).astype(np.float64) + r + 1))) for r in range(5)]


def test_demo_retrieve_rrf_over_a_host_index(tmp_path):
    from visrag_amd import demo
    C = unit(60, 64, 3)
    names = [f"deck_{i // 5}.pdf_{i % 5}.png" for i in range(60)]
    qs = unit(3, 64, 4)
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    ix = HostIndex(64, 60)
    ix.add(C)
    want = ix.search_rrf(qs, [0, 3], 8, 20, 60.0)
    p, s, h = demo.retrieve_rrf(kb, qs, 8, None, None, index=ix, names=names, depth=20, return_scores=True)
    assert p == [os.path.join(kb, names[i]) for i in want[1][0]] and s == [float(x) for x in want[0][0]] and h == want[2][0].tolist()
    assert demo.retrieve_rrf(kb, qs, 8, None, None, index=ix, names=names, depth=20) == p
    docs = ["deck_2.pdf", "deck_7.pdf"]
    p = demo.retrieve_rrf(kb, qs, 20, None, None, index=ix, names=names, depth=20, documents=docs, weights=[1.0, 2.0, 0.5])
    allowed = np.array([n.rsplit("_", 1)[0] in docs for n in names])
    _, ids = ix.search(qs, 20, allowed)
    want = RR.rrf_ref(ids, [0, 3], 10, 60.0, [1.0, 2.0, 0.5])
    assert len(p) == 10 and p == [os.path.join(kb, names[i]) for i in want[1][0]]
    assert demo.retrieve_rrf(kb, qs, 5, None, None, index=ix, names=names, documents=["nothing.pdf"]) == []
    assert demo.retrieve_rrf(str(tmp_path / "none"), qs, 5, None, None) is None


# ------------------------------------------------------------------------------------------------ declarations ---
def test_the_four_symbols_are_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from visrag_amd import _lib, build, demo, engine
    from visrag_amd.engine import HipIndex
    header = open(os.path.join(root, "include", "visrag_hip.h")).read()
    for name in ("vr_rrf_fuse", "vr_rrf_max_entries", "vr_index_search_rrf", "vr_index_rrf_search_stats"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vr_rrf_fuse"][1]) == 14 and len(_lib.SIGNATURES["vr_index_search_rrf"][1]) == 16
    assert len(_lib.SIGNATURES["vr_rrf_max_entries"][1]) == 0 and len(_lib.SIGNATURES["vr_index_rrf_search_stats"][1]) == 3
    assert "search_rrf.hip" in build.SOURCES and build.SOURCES.index("search_rrf.hip") < build.SOURCES.index("index.hip")
    assert callable(HipIndex.search_rrf) and callable(HipIndex.rrf_max_entries) and callable(HipIndex.rrf_search_stats)
    assert callable(engine.rrf_fuse) and callable(retriever.retrieve_rrf) and callable(demo.retrieve_rrf) and callable(demo.retrieve_any)
    lib = _lib.load()
    assert lib.vr_rrf_max_entries() >= 8192
