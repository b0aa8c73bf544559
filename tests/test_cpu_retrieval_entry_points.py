"""The Python entry points of retrieval (visrag_amd/retriever.py over pickle shards, visrag_amd/demo.py over a knowledge base) on
one host stand-in for the index: what they return against a brute-force ranking, the calls they make on the index, and the
differences between them that a merge of their common passages could erase — which unknown names raise, when groups are set
from the names, which checks come before a file is read.  No GPU, no library."""
import os
import pickle
import types

import numpy as np
import pytest

from tests import group_search_ref as R
from visrag_amd import demo, retriever
from visrag_amd.documents import rrf_runs
from visrag_amd.utils import write_shard

DIM = 64


class HostIndex:
    """stands in for HipIndex: fp32-rounded fp64 scores, ties by lower row (document: lower group), on the host"""
    calls = []          # (method, figures) of every index of a test, in call order
    made = []           # every index of a test
    live = 0            # indexes made and not closed
    most_live = 0

    def __init__(self, dim, capacity, device=0):
        self.dim, self.capacity = dim, capacity
        self.C = np.zeros((0, dim), dtype=np.float32)
        self.n_groups = self.n_filters = self.closed = 0
        HostIndex.made.append(self)
        HostIndex.live += 1
        HostIndex.most_live = max(HostIndex.most_live, HostIndex.live)

    @classmethod
    def fresh(cls):
        cls.calls, cls.made, cls.live, cls.most_live = [], [], 0, 0

    @classmethod
    def names(cls):
        return [c[0] for c in cls.calls]

    def _log(self, *what):
        HostIndex.calls.append(what)

    def add(self, reps):
        self._log("add", len(reps), np.asarray(reps).dtype.name)
        self.C = np.concatenate([self.C, np.asarray(reps, dtype=np.float32)])
        self.n_groups = self.n_filters = 0

    def __len__(self):
        return len(self.C)

    def close(self):
        self.closed += 1
        HostIndex.live -= 1

    def rows(self, ids):
        return self.C[np.asarray(ids, dtype=np.int64)]

    def set_groups(self, offsets):
        self.off = np.asarray(offsets, dtype=np.int64)
        assert self.off[0] == 0 and self.off[-1] == len(self.C) and (np.diff(self.off) > 0).all()
        self.n_groups = len(self.off) - 1
        self._log("set_groups", self.n_groups)

    def set_filters(self, masks):
        self.masks = np.atleast_2d(np.asarray(masks, dtype=bool))
        assert self.masks.shape[1] == len(self.C)
        self.n_filters = len(self.masks)
        self._log("set_filters", self.n_filters)

    # ---- the ranking rule ----
    def _scores(self, Q):
        Q = np.asarray(Q.detach().cpu() if hasattr(Q, "detach") else Q, dtype=np.float32)
        assert Q.ndim == 2 and Q.shape[1] == self.dim
        return R.scores64(Q, self.C).astype(np.float32)

    def _allowed(self, n, f):
        if f is None:
            return np.ones((n, len(self.C)), dtype=bool)
        f = np.broadcast_to(np.asarray(f, dtype=np.int64), (n,))
        assert self.n_filters and ((f >= -1) & (f < self.n_filters)).all()
        return np.stack([np.ones(len(self.C), dtype=bool) if i < 0 else self.masks[i] for i in f])

    @staticmethod
    def _ranked(s, allowed):
        """one query: the allowed ids by score descending, then id ascending"""
        ids = np.flatnonzero(allowed)
        return ids[np.lexsort((ids, -s[ids].astype(np.float64)))]

    @staticmethod
    def _table(lists, k, *values):
        """per-query id lists -> (values[0] of the ids [n, k] f32, ids [n, k] i64, further values i32), tails (-inf, -1, -1)"""
        out = [np.full((len(lists), k), -np.inf, dtype=np.float32), np.full((len(lists), k), -1, dtype=np.int64)]
        out += [np.full((len(lists), k), -1, dtype=np.int32) for _ in values[1:]]
        for q, ids in enumerate(lists):
            ids = ids[:k]
            out[1][q, :len(ids)] = ids
            for o, v in zip([out[0]] + out[2:], values):
                o[q, :len(ids)] = v[q][ids]
        return tuple(out)

    def _rows_call(self, Q, first, k, f):
        S = self._scores(Q)
        A = self._allowed(len(S), f)
        return self._table([self._ranked(S[q], A[q])[first:] for q in range(len(S))], k, S)

    def search(self, Q, k):
        assert 1 <= k <= 1000
        self._log("search", int(k))
        return self._rows_call(Q, 0, k, None)

    def search_filtered(self, Q, k, filter_of_query=None):
        assert 1 <= k <= 1000 and self.n_filters
        self._log("search_filtered", int(k))
        return self._rows_call(Q, 0, k, filter_of_query)

    def search_window(self, Q, offset, k, filter_of_query=None):
        assert 1 <= k <= 1000 and offset >= 0
        self._log("search_window", int(offset), int(k), filter_of_query is not None)
        return self._rows_call(Q, int(offset), k, filter_of_query)

    def search_diverse(self, Q, k, pool=None, lambda_=0.5, filter_of_query=None):
        assert 1 <= k <= 1000
        self._log("search_diverse", int(k), pool, float(lambda_), filter_of_query is not None)
        pool = min(1000, max(4 * k, 32)) if pool is None else pool
        S = self._scores(Q)
        A = self._allowed(len(S), filter_of_query)
        picks = []
        for q in range(len(S)):
            cand, got = list(self._ranked(S[q], A[q])[:pool]), []
            while cand and len(got) < k:
                pen = [max((float(self.C[i].astype(np.float64) @ self.C[j].astype(np.float64)) for j in got), default=0.0) for i in cand]
                mmr = [lambda_ * float(S[q, i]) - (1 - lambda_) * p if got else float(S[q, i]) for i, p in zip(cand, pen)]
                got.append(cand.pop(int(np.argmax(mmr))))
            picks.append(np.asarray(got, dtype=np.int64))
        return self._table(picks, k, S)

    def search_range(self, Q, threshold, filter_of_query=None, max_total=None, sort=True):
        self._log("search_range", float(threshold), filter_of_query is not None, sort)
        S = self._scores(Q)
        A = self._allowed(len(S), filter_of_query)
        per = []
        for q in range(len(S)):
            ids = self._ranked(S[q], A[q] & (S[q] >= np.float32(threshold)))
            per.append(ids if sort else np.sort(ids))
        lims = np.concatenate([[0], np.cumsum([len(i) for i in per])]).astype(np.int64)
        return lims, np.concatenate([S[q][i] for q, i in enumerate(per)]).astype(np.float32), np.concatenate(per).astype(np.int64)

    @staticmethod
    def _pairs(values, lims, nq):
        v = np.asarray(values)
        if lims is None:
            assert v.ndim == 2 and v.shape[0] == nq
            return v.reshape(-1), np.arange(nq + 1) * v.shape[1], v.shape
        assert len(lims) == nq + 1 and lims[-1] == v.size
        return v.reshape(-1), np.asarray(lims), (v.size,)

    def rank_rows(self, Q, ids, lims=None, filter_of_query=None):
        S = self._scores(Q)
        A = self._allowed(len(S), filter_of_query)
        flat, lims, shape = self._pairs(ids, lims, len(S))
        self._log("rank_rows", len(flat), filter_of_query is not None)
        sc, rk = np.zeros(len(flat), np.float32), np.zeros(len(flat), np.int64)
        for q in range(len(S)):
            for j in range(lims[q], lims[q + 1]):
                t = int(flat[j])
                sc[j] = S[q, t]
                rk[j] = int((A[q] & ((S[q] > S[q, t]) | ((S[q] == S[q, t]) & (np.arange(len(self.C)) < t)))).sum())
        return sc.reshape(shape), rk.reshape(shape)

    def count_range(self, Q, thresholds, lims=None, filter_of_query=None, strict=False):
        S = self._scores(Q)
        flat, lims, shape = self._pairs(thresholds, lims, len(S))
        self._log("count_range", len(flat), bool(strict))
        out = np.zeros(len(flat), np.int64)
        for q in range(len(S)):
            for j in range(lims[q], lims[q + 1]):
                out[j] = int((S[q] > flat[j]).sum() if strict else (S[q] >= flat[j]).sum())
        return out.reshape(shape)

    def _fused(self, X, lims, fuse):
        """X [n_sub][ids] -> (fused [n_groups][ids], which [n_groups][ids]): max or min over a group's sub-queries, lowest decider"""
        F, W = [], []
        for a, b in zip(lims[:-1], lims[1:]):
            x = X[a:b]
            F.append(x.max(0) if fuse == "max" else x.min(0))
            W.append((x.argmax(0) if fuse == "max" else x.argmin(0)).astype(np.int32))
        return np.stack(F), np.stack(W)

    def search_multi(self, Q, lims, k, fuse="max", filter_of_group=None):
        assert 1 <= k <= 1000 and fuse in ("max", "min")
        lims = np.asarray(lims, dtype=np.int64)
        self._log("search_multi", len(Q), int(k), fuse, filter_of_group is not None)
        F, W = self._fused(self._scores(Q), lims, fuse)
        A = self._allowed(len(F), filter_of_group)
        return self._table([self._ranked(F[g], A[g]) for g in range(len(F))], k, F, W)

    def search_rrf(self, Q, lims, k, depth=100, c=60.0, weights=None, filter_of_group=None):
        assert 1 <= k <= 1000 and 1 <= depth <= 1000
        lims = np.asarray(lims, dtype=np.int64)
        self._log("search_rrf", len(Q), int(k), int(depth), float(c), filter_of_group is not None)
        f = None if filter_of_group is None else np.repeat(np.broadcast_to(filter_of_group, (len(lims) - 1,)), np.diff(lims))
        return rrf_runs(self._rows_call(Q, 0, depth, f)[1], lims, k, c, weights)

    # ---- documents: a group scores as its best allowed row does, that row (the lowest among equals) is its best row ----
    def _best(self, S, A):
        """-> (E [n][n_groups] f32, -inf where no row is allowed, best rows [n][n_groups], present [n][n_groups])"""
        E = np.full((len(S), self.n_groups), -np.inf, dtype=np.float32)
        best = np.full((len(S), self.n_groups), -1, dtype=np.int64)
        for q in range(len(S)):
            for g in range(self.n_groups):
                ids = np.arange(self.off[g], self.off[g + 1])[A[q, self.off[g]:self.off[g + 1]]]
                if len(ids):
                    best[q, g] = ids[np.argmax(S[q, ids])]
                    E[q, g] = S[q, best[q, g]]
        return E, best, best >= 0

    def _groups_call(self, Q, first, k, f):
        assert self.n_groups
        S = self._scores(Q)
        E, best, present = self._best(S, self._allowed(len(S), f))
        sc, groups, rows = self._table([self._ranked(E[q], present[q])[first:] for q in range(len(S))], k, E, best)
        return sc, rows.astype(np.int64), groups

    def search_groups(self, Q, k):
        assert 1 <= k <= 1000
        self._log("search_groups", int(k))
        return self._groups_call(Q, 0, k, None)

    def search_groups_window(self, Q, offset, k, filter_of_query=None):
        assert 1 <= k <= 1000
        self._log("search_groups_window", int(offset), int(k), filter_of_query is not None)
        return self._groups_call(Q, int(offset), k, filter_of_query)

    def search_groups_range(self, Q, threshold, filter_of_query=None, max_total=None, sort=True):
        assert self.n_groups
        self._log("search_groups_range", float(threshold), filter_of_query is not None)
        S = self._scores(Q)
        E, best, present = self._best(S, self._allowed(len(S), filter_of_query))
        per = [self._ranked(E[q], present[q] & (E[q] >= np.float32(threshold))) for q in range(len(S))]
        lims = np.concatenate([[0], np.cumsum([len(g) for g in per])]).astype(np.int64)
        cat = lambda X, t: np.concatenate([X[q][g] for q, g in enumerate(per)]).astype(t)      # noqa: E731
        return lims, cat(E, np.float32), cat(best, np.int64), np.concatenate(per).astype(np.int64)

    def rank_groups(self, Q, groups, lims=None, filter_of_query=None):
        assert self.n_groups
        S = self._scores(Q)
        E, best, present = self._best(S, self._allowed(len(S), filter_of_query))
        flat, lims, shape = self._pairs(groups, lims, len(S))
        self._log("rank_groups", len(flat), filter_of_query is not None)
        sc, rows, rk = np.full(len(flat), -np.inf, np.float32), np.full(len(flat), -1, np.int64), np.full(len(flat), -1, np.int64)
        for q in range(len(S)):
            for j in range(lims[q], lims[q + 1]):
                g = int(flat[j])
                if present[q, g]:
                    ahead = present[q] & ((E[q] > E[q, g]) | ((E[q] == E[q, g]) & (np.arange(self.n_groups) < g)))
                    sc[j], rows[j], rk[j] = E[q, g], best[q, g], int(ahead.sum())
        return sc.reshape(shape), rows.reshape(shape), rk.reshape(shape)

    def search_multi_groups(self, Q, lims, k, fuse="max", filter_of_group=None, evidence=False):
        assert 1 <= k <= 1000 and fuse in ("max", "min") and self.n_groups and evidence
        lims = np.asarray(lims, dtype=np.int64)
        self._log("search_multi_groups", len(Q), int(k), fuse, filter_of_group is not None)
        S = self._scores(Q)
        sub_filter = None if filter_of_group is None else np.repeat(np.broadcast_to(filter_of_group, (len(lims) - 1,)), np.diff(lims))
        E, best, present = self._best(S, self._allowed(len(S), sub_filter))
        F, W = self._fused(E, lims, fuse)
        ng = len(lims) - 1
        sc, docs, which = self._table([self._ranked(F[g], present[lims[g]]) for g in range(ng)], k, F, W)
        rows = np.full((ng, k), -1, dtype=np.int64)
        ev_s, ev_r = np.full(len(Q) * k, -np.inf, dtype=np.float32), np.full(len(Q) * k, -1, dtype=np.int64)
        for g in range(ng):
            m = lims[g + 1] - lims[g]
            for slot, d in enumerate(docs[g]):
                if d >= 0:
                    rows[g, slot] = best[lims[g] + which[g, slot], d]
                    at = k * lims[g] + slot * m
                    ev_s[at:at + m], ev_r[at:at + m] = E[lims[g]:lims[g + 1], d], best[lims[g]:lims[g + 1], d]
        return sc, rows, docs, which, ev_s, ev_r


def brute(q, C, ids=None):
    """[(id, fp32 score)] of one query over the rows `ids` of C (every row), score descending, then the order of `ids`"""
    ids = np.arange(len(C)) if ids is None else np.asarray(ids, dtype=np.int64)
    s = R.scores64(np.asarray(q, np.float32).reshape(1, -1), C[ids]).astype(np.float32)[0]
    return [(int(ids[j]), float(s[j])) for j in np.lexsort((np.arange(len(ids)), -s.astype(np.float64)))]


# ------------------------------------------------------------------------------------------------ retriever.py ---
BOUNDS = (0, 20, 55, 70)
QIDS = [f"q{q}" for q in range(5)]


def _corpus():
    """six decks of five near-identical pages and forty one-page documents: tests/test_cpu_group_window_search_ref.py::_base"""
    D, _ = R.decks(6, 5, DIM, 0.05)
    C = np.concatenate([D, R.unit(40, DIM, 9)])
    names = [f"deck_{d}.pdf_{i}.png" for d in range(6) for i in range(5)] + [f"other_{j}.pdf_0.png" for j in range(40)]
    return C, names


@pytest.fixture
def shards(tmp_path):
    """70 pages shuffled into three shards of 20, 35 and 15 rows, an EMPTY shard between them, five queries
    -> (args, C in shard order, page ids in shard order, Q)"""
    C, names = _corpus()
    perm = np.random.default_rng(3).permutation(len(C))                   # pages of a document are neither adjacent nor in one shard
    Cp, pids = C[perm], [names[i] for i in perm]
    for s, rank in enumerate((0, 2, 3)):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{rank}"), Cp[BOUNDS[s]:BOUNDS[s + 1]], pids[BOUNDS[s]:BOUNDS[s + 1]])
    write_shard(str(tmp_path / "embeddings.corpus.rank.1"), np.zeros((0, DIM), np.float32), [])
    Q = R.unit(5, DIM, 42)
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, QIDS)
    HostIndex.fresh()
    return types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0"), Cp, pids, Q


def _label(pid):
    return "decks" if pid.startswith("deck") else ("odd" if int(pid.split("_")[1].split(".")[0]) % 2 else "even")


def test_retrieve_filtered(shards):
    args, C, pids, Q = shards
    wanted = {"q0": None, "q1": {"decks"}, "q2": {"odd", "decks"}, "q3": {"none-such"}, "q4": {"decks"}}
    res = retriever.retrieve_filtered(args, 7, _label, lambda q: wanted[q], index_factory=HostIndex)
    # ONE index over all shards, one filter per DISTINCT label set (q1 and q4 share one), closed once
    assert HostIndex.calls == [("add", 70, "float32"), ("set_filters", 4), ("search_filtered", 7)]
    assert len(HostIndex.made) == 1 and HostIndex.made[0].closed == 1 and HostIndex.made[0].capacity == 70
    for qi, q in enumerate(QIDS):
        ids = [i for i in range(70) if wanted[q] is None or _label(pids[i]) in wanted[q]]
        want = brute(Q[qi], C, ids)[:7]
        assert list(res[q].items()) == [(pids[i], s) for i, s in want], q
    assert res["q3"] == {} and len(res["q1"]) == 7
    HostIndex.fresh()
    assert len(retriever.retrieve_filtered(args, 500, _label, lambda q: None, index_factory=HostIndex)["q0"]) == 70
    assert HostIndex.calls[-1] == ("search_filtered", 70)                # k is cut at the rows
    HostIndex.fresh()
    assert retriever.retrieve_filtered(args, 0, _label, lambda q: None, index_factory=HostIndex) == {q: {} for q in QIDS}
    assert HostIndex.made == []


def test_retrieve_range_takes_one_shard_at_a_time(shards):
    args, C, pids, Q = shards
    res = retriever.retrieve_range(args, 0.1, index_factory=HostIndex)
    t = float(np.float32(0.1))
    per_shard = [("add", n, "float32") for n in (20, 35, 15)]
    assert HostIndex.calls == [c for a in per_shard for c in (a, ("search_range", 0.1, False, True))]      # the empty shard: no index
    assert [ix.capacity for ix in HostIndex.made] == [20, 35, 15] and all(ix.closed == 1 for ix in HostIndex.made)
    assert HostIndex.most_live == 1
    for qi, q in enumerate(QIDS):
        want = [(pids[i], s) for i, s in brute(Q[qi], C) if s >= t]
        assert list(res[q].items()) == want and len(want) > 1, q
    cut = retriever.retrieve_range(args, 0.1, max_per_query=2, index_factory=HostIndex)
    assert all(list(cut[q].items()) == list(res[q].items())[:2] for q in QIDS)
    assert retriever.retrieve_range(args, 0.1, max_per_query=-3, index_factory=HostIndex) == {q: {} for q in QIDS}
    assert retriever.retrieve_range(args, 2.0, index_factory=HostIndex) == {q: {} for q in QIDS}


def test_rank_rows_adds_counts_over_shards(shards):
    args, C, pids, Q = shards
    targets = {"q0": [pids[3], pids[60], pids[3]], "q1": [pids[25]], "q3": [pids[69], pids[0], pids[30]]}      # q2, q4: none
    res = retriever.rank_rows(args, targets, index_factory=HostIndex)
    assert HostIndex.most_live == 1 and all(ix.closed == 1 for ix in HostIndex.made)
    assert all(c[2] == "float32" for c in HostIndex.calls if c[0] == "add")
    # pass 1: the three shards that hold a target; pass 2: each shard once, for the targets of the other shards
    # (the targets lie in the shards of 20, 35 and 15 rows: 2, 2 and 2 of the 6 pairs)
    assert [c for c in HostIndex.names() if c != "add"] == ["rank_rows"] * 3 + ["count_range"] * 4
    assert [(c[1], c[2]) for c in HostIndex.calls if c[0] == "count_range"] == [(4, False), (2, False), (2, True), (4, True)]
    assert [ix.capacity for ix in HostIndex.made] == [20, 35, 15] * 2
    for qi, q in enumerate(QIDS):
        order = [i for i, _ in brute(Q[qi], C)]
        want = {d: (float(R.scores64(Q[qi:qi + 1], C[pids.index(d):pids.index(d) + 1]).astype(np.float32)[0, 0]), order.index(pids.index(d)))
                for d in dict.fromkeys(targets.get(q, ()))}
        assert res[q] == want and list(res[q]) == list(want), q
    assert res["q0"][pids[3]][1] != res["q0"][pids[60]][1] and res["q2"] == {}
    assert retriever.rank_rows(args, lambda q: [pids[11]], index_factory=HostIndex)["q4"][pids[11]][1] == [i for i, _ in brute(Q[4], C)].index(11)
    with pytest.raises(ValueError, match="no such document in the corpus shards: nowhere"):
        retriever.rank_rows(args, {"q1": [pids[2], "nowhere"]}, index_factory=HostIndex)
    HostIndex.fresh()
    assert retriever.rank_rows(args, {}, index_factory=HostIndex) == {q: {} for q in QIDS} and HostIndex.made == []


def test_distributed_parallel_retrieve_union_of_shard_lists_and_global_list(shards):
    args, C, pids, Q = shards
    res = retriever.distributed_parallel_retrieve(args, 4, index_factory=HostIndex)
    assert HostIndex.calls == [c for n in (20, 35, 15) for c in (("add", n, "float32"), ("search", 4))]
    assert [ix.capacity for ix in HostIndex.made] == [20, 35, 15] and all(ix.closed == 1 for ix in HostIndex.made) and HostIndex.most_live == 1
    for qi, q in enumerate(QIDS):
        want = [(pids[i], s) for a, b in zip(BOUNDS, BOUNDS[1:]) for i, s in brute(Q[qi], C, range(a, b))[:4]]
        assert list(res[q].items()) == want and len(want) == 12, q
    HostIndex.fresh()
    res = retriever.distributed_parallel_retrieve(args, 4, global_topk=True, index_factory=HostIndex)
    assert HostIndex.calls == [("add", 20, "float32"), ("add", 35, "float32"), ("add", 15, "float32"), ("search", 4)]
    assert len(HostIndex.made) == 1 and HostIndex.made[0].capacity == 70 and HostIndex.made[0].closed == 1
    for qi, q in enumerate(QIDS):
        assert list(res[q].items()) == [(pids[i], s) for i, s in brute(Q[qi], C)[:4]], q


def test_only_distributed_parallel_retrieve_hands_the_shard_rows_over_as_they_are(tmp_path):
    C, names = _corpus()
    with open(str(tmp_path / "embeddings.corpus.rank.0"), "wb") as f:
        pickle.dump((C.astype(np.float64), names), f, protocol=4)
    write_shard(str(tmp_path / "embeddings.query.rank.0"), R.unit(2, DIM, 42), ["a", "b"])
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    doc = demo.doc_of_page
    runs = {
        "union": lambda: retriever.distributed_parallel_retrieve(args, 3, index_factory=HostIndex),
        "global": lambda: retriever.distributed_parallel_retrieve(args, 3, global_topk=True, index_factory=HostIndex),
        "documents": lambda: retriever.retrieve_documents(args, 3, doc, index_factory=HostIndex),
        "filtered": lambda: retriever.retrieve_filtered(args, 3, _label, lambda q: None, index_factory=HostIndex),
        "documents_filtered": lambda: retriever.retrieve_documents_filtered(args, 3, doc, _label, lambda q: None, index_factory=HostIndex),
        "rank_documents": lambda: retriever.rank_documents(args, {"a": ["deck_1.pdf"]}, doc, index_factory=HostIndex),
        "documents_range": lambda: retriever.retrieve_documents_range(args, 0.2, doc, index_factory=HostIndex),
        "range": lambda: retriever.retrieve_range(args, 0.2, index_factory=HostIndex),
        "rank_rows": lambda: retriever.rank_rows(args, {"a": [names[4]]}, index_factory=HostIndex),
        "deep": lambda: retriever.retrieve_deep(args, 3, index_factory=HostIndex),
        "fused": lambda: retriever.retrieve_fused(args, lambda q: 0, 3, index_factory=HostIndex),
        "documents_fused": lambda: retriever.retrieve_documents_fused(args, lambda q: 0, 3, doc, index_factory=HostIndex),
        "rrf": lambda: retriever.retrieve_rrf(args, lambda q: 0, 3, depth=5, index_factory=HostIndex,
                                              fuse_lists=lambda ids, lims, k, c, w, dev: rrf_runs(ids, lims, k, c, w)),
        "negatives": lambda: retriever.mine_negatives(args, {}, 1, 3, index_factory=HostIndex),
    }
    for name, run in runs.items():
        HostIndex.fresh()
        run()
        dtypes = {c[2] for c in HostIndex.calls if c[0] == "add"}
        assert dtypes == ({"float64"} if name in ("union", "global") else {"float32"}), name


def _every_entry_point(args):
    doc, one = demo.doc_of_page, lambda q: 0
    return [
        lambda: retriever.distributed_parallel_retrieve(args, 3, index_factory=HostIndex),
        lambda: retriever.distributed_parallel_retrieve(args, 3, global_topk=True, index_factory=HostIndex),
        lambda: retriever.retrieve_documents(args, 3, doc, index_factory=HostIndex),
        lambda: retriever.retrieve_filtered(args, 3, _label, lambda q: None, index_factory=HostIndex),
        lambda: retriever.retrieve_documents_filtered(args, 3, doc, _label, lambda q: None, index_factory=HostIndex),
        lambda: retriever.rank_documents(args, {}, doc, index_factory=HostIndex),
        lambda: retriever.retrieve_documents_range(args, 0.2, doc, index_factory=HostIndex),
        lambda: retriever.retrieve_range(args, 0.2, index_factory=HostIndex),
        lambda: retriever.rank_rows(args, {}, index_factory=HostIndex),
        lambda: retriever.retrieve_deep(args, 3, index_factory=HostIndex),
        lambda: retriever.retrieve_fused(args, one, 3, index_factory=HostIndex),
        lambda: retriever.retrieve_documents_fused(args, one, 3, doc, index_factory=HostIndex),
        lambda: retriever.retrieve_rrf(args, one, 3, index_factory=HostIndex, fuse_lists=lambda *a: None),
        lambda: retriever.mine_negatives(args, {}, 0, 3, index_factory=HostIndex),
    ]


def test_missing_queries_are_reported_before_missing_documents(tmp_path):
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    HostIndex.fresh()
    for run in _every_entry_point(args):                                  # neither queries nor documents
        with pytest.raises(ValueError, match="No pre-computed query embeddings found"):
            run()
    write_shard(str(tmp_path / "embeddings.query.rank.0"), R.unit(2, DIM, 42), ["a", "b"])
    for run in _every_entry_point(args):                                  # queries, no document shard
        with pytest.raises(ValueError, match="No pre-computed document embeddings found"):
            run()
    assert HostIndex.made == []


def test_checks_that_come_before_a_file_is_read(tmp_path):
    nowhere = types.SimpleNamespace(output_dir=str(tmp_path / "nowhere"), process_index=0, device="cuda:0")
    doc = demo.doc_of_page
    with pytest.raises(ValueError, match="offset must be >= 0"):
        retriever.retrieve_documents_filtered(nowhere, 3, doc, _label, lambda q: None, offset=-1, index_factory=HostIndex)
    for lone in ({"label_of_doc": _label}, {"labels_of_query": lambda q: None}):
        with pytest.raises(ValueError, match="label_of_doc and labels_of_query go together"):
            retriever.rank_documents(nowhere, {"a": ["x"]}, doc, index_factory=HostIndex, **lone)
        with pytest.raises(ValueError, match="label_of_doc and labels_of_query go together"):
            retriever.retrieve_documents_range(nowhere, 0.2, doc, index_factory=HostIndex, **lone)
    # mine_negatives looks at start and count only after it has listed the shards
    with pytest.raises(ValueError, match="No pre-computed query embeddings found"):
        retriever.mine_negatives(nowhere, {}, -1, 3, index_factory=HostIndex)
    write_shard(str(tmp_path / "embeddings.query.rank.0"), R.unit(2, DIM, 42), ["a", "b"])
    here = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    with pytest.raises(ValueError, match="No pre-computed document embeddings found"):
        retriever.mine_negatives(here, {}, -1, 3, index_factory=HostIndex)
    write_shard(str(tmp_path / "embeddings.corpus.rank.0"), R.unit(4, DIM, 1), list("wxyz"))
    HostIndex.fresh()
    for start, count in ((-1, 3), (0, -3)):
        with pytest.raises(ValueError, match="start and count must be >= 0"):
            retriever.mine_negatives(here, {}, start, count, index_factory=HostIndex)
    assert HostIndex.made == []


def test_label_arguments_of_the_document_functions(shards):
    args, C, pids, Q = shards
    doc, group = demo.doc_of_page, lambda q: "one" if q in ("q0", "q1") else "two"
    plain = retriever.retrieve_documents_fused(args, group, 5, doc, index_factory=HostIndex)
    assert HostIndex.names() == ["add", "set_groups", "search_multi_groups"] and HostIndex.calls[-1] == ("search_multi_groups", 5, 5, "max", False)
    for lone in ({"label_of_doc": _label}, {"labels_of_group": lambda g: {"decks"}}):      # a lone one is ignored: no filter
        HostIndex.fresh()
        assert retriever.retrieve_documents_fused(args, group, 5, doc, index_factory=HostIndex, **lone) == plain
        assert "set_filters" not in HostIndex.names()
    HostIndex.fresh()
    sc, ev = retriever.retrieve_documents_fused(args, group, 5, doc, label_of_doc=_label, index_factory=HostIndex,
                                                labels_of_group=lambda g: {"decks"} if g == "one" else None)
    assert HostIndex.names() == ["add", "set_groups", "set_filters", "search_multi_groups"] and HostIndex.calls[2] == ("set_filters", 2)
    assert list(sc) == ["one", "two"] and all(d.startswith("deck") for d in sc["one"]) and sc["two"] == plain[0]["two"]
    assert [len(v) for v in ev["one"].values()] == [2] * 5 and [len(v) for v in ev["two"].values()] == [3] * 5
    assert all(doc(p) == d for g in ev for d, pages in ev[g].items() for p in pages)
    # the documents' scores: the best page of the document for the question's best sub-query
    for g, rows in (("one", (0, 1)), ("two", (2, 3, 4))):
        best = {}
        for qi in rows:
            for i, s in brute(Q[qi], C):
                best[doc(pids[i])] = max(best.get(doc(pids[i]), -np.inf), s)
        want = sorted(best.items(), key=lambda e: -e[1])[:5]
        assert sorted(plain[0][g].items(), key=lambda e: -e[1]) == want and list(plain[0][g].values()) == [s for _, s in want]


def test_document_entry_points_build_one_reordered_index(shards, monkeypatch):
    args, C, pids, Q = shards
    doc = demo.doc_of_page
    n_docs = 46
    everything, best_page = retriever.retrieve_documents(args, 500, doc, index_factory=HostIndex)
    assert HostIndex.calls == [("add", 70, "float32"), ("set_groups", n_docs), ("search_groups", n_docs)]
    assert len(HostIndex.made) == 1 and HostIndex.made[0].closed == 1
    for qi, q in enumerate(QIDS):
        best = {}
        for i, s in brute(Q[qi], C):
            best.setdefault(doc(pids[i]), (s, pids[i]))
        want = sorted(best.items(), key=lambda e: -e[1][0])
        assert list(everything[q].items()) == [(d, s) for d, (s, _) in want] and best_page[q] == {d: p for d, (_, p) in want}
    wanted = {"q0": None, "q1": {"decks"}, "q2": {"odd", "decks"}, "q3": {"none-such"}, "q4": {"decks"}}
    # rank_documents: "no targets" before an index is built; with labels one filter per distinct set
    HostIndex.fresh()
    assert retriever.rank_documents(args, {}, doc, index_factory=HostIndex) == {q: {} for q in QIDS} and HostIndex.made == []
    res = retriever.rank_documents(args, {"q1": ["deck_3.pdf", "other_7.pdf"], "q0": ["other_7.pdf"]}, doc, _label, lambda q: wanted[q],
                                   index_factory=HostIndex)
    assert HostIndex.calls == [("add", 70, "float32"), ("set_groups", n_docs), ("set_filters", 4), ("rank_groups", 3, True)]
    assert res["q0"]["other_7.pdf"] == (everything["q0"]["other_7.pdf"], best_page["q0"]["other_7.pdf"], list(everything["q0"]).index("other_7.pdf"))
    assert res["q1"]["other_7.pdf"] == (-np.inf, None, -1) and res["q1"]["deck_3.pdf"][0] == everything["q1"]["deck_3.pdf"]
    assert res["q1"]["deck_3.pdf"][2] == [d for d in everything["q1"] if d.startswith("deck")].index("deck_3.pdf") and res["q2"] == {}
    HostIndex.fresh()
    retriever.rank_documents(args, {"q1": ["deck_3.pdf"]}, doc, index_factory=HostIndex)
    assert HostIndex.calls == [("add", 70, "float32"), ("set_groups", n_docs), ("rank_groups", 1, False)]
    with pytest.raises(ValueError, match="no such document in the corpus shards: nowhere.pdf"):
        retriever.rank_documents(args, {"q1": ["nowhere.pdf"]}, doc, index_factory=HostIndex)
    # retrieve_documents_range: filter only with labels; best first; max_per_query
    HostIndex.fresh()
    sc, pg = retriever.retrieve_documents_range(args, 0.1, doc, index_factory=HostIndex)
    assert HostIndex.calls == [("add", 70, "float32"), ("set_groups", n_docs), ("search_groups_range", 0.1, False)]
    t = float(np.float32(0.1))
    for q in QIDS:
        assert list(sc[q].items()) == [(d, s) for d, s in everything[q].items() if s >= t] and pg[q] == {d: best_page[q][d] for d in sc[q]}
    HostIndex.fresh()
    sc2, _ = retriever.retrieve_documents_range(args, 0.1, doc, _label, lambda q: wanted[q], max_per_query=2, index_factory=HostIndex)
    assert HostIndex.names() == ["add", "set_groups", "set_filters", "search_groups_range"]
    for q in QIDS:
        assert list(sc2[q]) == [d for d in sc[q] if wanted[q] is None or _label(d) in wanted[q]][:2]
    # retrieve_documents_filtered pages in steps of WINDOW_PAGE
    monkeypatch.setattr(retriever, "WINDOW_PAGE", 4)
    HostIndex.fresh()
    sc3, pg3 = retriever.retrieve_documents_filtered(args, 10, doc, _label, lambda q: wanted[q], offset=3, index_factory=HostIndex)
    assert HostIndex.calls == [("add", 70, "float32"), ("set_groups", n_docs), ("set_filters", 4),
                               ("search_groups_window", 3, 4, True), ("search_groups_window", 7, 4, True), ("search_groups_window", 11, 2, True)]
    for q in QIDS:
        want = [d for d in everything[q] if wanted[q] is None or _label(d) in wanted[q]][3:13]
        assert list(sc3[q]) == want and [pg3[q][d] for d in want] == [best_page[q][d] for d in want]


def test_shard_by_shard_entry_points_shift_rows_by_the_shards_before(shards):
    args, C, pids, Q = shards
    group = lambda q: "one" if q in ("q0", "q3") else "two"      # noqa: E731
    deep = retriever.retrieve_deep(args, 30, index_factory=HostIndex)
    assert HostIndex.calls == [c for n, k in ((20, 20), (35, 30), (15, 15)) for c in (("add", n, "float32"), ("search_window", 0, k, False))]
    assert HostIndex.most_live == 1 and all(ix.closed == 1 for ix in HostIndex.made)
    for qi, q in enumerate(QIDS):
        assert list(deep[q].items()) == [(pids[i], s) for i, s in brute(Q[qi], C)[:30]]
    HostIndex.fresh()
    fused = retriever.retrieve_fused(args, group, 6, fuse="min", index_factory=HostIndex)
    assert HostIndex.calls == [c for n in (20, 35, 15) for c in (("add", n, "float32"), ("search_multi", 5, 6, "min", False))]
    assert HostIndex.most_live == 1 and list(fused) == ["one", "two"]
    for g, rows in (("one", (0, 3)), ("two", (1, 2, 4))):
        S = R.scores64(Q[list(rows)], C).astype(np.float32).min(0)
        order = np.lexsort((np.arange(70), -S.astype(np.float64)))[:6]
        assert list(fused[g].items()) == [(pids[i], float(S[i])) for i in order]
    HostIndex.fresh()
    seen = []

    def fuse_lists(ids, lims, k, c, w, dev):
        seen.append((np.asarray(ids).copy(), list(lims), k, c, None if w is None else list(w)))
        return rrf_runs(ids, lims, k, c, w)

    rrf = retriever.retrieve_rrf(args, group, 6, depth=8, c=10.0, weight_of_query=lambda q: 2.0 if q == "q3" else 1.0,
                                 index_factory=HostIndex, fuse_lists=fuse_lists)
    assert HostIndex.calls == [c for n in (20, 35, 15) for c in (("add", n, "float32"), ("search", 8))] and HostIndex.most_live == 1
    (ids, lims, k, c, w), = seen
    assert (lims, k, c, w) == ([0, 2, 5], 6, 10.0, [1.0, 2.0, 1.0, 1.0, 1.0])
    for row, qi in enumerate((0, 3, 1, 2, 4)):                            # the queries in group order, global positions
        assert ids[row].tolist() == [i for i, _ in brute(Q[qi], C)[:8]]
    want = rrf_runs(ids, lims, 6, 10.0, w)
    assert [list(rrf[g].items()) for g in ("one", "two")] == \
        [[(pids[int(j)], float(s)) for s, j in zip(want[0][gi], want[1][gi]) if j >= 0] for gi in range(2)]
    # mine_negatives: several shards -> every row above the window's end, merged
    HostIndex.fresh()
    positives = {"q0": [pids[i] for i, _ in brute(Q[0], C)[2:4]], "q1": ["not in the corpus"]}
    neg = retriever.mine_negatives(args, positives, 2, 5, index_factory=HostIndex)
    assert HostIndex.calls == [c for n, k in ((20, 9), (35, 9), (15, 9)) for c in (("add", n, "float32"), ("search_window", 0, k, False))]
    assert HostIndex.most_live == 1 and all(ix.closed == 1 for ix in HostIndex.made)
    for qi, q in enumerate(QIDS):
        ranking = [pids[i] for i, _ in brute(Q[qi], C)]
        assert neg[q] == [d for d in ranking[2:9] if d not in positives.get(q, ())][:5], q
    assert retriever.mine_negatives(args, {}, 0, 0, index_factory=HostIndex) == {q: [] for q in QIDS}


# ------------------------------------------------------------------------------------------------ demo.py ---
@pytest.fixture
def base(tmp_path):
    """-> (path of an existing, empty directory, C, page names, index holding C, one query embedding)"""
    C, names = _corpus()
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    HostIndex.fresh()
    ix = HostIndex(DIM, len(C))
    ix.add(C)
    HostIndex.calls = []
    return kb, C, names, ix, R.unit(6, DIM, 5)[2:3]


def _paths(kb, names, ranked):
    return [os.path.join(kb, names[i]) for i, _ in ranked], [s for _, s in ranked]


def _rows_of(names, documents):
    return [i for i, n in enumerate(names) if demo.doc_of_page(n) in documents]


DOCS = ["deck_2.pdf", "other_7.pdf", "deck_4.pdf"]


def test_demo_retrieve_plain_documents_offset_diverse(base):
    kb, C, names, ix, q = base
    full = brute(q, C)
    # documents=: one filter, k cut at the allowed rows; an unknown name contributes nothing
    got = demo.retrieve(kb, q, 20, None, None, index=ix, names=names, documents=DOCS + ["nowhere.pdf"], return_scores=True)
    assert HostIndex.calls == [("set_filters", 1), ("search_filtered", 11)]
    assert got == _paths(kb, names, brute(q, C, _rows_of(names, DOCS)))
    HostIndex.calls = []
    assert demo.retrieve(kb, q, 5, None, None, index=ix, names=names, documents=["nowhere.pdf"], return_scores=True) == ([], [])
    assert demo.retrieve(kb, q, 0, None, None, index=ix, names=names, documents=DOCS) == [] and HostIndex.calls == []
    # offset=: the window; with documents through the filter
    assert demo.retrieve(kb, q, 7, None, None, index=ix, names=names, offset=4, return_scores=True) == _paths(kb, names, full[4:11])
    assert HostIndex.calls == [("search_window", 4, 7, False)]
    assert demo.retrieve(kb, q, 7, None, None, index=ix, names=names, offset=66) == _paths(kb, names, full[66:])[0]
    assert HostIndex.calls[-1] == ("search_window", 66, 4, False)
    HostIndex.calls = []
    assert demo.retrieve(kb, q, 7, None, None, index=ix, names=names, offset=70) == [] and HostIndex.calls == []
    got = demo.retrieve(kb, q, 20, None, None, index=ix, names=names, offset=3, documents=DOCS + ["nowhere.pdf"], return_scores=True)
    assert HostIndex.calls == [("set_filters", 1), ("search_window", 3, 8, True)]
    assert got == _paths(kb, names, brute(q, C, _rows_of(names, DOCS))[3:])
    # diverse=: pick order; pool at least k; with documents through the filter
    HostIndex.calls = []
    paths, scores = demo.retrieve(kb, q, 4, None, None, index=ix, names=names, diverse=0.5, pool=2, return_scores=True)
    assert HostIndex.calls == [("search_diverse", 4, 4, 0.5, False)]
    assert paths[0] == os.path.join(kb, names[full[0][0]]) and sorted(paths) == sorted(_paths(kb, names, full[:4])[0])
    assert sorted(scores) == sorted(s for _, s in full[:4])
    HostIndex.calls = []
    paths = demo.retrieve(kb, q, 30, None, None, index=ix, names=names, diverse=1.0, documents=DOCS + ["nowhere.pdf"])
    assert HostIndex.calls == [("set_filters", 1), ("search_diverse", 11, None, 1.0, True)]
    assert paths == _paths(kb, names, brute(q, C, _rows_of(names, DOCS)))[0]      # lambda 1: relevance alone
    with pytest.raises(ValueError, match="exclude each other"):
        demo.retrieve(kb, q, 5, None, None, index=ix, names=names, diverse=0.5, offset=2)
    with pytest.raises(ValueError, match="offset must be >= 0"):
        demo.retrieve(kb, q, 5, None, None, index=ix, names=names, offset=-1)
    assert demo.retrieve(os.path.join(kb, "missing"), q, 5, None, None, offset=-1) is None
    assert ix.closed == 0                                                 # a caller's index stays open


class _Model:
    """encodes a string as a unit vector drawn from its length; counts the calls"""
    encoder = types.SimpleNamespace(device=0)
    asked = []


def _fake_encode(model, tokenizer, texts):
    _Model.asked.append(list(texts))
    return np.concatenate([R.unit(1, DIM, len(t)) for t in texts])


def test_demo_retrieve_plain_loads_and_closes_its_own_index(base, monkeypatch):
    kb, C, names, ix, _ = base
    loads = []
    monkeypatch.setattr(demo, "load_knowledge_base", lambda path, device=None: (loads.append((path, device)), (ix, names))[1])
    monkeypatch.setattr(demo, "encode", _fake_encode)
    _Model.asked = []
    got = demo.retrieve(kb, "what?", 500, _Model, None, return_scores=True)
    assert loads == [(kb, 0)] and ix.closed == 1 and HostIndex.calls == [("search", 70)]
    assert _Model.asked == [[demo.QUERY_INSTRUCTION + "what?"]]
    assert got == _paths(kb, names, brute(R.unit(1, DIM, len(demo.QUERY_INSTRUCTION + "what?")), C))
    for kw in ({"documents": DOCS}, {"offset": 2}, {"diverse": 0.3}, {"documents": DOCS, "offset": 2}):
        demo.retrieve(kb, "what?", 5, _Model, None, **kw)
    assert len(loads) == 5 and ix.closed == 5


def test_demo_retrieve_any_and_rrf(base, monkeypatch):
    kb, C, names, ix, _ = base
    Qs = R.unit(3, DIM, 11)
    F = R.scores64(Qs, C).astype(np.float32)
    paths, scores, deciding = demo.retrieve_any(kb, Qs, 6, None, None, index=ix, names=names, return_scores=True)
    assert HostIndex.calls == [("search_multi", 3, 6, "max", False)]
    order = np.lexsort((np.arange(70), -F.max(0).astype(np.float64)))[:6]
    assert paths == [os.path.join(kb, names[i]) for i in order] and scores == [float(F.max(0)[i]) for i in order]
    assert deciding == [int(F[:, i].argmax()) for i in order]
    HostIndex.calls = []
    paths = demo.retrieve_any(kb, Qs, 500, None, None, index=ix, names=names, fuse="min", documents=DOCS + ["nowhere.pdf"])
    assert HostIndex.calls == [("set_filters", 1), ("search_multi", 3, 11, "min", True)]      # min(topk, rows, 1000)
    rows = np.asarray(_rows_of(names, DOCS))
    assert paths == [os.path.join(kb, names[i]) for i in rows[np.lexsort((rows, -F.min(0)[rows].astype(np.float64)))]]
    HostIndex.calls = []
    assert demo.retrieve_any(kb, Qs, 5, None, None, index=ix, names=names, documents=["nowhere.pdf"], return_scores=True) == ([], [], [])
    assert demo.retrieve_any(kb, Qs[:0], 5, None, None, index=ix, names=names) == [] and HostIndex.calls == []
    paths, scores, hits = demo.retrieve_rrf(kb, Qs, 500, None, None, index=ix, names=names, depth=7, c=20.0, weights=[1, 2, 1], return_scores=True)
    assert HostIndex.calls == [("search_rrf", 3, 70, 7, 20.0, False)]
    lists = np.asarray([[i for i, _ in brute(Qs[j], C)[:7]] for j in range(3)])
    sc, ids, h = rrf_runs(lists, [0, 3], 70, 20.0, [1, 2, 1])
    keep = [int(i) for i in ids[0] if i >= 0]
    assert paths == [os.path.join(kb, names[i]) for i in keep] and scores == [float(s) for s in sc[0][:len(keep)]]
    assert hits == [int(x) for x in h[0][:len(keep)]] and 7 <= len(keep) <= 21
    HostIndex.calls = []
    demo.retrieve_rrf(kb, Qs, 500, None, None, index=ix, names=names, documents=DOCS + ["nowhere.pdf"])
    assert HostIndex.calls == [("set_filters", 1), ("search_rrf", 3, 11, 100, 60.0, True)]
    assert demo.retrieve_rrf(kb, Qs, 5, None, None, index=ix, names=names, documents=["nowhere.pdf"]) == []
    # strings are encoded with the instruction in front; an index of its own is loaded and closed
    monkeypatch.setattr(demo, "load_knowledge_base", lambda path, device=None: (ix, names))
    monkeypatch.setattr(demo, "encode", _fake_encode)
    _Model.asked = []
    demo.retrieve_any(kb, ["a", "bb"], 3, _Model, None)
    demo.retrieve_rrf(kb, ("a", "bb"), 3, _Model, None)
    assert _Model.asked == [[demo.QUERY_INSTRUCTION + "a", demo.QUERY_INSTRUCTION + "bb"]] * 2 and ix.closed == 2
    assert demo.retrieve_any(os.path.join(kb, "missing"), Qs, 5, None, None) is None
    assert demo.retrieve_rrf(os.path.join(kb, "missing"), Qs, 5, None, None) is None


def test_demo_retrieve_above(base):
    kb, C, names, ix, q = base
    full = brute(q, C)
    t = float(np.float32(0.05))
    above = [(i, s) for i, s in full if s >= t]
    assert demo.retrieve_above(kb, q, 0.05, None, None, index=ix, names=names, return_scores=True) == _paths(kb, names, above)
    assert HostIndex.calls == [("search_range", 0.05, False, True)] and len(above) > 3
    assert demo.retrieve_above(kb, q, 0.05, None, None, index=ix, names=names, max_pages=3) == _paths(kb, names, above[:3])[0]
    HostIndex.calls = []
    got = demo.retrieve_above(kb, q[0], -1.0, None, None, index=ix, names=names, documents=DOCS + ["nowhere.pdf"], return_scores=True)
    assert HostIndex.calls == [("set_filters", 1), ("search_range", -1.0, True, True)]
    assert got == _paths(kb, names, brute(q, C, _rows_of(names, DOCS)))
    HostIndex.calls = []
    assert demo.retrieve_above(kb, q, -1.0, None, None, index=ix, names=names, documents=["nowhere.pdf"], return_scores=True) == ([], [])
    assert demo.retrieve_above(kb, q, -1.0, None, None, index=ix, names=names, max_pages=0) == [] and HostIndex.calls == []
    assert demo.retrieve_above(os.path.join(kb, "missing"), q, 0.0, None, None) is None


def test_demo_explain(base, monkeypatch):
    kb, C, names, ix, q = base
    order = [i for i, _ in brute(q, C)]
    pages = [names[40], names[3], names[40]]
    got = demo.explain(kb, q, pages, index=ix, names=names)
    assert HostIndex.calls == [("rank_rows", 3, False)]
    assert got == [(float(R.scores64(q, C[i:i + 1]).astype(np.float32)[0, 0]), order.index(i)) for i in (40, 3, 40)]
    assert demo.explain(kb, q, names[3], index=ix, names=names) == got[1]
    HostIndex.calls = []
    inside = demo.explain(kb, q, [names[12], names[3]], documents=DOCS + ["nowhere.pdf"], index=ix, names=names)      # an unknown document: ignored
    assert HostIndex.calls == [("set_filters", 1), ("rank_rows", 2, True)]
    among = [i for i, _ in brute(q, C, _rows_of(names, DOCS))]
    assert inside[0][1] == among.index(12) and inside[1] == (got[1][0], sum(order.index(i) < order.index(3) for i in among))
    HostIndex.calls = []
    assert demo.explain(kb, q, [], index=ix, names=names) == [] and HostIndex.calls == []
    with pytest.raises(ValueError, match="no such page in .*: nowhere.png"):
        demo.explain(kb, q, [names[3], "nowhere.png"], index=ix, names=names)
    assert ix.closed == 0 and demo.explain(os.path.join(kb, "missing"), q, pages) is None
    monkeypatch.setattr(demo, "load_knowledge_base", lambda path, device=None: (ix, names))
    with pytest.raises(ValueError, match="no such page"):
        demo.explain(kb, q, "nowhere.png")
    assert ix.closed == 1                                                 # its own index: closed on the way out
    assert demo.explain(kb, q, names[3]) == got[1] and ix.closed == 2


def test_demo_duplicate_pages(base, monkeypatch):
    kb, C, names, ix, _ = base
    np.save(os.path.join(kb, "reps.npy"), C)
    groups = demo.duplicate_pages(kb, 0.8, index=ix, names=names, batch=32)
    assert HostIndex.calls == [("search_range", 0.8, False, False)] * 3      # 70 rows, 32 per call, unsorted
    assert groups == [[f"deck_{d}.pdf_{i}.png" for i in range(5)] for d in range(6)]
    assert demo.duplicate_pages(kb, 1.5, index=ix, names=names) == []
    np.save(os.path.join(kb, "reps.npy"), C[:69])
    with pytest.raises(ValueError, match="69 rows in .* but 70 in the index"):
        demo.duplicate_pages(kb, 0.8, index=ix, names=names)
    assert ix.closed == 0 and demo.duplicate_pages(os.path.join(kb, "missing"), 0.8) is None
    np.save(os.path.join(kb, "reps.npy"), C)
    monkeypatch.setattr(demo, "load_knowledge_base", lambda path, device=None: (ix, names))
    assert demo.duplicate_pages(kb, 0.8) == groups and ix.closed == 1


def test_unknown_documents_page_functions_ignore_them_document_functions_raise(base):
    kb, C, names, ix, q = base
    Qs = R.unit(2, DIM, 11)
    two = ["deck_1.pdf", "nowhere.pdf", "neither.pdf"]
    # page level: an unknown name contributes nothing
    assert len(demo.retrieve(kb, q, 9, None, None, index=ix, names=names, documents=two)) == 5
    assert len(demo.retrieve(kb, q, 9, None, None, index=ix, names=names, documents=two, offset=1)) == 4
    assert len(demo.retrieve(kb, q, 9, None, None, index=ix, names=names, documents=two, diverse=0.5)) == 5
    assert len(demo.retrieve_any(kb, Qs, 9, None, None, index=ix, names=names, documents=two)) == 5
    assert len(demo.retrieve_rrf(kb, Qs, 9, None, None, index=ix, names=names, documents=two)) == 5
    assert len(demo.retrieve_above(kb, q, -1.0, None, None, index=ix, names=names, documents=two)) == 5
    assert len(demo.explain(kb, q, [names[7]], documents=two, index=ix, names=names)) == 1
    # document level: ValueError that names the first in sorted order and counts the others
    message = "no page of the base belongs to 'neither.pdf' \\(and 1 more\\)"
    with pytest.raises(ValueError, match=message):
        demo.retrieve_documents(kb, q, 9, None, None, index=ix, names=names, documents=two)
    with pytest.raises(ValueError, match=message):
        demo.retrieve_documents_any(kb, Qs, 9, None, None, index=ix, names=names, documents=two)
    with pytest.raises(ValueError, match=message):
        demo.retrieve_documents_above(kb, q, -1.0, None, None, index=ix, names=names, documents=two)
    with pytest.raises(ValueError, match="no page of the base belongs to 'nowhere.pdf'$"):
        demo.retrieve_documents(kb, q, 9, None, None, index=ix, names=names, documents=["nowhere.pdf"], offset=2)
    # explain_documents: its own message — the first in the caller's order, wanted before documents, no count
    with pytest.raises(ValueError, match="no page of the base belongs to 'nowhere.pdf'$"):
        demo.explain_documents(kb, q, ["deck_1.pdf"], documents=two, index=ix, names=names)
    with pytest.raises(ValueError, match="no page of the base belongs to 'zzz.pdf'$"):
        demo.explain_documents(kb, q, ["zzz.pdf", "aaa.pdf"], documents=two, index=ix, names=names)
    assert ix.closed == 0


def test_when_the_groups_are_set_from_the_names(base):
    kb, C, names, ix, q = base
    Qs = R.unit(2, DIM, 11)
    empty = HostIndex(DIM, 1)
    # an empty index without groups: retrieve_documents_above leaves it alone, retrieve_documents / _any set (zero) groups
    assert demo.retrieve_documents_above(kb, q, 0.0, None, None, index=empty, names=[]) == [] and HostIndex.calls == []
    assert demo.retrieve_documents(kb, q, 3, None, None, index=empty, names=[]) == [] and HostIndex.calls == [("set_groups", 0)]
    assert demo.retrieve_documents_any(kb, Qs, 3, None, None, index=empty, names=[]) == [] and HostIndex.calls == [("set_groups", 0)] * 2
    assert demo.explain_documents(kb, q, [], index=empty, names=[]) == [] and len(HostIndex.calls) == 2
    # explain_documents checks the names before it sets the groups
    with pytest.raises(ValueError, match="no page of the base belongs to"):
        demo.explain_documents(kb, q, ["nowhere.pdf"], index=ix, names=names)
    assert ix.n_groups == 0 and len(HostIndex.calls) == 2
    # the others set the groups, then check
    with pytest.raises(ValueError, match="no page of the base belongs to"):
        demo.retrieve_documents_above(kb, q, 0.0, None, None, index=ix, names=names, documents=["nowhere.pdf"])
    assert ix.n_groups == 46 and HostIndex.calls[2:] == [("set_groups", 46)]
    # groups that are set are left alone; rows that are not adjacent per document raise
    HostIndex.calls = []
    full = demo.retrieve_documents(kb, q, 0, None, None, index=ix, names=names, return_scores=True)
    assert full == ([], []) and HostIndex.calls == [("search_groups", 1)]      # max(1, min(topk, n_groups)), then [:topk]
    HostIndex.calls = []
    got = demo.explain_documents(kb, q, ["deck_2.pdf", "other_7.pdf"], documents=DOCS, index=ix, names=names)
    assert HostIndex.calls == [("set_filters", 1), ("rank_groups", 2, True)]
    ranked = demo.retrieve_documents(kb, q, 46, None, None, index=ix, names=names, documents=DOCS, return_scores=True)
    for (s, page, rank), d in zip(got, ("deck_2.pdf", "other_7.pdf")):
        assert ranked[0][rank] == os.path.join(kb, page) and ranked[1][rank] == s and demo.doc_of_page(page) == d
    assert demo.explain_documents(kb, q, "other_3.pdf", documents=DOCS, index=ix, names=names) == (-np.inf, None, -1)
    mixed = HostIndex(DIM, 70)
    mixed.add(C[::-1][np.r_[0:45, 46:70, 45]])
    bad = [names[::-1][i] for i in np.r_[0:45, 46:70, 45]]                # a deck's page away from its deck
    for call in (lambda: demo.retrieve_documents(kb, q, 3, None, None, index=mixed, names=bad),
                 lambda: demo.retrieve_documents_any(kb, Qs, 3, None, None, index=mixed, names=bad),
                 lambda: demo.retrieve_documents_above(kb, q, 0.0, None, None, index=mixed, names=bad),
                 lambda: demo.explain_documents(kb, q, ["deck_0.pdf"], index=mixed, names=bad)):
        with pytest.raises(ValueError, match="not adjacent in this index"):
            call()


def test_demo_document_functions_against_the_page_ranking(base, monkeypatch):
    kb, C, names, ix, q = base
    best = {}
    for i, s in brute(q, C):
        best.setdefault(demo.doc_of_page(names[i]), (i, s))
    ranked = sorted(best.values(), key=lambda e: -e[1])
    assert demo.retrieve_documents(kb, q, 5, None, None, index=ix, names=names, return_scores=True) == _paths(kb, names, ranked[:5])
    assert HostIndex.calls == [("set_groups", 46), ("search_groups", 5)]
    t = float(np.float32(0.05))
    HostIndex.calls = []
    assert demo.retrieve_documents_above(kb, q, 0.05, None, None, index=ix, names=names, return_scores=True) == \
        _paths(kb, names, [e for e in ranked if e[1] >= t])
    assert demo.retrieve_documents_above(kb, q, 0.05, None, None, index=ix, names=names, max_documents=2) == _paths(kb, names, ranked[:2])[0]
    assert demo.retrieve_documents_above(kb, q, 0.05, None, None, index=ix, names=names, max_documents=0) == []
    assert HostIndex.calls == [("search_groups_range", 0.05, False)] * 2
    HostIndex.calls = []
    got = demo.retrieve_documents_above(kb, q, -1.0, None, None, index=ix, names=names, documents=DOCS, return_scores=True)
    assert HostIndex.calls == [("set_filters", 1), ("search_groups_range", -1.0, True)]
    assert got == _paths(kb, names, [e for e in ranked if demo.doc_of_page(names[e[0]]) in DOCS])
    Qs = R.unit(2, DIM, 11)
    HostIndex.calls = []
    paths, scores, evidence = demo.retrieve_documents_any(kb, Qs, 500, None, None, index=ix, names=names, documents=DOCS, return_evidence=True)
    assert HostIndex.calls == [("set_filters", 1), ("search_multi_groups", 2, 3, "max", True)]      # min(topk, documents named, 1000)
    assert len(paths) == 3 and scores == sorted(scores, reverse=True) and [len(e) for e in evidence] == [2, 2, 2]
    for p, s, ev in zip(paths, scores, evidence):
        assert s == max(v for _, v in ev) and p in [x for x, _ in ev]
        assert len({demo.doc_of_page(os.path.basename(x)) for x, _ in ev} | {demo.doc_of_page(os.path.basename(p))}) == 1
    HostIndex.calls = []
    assert len(demo.retrieve_documents_any(kb, Qs, 4, None, None, index=ix, names=names, fuse="min")) == 4
    assert HostIndex.calls == [("search_multi_groups", 2, 4, "min", False)]
    # their own index: a document base, loaded and closed
    loads = []
    monkeypatch.setattr(demo, "load_document_base", lambda path, device=None: (loads.append(path), (ix, names))[1])
    monkeypatch.setattr(demo, "load_knowledge_base", lambda path, device=None: pytest.fail("a page base for a document function"))
    demo.retrieve_documents(kb, q, 5, None, None)
    demo.retrieve_documents(kb, q, 5, None, None, documents=DOCS, offset=1)
    demo.retrieve_documents_any(kb, Qs, 5, None, None)
    demo.retrieve_documents_above(kb, q, 0.0, None, None)
    demo.explain_documents(kb, q, "deck_1.pdf")
    assert loads == [kb] * 5 and ix.closed == 5


def test_demo_pages_in_steps_of_a_thousand(tmp_path):
    kb = str(tmp_path)
    C = R.unit(1100, DIM, 21)
    names = [f"doc_{i}.pdf_0.png" for i in range(1100)]
    HostIndex.fresh()
    ix = HostIndex(DIM, 1100)
    ix.add(C)
    q = R.unit(1, DIM, 22)
    HostIndex.calls = []
    paths = demo.retrieve(kb, q, 1050, None, None, index=ix, names=names, offset=5)
    assert HostIndex.calls == [("search_window", 5, 1000, False), ("search_window", 1005, 50, False)]
    assert paths == _paths(kb, names, brute(q, C)[5:1055])[0]
    HostIndex.calls = []
    docs = demo.retrieve_documents(kb, q, 1200, None, None, index=ix, names=names, offset=50)
    assert HostIndex.calls == [("set_groups", 1100), ("search_groups_window", 50, 1000, False), ("search_groups_window", 1050, 50, False)]
    assert docs == _paths(kb, names, brute(q, C)[50:])[0]
    HostIndex.calls = []
    assert len(demo.retrieve_any(kb, q, 5000, None, None, index=ix, names=names)) == 1000
    assert len(demo.retrieve_rrf(kb, q, 5000, None, None, index=ix, names=names, depth=3)) == 3
    assert HostIndex.calls == [("search_multi", 1, 1000, "max", False), ("search_rrf", 1, 1000, 3, 60.0, False)]


# ------------------------------------------------------------------------------------------------ close on error ---
def test_an_index_the_call_opened_is_closed_when_the_call_raises(base, monkeypatch):
    kb, C, names, ix, q = base
    loads = []
    monkeypatch.setattr(demo, "load_document_base", lambda path, device=None: (loads.append(path), (ix, names))[1])
    with pytest.raises(ValueError, match="no page of the base belongs to 'nowhere.pdf'"):
        demo.retrieve_documents_above(kb, q, 0.0, None, None, documents=["nowhere.pdf"])
    assert loads == [kb] and ix.closed == 1


def test_a_negative_offset_raises_before_anything_is_loaded(base, monkeypatch):
    kb, C, names, ix, q = base
    loads = []
    monkeypatch.setattr(demo, "load_knowledge_base", lambda path, device=None: (loads.append(path), (ix, names))[1])
    monkeypatch.setattr(demo, "load_document_base", lambda path, device=None: (loads.append(path), (ix, names))[1])
    with pytest.raises(ValueError, match="offset must be >= 0"):
        demo.retrieve(kb, q, 5, None, None, documents=DOCS, offset=-1)
    assert loads == [] and ix.closed == 0
