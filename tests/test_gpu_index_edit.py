"""-m gpu: the index edited in place (vr_index_remove / vr_index_update / vr_index_get_rows, csrc/index_edit.hip and index_rows.hip)
against the numpy model tests/index_edit_ref.py.

One bar, no tolerance: the edited index E and a FRESH index F — a new HipIndex, `add` of the model's rows, the model's compacted
filters set, default certification — agree bit for bit: the stored rows (fp32 and the bf16 copy, which also equal the model's
array and its round-to-nearest-even), `error_model()`, `len()`, `search_plan()`, and the scores (as uint32), ids, groups and lims
of `search` (k = 10: the fused sweep, k = 100: the deep path), `search_filtered`, `search_range` (thresholds: F's own 30th score),
`search_diverse` and `search_groups`.  Every score the library returns is one fp32 dot product in one summation order and every id
list is the fp32 ranking with a deterministic tie rule, so two indices that hold the same rows have nothing to differ in."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import group_search_ref as R  # noqa: E402
from tests import index_edit_ref as M  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.documents import compact_filters, doc_of_page, remap_rows  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

VR_OK, VR_ERR_INVALID, VR_ERR_STATE, VR_ERR_CAPACITY = 0, 1, 3, 4


def _np(*xs):
    return [x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in xs]


def _bits(got):
    """a search's outputs with the float arrays as their bits"""
    return [a.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist() for a in _np(*got)]


def _edited(rows, masks=None, capacity=None):
    ix = HipIndex(rows.shape[1], capacity or len(rows))
    ix.add(rows[: len(rows) // 2]); ix.add(rows[len(rows) // 2:])
    if masks is not None:
        ix.set_filters(masks)
    return ix


def _fresh(model):
    ix = HipIndex(model.rows.shape[1], max(len(model), 1))
    if len(model):
        ix.add(model.rows)
        if model.masks is not None:
            ix.set_filters(model.masks)
    return ix


def _stored_rows_equal(E, F, model):
    rows, rows_f = E.rows(), F.rows()
    assert rows.dtype == np.float32 and rows.shape == model.rows.shape
    assert np.array_equal(rows.view(np.uint32), model.rows.view(np.uint32))
    assert np.array_equal(rows.view(np.uint32), rows_f.view(np.uint32))
    b, b_f = E.rows(bf16=True), F.rows(bf16=True)
    assert b.dtype == np.uint16 and np.array_equal(b, b_f)
    want = torch.from_numpy(model.rows).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(b, want)


def _error_model_bits(ix):
    return {k: np.float32(v).view(np.uint32) for k, v in ix.error_model().items()}


def _same(E, model, Q, full=True):
    """the bar of the module docstring; -> F's top-10 (scores, ids)"""
    F = _fresh(model)
    try:
        n, nq = len(model), len(Q)
        assert len(E) == n == len(F)
        assert _error_model_bits(E) == _error_model_bits(F)
        assert E.search_plan(nq) == F.search_plan(nq)
        if n:
            _stored_rows_equal(E, F, model)
        top = F.search(Q, 10)
        assert _bits(E.search(Q, 10)) == _bits(top)
        if n == 0:
            assert np.isneginf(top[0]).all() and (top[1] == -1).all()
            lims = E.search_range(Q, 0.0)[0]
            assert lims.tolist() == [0] * (nq + 1)
            return top
        assert (top[1] < n).all()
        if not full:
            return top
        assert _bits(E.search(Q, 100)) == _bits(F.search(Q, 100))
        if model.masks is not None:
            assert E.n_filters == F.n_filters == len(model.masks)
            foq = (np.arange(nq) % (len(model.masks) + 1)) - 1             # -1, 0, 1, ... cycling over the queries
            assert _bits(E.search_filtered(Q, 10, foq)) == _bits(F.search_filtered(Q, 10, foq))
        k30 = min(30, n)
        thr = F.search(Q, k30)[0][:, k30 - 1].copy()                       # F's own 30th score: 30 rows or a few more per query
        got, want = E.search_range(Q, thr), F.search_range(Q, thr)
        assert _bits(got) == _bits(want) and int(want[0][-1]) >= nq * k30
        assert _bits(E.search_diverse(Q, 5, 20)) == _bits(F.search_diverse(Q, 5, 20))
        off = np.concatenate([np.arange(0, n, 7), [n]]).astype(np.int64)
        E.set_groups(off); F.set_groups(off)
        assert _bits(E.search_groups(Q, 5)) == _bits(F.search_groups(Q, 5))
        return top
    finally:
        F.close()


def _masks(n, seed=4):
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(n) < 0.5, rng.random(n) < 0.01, np.ones(n, dtype=bool)])


def _queries(rows, dim, extra=()):
    """16 queries: random unit vectors, a few of the rows themselves, and `extra`"""
    q = [R.unit(12, dim, 2), rows[[0, len(rows) // 2, len(rows) - 1]], rows[len(rows) // 3: len(rows) // 3 + 1]]
    return np.ascontiguousarray(np.concatenate(q + [np.asarray(e, np.float32) for e in extra]), dtype=np.float32)


# --------------------------------------------------------------------------------------------- the worst overlap ---
def test_remove_row_0_of_a_store_of_several_chunks():
    """20000 x 2304: 184 MB of fp32 rows, three chunks of the 64 MiB scratch.  Row 0 alone: every row moves down by one — each
    row written is the source of the row before it.  The last row alone: nothing moves.  A block of 2000 rows near the front:
    from there on a window's source lies wholly behind it, and the rows move without scratch."""
    rows = R.unit(20000, 2304, 1)
    model = M.Model(rows, _masks(len(rows)))
    E = _edited(rows, model.masks)
    Q = _queries(rows, 2304)
    nid = E.remove([0])
    assert np.array_equal(nid, model.remove([0])) and E.n_groups == 0 and E.n_filters == 3
    top = _same(E, model, Q)
    assert np.array_equal(Q[12], rows[0]) and top[0][12, 0] < 0.9           # the query that WAS row 0 finds no copy of itself
    last = len(model) - 1
    assert np.array_equal(E.remove([last]), model.remove([last]))
    _same(E, model, Q, full=False)
    block = np.arange(100, 2100)
    assert np.array_equal(E.remove(block), model.remove(block))
    _same(E, model, Q, full=False)
    E.close()


# ----------------------------------------------------------------------------------------------------- patterns ---
SHAPES = [(3001, 128), (5000, 256), (1000, 192)]


def _pattern(name, n):
    rng = np.random.default_rng(11)
    if name == "block":
        return np.arange(250, min(1290, n - 5))             # crosses 256-row tiles and 32-bit filter words
    if name == "random30":
        return rng.choice(n, size=int(0.3 * n), replace=False)
    if name == "every_other":
        return np.arange(0, n, 2)
    if name == "all_but_one":
        return np.delete(np.arange(n), n // 3)
    if name == "all":
        return np.arange(n)
    if name == "unsorted_duplicates":
        ids = rng.choice(n, size=n // 5, replace=False)
        return rng.permutation(np.concatenate([ids, ids[: len(ids) // 2], ids[:3]]))
    raise KeyError(name)


@pytest.mark.parametrize("name", ["block", "random30", "every_other", "all_but_one", "all", "unsorted_duplicates"])
@pytest.mark.parametrize("n,dim", SHAPES)
def test_remove_patterns(n, dim, name):
    rows = R.unit(n, dim, 1)
    model = M.Model(rows, _masks(n))
    E = _edited(rows, model.masks)
    E.set_groups([0, n // 2, n])
    ids = _pattern(name, n)
    Q = _queries(rows, dim, extra=[rows[ids[:2]]])           # two of the removed rows ask for themselves
    removed = ctypes.c_int64(-1)
    a = np.ascontiguousarray(ids, dtype=np.int64)
    assert _lib.load().vr_index_remove(E._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(a), ctypes.byref(removed),
                                       ctypes.c_void_p(_stream_ptr(0))) == VR_OK
    assert removed.value == len(np.unique(ids))              # duplicates count once
    nid = model.remove(ids)
    assert len(E) == n - removed.value == len(model)
    assert np.array_equal(compact_filters(_masks(n), nid), model.masks)
    _same(E, model, Q)
    E.close()


def test_stale_tail_is_never_returned():
    """the removed rows sat at the END of the store: their data is still behind the last row, and they are the queries"""
    n, dim = 3001, 128
    rows = R.unit(n, dim, 1)
    model = M.Model(rows, _masks(n))
    E = _edited(rows, model.masks)
    gone = np.arange(n - 300, n)
    E.remove(gone); model.remove(gone)
    Q = np.ascontiguousarray(rows[gone[::19]])               # 16 of them
    top = _same(E, model, Q)
    assert (top[1] >= 0).all() and (top[1] < n - 300).all() and (top[0][:, 0] < 0.9).all()   # nothing scores like a copy of the query
    for k in (1, 10, 100):
        sc, ids = E.search(Q, k)
        assert (ids >= 0).all() and (ids < n - 300).all()
    E.close()


# ------------------------------------------------------------------------------------------------------ filters ---
def test_filters_are_carried_and_a_filter_may_end_up_empty():
    n, dim = 3001, 128
    rows = R.unit(n, dim, 1)
    masks = _masks(n)
    model = M.Model(rows, masks)
    E = _edited(rows, masks)
    sparse = np.nonzero(masks[1])[0]
    assert 10 <= len(sparse) <= 60
    ids = np.concatenate([sparse, np.arange(40, 75)])         # every row filter 1 allows, and a run across a filter word
    nid = E.remove(ids)
    assert np.array_equal(nid, model.remove(ids)) and not model.masks[1].any() and E.n_filters == 3
    Q = _queries(rows, dim)
    sc, got = E.search_filtered(Q, 10, 1)                     # no new set_filters: the filters came along
    assert np.isneginf(sc).all() and (got == -1).all()
    before = E.filter_search_stats()
    _same(E, model, Q)
    after = E.filter_search_stats()
    assert sum(after.values()) > sum(before.values())          # the counters still answer, and count
    kept = np.setdiff1d(np.arange(n), ids)[[5, 50, -1]]
    held = np.array([kept[0], sparse[0], kept[2], 41, kept[1]], dtype=np.int64)
    assert remap_rows(nid, held).tolist() == [int(nid[kept[0]]), int(nid[kept[2]]), int(nid[kept[1]])]
    E.close()


# -------------------------------------------------------------------------------------------------------- state ---
def _status(fn, *args):
    return int(fn(*args))


def test_state_after_remove():
    n, dim = 1000, 64
    rows = R.unit(n, dim, 1)
    E = _edited(rows, _masks(n))
    lib = _lib.load()
    Q = np.ascontiguousarray(R.unit(4, dim, 2))
    E.set_groups([0, 500, n])
    lims, _, _ = E.search_range(Q, 0.3)
    sc, ids = np.empty(1, np.float32), np.empty(1, np.int64)
    stream = ctypes.c_void_p(_stream_ptr(0))
    assert _status(lib.vr_index_range_results, E._h, ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(ids.ctypes.data), 0, 0, stream) == VR_OK
    E.remove([10, 20])
    assert E.n_groups == 0 and E.n_filters == 3
    with pytest.raises(_lib.VisragHipError, match=r"status 3"):
        E.search_groups(Q, 3)
    assert _status(lib.vr_index_range_results, E._h, ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(ids.ctypes.data), 0, 0, stream) == VR_ERR_STATE
    fsc, fids = E.search_filtered(Q, 5, 0)                    # works without a new set_filters
    assert (fids >= 0).all() and np.isfinite(fsc).all()
    E.set_groups([0, 400, n - 2])
    assert (E.search_groups(Q, 2)[2] >= 0).all()
    E.close()


# ------------------------------------------------------------------------------------------------------- update ---
def test_update():
    n, dim = 4000, 256
    rows, _ = M.scaled_rows(n, dim)
    model = M.Model(rows, _masks(n))
    E = _edited(rows, model.masks)
    off = np.concatenate([np.arange(0, n, 7), [n]]).astype(np.int64)
    E.set_groups(off)
    Q0 = _queries(rows, dim)
    _same(E, model, Q0, full=False)
    big = int(np.argmax(np.linalg.norm(rows.astype(np.float64), axis=1)))
    before = E.error_model()["max_row_norm"]
    new = R.unit(1, dim, 21)
    E.update([big], new); model.update([big], new)
    assert E.n_groups == len(off) - 1 and E.n_filters == 3    # no row moved
    after = E.error_model()["max_row_norm"]
    assert after < before                                     # the maximum goes DOWN: recomputed, not only raised (bits vs F: _same)
    sc_g = E.search_groups(Q0, 5)                             # the grouping set before the update still answers ...
    _same(E, model, Q0)                                       # (sets the same offsets on E and F)
    assert _bits(E.search_groups(Q0, 5)) == _bits(sc_g)       # ... and answered what the fresh index does
    rng = np.random.default_rng(5)
    ids = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=30, replace=False)]).astype(np.int64)
    new = (2 * R.unit(len(ids), dim, 22)).astype(np.float32)
    E.update(ids, new); model.update(ids, new)                # from numpy, ids unsorted
    Q = np.ascontiguousarray(np.concatenate([new[:8], R.unit(8, dim, 2)]))
    top = _same(E, model, Q)
    assert top[1][:8, 0].tolist() == ids[:8].tolist()          # a query equal to a new row finds it first
    ids2 = rng.choice(n, size=32, replace=False).astype(np.int64)
    new2 = (2 * R.unit(len(ids2), dim, 23)).astype(np.float32)
    E.update(torch.from_numpy(ids2), torch.from_numpy(new2).cuda()); model.update(ids2, new2)     # from a cuda tensor
    Q2 = np.ascontiguousarray(np.concatenate([new2[:8], R.unit(8, dim, 2)]))
    top = _same(E, model, Q2)
    assert top[1][:8, 0].tolist() == ids2[:8].tolist()
    dev = E.rows(ids2, device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint32), new2.view(np.uint32))
    devb = E.rows(ids2[[3, 3, 0]], bf16=True, device=True)    # duplicates allowed
    assert np.array_equal(devb.cpu().numpy().view(np.uint16), M.bf16_bits(new2[[3, 3, 0]]))
    E.close()


# ----------------------------------------------------------------------------------------------------- sequence ---
def test_random_sequence_of_edits_and_capacity():
    dim, cap = 128, 2600
    rng = np.random.default_rng(77)
    pool = R.unit(6000, dim, 31)                              # rows to add and to update with, drawn in order
    used = 2000
    model = M.Model(pool[:used])
    E = _edited(model.rows, capacity=cap)
    Q = np.ascontiguousarray(R.unit(16, dim, 2))
    ops = []
    for step in range(12):
        n = len(model)
        op = ["add", "remove", "update"][int(rng.integers(3))] if step >= 3 else ["remove", "add", "update"][step]
        if op == "add" and cap - n < 1:
            op = "remove"
        if op == "remove" and n < 2:
            op = "add"
        if op == "add":
            m = int(rng.integers(1, min(300, cap - n) + 1))
            E.add(pool[used:used + m]); model.add(pool[used:used + m])
        elif op == "remove":
            ids = rng.choice(n, size=int(rng.integers(1, max(2, int(0.3 * n)))), replace=False)
            assert np.array_equal(E.remove(ids), model.remove(ids))
        else:
            m = int(rng.integers(1, 41))
            ids = rng.choice(n, size=m, replace=False)
            E.update(ids, pool[used:used + m]); model.update(ids, pool[used:used + m])
        used += 300
        ops.append(op)
        _same(E, model, Q, full=False)                        # rows, error model, plan, search(k = 10)
    assert {"add", "remove", "update"} <= set(ops)
    # capacity is counted in rows: what a removal frees can be added again, and not one row more
    E.add(pool[: cap - len(model)]); model.add(pool[: cap - len(model)])
    r = 137
    ids = rng.choice(cap, size=r, replace=False)
    E.remove(ids); model.remove(ids)
    E.add(pool[100:100 + r]); model.add(pool[100:100 + r])
    assert len(E) == cap
    with pytest.raises(_lib.VisragHipError, match=r"status 4"):
        E.add(pool[:1])
    _same(E, model, Q, full=False)
    E.close()


# ------------------------------------------------------------------------------------------------------- errors ---
def _p64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def test_errors_leave_the_index_unchanged():
    n, dim = 1000, 64
    rows = R.unit(n, dim, 1)
    model = M.Model(rows, _masks(n))
    E = _edited(rows, model.masks)
    E.set_groups([0, 300, n])
    lib, stream = _lib.load(), ctypes.c_void_p(_stream_ptr(0))
    Q = np.ascontiguousarray(R.unit(4, dim, 2))
    E.search_range(Q, 0.3)
    reps = np.ascontiguousarray(R.unit(3, dim, 8))
    out = np.empty((3, dim), np.float32)
    removed = ctypes.c_int64(-7)
    for bad in ([3, n, 5], [3, -1, 5], [2 ** 40, 1, 2]):
        a = np.asarray(bad, dtype=np.int64)
        assert lib.vr_index_remove(E._h, _p64(a), 3, ctypes.byref(removed), stream) == VR_ERR_INVALID
        assert lib.vr_index_update(E._h, _p64(a), ctypes.c_void_p(reps.ctypes.data), 3, 0, stream) == VR_ERR_INVALID
        assert lib.vr_index_get_rows(E._h, _p64(a), 3, ctypes.c_void_p(out.ctypes.data), None, 0, stream) == VR_ERR_INVALID
    assert removed.value == -7
    dup = np.asarray([4, 9, 4], dtype=np.int64)
    assert lib.vr_index_update(E._h, _p64(dup), ctypes.c_void_p(reps.ctypes.data), 3, 0, stream) == VR_ERR_INVALID
    ok = np.asarray([4, 9, 5], dtype=np.int64)
    assert lib.vr_index_remove(None, _p64(ok), 3, None, stream) == VR_ERR_INVALID
    assert lib.vr_index_remove(E._h, None, 3, None, stream) == VR_ERR_INVALID
    assert lib.vr_index_remove(E._h, _p64(ok), -1, None, stream) == VR_ERR_INVALID
    assert lib.vr_index_update(None, _p64(ok), ctypes.c_void_p(reps.ctypes.data), 3, 0, stream) == VR_ERR_INVALID
    assert lib.vr_index_update(E._h, None, ctypes.c_void_p(reps.ctypes.data), 3, 0, stream) == VR_ERR_INVALID
    assert lib.vr_index_update(E._h, _p64(ok), None, 3, 0, stream) == VR_ERR_INVALID
    assert lib.vr_index_update(E._h, _p64(ok), ctypes.c_void_p(reps.ctypes.data), -1, 0, stream) == VR_ERR_INVALID
    assert lib.vr_index_get_rows(None, _p64(ok), 3, ctypes.c_void_p(out.ctypes.data), None, 0, stream) == VR_ERR_INVALID
    assert lib.vr_index_get_rows(E._h, None, 3, ctypes.c_void_p(out.ctypes.data), None, 0, stream) == VR_ERR_INVALID
    assert lib.vr_index_get_rows(E._h, _p64(ok), -1, ctypes.c_void_p(out.ctypes.data), None, 0, stream) == VR_ERR_INVALID
    assert lib.vr_index_get_rows(E._h, _p64(ok), 3, None, None, 0, stream) == VR_ERR_INVALID
    # n == 0: nothing is touched — not the grouping, the filters or the range result
    assert lib.vr_index_remove(E._h, None, 0, ctypes.byref(removed), stream) == VR_OK and removed.value == 0
    assert lib.vr_index_update(E._h, None, None, 0, 0, stream) == VR_OK
    assert lib.vr_index_get_rows(E._h, None, 0, ctypes.c_void_p(out.ctypes.data), None, 0, stream) == VR_OK
    assert E.remove([]).tolist() == list(range(n)) and E.n_groups == 2
    sc, ids = np.empty(1, np.float32), np.empty(1, np.int64)
    assert lib.vr_index_range_results(E._h, ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(ids.ctypes.data), 0, 0, stream) == VR_OK
    assert (E.search_groups(Q, 2)[2] >= 0).all()
    with pytest.raises(ValueError):
        E.update([1, 2], reps)                                # two ids, three rows
    # after all of that: the index as it was
    assert len(E) == n and E.n_filters == 3
    _same(E, model, _queries(rows, dim))
    E.close()


# --------------------------------------------------------------------------------------------------------- demo ---
def _write_kb(path, C, names):
    os.makedirs(path)
    np.save(os.path.join(path, "reps.npy"), C)
    with open(os.path.join(path, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))


def test_demo_remove_documents_with_a_resident_index(tmp_path, monkeypatch):
    from visrag_amd import demo
    C, _ = R.decks(30, 10, 64, 0.05)
    names = [f"deck_{d}.pdf_{i}.png" for d in range(30) for i in range(10)]
    base = R.unit(30, 64, 5)                                  # the decks' own vectors
    docs = ["deck_3.pdf", "deck_17.pdf", "deck_29.pdf"]
    kb, kb2 = str(tmp_path / "kb"), str(tmp_path / "kb2")
    _write_kb(kb, C, names)
    keep = np.array([doc_of_page(n) not in docs for n in names])
    _write_kb(kb2, C[keep], [n for n, k in zip(names, keep) if k])      # a base built without those documents
    qvec = [None]
    monkeypatch.setattr(demo, "encode", lambda model, tok, texts: qvec[0])
    ix, nm = demo.load_knowledge_base(kb, 0)
    ix2, nm2 = demo.load_knowledge_base(kb2, 0)
    gone = demo.remove_documents(kb, docs, index=ix, names=nm)
    assert gone == [n for n in names if doc_of_page(n) in docs] and len(ix) == 270 and nm == nm2
    for d in (3, 17, 29, 8):                                  # the removed decks' own vectors ask, and one that stayed
        qvec[0] = base[d:d + 1]
        got = demo.retrieve(kb, "which deck?", 15, None, None, index=ix, names=nm, return_scores=True)
        want = demo.retrieve(kb2, "which deck?", 15, None, None, index=ix2, names=nm2, return_scores=True)
        assert [os.path.basename(p) for p in got[0]] == [os.path.basename(p) for p in want[0]] and got[1] == want[1]
        assert len(got[0]) == 15 and not any(doc_of_page(os.path.basename(p)) in docs for p in got[0])
        gd = demo.retrieve_documents(kb, base[d], 30, None, None, index=ix, names=nm, return_scores=True)
        wd = demo.retrieve_documents(kb2, base[d], 30, None, None, index=ix2, names=nm2, return_scores=True)
        assert [os.path.basename(p) for p in gd[0]] == [os.path.basename(p) for p in wd[0]] and gd[1] == wd[1]
        assert len(gd[0]) == 27 and not any(doc_of_page(os.path.basename(p)) in docs for p in gd[0])
    assert np.array_equal(np.load(os.path.join(kb, "reps.npy")).view(np.uint32), C[keep].view(np.uint32))
    assert demo.duplicate_pages(kb, 0.9, index=ix, names=nm) == demo.duplicate_pages(kb2, 0.9, index=ix2, names=nm2)
    ix.close(); ix2.close()
