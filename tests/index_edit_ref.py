"""Plain numpy statement of the index edited in place (include/visrag_hip.h: vr_index_remove / vr_index_update / vr_index_get_rows),
the reference of tests/test_gpu_index_edit.py.  The model is an array of rows plus the bool filters the index carries; an edit of
the model is the obvious numpy statement (np.delete, an indexed assignment, a concatenation), and the contract is that the edited
HipIndex answers every search bit for bit like a FRESH HipIndex built from the model's rows with the model's filters set.
tests/test_cpu_index_edit_ref.py pins the model on hand-worked cases.  Nothing here needs a GPU or the built library."""
import numpy as np

from tests.group_search_ref import unit  # noqa: F401  (the corpora of the tests)


def new_id_of_old(n_rows, removed):
    """int64 [n_rows]: the new id of every old row once the rows `removed` (any order, duplicates count once) are gone — old id
    minus the removed ids below it — and -1 for a removed row"""
    rem = np.unique(np.asarray(removed, dtype=np.int64).reshape(-1))
    assert len(rem) == 0 or (rem[0] >= 0 and rem[-1] < n_rows)
    out = np.full(int(n_rows), -1, dtype=np.int64)
    nxt = 0
    gone = set(rem.tolist())
    for i in range(int(n_rows)):
        if i not in gone:
            out[i] = nxt
            nxt += 1
    return out


def compact_filters(masks, nid):
    """bool [n_filters][old rows] -> bool [n_filters][rows left]: entry j = the old entry of the row now at j"""
    masks = np.atleast_2d(np.asarray(masks, dtype=bool))
    nid = np.asarray(nid, dtype=np.int64)
    out = np.zeros((masks.shape[0], int((nid >= 0).sum())), dtype=bool)
    for old, new in enumerate(nid):
        if new >= 0:
            out[:, new] = masks[:, old]
    return out


class Model:
    """rows float32 [n][dim] and the filters (bool [n_filters][n] or None) of an index, edited like the library edits it"""

    def __init__(self, rows, masks=None):
        self.rows = np.array(rows, dtype=np.float32)
        self.masks = None if masks is None else np.array(np.atleast_2d(masks), dtype=bool)

    def __len__(self):
        return len(self.rows)

    def add(self, reps):
        self.rows = np.concatenate([self.rows, np.asarray(reps, dtype=np.float32)])
        self.masks = None                          # vr_index_add drops the filters

    def remove(self, ids):
        nid = new_id_of_old(len(self.rows), ids)
        self.rows = np.ascontiguousarray(self.rows[nid >= 0])
        if self.masks is not None:
            self.masks = compact_filters(self.masks, nid)
        return nid

    def update(self, ids, reps):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        assert len(np.unique(ids)) == len(ids)
        self.rows[ids] = np.asarray(reps, dtype=np.float32)


def bf16_bits(rows):
    """float32 -> the bits of its bf16 rounding (to nearest, ties to even), uint16: integer arithmetic on the fp32 bits, valid
    for finite values"""
    u = np.ascontiguousarray(rows, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def scaled_rows(n, dim, seed=1, norm_seed=14):
    """unit rows scaled to norms U[0.5, 3] -> (rows f32, norms f64 as drawn)"""
    norms = np.random.default_rng(norm_seed).uniform(0.5, 3.0, size=(n, 1))
    return (unit(n, dim, seed) * norms).astype(np.float32), norms[:, 0]
