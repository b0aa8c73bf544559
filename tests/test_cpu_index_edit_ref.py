"""The numpy model of the index edited in place (tests/index_edit_ref.py) and the host helpers that go with it
(visrag_amd/documents.py, visrag_amd/demo.py with no resident index), pinned against np.delete on small arrays.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import index_edit_ref as E
from visrag_amd import documents as D


def _cases():
    rng = np.random.default_rng(0)
    yield 1, [0]
    yield 7, []
    yield 7, [0]
    yield 7, [6]
    yield 7, [3, 3, 1, 6, 1]
    yield 70, list(range(70))
    yield 70, list(range(25, 60))
    yield 70, list(range(0, 70, 2))
    for n in (33, 64, 65):
        yield n, rng.choice(n, size=n // 3, replace=False).tolist()


@pytest.mark.parametrize("n,removed", list(_cases()))
def test_new_id_of_old_and_compact_filters_against_np_delete(n, removed):
    nid = E.new_id_of_old(n, removed)
    assert nid.dtype == np.int64 and nid.shape == (n,)
    left = np.delete(np.arange(n), np.unique(np.asarray(removed, dtype=np.int64)))
    assert (nid[left] == np.arange(len(left))).all()               # the survivors keep their order and close up
    assert (nid[np.asarray(removed, dtype=np.int64)] == -1).all() and (nid >= 0).sum() == len(left)
    for i in left:                                                 # new id = old id - removed ids below it
        assert nid[i] == i - sum(1 for r in set(removed) if r < i)
    assert np.array_equal(D.new_id_of_old(n, removed), nid)        # the library's host helper states the same map
    masks = np.random.default_rng(1).random((3, n)) < 0.4
    want = np.delete(masks, np.unique(np.asarray(removed, dtype=np.int64)), axis=1)
    assert np.array_equal(E.compact_filters(masks, nid), want)
    assert np.array_equal(D.compact_filters(masks, nid), want)
    assert D.compact_filters(masks[0], nid).shape == (1, len(left))


def test_model_edits():
    rows = np.arange(24, dtype=np.float32).reshape(6, 4)
    m = E.Model(rows, np.array([[1, 0, 1, 0, 1, 1], [0, 0, 0, 1, 0, 0]], dtype=bool))
    nid = m.remove([3, 0, 3])
    assert nid.tolist() == [-1, 0, 1, -1, 2, 3] and len(m) == 4
    assert np.array_equal(m.rows, np.delete(rows, [0, 3], axis=0))
    assert m.masks.tolist() == [[False, True, True, True], [False, False, False, False]]     # filter 1 lost its only row
    m.update([3, 0], np.full((2, 4), 7, np.float32) * np.array([[1], [2]], np.float32))
    assert m.rows[3].tolist() == [7] * 4 and m.rows[0].tolist() == [14] * 4 and m.rows[1].tolist() == rows[2].tolist()
    assert m.masks is not None                                     # no row moved: the filters stay
    m.add(np.zeros((2, 4), np.float32))
    assert len(m) == 6 and m.masks is None                         # vr_index_add drops them
    assert rows[0, 0] == 0                                         # the model works on its own copy


def test_bf16_bits_is_round_to_nearest_even():
    x = np.concatenate([E.unit(50, 64, 3).reshape(-1), np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0, 3.0e-39],
                                                                 dtype=np.float32)])   # two ties: to even down, to even up
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(E.bf16_bits(x), want)
    assert E.bf16_bits(np.float32([1.00390625]))[0] == 0x3F80 and E.bf16_bits(np.float32([1.01171875]))[0] == 0x3F82


def test_documents_helpers():
    names = ["a.pdf_0.png", "a.pdf_1.png", "b.pdf_0.png", "my_c.pdf_0.png", "a.pdf_2.png", "my_c.pdf_1.png", "solo.png"]
    ids = D.rows_of_documents(names, ["a.pdf", "my_c.pdf", "no_such.pdf"])
    assert ids.dtype == np.int64 and ids.tolist() == [0, 1, 3, 4, 5]
    assert D.rows_of_documents(names, []).tolist() == [] and D.rows_of_documents(names, ["solo.png"]).tolist() == [6]
    nid = D.new_id_of_old(len(names), ids)
    assert nid.tolist() == [-1, -1, 0, -1, -1, -1, 1]
    assert D.remap_rows(nid, [6, 0, 2, 2, 5]).tolist() == [1, 0, 0]              # order kept, removed rows dropped
    assert D.remap_rows(nid, []).tolist() == []
    with pytest.raises(ValueError):
        D.new_id_of_old(3, [3])
    with pytest.raises(ValueError):
        D.new_id_of_old(3, [-1])
    with pytest.raises(ValueError):
        D.compact_filters(np.ones((1, 4), bool), nid)


def test_demo_remove_documents_on_disk(tmp_path):
    from PIL import Image
    from visrag_amd import demo
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    names = [f"doc_{d}.pdf_{i}.png" for d in range(4) for i in range(3)]
    reps = E.unit(len(names), 64, 2)
    np.save(os.path.join(kb, "reps.npy"), reps)
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))
    for nm in names:
        Image.new("RGB", (4, 4)).save(os.path.join(kb, nm))
    outside = tmp_path / "doc_1.pdf_0.png"                              # the same file name outside the base: not ours to delete
    outside.write_bytes(b"keep")
    held = list(names)
    gone = demo.remove_documents(kb, ["doc_1.pdf", "doc_3.pdf", "no_such.pdf"], names=held)
    assert gone == [n for n in names if n.startswith(("doc_1", "doc_3"))]
    left = [n for n in names if n not in gone]
    assert held == left                                                  # edited in place
    assert open(os.path.join(kb, "index2img_filename.txt")).read().split("\n") == left
    keep = np.array([n in left for n in names])
    on_disk = np.load(os.path.join(kb, "reps.npy"))
    assert on_disk.dtype == np.float32 and np.array_equal(on_disk.view(np.uint32), reps[keep].view(np.uint32))
    assert all(not os.path.exists(os.path.join(kb, n)) for n in gone)
    assert all(os.path.exists(os.path.join(kb, n)) for n in left) and outside.read_bytes() == b"keep"
    assert demo.remove_documents(kb, ["no_such.pdf"]) == []              # nothing to do: nothing rewritten
    assert demo.remove_documents(kb, ["doc_0.pdf"], delete_images=False) == names[:3]
    assert os.path.exists(os.path.join(kb, names[0])) and len(np.load(os.path.join(kb, "reps.npy"))) == 3
    assert demo.remove_documents(str(tmp_path / "missing"), ["doc_0.pdf"]) is None
    with pytest.raises(ValueError):
        demo.remove_documents(kb, ["doc_2.pdf"], names=list(reversed(left)))
    with pytest.raises(ValueError):
        demo.update_pages(None, None, [Image.new("RGB", (4, 4))], kb, ["doc_9.pdf_0.png"])      # an unknown page
