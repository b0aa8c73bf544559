"""visrag_amd.documents: pages -> documents on the host (no GPU)."""
import numpy as np

from visrag_amd.documents import doc_of_page, group_rows


def test_group_rows_interleaved_labels():
    labels = ["b", "a", "b", "c", "a", "b"]
    order, offsets, names = group_rows(labels)
    assert names == ["b", "a", "c"]                                   # first appearance
    assert order.tolist() == [0, 2, 5, 1, 4, 3]                       # stable inside a group
    assert offsets.tolist() == [0, 3, 5, 6]
    assert order.dtype == np.int64 and offsets.dtype == np.int64
    for g, name in enumerate(names):
        assert all(labels[i] == name for i in order[offsets[g]:offsets[g + 1]])


def test_group_rows_contiguous_labels_give_the_identity():
    labels = ["x"] * 3 + ["y"] + ["z"] * 2
    order, offsets, names = group_rows(labels)
    assert order.tolist() == list(range(6)) and offsets.tolist() == [0, 3, 4, 6] and names == ["x", "y", "z"]
    order, offsets, names = group_rows([7])
    assert order.tolist() == [0] and offsets.tolist() == [0, 1] and names == [7]
    order, offsets, names = group_rows([])
    assert len(order) == 0 and offsets.tolist() == [0] and names == []


def test_group_rows_ids_round_trip_through_order():
    rng = np.random.default_rng(0)
    labels = [f"doc{d}" for d in rng.integers(0, 40, size=500)]
    order, offsets, names = group_rows(labels)
    assert sorted(order.tolist()) == list(range(500))
    grouped = [labels[i] for i in order]
    # a row id of the grouped layout maps back to the input row through `order`, and its group names its label
    group_of = np.repeat(np.arange(len(names)), np.diff(offsets))
    for j in range(500):
        assert labels[order[j]] == grouped[j] == names[group_of[j]]
    inverse = np.empty(500, np.int64); inverse[order] = np.arange(500)
    assert all(order[inverse[i]] == i for i in range(500))
    # every label is one run
    assert sum(1 for j in range(500) if j == 0 or grouped[j] != grouped[j - 1]) == len(names) == len(set(labels))


def test_doc_of_page_splits_on_the_last_underscore():
    assert doc_of_page("report.pdf_3.png") == "report.pdf"
    assert doc_of_page("my_annual_report.pdf_12.png") == "my_annual_report.pdf"
    assert doc_of_page("a_b") == "a"
    assert doc_of_page("page.png") == "page.png"                      # no underscore: its own document
    assert doc_of_page("") == ""
    assert doc_of_page("deck_") == "deck"
    assert doc_of_page("_7.png") == ""                                # the rule as stated: everything before the last underscore
    assert doc_of_page("x__1.png") == "x_"
