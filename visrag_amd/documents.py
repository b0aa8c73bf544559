"""Documents over pages: the host side of the document-level search (HipIndex.set_groups / search_groups).

The index ranks rows (pages); a corpus is usually documents embedded page after page.  `search_groups` wants every document
to be ONE run of adjacent rows.  `group_rows` turns per-row labels into that layout, `doc_of_page` is the label rule of the demo's
knowledge base (`<pdf>_<idx>.png`).  Pure numpy: nothing here touches the GPU.
"""
from __future__ import annotations

from typing import Hashable, List, Sequence, Tuple

import numpy as np


def group_rows(labels: Sequence[Hashable]) -> Tuple[np.ndarray, np.ndarray, List[Hashable]]:
    """-> (order, offsets, names).

    `order` (int64 [n]) is a stable permutation of the rows that makes equal labels adjacent: row `order[j]` of the input is row
    j of the grouped layout; groups come in the order their label first appears and rows keep their order inside a group, so
    labels that are contiguous already give the identity.  `offsets` (int64 [n_groups + 1]) are the groups' first rows in the
    grouped layout — what `HipIndex.set_groups` takes — and `names[g]` is the label of group g.  A row id `i` returned by a
    search over the grouped layout is row `order[i]` of the input."""
    first: dict = {}
    gid = np.empty(len(labels), dtype=np.int64)
    names: List[Hashable] = []
    for i, lab in enumerate(labels):
        g = first.get(lab)
        if g is None:
            g = first[lab] = len(names)
            names.append(lab)
        gid[i] = g
    order = np.argsort(gid, kind="stable").astype(np.int64)
    counts = np.bincount(gid, minlength=len(names)).astype(np.int64)
    offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts)]).astype(np.int64)
    return order, offsets, names


def doc_of_page(name: str) -> str:
    """The document of a page file name of the demo's knowledge base: `<pdf>_<idx>.png` -> `<pdf>`.  The split is on the LAST
    underscore (`my_report.pdf_12.png` -> `my_report.pdf`); a name without an underscore is its own document."""
    head, sep, _ = name.rpartition("_")
    return head if sep else name
