"""From top-k pages to one answer, host side (visrag_amd/answer.py, VisRAGRet.weighted_selection's rule, the n-best list of
the beam rule): no GPU.  The reference side is tests/golden/weighted_tiny.npz (tools/gen_golden_weighted.py)."""
import numpy as np
import pytest
from PIL import Image

from tests.answer_util import FIX, REF_BAR, BeamReplay, Words, msgs_of, question_pages
from visrag_amd.answer import concat_pages, top_pages
from visrag_amd.config import tiny_config
from visrag_amd.generation import beam_rule, prefill_groups, run_rule
from visrag_amd.modeling import _prompt_item, chat_prompt, select_weighted


def _page(w, h, seed):
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))


# 101 x 67 scaled to height 80 is 120.597.. wide and truncates to 120; scaled to width 101, 64 x 80 is 126.25 high
PAGES = [(101, 67), (64, 80), (33, 33)]


@pytest.mark.parametrize("kind", ["horizontal", "vertical"])
def test_concat_pages_against_pillow(kind):
    pages = [_page(w, h, i) for i, (w, h) in enumerate(PAGES)]
    got = concat_pages(pages, kind)
    if kind == "horizontal":
        sizes = [(120, 80), (64, 80), (80, 80)]
        assert [int(w * (80 / h)) for w, h in PAGES] == [s[0] for s in sizes] == [int(w * 80 / h) for w, h in PAGES]
        assert got.size == (264, 80)
    else:
        sizes = [(101, 67), (101, 126), (101, 101)]
        assert [int(h * (101 / w)) for w, h in PAGES] == [s[1] for s in sizes] == [int(h * 101 / w) for w, h in PAGES]
        assert got.size == (101, 294)
    assert got.mode == "RGB"
    arr, at = np.asarray(got), 0
    for im, size in zip(pages, sizes):
        want = np.asarray(im.resize(size, Image.Resampling.BICUBIC))
        part = arr[:, at:at + size[0]] if kind == "horizontal" else arr[at:at + size[1]]
        assert np.array_equal(part, want)
        at += size[0] if kind == "horizontal" else size[1]


@pytest.mark.parametrize("kind", ["horizontal", "vertical"])
def test_concat_one_page_keeps_its_size(kind):
    page = _page(101, 67, 5)
    got = concat_pages([page], kind)
    assert got.size == page.size and np.array_equal(np.asarray(got), np.asarray(page))
    with pytest.raises(ValueError):
        concat_pages([], kind)
    with pytest.raises(ValueError):
        concat_pages([page], "diagonal")


def test_top_pages_order_ties_and_short_run():
    run = {"q1": {"a": 0.5, "b": 0.9, "c": 0.5, "d": 0.7, "e": 0.1}, "q2": {"x": 1.0}}
    assert top_pages(run, "q1", 3) == (["b", "d", "a"], [0.9, 0.7, 0.5])          # a before c: equal scores keep the run's order
    assert top_pages(run, "q1", 4) == (["b", "d", "a", "c"], [0.9, 0.7, 0.5, 0.5])
    assert top_pages(run, "q2", 1) == (["x"], [1.0])
    with pytest.raises(ValueError, match="fewer than topk"):
        top_pages(run, "q2", 2)
    with pytest.raises(KeyError):
        top_pages(run, "q3", 1)


def test_select_weighted_rule():
    idx, w, p = select_weighted([-1.0, -1.0], [0.3, 0.3])
    assert idx == 0 and w[0] == w[1] and p == [0.5, 0.5]                           # the first page wins a tie
    idx, w, p = select_weighted([-2.0, -0.5, -0.6], [5.0, 1.0, 1.0])
    assert idx == 0                                                                # the document score can outweigh the answer's
    idx, _, _ = select_weighted([-2.0, -0.5, -0.6], [1.2, 1.0, 1.0])
    assert idx == 1
    _, _, p = select_weighted([0.0, 0.0], [1000.0, 999.0])                         # no overflow
    assert np.isclose(p[0], 1 / (1 + np.exp(-1.0)))


def test_selection_and_nbest_replayed_from_the_fixture():
    F = np.load(FIX)
    k, nb, n_new = int(F["k"]), int(F["num_beams"]), int(F["max_new"])
    n_decisive, kinds = 0, set()
    for q in range(int(F["n_questions"])):
        res = []
        for i in range(k):
            P = q * k + i
            r = run_rule(beam_rule(nb, n_new), BeamReplay(F, P))
            assert r["tokens"] == F[f"p{P}_beam_tokens"].tolist(), (q, i)
            assert r["hyps"][0] == (r["score"], r["tokens"])
            assert np.isclose(r["score"], float(F[f"p{P}_beam_score"]), rtol=1e-6, atol=0)
            s2 = F[f"p{P}_beam_scores2"]
            assert len(r["hyps"]) >= len(s2) and all(a[0] >= b[0] for a, b in zip(r["hyps"], r["hyps"][1:]))
            np.testing.assert_allclose([h[0] for h in r["hyps"][:len(s2)]], s2, rtol=1e-6, atol=0)
            if len(s2) > 1:
                assert r["hyps"][1][1] == F[f"p{P}_beam_tokens2"].tolist()
            res.append(r)
        ds = F[f"q{q}_doc_scores"].tolist()
        idx, w, p = select_weighted([r["score"] for r in res], ds)
        assert idx == int(F[f"q{q}_index"]), q
        np.testing.assert_allclose(p, F[f"q{q}_probs"], rtol=1e-6, atol=0)           # (the reference's softmax is float32)
        np.testing.assert_allclose(w, F[f"q{q}_weights"], rtol=2e-6, atol=0)
        # the conditions the tool wrote the fixture under, restated from the recorded figures
        amax = max(float(F[f"p{q * k + i}_beam_absmax"].max()) for i in range(k))
        steps_ok = all((F[f"p{q * k + i}_beam_set_margin"] > 4 * REF_BAR * F[f"p{q * k + i}_beam_absmax"]).all() for i in range(k))
        order = sorted(w, reverse=True)
        decisive = steps_ok and order[0] / order[1] > np.exp(2 * REF_BAR * amax)
        assert bool(F[f"q{q}_decisive"]) <= decisive, q
        if bool(F[f"q{q}_decisive"]):
            n_decisive += 1
            kinds |= {"doc"} if idx != ds.index(max(ds)) else set()
            kinds |= {"seq"} if idx != int(np.argmax([r["score"] for r in res])) else set()
    assert n_decisive >= 2 and kinds == {"doc", "seq"}


def test_answer_prompt_ids_match_the_reference():
    F = np.load(FIX)
    cfg = tiny_config()
    tok = Words(cfg.vocab_size)
    k = int(F["k"])
    for q in range(int(F["n_questions"])):
        for i, img in enumerate(question_pages(F, cfg, q)):
            prompt, imgs = chat_prompt(msgs_of(F, q), img, tok, cfg)
            assert prompt + "<AI>" == str(F[f"p{q * k + i}_prompt"])
            assert len(imgs) == int(F[f"p{q * k + i}_n_slices"])
            assert _prompt_item(prompt + "<AI>", imgs, tok, 2048).input_ids == F[f"p{q * k + i}_ids"].tolist()


def test_prefill_groups_split_on_the_workspace():
    assert prefill_groups([5, 5, 5], 100, 8) == [[0, 1, 2]]
    assert prefill_groups([60, 50, 40, 10], 100, 8) == [[0], [1, 2, 3]]
    assert prefill_groups([10, 10, 10, 10, 10], 100, 2) == [[0, 1], [2, 3], [4]]
    assert prefill_groups([150, 10], 100, 8) == [[0], [1]]                          # too long on its own: fails as it would alone
    assert prefill_groups([], 100, 8) == []


def test_generate_items_argument_checks():
    from visrag_amd.generation import generate_items

    class _NoChat:
        max_rows, max_slots, max_new = 3, 1, 32
    with pytest.raises(ValueError, match="prefill"):
        generate_items(_NoChat(), [], prefill="both")
    for kw in ({"num_return_sequences": 2}, {"num_return_sequences": 4, "num_beams": 3}, {"num_return_sequences": 0, "num_beams": 3},
               {"num_return_sequences": 2, "do_sample": True}):
        with pytest.raises(ValueError, match="num_return_sequences"):
            generate_items(_NoChat(), [], **kw)
    assert generate_items(_NoChat(), [], num_beams=3, num_return_sequences=3, prefill="batched") == []


def test_weighted_selection_argument_checks():
    from visrag_amd.modeling import VisRAGRet
    m = VisRAGRet.__new__(VisRAGRet)
    page = _page(8, 8, 0)
    with pytest.raises(NotImplementedError):
        VisRAGRet.weighted_selection(m, [page], [], [0.5], None, sampling=True)
    with pytest.raises(ValueError):
        VisRAGRet.weighted_selection(m, [], [], [], None)
    with pytest.raises(ValueError):
        VisRAGRet.weighted_selection(m, [page, page], [], [0.5], None)
    with pytest.raises(NotImplementedError):
        VisRAGRet.chat(m, [page], [[]], None, sampling=True, return_scores=True)


class _FakeChat:
    """Records the device calls of generate_items; every select answers with the same candidates."""
    max_rows, max_slots, max_new = 9, 3, 8

    def __init__(self):
        from types import SimpleNamespace
        self.enc = SimpleNamespace(max_tokens=100, max_seqs=2)
        self.calls = []

    def prefill(self, slot, row, item):
        self.calls.append(("prefill", slot, row, len(item.input_ids)))

    def prefill_batch(self, slots, rows, items):
        self.calls.append(("prefill_batch", list(slots), list(rows), [len(it.input_ids) for it in items]))

    def select(self, mode, groups, k, beam_scores=None, **kw):
        G = len(groups)
        sc = np.tile(-np.arange(1, k + 1, dtype=np.float32), (G, 1))
        return sc, np.tile(10 + np.arange(k, dtype=np.int32), (G, 1)), np.zeros((G, k), dtype=np.int32)

    def reorder(self, rows, parents):
        pass

    def step(self, slots, rows, tokens):
        self.calls.append(("step", list(slots), list(rows)))


def test_generate_items_prefill_calls():
    from visrag_amd.generation import generate_items
    from visrag_amd.preprocess import PreparedItem
    items = [PreparedItem(input_ids=[1] * n, image_bound=[], slices=[]) for n in (60, 50, 30, 10)]
    chat = _FakeChat()
    single = generate_items(chat, items, max_new_tokens=2, num_beams=3, details=True)
    assert [c for c in chat.calls if c[0] != "step"] == [("prefill", 0, 0, 60), ("prefill", 1, 3, 50), ("prefill", 2, 6, 30),
                                                         ("prefill", 0, 0, 10)]
    chat = _FakeChat()
    batched = generate_items(chat, items, max_new_tokens=2, num_beams=3, details=True, prefill="batched", num_return_sequences=2)
    assert [c for c in chat.calls if c[0] != "step"] == [("prefill_batch", [0], [0], [60]), ("prefill_batch", [1, 2], [3, 6], [50, 30]),
                                                         ("prefill_batch", [0], [0], [10])]
    assert [r["tokens"] for r in single] == [r["tokens"] for r in batched]
    assert all(len(r["hyps"]) == 1 for r in single) and all(len(r["hyps"]) == 2 for r in batched)
    lists = generate_items(_FakeChat(), items[:1], max_new_tokens=2, num_beams=3, num_return_sequences=3)
    assert len(lists) == 1 and len(lists[0]) == 3 and lists[0][0] == single[0]["tokens"]
