"""score_items / score_answers / choose / marginal_selection over host stand-ins for HipChat.score: one replays the reference
model's recorded beam log-probs (tests/golden/chat_tiny.npz), one follows a formula, so that what the Python layer adds —
chunking, tokenisation of answers, penalties, the selection rules — is checked without a device."""
import os
import types

import numpy as np
import pytest
from PIL import Image

from tests.answer_util import Words
from visrag_amd.config import tiny_config
from visrag_amd.generation import marginal_weights, prefill_groups, score_items, sequence_score
from visrag_amd.modeling import VisRAGRet, _prompt_item, answer_ids, chat_prompt
from visrag_amd.preprocess import PreparedItem

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chat_tiny.npz")


class _Replay:
    """HipChat.score from the recorded per-(beam prefix) top-64 log-softmax rows: logit = the recorded log-prob, lse = 0."""

    def __init__(self, F, max_tokens, max_seqs):
        self.enc = types.SimpleNamespace(max_tokens=max_tokens, max_seqs=max_seqs)
        self.calls = []
        self.prompts, self.tables = [], []
        for p in range(int(F["n_prompts"])):
            pre, ln = F[f"p{p}_beam_q_prefix"], F[f"p{p}_beam_q_len"]
            self.prompts.append(F[f"p{p}_ids"].tolist())
            self.tables.append({tuple(pre[i, :ln[i]].tolist()): (F[f"p{p}_beam_q_ids"][i], F[f"p{p}_beam_q_logprobs"][i])
                                for i in range(len(ln))})

    def score(self, items, cont_lens):
        assert len(items) <= self.enc.max_seqs
        self.calls.append([len(it.input_ids) for it in items])
        out = []
        for it, c in zip(items, cont_lens):
            ids = list(it.input_ids)
            prompt, cont = ids[:-c], ids[-c:]
            table = self.tables[self.prompts.index(prompt)]
            lp, top = [], []
            for t, tok in enumerate(cont):
                row_ids, row = table[tuple(cont[:t])]
                (j,) = np.nonzero(row_ids == tok)[0]
                lp.append(row[j]); top.append(row_ids[int(np.argmax(row))])
            out.append({"logit": np.asarray(lp, np.float32), "lse": np.zeros(c, np.float32),
                        "top_logit": np.zeros(c, np.float32), "top_token": np.asarray(top, np.int32)})
        return out


def _logprob(key, prefix, tok):
    return -(((tok * 7 + len(prefix) * 3 + key) % 11) + 1) / 4.0


class _Formula:
    """log p(tok | page, prefix) = -(((7 tok + 3 len(prefix) + key(page)) mod 11) + 1) / 4; the row's argmax is token 16 + len(prefix)."""

    def __init__(self, max_tokens=4096, max_seqs=4):
        self.enc = types.SimpleNamespace(max_tokens=max_tokens, max_seqs=max_seqs)
        self.seen = []

    @staticmethod
    def key(item):
        return int(sum(int(np.asarray(s, dtype=np.int64).sum()) for s in item.slices) % 97)

    def score(self, items, cont_lens):
        assert len(items) <= self.enc.max_seqs
        out = []
        for it, c in zip(items, cont_lens):
            ids = list(it.input_ids)
            cont = ids[-c:]
            self.seen.append((ids[:-c], cont))
            lp = [_logprob(self.key(it), cont[:t], tok) for t, tok in enumerate(cont)]
            out.append({"logit": np.asarray(lp, np.float32) + np.float32(3.0), "lse": np.full(c, 3.0, np.float32),
                        "top_logit": np.zeros(c, np.float32), "top_token": np.asarray([16 + t for t in range(c)], np.int32)})
        return out


def test_score_items_replays_the_reference_beam_scores_in_chunks():
    F = np.load(FIX)
    n = int(F["n_prompts"])
    items = [PreparedItem(input_ids=F[f"p{p}_ids"].tolist(), image_bound=[], slices=[]) for p in range(n)]
    conts = [F[f"p{p}_beam_tokens"].tolist() for p in range(n)]
    lens = [len(it.input_ids) + len(c) for it, c in zip(items, conts)]
    whole = _Replay(F, max_tokens=sum(lens), max_seqs=4)
    res = score_items(whole, items, conts, repetition_penalty=float(F["pen_beam"]))
    assert whole.calls == [lens]
    for p, r in enumerate(res):
        assert r["token_logprobs"].dtype == np.float64 and r["token_logprobs"].shape == (20,)
        assert abs(r["score"] - float(F[f"p{p}_beam_score"])) < 1e-6
        assert abs(r["sum"] - 20 * r["score"]) < 1e-12
        assert r["greedy_match"].dtype == bool and r["greedy_match"].shape == (20,)
        assert np.array_equal(r["greedy_match"], r["top_tokens"] == np.asarray(conts[p]))
    # a workspace of 1400 tokens / 2 sequences: the cuts are prefill_groups' over prompt + continuation lengths
    small = _Replay(F, max_tokens=1400, max_seqs=2)
    res2 = score_items(small, items, conts, repetition_penalty=float(F["pen_beam"]))
    groups = prefill_groups(lens, 1400, 2)
    assert len(groups) > 1 and small.calls == [[lens[i] for i in g] for g in groups]
    for a, b in zip(res, res2):
        assert np.array_equal(a["token_logprobs"], b["token_logprobs"]) and a["score"] == b["score"]
    # penalties
    plain = score_items(whole, items[:1], conts[:1])[0]
    assert abs(plain["sum"] - plain["token_logprobs"].sum()) < 1e-12 and abs(plain["score"] - plain["sum"] / 20) < 1e-12
    assert score_items(whole, items[:1], conts[:1], length_penalty=0.0)[0]["score"] == plain["sum"]


def test_score_items_argument_errors():
    chat = _Formula()
    it = PreparedItem(input_ids=[1, 20, 21], image_bound=[], slices=[])
    with pytest.raises(ValueError):
        score_items(chat, [it], [[]])
    with pytest.raises(ValueError):
        score_items(chat, [it, it], [[5]])
    assert score_items(chat, [], []) == []
    assert it.input_ids == [1, 20, 21]                       # the prompt items are not written to


@pytest.fixture(scope="module")
def model():
    cfg = tiny_config()
    m = VisRAGRet(types.SimpleNamespace(cfg=cfg))
    m._chat = _Formula()
    return cfg, m, Words(cfg.vocab_size)


def _page(cfg, v):
    return Image.fromarray(np.full((cfg.scale_resolution, cfg.scale_resolution, 3), v, dtype=np.uint8))


MSGS = [{"role": "user", "content": "what is on the page"}]


def _item(cfg, tok, image):
    p, sl = chat_prompt(MSGS, image, tok, cfg)
    return _prompt_item(p + "<AI>", sl, tok, 2048)


def test_score_answers_tokenises_answers_as_the_generator_emits_them(model):
    cfg, m, tok = model
    chat = m._chat
    chat.seen.clear()
    pages = [_page(cfg, 10), _page(cfg, 200)]
    out = m.score_answers(pages, [MSGS, MSGS], [["a cat", "a dog on a mat"], ["nothing"]], tok)
    assert [len(o) for o in out] == [2, 1]
    words = lambda s: [tok._word_id(w) for w in s.split()]  # noqa: E731
    assert [c for _, c in chat.seen] == [words("a cat") + [tok.eos_id], words("a dog on a mat") + [tok.eos_id], words("nothing") + [tok.eos_id]]
    for (prompt, cont), image in zip(chat.seen, [pages[0], pages[0], pages[1]]):
        assert prompt == _item(cfg, tok, image).input_ids                       # chat(assistant_turn=True)'s prompt
        assert (prompt + cont).count(tok.bos_id) == 1 and prompt[0] == tok.bos_id and tok.bos_id not in cont
    assert len(out[0][1]["token_logprobs"]) == 6
    chat.seen.clear()
    out2 = m.score_answers(pages[:1], [MSGS], [["a cat"]], tok, append_eos=False)
    assert [c for _, c in chat.seen] == [words("a cat")]
    assert np.array_equal(out2[0][0]["token_logprobs"], out[0][0]["token_logprobs"][:2])
    # a tokenizer that adds no BOS of its own: the prompt still gets one, the answer none
    nobos = Words(cfg.vocab_size)
    nobos.add_bos_token = False
    assert answer_ids("a cat", nobos) == answer_ids("a cat", tok) == words("a cat") + [tok.eos_id]
    with pytest.raises(ValueError):
        m.score_answers(pages[:1], [MSGS], [["  "]], tok)
    with pytest.raises(ValueError):
        m.score_answers(pages, [MSGS], [["a"], ["b"]], tok)
    with pytest.raises(RuntimeError):
        VisRAGRet(types.SimpleNamespace(cfg=cfg)).score_answers(pages[:1], [MSGS], [["a"]], tok)


def test_choose_takes_the_first_largest(model):
    cfg, m, tok = model
    page = _page(cfg, 10)
    options = ["a cat", "a dog on a mat", "a cat", "nothing at all here"]
    index, scores = m.choose(page, MSGS, options, tok)
    keys = [s["score"] for s in scores]
    assert len(scores) == 4 and keys[0] == keys[2]
    assert index == keys.index(max(keys))
    by_sum = [s["sum"] for s in scores]
    index_sum, _ = m.choose(page, MSGS, options, tok, normalise=False)
    assert index_sum == by_sum.index(max(by_sum))
    # two equal options alone: the first wins under either rule
    assert m.choose(page, MSGS, ["a cat", "a cat"], tok)[0] == 0 and m.choose(page, MSGS, ["a cat", "a cat"], tok, normalise=False)[0] == 0
    # the stand-in's numbers, by hand, for one option: sum of the formula over ("a", "cat", eos) and its mean
    key = m._chat.key(_item(cfg, tok, page))
    cont = answer_ids("a cat", tok)
    want = [_logprob(key, cont[:t], t_) for t, t_ in enumerate(cont)]
    np.testing.assert_allclose(scores[0]["token_logprobs"], want, atol=1e-6)
    assert abs(scores[0]["score"] - sum(want) / 3) < 1e-6
    with pytest.raises(ValueError):
        m.choose(page, MSGS, [], tok)


class _Canned(VisRAGRet):
    """weighted_selection replaced by a recorded result: the generation needs a device, what follows it does not"""

    def weighted_selection(self, image_list, msgs, doc_scores, tokenizer, details=False, **kwargs):
        self.ws_kwargs = kwargs
        tokens = [self.answers[int(np.asarray(im)[0, 0, 0])] for im in image_list]
        return "canned", {"tokens": tokens, "weights": [0.0] * len(tokens)}


def test_marginal_selection_over_a_recorded_generation():
    cfg = tiny_config()
    tok = Words(cfg.vocab_size)
    m = _Canned(types.SimpleNamespace(cfg=cfg))
    m._chat = _Formula()
    m.answers = {10: [30, 31, 2], 200: [40, 2], 90: [30, 31, 2]}
    pages = [_page(cfg, 10), _page(cfg, 200), _page(cfg, 90)]
    doc = [0.3, 0.9, 0.1]
    answer, d = m.marginal_selection(pages, MSGS, doc, tok, details=True, max_new_tokens=5)
    assert m.ws_kwargs == {"max_new_tokens": 5}
    assert d["candidates"] == [[30, 31, 2], [40, 2]]                 # distinct id lists, first seen first
    S = np.asarray(d["S"])
    assert S.shape == (2, 3)
    keys = [m._chat.key(_item(cfg, tok, im)) for im in pages]
    for a, cand in enumerate(d["candidates"]):
        for i in range(3):
            lp = [_logprob(keys[i], cand[:t], t_) for t, t_ in enumerate(cand)]
            assert abs(S[a, i] - sequence_score(lp, cand, 1.2)) < 1e-6      # the beam's default penalty
    index, weights, p = marginal_weights(S, doc)
    assert d["index"] == index and d["weights"] == weights and d["doc_probs"] == p
    assert answer == d["answers"][index] == tok.decode(d["candidates"][index][:-1]).strip()
    assert d["weighted_selection"][0] == "canned"
    # sums instead of means, and a penalty passed to the generation reaches the scoring
    _, d2 = m.marginal_selection(pages, MSGS, doc, tok, normalise=False, details=True, repetition_penalty=1.0)
    lp = [_logprob(keys[1], [40, 2][:t], t_) for t, t_ in enumerate([40, 2])]
    assert abs(d2["S"][1][1] - sum(lp)) < 1e-6
    assert m.marginal_selection(pages, MSGS, doc, tok) == answer
    # the same image twice: one candidate
    _, d3 = m.marginal_selection([pages[0], pages[0]], MSGS, [0.5, 0.5], tok, details=True)
    assert d3["candidates"] == [[30, 31, 2]] and abs(d3["weights"][0] - float(np.exp(d3["S"][0][0]))) < 1e-12
