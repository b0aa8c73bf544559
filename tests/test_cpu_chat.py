"""Host-side rules of MiniCPM-V 2.0 answer generation (visrag_amd/generation.py, VisRAGRet.chat's prompt): no GPU.

The reference side is tests/golden/chat_tiny.npz, recorded by tools/gen_golden_chat.py from the reference model's forward,
its own chat() prompts and a written-out statement of the transformers 4.40.2 greedy / beam rules."""
import os

import numpy as np
import pytest

from visrag_amd.config import tiny_config
from visrag_amd.generation import _Hyps, beam_search, chat_generation_config, decode_text, greedy_search
from visrag_amd.modeling import _prompt_item, chat_prompt
from visrag_amd.tokenizer import StandInTokenizer

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chat_tiny.npz")


class _Tok(StandInTokenizer):
    """The stand-in tokenizer with the fixture's decode: ids -> "w<id>" words."""

    def decode(self, ids):
        return " ".join(f"w{int(i)}" for i in ids) + " "


def test_decode_text_rules():
    tok = _Tok(1000)
    assert decode_text([[1, 5, 6, 2, 0, 0]], tok) == ["w5 w6"]
    assert decode_text([[0, 5, 0, 6]], tok) == ["w5 w6"]
    assert decode_text([[5, 2, 2]], tok) == ["w5 w2"]          # one trailing eos only


def test_generation_config_merge():
    assert chat_generation_config(False, {"num_beams": 1, "top_p": 0.5}) == {"num_beams": 1, "repetition_penalty": 1.2}
    assert chat_generation_config(True, {"temperature": 0.1, "num_beams": 4}) == {"temperature": 0.1, "do_sample": True,
                                                                                 "repetition_penalty": 1.02}


def test_unsupported_generation_options_raise():
    from visrag_amd.generation import generate_items

    class _NoChat:
        max_rows, max_slots, max_new = 3, 1, 32
    for kw in ({"top_p": 0.9}, {"length_penalty": 2.0}, {"do_sample": True, "num_beams": 3}, {"do_sample": True, "top_k": 0},
               {"do_sample": True, "top_k": 100}, {"no_repeat_ngram_size": 3}):
        with pytest.raises(NotImplementedError):
            generate_items(_NoChat(), [], **kw)


def test_hypothesis_score_counts_eos_and_done_rule():
    h = _Hyps(2)
    h.add([5, 6], -3.0, 3)                  # two tokens + eos: length 3
    assert np.isclose(h.beams[0][0], -1.0)
    assert not h.is_done(-0.5, 3)
    h.add([7], -1.0, 2)
    assert h.worst == -1.0
    assert h.is_done(-3.0, 3) and not h.is_done(-2.0, 3)
    h.add([8], -0.2, 2)                     # better: the worst (-1.0) is dropped
    assert len(h.beams) == 2 and h.worst == -0.5


def _penalise(vals, ids, seen, pen):
    v = vals.copy()
    m = np.isin(ids, list(seen))
    v[m] = np.where(v[m] < 0, v[m] * np.float32(pen), v[m] / np.float32(pen)).astype(np.float32)
    return v


class _BeamReplay:
    """The reference's per-(beam prefix) top-64 log_softmax rows as the backend of the decode rules, with the repetition
    penalty and the beam scores applied as the reference applies them (float32)."""

    def __init__(self, F, p):
        self.V, self.pen = 1000, float(F["pen_beam"])
        pre, ln = F[f"p{p}_beam_q_prefix"], F[f"p{p}_beam_q_len"]
        self.table = {tuple(pre[i, :ln[i]].tolist()): (F[f"p{p}_beam_q_ids"][i], F[f"p{p}_beam_q_logprobs"][i])
                      for i in range(len(ln))}
        self.seqs = [[]]

    def select(self, n, scores, k):
        cand = []
        for b in range(n):
            ids, lp = self.table[tuple(self.seqs[b])]        # KeyError: a prefix the reference's search never reached
            v = _penalise(lp, ids, set(self.seqs[b]), self.pen) + np.float32(scores[b])
            cand += [(float(x), int(t), b) for x, t in zip(v, ids)]
        cand.sort(key=lambda c: (-c[0], c[2] * self.V + c[1]))
        return cand[:k]

    def advance(self, parents, tokens):
        self.seqs = [self.seqs[p] + [t] for p, t in zip(parents, tokens)]


class _GreedyReplay:
    def __init__(self, F, p):
        self.ids, self.vals, self.pen = F[f"p{p}_greedy_top_ids"], F[f"p{p}_greedy_top_logits"], float(F["pen_greedy"])
        self.toks = []

    def select(self, n, scores, k):
        i = len(self.toks)
        v = _penalise(self.vals[i], self.ids[i], set(self.toks), self.pen)
        j = int(np.argmax(v))
        return [(float(v[j]), int(self.ids[i][j]), 0)]

    def advance(self, parents, tokens):
        self.toks.append(tokens[0])


def test_beam_rules_reproduce_the_reference_run():
    F = np.load(FIX)
    for p in range(int(F["n_prompts"])):
        r = beam_search(_BeamReplay(F, p), int(F["num_beams"]), int(F["max_new"]))
        assert r["tokens"] == F[f"p{p}_beam_tokens"].tolist(), p
        assert np.isclose(r["score"], float(F[f"p{p}_beam_score"]), rtol=1e-6, atol=0), p
        nt, npar = F[f"p{p}_beam_next_tokens"], F[f"p{p}_beam_next_parents"]
        assert len(r["steps"]) == len(nt)
        for s, (_, nxt) in enumerate(r["steps"]):
            assert [t for _, t, _ in nxt] == nt[s].tolist() and [q for _, _, q in nxt] == npar[s].tolist(), (p, s)


def test_greedy_rule_reproduces_the_reference_run():
    F = np.load(FIX)
    for p in range(int(F["n_prompts"])):
        r = greedy_search(_GreedyReplay(F, p), int(F["max_new"]))
        assert r["tokens"] == F[f"p{p}_greedy_tokens"].tolist(), p


def test_prompts_and_decoded_text_match_the_reference():
    from PIL import Image
    F = np.load(FIX)
    cfg = tiny_config()
    tok = _Tok(cfg.vocab_size)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
    questions = ["What animal is in the picture?", "Describe the image."]
    for p, name in enumerate(["cat.jpeg", "dog.jpg"]):
        img = Image.open(os.path.join(root, name)).convert("RGB")
        prompt, imgs = chat_prompt([{"role": "user", "content": questions[p]}], img, tok, cfg)
        assert prompt == str(F[f"p{p}_prompt"])                                   # the reference chat()'s prompt
        assert len(imgs) == int(F[f"p{p}_n_slices"])
        assert _prompt_item(prompt, imgs, tok, 2048).input_ids == F[f"p{p}_ids"].tolist()
    for p in range(int(F["n_prompts"])):
        for kind in ("greedy", "beam"):
            assert decode_text([F[f"p{p}_{kind}_tokens"].tolist()], tok)[0] == str(F[f"p{p}_{kind}_text"])
