"""Shared by tests/test_cpu_answer.py and tests/test_gpu_answer.py: the weighted-selection fixture
(tools/gen_golden_weighted.py -> tests/golden/weighted_tiny.npz), its pages and a replay backend of its recorded log-probs."""
import os

import numpy as np

from visrag_amd.tokenizer import StandInTokenizer

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "weighted_tiny.npz")
REF_BAR = 1e-2          # device vs reference logits, relative to max |logit| (tests/test_gpu_chat.py)


class Words(StandInTokenizer):
    """The stand-in tokenizer with the fixture's decode: ids -> "w<id>" words."""

    def decode(self, ids):
        return " ".join(f"w{int(i)}" for i in ids) + " "


def page_image(cfg, src):
    """A page of the fixture: a file under tests/golden/inputs, or "<n>": page n of synth_pages(seed=0)."""
    from PIL import Image

    from visrag_amd.synth import synth_pages
    if src.isdigit():
        return Image.fromarray(synth_pages(1, size=cfg.scale_resolution, seed=0, first=int(src))[0])
    return Image.open(os.path.join(HERE, "golden", "inputs", src)).convert("RGB")


def question_pages(F, cfg, q):
    return [page_image(cfg, str(s)) for s in F[f"q{q}_pages"]]


def msgs_of(F, q):
    return [{"role": "user", "content": str(F[f"q{q}_question"])}]


def _penalise(vals, ids, seen, pen):
    v = vals.copy()
    m = np.isin(ids, list(seen))
    v[m] = np.where(v[m] < 0, v[m] * np.float32(pen), v[m] / np.float32(pen)).astype(np.float32)
    return v


class BeamReplay:
    """The reference's per-(beam prefix) top-64 log_softmax rows of page P as the backend of the decode rules, the repetition
    penalty and the beam scores applied as the reference applies them (float32)."""

    def __init__(self, F, P):
        self.V, self.pen = 1000, float(F["pen_beam"])
        pre, ln = F[f"p{P}_beam_q_prefix"], F[f"p{P}_beam_q_len"]
        self.table = {tuple(pre[i, :ln[i]].tolist()): (F[f"p{P}_beam_q_ids"][i], F[f"p{P}_beam_q_logprobs"][i]) for i in range(len(ln))}
        self.seqs = [[]]

    def select(self, n, scores, k):
        cand = []
        for b in range(n):
            ids, lp = self.table[tuple(self.seqs[b])]
            v = _penalise(lp, ids, set(self.seqs[b]), self.pen) + np.float32(scores[b])
            cand += [(float(x), int(t), b) for x, t in zip(v, ids)]
        cand.sort(key=lambda c: (-c[0], c[2] * self.V + c[1]))
        return cand[:k]

    def advance(self, parents, tokens):
        self.seqs = [self.seqs[p] + [t] for p, t in zip(parents, tokens)]


def running_sets(tokens, parents):
    """the running beam sequences after every step, from the per-step (next tokens, parents)"""
    cur, out = [[]], []
    for t, p in zip(tokens, parents):
        cur = [cur[q] + [int(x)] for x, q in zip(t, p)]
        out.append(sorted(map(tuple, cur)))
    return out
