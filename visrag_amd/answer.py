"""From the top-k pages of a retrieval run to one answer: the two single-image settings of the reference's generator script
(visrag_scripts/generate/generate.py) for MiniCPM-V 2.0.

* weighted selection: one beam-search answer per page, the page with the largest softmax(doc score) * exp(sequence score)
  answers (VisRAGRet.weighted_selection);
* page concatenation: the pages side by side (or stacked) in one image, one beam-search answer on it
  (generation_utils.py:171-247, generate.py:421-431).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

from PIL import Image


def top_pages(run: Dict[str, Dict[str, float]], qid: str, k: int) -> Tuple[List[str], List[float]]:
    """The k best (docid, score) of run[qid] (generate.py:285-296): by score, highest first; entries with equal scores keep
    the run's own order.  Fewer than k entries is an error."""
    ranked = sorted(run[qid].items(), key=lambda item: item[1], reverse=True)[:k]
    if len(ranked) < k:
        raise ValueError(f"the run holds {len(ranked)} pages for {qid!r}, fewer than topk={k}")
    return [d for d, _ in ranked], [s for _, s in ranked]


def concat_pages(images: Sequence[Image.Image], kind: str = "horizontal") -> Image.Image:
    """horizontal: every page scaled (bicubic) to the tallest page's height, width int(w * (max_h / h)) — the ratio first, as
    the reference computes it —, pasted left to right on a new RGB canvas; vertical: scaled to the widest page's width,
    height int(h * (max_w / w)), pasted top to bottom."""
    if kind not in ("horizontal", "vertical"):
        raise ValueError(f"kind={kind!r}: 'horizontal' or 'vertical'")
    images = list(images)
    if not images:
        raise ValueError("concat_pages needs at least one page")
    if kind == "horizontal":
        m = max(im.height for im in images)
        scaled = [im.resize((int(im.width * (m / im.height)), m), Image.Resampling.BICUBIC) for im in images]
        canvas = Image.new("RGB", (sum(im.width for im in scaled), m))
        x = 0
        for im in scaled:
            canvas.paste(im, (x, 0))
            x += im.width
    else:
        m = max(im.width for im in images)
        scaled = [im.resize((m, int(im.height * (m / im.width))), Image.Resampling.BICUBIC) for im in images]
        canvas = Image.new("RGB", (m, sum(im.height for im in scaled)))
        y = 0
        for im in scaled:
            canvas.paste(im, (0, y))
            y += im.height
    return canvas


def answer_weighted_selection(model, tokenizer, msgs, pages: Sequence[Image.Image], scores: Sequence[float],
                              max_new_tokens: int = 20, **kw):
    """generate.py's weighted_selection task for one query: `pages` and `scores` as top_pages orders them."""
    return model.weighted_selection(list(pages), msgs, list(scores), tokenizer, max_new_tokens=max_new_tokens, sampling=False, **kw)


def answer_marginal_selection(model, tokenizer, msgs, pages: Sequence[Image.Image], scores: Sequence[float],
                              max_new_tokens: int = 20, **kw):
    """Weighted selection with every candidate answer scored on every page (VisRAGRet.marginal_selection): pages that agree
    reinforce each other instead of competing.  `pages` and `scores` as top_pages orders them."""
    return model.marginal_selection(list(pages), msgs, list(scores), tokenizer, max_new_tokens=max_new_tokens, **kw)


def answer_page_concatenation(model, tokenizer, msgs, pages: Sequence[Image.Image], kind: str = "horizontal",
                              max_new_tokens: int = 20, sampling: bool = False, **kw) -> str:
    """generate.py's page_concatenation task for one query: one beam-search chat on the concatenated image.  sampling=True:
    the sampled answer of the answer-generation package's chat instead (nucleus top_p 0.8 / top_k 100, temperature 0.7,
    repetition_penalty 1.05; `seed` in kw selects the noise)."""
    image = concat_pages(pages, kind)
    if sampling:
        return model.chat([image], [msgs], tokenizer, sampling=True, max_new_tokens=max_new_tokens, assistant_turn=True,
                          answer_defaults=True, **kw)[0]
    return model.chat([image], [msgs], tokenizer, sampling=False, max_new_tokens=max_new_tokens, assistant_turn=True, **kw)[0]
