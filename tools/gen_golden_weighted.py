"""Record tests/golden/weighted_tiny.npz: weighted selection over the top-3 pages by the REFERENCE model at the tiny dims.

The reference's weighted-selection package (src/openmatch/modeling/weighted_selection/MiniCPMV20) cannot be imported here
(it needs peft), and its tower, resampler and LM forward are the retrieval package's math.  So this script builds the model as
tools/gen_golden_chat.py does, reuses that tool's forward-driven beam search, and applies the three differences of the
package's chat() (modeling_minicpmv.py:321-392):
  * the prompt ends in "<AI>";
  * _decode asks for num_return_sequences=2 with scores: the two best finished hypotheses' sequences_scores are recorded;
  * the sampling defaults differ (top_p 0.8 / top_k 100 / repetition_penalty 1.05) — never reached: weighted selection needs
    sequences_scores, which only beam search yields (generate.py always passes sampling=False).
and its weighted_selection (:394-425): p = softmax(doc_scores) (float32, as torch.tensor of Python floats gives), the page
with the largest p_i * exp(sequences_scores_i[0]) answers, the first among equals.

Three questions, k = 3 pages each, max_new 3.  Page keys are flat: page i of question q is "p<3q+i>_..." with the key layout
of chat_tiny.npz (ids, beam tokens / score, the queried (prefix -> top-64 log_softmax) rows, next beams, margin, absmax)
plus "beam_set_margin" (the gap that decides the step's running set: the rule of tests/test_gpu_chat.py) and "beam_scores2"
(sequences_scores, best first).  Per question "q<q>_...": question, page sources, doc_scores, probs, weights, index,
decisive.

Question 0 takes its pages from tests/golden/inputs; questions 1 and 2 take synth_pages whose seeds (PAGES below) were found
by `--search`: pages on which every beam step of the reference is decided by more than 4 x REF_BAR x max|logit| and the
best hypothesis leads by more than 2 x REF_BAR x max|logit|.  doc_scores are picked from a grid so that the winner leads by
more than exp(2 x REF_BAR x max|logit|), in question 1 against the page with the highest doc_score and in question 2
against the page with the best sequence score.  Every condition is checked before the file is written.

    python tools/gen_golden_weighted.py                      # writes tests/golden/weighted_tiny.npz
    python tools/gen_golden_weighted.py --search 3000 --q 1  # list decisive synth pages for question 1
"""
import argparse
import itertools
import math
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import gen_golden_chat as G  # noqa: E402
from oracle.ref_harness import build_reference_model  # noqa: E402
from visrag_amd.config import tiny_config  # noqa: E402
from visrag_amd.synth import synth_lm_head, synth_pages, synth_state_dict  # noqa: E402

MAX_NEW = 3
K = 3
REF_BAR = 1e-2          # tests/test_gpu_chat.py: device vs reference logits, relative to max |logit|
QUESTIONS = ["What animal or chart is on this page?", "What is the title?", "What is shown?"]
# per question its pages: a file under tests/golden/inputs, or the index of a synth_pages(seed=0) page
PAGES = [["cat.jpeg", "dog.jpg", "infovqa_0.jpg"], [6965, 2278, 7453], [975, 860, 2337]]
GRID = [round(0.30 + 0.05 * i, 2) for i in range(13)]      # doc_scores the tool picks from (inner products of unit vectors)


def prompt_embeds(model, tok, img, question):
    """The reference chat()'s prompt for (img, question) + "<AI>" -> (prompt, ids, n_slices, inputs_embeds)."""
    captured = {}

    def fake_generate(data_list=None, img_list=None, **kw):
        captured.update(data_list=data_list, img_list=img_list)
        return [""], None

    model.generate = fake_generate
    model.chat([img], [[{"role": "user", "content": question}]], tok, sampling=False, max_new_tokens=MAX_NEW)
    del model.generate
    data_list, img_list = [captured["data_list"][0] + "<AI>"], captured["img_list"]
    inputs = model._process_list(tok, data_list, 2048, padding_side="right")
    inputs["pixel_values"] = [[model.transform(im) for im in img_list[0]]]
    with torch.no_grad():
        embeds, _ = model.get_vllm_embedding(inputs)
    return data_list[0], inputs["input_ids"][0].numpy().astype(np.int32), len(img_list[0]), embeds


def set_margins(queries, steps, V):
    """Per beam step the score gap that decides its running set: between the last kept candidate and the next one, or, with
    an eos among the first num_beams + 1, the smallest gap among them.  From the full log-prob rows of the search."""
    nb, pen = G.NUM_BEAMS, G.PEN_BEAM
    seqs, scores, out = [[]], [0.0], []
    for toks, parents, _, _ in steps:
        rows = torch.stack([G.penalise(queries[tuple(q)][4], q, pen) + scores[b] for b, q in enumerate(seqs)]).view(-1)
        top_s, top_i = torch.topk(rows, nb + 1)
        gaps = (top_s[:-1] - top_s[1:]).tolist()
        out.append(min(gaps) if any(int(i) % V == G.EOS for i in top_i) else gaps[nb - 1])
        flat = {(int(i) // V, int(i) % V): float(s) for s, i in zip(*torch.topk(rows, 2 * nb))}
        scores = [flat[(p, t)] for t, p in zip(toks, parents)]
        seqs = [seqs[p] + [t] for t, p in zip(toks, parents)]
    return out


def run_page(model, tok, img, question):
    prompt, ids, n_slices, embeds = prompt_embeds(model, tok, img, question)
    lm = G.RefLM(model, embeds)
    toks, score, queries, steps, ranked = G.beam(lm, max_new=MAX_NEW, nbest=True)
    V = model.llm.config.vocab_size
    margins = set_margins(queries, steps, V)
    amax = [s[3] for s in steps]
    lead = ranked[0][0] - ranked[1][0] if len(ranked) > 1 else float("inf")
    decisive = all(m > 4 * REF_BAR * a for m, a in zip(margins, amax)) and lead > 2 * REF_BAR * max(amax)
    return {"prompt": prompt, "ids": ids, "n_slices": n_slices, "tokens": toks, "score": score, "queries": queries, "steps": steps,
            "ranked": ranked, "set_margins": margins, "amax": amax, "lead": lead, "decisive": decisive}


def quick_reject(model, tok, img, question):
    """The first beam step alone: most pages fail there (one forward instead of seven)."""
    _, _, _, embeds = prompt_embeds(model, tok, img, question)
    l = G.RefLM(model, embeds).logits([])
    v = torch.topk(torch.log_softmax(l, -1), G.NUM_BEAMS + 1).values
    return float(v[-2] - v[-1]) <= 4 * REF_BAR * float(l.abs().max())


def softmax32(doc_scores):
    return torch.nn.functional.softmax(torch.tensor(doc_scores), dim=0).tolist()


def pick_doc_scores(seq_scores, factor, want):
    """Three distinct grid values whose winner leads the runner-up by more than `factor` (the widest lead wins; ties: the
    first in grid order).  want: "not_top_doc" (the winner is not the page with the highest doc_score), "not_top_seq" (not
    the page with the best sequence score) or None."""
    best = None
    for ds in itertools.permutations(GRID, len(seq_scores)):
        p = softmax32(list(ds))
        w = [pi * math.exp(s) for pi, s in zip(p, seq_scores)]
        idx = w.index(max(w))
        order = sorted(w, reverse=True)
        lead = order[0] / order[1]
        if lead <= factor:
            continue
        if want == "not_top_doc" and idx == ds.index(max(ds)):
            continue
        if want == "not_top_seq" and idx == seq_scores.index(max(seq_scores)):
            continue
        if best is None or lead > best[0]:
            best = (lead, list(ds))
    return best


def page_image(cfg, src):
    if isinstance(src, str):
        return Image.open(os.path.join(ROOT, "tests", "golden", "inputs", src)).convert("RGB")
    return Image.fromarray(synth_pages(1, size=cfg.scale_resolution, seed=0, first=int(src))[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", type=int, default=0, help="scan this many synth pages for decisive ones and exit")
    ap.add_argument("--q", type=int, default=1, help="the question to search pages for")
    ap.add_argument("--first", type=int, default=0, help="the first synth page of the search")
    ap.add_argument("--question", default=None, help="search with this question text instead of QUESTIONS[--q]")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")
    cfg = tiny_config()
    W = dict(synth_state_dict(cfg, 0))
    W["llm.lm_head.weight"] = synth_lm_head(cfg, 0)
    model = build_reference_model(cfg, W)
    tok = G.FixtureTokenizer(cfg.vocab_size)

    if args.search:
        if args.question:
            QUESTIONS[args.q] = args.question
        for base in range(args.first, args.first + args.search, 50):
            pages = synth_pages(50, size=cfg.scale_resolution, seed=0, first=base)
            for k in range(50):
                img = Image.fromarray(pages[k])
                if quick_reject(model, tok, img, QUESTIONS[args.q]):
                    continue
                r = run_page(model, tok, img, QUESTIONS[args.q])
                if r["decisive"]:
                    print(f"page {base + k}: tokens {r['tokens']} score {r['score']:.4f} lead {r['lead']:.3f} "
                          f"min margin/bar {min(m / (4 * REF_BAR * a) for m, a in zip(r['set_margins'], r['amax'])):.2f} "
                          f"max|logit| {max(r['amax']):.2f}", flush=True)
        return

    out = {"max_new": np.int32(MAX_NEW), "num_beams": np.int32(G.NUM_BEAMS), "pen_beam": np.float32(G.PEN_BEAM),
           "dim_model_base": np.float32(256.0), "n_questions": np.int32(len(QUESTIONS)), "k": np.int32(K),
           "ref_bar": np.float32(REF_BAR)}
    wants = [None, "not_top_doc", "not_top_seq"]
    n_decisive, saw = 0, set()
    for q, question in enumerate(QUESTIONS):
        runs = [run_page(model, tok, page_image(cfg, src), question) for src in PAGES[q]]
        seq = [float(r["score"]) for r in runs]
        amax = max(max(r["amax"]) for r in runs)
        factor = math.exp(2 * REF_BAR * amax)
        picked = pick_doc_scores(seq, factor, wants[q]) or pick_doc_scores(seq, 1.0, None)
        doc_scores = picked[1]
        p = softmax32(doc_scores)
        weights = [pi * math.exp(s) for pi, s in zip(p, seq)]
        index = weights.index(max(weights))
        order = sorted(weights, reverse=True)
        decisive = all(r["decisive"] for r in runs) and order[0] / order[1] > factor
        if decisive:
            n_decisive += 1
            if index != doc_scores.index(max(doc_scores)):
                saw.add("not_top_doc")
            if index != seq.index(max(seq)):
                saw.add("not_top_seq")
        out.update({f"q{q}_question": np.array(question), f"q{q}_pages": np.array([str(s) for s in PAGES[q]]),
                    f"q{q}_doc_scores": np.array(doc_scores, dtype=np.float64), f"q{q}_probs": np.array(p, dtype=np.float64),
                    f"q{q}_weights": np.array(weights, dtype=np.float64), f"q{q}_index": np.int32(index),
                    f"q{q}_decisive": np.bool_(decisive), f"q{q}_absmax": np.float32(amax)})
        for i, r in enumerate(runs):
            P = q * K + i
            keys = list(r["queries"])
            qp = np.full((len(keys), MAX_NEW), -1, dtype=np.int32)
            for j, key in enumerate(keys):
                qp[j, :len(key)] = key
            out.update({
                f"p{P}_prompt": np.array(r["prompt"]), f"p{P}_ids": r["ids"], f"p{P}_n_slices": np.int32(r["n_slices"]),
                f"p{P}_beam_tokens": np.array(r["tokens"], dtype=np.int32), f"p{P}_beam_score": np.float32(r["score"]),
                f"p{P}_beam_scores2": np.array([s for s, _ in r["ranked"][:2]], dtype=np.float32),
                f"p{P}_beam_tokens2": np.array(r["ranked"][1][1] if len(r["ranked"]) > 1 else [], dtype=np.int32),
                f"p{P}_beam_q_prefix": qp, f"p{P}_beam_q_len": np.array([len(key) for key in keys], dtype=np.int32),
                f"p{P}_beam_q_ids": np.stack([r["queries"][key][0] for key in keys]).astype(np.int32),
                f"p{P}_beam_q_logprobs": np.stack([r["queries"][key][1] for key in keys]).astype(np.float32),
                f"p{P}_beam_next_tokens": np.array([s[0] for s in r["steps"]], dtype=np.int32),
                f"p{P}_beam_next_parents": np.array([s[1] for s in r["steps"]], dtype=np.int32),
                f"p{P}_beam_margin": np.array([s[2] for s in r["steps"]], dtype=np.float32),
                f"p{P}_beam_set_margin": np.array(r["set_margins"], dtype=np.float32),
                f"p{P}_beam_absmax": np.array(r["amax"], dtype=np.float32), f"p{P}_decisive": np.bool_(r["decisive"]),
            })
            print(f"q{q} page {PAGES[q][i]}: {len(r['ids'])} ids, {r['n_slices']} slices; beam {r['tokens']} score {r['score']:.4f} "
                  f"lead {r['lead']:.3f} decisive {r['decisive']}")
        print(f"q{q}: doc_scores {doc_scores} weights {[round(w, 4) for w in weights]} -> page {index}; lead "
              f"{order[0] / order[1]:.3f} vs {factor:.3f}; decisive {decisive}")
    if n_decisive < 2 or saw != {"not_top_doc", "not_top_seq"}:
        raise SystemExit(f"refusing to write: {n_decisive} fully decisive questions, conditions met: {sorted(saw)} "
                         "(need two, one whose winner is not the top doc_score and one whose winner is not the best sequence score)")
    path = os.path.join(ROOT, "tests", "golden", "weighted_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
