"""Record tests/golden/chat_tiny.npz: MiniCPM-V 2.0 answer generation by the REFERENCE model at the tiny dims.

The reference's own `llm.generate` does not run under the installed transformers (no GenerationMixin on MiniCPMForCausalLM,
then DynamicCache API drift), but its forward does.  So this script
  * builds the reference VisRAG_Ret (MiniCPMV) with oracle.ref_harness.build_reference_model on tiny_config(), the synthetic
    weights of visrag_amd.synth plus synth_lm_head (dim_model_base 256: the harness's value);
  * builds the prompts with the reference's own chat(): its prompt assembly and get_slice_image_placeholder run, and the call
    it makes to generate() is captured; then generate()'s _process_list / transform / get_vllm_embedding give the prompt's
    inputs_embeds — for tests/golden/inputs/cat.jpeg, dog.jpg and one text-only message;
  * drives model.llm(inputs_embeds=...) step by step over the FULL prefix (prompt embeddings + embed_tokens(generated) *
    scale_emb, what HF generate feeds after its first step) and applies a written-out statement of the transformers 4.40.2
    greedy search and beam search (BeamSearchScorer.process / BeamHypotheses / finalize) below — not the product's code.

Recorded per prompt (keys "p<i>_..."): prompt string and ids; greedy tokens, per-step top-64 raw logits (ids, values), the
penalised top-1 - top-2 margin and max |logit|; beam tokens and score, every (beam prefix -> top-64 log_softmax) the search
queried, the chosen next beams per step, the step's margin (smallest gap among the 2 * num_beams + 1 best candidates) and
max |logit|; the reference _decode_text of both results.

    python tools/gen_golden_chat.py            # writes tests/golden/chat_tiny.npz
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from oracle.ref_harness import build_reference_model  # noqa: E402
from visrag_amd.config import tiny_config  # noqa: E402
from visrag_amd.synth import synth_lm_head, synth_state_dict  # noqa: E402
from visrag_amd.tokenizer import StandInTokenizer  # noqa: E402

MAX_NEW = 20
NUM_BEAMS = 3
PEN_BEAM = 1.2
PEN_GREEDY = 1.2
TOP = 64
EOS = 2
QUESTIONS = ["What animal is in the picture?", "Describe the image.", "What is the capital of France?"]


class FixtureTokenizer(StandInTokenizer):
    """The stand-in tokenizer with a decode (ids -> "w<id>" words) for the reference's _decode_text."""

    def decode(self, ids):
        return " ".join(f"w{int(i)}" for i in ids) + " "


def penalise(scores, ids, penalty):
    """RepetitionPenaltyLogitsProcessor (4.40.2): gather the ids' scores, negative * penalty, positive / penalty, scatter."""
    s = scores.clone()
    if len(ids):
        idx = torch.tensor(sorted(set(ids)), dtype=torch.long)
        g = s[idx]
        s[idx] = torch.where(g < 0, g * penalty, g / penalty)
    return s


class RefLM:
    def __init__(self, model, prompt_embeds):
        self.model, self.pe = model, prompt_embeds

    @torch.no_grad()
    def logits(self, generated):
        emb = self.pe
        if generated:
            ids = torch.tensor([generated], dtype=torch.long)
            emb = torch.cat([emb, self.model.llm.model.embed_tokens(ids) * self.model.llm.config.scale_emb], dim=1)
        mask = torch.ones(emb.shape[:2], dtype=torch.long)
        return self.model.llm(inputs_embeds=emb, attention_mask=mask, use_cache=False).logits[0, -1].float()


def greedy(lm):
    toks, top_ids, top_v, margin, amax = [], [], [], [], []
    for _ in range(MAX_NEW):
        l = lm.logits(toks)
        v, i = torch.topk(l, TOP)
        top_ids.append(i.numpy()); top_v.append(v.numpy()); amax.append(float(l.abs().max()))
        p = penalise(l, toks, PEN_GREEDY)
        pv = torch.topk(p, 2).values
        margin.append(float(pv[0] - pv[1]))
        nxt = int(torch.argmax(p))
        toks.append(nxt)
        if nxt == EOS:
            break
    return toks, np.stack(top_ids), np.stack(top_v), np.array(margin), np.array(amax)


class Hyps:
    """BeamHypotheses (4.40.2), length_penalty 1.0, early_stopping False."""

    def __init__(self, n):
        self.n, self.beams, self.worst_score = n, [], 1e9

    def add(self, hyp, sum_logprobs, generated_len):
        score = sum_logprobs / generated_len
        if len(self.beams) < self.n or score > self.worst_score:
            self.beams.append((score, hyp))
            if len(self.beams) > self.n:
                s = sorted([(s, idx) for idx, (s, _) in enumerate(self.beams)])
                del self.beams[s[0][1]]
                self.worst_score = s[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self.beams) < self.n:
            return False
        return self.worst_score >= best_sum_logprobs / cur_len


def beam(lm, max_new=None, nbest=False):
    """_beam_search + BeamSearchScorer (4.40.2) for one item with inputs_embeds (input_ids start empty: decoder_prompt_len 0).
    nbest: also return every finished hypothesis as (score, output ids), best first — finalize's repeated
    `sorted(...).pop()`, what num_return_sequences > 1 and output_scores hand out as sequences / sequences_scores."""
    max_new = MAX_NEW if max_new is None else max_new
    V = lm.model.llm.config.vocab_size
    input_ids = [[] for _ in range(NUM_BEAMS)]
    beam_scores = torch.zeros(NUM_BEAMS)
    beam_scores[1:] = -1e9
    hyps = Hyps(NUM_BEAMS)
    queries, steps, done = {}, [], False
    for step in range(max_new):
        rows = []
        for b in range(NUM_BEAMS):
            key = tuple(input_ids[b])
            if key not in queries:
                logits = lm.logits(input_ids[b])
                lp = torch.log_softmax(logits, dim=-1)
                v, i = torch.topk(lp, TOP)
                queries[key] = (i.numpy(), v.numpy(), float(logits.abs().max()), step, lp)
            lp = queries[key][4]
            rows.append(penalise(lp, input_ids[b], PEN_BEAM) + beam_scores[b])
        scores = torch.stack(rows).view(-1)
        top_s, top_i = torch.topk(scores, 2 * NUM_BEAMS + 1, largest=True, sorted=True)
        margin = float((top_s[:-1] - top_s[1:]).min())
        amax = max(queries[tuple(input_ids[b])][2] for b in range(NUM_BEAMS) if beam_scores[b] > -1e8)
        next_scores, next_tokens = top_s[:-1], top_i[:-1]
        next_indices = next_tokens // V
        next_tokens = next_tokens % V
        cur_len = step + 1
        nb_scores, nb_tokens, nb_idx = [], [], []
        for rank, (tok, sc, idx) in enumerate(zip(next_tokens.tolist(), next_scores.tolist(), next_indices.tolist())):
            if tok == EOS:
                if rank >= NUM_BEAMS:
                    continue
                hyps.add(list(input_ids[idx]), sc, cur_len)
            else:
                nb_scores.append(sc); nb_tokens.append(tok); nb_idx.append(idx)
            if len(nb_scores) == NUM_BEAMS:
                break
        steps.append((nb_tokens, nb_idx, margin, amax))
        done = hyps.is_done(float(next_scores.max()), cur_len)
        if done:
            break
        input_ids = [input_ids[i] + [t] for i, t in zip(nb_idx, nb_tokens)]
        beam_scores = torch.tensor(nb_scores)
    if not done:                                              # finalize: the open beams join
        for b in range(NUM_BEAMS):
            hyps.add(list(input_ids[b]), float(beam_scores[b]), len(input_ids[b]))
    best_score, best = sorted(hyps.beams, key=lambda x: x[0]).pop()
    out = best + ([EOS] if len(best) < max_new else [])
    if nbest:
        ranked = [(sc, h + ([EOS] if len(h) < max_new else [])) for sc, h in sorted(hyps.beams, key=lambda x: x[0])[::-1]]
        return out, best_score, queries, steps, ranked
    return out, best_score, queries, steps


def main():
    cfg = tiny_config()
    W = dict(synth_state_dict(cfg, 0))
    W["llm.lm_head.weight"] = synth_lm_head(cfg, 0)
    model = build_reference_model(cfg, W)
    tok = FixtureTokenizer(cfg.vocab_size)
    images = [Image.open(os.path.join(ROOT, "tests", "golden", "inputs", n)).convert("RGB") for n in ("cat.jpeg", "dog.jpg")]
    cases = [(images[0], QUESTIONS[0]), (images[1], QUESTIONS[1]), (None, QUESTIONS[2])]
    out = {"max_new": np.int32(MAX_NEW), "num_beams": np.int32(NUM_BEAMS), "pen_beam": np.float32(PEN_BEAM),
           "pen_greedy": np.float32(PEN_GREEDY), "dim_model_base": np.float32(256.0), "n_prompts": np.int32(len(cases))}
    for p, (img, q) in enumerate(cases):
        captured = {}

        def fake_generate(data_list=None, img_list=None, **kw):
            captured.update(data_list=data_list, img_list=img_list)
            return [""], None

        model.generate = fake_generate
        if img is None:       # text-only: the chat() prompt layout without an image (its first message always carries one)
            data_list, img_list = ["<用户>" + q], [[]]
        else:
            model.chat([img], [[{"role": "user", "content": q}]], tok, sampling=False, max_new_tokens=MAX_NEW)
            data_list, img_list = captured["data_list"], captured["img_list"]
        del model.generate
        inputs = model._process_list(tok, data_list, 2048, padding_side="right")
        inputs["pixel_values"] = [[model.transform(im) for im in img_list[0]]]
        with torch.no_grad():
            embeds, _ = model.get_vllm_embedding(inputs)
        lm = RefLM(model, embeds)
        g_toks, g_ids, g_v, g_m, g_a = greedy(lm)
        b_toks, b_score, queries, steps = beam(lm)
        keys = list(queries)
        qp = np.full((len(keys), MAX_NEW), -1, dtype=np.int32)
        for i, k in enumerate(keys):
            qp[i, :len(k)] = k
        out.update({
            f"p{p}_prompt": np.array(data_list[0]), f"p{p}_ids": inputs["input_ids"][0].numpy().astype(np.int32),
            f"p{p}_n_slices": np.int32(len(img_list[0])),
            f"p{p}_greedy_tokens": np.array(g_toks, dtype=np.int32), f"p{p}_greedy_top_ids": g_ids.astype(np.int32),
            f"p{p}_greedy_top_logits": g_v.astype(np.float32), f"p{p}_greedy_margin": g_m.astype(np.float32),
            f"p{p}_greedy_absmax": g_a.astype(np.float32),
            f"p{p}_beam_tokens": np.array(b_toks, dtype=np.int32), f"p{p}_beam_score": np.float32(b_score),
            f"p{p}_beam_q_prefix": qp, f"p{p}_beam_q_len": np.array([len(k) for k in keys], dtype=np.int32),
            f"p{p}_beam_q_ids": np.stack([queries[k][0] for k in keys]).astype(np.int32),
            f"p{p}_beam_q_logprobs": np.stack([queries[k][1] for k in keys]).astype(np.float32),
            f"p{p}_beam_next_tokens": np.array([s[0] for s in steps], dtype=np.int32),
            f"p{p}_beam_next_parents": np.array([s[1] for s in steps], dtype=np.int32),
            f"p{p}_beam_margin": np.array([s[2] for s in steps], dtype=np.float32),
            f"p{p}_beam_absmax": np.array([s[3] for s in steps], dtype=np.float32),
            f"p{p}_greedy_text": np.array(model._decode_text([torch.tensor(g_toks)], tok)[0]),
            f"p{p}_beam_text": np.array(model._decode_text([torch.tensor(b_toks)], tok)[0]),
        })
        print(f"prompt {p}: {len(inputs['input_ids'][0])} ids, {len(img_list[0])} slices; greedy {g_toks}; beam {b_toks} "
              f"score {b_score:.4f}; {len(keys)} beam queries")
    path = os.path.join(ROOT, "tests", "golden", "chat_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
