"""MiniCPM-V 2.0 answer generation (the generator VisRAG pairs with its retriever) on the VisRAG-Ret weights.

Mirrors the reference's `MiniCPMV.generate` / `chat` (src/openmatch/modeling/modeling_minicpmv/modeling_minicpmv.py:218-237,
276-400) and the HF generate rules they rely on (the reference pins transformers==4.40.2):

* beam search (`chat(sampling=False)`: num_beams=3, repetition_penalty=1.2): per row log_softmax, then the repetition
  penalty (negative scores * penalty, positive / penalty) on that beam's GENERATED ids, plus the beam score; the top
  2 * num_beams of num_beams x vocab per prompt.  An eos among the first num_beams candidates closes a hypothesis with score
  sum_logprobs / generated_len ** length_penalty, where generated_len counts the eos (4.40.2 `process` adds with
  cur_len = generated tokens + 1; 5.x `_update_finished_beams` divides by cur_len + 1 - prompt_len: the same).  length_penalty
  1.0, early_stopping=False: an item is done when it holds num_beams hypotheses and worst_score >= best candidate score /
  cur_len.  After max_new_tokens the running beams join the hypotheses (length = max_new_tokens); the best hypothesis wins
  (ties: the one added last, like `sorted(...).pop()`), followed by one eos when shorter than max_new_tokens.  The 5.x
  `n_tokens_to_keep` / `beams_to_keep` cut is the same 2 * num_beams with one eos id.  Initial beam scores are 0 for beam 0
  and -1e9 for the others: the first step's candidates all come from beam 0, so it is run on that one row.
* greedy (num_beams=1, do_sample=False): penalty on the raw logits, argmax (lowest id on ties), stop after eos.
* sampling (`chat(sampling=True)`: temperature 0.7, repetition_penalty 1.02): penalty, / temperature, top_k 50 (HF's
  default), softmax, one draw — here from counter-based noise selected by (seed, step), so a seed reproduces a run; the
  reference draws from torch's global generator.
* nucleus sampling (the answer-generation package's `chat(sampling=True)`: top_p 0.8, top_k 100, temperature 0.7,
  repetition_penalty 1.05): penalty, / temperature, top-k, top-p (min_tokens_to_keep 1), softmax, one draw — a second
  sampler (`NucleusSampling`, `HipChat.sample`, `generate_items(nucleus=...)`) beside the one above, same noise.
* Generation starts from `inputs_embeds` (modeling_minicpmv.py:218-226), so HF starts `input_ids` EMPTY: the repetition
  penalty only ever sees generated tokens, never the prompt.

* scoring (`HipChat.score`, `score_items`, `sequence_score`): the log-probs of GIVEN continuations from one packed
  teacher-forced pass (vr_chat_score); since the penalty follows the log-softmax, the beam's sequence score of a forced
  continuation is a host function of per-position (logit, log-sum-exp) alone.

Batches: every item is generated independently — an item's output is a function of the item alone.  The reference
right-pads a batch (`_process_list(padding_side="right")`) and a shorter item then continues after pad rows of the longer
ones; that behaviour is NOT reproduced (parity is defined per item).

The decoding rules are generators of `select` / `advance` requests: `run_rule` drives one against any backend (the tests
replay recorded log-probs), `generate_items` serves the requests of all items of a batch in one device call per phase.
Options HF would accept but this generator does not implement (top_p, length_penalty, beam sampling, ...) raise
NotImplementedError instead of being dropped.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

EOS_ID, PAD_ID, BOS_ID = 2, 0, 1
GREEDY, BEAM, SAMPLE = 0, 1, 2


# ------------------------------------------------------------------------------------------ config ---
@dataclass
class GenerationConfig:
    """The MiniCPM-V 2.0 checkpoint fields the generator needs beyond VisRAGRetConfig (config.json)."""
    dim_model_base: float = 256.0
    tie_word_embeddings: bool = False
    eos_token_id: int = EOS_ID
    pad_token_id: int = PAD_ID


def generation_config_from_checkpoint(path: str) -> GenerationConfig:
    with open(os.path.join(path, "config.json")) as f:
        j = json.load(f)
    g = GenerationConfig()
    g.dim_model_base = float(j.get("dim_model_base", g.dim_model_base))
    g.tie_word_embeddings = bool(j.get("tie_word_embeddings", g.tie_word_embeddings))
    return g


def chat_generation_config(sampling: bool, kwargs: Dict) -> Dict:
    """modeling_minicpmv.py:369-383: the defaults of the mode, and only THEIR keys overridden from kwargs."""
    if sampling:
        cfg = {"temperature": 0.7, "do_sample": True, "repetition_penalty": 1.02}
    else:
        cfg = {"num_beams": 3, "repetition_penalty": 1.2}
    cfg.update((k, kwargs[k]) for k in cfg.keys() & kwargs.keys())
    return cfg


def answer_chat_generation_config(sampling: bool, kwargs: Dict) -> Dict:
    """The chat defaults of the reference's answer-generation package (weighted_selection/MiniCPMV20/modeling_minicpmv.py:
    361-377) and its merge rule: the defaults of the mode, and only THEIR keys overridden from kwargs.  Its sampled answer is
    a nucleus: top_p 0.8 over the top_k 100 (generate_items(nucleus=NucleusSampling(top_p, top_k)))."""
    if sampling:
        cfg = {"top_p": 0.8, "top_k": 100, "temperature": 0.7, "do_sample": True, "repetition_penalty": 1.05}
    else:
        cfg = {"num_beams": 3, "repetition_penalty": 1.2}
    cfg.update((k, kwargs[k]) for k in cfg.keys() & kwargs.keys())
    return cfg


@dataclass(frozen=True)
class NucleusSampling:
    """top_p over the top_k best (top_k = 0: over the whole vocabulary) — the sampler of vr_chat_sample (include/visrag_hip.h
    holds the definition).  Checked as the C ABI checks: 0 < top_p <= 1, top_k >= 0."""
    top_p: float = 0.8
    top_k: int = 100

    def __post_init__(self):
        if isinstance(self.top_k, bool) or int(self.top_k) != self.top_k or self.top_k < 0:
            raise ValueError(f"top_k={self.top_k!r}: 0 (off) or a positive integer")
        if not (0.0 < float(self.top_p) <= 1.0):                 # (a NaN fails both comparisons)
            raise ValueError(f"top_p={self.top_p!r}: must be in (0, 1]")


def decode_text(result_ids: Sequence[Sequence[int]], tokenizer) -> List[str]:
    """modeling_minicpmv.py:228-237: drop 0s, a leading bos and a trailing eos, decode, strip."""
    out = []
    for result in result_ids:
        r = [int(t) for t in result if int(t) != 0]
        if r and r[0] == tokenizer.bos_id:
            r = r[1:]
        if r and r[-1] == tokenizer.eos_id:
            r = r[:-1]
        out.append(tokenizer.decode(r).strip())
    return out


# ------------------------------------------------------------------------------------- decode rules ---
class _Hyps:
    """BeamHypotheses of HF 4.40.2 (length_penalty, early_stopping=False)."""

    def __init__(self, num_beams: int, length_penalty: float = 1.0):
        self.n, self.lp = num_beams, length_penalty
        self.beams: List[Tuple[float, List[int]]] = []
        self.worst = 1e9

    def add(self, tokens: List[int], sum_logprobs: float, generated_len: int) -> None:
        score = sum_logprobs / (generated_len ** self.lp)
        if len(self.beams) < self.n or score > self.worst:
            self.beams.append((score, list(tokens)))
            if len(self.beams) > self.n:
                order = sorted((s, i) for i, (s, _) in enumerate(self.beams))
                del self.beams[order[0][1]]
                self.worst = order[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best_sum_logprobs: float, cur_len: int) -> bool:
        if len(self.beams) < self.n:
            return False
        return self.worst >= best_sum_logprobs / (cur_len ** self.lp)

    def best(self) -> Tuple[float, List[int]]:
        return sorted(self.beams, key=lambda x: x[0]).pop()

    def ranked(self) -> List[Tuple[float, List[int]]]:
        """Best first, in the order repeated `sorted(...).pop()` (HF's finalize) hands them out: among equal scores the one
        added last comes first."""
        return sorted(self.beams, key=lambda x: x[0])[::-1]


def beam_rule(num_beams: int, max_new_tokens: int, eos: int = EOS_ID, length_penalty: float = 1.0):
    """One item's beam search as a generator of requests: yields ("select", n_rows, beam_scores, k) and receives the
    candidates [(score, token, parent)] best first over the first n_rows beams; yields ("advance", parents, tokens) (beam i
    continues beam parents[i] with tokens[i]) and receives None.  Returns {"tokens": output ids (one eos appended when
    shorter than max_new_tokens), "score": the best hypothesis score, "steps": [(candidates, next beams)] per step,
    "hyps": every finished hypothesis as (score, output ids), best first — HF's sequences_scores / sequences for
    num_return_sequences up to num_beams; hyps[0] is (score, tokens)}."""
    hyps = _Hyps(num_beams, length_penalty)
    seqs: List[List[int]] = [[]]
    scores = [0.0]
    done = False
    steps = []
    for step in range(max_new_tokens):
        cand = yield ("select", len(seqs), list(scores), 2 * num_beams)
        cur_len = step + 1
        nxt = []
        for rank, (s, tok, par) in enumerate(cand):
            if tok == eos:
                if rank >= num_beams:
                    continue
                hyps.add(seqs[par], s, cur_len)
            else:
                nxt.append((s, tok, par))
            if len(nxt) == num_beams:
                break
        steps.append((list(cand), list(nxt)))
        done = hyps.is_done(cand[0][0], cur_len)
        if done:
            break
        seqs = [seqs[p] + [t] for _, t, p in nxt]
        scores = [s for s, _, _ in nxt]
        if step + 1 == max_new_tokens:
            break
        yield ("advance", [p for _, _, p in nxt], [t for _, t, _ in nxt])
    if not done:
        for s, q in zip(scores, seqs):
            hyps.add(q, s, len(q))
    ranked = [(sc, q + ([eos] if len(q) < max_new_tokens else [])) for sc, q in hyps.ranked()]
    score, tokens = ranked[0]
    return {"tokens": tokens, "score": score, "steps": steps, "hyps": ranked}


def greedy_rule(max_new_tokens: int, eos: int = EOS_ID):
    """One item, greedy search or sampling (the draw is the device's select with k = 1): the request protocol of beam_rule."""
    tokens, steps = [], []
    for step in range(max_new_tokens):
        s, tok, _ = (yield ("select", 1, [0.0], 1))[0]
        tokens.append(tok)
        steps.append(s)
        if tok == eos or step + 1 == max_new_tokens:
            break
        yield ("advance", [0], [tok])
    return {"tokens": tokens, "scores": steps}


def run_rule(rule, backend) -> Dict:
    """Drive one rule against a backend with select(n_rows, beam_scores, k) and advance(parents, tokens)."""
    try:
        req = next(rule)
        while True:
            if req[0] == "select":
                req = rule.send(backend.select(req[1], req[2], req[3]))
            else:
                backend.advance(req[1], req[2])
                req = rule.send(None)
    except StopIteration as stop:
        return stop.value


def beam_search(backend, num_beams: int, max_new_tokens: int, eos: int = EOS_ID, length_penalty: float = 1.0) -> Dict:
    return run_rule(beam_rule(num_beams, max_new_tokens, eos, length_penalty), backend)


def greedy_search(backend, max_new_tokens: int, eos: int = EOS_ID) -> Dict:
    return run_rule(greedy_rule(max_new_tokens, eos), backend)


# ------------------------------------------------------------------------------------------ device ---
class HipChat:
    """Owner of a vr_chat_t: prompt slots, beam rows, KV cache and the logits processing on the device."""

    def __init__(self, encoder, max_len: int, max_rows: int = 3, dim_model_base: float = 256.0, max_slots: Optional[int] = None,
                 max_new: Optional[int] = None):
        """max_len: positions of a sequence (prompt + generated); max_rows: rows of a step (prompts x beams); max_slots:
        prompts held at once (default max_rows); max_new: generated tokens a row holds (default max_len - 1)."""
        self.lib, self.enc = _lib.load(), encoder
        self.device = encoder.device
        self.max_len, self.max_rows = int(max_len), int(max_rows)
        self.max_slots = int(max_slots) if max_slots else self.max_rows
        self.max_new = int(max_new) if max_new else self.max_len - 1
        self.V = encoder.cfg.vocab_size
        c = _lib.VRChatConfig(max_len=self.max_len, max_rows=self.max_rows, dim_model_base=float(dim_model_base),
                              max_slots=self.max_slots, max_new=self.max_new)
        self.prefills = 0                 # prefill / prefill_batch calls so far (a statistic: tests count them)
        self._slot_item = {}              # slot -> (ids, slices) of the item this wrapper prefilled there, with the slot's generation
        self._h = C.c_void_p()
        _lib.check(self.lib.vr_chat_create(encoder._h, C.byref(c), C.byref(self._h)), "vr_chat_create")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.vr_chat_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(int(torch.cuda.current_stream(self.device).cuda_stream))

    def load_head(self, t: torch.Tensor) -> None:
        dt = _lib.VR_DTYPE_BF16 if t.dtype == torch.bfloat16 else _lib.VR_DTYPE_F32
        t = (t if dt == _lib.VR_DTYPE_BF16 else t.to(torch.float32)).contiguous()
        shape = (C.c_int64 * 2)(*t.shape)
        _lib.check(self.lib.vr_chat_load_head(self._h, C.c_void_p(t.data_ptr()), shape, 2, dt, 1 if t.is_cuda else 0), "vr_chat_load_head")

    def prefill(self, slot: int, row: int, item) -> None:
        """One PreparedItem (token ids, image bounds, u8 slices) into prompt `slot`; its logits land on `row`."""
        Q = self.enc.cfg.query_num
        ids = np.ascontiguousarray(np.asarray(item.input_ids, dtype=np.int32))
        n = len(item.slices)
        keep = [np.ascontiguousarray(s, dtype=np.uint8) for s in item.slices]
        if n:
            ptrs = (C.c_void_p * n)(*[C.c_void_p(a.ctypes.data) for a in keep])
            hw = (C.c_int32 * (2 * n))(*[v for a in keep for v in (a.shape[0], a.shape[1])])
            rows = np.full((n, Q), -1, dtype=np.int32)
            for k, (b0, b1) in enumerate(item.image_bound[:n]):
                m = max(0, min(Q, b1 - b0))
                rows[k, :m] = b0 + np.arange(m, dtype=np.int32)
            rows = np.ascontiguousarray(rows.reshape(-1))
            rp = rows.ctypes.data_as(C.POINTER(C.c_int32))
        else:
            ptrs, hw, rp = None, None, None
        self.prefills += 1
        _lib.check(self.lib.vr_chat_prefill(self._h, int(slot), int(row), ptrs, hw, n, 0, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                            len(ids), rp, self._stream()), "vr_chat_prefill")
        self._remember(slot, item)

    def prefill_batch(self, slots: Sequence[int], rows: Sequence[int], items: Sequence) -> None:
        """PreparedItems in ONE packed pass: item b into prompt slot slots[b], its logits on row rows[b] (vr_chat_prefill_batch).
        The caller keeps the batch inside the encoder workspace (max_tokens, max_seqs)."""
        B, Q = len(items), self.enc.cfg.query_num
        if not (B == len(slots) == len(rows)) or B < 1:
            raise ValueError("prefill_batch needs one slot and one row per item, and at least one item")
        ids = np.ascontiguousarray(np.concatenate([np.asarray(it.input_ids, dtype=np.int32) for it in items]))
        off = np.zeros(B + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(it.input_ids) for it in items])
        keep, vrows = [], []
        for b, it in enumerate(items):
            n = len(it.slices)
            keep += [np.ascontiguousarray(s, dtype=np.uint8) for s in it.slices]
            r = np.full((n, Q), -1, dtype=np.int32)
            for k, (b0, b1) in enumerate(it.image_bound[:n]):
                m = max(0, min(Q, b1 - b0))
                r[k, :m] = int(off[b]) + b0 + np.arange(m, dtype=np.int32)
            vrows.append(r.reshape(-1))
        n = len(keep)
        if n:
            ptrs = (C.c_void_p * n)(*[C.c_void_p(a.ctypes.data) for a in keep])
            hw = (C.c_int32 * (2 * n))(*[v for a in keep for v in (a.shape[0], a.shape[1])])
            vr = np.ascontiguousarray(np.concatenate(vrows))
            rp = vr.ctypes.data_as(C.POINTER(C.c_int32))
        else:
            ptrs, hw, rp = None, None, None
        a = lambda v: (C.c_int32 * B)(*[int(x) for x in v])
        p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        self.prefills += 1
        _lib.check(self.lib.vr_chat_prefill_batch(self._h, B, a(slots), a(rows), ptrs, hw, n, 0, p32(ids), p32(off), rp, self._stream()),
                   "vr_chat_prefill_batch")
        for sl, it in zip(slots, items):
            self._remember(sl, it)

    def step(self, slots: Sequence[int], rows: Sequence[int], tokens: Sequence[int]) -> None:
        n = len(rows)
        a = lambda v: (C.c_int32 * n)(*[int(x) for x in v])
        _lib.check(self.lib.vr_chat_step(self._h, n, a(slots), a(rows), a(tokens), self._stream()), "vr_chat_step")

    def select(self, mode: int, groups: Sequence[Sequence[int]], k: int, beam_scores: Optional[Sequence[float]] = None,
               repetition_penalty: float = 1.0, temperature: float = 1.0, top_k: int = 50, seed: int = 0, step: int = 0):
        """-> (scores, tokens, parents), each [len(groups)][k] numpy."""
        rows = [int(r) for g in groups for r in g]
        off = np.cumsum([0] + [len(g) for g in groups]).astype(np.int32)
        G, n = len(groups), len(rows)
        bs = (C.c_float * n)(*([float(x) for x in beam_scores] if beam_scores is not None else [0.0] * n))
        sc = np.zeros((G, k), dtype=np.float32)
        tk = np.zeros((G, k), dtype=np.int32)
        pa = np.zeros((G, k), dtype=np.int32)
        p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        _lib.check(self.lib.vr_chat_select(self._h, int(mode), G, p32(off), (C.c_int32 * n)(*rows), bs, int(k), float(repetition_penalty),
                                           float(temperature), int(top_k), C.c_uint64(int(seed) & (2 ** 64 - 1)), int(step),
                                           sc.ctypes.data_as(C.POINTER(C.c_float)), p32(tk), p32(pa), self._stream()), "vr_chat_select")
        return sc, tk, pa

    def sample(self, rows: Sequence[int], repetition_penalty: float = 1.0, temperature: float = 1.0, top_k: int = 100,
               top_p: float = 0.8, seed: int = 0, step: int = 0):
        """One nucleus draw per row (vr_chat_sample) -> (scores, tokens, kept, cut), each [len(rows)] numpy."""
        n = len(rows)
        sc = np.zeros(n, dtype=np.float32)
        tk, kept, cut = (np.zeros(n, dtype=np.int32) for _ in range(3))
        p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        _lib.check(self.lib.vr_chat_sample(self._h, n, (C.c_int32 * n)(*[int(r) for r in rows]), float(repetition_penalty),
                                           float(temperature), int(top_k), float(top_p), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                           int(step), sc.ctypes.data_as(C.POINTER(C.c_float)), p32(tk), p32(kept), p32(cut),
                                           self._stream()), "vr_chat_sample")
        return sc, tk, kept, cut

    def reorder(self, rows: Sequence[int], parents: Sequence[int]) -> None:
        n = len(rows)
        a = lambda v: (C.c_int32 * n)(*[int(x) for x in v])
        _lib.check(self.lib.vr_chat_reorder(self._h, n, a(rows), a(parents), self._stream()), "vr_chat_reorder")

    def logits(self, row: int) -> np.ndarray:
        out = np.empty(self.V, dtype=np.float32)
        _lib.check(self.lib.vr_chat_logits(self._h, int(row), C.c_void_p(out.ctypes.data), self._stream()), "vr_chat_logits")
        return out

    def row_state(self, row: int) -> Tuple[int, int]:
        s, g = C.c_int32(), C.c_int32()
        _lib.check(self.lib.vr_chat_row_len(self._h, int(row), C.byref(s), C.byref(g)), "vr_chat_row_len")
        return int(s.value), int(g.value)

    def score(self, items: Sequence, cont_lens: Sequence[int]) -> List[Dict[str, np.ndarray]]:
        """Teacher-forced scoring of PreparedItems in ONE packed pass (vr_chat_score): the last cont_lens[b] tokens of item b
        are its continuation.  Per item dict(logit, lse, top_logit, top_token), numpy [cont_lens[b]]: the logit of each
        continuation token, the log-sum-exp of its row, the row's largest logit and its token.  Touches no slot, row or
        logits of a generation in progress.  The caller keeps the batch inside the encoder workspace (max_tokens, max_seqs)."""
        B, Q = len(items), self.enc.cfg.query_num
        if B < 1 or B != len(cont_lens):
            raise ValueError("score needs at least one item and one continuation length per item")
        ids = np.ascontiguousarray(np.concatenate([np.asarray(it.input_ids, dtype=np.int32) for it in items]))
        off = np.zeros(B + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(it.input_ids) for it in items])
        cl = np.ascontiguousarray(np.asarray([int(c) for c in cont_lens], dtype=np.int32))
        keep, vrows = [], []
        for b, it in enumerate(items):
            n = len(it.slices)
            keep += [np.ascontiguousarray(s, dtype=np.uint8) for s in it.slices]
            r = np.full((n, Q), -1, dtype=np.int32)
            for k, (b0, b1) in enumerate(it.image_bound[:n]):
                m = max(0, min(Q, b1 - b0))
                r[k, :m] = int(off[b]) + b0 + np.arange(m, dtype=np.int32)
            vrows.append(r.reshape(-1))
        n = len(keep)
        if n:
            ptrs = (C.c_void_p * n)(*[C.c_void_p(a.ctypes.data) for a in keep])
            hw = (C.c_int32 * (2 * n))(*[v for a in keep for v in (a.shape[0], a.shape[1])])
            vr = np.ascontiguousarray(np.concatenate(vrows))
            rp = vr.ctypes.data_as(C.POINTER(C.c_int32))
        else:
            ptrs, hw, rp = None, None, None
        M = int(np.clip(cl, 0, None).sum())
        logit, lse, top = (np.zeros(max(M, 1), dtype=np.float32) for _ in range(3))
        tok = np.zeros(max(M, 1), dtype=np.int32)
        p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        _lib.check(self.lib.vr_chat_score(self._h, B, ptrs, hw, n, 0, p32(ids), p32(off), rp, p32(cl), pf(logit), pf(lse), pf(top),
                                          p32(tok), self._stream()), "vr_chat_score")
        out, m = [], 0
        for c in cl.tolist():
            out.append({"logit": logit[m:m + c].copy(), "lse": lse[m:m + c].copy(), "top_logit": top[m:m + c].copy(),
                        "top_token": tok[m:m + c].copy()})
            m += c
        return out

    _SEEN_MODES = {"keep": 0, "join": 1, "clear": 2}

    def extend(self, slots: Sequence[int], rows: Sequence[int], token_lists: Sequence[Sequence[int]],
               targets: Optional[Sequence[Sequence[int]]] = None, seen: str = "keep") -> Optional[List[Dict[str, np.ndarray]]]:
        """Append token_lists[b] to row rows[b] of the cached prompt slots[b], all rows in ONE packed decoder pass
        (vr_chat_extend).  Afterwards a row's logits are those after its last appended token.  seen: "keep" leaves the rows'
        seen sets alone, "join" adds the appended ids, "clear" empties them (a new turn).  targets (one list per row, as long
        as its tokens, -1 = none): entry j is the distribution AFTER token j evaluated at targets[b][j] -> per row
        dict(logit, lse, top_logit, top_token), numpy [len(tokens)]; entries without a target hold (nan, nan, nan, -1).
        Without targets nothing is returned and the stream is not synchronised."""
        if seen not in self._SEEN_MODES:
            raise ValueError(f"seen={seen!r}: 'keep', 'join' or 'clear'")
        B = len(token_lists)
        if B < 1 or not (B == len(slots) == len(rows)):
            raise ValueError("extend needs one slot, one row and one token list per sequence, and at least one")
        lens = [len(t) for t in token_lists]
        off = np.zeros(B + 1, dtype=np.int32)
        off[1:] = np.cumsum(lens)
        M = int(off[B])
        toks = np.ascontiguousarray(np.asarray([int(t) for tl in token_lists for t in tl], dtype=np.int32))
        p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        a = lambda v: (C.c_int32 * B)(*[int(x) for x in v])
        tp = lo = ls = tl_ = tt = None
        if targets is not None:
            if len(targets) != B or any(len(t) != n for t, n in zip(targets, lens)):
                raise ValueError("extend needs one target per appended token (-1 = none)")
            tg = np.ascontiguousarray(np.asarray([int(t) for tl in targets for t in tl], dtype=np.int32))
            logit, lse, top = (np.full(max(M, 1), np.nan, dtype=np.float32) for _ in range(3))
            tok = np.full(max(M, 1), -1, dtype=np.int32)
            tp, lo, ls, tl_, tt = p32(tg), pf(logit), pf(lse), pf(top), p32(tok)
        _lib.check(self.lib.vr_chat_extend(self._h, B, a(slots), a(rows), p32(off), p32(toks) if M else None, tp,
                                           self._SEEN_MODES[seen], lo, ls, tl_, tt, self._stream()), "vr_chat_extend")
        if targets is None:
            return None
        return [{"logit": logit[off[b]:off[b + 1]].copy(), "lse": lse[off[b]:off[b + 1]].copy(),
                 "top_logit": top[off[b]:off[b + 1]].copy(), "top_token": tok[off[b]:off[b + 1]].copy()} for b in range(B)]

    def row_score(self, rows: Sequence[int], targets: Sequence[int]) -> Dict[str, np.ndarray]:
        """The four numbers of `score` from the CURRENT logits of rows[i] at targets[i] (vr_chat_row_score; rows may repeat)
        -> dict(logit, lse, top_logit, top_token), numpy [len(rows)]."""
        n = len(rows)
        if n < 1 or n != len(targets):
            raise ValueError("row_score needs at least one row and one target per row")
        logit, lse, top = (np.zeros(n, dtype=np.float32) for _ in range(3))
        tok = np.zeros(n, dtype=np.int32)
        a = lambda v: (C.c_int32 * n)(*[int(x) for x in v])
        p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        _lib.check(self.lib.vr_chat_row_score(self._h, n, a(rows), a(targets), pf(logit), pf(lse), pf(top), p32(tok), self._stream()),
                   "vr_chat_row_score")
        return {"logit": logit, "lse": lse, "top_logit": top, "top_token": tok}

    def slot_score(self, slots: Sequence[int], targets: Sequence[int]) -> Dict[str, np.ndarray]:
        """`row_score` from the logits of the slots' PROMPTS (their last position): they outlive a generation on the slot and
        are lost when the row the prefill named is prefilled or extended again (vr_chat_slot_score)."""
        n = len(slots)
        if n < 1 or n != len(targets):
            raise ValueError("slot_score needs at least one slot and one target per slot")
        logit, lse, top = (np.zeros(n, dtype=np.float32) for _ in range(3))
        tok = np.zeros(n, dtype=np.int32)
        a = lambda v: (C.c_int32 * n)(*[int(x) for x in v])
        p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        _lib.check(self.lib.vr_chat_slot_score(self._h, n, a(slots), a(targets), pf(logit), pf(lse), pf(top), p32(tok), self._stream()),
                   "vr_chat_slot_score")
        return {"logit": logit, "lse": lse, "top_logit": top, "top_token": tok}

    def _slot_state(self, slot: int) -> Tuple[int, bool, int]:
        n, ok, gen = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.vr_chat_slot_state(self._h, int(slot), C.byref(n), C.byref(ok), C.byref(gen)), "vr_chat_slot_state")
        return int(n.value), bool(ok.value), int(gen.value)

    def slot_state(self, slot: int) -> Tuple[int, bool]:
        """-> (prompt tokens the slot holds, whether `slot_score` can still read the prompt's logits)"""
        return self._slot_state(slot)[:2]

    def slot_generation(self, slot: int) -> int:
        """How often the slot has been prefilled, counted by the library whoever called it: a caller that keeps a prompt in
        a slot compares it with the count it saw after its own prefill."""
        return self._slot_state(slot)[2]

    def _remember(self, slot: int, item) -> None:
        self._slot_item[int(slot)] = ([int(t) for t in item.input_ids], [np.asarray(s) for s in item.slices],
                                      self.slot_generation(slot))

    def slot_holds(self, slot: int, item) -> bool:
        """Does `slot` hold exactly this item's prompt — the ids and slices this wrapper prefilled there, and nobody (this
        wrapper, another one of the same handle, the C API) has prefilled the slot since?"""
        rec = self._slot_item.get(int(slot))
        if rec is None or rec[2] != self.slot_generation(slot):
            return False
        ids, slices, _ = rec
        return (ids == [int(t) for t in item.input_ids] and len(slices) == len(item.slices) and
                all(a.shape == np.asarray(b).shape and np.array_equal(a, b) for a, b in zip(slices, item.slices)))

    def truncate(self, row: int, length: int) -> None:
        """Shorten the tail of `row` to `length` tokens; the row loses its logits, its seen set stays (vr_chat_row_truncate)."""
        _lib.check(self.lib.vr_chat_row_truncate(self._h, int(row), int(length)), "vr_chat_row_truncate")


# what HF generate would accept but this generator does not implement: refused rather than silently dropped
_NEUTRAL = {"top_p": 1.0, "length_penalty": 1.0, "min_new_tokens": 0, "no_repeat_ngram_size": 0,
            "early_stopping": False, "typical_p": 1.0, "num_beam_groups": 1, "diversity_penalty": 0.0}


def generate_items(chat: HipChat, items: Sequence, max_new_tokens: int = 20, num_beams: int = 1, do_sample: bool = False,
                   repetition_penalty: float = 1.0, temperature: float = 1.0, top_k: int = 50, seed: int = 0,
                   eos: int = EOS_ID, details: bool = False, prefill: str = "single", num_return_sequences: int = 1,
                   nucleus: Optional[NucleusSampling] = None, **kwargs) -> List:
    """Generate every PreparedItem independently, the items of a batch in lockstep (one decode step streams the weights once
    for all their rows).  Returns the output ids per item (HF's sequences without the empty prompt part), or with
    details=True the rule's result per item (tokens, score, per-step candidates; beam search: "hyps", the
    num_return_sequences best finished hypotheses as (score, tokens), best first).  num_return_sequences > 1 (beam search
    only, up to num_beams) without details returns per item the list of that many output id lists.

    prefill: "single" runs one prefill pass per item — an item's output is then a function of the item alone, bit for
    bit, whatever else is in flight.  "batched" packs the prompts of a chunk into as few passes as the encoder workspace
    (max_tokens, max_seqs) allows: the decoder's tile and split-K choices follow the packed token count, so an item's logits
    then agree with its lone run to bf16 accuracy only — for callers whose unit of work is the group (weighted selection).

    nucleus: a NucleusSampling sends every step's draw to HipChat.sample (top_p over any top_k; 0 = the whole vocabulary).  It
    needs do_sample=True, num_beams == 1 and the top_k argument left at its default (the nucleus carries its own).  Without
    it the HF-named options keep their refusals (top_p, top_k outside 1..64)."""
    if nucleus is not None:
        if not isinstance(nucleus, NucleusSampling):
            raise ValueError(f"nucleus={nucleus!r}: a NucleusSampling or None")
        if not do_sample or int(num_beams) != 1:
            raise ValueError("nucleus sampling needs do_sample=True and num_beams == 1")
        if top_k != 50:
            raise ValueError(f"top_k={top_k!r} next to nucleus=: the nucleus carries its own top_k")
    for k, v in kwargs.items():
        if k not in _NEUTRAL or v != _NEUTRAL[k]:
            raise NotImplementedError(f"generation option {k}={v!r} is not supported")
    nb = int(num_beams)
    if nb < 1:
        raise ValueError("num_beams must be positive")
    if do_sample and nb > 1:
        raise NotImplementedError("beam sampling (do_sample=True with num_beams > 1) is not supported")
    if do_sample and not (1 <= int(top_k) <= 64):
        raise NotImplementedError(f"top_k={top_k}: sampling supports a top-k filter of 1..64 candidates")
    if do_sample and not temperature > 0:
        raise ValueError("temperature must be positive when sampling")
    if nb > chat.max_rows:
        raise ValueError(f"num_beams={nb} exceeds the chat handle's max_rows={chat.max_rows}")
    if prefill not in ("single", "batched"):
        raise ValueError(f"prefill={prefill!r}: 'single' or 'batched'")
    nret = int(num_return_sequences)
    if nret < 1 or nret > (nb if nb > 1 and not do_sample else 1):
        raise ValueError(f"num_return_sequences={nret}: 1..num_beams for beam search, 1 for greedy search and sampling")
    if max_new_tokens > chat.max_new:
        raise ValueError(f"max_new_tokens={max_new_tokens} exceeds the chat handle's max_new={chat.max_new}")
    per = max(1, min(chat.max_rows // nb, chat.max_slots))
    out: List[List[int]] = []
    for lo in range(0, len(items), per):
        res = _generate_chunk(chat, items[lo:lo + per], max_new_tokens, nb, do_sample, repetition_penalty, temperature, top_k, seed, eos,
                              prefill, nucleus)
        for r in res:
            if "hyps" in r:
                r["hyps"] = r["hyps"][:nret]
        if details:
            out += res
        elif nret > 1:
            out += [[t for _, t in r["hyps"]] for r in res]
        else:
            out += [r["tokens"] for r in res]
    return out


def prefill_groups(lengths: Sequence[int], max_tokens: int, max_seqs: int) -> List[List[int]]:
    """Consecutive runs of the items that fit one packed pass each: at most max_tokens tokens and max_seqs items (an item
    longer than max_tokens stands alone and fails as it would on its own)."""
    groups, cur, tok = [], [], 0
    for i, n in enumerate(lengths):
        if cur and (tok + n > max_tokens or len(cur) >= max_seqs):
            groups.append(cur)
            cur, tok = [], 0
        cur.append(i)
        tok += n
    if cur:
        groups.append(cur)
    return groups


def _generate_chunk(chat, items, max_new, nb, do_sample, pen, temp, top_k, seed, eos, prefill="single", nucleus=None):
    """Every item's rule is a generator of select / advance requests; each round serves all pending requests of one kind in
    ONE device call (advances first: a select must see the appended token), so the items advance in lockstep.
    prefill="resident": item i's prompt (and whatever its row already appended) sits in slot i with its logits on row i * nb
    (ChatSession); nothing is prefilled."""
    rules, rows, reqs, results = [], [], [], [None] * len(items)
    if prefill == "batched":
        for g in prefill_groups([len(it.input_ids) for it in items], chat.enc.max_tokens, chat.enc.max_seqs):
            chat.prefill_batch(g, [i * nb for i in g], [items[i] for i in g])
    for i, it in enumerate(items):
        r = list(range(i * nb, (i + 1) * nb))
        if prefill == "single":
            chat.prefill(i, r[0], it)
        rule = greedy_rule(max_new, eos) if (do_sample or nb == 1) else beam_rule(nb, max_new, eos)
        rules.append(rule); rows.append(r); reqs.append(next(rule))
    mode = SAMPLE if do_sample else (BEAM if nb > 1 else GREEDY)
    step = 0
    while any(q is not None for q in reqs):
        live = [i for i, q in enumerate(reqs) if q is not None]
        kind = "advance" if any(reqs[i][0] == "advance" for i in live) else "select"
        sel = [i for i in live if reqs[i][0] == kind]
        answers = {}
        if kind == "select" and nucleus is not None:         # one draw per pending item (each holds one row), in one call
            sc, tk, _, _ = chat.sample([rows[i][0] for i in sel], repetition_penalty=pen, temperature=temp, top_k=nucleus.top_k,
                                       top_p=nucleus.top_p, seed=seed, step=step)
            step += 1
            for j, i in enumerate(sel):
                answers[i] = [(float(sc[j]), int(tk[j]), 0)] if tk[j] >= 0 else []
        elif kind == "select":
            k = reqs[sel[0]][3]
            groups = [rows[i][:reqs[i][1]] for i in sel]
            sc, tk, pa = chat.select(mode, groups, k, [s for i in sel for s in reqs[i][2]], repetition_penalty=pen,
                                     temperature=temp, top_k=top_k, seed=seed, step=step)
            step += 1
            for j, i in enumerate(sel):
                answers[i] = [(float(sc[j, q]), int(tk[j, q]), int(pa[j, q])) for q in range(k) if tk[j, q] >= 0]
        else:
            slots, srows, toks = [], [], []
            for i in sel:
                parents, tokens = reqs[i][1], reqs[i][2]
                src = [rows[i][p] for p in parents]
                dst = rows[i][:len(parents)]
                if src != dst:
                    chat.reorder(dst, src)
                slots += [i] * len(dst); srows += dst; toks += tokens
            chat.step(slots, srows, toks)
            answers = {i: None for i in sel}
        for i in sel:
            try:
                reqs[i] = rules[i].send(answers[i])
            except StopIteration as stop:
                results[i], reqs[i] = stop.value, None
    return results


# ------------------------------------------------------------------------------------------ scoring ---
def sequence_score(token_logprobs, tokens: Sequence[int], repetition_penalty: float = 1.0, length_penalty: float = 1.0,
                   return_sum: bool = False):
    """The beam's sequence score of a forced continuation from its per-token log-probs (pure numpy, fp64).  HF's order:
    log-softmax first, then the repetition penalty on the ids generated SO FAR — the log-prob of tokens[t] is multiplied by
    the penalty iff that id occurs in tokens[:t] (log-probs are <= 0: the `negative score * penalty` branch).  The sum is
    divided by len(tokens) ** length_penalty: the score `beam_rule` / `_Hyps.add` gives a hypothesis whose output ids, eos
    included, are `tokens`.  return_sum=True -> (score, penalised sum)."""
    lp = np.asarray(token_logprobs, dtype=np.float64).reshape(-1)
    toks = [int(t) for t in tokens]
    if len(toks) != lp.shape[0] or not toks:
        raise ValueError("sequence_score needs one log-prob per token and at least one token")
    if not repetition_penalty > 0:
        raise ValueError("repetition_penalty must be positive")
    seen, total = set(), 0.0
    for t, x in zip(toks, lp.tolist()):
        total += x * float(repetition_penalty) if t in seen else x
        seen.add(t)
    score = total / (len(toks) ** float(length_penalty))
    return (score, total) if return_sum else score


def score_items(chat, items: Sequence, continuations: Sequence[Sequence[int]], repetition_penalty: float = 1.0,
                length_penalty: float = 1.0) -> List[Dict]:
    """How likely is continuations[i] after the prompt items[i]?  Every (prompt + continuation) runs as one sequence of a
    packed causal pass (`chat.score`; as many passes as `prefill_groups` cuts the batch into), every continuation position
    through the fused head.  Per item {"token_logprobs": fp64 logit - lse per token (no penalty), "sum": their sum with the
    repetition penalty of `sequence_score`, "score": sum / len ** length_penalty, "greedy_match": per position whether the
    token is the row's argmax, "top_tokens": that argmax}.  Sampling warpers (temperature, top-k, top-p) have no part in it."""
    from dataclasses import replace
    items, conts = list(items), [[int(t) for t in c] for c in continuations]
    if len(items) != len(conts):
        raise ValueError(f"{len(items)} items but {len(conts)} continuations")
    for i, c in enumerate(conts):
        if not c:
            raise ValueError(f"continuation {i} is empty")
    full = [replace(it, input_ids=[int(t) for t in it.input_ids] + c) for it, c in zip(items, conts)]
    out: List[Dict] = []
    for g in prefill_groups([len(it.input_ids) for it in full], chat.enc.max_tokens, chat.enc.max_seqs):
        res = chat.score([full[i] for i in g], [len(conts[i]) for i in g])
        for i, r in zip(g, res):
            lp = np.asarray(r["logit"], dtype=np.float64) - np.asarray(r["lse"], dtype=np.float64)
            score, total = sequence_score(lp, conts[i], repetition_penalty, length_penalty, return_sum=True)
            top = np.asarray(r["top_token"], dtype=np.int64)
            out.append({"token_logprobs": lp, "sum": total, "score": score,
                        "greedy_match": top == np.asarray(conts[i], dtype=np.int64), "top_tokens": top})
    return out


def _score_on_slot(chat, slot: int, prow: int, conts: List[List[int]], repetition_penalty: float, length_penalty: float) -> List[Dict]:
    """The continuations of ONE resident prompt: token 0 of every continuation from the prompt's logits (one `row_score`
    call on the prompt's row, or — prow None: a generation has moved the row on — one `slot_score` call), tokens 1.. from
    `extend` on rows of that slot, at most max_rows of them per call."""
    if prow is None:
        first = chat.slot_score([slot] * len(conts), [c[0] for c in conts])
    else:
        first = chat.row_score([prow] * len(conts), [c[0] for c in conts])
    logit = [[float(first["logit"][a])] for a in range(len(conts))]
    lse = [[float(first["lse"][a])] for a in range(len(conts))]
    top = [[int(first["top_token"][a])] for a in range(len(conts))]
    # rows free for the tails: unbound ones and those of this slot (rows of other slots — other items of the pack, a generation
    # in progress — are left alone); the prompt's own row only when there is no other
    cands = [r for r in range(chat.max_rows) if r != prow and chat.row_state(r)[0] in (-1, slot)] or [prow]
    if cands == [None]:
        raise ValueError(f"no row is free for the continuations of slot {slot}")
    longer = [a for a, c in enumerate(conts) if len(c) > 1]
    per = max(1, min(len(cands), chat.enc.max_seqs))
    lo = 0
    while lo < len(longer):
        chunk, tok = [], 0
        while lo + len(chunk) < len(longer) and len(chunk) < per:
            n = len(conts[longer[lo + len(chunk)]]) - 1
            if chunk and tok + n > chat.enc.max_tokens:
                break
            chunk.append(longer[lo + len(chunk)])
            tok += n
        lo += len(chunk)
        rows = cands[:len(chunk)]
        for r in rows:                                   # a row that carried an earlier chunk starts over
            if chat.row_state(r) != (slot, 0) and chat.row_state(r)[0] == slot:
                chat.truncate(r, 0)
        res = chat.extend([slot] * len(chunk), rows, [conts[a][:-1] for a in chunk], targets=[conts[a][1:] for a in chunk])
        for a, r in zip(chunk, res):
            logit[a] += [float(x) for x in r["logit"]]
            lse[a] += [float(x) for x in r["lse"]]
            top[a] += [int(x) for x in r["top_token"]]
    out = []
    for a, c in enumerate(conts):
        lp = np.asarray(logit[a], dtype=np.float64) - np.asarray(lse[a], dtype=np.float64)
        score, total = sequence_score(lp, c, repetition_penalty, length_penalty, return_sum=True)
        t = np.asarray(top[a], dtype=np.int64)
        out.append({"token_logprobs": lp, "sum": total, "score": score, "greedy_match": t == np.asarray(c, dtype=np.int64),
                    "top_tokens": t})
    return out


def score_items_shared(chat, items: Sequence, continuations_of_item: Sequence[Sequence[Sequence[int]]],
                       repetition_penalty: float = 1.0, length_penalty: float = 1.0,
                       prefilled: Optional[Dict[int, Tuple[int, int]]] = None) -> List[List[Dict]]:
    """`score_items` for SEVERAL continuations per prompt over ONE prefill per prompt: item i is prefilled once
    (`prefill_batch`, the items in `prefill_groups` packs), the first token of each of its continuations is read off the
    prompt row's logits (`row_score`), the others come from `extend` with tokens c[0..n-2] and targets c[1..n-1] on rows of
    that slot, at most max_rows rows per call (a one-token continuation needs no extend).  -> per item, per continuation, the
    dict of `score_items`; the two routes agree to bf16 accuracy.

    prefilled: {item index: (slot, row)} for prompts already resident — `row` holds the prompt's logits and an empty tail on
    `slot`, or row is None: the slot's prompt logits are still readable (`slot_state`) although a generation has moved its
    rows on, which are then overwritten; those items are not prefilled again.  With a row the caller vouches that the slot
    holds THIS item's prompt (only the row's binding is checked); with None the handle checks it (`slot_holds`: the ids and
    slices it prefilled there, the slot not prefilled since) and anything else raises ValueError.  The other items use the slots and rows `prefilled` does not name; rows bound
    to a scored slot (other than the prompt's row) are overwritten.  A continuation longer than max_new raises ValueError."""
    items = list(items)
    conts = [[[int(t) for t in c] for c in cs] for cs in continuations_of_item]
    if len(items) != len(conts):
        raise ValueError(f"{len(items)} items but {len(conts)} continuation lists")
    for i, cs in enumerate(conts):
        if not cs:
            raise ValueError(f"item {i} has no continuation")
        for a, c in enumerate(cs):
            if not c:
                raise ValueError(f"continuation {a} of item {i} is empty")
            if len(c) > chat.max_new:
                raise ValueError(f"continuation {a} of item {i}: {len(c)} tokens exceed the chat handle's max_new={chat.max_new}")
    prefilled = {int(i): (int(s), None if r is None else int(r)) for i, (s, r) in (prefilled or {}).items()}
    for i, (s, r) in prefilled.items():
        if not 0 <= i < len(items):
            raise ValueError(f"prefilled names item {i} of {len(items)}")
        if r is None:
            if not chat.slot_holds(s, items[i]) or chat.slot_state(s) != (len(items[i].input_ids), True):
                raise ValueError(f"prefilled item {i}: slot {s} does not hold its prompt with readable logits")
        elif chat.row_state(r) != (s, 0):
            raise ValueError(f"prefilled item {i}: row {r} does not hold the prompt of slot {s} with an empty tail")
    out: List[Optional[List[Dict]]] = [None] * len(items)
    for i, (s, r) in prefilled.items():
        out[i] = _score_on_slot(chat, s, r, conts[i], repetition_penalty, length_penalty)
    todo = [i for i in range(len(items)) if i not in prefilled]
    if todo:
        free_slots = [s for s in range(chat.max_slots) if s not in {s_ for s_, _ in prefilled.values()}]
        free_rows = [r for r in range(chat.max_rows) if r not in {r_ for _, r_ in prefilled.values()} and
                     chat.row_state(r)[0] not in {s_ for s_, _ in prefilled.values()}]
        if not free_slots or not free_rows:
            raise ValueError("prefilled leaves no slot or row for the other items")
        # a pack keeps half its rows for the tails (one row per prompt, the rest for the continuations of the prompt at hand)
        per = max(1, min(len(free_slots), len(free_rows) // 2))
        for lo in range(0, len(todo), per):
            pack = todo[lo:lo + per]
            for g in prefill_groups([len(items[i].input_ids) for i in pack], chat.enc.max_tokens, chat.enc.max_seqs):
                chat.prefill_batch([free_slots[j] for j in g], [free_rows[j] for j in g], [items[pack[j]] for j in g])
            for j, i in enumerate(pack):
                out[i] = _score_on_slot(chat, free_slots[j], free_rows[j], conts[i], repetition_penalty, length_penalty)
    return out


def resident_after_generation(chat, items: Sequence, num_beams: int) -> Dict[int, Tuple[int, None]]:
    """Which items does `generate_items(chat, items, num_beams=...)` leave resident for `score_items_shared(prefilled=...)`?
    It cuts the items into chunks of max_rows // num_beams (at most max_slots) and puts item i of a chunk in slot i, so only
    a generation of ONE chunk leaves item i in slot i; of those, the slots that hold exactly the item's prompt (`slot_holds`:
    ids and slices, not prefilled since) with readable prompt logits.  -> {item index: (slot, None)}."""
    n = len(items)
    if n > max(1, min(chat.max_rows // max(1, int(num_beams)), chat.max_slots)):
        return {}
    return {i: (i, None) for i in range(n)
            if chat.slot_holds(i, items[i]) and chat.slot_state(i) == (len(items[i].input_ids), True)}


class ChatSession:
    """Several turns about one page over ONE cached prompt: slot 0 and rows [0, num_beams) of `chat`.  `make_item(msgs)`
    builds the PreparedItem of the whole history as chat(assistant_turn=True) does.  The session keeps the ids it has fed
    (prompt, then the row's tail).  `ask`: if the fed ids are a prefix of the new ids it appends the remainder (`extend`,
    seen="clear": HF penalises only ids generated in the current generate); if the two part inside the tail it truncates
    the tail to the common prefix and appends; if they part inside the prompt, the slices differ or the tail would not fit,
    it prefills afresh.  Then it decodes with the rules of `generate_items`.  The contract is on id lists — a turn equals a
    fresh prefill of the same ids to bf16 accuracy; whether a tokenizer splits concatenated text alike only decides which
    path is taken.  `counts` / `last_path` ("prefill", "extend", "truncate") say which.  Slot 0 and rows [0, num_beams) of
    the handle belong to the session: before it extends, it checks that row 0 still continues slot 0 with the tail it fed and
    that slot 0 has not been prefilled since its own prefill (`slot_generation`: the library counts the prefills of a slot,
    whoever called them); otherwise, or when the remainder exceeds the encoder's max_tokens, it prefills afresh."""

    def __init__(self, chat, make_item, eos: int = EOS_ID, max_new_tokens: int = 20, num_beams: int = 1, do_sample: bool = False,
                 repetition_penalty: float = 1.0, temperature: float = 1.0, top_k: int = 50, seed: int = 0,
                 nucleus: Optional[NucleusSampling] = None):
        nb = int(num_beams)
        if nb < 1 or nb > chat.max_rows:
            raise ValueError(f"num_beams={num_beams} outside 1..max_rows={chat.max_rows}")
        if do_sample and nb > 1:
            raise NotImplementedError("beam sampling (do_sample=True with num_beams > 1) is not supported")
        if max_new_tokens < 1 or max_new_tokens > chat.max_new:
            raise ValueError(f"max_new_tokens={max_new_tokens} outside 1..max_new={chat.max_new}")
        self.chat, self.make_item, self.eos = chat, make_item, int(eos)
        self.max_new_tokens, self.nb, self.do_sample = int(max_new_tokens), nb, bool(do_sample)
        self.pen, self.temp, self.top_k, self.seed, self.nucleus = repetition_penalty, temperature, top_k, seed, nucleus
        self.fed: List[int] = []          # ids the cache of row 0 holds: the prompt, then the tail
        self.plen = 0
        self.slices: List[np.ndarray] = []
        self.counts = {"prefill": 0, "extend": 0, "truncate": 0}
        self.last_path: Optional[str] = None
        self._stamp = None                # slot 0's generation after the session's own prefill

    def _intact(self) -> bool:
        """row 0 still continues slot 0 with the tail the session fed, and nobody has prefilled slot 0 since"""
        return self._stamp == self.chat.slot_generation(0) and self.chat.row_state(0) == (0, len(self.fed) - self.plen)

    def _same_slices(self, slices) -> bool:
        return len(slices) == len(self.slices) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(slices, self.slices))

    def feed(self, item) -> str:
        """Bring row 0 to `item.input_ids` with its logits current -> the path taken."""
        ids = [int(t) for t in item.input_ids]
        slices = [np.asarray(s) for s in item.slices]
        common = 0
        while common < min(len(ids), len(self.fed)) and ids[common] == self.fed[common]:
            common += 1
        common = min(common, len(ids) - 1)               # at least one token is appended: the logits are those after it
        fits = (len(ids) - self.plen + self.max_new_tokens <= self.chat.max_new and len(ids) + self.max_new_tokens <= self.chat.max_len and
                len(ids) - common <= self.chat.enc.max_tokens)
        if not self.fed or common < self.plen or not self._same_slices(slices) or not fits or not self._intact():
            self.chat.prefill(0, 0, item)
            self._stamp = self.chat.slot_generation(0)
            self.fed, self.plen, self.slices, path = ids, len(ids), slices, "prefill"
        else:
            path = "extend"
            if common < len(self.fed):
                self.chat.truncate(0, common - self.plen)
                path = "truncate"
            self.chat.extend([0], [0], [ids[common:]], seen="clear")
            self.fed = ids
        self.counts[path] += 1
        self.last_path = path
        return path

    def ask_ids(self, msgs) -> List[int]:
        """One turn -> the output ids (as generate_items returns them)."""
        self.feed(self.make_item(msgs))
        base = len(self.fed) - self.plen                 # the tail before this turn's generation
        res = _generate_chunk(self.chat, [None], self.max_new_tokens, self.nb, self.do_sample, self.pen, self.temp, self.top_k,
                              self.seed, self.eos, prefill="resident", nucleus=self.nucleus)[0]
        tokens = [int(t) for t in res["tokens"]]
        if self.nb == 1:                                 # row 0 holds the tokens it was stepped with: they count as fed
            kept = self.chat.row_state(0)[1] - base
            self.fed = self.fed + tokens[:kept]
        else:                                            # which beam ended on row 0 is the rule's business: keep the fed ids only
            self.chat.truncate(0, base)
        return tokens


def marginal_weights(S, doc_scores):
    """RAG-Sequence marginalisation over pages: S[a][i] = score of candidate answer a on page i, p = softmax(doc_scores) in
    fp64 (select_weighted's), weight[a] = sum_i p_i * exp(S[a][i]).  -> (index of the first largest weight, weights, p)."""
    S = np.asarray(S, dtype=np.float64)
    d = np.asarray(doc_scores, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] < 1 or S.shape[1] != d.shape[0] or d.shape[0] < 1:
        raise ValueError("marginal_weights needs S [answers][pages] and one doc score per page")
    e = np.exp(d - d.max())
    p = e / e.sum()
    weights = [float(np.sum(p * np.exp(S[a]))) for a in range(S.shape[0])]
    return weights.index(max(weights)), weights, p.tolist()
