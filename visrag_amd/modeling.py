"""Drop-in for the reference's retrieval-model wrapper on the encode path.

Mirrors src/openmatch/modeling/dense_retrieval_model.py:
  * `DROutput` (q_reps / p_reps)                                   :30-36
  * `DRModelForInference.build(model_args, ...)`                   :233-364, 387-391
  * `forward(query=..., passage=..., **kwargs)` / `encode_query` /
    `encode_passage`                                               :142-231, 393-408
where `query` / `passage` are the batch dicts of inference.py:85-101 (`id`, `text`, `image`
lists; extra keys are ignored) and kwargs carry `tokenizer` and `max_inp_length`.
Pooling `wmean` + `normalize=True` (the published VisRAG-Ret setting, eval.sh:62-63) are
fused into the device path; other poolings raise.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from .config import VisRAGRetConfig, full_config
from .engine import HipEncoder, overlapping_streams
from .preprocess import PreparedItem, prepare_batch


@dataclass
class DROutput:
    q_reps: Optional[torch.Tensor] = None
    p_reps: Optional[torch.Tensor] = None
    loss: Optional[torch.Tensor] = None
    scores: Optional[torch.Tensor] = None


class DRModelForInference:
    """HIP-backed equivalent of openmatch's DRModelForInference for VisRAG-Ret."""

    def __init__(self, cfg: VisRAGRetConfig, encoder: HipEncoder, pooling: str = "wmean",
                 normalize: bool = True, gpu_preprocess: bool = True):
        if pooling in ("drop_wmean", "drop_mean", "lasttoken_simcse"):
            # the reference applies dropout in TRAINING mode inside these even at inference (a fresh nn.Dropout1d(0.3),
            # dense_retrieval_model.py:187,196; F.dropout(training=True), :215): its own output is random
            raise ValueError(f"pooling {pooling!r} is stochastic in the reference (training-mode dropout); use "
                             "wmean / mean / lasttoken / cls")
        if pooling not in HipEncoder.POOLINGS:
            raise ValueError("Unknown pooling type: {}".format(pooling))      # dense_retrieval_model.py:220
        assert normalize == True, "Normalize must be true"   # dense_retrieval_model.py:222
        encoder.set_pooling(pooling)
        self.cfg, self.encoder = cfg, encoder
        self.pooling, self.normalize = pooling, normalize
        self.micro_batch = encoder.max_seqs
        # batches in flight: slot j = its own HipEncoder (clone: same weights, own workspace) + HIP stream.
        # Consecutive model(...) calls rotate over the slots, so batch i+1 (pre-processing included) runs
        # while batch i is still on the GPU; the caller's stream waits for each result, never the reverse.
        self._slots = [(encoder, None)]
        self._rr = 0
        self._uploaders = {}            # per slot: pinned staging + device buffer for a batch's page pixels
        # page resize + slicing on the GPU (bit-identical to PIL, gpu_resize.py) instead of on the host
        self.gpu_preprocess = gpu_preprocess

    # ---- construction -----------------------------------------------------------------------
    @classmethod
    def build(cls, model_args=None, cfg: Optional[VisRAGRetConfig] = None,
              state_dict: Optional[Iterable[Tuple[str, torch.Tensor]]] = None, device: Optional[int] = None,
              max_images: int = 32, max_tokens: int = 4096, max_seqs: int = 64, pipeline: int = 2, **_):
        """`model_args` needs `.model_name_or_path` (a HF checkpoint dir with *.safetensors /
        pytorch_model*.bin and config.json) unless `state_dict` is given; `.pooling` and
        `.normalize` are honoured like the reference (arguments.py).

        `device=None` (what the unchanged driver passes, driver/eval.py:124-127) resolves like the
        reference's `encoding_args.device`: this process's LOCAL_RANK under torchrun, else torch's
        current device — one process per GPU, never "all ranks on GPU 0"."""
        device = default_device() if device is None else _device_index(device)
        pooling = (getattr(model_args, "pooling", None) if model_args is not None else None) or \
                  (getattr(cfg, "pooling", None) if cfg is not None else None) or "wmean"
        normalize = getattr(model_args, "normalize", True) if model_args is not None else True
        path = getattr(model_args, "model_name_or_path", None) if model_args is not None else None
        if cfg is None:
            cfg = config_from_checkpoint(path) if path else full_config()
        enc = HipEncoder(cfg, device=device, max_images=max_images, max_tokens=max_tokens, max_seqs=max_seqs)
        if state_dict is None:
            if not path:
                raise ValueError("need model_args.model_name_or_path or state_dict")
            state_dict = iter_checkpoint(path)
        enc.load_state_dict(state_dict)
        model = cls(cfg, enc, pooling=pooling, normalize=normalize)
        model.set_pipeline(pipeline)
        return model

    def set_pipeline(self, depth: int) -> None:
        """depth >= 2: keep that many batches in flight (one workspace + stream each, weights shared)."""
        depth = max(1, int(depth))
        enc = self.encoder
        dev = torch.device(f"cuda:{enc.device}")
        # (streams that really overlap: two pool streams can share a hardware queue, engine.py::overlapping_streams)
        self._slots = [(enc, None)] if depth == 1 else \
            [(enc if j == 0 else enc.clone(), st) for j, st in enumerate(overlapping_streams(dev, depth))]
        self._rr = 0

    def eval(self):
        return self

    def to(self, device=None, *_a, **_k):
        """The reference driver calls `model.to(encoding_args.device)` after build()
        (driver/eval.py:128-129).  Weights already live on the build device: the same device is a
        no-op, a different one is refused (silently staying put would send every rank to one GPU)."""
        if device is None or isinstance(device, torch.dtype):
            return self
        want = _device_index(device)
        if want is not None and want != self.encoder.device:
            raise RuntimeError(f"model was built on cuda:{self.encoder.device}, to({device!r}) asks for cuda:{want}: "
                               "set LOCAL_RANK / torch.cuda.set_device() before build(), or pass build(device=...)")
        return self

    @property
    def device(self) -> torch.device:
        return torch.device(f"cuda:{self.encoder.device}")

    @property
    def lm_q(self) -> "VisRAGRet":
        """The underlying model with its HF-style forward (dense_retrieval_model.py:67-68: `lm_q` / `lm_p`, tied)."""
        return VisRAGRet(self)

    lm_p = lm_q

    # ---- reference API ----------------------------------------------------------------------
    def encode(self, items: Optional[Dict], is_query: bool = False, tokenizer=None,
               max_inp_length: int = 2048, **_):
        if items is None:
            return None, None
        if tokenizer is None:
            raise ValueError("tokenizer is required (model(passage=batch, tokenizer=tok, ...))")
        texts, images = list(items["text"]), list(items.get("image", [None] * len(items["text"])))
        enc, side = self._slots[self._rr % len(self._slots)]
        self._rr += 1

        def run():
            if self.gpu_preprocess and any(im is not None for im in images):
                from .gpu_resize import PageUploader, prepare_item_gpu
                up = self._uploaders.setdefault(id(enc), PageUploader(enc.device))
                dev_images = up.upload(images)             # the whole batch's pixels in one asynchronous copy
                prepared = [prepare_item_gpu(t, im, tokenizer, self.cfg, max_inp_length, enc.device)[0]
                            for t, im in zip(texts, dev_images)]
            else:
                prepared = prepare_batch(texts, images, tokenizer, self.cfg, max_inp_length)
            return self.encode_prepared(prepared, enc)

        if side is None:
            return None, run()
        cur = torch.cuda.current_stream(side.device)
        with torch.cuda.stream(side):          # resize kernels + encode of this batch: all on the slot's stream
            reps = run()
            done = side.record_event()
        cur.wait_event(done)                   # consumers on the caller's stream are ordered after the batch
        reps.record_stream(cur)
        return None, reps

    def encode_prepared(self, prepared: List[PreparedItem], enc: Optional[HipEncoder] = None) -> torch.Tensor:
        """Splits into micro-batches that fit the workspace (tokens / sequences).

        The precision route is chosen PER ITEM, not per batch: the library runs a micro-batch without image slices through the
        split-precision decoder pass (fp32-class; include/visrag_hip.h: text_split_precision) and one with slices through the
        bf16 pass, so token-only items are grouped into micro-batches of their own — a query's embedding no longer depends
        on whether a page happens to sit in the same call.  Item order of the result = item order of the call."""
        enc = enc or self.encoder
        text_only = [i for i, it in enumerate(prepared) if not it.slices]
        if 0 < len(text_only) < len(prepared) and getattr(self.cfg, "text_split_precision", 1):
            with_img = [i for i, it in enumerate(prepared) if it.slices]
            parts = [(text_only, self._encode_group([prepared[i] for i in text_only], enc)),
                     (with_img, self._encode_group([prepared[i] for i in with_img], enc))]
            out = torch.empty((len(prepared), parts[0][1].shape[1]), dtype=parts[0][1].dtype, device=parts[0][1].device)
            for idx, reps in parts:
                out[torch.as_tensor(idx, device=out.device)] = reps
            return out
        return self._encode_group(prepared, enc)

    def _encode_group(self, prepared: List[PreparedItem], enc: HipEncoder) -> torch.Tensor:
        outs, cur, tok = [], [], 0
        for it in prepared:
            n = len(it.input_ids)
            if n > enc.max_tokens:
                # (items are already truncated to max_inp_length like the reference's _convert_to_tensors,
                # modeling_minicpmv.py:179-180: this is the WORKSPACE being smaller than max_inp_length)
                raise ValueError(f"sequence of {n} tokens exceeds the encoder workspace (max_tokens={enc.max_tokens}): build "
                                 "with max_tokens >= max_inp_length")
            if cur and (tok + n > enc.max_tokens or len(cur) >= enc.max_seqs):
                outs.append(enc.encode_items(cur)); cur, tok = [], 0
            cur.append(it); tok += n
        if cur:
            outs.append(enc.encode_items(cur))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def encode_passage(self, psg, **kwargs):
        return self.encode(psg, is_query=False, **kwargs)

    def encode_query(self, qry, **kwargs):
        return self.encode(qry, is_query=True, **kwargs)

    def forward(self, query: Optional[Dict] = None, passage: Optional[Dict] = None, **kwargs) -> DROutput:
        _, q_reps = self.encode_query(query, **kwargs)
        _, p_reps = self.encode_passage(passage, **kwargs)
        return DROutput(q_reps=q_reps, p_reps=p_reps)

    __call__ = forward


@dataclass
class BaseModelOutputWithAttentionMask:
    """modeling_visrag_ret.py:24-27"""
    last_hidden_state: Optional[torch.Tensor] = None
    attention_mask: Optional[torch.Tensor] = None


class VisRAGRet:
    """The HF-style forward of the reference's SECOND caller: the demo scripts hold the bare
    `VisRAG_Ret` model and pool its output themselves,

        outputs = model(text=[...], image=[PIL | None, ...], tokenizer=tokenizer)      # demo/visrag_pipeline/utils.py:12-32
        reps = weighted_mean_pooling(outputs.last_hidden_state, outputs.attention_mask)

    (modeling_visrag_ret.py:86-126).  Same call here: `last_hidden_state` [B, L, hidden] float32 on the device, right-padded
    with zeros, `attention_mask` [B, L] int8 (modeling_minicpmv.py:464), both from ONE pass of the library
    (vr_encode_hidden).  `DRModelForInference.lm_q` / `.lm_p` are this object, like the reference's attributes."""

    def __init__(self, owner: "DRModelForInference"):
        self._owner = owner
        self.config = owner.cfg

    @classmethod
    def from_pretrained(cls, path: str, **kw) -> "VisRAGRet":
        return DRModelForInference.build(types_namespace(model_name_or_path=path), **kw).lm_q

    def eval(self):
        return self

    def to(self, *a, **k):
        self._owner.to(*a, **k)
        return self

    @property
    def device(self) -> torch.device:
        return self._owner.device

    def forward(self, text: List[str], image: List, tokenizer, max_inp_length: int = 2048, **_) -> BaseModelOutputWithAttentionMask:
        if len(text) != len(image):
            raise ValueError("text and image lists must have the same length")
        own = self._owner
        enc = own.encoder
        prepared = prepare_batch(list(text), list(image), tokenizer, own.cfg, max_inp_length)
        L = max(len(it.input_ids) for it in prepared)
        dev = torch.device(f"cuda:{enc.device}")
        hidden = torch.empty((len(prepared), L, own.cfg.hidden_size), dtype=torch.float32, device=dev)
        mask = torch.zeros((len(prepared), L), dtype=torch.int8)
        for i, it in enumerate(prepared):
            mask[i, :len(it.input_ids)] = 1
        # one library call per precision route and workspace-sized micro-batch, each writing its rows of `hidden`
        text_only = [i for i, it in enumerate(prepared) if not it.slices]
        with_img = [i for i, it in enumerate(prepared) if it.slices]
        split = bool(text_only) and bool(with_img) and bool(getattr(own.cfg, "text_split_precision", 1))
        for group in ([text_only, with_img] if split else [list(range(len(prepared)))]):
            cur, tok = [], 0
            for i in group + [None]:
                n = 0 if i is None else len(prepared[i].input_ids)
                if cur and (i is None or tok + n > enc.max_tokens or len(cur) >= enc.max_seqs):
                    contiguous = cur == list(range(cur[0], cur[0] + len(cur)))
                    part = hidden[cur[0]:cur[0] + len(cur)] if contiguous else torch.empty((len(cur), L, hidden.shape[2]), dtype=torch.float32, device=dev)
                    enc.encode_items([prepared[j] for j in cur], hidden_out=part)
                    if not contiguous:
                        hidden[torch.as_tensor(cur, device=dev)] = part
                    cur, tok = [], 0
                if i is not None:
                    if n > enc.max_tokens:
                        raise ValueError(f"sequence of {n} tokens exceeds the encoder workspace (max_tokens={enc.max_tokens})")
                    cur.append(i); tok += n
        return BaseModelOutputWithAttentionMask(last_hidden_state=hidden, attention_mask=mask.to(dev))

    __call__ = forward

    # ---- MiniCPM-V 2.0 answer generation (the reference's MiniCPMV.generate / chat, modeling_minicpmv.py:276-400) ----------
    def attach_generator(self, lm_head: torch.Tensor, gen_cfg=None, max_inp_length: int = 2048, max_new_tokens: int = 1024,
                         num_beams: int = 3, batch: int = 1) -> "VisRAGRet":
        """Give the model its LM head (`llm.lm_head.weight`; with tied embeddings the embedding matrix): the retrieval path
        drops it at load.  The cache holds `batch` prompts of up to max_inp_length tokens, each with num_beams rows of up to
        max_new_tokens generated tokens (chat()'s defaults: 2048, 1024, 3 beams; 2.3 GB at full dims for one prompt)."""
        from .generation import GenerationConfig, HipChat
        gen_cfg = gen_cfg or GenerationConfig()
        self._gen_cfg = gen_cfg
        self._chat = HipChat(self._owner.encoder, max_inp_length + max_new_tokens, num_beams * batch, gen_cfg.dim_model_base,
                             max_slots=batch, max_new=max_new_tokens)
        self._chat.load_head(lm_head)
        return self

    def generate(self, data_list=None, img_list=None, tokenizer=None, max_inp_length: Optional[int] = None,
                 vision_hidden_states=None, return_vision_hidden_states=False, **kwargs):
        """data_list: prompts that already hold their image placeholders; img_list: per prompt the PIL slices in placeholder
        order.  kwargs: max_new_tokens, num_beams, do_sample, temperature, repetition_penalty, top_k, seed, nucleus."""
        from .generation import decode_text, generate_items
        if data_list is None:
            raise ValueError("data_list is required")
        if vision_hidden_states is not None or return_vision_hidden_states:
            raise NotImplementedError("vision_hidden_states are not supported")
        if getattr(self, "_chat", None) is None:
            raise RuntimeError("generate() needs an LM head: call attach_generator() first (or load_generator())")
        if img_list is None:
            img_list = [[] for _ in data_list]
        if len(img_list) != len(data_list):
            raise ValueError("data_list and img_list must have the same length")
        items = [_prompt_item(t, imgs, tokenizer, max_inp_length) for t, imgs in zip(data_list, img_list)]
        kwargs.setdefault("max_new_tokens", 20)
        ids = generate_items(self._chat, items, eos=tokenizer.eos_id, **kwargs)
        return decode_text(ids, tokenizer)

    def chat(self, image_list, msgs_list, tokenizer, vision_hidden_states=None, max_new_tokens: int = 1024, sampling: bool = True,
             max_inp_length: int = 2048, seed: int = 0, assistant_turn: bool = False, return_scores: bool = False,
             answer_defaults: bool = False, **kwargs):
        """The reference's chat (modeling_minicpmv.py:321-398).  `seed` (not in the reference, whose draws come from torch's
        global generator) selects the sampling noise: chat(sampling=True) with one seed returns the same answer each call.
        assistant_turn=True ends the prompt with "<AI>", as the chat of the reference's answer-generation package does;
        return_scores=True (beam search only) returns (answers, scores): per item the sequence scores of its finished
        hypotheses, best first — that package's `sequences_scores` (it asks for num_return_sequences=2).
        answer_defaults=True takes the generation defaults of that package's chat (answer_chat_generation_config): its
        sampled answer is a nucleus, top_p 0.8 over top_k 100 at temperature 0.7, repetition_penalty 1.05."""
        from .generation import (NucleusSampling, answer_chat_generation_config, chat_generation_config, decode_text,
                                 generate_items)
        if return_scores and sampling:
            raise NotImplementedError("return_scores needs beam search (sampling=False): sampling yields no sequence scores")
        prompts, images = [], []
        for msgs, image in zip(msgs_list, image_list):
            p, imgs = chat_prompt(msgs, image, tokenizer, self.config)
            prompts.append(p + ("<AI>" if assistant_turn else ""))
            images.append(imgs)
        if answer_defaults:
            gen = answer_chat_generation_config(sampling, kwargs)
            if sampling:
                gen["nucleus"] = NucleusSampling(gen.pop("top_p"), gen.pop("top_k"))
        else:
            gen = chat_generation_config(sampling, kwargs)
        if not return_scores:
            return self.generate(data_list=prompts, img_list=images, tokenizer=tokenizer, max_inp_length=max_inp_length,
                                 vision_hidden_states=vision_hidden_states, max_new_tokens=max_new_tokens, seed=seed, **gen)
        if vision_hidden_states is not None:
            raise NotImplementedError("vision_hidden_states are not supported")
        if getattr(self, "_chat", None) is None:
            raise RuntimeError("chat() needs an LM head: call attach_generator() first (or load_generator())")
        items = [_prompt_item(t, imgs, tokenizer, max_inp_length) for t, imgs in zip(prompts, images)]
        res = generate_items(self._chat, items, eos=tokenizer.eos_id, max_new_tokens=max_new_tokens, details=True,
                             num_return_sequences=min(2, gen["num_beams"]), **gen)
        return decode_text([r["tokens"] for r in res], tokenizer), [[sc for sc, _ in r["hyps"]] for r in res]

    def weighted_selection(self, image_list, msgs, doc_scores, tokenizer, max_new_tokens: int = 1024, sampling: bool = False,
                           max_inp_length: int = 2048, details: bool = False, prefill: str = "single", **kwargs):
        """The reference's weighted selection (weighted_selection/MiniCPMV20/modeling_minicpmv.py:394-425): one beam-search
        answer per retrieved page, the answer of the page with the largest softmax(doc_scores)_i * exp(sequence score_i)
        wins (the first page among equals).  The pages of a request are decoded in lockstep; prefill="batched" also
        prefills them in one packed pass (vr_chat_prefill_batch; the default stays "single" until the batched pass has been
        timed on an MI355X: DESIGN.md ledger 70).  Either way the request is the unit: its result depends on (question,
        pages, scores) and on nothing else in flight.
        details=True -> (answer, {"answers": per page, "scores": per page its sequence scores best first, "weights",
        "doc_probs", "index": the chosen page, "tokens": per page, "results": generate_items' details per page})."""
        from .generation import chat_generation_config, decode_text, generate_items
        if sampling:
            raise NotImplementedError("weighted selection needs sequence scores: beam search only (sampling=False)")
        image_list, doc_scores = list(image_list), [float(x) for x in doc_scores]
        if not image_list:
            raise ValueError("weighted_selection needs at least one page")
        if len(image_list) != len(doc_scores):
            raise ValueError(f"{len(image_list)} pages but {len(doc_scores)} doc_scores")
        if getattr(self, "_chat", None) is None:
            raise RuntimeError("weighted_selection() needs an LM head: call attach_generator() first (or load_generator())")
        items = []
        for image in image_list:
            p, imgs = chat_prompt(msgs, image, tokenizer, self.config)
            items.append(_prompt_item(p + "<AI>", imgs, tokenizer, max_inp_length))
        gen = chat_generation_config(False, kwargs)
        # generate_items cuts the pages into chunks of max_rows // num_beams
        res = generate_items(self._chat, items, eos=tokenizer.eos_id, max_new_tokens=max_new_tokens, details=True, prefill=prefill,
                             num_return_sequences=min(2, gen["num_beams"]), **gen)
        answers = decode_text([r["tokens"] for r in res], tokenizer)
        index, weights, p = select_weighted([r["score"] for r in res], doc_scores)
        if not details:
            return answers[index]
        return answers[index], {"answers": answers, "scores": [[sc for sc, _ in r["hyps"]] for r in res], "weights": weights,
                                "doc_probs": p, "index": index, "tokens": [r["tokens"] for r in res], "results": res}

    # ---- answer scoring: teacher-forced log-probs of GIVEN answers (vr_chat_score, the fused head of csrc/head_score.hip) ---
    def _scoring_chat(self, what: str):
        if getattr(self, "_chat", None) is None:
            raise RuntimeError(f"{what}() needs an LM head: call attach_generator() first (or load_generator())")
        return self._chat

    def score_answers(self, image_list, msgs_list, answers_list, tokenizer, max_inp_length: int = 2048, append_eos: bool = True,
                      repetition_penalty: float = 1.0, length_penalty: float = 1.0, shared_prefill: bool = False):
        """How likely is each given answer after (page, question)?  Prompts are built as chat(assistant_turn=True) builds
        them; every answer of answers_list[i] is tokenised without BOS (append_eos: followed by the eos the generator would
        close it with) and scored on item i in a packed teacher-forced pass.  Returns per item the list of
        `generation.score_items` dicts of its answers (token_logprobs, sum, score, greedy_match, top_tokens).  The
        penalties are those of `generation.sequence_score`; sampling warpers have no part in it.
        shared_prefill=True prefills every item ONCE and appends its answers to that cached prompt
        (`generation.score_items_shared`: the tower and the prompt's decoder rows run once per item instead of once per
        answer); the result agrees with the default route to bf16 accuracy.  It uses the chat handle's slots and rows: a
        generation in progress on the same handle does not survive it."""
        from .generation import score_items, score_items_shared
        chat = self._scoring_chat("score_answers")
        image_list, msgs_list, answers_list = list(image_list), list(msgs_list), [list(a) for a in answers_list]
        if not (len(image_list) == len(msgs_list) == len(answers_list)):
            raise ValueError(f"{len(image_list)} images, {len(msgs_list)} message lists and {len(answers_list)} answer lists")
        if shared_prefill:
            uniq, cont_lists, owner = [], [], []
            for i, (msgs, image, answers) in enumerate(zip(msgs_list, image_list, answers_list)):
                if not answers:
                    continue
                p, imgs = chat_prompt(msgs, image, tokenizer, self.config)
                uniq.append(_prompt_item(p + "<AI>", imgs, tokenizer, max_inp_length))
                cont_lists.append([answer_ids(a, tokenizer, append_eos) for a in answers]); owner.append(i)
            out = [[] for _ in answers_list]
            if uniq:
                for i, rs in zip(owner, score_items_shared(chat, uniq, cont_lists, repetition_penalty, length_penalty)):
                    out[i] = rs
            return out
        items, conts, owner = [], [], []
        for i, (msgs, image, answers) in enumerate(zip(msgs_list, image_list, answers_list)):
            p, imgs = chat_prompt(msgs, image, tokenizer, self.config)
            item = _prompt_item(p + "<AI>", imgs, tokenizer, max_inp_length)
            for a in answers:
                items.append(item); conts.append(answer_ids(a, tokenizer, append_eos)); owner.append(i)
        out = [[] for _ in answers_list]
        if items:
            for i, r in zip(owner, score_items(chat, items, conts, repetition_penalty, length_penalty)):
                out[i].append(r)
        return out

    def choose(self, image, msgs, options, tokenizer, normalise: bool = True, **kwargs):
        """Multiple choice: score every option as an answer to (image, msgs) and take the best -> (index, scores).  The
        argmax is over `score` (the length-normalised sum) when normalise is true, over `sum` otherwise; the first option wins
        among equals.  kwargs: score_answers' (max_inp_length, append_eos, repetition_penalty, length_penalty,
        shared_prefill)."""
        options = list(options)
        if not options:
            raise ValueError("choose needs at least one option")
        scores = self.score_answers([image], [msgs], [options], tokenizer, **kwargs)[0]
        keys = [float(s["score" if normalise else "sum"]) for s in scores]
        return keys.index(max(keys)), scores

    def marginal_selection(self, image_list, msgs, doc_scores, tokenizer, normalise: bool = True, details: bool = False,
                           shared_prefill: bool = False, **kwargs):
        """Weighted selection in its RAG-Sequence form: weighted_selection's generation as it is, then every candidate answer
        (the distinct output id lists of the pages' best hypotheses, in first-seen order) is scored on EVERY page —
        S[a][i] = score_items of candidate a on page i under the beam's repetition_penalty (`score` when normalise is true,
        `sum` otherwise) — and weight[a] = sum_i softmax(doc_scores)_i * exp(S[a][i]) in fp64.  The answer is the first
        largest weight: two pages that agree reinforce each other where weighted selection lets them compete.
        details=True -> (answer, {"S", "weights", "candidates", "index", "doc_probs", "answers": per candidate,
        "weighted_selection": (answer, details) of the plain selection}).  kwargs: weighted_selection's.
        shared_prefill=True scores the candidates on the cached prompts (`generation.score_items_shared`): the slots the
        generation left behind are REUSED when they still hold the pages' prompts with readable prompt logits (all pages fit
        one chunk of the generator's cache: no prefill at all), and are prefilled once per page otherwise."""
        from .generation import (chat_generation_config, decode_text, marginal_weights, resident_after_generation, score_items,
                                 score_items_shared)
        chat = self._scoring_chat("marginal_selection")
        image_list = list(image_list)
        ws_answer, ws = self.weighted_selection(image_list, msgs, doc_scores, tokenizer, details=True, **kwargs)
        candidates = []
        for toks in ws["tokens"]:
            if list(toks) not in candidates:
                candidates.append(list(toks))
        items = []
        for image in image_list:
            p, imgs = chat_prompt(msgs, image, tokenizer, self.config)
            items.append(_prompt_item(p + "<AI>", imgs, tokenizer, kwargs.get("max_inp_length", 2048)))
        pen = chat_generation_config(False, kwargs)["repetition_penalty"]
        n = len(items)
        key = "score" if normalise else "sum"
        if shared_prefill:
            # the pages the generation (one chunk, with the num_beams it actually ran) left in their slots, checked by content
            resident = resident_after_generation(chat, items, chat_generation_config(False, kwargs)["num_beams"])
            per_page = score_items_shared(chat, items, [candidates] * n, pen, 1.0, prefilled=resident)
            S = [[float(per_page[i][a][key]) for i in range(n)] for a in range(len(candidates))]
        else:
            res = score_items(chat, [it for _ in candidates for it in items], [c for c in candidates for _ in items], pen, 1.0)
            S = [[float(res[a * n + i][key]) for i in range(n)] for a in range(len(candidates))]
        index, weights, p = marginal_weights(S, [float(x) for x in doc_scores])
        answers = decode_text(candidates, tokenizer)
        if not details:
            return answers[index]
        return answers[index], {"S": S, "weights": weights, "candidates": candidates, "index": index, "doc_probs": p,
                                "answers": answers, "weighted_selection": (ws_answer, ws)}

    def chat_session(self, image, tokenizer, **kwargs) -> "PageChatSession":
        """Several questions about ONE page over one cached prompt (generation.ChatSession on slot 0, rows [0, num_beams) of
        the generator's cache): session.ask(msgs) answers the whole ChatML history `msgs` as chat(assistant_turn=True)
        would, feeding only the ids the cache does not hold yet.  kwargs: chat()'s (max_new_tokens, sampling,
        max_inp_length, seed, answer_defaults and the generation options of the mode); max_new_tokens defaults to chat()'s
        1024 or the generator's max_new, whichever is smaller.  Slot 0 and rows [0, num_beams) of the generator's cache
        belong to the session; another call that prefills the generator in between is noticed and costs the session a fresh
        prefill, never a wrong answer."""
        return _chat_session(self, image, tokenizer, **kwargs)


class PageChatSession:
    """VisRAGRet.chat_session's handle: `ask(msgs)` -> the answer to the whole ChatML history `msgs` about the session's
    page; `session` is the generation.ChatSession underneath (counts, last_path, fed).  ask(msgs, image=other) moves the
    session to another page: its slices differ, so the prompt is prefilled afresh."""

    def __init__(self, session, tokenizer, page):
        self.session, self.tokenizer, self._page = session, tokenizer, page

    def ask(self, msgs, image=None) -> str:
        from .generation import decode_text
        if image is not None:
            self._page["image"] = image
        return decode_text([self.session.ask_ids(msgs)], self.tokenizer)[0]


def _chat_session(model: "VisRAGRet", image, tokenizer, max_new_tokens: Optional[int] = None, sampling: bool = True,
                  max_inp_length: int = 2048, seed: int = 0, answer_defaults: bool = False, **kwargs) -> PageChatSession:
    from .generation import ChatSession, NucleusSampling, answer_chat_generation_config, chat_generation_config
    if getattr(model, "_chat", None) is None:
        raise RuntimeError("chat_session() needs an LM head: call attach_generator() first (or load_generator())")
    if max_new_tokens is None:            # chat()'s 1024, or what the attached generator's rows hold
        max_new_tokens = min(1024, model._chat.max_new)
    if answer_defaults:
        gen = answer_chat_generation_config(sampling, kwargs)
        if sampling:
            gen["nucleus"] = NucleusSampling(gen.pop("top_p"), gen.pop("top_k"))
    else:
        gen = chat_generation_config(sampling, kwargs)

    page = {"image": image}

    def make_item(msgs):
        p, imgs = chat_prompt(msgs, page["image"], tokenizer, model.config)
        return _prompt_item(p + "<AI>", imgs, tokenizer, max_inp_length)

    return PageChatSession(ChatSession(model._chat, make_item, eos=tokenizer.eos_id, max_new_tokens=max_new_tokens, seed=seed, **gen),
                           tokenizer, page)


def select_weighted(seq_scores, doc_scores):
    """-> (index, weights, p): p = softmax(doc_scores) in fp64, weights[i] = p[i] * exp(seq_scores[i]), index = the first
    largest weight (`list.index(max(..))` of the reference)."""
    d = np.asarray(doc_scores, dtype=np.float64)
    e = np.exp(d - d.max())
    p = (e / e.sum()).tolist()
    weights = [pi * float(np.exp(np.float64(s))) for pi, s in zip(p, seq_scores)]
    return weights.index(max(weights)), weights, p


def chat_prompt(msgs, image, tokenizer, cfg):
    """modeling_minicpmv.py:335-367: ChatML messages + one image -> (prompt, image slices)."""
    from .preprocess import get_grid_placeholder, image_placeholder, slice_image
    if not isinstance(msgs, list):
        raise NotImplementedError(f"chatml format expected, expect outmost type to be list but got {type(msgs)}")
    prompt, images = "", []
    for i, msg in enumerate(msgs):
        role, content = msg["role"], msg["content"]
        assert role in ["user", "assistant"]
        if i == 0:
            assert role == "user", "The role of first msg should be user"
            if cfg.slice_mode:
                src, patches, grid = slice_image(image, cfg.max_slice_nums, cfg.scale_resolution, cfg.patch_size)
                images = [src] + [p for row in patches for p in row]
                ph = image_placeholder(tokenizer, cfg.query_num)
                if patches:
                    ph += get_grid_placeholder(tokenizer, grid, cfg.query_num)
            else:
                images = [image]
                ph = image_placeholder(tokenizer, cfg.query_num)
            content = ph + "\n" + content
        prompt += "<用户>" if role == "user" else "<AI>"
        prompt += content
    return prompt, images


def _prompt_item(text, images, tokenizer, max_inp_length):
    """MiniCPMV._convert_to_tensors (modeling_minicpmv.py:173-200) for a prompt that already holds its placeholders."""
    ids = list(tokenizer.encode(text))
    if not getattr(tokenizer, "add_bos_token", True):
        ids = [tokenizer.bos_id] + ids
    if max_inp_length is not None:
        ids = ids[:max_inp_length]
    arr = np.asarray(ids, dtype=np.int64)
    starts = np.nonzero(arr == tokenizer.im_start_id)[0] + 1
    ends = np.nonzero(arr == tokenizer.im_end_id)[0]
    if len(starts) != len(ends):
        raise ValueError("unbalanced <image> / </image> markers after truncation; raise max_inp_length")
    bound = [(int(s), int(e)) for s, e in zip(starts, ends)]
    slices = [np.asarray(im if im.mode == "RGB" else im.convert("RGB"), dtype=np.uint8) for im in images]
    return PreparedItem(input_ids=ids, image_bound=bound, slices=slices)


def answer_ids(text: str, tokenizer, append_eos: bool = True) -> List[int]:
    """An answer's token ids as the generator would emit them: no BOS (the tokenizer's own leading bos is dropped, none is
    added), no eos of the tokenizer's (add_eos_token), then one eos when append_eos.  An answer without a token: ValueError."""
    ids = [int(t) for t in tokenizer.encode(text)]
    if getattr(tokenizer, "add_bos_token", True) and ids and ids[0] == tokenizer.bos_id:
        ids = ids[1:]
    if getattr(tokenizer, "add_eos_token", False) and ids and ids[-1] == tokenizer.eos_id:
        ids = ids[:-1]
    if not ids:
        raise ValueError(f"answer {text!r} holds no token")
    return ids + [int(tokenizer.eos_id)] if append_eos else ids


def load_generator(path: str, device=None, **cache) -> "VisRAGRet":
    """A MiniCPM-V 2.0 checkpoint directory -> VisRAGRet with generate / chat (config.json: dim_model_base,
    tie_word_embeddings; the head is llm.lm_head.weight, or the embedding matrix when tied).  `cache`: attach_generator's
    sizes."""
    from .generation import generation_config_from_checkpoint
    gcfg = generation_config_from_checkpoint(path)
    model = VisRAGRet.from_pretrained(path) if device is None else VisRAGRet.from_pretrained(path, device=device)
    want = "llm.model.embed_tokens.weight" if gcfg.tie_word_embeddings else "llm.lm_head.weight"
    return model.attach_generator(checkpoint_tensor(path, want), gcfg, **cache)


def checkpoint_tensor(path: str, key: str) -> torch.Tensor:
    """One tensor of a checkpoint directory: read from the safetensors shard that holds it (only that tensor is
    materialised); .bin shards are loaded one at a time until the key turns up."""
    files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
    if files:
        from safetensors import safe_open
        for fn in files:
            with safe_open(os.path.join(path, fn), framework="pt", device="cpu") as f:
                if key in f.keys():
                    return f.get_tensor(key)
    else:
        for fn in sorted(f for f in os.listdir(path) if f.startswith("pytorch_model") and f.endswith(".bin")):
            sd = torch.load(os.path.join(path, fn), map_location="cpu", weights_only=True)
            if key in sd:
                return sd[key]
    raise KeyError(f"{key} not found under {path}")


def types_namespace(**kw):
    import types
    return types.SimpleNamespace(**kw)


def default_device() -> int:
    """cuda index of this process: LOCAL_RANK (torchrun / torch.distributed.run) if set, else
    torch's current device."""
    lr = os.environ.get("LOCAL_RANK")
    if lr is not None and lr.strip() != "":
        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
        return int(lr) % n if n else int(lr)
    return int(torch.cuda.current_device()) if torch.cuda.is_available() else 0


def _device_index(device) -> Optional[int]:
    """int | 'cuda' | 'cuda:3' | torch.device -> cuda index ('cuda' = this process's default); None for
    anything that is not a cuda device spec (e.g. a dtype passed to .to())."""
    if isinstance(device, bool):
        return None
    if isinstance(device, int):
        return device
    if isinstance(device, str):
        try:
            device = torch.device(device)
        except (RuntimeError, ValueError):
            return None
    if isinstance(device, torch.device):
        if device.type != "cuda":
            raise RuntimeError(f"visrag_amd runs on HIP devices only (got {device}); there is no CPU fallback")
        return default_device() if device.index is None else int(device.index)
    return None


@torch.no_grad()
def encode(model: DRModelForInference, tokenizer, text_or_image_list) -> np.ndarray:
    """Demo helper with the signature of visrag_scripts/demo/visrag_pipeline/utils.py:12-32."""
    if isinstance(text_or_image_list[0], str):
        batch = {"text": list(text_or_image_list), "image": [None] * len(text_or_image_list)}
        out = model(query=batch, tokenizer=tokenizer).q_reps
    else:
        batch = {"text": [""] * len(text_or_image_list), "image": list(text_or_image_list)}
        out = model(passage=batch, tokenizer=tokenizer).p_reps
    return out.detach().cpu().numpy()


# ------------------------------------------------------------------ checkpoint plumbing ----
def config_from_checkpoint(path: str) -> VisRAGRetConfig:
    """config.json of a MiniCPM-V-2.0 / VisRAG-Ret checkpoint -> VisRAGRetConfig
    (dense_retrieval_model.py:248-269 dispatches on the same file)."""
    with open(os.path.join(path, "config.json")) as f:
        j = json.load(f)
    c = full_config()
    c.hidden_size = j.get("hidden_size", c.hidden_size)
    c.num_layers = j.get("num_hidden_layers", c.num_layers)
    c.num_heads = j.get("num_attention_heads", c.num_heads)
    c.intermediate_size = j.get("intermediate_size", c.intermediate_size)
    c.vocab_size = j.get("vocab_size", c.vocab_size)
    c.rms_norm_eps = j.get("rms_norm_eps", c.rms_norm_eps)
    c.rope_theta = j.get("rope_theta", c.rope_theta)
    c.scale_emb = j.get("scale_emb", c.scale_emb)
    c.scale_depth = j.get("scale_depth", c.scale_depth)
    c.query_num = j.get("query_num", c.query_num)
    c.patch_size = j.get("patch_size", c.patch_size)
    c.max_slice_nums = j.get("max_slice_nums", c.max_slice_nums)
    c.scale_resolution = j.get("scale_resolution", c.scale_resolution)
    c.slice_mode = j.get("slice_mode", c.slice_mode)
    return c


def iter_checkpoint(path: str):
    """Yield (key, tensor) from *.safetensors (preferred) or pytorch_model*.bin shards."""
    files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
    if files:
        from safetensors import safe_open
        for fn in files:
            with safe_open(os.path.join(path, fn), framework="pt", device="cpu") as f:
                for k in f.keys():
                    yield k, f.get_tensor(k)
        return
    files = sorted(f for f in os.listdir(path) if f.startswith("pytorch_model") and f.endswith(".bin"))
    if not files:
        raise FileNotFoundError(f"no *.safetensors / pytorch_model*.bin under {path}")
    for fn in files:
        sd = torch.load(os.path.join(path, fn), map_location="cpu", weights_only=True)
        for k, v in sd.items():
            yield k, v
