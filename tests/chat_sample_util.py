"""Helpers of tests/test_gpu_chat_sample.py: vr_op_chat_sample on torch containers, and the tiny chat model of
tests/golden/chat_tiny.npz loaded as tests/test_gpu_chat.py loads it."""
import ctypes as C
import os

import numpy as np
import torch

from tests import chat_ref
from tests.gpu_util import P
from visrag_amd import _lib

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
QUESTIONS = ["What animal is in the picture?", "Describe the image.", "What is the capital of France?"]


def op_chat_sample_raw(device, logits_ptr, ld, V, seen_ptr, words, n, penalty, temperature, top_k, top_p, seed, step, outs):
    """the bare entry: pointers as given, outs = (scores f32, tokens, kept, cut i32 numpy or None) -> status"""
    f = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None  # noqa: E731
    return _lib.load().vr_op_chat_sample(device, logits_ptr, ld, V, seen_ptr, words, n, float(penalty), float(temperature), int(top_k),
                                         float(top_p), C.c_uint64(int(seed) & (2 ** 64 - 1)), int(step), f(outs[0], C.c_float),
                                         f(outs[1], C.c_int32), f(outs[2], C.c_int32), f(outs[3], C.c_int32), None)


def op_chat_sample(logits, seen, V, penalty=1.0, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0):
    """logits fp32 [n][ld], seen int32 words [n][words] (cuda) -> (scores, tokens, kept, cut), numpy [n]"""
    n = logits.shape[0]
    outs = (np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    _lib.check(op_chat_sample_raw(logits.device.index or 0, P(logits), logits.stride(0), V, P(seen), seen.stride(0), n, penalty,
                                  temperature, top_k, top_p, seed, step, outs), "vr_op_chat_sample")
    return outs


def upload(logits, seen=None):
    """numpy logits [n][V] (and bool seen [n][V]) -> (logits [n][ld] with 1e30 in the columns >= V — they would win if they
    were read —, seen words) on the device"""
    logits = np.array(logits, np.float32)                       # (a copy: the shared rows are read-only)
    n, V = logits.shape
    ld = (V + 127) // 128 * 128
    lg = torch.full((n, ld), 1e30, dtype=torch.float32, device=DEV)
    lg[:, :V] = torch.from_numpy(logits).to(DEV)
    seen = np.zeros((n, V), bool) if seen is None else seen
    sw = torch.from_numpy(chat_ref.seen_words(seen).view(np.int32)).to(DEV)
    torch.cuda.synchronize()
    return lg, sw


def load_tiny_chat(max_rows=9, max_slots=3, max_new=40):
    """(cfg, encoder, head, chat, fixture, the three prompt items, tokenizer) of the recorded tiny model"""
    from PIL import Image
    from visrag_amd.config import tiny_config
    from visrag_amd.engine import HipEncoder
    from visrag_amd.generation import HipChat
    from visrag_amd.modeling import _prompt_item, chat_prompt
    from visrag_amd.synth import iter_synth_weights, synth_lm_head
    from visrag_amd.tokenizer import StandInTokenizer

    class _Words(StandInTokenizer):
        def decode(self, ids):
            return " ".join(f"w{int(i)}" for i in ids) + " "

    cfg = tiny_config()
    F = np.load(os.path.join(HERE, "golden", "chat_tiny.npz"))
    enc = HipEncoder(cfg, device=0, max_images=4, max_tokens=1024, max_seqs=4)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    head = synth_lm_head(cfg, 0)
    chat = HipChat(enc, max_len=720, max_rows=max_rows, dim_model_base=float(F["dim_model_base"]), max_slots=max_slots, max_new=max_new)
    chat.load_head(head.cuda())
    tok = _Words(cfg.vocab_size)
    items = []
    for p, name in enumerate(["cat.jpeg", "dog.jpg"]):
        img = Image.open(os.path.join(HERE, "golden", "inputs", name)).convert("RGB")
        items.append(_prompt_item(*chat_prompt([{"role": "user", "content": QUESTIONS[p]}], img, tok, cfg), tok, 2048))
    items.append(_prompt_item("<用户>" + QUESTIONS[2], [], tok, 2048))
    for p, it in enumerate(items):
        assert it.input_ids == F[f"p{p}_ids"].tolist()
    return cfg, enc, head, chat, F, items, tok
