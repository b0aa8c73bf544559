"""Answer scoring next to what it replaces, on one GPU, alternating in one process:

    python tools/answer_score_bench.py [--reps 10] [--skip-model] [--skip-kernel]

Kernel level (the head's shape at full dims: V 122 753, K 2 304, synthetic bf16 operands; M = 32, 256, 2 048 rows):
  head_score    vr_op_head_score: x_t, lse, top_x, top_id per row, the logits never written
  materialise   vr_op_gemm with the fp32 epilogue into a logits buffer [M][122 880] + torch.logsumexp over its rows
and, for the first, the fraction of the head's weight bytes (V x K x 2 = 565.6 MB) over the time that an HBM read of them
at 6.3 TB/s (the rate a streaming copy reaches on an MI355X; 8.0 TB/s is the part's specification) would take.

Model level (full dims, synthetic weights, one 448 x 448 page; answers of 32 and of 256 tokens; 1 and 9 sequences):
  score_items   one packed teacher-forced pass + the fused head
  workaround    per sequence vr_chat_prefill, then per answer token vr_chat_logits (a 491 KB copy), a host log-softmax and
                vr_chat_step
with the largest difference between the two routes' token log-probs.

Every measurement lies between two device events (host work between them included); `--reps` alternations, median
(min - max) in milliseconds.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from visrag_amd import _lib  # noqa: E402

EPI_F32, VARIANT_AUTO = 2, 3
HBM_STREAM_BPS = 6.3e12


def spread_ms(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(todo, reps):
    for _, fn in todo:
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in todo}
    last = {}
    for _ in range(reps):
        for name, fn in todo:
            t, last[name] = timed(fn)
            ms[name].append(t)
    return {name: spread_ms(v) for name, v in ms.items()}, last


def kernel_level(reps):
    lib = _lib.load()
    V, K = 122753, 2304
    Vp = (V + 255) // 256 * 256
    g = torch.Generator(device="cuda").manual_seed(0)
    W = torch.zeros((Vp, K), dtype=torch.bfloat16, device="cuda")
    W[:V] = (torch.randn((V, K), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    res = {"V": V, "K": K, "weight_bytes": V * K * 2, "unit": "ms, device events"}
    for M in (32, 256, 2048):
        Mp = (M + 255) // 256 * 256
        A = torch.zeros((Mp, K), dtype=torch.bfloat16, device="cuda")
        A[:M] = torch.randn((M, K), generator=g, device="cuda").to(torch.bfloat16)
        tgt = torch.randint(0, V, (M,), generator=g, device="cuda", dtype=torch.int32)
        outs = [torch.zeros(M, dtype=torch.float32, device="cuda") for _ in range(3)] + [torch.zeros(M, dtype=torch.int32, device="cuda")]
        logits = torch.zeros((Mp, Vp), dtype=torch.float32, device="cuda")

        def head():
            _lib.check(lib.vr_op_head_score(0, ptr(A), K, ptr(W), K, M, V, K, ptr(tgt), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                            ptr(outs[3]), None), "vr_op_head_score")
            return outs[1].clone()

        def materialise():
            _lib.check(lib.vr_op_gemm(0, ptr(A), K, ptr(W), K, M, Vp, K, EPI_F32, None, None, 1.0, ptr(logits), Vp, None, None, 0,
                                      VARIANT_AUTO, None), "vr_op_gemm")
            return torch.logsumexp(logits[:M, :V], dim=1)

        t, last = alternate([("head_score", head), ("materialise", materialise)], reps)
        t["lse_max_abs_diff"] = float((last["head_score"] - last["materialise"]).abs().max())
        t["weight_read_fraction_of_hbm_stream_rate"] = round((V * K * 2 / HBM_STREAM_BPS * 1e3) / t["head_score"]["median"], 4)
        t["head_score_tflops"] = round(2.0 * Mp * Vp * K / (t["head_score"]["median"] * 1e-3) / 1e12, 1)
        res[f"M{M}"] = t
        del logits
    return res


def model_level(reps):
    from PIL import Image

    from visrag_amd.config import full_config
    from visrag_amd.engine import HipEncoder
    from visrag_amd.generation import HipChat, score_items
    from visrag_amd.preprocess import prepare_item
    from visrag_amd.synth import iter_synth_weights, synth_lm_head, synth_pages
    from visrag_amd.tokenizer import StandInTokenizer
    cfg = full_config()
    enc = HipEncoder(cfg, device=0, max_images=9, max_tokens=3328, max_seqs=9)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    chat = HipChat(enc, max_len=640, max_rows=1, dim_model_base=256.0, max_slots=1, max_new=260)
    chat.load_head(synth_lm_head(cfg, 0, device="cuda"))
    tok = StandInTokenizer(cfg.vocab_size)
    page = Image.fromarray(synth_pages(1, size=448, seed=0)[0])
    item = prepare_item("<用户>what is shown on this page", page, tok, cfg, 2048)
    rng = np.random.default_rng(0)
    res = {"prompt_tokens": len(item.input_ids), "slices": len(item.slices), "unit": "ms, device events"}

    def workaround(conts):
        out = []
        for cont in conts:
            chat.prefill(0, 0, item)
            lps = []
            for t, tk in enumerate(cont):
                l = chat.logits(0).astype(np.float64)
                lps.append(l[tk] - (l.max() + np.log(np.exp(l - l.max()).sum())))
                if t + 1 < len(cont):
                    chat.step([0], [0], [int(tk)])
            out.append(np.asarray(lps))
        return out

    for n_seq in (1, 9):
        for n_tok in (32, 256):
            conts = [rng.integers(16, cfg.vocab_size, n_tok).tolist() for _ in range(n_seq)]
            t, last = alternate([("score_items", lambda: [r["token_logprobs"] for r in score_items(chat, [item] * n_seq, conts)]),
                                 ("workaround", lambda: workaround(conts))], reps)
            t["max_abs_logprob_diff"] = float(max(np.abs(a - b).max() for a, b in zip(last["score_items"], last["workaround"])))
            t["speedup_median"] = round(t["workaround"]["median"] / t["score_items"]["median"], 1)
            res[f"seqs{n_seq}_tokens{n_tok}"] = t
    chat.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("answer_score_bench needs a GPU: there is no CPU fallback")
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0)}
    if not a.skip_kernel:
        res["kernel"] = kernel_level(a.reps)
        print(json.dumps({"kernel": res["kernel"]}), file=sys.stderr, flush=True)
    if not a.skip_model:
        res["model"] = model_level(a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
