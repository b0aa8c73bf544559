"""The nucleus sampler (vr_op_chat_sample) next to the present top-k sampler (vr_op_chat_select in SAMPLE mode) on one GPU,
alternating in one process, at the vocabulary of the full model:

    python tools/chat_sample_bench.py [--vocab 122753 --reps 10] [--step-share]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/chat_sample_bench.py --reps 3

Rows are seeded normal logits (standard deviation 3) with 20 seen ids each, repetition penalty 1.05, temperature 0.7; 1 and 16
rows.  Every call — launch, the copy of the results to the host, the stream synchronisation the entry ends with — lies between
two device events; `--reps` alternations, median (min - max) in microseconds.  The two samplers return different things (the
nucleus sampler also counts the kept set and names its last token, the present one cannot go past 64 candidates or filter by
mass): only (top_k <= 64, top_p = 1) is comparable, and there the tool also checks that both draw the same tokens.

--step-share: a chat handle at the full model's dimensions (synthetic weights, one text prompt): the time of one
vr_chat_step and of one vr_chat_sample draw (top_k 100, top_p 0.8) on its logits, host clock around each call.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from visrag_amd import _lib  # noqa: E402

SAMPLE = 2
PEN, TEMP = 1.05, 0.7


def spread_us(v):
    v = sorted(v)
    return {"median": round(1e3 * v[len(v) // 2], 1), "min": round(1e3 * v[0], 1), "max": round(1e3 * v[-1], 1)}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=122753)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-share", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chat_sample_bench needs a GPU: there is no CPU fallback")
    lib = _lib.load()
    V, ld, words = a.vocab, (a.vocab + 127) // 128 * 128, (a.vocab + 31) // 32
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.zeros((16, ld), dtype=torch.float32, device="cuda")
    logits[:, :V] = 3.0 * torch.randn((16, V), generator=g, device="cuda")
    rng = np.random.default_rng(0)
    sw = np.zeros((16, words), np.uint32)
    for r in range(16):
        for t in rng.integers(0, V, 20):
            sw[r, t >> 5] |= np.uint32(1 << (t & 31))
    seen = torch.from_numpy(sw.view(np.int32)).cuda()
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    step = [0]

    def sample(n, top_k, top_p):
        sc, tk, kept, cut = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)

        def run():
            _lib.check(lib.vr_op_chat_sample(0, ptr(logits), ld, V, ptr(seen), words, n, PEN, TEMP, top_k, top_p, C.c_uint64(7), step[0],
                                             pf(sc), p32(tk), p32(kept), p32(cut), None), "vr_op_chat_sample")
            return tk.copy(), kept.copy()
        return run

    def select(n, K):
        sc, tk, pa = np.zeros((n, 1), np.float32), np.zeros((n, 1), np.int32), np.zeros((n, 1), np.int32)
        off = (C.c_int32 * (n + 1))(*range(n + 1))

        def run():
            _lib.check(lib.vr_op_chat_select(0, SAMPLE, ptr(logits), ld, V, ptr(seen), words, n, off, None, K, 1, PEN, TEMP, C.c_uint64(7),
                                             step[0], pf(sc), p32(tk), p32(pa), None), "vr_op_chat_select")
            return tk[:, 0].copy(), None
        return run

    res = {"vocab": V, "reps": a.reps, "penalty": PEN, "temperature": TEMP, "unit": "us per call, device events"}
    for n in (1, 16):
        todo = [("sample_k100_p0.8", sample(n, 100, 0.8)), ("sample_k0_p0.8", sample(n, 0, 0.8)), ("sample_k1000_p1", sample(n, 1000, 1.0)),
                ("sample_k0_p1", sample(n, 0, 1.0)), ("sample_k50_p1", sample(n, 50, 1.0)), ("sample_k64_p1", sample(n, 64, 1.0)),
                ("select_K50", select(n, 50)), ("select_K64", select(n, 64))]
        for _, fn in todo:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in todo}
        kept = {}
        for rep in range(a.reps):
            step[0] = rep
            drawn = {}
            for name, fn in todo:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                drawn[name], k = fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
                if k is not None:
                    kept[name] = [int(k.min()), int(k.max())]
            for K in (50, 64):
                if drawn[f"sample_k{K}_p1"].tolist() != drawn[f"select_K{K}"].tolist():
                    raise SystemExit(f"rows={n} rep={rep}: the two samplers disagree at top_k={K}, top_p=1")
        res[f"rows{n}"] = {name: spread_us(v) for name, v in ms.items()}
        res[f"rows{n}"]["kept_min_max"] = kept
    if a.step_share:
        from visrag_amd.config import full_config
        from visrag_amd.engine import HipEncoder
        from visrag_amd.generation import HipChat
        from visrag_amd.modeling import _prompt_item
        from visrag_amd.synth import iter_synth_weights, synth_lm_head
        from visrag_amd.tokenizer import StandInTokenizer
        cfg = full_config()
        enc = HipEncoder(cfg, device=0, max_images=1, max_tokens=256, max_seqs=1)
        enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
        chat = HipChat(enc, max_len=128, max_rows=1, dim_model_base=256.0, max_slots=1, max_new=a.reps + 8)
        chat.load_head(synth_lm_head(cfg, 0, device="cuda"))
        tok = StandInTokenizer(cfg.vocab_size)
        chat.prefill(0, 0, _prompt_item("<用户>What is the capital of France?", [], tok, 2048))
        t_step, t_draw = [], []
        for rep in range(a.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, tk, _, _ = chat.sample([0], PEN, TEMP, 100, 0.8, seed=7, step=rep)
            t1 = time.perf_counter()
            chat.step([0], [0], [int(tk[0])])
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep >= 2:
                t_draw.append((t1 - t0) * 1e3)
                t_step.append((t2 - t1) * 1e3)
        d, s = spread_us(t_draw), spread_us(t_step)
        res["full_model_one_row"] = {"unit": "us, host clock", "vr_chat_sample": d, "vr_chat_step": s,
                                     "draw_share_of_step_plus_draw": round(d["median"] / (d["median"] + s["median"]), 4)}
        chat.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
