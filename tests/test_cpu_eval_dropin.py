"""The advertised drop-in, executed: the retrieve phase of the reference's `src/openmatch/driver/eval.py` (`retrieve()` +
`save_results()`) with the names `INTEGRATION.md` section 2 swaps bound to `visrag_amd`, over the same pickle shards and
qrels the reference's own driver ran on, and everything it leaves behind must equal what the reference's driver left
(tests/golden/eval_driver.npz, oracle/gen_golden.py --evaldriver): the TREC file byte for byte, `test_result.log`, the
printed nDCG@10 / Recall@10 / MRR@10 lines.  `eval_mrr` is held to the reference's own results on fixed cases
(tests/golden/eval_mrr.json, oracle/gen_golden.py --evalmrr).  (`pytrec_eval` is not installable here: the run imports
`visrag_amd.pytrec_eval` under that name, as INTEGRATION.md says; its arithmetic has its own known-answer tests below.)
CPU only: the index is the host stand-in of the gloo tests.
"""
import glob
import io
import json
import os
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import visrag_ret_oracle as O  # noqa: E402
from visrag_amd import pytrec_eval as shim  # noqa: E402
from visrag_amd import utils as U  # noqa: E402


class HostIndex:                      # CPU stand-in for HipIndex: the oracle's matmul + top-k
    def __init__(self, dim, capacity, device=0):
        self.rows = np.zeros((0, dim), np.float32)

    def add(self, reps):
        self.rows = np.concatenate([self.rows, np.asarray(reps, np.float32)])

    def __len__(self):
        return len(self.rows)

    def search(self, q, k):
        q = q.numpy() if isinstance(q, torch.Tensor) else q
        kk = min(k, len(self.rows))
        s, i = O.search_topk(q, self.rows, kk)
        return (np.pad(s, ((0, 0), (0, k - kk)), constant_values=-np.inf), np.pad(i, ((0, 0), (0, k - kk)), constant_values=-1))

    def close(self):
        pass


def _on_grid(x):
    """Round to multiples of 2^-10: every product of two unit-vector entries is then a multiple of 2^-20 and every partial
    sum of a 64-wide dot product stays below 2, so fp32 holds each score EXACTLY whatever the summation order (BLAS
    blocking, SIMD width, the GPU's rescoring) and the recorded TREC file is the same bytes on any host."""
    return (np.round(x.astype(np.float64) * 1024.0) / 1024.0).astype(np.float32)


def _write_case(out, golden_dir):
    """Pickle shards as `--phase encode` leaves them (two corpus ranks, one of them split; two query ranks) and a BEIR qrels
    file with graded judgments placed on known reference ranks."""
    g = np.load(os.path.join(golden_dir, "retrieve.npz"))
    C, Q = _on_grid(g["C"]), _on_grid(g["Q"])
    docs = [f"doc{j}" for j in range(len(C))]
    os.makedirs(out, exist_ok=True)
    U.write_shard(os.path.join(out, U.shard_name("corpus", 0, 0, 250)), C[:250], docs[:250])
    U.write_shard(os.path.join(out, U.shard_name("corpus", 0, 250, 400)), C[250:400], docs[250:400])
    U.write_shard(os.path.join(out, U.shard_name("corpus", 1)), C[400:], docs[400:])
    qids = [f"q{j}" for j in range(len(Q))]
    U.write_shard(os.path.join(out, U.shard_name("query", 0)), Q, qids)
    order = np.argsort(-(Q @ C.T), axis=1, kind="stable")
    qrels = os.path.join(out, "qrels.tsv")
    with open(qrels, "w") as f:
        f.write("query-id\tcorpus-id\tscore\n")
        for qi, q in enumerate(qids[:-1]):                          # the last query has no judgments: not evaluated
            for rank, rel in ((qi % 4, 2), (5 + qi, 1), (14, 1), (300, 3), (20 + qi, 0)):
                f.write(f"{q}\t{docs[order[qi, rank]]}\t{rel}\n")
        f.write("q_unranked\tdoc0\t1\n")                             # a judged query the run does not hold
    return qrels


def _run_driver(out, qrels_path, device):
    """driver/eval.py's retrieve() + save_results() (:210-304) statement for statement, with the swapped imports of
    INTEGRATION.md section 2: distributed_parallel_retrieve, save_as_trec, glob + load_from_trec, pytrec_eval ndcg_cut.10 /
    recall.10 (every metric line rewrites test_result.log), eval_mrr(...)['all']."""
    from visrag_amd import pytrec_eval
    from visrag_amd.retriever import distributed_parallel_retrieve
    from visrag_amd.utils import eval_mrr, load_from_trec, save_as_trec
    qrels = {}
    for ln in open(qrels_path).read().strip().split("\n")[1:]:                    # load_beir_qrels, eval.py:58-68
        q, d, r = ln.split("\t")
        qrels.setdefault(q, {})[d] = int(r)
    enc = types.SimpleNamespace(output_dir=out, process_index=0, world_size=1, retrieve_depth=10, trec_save_path=None, device=device)
    buf = io.StringIO()
    with redirect_stdout(buf):
        run = distributed_parallel_retrieve(args=enc, topk=enc.retrieve_depth, index_factory=HostIndex)
        save_as_trec(run, os.path.join(out, f"test.{enc.process_index}.trec"))
        run = {}
        for part in glob.glob(os.path.join(out, "test.*.trec")):
            print("loading", part)
            run.update(load_from_trec(part))
        ev = pytrec_eval.RelevanceEvaluator(qrels, {"ndcg_cut.10", "recall.10"}).evaluate(run)
        for measure in sorted(sorted(ev.items())[-1][1].keys()):
            value = pytrec_eval.compute_aggregated_measure(measure, [m[measure] for m in ev.values()])
            print("{:25s}{:8s}{:.4f}".format(measure, "all", value))
            with open(os.path.join(out, "test_result.log"), "w", encoding="utf-8") as fw:
                fw.write("{:25s}{:8s}{:.4f}\n".format(measure, "all", value))
        print(f"MRR@10: {eval_mrr(qrels, run, 10)['all']}")
    trec = open(os.path.join(out, "test.0.trec"), "rb").read()
    log = open(os.path.join(out, "test_result.log"), "rb").read()
    lines = [ln for ln in buf.getvalue().splitlines() if not ln.startswith("loading")]
    return trec, log, lines


def test_reference_eval_driver_runs_unchanged_with_the_swapped_imports(tmp_path, golden_dir, monkeypatch):
    g = np.load(os.path.join(golden_dir, "eval_driver.npz"))
    ref = (str(g["trec"]).encode(), str(g["log"]).encode(), [str(x) for x in g["lines"]])     # what the reference's driver left
    b = str(tmp_path / "ours")
    qrels = _write_case(b, golden_dir)
    assert open(qrels).read() == str(g["qrels"])                      # the same shards and judgments as the reference's run
    monkeypatch.setitem(sys.modules, "pytrec_eval", shim)            # `import visrag_amd.pytrec_eval as pytrec_eval`
    ours = _run_driver(b, qrels, "cuda:0")   # (a cpu device is refused: no CPU fallback; the stand-in ignores it)

    assert ours[0] == ref[0] and len(ref[0]) > 0                      # test.0.trec, byte for byte
    assert ours[1] == ref[1] and ref[1].startswith(b"recall_10")      # test_result.log (the driver keeps the last measure)
    assert ours[2] == ref[2], (ours[2], ref[2])                       # ndcg_cut_10 / recall_10 / MRR@10 lines
    assert [ln.split()[0] for ln in ref[2]] == ["ndcg_cut_10", "recall_10", "MRR@10:"]
    mrr = float(ref[2][2].split()[1])
    assert 0.3 < mrr < 1.0
    # the DataLoader-facing half of the swap imports too (the encode phase needs a GPU: tests/test_gpu_config*.py)
    import visrag_amd.inference as inf, visrag_amd.modeling as mod
    assert callable(inf.distributed_parallel_embedding_inference) and hasattr(mod.DRModelForInference, "build")


def test_eval_mrr_equals_the_reference(golden_dir):
    qrel = {"q1": {"d1": 1}, "q2": {"d9": 1}}
    run = {"q1": {"d0": .9, "d1": .5}, "q3": {"d1": 1.0}}
    assert U.eval_mrr(qrel, run, 10) == {"q1": 0.5, "all": 0.5}                                  # the verdict's example
    with open(os.path.join(golden_dir, "eval_mrr.json")) as f:
        cases = json.load(f)                                          # the reference's eval_mrr on the same inputs
    assert len(cases) == 42 and cases[0]["results"] == [[10, {"q1": 0.5, "all": 0.5}]]
    for n, case in enumerate(cases):
        for cutoff, want in case["results"]:
            if want == "ZeroDivisionError":
                with pytest.raises(ZeroDivisionError):
                    U.eval_mrr(case["qrel"], case["run"], cutoff)
                continue
            got = U.eval_mrr(case["qrel"], case["run"], cutoff)
            assert got == want and list(got) == list(want), (n, cutoff)
    assert cases[-1]["results"] == [[10, "ZeroDivisionError"]]


def test_pytrec_eval_shim_known_answers():
    """trec_eval's definitions on a case worked by hand: judgments d1:2 d2:1 d3:0 d4:1 d5:3 (d5 never retrieved); the run
    ranks dA dZ (tie at 0.9: doc id DESCENDING -> dZ first) ... """
    qrel = {"q": {"d1": 2, "d2": 1, "d3": 0, "d4": 1, "d5": 3}, "unjudged_only": {"x": 0}, "absent": {"d1": 1}}
    run = {"q": {"dZ": 0.9, "dA": 0.9, "d1": 0.8, "d3": 0.7, "d2": 0.6, "u1": 0.5, "d4": 0.4},
           "unjudged_only": {"x": 1.0, "y": 0.5}, "not_in_qrels": {"d1": 1.0}}
    ev = shim.RelevanceEvaluator(qrel, {"ndcg_cut.3,10", "recall.3,10", "P.5", "map", "recip_rank", "num_rel", "num_rel_ret", "Rprec",
                                        "success.1,5", "map_cut.5", "ndcg"}).evaluate(run)
    assert set(ev) == {"q", "unjudged_only"}
    m = ev["q"]
    # ranking: dZ dA d1 d3 d2 u1 d4 -> judgments - - 2 0 1 - 1
    l2 = np.log2
    dcg10 = 2 / l2(4) + 1 / l2(6) + 1 / l2(8)
    idcg = 3 / l2(2) + 2 / l2(3) + 1 / l2(4) + 1 / l2(5)
    assert m["ndcg_cut_10"] == pytest.approx(dcg10 / idcg, abs=1e-12) and m["ndcg"] == pytest.approx(dcg10 / idcg, abs=1e-12)
    assert m["ndcg_cut_3"] == pytest.approx((2 / l2(4)) / (3 / l2(2) + 2 / l2(3) + 1 / l2(4)), abs=1e-12)
    assert m["recall_3"] == 0.25 and m["recall_10"] == 0.75 and m["P_5"] == 0.4
    assert m["recip_rank"] == pytest.approx(1 / 3) and m["num_rel"] == 4.0 and m["num_rel_ret"] == 3.0
    assert m["map"] == pytest.approx((1 / 3 + 2 / 5 + 3 / 7) / 4) and m["map_cut_5"] == pytest.approx((1 / 3 + 2 / 5) / 4)
    assert m["Rprec"] == 0.25 and m["success_1"] == 0.0 and m["success_5"] == 1.0
    z = ev["unjudged_only"]
    assert z["ndcg_cut_10"] == 0.0 and z["recall_10"] == 0.0 and z["map"] == 0.0 and z["num_rel"] == 0.0
    # ties: descending doc id decides which of two equal scores is "first"
    t = shim.RelevanceEvaluator({"q": {"a": 1}}, {"recip_rank"}).evaluate({"q": {"a": 1.0, "b": 1.0}})
    assert t["q"]["recip_rank"] == 0.5
    # scores pass through C floats: 1 + 1e-9 and 1.0 are the same sim
    t = shim.RelevanceEvaluator({"q": {"a": 1}}, {"recip_rank"}).evaluate({"q": {"a": 1.0 + 1e-9, "b": 1.0}})
    assert t["q"]["recip_rank"] == 0.5
    assert shim.compute_aggregated_measure("ndcg_cut_10", [0.5, 1.0]) == 0.75
    assert shim.compute_aggregated_measure("num_rel", [4.0, 1.0]) == 5.0
    with pytest.raises(ValueError):
        shim.RelevanceEvaluator(qrel, {"no_such_measure"})
    with pytest.raises(TypeError):
        shim.RelevanceEvaluator({"q": {"d": 1.5}}, {"map"})
    # default cutoffs, pytrec_eval's naming
    assert "ndcg_cut_1000" in shim.RelevanceEvaluator(qrel, {"ndcg_cut"}).evaluate(run)["q"]
    nd, rc = U.ndcg_recall_at_k(qrel, run, 10)
    assert nd == pytest.approx((dcg10 / idcg + 0.0) / 2) and rc == pytest.approx(0.375)
