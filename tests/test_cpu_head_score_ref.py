"""The references of the answer-scoring tests, checked on the CPU: the fp64 head and its bound (tests/head_score_ref.py) on
the planted inputs, a model of the kernel's tiling that shows the GPU test can fail, `sequence_score` on the reference
model's recorded beam log-probs (tests/golden/chat_tiny.npz), and the marginal-selection arithmetic worked by hand."""
import os

import numpy as np
import torch

from tests import head_score_ref as R
from visrag_amd.generation import marginal_weights, sequence_score
from visrag_amd.modeling import select_weighted

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chat_tiny.npz")
LSE_SLACK = 2e-5        # the GPU test's allowance on top of max_v bound (fp32 exp / log and the hierarchical sum)


def _case():
    c = R.make_case(40, 1000, 256, "cpu")
    return c, R.head_score_ref(c["A"][:40], c["W"][:1000], c["target"])


def test_planted_rows_have_a_decided_maximum():
    c, ref = _case()
    kinds = c["kinds"]
    assert {"planted", "all_negative", "spike80", "magnitude300", "all_equal", "tie_tiles", "tie_waves"} == set(kinds)
    for m, k in enumerate(kinds):
        margin = ref["top_x"][m] - ref["second"][m]
        if k in ("all_equal", "tie_tiles", "tie_waves"):
            assert margin == 0.0                         # exact ties: the tie rule decides
        else:
            assert margin > 2 * ref["bound_max"][m], (m, k)
    m = kinds.index("all_negative")
    assert ref["top_x"][m] <= -20
    m = kinds.index("spike80")
    assert ref["top_x"][m] - ref["second"][m] >= 80 and abs(ref["lse"][m] - ref["top_x"][m]) < 1e-12
    m = kinds.index("magnitude300")
    assert 250 < ref["top_x"][m] < 400
    m = kinds.index("all_equal")
    assert ref["top_id"][m] == 0 and abs(ref["lse"][m] - (1.5 + np.log(1000))) < 1e-12
    assert ref["top_id"][kinds.index("tie_tiles")] == R.TIE_A[0] and ref["top_x"][kinds.index("tie_tiles")] == 2.0
    assert ref["top_id"][kinds.index("tie_waves")] == R.TIE_B[0]
    # targets: equal to and different from the argmax, in the same and in another tile; the columns the issue names
    same = c["target"] == ref["top_id"]
    tile = c["target"] // 256 == ref["top_id"] // 256
    assert same.any() and (~same & tile).any() and (~same & ~tile).any()
    assert {0, 255, 256, 999} <= set(c["target"].tolist())
    assert any(768 < t < 999 for t in c["target"].tolist())
    assert {0, 3} <= set((ref["top_id"] // 256).tolist())           # a maximum in the first and in the last tile


def test_the_bound_covers_fp32_accumulation():
    """x computed with fp32 accumulation in a hostile order (a serial chain) stays within the bound of the fp64 value."""
    c, ref = _case()
    A, W = c["A"][:40].to(torch.float32), c["W"][:1000].to(torch.float32)
    acc = torch.zeros((40, 1000), dtype=torch.float32)
    for k in range(256):
        acc += A[:, k:k + 1] * W[:, k][None, :]
    x64 = (A.to(torch.float64) @ W.to(torch.float64).T)
    bound = (A.abs().to(torch.float64) @ W.abs().to(torch.float64).T) * (256 * 2.0 ** -24)
    assert bool(((acc.to(torch.float64) - x64).abs() <= bound).all())
    assert float(bound.max()) < 1e-2


def test_the_gpu_test_can_fail():
    c, ref = _case()
    A, W = c["A"][:40], c["W"][:1000]
    bar = ref["bound_max"] + LSE_SLACK
    honest = R.tiled_model(A, W, 1000)
    assert (np.abs(honest - ref["lse"]) < 1e-9).all()
    # counting the 24 zero pad columns: log(24) above an all-negative row's true lse of about -38
    m = c["kinds"].index("all_negative")
    padded = R.tiled_model(A, W, 1000, count_pad=True)
    assert abs(padded[m] - ref["lse"][m]) > 1e4 * bar[m]
    assert (np.abs(padded - ref["lse"]) > bar).sum() >= 30         # ... and most other rows move as well
    # losing one vocab tile's partial
    for t in range(4):
        dropped = R.tiled_model(A, W, 1000, drop_tile=t)
        assert (np.abs(dropped - ref["lse"]) > 100 * bar).any(), t


def test_sequence_score_on_the_recorded_reference_beams():
    F = np.load(FIX)
    pen = float(F["pen_beam"])
    for p in range(int(F["n_prompts"])):
        pre, ln = F[f"p{p}_beam_q_prefix"], F[f"p{p}_beam_q_len"]
        table = {tuple(pre[i, :ln[i]].tolist()): (F[f"p{p}_beam_q_ids"][i], F[f"p{p}_beam_q_logprobs"][i]) for i in range(len(ln))}
        toks = F[f"p{p}_beam_tokens"].tolist()
        lps = []
        for t, tok in enumerate(toks):
            ids, lp = table[tuple(toks[:t])]
            (j,) = np.nonzero(ids == tok)[0]
            lps.append(float(lp[j]))
        assert len(lps) == 20
        got = sequence_score(lps, toks, pen)
        assert abs(got - float(F[f"p{p}_beam_score"])) < 1e-6, (p, got)
        plain, total = sequence_score(lps, toks, return_sum=True)
        assert abs(total - sum(lps)) < 1e-12 and abs(plain - sum(lps) / 20) < 1e-12
        assert abs(sequence_score(lps, toks, 1.0, 2.0) - sum(lps) / 400) < 1e-12


def test_sequence_score_penalises_repeats_only():
    lp = [-1.0, -2.0, -0.5, -0.25]
    assert sequence_score(lp, [5, 6, 5, 7], 2.0) == (-1.0 - 2.0 - 1.0 - 0.25) / 4
    assert sequence_score(lp, [5, 6, 8, 7], 2.0) == (-3.75) / 4
    assert sequence_score(lp, [5, 5, 5, 5], 2.0, 0.0) == -1.0 - 4.0 - 1.0 - 0.5


def test_marginal_selection_arithmetic_by_hand():
    """Three pages, p = (1/2, 1/4, 1/4).  Page 0 answers X, pages 1 and 2 both answer Y.  Each page scores its own answer at
    log(0.6) and the other answer at log(0.1).  Weighted selection: X 0.5 * 0.6 = 0.30 beats Y's 0.25 * 0.6 = 0.15 per page.
    Marginal: X = 0.5 * 0.6 + 0.25 * 0.1 + 0.25 * 0.1 = 0.35;  Y = 0.5 * 0.1 + 0.25 * 0.6 + 0.25 * 0.6 = 0.35 ... a tie, so
    the pages' agreement is made to count by scoring Y at log(0.7) on its pages: Y = 0.05 + 0.175 + 0.175 = 0.40 > 0.35,
    while weighted selection still prefers X (0.30 against 0.175)."""
    doc = np.log([0.5, 0.25, 0.25])
    l = np.log
    S = [[l(0.6), l(0.1), l(0.1)],       # X on pages 0, 1, 2
         [l(0.1), l(0.7), l(0.7)]]       # Y
    index, weights, p = marginal_weights(S, doc)
    np.testing.assert_allclose(p, [0.5, 0.25, 0.25], rtol=1e-12)
    np.testing.assert_allclose(weights, [0.35, 0.40], rtol=1e-12)
    assert index == 1
    ws_index, ws_weights, _ = select_weighted([l(0.6), l(0.7), l(0.7)], doc)
    assert ws_index == 0
    np.testing.assert_allclose(ws_weights, [0.30, 0.175, 0.175], rtol=1e-12)
    assert weights[0] >= ws_weights[0] and weights[1] >= max(ws_weights[1:])
    # the full 3 x 3 form (every page's answer a candidate of its own): the duplicate rows tie and the first one wins
    S3 = [S[0], S[1], S[1]]
    index3, weights3, _ = marginal_weights(S3, doc)
    assert index3 == 1 and weights3[1] == weights3[2]
    # first among equals
    assert marginal_weights([[0.0, 0.0], [0.0, 0.0]], [1.0, 2.0])[0] == 0
