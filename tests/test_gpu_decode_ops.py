"""-m gpu: the decode step's kernels at op level — decode attention, the weight-streaming GEMM, its plane consumers
(residual + RMSNorm, SwiGLU) and the candidate selection / sampler of csrc/chat_kernels.hip — each called through the C ABI
(vr_op_gemm_skinny / vr_op_plane_sum / vr_op_chat_attention / vr_op_chat_select) against the fp64 numpy references of
tests/chat_ref.py on the same bf16-rounded inputs.  tests/test_cpu_chat_ref.py shows on the host that these comparisons can
fail (a dropped key, the other temperature, a wrong tie order).  Tolerances are stated per test; the fp32 terms are measured
(tests/decode_bars.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import chat_ref as R  # noqa: E402
from tests import gen_ops_ref as G  # noqa: E402
from tests.decode_bars import ACCUM_FP32_TERM, ATTN_FP32_TERM, SWIGLU_FP32_TERM  # noqa: E402
from tests.gpu_util import from_bf16_bits, op_chat_attention, op_chat_select, op_gemm_skinny, op_plane_sum  # noqa: E402

DEV = "cuda:0"


def _bf(x):
    return from_bf16_bits(R.bf16_bits(x), DEV)


# --------------------------------------------------------------------------- decode attention ---
# Every case prints its worst |got - ref| / (2^-8 |ref| + ATTN_FP32_TERM) (1.0 = the bar) and its worst relative error.
# First MI355X run, worst (error / tolerance, relative error where |ref| >= 1e-2) per case — the bf16 rounding alone reaches
# 2^-8 = 3.9e-3, so ratios close to 1 are the rounding, not the kernel:
#   P1_nb1 0.50 2.0e-3 | P1_nb5 0.94 3.8e-3 | P255 0.84 / 0.85 3.8e-3 | P256 0.86 / 0.80 3.6e-3 | P257 0.95 / 0.79 3.7e-3
#   P513 0.63 / 0.87 3.8e-3 | P2049 0.89 / 0.90 3.6e-3 | P2600 0.96 / 0.97 3.9e-3 | mixed16 0.93 3.8e-3
#   tails_1_256_257_300 0.90 3.6e-3 | spike_last_tail 0.56 2.6e-3 | spike_first_prompt 0.64 3.0e-3
#   spike_all_negative 0.83 3.8e-3 | empty_splits 0.76 3.4e-3
# With `min(CHAT_KEYS - 1, len - j0)` in the kernel's tail loop (one key dropped) tails_1_256_257_300 reads 275.
def _run_attention(name):
    c = R.attention_case(name)
    E, L, l = c["E"], R.ATTN_LAYERS, R.ATTN_LAYER
    g = torch.Generator(device=DEV).manual_seed(R.hash_name(name))
    # everything the step must NOT read (the other layer, other slots and rows, keys past the lengths) holds noise three
    # times the size of the data: a wrong plane, slot, row or length shows
    prompt = (3.0 * torch.randn((L, 2, c["slots"], c["max_len"], E), generator=g, device=DEV)).to(torch.bfloat16)
    tails = (3.0 * torch.randn((L, 2, c["rows"], c["max_new"], E), generator=g, device=DEV)).to(torch.bfloat16)
    for slot, k in c["pk"].items():
        prompt[l, 0, slot, :k.shape[0]] = _bf(k)
        prompt[l, 1, slot, :k.shape[0]] = _bf(c["pv"][slot])
    for row, k in c["tk"].items():
        tails[l, 0, row, :k.shape[0]] = _bf(k)
        tails[l, 1, row, :k.shape[0]] = _bf(c["tv"][row])
    got = op_chat_attention(_bf(c["q"]), prompt, tails, l, [s[0] for s in c["step"]], [s[1] for s in c["step"]],
                            [s[2] for s in c["step"]], c["plen"], c["force"]).float().cpu().numpy().astype(np.float64)
    ref = R.decode_attention_ref(c)
    assert np.isfinite(got).all()
    ratio = np.abs(got - ref) / R.bf16_tol(ref, ATTN_FP32_TERM)
    rel = float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-2)).max())
    i, ch = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"attention {name}: worst |got - ref| / tolerance {ratio.max():.3f} at step row {i}, channel {ch}; "
          f"worst relative error (|ref| >= 1e-2) {rel:.3e}")
    return ratio.max(), (name, int(i), int(ch), float(got[i, ch]), float(ref[i, ch]))


@pytest.mark.parametrize("name", [n for n in R.ATTN_CASES])
def test_chat_attention(name):
    """|got - ref| <= 2^-8 |ref| + ATTN_FP32_TERM: the output is rounded ONCE to bf16, P stays fp32.
    Cases (tests/chat_ref.py::ATTN_CASES; E = 3 x 64, layer 1 of 2, slots 2 and 0):
      P{1,255,256,257,513,2049,2600}_nb{1,5}  chunk and split edges; 5 rows: the accumulator slots acc[1] and rows wave + 4;
                                               2049 / 2600: eight splits, 2600: two chunks per split
      mixed16               16 rows in 5 groups [1, 3, 5, 4, 3], gsplit 1, 2, 8, 1, 3: the early return at sp >= S
      tails_1_256_257_300   the tail loop's second chunk
      spike_*               running maximum raised by the last tail key / set by the first prompt key / far below zero
      empty_splits          forced ranges that hold no key: m = -inf, l = 0 into the merge
    """
    worst, where = _run_attention(name)
    assert worst <= 1.0, where


# ------------------------------------------------------------------------------- skinny GEMM ---
SENTINEL = 12345.0

# (M, N, K, ksplit): every M, N, K, ksplit of the issue's lists; K-splits that do not divide the K-steps (5 steps / 2, 3;
# 36 / 7), more splits than steps (1 step / 2, 3 / 7, 4 / 9), N off the 256 tile (260, 384, 1000), both row-block forms
GEMM_CASES = [(1, 256, 64, 1), (1, 1000, 2304, 7), (5, 260, 320, 2), (5, 384, 192, 7), (16, 256, 256, 3), (16, 1000, 320, 3),
              (17, 260, 64, 2), (17, 384, 2304, 2), (32, 256, 320, 7), (32, 1000, 192, 1), (16, 384, 256, 9), (32, 260, 2304, 3)]


@pytest.mark.parametrize("M,N,K,ksplit", GEMM_CASES)
def test_gemm_skinny_planes(M, N, K, ksplit):
    A, W, b = R.gemm_inputs(M, N, K, 1000 + M + N + K + ksplit)
    rows = 16 if M <= 16 else 32
    Ad = torch.zeros((rows, K), dtype=torch.bfloat16, device=DEV)
    Ad[:M] = _bf(A)
    Wd = torch.zeros(((N + 255) // 256 * 256, K), dtype=torch.bfloat16, device=DEV)
    Wd[:N] = _bf(W)
    ldo = N + 12                                               # room behind the last column
    out = torch.full((ksplit, rows + 3, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    op_gemm_skinny(Ad, Wd, M, N, K, ksplit, bias=torch.from_numpy(b).to(DEV), out=out)
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(got[:, M:, :] == SENTINEL) and np.all(got[:, :, N:] == SENTINEL)       # rows >= M, columns >= N untouched
    planes = R.gemm_split_ref(A, W, ksplit, b)
    # every plane is its own K range (bias on split 0 only; splits past the end are exactly zero) ...
    np.testing.assert_allclose(got[:, :M, :N], planes, rtol=1e-5, atol=1e-4)
    steps, per = K // 64, (K // 64 + ksplit - 1) // ksplit
    for s in range(ksplit):
        if s * per >= steps and s > 0:
            assert np.all(got[s, :M, :N] == 0.0), s
    # ... and their host sum in fp64 is the product, inside the suite's fp32-epilogue bar
    np.testing.assert_allclose(got[:, :M, :N].sum(0), R.gemm_ref(A, W, b), rtol=1e-5, atol=1e-4)
    # without a bias split 0 is the bare product
    out0 = torch.full((ksplit, rows + 3, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    op_gemm_skinny(Ad, Wd, M, N, K, ksplit, out=out0)
    np.testing.assert_allclose(out0[0, :M, :N].cpu().numpy(), R.gemm_split_ref(A, W, ksplit)[0], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("M,I,K,seed", R.SWIGLU_CASES)
def test_swiglu_fused_and_summed(M, I, K, seed):
    """Fused SwiGLU epilogue (ksplit 1) and swiglu_sum over 3 planes: both against the fp64 reference at
    2^-8 |ref| + SWIGLU_FP32_TERM, and against each other to one bf16 ulp.  First MI355X run: worst error / tolerance 0.95
    and 0.98 (the bf16 rounding), the same for both forms."""
    A, Wi, bi, ref = R.swiglu_case(M, I, K, seed)
    N = 2 * I
    Ad = torch.zeros((16, K), dtype=torch.bfloat16, device=DEV)
    Ad[:M] = _bf(A)
    Wd = torch.zeros(((N + 255) // 256 * 256, K), dtype=torch.bfloat16, device=DEV)
    Wd[:N] = _bf(Wi)
    bd = torch.from_numpy(np.ascontiguousarray(bi)).to(DEV)
    ldo = I + 8
    bits = torch.full((19, ldo), SENTINEL, dtype=torch.bfloat16, device=DEV)
    sent = float(bits[0, 0])
    fused = op_gemm_skinny(Ad, Wd, M, N, K, 1, bias=bd, swiglu=True, out=bits.clone()).float().cpu().numpy().astype(np.float64)
    planes = torch.zeros((3, 16, N), dtype=torch.float32, device=DEV)
    op_gemm_skinny(Ad, Wd, M, N, K, 3, bias=bd, out=planes)
    summed = op_plane_sum(1, planes, M, I, out=bits.clone()).float().cpu().numpy().astype(np.float64)
    for name, got in (("fused", fused), ("summed", summed)):
        assert np.all(got[M:] == sent) and np.all(got[:, I:] == sent), name
        ratio = np.abs(got[:M, :I] - ref) / R.bf16_tol(ref, SWIGLU_FP32_TERM)
        print(f"swiglu {name} M={M} I={I} K={K}: worst |got - ref| / tolerance {ratio.max():.3f}")
        assert ratio.max() <= 1.0, name
    assert np.all(np.abs(fused[:M, :I] - summed[:M, :I]) <= R.bf16_ulp(np.maximum(np.abs(fused[:M, :I]), np.abs(summed[:M, :I]))))


# ---------------------------------------------------------------------------- rmsnorm_accum ---
@pytest.mark.parametrize("rows,dim,nsplit,seed", R.ACCUM_CASES)
def test_rmsnorm_accum(rows, dim, nsplit, seed):
    """x += alpha * sum of the planes, then RMSNorm: rows 1 / 16 take the row kernel (planes fetched eight at a time: nsplit 8,
    9, 17 walk its unroll and remainder), 17 / 45 the wave kernel (dim 256 / 2304: NORM_STDV, 3584: NORM_MAXV).  The updated x
    against fp64 at |ref| 2^-23 + ACCUM_FP32_TERM, out at test_rmsnorm's 8e-3 bar; padding columns zero; out = NULL.
    First MI355X run: worst |x - ref| 2.3e-7 .. 7.4e-7 over the cases."""
    x, parts, w, alpha = R.accum_case(rows, dim, nsplit, seed)
    xn, y = R.accum_ref(x, parts, w, alpha)
    ldp = dim + 4
    pd = torch.full((nsplit, rows + 1, ldp), SENTINEL, dtype=torch.float32, device=DEV)
    pd[:, :rows, :dim] = torch.from_numpy(parts).to(DEV)
    wd = torch.from_numpy(w).to(DEV)
    for ldo in ([dim, dim + 64] if dim + 64 <= 3584 else [dim]):
        xd = torch.full((rows + 1, dim + 8), SENTINEL, dtype=torch.float32, device=DEV)
        xd[:rows, :dim] = torch.from_numpy(x).to(DEV)
        out = torch.full((rows + 1, ldo), 7.0, dtype=torch.bfloat16, device=DEV)
        op_plane_sum(0, pd, rows, dim, x=xd, alpha=alpha, weight=wd, eps=1e-5, out=out)
        gx, go = xd.cpu().numpy().astype(np.float64), out.float().cpu().numpy().astype(np.float64)
        assert np.all(gx[rows:] == SENTINEL) and np.all(gx[:, dim:] == SENTINEL) and np.all(go[rows:] == 7.0)
        err = np.abs(gx[:rows, :dim] - xn)
        print(f"rmsnorm_accum rows={rows} dim={dim} nsplit={nsplit} ldo={ldo}: worst |x - ref| {err.max():.3e} (term {ACCUM_FP32_TERM:.1e})")
        assert np.all(err <= 2.0 ** -23 * np.abs(xn) + ACCUM_FP32_TERM)
        np.testing.assert_allclose(go[:rows, :dim], y, rtol=8e-3, atol=8e-3)
        assert np.all(go[:rows, dim:] == 0.0)                   # ldo > dim: the padding columns are written as zero
    # out = NULL: the update alone, the same bits
    xd2 = torch.full((rows + 1, dim + 8), SENTINEL, dtype=torch.float32, device=DEV)
    xd2[:rows, :dim] = torch.from_numpy(x).to(DEV)
    op_plane_sum(0, pd, rows, dim, x=xd2, alpha=alpha, weight=None, out=None)
    assert torch.equal(xd2, xd)


# -------------------------------------------------------------------------------- selection ---
def _select(c, **kw):
    off = [0] + np.cumsum(c["sizes"]).tolist()
    V = c["V"]
    ld = (V + 127) // 128 * 128
    lg = torch.full((len(c["logits"]), ld), 1e30, dtype=torch.float32, device=DEV)       # columns >= V would win if they were read
    lg[:, :V] = torch.from_numpy(c["logits"]).to(DEV)
    seen = torch.from_numpy(R.seen_words(c["seen"]).view(np.int32)).to(DEV)
    return op_chat_select(c["mode"], lg, seen, V, off, c["K"], c["kout"], beam_scores=c["bscore"], penalty=c["pen"], **kw)


@pytest.mark.parametrize("name", list(R.selection_cases()))
def test_chat_select(name):
    """Ids and parents equal the reference exactly (ties to the lower flat index parent * V + token; gaps between distinct
    scores >= 1e-3 by construction); scores within 1e-4, the bar of test_beam_search_rules_on_device_candidates.
    Cases (tests/chat_ref.py::selection_cases): one_slice, one_per_slice (K = 64), short_slices (16 candidates per slice,
    K = 50), groups_K32 / groups_K64 / groups_kout_gt_K (beam groups [1, 3, 5, 4, 3]), neg_inf_* (masked tokens are no
    candidates; 3 finite tokens with K = 6), seen_edges_* (tokens 0, 31, 32, V - 1; penalty 1.2 / 1.0), ties_*."""
    c = R.selection_cases()[name]
    sc, tk, pa = _select(c)
    for g, (rs, rt, rp, _) in enumerate(R.selection_ref(c)):
        assert tk[g].tolist() == rt.tolist(), (name, g)
        assert pa[g].tolist() == rp.tolist(), (name, g)
        k = int((rt >= 0).sum())
        np.testing.assert_allclose(sc[g, :k], rs[:k], rtol=0, atol=1e-4)
        assert np.all(sc[g, k:] == -np.inf)
        live = list(zip(pa[g, :k].tolist(), tk[g, :k].tolist()))
        assert len(set(live)) == k                              # no candidate twice


# Chi-square with 7 degrees of freedom, critical value 40.5 at p = 1e-6.  The host Gumbel-max sampler of
# tests/test_cpu_chat_ref.py gives 3.5 .. 8.1 against its own temperature and 694 .. 1101 against the other one; the test
# prints the device's statistics per (temperature, seed).  First MI355X run, (own, other) per seed:
#   T = 0.7: (8.8, 731) (4.7, 799);  T = 1.5: (6.5, 1078) (8.5, 921).
@pytest.mark.parametrize("T,other", [R.SAMPLE_TEMPS, R.SAMPLE_TEMPS[::-1]])
def test_chat_sampler_distribution(T, other):
    """4096 draws (step = 0..4095) per seed among the top 8 of planted logits: the counts pass a chi-square test against
    softmax(top-8 / T) of the reference and fail it against the other temperature's distribution; nothing outside the top 8 is
    drawn.  A Gumbel-max that returned the argmax, ignored the temperature or reused its noise would fail."""
    x, ids = R.sampling_logits()
    c = dict(mode=R.SAMPLE, V=x.size, sizes=[1], logits=x[None], seen=np.zeros((1, x.size), bool), K=R.SAMPLE_TOPK, kout=1, pen=1.0,
             bscore=None)
    tok, p = R.sampler_probs(x.astype(np.float64), R.SAMPLE_TOPK, T)
    _, p_other = R.sampler_probs(x.astype(np.float64), R.SAMPLE_TOPK, other)
    assert (R.SAMPLE_DRAWS * p).min() >= 40.0
    crit = R.chi2_critical(R.SAMPLE_TOPK - 1, 1e-6)
    index = {int(t): i for i, t in enumerate(tok)}
    for seed in R.SAMPLE_SEEDS:
        counts = np.zeros(len(tok), np.int64)
        draw = _sampler_loop(c, T, seed)
        for step in range(R.SAMPLE_DRAWS):
            sc, tk, pa = draw(step)
            t = int(tk[0, 0])
            assert t in index, (seed, step, t)                  # never outside the top 8
            assert pa[0, 0] == 0 and sc[0, 0] == x[t]
            counts[index[t]] += 1
        own, cross = R.chi2_stat(counts, p), R.chi2_stat(counts, p_other)
        print(f"sampler T={T} seed={seed}: chi2 against own distribution {own:.1f}, against T={other} {cross:.1f}, critical {crit:.1f}")
        assert own < crit, (T, seed, counts.tolist())
        assert cross > crit, (T, seed, counts.tolist())


def _sampler_loop(c, T, seed):
    """the same select with the device buffers kept (4096 calls: no re-upload)"""
    V = c["V"]
    ld = (V + 127) // 128 * 128
    lg = torch.full((1, ld), 1e30, dtype=torch.float32, device=DEV)
    lg[:, :V] = torch.from_numpy(c["logits"]).to(DEV)
    seen = torch.zeros((1, (V + 31) // 32), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    return lambda step: op_chat_select(R.SAMPLE, lg, seen, V, [0, 1], c["K"], 1, temperature=T, seed=seed, step=step)


@pytest.mark.parametrize("seed,step,idx", G.defective_triples())
def test_chat_sampler_defective_draw(seed, step, idx):
    """The chat twin of tests/test_gpu_gen_ops.py::test_sampler_defective_draw: (seed, step, idx) hashes to the draw 0xFFFFFF,
    whose noise the parent's map made infinite.  K = 64 candidates: D at logit 30, token idx and 62 others at 0, everything else
    at -20; T = 1.  The finite noise lies in [-2.86, 16.64], so the draw is D."""
    V = 4096
    D = (idx + 1500) % V
    x = np.full((1, V), -20.0, np.float32)
    others = [t for t in range(7, V, 61) if t not in (idx, D)][:62]
    x[0, others] = 0.0
    x[0, idx] = 0.0
    x[0, D] = 30.0
    c = dict(mode=R.SAMPLE, V=V, sizes=[1], logits=x, seen=np.zeros((1, V), bool), K=64, kout=1, pen=1.0, bscore=None)
    sc, tk, pa = _select(c, temperature=1.0, seed=seed, step=step)
    assert int(tk[0, 0]) == D and pa[0, 0] == 0 and sc[0, 0] == 30.0


def test_chat_sampler_top64_membership():
    """top_k = CHAT_TOPK_MAX: every draw lies among the 64 best penalised logits"""
    x = R.grid_logits(1, 1000, 301, step=0.05)
    seen = np.zeros((1, 1000), bool)
    seen[0, np.argsort(-x[0])[:5]] = True                       # the five best are penalised: the kept set changes
    s = R.candidate_scores(x, seen, R.SAMPLE, 1.3)
    top = set(np.argsort(-s[0], kind="stable")[:64].tolist())
    c = dict(mode=R.SAMPLE, V=1000, sizes=[1], logits=x, seen=seen, K=64, kout=1, pen=1.3, bscore=None)
    drawn = set()
    for step in range(200):
        sc, tk, pa = _select(c, temperature=1.5, seed=3, step=step)
        assert int(tk[0, 0]) in top
        drawn.add(int(tk[0, 0]))
    assert len(drawn) > 10                                      # (and not one token over and over)


def test_chat_sampler_masked_rows():
    """-inf logits in SAMPLE mode, one row per group: a row that is all -inf has no candidate and reports (-inf, -1, -1) in
    every output (not what an earlier call left in the buffers); a row with 3 finite tokens and top_k = 6 draws among those
    three only, and over 64 steps not one of them alone."""
    x = R.grid_logits(3, 1000, 311)
    keep = [17, 500, 999]
    x[0] = -np.inf
    x[1] = -np.inf
    x[1, keep] = [0.5, 2.0, -1.0]
    c = dict(mode=R.SAMPLE, V=1000, sizes=[1, 1, 1], logits=x, seen=np.zeros((3, 1000), bool), K=6, kout=2, pen=1.0, bscore=None)
    full = dict(c, logits=R.grid_logits(3, 1000, 312))
    drawn = set()
    for step in range(64):
        if step % 16 == 0:
            _, tk, _ = _select(full, temperature=1.0, seed=11, step=step)      # the output buffers hold three valid draws
            assert np.all(tk[:, 0] >= 0)
        sc, tk, pa = _select(c, temperature=1.0, seed=11, step=step)
        assert np.all(sc[0] == -np.inf) and tk[0].tolist() == [-1, -1] and pa[0].tolist() == [-1, -1], step
        assert int(tk[1, 0]) in keep and pa[1, 0] == 0 and sc[1, 0] == x[1, tk[1, 0]], step
        assert sc[1, 1] == -np.inf and tk[1, 1] == -1 and pa[1, 1] == -1
        top6 = np.argsort(-x[2], kind="stable")[:6]
        assert int(tk[2, 0]) in top6 and pa[2, 0] == 0
        drawn.add(int(tk[1, 0]))
    assert len(drawn) >= 2


# ------------------------------------------------------------------------------- arguments ---
def test_entries_refuse_bad_arguments():
    """counts, capacities, alignment and NULLs are refused on the host (VR_ERR_INVALID = 1 / VR_ERR_CAPACITY = 4): nothing is
    launched.  Shapes the device could not survive are never passed down to see what happens."""
    from visrag_amd._lib import VisragHipError
    A = torch.zeros((32, 64), dtype=torch.bfloat16, device=DEV)
    W = torch.zeros((256, 64), dtype=torch.bfloat16, device=DEV)
    out = torch.zeros((1, 32, 256), dtype=torch.float32, device=DEV)
    for kw, status in ((dict(M=33, N=256, K=64), 4), (dict(M=0, N=256, K=64), 1), (dict(M=4, N=254, K=64), 1), (dict(M=4, N=256, K=32), 1),
                       (dict(M=4, N=256, K=64, ksplit=0), 1), (dict(M=17, N=256, K=64, swiglu=True), 4),
                       (dict(M=4, N=256, K=64, ksplit=2, swiglu=True), 1), (dict(M=4, N=256, K=64, ldo=128), 1)):
        with pytest.raises(VisragHipError, match=f"status {status}"):
            op_gemm_skinny(A, W, out=out, **kw)
    with pytest.raises(VisragHipError, match="status 1"):
        op_gemm_skinny(A, W, 4, 256, 64, out=None, ldo=256, split_stride=0)
    parts = torch.zeros((2, 4, 256), dtype=torch.float32, device=DEV)
    x = torch.zeros((4, 256), dtype=torch.float32, device=DEV)
    with pytest.raises(VisragHipError, match="status 1"):
        op_plane_sum(0, parts, 4, 256, x=None)
    with pytest.raises(VisragHipError, match="status 1"):
        op_plane_sum(0, parts, 4, 254, x=x)
    with pytest.raises(VisragHipError, match="status 1"):
        op_plane_sum(1, parts, 4, 256, out=torch.zeros((4, 256), dtype=torch.bfloat16, device=DEV))      # ldp < 2 dim
    with pytest.raises(VisragHipError, match="status 1"):
        op_plane_sum(2, parts, 4, 256, x=x)
    q = torch.zeros((17, 192), dtype=torch.bfloat16, device=DEV)
    prompt = torch.zeros((2, 2, 3, 10, 192), dtype=torch.bfloat16, device=DEV)
    tails = torch.zeros((2, 2, 17, 4, 192), dtype=torch.bfloat16, device=DEV)
    for args, status in ((([0], [0], [4], [5, 0, 0]), 4),                 # tail index past max_new
                         (([0], [0], [0], [11, 0, 0]), 4),                # prompt longer than max_len
                         (([0], [1], [0], [5, 0, 0]), 1),                 # slot without a prompt
                         (([0, 0], [0, 0], [0, 0], [5, 0, 0]), 1),        # a row twice
                         (([0, 1, 2], [0, 1, 0], [0, 0, 0], [5, 5, 0]), 1),   # a slot's rows apart
                         (([17], [0], [0], [5, 0, 0]), 1),                # row out of range
                         ((list(range(17)), [0] * 17, [0] * 17, [5, 0, 0]), 4)):   # more than 16 rows
        with pytest.raises(VisragHipError, match=f"status {status}"):
            op_chat_attention(q[:len(args[0])], prompt, tails, 1, *args)
    with pytest.raises(VisragHipError, match="status 1"):
        op_chat_attention(q[:1], prompt, tails, 2, [0], [0], [0], [5, 0, 0])          # layer out of range
    lg = torch.zeros((2, 128), dtype=torch.float32, device=DEV)
    sn = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    for kw, status in ((dict(K=65, kout=1), 4), (dict(K=1, kout=65), 4), (dict(K=0, kout=1), 1), (dict(K=4, kout=4, penalty=0.0), 1),
                       (dict(K=4, kout=4, V=200), 1)):
        with pytest.raises(VisragHipError, match=f"status {status}"):
            op_chat_select(R.BEAM, lg, sn, kw.pop("V", 100), [0, 2], **kw)
    with pytest.raises(VisragHipError, match="status 1"):
        op_chat_select(R.GREEDY, lg, sn, 100, [0, 2], 4, 4)                            # a greedy group of two rows
    with pytest.raises(VisragHipError, match="status 1"):
        op_chat_select(R.SAMPLE, lg, sn, 100, [0, 1], 4, 1, temperature=0.0)
