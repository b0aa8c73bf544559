"""-m gpu: the EVisRAG generator's small kernels (csrc/gen_kernels.hip) at op level — multimodal RoPE + KV-cache append, the vision
tower's 2-D rotary embedding, the row movers, decode_begin, mark_seen and the sampler — each called through the C ABI
(vr_op_gen_*) against the numpy restatements of tests/gen_ops_ref.py: one launch, float64 reference, the shapes at which the
kernel can go wrong.  tests/test_cpu_gen_ops_ref.py pins the restatements against the oracles and shows on the host that the
comparisons can fail (swapped sections, a neighbouring frequency, the parent's noise map).  Every buffer a kernel writes is the
test's, prefilled with a sentinel, and is compared whole: what must not be written is checked as strictly as what must."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import chat_ref as C  # noqa: E402
from tests import gen_ops_ref as R  # noqa: E402
from tests.gpu_util import (from_bf16_bits, op_gen_decode_begin, op_gen_mark_seen, op_gen_mrope_cache, op_gen_rope2d,  # noqa: E402
                            op_gen_rows, op_gen_sample)

DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                         # (a copy: the case tables are read-only)


def _bits(t):
    """bf16 tensor -> uint16 bit patterns (numpy)"""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _sentinel_bf16(shape):
    t = torch.full(shape, R.SENTINEL, dtype=torch.bfloat16, device=DEV)
    return t, int(_bits(t).reshape(-1)[0])


# --------------------------------------------------------------------------- M-RoPE + cache ---
def _run_mrope(H, KV, T, placement, first, x, src_kw):
    """one launch -> (q bits [T + 2][ldq], k bits, v bits [16][ld_cache], cu_kv or None, the sentinel's bits)"""
    cols, ldq, ldc = (H + 2 * KV) * 128, H * 128 + R.MROPE_PAD, KV * 128 + R.MROPE_PAD
    pos3 = R.mrope_positions(T, first)
    q, sent = _sentinel_bf16((T + 2, ldq))
    k, _ = _sentinel_bf16((R.MROPE_CACHE_ROWS, ldc))
    v, _ = _sentinel_bf16((R.MROPE_CACHE_ROWS, ldc))
    kw = dict(cache_row0=R.MROPE_ROW0[placement])
    cu = None
    if placement != "cache_rows":
        cu = torch.full((4,), -5, dtype=torch.int32, device=DEV)
        kw["cu_kv"] = cu
    if placement == "device_row0":
        kw.update(cache_row0=1, row0_dev=_dev(np.array([R.MROPE_ROW0[placement], -9], np.int32)))       # the host's value is NOT the row
    if placement == "cache_rows":
        kw["cache_rows"] = _dev(np.array(R.MROPE_ROWS[:T], np.int32))
    op_gen_mrope_cache(T, H, KV, _dev(pos3), pos3.shape[1], R.MROPE_SECTIONS, _dev(R.mrope_inv_freq()), q, ldq, k, v, ldc, **src_kw, **kw)
    return _bits(q), _bits(k), _bits(v), (cu.cpu().numpy() if cu is not None else None), sent, pos3, cols


def _check_mrope(H, KV, T, placement, first, x, src_kw, tag):
    """x: the float32 rows the kernel rotates (the bf16 rows, or the float32 plane sum)"""
    qb, kb, vb, cu, sent, pos3, cols = _run_mrope(H, KV, T, placement, first, x, src_kw)
    rows = R.mrope_cache_rows(placement, T)
    ref = R.mrope_ref(x, pos3, R.mrope_inv_freq(), H, KV)
    # everything outside the written rows and columns keeps the sentinel
    assert (qb[T:] == sent).all() and (qb[:, H * 128:] == sent).all(), tag
    other = np.ones(R.MROPE_CACHE_ROWS, bool)
    other[rows] = False
    for cb in (kb, vb):
        assert (cb[other] == sent).all() and (cb[:, KV * 128:] == sent).all(), tag
    if cu is not None:
        assert cu.tolist() == [0, R.MROPE_ROW0[placement] + T, -5, -5], tag
    # v: copied, the bf16 of the float32 rows bit for bit
    np.testing.assert_array_equal(vb[rows, :KV * 128], R.bf16_bits(x[:, (H + KV) * 128:]), err_msg=tag)
    # q and k: one bf16 rounding of the float32 rotation
    got = np.concatenate([R.bf16_to_f32(qb[:T, :H * 128]), R.bf16_to_f32(kb[rows, :KV * 128])], axis=1).astype(np.float64)
    worst, same = R.rotation_check(got, ref[:, :(H + KV) * 128])
    print(f"mrope {tag}: worst (|got - ref| - ulp/2) / margin {worst:.3f}, share of elements with the reference's bits {same:.4f}")
    assert worst <= 1.0, tag
    assert same >= R.ROT_EXACT_SHARE, tag


@pytest.mark.parametrize("T", R.MROPE_T)
@pytest.mark.parametrize("H,KV", R.MROPE_HEADS)
def test_mrope_cache_bf16_rows(H, KV, T):
    """bf16 qkv rows with ld beyond the used columns, every cache placement; the positions walk R.MROPE_POS from a different
    start per case (T = 5 covers five of the six rows, the three T = 1 cases of a geometry three different ones).
    First MI355X run: worst excess / margin -3.18 .. -0.000 over the 36 launches (no element outside half a bf16 ulp of the
    reference), share of exact bits 1.0 in every one."""
    x = R.mrope_rows_input(H, KV, T)
    cols = x.shape[1]
    src = torch.full((T + 1, cols + R.MROPE_PAD), 3.0, dtype=torch.bfloat16, device=DEV)
    src[:T, :cols] = from_bf16_bits(R.bf16_bits(x), DEV)
    for i, placement in enumerate(R.MROPE_PLACEMENTS):
        first = (H + T + 2 * i) % len(R.MROPE_POS)
        _check_mrope(H, KV, T, placement, first, x, dict(src=src, ld=cols + R.MROPE_PAD), f"H={H} KV={KV} T={T} {placement} first={first}")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("n_parts", R.MROPE_PARTS)
def test_mrope_cache_split_k_planes(n_parts, bias):
    """fp32 split-K planes (+ bias): the sum is the sequential float32 sum bias + p0 + p1 + ... — the v slots carry its bf16 bits
    exactly — with 1, 7, 8, 9, 16, 17 planes (the 8-wide unrolled sum, its tail, two rounds, two rounds and a tail).
    First MI355X run: worst excess / margin -0.19 .. +0.000 (below 0.0005) over the 24 launches, share of exact bits 1.0 in every one."""
    for (H, KV, T), placement in (((3, 1, 3), R.MROPE_PLACEMENTS[n_parts % 3]), ((4, 2, 5), R.MROPE_PLACEMENTS[(n_parts + 1) % 3])):
        parts, b = R.mrope_planes_input(H, KV, T, n_parts)
        cols, ld = parts.shape[2], parts.shape[2] + R.MROPE_PAD
        stride = (T + 1) * ld + 16                                            # a plane is more than its rows
        pd = torch.full((n_parts, stride), 1.0e4, dtype=torch.float32, device=DEV)
        rows_view = pd[:, :T * ld].view(n_parts, T, ld)
        rows_view[:, :, :cols] = _dev(parts)
        x = R.plane_sum_f32(parts, b if bias else None)
        kw = dict(parts=pd, n_parts=n_parts, plane_stride=stride, ld=ld, bias=_dev(b) if bias else None)
        _check_mrope(H, KV, T, placement, n_parts, x, kw, f"planes={n_parts} bias={bias} H={H} KV={KV} T={T} {placement}")


# ------------------------------------------------------------------------ vision 2-D RoPE ---
@pytest.mark.parametrize("hh,heads,T", R.ROPE2D_CASES)
def test_rope2d_in_place(hh, heads, T):
    """q and k head slots rotated in place (hh = 40: the 7B tower's head_dim 80, lanes >= hh idle), pos_h != pos_w in every row,
    sec_h = hh / 2; the v columns and the padding keep their bits.  First MI355X run: worst excess / margin -0.58 / -0.026 / -0.005 / -0.038
    in the order of the cases, share of exact bits 1.0 in every one."""
    x = R.rope2d_input(hh, heads, T)
    ph, pw = R.rope2d_positions(T)
    f = R.rope2d_freq(hh)
    ld, n_slots = x.shape[1], 2 * heads
    qkv = torch.full((T + 1, ld), 3.0, dtype=torch.bfloat16, device=DEV)
    qkv[:T] = from_bf16_bits(R.bf16_bits(x), DEV)
    before = _bits(qkv).copy()
    op_gen_rope2d(qkv, ld, T, n_slots, hh, _dev(ph), _dev(pw), hh // 2, _dev(f))
    after = _bits(qkv)
    used = n_slots * 2 * hh
    np.testing.assert_array_equal(after[:, used:], before[:, used:])          # v and padding
    np.testing.assert_array_equal(after[T:], before[T:])
    ref = R.rope2d_ref(x, hh, n_slots, ph, pw, hh // 2, f)
    worst, same = R.rotation_check(R.bf16_to_f32(after[:T, :used]), ref[:, :used])
    print(f"rope2d hh={hh} heads={heads} T={T}: worst excess / margin {worst:.3f}, share of exact bits {same:.4f}")
    assert worst <= 1.0 and same >= R.ROT_EXACT_SHARE
    assert (after[:T, :used] != before[:T, :used]).mean() > 0.5               # (and it did rotate: row 0 has pos_h = 0, slow pairs barely turn)


# ----------------------------------------------------------------------------- row movers ---
def test_scatter_and_gather_rows():
    g = R.rng(7500)
    n, dim, idx = len(R.ROWS_IDX), R.ROWS_DIM, np.array(R.ROWS_IDX, np.int32)
    # scatter: dst[idx[i]][:dim] = src[i]
    src = g.standard_normal((n, dim)).astype(np.float32)
    dst = torch.full((R.ROWS_SRC + 1, R.ROWS_LD_SCATTER), R.SENTINEL, dtype=torch.float32, device=DEV)
    op_gen_rows(0, n, dst, R.ROWS_LD_SCATTER, src=_dev(src), row_idx=_dev(idx), dim=dim)
    want = np.full((R.ROWS_SRC + 1, R.ROWS_LD_SCATTER), R.SENTINEL, np.float32)
    want[idx, :dim] = src
    np.testing.assert_array_equal(dst.cpu().numpy(), want)
    # gather: dst[i] = bf16(src[idx[i]]), zero pad; rows from n on untouched
    src = (g.standard_normal((R.ROWS_SRC, dim)) * 3.0).astype(np.float32)
    out, sent = _sentinel_bf16((n + 2, R.ROWS_LD_GATHER))
    op_gen_rows(1, n, out, R.ROWS_LD_GATHER, src=_dev(src), row_idx=_dev(idx), dim=dim)
    got = _bits(out)
    np.testing.assert_array_equal(got[:n, :dim], R.bf16_bits(src[idx]))
    assert (got[:n, dim:] == 0).all() and (got[n:] == sent).all()


def test_patch_rows_u8():
    """two pages of different widths, every patch of both (last row, last column), P = 14, tp = 2, ld = 1176 + 8: the bits of the
    float32 restatement, identical temporal copies, zero pad"""
    pages = R.patch_pages()
    img, ph, pw = R.patch_list()
    n = len(img)
    out, sent = _sentinel_bf16((n + 1, R.PATCH_LD))
    op_gen_rows(2, n, out, R.PATCH_LD, pages=[_dev(p) for p in pages], page_w=[p.shape[1] for p in pages], img=_dev(img), ph=_dev(ph),
                pw=_dev(pw), patch=R.PATCH_P, tp=R.PATCH_TP, mean=R.PATCH_MEAN, std=R.PATCH_STD)
    got = _bits(out)
    np.testing.assert_array_equal(got[:n], R.patch_rows_ref(pages, img, ph, pw))
    assert (got[n] == sent).all() and (got[:n, R.PATCH_DIM:] == 0).all()
    v = got[:n, :R.PATCH_DIM].reshape(n, 3, R.PATCH_TP, -1)
    np.testing.assert_array_equal(v[:, :, 0], v[:, :, 1])


# --------------------------------------------------------------------------- decode_begin ---
@pytest.mark.parametrize("q_rows", R.KV_Q_ROWS)
def test_decode_begin(q_rows):
    """splits, cu_q, cu_kv for L = len + 1 at the edges of the rule, the 17th boundary and the empty ranges included; the other
    words of the state keep their values"""
    for L in R.KV_L:
        st = np.arange(-100, -100 + R.STATE_WORDS, dtype=np.int32)
        st[R.ST_LEN] = L - 1
        d = _dev(np.concatenate([st, np.array([77, 78], np.int32)]))
        op_gen_decode_begin(d, q_rows)
        got = d.cpu().numpy()
        np.testing.assert_array_equal(got[:R.STATE_WORDS], R.decode_begin_ref(st, q_rows), err_msg=f"L={L}")
        assert got[R.STATE_WORDS:].tolist() == [77, 78]


# ------------------------------------------------------------------------------ mark_seen ---
def test_mark_seen():
    V = 1000
    ids = np.array([-1, V, 0, 31, 32, V - 1, 5, 5, 31, 640, V + 31, -32, 2 ** 31 - 1], np.int32)
    before = np.zeros(33, np.uint32)
    before[[0, 3, 31, 32]] = [0x80000000, 0x00010000, 0x1, 0xDEADBEEF]          # bits that are already there stay; word 32 is not the set's
    seen = _dev(before.view(np.int32))
    op_gen_mark_seen(_dev(ids), len(ids), seen, V)
    got = seen.cpu().numpy().view(np.uint32)
    want = R.mark_seen_ref(before, ids.tolist(), V)
    np.testing.assert_array_equal(got, want)
    assert want[0] == 0x80000021 | 0x80000000 and want[1] == 0x1 and want[31] == 0x1 | (1 << (999 & 31)) and want[32] == 0xDEADBEEF


# ------------------------------------------------------------------------ sampler, greedy ---
@pytest.mark.parametrize("V", R.SAMPLE_V)
def test_sampler_temperature_zero(V):
    """exactly the argmax of the penalised logits, ties to the lowest id; seen ids 0, 31, 32, V - 1; the pick's bit is set
    afterwards and no other bit changes (V around 64 x 256: workgroups that see nothing / one element / a second round)"""
    words = (V + 31) // 32
    for name, (x, seen) in R.greedy_cases(V).items():
        lg = torch.full((V + 64,), 1.0e30, dtype=torch.float32, device=DEV)      # logits past V would win if they were read
        lg[:V] = _dev(x)
        before = np.concatenate([C.seen_words(seen[None])[0], np.array([0xDEADBEEF], np.uint32)])
        sd = _dev(before.view(np.int32))
        tok = op_gen_sample(lg, V, sd, penalty=R.SAMPLE_PENALTY, temperature=0.0, seed=5, step=3)
        want = R.greedy_ref(x, seen)
        assert tok == want, (V, name, tok, want)
        after = before.copy()
        after[want >> 5] |= np.uint32(1 << (want & 31))
        np.testing.assert_array_equal(sd.cpu().numpy().view(np.uint32), after, err_msg=f"{V} {name}")
        assert len(after) == words + 1


# -------------------------------------------------------------------- sampler, state form ---
def test_sampler_state_form():
    """step_from_state: the pick of the explicit-step call with the same index; advance: len, step and the three positions grow by
    one and `token` holds the pick; nothing else of the state changes"""
    V = 1000
    x, _ = C.sampling_logits()
    lg = _dev(x)
    fresh = lambda: torch.zeros(((V + 31) // 32,), dtype=torch.int32, device=DEV)  # noqa: E731
    picks = set()
    for step in (0, 1, 77, 4095):
        want = op_gen_sample(lg, V, fresh(), temperature=1.5, seed=99, step=step)
        picks.add(want)
        st = np.arange(500, 500 + R.STATE_WORDS, dtype=np.int32)
        st[R.ST_STEP] = step
        for advance in (False, True):
            d = _dev(st)
            seen = fresh()
            got = op_gen_sample(lg, V, seen, temperature=1.5, seed=99, step=step + 1000, state=d, step_from_state=True, advance=advance)
            assert got == want, (step, advance)
            after = st.copy()
            after[R.ST_TOKEN] = want
            if advance:
                after[[1, 2, 3, R.ST_LEN, R.ST_STEP]] += 1
            np.testing.assert_array_equal(d.cpu().numpy(), after)
            assert int(seen.cpu().numpy().view(np.uint32)[want >> 5]) == 1 << (want & 31)
        # a state that is only written: the explicit step rules, the token still lands in word 0
        d = _dev(st)
        assert op_gen_sample(lg, V, fresh(), temperature=1.5, seed=99, step=step, state=d) == want
        after = st.copy()
        after[R.ST_TOKEN] = want
        np.testing.assert_array_equal(d.cpu().numpy(), after)
    assert len(picks) > 1                                                        # (the step does select the noise)


# ------------------------------------------------------------------------- sampler, noise ---
@pytest.mark.parametrize("seed,step,idx", R.defective_triples())
def test_sampler_defective_draw(seed, step, idx):
    """(seed, step, idx) hashes to the 24-bit draw 0xFFFFFF, whose uniform the parent's map rounded to 1.0: infinite noise, and
    token idx was drawn whatever its logit.  One token D != idx at logit 30, everything else at 0, T = 1: the noise of every
    draw lies in [-2.86, 16.64], so D wins unless some noise_i - noise_D exceeds 30 — probability < 4096 e^-30.
    Fails with the parent's map (the pick is idx), passes with the shared one of csrc/gen_math.h."""
    V = 4096
    x, D = R.defective_logits(V, idx)
    seen = torch.zeros((V // 32,), dtype=torch.int32, device=DEV)
    assert op_gen_sample(_dev(x), V, seen, temperature=1.0, seed=seed, step=step) == D


# Chi-square with 7 degrees of freedom, critical value 40.5 at p = 1e-6; the restated sampler of tests/test_cpu_gen_ops_ref.py
# (the same hash, numpy's logarithms) gives 1.5 .. 9.5 against its own temperature and 700 .. 1100 against the other.
# First MI355X run, (own, other) per seed:
#   T = 0.7: (8.8, 731) (4.7, 799);  T = 1.5: (6.5, 1078) (8.5, 921)
# — the figures of test_chat_sampler_distribution: the same hash, the same seeds, the same eight logits, and no draw of these
# 16 384 is the defective one.
@pytest.mark.parametrize("T,other", [C.SAMPLE_TEMPS, C.SAMPLE_TEMPS[::-1]])
def test_sampler_distribution(T, other):
    """the generator's twin of test_chat_sampler_distribution: 4096 draws (step = 0..4095) per seed over V = 1000 logits,
    chat_ref.sampling_logits() with the 992 others lowered by R.SAMPLE_TAIL_DROP (this sampler has no top-k filter: see there).
    The counts pass a chi-square test against softmax(top 8 / T) and fail it against the other temperature's; nothing outside
    the planted top 8 is drawn."""
    x, ids = C.sampling_logits()
    x = x.copy()
    rest = np.ones(x.size, bool)
    rest[ids] = False
    x[rest] -= np.float32(R.SAMPLE_TAIL_DROP)
    tok, p = C.sampler_probs(x.astype(np.float64), C.SAMPLE_TOPK, T)
    _, p_other = C.sampler_probs(x.astype(np.float64), C.SAMPLE_TOPK, other)
    assert (C.SAMPLE_DRAWS * p).min() >= 40.0 and set(tok.tolist()) == set(ids.tolist())
    crit = C.chi2_critical(C.SAMPLE_TOPK - 1, 1e-6)
    index = {int(t): i for i, t in enumerate(tok)}
    lg = _dev(x)
    seen = torch.zeros(((x.size + 31) // 32,), dtype=torch.int32, device=DEV)
    for seed in C.SAMPLE_SEEDS:
        counts = np.zeros(len(tok), np.int64)
        for step in range(C.SAMPLE_DRAWS):
            t = op_gen_sample(lg, x.size, seen, penalty=1.0, temperature=T, seed=seed, step=step)
            assert t in index, (seed, step, t)                                   # never outside the top 8
            counts[index[t]] += 1
        own, cross = C.chi2_stat(counts, p), C.chi2_stat(counts, p_other)
        print(f"gen sampler T={T} seed={seed}: chi2 against own distribution {own:.1f}, against T={other} {cross:.1f}, critical {crit:.1f}")
        assert own < crit, (T, seed, counts.tolist())
        assert cross > crit, (T, seed, counts.tolist())


# ------------------------------------------------------------------------------- refusals ---
def test_gen_entries_refuse_bad_arguments():
    """NULL pointers and non-positive counts: VR_ERR_INVALID (1) on the host, nothing launched; hh > 64: refused by the launcher
    (VR_ERR_HIP = 2) before its kernel, the rows untouched"""
    from visrag_amd._lib import VisragHipError
    z16 = torch.zeros((4, 1024), dtype=torch.bfloat16, device=DEV)
    zf = torch.zeros((4, 1024), dtype=torch.float32, device=DEV)
    zi = torch.zeros((64,), dtype=torch.int32, device=DEV)
    inv = torch.zeros((64,), dtype=torch.float32, device=DEV)
    good = dict(T=1, H=2, KV=1, pos3=zi, pos_stride=4, sections=R.MROPE_SECTIONS, inv_freq=inv, q_out=z16, ldq=1024, k_cache=z16,
                v_cache=z16, ld_cache=1024, ld=1024, src=z16)
    for bad in (dict(src=None), dict(q_out=None), dict(pos3=None), dict(inv_freq=None), dict(k_cache=None), dict(v_cache=None), dict(T=0), dict(H=0),
                dict(KV=0), dict(T=-1), dict(src=None, parts=zf, n_parts=0)):
        with pytest.raises(VisragHipError, match="status 1"):
            op_gen_mrope_cache(**{**good, **bad})
    for bad in (dict(qkv=None), dict(pos_h=None), dict(pos_w=None), dict(freq=None), dict(T=0), dict(n_slots=0)):
        kw = {**dict(qkv=z16, ld=1024, T=2, n_slots=2, hh=16, pos_h=zi, pos_w=zi, sec_h=8, freq=inv), **bad}
        with pytest.raises(VisragHipError, match="status 1"):
            op_gen_rope2d(**kw)
    rows = torch.full((2, 1024), 3.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(VisragHipError, match="status 2"):
        op_gen_rope2d(rows, 1024, 2, 2, 65, zi, zi, 32, inv)
    assert (rows == 3.0).all()
    with pytest.raises(VisragHipError, match="status 1"):
        op_gen_rope2d(rows, 1024, -1, 2, 16, zi, zi, 8, inv)
    for kw in (dict(logits=None), dict(seen=None), dict(vocab=0), dict(vocab=-3), dict(step_from_state=True), dict(advance=True)):
        a = {**dict(logits=zf, vocab=100, seen=zi), **kw}
        with pytest.raises(VisragHipError, match="status 1"):
            op_gen_sample(a.pop("logits"), a.pop("vocab"), a.pop("seen"), **a)
    for a in ((None, 4, zi, 100), (zi, 4, None, 100), (zi, 0, zi, 100), (zi, 4, zi, 0)):
        with pytest.raises(VisragHipError, match="status 1"):
            op_gen_mark_seen(*a)
    for a in ((None, 1), (zi, 0)):
        with pytest.raises(VisragHipError, match="status 1"):
            op_gen_decode_begin(*a)
    page = torch.zeros((14, 14, 3), dtype=torch.uint8, device=DEV)
    for kind, kw in ((3, dict(src=zf, row_idx=zi, dim=8)), (0, dict(src=None, row_idx=zi, dim=8)), (1, dict(src=zf, row_idx=None, dim=8)),
                     (0, dict(src=zf, row_idx=zi, dim=0)), (2, dict(pages=[page], page_w=[14], img=zi, ph=zi, pw=None, patch=14, tp=2,
                                                                    mean=R.PATCH_MEAN, std=R.PATCH_STD)),
                     (2, dict(pages=[None], page_w=[14], img=zi, ph=zi, pw=zi, patch=14, tp=2, mean=R.PATCH_MEAN, std=R.PATCH_STD)),
                     (2, dict(pages=[page], page_w=[14], img=zi, ph=zi, pw=zi, patch=0, tp=2, mean=R.PATCH_MEAN, std=R.PATCH_STD)),
                     (2, dict(pages=[page], page_w=[14], img=zi, ph=zi, pw=zi, patch=14, tp=2, mean=None, std=R.PATCH_STD))):
        with pytest.raises(VisragHipError, match="status 1"):
            op_gen_rows(kind, 1, z16, 1024, **kw)
    with pytest.raises(VisragHipError, match="status 1"):
        op_gen_rows(0, 0, zf, 1024, src=zf, row_idx=zi, dim=8)
    with pytest.raises(VisragHipError, match="status 1"):
        op_gen_rows(0, 1, None, 1024, src=zf, row_idx=zi, dim=8)

