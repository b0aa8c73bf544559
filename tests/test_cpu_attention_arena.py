"""The guarded arena of tests/attention_arena.py, on the host: its masks are what they claim to be, and the comparison
tests/test_gpu_attention_isolation.py makes CAN fail — at every shape used there, a reference that is wrong the way a kernel
could be (one key past a range, the neighbouring head's columns, a causal limit off by one) leaves the tolerance."""
import numpy as np
import pytest

from tests import attention_arena as A
from tests import launch_args_ref as R

CASES = A.cases()
IDS = [c.name for c in CASES]


def _moved(got, ref):
    """some output cell of `ref` is missed by more than the GPU test's tolerance (a NaN / inf in `got` counts)"""
    return A.worst_ratio(got, ref) > 1.0


def test_the_case_list_is_the_one_the_routes_need():
    names = set(IDS)
    for hd in (64, 72, 80):
        for lens in ("64_1_63", "65_64", "128_127", "129_65_1"):
            assert f"tiled{hd}_{lens}" in names
        assert f"tiled{hd}_129_65_1_causal" in names
    assert {"tiled64_64_1_63_causal", "tiled64_65_64_causal", "tiled64_128_127_causal"} <= names
    assert {"tiled72_223", "tiled72_257_30", "hd128_resampler", "hd128_segments", "small", "small_causal", "72w_224",
            "72w_256_224_1", "72w_448_33", "decode_shared_q", "decode_batched"} <= names
    for c in CASES:
        assert c.cu_q[0] == A.FRONT and c.cu_kv.min() == A.FRONT, c.name                     # no cu starts at 0
        assert c.ld % 8 == 0 and c.q_col % 8 == 0 and c.k_col % 8 == 0 and c.v_col % 8 == 0 and c.ldo % 4 == 0
        assert 0 < c.v_col - c.k_col < c.ld and c.v_col - c.k_col >= c.Wkv                  # attention72w_ok's "same rows"
        assert c.max_q == int(np.diff(c.cu_q).max())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_masks_partition_the_arena_and_views_alias_their_data(c):
    a = A.arena_of(c.name)
    assert a.bits.shape == (A.FRONT + c.rows + A.BACK, c.ld)
    # data and guard partition the arena; q, k and v cells are disjoint (build asserts it) and lie in their own columns
    assert (a.data ^ a.guard).all() and not (a.data & a.guard).any()
    assert not a.data[:A.FRONT].any() and not a.data[A.FRONT + c.rows:].any()
    cols = np.arange(c.ld)
    for m, lo, w in ((a.q_mask, c.q_col, c.Wq), (a.k_mask, c.k_col, c.Wkv), (a.v_mask, c.v_col, c.Wkv)):
        assert m.any() and not m[:, (cols < lo) | (cols >= lo + w)].any()
    assert not (a.finite_only & a.data).any() and a.finite_only.any() == (c.route == A.W72)
    # the guard cells of the clean fill are zero, every fill leaves the data bits alone and puts its pattern everywhere else
    clean = a.filled("clean")
    assert np.array_equal(clean, a.bits) and not clean[a.guard].any()
    for fill in ("nan", "huge"):
        f = a.filled(fill)
        assert np.array_equal(f[a.data], a.bits[a.data])
        g = f[a.guard & ~a.finite_only]
        assert set(np.unique(g)) == set(A.FILL_BITS[fill])
        v = A.from_bits(g)
        assert np.isnan(v).all() if fill == "nan" else (np.isfinite(v).all() and (np.abs(v) > 3e38).all())
        assert np.isfinite(A.from_bits(f[a.finite_only])).all()
    # the views a launch gets alias exactly their data cells: what plain slices of them hold is what the addressing reaches
    marked = a.filled("clean").copy()
    qv, kv, vv = a.views(marked)
    want = np.zeros_like(a.bits, bool)
    wq, wk, wv = a.views(want)
    for b in range(c.B):
        if not c.live(b):
            continue
        lo, hi = c.kv_range(b)
        wk[lo:hi, :] = True
        wv[lo:hi, :] = True
        nq = c.cu_q[b + 1] - c.cu_q[b]
        if c.q_rows_per_head:                                   # the decode form: heads as rows, `group` rows per KV head
            first = c.q_in_rows[b] if c.q_in_rows is not None else 0
            wq[first:first + c.heads * c.q_rows_per_head, :] = True
            assert nq == c.q_rows_per_head
        elif c.q_shared:
            wq[:nq, :] = True
        else:
            wq[c.cu_q[b]:c.cu_q[b + 1], :] = True
    assert np.array_equal(want, a.data)
    assert qv.base is not None and kv.base is not None and vv.base is not None                # views, not copies
    # the sentinels and the cells a launch must write
    out, lse = a.out_sentinels()
    assert out.shape == (c.out_rows, c.Wo + 8) and (A.from_bits(out) == 7.0).all() and (lse == -77.25).all()
    assert not a.out_mask[:, c.Wo:].any() and not a.out_mask[:A.FRONT].any() and not a.out_mask[c.out_rows - A.BACK:].any()
    assert a.lse_mask.any() == c.lse


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_is_attn_range_on_slices_and_of_the_size_of_v(c):
    """the reference built from flat addresses is launch_args_ref.attn_range on plain slices of the views; no output near 0"""
    a = A.arena_of(c.name)
    ref, lse = A.reference_of(c.name)
    assert np.array_equal(~np.isnan(ref), a.out_mask[:, :c.Wo]) and np.array_equal(~np.isnan(lse), a.out_mask[:, ::c.hd][:, :c.heads])
    assert np.median(np.abs(ref[a.out_mask[:, :c.Wo]])) > 0.1
    if c.q_rows_per_head or c.q_shared:
        return
    qv, kv, vv = (A.from_bits(x) for x in a.views(a.bits))
    b, h = c.B - 1, c.heads - 1
    lo, hi = c.kv_range(b)
    rows = slice(c.cu_q[b], c.cu_q[b + 1])
    o, _ = R.attn_range(qv[rows, h * c.hd:(h + 1) * c.hd], kv[lo:hi, h * c.hd:(h + 1) * c.hd], vv[lo:hi, h * c.hd:(h + 1) * c.hd], c.scale,
                        causal_from=0 if c.causal else None)
    np.testing.assert_array_equal(ref[rows, h * c.hd:(h + 1) * c.hd], o)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_a_wrong_kernel_would_leave_the_tolerance(c):
    a = A.arena_of(c.name)
    ref, lse = A.reference_of(c.name)
    # one key past a range: the next item's first row where ranges touch, a guard row otherwise — with hostile guards (the GPU
    # test's nan run) and, where the case has ranges that touch, by value alone with the guards zero.  (A case of ONE long
    # sequence, [223] and [224]: a zero key next to 223 real ones of size KEY_GAIN weighs ~e^-10 — only the hostile fills show
    # it, which is why the GPU test has them.  Causal self-attention: key L is behind every query's own limit — there the
    # off-by-one below is the test.)
    for fill in () if c.causal else ("nan", "clean") if c.B > 1 else ("nan", "huge"):
        got, got_lse = A.reference(c, a.filled(fill), extra_keys=1)
        assert _moved(got, ref), fill
        if c.lse:
            assert A.worst_ratio(got_lse, lse, rtol=0, atol=A.LSE_ATOL) > 1.0, fill
    # the neighbouring head's columns: one 16-byte chunk further (the last head reaches the guard columns behind k and v)
    got, _ = A.reference(c, a.filled("clean"), col_shift=8)
    assert _moved(got, ref)
    got, _ = A.reference(c, a.filled("nan"), col_shift=8)
    assert _moved(got[:, (c.heads - 1) * c.hd:], ref[:, (c.heads - 1) * c.hd:])
    # a causal limit off by one, either way
    if c.causal:
        for shift in (1, -1):
            got, _ = A.reference(c, a.filled("clean"), causal_shift=shift)
            assert _moved(got, ref), shift
