"""The references of tests/launch_args_ref.py pinned to identities that need no kernel, and the conditions the inputs of
tests/test_gpu_launch_args.py have to meet for its tolerances to mean something.  No GPU, no library."""
import numpy as np
import pytest

from tests import launch_args_ref as R


def test_split_planes_sum_to_the_full_product():
    A, W, b = R.rand_bf16((37, 384), 1), R.rand_bf16((128, 384), 2, 0.1), R.rand_f32((128,), 3)
    full = R.gemm_acc(A, W, b)
    for ks in (1, 2, 3, 6):
        planes = R.split_planes(A, W, ks, b)
        assert planes.shape == (ks, 37, 128)
        np.testing.assert_allclose(planes.sum(axis=0), full, rtol=0, atol=1e-11)
        # the bias is on plane 0 only: every other plane is a pure product
        for s in range(1, ks):
            np.testing.assert_allclose(planes[s], R.gemm_acc(A, W, k_lo=s * 384 // ks, k_hi=(s + 1) * 384 // ks), rtol=0, atol=0)


def test_row_map_with_drops_then_gather_is_the_plain_product():
    M, rows_out = 300, 400
    rm = R.row_map(M, rows_out, 5)
    kept = rm >= 0
    # an injection: no output row is written twice; one row in eight is dropped, at most a quarter (the cap the GPU test states)
    assert len(set(rm[kept].tolist())) == kept.sum() and rm[kept].max() < rows_out
    assert (~kept).sum() == len(range(3, M, 8))
    assert 0 < (~kept).mean() <= 0.25
    A, W = R.rand_bf16((M, 128), 6), R.rand_bf16((256, 128), 7, 0.1)
    acc = R.gemm_acc(A, W)
    out, written = R.scatter_rows(acc, rm, rows_out)
    assert written.sum() == kept.sum() and np.isnan(out[~written]).all()
    np.testing.assert_array_equal(out[rm[kept]], acc[kept])
    # the map moves rows: a kernel that ignored it would be caught (almost no row maps to itself)
    assert (rm[kept] == np.arange(M)[kept]).mean() < 0.05


def test_row_bias_and_column_scale_touch_only_their_columns():
    A, W, b = R.rand_bf16((600, 64), 8), R.rand_bf16((256, 64), 9, 0.1), R.rand_f32((256,), 10)
    rb = R.rand_f32((100, 128), 11)
    plain = R.gemm_acc(A, W, b)
    got = R.gemm_acc(A, W, b, rowbias=rb, period=100, cols=96)
    np.testing.assert_array_equal(got[:, 96:], plain[:, 96:])
    np.testing.assert_allclose(got[:, :96] - plain[:, :96], rb[np.arange(600) % 100][:, :96].astype(np.float64), rtol=0, atol=1e-12)
    # rows a period apart get the same bias row, neighbours do not
    assert np.abs((got - plain)[0] - (got - plain)[100]).max() < 1e-12 and np.abs((got - plain)[0] - (got - plain)[1]).max() > 0.1
    sc = R.gemm_acc(A, W, b, rowbias=rb, period=100, cols=96, col_scale=0.17, col_scale_n=128)
    np.testing.assert_array_equal(sc[:, 128:], got[:, 128:])
    np.testing.assert_allclose(sc[:, :128], got[:, :128] * np.float64(np.float32(0.17)), rtol=1e-15, atol=0)


def test_rows_left_by_a_device_side_count():
    assert R.rows_left(0, 700) == (0, 0)
    assert R.rows_left(1, 700) == (1, 256)
    assert R.rows_left(256, 700) == (256, 256)
    assert R.rows_left(257, 700) == (257, 512)
    assert R.rows_left(700, 700) == (700, 768)
    assert R.rows_left(-5, 700) == (0, 0)


def test_swiglu_and_rope_helpers_match_their_definitions():
    g, u = R.rand_f32((64, 5), 12), R.rand_f32((64, 5), 13)
    il = R.interleave16(g, u)
    assert np.array_equal(il[:16], g[:16]) and np.array_equal(il[16:32], u[:16]) and np.array_equal(il[32:48], g[16:32])
    acc = np.asarray(il.T, np.float64)                                   # [5][128] "over interleaved rows"
    np.testing.assert_allclose(R.swiglu_of_interleaved(acc), (g / (1 + np.exp(-g.astype(np.float64))) * u).T, rtol=1e-12)
    tab = R.rope_table(50)
    x = np.asarray(R.rand_f32((7, 192), 14), np.float64)
    pos = np.arange(7) * 3
    y = R.rope(x, pos, tab, 128)
    np.testing.assert_array_equal(y[:, 128:], x[:, 128:])                # columns past rope_cols are copied
    np.testing.assert_allclose((y[:, :128] ** 2).sum(1), (x[:, :128] ** 2).sum(1), rtol=1e-6)    # a rotation
    np.testing.assert_allclose(y[0], x[0], rtol=0, atol=1e-12)           # position 0: the identity


@pytest.mark.parametrize("group", [1, 4, 7])
def test_ranges_merged_by_lse_equal_attention_over_their_union(group):
    q, k, v = R.decode_case(group, 100 + group)
    lo, hi = R.range_bounds(R.RANGE_LENS)
    # the ranges tile the cache, their lengths cross the 64-key tile both ways, some are empty — and fewer than 16 are real
    assert hi[-1] == R.CACHE_ROWS and len(R.RANGE_LENS) == R.GEN_ATT_SPLITS
    assert {0, 1, 63, 64, 65} <= set(R.RANGE_LENS)
    n_real = sum(1 for x in R.RANGE_LENS if x > 0)
    assert n_real < R.GEN_ATT_SPLITS and all(x > 0 for x in R.RANGE_LENS[:n_real])
    outs, lses, whole = R.decode_ref(q[0], k[0], v[0], group, lo, hi)
    assert [o is None for o in outs] == [x == 0 for x in R.RANGE_LENS]
    merged = R.merged_to_heads(R.merge_ranges(outs, lses))
    np.testing.assert_allclose(merged, whole, rtol=1e-11, atol=1e-12)
    # a range of one key returns that key's value row and lse = log2 exp(scale * s)
    np.testing.assert_allclose(outs[0][0, 1], v[0, 0, R.HD:2 * R.HD], rtol=0, atol=1e-12)
    s00 = float(np.dot(q[0, 0].astype(np.float64), k[0, 0, :R.HD].astype(np.float64))) * R.HD ** -0.5
    assert abs(lses[0][0, 0] - s00 * R.LOG2E) < 1e-10
    # the merge is the thing under test there: leaving a range out, or weighting all alike, is far outside the tolerance
    flat = R.merged_to_heads(np.mean([o for o in outs if o is not None], axis=0))
    assert np.abs(flat - whole).max() > 0.2
    # magnitude: with atol = 2e-2 the outputs must not be ~0 (launch_args_ref.decode_case)
    assert np.median(np.abs(whole)) >= 0.2
    assert min(np.median(np.abs(o)) for o in outs if o is not None) >= 0.2


def test_batched_ranges_point_into_different_caches():
    lo, hi, counts = R.batch_ranges(R.BATCH_LENS)
    assert counts == [13, 6, 1] and len(lo) == len(hi) == 3 * R.GEN_ATT_SPLITS
    for r in range(3):
        a, b = lo[r * 16:(r + 1) * 16], hi[r * 16:(r + 1) * 16]
        assert a[0] == r * R.CACHE_ROWS and b.max() <= (r + 1) * R.CACHE_ROWS and (b >= a).all()
        assert ((b - a) > 0).sum() == counts[r] and ((b - a)[:counts[r]] > 0).all()
    q, k, v = R.decode_case(4, 200, n_rows=3)
    for r in range(3):
        a, b = lo[r * 16:(r + 1) * 16] - r * R.CACHE_ROWS, hi[r * 16:(r + 1) * 16] - r * R.CACHE_ROWS
        outs, lses, whole = R.decode_ref(q[r], k[r], v[r], 4, a, b)
        np.testing.assert_allclose(R.merged_to_heads(R.merge_ranges(outs, lses)), whole, rtol=1e-11, atol=1e-12)
        assert np.median(np.abs(whole)) >= 0.2


def test_causal_grouped_reference_matches_a_per_head_loop():
    q, k, v = R.rand_bf16((5, 16), 20), R.rand_bf16((5, 16), 21), R.rand_bf16((5, 16), 22)
    out, lse = R.attn_range(q, k, v, 0.25, causal_from=0)
    for i in range(5):
        o, l = R.attn_range(q[i:i + 1], k[:i + 1], v[:i + 1], 0.25)
        np.testing.assert_allclose(out[i], o[0], rtol=1e-12, atol=1e-13)
        assert abs(lse[i] - l[0]) < 1e-12
