"""Plain numpy references (fp64, on the bf16-rounded inputs) of what the optional launch arguments of the GEMM and attention
kernels mean (GemmArgs / AttnArgs, csrc/kernels.h), and the inputs tests/test_gpu_launch_args.py runs them on.
tests/test_cpu_launch_args_ref.py pins these references to identities that need no kernel (split planes sum to the product,
ranges merged by their log-sum-exp equal attention over the union, a scatter followed by a gather is the plain product) and
checks the conditions the GPU tests rely on.  Nothing here needs a GPU or the built library."""
import math

import numpy as np

from tests.chat_ref import bf16_round

EPI_BF16, EPI_GELU, EPI_F32, EPI_RESID, EPI_SWIGLU, EPI_ROPE = range(6)
GEN_ATT_SPLITS = 16       # KV ranges of one decode step's attention (csrc/kernels.h)
LOG2E = 1.4426950408889634


def rand_bf16(shape, seed, scale=1.0):
    """normal values rounded to bf16 (float32 array): what the kernels read exactly"""
    return bf16_round((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def rand_f32(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


# ------------------------------------------------------------------------------- GEMM ---
def gemm_acc(A, W, bias=None, rowbias=None, period=0, cols=0, col_scale=1.0, col_scale_n=0, k_lo=0, k_hi=None):
    """(A W^T over K columns [k_lo, k_hi) + bias + rowbias[m % period][n] for n < cols) * col_scale for n < col_scale_n"""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    acc = A[:, k_lo:k_hi] @ W[:, k_lo:k_hi].T
    if bias is not None:
        acc = acc + np.asarray(bias, np.float64)[None, :]
    if rowbias is not None:
        rb = np.asarray(rowbias, np.float64)
        acc[:, :cols] += rb[np.arange(A.shape[0]) % period][:, :cols]
    if col_scale_n:
        acc[:, :col_scale_n] *= np.float64(np.float32(col_scale))
    return acc


def gelu(x):
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


def interleave16(g, u):
    """EPI_SWIGLU's weight / bias layout: rows in blocks of [16 gate | 16 up]"""
    I = g.shape[0]
    return np.stack([g.reshape(I // 16, 16, *g.shape[1:]), u.reshape(I // 16, 16, *u.shape[1:])], axis=1).reshape(2 * I, *g.shape[1:])


def swiglu_of_interleaved(acc):
    """acc [M][N] over interleaved W rows -> silu(gate) * up [M][N / 2]"""
    M, N = acc.shape
    b = acc.reshape(M, N // 32, 2, 16)
    g, u = b[:, :, 0, :].reshape(M, N // 2), b[:, :, 1, :].reshape(M, N // 2)
    return g / (1.0 + np.exp(-g)) * u


def rope_table(max_pos):
    """f32 [max_pos][32 cos | 32 sin] of head_dim 64"""
    inv = 1.0 / (10000.0 ** (np.arange(0, 64, 2, dtype=np.float64) / 64))
    fr = np.outer(np.arange(max_pos, dtype=np.float64), inv)
    return np.concatenate([np.cos(fr), np.sin(fr)], axis=1).astype(np.float32)


def rope(acc, pos, table, rope_cols):
    out = acc.copy()
    t = np.asarray(table, np.float64)[pos]
    c, s = t[:, :32], t[:, 32:]
    for h in range(rope_cols // 64):
        x1, x2 = acc[:, h * 64:h * 64 + 32], acc[:, h * 64 + 32:h * 64 + 64]
        out[:, h * 64:h * 64 + 32] = x1 * c - x2 * s
        out[:, h * 64 + 32:h * 64 + 64] = x2 * c + x1 * s
    return out


def row_map(M, rows_out, seed):
    """output row of input row m: a random injection into [0, rows_out), every eighth row dropped (-1)"""
    rng = np.random.default_rng(seed)
    rm = rng.permutation(rows_out)[:M].astype(np.int32)
    rm[3::8] = -1
    return rm


def scatter_rows(vals, rowmap, rows_out):
    """(out [rows_out][N] with row rowmap[m] = vals[m], written [rows_out] bool); rows nobody maps to stay NaN / False"""
    out = np.full((rows_out, vals.shape[1]), np.nan)
    written = np.zeros(rows_out, bool)
    keep = rowmap >= 0
    out[rowmap[keep]] = vals[keep]
    written[rowmap[keep]] = True
    return out, written


def split_planes(A, W, ksplit, bias=None):
    """[ksplit][M][N]: split s covers the K columns [s, s + 1) * K / ksplit; the bias rides with plane 0"""
    K = A.shape[1]
    assert K % ksplit == 0
    Ks = K // ksplit
    return np.stack([gemm_acc(A, W, bias if s == 0 else None, k_lo=s * Ks, k_hi=(s + 1) * Ks) for s in range(ksplit)])


def rows_left(count, M, tile=256):
    """A device-side row count: (rows that must hold the product, first row that must be untouched); between them: unspecified"""
    count = max(0, count)
    return min(count, M), (count + tile - 1) // tile * tile


# -------------------------------------------------------------------------- attention ---
def attn_range(q, k, v, scale, causal_from=None):
    """q [nq][hd] against keys k, v [L][hd] -> (out [nq][hd], lse [nq] = log2 sum_k exp(scale * s_k)); causal_from = position
    of query 0 among the keys (query i sees keys <= causal_from + i)"""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    s = (q @ k.T) * scale
    if causal_from is not None:
        s = np.where(np.arange(k.shape[0])[None, :] <= causal_from + np.arange(q.shape[0])[:, None], s, -np.inf)
    m = s.max(axis=1, keepdims=True)
    p = np.exp(s - m)
    den = p.sum(axis=1, keepdims=True)
    return (p @ v) / den, (m[:, 0] + np.log(den[:, 0])) * LOG2E


def merge_ranges(outs, lses):
    """Ranges merged by their lse: sum_s 2^lse_s out_s / sum_s 2^lse_s.  outs [S][...][hd], lses [S][...]; an EMPTY range is
    None in both lists (it has written nothing) and takes no part."""
    live = [i for i, l in enumerate(lses) if l is not None]
    L = np.stack([np.asarray(lses[i], np.float64) for i in live])
    O = np.stack([np.asarray(outs[i], np.float64) for i in live])
    w = np.exp2(L - L.max(axis=0, keepdims=True))
    return (w[..., None] * O).sum(axis=0) / w.sum(axis=0)[..., None]


# ---- the generator's decode form: the `group` query heads of a KV head as the ROWS of one tile, KV ranges as batch items
KV_HEADS, HD = 2, 128
CACHE_ROWS = 333
RANGE_LENS = [1, 63, 64, 65, 20, 30, 10, 5, 40, 15, 7, 8, 5, 0, 0, 0]     # 13 ranges that tile the 333 rows, then empty ones
KEY_GAIN = 4.0            # keys this much larger than unit normals: a few keys carry a row (see decode_case)


def decode_case(group, seed, n_rows=1, rows=CACHE_ROWS):
    """q bf16 values [n_rows][KV * group][128] (query head hq = hkv * group + g), caches k, v [n_rows][rows][KV * 128].  With unit
    keys the softmax over hundreds of keys is nearly flat and the output a mean of ~N(0, 1) values, |out| ~ 0.04: the
    attention tolerance atol = 2e-2 would accept almost anything.  Keys of size KEY_GAIN make the logits ~N(0, 16): a handful
    of keys carries each row and the output is of the size of v itself."""
    H = KV_HEADS * group
    q = rand_bf16((n_rows, H, HD), seed)
    k = rand_bf16((n_rows, rows, KV_HEADS * HD), seed + 1, KEY_GAIN)
    v = rand_bf16((n_rows, rows, KV_HEADS * HD), seed + 2)
    return q, k, v


def range_bounds(lens):
    lo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return lo[:-1].copy(), lo[1:].copy()


def decode_ref(q, k, v, group, lo, hi):
    """One sequence: per-range partial attention in SkinnyCombine's layout — out [S][group][KV][128], lse [S][group][KV], None for
    an empty range — and the attention over the union of the ranges [H = KV * group][128]."""
    scale = HD ** -0.5
    outs, lses = [], []
    for a, b in zip(lo, hi):
        if b <= a:
            outs.append(None); lses.append(None)
            continue
        o = np.zeros((group, KV_HEADS, HD)); l = np.zeros((group, KV_HEADS))
        for hkv in range(KV_HEADS):
            qq = q[hkv * group:(hkv + 1) * group]
            o[:, hkv], l[:, hkv] = attn_range(qq, k[a:b, hkv * HD:(hkv + 1) * HD], v[a:b, hkv * HD:(hkv + 1) * HD], scale)
        outs.append(o); lses.append(l)
    rows = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]).astype(np.int64)
    whole = np.zeros((KV_HEADS * group, HD))
    for hkv in range(KV_HEADS):
        whole[hkv * group:(hkv + 1) * group] = attn_range(q[hkv * group:(hkv + 1) * group], k[rows, hkv * HD:(hkv + 1) * HD],
                                                          v[rows, hkv * HD:(hkv + 1) * HD], scale)[0]
    return outs, lses, whole


def merged_to_heads(merged):
    """[group][KV][128] (the partial rows' layout) -> [H = KV * group][128] in query-head order hq = hkv * group + g"""
    return np.transpose(merged, (1, 0, 2)).reshape(-1, merged.shape[-1])


def batch_ranges(lens_per_row, rows=CACHE_ROWS):
    """vg_decode_batch's items: row r of the step owns the ranges [16 r, 16 r + 16), its keys live in cache r (rows
    [r * rows, (r + 1) * rows) of one buffer).  Returns kv_lo, kv_hi [n * 16] (cache rows), counts [n] = non-empty ranges."""
    lo_all, hi_all, counts = [], [], []
    for r, lens in enumerate(lens_per_row):
        lens = list(lens) + [0] * (GEN_ATT_SPLITS - len(lens))
        lo, hi = range_bounds(lens)
        lo_all.append(lo + r * rows); hi_all.append(hi + r * rows)
        counts.append(sum(1 for x in lens if x > 0))
    return np.concatenate(lo_all).astype(np.int32), np.concatenate(hi_all).astype(np.int32), counts


BATCH_LENS = [RANGE_LENS[:13], [64, 64, 64, 64, 64, 13], [200]]       # 13, 6 and 1 ranges: three different caches
