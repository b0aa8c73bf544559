"""Plain numpy restatements of the fp32 text path's kernels (csrc/hp_text.hip) and of the encode glue kernels (csrc/misc.hip,
csrc/patch_embed.hip, csrc/norm.hip), the case tables tests/test_gpu_text_ops.py runs them on, and the bars it holds the
kernels to.  Every operation takes a `dtype`: np.float64 is the reference, np.float32 the "float32 restatement" — the same
formulas, a plain softmax, numpy's own summation order — whose distance from the reference is the yardstick of the bars that are
stated as a multiple of it.  tests/test_cpu_text_ops_ref.py pins all of this against oracle/visrag_ret_oracle.py, torch's
conv2d and torch's bf16 rounding.  Nothing here needs a GPU or the built library."""
import numpy as np

from tests.launch_args_ref import rope_table  # noqa: F401  (f32 [pos][32 cos | 32 sin])

F32_ULP = 2.0 ** -23
TINY = 2.0 ** -126          # smallest normal float32 / bf16


# ------------------------------------------------------------------------------ bf16 ---
def bf16_bits(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even; NaN stays NaN (quiet)"""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, np.float32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r).reshape(np.shape(x))


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_to_f32(bf16_bits(x)).reshape(np.shape(x))


def split_hi_lo(v):
    """the kernels' split: hi = bf16(v), lo = bf16(v - hi); v - hi is exact in float32"""
    v = np.asarray(v, np.float32)
    hi = bf16_round(v)
    with np.errstate(invalid="ignore"):
        lo = bf16_round((v - hi).astype(np.float32))
    return hi, lo


def ulp_bf16(x):
    """2^(floor(log2|x|) - 7): the spacing of bf16 at x"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), TINY)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def ulp_f32(x):
    a = np.maximum(np.abs(np.asarray(x, np.float64)), TINY)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def rng(seed):
    return np.random.default_rng(seed)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- the split bars: checks (a) and (b) of rmsnorm_split and swiglu_split ---------------
# (a) |hi + lo - ref| <= 1.25 * 2^-16 |ref|: the split alone is bounded by 2^-16 (bf16's unit roundoff 2^-8, applied twice), the fp32
#     evaluation adds about 2^-20; the float32 restatement stays below 7.7e-6 (~ 2^-17) at every width of the table below
#     (test_cpu_text_ops_ref.py asserts it).  A missing or mis-signed lo sits at 2^-8 .. 2^-9.
# (b) |lo| <= 2^-8 |hi|: hi is the ROUNDING of the value, not its truncation (a truncated hi leaves a lo of up to 2^-7 |hi|).
SPLIT_REL = 1.25 * 2.0 ** -16
LO_REL = 2.0 ** -8
# below 2^-118 bf16 has fewer than 8 significant bits left above its fixed subnormal spacing 2^-133: (b) is asked of normal his
# with room for a full lo only
LO_REL_FLOOR = 2.0 ** -118


def split_errors(hi, lo, ref, floor=0.0):
    """(err, bar, ratio): |hi + lo - ref| and its bar max(SPLIT_REL |ref|, floor) per element — (a) is err <= bar — and the
    largest |lo| / (LO_REL |hi|) over the his of at least LO_REL_FLOOR — (b) is ratio <= 1"""
    hi, lo, ref = np.asarray(hi, np.float64), np.asarray(lo, np.float64), np.asarray(ref, np.float64)
    bar = np.maximum(SPLIT_REL * np.abs(ref), floor)
    err = np.abs(hi + lo - ref)
    big = np.abs(hi) >= LO_REL_FLOOR
    ratio = float(np.max(np.abs(lo[big]) / (LO_REL * np.abs(hi[big])), initial=0.0))
    return err, bar, ratio


# ------------------------------------------------------------------------ rmsnorm_split ---
RMS_EPS = 1e-5
RMSNORM_ROWS = (1, 4, 5, 7)                     # one wave per row, four rows per workgroup: partial last workgroups
RMSNORM_DIMS = (64, 256, 260, 2304, 2560)       # nv = 16, 64 (one full pass), 65 (one lane into the second), the encoder's, the limit
RMSNORM_REFUSED = (2564, 66)                    # past the ten registers; dim % 4


def rms_norm(x, w, eps, dtype=np.float64):
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    var = np.mean(x * x, axis=-1, keepdims=True, dtype=dtype)
    return (x * (dtype(1.0) / np.sqrt(var + dtype(eps))) * w).astype(dtype)


def rmsnorm_inputs(dim, seed=0):
    """x f32 [7][dim]: row 1 all zero, row 2 one element 3e4 among unit-variance ones; w f32 [dim] around 1"""
    g = rng(100 + dim + seed)
    x = (g.standard_normal((7, dim)) * 1.5).astype(np.float32)
    x[1] = 0.0
    x[2, (dim * 2) // 3] = 3.0e4
    w = (1.0 + 0.3 * g.standard_normal(dim)).astype(np.float32)
    return frozen(x, w)


# --------------------------------------------------------------------------------- rope ---
ROPE_E = (64, 320)                 # rope_cols / 2 = 64 and 320 pairs: the 256-thread loop runs once and twice
ROPE_POS = (0, 1, 2, 0, 7)         # packed sequences restart
ROPE_PAD = 8
ROPE_ULPS = 4.0


def rope_inputs(E, seed=0):
    T, ld = len(ROPE_POS), 3 * E + ROPE_PAD
    qkv = rng(200 + E + seed).standard_normal((T, ld)).astype(np.float32)
    return frozen(qkv, np.array(ROPE_POS, np.int32), rope_table(8))


def rope_ref(qkv, pos, table, rope_cols):
    """float64 rotation of the heads (64 columns, pairs (c, c + 32)) below rope_cols by the SAME fp32 table entries.  Returns
    (ref, mag): mag is the larger of |ref| and its two products — the magnitude the roundings of the two products and the sum
    happen at (the products' roundings do not shrink when the sum cancels)."""
    x = np.asarray(qkv, np.float64)
    ref, mag = x.copy(), np.abs(x)
    t = np.asarray(table, np.float64)[np.asarray(pos)]
    c, s = t[:, :32], t[:, 32:]
    for h in range(rope_cols // 64):
        a, b = x[:, h * 64:h * 64 + 32], x[:, h * 64 + 32:h * 64 + 64]
        ref[:, h * 64:h * 64 + 32] = a * c - b * s
        ref[:, h * 64 + 32:h * 64 + 64] = b * c + a * s
        m = np.maximum(np.abs(a * c), np.abs(b * s))
        m2 = np.maximum(np.abs(b * c), np.abs(a * s))
        mag[:, h * 64:h * 64 + 32] = np.maximum(m, np.abs(ref[:, h * 64:h * 64 + 32]))
        mag[:, h * 64 + 32:h * 64 + 64] = np.maximum(m2, np.abs(ref[:, h * 64 + 32:h * 64 + 64]))
    return ref, mag


# ---------------------------------------------------------------------------- attention ---
ATTN_HEADS = (1, 3)
ATTN_SEQS = ((1,), (64,), (65,), (63, 1, 66), (129,), (200, 3))     # the 64-key rounds: one, one + 1, two + 1, three + 8
ATTN_QK_GAIN = (1.0, 6.0)
ATTN_PAD = 4
ATTN_SCORE_CASES = ("dominant_second_group", "dominant_third_group", "rising", "all_below_minus_60", "huge_first")
ATTN_BAR_FACTOR = 8.0      # the kernel sums in a 64-lane tree and rescales every 64 keys, the restatement does neither
# Largest float32-restatement errors (max |f32 - f64| over a case's output; test_cpu_text_ops_ref.py prints and bounds them):
#   unit-variance q / k: 2.7e-7 .. 1.2e-6 (0 for the single token)      six-fold q / k: 5.9e-6 .. 3.5e-5
#   score cases: 1.3e-6 .. 3.1e-6, all_below_minus_60 (scores around -290) 7.4e-5
# bf16 operands would give 6e-3 .. 0.2.


def attn_inputs(heads, lens, gain=1.0, seed=0):
    """qkv f32 [T][3 E + 4]: q | k | v | pad; q and k scaled by `gain`"""
    E, T = 64 * heads, int(sum(lens))
    qkv = rng(300 + 7 * heads + 13 * T + seed).standard_normal((T, 3 * E + ATTN_PAD)).astype(np.float32)
    qkv[:, :2 * E] *= np.float32(gain)
    return frozen(qkv)


def attn_score_case(case, seed=0):
    """one sequence of 200 tokens, one head (four rounds of 64 keys for the last rows)"""
    L = 200
    g = rng(350 + seed)
    q, k, v = (g.standard_normal((L, 64)).astype(np.float32) for _ in range(3))
    qm = q.mean(0, keepdims=True)
    if case == "dominant_second_group":
        for row, key, gain in ((100, 70, 8.0), (199, 127, 12.0), (80, 64, 6.0)):
            k[key] = q[row] * gain
    elif case == "dominant_third_group":
        for row, key, gain in ((150, 130, 8.0), (199, 191, 12.0), (128, 128, 9.0)):
            k[key] = q[row] * gain
    elif case == "rising":
        k = k * np.linspace(0.2, 6.0, L, dtype=np.float32)[:, None] + qm * np.linspace(0.0, 3.0, L, dtype=np.float32)[:, None]
    elif case == "all_below_minus_60":
        q = q * 0.05 + 6.0
        k = k * 0.05 - 6.0          # q . k / 8 ~ -64 * 36 / 8 = -288
    elif case == "huge_first":
        q = q + 1.0
        k[0] = 4.0                  # q . k_0 / 8 ~ 32, every later score ~ N(0, 2)
    else:
        raise ValueError(case)
    qkv = np.concatenate([q, k, v, np.zeros((L, ATTN_PAD), np.float32)], axis=1).astype(np.float32)
    return frozen(qkv)


def attn_ref(qkv, heads, lens, scale, dtype=np.float64):
    """causal softmax(q k^T scale) v per (sequence, head), plain softmax; out [T][E]"""
    E = 64 * heads
    x = np.asarray(qkv, dtype)
    out = np.zeros((x.shape[0], E), dtype)
    t0 = 0
    for L in lens:
        for h in range(heads):
            q, k, v = (x[t0:t0 + L, o + h * 64:o + (h + 1) * 64] for o in (0, E, 2 * E))
            s = (q @ k.T) * dtype(scale)
            s = np.where(np.tril(np.ones((L, L), bool)), s, dtype(-np.inf))
            p = np.exp(s - s.max(axis=-1, keepdims=True))
            p = p / p.sum(axis=-1, keepdims=True, dtype=dtype)
            out[t0:t0 + L, h * 64:(h + 1) * 64] = p @ v
        t0 += L
    return out


def restatement_bar(ref64, ref32, factor=ATTN_BAR_FACTOR):
    """(bar, float32 error): factor x the largest absolute error of the float32 restatement"""
    e32 = float(np.max(np.abs(np.asarray(ref32, np.float64) - ref64), initial=0.0))
    return factor * e32, e32


# ------------------------------------------------------------------------------- swiglu ---
SWIGLU_SHAPES = ((16, 16, 128), (48, 64, 128), (1040, 1280, 2176))     # (I, ld_act, ld_gu); 1280 / 4 = 320 float4: the loop runs twice
SWIGLU_T = (1, 3)
SWIGLU_GATES = (0.0, -0.0, 20.0, -20.0, -88.0, -100.0, 90.0)
SWIGLU_REFUSED = ((24, 64, 128), (16, 18, 128), (32, 16, 128))           # I % 16, ld_act % 4, ld_act < I


def interleave_gu(g, u, ld_gu, fill=np.nan):
    """gate / up [T][I] -> gu [T][ld_gu] in blocks of [16 gate | 16 up]; the columns past 2 I hold `fill`"""
    T, I = g.shape
    gu = np.full((T, ld_gu), fill, np.float32)
    b = np.stack([g.reshape(T, I // 16, 16), u.reshape(T, I // 16, 16)], axis=2).reshape(T, 2 * I)
    gu[:, :2 * I] = b
    return gu


def swiglu_inputs(I, T, seed=0):
    """gate f32 [T][I] with the special gates planted in every row, up f32 [T][I]"""
    g_ = rng(400 + I + T + seed)
    g = (g_.standard_normal((T, I)) * 3.0).astype(np.float32)
    u = g_.standard_normal((T, I)).astype(np.float32)
    for t in range(T):
        cols = (np.arange(len(SWIGLU_GATES)) * 2 + t) % I
        g[t, cols] = np.array(SWIGLU_GATES, np.float32)
    return frozen(g, u)


def swiglu_ref(g, u, dtype=np.float64):
    g, u = np.asarray(g, dtype), np.asarray(u, dtype)
    with np.errstate(over="ignore"):
        return (g / (dtype(1.0) + np.exp(-g)) * u).astype(dtype)


# ------------------------------------------------------------------------------- gather ---
GATHER_DIMS = (64, 1028, 2304)       # 1028: one float4 past the 1024-column stride
GATHER_IDS = (10, 0, 3, 3, 10)
GATHER_ROWS = 11
GATHER_SCALES = (12.0, 1.0)


def gather_inputs(dim, seed=0):
    g = rng(500 + dim + seed)
    v = g.standard_normal((GATHER_ROWS, dim)).astype(np.float32)
    hi, lo = split_hi_lo(v)
    return frozen(hi, lo, np.array(GATHER_IDS, np.int32))


def gather_ref(hi, lo, ids, scale):
    """float32, the kernel's two operations: (hi + lo) * scale, or hi * scale without a low table"""
    a = np.asarray(hi, np.float32)[ids]
    if lo is not None:
        a = a + np.asarray(lo, np.float32)[ids]
    return (a * np.float32(scale)).astype(np.float32)


# --------------------------------------------------------------------------------- pool ---
POOL_MODES = (0, 1, 2, 3)            # wmean, mean, lasttoken, cls
POOL_MODE_NAMES = ("wmean", "mean", "lasttoken", "cls")
POOL_DIMS = (64, 260, 2304, 2560)
POOL_LENS = ((1, 2, 5), (4, 67))     # fewer tokens than waves, one wave's tail, 17 passes of the four waves
POOL_ZERO_SEQ = {(1, 2, 5): 1, (4, 67): 0}
POOL_BAR_FACTOR = 8.0
# Largest float32-restatement errors over the table (test_cpu_text_ops_ref.py prints and bounds them):
#   pooled rows: 6.6e-9 .. 4.5e-8 (values ~ dim^-1/2)        normed token rows (the tap): 3.2e-7 .. 7.6e-7 (values ~ 1)


def pool_inputs(dim, lens, seed=0):
    T = int(sum(lens))
    g = rng(600 + dim + T + seed)
    h = (g.standard_normal((T, dim)) * 2.0 + 0.3).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    z = POOL_ZERO_SEQ[tuple(lens)]
    h[off[z]:off[z + 1]] = 0.0
    w = (1.0 + 0.3 * g.standard_normal(dim)).astype(np.float32)
    return frozen(h, w, off)


def pool_ref(h, w, off, eps, mode, dtype=np.float64):
    """(pooled [B][dim], normed [T][dim]): RMSNorm -> pooling -> x / max(|x|, 1e-12)"""
    y = rms_norm(h, w, eps, dtype)
    out = np.zeros((len(off) - 1, y.shape[1]), dtype)
    for b in range(len(off) - 1):
        r = y[off[b]:off[b + 1]]
        L = r.shape[0]
        if mode == 0:
            wt = np.arange(1, L + 1, dtype=dtype)
            p = (r * wt[:, None]).sum(axis=0, dtype=dtype) / wt.sum(dtype=dtype)
        elif mode == 1:
            p = r.sum(axis=0, dtype=dtype) / dtype(L)
        elif mode == 2:
            p = r[L - 1]
        else:
            p = r[0]
        n = np.sqrt((p * p).sum(dtype=dtype))
        out[b] = p / max(n, dtype(1e-12))
    return out, y


# -------------------------------------------------------------------------- conversions ---
CONVERT_N = (1, 3, 4, 5, 1023, 2048 * 256 * 4 + 1203)      # the last: past 2048 blocks x 256 threads x 4, the stride loop runs
CONVERT_PAD = ((0, 8), (8, 8), (12, 2304), (2304 * 3, 2304 * 8))
SPLIT_N = (1, 255, 2048 * 256 + 7)
NONZERO_N = (1, 63, 65)
NONZERO_FAR = 2048 * 256 + 5                               # an index only the stride loop reaches
SEQ_OFFSETS = (0, 1, 300, 301, 563)                        # lengths 1, 299 (past the 256 threads), 1, 262


def rounding_patterns():
    """float32 bit patterns (uint32) around every bf16 rounding decision: for each of the 128 bf16 significands of the binade
    [1, 2) and of a subnormal-result binade, the midpoint to the next one (a tie: to even for even significands, to odd + 1 for
    odd ones) and both its float32 neighbours; +-0, float32 and bf16 subnormals, the largest finite float (rounds to inf), the
    largest value that stays finite, +-inf, NaNs (quiet, signalling, with a payload in the low half only)."""
    pats = []
    for base in (0x3F800000, 0xBF800000, 0x00000000, 0x7F000000):
        m = np.arange(128, dtype=np.uint32) << 16
        for low in (0x7FFF, 0x8000, 0x8001, 0x0000, 0x0001, 0xFFFF):
            pats.append(base | m | np.uint32(low))
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00007FFF, 0x00008001, 0x007FFFFF, 0x807FFFFF,
                        0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                        0x7F800001, 0x7FA00000, 0x7F80FFFF, 0xFF800001], np.uint32)
    return np.concatenate([np.concatenate(pats), special]).astype(np.uint32)


def convert_input(n, seed=0):
    """n float32 values as bit patterns: the rounding patterns first (repeated from the far end too), random bit patterns between"""
    u = rng(700 + seed + n % 1000).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    p = rounding_patterns()
    k = min(n, p.size)
    u[:k] = p[:k]
    if n > 2 * p.size:
        u[n - p.size:] = p
    return frozen(u)


def split_input(n, seed=0):
    """finite float32 values over many binades, the rounding patterns among them"""
    g = rng(710 + seed + n % 1000)
    v = (g.standard_normal(n) * np.exp2(g.integers(-40, 40, size=n))).astype(np.float32)
    p = rounding_patterns().view(np.float32)
    p = p[np.isfinite(p) & (np.abs(p) < 3.0e38)]
    k = min(n, p.size)
    v[n - k:] = p[:k]
    return frozen(v)


def positions_ref(offsets, fill):
    """(pos [T_alloc], seq_of [T_alloc]) for offsets [B + 1]; entries from offsets[-1] on keep `fill`"""
    T = offsets[-1] + 16
    pos, seq = np.full(T, fill, np.int32), np.full(T, fill, np.int32)
    for b in range(len(offsets) - 1):
        pos[offsets[b]:offsets[b + 1]] = np.arange(offsets[b + 1] - offsets[b])
        seq[offsets[b]:offsets[b + 1]] = b
    return pos, seq


# --------------------------------------------------------------------------- planes_sum ---
PLANES_N_PARTS = (1, 2, 3, 9)
PLANES_T = (1, 5)
PLANES_SHAPES = ((64, 128, 64), (2304, 2304, 2304), (1028, 1152, 1100))     # (N, ldp, ldo); 1028 / 4 = 257: a second block of one thread
PLANES_ALPHA = (1.0, 0.25)          # powers of two: a * alpha is exact, so a fused multiply-add gives the bits of multiply, then add
PLANES_REFUSED = ((66, 128, 128), (64, 130, 64), (64, 128, 66))
HP_GEMM_BAR = 2.0 ** -15            # x sum_k |a_k| |w_k|: the dropped lo x lo term and the two splits are each <= 2^-16 of that sum


def planes_inputs(n_parts, T, N, ldp, seed=0):
    g = rng(800 + n_parts + T + N + seed)
    parts = g.standard_normal((n_parts, T + 2, ldp)).astype(np.float32)        # (two rows of pitch between the planes)
    out0 = g.standard_normal((T, N)).astype(np.float32)
    return frozen(parts, out0)


def planes_sum_ref(parts, T, N, out0, alpha, accumulate):
    """float32, the kernel's order: planes in order, then * alpha, then + out"""
    a = np.asarray(parts[0][:T, :N], np.float32).copy()
    for p in range(1, parts.shape[0]):
        a = a + parts[p][:T, :N]
    r = (a * np.float32(alpha)).astype(np.float32)
    if accumulate:
        r = r + np.asarray(out0, np.float32)
    return r.astype(np.float32)


# -------------------------------------------------------------------------- patch embed ---
PATCH_P = 14
PATCH_K = 640                       # 3 * 14 * 14 = 588 padded to the weight's pitch
PATCH_D = (128, 256)
PATCH_IMAGES = ((1, 2, 2), (3, 3, 5), (10, 13, 1), (2, 9, 8))       # (n, H / P, W / P): M = 4, 45, 130 (2 past a tile), 144 (16 past)
# Bar: 2^-20 sum |a| |w| + 2^-23 |ref| (fp32 accumulation of 588 exact bf16 products, two fp32 additions).  The float32
# restatement's error is 2.6e-7 .. 7.7e-7 absolute at these shapes, 0.02 .. 0.07 of the bar (test_cpu_text_ops_ref.py prints it).


# whole images of one value, per image count n: {image: value}.  A single image stays random (it is the only operand the case has), two
# images carry the all-255 one, three and more both
PATCH_CONST = {1: {}, 2: {1: 255}, 3: {1: 0, 2: 255}, 10: {3: 0, 4: 255}}


def patch_inputs(n, gh, gw, D, seed=0):
    """images u8 [n][H][W][3]: random, and the whole images PATCH_CONST names all 0 / all 255 (image 0 always stays random);
    conv weight f32 [D][3][P][P], bias f32 [D], pos f32 [gh gw][D]"""
    P = PATCH_P
    g = rng(900 + n + 10 * gh + 100 * gw + D + seed)
    imgs = g.integers(0, 256, size=(n, gh * P, gw * P, 3), dtype=np.uint8)
    for i, value in PATCH_CONST[n].items():
        imgs[i] = value
    w = (g.standard_normal((D, 3, P, P)) * 0.05).astype(np.float32)
    b = g.standard_normal(D).astype(np.float32)
    pos = g.standard_normal((gh * gw, D)).astype(np.float32)
    return frozen(imgs, w, b, pos)


def pixels_bf16(u8):
    """the kernel's operand: bf16((x / 255 - 0.5) / 0.5) evaluated in float32"""
    x = np.asarray(u8).astype(np.float32)
    return bf16_round(((x / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5))


def patch_rows(imgs):
    """u8 [n][H][W][3] -> [n gh gw][3][P][P] operands in the conv weight's order"""
    P = PATCH_P
    a = pixels_bf16(imgs)
    n, H, W, _ = a.shape
    a = a.reshape(n, H // P, P, W // P, P, 3).transpose(0, 1, 3, 5, 2, 4)      # n, py, px, c, ky, kx
    return a.reshape(n * (H // P) * (W // P), 3, P, P)


def patch_embed_ref(imgs, w, b, pos, dtype=np.float64):
    """(ref [M][D], sum |a||w| [M][D]) on the operands rounded as the kernel rounds them"""
    A = patch_rows(imgs).reshape(-1, 3 * PATCH_P * PATCH_P)
    Wb = bf16_round(w).reshape(w.shape[0], -1)
    acc = np.asarray(A, dtype) @ np.asarray(Wb, dtype).T
    mag = np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(Wb, np.float64)).T
    M = A.shape[0]
    ref = acc + np.asarray(b, dtype)[None, :] + np.asarray(pos, dtype)[np.arange(M) % pos.shape[0]]
    return ref.astype(dtype), mag


def patch_bar(ref, mag):
    return 2.0 ** -20 * mag + 2.0 ** -23 * np.abs(ref)


# -------------------------------------------------------------------------------- norms ---
LN_EPS = 1e-6
LN_SHAPES = ((288, 384, 384), (1152, 1152, 1152), (1280, 1280, 1280), (1284, 1284, 1284), (2560, 2560, 2560), (3584, 3584, 3584))
LN_ROWS = (1, 2, 7, 8, 9)           # (dim, ldx, ldo); the widths up to 1280 run two rows per wave: odd counts, a partial last workgroup
RMS_SHAPES = ((64, 64, 64), (2304, 2304, 2304), (2564, 2564, 2564), (3584, 3584, 3584))
RMS_ROWS = (1, 5)
NORM_REFUSED = ((3588, 3588, 3588), (66, 68, 68), (64, 60, 64), (64, 64, 60))     # too wide; dim % 4; ldx < dim; ldo < dim
# Bar: |out - ref| <= ulp_bf16(ref): an fp32 error can move the rounding to the neighbouring bf16 value and no further.  A float32
# layer_norm lands within 0.53 ulp at width 3584 (test_cpu_text_ops_ref.py bounds it at 0.6).


NORM_CANCEL = 2.0 ** -12


def norm_inputs(dim, rows, seed=0):
    """x f32 [rows][dim], w, b f32 [dim].  The one-ulp bar presumes that an fp32 evaluation is good to half a bf16 ulp OF THE
    RESULT: a handful of fp32 roundings, 2^-21 of |a w| + |b| (a = the normalised x), must stay below 2^-9 |ref|.  A draw in
    which a product cancels against its bias to below 2^-12 of their sizes breaks that for ANY fp32 evaluation (numpy's float32
    layer_norm misses the bar there by the same 1.05 ulp the kernel does), so the bias of such a column is stepped by 1 / 32 of
    its value until no row cancels — decided on the float64 reference alone.  (The RMSNorm cases draw from here too and ignore b:
    without a bias nothing cancels, the stepping changes nothing they read.)"""
    g = rng(1000 + dim + rows + seed)
    x = (g.standard_normal((rows, dim)) * 1.7 + 0.4).astype(np.float32)
    w = (1.0 + 0.3 * g.standard_normal(dim)).astype(np.float32)
    b = (0.2 * g.standard_normal(dim)).astype(np.float32)
    for _ in range(64):
        cols = np.nonzero(layer_norm_cancels(x, w, b).any(axis=0))[0]
        if not cols.size:
            break
        b[cols] = (b[cols] * np.float32(1.03125)).astype(np.float32)
    assert not layer_norm_cancels(x, w, b).any()
    return frozen(x, w, b)


def layer_norm_cancels(x, w, b):
    """elements whose float64 LayerNorm is below NORM_CANCEL of |a w| + |b|"""
    x64 = np.asarray(x, np.float64)
    a = (x64 - x64.mean(axis=-1, keepdims=True)) / np.sqrt(x64.var(axis=-1, keepdims=True) + LN_EPS)
    aw = a * np.asarray(w, np.float64)
    return np.abs(aw + b) < NORM_CANCEL * (np.abs(aw) + np.abs(np.asarray(b, np.float64)))


def layer_norm(x, w, b, eps, dtype=np.float64):
    x, w, b = np.asarray(x, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    mu = x.mean(axis=-1, keepdims=True, dtype=dtype)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True, dtype=dtype)
    return ((x - mu) / np.sqrt(var + dtype(eps)) * w + b).astype(dtype)
