"""Plain numpy restatements of the EVisRAG generator's small kernels (csrc/gen_kernels.hip: multimodal RoPE + KV-cache append, the
vision tower's 2-D rotary embedding, the sampler and its noise, mark_seen, decode_begin, the row movers), the case tables
tests/test_gpu_gen_ops.py runs them on, and the bars it holds the kernels to.  Every arithmetic operation takes a `dtype`:
np.float64 is the reference, np.float32 the "float32 restatement" — the same formulas in numpy's float32 — whose distance from
the reference is the yardstick of the rotation bar.  tests/test_cpu_gen_ops_ref.py pins all of this against
oracle/qwen_gen_oracle.py and oracle/qwen_vision_oracle.py.  Nothing here needs a GPU or the built library."""
import functools

import numpy as np

from tests.chat_ref import grid_logits
from tests.text_ops_ref import bf16_bits, bf16_round, bf16_to_f32, frozen, rng, ulp_bf16  # noqa: F401

F32 = np.float32
SENTINEL = 12345.0          # (a bf16 buffer holds it as 12352: the tests compare with the fill they read back)


# ------------------------------------------------------------------------- rotation bar ---
# |out - ref64| <= 1/2 ulp_bf16(ref64) + ROT_MARGIN for every rotated element, and at least ROT_EXACT_SHARE of them carry the
# reference's bf16 bits: the output is the ONE bf16 rounding of a float32 rotation.  ROT_MARGIN is four times the largest
# distance of the float32 restatement from the float64 reference over the cases of this file (test_cpu_gen_ops_ref.py measures
# and bounds it: M-RoPE 9.3e-7 at |x| up to 14.2, vision 5.5e-7 at |x| up to 11.8) — half a bf16 ulp of a value of size 1 is
# 2e-3 .. 4e-3, a rotation by a neighbouring pair's angle or the wrong position component moves an element by its own size.
ROT_F32_DIST = 1.2e-6
ROT_MARGIN = 4.0 * ROT_F32_DIST
ROT_EXACT_SHARE = 0.95


def rotation_check(got, ref64):
    """(worst (|got - ref| - 1/2 ulp) over ROT_MARGIN [<= 1 passes], share of elements with the reference's bf16 bits)"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    excess = np.abs(got - ref64) - 0.5 * ulp_bf16(ref64)
    same = bf16_bits(got.astype(F32)) == bf16_bits(ref64.astype(F32))
    return float(excess.max() / ROT_MARGIN), float(same.mean())


def rotate_pairs(x1, x2, ang32, dtype=np.float64):
    """x * cos + rotate_half(x) * sin on the pair (x1, x2); the ANGLE is float32 (HF: float32 position times float32 inverse
    frequency), its cosine and sine are taken in `dtype`"""
    a = np.asarray(ang32, F32).astype(dtype)
    c, s = np.cos(a), np.sin(a)
    x1, x2 = np.asarray(x1, dtype), np.asarray(x2, dtype)
    return (x1 * c - x2 * s).astype(dtype), (x2 * c + x1 * s).astype(dtype)


# ------------------------------------------------------------------------------ M-RoPE ---
MROPE_SECTIONS = (16, 24, 24)
MROPE_THETA = 1000000.0
MROPE_HEADS = ((28, 4), (4, 2), (2, 2), (3, 1))       # (3, 1): 5 head slots, the last workgroup holds waves past the end
MROPE_T = (1, 3, 5)
MROPE_PARTS = (1, 7, 8, 9, 16, 17)                    # the 8-wide unrolled plane sum and its tail
MROPE_PLACEMENTS = ("host_row0", "device_row0", "cache_rows")
MROPE_CACHE_ROWS = 16
MROPE_ROW0 = {"host_row0": 5, "device_row0": 7, "cache_rows": 1}
MROPE_ROWS = (9, 2, 11, 4, 0)                         # cache_rows: one cache row per token, not adjacent, not ordered
MROPE_PAD = 8                                         # ld, ldq, ld_cache beyond the used columns
# (temporal, height, width) of a token: components far apart (a section mix-up moves every element), then 0, 1, 8191, 32767
MROPE_POS = ((1000, 17, 333), (0, 0, 0), (1, 1, 1), (8191, 8191, 8191), (32767, 32767, 32767), (32767, 1, 8191))


def mrope_inv_freq(theta=MROPE_THETA):
    """float32 [64]: theta^(-2p/128), evaluated as HF does (float32 exponent, float32 power, float32 reciprocal)"""
    e = (np.arange(0, 128, 2, dtype=F32) / F32(128)).astype(F32)
    return (F32(1.0) / np.power(F32(theta), e).astype(F32)).astype(F32)


def mrope_section_of(sections=MROPE_SECTIONS):
    """[64] -> 0 / 1 / 2: the position component of pair p"""
    return np.repeat(np.arange(3), sections)


def mrope_angles(pos3, inv_freq, sections=MROPE_SECTIONS):
    """pos3 int [3][T] -> float32 angles [T][64]"""
    sel = mrope_section_of(sections)
    pos = np.asarray(pos3)[sel].astype(F32)                       # [64][T]
    return (pos * np.asarray(inv_freq, F32)[:, None]).astype(F32).T


def mrope_positions(T, first):
    """pos3 int32 [3][T + 3]: token t at MROPE_POS[(first + t) % 6]; the stride's tail holds positions nobody may read"""
    p = np.full((3, T + 3), 12345, np.int32)
    for t in range(T):
        p[:, t] = MROPE_POS[(first + t) % len(MROPE_POS)]
    return p


def plane_sum_f32(parts, bias=None):
    """the kernel's float32 sum: bias (or 0) + plane 0 + plane 1 + ... in that order"""
    parts = np.asarray(parts, F32)
    acc = np.zeros(parts.shape[1:], F32) if bias is None else np.broadcast_to(np.asarray(bias, F32), parts.shape[1:]).copy()
    for p in parts:
        acc = (acc + p).astype(F32)
    return acc


def mrope_ref(x, pos3, inv_freq, H, KV, sections=MROPE_SECTIONS, dtype=np.float64):
    """x float32 [T][(H + 2 KV) * 128] (the summed rows) -> the same shape in `dtype`: q and k heads rotated, v heads copied"""
    T = x.shape[0]
    ang = mrope_angles(np.asarray(pos3)[:, :T], inv_freq, sections)
    out = np.asarray(x, dtype).copy()
    for hs in range(H + KV):
        a, b = x[:, hs * 128:hs * 128 + 64], x[:, hs * 128 + 64:hs * 128 + 128]
        out[:, hs * 128:hs * 128 + 64], out[:, hs * 128 + 64:hs * 128 + 128] = rotate_pairs(a, b, ang, dtype)
    return out


def mrope_rows_input(H, KV, T, seed=0):
    """bf16-representable rows [T][(H + 2 KV) * 128], a few elements of each row at 4x the others"""
    g = rng(7000 + 131 * H + 17 * KV + T + seed)
    x = g.standard_normal((T, (H + 2 * KV) * 128)).astype(F32)
    x[:, ::37] *= F32(4.0)
    return frozen(bf16_round(x))


def mrope_planes_input(H, KV, T, n_parts, seed=0):
    """(parts f32 [n_parts][T][cols], bias f32 [cols]): planes of mixed sign and size, so that the ORDER of the sum matters; scaled
    so that the sums are of the size of the bf16 rows"""
    cols = (H + 2 * KV) * 128
    g = rng(7100 + 131 * H + 17 * KV + T + 1000 * n_parts + seed)
    parts = (g.standard_normal((n_parts, T, cols)) * (0.4 + 1.2 * g.random((n_parts, 1, 1))) / np.sqrt(n_parts)).astype(F32)
    bias = (0.5 * g.standard_normal(cols)).astype(F32)
    return frozen(parts, bias)


def mrope_cache_rows(placement, T):
    """the cache row of token t"""
    if placement == "cache_rows":
        return list(MROPE_ROWS[:T])
    return [MROPE_ROW0[placement] + t for t in range(T)]


# --------------------------------------------------------------------- vision 2-D RoPE ---
ROPE2D_CASES = ((16, 1, 3), (40, 3, 3), (64, 1, 5), (40, 1, 5))       # (hh, heads, T): T * 2 heads is no multiple of 4
ROPE2D_PAD = 8


def rope2d_freq(hh):
    """float32 [64]: pair p < hh turns by 10000^(-2 (p mod hh/2) / hh) — the first half of the pairs with h, the second with w;
    entries from hh on are never used (zero)"""
    q = hh // 2
    f = np.zeros(64, F32)
    e = (np.arange(0, hh, 2, dtype=F32) / F32(hh)).astype(F32)
    inv = (F32(1.0) / np.power(F32(10000.0), e).astype(F32)).astype(F32)          # [hh / 2]
    f[:hh] = np.concatenate([inv, inv])[:hh]
    assert len(inv) == q
    return f


def rope2d_positions(T, seed=0):
    """(pos_h, pos_w) int32 [T]: different in every row, up to the 72 x 72 grid of a full page, row 0 at (0, 71)"""
    g = rng(7200 + T + seed)
    ph = g.integers(0, 72, T).astype(np.int32)
    pw = ((ph + 1 + g.integers(0, 70, T)) % 72).astype(np.int32)
    ph[0], pw[0] = 0, 71
    return frozen(ph, pw)


def rope2d_input(hh, heads, T, seed=0):
    """bf16-representable qkv rows [T][3 * heads * 2 hh + pad]"""
    g = rng(7300 + 11 * hh + heads + T + seed)
    x = g.standard_normal((T, 3 * heads * 2 * hh + ROPE2D_PAD)).astype(F32)
    x[:, ::29] *= F32(4.0)
    return frozen(bf16_round(x))


def rope2d_ref(qkv, hh, n_slots, pos_h, pos_w, sec_h, freq, dtype=np.float64):
    """the first n_slots head slots (2 hh columns, pairs (p, p + hh)) rotated, everything else as it was"""
    x = np.asarray(qkv, F32)
    p = np.arange(hh)
    pos = np.where(p[None, :] < sec_h, np.asarray(pos_h)[:, None], np.asarray(pos_w)[:, None]).astype(F32)     # [T][hh]
    ang = (pos * np.asarray(freq, F32)[None, :hh]).astype(F32)
    out = x.astype(dtype).copy()
    for j in range(n_slots):
        c0 = j * 2 * hh
        out[:, c0:c0 + hh], out[:, c0 + hh:c0 + 2 * hh] = rotate_pairs(x[:, c0:c0 + hh], x[:, c0 + hh:c0 + 2 * hh], ang, dtype)
    return out


# ------------------------------------------------------------------------ decode_begin ---
GEN_ATT_SPLITS = 16
STATE_WORDS = 42            # token | pos[3] | len | step | splits | pad | cu_q[17] | cu_kv[17]
ST_TOKEN, ST_POS, ST_LEN, ST_STEP, ST_SPLITS, ST_CU_Q, ST_CU_KV = 0, 1, 4, 5, 6, 8, 25
KV_L = (1, 64, 127, 128, 129, 2048, 2049, 8191, 8192, 32768)
KV_Q_ROWS = (1, 7)


def gen_kv_split(L):
    """(splits, chunk) of csrc/kernels.h, restated"""
    splits = min(GEN_ATT_SPLITS, max(1, (L + 127) // 128))
    chunk = ((L + splits - 1) // splits + 63) // 64 * 64
    return (L + chunk - 1) // chunk, chunk


def kv_split_direct(L):
    """the same rule said directly: the smallest multiple of 64 that covers L rows with the planned number of ranges (one per 128
    rows begun, at most 16); the ranges that hold a row are counted"""
    want = min(GEN_ATT_SPLITS, max(1, -(-L // 128)))
    chunk = 64
    while chunk * want < L:
        chunk += 64
    return sum(1 for i in range(GEN_ATT_SPLITS) if i * chunk < L), chunk


def decode_begin_ref(state, q_rows):
    """state int32 [42] -> the state after decode_begin"""
    st = np.array(state, np.int32)
    L = int(st[ST_LEN]) + 1
    splits, chunk = gen_kv_split(L)
    st[ST_SPLITS] = splits
    for i in range(GEN_ATT_SPLITS + 1):
        st[ST_CU_Q + i] = i * q_rows
        st[ST_CU_KV + i] = min(L, i * chunk)
    return st


# --------------------------------------------------------------------------- mark_seen ---
def mark_seen_ref(words, ids, V):
    """uint32 words with the bits of the ids inside [0, V) set"""
    out = np.array(words, np.uint32)
    for i in ids:
        if 0 <= i < V:
            out[i >> 5] |= np.uint32(1 << (i & 31))
    return out


# ----------------------------------------------------------------------------- sampler ---
SAMPLE_V = (1, 255, 16383, 16384, 16385, 152064)     # around 64 x 256: workgroups that see nothing, one element, a second round
SAMPLE_PENALTY = 1.3


def penalised(logits, seen, penalty, dtype=np.float64):
    x = np.asarray(logits, dtype)
    return np.where(np.asarray(seen, bool), np.where(x > 0, x / dtype(penalty), x * dtype(penalty)), x).astype(dtype)


@functools.lru_cache(maxsize=None)
def greedy_cases(V):
    """name -> (logits f32 [V], seen bool [V]) for temperature 0 at penalty SAMPLE_PENALTY.  The seen ids are 0, 31, 32, V - 1
    (those below V).  Distinct penalised values are >= 1e-3 apart (test_cpu_gen_ops_ref.py), equal ones are planted."""
    edge = sorted({i for i in (0, 31, 32, V - 1) if i < V})
    seen = np.zeros(V, bool)
    seen[edge] = True
    out = {}
    # the seen ids carry the largest raw logits; after the penalty an unseen neighbour wins (V = 1: the only token does)
    x = grid_logits(1, V, 8000 + V)[0].copy()
    top = F32(x.max())
    near = [i for i in (1, 30, 33, V - 2) if 0 <= i < V and i not in edge]
    x[edge] = top + F32(3.0) + F32(0.5) * np.arange(len(edge), dtype=F32)
    x[near] = top + F32(2.8) + F32(0.5) * np.arange(len(near), dtype=F32)
    out["seen_on_top"] = frozen(x, seen.copy())
    # every logit negative, the seen ones made more so; one seen logit exactly 0 stays 0 and wins
    y = grid_logits(1, V, 8100 + V)[0].copy()
    y -= F32(y.max() + F32(0.25))
    out["all_negative"] = frozen(y.copy(), seen.copy())
    z = y.copy()
    z[edge[-1]] = F32(0.0)
    out["seen_zero"] = frozen(z, seen.copy())
    # the maximum twice, in different workgroups where V allows, and a third time at a seen id (penalised: out of the race)
    w = grid_logits(1, V, 8200 + V)[0].copy()
    if V >= 3:
        m = F32(w.max() + F32(1.0))
        a, b = min(V // 3 + 1, V - 2), V - 2
        w[a], w[b], w[edge[0]] = m, m, m
    out["ties"] = frozen(w, seen.copy())
    return out


def greedy_ref(logits, seen, penalty=SAMPLE_PENALTY):
    """argmax of the penalised logits in float64, the lowest id among equals"""
    return int(np.argmax(penalised(logits, seen, penalty)))


# the distribution test: chat_ref.sampling_logits() with everything outside the planted top 8 lowered by SAMPLE_TAIL_DROP.  The
# generator's sampler has no top-k filter: at their own -6 .. -9 the other 992 tokens would hold 0.1 % (T = 0.7) to 30 % (T = 1.5)
# of the mass and "nothing outside the top 8" would be false of a correct sampler; at -66 .. -69 their scaled logits lie below
# -44 and the finite noise range [-2.86, 16.64] cannot lift them over the top 8 (>= -2.86).
SAMPLE_TAIL_DROP = 60.0


# ------------------------------------------------------------------------------- noise ---
MASK64 = (1 << 64) - 1
DEFECTIVE_DRAW = 0xFFFFFF
U_MAX = F32(1.0) - F32(2.0 ** -24)                   # the largest float32 below 1
# (seed, step, idx) whose draw is 0xFFFFFF with idx < 4096
KNOWN_DEFECTIVE = ((0, 5314, 2909), (0, 6688, 947), (11, 1314, 955))


def noise_draw(seed, step, idx):
    """the 24-bit draw of (seed, step, idx): the kernels' counter hash (splitmix64's finaliser), uint64 arrays broadcast"""
    with np.errstate(over="ignore"):
        ctr = (np.asarray(step, np.uint64) << np.uint64(32)) | np.asarray(idx, np.uint64)
        x = np.uint64(seed & MASK64) + np.uint64(0x9E3779B97F4A7C15) * ctr
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(40)).astype(np.uint32)


def uniform_old(draw):
    """the parent's map, float32 bit for bit: (float(draw) + 0.5) * 2^-24 — 1.0 at the draw 0xFFFFFF"""
    return ((np.asarray(draw, np.uint32).astype(F32) + F32(0.5)).astype(F32) * F32(2.0 ** -24)).astype(F32)


def uniform_new(draw):
    """the kernels' map: the same, held at the largest float32 below 1"""
    return np.minimum(uniform_old(draw), U_MAX).astype(F32)


def gumbel(u, dtype=np.float64):
    u = np.asarray(u, dtype)
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(u))


def find_defective(seed, V, steps, chunk=512):
    """every (seed, step, idx) with step < steps, idx < V whose draw is 0xFFFFFF, in (step, idx) order"""
    idx = np.arange(V, dtype=np.uint64)[None, :]
    out = []
    for s0 in range(0, steps, chunk):
        st = np.arange(s0, min(steps, s0 + chunk), dtype=np.uint64)[:, None]
        hit = np.argwhere(noise_draw(seed, st, idx) == DEFECTIVE_DRAW)
        out += [(seed, int(s0 + a), int(b)) for a, b in hit]
    return out


@functools.lru_cache(maxsize=None)
def defective_triples(V=4096):
    """the known triples and what the search finds for seed 0 in the first 8192 steps (it finds the first two again)"""
    found = find_defective(0, V, 8192)
    return tuple(sorted(set(KNOWN_DEFECTIVE) | set(found)))


def defective_logits(V, idx):
    """(logits f32 [V], D): everything 0 but token D != idx at 30"""
    D = (idx + 1500) % V
    x = np.zeros(V, F32)
    x[D] = F32(30.0)
    return x, D


# -------------------------------------------------------------------------- row movers ---
ROWS_DIM, ROWS_LD_SCATTER, ROWS_LD_GATHER, ROWS_SRC, ROWS_IDX = 300, 308, 320, 9, (7, 0, 3, 8, 2)
PATCH_P, PATCH_TP = 14, 2
PATCH_DIM = 3 * PATCH_TP * PATCH_P * PATCH_P                      # 1176
PATCH_LD = PATCH_DIM + 8
PATCH_PAGES = ((28, 56), (56, 28))                                # (H, W): 2 x 4 and 4 x 2 patches
PATCH_MEAN = (0.48145466, 0.4578275, 0.40821073)                  # the processor's (OPENAI_CLIP_MEAN / STD)
PATCH_STD = (0.26862954, 0.26130258, 0.27577711)


def patch_pages(seed=0):
    g = rng(7400 + seed)
    pages = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PATCH_PAGES]
    pages[0][-1, -1] = (0, 255, 128)                              # the last pixel of a page, extreme values
    return frozen(*pages)


def patch_list():
    """(img, ph, pw) int32: every patch of both pages (so each page's last row and last column), interleaved and reversed"""
    items = [(i, y, x) for i, (h, w) in enumerate(PATCH_PAGES) for y in range(h // PATCH_P) for x in range(w // PATCH_P)]
    items = items[::-2] + items[-2::-2]
    a = np.array(items, np.int32)
    return frozen(a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy())


def normalise_px(px, c, dtype=F32, fused=False):
    """(px / 255 - mean[c]) / std[c] as the kernel evaluates it in float32: px * (1 / 255) - mean, then the division.  fused: the
    product and the difference rounded ONCE (a compiler may contract them) — the cases' bf16 bits do not depend on it."""
    px = np.asarray(px)
    m, s = np.asarray(PATCH_MEAN, F32)[c], np.asarray(PATCH_STD, F32)[c]
    if dtype is not F32:
        return (px.astype(np.float64) / 255.0 - m.astype(np.float64)) / s.astype(np.float64)
    r = F32(1.0) / F32(255.0)
    if fused:
        d = (px.astype(np.float64) * np.float64(r) - m.astype(np.float64)).astype(F32)
    else:
        d = ((px.astype(F32) * r).astype(F32) - m).astype(F32)
    return (d / s).astype(F32)


def patch_rows_ref(pages, img, ph, pw, ld=PATCH_LD):
    """bf16 bits [n][ld] of the float32 restatement: element (c, t, y, x) of the patch, zero pad"""
    P, tp = PATCH_P, PATCH_TP
    out = np.zeros((len(img), ld), F32)
    for i, (im, y, x) in enumerate(zip(img, ph, pw)):
        patch = np.asarray(pages[im])[y * P:(y + 1) * P, x * P:(x + 1) * P]          # [P][P][3]
        for c in range(3):
            v = normalise_px(patch[:, :, c], c)                                       # [P][P]
            out[i, c * tp * P * P:(c + 1) * tp * P * P] = np.tile(v.reshape(-1), tp)
    return bf16_bits(out)
