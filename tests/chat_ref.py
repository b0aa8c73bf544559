"""Plain numpy references (fp64, on the bf16-rounded inputs) of the decode step's kernels, and the planted inputs the op-level
tests of tests/test_gpu_decode_ops.py run on.  tests/test_cpu_chat_ref.py shows, with these references alone, that those
tests can fail: a dropped key moves the attention output by far more than the tolerance, the chi-square test separates the
two temperatures, the top-k equals a stable sort on exact ties.  Nothing here needs a GPU or the built library."""
import functools
import math

import numpy as np

HD = 64                   # head dim of the decode attention
CHAT_KEYS = 256           # keys per chunk (csrc/kernels.h)
CHAT_ATT_SPLITS = 8       # most prompt-key ranges per (prompt, head)
CHAT_SEL_WGS = 64         # slices of a group's flat candidate range
GREEDY, BEAM, SAMPLE = 0, 1, 2


# ------------------------------------------------------------------------------ bf16 ---
def bf16_bits(x):
    """float -> uint16 bf16 bit patterns, round to nearest even (finite inputs and infinities)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u.astype(np.uint16)


def bf16_round(x):
    """x rounded to bf16, as float32."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def bf16_ulp(x):
    """spacing of bf16 at |x| (8 significand bits)"""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126))) - 7)


# ------------------------------------------------------------------- decode attention ---
def split_ranges(P, force=0):
    """Prompt-key ranges [lo, hi) of a group with P prompt keys: the kernel's split policy restated — used only to decide
    WHERE to plant keys, never as the thing under test."""
    S = force if force else min(CHAT_ATT_SPLITS, max(1, (P + CHAT_KEYS - 1) // CHAT_KEYS))
    per = (P + S - 1) // S
    out = []
    for sp in range(S):
        lo = min(P, sp * per)
        out.append((lo, min(P, lo + per)))
    return out


def _planted_prompt_keys(P, force=0):
    keys = {P - 1}
    for lo, hi in split_ranges(P, force):
        if lo < hi:
            keys.add(lo)                                    # the first key of every split
            keys.update(j for j in (lo + CHAT_KEYS - 1, lo + CHAT_KEYS) if j < hi)   # the chunk edge inside the split
    keys.update(j for j in (CHAT_KEYS - 1, CHAT_KEYS) if j < P)
    return sorted(keys)


def _planted_tail_keys(n):
    keys = {0, n - 1}
    keys.update(j for j in (CHAT_KEYS - 1, CHAT_KEYS) if j < n)
    return sorted(keys)


# name -> (groups [(slot, plen, [(cache row, tail keys)])], slots, rows, max_new, spike, force_splits)
def _case_table():
    t = {}
    tails5 = [3, 1, 6, 2, 4]
    for P in (1, 255, 256, 257, 513, 2049, 2600):
        t[f"P{P}_nb1"] = dict(groups=[(2, P, [(3, 2)])], slots=3, rows=6, max_new=8)
        t[f"P{P}_nb5"] = dict(groups=[(0, P, list(zip([4, 1, 0, 5, 2], tails5)))], slots=3, rows=6, max_new=8)
    # 16 rows, 5 groups [1, 3, 5, 4, 3]; gsplit 1, 2, 8, 1, 3 differ: the early return at sp >= S runs; unequal tails from 1 up
    sizes, plens, gslots = [1, 3, 5, 4, 3], [7, 300, 2049, 256, 700], [3, 0, 4, 1, 2]
    rows = [9, 3, 14, 0, 7, 12, 1, 15, 5, 10, 2, 13, 6, 11, 4, 8]
    groups, i = [], 0
    for nb, P, sl in zip(sizes, plens, gslots):
        groups.append((sl, P, [(rows[i + b], 1 + (3 * (i + b)) % 11) for b in range(nb)]))
        i += nb
    t["mixed16"] = dict(groups=groups, slots=5, rows=16, max_new=12)
    # tails across the chunk edge: the tail loop's second chunk
    t["tails_1_256_257_300"] = dict(groups=[(2, 40, [(2, 1), (0, 256), (3, 257), (1, 300)])], slots=3, rows=4, max_new=300)
    for spike in ("last_tail", "first_prompt", "all_negative"):
        t[f"spike_{spike}"] = dict(groups=[(2, 300, [(1, 3), (0, 5)]), (0, 9, [(2, 4)])], slots=3, rows=3, max_new=8, spike=spike)
    # ranges that hold no key (m = -inf, l = 0 into the merge): the policy never makes one, force_splits does
    t["empty_splits"] = dict(groups=[(2, 1, [(1, 2), (0, 1)]), (0, 3, [(2, 3)])], slots=3, rows=3, max_new=8, force=8)
    return t


ATTN_CASES = _case_table()
ATTN_HEADS = 3            # E = 3 x 64: an odd head count
ATTN_LAYERS, ATTN_LAYER = 2, 1


@functools.lru_cache(maxsize=None)
def attention_case(name):
    """The planted tensors of one case (fixed seed; bf16-rounded float32).  Returns a dict:
    q [n][E]; pk / pv {slot: [plen][E]}; tk / tv {cache row: [tail keys][E]}; step rows (row, slot, tail index) in step order;
    plen per slot; drops: [(kind, owner, key index, affected step rows)] — the keys the dropped-key check removes.
    Every planted key is aligned with the q rows that see it (softmax weight of order 0.1 when there are few of them, never
    negligible) and carries a v row of magnitude >= 1 on a channel of its own."""
    spec = ATTN_CASES[name]
    rng = np.random.default_rng(hash_name(name))
    E, H = ATTN_HEADS * HD, ATTN_HEADS
    spike, force = spec.get("spike"), spec.get("force", 0)
    n = sum(len(g[2]) for g in spec["groups"])
    q = np.zeros((n, E), np.float32)
    pk, pv, tk, tv, step, drops = {}, {}, {}, {}, [], []
    plen = [0] * spec["slots"]
    i0 = 0
    for slot, P, members in spec["groups"]:
        plen[slot] = P
        nb = len(members)
        u = rng.standard_normal((H, HD))
        u /= np.linalg.norm(u, axis=1, keepdims=True)            # the group's common q direction per head
        qg = 6.0 * u[None] + 0.5 * rng.standard_normal((nb, H, HD))
        K = 0.5 * rng.standard_normal((P, H, HD))
        V = rng.standard_normal((P, H, HD))
        pkeys = _planted_prompt_keys(P, force)
        most = max(t for _, t in members)
        n_plant = len(pkeys) + len(_planted_tail_keys(most))
        # planted keys share ~3/4 of the softmax mass: exp(s) = 3 * (random keys' mass ~ 1.13 each) / planted keys
        s_star = max(1.5, math.log(3.0 * 1.13 * (P + most) / n_plant))
        gamma = s_star / (0.125 * 6.0)
        for c, j in enumerate(pkeys):
            K[j] = gamma * u
            V[j] = 0.0
            V[j, :, (7 * c) % HD] = 4.0 if c % 2 == 0 else -4.0
        lift = (s_star + 6.0) / s_star                          # a spiked key: 6 nats (8.7 in the exp2 domain) above the planted ones
        if spike == "first_prompt":
            K[0] = lift * gamma * u
        if spike == "all_negative":                              # every score ~ -30: the same softmax, far below zero
            K = K - 40.0 * u[None]
        pk[slot], pv[slot] = bf16_round(K.reshape(P, E)), bf16_round(V.reshape(P, E))
        rows_i = list(range(i0, i0 + nb))
        for j in pkeys:
            drops.append(("prompt", slot, j, rows_i))
        for b, (row, tl) in enumerate(members):
            Kt = 0.5 * rng.standard_normal((tl, H, HD))
            Vt = rng.standard_normal((tl, H, HD))
            for c, j in enumerate(_planted_tail_keys(tl)):
                Kt[j] = gamma * u
                Vt[j] = 0.0
                Vt[j, :, (7 * (c + len(pkeys)) + 3 * b) % HD] = -4.0 if c % 2 == 0 else 4.0
                drops.append(("tail", row, j, [i0 + b]))
            if spike == "last_tail":
                Kt[tl - 1] = lift * gamma * u
            if spike == "all_negative":
                Kt = Kt - 40.0 * u[None]
            tk[row], tv[row] = bf16_round(Kt.reshape(tl, E)), bf16_round(Vt.reshape(tl, E))
            step.append((row, slot, tl - 1))
        q[i0:i0 + nb] = bf16_round(qg.reshape(nb, E))
        i0 += nb
    return dict(name=name, E=E, H=H, n=n, q=q, pk=pk, pv=pv, tk=tk, tv=tv, step=step, plen=plen, drops=drops, slots=spec["slots"],
                rows=spec["rows"], max_new=spec["max_new"], max_len=max(plen) + 1, force=force)


def hash_name(name):
    """a seed that does not depend on the interpreter's string hashing"""
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def decode_attention_ref(case, drop=None, dtype=np.float64, only_rows=None):
    """att [n][E]: per step row and head ONE softmax over [the slot's prompt keys | the row's own tail keys], scale 64^-0.5.
    drop = (kind, owner, key index): that key does not exist.  dtype float32: the same statement in fp32 (for the fp32 term)."""
    E, H = case["E"], case["H"]
    out = np.zeros((case["n"], E), dtype)
    for i, (row, slot, tl) in enumerate(case["step"]):
        if only_rows is not None and i not in only_rows:
            continue
        K = np.concatenate([case["pk"][slot], case["tk"][row][:tl + 1]]).astype(dtype)
        V = np.concatenate([case["pv"][slot], case["tv"][row][:tl + 1]]).astype(dtype)
        if drop is not None:
            kind, owner, j = drop[:3]
            at = j if (kind == "prompt" and owner == slot) else case["plen"][slot] + j if (kind == "tail" and owner == row) else None
            if at is not None:
                K, V = np.delete(K, at, axis=0), np.delete(V, at, axis=0)
        qi = case["q"][i].astype(dtype)
        for h in range(H):
            c = slice(h * HD, (h + 1) * HD)
            # (sums spelled out, not BLAS: the fp32 statement must not depend on the machine's matmul)
            s = (K[:, c] * qi[c]).sum(axis=1, dtype=dtype) * dtype(0.125)
            p = np.exp(s - s.max())
            out[i, c] = ((p / p.sum(dtype=dtype))[:, None] * V[:, c]).sum(axis=0, dtype=dtype)
    return out


def bf16_tol(ref, a):
    """|got - ref| allowed after ONE bf16 rounding of an fp32 result: 2^-8 |ref| (half a bf16 ulp is at most 2^-8 of the value)
    plus a, the fp32 accumulation term"""
    return 2.0 ** -8 * np.abs(ref) + a


def fp32_term(cases_fn, ref_fn):
    """8 x the largest |fp32 restatement - fp64 reference| over the planted inputs (8: another summation order, hardware exp2)"""
    worst = 0.0
    for c in cases_fn():
        worst = max(worst, float(np.abs(ref_fn(c, dtype=np.float32).astype(np.float64) - ref_fn(c)).max()))
    return 8.0 * worst


def all_attention_cases():
    return (attention_case(n) for n in ATTN_CASES)


# -------------------------------------------------------- skinny GEMM, SwiGLU, RMSNorm ---
def gemm_inputs(M, N, K, seed):
    """bf16-rounded A [M][K] (unit scale), W [N][K] (0.1) and an fp32 bias [N]: the input scales of test_gemm_192_tile"""
    rng = np.random.default_rng(seed)
    return (bf16_round(rng.standard_normal((M, K))), bf16_round(0.1 * rng.standard_normal((N, K))),
            rng.standard_normal(N).astype(np.float32))


def gemm_ref(A, W, bias=None, dtype=np.float64):
    if dtype == np.float64:
        out = A.astype(dtype) @ W.astype(dtype).T
    else:                                                    # (spelled out, not BLAS: must not depend on the machine's matmul)
        out = (A.astype(dtype)[:, None, :] * W.astype(dtype)[None]).sum(-1, dtype=dtype)
    return out + bias.astype(dtype) if bias is not None else out


def gemm_split_ref(A, W, ksplit, bias=None):
    """the planes [ksplit][M][N]: split s covers the K-steps [s * ceil(steps / ksplit), ...), bias on split 0 only"""
    M, K = A.shape
    steps = K // 64
    per = (steps + ksplit - 1) // ksplit
    out = np.zeros((ksplit, M, W.shape[0]))
    for s in range(ksplit):
        lo, hi = min(K, s * per * 64), min(K, (s + 1) * per * 64)
        out[s] = A[:, lo:hi].astype(np.float64) @ W[:, lo:hi].astype(np.float64).T
    if bias is not None:
        out[0] += bias
    return out


def interleave16(gate, up):
    """[16 gate | 16 up | ...] along axis 0 (EPI_SWIGLU's weight-row layout)"""
    I = gate.shape[0]
    g = gate.reshape(I // 16, 16, *gate.shape[1:])
    u = up.reshape(I // 16, 16, *up.shape[1:])
    return np.stack([g, u], axis=1).reshape(2 * I, *gate.shape[1:])


def swiglu_ref(gate, up, dtype=np.float64):
    g, u = gate.astype(dtype), up.astype(dtype)
    return g / (dtype(1) + np.exp(-g)) * u


def swiglu_case(M, I, K, seed, dtype=np.float64):
    """(A, interleaved W [2I][K], interleaved bias [2I], act reference [M][I])"""
    rng = np.random.default_rng(seed)
    A = bf16_round(rng.standard_normal((M, K)))
    Wg, Wu = bf16_round(0.1 * rng.standard_normal((I, K))), bf16_round(0.1 * rng.standard_normal((I, K)))
    bg, bu = (0.5 * rng.standard_normal(I)).astype(np.float32), (0.5 * rng.standard_normal(I)).astype(np.float32)
    ref = swiglu_ref(gemm_ref(A, Wg, bg, dtype), gemm_ref(A, Wu, bu, dtype), dtype)
    return A, interleave16(Wg, Wu), interleave16(bg, bu), ref


SWIGLU_CASES = [(5, 160, 320, 71), (16, 496, 192, 72)]       # (M, I, K, seed); 2 I = 320 / 992: column edges of the 256 tile


def accum_case(rows, dim, nsplit, seed):
    """x [rows][dim], planes [nsplit][rows][dim], norm weight [dim], alpha (all fp32 values)"""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((rows, dim))).astype(np.float32)
    parts = rng.standard_normal((nsplit, rows, dim)).astype(np.float32)
    w = (1.0 + 0.2 * rng.standard_normal(dim)).astype(np.float32)
    return x, parts, w, np.float32(0.2214)


def accum_ref(x, parts, w, alpha, eps=1e-5, dtype=np.float64):
    """x + alpha * sum_s parts[s] (plane order), and its RMSNorm * w"""
    acc = parts[0].astype(dtype)
    for s in range(1, parts.shape[0]):
        acc = acc + parts[s].astype(dtype)
    xn = x.astype(dtype) + dtype(alpha) * acc
    y = xn / np.sqrt((xn * xn).mean(-1, keepdims=True) + dtype(eps)) * w.astype(dtype)
    return xn, y


ACCUM_CASES = [(1, 256, 1, 81), (1, 3584, 17, 82), (16, 2304, 9, 83), (16, 256, 8, 84), (17, 256, 9, 85), (17, 3584, 8, 86),
               (45, 2304, 17, 87), (45, 3584, 1, 88)]        # (rows, dim, nsplit, seed)


# ------------------------------------------------------------------------- selection ---
def candidate_scores(logits, seen, mode, penalty, beam_scores=None):
    """[nb][V] fp64 scores of one group in HF order: log_softmax (beams) -> repetition penalty on the seen ids -> + beam score.
    logits fp32 [nb][V], seen bool [nb][V]."""
    x = np.asarray(logits, np.float64).copy()
    if mode == BEAM:
        m = x.max(-1, keepdims=True)
        x = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    x = np.where(seen, np.where(x < 0, x * penalty, x / penalty), x)
    if mode == BEAM and beam_scores is not None:
        x = x + np.asarray(beam_scores, np.float64)[:, None]
    return x


def topk_ref(scores, K, kout=None):
    """The K best of the group's flat candidates r * V + tok, ties to the lower flat index; a score of -inf is no candidate.
    -> (scores, tokens, parents) of length kout (default K), padded with (-inf, -1, -1)."""
    kout = kout or K
    nb, V = scores.shape
    flat = scores.reshape(-1)
    best, taken = [], np.zeros(flat.size, bool)
    for _ in range(min(K, kout)):
        cand = np.where(taken, -np.inf, flat)
        f = int(np.argmax(cand))                             # argmax: the first (lowest) index among equals
        if cand[f] == -np.inf:
            break
        taken[f] = True
        best.append(f)
    sc = np.full(kout, -np.inf)
    tok = np.full(kout, -1, np.int64)
    par = np.full(kout, -1, np.int64)
    for i, f in enumerate(best):
        sc[i], tok[i], par[i] = flat[f], f % V, f // V
    return sc, tok, par


def sampler_probs(scores_row, top_k, temperature):
    """(tokens, probabilities) the sampler must draw from: softmax(top_k best scores / T), best first"""
    sc, tok, _ = topk_ref(scores_row[None], top_k)
    keep = tok >= 0
    z = sc[keep] / temperature
    p = np.exp(z - z.max())
    return tok[keep], p / p.sum()


def slice_bounds(nb, V):
    """flat ranges of the 64 slices of the candidate pass (restated to PLANT candidates, not under test)"""
    total = nb * V
    per = (total + CHAT_SEL_WGS - 1) // CHAT_SEL_WGS
    return [(min(total, w * per), min(total, (w + 1) * per)) for w in range(CHAT_SEL_WGS)]


def grid_logits(nb, V, seed, step=0.01):
    """[nb][V] fp32 logits whose distinct values are >= step apart within a row: a permutation of a grid around zero"""
    rng = np.random.default_rng(seed)
    base = (np.arange(V) - V // 2) * step + step / 2          # (no exact zero: +0 and -0 order differently on the device)
    return np.stack([base[rng.permutation(V)] for _ in range(nb)]).astype(np.float32)


def seen_words(seen):
    """bool [n][V] -> uint32 bit sets [n][ceil(V / 32)] (bit tok & 31 of word tok >> 5)"""
    n, V = seen.shape
    words = (V + 31) // 32
    pad = np.zeros((n, words * 32), bool)
    pad[:, :V] = seen
    return (pad.reshape(n, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


# -------------------------------------------------------------------------- sampling ---
SAMPLE_TOP = np.array([2.0, 1.6, 1.3, 1.0, 0.8, 0.5, 0.3, 0.0])     # the 8 best logits: every expected count of 4096 draws >= 40
SAMPLE_DRAWS, SAMPLE_TOPK, SAMPLE_TEMPS, SAMPLE_SEEDS = 4096, 8, (0.7, 1.5), (20240611, 77)


def sampling_logits(V=1000, seed=5):
    """one row: SAMPLE_TOP at scattered ids, everything else far below"""
    rng = np.random.default_rng(seed)
    x = (-6.0 - 3.0 * rng.random(V)).astype(np.float32)
    ids = rng.permutation(V)[:len(SAMPLE_TOP)]
    x[ids] = SAMPLE_TOP
    return x, ids


def chi2_critical(df, p):
    """upper quantile of the chi-square distribution: scipy when it is there, else Wilson-Hilferty"""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p, df))
    except Exception:
        # normal upper quantile by bisection on erfc, then the cube-root transformation
        lo, hi = 0.0, 40.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if 0.5 * math.erfc(mid / math.sqrt(2.0)) > p:
                lo = mid
            else:
                hi = mid
        z = 0.5 * (lo + hi)
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def chi2_stat(counts, probs):
    counts, probs = np.asarray(counts, np.float64), np.asarray(probs, np.float64)
    exp = counts.sum() * probs
    return float(((counts - exp) ** 2 / exp).sum())


def gumbel_max_draws(scores, temperature, n, seed):
    """a host Gumbel-max sampler over `scores` (the kept candidates): n draws -> counts per candidate"""
    rng = np.random.default_rng(seed)
    g = -np.log(-np.log(rng.random((n, len(scores)))))
    return np.bincount(np.argmax(np.asarray(scores)[None] / temperature + g, axis=1), minlength=len(scores))


# ------------------------------------------------------------ planted selection cases ---
def _beam_scores(sizes):
    """per row of every group: -0.102 * (index in the group): rows of one group sit a fifth of the grid step apart"""
    return np.concatenate([-0.102 * np.arange(nb) for nb in sizes]).astype(np.float32)


def _put_top(row, tokens):
    """rearrange one row so that its largest values sit at `tokens`, best first (still a permutation of the grid)"""
    tokens = list(tokens)
    order = np.argsort(-row, kind="stable")
    top = np.zeros(row.size, bool)
    top[order[:len(tokens)]] = True
    free = np.ones(row.size, bool)
    free[tokens] = False
    out = row.copy()
    out[free] = row[~top]                                    # the other values keep their relative order
    out[tokens] = row[order[:len(tokens)]]
    return out


@functools.lru_cache(maxsize=None)
def selection_cases():
    """name -> dict(mode, V, sizes, logits fp32 [n][V], seen bool [n][V], bscore [n] or None, K, kout, pen)"""
    out = {}

    def add(name, mode, V, sizes, logits, K, kout=None, seen=None, pen=1.0, bscore=True):
        n = sum(sizes)
        assert logits.shape == (n, V)
        out[name] = dict(name=name, mode=mode, V=V, sizes=list(sizes), logits=np.ascontiguousarray(logits, np.float32),
                         seen=seen if seen is not None else np.zeros((n, V), bool), K=K, kout=kout or K, pen=pen,
                         bscore=None if mode != BEAM else _beam_scores(sizes) if bscore is True else np.asarray(bscore, np.float32))

    def rand_seen(n, V, seed, count=6, among_top=40, logits=None):
        rng = np.random.default_rng(seed)
        s = np.zeros((n, V), bool)
        for r in range(n):
            top = np.argsort(-logits[r])[:among_top]
            s[r, rng.choice(top, count, replace=False)] = True
        return s

    # the K best all inside ONE of the 64 slices (a per-slice top-1 would return one of them)
    V, sizes = 4099, [3]
    x = grid_logits(3, V, 101)
    lo, hi = slice_bounds(3, V)[5]
    x[0] = _put_top(x[0], list(range(lo + 4, lo + 20)))
    add("one_slice", BEAM, V, sizes, x, 16, bscore=[0.0, -1.002, -2.004])
    # the K best one per slice; K = CHAT_TOPK_MAX
    x = grid_logits(1, V, 102)
    x[0] = _put_top(x[0], [lo_ + (w % 4) for w, (lo_, _) in enumerate(slice_bounds(1, V))])
    add("one_per_slice", GREEDY, V, [1], x, 64)
    # slices with fewer than K candidates: 1000 / 64 = 16 per slice, K = 50
    x = grid_logits(2, 1000, 103)
    add("short_slices", GREEDY, 1000, [1, 1], x, 50, seen=rand_seen(2, 1000, 1, logits=x), pen=1.2)
    # beam groups of 1, 3, 5, 4, 3 rows
    g = [1, 3, 5, 4, 3]
    x = grid_logits(16, 1000, 104)
    add("groups_K32", BEAM, 1000, g, x, 32, seen=rand_seen(16, 1000, 2, logits=x), pen=1.2)
    x = grid_logits(16, V, 105)
    add("groups_K64", BEAM, V, g, x, 64, seen=rand_seen(16, V, 3, logits=x), pen=1.2)
    x = grid_logits(16, 1000, 106)
    add("groups_kout_gt_K", BEAM, 1000, g, x, 6, kout=10, seen=rand_seen(16, 1000, 4, logits=x), pen=1.2)
    # -inf logits: masked tokens are no candidates; a row with 3 finite tokens and K = 6 returns 3 and three times "none"
    for mode, name in ((BEAM, "neg_inf_beam"), (GREEDY, "neg_inf_greedy")):
        sizes = [2, 1] if mode == BEAM else [1, 1, 1]
        x = grid_logits(3, 1000, 107)
        rng = np.random.default_rng(9)
        x[0, np.argsort(-x[0])[:3]] = -np.inf                  # the three best of row 0 are masked
        x[1, rng.permutation(1000)[:400]] = -np.inf
        keep = [17, 500, 999]
        few = np.full(1000, -np.inf, np.float32)
        few[keep] = [0.5, 2.0, -1.0]
        x[2] = few
        add(name, mode, 1000, sizes, x, 6)
    # seen bits at the word boundaries, on positive and on negative logits, penalty 1.2 and 1.0
    for mode, V, tag in ((GREEDY, 1000, "greedy"), (BEAM, 4099, "beam")):
        edge = [0, 31, 32, V - 1]
        x = grid_logits(2, V, 108)
        near = [1, 30, 33, V - 2]                              # their unseen neighbours: never penalised
        for r in range(2):
            top = x[r].max()
            x[r, edge] = top + np.array([3.0, 3.5, 4.0, 4.5], np.float32)
            x[r, near] = top + np.array([2.8, 3.3, 3.8, 4.3], np.float32)
        if mode == GREEDY:
            x[1] -= np.float32(x[1].max() + 0.25)              # row 1: every logit negative (the penalty multiplies)
        seen = np.zeros((2, V), bool)
        seen[:, edge] = True
        for pen in (1.2, 1.0):
            add(f"seen_edges_{tag}_pen{pen}", mode, V, [2] if mode == BEAM else [1, 1], x, 16, seen=seen, pen=pen)
    # exact ties: the same logit twice in a row; identical rows with equal beam scores
    x = grid_logits(3, 1000, 109)
    x[2] = x[0]
    best = np.argsort(-x[1])[:2]
    x[1, best[1]] = x[1, best[0]]
    x[0, 20], x[0, 700] = x[0].max(), x[0].max()
    x[2] = x[0]
    add("ties_beam", BEAM, 1000, [3], x, 12, bscore=[-0.1, -0.1233, -0.1])
    add("ties_greedy", GREEDY, 1000, [1, 1, 1], x, 5)
    return out


def selection_ref(case):
    """per group: (scores, tokens, parents) of the reference, each [kout]"""
    res, i = [], 0
    for nb in case["sizes"]:
        bs = case["bscore"][i:i + nb] if case["bscore"] is not None else None
        s = candidate_scores(case["logits"][i:i + nb], case["seen"][i:i + nb], case["mode"], case["pen"], bs)
        res.append(topk_ref(s, case["K"], case["kout"]) + (s,))
        i += nb
    return res
