"""The nucleus sampler's kept set (steps 1-5 of the definition at vr_chat_sample, include/visrag_hip.h) restated in numpy:
z in fp32 as the kernel computes it, then the masses, A_j / Z and the kept flags in fp64.  tests/test_cpu_chat_sample_ref.py
pins it on hand-worked rows and against transformers' warpers; tests/test_gpu_chat_sample.py compares the device with it.
Nothing here needs a GPU or the built library."""
import numpy as np

# |A_j / Z (device) - A_j / Z (fp64)| allowed at the nucleus edge.  Derived, not measured: a term that matters has
# |z - m| <= 24 (the rest sum to < V e^-24 ~ 5e-6 of the largest term); its fp32 argument (half an ulp of 24: 9.5e-7) and its
# fp32 exponential (a few ulp of 6e-8) carry a relative error of at most about 3e-6; A and Z each carry that much, their ratio
# twice that: 6e-6.  DELTA is three times that; the 2^-40 truncation of each of at most 122 753 terms adds < 1.2e-7.
DELTA = 2e-5


def tempered(logits, seen, penalty, temperature):
    """(s, z) fp32 [V]: the penalised logit (x * pen if x < 0 else x / pen on seen ids) and s * (1 / T), each operation rounded
    to fp32 as the device rounds it."""
    x = np.asarray(logits, np.float32)
    pen = np.float32(penalty)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(np.asarray(seen, bool), np.where(x < 0, x * pen, x / pen), x).astype(np.float32)
        inv_t = np.float32(1.0) / np.float32(temperature)
        z = (s * inv_t).astype(np.float32)
    return s, z


def f2ord(z):
    """the order-preserving 32-bit key of the device (-0 sorts below +0)"""
    b = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def candidate_order(z):
    """token ids of the candidates (z neither -inf nor NaN), by z descending, then token ascending"""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(z > -np.inf)
    key = f2ord(z[cand]).astype(np.int64)
    return cand[np.lexsort((cand, -key))]


def masses(z_sorted):
    """fp64 exp(z - m) of candidates in order (m = the first)"""
    z = np.asarray(z_sorted, np.float64)
    if z.size == 0:
        return z
    with np.errstate(invalid="ignore"):
        w = np.exp(z - z[0])
    w[np.asarray(z_sorted) == z_sorted[0]] = 1.0                 # (m = +inf: inf - inf)
    return w


def _first_k(w, top_k):
    C = len(w)
    K = C if top_k == 0 else min(int(top_k), C)
    w = np.asarray(w, np.float64)[:K]
    A = np.concatenate([[0.0], np.cumsum(w)[:-1]]) if K else np.zeros(0)
    return K, A, float(w.sum())


def kept_count(w, top_k, top_p):
    """n_kept for masses w in candidate order: j < K and (top_p == 1 or A_j < top_p * Z)"""
    K, A, Z = _first_k(w, top_k)
    if K == 0 or top_p == 1:
        return K
    return int(np.count_nonzero(A < top_p * Z))


def kept_interval(w, top_k, top_p, delta=DELTA):
    """(lo, hi, edge): #(j < K : A_j / Z < top_p - delta), #(... < top_p + delta), and the reference's own distance
    min_j |A_j / Z - top_p| (inf when top_p == 1)"""
    K, A, Z = _first_k(w, top_k)
    if K == 0 or top_p == 1:
        return K, K, np.inf
    r = A / Z
    return int(np.count_nonzero(r < top_p - delta)), int(np.count_nonzero(r < top_p + delta)), float(np.abs(r - top_p).min())


class Row:
    """One row's order, computed once and shared by every (top_k, top_p) asked of it."""

    def __init__(self, logits, seen=None, penalty=1.0, temperature=1.0):
        logits = np.asarray(logits, np.float32)
        seen = np.zeros(logits.shape, bool) if seen is None else np.asarray(seen, bool)
        self.s, self.z = tempered(logits, seen, penalty, temperature)
        self.order = candidate_order(self.z)
        self.w = masses(self.z[self.order])
        self.w.setflags(write=False)
        self.order.setflags(write=False)

    @property
    def candidates(self):
        return len(self.order)

    def n_kept(self, top_k, top_p):
        return kept_count(self.w, top_k, top_p)

    def interval(self, top_k, top_p, delta=DELTA):
        return kept_interval(self.w, top_k, top_p, delta)

    def kept(self, top_k, top_p):
        """token ids of the kept set, in order"""
        return self.order[:self.n_kept(top_k, top_p)]

    def cut_token(self, n_kept):
        return int(self.order[n_kept - 1]) if n_kept else -1

    def probs(self, top_k, top_p):
        """(tokens, probabilities) of the distribution the draw follows: the kept masses renormalised"""
        n = self.n_kept(top_k, top_p)
        return self.order[:n], self.w[:n] / self.w[:n].sum()
