"""The fused scoring head (csrc/head_score.hip, vr_op_head_score) restated in fp64, its error bound, the planted inputs of
tests/test_gpu_head_score.py, and a model of the kernel's tile / partial / combine structure that can be made to go wrong.

Per row m of A [M][K] and weight W [V][K] (both bf16):  x[m][v] = A[m] . W[v];  x_t = x[m][target[m]],
lse = log sum_{v < V} exp x[m][v],  top_x = max_v x[m][v],  top_id = the lowest v that attains it.

Inputs (`make_case`).  Three features of K are reserved: W[v][0] = 1 for every real column (a row's A[m][0] shifts all its
logits alike), W[v][1] and W[v][2] are zero but for two columns each (the exact-tie rows); the other features are
N(0, 1/16).  A PLANTED row is alpha * W[c] + small noise: its logit at c is alpha * |W[c]|^2 ~ alpha * K / 16, every other
one alpha * W[v] . W[c] ~ alpha * sqrt(K) / 16 * N(0, 1), so column c is the maximum by a margin far above the bound — for
every planted row, which the tests assert from the reference, not assume.  Tie rows hold exact small dyadic logits: their
argmax is defined by the tie rule alone."""
import numpy as np
import torch

TILE = 256
NAN_BITS = 0x7FC0


def pad_to(n, mult=TILE):
    return (n + mult - 1) // mult * mult


def head_score_ref(A, W, target):
    """A [M][K], W [V][K] (any float dtype holding bf16-representable values; torch, any device), target int [M] ->
    dict of numpy fp64 / int64 [M]: x_t, lse, top_x, top_id, second (the largest logit outside top_id), bound_t (the bound at
    the target), bound_top (at top_id), bound_max (max over v).  Computed in row blocks: no M x V x K tensor."""
    A64, W64 = A.to(torch.float64), W.to(torch.float64)
    M, K = A64.shape
    V = W64.shape[0]
    tgt = torch.as_tensor(np.asarray(target, dtype=np.int64), device=A64.device)
    out = {k: np.zeros(M, dtype=np.float64) for k in ("x_t", "lse", "top_x", "second", "bound_t", "bound_top", "bound_max")}
    out["top_id"] = np.zeros(M, dtype=np.int64)
    gamma = K * 2.0 ** -24
    step = max(1, min(M, (1 << 24) // max(V, 1)))
    for lo in range(0, M, step):
        a = A64[lo:lo + step]
        x = a @ W64.T
        b = (a.abs() @ W64.abs().T) * gamma
        r = torch.arange(a.shape[0], device=a.device)
        t = tgt[lo:lo + step]
        mx, am = x.max(dim=1)
        # torch.max may return any of several equal maxima: the contract wants the lowest index
        am = torch.where(x == mx[:, None], torch.arange(V, device=a.device)[None, :], V).min(dim=1).values
        x2 = x.clone()
        x2[r, am] = -np.inf
        sl = slice(lo, lo + a.shape[0])
        out["x_t"][sl] = x[r, t].cpu().numpy()
        out["lse"][sl] = (mx + torch.log(torch.exp(x - mx[:, None]).sum(dim=1))).cpu().numpy()
        out["top_x"][sl] = mx.cpu().numpy()
        out["top_id"][sl] = am.cpu().numpy()
        out["second"][sl] = x2.max(dim=1).values.cpu().numpy() if V > 1 else -np.inf
        out["bound_t"][sl] = b[r, t].cpu().numpy()
        out["bound_top"][sl] = b[r, am].cpu().numpy()
        out["bound_max"][sl] = b.max(dim=1).values.cpu().numpy()
    return out


def tiled_model(A, W, V, count_pad=False, drop_tile=None):
    """The kernel's structure in fp64 on a ZERO-padded weight: per 256-column tile a partial (max, sum exp(x - max)) over the
    tile's columns, merged by the (max, sum) rescale.  count_pad=True counts the pad columns of the last tile (logit 0, what
    deciding by value instead of by index would do); drop_tile=t loses that tile's partial.  -> lse fp64 [M]."""
    A64, W64 = A.to(torch.float64).cpu(), W.to(torch.float64).cpu()
    Vp = pad_to(V)
    Wp = torch.zeros((Vp, W64.shape[1]), dtype=torch.float64)
    Wp[:V] = W64[:V]
    x = (A64 @ Wp.T).numpy()
    M = x.shape[0]
    mx, sm = np.full(M, -np.inf), np.zeros(M)
    for t in range(Vp // TILE):
        if t == drop_tile:
            continue
        hi = (t + 1) * TILE if count_pad else min(V, (t + 1) * TILE)
        xt = x[:, t * TILE:hi]
        if xt.shape[1] == 0:
            continue
        pm = xt.max(axis=1)
        ps = np.exp(xt - pm[:, None]).sum(axis=1)
        nm = np.maximum(mx, pm)
        sm = sm * np.exp(mx - nm) + ps * np.exp(pm - nm)
        mx = nm
    return mx + np.log(sm)


# ---- the planted inputs -----------------------------------------------------------------------------------------------------
TIE_A = (300, 900)      # feature 1: an exact tie at the maximum across two vocab tiles (V = 1000: tiles 1 and 3)
TIE_B = (5, 200)        # feature 2: ... across two waves' column slabs of one tile


def planted_columns(V):
    """columns worth planting a maximum / aiming a target at: both ends of the first tile, the first column of the second,
    the last column, one inside the tail tile, one in the middle"""
    tail0 = (V - 1) // TILE * TILE
    cols = [0, 255, 256, V - 1, (tail0 + V - 1) // 2, V // 2]
    return [min(max(c, 0), V - 1) for c in cols]


def make_case(M, V, K, device, seed=0):
    """-> dict(A bf16 [pad256(M) + 8][K], W bf16 [pad256(V) + 8][K], target int32 [M], kinds: per row a label, M, V, K).
    Rows [M, pad256(M)) of A and [V, pad256(V)) of W hold large junk (readable, must not count); the 8 rows beyond are NaN
    canaries outside the extents the contract names."""
    g = torch.Generator(device=device).manual_seed(1000 * seed + M + 7 * V + 13 * K)
    Mp, Vp = pad_to(M), pad_to(V)
    W = torch.randn((V, K), generator=g, dtype=torch.float32, device=device) * 0.25
    W[:, 0] = 1.0
    W[:, 1] = 0.0
    W[:, 2] = 0.0
    has_ties = V > max(TIE_A + TIE_B) and K >= 8
    if has_ties:
        W[list(TIE_A), 1] = 2.0
        W[list(TIE_B), 2] = 2.0
    W = W.to(torch.bfloat16)
    cols = planted_columns(V)
    alpha = 32.0 / K                                   # a planted maximum near 2: alpha * K / 16
    noise = torch.randn((M, K), generator=g, dtype=torch.float32, device=device) * (0.02 / np.sqrt(K / 256.0))
    noise[:, :3] = 0.0
    A = torch.zeros((M, K), dtype=torch.float32, device=device)
    target = np.zeros(M, dtype=np.int32)
    kinds = []
    Wf = W.to(torch.float32)
    specials = ["all_negative", "spike80", "magnitude300", "all_equal", "tie_tiles", "tie_waves"] if (M >= 16 and has_ties) else []
    first_special = M - len(specials)
    for m in range(M):
        c = cols[m % len(cols)]
        # target: the argmax itself, a column of the same tile, a column of another tile — in turn
        how = (m + m // len(cols)) % 3
        t = c if how == 0 else ((c // TILE * TILE + (c + 17) % TILE) if how == 1 else cols[(m + 1) % len(cols)])
        target[m] = min(t, V - 1)
        kind = "planted"
        if m >= first_special:
            kind = specials[m - first_special]
        if kind == "planted":
            A[m] = alpha * Wf[c] + noise[m]
        elif kind == "all_negative":                   # every logit <= -20: pad columns (logit 0) must not count
            A[m] = alpha * Wf[c] + noise[m]
            A[m, 0] = -40.0
        elif kind == "spike80":                        # one logit 80 above the rest: lse == top_x
            A[m] = 64.0 * alpha * Wf[c]
        elif kind == "magnitude300":                   # logits of magnitude ~300
            A[m] = 160.0 * alpha * Wf[c]
            A[m, 0] = 8.0
        elif kind == "all_equal":                      # x = 1.5 everywhere: lse = 1.5 + log V, top_id 0
            A[m, 0] = 1.5
        elif kind == "tie_tiles":                      # x = 2 at TIE_A, 0 elsewhere
            A[m, 1] = 1.0
        elif kind == "tie_waves":
            A[m, 2] = 1.0
        kinds.append(kind)
    A = A.to(torch.bfloat16)
    Ap = torch.full((Mp + 8, K), 300.0, dtype=torch.bfloat16, device=device)
    Wp = torch.full((Vp + 8, K), 300.0, dtype=torch.bfloat16, device=device)
    Ap[:M] = A
    Wp[:V] = W
    nan = torch.tensor([NAN_BITS], dtype=torch.int32).to(torch.int16).view(torch.bfloat16).to(device)
    Ap[Mp:] = nan
    Wp[Vp:] = nan
    return {"A": Ap, "W": Wp, "target": target, "kinds": kinds, "M": M, "V": V, "K": K}
