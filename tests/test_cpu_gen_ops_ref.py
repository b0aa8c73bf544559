"""The restatements of tests/gen_ops_ref.py pinned against the oracles that are already trusted here (oracle/qwen_gen_oracle.py,
oracle/qwen_vision_oracle.py), the float32-restatement distance the rotation bar of tests/test_gpu_gen_ops.py rests on (printed,
and bounded so that a drift of the yardstick shows), the sampling noise over all 2^24 draws, and the conditions the case tables
have to meet.  No GPU, no library."""
import numpy as np
import pytest
import torch

from oracle import qwen_gen_oracle as G
from oracle import qwen_vision_oracle as V
from tests import chat_ref as C
from tests import gen_ops_ref as R


# -------------------------------------------------------------------------------- M-RoPE ---
def test_mrope_angles_and_sections_are_the_oracles():
    cfg = G.QwenGenConfig()
    assert tuple(cfg.mrope_section) == R.MROPE_SECTIONS and cfg.head_dim == 128 and cfg.rope_theta == R.MROPE_THETA
    inv_t = (1.0 / (cfg.rope_theta ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))).numpy()
    np.testing.assert_allclose(R.mrope_inv_freq(), inv_t, rtol=2.5e-7, atol=0)           # numpy's float32 power and reciprocal: two ulps at most
    pos3 = np.array(R.MROPE_POS, np.int64).T                                             # [3][6]
    cos, sin = G.mrope_cos_sin(cfg, torch.from_numpy(pos3))
    ang = R.mrope_angles(pos3, inv_t)
    assert ang.dtype == np.float32
    # the oracle's float32 cos / sin of the SAME float32 angles: an ulp or two of their float32 evaluation
    np.testing.assert_allclose(np.cos(ang.astype(np.float64)), cos[:, :64].numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose(np.sin(ang.astype(np.float64)), sin[:, :64].numpy(), rtol=0, atol=2e-7)
    np.testing.assert_array_equal(cos[:, :64].numpy(), cos[:, 64:].numpy())
    # section choice: with components far apart every pair's angle names its component
    far = ang[0] / inv_t
    np.testing.assert_allclose(far, np.array(R.MROPE_POS[0], np.float32)[R.mrope_section_of()], rtol=2e-7)
    assert R.mrope_section_of().tolist() == [0] * 16 + [1] * 24 + [2] * 24
    # a float64 angle is NOT the definition: at 32767 its cosine differs from the float32 angle's by 2.6e-4, fifty times the margin
    # of the rotation bar — that difference is not the kernel's error
    a64 = 32767.0 * inv_t.astype(np.float64)
    assert np.abs(np.cos(a64) - np.cos(ang[4].astype(np.float64))).max() > 50.0 * R.ROT_MARGIN


def test_mrope_reference_is_the_oracles_rotation():
    cfg = G.QwenGenConfig()
    H, KV, T = 4, 2, 5
    x = R.mrope_rows_input(H, KV, T)
    pos3 = R.mrope_positions(T, 0)
    inv = R.mrope_inv_freq()
    ref = R.mrope_ref(x, pos3, inv, H, KV)
    ang = torch.from_numpy(R.mrope_angles(pos3[:, :T], inv).astype(np.float64))
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos()[:, None, :], emb.sin()[:, None, :]
    qk = torch.from_numpy(x[:, :(H + KV) * 128].astype(np.float64)).view(T, H + KV, 128)
    want = (qk * cos + G.rotate_half(qk) * sin).reshape(T, -1).numpy()
    np.testing.assert_allclose(ref[:, :(H + KV) * 128], want, rtol=1e-14, atol=1e-15)
    np.testing.assert_array_equal(ref[:, (H + KV) * 128:], x[:, (H + KV) * 128:].astype(np.float64))      # v: copied
    np.testing.assert_array_equal(ref[1], x[1].astype(np.float64))                                        # position 0: untouched
    # the bar sees what it is for: the height and width sections swapped, or the neighbouring pair's frequency
    swapped = R.mrope_ref(x, pos3[[0, 2, 1]], inv, H, KV)
    shifted = R.mrope_ref(x, pos3, np.roll(inv, 1), H, KV)
    for bad in (swapped, shifted):                                                                        # (row 0: components far apart)
        worst, same = R.rotation_check(R.bf16_round(bad[:1, :(H + KV) * 128].astype(np.float32)), ref[:1, :(H + KV) * 128])
        assert worst > 100.0 and same < 0.5
    worst, same = R.rotation_check(R.bf16_round(ref.astype(np.float32)), ref)
    assert worst <= 0.0 and same == 1.0


def test_plane_sum_is_sequential_float32():
    parts, bias = R.mrope_planes_input(3, 1, 3, 17)
    acc = bias.astype(np.float32).copy()
    acc = np.broadcast_to(acc, parts.shape[1:]).copy()
    for p in parts:
        acc += p
    np.testing.assert_array_equal(R.plane_sum_f32(parts, bias), acc)
    # the order matters at these sizes: a pairwise sum differs in some bits (the kernel's order is part of the contract)
    assert (R.plane_sum_f32(parts[::-1], bias) != R.plane_sum_f32(parts, bias)).any()
    np.testing.assert_array_equal(R.plane_sum_f32(parts[:1]), parts[0])


def test_rotation_margin_is_the_float32_restatements_distance():
    """ROT_F32_DIST bounds max |float32 restatement - float64 reference| over every case of the two rotation tests"""
    inv = R.mrope_inv_freq()
    worst_m, big_m = 0.0, 0.0
    for H, KV in R.MROPE_HEADS:
        for T in R.MROPE_T:
            for first in range(len(R.MROPE_POS)):
                x, pos3 = R.mrope_rows_input(H, KV, T), R.mrope_positions(T, first)
                d = np.abs(R.mrope_ref(x, pos3, inv, H, KV, dtype=np.float32).astype(np.float64) - R.mrope_ref(x, pos3, inv, H, KV))
                worst_m, big_m = max(worst_m, float(d.max())), max(big_m, float(np.abs(x).max()))
    for n_parts in R.MROPE_PARTS:
        for H, KV, T in ((3, 1, 3), (4, 2, 5)):
            parts, bias = R.mrope_planes_input(H, KV, T, n_parts)
            for b in (None, bias):
                x, pos3 = R.plane_sum_f32(parts, b), R.mrope_positions(T, n_parts)
                d = np.abs(R.mrope_ref(x, pos3, inv, H, KV, dtype=np.float32).astype(np.float64) - R.mrope_ref(x, pos3, inv, H, KV))
                worst_m, big_m = max(worst_m, float(d.max())), max(big_m, float(np.abs(x).max()))
    worst_v, big_v = 0.0, 0.0
    for hh, heads, T in R.ROPE2D_CASES:
        x, (ph, pw), f = R.rope2d_input(hh, heads, T), R.rope2d_positions(T), R.rope2d_freq(hh)
        d = np.abs(R.rope2d_ref(x, hh, 2 * heads, ph, pw, hh // 2, f, np.float32).astype(np.float64) - R.rope2d_ref(x, hh, 2 * heads, ph, pw, hh // 2, f))
        worst_v, big_v = max(worst_v, float(d.max())), max(big_v, float(np.abs(x).max()))
    print(f"float32 restatement - float64: M-RoPE {worst_m:.3g} (|x| <= {big_m:.3g}), vision {worst_v:.3g} (|x| <= {big_v:.3g}); "
          f"ROT_F32_DIST {R.ROT_F32_DIST:.3g}")
    assert max(worst_m, worst_v) <= R.ROT_F32_DIST <= 2.0 * max(worst_m, worst_v)
    assert R.ROT_MARGIN == 4.0 * R.ROT_F32_DIST and R.ROT_MARGIN < 0.01 * 0.5 * 2.0 ** -8     # far below half a bf16 ulp at 1


# ----------------------------------------------------------------------- vision 2-D RoPE ---
@pytest.mark.parametrize("cfg", [V.tiny_vision_config(), V.hd80_vision_config()], ids=["tiny_hd40", "hd80"])
def test_rope2d_reference_is_the_vision_oracles_rotary(cfg):
    hd = cfg.head_dim
    hh = hd // 2
    grids = [(1, 4, 6), (1, 2, 2)]
    orc = V.QwenVisionOracle(cfg, V.synth_vision_weights(cfg))
    cos, sin = orc.rotary(grids)
    pos = V.position_hw(grids, cfg.spatial_merge_size).numpy()
    T = pos.shape[0]
    f = R.rope2d_freq(hh)
    inv_t = (1.0 / (10000.0 ** (torch.arange(0, hd // 2, 2, dtype=torch.float32) / (hd // 2)))).numpy()
    np.testing.assert_allclose(f[:hh], np.concatenate([inv_t, inv_t]), rtol=2.5e-7, atol=0)
    assert (f[hh:] == 0).all()
    f_t = np.zeros(64, np.float32)
    f_t[:hh] = np.concatenate([inv_t, inv_t])
    x = R.rope2d_input(hh, 2, T)[:, :2 * hd].copy()                                    # two head slots
    ref = R.rope2d_ref(x, hh, 2, pos[:, 0], pos[:, 1], hh // 2, f_t)
    c64, s64 = cos.double()[:, None, :], sin.double()[:, None, :]
    xt = torch.from_numpy(x.astype(np.float64)).view(T, 2, hd)
    want = (xt * c64 + V._rot_half(xt) * s64).reshape(T, -1).numpy()
    # (the oracle's cos / sin are float32: 1e-7 of an ulp-sized difference times |x| <= 5.3)
    np.testing.assert_allclose(ref, want, rtol=0, atol=2e-6)
    # h and w swapped is a different rotation wherever pos_h != pos_w
    swapped = R.rope2d_ref(x, hh, 2, pos[:, 1], pos[:, 0], hh // 2, f_t)
    rows = pos[:, 0] != pos[:, 1]
    assert rows.any() and np.abs(swapped[rows] - ref[rows]).max() > 0.5


def test_rope2d_cases_meet_their_conditions():
    for hh, heads, T in R.ROPE2D_CASES:
        assert (T * 2 * heads) % 4 != 0 and hh <= 64
        ph, pw = R.rope2d_positions(T)
        assert (ph != pw).all()
    assert {c[0] for c in R.ROPE2D_CASES} == {16, 40, 64}


# -------------------------------------------------------------------------- decode_begin ---
def test_kv_split_rule():
    for L in list(range(1, 4200)) + list(R.KV_L) + [32767, 32769, 100000]:
        splits, chunk = R.gen_kv_split(L)
        assert (splits, chunk) == R.kv_split_direct(L), L
        cu = [min(L, i * chunk) for i in range(R.GEN_ATT_SPLITS + 1)]
        assert chunk % 64 == 0 and 1 <= splits <= R.GEN_ATT_SPLITS
        assert cu[0] == 0 and cu[splits] == L and cu[-1] == L                            # the ranges tile [0, L)
        assert all(cu[i] < cu[i + 1] for i in range(splits)) and all(cu[i] == L for i in range(splits, R.GEN_ATT_SPLITS + 1))
    st = np.arange(100, 100 + R.STATE_WORDS, dtype=np.int32)
    st[R.ST_LEN] = 2048
    out = R.decode_begin_ref(st, 7)
    assert out[R.ST_SPLITS] == 11 and out[R.ST_CU_Q + 16] == 112 and out[R.ST_CU_KV + 1] == 192 and out[R.ST_CU_KV + 16] == 2049
    keep = [R.ST_TOKEN, 1, 2, 3, R.ST_LEN, R.ST_STEP, 7]
    np.testing.assert_array_equal(out[keep], st[keep])
    assert R.ST_CU_KV + R.GEN_ATT_SPLITS + 1 == R.STATE_WORDS


# ------------------------------------------------------------------ mark_seen, the penalty ---
def test_mark_seen_reference_is_seen_words():
    Vv = 1000
    ids = [-1, Vv, 0, 31, 32, Vv - 1, 5, 5, 31, 640]
    seen = np.zeros((1, Vv), bool)
    seen[0, [i for i in ids if 0 <= i < Vv]] = True
    np.testing.assert_array_equal(R.mark_seen_ref(np.zeros(32, np.uint32), ids, Vv), C.seen_words(seen)[0])
    before = np.full(32, 0x80000001, np.uint32)
    np.testing.assert_array_equal(R.mark_seen_ref(before, ids, Vv), C.seen_words(seen)[0] | before)


@pytest.mark.parametrize("Vv", R.SAMPLE_V)
def test_greedy_cases_and_the_penalty(Vv):
    cases = R.greedy_cases(Vv)
    for name, (x, seen) in cases.items():
        assert seen[[i for i in (0, 31, 32, Vv - 1) if i < Vv]].all() and seen.sum() == len({i for i in (0, 31, 32, Vv - 1) if i < Vv})
        pen = R.penalised(x, seen, R.SAMPLE_PENALTY)
        want = G.apply_repetition_penalty(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(np.flatnonzero(seen)), R.SAMPLE_PENALTY)
        np.testing.assert_array_equal(pen, want.numpy())
        # the float32 restatement picks the same token: the winner is decided by 1e-3 or by an exact, planted tie
        best = R.greedy_ref(x, seen)
        assert int(np.argmax(R.penalised(x, seen, R.SAMPLE_PENALTY, np.float32))) == best
        others = np.delete(pen, best)
        if name == "ties" and Vv >= 3:
            assert (pen == pen[best]).sum() == 2 and best == int(np.flatnonzero(pen == pen[best])[0])
            assert x[np.flatnonzero(seen)[0]] == x[best] and pen[np.flatnonzero(seen)[0]] < pen[best] - 1e-3
            others = pen[pen != pen[best]]
        if others.size:
            assert pen[best] - others.max() >= 1e-3, (Vv, name)
    if Vv > 33:
        x, seen = cases["seen_on_top"]
        assert seen[int(np.argmax(x))] and not seen[R.greedy_ref(x, seen)]              # without the penalty a seen id would win
        x, seen = cases["seen_zero"]
        assert x[R.greedy_ref(x, seen)] == 0.0 and seen[R.greedy_ref(x, seen)] and (np.delete(x, R.greedy_ref(x, seen)) < 0).all()
        x, seen = cases["all_negative"]
        assert (x < 0).all() and not seen[R.greedy_ref(x, seen)]


# --------------------------------------------------------------------------------- noise ---
def test_uniform_lies_inside_the_unit_interval_for_every_draw():
    draws = np.arange(1 << 24, dtype=np.uint32)
    old, new = R.uniform_old(draws), R.uniform_new(draws)
    assert old.dtype == new.dtype == np.float32
    assert (new > 0).all() and (new < 1).all()
    diff = np.flatnonzero(old.view(np.uint32) != new.view(np.uint32))
    assert diff.tolist() == [R.DEFECTIVE_DRAW]                                           # every other draw keeps its bits
    assert old[R.DEFECTIVE_DRAW] == 1.0 and new[R.DEFECTIVE_DRAW] == R.U_MAX == np.nextafter(np.float32(1), np.float32(0))
    g_old = R.gumbel(old.astype(np.float64))
    assert np.isinf(g_old[R.DEFECTIVE_DRAW]) and np.isfinite(np.delete(g_old, R.DEFECTIVE_DRAW)).all()
    g = R.gumbel(new.astype(np.float64))
    print(f"noise over all 2^24 draws: [{g.min():.4f}, {g.max():.4f}]")
    assert np.isfinite(g).all() and -2.86 < g.min() and g.max() < 16.65
    # the same in float32 (numpy's log, not the device's): finite as well
    assert np.isfinite(R.gumbel(new, np.float32)).all()


def test_noise_hash_known_answers_and_search():
    for seed, step, idx in R.KNOWN_DEFECTIVE:
        assert int(R.noise_draw(seed, step, idx)) == R.DEFECTIVE_DRAW
    # scalar python integers, independently of numpy's wrap-around
    def draw(seed, step, idx):
        x = (seed + 0x9E3779B97F4A7C15 * ((step << 32) | idx)) & R.MASK64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & R.MASK64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & R.MASK64
        return (x ^ (x >> 31)) >> 40
    g = np.random.default_rng(1)
    for seed, step, idx in zip(g.integers(0, 2 ** 63, 200), g.integers(0, 2 ** 31, 200), g.integers(0, 152064, 200)):
        assert int(R.noise_draw(int(seed), int(step), int(idx))) == draw(int(seed), int(step), int(idx))
    assert int(R.noise_draw(2 ** 64 - 1, 3, 5)) == draw(2 ** 64 - 1, 3, 5)
    found = R.find_defective(0, 4096, 8192)
    assert (0, 5314, 2909) in found and (0, 6688, 947) in found
    assert R.find_defective(11, 4096, 1400, chunk=700) == [(11, 1314, 955)]
    trip = R.defective_triples()
    assert set(R.KNOWN_DEFECTIVE) <= set(trip) and all(int(R.noise_draw(s, t, i)) == R.DEFECTIVE_DRAW and i < 4096 for s, t, i in trip)
    for s, t, i in trip:
        x, D = R.defective_logits(4096, i)
        assert D != i and x[D] == 30.0 and x[i] == 0.0 and int(R.noise_draw(s, t, D)) != R.DEFECTIVE_DRAW
        # the pick of the restated sampler: D with the new map, the defective token with the old one
        draws = R.noise_draw(s, t, np.arange(4096, dtype=np.uint64))
        assert int(np.argmax(x + R.gumbel(R.uniform_new(draws)))) == D
        assert int(np.argmax(x + R.gumbel(R.uniform_old(draws)))) == i


def test_restated_sampler_draws_from_the_softmax():
    """the hash's noise through the new map is Gumbel noise: 4096 steps among the planted top 8 pass the chi-square test
    against their own temperature and fail it against the other (what the GPU test asks of the kernel)"""
    x, ids = C.sampling_logits()
    x = x.astype(np.float64)
    rest = np.ones(x.size, bool)
    rest[ids] = False
    x[rest] -= R.SAMPLE_TAIL_DROP
    crit = C.chi2_critical(C.SAMPLE_TOPK - 1, 1e-6)
    idx = np.arange(x.size, dtype=np.uint64)[None, :]
    steps = np.arange(C.SAMPLE_DRAWS, dtype=np.uint64)[:, None]
    for T, other in (C.SAMPLE_TEMPS, C.SAMPLE_TEMPS[::-1]):
        tok, p = C.sampler_probs(x, C.SAMPLE_TOPK, T)
        _, p_other = C.sampler_probs(x, C.SAMPLE_TOPK, other)
        assert set(tok.tolist()) == set(ids.tolist()) and (C.SAMPLE_DRAWS * p).min() >= 40.0
        # the tail cannot be drawn: its best scaled logit plus the largest noise stays below the top 8's worst with the smallest
        assert x[rest].max() / T + 16.65 < x[ids].min() / T - 2.86
        for seed in C.SAMPLE_SEEDS:
            g = R.gumbel(R.uniform_new(R.noise_draw(seed, steps, idx)))
            picks = np.argmax(x[None] / T + g, axis=1)
            assert np.isin(picks, ids).all()
            counts = np.array([(picks == t).sum() for t in tok])
            own, cross = C.chi2_stat(counts, p), C.chi2_stat(counts, p_other)
            print(f"restated sampler T={T} seed={seed}: chi2 own {own:.1f}, other {cross:.1f}, critical {crit:.1f}")
            assert own < crit < cross


# ---------------------------------------------------------------------------- row movers ---
def test_patch_rows_reference_is_patchify_of_the_normalised_page():
    cfg = V.QwenVisionConfig()
    assert (cfg.patch_size, cfg.temporal_patch_size, cfg.patch_dim) == (R.PATCH_P, R.PATCH_TP, R.PATCH_DIM)
    pages = R.patch_pages()
    img, ph, pw = R.patch_list()
    got = R.patch_rows_ref(pages, img, ph, pw)
    assert (got[:, R.PATCH_DIM:] == 0).all() and R.PATCH_LD > R.PATCH_DIM
    m = cfg.spatial_merge_size
    for i, page in enumerate(pages):
        chw = np.stack([R.normalise_px(page[:, :, c], c) for c in range(3)])             # float32 [3][H][W]
        rows, (_, gh, gw) = V.patchify(torch.from_numpy(chw), cfg)
        hw = V.position_hw([(1, gh, gw)], m).numpy()                                     # the (h, w) of patchify's rows
        for r, (y, x) in enumerate(hw):
            mine = np.flatnonzero((img == i) & (ph == y) & (pw == x))
            assert mine.size == 1                                                        # every patch of the page is in the list once
            np.testing.assert_array_equal(got[mine[0], :R.PATCH_DIM], R.bf16_bits(rows[r].numpy()))
        # ... the last row and the last column of the page among them
        assert ((img == i) & (ph == gh - 1)).any() and ((img == i) & (pw == gw - 1)).any()
    # the temporal copies are identical
    v = got[:, :R.PATCH_DIM].reshape(len(img), 3, R.PATCH_TP, -1)
    np.testing.assert_array_equal(v[:, :, 0], v[:, :, 1])
    assert R.PATCH_PAGES[0][1] != R.PATCH_PAGES[1][1] and len(set(R.PATCH_MEAN)) == 3 and len(set(R.PATCH_STD)) == 3


def test_patch_normalisation_bits_do_not_depend_on_contraction():
    """px * (1 / 255) - mean may be contracted into one fused operation by the compiler: for every pixel value and channel the
    bf16 bits are the same either way, and within half a bf16 ulp (+ 1e-6) of the float64 value"""
    px = np.arange(256)
    for c in range(3):
        a, b = R.normalise_px(px, c), R.normalise_px(px, c, fused=True)
        np.testing.assert_array_equal(R.bf16_bits(a), R.bf16_bits(b))
        ref = R.normalise_px(px, c, np.float64)
        assert (np.abs(R.bf16_round(a).astype(np.float64) - ref) <= 0.5 * R.ulp_bf16(ref) + 1e-6).all()


def test_row_mover_tables():
    assert R.ROWS_DIM % 256 and R.ROWS_LD_SCATTER > R.ROWS_DIM and R.ROWS_LD_GATHER > R.ROWS_DIM
    assert len(set(R.ROWS_IDX)) == len(R.ROWS_IDX) and max(R.ROWS_IDX) < R.ROWS_SRC and list(R.ROWS_IDX) != sorted(R.ROWS_IDX)
