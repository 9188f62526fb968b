"""The numpy model of adaptive sampling (tests/adaptive_ref.py) against itself and against
atrous_ref: what the GPU tests of test_gpu_adaptive.py then hold the kernels to."""
import numpy as np
import pytest

import adaptive_ref as ad
import atrous_ref as ar

F = np.float32


def _moments(W, H, n, seed):
    """Random moments of n samples with a population variance of 0.1 .. 0.5 at means of 0.5 .. 3.
    m2 / n - mean^2 cancels: the float32 rounding of its two terms (about 3 * 2^-24 * mean^2) is
    amplified by mean^2 / variance <= 90 into v, so Sv may be off by about 2e-5 relative if every
    pixel erred the same way, and err = sqrt(..) by half of that; draws with a variance near zero
    would test the cancellation, not the sums."""
    rng = np.random.default_rng(seed)
    m1 = (n * rng.uniform(0.5, 3.0, (H, W))).astype(F)
    m2 = (m1 * m1 / n + n * rng.uniform(0.1, 0.5, (H, W))).astype(F)
    return np.stack([m1, m2], -1).astype(F)


@pytest.mark.parametrize("W,H", [(45, 37), (16, 16), (64, 48), (264, 256)])
def test_float32_tile_error_against_float64(W, H):
    """rtol 1e-5: a 64-term sum of non-negative float32 terms in another order differs by at most
    63 * 2^-24 = 3.8e-6 relative, the few operations after it add about an ulp each, and the
    per-pixel terms stay within _moments' bound."""
    tx, ty = ad.tile_grid(W, H)
    rng = np.random.default_rng(W)
    counts = rng.integers(2, 40, tx * ty).astype(np.uint32)
    n = np.repeat(np.repeat(counts.reshape(ty, tx), 8, 0), 8, 1)[:H, :W]
    mom = _moments(W, H, n.astype(np.float64), seed=H)
    e32 = ad.tile_error(mom, counts, W, H, 1e-3, F)
    e64 = ad.tile_error(mom, counts, W, H, 1e-3, np.float64)
    assert e32.dtype == F and e32.shape == (tx * ty,) and np.isfinite(e32).all() and (e32 > 0).all()
    np.testing.assert_allclose(e32, e64, rtol=1e-5, atol=0)


def test_tile_error_edges():
    W, H = 45, 37
    tx, ty = ad.tile_grid(W, H)
    mom = _moments(W, H, 6.0, seed=1)
    mom[:8, :8] = 0.0                                   # tile 0: all zero -> 0 / floor = 0
    mom[8:16, :8, 1] = mom[8:16, :8, 0] ** 2 / F(6)      # tile tx: (nearly) zero variance
    counts = np.full(tx * ty, 6, np.uint32)
    counts[1], counts[2] = 0, 1                          # not judged yet
    e = ad.tile_error(mom, counts, W, H, 1e-3)
    assert e[0] == 0 and np.isposinf(e[1]) and np.isposinf(e[2]) and not np.isnan(e).any()
    assert e[tx] < 1e-3
    # the partial last column and row: c counts the pixels inside the image only
    lanes, inside = ad.tile_lanes(mom[..., 0], W, H)
    assert inside.sum(1).reshape(ty, tx)[-1, -1] == (W - 8 * (tx - 1)) * (H - 8 * (ty - 1)) == 25
    assert (lanes[~inside] == 0).all()
    # a constant tile of mean m, variance v per pixel: err = sqrt(v / (n - 1)) / (m + floor)
    flat = np.zeros((8, 8, 2), F)
    flat[..., 0], flat[..., 1] = 4 * 2.0, 4 * (2.0 * 2.0 + 1.0)
    got = ad.tile_error(flat, np.array([4], np.uint32), 8, 8, 1e-3)[0]
    assert abs(got - np.sqrt(1.0 / 3.0) / 2.001) < 1e-6


def test_step_with_every_tile_listed_is_the_plain_accumulate():
    W, H = 45, 37
    tx, ty = ad.tile_grid(W, H)
    rng = np.random.default_rng(3)
    frames = [(10.0 ** rng.uniform(-3, 3.5, (H, W, 4))).astype(F) for _ in range(7)]   # some above the clamp
    frames[2][5, 7] = np.nan
    every = np.arange(tx * ty)
    s = ad.step(ad.new_state(W, H), frames[:1], every)
    s = ad.step(s, frames[1:4], every)       # a batch of 3
    s = ad.step(s, frames[4:], every)
    want = ar.accumulate_moments(frames)
    np.testing.assert_array_equal(s["mom"].view(np.uint32), want.view(np.uint32))
    ws = np.zeros((H, W, 4), F)
    for fr in frames:
        ws = ws + ar.cl_clamp(fr, 0, 1000)
    np.testing.assert_array_equal(s["wsum"].view(np.uint32), ws.view(np.uint32))
    assert (s["wts"] == 7).all() and (s["counts"] == 7).all()


def test_step_touches_only_the_listed_tiles():
    W, H = 24, 16
    rng = np.random.default_rng(4)
    frames = [rng.uniform(0, 2, (H, W, 4)).astype(F) for _ in range(3)]
    s0 = ad.step(ad.new_state(W, H), frames[:1], np.arange(6))
    s1 = ad.step(s0, frames[1:], [1, 5])
    m = ad.tile_mask([1, 5], W, H)
    assert m.sum() == 128 and m[0, 8] and m[8, 16] and not m[0, 0]
    for k in ("wsum", "wts", "mom"):
        np.testing.assert_array_equal(s1[k][~m], s0[k][~m])
        assert (s1[k][m] != s0[k][m]).any()
    assert list(s1["counts"]) == [1, 3, 1, 1, 1, 3]
    assert (s1["wts"][m] == 3).all()
    assert ad.step(s1, frames, [])["counts"].tolist() == s1["counts"].tolist()
    var = ad.prepare_var(s1["mom"], s1["counts"], W, H)
    assert (var[~m] == 1).all() and (var[m] != 1).any()   # n = 1: no variance yet
    c, want = ar.prepare(np.zeros((H, W, 4), F), None, s1["mom"], 3)
    np.testing.assert_array_equal(var[m], want[m])


def test_active_rule_and_list_order():
    err = np.array([0.5, 0.1, np.inf, 0.3, 0.0, 0.2, 0.2000001, 0.9], F)
    counts = np.array([8, 8, 1, 7, 8, 8, 8, 32])
    p = dict(error_threshold=0.2, min_samples=8, max_samples=32)
    a = ad.active(err, counts, **p)
    #                 above  below  unjudged  unjudged  zero   equal  just above  capped
    assert a.tolist() == [True, False, True, True, False, False, True, False]
    ids = ad.active_list(err, counts, **p)
    assert ids.dtype == np.uint32 and ids.tolist() == [0, 2, 3, 6]
    assert (np.diff(ids.astype(np.int64)) > 0).all()
    assert ad.active_list(err, counts, error_threshold=0.2, min_samples=8).tolist() == [0, 2, 3, 6, 7]   # no cap
    assert ad.active(err, counts, error_threshold=0.0, min_samples=33).all()           # nobody judged yet
    assert not ad.active(err, np.full(8, 6), error_threshold=0.0, min_samples=2, max_samples=6).any()


def test_gap_threshold():
    e = np.array([0.0, 0.0, 0.1, 0.2, 0.3, 0.6, 0.7, 5.0])
    thr, rel, below, above = ad.gap_threshold(e)
    assert thr == pytest.approx(0.45) and rel == pytest.approx(0.3 / 0.45) and (below, above) == (5, 3)
