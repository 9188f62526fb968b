"""Properties of the temporal history rule (tests/temporal_ref.py, the numpy restatement of k_temporal
and k_temporal_var) on the analytic scene: which pixels keep their history across a camera move,
near the origin and 1000 units from it, what identical cameras integrate, and the spatial variance
estimate against a brute-force loop.  Runs without a GPU."""
import numpy as np
import pytest

import temporal_ref as tr
from denoise_harness import pair_a
from mcrt.camera import make_camera

F = np.float32
SIZES = [(45, 37), (16, 16)]
MIN_FULL = {(45, 37): 1000, (16, 16): 100}
MIN_NONE = {(45, 37): 20, (16, 16): 3}


def guides(cam, offset, rng):
    sid, npl, depth = tr.scene_guides(cam, offset)
    ad = np.concatenate([rng.uniform(0.1, 1.0, depth.shape + (3,)).astype(F), depth[..., None]], -1)
    ad[sid == 0, :3] = 0.0
    return sid, npl, ad


def history_of(cam, offset, rng):
    sid, npl, ad = guides(cam, offset, rng)
    H, W = sid.shape
    colour = rng.uniform(0.1, 2.0, (H, W, 4)).astype(F)
    mu1 = rng.uniform(0.2, 2.0, (H, W)).astype(F)
    mom = np.stack([mu1, mu1 * mu1 + rng.uniform(0.0, 0.3, (H, W)).astype(F),
                    rng.integers(1, 41, (H, W)).astype(F), ad[..., 3]], -1).astype(F)
    return sid, (colour, mom, npl, cam)


def tap_ids(prev_sid, info):
    """Surface ids of the four history taps per pixel; -1 outside the image or when the pixel is
    not reprojected at all."""
    H, W = prev_sid.shape
    out = []
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = info["ix"] + i, info["iy"] + j
            inside = info["reprojected"] & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            out.append(np.where(inside, prev_sid[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], -1))
    return np.stack(out, -1)


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (1000.0, 1000.0, 1000.0)], ids=["origin", "far"])
@pytest.mark.parametrize("size", SIZES, ids=["45x37", "16x16"])
def test_history_follows_the_surface_across_a_camera_move(size, offset):
    W, H = size
    rng = np.random.default_rng(W)
    prev, cur = pair_a(W, H, offset)
    prev_sid, hist = history_of(prev, offset, rng)
    sid, npl, ad = guides(cur, offset, rng)
    img = rng.uniform(0.1, 2.0, (H, W, 4)).astype(F)
    info = {}
    colour, mom, nrm = tr.accumulate(img, npl, ad, cur, hist, info=info, **tr.DEFAULTS)
    ids = tap_ids(prev_sid, info)
    hit = sid > 0
    own = ids == sid[..., None]
    full = hit & own.all(-1)
    none = hit & ~own.any(-1)
    partial = hit & ~full & ~none
    print(f"{W}x{H} offset {offset[0]:g}: full-history {full.sum()}, no-history {none.sum()}, partial {partial.sum()}")
    assert full.sum() >= MIN_FULL[size] and none.sum() >= MIN_NONE[size]
    assert (info["valid_taps"][full] == 4).all()
    assert (info["valid_taps"][none] == 0).all()
    assert (mom[..., 2][none] == 1).all()
    np.testing.assert_array_equal(colour[none].view(np.uint32), img[none].view(np.uint32))
    l = tr.luminance(img)
    np.testing.assert_array_equal(mom[..., 0][none].view(np.uint32), l[none].view(np.uint32))
    # a pixel with history moved away from the current colour, and its length grew by one (capped)
    assert (mom[..., 2][full] > 1).all() and (mom[..., 2][full] <= 32).all()
    # misses never have history; the normal-plane and depth written are the current guides
    assert (mom[..., 2][~hit] == 1).all()
    np.testing.assert_array_equal(nrm, npl)
    np.testing.assert_array_equal(mom[..., 3], ad[..., 3])
    # no decision sits near a threshold: plane residuals of own-surface taps and of the others
    r = info["r"].astype(np.float64)
    zr = np.linalg.norm(r, axis=-1)
    pn = hist[2].astype(np.float64)
    res_own, res_other = [0.0], [np.inf]
    for t, (j, i) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        qx, qy = np.clip(info["ix"] + i, 0, W - 1), np.clip(info["iy"] + j, 0, H - 1)
        q = pn[qy, qx]
        res = np.abs((q[..., :3] * r).sum(-1) - q[..., 3]) / zr
        tapped = hit & (ids[..., t] > 0)
        res_own.append(res[tapped & own[..., t]].max(initial=0.0))
        # another surface with the same normal (square / wall) is told apart by the plane alone;
        # one with another normal (floor / wall: |dn|^2 = 2) by the normal test
        dn2 = ((npl[..., :3].astype(np.float64) - q[..., :3]) ** 2).sum(-1)
        other = tapped & ~own[..., t]
        assert ((dn2[other] < 1e-6) | (dn2[other] > 1.9)).all()
        res_other.append(res[other & (dn2 < 1e-6)].min(initial=np.inf))
    print(f"  plane residual / z: own surface <= {max(res_own):.2e}, other surfaces >= {min(res_other):.3f}")
    assert max(res_own) < 1e-3 and min(res_other) > 0.1   # the threshold is 0.01


@pytest.mark.parametrize("jitter", [(0.0, 0.0), (1.7, -1.3)], ids=["still", "jittered"])
@pytest.mark.parametrize("size", SIZES, ids=["45x37", "16x16"])
def test_identical_cameras_integrate_the_running_mean(size, jitter):
    W, H = size
    rng = np.random.default_rng(7)
    prev = make_camera((0.0, 1.0, -4.0), (0.0, 0.6, 0.0), W, H, fovy=50.0)
    cur = make_camera((0.0, 1.0, -4.0), (0.0, 0.6, 0.0), W, H, fovy=50.0, pixel_offset=jitter)
    _, npl0, ad0 = guides(prev, (0, 0, 0), rng)
    sid, npl, ad = guides(cur, (0, 0, 0), rng)
    hit = sid > 0
    if jitter == (0.0, 0.0):
        _, fx, fy, ok = tr.reproject(ad, cur, prev)
        assert ok[hit].all()
        ys, xs = np.mgrid[0:H, 0:W]
        d = max(np.abs(fx - xs)[hit].max(), np.abs(fy - ys)[hit].max())
        print(f"{W}x{H}: reprojected position within {d:.2e} pixel of the pixel")
        assert d <= 8e-6
    values = [0.7, 1.9, 0.4, 1.1, 2.6, 0.9]
    params = dict(tr.DEFAULTS, alpha=0.0, alpha_moments=0.0, max_history=64)
    history = None
    for k, val in enumerate(values, 1):
        img = np.full((H, W, 4), val, F)
        # frame 1 is written by the unjittered camera, the later ones through the jittered one
        g, a, cam = (npl0, ad0, prev) if k == 1 else (npl, ad, cur)
        info = {}
        colour, mom, nrm = tr.accumulate(img, g, a, cam, history, info=info, **params)
        history = (colour, mom, nrm, cam)
        if k == 1:
            continue
        assert info["have"][hit].all(), f"frame {k}: {(~info['have'][hit]).sum()} hit pixels lost their history"
        mean = np.mean(values[:k])
        assert np.abs(colour[..., :3][hit] / mean - 1).max() <= 1e-4
        assert np.abs(mom[..., 2][hit] - k).max() <= 1e-3
        lum_mean = np.mean([float(tr.luminance(np.full(3, v, F))) for v in values[:k]])
        assert np.abs(mom[..., 0][hit] / lum_mean - 1).max() <= 1e-4


@pytest.mark.parametrize("size", SIZES, ids=["45x37", "16x16"])
def test_spatial_variance_equals_a_brute_force_loop(size):
    W, H = size
    rng = np.random.default_rng(3)
    _, cur = pair_a(W, H)
    sid, npl, ad = guides(cur, (0, 0, 0), rng)
    mu1 = rng.uniform(0.2, 2.0, (H, W)).astype(F)
    mu2 = (mu1 * mu1 + rng.uniform(0.0, 0.3, (H, W)).astype(F)).astype(F)
    N = rng.integers(1, 9, (H, W)).astype(F)
    mom = np.stack([mu1, mu2, N, ad[..., 3]], -1).astype(F)
    got = tr.variance(mom, npl, min_history=4, normal_threshold=0.1, plane_threshold=0.01)
    want = np.zeros((H, W), F)
    for y in range(H):
        for x in range(W):
            if N[y, x] >= 4:
                want[y, x] = max(F(0), mu2[y, x] - mu1[y, x] * mu1[y, x])
                continue
            s1 = s2 = cnt = F(0)
            zp = ad[y, x, 3]
            for yy in range(max(0, y - 3), min(H, y + 4)):
                for xx in range(max(0, x - 3), min(W, x + 4)):
                    zq = ad[yy, xx, 3]
                    if (yy, xx) != (y, x):
                        if zp > 0:
                            dn = npl[y, x, :3] - npl[yy, xx, :3]
                            dd = npl[y, x, 3] - npl[yy, xx, 3]
                            t = F(0.01) * zp
                            if not (zq > 0 and (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2] <= F(0.1)
                                    and dd * dd <= t * t):
                                continue
                        elif zq > 0:
                            continue
                    s1, s2, cnt = F(s1 + mu1[yy, xx]), F(s2 + mu2[yy, xx]), F(cnt + F(1))
            m1, m2 = F(s1 / cnt), F(s2 / cnt)
            want[y, x] = F(max(F(0), F(m2 - F(m1 * m1))) * F(F(4) / N[y, x]))
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    spatial = N < 4
    assert spatial.sum() > 50 and (~spatial).sum() > 50
    # the estimate mixes only p's surface: on a hit pixel next to a miss it ignores the miss
    assert (sid == 0).any() and np.isfinite(got).all()
