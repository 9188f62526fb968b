"""Properties of the temporal history rule with per-object motion (tests/temporal_ref.py's numpy
restatement of k_temporal given motion planes) on tests/temporal_motion_ref.py's analytic scene
with one moving rectangle: what a slide within its own plane, a translation out of it and a turn keep, what the static rule
(no motion planes) does with the same input, and what restarts.  Static camera, 45x37, at the
origin and with everything 1000 units away.  Runs without a GPU.

"Interior" below is the set of current rectangle pixels whose four motion-reprojected history taps
carried the rectangle in the previous frame.  On this planar scene the plane test is exact up to
rounding, so every interior pixel must keep four valid taps.
"""
import numpy as np
import pytest

import temporal_motion_ref as mr
import temporal_ref as tr
from mcrt.camera import make_camera

F = np.float32
W, H = 45, 37
OFFSETS = [(0.0, 0.0, 0.0), (1000.0, 1000.0, 1000.0)]
IDS = ["origin", "far"]
# the pixel footprint at the rectangle: 4.5 units away, fovy 50 degrees over 37 rows = 0.113 units
SLIDE = 0.23                                   # about two pixels along x
RAMP = np.array([1.0, 0.8, 0.5])               # colour = RAMP[0] + RAMP[1] * u + RAMP[2] * v in object space
N_HIST = 4.0                                   # history length of every previous pixel
MOVES = {"slide": mr.pose((SLIDE, 0.0, 0.0)), "out_of_plane": mr.pose((0.0, 0.0, -0.3)),
         "turn": mr.pose(turn_deg=20.0), "lift": mr.pose((0.0, 0.25, 0.0))}
PARAMS = dict(tr.DEFAULTS)


def camera(offset):
    o = np.asarray(offset, np.float64)
    return make_camera(tuple(o + (0.0, 1.0, -4.0)), tuple(o + (0.0, 0.6, 0.0)), W, H, fovy=50.0)


def ramp(uv):
    return (RAMP[0] + RAMP[1] * uv[..., 0]) + RAMP[2] * uv[..., 1]


def albedo_depth(s):
    ad = np.full((H, W, 4), 0.5, F)
    ad[s["sid"] == 0, :3] = 0.0
    ad[..., 3] = s["depth"]
    return ad


def frames(move, offset, seed=1):
    """Previous frame (rectangle at REST) as a history, current frame (rectangle at `move`) as guides
    with a black image: with N_HIST = 4 and alpha = 0.2 a kept pixel integrates 0.8 x its history."""
    rng = np.random.default_rng(seed)
    cam = camera(offset)
    before = mr.scene(cam, mr.REST, None, offset)
    now = mr.scene(cam, move, mr.REST, offset)
    colour = rng.uniform(0.1, 2.0, (H, W, 4)).astype(F)
    rect0 = before["sid"] == mr.RECT_ID
    colour[rect0, :3] = ramp(before["uv"][rect0])[:, None].astype(F)
    mu1 = rng.uniform(0.2, 2.0, (H, W)).astype(F)
    mom = np.stack([mu1, mu1 * mu1 + rng.uniform(0.0, 0.3, (H, W)).astype(F), np.full((H, W), N_HIST, F),
                    before["depth"]], -1).astype(F)
    hist = (colour, mom, before["normal_plane"], cam)
    img = np.zeros((H, W, 4), F)
    img[..., 3] = 1.0
    return cam, before, now, hist, img


def run_motion(cam, now, hist, img, **kw):
    info = {}
    out = tr.accumulate(img, now["normal_plane"], albedo_depth(now), cam, hist, now["motion"], now["prev_normal"],
                        info=info, **dict(PARAMS, **kw))
    return out, info


def run_static(cam, now, hist, img):
    info = {}
    out = tr.accumulate(img, now["normal_plane"], albedo_depth(now), cam, hist, info=info, **PARAMS)
    return out, info


def interior(before, now, info):
    ids = mr.tap_ids(before["sid"], info)
    return (now["sid"] == mr.RECT_ID) & (ids == mr.RECT_ID).all(-1)


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS, ids=IDS)
@pytest.mark.parametrize("demod", [False, True], ids=["plain", "demodulated"])
def test_zero_motion_is_the_static_rule_bit_for_bit(offset, demod):
    rng = np.random.default_rng(3)
    o = np.asarray(offset, np.float64)
    prev = make_camera(tuple(o + (0.0, 1.0, -4.0)), tuple(o + (0.0, 0.6, 0.0)), W, H, fovy=50.0)
    cur = make_camera(tuple(o + (0.6, 1.1, -3.8)), tuple(o + (0.1, 0.6, 0.0)), W, H, fovy=50.0)
    before, now = mr.scene(prev, offset=offset), mr.scene(cur, offset=offset)
    ad = albedo_depth(now)
    ad[..., :3] = rng.uniform(0.0, 1.0, (H, W, 3))
    img = rng.uniform(0.1, 2.0, (H, W, 4)).astype(F)
    mu1 = rng.uniform(0.2, 2.0, (H, W)).astype(F)
    mom = np.stack([mu1, mu1 * mu1 + F(0.1), rng.integers(1, 41, (H, W)).astype(F), before["depth"]], -1).astype(F)
    hist = (rng.uniform(0.1, 2.0, (H, W, 4)).astype(F), mom, before["normal_plane"], prev)
    zero = np.zeros((H, W, 4), F)
    params = dict(PARAMS, demodulate_albedo=demod)
    info = {}
    got = tr.accumulate(img, now["normal_plane"], ad, cur, hist, zero, zero, info=info, **params)
    want = tr.accumulate(img, now["normal_plane"], ad, cur, hist, **params)
    assert (info["valid_taps"] == 4).sum() > 500 and (info["valid_taps"] == 0).sum() > 20
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    # without history, too
    for a, b in zip(tr.accumulate(img, now["normal_plane"], ad, cur, None, zero, zero, **params),
                    tr.accumulate(img, now["normal_plane"], ad, cur, None, **params)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS, ids=IDS)
def test_a_slide_in_its_own_plane_follows_the_object_where_the_static_rule_ghosts(offset):
    cam, before, now, hist, img = frames(MOVES["slide"], offset)
    (colour, mom, _), info = run_motion(cam, now, hist, img)
    inner = interior(before, now, info)
    print(f"slide, offset {offset[0]:g}: {inner.sum()} interior pixels of {(now['sid'] == mr.RECT_ID).sum()}")
    assert inner.sum() >= 30
    assert (info["valid_taps"][inner] == 4).all()
    assert (mom[..., 2][inner] == N_HIST + 1).all()
    # colour = 0.8 x the bilinear resampling of the ramp = 0.8 x the ramp at the pixel's own object-space
    # point: exact for a linear ramp up to rounding.  The history position is off by < 4e-5 pixel (the
    # float32 steps of depth, r, motion, the division and the scale to pixels, at |f| <= 45), the ramp
    # changes by < 0.11 per pixel, and the weights, products and sums round at 6e-8 relative of <= 2:
    # < 5e-6 + 1e-6, asserted at 2e-5.
    own = ramp(now["uv"])
    resampled = colour[..., 0].astype(np.float64) / 0.8
    err = np.abs(resampled - own)[inner].max()
    print(f"  |resampled history - ramp at the own point| <= {err:.2e}")
    assert err <= 2e-5
    # the static rule finds valid taps as well (same plane, same normal) but integrates the point of
    # the previous rectangle that was where the pixel's point is now: the ramp displaced by the shift
    (scolour, smom, _), sinfo = run_static(cam, now, hist, img)
    both = inner & (sinfo["valid_taps"] == 4) & (mr.tap_ids(before["sid"], sinfo) == mr.RECT_ID).all(-1)
    assert both.sum() >= 20
    ghost = scolour[..., 0].astype(np.float64) / 0.8 - resampled
    np.testing.assert_allclose(ghost[both], RAMP[1] * SLIDE, atol=4e-5)


# ---- 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS, ids=IDS)
def test_a_translation_out_of_its_plane_is_kept_where_the_static_rule_rejects(offset):
    cam, before, now, hist, img = frames(MOVES["out_of_plane"], offset)
    rect = now["sid"] == mr.RECT_ID
    # the static rule's plane residual on the old rectangle is 0.3 |n . dir| (dir the unit translation,
    # here along the normal) against a tolerance of 0.01 |r|: float64, every rectangle pixel
    m = tr.pixel_dirs(cam, W, H, np.float64)
    r = m * (now["depth"].astype(np.float64) / np.linalg.norm(m, axis=-1))[..., None]
    n = before["normal_plane"][before["sid"] == mr.RECT_ID][0, :3].astype(np.float64)
    assert (0.3 * abs(n @ np.array([0.0, 0.0, -1.0])) > 0.01 * np.linalg.norm(r, axis=-1)[rect]).all()
    (scolour, smom, _), sinfo = run_static(cam, now, hist, img)
    assert rect.sum() >= 60 and (sinfo["valid_taps"][rect] == 0).all()
    assert (smom[..., 2][rect] == 1).all()
    (colour, mom, _), info = run_motion(cam, now, hist, img)
    inner = interior(before, now, info)
    print(f"out of plane, offset {offset[0]:g}: {inner.sum()} interior pixels of {rect.sum()}")
    assert inner.sum() >= 30
    assert (info["valid_taps"][inner] == 4).all() and (mom[..., 2][inner] == N_HIST + 1).all()


# ---- 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS, ids=IDS)
def test_a_turn_is_kept_only_through_the_previous_normal(offset):
    cam, before, now, hist, img = frames(MOVES["turn"], offset)
    rect = now["sid"] == mr.RECT_ID
    dn = now["normal_plane"][rect][:, :3].astype(np.float64) - now["prev_normal"][rect][:, :3].astype(np.float64)
    np.testing.assert_allclose((dn * dn).sum(-1), 2 - 2 * np.cos(np.radians(20.0)), atol=1e-6)   # 0.1206 > 0.1
    (colour, mom, _), info = run_motion(cam, now, hist, img)
    inner = interior(before, now, info)
    print(f"turn, offset {offset[0]:g}: {inner.sum()} interior pixels of {rect.sum()}")
    assert inner.sum() >= 30
    assert (info["valid_taps"][inner] == 4).all() and (mom[..., 2][inner] == N_HIST + 1).all()
    # with gp = g the same taps fail the normal test
    (_, mom_g, _), info_g = run_motion(cam, now, hist, img, use_prev_normal=False)
    assert (info_g["valid_taps"][inner] == 0).all() and (mom_g[..., 2][inner] == 1).all()


# ---- 5, 6 ---------------------------------------------------------------------------------------
def _assert_restarted(planes, sel, img, now):
    colour, mom, nrm = planes
    l = tr.luminance(img)
    assert sel.sum() > 0
    assert (mom[..., 2][sel] == 1).all()
    np.testing.assert_array_equal(colour[sel].view(np.uint32), img[sel].view(np.uint32))
    np.testing.assert_array_equal(mom[..., 0][sel].view(np.uint32), l[sel].view(np.uint32))
    np.testing.assert_array_equal(mom[..., 1][sel].view(np.uint32), (l * l)[sel].view(np.uint32))
    np.testing.assert_array_equal(mom[..., 3][sel].view(np.uint32), now["depth"][sel].view(np.uint32))
    np.testing.assert_array_equal(nrm.view(np.uint32), now["normal_plane"].view(np.uint32))


@pytest.mark.parametrize("offset", OFFSETS, ids=IDS)
@pytest.mark.parametrize("move", ["slide", "lift"])   # the moves that uncover whole pixels
def test_uncovered_wall_pixels_restart(move, offset):
    cam, before, now, hist, img = frames(MOVES[move], offset)
    img[..., :3] = np.random.default_rng(5).uniform(0.1, 2.0, (H, W, 3))
    planes, info = run_motion(cam, now, hist, img)
    # wall now (flag 0: reprojected onto itself), every tap on what was the rectangle
    uncovered = (now["sid"] == 2) & (mr.tap_ids(before["sid"], info) == mr.RECT_ID).all(-1)
    print(f"{move}, offset {offset[0]:g}: {uncovered.sum()} uncovered wall pixels")
    assert (now["motion"][uncovered] == 0).all()
    assert (info["valid_taps"][uncovered] == 0).all()
    _assert_restarted(planes, uncovered, img, now)


def test_pixels_without_a_previous_pose_restart():
    cam, before, now, hist, img = frames(MOVES["slide"], OFFSETS[0])
    rng = np.random.default_rng(6)
    img[..., :3] = rng.uniform(0.1, 2.0, (H, W, 3))
    _, info = run_motion(cam, now, hist, img)
    kept = info["valid_taps"] == 4
    gone = (rng.random((H, W)) < 0.3) & (now["sid"] > 0)
    assert (gone & kept & (now["sid"] == mr.RECT_ID)).sum() >= 5 and (gone & kept & (now["sid"] != mr.RECT_ID)).sum() > 50
    marked = dict(now, motion=now["motion"].copy(), prev_normal=now["prev_normal"].copy())
    marked["motion"][gone] = (0.0, 0.0, 0.0, -1.0)
    marked["prev_normal"][gone] = 0.0
    planes, info2 = run_motion(cam, marked, hist, img)
    assert (info2["valid_taps"][gone] == 0).all()
    _assert_restarted(planes, gone, img, now)
    # the others do not notice
    ref, _ = run_motion(cam, now, hist, img)
    for a, b in zip(planes, ref):
        np.testing.assert_array_equal(a[~gone].view(np.uint32), b[~gone].view(np.uint32))


# ---- 7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", sorted(MOVES))
def test_the_kept_and_restarted_sets_do_not_depend_on_the_distance_from_the_origin(move):
    sets = []
    for offset in OFFSETS:
        cam, before, now, hist, img = frames(MOVES[move], offset)
        (_, mom, _), info = run_motion(cam, now, hist, img)
        sets.append((now["sid"], info["valid_taps"], info["have"], mom[..., 2]))
    for a, b in zip(*sets):
        np.testing.assert_array_equal(a, b)
    restarted = ~sets[0][2] & (sets[0][0] > 0)
    assert (sets[0][1] == 4).sum() > 500 and (restarted.sum() > 0 or move not in ("slide", "lift"))
