"""Per-object motion for the temporal history on the GPU: mcrt_scene_motion_snapshot,
mcrt_render_guides_motion (k_guides_motion), mcrt_temporal_accumulate_motion (k_temporal's MOTION
form) against tests/motion_truth.py (float64 truth with forward bounds) and
tests/temporal_ref.py (the numpy restatement, operation for operation; tests/temporal_motion_ref.py
is its scene).

The accumulate is compared as tests/test_gpu_temporal.py compares the static one: planes expected
bit-equal, asserted at rtol 2e-5, atol 1e-7 (the variance: |d| <= 2e-5 mu2 + 1e-7), the number of
bit-different values printed.
"""
import ctypes

import numpy as np
import pytest

import motion_truth as mt
import temporal_motion_ref as mr
import temporal_ref as tr
from denoise_harness import Installed, bits, compare_planes, pair_a, synth_planes, tm_rmse
from mcrt import scenes
from mcrt import types as T
from mcrt.camera import scene_camera
from refit_util import translate, with_transforms

pytestmark = pytest.mark.gpu

F = np.float32
FAR = (1000.0, 1000.0, 1000.0)
SIZES = [(45, 37), (16, 16)]
SIZE_IDS = ["45x37", "16x16"]


def _about(centre, M):
    """M applied about `centre`."""
    c = np.asarray(centre, np.float64)
    return translate(c).astype(np.float64) @ np.asarray(M, np.float64) @ translate(-c).astype(np.float64)


def _moved(sc, moves):
    """`sc` with shape k at moves[k] @ its transform.  A pure translation leaves the three rows of the
    inverse transpose that transform normals as they were (mathematically they are unchanged; a
    fresh float64 inverse may round them differently)."""
    mats = [s["toWorldTransform"].copy() for s in sc.shapes]
    for k, M in moves.items():
        mats[k] = (np.asarray(M, np.float64) @ mats[k].astype(np.float64)).astype(F)
    out = with_transforms(sc, mats)
    for k, M in moves.items():
        if np.array_equal(np.asarray(M)[:3, :3], np.eye(3)):
            out.shapes["toWorldInverseTranspose"][k][:3] = sc.shapes["toWorldInverseTranspose"][k][:3]
    return out


def _shape_ids(fb, ds, cam):
    """Shape index per pixel from the texture-LOD AOV (o[1].y), -1 on a miss."""
    aov = fb.render_aov(ds, cam, T.AOV_TEXTURE_LOD)
    ids = np.ascontiguousarray(aov[:, :, 1, 1]).view(np.int32).copy()
    return ids


# ---- the two scenes and their moves --------------------------------------------------------------------
def _two_level():
    """instances_test_scene(): shape 2 (an instance of mesh A) translated, shape 4 (another instance of
    A) turned and rescaled non-uniformly, shape 1 (mesh A itself) mirrored about its centre."""
    sc = scenes.instances_test_scene()
    turn = scenes._affine(1.0, 25.0, (0.3, -0.2, 0.4), 10.0).astype(np.float64)
    turn[:3, :3] = turn[:3, :3] @ np.diag([1.3, 0.8, 1.1])
    moves = {2: translate((-0.5, 0.6, -1.0)), 4: _about((-4, 2, 1), turn),
             1: _about((0, 1, 0), np.diag([-1.0, 1.0, 1.0, 1.0]))}
    return sc, _moved(sc, moves), "instances_test", moves


def _flat():
    """test_scene(): shape 4 (a sphere) moved; shape 5 takes shape 3's vertices, lifted above shape 3 (a
    changed mesh key: no previous pose, whatever its matrices)."""
    sc = scenes.test_scene()
    turn = scenes._affine(1.0, -30.0, (0.4, 0.3, -0.6), 15.0).astype(np.float64)
    turn[:3, :3] = turn[:3, :3] @ np.diag([0.9, 1.2, 1.0])
    moves = {4: _about((-0.1, 0.9, -1.5), turn)}
    moved = _moved(sc, {**moves, 5: translate((0.0, 1.7, 0.0))})
    assert moved.shapes["numTriangles"][5] == moved.shapes["numTriangles"][3]
    moved.shapes["startVertex"][5] = moved.shapes["startVertex"][3]
    return sc, moved, "mixed", moves


def _apply(ds, moved, two_level):
    if two_level:
        ds.update_transforms(moved.shapes)
    else:
        ds.update_shapes(moved.shapes)
        ds.build()


# ---- 1. guide planes --------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("which", ["two_level", "flat"])
def test_guides_are_those_of_render_guides_and_no_snapshot_means_no_motion(hip_ctx, which, size):
    from mcrt import lib
    W, H = size
    sc, moved, camname, _ = _two_level() if which == "two_level" else _flat()
    ds = lib.DeviceScene(hip_ctx, sc)
    assert ds.layout()["two_level"] == (1 if which == "two_level" else 0)
    cam = scene_camera(camname, W, H)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    for lod in (False, True):
        fb.render_guides(ds, cam, texture_lod=lod)
        want = [fb.read_guides(w) for w in (0, 1)]
        fb.render_guides_motion(ds, cam, texture_lod=lod)
        got = [fb.read_guides(w) for w in (0, 1)]
        for a, b in zip(got, want):
            np.testing.assert_array_equal(bits(a), bits(b))
        assert (want[1][..., 3] > 0).sum() > 50
        for w in (0, 1):
            assert (bits(fb.read_motion(w)) == 0).all()
    # with a snapshot, and with the shapes moved, the guide planes are still k_guides'
    ds.motion_snapshot()
    _apply(ds, moved, which == "two_level")
    fb.render_guides(ds, cam)
    want = [fb.read_guides(w) for w in (0, 1)]
    fb.render_guides_motion(ds, cam)
    for w in (0, 1):
        np.testing.assert_array_equal(bits(fb.read_guides(w)), bits(want[w]))
    assert (fb.read_motion(0)[..., 3] == 1).any()
    fb.close()
    ds.close()


# ---- 2. motion and previous normal after a move -------------------------------------------------------
def _check_moved(sc, moved, cam, ids, depth, npl, motion, pnorm, moved_shapes, gone_shapes=()):
    hit = depth > 0
    flag = motion[..., 3]
    is_moved = hit & np.isin(ids, list(moved_shapes))
    is_gone = hit & np.isin(ids, list(gone_shapes))
    np.testing.assert_array_equal(flag == 1, is_moved)
    np.testing.assert_array_equal(flag == -1, is_gone)
    still = ~is_moved
    assert (bits(motion[still][:, :3]) == 0).all() and (bits(pnorm[still]) == 0).all()
    assert (bits(flag[~is_moved & ~is_gone]) == 0).all()
    assert (pnorm[..., 3] == 0).all()
    worst_d = worst_n = 0.0
    for k in moved_shapes:
        sel = hit & (ids == k)
        if not sel.any():
            continue
        Mp, Mc = sc.shapes["toWorldTransform"][k], moved.shapes["toWorldTransform"][k]
        ITp, ITc = sc.shapes["toWorldInverseTranspose"][k], moved.shapes["toWorldInverseTranspose"][k]
        d, P, D = mt.truth_motion(cam, depth, Mp, Mc)
        bound = mt.bound_motion(cam, depth, d, D, Mp, Mc, mt.shape_vertices(moved, k))
        err = np.abs(motion[..., :3].astype(np.float64) - d).max(-1)
        worst_d = max(worst_d, float((err / bound)[sel].max()))
        assert (err[sel] <= bound[sel]).all(), (k, float(err[sel].max()), float(bound[sel].min()))
        assert np.abs(d[sel]).max() > 50 * bound[sel].max()         # the bound is far below the motion itself
        length = np.linalg.norm(pnorm[sel][:, :3].astype(np.float64), axis=-1)
        np.testing.assert_allclose(length, 1.0, atol=8 * mt.U)     # 3 squares, 2 sums, rsqrt, a product: <= 8 roundings
        if np.array_equal(ITp[:3], ITc[:3]):    # a pure translation: the same normal, bit for bit
            np.testing.assert_array_equal(bits(pnorm[sel][:, :3]), bits(npl[sel][:, :3]))
        else:
            want, e_n = mt.truth_normal(npl[..., :3], ITp, ITc)
            en = np.abs(pnorm[..., :3].astype(np.float64) - want).max(-1)
            worst_n = max(worst_n, float(en[sel].max() / e_n))
            assert (en[sel] <= e_n).all(), (k, float(en[sel].max()), e_n)
    return worst_d, worst_n


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_motion_planes_of_moved_instances(hip_ctx, size):
    from mcrt import lib
    W, H = size
    sc, moved, camname, moves = _two_level()
    ds = lib.DeviceScene(hip_ctx, sc)
    cam = scene_camera(camname, W, H)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    ds.motion_snapshot()
    ds.update_transforms(moved.shapes)
    fb.render_guides_motion(ds, cam)
    npl, ad = fb.read_guides(0), fb.read_guides(1)
    motion, pnorm = fb.read_motion(0), fb.read_motion(1)
    ids = _shape_ids(fb, ds, cam)
    counts = {k: int(((ids == k) & (ad[..., 3] > 0)).sum()) for k in moves}
    wd, wn = _check_moved(sc, moved, cam, ids, ad[..., 3], npl, motion, pnorm, moves)
    print(f"{W}x{H}: pixels per moved shape {counts}; largest error / bound: motion {wd:.3f}, previous normal {wn:.3f}")
    assert sum(counts.values()) > 0
    if W == 45:
        assert all(c > 0 for c in counts.values()), counts
        # two instances of one mesh (shapes 2 and 4 of mesh A) moved differently: their own motion
        a, b = (motion[(ids == k) & (ad[..., 3] > 0)][:, :3].astype(np.float64) for k in (2, 4))
        np.testing.assert_allclose(a, np.broadcast_to([0.5, -0.6, 1.0], a.shape), atol=2e-5)   # P_prev - P
        assert np.abs(b - b.mean(0)).max() > 0.05
    # the next snapshot makes everything static again
    ds.motion_snapshot()
    fb.render_guides_motion(ds, cam)
    for w in (0, 1):
        assert (bits(fb.read_motion(w)) == 0).all()
    fb.close()
    ds.close()


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_motion_planes_of_a_flat_scene_and_a_changed_mesh_key(hip_ctx, size):
    from mcrt import lib
    W, H = size
    sc, moved, camname, moves = _flat()
    ds = lib.DeviceScene(hip_ctx, sc)
    cam = scene_camera(camname, W, H)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    ds.motion_snapshot()          # before any change; needs no build of its own
    _apply(ds, moved, False)
    fb.render_guides_motion(ds, cam)
    npl, ad = fb.read_guides(0), fb.read_guides(1)
    motion, pnorm = fb.read_motion(0), fb.read_motion(1)
    ids = _shape_ids(fb, ds, cam)
    hit = ad[..., 3] > 0
    counts = {k: int(((ids == k) & hit).sum()) for k in (4, 5)}
    wd, wn = _check_moved(sc, moved, cam, ids, ad[..., 3], npl, motion, pnorm, moves, gone_shapes=(5,))
    print(f"{W}x{H}: moved pixels {counts[4]}, changed-key pixels {counts[5]}; largest error / bound: motion {wd:.3f}, "
          f"previous normal {wn:.3f}")
    if W == 45:
        assert counts[4] > 0 and counts[5] > 0
        gone = hit & (ids == 5)
        assert (bits(motion[gone]) == bits(np.array([0, 0, 0, -1], F))).all()
    fb.close()
    ds.close()


# ---- 3. k_temporal's MOTION form against the restatement -------------------------------------------------
_CASES = {}


def _case(W, H, offset, seed):
    """Camera pair A with the rectangle slid, lifted and turned between the frames (flag 1), a seventh of
    the other hit pixels without a previous pose (flag -1), the rest static; history planes of the
    previous camera with values over six decades on a fifth of the pixels, N in 1..40, some
    zero-variance moments, zero and sub-1e-3 albedo channels (as tests/test_gpu_temporal.py)."""
    key = (W, H, offset, seed)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(seed)
    prev, cur = pair_a(W, H, offset)
    before = mr.scene(prev, mr.REST, None, offset)
    now = mr.scene(cur, mr.pose((0.17, 0.08, -0.1), turn_deg=12.0), mr.REST, offset)
    sid, depth = now["sid"], now["depth"]
    motion, pnorm = now["motion"].copy(), now["prev_normal"].copy()
    gone = (sid > 0) & (sid != mr.RECT_ID) & (rng.random((H, W)) < 1 / 7)
    motion[gone] = (0.0, 0.0, 0.0, -1.0)
    ad, img, hc, hm = synth_planes(rng, sid, depth, before["depth"])
    case = dict(prev=prev, cur=cur, sid=sid, npl=now["normal_plane"], ad=ad, img=img, motion=motion, pnorm=pnorm,
                hist=(hc, hm, before["normal_plane"]), before_sid=before["sid"])
    _CASES[key] = case
    return case


@pytest.mark.parametrize("demod", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), FAR], ids=["origin", "far"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_one_step_matches_the_reference(hip_ctx, size, offset, demod, monkeypatch):
    W, H = size
    case = _case(W, H, offset, seed=W)
    params = dict(tr.DEFAULTS, demodulate_albedo=demod)
    info = {}
    rc, rm, rn = tr.accumulate(case["img"], case["npl"], case["ad"], case["cur"], case["hist"] + (case["prev"],),
                               case["motion"], case["pnorm"], info=info, **params)
    rv = tr.variance(rm, rn, **params)
    flag, taps, hit = case["motion"][..., 3], info["valid_taps"], case["sid"] > 0
    # the case mixes all three flags; moved pixels keep history only through the motion path
    assert (flag == 1).sum() >= (4 if W == 16 else 40) and (flag == -1).sum() >= 10 and (hit & (flag == 0)).sum() >= 100
    assert (taps[flag == 1] == 4).sum() >= (1 if W == 16 else 20)
    assert (taps[flag == -1] == 0).all() and (rm[..., 2][flag == -1] == 1).all()
    assert (taps[hit & (flag == 0)] == 4).sum() >= 100 and ((taps > 0) & (taps < 4)).any()
    static = {}
    tr.accumulate(case["img"], case["npl"], case["ad"], case["cur"], case["hist"] + (case["prev"],), info=static, **params)
    assert (static["valid_taps"][flag == 1] < taps[flag == 1]).any()
    for loads in ("eager", "lazy"):            # both load forms of k_temporal: the same bits
        monkeypatch.setenv("MCRT_TEMPORAL_LOADS", loads)
        inst = Installed(hip_ctx, case)
        inst.fb.temporal_accumulate_motion(case["cur"], **params)
        got = inst.planes()
        inst.close()
        compare_planes(got, (rc, rm, rv, rn), f"{W}x{H} offset {offset[0]:g} demod {demod} {loads}")


# ---- 4. zero motion -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_installed_zero_motion_is_temporal_accumulate(hip_ctx, size, monkeypatch):
    W, H = size
    case = dict(_case(W, H, (0.0, 0.0, 0.0), seed=3))
    case["motion"] = np.zeros((H, W, 4), F)
    case["pnorm"] = np.zeros((H, W, 4), F)
    for loads in ("eager", "lazy"):
        monkeypatch.setenv("MCRT_TEMPORAL_LOADS", loads)
        for history in (True, False):
            a, b = Installed(hip_ctx, case, history), Installed(hip_ctx, case, history, motion=False)
            a.fb.temporal_accumulate_motion(case["cur"])
            b.fb.temporal_accumulate(case["cur"])
            for x, y in zip(a.planes(), b.planes()):
                np.testing.assert_array_equal(bits(x), bits(y))
            a.close()
            b.close()


# ---- 5. end to end ------------------------------------------------------------------------------------------
RW, RH = 64, 48
FRAMES = 8
MOVER = 1        # mesh A itself, in the middle of the image


def _pose_at(sc, d):
    """Frame d: the mover 0.2 units (about a pixel) along x and 3 degrees about the vertical per frame."""
    step = translate((0.2 * d, 0, 0)).astype(np.float64) @ _about((0, 1, 0), scenes._affine(1.0, 3.0 * d, (0, 0, 0)))
    return _moved(sc, {MOVER: step})


def _interactive(ctx, sc, cam, motion):
    """1 spp per displayed frame, the mover at its pose of each frame; returns the last display, N, the
    colour and moments history and the per-frame coverage of the mover."""
    from mcrt import lib
    box = T.make_filter(T.BOX)
    ds = lib.DeviceScene(ctx, sc)
    fb = lib.FrameBuffer(ctx, RW, RH)
    covered = np.zeros((RH, RW), bool)
    for d in range(FRAMES):
        if motion:
            ds.motion_snapshot()
        ds.update_transforms(_pose_at(sc, d).shapes)
        fb.render(ds, cam, frame=d, max_depth=2)
        fb.accumulate(box, 0)
        if motion:
            fb.render_guides_motion(ds, cam)
            fb.temporal_accumulate_motion(cam)
        else:
            fb.render_guides(ds, cam)
            fb.temporal_accumulate(cam)
        fb.denoise_guided_temporal(feedback_level=-1)
        covered |= (_shape_ids(fb, ds, cam) == MOVER) & (fb.read_guides(T.GUIDE_ALBEDO_DEPTH)[..., 3] > 0)
    out = dict(display=fb.read(3), colour=fb.read_temporal(T.TEMPORAL_COLOUR), moments=fb.read_temporal(T.TEMPORAL_MOMENTS),
               covered=covered)
    out["on_mover"] = (_shape_ids(fb, ds, cam) == MOVER) & (fb.read_guides(T.GUIDE_ALBEDO_DEPTH)[..., 3] > 0)
    if not motion:
        fb.denoise_guided()
        out["single"] = fb.read(3)
        # the truth at the final pose: the mean of frames 16..271
        tb = lib.FrameBuffer(ctx, RW, RH)
        for i, f0 in enumerate(range(16, 272, 64)):
            tb.render_frames(ds, [cam] * 64, frame=f0, max_depth=2)
            tb.accumulate_frames([box], i * 64)
        out["truth"] = tb.read(2)
        tb.close()
    fb.close()
    ds.close()
    assert np.isfinite(out["display"]).all()
    return out


def test_a_moving_instance_keeps_its_history_end_to_end(hip_ctx):
    """instances_test_scene(), 64x48, depth 2, 1 spp per displayed frame, static camera, 8 displayed
    frames, mesh A moving about a pixel and turning 3 degrees per frame; truth = the mean of frames
    16..271 at the final pose; error = tone-mapped (x / (1 + x)) RMSE on the mover's pixels.  The
    filter feeds nothing back (feedback_level -1), so that the two paths' histories differ only where
    the rule does.  DESIGN.md 2h records a run."""
    sc = scenes.instances_test_scene()
    cam = scene_camera("instances_test", RW, RH)
    m = _interactive(hip_ctx, sc, cam, True)
    s = _interactive(hip_ctx, sc, cam, False)
    on = s["on_mover"]
    np.testing.assert_array_equal(on, m["on_mover"])
    e_m, e_s, e_1 = (tm_rmse(a, s["truth"], on) for a in (m["display"], s["display"], s["single"]))
    n_m, n_s = int((m["moments"][..., 2][on] >= 4).sum()), int((s["moments"][..., 2][on] >= 4).sum())
    print(f"mover: {on.sum()} pixels; tone-mapped RMSE temporal with motion + filter {e_m:.4f}, static temporal + filter "
          f"{e_s:.4f}, single-frame guided {e_1:.4f}; pixels with N >= 4: with motion {n_m} ({n_m / on.sum():.0%}), "
          f"static {n_s} ({n_s / on.sum():.0%})")
    assert on.sum() > 30
    assert e_m < e_s and e_m < e_1, (e_m, e_s, e_1)
    assert n_m > n_s, (n_m, n_s)
    # Unmoved shapes, never covered by the mover: the same history, bit for bit.  The rule reads the
    # 2 x 2 taps around the pixel's own position, so a neighbour the mover covered at some frame is
    # excluded as well (one pixel of dilation).
    near = s["covered"] | m["covered"]
    grown = near.copy()
    grown[1:] |= near[:-1]
    grown[:-1] |= near[1:]
    g2 = grown.copy()
    g2[:, 1:] |= grown[:, :-1]
    g2[:, :-1] |= grown[:, 1:]
    far = ~g2
    assert far.sum() > 0.5 * RW * RH
    for k in ("colour", "moments"):
        np.testing.assert_array_equal(bits(m[k])[far], bits(s[k])[far])


# ---- 6. nothing existing moves ------------------------------------------------------------------------
def test_existing_outputs_do_not_notice_the_motion_calls(hip_ctx):
    from mcrt import lib
    W, H = 40, 24
    sc, moved, camname, _ = _two_level()
    cam = scene_camera(camname, W, H)
    box = T.make_filter(T.BOX)

    def sequence(motion):
        ds = lib.DeviceScene(hip_ctx, sc)
        fb = lib.FrameBuffer(hip_ctx, W, H)
        out = []
        for f, shapes in enumerate((sc.shapes, moved.shapes, sc.shapes)):
            if motion:
                ds.motion_snapshot()
            ds.update_transforms(shapes)
            fb.render(ds, cam, frame=f, max_depth=2)
            out.append(fb.read(0))
            fb.accumulate(box, 0)
            if motion:
                fb.render_guides_motion(ds, cam)
                fb.read_motion(0)
                scratch = lib.FrameBuffer(hip_ctx, W, H)     # the motion accumulate runs on another frame buffer
                scratch.render(ds, cam, frame=f, max_depth=2)
                scratch.accumulate(box, 0)
                scratch.render_guides_motion(ds, cam)
                scratch.temporal_accumulate_motion(cam)
                scratch.close()
            fb.render_guides(ds, cam)
            fb.temporal_accumulate(cam)
            fb.denoise_guided_temporal()
            out += [fb.read(2), fb.read(3)] + [fb.read_guides(w) for w in (0, 1)] + [fb.read_temporal(w) for w in range(4)]
        fb.close()
        ds.close()
        return out

    for a, b in zip(sequence(True), sequence(False)):
        np.testing.assert_array_equal(bits(a), bits(b))


# ---- 7. status codes ------------------------------------------------------------------------------------
def test_status_codes(hip_ctx):
    from mcrt import lib
    OK, INVALID, NOT_READY = 0, 1, 4
    L = lib.lib()
    W = H = 16
    case = _case(W, H, (0.0, 0.0, 0.0), seed=2)
    cam = np.ascontiguousarray(case["cur"])
    camp = cam.ctypes.data
    good = T.TemporalParams(0.2, 0.2, 32, 4, 0.1, 0.01, 1)
    fp = T.FrameParams(0, 1, T.SAMPLER_RANDOM, 0, 3, 8, 1, 0, T.INTEGRATOR_PT, 0)
    one = ctypes.c_void_p(1)
    sc = scenes.test_scene()
    ds = lib.DeviceScene(hip_ctx, sc, build=False)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    scam = np.ascontiguousarray(scene_camera("mixed", W, H))
    # NULL arguments
    assert L.mcrt_scene_motion_snapshot(None) == INVALID
    for args in ((None, fb.h, scam.ctypes.data, ctypes.byref(fp)), (ds.h, None, scam.ctypes.data, ctypes.byref(fp)),
                 (ds.h, fb.h, None, ctypes.byref(fp)), (ds.h, fb.h, scam.ctypes.data, None)):
        assert L.mcrt_render_guides_motion(*args) == INVALID
    assert L.mcrt_temporal_accumulate_motion(None, camp, ctypes.byref(good)) == INVALID
    assert L.mcrt_temporal_accumulate_motion(fb.h, None, ctypes.byref(good)) == INVALID
    assert L.mcrt_temporal_accumulate_motion(fb.h, camp, None) == INVALID
    for args in ((None, one, one), (fb.h, None, one), (fb.h, one, None)):
        assert L.mcrt_framebuffer_set_motion(*args) == INVALID
    assert L.mcrt_framebuffer_read_motion(None, 0, None, 0, None) == INVALID
    assert L.mcrt_framebuffer_read_motion(fb.h, 2, None, 0, None) == INVALID
    assert L.mcrt_framebuffer_read_motion(fb.h, -1, None, 0, None) == INVALID
    # the read protocol of mcrt_framebuffer_read_guides
    need = ctypes.c_uint64()
    for which in (0, 1):
        assert L.mcrt_framebuffer_read_motion(fb.h, which, None, 0, ctypes.byref(need)) == OK
        assert need.value == W * H * 16
        assert L.mcrt_framebuffer_read_motion(fb.h, which, one, 1 << 30, None) == NOT_READY   # no plane yet
    # the snapshot needs no build; the render call does
    assert L.mcrt_scene_motion_snapshot(ds.h) == OK
    assert L.mcrt_render_guides_motion(ds.h, fb.h, scam.ctypes.data, ctypes.byref(fp)) == NOT_READY
    ds.build()
    other = np.ascontiguousarray(scene_camera("mixed", W + 1, H))
    assert L.mcrt_render_guides_motion(ds.h, fb.h, other.ctypes.data, ctypes.byref(fp)) == INVALID
    # no guides
    assert L.mcrt_temporal_accumulate_motion(fb.h, scam.ctypes.data, ctypes.byref(good)) == NOT_READY
    # guides without motion planes, then motion planes made stale by render_guides / set_guides
    fb.render(ds, scam, frame=0, max_depth=2)
    fb.accumulate(T.make_filter(T.BOX), 0)
    fb.render_guides(ds, scam)
    assert L.mcrt_temporal_accumulate_motion(fb.h, scam.ctypes.data, ctypes.byref(good)) == NOT_READY
    fb.render_guides_motion(ds, scam)
    assert L.mcrt_temporal_accumulate_motion(fb.h, other.ctypes.data, ctypes.byref(good)) == INVALID
    for bad in (dict(alpha=-0.1), dict(alpha_moments=1.01), dict(max_history=0), dict(min_history=0),
                dict(normal_threshold=0.0), dict(plane_threshold=0.0)):
        with pytest.raises(lib.MCRTError, match="status 1"):
            fb.temporal_accumulate_motion(scam, **bad)
    assert L.mcrt_temporal_accumulate_motion(fb.h, scam.ctypes.data, ctypes.byref(good)) == OK
    fb.render_guides(ds, scam)
    assert L.mcrt_temporal_accumulate_motion(fb.h, scam.ctypes.data, ctypes.byref(good)) == NOT_READY
    assert L.mcrt_temporal_accumulate(fb.h, scam.ctypes.data, ctypes.byref(good)) == OK
    fb.render_guides_motion(ds, scam)
    buf = np.zeros((H, W), F)
    assert L.mcrt_framebuffer_read_motion(fb.h, 0, buf.ctypes.data, buf.nbytes, None) == INVALID   # too small
    inst = Installed(hip_ctx, case)
    assert L.mcrt_temporal_accumulate_motion(inst.fb.h, camp, ctypes.byref(good)) == OK
    inst.fb.set_guides(inst.keep[2].data_ptr(), inst.keep[3].data_ptr())
    assert L.mcrt_temporal_accumulate_motion(inst.fb.h, camp, ctypes.byref(good)) == NOT_READY
    inst.close()
    fb.close()
    # a band-split BDPT frame waiting for its gather
    W, H = 32, 16
    cam = np.ascontiguousarray(scene_camera("mixed", W, H))
    fb = lib.FrameBuffer(hip_ctx, W, H)
    fb.render(ds, cam, frame=0, max_depth=2)
    fb.accumulate(T.make_filter(T.BOX), 0)
    fb.render_guides_motion(ds, cam)
    fb.temporal_accumulate_motion(cam)
    fb.render(ds, cam, frame=0, max_depth=2, integrator=T.INTEGRATOR_BDPT, band_rows=8, num_bands=2, band_index=0)
    assert L.mcrt_temporal_accumulate_motion(fb.h, cam.ctypes.data, ctypes.byref(good)) == NOT_READY
    fb.bdpt_gather(None)
    fb.accumulate(T.make_filter(T.BOX), 0)
    assert L.mcrt_temporal_accumulate_motion(fb.h, cam.ctypes.data, ctypes.byref(good)) == OK
    assert np.isfinite(fb.read_temporal(0)).all()
    fb.close()
    ds.close()


# ---- 8. ordering ----------------------------------------------------------------------------------------
def test_ordering_with_frames_in_flight(hip_ctx):
    from mcrt import lib
    W, H = 64, 48
    sc = scenes.instances_test_scene()
    cam = scene_camera("instances_test", W, H)
    box = T.make_filter(T.BOX)

    def sequence(sync):
        ds = lib.DeviceScene(hip_ctx, sc)
        fb = lib.FrameBuffer(hip_ctx, W, H)
        fb.set_frames_in_flight(2)
        step = hip_ctx.sync if sync else (lambda: None)
        for d in range(3):
            ds.motion_snapshot()
            step()
            ds.update_transforms(_pose_at(sc, d + 1).shapes)
            step()
            fb.render_frames(ds, [cam, cam], frame=2 * d, max_depth=2)
            step()
            fb.accumulate_frames([box, box], 0)
            step()
            fb.render_guides_motion(ds, cam)
            step()
            fb.temporal_accumulate_motion(cam)
            step()
            if d == 2:
                fb.render(ds, cam, frame=100, max_depth=2)   # in flight on its slot's stream, never accumulated
                step()
            fb.denoise_guided_temporal()
            step()
        out = [fb.read(3)] + [fb.read_temporal(w) for w in range(4)] + [fb.read_motion(w) for w in (0, 1)]
        fb.close()
        ds.close()
        return out

    seq = sequence(False)
    assert (seq[5][..., 3] == 1).any()
    for a, b in zip(seq, sequence(True)):
        np.testing.assert_array_equal(bits(a), bits(b))
