"""Temporal reprojection and history on the GPU (mcrt_temporal_accumulate, k_temporal,
k_temporal_var, mcrt_denoise_guided_temporal) against the numpy restatement tests/temporal_ref.py.

The restatement is operation for operation (no transcendental, IEEE division and square root), so
the planes are expected bit-equal; the asserted bound is test_gpu_denoise_guided.py's rtol 2e-5,
atol 1e-7, and |d| <= 2e-5 mu2 + 1e-7 for the variance plane, a difference of two near-equal
numbers.  Each comparison prints the number of bit-different values.
"""
import ctypes

import numpy as np
import pytest

import atrous_ref as ar
import temporal_ref as tr
from denoise_harness import ATOL, RTOL, Installed, bits, compare_planes, pair_a, synth_planes, tm_rmse
from mcrt import scenes
from mcrt import types as T
from mcrt.camera import make_camera, scene_camera

pytestmark = pytest.mark.gpu

F = np.float32
SIGMAS = dict(sigma_normal=0.1, sigma_depth=0.02, sigma_luminance=4.0)
FAR = (1000.0, 1000.0, 1000.0)


def _case(W, H, offset, seed):
    """Guides of pair A's current camera, history planes of its previous camera: a colour history
    with values over six decades on a fifth of the pixels, N in 1..40, some zero-variance moments,
    zero and sub-1e-3 albedo channels."""
    rng = np.random.default_rng(seed)
    prev, cur = pair_a(W, H, offset)
    sid, npl, depth = tr.scene_guides(cur, offset)
    _, pnpl, pdepth = tr.scene_guides(prev, offset)
    ad, img, hc, hm = synth_planes(rng, sid, depth, pdepth)
    return dict(prev=prev, cur=cur, sid=sid, npl=npl, ad=ad, img=img, hist=(hc, hm, pnpl))


# ---- 1. one step against the reference --------------------------------------------------------
@pytest.mark.parametrize("demod", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), FAR], ids=["origin", "far"])
@pytest.mark.parametrize("size", [(45, 37), (16, 16)], ids=["45x37", "16x16"])
def test_one_step_matches_the_reference(hip_ctx, size, offset, demod, monkeypatch):
    W, H = size
    case = _case(W, H, offset, seed=W)
    params = dict(tr.DEFAULTS, demodulate_albedo=demod)
    info = {}
    rc, rm, rn = tr.accumulate(case["img"], case["npl"], case["ad"], case["cur"], case["hist"] + (case["prev"],),
                               info=info, **params)
    rv = tr.variance(rm, rn, **params)
    hit = case["sid"] > 0
    taps = info["valid_taps"]
    # the case covers full history, disocclusions, partial taps, the history cap and both variance paths
    assert (taps[hit] == 4).sum() >= (100 if W == 16 else 1000) and (taps[hit] == 0).sum() >= 3
    assert ((taps > 0) & (taps < 4)).any() and (rm[..., 2] == 32).any()
    assert (rm[..., 2] < 4).sum() > 10 and (rm[..., 2] >= 4).sum() > 10
    for loads in ("eager", "lazy"):            # both load forms of k_temporal: the same bits
        monkeypatch.setenv("MCRT_TEMPORAL_LOADS", loads)
        inst = Installed(hip_ctx, case)
        inst.fb.temporal_accumulate(case["cur"], **params)
        got = inst.planes()
        inst.close()
        compare_planes(got, (rc, rm, rv, rn), f"{W}x{H} offset {offset[0]:g} demod {demod} {loads}")


# ---- 2. reset and first call --------------------------------------------------------------------
@pytest.mark.parametrize("demod", [True, False], ids=["demodulated", "plain"])
def test_reset_and_first_call_start_without_history(hip_ctx, demod):
    case = _case(45, 37, (0.0, 0.0, 0.0), seed=5)
    want, _ = ar.prepare(case["img"], case["ad"], demodulate=demod)
    lum = ar.luminance(want)
    for first in (True, False):
        inst = Installed(hip_ctx, case, history=not first)
        if not first:
            inst.fb.temporal_accumulate(case["cur"], demodulate_albedo=demod)
            assert (inst.fb.read_temporal(T.TEMPORAL_MOMENTS)[..., 2] > 1).any()
            inst.fb.temporal_reset()
        inst.fb.temporal_accumulate(case["cur"], demodulate_albedo=demod)
        colour, mom, var, nrm = inst.planes()
        inst.close()
        np.testing.assert_array_equal(mom[..., 2], 1.0)
        np.testing.assert_array_equal(bits(colour), bits(want))
        np.testing.assert_array_equal(bits(mom[..., 0]), bits(lum))
        np.testing.assert_array_equal(bits(mom[..., 1]), bits(lum * lum))
        np.testing.assert_array_equal(bits(mom[..., 3]), bits(case["ad"][..., 3]))
        np.testing.assert_array_equal(bits(nrm), bits(case["npl"]))
        np.testing.assert_array_equal(bits(var), bits(tr.variance(mom, nrm, **tr.DEFAULTS)))


# ---- 3. the filter chain ------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(45, 37), (16, 16)], ids=["45x37", "16x16"])
def test_filter_chain_and_feedback(hip_ctx, size):
    W, H = size
    case = _case(W, H, (0.0, 0.0, 0.0), seed=W + 1)

    def accumulated():
        inst = Installed(hip_ctx, case)
        inst.fb.temporal_accumulate(case["cur"], demodulate_albedo=False)
        return inst

    plain = accumulated()
    colour, mom, var, nrm = plain.planes()
    plain.fb.denoise_guided_temporal(levels=1, demodulate_albedo=False, feedback_level=-1, **SIGMAS)
    display = plain.fb.read(3)
    ref_c, ref_v = ar.level(colour, var, case["npl"], case["ad"], 1, SIGMAS["sigma_normal"], SIGMAS["sigma_depth"],
                            ar.sigma_of_level(0, SIGMAS["sigma_luminance"], True), True)
    np.testing.assert_allclose(display, ref_c, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(plain.fb.read_guides(T.GUIDE_FILTERED_VARIANCE), ref_v, rtol=RTOL, atol=ATOL)
    # nothing was fed back: the history is as it was, and the call may be repeated
    np.testing.assert_array_equal(bits(plain.fb.read_temporal(T.TEMPORAL_COLOUR)), bits(colour))
    plain.fb.denoise_guided_temporal(levels=1, demodulate_albedo=False, feedback_level=-1, **SIGMAS)
    np.testing.assert_array_equal(bits(plain.fb.read(3)), bits(display))
    level0_var = plain.fb.read_guides(T.GUIDE_FILTERED_VARIANCE)
    plain.close()
    # level 0 fed back = the display of the feedback-less one-level run, bit for bit
    fed = accumulated()
    fed.fb.denoise_guided_temporal(levels=2, demodulate_albedo=False, feedback_level=0, **SIGMAS)
    two_levels = fed.fb.read(3)
    np.testing.assert_array_equal(bits(fed.fb.read_temporal(T.TEMPORAL_COLOUR)), bits(display))
    np.testing.assert_array_equal(bits(fed.fb.read_temporal(T.TEMPORAL_MOMENTS)), bits(mom))
    # the second level at single-pass accuracy: one reference level over the GPU's own level 0
    ref2, _ = ar.level(display, level0_var, case["npl"], case["ad"], 2, SIGMAS["sigma_normal"], SIGMAS["sigma_depth"],
                       ar.sigma_of_level(1, SIGMAS["sigma_luminance"], True), True)
    np.testing.assert_allclose(two_levels, ref2, rtol=RTOL, atol=ATOL)
    # a second accumulate integrates that plane
    fed.fb.temporal_accumulate(case["cur"], demodulate_albedo=False)
    got = fed.planes()
    fed.close()
    rc, rm, rn = tr.accumulate(case["img"], case["npl"], case["ad"], case["cur"], (display, mom, nrm, case["cur"]),
                               **tr.DEFAULTS)
    compare_planes(got, (rc, rm, tr.variance(rm, rn, **tr.DEFAULTS), rn), f"{W}x{H} accumulate after feedback")


def test_remodulation_and_tonemap_as_the_single_frame_filter(hip_ctx):
    """With demodulation the chain multiplies the albedo back after the last level and tone-maps
    like mcrt_denoise_guided: one level over the history equals mcrt_denoise_guided's one level over
    an image that demodulates to that history."""
    case = _case(45, 37, (0.0, 0.0, 0.0), seed=11)
    inst = Installed(hip_ctx, case, history=False)
    inst.fb.temporal_accumulate(case["cur"], demodulate_albedo=True)   # no history: colour = image / albedo
    colour, mom, var, nrm = inst.planes()
    inst.fb.denoise_guided_temporal(levels=1, demodulate_albedo=True, feedback_level=-1, **SIGMAS)
    got = inst.fb.read(3)
    ref_c, _ = ar.level(colour, var, case["npl"], case["ad"], 1, SIGMAS["sigma_normal"], SIGMAS["sigma_depth"],
                        ar.sigma_of_level(0, SIGMAS["sigma_luminance"], True), True, remodulate=True)
    np.testing.assert_allclose(got, ref_c, rtol=RTOL, atol=ATOL)
    inst.fb.denoise_guided_temporal(levels=1, demodulate_albedo=True, feedback_level=-1, tonemap=True,
                                    min_luminance=1.7, **SIGMAS)
    mapped = inst.fb.read(3)
    inst.close()
    other = Installed(hip_ctx, dict(case, img=got), history=False)
    other.fb.postprocess(tonemap=True, min_luminance=1.7)
    want = other.fb.read(3)
    other.close()
    np.testing.assert_array_equal(bits(mapped), bits(want))


# ---- 4. it helps a real render --------------------------------------------------------------------
RW, RH = 64, 48


def _truth(ctx, ds, cam):
    from mcrt import lib
    box = T.make_filter(T.BOX)
    fb = lib.FrameBuffer(ctx, RW, RH)
    for i, f0 in enumerate(range(16, 272, 64)):
        fb.render_frames(ds, [cam] * 64, frame=f0, max_depth=2)
        fb.accumulate_frames([box], i * 64)
    out = fb.read(2)
    fb.close()
    return out


def _mixed_camera(shift):
    pos, target, fov = scenes.CAMERAS["mixed"]
    s = np.asarray(shift, np.float64)
    return make_camera(tuple(np.asarray(pos) + s), tuple(np.asarray(target) + s), RW, RH, fovy=fov)


def _displayed_frames(ctx, ds, cams):
    """1 spp per displayed frame through temporal accumulation and the filter; returns the last
    display, the last raw frame, its single-frame guided denoise, N and the hit mask."""
    from mcrt import lib
    box = T.make_filter(T.BOX)
    fb = lib.FrameBuffer(ctx, RW, RH)
    for d, cam in enumerate(cams):
        fb.render(ds, cam, frame=d, max_depth=2)
        fb.accumulate(box, 0)
        fb.render_guides(ds, cam)
        fb.temporal_accumulate(cam)
        fb.denoise_guided_temporal()
    out = fb.read(3)
    raw = fb.read(2)
    N = fb.read_temporal(T.TEMPORAL_MOMENTS)[..., 2]
    hit = fb.read_guides(T.GUIDE_ALBEDO_DEPTH)[..., 3] > 0
    fb.denoise_guided()
    single = fb.read(3)
    fb.close()
    assert np.isfinite(out).all()
    return out, raw, single, N, hit


def test_it_helps_a_1spp_interactive_render(hip_ctx):
    """test_scene(), "mixed" camera, 64x48, depth 2, 1 spp per displayed frame, 8 displayed frames;
    ground truth = the mean of frames 16..271; error = tone-mapped (x / (1 + x)) RMSE.  Static
    camera: temporal + filter must beat both the single-frame guided denoise of frame 8 and the raw
    frame.  Camera moved by 0.04 units a frame: at least half of the hit pixels end with
    N >= min_history, and on them the error is no worse than the single-frame guided denoise of the
    same final frame against the truth rendered at the final camera.  No fixed numbers asserted;
    the measured ones are printed (DESIGN.md 2g records a run)."""
    from mcrt import lib
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    cam = scene_camera("mixed", RW, RH)
    truth = _truth(hip_ctx, ds, cam)
    out, raw, single, N, hit = _displayed_frames(hip_ctx, ds, [cam] * 8)
    e_t, e_s, e_r = tm_rmse(out, truth), tm_rmse(single, truth), tm_rmse(raw, truth)
    print(f"static camera, frame 8: raw {e_r:.4f}, single-frame guided {e_s:.4f}, temporal + filter {e_t:.4f}")
    assert e_t < e_s and e_t < e_r, (e_t, e_s, e_r)
    cams = [_mixed_camera((0.04 * d, 0.0, 0.0)) for d in range(8)]
    truth_m = _truth(hip_ctx, ds, cams[-1])
    out, raw, single, N, hit = _displayed_frames(hip_ctx, ds, cams)
    kept = hit & (N >= 4)
    e_t, e_s, e_r = (tm_rmse(a, truth_m, kept) for a in (out, single, raw))
    print(f"moving camera, frame 8: {kept.sum()} of {hit.sum()} hit pixels with N >= 4; on them raw {e_r:.4f}, "
          f"single-frame guided {e_s:.4f}, temporal + filter {e_t:.4f}")
    assert kept.sum() >= 0.5 * hit.sum()
    assert e_t <= e_s, (e_t, e_s)
    ds.close()


# ---- 5. nothing existing moves ----------------------------------------------------------------------
def test_existing_outputs_do_not_notice_the_temporal_calls(hip_ctx):
    from mcrt import lib
    W, H = 40, 24
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    cam = scene_camera("mixed", W, H)
    box = T.make_filter(T.BOX)

    def sequence(temporal):
        fb = lib.FrameBuffer(hip_ctx, W, H)
        fb.enable_moments()
        for f in range(3):
            fb.render(ds, cam, frame=f, max_depth=2)
            fb.accumulate(box, f)
        fb.render_guides(ds, cam)
        if temporal:
            for _ in range(2):
                fb.temporal_accumulate(cam)
                fb.denoise_guided_temporal()
            fb.temporal_reset()
        out = [fb.read(2)] + [fb.read_guides(w) for w in range(3)]
        fb.denoise_guided()
        out += [fb.read(3), fb.read_guides(T.GUIDE_FILTERED_VARIANCE)]
        fb.close()
        return out

    for a, b in zip(sequence(True), sequence(False)):
        np.testing.assert_array_equal(bits(a), bits(b))
    ds.close()


# ---- 6. status codes ----------------------------------------------------------------------------------
def test_status_codes(hip_ctx):
    from mcrt import lib
    OK, INVALID, NOT_READY = 0, 1, 4
    L = lib.lib()
    W = H = 16
    case = _case(W, H, (0.0, 0.0, 0.0), seed=2)
    cam = np.ascontiguousarray(case["cur"])
    camp = cam.ctypes.data
    good = T.TemporalParams(0.2, 0.2, 32, 4, 0.1, 0.01, 1)
    filt = T.GuidedDenoiseParams(5, 0.1, 0.02, 4.0, 1, 1, 0, 2.0)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    # NULL arguments
    assert L.mcrt_temporal_accumulate(None, camp, ctypes.byref(good)) == INVALID
    assert L.mcrt_temporal_accumulate(fb.h, None, ctypes.byref(good)) == INVALID
    assert L.mcrt_temporal_accumulate(fb.h, camp, None) == INVALID
    assert L.mcrt_temporal_reset(None) == INVALID
    assert L.mcrt_denoise_guided_temporal(None, ctypes.byref(filt), 0) == INVALID
    assert L.mcrt_denoise_guided_temporal(fb.h, None, 0) == INVALID
    one = ctypes.c_void_p(1)
    for args in ((None, one, one, one, camp), (fb.h, None, one, one, camp), (fb.h, one, None, one, camp),
                 (fb.h, one, one, None, camp), (fb.h, one, one, one, None)):
        assert L.mcrt_framebuffer_set_temporal_history(*args) == INVALID
    assert L.mcrt_framebuffer_read_temporal(None, 0, None, 0, None) == INVALID
    assert L.mcrt_framebuffer_read_temporal(fb.h, 4, None, 0, None) == INVALID
    assert L.mcrt_framebuffer_read_temporal(fb.h, -1, None, 0, None) == INVALID
    # the read protocol of mcrt_framebuffer_read_guides
    need = ctypes.c_uint64()
    for which, size in ((0, 16), (1, 16), (2, 4), (3, 16)):
        assert L.mcrt_framebuffer_read_temporal(fb.h, which, None, 0, ctypes.byref(need)) == OK
        assert need.value == W * H * size
        assert L.mcrt_framebuffer_read_temporal(fb.h, which, one, 1 << 30, None) == NOT_READY   # no plane yet
    # no guides
    assert L.mcrt_temporal_accumulate(fb.h, camp, ctypes.byref(good)) == NOT_READY
    assert L.mcrt_denoise_guided_temporal(fb.h, ctypes.byref(filt), 0) == NOT_READY
    fb.close()
    inst = Installed(hip_ctx, case)
    fb = inst.fb
    # guides and an installed history, but no accumulate yet
    assert L.mcrt_denoise_guided_temporal(fb.h, ctypes.byref(filt), 0) == NOT_READY
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha_moments=-0.1),
                dict(alpha_moments=1.01), dict(max_history=0), dict(min_history=0), dict(normal_threshold=0.0),
                dict(normal_threshold=-1.0), dict(plane_threshold=0.0)):
        with pytest.raises(lib.MCRTError, match="status 1"):
            fb.temporal_accumulate(cam, **bad)
    for w, h in ((W + 1, H), (W, H - 1)):
        other = make_camera((0.0, 1.0, -4.0), (0.0, 0.6, 0.0), w, h)
        with pytest.raises(lib.MCRTError, match="status 1"):
            fb.temporal_accumulate(other)
        with pytest.raises(lib.MCRTError, match="status 1"):
            fb.set_temporal_history(inst.keep[4].data_ptr(), inst.keep[5].data_ptr(), inst.keep[6].data_ptr(), other)
    buf = np.zeros((H, W), F)
    assert L.mcrt_framebuffer_read_temporal(fb.h, 0, buf.ctypes.data, buf.nbytes, None) == INVALID   # too small
    fb.temporal_accumulate(cam, alpha=0.0, alpha_moments=1.0, max_history=1, min_history=1)   # the limits are valid
    fb.temporal_accumulate(cam, demodulate_albedo=True)
    for level in (-2, 4, 5):
        with pytest.raises(lib.MCRTError, match="status 1"):
            fb.denoise_guided_temporal(levels=5, feedback_level=level)
    with pytest.raises(lib.MCRTError, match="status 1"):
        fb.denoise_guided_temporal(levels=1, feedback_level=0)
    for bad in (dict(levels=0), dict(levels=9), dict(sigma_normal=0.0), dict(sigma_depth=-1.0),
                dict(sigma_luminance=0.0)):
        with pytest.raises(lib.MCRTError, match="status 1"):
            fb.denoise_guided_temporal(**bad)
    with pytest.raises(lib.MCRTError, match="status 1"):
        fb.denoise_guided_temporal(demodulate_albedo=False)   # the accumulate demodulated
    fb.denoise_guided_temporal(levels=5, feedback_level=-1)
    fb.denoise_guided_temporal(levels=5, feedback_level=3)    # levels - 2: the last one allowed
    with pytest.raises(lib.MCRTError, match="status 4"):
        fb.denoise_guided_temporal(levels=5, feedback_level=-1)   # the history already holds a filtered level
    fb.temporal_accumulate(cam, demodulate_albedo=True)
    fb.denoise_guided_temporal()
    assert np.isfinite(fb.read(3)).all()
    inst.close()
    # a band-split BDPT frame waiting for its gather
    W, H = 32, 16
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    cam = np.ascontiguousarray(scene_camera("mixed", W, H))
    fb = lib.FrameBuffer(hip_ctx, W, H)
    fb.render_guides(ds, cam)
    fb.render(ds, cam, frame=0, max_depth=2)
    fb.accumulate(T.make_filter(T.BOX), 0)
    fb.temporal_accumulate(cam)
    fb.render(ds, cam, frame=0, max_depth=2, integrator=T.INTEGRATOR_BDPT, band_rows=8, num_bands=2, band_index=0)
    assert L.mcrt_temporal_accumulate(fb.h, cam.ctypes.data, ctypes.byref(good)) == NOT_READY
    assert L.mcrt_denoise_guided_temporal(fb.h, ctypes.byref(filt), 0) == NOT_READY
    fb.bdpt_gather(None)
    fb.accumulate(T.make_filter(T.BOX), 0)
    assert L.mcrt_temporal_accumulate(fb.h, cam.ctypes.data, ctypes.byref(good)) == OK
    assert L.mcrt_denoise_guided_temporal(fb.h, ctypes.byref(filt), 0) == OK
    assert np.isfinite(fb.read(3)).all()
    fb.close()
    ds.close()


# ---- 7. ordering ------------------------------------------------------------------------------------------
def test_ordering_with_frames_in_flight(hip_ctx):
    from mcrt import lib
    W, H = 64, 48
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    cam = scene_camera("mixed", W, H)
    box = T.make_filter(T.BOX)

    def sequence(sync):
        fb = lib.FrameBuffer(hip_ctx, W, H)
        fb.set_frames_in_flight(2)
        step = hip_ctx.sync if sync else (lambda: None)
        for d in range(3):
            fb.render_frames(ds, [cam, cam], frame=2 * d, max_depth=2)   # a batch of two frames per displayed frame
            step()
            fb.accumulate_frames([box, box], 0)
            step()
            fb.render_guides(ds, cam)
            step()
            fb.temporal_accumulate(cam)
            step()
            if d == 2:
                fb.render(ds, cam, frame=100, max_depth=2)   # in flight on its slot's stream, never accumulated
                step()
            fb.denoise_guided_temporal()
            step()
        out = [fb.read(3)] + [fb.read_temporal(w) for w in range(4)]
        fb.close()
        return out

    for a, b in zip(sequence(False), sequence(True)):
        np.testing.assert_array_equal(bits(a), bits(b))
    ds.close()
