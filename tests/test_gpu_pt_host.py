"""The path tracer's host side (mcrt_pt_host.cpp): what mcrt_render_frame(s) returns when it refuses,
and how the read-backs of a PT call's counter block relate to each other.  Both tests were written
against the code while it still lived in mcrt_capi.cpp and quote its messages; they use the `mixed`
scene at 96x64 and 32x32 (whole 8x8 tiles)."""
import ctypes

import numpy as np
import pytest

from clref_job import build_scene
from helpers import refused
from mcrt import types as T
from mcrt.camera import scene_camera

pytestmark = pytest.mark.gpu
INVALID_ARG, NOT_READY = 1, 4
NAME, W, H = "mixed", 96, 64


def _params(frame=0, max_depth=2, sampler=T.SAMPLER_RANDOM, band_rows=8, num_bands=1, band_index=0,
            integrator=T.INTEGRATOR_PT):
    return T.FrameParams(frame, max_depth, sampler, 0, 3, band_rows, num_bands, band_index, integrator, 0)


def test_render_refusals(hip_ctx):
    """Status code and message of every refusal of mcrt_render_frame(s), in the order the entry
    function checks them: NULL arguments, a frame buffer of another context, a scene without
    mcrt_accel_build, the frame count (and BDPT's smaller limit), the cameras' size, max_depth, the
    sampler, Sobol without its matrices, the integrator, the band arguments.  A call with two faults
    reports the earlier one.  (The two 2^31 size checks need a frame buffer too large for a test.)
    No refusal leaves state behind: a good frame renders afterwards."""
    from mcrt import lib
    L = lib.lib()
    sc = build_scene(NAME)
    assert sc.sobol is None
    ds = lib.DeviceScene(hip_ctx, sc)
    unbuilt = lib.DeviceScene(hip_ctx, sc, build=False)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    other = lib.Context(0)
    fb_other = lib.FrameBuffer(other, W, H)
    cam = scene_camera(NAME, W, H)
    small = scene_camera(NAME, 32, 32)
    many = np.repeat(cam, 257)   # a refused count never reads them; they are there all the same
    BDPT = T.INTEGRATOR_BDPT

    def frames(cams, count, p, scene=ds, target=fb, ctx=hip_ctx):
        """mcrt_render_frames through ctypes; the message is read from `ctx` (None: the thread's)."""
        cams = None if cams is None else np.ascontiguousarray(cams)
        st = L.mcrt_render_frames(scene.h if scene else None, target.h if target else None, lib._p(cams), count,
                                  ctypes.byref(p) if p else None)
        lib._check(st, ctx.h if ctx else None)

    def frame(cams, p, scene=ds, target=fb, ctx=hip_ctx):
        cams = None if cams is None else np.ascontiguousarray(cams)
        st = L.mcrt_render_frame(scene.h if scene else None, target.h if target else None, lib._p(cams),
                                 ctypes.byref(p) if p else None)
        lib._check(st, ctx.h if ctx else None)

    try:
        # NULL arguments, both entry points; without a scene there is no context to hold the message
        for call in (lambda **kw: frames(kw.pop("cams", cam), 1, kw.pop("p", _params()), **kw),
                     lambda **kw: frame(kw.pop("cams", cam), kw.pop("p", _params()), **kw)):
            refused(lambda: call(scene=None, ctx=None), INVALID_ARG, "NULL argument")
            refused(lambda: call(target=None), INVALID_ARG, "NULL argument")
            refused(lambda: call(cams=None), INVALID_ARG, "NULL argument")
            refused(lambda: call(p=None), INVALID_ARG, "NULL argument")
        # ... before the context check: a NULL camera with another context's frame buffer
        refused(lambda: frames(None, 1, _params(), target=fb_other), INVALID_ARG, "NULL argument")
        another = "frame buffer belongs to another context"
        refused(lambda: frames(cam, 1, _params(), target=fb_other), INVALID_ARG, another)
        refused(lambda: frames(cam, 1, _params(), scene=unbuilt, target=fb_other), INVALID_ARG, another)
        not_built = "mcrt_accel_build has not been called"
        refused(lambda: fb.render(unbuilt, cam), NOT_READY, not_built)
        refused(lambda: frames(cam, 0, _params(), scene=unbuilt), NOT_READY, not_built)
        count = "frame count must be 1 .. MCRT_MAX_BATCH_FRAMES (256)"
        refused(lambda: frames(cam, 0, _params()), INVALID_ARG, count)
        refused(lambda: frames(many, 257, _params()), INVALID_ARG, count)
        refused(lambda: frames(cam, -1, _params()), INVALID_ARG, count)
        refused(lambda: frames(cam, 0, _params(integrator=7)), INVALID_ARG, count)   # two faults: the count first
        refused(lambda: frames(many, 257, _params(integrator=BDPT)), INVALID_ARG, count)
        bdpt_count = "BDPT frame count must be 1 .. MCRT_MAX_BDPT_BATCH_FRAMES (32)"
        refused(lambda: frames(many, 33, _params(integrator=BDPT)), INVALID_ARG, bdpt_count)
        refused(lambda: frames(np.repeat(small, 33), 33, _params(integrator=BDPT)), INVALID_ARG, bdpt_count)
        camera = "camera size differs from the frame buffer"
        refused(lambda: fb.render(ds, small), INVALID_ARG, camera)
        refused(lambda: fb.render_frames(ds, [cam, cam, small]), INVALID_ARG, camera)   # any camera of the batch
        refused(lambda: fb.render(ds, small, max_depth=0), INVALID_ARG, camera)         # two faults: the camera first
        refused(lambda: fb.render(ds, small, integrator=BDPT), INVALID_ARG, camera)
        depth = "max_depth out of range"
        refused(lambda: fb.render(ds, cam, max_depth=0), INVALID_ARG, depth)
        refused(lambda: fb.render(ds, cam, max_depth=33), INVALID_ARG, depth)
        refused(lambda: fb.render(ds, cam, max_depth=33, sampler=7), INVALID_ARG, depth)
        refused(lambda: fb.render(ds, cam, sampler=7), INVALID_ARG, "unknown sampler")
        refused(lambda: fb.render(ds, cam, sampler=7, integrator=7), INVALID_ARG, "unknown sampler")
        sobol = "Sobol sampler requires the 1024x52 Sobol matrices in the scene"
        refused(lambda: fb.render(ds, cam, sampler=T.SAMPLER_SOBOL), INVALID_ARG, sobol)
        refused(lambda: fb.render(ds, cam, sampler=T.SAMPLER_SOBOL, integrator=7), INVALID_ARG, sobol)
        refused(lambda: fb.render(ds, cam, integrator=7), INVALID_ARG, "unknown integrator")
        refused(lambda: fb.render(ds, cam, integrator=7, num_bands=2, band_index=2), INVALID_ARG, "unknown integrator")
        # frame_args
        refused(lambda: fb.render(ds, cam, num_bands=2, band_index=2), INVALID_ARG, "band_index out of range")
        refused(lambda: fb.render(ds, cam, num_bands=2, band_index=-1), INVALID_ARG, "band_index out of range")
        refused(lambda: fb.render(ds, cam, num_bands=2, band_rows=4), INVALID_ARG,
                "band_rows must be a positive multiple of 8")
        refused(lambda: fb.render(ds, cam, num_bands=2, band_rows=4, band_index=2), INVALID_ARG,
                "band_rows must be a positive multiple of 8")
        # nothing was rendered, nothing is left behind
        assert fb.queue_counts(8) == ([0] * 8, [0] * 8)
        refused(lambda: fb.read_queue(0), INVALID_ARG, "nothing rendered yet")
        for integrator in (T.INTEGRATOR_PT, BDPT):
            fb.render(ds, cam, integrator=integrator)
            img = fb.read(0)
            assert np.isfinite(img).all() and img[..., :3].max() > 0
    finally:
        fb_other.close()
        other.close()
        fb.close()
        unbuilt.close()
        ds.close()


def _readbacks(fb):
    shadow, ext = fb.queue_counts(8)
    return {"stats": fb.stats(), "shadow": shadow, "ext": ext, "hints": fb.hint_counts(8),
            "retraces": fb.retrace_counts(8), "queue": [fb.read_queue(0), fb.read_queue(1)]}


def _check_pt_readbacks(r, pixels, D):
    """The relations between the read-backs of a PT call of `pixels` camera paths at depth D."""
    shadow, ext, st = r["shadow"], r["ext"], r["stats"]
    print(f"D={D} pixels={pixels} stats={st} shadow={shadow} ext={ext} hints={r['hints']} retraces={r['retraces']} "
          f"queue records={[len(q[0]) for q in r['queue']]}")
    assert st["closest_rays"] == pixels + sum(ext[:D - 1])
    assert st["shaded_paths"] == st["closest_rays"]
    assert st["any_rays"] == sum(shadow[:D])
    assert all(n >= 0 for n in shadow + ext)
    assert shadow[0] > 0 and (D == 1 or ext[0] > 0)   # the frame sees the scene: the counters are live
    assert all(shadow[b] == 0 for b in range(D, 8))
    assert all(ext[b] == 0 for b in range(max(D - 1, 0), 8))
    assert all(0 <= r["hints"][b] <= shadow[b] for b in range(8))
    assert all(r["hints"][b] == 0 for b in range(D, 8))
    assert all(0 <= r["retraces"][b] <= ext[b] for b in range(8))
    assert all(r["retraces"][b] == 0 for b in range(max(D - 1, 0), 8))
    assert len(r["queue"][0][0]) == shadow[D - 1]
    assert len(r["queue"][1][0]) == (ext[D - 2] if D >= 2 else 0)
    for q in r["queue"]:
        assert len(q[0]) == len(q[1]) == len(q[2])
        for plane in q:
            assert np.isfinite(plane).all()


def test_pt_counter_readbacks(hip_ctx):
    """mcrt_framebuffer_stats, _queue_counts, _hint_counts, _retrace_counts and _read_queue after PT
    calls at 96x64 (depth 3, depth 1, a batch of 3 frames) with the hint and retrace counters on
    (profiling level 2): which entries are live and how they add up, with no measured constant.  A
    fresh frame buffer reads all zero and has no queue to read; after a BDPT frame the per-bounce
    read-backs are zero and the ray statistics follow BDPT's rule; one and two frames in flight read
    back the same.  (Between the runs with one and two frames in flight the hint counts are left out:
    a shadow ray reads its occluder hint while other waves of the launch write theirs to the same
    origin-cell table, so that count may differ between two runs of one configuration.)"""
    from mcrt import lib
    sc = build_scene(NAME)
    tiles = (W // 8) * (H // 8)
    cams = [scene_camera(NAME, W, H, frame=k, jitter=True) for k in range(3)]
    filt = T.make_filter(T.BOX)
    hip_ctx.set_profiling(2)
    try:
        ds = lib.DeviceScene(hip_ctx, sc)
        fb = lib.FrameBuffer(hip_ctx, W, H)
        zero = [0] * 8
        assert fb.queue_counts(8) == (zero, zero) and fb.hint_counts(8) == zero and fb.retrace_counts(8) == zero
        assert fb.stats() == {"closest_rays": 0, "any_rays": 0, "shaded_paths": 0}
        for which in (0, 1):
            refused(lambda: fb.read_queue(which), INVALID_ARG, "nothing rendered yet")
        # twice each, so that every case also runs in a slot that has rendered another depth before
        for rnd in range(2):
            fb.render(ds, cams[0], frame=rnd, max_depth=3)
            _check_pt_readbacks(_readbacks(fb), tiles * 64, 3)
            fb.accumulate(filt, 4 * rnd)
            fb.render(ds, cams[0], frame=rnd, max_depth=1)
            _check_pt_readbacks(_readbacks(fb), tiles * 64, 1)
            fb.accumulate(filt, 4 * rnd + 1)
            fb.render_frames(ds, cams, frame=rnd, max_depth=3)
            _check_pt_readbacks(_readbacks(fb), tiles * 64 * 3, 3)
            fb.accumulate_frames([filt] * 3, 4 * rnd + 2)
        # a BDPT frame: the per-bounce read-backs are PT's
        fb.render(ds, cams[0], frame=0, max_depth=3, integrator=T.INTEGRATOR_BDPT)
        assert fb.queue_counts(8) == (zero, zero) and fb.hint_counts(8) == zero and fb.retrace_counts(8) == zero
        st = fb.stats()
        print("bdpt", st)
        assert st["shaded_paths"] == st["closest_rays"] > 0 and st["any_rays"] > 0
        fb.accumulate(filt, 9)
        # ... and a PT frame after it reads back as before
        fb.render(ds, cams[0], frame=0, max_depth=3)
        _check_pt_readbacks(_readbacks(fb), tiles * 64, 3)
        hip_ctx.reset_stats()   # the pending launch timings name this frame buffer's counters
        fb.close()
        ds.close()

        # the same frames with one and with two frames in flight, each from a fresh scene and frame buffer
        def run(fif):
            ds = lib.DeviceScene(hip_ctx, sc)
            fb = lib.FrameBuffer(hip_ctx, W, H)
            fb.set_frames_in_flight(fif)
            out = []
            for k in range(3):
                fb.render(ds, cams[k], frame=k, max_depth=3)
                fb.accumulate(filt, k)
                r = _readbacks(fb)
                _check_pt_readbacks(r, tiles * 64, 3)
                r["queue"] = [len(q[0]) for q in r["queue"]]   # the order inside a queue is the atomics'
                del r["hints"]
                out.append(r)
            img = fb.read(2)
            hip_ctx.reset_stats()
            fb.close()
            ds.close()
            return out, img
        one, img1 = run(1)
        two, img2 = run(2)
        assert one == two
        np.testing.assert_array_equal(img1.view(np.uint32), img2.view(np.uint32))
    finally:
        hip_ctx.set_profiling(False)
