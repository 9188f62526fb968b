"""Adaptive sampling on the GPU (mcrt_framebuffer_set_adaptive, mcrt_adaptive_update,
mcrt_framebuffer_set_active_tiles) against its numpy restatement tests/adaptive_ref.py and against a
plain frame buffer rendering the same frames.

Every render is the small test scene at 64x48 (48 whole tiles), depth 2, random sampler, box
filter.  The plain frame buffer's per-frame radiance is rendered once per parameter set and shared.
"""
import numpy as np
import pytest

import adaptive_ref as ad
import atrous_ref as ar
from denoise_harness import ATOL, RTOL, bits, ndiff
from mcrt import scenes
from mcrt import types as T
from mcrt.camera import scene_camera

pytestmark = pytest.mark.gpu

F = np.float32
W, H, TILES, DEPTH = 64, 48, 48, 2
PLAIN_FRAMES = 32
INVALID_ARG, NOT_READY = 1, 4
RR = {"plain": dict(rr=False), "rr": dict(rr=True, rr_start=1)}
SIGMAS = dict(sigma_normal=0.1, sigma_depth=0.02, sigma_luminance=4.0)


def refused(call, status, *words):
    """`call` raises MCRTError with this status code and a message holding every word."""
    from mcrt import lib
    with pytest.raises(lib.MCRTError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith(f"mcrt status {status}: "), msg
    for w in words:
        assert w in msg, msg


@pytest.fixture(scope="module")
def world(hip_ctx):
    from mcrt import lib
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    yield hip_ctx, ds, scene_camera("mixed", W, H), T.make_filter(T.BOX)
    ds.close()


def _wts(fb):
    import torch
    w = torch.zeros(fb.H * fb.W, dtype=torch.float32, device="cuda")
    fb.copy_device(3, w.data_ptr())
    fb.ctx.sync()
    return w.cpu().numpy().reshape(fb.H, fb.W)


def _planes(fb):
    return dict(wsum=fb.read(1), wts=_wts(fb), image=fb.read(2), mom=fb.read_guides(T.GUIDE_MOMENTS))


@pytest.fixture(scope="module")
def plain_frames(world):
    """Radiance of frames 0 .. PLAIN_FRAMES - 1 of a plain frame buffer, per parameter set."""
    from mcrt import lib
    ctx, ds, cam, filt = world
    out = {}
    for name, kw in RR.items():
        fb = lib.FrameBuffer(ctx, W, H)
        frames = []
        for f in range(PLAIN_FRAMES):
            fb.render(ds, cam, frame=f, max_depth=DEPTH, **kw)
            frames.append(fb.read(0))
            fb.accumulate(filt, f)
        fb.close()
        out[name] = frames
    assert ndiff(out["plain"][3], out["rr"][3]) > 0   # Russian roulette takes effect at this depth
    return out


# ---- 1. error and list, render-free ----------------------------------------------------------
@pytest.mark.parametrize("size", [(45, 37), (16, 16), (264, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_error_and_list_of_installed_moments(hip_ctx, size):
    import torch
    from mcrt import lib
    from test_gpu_denoise_guided import MOMENT_FRAMES, _synthetic
    w, h = size
    tx, ty = ad.tile_grid(w, h)
    mom = _synthetic(w, h, seed=w)[3]
    if (w, h) == (16, 16):
        mom[:8, 8:] = 0.0   # one all-zero tile: error exactly 0
    counts = np.full(tx * ty, MOMENT_FRAMES, np.uint32)
    model = ad.tile_error(mom, counts, w, h, 1e-3)
    assert np.isfinite(model).all()
    thr, rel, below, above = ad.gap_threshold(model)
    print(f"{w}x{h}: {tx * ty} tiles, threshold {thr:.6g}, gap {rel:.3g} relative, {below} below, {above} above")
    # no tile within rounding of the decision, and a real split
    assert rel > 1e-4 and 4 * below >= tx * ty and 4 * above >= tx * ty
    fb = lib.FrameBuffer(hip_ctx, w, h)
    try:
        fb.set_adaptive(error_threshold=thr, min_samples=2)
        assert np.isposinf(fb.read_adaptive(T.ADAPTIVE_TILE_ERROR)).all()
        assert fb.read_adaptive(T.ADAPTIVE_ACTIVE_LIST).tolist() == list(range(tx * ty))
        dev = torch.from_numpy(mom.reshape(-1)).cuda()
        fb.set_moments(dev.data_ptr(), MOMENT_FRAMES)
        assert (fb.read_adaptive(T.ADAPTIVE_TILE_SAMPLES) == MOMENT_FRAMES).all()
        n = fb.adaptive_update()
        got = fb.read_adaptive(T.ADAPTIVE_TILE_ERROR)
        print(f"{w}x{h}: tile errors differing in their bits: {ndiff(got, model)} of {got.size}")
        np.testing.assert_allclose(got, model, rtol=1e-5, atol=0)
        want = ad.active_list(model, counts, error_threshold=thr, min_samples=2)
        ids = fb.read_adaptive(T.ADAPTIVE_ACTIVE_LIST)
        assert n == len(want) == len(ids) and ids.tolist() == want.tolist()
        # nobody judged yet: every tile; everybody at the cap: none
        fb.set_adaptive(error_threshold=thr, min_samples=MOMENT_FRAMES + 1)
        fb.set_moments(dev.data_ptr(), MOMENT_FRAMES)
        assert fb.adaptive_update() == tx * ty
        assert fb.read_adaptive(T.ADAPTIVE_ACTIVE_LIST).tolist() == list(range(tx * ty))
        fb.set_adaptive(error_threshold=0.0, min_samples=2, max_samples=MOMENT_FRAMES)
        fb.set_moments(dev.data_ptr(), MOMENT_FRAMES)
        assert fb.adaptive_update() == 0 and fb.read_adaptive(T.ADAPTIVE_ACTIVE_LIST).size == 0
    finally:
        fb.close()


# ---- 2. all tiles active changes nothing -----------------------------------------------------
CALLS = [(0, 1), (1, 1), (2, 1), (3, 1), (4, 3), (7, 5)]   # (first frame, batch): frames 0 .. 11


def _sequence(world, adaptive, hook=None):
    """Frames 0 .. 11 in CALLS with two frames in flight: every frame's radiance, then the planes
    and a guided denoise.  adaptive: the mode with every tile kept active (nobody is judged before
    64 samples; a threshold of 0 alone would retire the all-miss tiles, whose error is 0) and an
    update after every call.  hook(fb, ds, cam, filt, stage, frame) runs before each render and
    between a render and its accumulate."""
    from mcrt import lib
    ctx, ds, cam, filt = world
    fb = lib.FrameBuffer(ctx, W, H)
    try:
        fb.set_frames_in_flight(2)
        if adaptive:
            fb.set_adaptive(error_threshold=0.0, min_samples=64, max_samples=0)
        else:
            fb.enable_moments(True)
        rad = []
        for first, batch in CALLS:
            if hook:
                hook(fb, ds, cam, filt, "render", first)
            if batch == 1:
                fb.render(ds, cam, frame=first, max_depth=DEPTH)
            else:
                fb.render_frames(ds, [cam] * batch, frame=first, max_depth=DEPTH)
            rad += [fb.read_frame(k) for k in range(batch)]
            if hook:
                hook(fb, ds, cam, filt, "accumulate", first)
            if batch == 1:
                fb.accumulate(filt, first)
            else:
                fb.accumulate_frames([filt] * batch, first)
            if adaptive:
                assert fb.adaptive_update() == TILES
        out = _planes(fb)
        out["rad"] = rad
        if adaptive:
            assert (fb.read_adaptive(T.ADAPTIVE_TILE_SAMPLES) == 12).all()
        fb.render_guides(ds, cam)
        fb.denoise_guided(levels=3, use_variance=True, demodulate_albedo=True, **SIGMAS)
        out["denoised"] = fb.read(3)
        out["fvar"] = fb.read_guides(T.GUIDE_FILTERED_VARIANCE)
        return out
    finally:
        fb.close()


def _same(got, want):
    for k in ("wsum", "wts", "image", "mom", "denoised", "fvar"):
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)
    assert len(got["rad"]) == len(want["rad"]) == 12
    for f, (a, b) in enumerate(zip(got["rad"], want["rad"])):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"radiance of frame {f}")


@pytest.fixture(scope="module")
def plain_sequence(world):
    return _sequence(world, adaptive=False)


def test_all_tiles_active_changes_nothing(world, plain_sequence, plain_frames):
    for f in range(12):   # the batched calls of the plain frame buffer give the single calls' frames
        np.testing.assert_array_equal(bits(plain_sequence["rad"][f]), bits(plain_frames["plain"][f]))
    assert np.abs(plain_sequence["denoised"] - plain_sequence["image"]).max() > 1e-3
    _same(_sequence(world, adaptive=True), plain_sequence)


# ---- 3. a listed call renders exactly its tiles ----------------------------------------------
def _lists():
    checker = [t for t in range(TILES) if (t % 8 + t // 8) % 2 == 0]
    return {"none": [], "last": [47], "seven": [1, 6, 8, 15, 22, 40, 47], "nine": [0, 2, 9, 11, 18, 27, 36, 45, 46],
            "checker": checker, "all-but-one": [t for t in range(TILES) if t != 5], "all": list(range(TILES))}


@pytest.mark.parametrize("params", list(RR), ids=list(RR))
def test_listed_calls_render_exactly_their_tiles(world, plain_frames, params):
    from mcrt import lib
    ctx, ds, cam, filt = world
    kw, plain = RR[params], plain_frames[params]
    lists = _lists()
    assert [len(v) for v in lists.values()] == [0, 1, 7, 9, 24, 47, 48]
    fb = lib.FrameBuffer(ctx, W, H)
    try:
        fb.set_adaptive(error_threshold=0.0, min_samples=2)
        fb.render(ds, cam, frame=0, max_depth=DEPTH, **kw)
        fb.accumulate(filt, 0)
        model = ad.step(ad.new_state(W, H), plain[:1], np.arange(TILES))
        frame = 1
        for name, ids in lists.items():
            m = ad.tile_mask(ids, W, H)
            for batch in (1, 3):
                before = _planes(fb)
                fb.set_active_tiles(ids)
                assert fb.read_adaptive(T.ADAPTIVE_ACTIVE_LIST).tolist() == ids
                if batch == 1:
                    fb.render(ds, cam, frame=frame, max_depth=DEPTH, **kw)
                else:
                    fb.render_frames(ds, [cam] * batch, frame=frame, max_depth=DEPTH, **kw)
                st = fb.stats()
                if not ids:
                    assert st == {"closest_rays": 0, "any_rays": 0, "shaded_paths": 0}
                else:
                    assert len(ids) * 64 * batch <= st["shaded_paths"] <= 2 * len(ids) * 64 * batch
                for k in range(batch):   # on the listed tiles: the plain frame buffer's same frame
                    np.testing.assert_array_equal(bits(fb.read_frame(k))[m], bits(plain[frame + k])[m],
                                                  err_msg=f"{name}, batch {batch}, frame {frame + k}")
                if batch == 1:
                    fb.accumulate(filt, frame)
                else:
                    fb.accumulate_frames([filt] * batch, frame)
                model = ad.step(model, plain[frame:frame + batch], ids)
                frame += batch
                after = _planes(fb)
                what = f"{name}, batch {batch}"
                for k in ("wsum", "wts", "mom"):
                    np.testing.assert_array_equal(bits(after[k]), bits(model[k]), err_msg=f"{k}: {what}")
                np.testing.assert_array_equal(fb.read_adaptive(T.ADAPTIVE_TILE_SAMPLES), model["counts"], err_msg=what)
                # cl_div is the 2.5-ulp division
                np.testing.assert_allclose(after["image"], model["wsum"] / model["wts"][..., None], rtol=1e-6, atol=0,
                                           err_msg=what)
                for k in ("wsum", "wts", "image", "mom"):   # unlisted tiles keep their bits
                    np.testing.assert_array_equal(bits(after[k])[~m], bits(before[k])[~m], err_msg=f"{k} kept: {what}")
        assert frame <= PLAIN_FRAMES and len(set(model["counts"].tolist())) > 3
    finally:
        fb.close()


# ---- 4. the loop end to end ------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop(world, plain_frames):
    """min_samples 8, rounds of 4 frames, max_samples 32, the threshold from the model's errors of
    the plain frame buffer's first 8 frames; the model is fed the plain per-frame radiance.  Yields
    the frame buffer after the last round, the model's state and the log of the rounds."""
    from mcrt import lib
    ctx, ds, cam, filt = world
    plain = plain_frames["plain"]
    first8 = ad.step(ad.new_state(W, H), plain[:8], np.arange(TILES))
    err8 = ad.tile_error(first8["mom"], first8["counts"], W, H, 1e-3)
    thr, rel, below, above = ad.gap_threshold(err8)
    print(f"threshold {thr:.6g}: gap {rel:.3g} relative at rank {below} of {TILES}; errors after 8 frames "
          f"min {err8.min():.3g} median {np.median(err8):.3g} max {err8.max():.3g}")
    p = dict(error_threshold=thr, min_samples=8, max_samples=32)
    fb = lib.FrameBuffer(ctx, W, H)
    fb.set_adaptive(luminance_floor=1e-3, **p)
    model, ids, log = ad.new_state(W, H), np.arange(TILES, dtype=np.uint32), []
    for rnd in range(PLAIN_FRAMES // 4):
        f0 = 4 * rnd
        fb.render_frames(ds, [cam] * 4, frame=f0, max_depth=DEPTH)
        fb.accumulate_frames([filt] * 4, f0)
        model = ad.step(model, plain[f0:f0 + 4], ids)
        n = fb.adaptive_update()
        err = ad.tile_error(model["mom"], model["counts"], W, H, 1e-3)
        ids = ad.active_list(err, model["counts"], **p)
        log.append(dict(n=n, got=fb.read_adaptive(T.ADAPTIVE_ACTIVE_LIST), want=ids, err=err,
                        got_err=fb.read_adaptive(T.ADAPTIVE_TILE_ERROR), planes=_planes(fb), model=model,
                        counts=fb.read_adaptive(T.ADAPTIVE_TILE_SAMPLES)))
        if n == 0:
            break
    yield fb, model, log, dict(thr=thr, rel=rel, below=below, above=above, err8=err8)
    fb.close()


def test_loop_follows_the_model(loop):
    fb, model, log, pick = loop
    assert pick["rel"] > 1e-4 and 4 * pick["below"] >= TILES and 4 * pick["above"] >= TILES
    for rnd, r in enumerate(log):
        what = f"round {rnd}"
        for k in ("wsum", "wts", "mom"):
            np.testing.assert_array_equal(bits(r["planes"][k]), bits(r["model"][k]), err_msg=f"{k}: {what}")
        np.testing.assert_array_equal(r["counts"], r["model"]["counts"], err_msg=what)
        print(f"{what}: {r['n']} active, tile errors differing in their bits: {ndiff(r['got_err'], r['err'])}")
        np.testing.assert_allclose(r["got_err"], r["err"], rtol=1e-5, atol=0, err_msg=what)
        assert r["n"] == len(r["want"]) and r["got"].tolist() == r["want"].tolist(), what
    assert log[0]["n"] == TILES                       # 4 samples: nobody is judged yet
    missed = np.flatnonzero(pick["err8"] == 0)        # the all-miss tiles: zero radiance, zero error
    assert len(missed) == 3
    assert not set(missed.tolist()) & set(log[1]["got"].tolist())   # ... leave at the first judging update
    assert 0 < log[1]["n"] == pick["above"] < TILES
    assert log[-1]["n"] == 0 and len(log) <= 8        # the run ends with an empty list
    counts = log[-1]["counts"]
    assert counts.min() == 8 and counts.max() == 32 and len(set(counts.tolist())) > 2   # not all equal


# ---- 5. denoiser with uneven counts ----------------------------------------------------------
def test_denoiser_takes_n_from_the_tile_counts(world, loop):
    ctx, ds, cam, filt = world
    fb, model, log, pick = loop
    fb.render_guides(ds, cam)
    npl, adp = fb.read_guides(T.GUIDE_NORMAL_PLANE), fb.read_guides(T.GUIDE_ALBEDO_DEPTH)
    image, mom = fb.read(2), fb.read_guides(T.GUIDE_MOMENTS)
    counts = fb.read_adaptive(T.ADAPTIVE_TILE_SAMPLES)
    fb.denoise_guided(levels=1, use_variance=True, demodulate_albedo=False, **SIGMAS)
    got_c, got_v = fb.read(3), fb.read_guides(T.GUIDE_FILTERED_VARIANCE)
    var = ad.prepare_var(mom, counts, W, H)
    uniform = ar.prepare(image, adp, mom, int(counts.max()))[1]
    assert ndiff(var, uniform) > W * H // 4          # the counts matter
    ref_c, ref_v = ar.level(image, var, npl, adp, 1, SIGMAS["sigma_normal"], SIGMAS["sigma_depth"],
                            ar.sigma_of_level(0, SIGMAS["sigma_luminance"], True), True)
    np.testing.assert_allclose(got_c, ref_c, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got_v, ref_v, rtol=RTOL, atol=ATOL)


# ---- 6. status codes -------------------------------------------------------------------------
def test_refusals_change_nothing(world, plain_sequence):
    from mcrt import lib
    ctx, ds, cam, filt = world
    seen = []

    def hook(fb, ds, cam, filt, stage, frame):
        seen.append((stage, frame))
        if stage == "render" and frame == 0:
            # frame_index 0 with a partial list; the reset then drops the rendered frame
            fb.set_active_tiles([0, 1])
            fb.render(ds, cam, frame=0, max_depth=DEPTH)
            refused(lambda: fb.accumulate(filt, 0), INVALID_ARG, "mcrt_adaptive_reset")
            refused(lambda: fb.set_active_tiles([3]), NOT_READY, "not been accumulated")
            fb.adaptive_reset()
            refused(lambda: fb.accumulate(filt, 0), NOT_READY, "no rendered frame")
            for bad in (dict(error_threshold=-1.0), dict(error_threshold=float("nan")), dict(min_samples=1),
                        dict(min_samples=8, max_samples=7), dict(luminance_floor=0.0)):
                refused(lambda: fb.set_adaptive(**{**dict(error_threshold=0.0, min_samples=64), **bad}), INVALID_ARG)
        elif stage == "render" and frame == 1:
            refused(lambda: fb.render(ds, cam, frame=frame, max_depth=DEPTH, integrator=T.INTEGRATOR_BDPT),
                    INVALID_ARG, "BDPT")
            refused(lambda: fb.render(ds, cam, frame=frame, max_depth=DEPTH, num_bands=2, band_rows=8), INVALID_ARG,
                    "num_bands")
        elif stage == "render" and frame == 2:
            refused(lambda: fb.set_active_tiles([5, 4]), INVALID_ARG, "ascending")
            refused(lambda: fb.set_active_tiles([4, 4]), INVALID_ARG, "ascending")
            refused(lambda: fb.set_active_tiles([0, TILES]), INVALID_ARG, "past the image")
            refused(lambda: fb.enable_moments(False), INVALID_ARG, "adaptive")
        elif stage == "render" and frame == 4:
            fb.render_guides(ds, cam)
            refused(lambda: fb.temporal_accumulate(cam), INVALID_ARG, "adaptive")
            refused(lambda: fb.temporal_accumulate_motion(cam), INVALID_ARG, "adaptive")
        elif stage == "accumulate" and frame == 3:
            refused(lambda: fb.adaptive_update(), NOT_READY, "not been accumulated")
            refused(lambda: fb.accumulate(filt, frame + 1), INVALID_ARG, "frame_index")
            refused(lambda: fb.accumulate(filt, 0), INVALID_ARG, "frame_index")
        elif stage == "accumulate" and frame == 7:
            refused(lambda: fb.accumulate_frames([filt] * 5, frame - 1), INVALID_ARG, "frame_index")
            refused(lambda: fb.adaptive_update(), NOT_READY)

    got = _sequence(world, adaptive=True, hook=hook)
    assert len(seen) == 2 * len(CALLS)
    _same(got, plain_sequence)
    # with the mode off the adaptive calls are refused, and switching it off frees the state
    fb = lib.FrameBuffer(ctx, W, H)
    try:
        for call in (lambda: fb.set_active_tiles([0]), fb.adaptive_update, fb.adaptive_reset,
                     lambda: fb.read_adaptive(T.ADAPTIVE_TILE_ERROR)):
            refused(call, INVALID_ARG, "adaptive mode is off")
        fb.set_adaptive(error_threshold=0.1, min_samples=4)
        fb.set_active_tiles([7])
        fb.set_adaptive(on=False)
        refused(lambda: fb.set_active_tiles([0]), INVALID_ARG, "adaptive mode is off")
        fb.enable_moments(False)
        fb.render(ds, cam, frame=0, max_depth=DEPTH)   # a plain frame again, every tile
        np.testing.assert_array_equal(bits(fb.read(0)), bits(plain_sequence["rad"][0]))
    finally:
        fb.close()
