"""The film (mcrt_film.hip): the frame buffer's own planes -- created, read back, copied, installed,
packed for the band gather and post-processed.  What each entry point returns when it refuses,
which plane each `which` selects, mcrt_framebuffer_set_accumulation's image, and k_denoise where the
image is not whole 16x16 denoise tiles.  The tests were written against the code while it still
lived in mcrt_capi.cpp and mcrt_kernels.hip and quote its messages; they use the `mixed` scene at
96x64 and 24x40 (whole 8x8 tiles)."""
import ctypes

import numpy as np
import pytest

from clref_job import build_scene
from helpers import refused
from mcrt import types as T
from mcrt.camera import scene_camera
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
INVALID_ARG, NOT_READY = 1, 4
NAME, W, H = "mixed", 96, 64


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device(n_floats):
    import torch
    return torch.full((n_floats,), float("nan"), dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def scene(hip_ctx):
    from mcrt import lib
    ds = lib.DeviceScene(hip_ctx, build_scene(NAME))
    yield ds
    ds.close()


@pytest.fixture(scope="module")
def film(hip_ctx, scene):
    """A 96x64 frame buffer after a 2-frame batch, its accumulation and a tone-mapped post-process."""
    from mcrt import lib
    fb = lib.FrameBuffer(hip_ctx, W, H)
    cams = [scene_camera(NAME, W, H, frame=f, jitter=True) for f in range(2)]
    fb.render_frames(scene, cams, frame=0, max_depth=2)
    fb.accumulate(T.make_filter(T.BOX), 0)
    fb.postprocess(tonemap=True, min_luminance=2.0)
    hip_ctx.sync()
    yield fb
    fb.close()


def test_film_refusals(hip_ctx, scene):
    """Status code and message of every refusal of the film's entry points, in the order each checks:
    NULL handles and destinations, the frame buffer's size (before anything is allocated), `which`
    and the frame index, the band entry points before a render, a gather chunk that is too small,
    the denoise radius.  Without a frame buffer there is no context to hold the message.  After
    the refusals a good call still works."""
    from mcrt import lib
    L = lib.lib()
    host = np.zeros((H, W, 4), np.float32)
    dev = _device(W * H * 4)
    dptr = dev.data_ptr()

    def call(fn, *args, ctx=hip_ctx):
        lib._check(fn(*args), ctx.h if ctx else None)

    # mcrt_framebuffer_create: one message for its five checks
    size = "invalid frame buffer size"
    out = ctypes.c_void_p()
    refused(lambda: call(L.mcrt_framebuffer_create, None, W, H, ctypes.byref(out), ctx=None), INVALID_ARG, size)
    refused(lambda: call(L.mcrt_framebuffer_create, hip_ctx.h, W, H, None), INVALID_ARG, size)
    refused(lambda: call(L.mcrt_framebuffer_create, hip_ctx.h, 0, H, ctypes.byref(out)), INVALID_ARG, size)
    refused(lambda: call(L.mcrt_framebuffer_create, hip_ctx.h, W, 0, ctypes.byref(out)), INVALID_ARG, size)
    # 2^30 + 2^15 pixels (16 GiB a plane): refused before anything is allocated
    refused(lambda: call(L.mcrt_framebuffer_create, hip_ctx.h, 32769, 32768, ctypes.byref(out)), INVALID_ARG, size)
    assert out.value is None
    assert L.mcrt_framebuffer_destroy(None) == 0   # destroying nothing is not an error

    fb = lib.FrameBuffer(hip_ctx, W, H)
    try:
        # NULL frame buffer: the message is the thread's
        refused(lambda: call(L.mcrt_framebuffer_device_ptrs, None, None, None, None, None, ctx=None), INVALID_ARG,
                "fb is NULL")
        refused(lambda: call(L.mcrt_framebuffer_band_layout, None, None, None, None, ctx=None), INVALID_ARG, "fb is NULL")
        refused(lambda: call(L.mcrt_postprocess, None, ctypes.byref(T.PostprocessParams()), ctx=None), INVALID_ARG,
                "NULL argument")
        for fn, args in ((L.mcrt_framebuffer_read, (0, lib._p(host))), (L.mcrt_framebuffer_read_frame, (0, lib._p(host))),
                         (L.mcrt_framebuffer_copy_device, (0, dptr)), (L.mcrt_framebuffer_copy_device_frame, (0, dptr)),
                         (L.mcrt_framebuffer_set_accumulation, (dptr, dptr)), (L.mcrt_framebuffer_bands_pack, (dptr,)),
                         (L.mcrt_framebuffer_bands_unpack, (dptr, 64))):
            refused(lambda: call(fn, None, *args, ctx=None), INVALID_ARG, "bad args")
        # NULL destination or source
        refused(lambda: call(L.mcrt_framebuffer_read, fb.h, 0, None), INVALID_ARG, "bad args")
        refused(lambda: call(L.mcrt_framebuffer_read_frame, fb.h, 0, None), INVALID_ARG, "bad args")
        refused(lambda: fb.copy_device(0, None), INVALID_ARG, "bad args")
        refused(lambda: fb.copy_device_frame(0, None), INVALID_ARG, "bad args")
        refused(lambda: fb.set_accumulation(None, dptr), INVALID_ARG, "bad args")
        refused(lambda: fb.set_accumulation(dptr, None), INVALID_ARG, "bad args")
        refused(lambda: call(L.mcrt_postprocess, fb.h, None), INVALID_ARG, "NULL argument")
        # ... before the band state is looked at
        refused(lambda: fb.bands_pack(None), INVALID_ARG, "bad args")
        refused(lambda: fb.bands_unpack(None, 64), INVALID_ARG, "bad args")
        # which
        for which in (-1, 4):
            refused(lambda: fb.read(which), INVALID_ARG, "bad args")
            refused(lambda: fb.copy_device(which, dptr), INVALID_ARG, "bad args")
        # the band entry points before any render; a too small max_rows is looked at after that
        nothing = "no frame rendered"
        refused(lambda: fb.bands_pack(dptr), NOT_READY, nothing)
        refused(lambda: fb.band_layout(), NOT_READY, nothing)
        refused(lambda: fb.bands_unpack(dptr, 64), NOT_READY, nothing)
        refused(lambda: fb.bands_unpack(dptr, 0), NOT_READY, nothing)
        # the frame index: one frame before any batch, then the batch's two
        index = "frame index outside the last mcrt_render_frames batch"
        for k in (-1, 1):
            refused(lambda: fb.read_frame(k), INVALID_ARG, index)
            refused(lambda: fb.copy_device_frame(k, dptr), INVALID_ARG, index)
        cams = [scene_camera(NAME, W, H, frame=f, jitter=True) for f in range(2)]
        fb.render_frames(scene, cams, frame=0, max_depth=2)
        fb.accumulate(T.make_filter(T.BOX), 0)
        for k in (-1, 2):
            refused(lambda: fb.read_frame(k), INVALID_ARG, index)
            refused(lambda: fb.copy_device_frame(k, dptr), INVALID_ARG, index)
        refused(lambda: call(L.mcrt_framebuffer_read_frame, fb.h, 2, None), INVALID_ARG, "bad args")   # two faults
        # a gather chunk one row short of the largest rank's share
        max_rows, bands, band = fb.band_layout()
        assert (max_rows, bands, band) == (H, 1, 0)
        small = _device(W * H * 5)
        refused(lambda: fb.bands_unpack(small.data_ptr(), max_rows - 1), INVALID_ARG,
                "max_rows below the largest rank's row count")
        refused(lambda: fb.bands_unpack(None, max_rows - 1), INVALID_ARG, "bad args")   # two faults
        # the denoise radius, looked at only when the pass is on
        refused(lambda: fb.postprocess(denoise=True, radius=17), INVALID_ARG,
                "denoise_radius > 16 (the GUI allows <= 10)")
        fb.postprocess(denoise=False, radius=17)
        # nothing is left behind: the good calls work
        img = fb.read(2)
        assert np.isfinite(img).all() and img[..., :3].max() > 0
        np.testing.assert_array_equal(_words(fb.read(3)), _words(img))
        fb.bands_pack(small.data_ptr())
        fb.bands_unpack(small.data_ptr(), max_rows)
        fb.postprocess(denoise=True, radius=16, sigma_spatial=2.0, sigma_range=0.5)
        hip_ctx.sync()
        np.testing.assert_array_equal(_words(fb.read(2)), _words(img))   # one band: the unpack rewrites the same image
        assert np.isfinite(fb.read(3)).all()
    finally:
        fb.close()


def test_plane_selection(hip_ctx, film):
    """mcrt_framebuffer_read 0..3 is the radiance of frame 0, wsum, image and display;
    mcrt_framebuffer_copy_device 0..3 is radiance, wsum, image and wts (4 bytes a pixel).  Word for
    word against each other and against the planes mcrt_framebuffer_device_ptrs names, which a second
    frame buffer copies out through its guide planes (mcrt_framebuffer_set_guides copies two float4
    planes from any device pointers, mcrt_framebuffer_read_guides reads them back)."""
    from mcrt import lib
    fb = film
    N = W * H
    read = [fb.read(k) for k in range(4)]
    dev = [_device(4 * N) for _ in range(3)] + [_device(4 * N)]   # plane 3 fills only the first N floats
    for k in range(4):
        fb.copy_device(k, dev[k].data_ptr())
    hip_ctx.sync()
    copied = [d.cpu().numpy() for d in dev]
    for k in range(3):
        np.testing.assert_array_equal(_words(copied[k]), _words(read[k]).reshape(-1))
    wts = copied[3][:N]
    assert np.isnan(copied[3][N:]).all()                      # 4 bytes a pixel were written, no more
    np.testing.assert_array_equal(wts, np.float32(2.0))       # two box-filtered frames
    # the four read planes are four different planes, and they are what they are said to be
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(_words(read[a]), _words(read[b])), (a, b)
    lit = read[0][..., :3].max(-1) > 0
    assert lit.any() and np.isfinite(read[0]).all()
    np.testing.assert_array_equal(_words(read[0]), _words(fb.read_frame(0)))
    both = np.clip(fb.read_frame(0), 0, 1000) + np.clip(fb.read_frame(1), 0, 1000)
    np.testing.assert_array_equal(_words(read[1]), _words(both))          # wsum = 1 * r0 + 1 * r1, one rounding
    np.testing.assert_allclose(read[2], read[1] / 2.0, rtol=3e-7, atol=1e-37)   # 2.5-ulp division
    ref = po.tonemap(read[2], 2.0)
    ok = np.isfinite(ref)
    np.testing.assert_allclose(read[3][ok], ref[ok], rtol=2e-5, atol=1e-7)
    # frame 1 of the batch, both ways
    f1 = _device(4 * N)
    fb.copy_device_frame(1, f1.data_ptr())
    hip_ctx.sync()
    frame1 = fb.read_frame(1)
    np.testing.assert_array_equal(_words(f1.cpu().numpy()), _words(frame1).reshape(-1))
    assert not np.array_equal(_words(frame1), _words(read[0]))
    # the device pointers: radiance, wsum, wts, image
    radiance, wsum, wts_ptr, image = fb.device_ptrs()
    assert len({radiance, wsum, wts_ptr, image}) == 4 and all((radiance, wsum, wts_ptr, image))
    probe = lib.FrameBuffer(hip_ctx, W, H)
    try:
        probe.set_guides(radiance, image)
        np.testing.assert_array_equal(_words(probe.read_guides(0)), _words(read[0]))
        np.testing.assert_array_equal(_words(probe.read_guides(1)), _words(read[2]))
        probe.set_guides(wsum, wsum)
        np.testing.assert_array_equal(_words(probe.read_guides(0)), _words(read[1]))
        four = _device(4 * N)   # wts is a quarter plane: copied out through the accumulation
        probe.set_accumulation(wsum, wts_ptr)
        probe.copy_device(3, four.data_ptr())
        hip_ctx.sync()
        np.testing.assert_array_equal(_words(four.cpu().numpy()[:N]), _words(wts))
    finally:
        probe.close()


def test_set_accumulation_resolves_the_same_image(hip_ctx, film):
    """wsum and wts copied into a fresh frame buffer (mcrt_framebuffer_set_accumulation): k_resolve's
    image equals k_accumulate's word for word -- the same division of the same words."""
    from mcrt import lib
    N = W * H
    wsum, wts = _device(4 * N), _device(N)
    film.copy_device(1, wsum.data_ptr())
    film.copy_device(3, wts.data_ptr())
    hip_ctx.sync()
    fresh = lib.FrameBuffer(hip_ctx, W, H)
    try:
        assert not fresh.read(2).any()   # created zero-filled
        fresh.set_accumulation(wsum.data_ptr(), wts.data_ptr())
        hip_ctx.sync()
        np.testing.assert_array_equal(_words(fresh.read(1)), _words(film.read(1)))
        np.testing.assert_array_equal(_words(fresh.read(2)), _words(film.read(2)))
        back = _device(N)
        fresh.copy_device(3, back.data_ptr())
        hip_ctx.sync()
        np.testing.assert_array_equal(_words(back.cpu().numpy()), _words(wts.cpu().numpy()))
    finally:
        fresh.close()
    assert film.read(2)[..., :3].max() > 0


def test_denoise_partial_denoise_tiles(hip_ctx, scene):
    """k_denoise at 24x40: whole 8x8 tiles, but 1.5 x 2.5 of its own 16x16 tiles, so the last column
    and the last row of workgroups stage a clamped apron and leave lanes idle.  The oracle's
    restatement, compared as test_gpu_postprocess.py::test_denoise_matches_oracle compares it."""
    from mcrt import lib
    w, h = 24, 40
    fb = lib.FrameBuffer(hip_ctx, w, h)
    try:
        cam = scene_camera(NAME, w, h)
        for f in range(4):
            fb.render(scene, cam, frame=f, max_depth=2)
            fb.accumulate(T.make_filter(T.BOX), f)
        img = fb.read(2)
        assert img.shape == (h, w, 4) and img[..., :3].max() > 0
        fb.postprocess(denoise=True, radius=3, sigma_spatial=2.0, sigma_range=0.5)
        got = fb.read(3)
        ref = po.denoise(img, 3, 2.0, 0.5)
        assert not np.array_equal(ref, img)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-7)
    finally:
        fb.close()
