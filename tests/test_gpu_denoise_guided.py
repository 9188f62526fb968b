"""The guide-buffer-driven a-trous denoiser on the GPU (mcrt_render_guides, k_moments,
mcrt_denoise_guided) against its numpy restatement tests/atrous_ref.py.

A level is compared at single-pass accuracy: the GPU's `levels = L` output against ONE reference
level applied to the GPU's own `levels = L - 1` output, so the amplification of an ulp through the
next level's luminance weight does not enter.  Tolerance rtol 2e-5, atol 1e-7: the kernel is the
same class as k_denoise (exponential weights, a normalised sum), test_gpu_postprocess.py's bound.
"""
import os

import numpy as np
import pytest

import atrous_ref as ar
from denoise_harness import ATOL, RTOL, Installed, bits, tm_rmse
from mcrt import scenes
from mcrt import types as T
from mcrt.camera import make_camera, scene_camera

pytestmark = pytest.mark.gpu

F = np.float32
MOMENT_FRAMES = 6
SIGMAS = dict(sigma_normal=0.1, sigma_depth=0.02, sigma_luminance=4.0)


def _synthetic(W, H, seed):
    """Two planes with different normals, a block of misses, zero-variance pixels, zero and
    sub-1e-3 albedo channels, values over six decades on a fifth of the pixels."""
    rng = np.random.default_rng(seed)
    npl = np.zeros((H, W, 4), F)
    npl[..., :3] = (0.0, 0.0, -1.0)
    npl[..., 3] = -3.0 + 0.02 * rng.standard_normal((H, W))
    xs = W * 11 // 20
    npl[:, xs:, :3] = (-0.6, 0.0, -0.8)
    npl[:, xs:, 3] = -5.0 + 0.02 * rng.standard_normal((H, W - xs))
    ad = np.empty((H, W, 4), F)
    ad[..., :3] = rng.uniform(0.05, 1.0, (H, W, 3))
    ad[..., 3] = rng.uniform(2.0, 6.0, (H, W))
    ad[..., 0][rng.random((H, W)) < 0.1] = 0.0
    ad[..., 1][rng.random((H, W)) < 0.1] = 5e-4
    npl[2:7, 3:9] = 0.0                       # misses
    ad[2:7, 3:9] = (0.0, 0.0, 0.0, -1.0)
    img = (np.linspace(0.5, 2.0, W)[None, :, None] * 10.0 ** rng.uniform(-0.05, 0.05, (H, W, 4))).astype(F)
    wild = rng.random((H, W)) < 0.2
    img[wild] = (10.0 ** rng.uniform(-3, 3, (int(wild.sum()), 4))).astype(F)
    img[..., 3] = rng.uniform(0, 1, (H, W))
    n = MOMENT_FRAMES
    m1 = (n * rng.uniform(0.5, 3.0, (H, W))).astype(F)
    m2 = (m1 * m1 / n + n * rng.uniform(0.0, 0.5, (H, W))).astype(F)
    mom = np.stack([m1, m2], -1).astype(F)
    mom[rng.random((H, W)) < 0.15] = 0.0       # zero variance
    return img.astype(F), npl, ad, mom


@pytest.fixture(scope="module", params=[(45, 37), (16, 16)], ids=["45x37", "16x16"])
def synthetic(request, hip_ctx):
    W, H = request.param
    img, npl, ad, mom = _synthetic(W, H, seed=W)
    inst = Installed(hip_ctx, dict(img=img, npl=npl, ad=ad, mom=mom, frames=MOMENT_FRAMES))
    np.testing.assert_array_equal(inst.fb.read(2), img)   # image = sum / 1: the input, bit for bit
    yield inst, img, npl, ad, mom
    inst.close()


# ---- 1. levels against the reference ---------------------------------------------------------
@pytest.mark.parametrize("use_var", [True, False], ids=["variance", "sigma-halving"])
def test_each_level_matches_one_reference_level(synthetic, use_var):
    inst, img, npl, ad, mom = synthetic
    c, var = ar.prepare(img, ad, mom if use_var else None, MOMENT_FRAMES)
    for L in range(1, 6):   # steps 1, 2, 4 run the tile-staged kernel, 8 and 16 the direct one
        got_c, got_v = inst.run(levels=L, use_variance=use_var, demodulate_albedo=False, **SIGMAS)
        ref_c, ref_v = ar.level(c, var, npl, ad, 1 << (L - 1), SIGMAS["sigma_normal"], SIGMAS["sigma_depth"],
                                ar.sigma_of_level(L - 1, SIGMAS["sigma_luminance"], use_var), use_var)
        assert np.isfinite(got_c).all() and np.isfinite(got_v).all()
        np.testing.assert_allclose(got_c, ref_c, rtol=RTOL, atol=ATOL, err_msg=f"colour, levels={L}")
        np.testing.assert_allclose(got_v, ref_v, rtol=RTOL, atol=ATOL, err_msg=f"variance, levels={L}")
        again_c, again_v = inst.run(levels=L, use_variance=use_var, demodulate_albedo=False, **SIGMAS)
        np.testing.assert_array_equal(bits(again_c), bits(got_c))
        np.testing.assert_array_equal(bits(again_v), bits(got_v))
        c, var = got_c, got_v   # the next level is judged on the GPU's own output


def test_staged_and_direct_kernels_agree_bit_for_bit(synthetic, monkeypatch):
    inst = synthetic[0]
    kw = dict(levels=3, use_variance=True, demodulate_albedo=True, **SIGMAS)
    monkeypatch.setenv("MCRT_ATROUS_LDS_MAX_STEP", "4")
    staged = inst.run(**kw)
    monkeypatch.setenv("MCRT_ATROUS_LDS_MAX_STEP", "0")
    direct = inst.run(**kw)
    monkeypatch.setenv("MCRT_ATROUS_LDS_MAX_STEP", "1")   # the switch between levels 0 and 1
    mixed = inst.run(**kw)
    for a, b in ((staged, direct), (staged, mixed)):
        np.testing.assert_array_equal(bits(a[0]), bits(b[0]))
        np.testing.assert_array_equal(bits(a[1]), bits(b[1]))


# ---- 2. demodulation, tone mapping -----------------------------------------------------------
def test_demodulation_and_tonemap(synthetic, hip_ctx):
    inst, img, npl, ad, mom = synthetic
    got_c, got_v = inst.run(levels=1, use_variance=True, demodulate_albedo=True, **SIGMAS)
    ref_c, ref_v = ar.denoise(img, npl, ad, mom, MOMENT_FRAMES, levels=1, use_variance=True, demodulate_albedo=True,
                              **SIGMAS)
    np.testing.assert_allclose(got_c, ref_c, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got_v, ref_v, rtol=RTOL, atol=ATOL)
    plain, _ = inst.run(levels=1, use_variance=True, demodulate_albedo=False, **SIGMAS)
    assert np.abs(plain - got_c).max() > 1e-3   # demodulation changes the result
    # tone mapping = k_tonemap over the untone-mapped output
    mapped, _ = inst.run(levels=1, use_variance=True, demodulate_albedo=True, tonemap=True, min_luminance=1.7,
                         **SIGMAS)
    other = Installed(hip_ctx, dict(img=got_c, npl=npl, ad=ad))
    np.testing.assert_array_equal(bits(other.fb.read(2)), bits(got_c))
    other.fb.postprocess(tonemap=True, min_luminance=1.7)
    want = other.fb.read(3)
    other.close()
    np.testing.assert_array_equal(bits(mapped), bits(want))


# ---- 3. guides from a render -----------------------------------------------------------------
GW, GH = 80, 56


@pytest.fixture(scope="module")
def rendered_guides(hip_ctx):
    from mcrt import lib
    sc = scenes.test_scene()
    ds = lib.DeviceScene(hip_ctx, sc)
    fb = lib.FrameBuffer(hip_ctx, GW, GH)
    cam = scene_camera("mixed", GW, GH)
    fb.render_guides(ds, cam)
    yield sc, ds, fb, cam, fb.read_guides(T.GUIDE_NORMAL_PLANE), fb.read_guides(T.GUIDE_ALBEDO_DEPTH)
    fb.close()
    ds.close()


def test_guide_albedo_normals_and_misses(rendered_guides):
    sc, ds, fb, cam, npl, ad = rendered_guides
    for lod in (False, True):
        fb.render_guides(ds, cam, texture_lod=lod)
        a = fb.read_guides(T.GUIDE_ALBEDO_DEPTH)
        aov = fb.render_aov(ds, cam, T.AOV_ALBEDO, texture_lod=lod)
        np.testing.assert_array_equal(bits(a[..., :3]), bits(aov[..., :3]))
    fb.render_guides(ds, cam)
    hit = ad[..., 3] >= 0
    assert hit.mean() > 0.5
    np.testing.assert_array_equal(ad[~hit], np.broadcast_to(F([0, 0, 0, -1]), ad[~hit].shape))
    np.testing.assert_array_equal(npl[~hit], 0.0)
    n = npl[hit][:, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6
    assert (npl[hit][:, 3] <= 0).all()         # n . (P - cam) <= 0: facing the camera
    assert (ad[hit][:, 3] > 0).all()


def test_guide_normals_of_an_axis_aligned_box(hip_ctx):
    from mcrt import lib
    b = scenes.SceneBuilder("box")
    b.add_mesh(*scenes.box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 2), b.add_material())
    ds = lib.DeviceScene(hip_ctx, b.build())
    W, H = 48, 40
    fb = lib.FrameBuffer(hip_ctx, W, H)
    pos = np.array([3.0, 2.5, -4.0])
    fb.render_guides(ds, make_camera(tuple(pos), (0.0, 0.0, 0.0), W, H))
    npl, ad = fb.read_guides(T.GUIDE_NORMAL_PLANE), fb.read_guides(T.GUIDE_ALBEDO_DEPTH)
    fb.close()
    ds.close()
    hit = ad[..., 3] >= 0
    assert 0.1 < hit.mean() < 0.9              # the box and the background
    np.testing.assert_array_equal(npl[~hit], 0.0)
    np.testing.assert_array_equal(ad[~hit][:, 3], -1.0)
    n = npl[hit][:, :3]
    axis = np.abs(n).argmax(1)
    want = np.zeros_like(n)
    want[np.arange(len(n)), axis] = np.sign(n[np.arange(len(n)), axis])
    assert np.abs(n - want).max() <= 1e-6
    # the visible faces are +x, +y, -z, and the camera-relative offset is that face's plane
    assert set(map(tuple, np.unique(want, axis=0).astype(int))) == {(1, 0, 0), (0, 1, 0), (0, 0, -1)}
    plane = 1.0 - np.abs((want * pos).sum(1))  # n . P - n . cam, P on the face: n . P = 1
    np.testing.assert_allclose(npl[hit][:, 3], plane, atol=1e-5)


def test_guide_depth_against_the_oracle(rendered_guides):
    """Guide depth |P - cam.pos| against the oracle's t |d| for its own camera rays and closest hits.

    Bound, per pixel whose closest hit the float64 ground truth (tests/ray_truth.py) determines, with
    u = 2^-24 and that module's half-widths ht (on t) and hb1, hb2 (on the barycentrics) of the
    determined triangle with edges e1, e2:
      * the oracle's float32 t lies within ht of the true t*, so t |d| within ht |d| of D* = t* |d|;
      * the kernel's hit point P = p0 (1 - b1 - b2) + p1 b1 + p2 b2 uses barycentrics within hb1, hb2
        of the true ones: P moves by at most hb1 |e1| + hb2 |e2|;
      * the three-term interpolation in float32: per coordinate the weight 1 - b1 - b2 (2 roundings),
        three products and two sums on magnitudes <= M (largest coordinate of the vertices and the
        camera), and the object-to-world transform before it (3 products, 3 sums): <= 12 u M per
        coordinate, <= 12 sqrt(3) u M < 21 u M in length;
      * P - cam.pos (1 rounding per coordinate), the dot product (3 products, 2 sums) and the
        square root (1 ulp): <= 8 u D*.
    bound = ht |d| + hb1 |e1| + hb2 |e2| + 21 u M + 8 u D*.  Nothing here is fitted to the kernel."""
    import helpers
    import ray_truth as rt
    from oracle import pyoracle as po
    sc, ds, fb, cam, npl, ad = rendered_guides
    o = po.OracleScene(sc)
    o.build()
    rays = helpers.path_rays(o, cam, frame=0, max_depth=1)[0]
    assert len(rays) == GW * GH
    hits = o.closest(rays)
    tris, sid, pid = rt.world_triangles64(sc)
    tr = rt.classify(tris, rays, shape=sid, prim=pid)
    slot = tr.closest_slot
    det = tr.closest_det & (tr.closest_tri >= 0)
    tri = tr.tri_index(hits["shapeid"], hits["primid"])
    use = det & (tri == tr.closest_tri) & (ad[..., 3].reshape(-1) >= 0)
    assert use.mean() > 0.5, use.mean()
    s = slot[use]
    d = rays["d"][use, :3].astype(np.float64)
    ld = np.linalg.norm(d, axis=1)
    tt = tris[tr.tri[s]]
    le1 = np.linalg.norm(tt[:, 1] - tt[:, 0], axis=1)
    le2 = np.linalg.norm(tt[:, 2] - tt[:, 0], axis=1)
    M = np.maximum(np.abs(tt).reshape(len(tt), 9).max(1), np.abs(rays["o"][use, :3]).max(1))
    ref = hits["uvwt"][use, 3].astype(np.float64) * ld
    dstar = tr.t[s] * ld
    bound = tr.ht[s] * ld + tr.hb1[s] * le1 + tr.hb2[s] * le2 + 21 * rt.U * M + 8 * rt.U * dstar
    err = np.abs(ad[..., 3].reshape(-1)[use].astype(np.float64) - ref)
    print(f"guide depth: {use.sum()} pixels, max |err| {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), (err.max(), np.max(err / bound))
    # the plane offset agrees with the normal and the oracle's hit point to the same bound (|n| = 1)
    P = rays["o"][use, :3].astype(np.float64) + hits["uvwt"][use, 3:4].astype(np.float64) * d
    off = (npl.reshape(-1, 4)[use, :3].astype(np.float64) * (P - rays["o"][use, :3].astype(np.float64))).sum(1)
    assert (np.abs(npl.reshape(-1, 4)[use, 3] - off) <= bound + 8 * rt.U * dstar).all()


def test_guide_bands_restrict_the_rows(rendered_guides, hip_ctx):
    import torch
    sc, ds, fb, cam, npl, ad = rendered_guides
    sentinel = torch.full((GH * GW * 4,), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fb.set_guides(sentinel.data_ptr(), sentinel.data_ptr())
    fb.render_guides(ds, cam, band_rows=8, num_bands=2, band_index=1)
    n1, a1 = fb.read_guides(T.GUIDE_NORMAL_PLANE), fb.read_guides(T.GUIDE_ALBEDO_DEPTH)
    own = ((np.arange(GH) // 8) % 2) == 1
    np.testing.assert_array_equal(bits(n1[own]), bits(npl[own]))
    np.testing.assert_array_equal(bits(a1[own]), bits(ad[own]))
    np.testing.assert_array_equal(n1[~own], 7.5)
    np.testing.assert_array_equal(a1[~own], 7.5)
    fb.render_guides(ds, cam)   # whole image again for the other tests


# ---- 4. moments -------------------------------------------------------------------------------
def test_moments_follow_the_accumulated_frames(hip_ctx):
    from mcrt import lib
    W, H, n = 40, 24, 6
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    cam = scene_camera("mixed", W, H)
    box = T.make_filter(T.BOX)
    fb, plain = lib.FrameBuffer(hip_ctx, W, H), lib.FrameBuffer(hip_ctx, W, H)
    fb.enable_moments()
    frames = []
    for f in range(n):
        for b in (fb, plain):
            b.render(ds, cam, frame=f, max_depth=2)
            b.accumulate(box, f)
        frames.append(fb.read_frame(0))
        if f == 2:
            after3 = fb.read_guides(T.GUIDE_MOMENTS)
    np.testing.assert_array_equal(bits(fb.read_guides(T.GUIDE_MOMENTS)), bits(ar.accumulate_moments(frames)))
    assert fb.read_guides(T.GUIDE_MOMENTS)[..., 0].max() > 0
    # the image and the weighted sums do not notice the moments
    for which in (1, 2):
        np.testing.assert_array_equal(bits(fb.read(which)), bits(plain.read(which)))
    # frame 0 resets
    fb.render(ds, cam, frame=0, max_depth=2)
    fb.accumulate(box, 0)
    np.testing.assert_array_equal(bits(fb.read_guides(T.GUIDE_MOMENTS)), bits(ar.accumulate_moments(frames[:1])))
    # a batch of three frames = three single frames
    fb.render_frames(ds, [cam, cam, cam], frame=0, max_depth=2)
    fb.accumulate_frames([box, box, box], 0)
    np.testing.assert_array_equal(bits(fb.read_guides(T.GUIDE_MOMENTS)), bits(after3))
    for k in range(3):
        np.testing.assert_array_equal(bits(fb.read_frame(k)), bits(frames[k]))
    fb.close()
    plain.close()
    ds.close()


# ---- 5. it denoises ----------------------------------------------------------------------------
def test_it_denoises_a_4spp_render(hip_ctx):
    """test_scene(), "mixed" camera, 64x48, depth 2: 4 frames accumulated with the box filter and
    the moments, denoised with the defaults; ground truth = the mean of frames 16..271.  The
    tone-mapped (x / (1 + x)) RMSE of the denoised image must be below the 4-spp image's.

    The same inequality evaluated on the CPU beforehand, with the oracle's frames, geometric normals
    as guides, no demodulation and tests/atrous_ref.py: 4 spp 0.1635 -> 0.1129 with the variance
    guidance, 0.1249 without it (raw RMSE 0.411 -> 0.261 and 0.266)."""
    from mcrt import lib
    W, H = 64, 48
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    cam = scene_camera("mixed", W, H)
    box = T.make_filter(T.BOX)
    truth_fb = lib.FrameBuffer(hip_ctx, W, H)
    for i, f0 in enumerate(range(16, 272, 64)):
        truth_fb.render_frames(ds, [cam] * 64, frame=f0, max_depth=2)
        # accumulation index i * 64: 0 starts the sum; the frames keep their own sampler index f0 + k
        truth_fb.accumulate_frames([box], i * 64)
    truth = truth_fb.read(2)
    truth_fb.close()
    fb = lib.FrameBuffer(hip_ctx, W, H)
    fb.enable_moments()
    for f in range(4):
        fb.render(ds, cam, frame=f, max_depth=2)
        fb.accumulate(box, f)
    fb.render_guides(ds, cam)
    noisy = fb.read(2)
    base = tm_rmse(noisy, truth)
    for use_var in (True, False):
        fb.denoise_guided(use_variance=use_var)
        out = fb.read(3)
        assert np.isfinite(out).all()
        e = tm_rmse(out, truth)
        print(f"tone-mapped RMSE: 4 spp {base:.4f} -> denoised {e:.4f} (use_variance={use_var})")
        assert e < base, (e, base)
    np.testing.assert_array_equal(bits(fb.read(2)), bits(noisy))   # the image itself is not touched
    fb.close()
    ds.close()


# ---- 6. errors and ordering ----------------------------------------------------------------------
def test_status_codes(hip_ctx):
    import ctypes
    from mcrt import lib
    OK, INVALID, NOT_READY = 0, 1, 4
    L = lib.lib()
    fb = lib.FrameBuffer(hip_ctx, 16, 16)
    good = T.GuidedDenoiseParams(5, 0.1, 0.02, 4.0, 1, 1, 0, 2.0)
    assert L.mcrt_denoise_guided(None, ctypes.byref(good)) == INVALID
    assert L.mcrt_denoise_guided(fb.h, None) == INVALID
    assert L.mcrt_denoise_guided(fb.h, ctypes.byref(good)) == NOT_READY   # no guides yet
    assert L.mcrt_framebuffer_read_guides(fb.h, 0, ctypes.c_void_p(1), 1 << 30, None) == NOT_READY
    assert L.mcrt_framebuffer_set_guides(fb.h, None, None) == INVALID
    assert L.mcrt_framebuffer_set_moments(fb.h, None, 2) == INVALID
    assert L.mcrt_render_guides(None, fb.h, None, None) == INVALID
    need = ctypes.c_uint64()
    assert L.mcrt_framebuffer_read_guides(fb.h, 2, None, 0, ctypes.byref(need)) == OK and need.value == 16 * 16 * 8
    assert L.mcrt_framebuffer_read_guides(fb.h, 4, None, 0, None) == INVALID
    img, npl, ad, mom = _synthetic(16, 16, 1)
    inst = Installed(hip_ctx, dict(img=img, npl=npl, ad=ad))
    for bad in (dict(levels=0), dict(levels=9), dict(sigma_normal=0.0), dict(sigma_depth=-1.0),
                dict(sigma_luminance=0.0)):
        with pytest.raises(lib.MCRTError, match="status 1"):
            inst.fb.denoise_guided(**bad)
    # use_variance without moments, or with fewer than two frames in them, degrades to var = 1
    want = inst.run(levels=2, use_variance=False, demodulate_albedo=False)
    got = inst.run(levels=2, use_variance=True, demodulate_albedo=False)
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
    inst.fb.enable_moments()
    got = inst.run(levels=2, use_variance=True, demodulate_albedo=False)
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
    inst.close()
    fb.close()
    # a band-split BDPT frame waiting for its gather: not ready until mcrt_bdpt_gather
    W, H = 32, 16
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    cam = scene_camera("mixed", W, H)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    fb.render_guides(ds, cam)
    fb.render(ds, cam, frame=0, max_depth=2, integrator=T.INTEGRATOR_BDPT, band_rows=8, num_bands=2, band_index=0)
    assert L.mcrt_denoise_guided(fb.h, ctypes.byref(good)) == NOT_READY
    fb.bdpt_gather(None)
    fb.accumulate(T.make_filter(T.BOX), 0)
    assert L.mcrt_denoise_guided(fb.h, ctypes.byref(good)) == OK
    assert np.isfinite(fb.read(3)).all()
    fb.close()
    ds.close()


def test_ordering_with_frames_in_flight_and_postprocess_untouched(hip_ctx):
    from mcrt import lib
    W, H = 64, 48
    ds = lib.DeviceScene(hip_ctx, scenes.test_scene())
    cam = scene_camera("mixed", W, H)
    box = T.make_filter(T.BOX)

    def sequence(sync):
        fb = lib.FrameBuffer(hip_ctx, W, H)
        fb.set_frames_in_flight(2)
        fb.enable_moments()
        step = hip_ctx.sync if sync else (lambda: None)
        fb.render_guides(ds, cam)
        step()
        for f in range(3):
            fb.render(ds, cam, frame=f, max_depth=2)
            step()
            fb.accumulate(box, f)
            step()
        fb.render(ds, cam, frame=3, max_depth=2)   # in flight on its slot's stream, never accumulated
        step()
        fb.denoise_guided()
        step()
        return fb, fb.read(3), fb.read_guides(T.GUIDE_FILTERED_VARIANCE)

    fb, out, var = sequence(False)
    fb2, out2, var2 = sequence(True)
    np.testing.assert_array_equal(bits(out), bits(out2))
    np.testing.assert_array_equal(bits(var), bits(var2))
    fb2.close()
    img = fb.read(2)
    assert np.abs(out - img).max() > 0
    fb.postprocess()
    np.testing.assert_array_equal(bits(fb.read(3)), bits(img))   # the plain image, as before
    fb.postprocess(denoise=True, radius=2, sigma_spatial=1.5, sigma_range=0.3)
    bilateral = fb.read(3)
    fb.denoise_guided()
    fb.postprocess(denoise=True, radius=0)   # writes nothing: shows the bilateral pass's own image
    np.testing.assert_array_equal(bits(fb.read(3)), bits(bilateral))
    fb.close()
    ds.close()
