"""The numpy restatement of the guided a-trous denoiser (tests/atrous_ref.py) checked on its own,
without a GPU: the properties the filter is built for, on inputs small enough to reason about.
One line checks that the library exports the entry point at all."""
import numpy as np

import atrous_ref as ar

F = np.float32


def _flat_guides(H, W, normal=(0.0, 0.0, -1.0), offset=-3.0, depth=3.0, albedo=0.5):
    npl = np.zeros((H, W, 4), F)
    npl[..., :3] = normal
    npl[..., 3] = offset
    ad = np.full((H, W, 4), albedo, F)
    ad[..., 3] = depth
    return npl, ad


def _two_planes(H, W):
    """Left half: a plane facing -z at offset -3; right half: a plane facing -x at offset -5."""
    npl, ad = _flat_guides(H, W)
    npl[:, W // 2:, :3] = (-1.0, 0.0, 0.0)
    npl[:, W // 2:, 3] = -5.0
    ad[:, W // 2:, 3] = 5.5
    return npl, ad


def test_constant_image_is_unchanged():
    H, W = 23, 31
    npl, ad = _two_planes(H, W)
    img = np.empty((H, W, 4), F)
    img[...] = (0.3, 1.7, 0.05, 0.9)
    for use_var in (False, True):
        mom = np.stack([np.full((H, W), 4.0, F), np.full((H, W), 4.5, F)], -1)
        out, var = ar.denoise(img, npl, ad, mom, 4, use_variance=use_var)
        # every level is a normalised average of equal values: sum(w c) / sum(w) within an ulp of c
        np.testing.assert_array_max_ulp(out[..., :3], img[..., :3], maxulp=1)
        np.testing.assert_array_equal(out[..., 3], img[..., 3])
        one, _ = ar.level(img, np.ones((H, W), F), npl, ad, 1, 0.1, 0.02, 4.0, False)
        np.testing.assert_array_max_ulp(one[..., :3], img[..., :3], maxulp=1)


def test_two_surfaces_do_not_mix():
    H, W = 24, 40
    rng = np.random.default_rng(3)
    npl, ad = _two_planes(H, W)
    img = rng.uniform(0.2, 1.0, (H, W, 4)).astype(F)
    other = img.copy()
    other[:, W // 2:, :3] = rng.uniform(5.0, 9.0, (H, W - W // 2, 3)).astype(F)   # change the right side only
    a, va = ar.denoise(img, npl, ad, use_variance=False)
    b, vb = ar.denoise(other, npl, ad, use_variance=False)
    np.testing.assert_allclose(a[:, :W // 2], b[:, :W // 2], rtol=0, atol=1e-6)
    np.testing.assert_allclose(va[:, :W // 2], vb[:, :W // 2], rtol=0, atol=1e-6)
    assert np.abs(a[:, W // 2:] - b[:, W // 2:]).max() > 1.0
    # and each side is really filtered: the noise inside a side shrinks
    assert a[:, :W // 2, :3].std() < 0.5 * img[:, :W // 2, :3].std()


def test_all_miss_image_is_one_region():
    H, W = 20, 20
    rng = np.random.default_rng(5)
    npl = np.zeros((H, W, 4), F)
    ad = np.zeros((H, W, 4), F)
    ad[..., 3] = -1.0
    img = (1.0 + 0.05 * rng.standard_normal((H, W, 4))).astype(F)
    out, _ = ar.denoise(img, npl, ad, use_variance=False, sigma_luminance=100.0)
    assert np.isfinite(out).all()
    # misses against misses have e = 0 but for the (wide) luminance term: the whole image averages
    assert out[..., :3].std() < 0.15 * img[..., :3].std()
    # a miss next to hits keeps to itself
    npl2, ad2 = _flat_guides(H, W)
    npl2[:, :5] = 0.0
    ad2[:, :5] = (0.0, 0.0, 0.0, -1.0)
    img2 = img.copy()
    img2[:, :5, :3] = 7.0
    out2, _ = ar.denoise(img2, npl2, ad2, use_variance=False, sigma_luminance=100.0)
    np.testing.assert_allclose(out2[:, :5, :3], 7.0, rtol=1e-6)


def test_variance_of_iid_noise_falls_at_every_level():
    H, W, n = 48, 48, 8
    rng = np.random.default_rng(11)
    npl, ad = _flat_guides(H, W)
    frames = (1.0 + 0.2 * rng.standard_normal((n, H, W, 3))).astype(F)
    mom = ar.accumulate_moments(frames)
    img = np.concatenate([frames.mean(0), np.ones((H, W, 1), F)], -1).astype(F)
    c, var = ar.prepare(img, ad, mom, n)
    assert abs(float(var.mean()) - 0.2 ** 2 * (0.212671 ** 2 + 0.715160 ** 2 + 0.072169 ** 2) / n) < 2e-4
    measured, estimated = [float(ar.luminance(c).var())], [float(var.mean())]
    for i in range(5):
        c, var = ar.level(c, var, npl, ad, 1 << i, 0.1, 0.02, 4.0, True)
        measured.append(float(ar.luminance(c).var()))
        estimated.append(float(var.mean()))
    assert all(b < a for a, b in zip(measured, measured[1:])), measured
    assert all(b < a for a, b in zip(estimated, estimated[1:])), estimated


def test_moments_are_sequential_float32_sums_and_frame_zero_resets():
    rng = np.random.default_rng(13)
    frames = (10.0 ** rng.uniform(-3, 3.5, (5, 6, 7, 4))).astype(F)   # some above the 1000 clamp
    m = ar.accumulate_moments(frames)
    m2 = ar.accumulate_moments(frames[3:], ar.accumulate_moments(frames[:3]))
    np.testing.assert_array_equal(m, m2)
    l0 = ar.luminance(np.minimum(frames[0, ..., :3], F(1000)))
    np.testing.assert_array_equal(ar.accumulate_moments(frames[:1])[..., 0], l0)
    assert m.dtype == F
    # a NaN radiance counts as 0 (the device's clamp returns its lower bound for NaN)
    holed = frames.copy()
    holed[2, 1, 1, :3] = np.nan
    zeroed = frames.copy()
    zeroed[2, 1, 1, :3] = 0
    np.testing.assert_array_equal(ar.accumulate_moments(holed), ar.accumulate_moments(zeroed))


def test_library_exports_guided_denoise():
    from mcrt import lib
    MCRT_ERROR_INVALID_ARG = 1
    assert lib.lib().mcrt_denoise_guided(None, None) == MCRT_ERROR_INVALID_ARG
