"""numpy restatement of the guided a-trous denoiser (csrc/mcrt_denoise.hip, include/mcrt_capi.h).

Every array is float32 and every line is one float32 operation in the order the comment above
k_atrous fixes; only exp is evaluated in float64 and rounded to float32 (the device's expf is
within an ulp of that).  Planes are (H, W, C) arrays: colour (H, W, 4), normal-plane (H, W, 4) =
(n, n.(P - cam)), albedo-depth (H, W, 4) = (Kd, depth; -1 on a miss), variance (H, W), moments
(H, W, 2) = (sum l, sum l*l).
"""
import numpy as np

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)
G3 = np.array([0.25, 0.5, 0.25], F)
DEFAULTS = dict(levels=5, sigma_normal=0.1, sigma_depth=0.02, sigma_luminance=4.0)


def luminance(rgb):
    """k_tonemap's coefficients, summed left to right."""
    rgb = np.asarray(rgb, F)
    return (F(0.212671) * rgb[..., 0] + F(0.715160) * rgb[..., 1]) + F(0.072169) * rgb[..., 2]


def guides_from_arrays(normals, points, albedo, hit, cam_pos):
    """Guide planes from per-pixel shading normals, hit points, albedo (H, W, 3 each), a hit mask
    (H, W) and the camera position: normals flipped to face the camera, camera-relative offsets."""
    n = np.asarray(normals, F).copy()
    v = np.asarray(points, F) - np.asarray(cam_pos, F)
    off = (n[..., 0] * v[..., 0] + n[..., 1] * v[..., 1]) + n[..., 2] * v[..., 2]
    flip = off > 0
    n[flip] = -n[flip]
    off = np.where(flip, -off, off).astype(F)
    depth = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(F)
    hit = np.asarray(hit, bool)
    npl = np.zeros(hit.shape + (4,), F)
    ad = np.zeros(hit.shape + (4,), F)
    ad[..., 3] = -1.0
    npl[hit] = np.concatenate([n, off[..., None]], -1)[hit]
    ad[hit] = np.concatenate([np.asarray(albedo, F), depth[..., None]], -1)[hit]
    return npl, ad


def cl_clamp(x, lo, hi):
    """The device's clamp (v_med3_f32) = OpenCL's fmin(fmax(x, lo), hi): a NaN x gives lo (np.clip
    would pass the NaN on)."""
    return np.fmin(np.fmax(np.asarray(x, F), F(lo)), F(hi))


def accumulate_moments(frames, moments=None):
    """k_moments: sequential float32 sums over `frames` (each (H, W, >=3) radiance); moments None
    starts at frame 0 (overwrite).  A NaN radiance counts as 0, as in k_accumulate."""
    for k, fr in enumerate(frames):
        l = luminance(cl_clamp(np.asarray(fr, F)[..., :3], 0, 1000))
        ll = l * l
        if moments is None:
            moments = np.stack([l, ll], -1).astype(F)
        else:
            moments = np.stack([moments[..., 0] + l, moments[..., 1] + ll], -1).astype(F)
    return moments


def _demod(albedo_depth):
    a = np.asarray(albedo_depth, F)[..., :3]
    return np.where(a > F(1e-3), a, F(1)).astype(F)


def prepare(image, albedo_depth, moments=None, frames=0, demodulate=False):
    """Level 0 input (k_atrous_prep): colour and variance.  moments None or frames < 2: var = 1."""
    c = np.asarray(image, F).copy()
    if demodulate:
        c[..., :3] = c[..., :3] / _demod(albedo_depth)
    if moments is not None and frames >= 2:
        m = np.asarray(moments, F)
        n = F(frames)
        mean = m[..., 0] / n
        var = np.maximum(F(0), m[..., 1] / n - mean * mean) / (n - F(1))
    else:
        var = np.ones(c.shape[:2], F)
    return c, var.astype(F)


def level(colour, var, normal_plane, albedo_depth, step, sigma_normal, sigma_depth, sigma_level, use_variance,
          remodulate=False):
    """One level of step `step` (k_atrous): returns (colour', var')."""
    c = np.asarray(colour, F)
    var = np.asarray(var, F)
    npl = np.asarray(normal_plane, F)
    ad = np.asarray(albedo_depth, F)
    H, W = var.shape
    isn2 = F(1) / (F(sigma_normal) * F(sigma_normal))
    sl2 = F(sigma_level) * F(sigma_level)
    zp = np.where(ad[..., 3] > 0, ad[..., 3], F(1)).astype(F)
    sdz = F(sigma_depth) * zp
    isd2 = F(1) / (sdz * sdz)
    if use_variance:
        vp = np.zeros((H, W), F)
        ys, xs = np.arange(H), np.arange(W)
        for j in (-1, 0, 1):
            yy = np.clip(ys + j, 0, H - 1)
            for i in (-1, 0, 1):
                xx = np.clip(xs + i, 0, W - 1)
                vp = vp + (G3[j + 1] * G3[i + 1]) * var[yy][:, xx]
    else:
        vp = np.ones((H, W), F)
    idl2 = F(1) / (sl2 * vp + F(1e-8))
    lum = luminance(c)
    sw = np.zeros((H, W), F)
    sc = np.zeros((H, W, 3), F)
    sv = np.zeros((H, W), F)
    with np.errstate(over="ignore", under="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = step * dy, step * dx
                # centre window [y0:y1, x0:x1] whose tap (y + oy, x + ox) is inside the image
                y0, y1 = max(0, -oy), min(H, H - oy)
                x0, x1 = max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                dn = npl[P][..., :3] - npl[Q][..., :3]
                dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                dd = npl[P][..., 3] - npl[Q][..., 3]
                dl = lum[P] - lum[Q]
                e = (dn2 * isn2 + (dd * dd) * isd2[P]) + (dl * dl) * idl2[P]
                w = (H5[dx + 2] * H5[dy + 2]) * np.exp(-e.astype(np.float64)).astype(F)
                sw[P] = sw[P] + w
                sc[P] = sc[P] + w[..., None] * c[Q][..., :3]
                sv[P] = sv[P] + (w * w) * var[Q]
    out = np.empty_like(c)
    out[..., :3] = sc / sw[..., None]
    out[..., 3] = c[..., 3]
    if remodulate:
        out[..., :3] = out[..., :3] * _demod(ad)
    return out, (sv / (sw * sw)).astype(F)


def sigma_of_level(i, sigma_luminance, use_variance):
    return F(sigma_luminance) if use_variance else F(sigma_luminance) * F(2.0 ** -i)


def denoise(image, normal_plane, albedo_depth, moments=None, frames=0, levels=5, sigma_normal=0.1, sigma_depth=0.02,
            sigma_luminance=4.0, use_variance=True, demodulate_albedo=False):
    """The full chain of mcrt_denoise_guided (without tone mapping): (display, filtered variance)."""
    use_var = bool(use_variance) and moments is not None and frames >= 2
    c, var = prepare(image, albedo_depth, moments if use_var else None, frames, demodulate_albedo)
    for i in range(levels):
        c, var = level(c, var, normal_plane, albedo_depth, 1 << i, sigma_normal, sigma_depth,
                       sigma_of_level(i, sigma_luminance, use_var), use_var,
                       remodulate=bool(demodulate_albedo) and i + 1 == levels)
    return c, var
