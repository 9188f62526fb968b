"""numpy restatement of the temporal history kernels (k_temporal in both its forms, k_temporal_var
in csrc/mcrt_denoise.hip; mcrt_temporal_accumulate and mcrt_temporal_accumulate_motion in
include/mcrt_capi.h) and a float64 analytic scene that makes consistent guides for any camera.

Every array is float32 and every line is one float32 operation in the order the comments above the
two kernels fix; division and square root are IEEE on both sides and no transcendental is involved,
so the restatement is operation for operation.  Planes are (H, W, C) arrays as in atrous_ref.py;
the moments history is (H, W, 4) = (mu1, mu2, N, z).  Cameras are mcrt.camera.make_camera records.
"""
import numpy as np

from atrous_ref import _demod, luminance

F = np.float32
DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, max_history=32, min_history=4, normal_threshold=0.1,
                plane_threshold=0.01)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cam3(cam, name):
    return np.asarray(cam[name], F).reshape(-1)[:3].copy()


def pixel_dirs(cam, W, H, dtype=F):
    """m of the kernel comment: the corner directions blended at (x / W, y / H), not normalised."""
    T = dtype
    u = (np.arange(W, dtype=T) / T(W))[None, :, None]
    v = (np.arange(H, dtype=T) / T(H))[:, None, None]
    r00, r10, r11, r01 = (_cam3(cam, k).astype(T) for k in ("r00", "r10", "r11", "r01"))
    a = r00 + (r10 - r00) * u
    b = r01 + (r11 - r01) * u
    return a + (b - a) * v


def reproject(ad, cam, prev, motion=None):
    """(r, fx, fy, ok): r = P - prev.pos per pixel (through the motion records where their flag is
    1), the history position in pixels, and whether the pixel gets as far as the taps (a hit, no
    negative motion flag, in front of prev, inside the guard band)."""
    ad = np.asarray(ad, F)
    H, W = ad.shape[:2]
    mv = np.zeros((H, W, 4), F) if motion is None else np.asarray(motion, F)
    m = pixel_dirs(cam, W, H)
    depth = ad[..., 3]
    hit = (depth > 0) & ~(mv[..., 3] < F(0))
    with np.errstate(all="ignore"):
        k = depth / np.sqrt(_dot3(m, m))
        dpos = _cam3(cam, "pos") - _cam3(prev, "pos")
        r = m * k[..., None] + dpos
        r = np.where((mv[..., 3] == F(1))[..., None], r + mv[..., :3], r)
        M = np.asarray(prev["worldToClip"], F).reshape(4, 4)
        cx = (M[0, 0] * r[..., 0] + M[0, 1] * r[..., 1]) + M[0, 2] * r[..., 2]
        cy = (M[1, 0] * r[..., 0] + M[1, 1] * r[..., 1]) + M[1, 2] * r[..., 2]
        cw = (M[3, 0] * r[..., 0] + M[3, 1] * r[..., 1]) + M[3, 2] * r[..., 2]
        front = hit & (cw > 0)
        fx = ((cx / cw + F(1)) * F(0.5)) * F(W)
        fy = ((cy / cw + F(1)) * F(0.5)) * F(H)
        ok = front & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
    return r, fx, fy, ok


def accumulate(image, normal_plane, albedo_depth, cam, history=None, motion=None, prev_normal=None, alpha=0.2,
               alpha_moments=0.2, max_history=32, normal_threshold=0.1, plane_threshold=0.01, demodulate_albedo=False,
               info=None, use_prev_normal=True, **_ignored):
    """k_temporal, both forms.  history = (colour, moments, normal_plane, prev_cam) or None; motion =
    (H, W, 4) records (P_prev - P, flag) and prev_normal = (H, W, 4) records (n_prev, 0) restate
    MOTION = true, motion=None is MOTION = false and behaves as an all-zero plane: the motion record
    is added to r where its flag is 1, the normal test then compares the history tap with the
    previous normal, and a negative flag tests no tap.  use_prev_normal=False keeps gp = g on moved
    pixels too (what the rule would do without the previous-normal plane; tests only).  Returns the
    new (colour, moments, normal_plane) planes; `info` (a dict) receives per pixel the number of valid
    taps, the tap corner (ix, iy), the history position and the reprojection flag."""
    img = np.asarray(image, F)
    g = np.asarray(normal_plane, F)
    ad = np.asarray(albedo_depth, F)
    H, W = ad.shape[:2]
    gp = g[..., :3]
    if motion is not None and use_prev_normal:
        gp = np.where((np.asarray(motion, F)[..., 3] == F(1))[..., None], np.asarray(prev_normal, F)[..., :3], gp)
    c = img.copy()
    if demodulate_albedo:
        c[..., :3] = c[..., :3] / _demod(ad)
    l = luminance(c)
    ll = l * l
    sw = np.zeros((H, W), F)
    sc = np.zeros((H, W, 3), F)
    s1, s2, sn = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    nvalid = np.zeros((H, W), int)
    ok = np.zeros((H, W), bool)
    if history is not None:
        hc, hm, hn, prev = history
        hc, hm, hn = np.asarray(hc, F), np.asarray(hm, F), np.asarray(hn, F)
        r, fx, fy, ok = reproject(ad, cam, prev, motion)
        fxs, fys = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        ix, iy = np.floor(fxs).astype(np.int64), np.floor(fys).astype(np.int64)
        tx, ty = fxs - ix.astype(F), fys - iy.astype(F)
        with np.errstate(all="ignore"):
            zr = np.sqrt(_dot3(r, r))
            tol = F(plane_threshold) * zr
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cqx, cqy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    m_q, n_q, c_q = hm[cqy, cqx], hn[cqy, cqx], hc[cqy, cqx]
                    dn = gp - n_q[..., :3]
                    res = np.abs(_dot3(n_q, r) - n_q[..., 3])
                    valid = inside & (m_q[..., 3] > 0) & (_dot3(dn, dn) <= F(normal_threshold)) & (res <= tol)
                    w = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                    sw = np.where(valid, sw + w, sw)
                    sc = np.where(valid[..., None], sc + w[..., None] * c_q[..., :3], sc)
                    s1 = np.where(valid, s1 + w * m_q[..., 0], s1)
                    s2 = np.where(valid, s2 + w * m_q[..., 1], s2)
                    sn = np.where(valid, sn + w * m_q[..., 2], sn)
                    nvalid += valid
        if info is not None:
            info.update(ix=ix, iy=iy, fx=fx, fy=fy, r=r)
    have = sw > F(1e-4)
    with np.errstate(all="ignore"):
        N = np.minimum(sn / sw + F(1), F(max_history))
        al = np.maximum(F(alpha), F(1) / N)
        am = np.maximum(F(alpha_moments), F(1) / N)
        out = (sc / sw[..., None]) * (F(1) - al)[..., None] + c[..., :3] * al[..., None]
        mu1 = (s1 / sw) * (F(1) - am) + l * am
        mu2 = (s2 / sw) * (F(1) - am) + ll * am
    colour = c.copy()
    colour[..., :3] = np.where(have[..., None], out, c[..., :3])
    moments = np.stack([np.where(have, mu1, l), np.where(have, mu2, ll), np.where(have, N, F(1)), ad[..., 3]],
                       -1).astype(F)
    if info is not None:
        info.update(valid_taps=nvalid, reprojected=ok, have=have)
    return colour.astype(F), moments, g.copy()


def variance(moments, normal_plane, min_history=4, normal_threshold=0.1, plane_threshold=0.01, **_ignored):
    """k_temporal_var over the planes `accumulate` returned."""
    mo = np.asarray(moments, F)
    g = np.asarray(normal_plane, F)
    H, W = mo.shape[:2]
    mu1, mu2, N, z = (mo[..., k] for k in range(4))
    hit = z > 0
    t = F(plane_threshold) * z
    t2 = t * t
    s1, s2, cnt = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            if dx == 0 and dy == 0:
                same = np.ones((y1 - y0, x1 - x0), bool)
            else:
                dn = g[P][..., :3] - g[Q][..., :3]
                dd = g[P][..., 3] - g[Q][..., 3]
                both = hit[P] & hit[Q] & (_dot3(dn, dn) <= F(normal_threshold)) & (dd * dd <= t2[P])
                same = np.where(hit[P], both, ~hit[Q])
            s1[P] = np.where(same, s1[P] + mu1[Q], s1[P])
            s2[P] = np.where(same, s2[P] + mu2[Q], s2[P])
            cnt[P] = np.where(same, cnt[P] + F(1), cnt[P])
    m1, m2 = s1 / cnt, s2 / cnt
    spatial = np.maximum(F(0), m2 - m1 * m1) * (F(min_history) / N)
    return np.where(N >= F(min_history), np.maximum(F(0), mu2 - mu1 * mu1), spatial).astype(F)


# ---- the analytic scene ------------------------------------------------------------------------
# id 1 floor y = 0 (|x| < 3, -6 < z < 2); id 2 wall z = 2 (|x| < 3, 0 < y < 2.2); id 3 a floating
# square z = 0.5 (|x| < 0.5, 0.3 < y < 1.3); id 0 everything else.  The square and the wall share a
# normal, so only the plane test separates them.
SURFACES = (
    (1, 1, 0.0, ((0, -3.0, 3.0), (2, -6.0, 2.0))),
    (2, 2, 2.0, ((0, -3.0, 3.0), (1, 0.0, 2.2))),
    (3, 2, 0.5, ((0, -0.5, 0.5), (1, 0.3, 1.3))),
)


def scene_guides(cam, offset=(0.0, 0.0, 0.0)):
    """Per-pixel (surface id (H, W) int, normal-plane (H, W, 4) float32, depth (H, W) float32, -1 on
    a miss) of the scene moved by `offset` seen through `cam`, evaluated in float64 relative to the
    camera position (so the guides are as good far from the origin as near it)."""
    W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
    m = pixel_dirs(cam, W, H, np.float64)
    rel = np.asarray(offset, np.float64) - _cam3(cam, "pos").astype(np.float64)   # scene origin - cam.pos
    best = np.full((H, W), np.inf)
    sid = np.zeros((H, W), int)
    npl = np.zeros((H, W, 4))
    with np.errstate(all="ignore"):
        for ident, axis, coord, bounds in SURFACES:
            t = (coord + rel[axis]) / m[..., axis]
            ok = np.isfinite(t) & (t > 0) & (t < best)
            for ax, lo, hi in bounds:
                q = m[..., ax] * t - rel[ax]          # scene-local coordinate of the hit
                ok &= (q > lo) & (q < hi)
            n = np.zeros(3)
            n[axis] = 1.0
            nm = m[..., axis]                          # n . m
            sign = np.where(nm > 0, -1.0, 1.0)         # face the camera
            best = np.where(ok, t, best)
            sid = np.where(ok, ident, sid)
            npl = np.where(ok[..., None], np.concatenate([sign[..., None] * n, (sign * nm * t)[..., None]], -1), npl)
    hit = sid > 0
    depth = np.where(hit, np.where(hit, best, 0.0) * np.linalg.norm(m, axis=-1), -1.0)
    return sid, npl.astype(F), depth.astype(F)
