"""numpy restatement of k_temporal's MOTION form (csrc/mcrt_denoise.hip; mcrt_temporal_accumulate_motion
in include/mcrt_capi.h) and a float64 analytic scene with one moving object.

`accumulate` is temporal_ref.accumulate with the lines the kernel comment lists changed: the motion
record is added to r where its flag is 1, the normal test then compares the history tap with the
previous normal, and a negative flag tests no tap.  Every array is float32 and every line one
float32 operation in the kernel's order, as in temporal_ref.py.

The scene is temporal_ref.SURFACES' floor and wall plus a unit rectangle (object space: the plane
z = 0, |x| < 0.5, |y| < 0.5, normal +z) under a rigid pose (R, t) per frame: world = R q + t.  The
pose REST puts it where temporal_ref's floating square is.
"""
import numpy as np

import temporal_ref as tr
from atrous_ref import _demod, luminance
from temporal_ref import F, _cam3, _dot3, pixel_dirs, reproject   # noqa: F401  (re-exported)

RECT_ID = 3
REST = (np.eye(3), np.array([0.0, 0.8, 0.5]))


def rot_y(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def pose(translate=(0.0, 0.0, 0.0), turn_deg=0.0):
    """REST turned about the vertical axis through the rectangle's centre, then translated."""
    return rot_y(turn_deg) @ REST[0], REST[1] + np.asarray(translate, np.float64)


def accumulate(image, normal_plane, albedo_depth, cam, history=None, motion=None, prev_normal=None, alpha=0.2,
               alpha_moments=0.2, max_history=32, normal_threshold=0.1, plane_threshold=0.01, demodulate_albedo=False,
               info=None, use_prev_normal=True, **_ignored):
    """k_temporal_motion.  history = (colour, moments, normal_plane, prev_cam) or None; motion =
    (H, W, 4) records (P_prev - P, flag), prev_normal = (H, W, 4) records (n_prev, 0).
    use_prev_normal=False keeps gp = g on moved pixels too (what the rule would do without the
    previous-normal plane; tests only).  Returns and `info` as temporal_ref.accumulate."""
    img = np.asarray(image, F)
    g = np.asarray(normal_plane, F)
    ad = np.asarray(albedo_depth, F)
    mv = np.asarray(motion, F)
    pnrm = np.asarray(prev_normal, F)
    H, W = ad.shape[:2]
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
        moved = mv[..., 3] == F(1)
        with np.errstate(all="ignore"):
            m = pixel_dirs(cam, W, H)
            depth = ad[..., 3]
            k = depth / np.sqrt(_dot3(m, m))
            dpos = _cam3(cam, "pos") - _cam3(prev, "pos")
            r = m * k[..., None] + dpos
            r = np.where(moved[..., None], r + mv[..., :3], r)
            gp = np.where(moved[..., None], pnrm[..., :3], g[..., :3]) if use_prev_normal else g[..., :3]
            M = np.asarray(prev["worldToClip"], F).reshape(4, 4)
            cx = (M[0, 0] * r[..., 0] + M[0, 1] * r[..., 1]) + M[0, 2] * r[..., 2]
            cy = (M[1, 0] * r[..., 0] + M[1, 1] * r[..., 1]) + M[1, 2] * r[..., 2]
            cw = (M[3, 0] * r[..., 0] + M[3, 1] * r[..., 1]) + M[3, 2] * r[..., 2]
            fx = ((cx / cw + F(1)) * F(0.5)) * F(W)
            fy = ((cy / cw + F(1)) * F(0.5)) * F(H)
            ok = (depth > 0) & ~(mv[..., 3] < F(0)) & (cw > 0)
            ok = ok & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
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


def scene(cam, cur=REST, prev=None, offset=(0.0, 0.0, 0.0)):
    """The scene moved by `offset` seen through `cam`, the rectangle at pose `cur`; `prev` is its pose
    in the previous frame (None: no motion data, every flag 0).  Evaluated in float64 relative to the
    camera position.  Returns a dict of per-pixel planes:
      sid (H, W) int, normal_plane (H, W, 4), depth (H, W) (-1 on a miss), motion (H, W, 4) =
      (P_prev - P, flag), prev_normal (H, W, 4), uv (H, W, 2) the rectangle's object-space point
      (NaN elsewhere)."""
    W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
    m = pixel_dirs(cam, W, H, np.float64)
    off = np.asarray(offset, np.float64)
    rel0 = off - _cam3(cam, "pos").astype(np.float64)          # scene origin - cam.pos
    best = np.full((H, W), np.inf)
    sid = np.zeros((H, W), int)
    npl = np.zeros((H, W, 4))
    with np.errstate(all="ignore"):
        for ident, axis, coord, bounds in tr.SURFACES[:2]:      # floor and wall, as temporal_ref.scene_guides
            t = (coord + rel0[axis]) / m[..., axis]
            ok = np.isfinite(t) & (t > 0) & (t < best)
            for ax, lo, hi in bounds:
                q = m[..., ax] * t - rel0[ax]
                ok &= (q > lo) & (q < hi)
            n = np.zeros(3)
            n[axis] = 1.0
            nm = m[..., axis]
            sign = np.where(nm > 0, -1.0, 1.0)
            best = np.where(ok, t, best)
            sid = np.where(ok, ident, sid)
            npl = np.where(ok[..., None], np.concatenate([sign[..., None] * n, (sign * nm * t)[..., None]], -1), npl)
        # the rectangle: a general ray-plane intersection
        R, tr_ = np.asarray(cur[0], np.float64), np.asarray(cur[1], np.float64)
        n = R @ np.array([0.0, 0.0, 1.0])
        rel = tr_ + rel0                                        # rectangle centre - cam.pos
        nm = m @ n
        t = (n @ rel) / nm
        q = (m * t[..., None] - rel) @ R                        # R^T (hit - centre)
        ok = np.isfinite(t) & (t > 0) & (t < best) & (np.abs(q[..., 0]) < 0.5) & (np.abs(q[..., 1]) < 0.5)
        sign = np.where(nm > 0, -1.0, 1.0)
        best = np.where(ok, t, best)
        sid = np.where(ok, RECT_ID, sid)
        npl = np.where(ok[..., None], np.concatenate([sign[..., None] * n, (sign * nm * t)[..., None]], -1), npl)
    hit = sid > 0
    depth = np.where(hit, np.where(hit, best, 0.0) * np.linalg.norm(m, axis=-1), -1.0)
    rect = sid == RECT_ID
    uv = np.where(rect[..., None], q[..., :2], np.nan)
    motion = np.zeros((H, W, 4))
    pnorm = np.zeros((H, W, 4))
    if prev is not None:
        Rp, tp = np.asarray(prev[0], np.float64), np.asarray(prev[1], np.float64)
        if not (np.array_equal(Rp, R) and np.array_equal(tp, tr_)):
            qq = np.where(rect[..., None], q, 0.0)
            d = (qq @ Rp.T + tp) - (qq @ R.T + tr_)             # the offset cancels
            motion = np.where(rect[..., None], np.concatenate([d, np.ones((H, W, 1))], -1), motion)
            npv = sign[..., None] * (Rp @ np.array([0.0, 0.0, 1.0]))
            pnorm = np.where(rect[..., None], np.concatenate([npv, np.zeros((H, W, 1))], -1), pnorm)
    return dict(sid=sid, normal_plane=npl.astype(F), depth=depth.astype(F), motion=motion.astype(F),
                prev_normal=pnorm.astype(F), uv=uv)


def tap_ids(prev_sid, info):
    """Surface ids of the four history taps per pixel; -1 outside the image or when the pixel is
    not reprojected at all."""
    H, W = prev_sid.shape
    out = []
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = info["ix"] + i, info["iy"] + j
            inside = info["reprojected"] & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            out.append(np.where(inside, prev_sid[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], -1))
    return np.stack(out, -1)
