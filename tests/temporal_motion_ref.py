"""A float64 analytic scene with one moving object, for k_temporal's MOTION form (its numpy
restatement is temporal_ref.accumulate with motion planes).

The scene is temporal_ref.SURFACES' floor and wall plus a unit rectangle (object space: the plane
z = 0, |x| < 0.5, |y| < 0.5, normal +z) under a rigid pose (R, t) per frame: world = R q + t.  The
pose REST puts it where temporal_ref's floating square is.
"""
import numpy as np

import temporal_ref as tr
from temporal_ref import F, _cam3, pixel_dirs

RECT_ID = 3
REST = (np.eye(3), np.array([0.0, 0.8, 0.5]))


def rot_y(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def pose(translate=(0.0, 0.0, 0.0), turn_deg=0.0):
    """REST turned about the vertical axis through the rectangle's centre, then translated."""
    return rot_y(turn_deg) @ REST[0], REST[1] + np.asarray(translate, np.float64)


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
