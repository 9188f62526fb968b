"""Float64 truth and forward bounds for the motion planes of k_guides_motion (csrc/mcrt_aov.hip).

Truth, per pixel of a moved shape with poses M_prev, M_cur (toWorldTransform) and IT_prev, IT_cur
(toWorldInverseTranspose), from the guide planes alone:
  P = cam.pos + m^ depth (m^ the pixel's unit direction),   d = (M_prev M_cur^-1 - I) P,
  n_prev = normalize(IT_prev IT_cur^-1 n).

Bounds, u = 2^-24, in the manner of tests/ray_truth.py (infinity norm per pixel):

  The kernel forms P_prev and P from the SAME three object-space vertices and barycentrics, each by
  three transformPoint3 (3 products, 3 sums per component: <= 4 roundings, fewer when contracted)
  and the blend p0 (1 - b1 - b2) + p1 b1 + p2 b2 (2 roundings for the first weight, 3 products, 2
  sums), then one subtraction.  With S_x = max over the shape's vertices v of (|M_x| |v| + |t_x|):
      e_chain = 9 u (S_prev + S_cur) + u |d|                                   CHAIN = 9
  against (M_prev - M_cur) q at the kernel's own surface point q.

  The truth's P is rebuilt from the guides instead: depth = |P - cam.pos| in float32 (a subtraction,
  three products, two sums, a square root: <= 6 roundings of relative size u on depth, and the
  subtraction's u (|P| + |cam.pos|)), the direction m^ in float64 from the float32 camera record
  (the kernel's own normalised direction differs by <= 4 u), and P itself carries the cur chain's
  9 u S_cur:
      e_rec = 10 u (depth + |cam.pos|) + 9 u S_cur                             REC = 10
  The kernel's point also lies off the pixel's ray by what the walk's barycentrics can be off:
  ray_truth's b half-width 4 u |b| + K_2L u M / h on each of b1, b2 (M the largest coordinate among
  the ray origin and the shape's world vertices, h the triangle's smallest height), times the edge
  they scale, L the longest edge:
      e_bary = 2 L (4 u + K_2L u M / h) <= 8 u L + 2 K_2L u M A,   A = max L / h over the shape.
  K_2L = 64 is ray_truth's constant for two-level walks (the flat walks' 32 is covered by it).
      e_d = |M_prev M_cur^-1 - I|_inf (e_rec + e_bary) + e_chain.

  n_prev: both normals are the same blend of the object-space normals through IT_x (3 x (3 products,
  2 sums), the blend as above, normalisation: 3 products, 2 sums, rsqrt, 3 products), <= 16
  roundings relative to sum |w_i| |IT n_i| <= 2 |sum w_i IT n_i| (vertex normals of one triangle
  of these meshes are within 60 degrees of each other).  The guide normal's error is carried through
  A = IT_prev IT_cur^-1 and the renormalisation, the previous normal's own adds once more:
      e_n = 32 u (cond_2(A) + 1)                                                NORMAL = 32

tests/test_motion_truth_cpu.py checks CHAIN, REC and NORMAL against a float32 numpy restatement of
those chains, never against a kernel.
"""
import numpy as np

from ray_truth import K_2L, U

CHAIN, REC, NORMAL = 9.0, 10.0, 32.0
F = np.float32


def shape_vertices(scene, k):
    """(T, 3, 3) float64 object-space triangles of shape k."""
    s = scene.shapes[k]
    n = int(s["numTriangles"])
    idx = scene.indices[int(s["startIdx"]): int(s["startIdx"]) + 3 * n].astype(np.int64) + int(s["startVertex"])
    return scene.positions[idx, :3].astype(np.float64).reshape(-1, 3, 3)


def chain_scale(M, verts):
    """S of the docstring for toWorldTransform M (4x4) over object-space vertices (..., 3)."""
    M = np.asarray(M, np.float64)
    v = np.abs(verts.reshape(-1, 3))
    return float((v @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])).max())


def aspect_and_edge(M, tris):
    """(A, L) of the docstring for the world triangles M tris."""
    M = np.asarray(M, np.float64)
    w = tris @ M[:3, :3].T + M[:3, 3]
    e = np.stack([w[:, 1] - w[:, 0], w[:, 2] - w[:, 1], w[:, 0] - w[:, 2]], 1)
    L = np.linalg.norm(e, axis=-1).max(-1)
    area2 = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=-1)
    ok = area2 > 0
    return float((L[ok] * L[ok] / area2[ok]).max()), float(L.max()), float(np.abs(w).max())


def unit_dirs(cam, W, H):
    from temporal_ref import pixel_dirs
    m = pixel_dirs(cam, W, H, np.float64)
    return m / np.linalg.norm(m, axis=-1, keepdims=True)


def truth_motion(cam, depth, M_prev, M_cur):
    """d = (M_prev M_cur^-1 - I) P per pixel, float64, and P."""
    H, W = depth.shape
    pos = np.asarray(cam["pos"], np.float64).reshape(-1)[:3]
    P = pos + unit_dirs(cam, W, H) * depth.astype(np.float64)[..., None]
    D = np.asarray(M_prev, np.float64) @ np.linalg.inv(np.asarray(M_cur, np.float64)) - np.eye(4)
    return P @ D[:3, :3].T + D[:3, 3], P, D


def bound_motion(cam, depth, d, D, M_prev, M_cur, tris):
    """e_d per pixel (H, W) for a shape with object-space triangles `tris`."""
    pos = np.abs(np.asarray(cam["pos"], np.float64).reshape(-1)[:3]).max()
    S_prev, S_cur = chain_scale(M_prev, tris), chain_scale(M_cur, tris)
    A, L, Mw = aspect_and_edge(M_cur, tris)
    M = max(Mw, pos)
    dep = depth.astype(np.float64)
    e_rec = REC * U * (dep + pos) + CHAIN * U * S_cur
    e_bary = 8 * U * L + 2 * K_2L * U * M * A
    amp = np.abs(D[:3, :3]).sum(-1).max()
    return amp * (e_rec + e_bary) + CHAIN * U * (S_prev + S_cur) + U * np.abs(d).max(-1)


def truth_normal(n, IT_prev, IT_cur):
    """normalize(IT_prev IT_cur^-1 n) per pixel and its bound e_n (a scalar)."""
    A = np.asarray(IT_prev, np.float64)[:3, :3] @ np.linalg.inv(np.asarray(IT_cur, np.float64)[:3, :3])
    v = n.astype(np.float64) @ A.T
    with np.errstate(all="ignore"):
        v = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return v, NORMAL * U * (np.linalg.cond(A) + 1.0)


# ---- float32 restatement of the kernel's two chains (CPU validation of the constants) --------------
def _xform_point(M, v):
    M = np.asarray(M, F)
    return np.stack([((M[i, 0] * v[..., 0] + M[i, 1] * v[..., 1]) + M[i, 2] * v[..., 2]) + M[i, 3] for i in range(3)], -1)


def _xform_vector(M, v):
    M = np.asarray(M, F)
    return np.stack([(M[i, 0] * v[..., 0] + M[i, 1] * v[..., 1]) + M[i, 2] * v[..., 2] for i in range(3)], -1)


def _blend(p, b):
    w0 = (F(1) - b[..., 0:1]) - b[..., 1:2]
    return (p[:, 0] * w0 + p[:, 1] * b[..., 0:1]) + p[:, 2] * b[..., 1:2]


def restate_motion(M_prev, M_cur, tris, bary):
    """float32: (P, d) as k_guides_motion forms them, uncontracted; tris (T, 3, 3), bary (T, 2) float32."""
    tris, bary = np.asarray(tris, F), np.asarray(bary, F)
    P = _blend(_xform_point(M_cur, tris), bary)
    Pp = _blend(_xform_point(M_prev, tris), bary)
    return P, Pp - P


def restate_normal(IT, nrm, bary):
    """float32: si.sn's expression over IT; nrm (T, 3, 3) object-space vertex normals."""
    v = _blend(_xform_vector(IT, np.asarray(nrm, F)), np.asarray(bary, F))
    ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return v / ln[..., None]
