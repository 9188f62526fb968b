"""Float64 brute-force ground truth for the ray queries (mcrt_trace_closest / mcrt_trace_any).

numpy only: no GPU, no oracle, no BVH.  Every ray is tested against every triangle with the
Moeller-Trumbore quantities exactly as RR common.cl:177-218 states them, in float64, and each
quantity carries a forward bound on what float32 evaluation can do to it.  The bounds decide, per
ray and triangle, whether float32 arithmetic CAN change the verdict:

  s1 = d x e2, den = s1 . e1, N1 = (o - A) . s1, s2 = (o - A) x e1, N2 = d . s2, N3 = e2 . s2,
  b1 = N1 / den, b2 = N2 / den, t = N3 / den,                      u = 2^-24,
  e_den = K u |d||e2||e1|, e_N1 = K u |o-A||d||e2|, e_N2 = K u |o-A||e1||d|, e_N3 = K u |e2||o-A||e1|.

A triangle is stable when |den| > e_den; then b_i lies within
  (e_Ni + |b_i| e_den) / (|den| - e_den) + 4 u |b_i| + K u M / h
of its float64 value (M: the largest absolute coordinate among the ray origin and the triangle's
vertices; h = 2 area / longest edge, the triangle's smallest height: the M / h term is the absolute
position error of the slab tests and of vertices rounded to float32 -- the "|o / d| ulp" effect
mcrt_traverse.h documents), and t within the same quotient bound + K u (M / |d| + |t|).

Per triangle: CLEAR HIT (every acceptance inequality b1 >= 0, b2 >= 0, b1 + b2 <= 1, 0 <= t <= tmax
holds over the whole interval), CLEAR MISS (one of them fails over the whole interval; or
|N_i| - e_Ni > |den| + e_den, some |b| > 1 whatever the denominator's rounding; or every product
term of den is exactly zero, so float32 gets exactly 0 in any evaluation order: coincident
vertices, axis rays against axis-aligned faces), else AMBIGUOUS (t_lo = 0 when unstable).
Per ray: closest is DETERMINED MISS without clear hit and ambiguous triangle, DETERMINED HIT j when
j is the nearest clear hit and t_hi(j) < t_lo(k) for every other clear or ambiguous k; any-hit is
determined with a clear hit (occluded) or without any candidate (free).  The ray mask (extra[0])
removes that shape's triangles first, as the walks' r.mask != shape id does.

judge(): determined rays get the STRONG check (exact shape, primitive, hit-or-miss, |t - t_truth|
within the triangle's t half-width, (u, v) within the b half-widths + UV_SLACK); every other ray
the WEAK one (a reported hit is a candidate whose t_lo does not exceed the smallest t_hi among the
clear hits, and its t and (u, v) lie in that triangle's own intervals where it is stable; a
reported miss needs that no clear hit exists).  No active ray goes unchecked; an
inactive ray (extra[1] = 0) must leave its output untouched.

Constants, all fixed on the CPU against the oracle's restatement of intersect_bvh2_lds.cl
(tests/test_ray_truth_cpu.py), never against a GPU result:
  K = 32      the oracle shows 0 strong and 0 weak failures on every family, scene and offset.
  K_2L = 2 K  two-level walks transform the ray once more (world -> object: a rounding of the
              same size on o and on d), so every bound doubles.
  UV_SLACK    the walks report barycentrics recomputed from the hit point o + t d (triBary,
              common.cl:249-277), not b1 / b2 themselves.  Measured over all families, scenes and
              offsets: the oracle's (u, v) never leave the b half-widths (largest excess
              -1.5e-6: the half-widths' M / h term already covers the hit point's rounding), so
              no slack is needed for the reference's arithmetic.  UV_SLACK = 4 u = 2.4e-7 allows
              for the one difference between a kernel and that restatement, v_rcp_f32 (1 ulp)
              in place of 1 / x in triBary, on values |b| <= 1; the older oracle comparison
              allows 2e-3.
"""
import numpy as np

from mcrt import scenes
from mcrt import types as T

U = 2.0 ** -24
K = 32.0
K_2L = 2.0 * K
UV_SLACK = 4 * U
CLEAR, AMBIGUOUS = 2, 1
_CHUNK = 512


# --------------------------------------------------------------------------------------------
# geometry
# --------------------------------------------------------------------------------------------
def world_triangles64(scene):
    """(tris (T, 3, 3) float64, shape id (T,), primitive id (T,)): the world triangles from the
    float32 mesh positions and toWorldTransform, evaluated in float64 (Scene.world_triangles()
    rounds to float32)."""
    tris, sid, pid = [], [], []
    for k, s in enumerate(scene.shapes):
        n = int(s["numTriangles"])
        idx = scene.indices[int(s["startIdx"]): int(s["startIdx"]) + 3 * n].astype(np.int64) + int(s["startVertex"])
        P = scene.positions[idx, :3].astype(np.float64).reshape(-1, 3, 3)
        M = s["toWorldTransform"].astype(np.float64)
        tris.append(P @ M[:3, :3].T + M[:3, 3])
        sid.append(np.full(n, k, np.int32))
        pid.append(np.arange(n, dtype=np.int32))
    return np.concatenate(tris), np.concatenate(sid), np.concatenate(pid)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _norm(a):
    return np.sqrt((a * a).sum(-1))


class Truth:
    """classify()'s result: the candidates (clear hits and ambiguous triangles) of every ray in CSR
    form (sorted by ray, then triangle) and the per-ray verdicts."""

    def __init__(self, n, shape, prim):
        self.n = n
        self.shape, self.prim = shape, prim
        self.T = len(shape)
        cnt = np.bincount(shape, minlength=int(shape.max()) + 1 if len(shape) else 0)
        self.shape_count = cnt
        self.shape_start = np.concatenate([[0], np.cumsum(cnt)])[:-1] if len(cnt) else np.zeros(0, np.int64)

    def tri_index(self, shapeid, primid):
        """Triangle index of (shape, primitive) pairs, -1 where there is no such triangle."""
        shapeid, primid = np.asarray(shapeid, np.int64), np.asarray(primid, np.int64)
        ok = (shapeid >= 0) & (shapeid < len(self.shape_count))
        s = np.where(ok, shapeid, 0)
        ok &= (primid >= 0) & (primid < self.shape_count[s])
        return np.where(ok, self.shape_start[s] + primid, -1)

    def lookup(self, ray, tri):
        """Candidate slot of (ray, triangle) pairs, -1 for a clear miss."""
        key = np.asarray(ray, np.int64) * self.T + np.asarray(tri, np.int64)
        pos = np.searchsorted(self.key, key)
        pos = np.minimum(pos, max(len(self.key) - 1, 0))
        found = (self.key[pos] == key) if len(self.key) else np.zeros(len(key), bool)
        return np.where(found & (np.asarray(tri) >= 0), pos, -1)


def classify(tris, rays, K=K, shape=None, prim=None):
    """Classifies every ray of `rays` (RAY_DTYPE) against the (T, 3, 3) float64 triangles `tris`
    (shape / prim: their ids, default shape 0 and 0..T-1).  Returns a Truth."""
    tris = np.asarray(tris, np.float64)
    nt = len(tris)
    shape = np.zeros(nt, np.int32) if shape is None else np.asarray(shape, np.int32)
    prim = np.arange(nt, dtype=np.int32) if prim is None else np.asarray(prim, np.int32)
    # triangles are addressed by (shape, prim): keep them grouped by shape, prim ascending
    assert np.all(np.diff(shape) >= 0)
    n = len(rays)
    tr = Truth(n, shape, prim)
    A = tris[:, 0]
    e1, e2 = tris[:, 1] - A, tris[:, 2] - A
    le1, le2 = _norm(e1), _norm(e2)
    area2 = _norm(_cross(e1, e2))
    longest = np.maximum(np.maximum(le1, le2), _norm(e2 - e1))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_h = np.where(area2 > 0, longest / area2, np.inf)          # 1 / h
    mtri = np.abs(tris).reshape(nt, 9).max(1)
    # every product term d_i e2_j e1_k of den exactly zero <=> no permutation has three non-zeros
    z1, z2 = e1 != 0, e2 != 0
    q = np.stack([(z2[:, (i + 1) % 3] & z1[:, (i + 2) % 3]) | (z2[:, (i + 2) % 3] & z1[:, (i + 1) % 3])
                  for i in range(3)], 0).astype(np.float64)           # (3, T)

    O = rays["o"][:, :3].astype(np.float64)
    D = rays["d"][:, :3].astype(np.float64)
    TM = rays["o"][:, 3].astype(np.float64)
    MASK = rays["extra"][:, 0].astype(np.int64)
    parts = {k: [] for k in ("ray", "tri", "kind", "t", "t_lo", "t_hi", "b1", "b2", "hb1", "hb2", "ht")}
    ku = K * U
    for c0 in range(0, n, _CHUNK):
        o, d, tmax = O[c0:c0 + _CHUNK, None, :], D[c0:c0 + _CHUNK, None, :], TM[c0:c0 + _CHUNK, None]
        with np.errstate(all="ignore"):
            s1 = _cross(d, e2[None])
            den = (s1 * e1[None]).sum(-1)
            oa = o - A[None]
            n1 = (oa * s1).sum(-1)
            s2 = _cross(oa, e1[None])
            n2 = (d * s2).sum(-1)
            n3 = (e2[None] * s2).sum(-1)
            ld, loa = _norm(d), _norm(oa)
            e_den = ku * ld * le2 * le1
            e_n1 = ku * loa * ld * le2
            e_n2 = ku * loa * le1 * ld
            e_n3 = ku * le2 * loa * le1
            aden = np.abs(den)
            stable = aden > e_den
            exact0 = ((d[:, 0, :] != 0).astype(np.float64) @ q) == 0
            big = (np.abs(n1) - e_n1 > aden + e_den) | (np.abs(n2) - e_n2 > aden + e_den)
            sden = np.where(stable, den, 1.0)
            gap = np.where(stable, aden - e_den, 1.0)
            b1, b2, t = n1 / sden, n2 / sden, n3 / sden
            m = np.maximum(np.abs(o).max(-1), mtri[None])
            pos = ku * m * inv_h[None]
            hb1 = (e_n1 + np.abs(b1) * e_den) / gap + 4 * U * np.abs(b1) + pos
            hb2 = (e_n2 + np.abs(b2) * e_den) / gap + 4 * U * np.abs(b2) + pos
            ht = (e_n3 + np.abs(t) * e_den) / gap + ku * (m / ld + np.abs(t))
            fin = stable & np.isfinite(hb1) & np.isfinite(hb2) & np.isfinite(ht)
            hit = fin & (b1 - hb1 >= 0) & (b2 - hb2 >= 0) & (b1 + b2 + hb1 + hb2 <= 1) & (t - ht >= 0) & (t + ht < tmax)
            miss = fin & ((b1 + hb1 < 0) | (b2 + hb2 < 0) | (b1 - hb1 > 1) | (b2 - hb2 > 1) |
                          (b1 + b2 - hb1 - hb2 > 1) | (t + ht < 0) | (t - ht > tmax))
            miss |= big | exact0 | (tmax < 0)
            assert not (hit & miss).any()
            masked = MASK[c0:c0 + _CHUNK, None] == shape[None, :]      # RR_RAY_MASK: not in the scene
            hit &= ~masked
            cand = ~(miss | masked)
            ri, ti = np.nonzero(cand)
            sel = (ri, ti)
            f = fin[sel]
            parts["ray"].append(ri + c0)
            parts["tri"].append(ti)
            parts["kind"].append(np.where(hit[sel], CLEAR, AMBIGUOUS).astype(np.int8))
            parts["t"].append(np.where(f, t[sel], np.nan))
            parts["t_lo"].append(np.where(f, np.maximum(t[sel] - ht[sel], 0.0), 0.0))
            parts["t_hi"].append(np.where(f, t[sel] + ht[sel], np.inf))
            parts["b1"].append(np.where(f, b1[sel], np.nan))
            parts["b2"].append(np.where(f, b2[sel], np.nan))
            parts["hb1"].append(np.where(f, hb1[sel], np.inf))
            parts["hb2"].append(np.where(f, hb2[sel], np.inf))
            parts["ht"].append(np.where(f, ht[sel], np.inf))
    for k, v in parts.items():
        setattr(tr, k, np.concatenate(v) if v else np.zeros(0))
    tr.ray = tr.ray.astype(np.int64)
    tr.tri = tr.tri.astype(np.int64)
    tr.key = tr.ray * max(nt, 1) + tr.tri
    _per_ray(tr)
    return tr


def _per_ray(tr):
    n, C = tr.n, len(tr.ray)
    clear = tr.kind == CLEAR
    tr.n_cand = np.bincount(tr.ray, minlength=n)
    tr.n_clear = np.bincount(tr.ray[clear], minlength=n)
    # smallest t_hi among the clear hits and the slot that holds it
    tr.min_clear_hi = np.full(n, np.inf)
    np.minimum.at(tr.min_clear_hi, tr.ray[clear], tr.t_hi[clear])
    best = np.full(n, -1, np.int64)
    is_best = clear & (tr.t_hi == tr.min_clear_hi[tr.ray])
    best[tr.ray[is_best][::-1]] = np.nonzero(is_best)[0][::-1]        # first such slot per ray
    # smallest t_lo among the other candidates
    other = np.ones(C, bool)
    other[best[best >= 0]] = False
    min_other_lo = np.full(n, np.inf)
    np.minimum.at(min_other_lo, tr.ray[other], tr.t_lo[other])
    tr.closest_slot = best
    tr.closest_det = (tr.n_cand == 0) | ((best >= 0) & (tr.min_clear_hi < min_other_lo))
    tr.closest_tri = np.where((best >= 0) & tr.closest_det, tr.tri[np.maximum(best, 0)] if C else -1, -1)
    tr.any_det = (tr.n_clear > 0) | (tr.n_cand == 0)
    tr.any_val = np.where(tr.n_clear > 0, 1, -1)


# --------------------------------------------------------------------------------------------
# judge
# --------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self):
        self.strong, self.weak = [], []       # (ray index, reason)
        self.active = self.determined = self.weak_only = 0
        self.uv_excess = -np.inf              # largest distance of a checked (u, v) beyond its b half-width

    @property
    def share(self):
        return self.determined / max(self.active, 1)

    def ok(self):
        return not self.strong and not self.weak

    def __str__(self):
        s = f"{self.active} active rays, {self.determined} determined ({self.share:.3f}), {self.weak_only} weak-only; " \
            f"{len(self.strong)} strong failures, {len(self.weak)} weak failures"
        for tag, lst in (("strong", self.strong), ("weak", self.weak)):
            for i, why in lst[:8]:
                s += f"\n  {tag}: ray {i}: {why}"
        return s


def judge(tr, rays, hits=None, occl=None, index=None, init=-7, uv_slack=UV_SLACK):
    """Checks a closest-hit answer (hits: ISECT_DTYPE) or an any-hit answer (occl: int32, 1 / -1)
    for `rays` against a Truth.  index: row i of rays / hits / occl is the Truth's ray index[i]
    (reordered, repeated or partial launches; default: the same order).  Outputs were pre-filled
    with `init`.  The failures name the Truth's ray index."""
    v = Verdict()
    ridx = np.arange(tr.n) if index is None else np.asarray(index, np.int64)
    assert len(ridx) == len(rays) == len(hits if occl is None else occl)
    active = rays["extra"][:, 1] != 0
    v.active = int(active.sum())

    def flag(lst, m, why):
        lst.extend((int(ridx[i]), why) for i in np.nonzero(m)[0])

    n_cand, n_clear = tr.n_cand[ridx], tr.n_clear[ridx]
    if occl is not None:
        occl = np.asarray(occl)
        flag(v.strong, ~active & (occl != init), "inactive ray's output touched")
        bad = active & (occl != 1) & (occl != -1)
        flag(v.strong, bad, "answer is neither 1 nor -1")
        any_det = tr.any_det[ridx]
        det = active & any_det
        v.determined = int(det.sum())
        v.weak_only = v.active - v.determined
        flag(v.strong, det & ~bad & (occl != tr.any_val[ridx]), "any-hit answer differs from the determined one")
        rest = active & ~any_det & ~bad
        flag(v.weak, rest & (occl == 1) & (n_cand == 0), "occluded without a candidate")
        flag(v.weak, rest & (occl == -1) & (n_clear > 0), "free although a clear hit exists")
        return v
    sid, pid = hits["shapeid"].astype(np.int64), hits["primid"].astype(np.int64)
    flag(v.strong, ~active & ((sid != init) | (pid != init)), "inactive ray's output touched")
    miss = (sid == -1) & (pid == -1)
    tri = tr.tri_index(sid, pid)
    bad = active & ~miss & (tri < 0)
    flag(v.strong, bad, "reported (shape, primitive) does not exist")
    slot = tr.lookup(ridx, tri)
    closest_det, closest_tri = tr.closest_det[ridx], tr.closest_tri[ridx]
    det = active & closest_det
    v.determined = int(det.sum())
    v.weak_only = v.active - v.determined
    good = active & ~bad
    # strong
    want_miss = closest_tri < 0
    flag(v.strong, det & good & want_miss & ~miss, "hit reported, determined miss")
    flag(v.strong, det & good & ~want_miss & miss, "miss reported, determined hit")
    flag(v.strong, det & good & ~want_miss & ~miss & (tri != closest_tri), "wrong triangle")
    same = det & good & ~want_miss & ~miss & (tri == closest_tri)
    s = np.maximum(slot, 0)
    if len(tr.ray):
        uvwt = hits["uvwt"].astype(np.float64)
        dt = np.abs(uvwt[:, 3] - tr.t[s])
        flag(v.strong, same & ~(dt <= tr.ht[s]), "t outside the triangle's t interval")
        du = np.abs(uvwt[:, 0] - tr.b1[s])
        dv = np.abs(uvwt[:, 1] - tr.b2[s])
        flag(v.strong, same & ~((du <= tr.hb1[s] + uv_slack) & (dv <= tr.hb2[s] + uv_slack)), "(u, v) outside the b intervals")
        v.uv_excess = float(np.max(np.where(same, np.maximum(du - tr.hb1[s], dv - tr.hb2[s]), -np.inf), initial=-np.inf))
    # weak
    rest = active & ~closest_det & ~bad
    flag(v.weak, rest & miss & (n_clear > 0), "miss reported although a clear hit exists")
    flag(v.weak, rest & ~miss & (slot < 0), "reported triangle is a clear miss")
    if len(tr.ray):
        flag(v.weak, rest & ~miss & (slot >= 0) & (tr.t_lo[s] > tr.min_clear_hi[ridx]),
             "reported triangle lies behind a clear hit")
        # the reported numbers belong to the reported triangle (the same bounds as the strong check,
        # where that triangle is stable: an unstable one has infinite half-widths)
        cand = rest & ~miss & (slot >= 0)
        flag(v.weak, cand & ~(dt <= tr.ht[s]) & np.isfinite(tr.ht[s]), "t outside the reported triangle's t interval")
        flag(v.weak, cand & np.isfinite(tr.hb1[s]) & ~((du <= tr.hb1[s] + uv_slack) & (dv <= tr.hb2[s] + uv_slack)),
             "(u, v) outside the reported triangle's b intervals")
    return v


# --------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------
LATTICE = (-2.0, -0.5, 1.0)


def _rot(yaw_deg, tilt_deg):
    return scenes._affine(1.0, yaw_deg, (0, 0, 0), tilt_deg)[:3, :3].astype(np.float64)


def _degenerate_mesh():
    """Coincident vertices (each pair), three collinear points (two ways), a point."""
    P = np.array([[-0.75, -0.75, -0.75], [-0.75, -0.75, -0.75], [-0.625, -0.5, -0.75],     # v0 = v1
                  [0.75, -0.75, 0.625], [0.875, -0.625, 0.75], [0.875, -0.625, 0.75],       # v1 = v2
                  [-0.75, 0.75, 0.75], [-0.625, 0.875, 0.625], [-0.75, 0.75, 0.75],         # v0 = v2
                  [0.625, 0.625, -0.75], [0.75, 0.75, -0.75], [0.875, 0.875, -0.75],        # collinear, v1 between
                  [-0.75, 0.625, -0.875], [-0.75, 0.875, -0.625], [-0.75, 0.75, -0.75],     # collinear, v2 between
                  [0.75, 0.75, 0.75], [0.75, 0.75, 0.75], [0.75, 0.75, 0.75]])              # a point
    return P, np.arange(len(P)).reshape(-1, 3)


def _scene_mesh(b, P, tris, m, offset, N=None):
    P = np.asarray(P, np.float64) + np.asarray(offset, np.float64)
    b.add_mesh(P, np.tile([0, 1, 0], (len(P), 1)) if N is None else N, np.zeros((len(P), 2)), tris, m)


def edge_scene(offset=(0.0, 0.0, 0.0), lights=False):
    """27 unit boxes on a lattice of binary fractions (faces in shared planes, exact in float32 at
    offset 1000 too), a rotated box, a 5 x 5 ground grid and a shape of degenerate triangles:
    1400 triangles in 30 shapes, identity transforms.  lights: a material per shape, an axis-
    parallel directional light and a point light, for the render tests (the ray queries ignore
    them)."""
    b = scenes.SceneBuilder("edge")
    shared = b.add_material()

    def mat():
        k = len(b.meshes)
        return b.add_material(kd=(0.2 + 0.02 * k, 0.8 - 0.02 * k, 0.3 + 0.05 * (k % 7)), ks=(0, 0, 0)) if lights else shared

    for x in LATTICE:
        for y in LATTICE:
            for z in LATTICE:
                P, N, _, tris = scenes.box((x, y, z), (x + 1, y + 1, z + 1), 2)
                _scene_mesh(b, P, tris, mat(), offset, N)
    P, N, _, tris = scenes.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), 2)
    _scene_mesh(b, P @ _rot(30.0, 20.0).T + (0.25, 3.0, -0.25), tris, mat(), offset, N @ _rot(30.0, 20.0).T)
    P, N, _, tris = scenes.grid((-3, -2.75, -3), (6, 0, 0), (0, 0, 6), 5, 5)
    _scene_mesh(b, P, tris, mat(), offset, N)
    P, tris = _degenerate_mesh()
    _scene_mesh(b, P, tris, mat(), offset)
    if lights:
        b.add_directional_light((0.0, -1.0, 0.0), (3.0, 3.0, 3.0))
        b.add_point_light(tuple(np.asarray(offset, np.float64) + (0.25, 0.25, -3.5)), (8.0, 8.0, 8.0))
    return b.build()


def tiny_scenes():
    """1, 2 and 3 triangles: the root is a leaf, or the tree has one or two internal nodes.  The
    triangles are axis aligned, so their boxes are flat."""
    out = []
    tri = [np.array([[-1, 0, -1], [1, 0, -1], [0, 0, 1]], np.float64),
           np.array([[0.5, -1, -1], [0.5, 1, -1], [0.5, 0, 1.5]], np.float64),
           np.array([[-1, -1, 0.25], [1.5, -1, 0.25], [0, 1, 0.25]], np.float64)]
    for n in (1, 2, 3):
        b = scenes.SceneBuilder(f"tiny{n}")
        m = b.add_material()
        for k in range(n):      # one shape per triangle: the shape id is checked too
            _scene_mesh(b, tri[k], [[0, 1, 2]], m, (0, 0, 0))
        out.append(b.build())
    return out


def instanced_edge_scene():
    """One box mesh (a unit box of 48 triangles) under five transforms: identity, a rotation, a
    non-uniform scale, a mirror and a translation of 1000 units -- the natural two-level path."""
    b = scenes.SceneBuilder("instanced_edge")
    m = b.add_material()
    P, N, UV, tris = scenes.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), 2)
    base = b.add_mesh(P, N, UV, tris, m)
    M = np.eye(4)
    M[:3, :3] = _rot(40.0, 25.0)
    M[:3, 3] = (2.0, 0.5, 0.0)
    b.add_instance(base, M.astype(np.float32))
    M = np.eye(4)
    M[:3, :3] = np.diag([2.0, 0.25, 1.5])
    M[:3, 3] = (-2.5, 0.0, 1.0)
    b.add_instance(base, M.astype(np.float32))
    M = np.eye(4)
    M[:3, :3] = np.diag([-1.0, 1.0, 1.0]) @ _rot(15.0, 0.0)
    M[:3, 3] = (0.0, 2.0, -2.0)
    b.add_instance(base, M.astype(np.float32))
    M = np.eye(4)
    M[:3, 3] = (1000.0, 0.0, 0.0)
    b.add_instance(base, M.astype(np.float32))
    return b.build()


# --------------------------------------------------------------------------------------------
# ray families
# --------------------------------------------------------------------------------------------
FAMILIES = ("generic", "axis", "axis_on_plane", "tiny", "aimed", "tmax", "far", "on_surface")
TINY_VALUES = np.array([0.0, 1e-9, -1e-9, 1e-8, -1e-8, 1.0000001e-8, 1e-7, -1e-6, 1e-38, -1e-45], np.float32)


def _rays(o, d, tmax=1000.0):
    r = np.zeros(len(o), T.RAY_DTYPE)
    r["o"][:, :3] = o
    r["o"][:, 3] = tmax
    r["d"][:, :3] = d
    r["extra"][:, 0] = -1
    r["extra"][:, 1] = 1
    assert np.isfinite(r["o"][:, :3]).all() and np.isfinite(r["d"][:, :3]).all()
    return r


def _bounds(tris, pad):
    P = tris.reshape(-1, 3)
    return P.min(0) - pad, P.max(0) + pad


def _axis_dirs(rng, n):
    """d = +-e_k, the other two components drawn from {+0.0, -0.0}."""
    d = np.where(rng.integers(0, 2, (n, 3)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    k = np.arange(n) % 3
    d[np.arange(n), k] = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
    return d


def _solid(tris):
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    return np.nonzero(_norm(_cross(e1, e2)) > 0)[0]


def _aimed(tris, rng, n, lo, hi, targets="cev"):
    """Rays from random origins towards centroids (c), edge midpoints (e) and vertices (v) of
    random triangles; d unnormalised, scaled by 1e-3, 1 or 37."""
    j = rng.choice(_solid(tris), n)
    P = tris[j]
    kind = np.array([targets[i % len(targets)] for i in range(n)])
    w = np.zeros((n, 3))
    w[kind == "c"] = 1.0 / 3.0
    ne = kind == "e"
    a = rng.integers(0, 3, n)
    w[ne, a[ne]] = 0.5
    w[ne, (a[ne] + 1) % 3] = 0.5
    nv = kind == "v"
    w[nv, a[nv]] = 1.0
    target = (P * w[:, :, None]).sum(1)
    o = rng.uniform(lo, hi, (n, 3))
    d = target - o
    d /= _norm(d)[:, None]
    d *= rng.choice([1e-3, 1.0, 37.0], n)[:, None]
    return o, d


def family(name, scene, seed, inside=True):
    """The rays of one family for `scene` (deterministic in seed).  inside: generic rays start
    inside the scene's bounds (False for the tiny scenes, whose bounds are flat)."""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    tris, _, _ = world_triangles64(scene)
    lo, hi = _bounds(tris, 1.0)
    if name == "generic":
        from helpers import random_rays
        return random_rays(scene, 1500, seed=seed, inside=inside)
    if name == "axis":
        n = 720
        return _rays(rng.uniform(lo, hi, (n, 3)), _axis_dirs(rng, n))
    if name == "axis_on_plane":
        # every coordinate on which a box face, a box's inner grid line or the gap between two
        # boxes lies, and one step outside
        off = np.round(0.5 * (lo + hi))          # the scene's offset (a whole number)
        coords = np.arange(-2.5, 2.51, 0.5)
        g = np.stack(np.meshgrid(coords, coords, indexing="ij"), -1).reshape(-1, 2)
        o, d = [], []
        for k in range(3):
            for sgn in (1.0, -1.0):
                p = np.zeros((len(g), 3))
                p[:, (k + 1) % 3], p[:, (k + 2) % 3] = g[:, 0], g[:, 1]
                start = np.where(np.arange(len(g)) % 2 == 0, -3.0 * sgn, rng.choice(coords, len(g)))
                p[:, k] = start
                dd = np.where(rng.integers(0, 2, (len(g), 3)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
                dd[:, k] = sgn
                o.append(p + off)
                d.append(dd)
        return _rays(np.concatenate(o), np.concatenate(d))
    if name == "tiny":
        n = 800
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        k = rng.integers(0, 3, n)
        d[np.arange(n), k] = rng.choice(TINY_VALUES, n)
        two = rng.integers(0, 2, n) == 1
        k2 = (k + 1 + rng.integers(0, 2, n)) % 3
        d[two, k2[two]] = rng.choice(TINY_VALUES, int(two.sum()))
        return _rays(rng.uniform(lo, hi, (n, 3)), d)
    if name == "aimed":
        o, d = _aimed(tris, rng, 900, lo, hi)
        return _rays(o, d)
    if name == "tmax":
        # aimed rays whose first hit is determined, then tmax on either side of it
        o, d = _aimed(tris, rng, 240, lo, hi, targets="c")
        base = _rays(o, d, tmax=np.inf)
        tr = classify(tris, base)
        ok = np.nonzero(tr.closest_det & (tr.closest_tri >= 0))[0][:150]
        t1 = tr.t[tr.closest_slot[ok]]
        out = []
        for f in (1 - 1e-3, 1 - 1e-6, 1.0, 1 + 1e-6, 1 + 1e-3):
            r = base[ok].copy()
            r["o"][:, 3] = t1 * f
            out.append(r)
        for tm in (0.0, -1.0, np.inf):
            r = base[ok].copy()
            r["o"][:, 3] = tm
            out.append(r)
        return np.concatenate(out)
    if name == "far":
        n = 600
        u = rng.normal(size=(n, 3))
        u /= _norm(u)[:, None]
        # 3 : 2 : 1 -- at 1e4 units the position term K u M / h alone is 5 % of a box triangle, so
        # few of those rays are determined; they still get the weak check
        R = np.array([1e2, 1e2, 1e2, 1e3, 1e3, 1e4])[np.arange(n) % 6]
        c = 0.5 * (lo + hi)
        o = (c + u * R[:, None]).astype(np.float32).astype(np.float64)
        j = rng.choice(_solid(tris), n)
        w = rng.dirichlet([4.0, 4.0, 4.0], n)
        target = (tris[j] * w[:, :, None]).sum(1)
        d = target - o
        d /= _norm(d)[:, None]
        return _rays(o, d, tmax=1e6)
    if name == "on_surface":
        n = 600
        j = rng.choice(_solid(tris), n)
        w = rng.dirichlet([1.0, 1.0, 1.0], n)
        o = (tris[j] * w[:, :, None]).sum(1)
        d = rng.normal(size=(n, 3))
        d /= _norm(d)[:, None]
        return _rays(o, d)
    raise KeyError(name)


def all_families(scene, seed, inside=True):
    """(rays, family index per ray): every family for `scene`, concatenated."""
    parts = [family(f, scene, seed, inside) for f in FAMILIES]
    fam = np.concatenate([np.full(len(p), i, np.int32) for i, p in enumerate(parts)])
    return np.concatenate(parts), fam


def octant(rays):
    """Sign octant of safeInvDir(d) (common.cl:220-232): copysign keeps the sign of -0.0 and of
    |d| <= 1e-8, so it is the sign bit of each component."""
    s = np.signbit(rays["d"][:, :3])
    return s[:, 0].astype(np.int32) | (s[:, 1].astype(np.int32) << 1) | (s[:, 2].astype(np.int32) << 2)


def octant_blocks(rays, block=64):
    """Index array that sorts `rays` by octant and pads every octant's run (repeating its rays) to
    whole blocks, so each block of 64 consecutive rays -- one wave -- is one octant."""
    oc = octant(rays)
    out = []
    for k in range(8):
        idx = np.nonzero(oc == k)[0]
        if len(idx):
            out.append(np.resize(idx, -(-len(idx) // block) * block))
    return np.concatenate(out)
