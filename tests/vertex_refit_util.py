"""Deformations and a structural check shared by tests/test_vertex_refit_cpu.py and
tests/test_gpu_vertex_refit.py (mcrt_scene_update_vertices + mcrt_accel_refit).

  deform / collapse   deterministic vertex motion: P' = P + a sin(k P.yzx + phi), or a range of
                      vertices moved to one point (zero-extent boxes, degenerate triangles);
  deformed            the Scene with such positions (and, on request, other normals);
  builder_triangles   the world triangles as the builders compute them, every product and sum
                      rounded to float32 on its own (xrow / xformPoint), shape transforms included;
  check_records       what holds for any flat tree of a scene, whatever its numbering: one parent
                      per record, the leaves a permutation of the triangles with the builders'
                      words, every stored child box EQUAL to the float32 min / max below it, by a
                      bottom-up pass over the child words.

Shares no code with the library and imports without a GPU."""
import copy

import numpy as np

from build_opts import same_words

f32 = np.float32

# The amplitude (in mean edge lengths, 0.596 here) of the GPU walks' deformed edge scene.  A property
# of the float64 truth alone: at 1.0 and at 0.25 one generic ray of 1500 grazes an edge and is not
# determined (closest 0.9987 / 0.9993), at 0.5, 0.2, 0.125 and 0.0625 all are; 0.2 is the next
# smaller one tried after 0.25.  tests/test_vertex_refit_cpu.py asserts it.
EDGE_AMPLITUDE = 0.2


def mean_edge(scene):
    """Mean edge length of the scene's triangles in object space."""
    e = []
    for s in scene.shapes:
        idx = scene.indices[s["startIdx"]: s["startIdx"] + 3 * s["numTriangles"]].astype(np.int64) + int(s["startVertex"])
        t = scene.positions[idx, :3].astype(np.float64).reshape(-1, 3, 3)
        e.append(np.linalg.norm(t - np.roll(t, 1, axis=1), axis=2).ravel())
    return float(np.concatenate(e).mean())


def deform(P, a, k=1.7, phi=0.3):
    """P' = P + a sin(k P.yzx + phi) on the xyz of float32 (V, 4) positions, evaluated in float64 and
    rounded once; w is kept.  A function of the position alone, so coincident vertices stay so."""
    P = np.ascontiguousarray(P, f32)
    q = P[:, :3].astype(np.float64)
    out = P.copy()
    out[:, :3] = (q + a * np.sin(k * q[:, [1, 2, 0]] + phi)).astype(f32)
    return out


def collapse(P, first, count, point):
    """Vertices [first, first + count) of float32 (V, 4) positions moved to `point`."""
    out = np.ascontiguousarray(P, f32).copy()
    out[first:first + count, :3] = np.asarray(point, f32)
    return out


def bent_normals(N, P, k=2.3, phi=1.1):
    """Other unit normals for a shading test: normalize(n + 0.25 sin(k P + phi)), float32 (V, 4)."""
    N = np.ascontiguousarray(N, f32)
    n = N[:, :3].astype(np.float64) + 0.25 * np.sin(k * np.asarray(P)[:, :3].astype(np.float64) + phi)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)
    out = N.copy()
    out[:, :3] = n.astype(f32)
    return out


def with_vertices(scene, positions, normals=None):
    """Copy of `scene` with these positions (and normals); everything else is shared."""
    sc = copy.copy(scene)
    sc.positions = np.ascontiguousarray(positions, f32)
    if normals is not None:
        sc.normals = np.ascontiguousarray(normals, f32)
    sc._desc = None
    assert sc.positions.shape == scene.positions.shape and sc.normals.shape == scene.normals.shape
    return sc


def deformed(scene, amplitude=1.0, k=1.7, phi=0.3, first=0, count=None, normals=False):
    """`scene` with vertices [first, first + count) deformed by `amplitude` mean edge lengths."""
    count = len(scene.positions) - first if count is None else count
    P = scene.positions.copy()
    P[first:first + count] = deform(P[first:first + count], amplitude * mean_edge(scene), k, phi)
    N = bent_normals(scene.normals, P) if normals else None
    return with_vertices(scene, P, N)


def shape_vertex_range(scene, shape):
    """(first, count) of the vertices the triangles of `shape` name."""
    s = scene.shapes[shape]
    idx = scene.indices[s["startIdx"]: s["startIdx"] + 3 * s["numTriangles"]].astype(np.int64) + int(s["startVertex"])
    return int(idx.min()), int(idx.max() - idx.min() + 1)


def shared_mesh_scene():
    """Two shapes with different non-identity transforms (rotation + non-uniform scale, a mirror +
    translation) that share one box mesh, and a ground grid under a third transform: built with
    force_flat, every world triangle goes through the builders' transform arithmetic."""
    from mcrt import scenes
    b = scenes.SceneBuilder("shared_mesh")
    m = b.add_material(kd=(0.6, 0.5, 0.4))
    A = scenes._affine(1.3, 35.0, (1.5, 0.7, -0.4), 20.0).astype(np.float64)
    A[:3, :3] = A[:3, :3] @ np.diag([1.0, 0.5, 1.75])
    B = np.eye(4)
    B[:3, :3] = np.diag([-1.0, 1.0, 1.0]) @ scenes._affine(0.8, 110.0, (0, 0, 0), -15.0)[:3, :3]
    B[:3, 3] = (-2.0, 1.1, 0.9)
    G = scenes._affine(1.0, 10.0, (0.1, -0.2, 0.3), 3.0)
    box = b.add_mesh(*scenes.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), 3), m, transform=A.astype(f32))
    b.add_instance(box, B.astype(f32))
    b.add_mesh(*scenes.grid((-4, -1, -4), (8, 0, 0), (0, 0, 8), 6, 6), m, transform=np.asarray(G, f32))
    b.add_point_light((0.0, 5.0, -3.0), (10, 10, 10))
    return b.build()


def builder_triangles(scene):
    """(T, 3, 3) float32 world triangles in shape order with the builders' arithmetic: per row of the
    shape's matrix acc = 0; acc += m.x x; acc += m.y y; acc += m.z z; acc += m.w 0; acc + m.w, each
    product and sum rounded to float32 (RR transform_point).  Also the (shape, prim) of each."""
    out, sid, pid = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for si, s in enumerate(scene.shapes):
            n = int(s["numTriangles"])
            idx = scene.indices[s["startIdx"]: s["startIdx"] + 3 * n].astype(np.int64) + int(s["startVertex"])
            P = scene.positions[idx, :3].astype(f32)
            M = np.asarray(s["toWorldTransform"], f32)
            W = np.empty_like(P)
            for r in range(3):
                acc = np.zeros(len(P), f32)
                for c in range(3):
                    acc = (acc + (M[r, c] * P[:, c]).astype(f32)).astype(f32)
                acc = (acc + f32(M[r, 3] * f32(0.0))).astype(f32)
                W[:, r] = (acc + M[r, 3]).astype(f32)
            out.append(W.reshape(-1, 3, 3))
            sid.append(np.full(n, si, np.int64))
            pid.append(np.arange(n, dtype=np.int64))
    return np.concatenate(out), np.concatenate(sid), np.concatenate(pid)


def leaves_by_triangle(rec, scene):
    """Index of the leaf record of every triangle of `scene` (in shape order), after checking that
    the leaves are a permutation of the triangles."""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 16)
    ids = rec.view(np.int32)
    lf = np.nonzero(ids[:, 12] < 0)[0]
    first = np.concatenate([[0], np.cumsum(scene.shapes["numTriangles"])[:-1]]).astype(np.int64)
    shape, prim = ids[lf, 3].astype(np.int64), ids[lf, 7].astype(np.int64)
    assert ((shape >= 0) & (shape < len(scene.shapes))).all()
    assert ((prim >= 0) & (prim < scene.shapes["numTriangles"][shape])).all()
    g = first[shape] + prim
    n = scene.num_triangles
    assert len(g) == n and (np.sort(g) == np.arange(n)).all(), "the leaves are not a permutation of the triangles"
    at = np.empty(n, np.int64)
    at[g] = lf
    return at


def check_records(rec, scene):
    """Asserts that the flat records `rec` are a correct BVH of `scene` in any numbering and under
    any shape transforms: 2n - 1 records; every record but record 0 has exactly one parent and is
    reached from record 0; the leaves hold every triangle once, with the builders' float32 vertex
    and edges and a leaf's id words (word 13: -1 or the parent's index); every stored child box
    EQUALS the float32 min / max of the vertices below it (min and max do not round: equality,
    +0 == -0).  Returns the level of the deepest leaf."""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 16)
    tri, _, _ = builder_triangles(scene)
    n = len(tri)
    N = 2 * n - 1
    assert rec.shape[0] == N, (rec.shape, n)
    ids = rec.view(np.int32)
    internal = ids[:, 12] >= 0
    assert int((~internal).sum()) == n
    p = np.nonzero(internal)[0]
    child = np.zeros((N, 2), np.int64)
    child[p] = ids[p, 12:14]
    assert ((child[p] > 0) & (child[p] < N)).all()
    assert (ids[p, 14:16] == 0).all()
    assert (np.sort(child[p].ravel()) == np.arange(1, N)).all(), "a record has no parent or two"
    parent = np.full(N, -1, np.int64)
    parent[child[p, 0]] = p
    parent[child[p, 1]] = p
    level = np.full(N, -1, np.int64)
    level[0] = 0
    frontier = np.array([0])
    while len(frontier):
        inner = frontier[internal[frontier]]
        nxt = child[inner].ravel()
        level[nxt] = np.repeat(level[inner] + 1, 2)
        frontier = nxt
    assert (level >= 0).all(), "records unreachable from the root"
    at = leaves_by_triangle(rec, scene)
    assert same_words(rec[at, 0:3], tri[:, 0]).all(), "a leaf's vertex is not the builders'"
    assert same_words(rec[at, 4:7], tri[:, 1] - tri[:, 0]).all(), "a leaf's first edge is not the builders'"
    assert same_words(rec[at, 8:11], tri[:, 2] - tri[:, 0]).all(), "a leaf's second edge is not the builders'"
    assert (ids[at, 11] == 0).all() and (ids[at, 12] == -1).all() and (ids[at, 14:16] == 0).all()
    assert ((ids[at, 13] == -1) | (ids[at, 13] == parent[at])).all()
    lo = np.zeros((N, 3), f32)
    hi = np.zeros((N, 3), f32)
    lo[at], hi[at] = tri.min(1), tri.max(1)
    for lv in range(int(level.max()) - 1, -1, -1):
        q = np.nonzero(internal & (level == lv))[0]
        c0, c1 = child[q, 0], child[q, 1]
        lo[q] = np.minimum(lo[c0], lo[c1])
        hi[q] = np.maximum(hi[c0], hi[c1])
    c0, c1 = child[p, 0], child[p, 1]
    want = np.stack([lo[c0, 0], hi[c0, 0], lo[c0, 1], hi[c0, 1], lo[c1, 0], hi[c1, 0], lo[c1, 1], hi[c1, 1],
                     lo[c0, 2], hi[c0, 2], lo[c1, 2], hi[c1, 2]], 1)
    ok = same_words(rec[p, :12], want)
    assert ok.all(), f"child boxes of records {p[~ok.all(1)][:8].tolist()} are not the bounds of their leaves"
    return int(level[~internal].max())


def leaf_words(rec, scene):
    """uint32 (T, 15): the leaf record of every triangle in shape order without word 13, the parent
    link, which is the tree's and not the triangle's."""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 16)
    w = rec.view(np.uint32)[leaves_by_triangle(rec, scene)]
    return np.delete(w, 13, axis=1)


class Case:
    """A scene, its rays of every family (tests/ray_truth.py, seed 7) and their float64 truths, one
    per K, computed on first use."""

    def __init__(self, scene, inside=True, seed=7):
        import ray_truth as rt
        self.scene = scene
        self.rays, self.fam = rt.all_families(scene, seed, inside)
        self.tris, self.sid, self.pid = rt.world_triangles64(scene)
        self._truth = {}

    def truth(self, K):
        import ray_truth as rt
        if K not in self._truth:
            self._truth[K] = rt.classify(self.tris, self.rays, K=K, shape=self.sid, prim=self.pid)
        return self._truth[K]

    def shares(self, K):
        """{family: (determined closest, determined any-hit)}"""
        import ray_truth as rt
        tr = self.truth(K)
        return {f: (float(tr.closest_det[self.fam == i].mean()), float(tr.any_det[self.fam == i].mean()))
                for i, f in enumerate(rt.FAMILIES)}


_cases = {}


def deformed_edge_case():
    """The Case of ray_truth.edge_scene() deformed by EDGE_AMPLITUDE mean edge lengths, and the
    undeformed scene it came from; made once per process."""
    import ray_truth as rt
    if "edge" not in _cases:
        base = rt.edge_scene()
        _cases["edge"] = (base, Case(deformed(base, EDGE_AMPLITUDE)))
    return _cases["edge"]


__all__ = ["mean_edge", "deform", "collapse", "bent_normals", "with_vertices", "deformed", "shape_vertex_range",
           "builder_triangles", "leaves_by_triangle", "check_records", "leaf_words"]
