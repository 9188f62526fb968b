"""Option tuples, scenes and a structural ground truth shared by the tests of the BVH builders under
non-default mcrt_accel_opts (tests/test_build_opts_cpu.py, tests/test_gpu_build_opts.py).

mcrt_accel_opts carries traversal_cost, num_bins and use_sah into four builders: the host Bvh2
restatement (mcrt_bvh.cpp), the host two-level build (mcrt_bvh2l.cpp), the device SAH build
(mcrt_sahbuild.hip, the default) and the device top-level build (mcrt_topbuild.hip).  GRID holds the
values at which their code takes another path; check_tree is a ground truth in plain numpy that
shares no code with any of them.  Imports without a GPU."""
import numpy as np

from mcrt import scenes
from test_hint_premise_cpu import check_nesting, leaf_depth

FLT_MAX = float(np.finfo(np.float32).max)

# (bins, cost, sah)
GRID = (
    (64, 10.0, True),       # the default
    (2, 10.0, True),        # smallest legal bin count: one candidate plane
    (3, 10.0, True),        # ext / bins is not exact
    (5, 10.0, True),
    (7, 10.0, True),
    (33, 10.0, True),
    (63, 10.0, True),       # one lane of the wave-wide sweep masked
    (64, 1e6, True),        # the prices round to a few values: ties, the first minimum wins
    (64, FLT_MAX, True),    # no bin wins: the plane is the centroid minimum, then the median fallback
    (64, float("inf"), True),   # every price inf or NaN; the host equals the reference here too
    (64, float("nan"), True),   # (tests/test_build_opts_cpu.py), so both are legal ground truth
    (64, 10.0, False),      # SAH off: every request takes the midpoint
    (5, 1e6, False),
    (65, 10.0, True),       # HOST_ONLY
    (200, 10.0, True),      # HOST_ONLY
)
# more bins than the device builders support: they must hand the build to the host
HOST_ONLY = tuple(t for t in GRID if t[0] > 64)


def opts(t):
    """The keyword options of lib.DeviceScene / lib.build_host_records / the reference builders."""
    return {"bins": t[0], "cost": t[1], "sah": t[2]}


def tuple_id(t):
    cost = "fltmax" if t[1] == FLT_MAX else f"{t[1]:g}"
    return f"b{t[0]}-c{cost}-{'sah' if t[2] else 'mid'}"


def _soup(kind, n, seed):
    """Synthetic stress cases: 'grid' (many equal centroid coordinates -> median fallbacks,
    ties in the bins), 'clusters' (identical triangles: zero centroid extent), 'coplanar'."""
    rng = np.random.default_rng(seed)
    b = scenes.SceneBuilder(kind)
    m = b.add_material(kd=(0.5, 0.5, 0.5))
    k = np.arange(n)
    if kind == "grid":
        c = np.stack([k % 97, (k // 97) % 13 * 0.5, np.zeros(n)], 1)
    elif kind == "clusters":
        c = np.where((k % 7 < 3)[:, None], np.stack([k % 7, np.ones(n), 2 * np.ones(n)], 1),
                     rng.uniform(-10, 10, (n, 3)))
    else:
        c = np.stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), np.zeros(n)], 1)
    off = rng.uniform(-0.05, 0.05, (n, 3, 3))
    if kind == "coplanar":
        off[..., 2] = 0.0
    if kind == "clusters":
        off[k % 7 < 3] = 0.01 * np.eye(3)
    P = (c[:, None, :] + off).reshape(-1, 3)
    tris = np.arange(3 * n).reshape(-1, 3)
    b.add_mesh(P, np.tile([0.0, 0.0, 1.0], (3 * n, 1)), np.zeros((3 * n, 2)), tris, m)
    b.add_point_light((0, 0, 20), (10, 10, 10))
    return b.build()


def _triangle_scene(name, P, light):
    b = scenes.SceneBuilder(name)
    m = b.add_material(kd=(0.5, 0.5, 0.5))
    n = len(P) // 3
    b.add_mesh(P, np.tile([0.0, 0.0, 1.0], (3 * n, 1)), np.zeros((3 * n, 2)), np.arange(3 * n).reshape(-1, 3), m)
    b.add_point_light(light, (10, 10, 10))
    return b.build()


def geo(n, seed=11):
    """Triangle k around x = 2^-(k % 100) (y, z within x / 2 of the axis), vertices jittered by
    1e-3 x.  A deep request's box has sides near 2^-99, so the products of its surface area are
    denormal or zero and the builders' reciprocal of the area sees both (rcp_ps of 0 is inf, the
    prices turn NaN, no bin wins); where a device flushed a denormal that SSE keeps, the tree would
    differ from the host's."""
    rng = np.random.default_rng(seed)
    x = 2.0 ** -(np.arange(n) % 100).astype(np.float64)
    c = x[:, None] * np.concatenate([np.ones((n, 1)), rng.uniform(-0.5, 0.5, (n, 2))], 1)
    P = c[:, None, :] + 1e-3 * x[:, None, None] * rng.uniform(-1.0, 1.0, (n, 3, 3))
    return _triangle_scene(f"geo_{n}", P.reshape(-1, 3), (2.0, 2.0, 2.0))


def geo_tame(levels=40, per=6, seed=12):
    """The same idea down to 2^-(levels - 1) only, with triangles of size 0.3 * 2^-k at level k:
    large enough for rays to hit, a tree as deep as the scene has levels once SAH is off."""
    rng = np.random.default_rng(seed)
    x = np.repeat(2.0 ** -np.arange(levels, dtype=np.float64), per)
    n = len(x)
    c = x[:, None] * np.concatenate([np.ones((n, 1)), rng.uniform(-0.5, 0.5, (n, 2))], 1)
    P = c[:, None, :] + 0.3 * x[:, None, None] * rng.uniform(-1.0, 1.0, (n, 3, 3))
    return _triangle_scene(f"geo_tame_{levels}x{per}", P.reshape(-1, 3), (0.5, 0.5, -2.0))


# a centroid extent at which float32 E * (1 / bins) != E / bins for 3, 5, 7, 33 and 63 bins
LATTICE_EXTENT = 36.9


def lattice_spots(bins, extent):
    """0, every p_k = k * (E / bins) in float32 (k = 1 .. bins - 1), the float below each p_k, and E."""
    f32 = np.float32
    E = f32(extent)
    step = E / f32(bins)                                     # correctly rounded float32 quotient
    p = (np.arange(1, bins, dtype=f32) * step).astype(f32)   # one rounding each
    return np.concatenate([[f32(0)], p, np.nextafter(p, f32(-np.inf)), [E]]).astype(f32)


def lattice(bins, n_min, extent=LATTICE_EXTENT, seed=13):
    """Centroids on the root's candidate planes.  With `bins` bins the root request of this scene
    (centroid minimum 0, centroid extent E = float32(extent) along x) prices the planes
    p_k = k * (E / bins), k = 1 .. bins - 1, in float32.  Every p_k carries triangles whose centroid
    is exactly p_k (they go right: c < split is false) and triangles one ulp below it (they go
    left), so a plane that is off by an ulp in either direction -- a step E * (1 / bins) instead of
    E / bins, a fused multiply-add -- sends some triangle to the other side, whichever k wins.  Each
    triangle lies in a plane x = const, which makes its centroid exact.  At least n_min triangles."""
    spots = lattice_spots(bins, extent)
    x = np.repeat(spots, -(-n_min // len(spots)))
    n = len(x)
    rng = np.random.default_rng(seed + bins)
    P = np.empty((n, 3, 3), np.float64)
    P[..., 0] = x[:, None]
    P[..., 1:] = rng.uniform(-1.0, 1.0, (n, 1, 2)) + rng.uniform(-0.05, 0.05, (n, 3, 2))
    return _triangle_scene(f"lattice_{bins}_{n}", P.reshape(-1, 3), (0.0, 0.0, 20.0))


# bins whose lattice scenes are built: one finished by one wave (9 .. 256 triangles), one that starts
# in the level passes (> 256)
LATTICE_BINS = (2, 3, 5, 7, 33, 63, 64)
LATTICE_SIZES = {"wave": 10, "level": 600}


# coplanar soups on each side of the builders' size thresholds: the <= 8 references one lane
# finishes, the 256 one wave finishes (SAH_SMALL), the 4096 of a level-pass workgroup (CHUNK)
ROOT_SIZES = (8, 9, 64, 65, 256, 257, 4096, 4097, 8193)

FLAT_SCENES = ("grid", "clusters", "coplanar", "mixed", "geo", "geo_tame")
_cache = {}


def flat_scene(name):
    """A flat scene by name (FLAT_SCENES, 'root<n>' or 'lattice<bins>_<wave|level>'), built once per
    process."""
    if name not in _cache:
        if name in ("grid", "clusters", "coplanar"):
            sc = _soup(name, 3000, 3)
        elif name == "mixed":
            sc = scenes.test_scene()
        elif name == "geo":
            sc = geo(3000)
        elif name == "geo_tame":
            sc = geo_tame()
        elif name.startswith("lattice"):
            bins, size = name[7:].split("_")
            sc = lattice(int(bins), LATTICE_SIZES[size])
        else:
            sc = _soup("coplanar", int(name[4:]), 5)
        _cache[name] = sc
    return _cache[name]


def same_words(a, b):
    """Element-wise uint32 equality of two float32 arrays with +0 == -0, the one freedom the device
    builders have (order-free min / max reductions)."""
    ai = np.ascontiguousarray(a, np.float32).view(np.uint32)
    bi = np.ascontiguousarray(b, np.float32).view(np.uint32)
    return (ai == bi) | (((ai & 0x7fffffff) == 0) & ((bi & 0x7fffffff) == 0))


def _levels(child, internal):
    """Level of every record (root 0) of a validated pre-order tree."""
    level = np.full(len(child), -1, np.int64)
    level[0] = 0
    frontier = np.array([0])
    while len(frontier):
        inner = frontier[internal[frontier]]
        nxt = child[inner].ravel()
        level[nxt] = np.repeat(level[inner] + 1, 2)
        frontier = nxt
    return level


def check_leaves(rec, scene, tri, lf, parent):
    """The leaf checks of check_tree and lbvh_truth.check_lbvh: the leaf records `lf` of `rec` hold
    every triangle of `scene` (tri: its world triangles) once, with its float32 vertex and edges,
    and their id words are a leaf's.  parent: the parent index of every record.  Returns the triangle
    number of every leaf."""
    ids = rec.view(np.int32)
    n = len(tri)
    # (shape, prim) pairs are a permutation of the scene's triangles; vertex and edges
    first = np.concatenate([[0], np.cumsum(scene.shapes["numTriangles"])[:-1]]).astype(np.int64)
    shape, prim = ids[lf, 3].astype(np.int64), ids[lf, 7].astype(np.int64)
    assert ((shape >= 0) & (shape < len(scene.shapes))).all()
    assert ((prim >= 0) & (prim < scene.shapes["numTriangles"][shape])).all()
    g = first[shape] + prim
    assert (np.sort(g) == np.arange(n)).all(), "the leaves are not a permutation of the triangles"
    t = tri[g]
    assert same_words(rec[lf, 0:3], t[:, 0]).all()
    assert same_words(rec[lf, 4:7], t[:, 1] - t[:, 0]).all()
    assert same_words(rec[lf, 8:11], t[:, 2] - t[:, 0]).all()
    assert (ids[lf, 11] == 0).all() and (ids[lf, 12] == -1).all() and (ids[lf, 14:16] == 0).all()
    # word 13 of a leaf: -1 as built, its parent's index once the scene is on the device
    assert ((ids[lf, 13] == -1) | (ids[lf, 13] == parent[lf])).all()
    return g


def check_tree(rec, scene, depth=None):
    """Asserts that the flat records `rec` are a correct BVH of `scene` (identity transforms), whatever
    the split policy: 2n - 1 records, n leaves that hold every triangle once with its float32 vertex
    and edges, pre-order numbering (child0 = i + 1, child1 = i + 2 * leaves under child0), and every
    stored child box equal to the exact float32 min / max over the vertices below it (min and max do
    not round, so equality is the assertion; +0 == -0).  depth: the builder's reported depth, which
    must be the deepest leaf's level.  Returns the deepest leaf's level."""
    rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 16)
    eye = np.eye(4, dtype=np.float32)
    assert (scene.shapes["toWorldTransform"] == eye).all(), "check_tree: identity transforms only"
    tri = scene.world_triangles()
    n = len(tri)
    N = 2 * n - 1
    assert rec.shape[0] == N, (rec.shape, n)
    ids = rec.view(np.int32)
    internal = ids[:, 12] >= 0
    leaf = ~internal
    assert int(leaf.sum()) == n
    idx = np.arange(N)
    # numbering: child0 follows its parent, child1 lies behind it, every record but the root has
    # exactly one parent
    p = idx[internal]
    child = np.zeros((N, 2), np.int64)
    child[p] = ids[p, 12:14]
    assert (child[p, 0] == p + 1).all()
    assert ((child[p, 1] > p + 1) & (child[p, 1] < N)).all()
    assert (ids[p, 14:16] == 0).all()
    assert (np.sort(child[p].ravel()) == np.arange(1, N)).all(), "a record has no parent or two"
    level = _levels(child, internal)
    assert (level >= 0).all()
    parent = np.zeros(N, np.int64)
    parent[child[p, 0]] = p
    parent[child[p, 1]] = p
    lf = idx[leaf]
    t = tri[check_leaves(rec, scene, tri, lf, parent)]
    # bottom-up: leaves and exact box below every record
    lo = np.zeros((N, 3), np.float32)
    hi = np.zeros((N, 3), np.float32)
    lo[lf], hi[lf] = t.min(1), t.max(1)
    count = leaf.astype(np.int64)
    for lv in range(int(level.max()) - 1, -1, -1):
        q = idx[internal & (level == lv)]
        c0, c1 = child[q, 0], child[q, 1]
        lo[q] = np.minimum(lo[c0], lo[c1])
        hi[q] = np.maximum(hi[c0], hi[c1])
        count[q] = count[c0] + count[c1]
    assert count[0] == n
    assert (child[p, 1] == p + 2 * count[child[p, 0]]).all()
    c0, c1 = child[p, 0], child[p, 1]
    want = np.stack([lo[c0, 0], hi[c0, 0], lo[c0, 1], hi[c0, 1], lo[c1, 0], hi[c1, 0], lo[c1, 1], hi[c1, 1],
                     lo[c0, 2], hi[c0, 2], lo[c1, 2], hi[c1, 2]], 1)
    ok = same_words(rec[p, :12], want)
    assert ok.all(), f"child boxes of records {p[~ok.all(1)][:8].tolist()} are not the bounds of their leaves"
    deepest = int(level[lf].max()) if n > 1 else 0
    assert deepest == leaf_depth(rec)
    if depth is not None:
        assert depth == deepest, (depth, deepest)
    return deepest


__all__ = ["GRID", "HOST_ONLY", "FLT_MAX", "ROOT_SIZES", "FLAT_SCENES", "opts", "tuple_id", "flat_scene", "geo",
           "geo_tame", "same_words", "check_leaves", "check_tree", "check_nesting", "leaf_depth"]
