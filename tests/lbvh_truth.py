"""A ground truth for the device linear BVH (mcrt_accel_opts.device_build = 1, mcrt_gpubuild.hip), in
plain numpy and Python ints; shared by tests/test_lbvh_truth_cpu.py and tests/test_gpu_lbvh.py.

  radix_tree   the definition of the tree over sorted keys, written top-down (split every range at
               the highest differing bit of its first and last augmented key) and not as the
               builder's per-node binary searches;
  check_lbvh   what holds for any LBVH of a scene, whatever its keys: numbering, one parent per
               record, leaves that are a permutation of the triangles, child boxes EQUAL to the
               exact float32 bounds, contiguous leaf ranges, the reported depth;
  morton_keys  k_prims / k_morton restated in float32; reproducible on the device only where the
               quotient (c - lo) / ext is exact (the builder is compiled with the 2.5-ulp division);
  dyadic, same_key   scenes whose quotients are exact, with many equal keys / one key only.

Shares no code with a builder and imports without a GPU."""
import numpy as np

from build_opts import _triangle_scene, check_leaves, same_words

KEY_BITS = 63
CELLS = 1 << 21            # Morton cells per axis


def radix_tree(keys):
    """The binary radix tree of the sorted 63-bit `keys` in the builder's numbering.

    Leaf j carries the augmented key (key << 32) | j, so no two leaves are equal.  The range [a, b]
    splits at g, the last index whose augmented key has the highest bit in which aug[a] and aug[b]
    differ clear.  Internal records are 0 .. n-2 (0 = the root, the range [0, n-1]); the node of the
    left range [a, g] is g, the node of the right range [g+1, b] is g + 1, a range of one leaf j is
    record n - 1 + j.  Returns (childL, childR, level of the deepest leaf)."""
    aug = [(int(k) << 32) | j for j, k in enumerate(keys)]
    n = len(aug)
    assert n >= 1 and all(0 <= int(k) < (1 << KEY_BITS) for k in keys)
    assert all(aug[j] < aug[j + 1] for j in range(n - 1)), "radix_tree: the keys are not sorted"
    childL = np.full(max(n - 1, 0), -1, np.int64)
    childR = np.full(max(n - 1, 0), -1, np.int64)
    deepest = 0
    todo = [(0, 0, n - 1, 0)] if n > 1 else []           # (node, a, b, level)
    while todo:
        node, a, b, level = todo.pop()
        assert childL[node] < 0, "radix_tree: a node numbered twice"
        bit = (aug[a] ^ aug[b]).bit_length() - 1
        g = a
        while not (aug[g + 1] >> bit) & 1:               # sorted: the clear ones come first
            g += 1
        for side, (lo, hi, number) in enumerate(((a, g, g), (g + 1, b, g + 1))):
            if lo == hi:
                rec = n - 1 + lo
                deepest = max(deepest, level + 1)
            else:
                rec = number
                todo.append((number, lo, hi, level + 1))
            (childR if side else childL)[node] = rec
    return childL, childR, deepest


def morton_keys(scene):
    """The 63-bit Morton key of every triangle of `scene` (identity transforms) as k_prims and
    k_morton compute it, every step in float32: the triangle's box, the centroid (mn + mx) * 0.5,
    the centroid bounds, t = (c - lo) / ext (0.5 where ext == 0) clamped to [0, 1],
    q = min(uint(t * 2^21), 2^21 - 1) and the interleave x << 2 | y << 1 | z.  The division here is
    IEEE; the device's may differ by 2.5 ulp wherever the quotient is not exact.
    Returns (keys uint64 (n,), cells uint32 (n, 3), centroid extent float32 (3,))."""
    f32 = np.float32
    tri = scene.world_triangles()
    mn, mx = tri.min(1), tri.max(1)
    c = ((mn + mx).astype(f32) * f32(0.5)).astype(f32)
    lo, hi = c.min(0), c.max(0)
    ext = (hi - lo).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(ext > 0, ((c - lo).astype(f32) / ext).astype(f32), f32(0.5)).astype(f32)
    t = np.minimum(np.maximum(t, f32(0)), f32(1))
    q = np.minimum((t * f32(CELLS)).astype(f32).astype(np.uint32), np.uint32(CELLS - 1))
    keys = np.zeros(len(tri), np.uint64)
    for axis in range(3):
        for b in range(21):
            keys |= ((q[:, axis].astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - axis)
    return keys, q, ext


def check_lbvh(rec, scene, depth):
    """Asserts that the flat records `rec` are a correct linear BVH of `scene` (identity transforms)
    in mcrt_gpubuild.hip's numbering, whatever the keys were:

      * 2n - 1 records, 0 .. n-2 internal (word 12 >= 0) and n-1 .. 2n-2 leaves (n == 1: one leaf);
      * every record but the root has exactly one parent and is reachable from record 0;
      * the leaves are a permutation of the triangles, each with its float32 vertex and edges and
        the id words of build_opts.check_tree (word 13: -1 or the parent's index);
      * every stored child box EQUALS the exact float32 min / max of the vertices below it (min and
        max do not round; +0 == -0), not merely contains them;
      * the leaves under every internal record i are a contiguous range of leaf numbers, the left
        child covers the lower part (and, when internal, is the last number of its part; the right
        child the first of its part: the builder's numbering), and i is the range's first or last;
      * depth == level of the deepest leaf + 1.  gpu_build_bvh returns the root's height plus one,
        ONE MORE than the SAH builders' convention (the deepest leaf's level, check_tree).  The
        value sizes the spill columns and switches the wave packets off, so it is pinned here as
        it is: a change in either direction is seen.

    Returns the level of the deepest leaf."""
    rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 16)
    eye = np.eye(4, dtype=np.float32)
    assert (scene.shapes["toWorldTransform"] == eye).all(), "check_lbvh: identity transforms only"
    tri = scene.world_triangles()
    n = len(tri)
    N = 2 * n - 1
    assert n >= 1 and rec.shape[0] == N, (rec.shape, n)
    ids = rec.view(np.int32)
    internal = ids[:, 12] >= 0
    assert internal[:n - 1].all() and not internal[n - 1:].any(), "internal records first, then the leaves"
    p = np.arange(n - 1)
    lf = np.arange(n - 1, N)
    child = np.zeros((N, 2), np.int64)
    child[p] = ids[p, 12:14]
    assert (ids[p, 14:16] == 0).all()
    assert (np.sort(child[p].ravel()) == np.arange(1, N)).all(), "a record has no parent or two"
    parent = np.full(N, -1, np.int64)
    parent[child[p, 0]] = p
    parent[child[p, 1]] = p
    # levels from the root; with one parent each, an unreached record lies on a cycle of its own
    level = np.full(N, -1, np.int64)
    level[0] = 0
    frontier = np.array([0])
    while len(frontier):
        inner = frontier[internal[frontier]]
        nxt = child[inner].ravel()
        level[nxt] = np.repeat(level[inner] + 1, 2)
        frontier = nxt
    assert (level >= 0).all(), "records unreachable from the root"
    t = tri[check_leaves(rec, scene, tri, lf, parent)]
    # bottom-up: the exact box and the range of leaf numbers below every record
    lo = np.zeros((N, 3), np.float32)
    hi = np.zeros((N, 3), np.float32)
    lo[lf], hi[lf] = t.min(1), t.max(1)
    first = np.zeros(N, np.int64)
    last = np.zeros(N, np.int64)
    first[lf] = last[lf] = lf - (n - 1)
    count = (~internal).astype(np.int64)
    for lv in range(int(level.max()) - 1, -1, -1):
        q = np.nonzero(internal & (level == lv))[0]
        c0, c1 = child[q, 0], child[q, 1]
        lo[q] = np.minimum(lo[c0], lo[c1])
        hi[q] = np.maximum(hi[c0], hi[c1])
        first[q] = np.minimum(first[c0], first[c1])
        last[q] = np.maximum(last[c0], last[c1])
        count[q] = count[c0] + count[c1]
    assert count[0] == n
    c0, c1 = child[p, 0], child[p, 1]
    want = np.stack([lo[c0, 0], hi[c0, 0], lo[c0, 1], hi[c0, 1], lo[c1, 0], hi[c1, 0], lo[c1, 1], hi[c1, 1],
                     lo[c0, 2], hi[c0, 2], lo[c1, 2], hi[c1, 2]], 1)
    ok = same_words(rec[p, :12], want)
    assert ok.all(), f"child boxes of records {p[~ok.all(1)][:8].tolist()} are not the bounds of their leaves"
    assert (last - first + 1 == count).all(), "the leaves under a record are not a contiguous range"
    assert (first[c0] == first[p]).all() and (last[c0] + 1 == first[c1]).all() and (last[c1] == last[p]).all(), \
        "a left child does not cover the lower part of its parent's range"
    assert ((p == first[p]) | (p == last[p])).all(), "an internal record is no endpoint of its range"
    assert (c0[internal[c0]] == last[c0[internal[c0]]]).all() and (c1[internal[c1]] == first[c1[internal[c1]]]).all()
    deepest = int(level[lf].max())
    assert depth == deepest + 1, (depth, deepest)
    return deepest


# --- scenes whose Morton quotients are exact ------------------------------------------------------

DYADIC_STEPS = 32                      # lattice of multiples of 2^-5 in [0, 1]^3
_CORNERS = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [1.0, -1.0, 0.0]])


def dyadic_centroids(n, seed=17):
    """The lattice points (n, 3) of dyadic(n, seed)'s triangles, in triangle order."""
    assert n >= 8
    rng = np.random.default_rng(seed)
    side = DYADIC_STEPS + 1
    cells = rng.permutation(side ** 3)
    cells = cells[(cells != 0) & (cells != side ** 3 - 1)]   # the two corners are placed by hand
    shared = (n - 2) // 2                                    # in groups of three on one point
    where = np.concatenate([np.arange(shared) // 3, shared + np.arange(n - 2 - shared)])
    cell = np.concatenate([[0, side ** 3 - 1], cells[where]])
    cell = cell[rng.permutation(n)]                          # numbered in shuffled order
    return np.stack([cell // (side * side), (cell // side) % side, cell % side], 1) / float(DYADIC_STEPS)


def dyadic(n, seed=17):
    """n triangles c + h {(-1,-1,-1), (1,1,1), (1,-1,0)}, h = 2^-8, whose centroids c are multiples of
    2^-5 in [0, 1]^3: mn + mx = 2 c, so the float32 centroid is c exactly; one triangle at (0,0,0)
    and one at (1,1,1) make lo = 0 and ext = 1 on every axis, so t = c / 1.  About half of the
    triangles share their lattice point (and so their key) with others, the rest do not, and the
    numbering is shuffled, so a stable sort has an order to keep.  tests/test_lbvh_truth_cpu.py
    asserts these premises."""
    c = dyadic_centroids(n, seed)
    P = c[:, None, :] + 2.0 ** -8 * _CORNERS[None]
    return _triangle_scene(f"dyadic_{n}", P.reshape(-1, 3), (0.5, 0.5, 3.0))


def same_key(n):
    """n distinct (nested) triangles c + (k + 1) 2^-12 {(-1,-1,-1), (1,1,1), (1,-1,0)} around one
    point c: every centroid is c exactly, the centroid extent is 0 on all axes and every key is
    equal, so the index tie-break of k_hierarchy's delta decides the whole tree."""
    c = np.array([0.5, 0.25, 0.75])
    s = (np.arange(n) + 1.0) * 2.0 ** -12
    P = c[None, None, :] + s[:, None, None] * _CORNERS[None]
    return _triangle_scene(f"same_key_{n}", P.reshape(-1, 3), (0.5, 0.25, 3.0))


__all__ = ["radix_tree", "morton_keys", "check_lbvh", "dyadic", "dyadic_centroids", "same_key"]
