"""The LBVH ground truth's own test (tests/lbvh_truth.py), without a GPU: radix_tree on trees written
out by hand and against a transcription of k_hierarchy's searches (mcrt_gpubuild.hip), check_lbvh
on records synthesised in numpy -- which pass -- and on single corruptions of them -- each of which
must fail --, and the premises of the dyadic and same_key scenes."""
import numpy as np
import pytest

import lbvh_truth as lt


# --- radix_tree ------------------------------------------------------------------------------------

HAND = {
    # keys: (childL, childR, deepest leaf level); leaf j is record n - 1 + j
    (0, 1): ([1], [2], 1),
    # all equal: the leaf numbers 0, 1, 2 decide; bit 1 splits {0, 1} | {2}, bit 0 splits {0} | {1}
    (5, 5, 5): ([1, 2], [4, 3], 2),
    # 001 010 | 100 100: bit 2 splits in the middle, the right half by its leaf numbers
    (1, 2, 4, 4): ([1, 3, 5], [2, 4, 6], 2),
    # 000 | 100 | 110 | 111: a chain to the right
    (0, 4, 6, 7): ([3, 4, 5], [1, 2, 6], 3),
    # 000 001 010 | 111 and 7 7 7 7 (balanced by the leaf numbers)
    (0, 1, 2, 7): ([2, 3, 1], [6, 4, 5], 3),
    (7, 7, 7, 7): ([1, 3, 5], [2, 4, 6], 2),
}


@pytest.mark.parametrize("keys", list(HAND), ids=["-".join(map(str, k)) for k in HAND])
def test_radix_tree_by_hand(keys):
    L, R, deepest = lt.radix_tree(keys)
    wantL, wantR, want_deepest = HAND[keys]
    assert L.tolist() == wantL and R.tolist() == wantR and deepest == want_deepest


def test_radix_tree_of_one_leaf():
    L, R, deepest = lt.radix_tree([9])
    assert len(L) == 0 and len(R) == 0 and deepest == 0


def _karras(keys):
    """k_hierarchy transcribed: per-node searches over delta (common prefix, index tie-break)."""
    n = len(keys)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        a, b = int(keys[i]), int(keys[j])
        if a == b:
            return 64 + (32 - (i ^ j).bit_length())
        return 64 - (a ^ b).bit_length()

    L, R = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax <<= 1
        l, t = 0, lmax >> 1
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t >>= 1
        j = i + l * d
        dnode = delta(i, j)
        s, div = 0, 2
        while True:
            t = (l + div - 1) // div
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
            div <<= 1
        g = i + s * d + min(d, 0)
        L[i] = n - 1 + g if min(i, j) == g else g
        R[i] = n - 1 + g + 1 if max(i, j) == g + 1 else g + 1
    return L, R


def test_radix_tree_equals_the_builders_searches():
    """The top-down definition and Karras's per-node searches give the same children on random key
    sets: wide keys, keys of a few distinct values (long runs of ties), one value only."""
    rng = np.random.default_rng(1)
    for trial in range(200):
        n = int(rng.integers(2, 70))
        kind = trial % 4
        if kind == 0:
            keys = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        elif kind == 1:
            keys = rng.choice(rng.integers(0, 1 << 63, 4, dtype=np.uint64), n)
        elif kind == 2:
            keys = rng.integers(0, 16, n).astype(np.uint64)
        else:
            keys = np.full(n, rng.integers(0, 1 << 63, dtype=np.uint64))
        keys = np.sort(keys)
        L, R, _ = lt.radix_tree(keys)
        kL, kR = _karras(keys)
        assert (L == kL).all() and (R == kR).all(), (trial, keys.tolist())


# --- check_lbvh on synthesised records -------------------------------------------------------------

def synthesise(scene):
    """(records, depth) of the LBVH of `scene` in numpy: morton_keys, a stable sort, radix_tree, the
    leaves in sorted order and the boxes bottom-up (children before parents, by recursion depth)."""
    tri = scene.world_triangles()
    n = len(tri)
    keys = lt.morton_keys(scene)[0]
    order = np.argsort(keys, kind="stable")
    L, R, deepest = lt.radix_tree(keys[order])
    rec = np.zeros((2 * n - 1, 16), np.float32)
    ids = rec.view(np.int32)
    first = np.concatenate([[0], np.cumsum(scene.shapes["numTriangles"])]).astype(np.int64)
    lo = np.zeros((2 * n - 1, 3), np.float32)
    hi = np.zeros((2 * n - 1, 3), np.float32)
    for j, g in enumerate(order):
        r = n - 1 + j
        t = tri[g]
        shape = int(np.searchsorted(first, g, side="right")) - 1
        rec[r, 0:3], rec[r, 4:7], rec[r, 8:11] = t[0], t[1] - t[0], t[2] - t[0]
        ids[r, 3], ids[r, 7] = shape, g - first[shape]
        ids[r, 12:14] = -1
        lo[r], hi[r] = t.min(0), t.max(0)
    done = np.zeros(2 * n - 1, bool)
    done[n - 1:] = True
    while not done.all():
        for i in range(n - 1):
            a, b = L[i], R[i]
            if not done[i] and done[a] and done[b]:
                rec[i, 0:4] = lo[a, 0], hi[a, 0], lo[a, 1], hi[a, 1]
                rec[i, 4:8] = lo[b, 0], hi[b, 0], lo[b, 1], hi[b, 1]
                rec[i, 8:12] = lo[a, 2], hi[a, 2], lo[b, 2], hi[b, 2]
                ids[i, 12:14] = a, b
                lo[i], hi[i] = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
                done[i] = True
    return rec, deepest + 1


SCENES = {"dyadic300": lambda: lt.dyadic(300), "same_key257": lambda: lt.same_key(257),
          "same_key1": lambda: lt.same_key(1), "same_key2": lambda: lt.same_key(2)}
_built = {}


def built(name):
    if name not in _built:
        sc = SCENES[name]()
        _built[name] = (sc,) + synthesise(sc)
    sc, rec, depth = _built[name]
    return sc, rec.copy(), depth


@pytest.mark.parametrize("name", list(SCENES))
def test_synthesised_records_pass(name):
    sc, rec, depth = built(name)
    assert lt.check_lbvh(rec, sc, depth) == depth - 1


def _internal_with_internal_children(rec, n):
    ids = rec.view(np.int32)
    i = np.nonzero((ids[:n - 1, 12] < n - 1) & (ids[:n - 1, 13] < n - 1))[0]
    return int(i[len(i) // 2])


def _duplicate_primitive(rec, n):
    rec.view(np.int32)[n - 1 + 5, 7] = rec.view(np.int32)[n - 1 + 40, 7]


def _box_an_ulp_lower(rec, n):
    i = _internal_with_internal_children(rec, n)
    rec[i, 5] = np.nextafter(rec[i, 5], np.float32(-np.inf))      # child 1's x maximum


def _box_an_ulp_wider(rec, n):
    i = _internal_with_internal_children(rec, n)
    rec[i, 8] = np.nextafter(rec[i, 8], np.float32(-np.inf))      # child 0's z minimum: still contains


def _children_swapped(rec, n):
    i = _internal_with_internal_children(rec, n)                  # boxes and indices: a consistent BVH
    rec[i] = rec[i, [4, 5, 6, 7, 0, 1, 2, 3, 10, 11, 8, 9, 13, 12, 14, 15]]


def _two_parents(rec, n):
    ids = rec.view(np.int32)
    i = _internal_with_internal_children(rec, n)
    ids[i, 12] = ids[0, 12] if i != 0 else ids[1, 12]


def _leaf_vertex_moved(rec, n):
    rec[n - 1 + 7, 1] = np.nextafter(rec[n - 1 + 7, 1], np.float32(np.inf))


CORRUPTIONS = {"duplicate primitive": _duplicate_primitive, "box an ulp lower": _box_an_ulp_lower,
               "box an ulp wider": _box_an_ulp_wider, "children swapped": _children_swapped,
               "two parents": _two_parents, "leaf vertex moved": _leaf_vertex_moved}


@pytest.mark.parametrize("what", list(CORRUPTIONS))
@pytest.mark.parametrize("name", ["dyadic300", "same_key257"])
def test_single_corruptions_fail(name, what):
    sc, rec, depth = built(name)
    before = rec.copy()
    CORRUPTIONS[what](rec, sc.num_triangles)
    changed = (rec.view(np.uint32) != before.view(np.uint32)).any(1)
    assert changed.sum() == 1, "one record corrupted"
    with pytest.raises(AssertionError):
        lt.check_lbvh(rec, sc, depth)


@pytest.mark.parametrize("off", [-1, 1])
@pytest.mark.parametrize("name", ["dyadic300", "same_key257", "same_key1"])
def test_depth_off_by_one_fails(name, off):
    sc, rec, depth = built(name)
    with pytest.raises(AssertionError):
        lt.check_lbvh(rec, sc, depth + off)


def test_non_identity_transform_is_refused():
    sc, rec, depth = built("same_key2")
    import copy
    moved = copy.copy(sc)
    moved.shapes = sc.shapes.copy()
    moved.shapes["toWorldTransform"][0, 0, 3] = 1.0
    with pytest.raises(AssertionError):
        lt.check_lbvh(rec, moved, depth)


# --- the scenes' premises --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [300, 1000])
def test_dyadic_premises(n):
    f32 = np.float32
    sc = lt.dyadic(n)
    c = lt.dyadic_centroids(n)
    tri = sc.world_triangles()
    assert len(tri) == n
    # the float32 centroid is the lattice point exactly, and the vertices are exact in float32
    assert (tri.astype(np.float64) == c[:, None, :] + 2.0 ** -8 * lt._CORNERS[None]).all()
    cen = ((tri.min(1) + tri.max(1)).astype(f32) * f32(0.5)).astype(f32)
    assert (cen.astype(np.float64) == c).all()
    assert (c * 32 == np.round(c * 32)).all() and c.min() == 0.0 and c.max() == 1.0
    keys, q, ext = lt.morton_keys(sc)
    assert (cen.min(0) == 0).all() and (ext == 1).all()
    # t = c exactly, so the cell is c * 2^21 (the point 1.0 clamps to the last cell)
    assert (q == np.minimum(c * 2 ** 21, 2 ** 21 - 1)).all()
    _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    shared = counts[inverse] > 1
    assert shared.sum() >= n / 4 and (~shared).sum() >= n / 4, (int(shared.sum()), n)
    # equal keys are equal lattice points, and they are not numbered side by side
    assert len(np.unique(c, axis=0)) == len(counts)
    order = np.argsort(keys, kind="stable")
    run = np.nonzero(np.diff(keys[order]) == 0)[0]
    assert (order[run + 1] - order[run] > 1).mean() > 0.9


@pytest.mark.parametrize("n", [1, 2, 64, 257])
def test_same_key_premises(n):
    sc = lt.same_key(n)
    tri = sc.world_triangles()
    assert len(tri) == n and len(np.unique(tri.reshape(n, 9), axis=0)) == n
    keys, q, ext = lt.morton_keys(sc)
    assert (ext == 0).all() and len(np.unique(keys)) == 1
    assert (q == 2 ** 20).all()            # t = 0.5 on every axis


def test_morton_interleave():
    """x << 2 | y << 1 | z, bit by bit, against Python ints."""
    sc = lt.dyadic(300)
    keys, q, _ = lt.morton_keys(sc)
    for k, (x, y, z) in zip(keys[:50].tolist(), q[:50].tolist()):
        want = 0
        for b in range(21):
            want |= ((x >> b) & 1) << (3 * b + 2) | ((y >> b) & 1) << (3 * b + 1) | ((z >> b) & 1) << (3 * b)
        assert k == want and k < (1 << 63)
