"""Shared by the tests of the compact records' order (test_qnode_order_cpu.py,
test_gpu_qnode_order.py): the triangle soup, the child table of a flat tree's 64-B records, and a
decoder of the compact copy that follows references from the root as the walk does."""
import numpy as np

import build_opts as bo

LINE_UNITS = 8   # a 128-B line in 16-B units


def soup(n, seed=21):
    """n random triangles of edge ~0.4 in the cube [-2, 2]^3."""
    rng = np.random.default_rng(seed + n)
    c = rng.uniform(-2.0, 2.0, (n, 1, 3))
    P = c + rng.uniform(-0.2, 0.2, (n, 3, 3))
    return bo._triangle_scene(f"soup_{n}", P.reshape(-1, 3), (0.0, 6.0, -6.0))


def kids_of(rec):
    """int32 (n, 2): the child record indices of a flat tree's 64-B records, (-1, -1) for a leaf."""
    w = np.ascontiguousarray(rec, np.float32).view(np.int32)[:, 12:14].copy()
    w[w[:, 0] < 0] = -1
    return w


def depths(kids):
    d = np.zeros(len(kids), np.int64)
    for i in range(len(kids)):   # parents come first
        if kids[i, 0] >= 0:
            d[kids[i]] = d[i] + 1
    return d


def decode(q, root, kids):
    """Follows the compact copy q (uint32 (units, 4)) from `root` beside the 64-B tree `kids`.
    Asserts that every record is reached exactly once, in its own units, in the 64-B tree's left /
    right roles.  Returns per 64-B record: its unit offset, and its box words -- origin, the twelve
    bytes and the three exponent fields of an internal record; all twelve words of a leaf."""
    n = len(kids)
    off = np.full(n, -1, np.int64)
    words = [None] * n
    used = np.zeros(len(q), bool)
    stack = [(0, int(root))]
    while stack:
        i, ref = stack.pop()
        u, leaf = ref >> 1, ref & 1
        assert off[i] < 0, f"record {i} reached twice"
        assert leaf == int(kids[i, 0] < 0), f"record {i}: leaf bit {leaf}"
        k = 3 if leaf else 2
        assert u + k <= len(q) and not used[u:u + k].any(), f"record {i} overlaps another"
        used[u:u + k] = True
        off[i] = u
        if leaf:
            assert q[u + 2, 3] & 0x7fffffff == i, f"leaf {i} names record {q[u + 2, 3] & 0x7fffffff}"
            words[i] = q[u:u + 3].reshape(-1).copy()
            continue
        meta = int(q[u + 1, 3])
        words[i] = np.concatenate([q[u, :3], q[u + 1, :3], [meta & 0x07ffffff]]).astype(np.uint32)
        cl = int(q[u, 3])
        stack += [(int(kids[i, 0]), cl), (int(kids[i, 1]), cl + (meta >> 27))]
    assert (off >= 0).all(), f"{int((off < 0).sum())} records not reached"
    return off, words
