"""The order of the compact records (mcrt_qnodes.hip qnode_order_offsets through
mcrt_accel_compact_order; no GPU): for both orders (1 sibling pairs, 2 treelets) and
trees of 1 (a root leaf), 2, 3 and 7 triangles, a left-deep chain of 40 levels and a 5,000-triangle
soup, every record has a place of its own inside the copy, no record crosses a 128-B line where the
order promises co-residence, the promised records share a line, and the right child's reference
follows from the left child's by the 5-bit step the converter stores."""
import numpy as np
import pytest

import qnode_order_util as qu
from mcrt import lib

ORDERS = {"siblings": 1, "treelets": 2}


def _chain(levels):
    """Left-deep: internal records 0 .. levels - 1, each one's left child the next record."""
    n = 2 * levels + 1
    kids = np.full((n, 2), -1, np.int32)
    for k in range(levels):
        kids[k] = (k + 1, levels + (levels - k))
    return kids


def _tree(name):
    if name == "chain40":
        return _chain(40)
    rec, info = lib.build_host_records(qu.soup(int(name[4:])))
    assert not info["two_level"]
    return qu.kids_of(rec)


TREES = ("soup1", "soup2", "soup3", "soup7", "chain40", "soup5000")


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", TREES)
def test_order(name, order):
    kids = _tree(name)
    n = len(kids)
    assert n == (2 * int(name[4:]) - 1 if name.startswith("soup") else 81)
    off, total = lib.compact_order(kids, ORDERS[order])
    off = off.astype(np.int64)
    leaf = kids[:, 0] < 0
    units = np.where(leaf, 3, 2)
    # a place of its own: sorted by offset, each record ends where or before the next begins
    by = np.argsort(off)
    assert off[by[0]] == 0 and by[0] == 0, "the root is the first record"
    assert (off[by][1:] >= (off + units)[by][:-1]).all() and off[by[-1]] + units[by[-1]] == total
    # two lines in a row hold more than one line's worth: what opens the second did not fit the first
    packed = int(units.sum())
    assert packed <= total <= 2 * packed + 8
    # reachable exactly once by the walk's own arithmetic: left reference stored, right = left + step
    seen = np.zeros(n, bool)
    stack = [(0, (0 << 1) | int(leaf[0]))]
    while stack:
        i, ref = stack.pop()
        assert not seen[i] and ref >> 1 == off[i] and (ref & 1) == int(leaf[i])
        seen[i] = True
        if leaf[i]:
            continue
        l, r = kids[i]
        step = 2 * (off[r] - off[l]) + int(leaf[r]) - int(leaf[l])
        assert 3 <= step <= 31, step
        cl = (int(off[l]) << 1) | int(leaf[l])
        stack += [(l, cl), (r, cl + int(step))]
    assert seen.all()
    # co-residence
    line = off // 8
    last = (off + units - 1) // 8
    inner = np.flatnonzero(~leaf)
    l, r = kids[inner, 0], kids[inner, 1]
    assert (line == last).all(), "a record crosses a line"
    if order == "siblings":
        assert (line[l] == line[r]).all()
        return
    depth = qu.depths(kids)
    heads = inner[depth[inner] % 2 == 0]   # the records that start a treelet: even levels
    assert (line[kids[heads, 0]] == line[heads]).all() and (line[kids[heads, 1]] == line[heads]).all()


def test_refuses_children_below_their_parent():
    kids = np.array([[1, 2], [-1, -1], [-1, -1]], np.int32)
    assert lib.compact_order(kids, 1)[1] == 8
    bad = kids.copy()
    bad[0] = (0, 2)
    with pytest.raises(Exception):
        lib.compact_order(bad, 1)
    with pytest.raises(Exception):
        lib.compact_order(kids, 3)
