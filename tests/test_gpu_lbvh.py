"""The device linear BVH (mcrt_accel_opts.device_build = 1, mcrt_gpubuild.hip) against the ground truth
of tests/lbvh_truth.py, record for record.

  * structure: lbvh_truth.check_lbvh (numbering, one parent each, the leaves a permutation of the
    triangles, child boxes EQUAL to the exact float32 bounds, contiguous leaf ranges, the reported
    depth == deepest leaf level + 1) on the flat scenes of tests/build_opts.py, on the dyadic and
    same_key scenes and on coplanar soups on each side of the builder's 256-thread block;
  * the exact tree: on scenes whose Morton quotients are exact, leaf j is triangle order[j] of a
    STABLE sort of lbvh_truth.morton_keys and every internal record's children are
    lbvh_truth.radix_tree's (on same_key the index tie-break of delta decides the whole tree);
  * determinism: two builds give the same bytes, though atomics order the bottom-up pass;
  * deep trees: geo_tame and geo switch the wave packets off and need three and more spill blocks;
    the walk and a PT frame over such a tree are judged by criteria existing tests fixed
    (test_gpu_build_opts.py's deep tree against the oracle, test_gpu_build.py's 99.9 % of pixels).

Every assertion is an equality or one of those criteria.  One exception to the 64-B-records-only
evidence: with one or two triangles the LBVH's numbering is depth-first, the converter to compact
records takes it, and info()["bytes"] > 64 * nodes (see lbvh()).

Per scene, measured (printed with -s; the key counts are recomputed with an IEEE division, so only
those of dyadic and same_key are the device's for certain):

  scene         n      distinct keys  deepest leaf  reported depth  spill blocks  2 * depth > 64
  grid          3000   3000           16            17              2             no
  clusters      3000   1716           23            24              2             no
  coplanar      3000   3000           15            16              2             no
  mixed         15252  15222          24            25              2             no
  geo           3000   594            48            49              4             yes
  geo_tame      240    127            39            40              3             yes
  dyadic300     300    201            13            14              1             no
  same_key257   257    1              9             10              1             no
  root1         1      1              0             1               1             no
  root2         2      2              1             2               1             no
  root3         3      3              2             3               1             no
  root255       255    255            11            12              1             no
  root256       256    256            11            12              1             no
  root257       257    257            11            12              1             no
  root511       511    511            12            13              1             no
  root513       513    513            12            13              1             no

The deepest levels equal those of a numpy emulation with an IEEE division on every scene.  The three
premises hold on the device: the fast division returns c for c / 1.0 (dyadic's leaf order is the
recomputed one), the depth is the deepest leaf's level + 1, equal keys keep ascending triangle number.

What the tests notice was checked once with deliberately wrong libraries (mutants that cannot change
an index, a loop bound or a launch size); "before": test_gpu_build.py's queries and frames,
test_gpu_ray_truth.py's lbvh layout, test_gpu_shadow_hints.py's nesting / depth and hints tests of
builder 1, test_gpu_quant_nodes.py::test_lbvh_keeps_64b_records:

  k_bottom_up takes boxMin.z from the left child only
      here:   13 of 26 fail: test_structure on every scene that is not flat in z (7), test_exact_tree
              (4, through check_lbvh), the deep walk and the deep frame
      before: caught as well -- the four query cases, the edge and tiny scenes of the ray truth, the
              frames, the nesting test and the hints test all fail (boxes that small lose hits)
  the leaf record stores primOf[j] instead of primOf[prim]
      here:   17 of 26 fail: test_structure from 3 triangles on (13; same_key257's nested triangles
              sort into triangle order, so j == prim there), test_exact_tree on dyadic, the deep walk
              and the deep frame
      before: caught as well -- the four query cases and the edge scene of the ray truth (every leaf
              is wrong; a few wrong leaves would pass their 99.99 %).  Its renders were not run:
              shading would index with another triangle's primitive number
  *depthOut = h
      here:   22 of 26 fail: every test_structure and test_exact_tree case and the deep-tree figures
      before: NOT caught -- all ten existing LBVH tests pass (depth >= leaf_depth still holds)
"""
import numpy as np
import pytest

import build_opts as bo
import lbvh_truth as lt
import refit_util as ru
from helpers import random_rays
from test_gpu_build_opts import deep_answers_against_the_oracle, deep_camera
from test_gpu_ray_truth import _trace

pytestmark = pytest.mark.gpu

BLOCK_EDGES = (1, 2, 3, 255, 256, 257, 511, 513)        # k_prims .. k_bottom_up run 256 threads a block
STRUCTURE = bo.FLAT_SCENES + ("dyadic300", "same_key257") + tuple(f"root{n}" for n in BLOCK_EDGES)
EXACT = ("dyadic300", "dyadic1000", "same_key2", "same_key64", "same_key257")
_cache = {}


def scene(name):
    if name.startswith("dyadic") or name.startswith("same_key"):
        if name not in _cache:
            _cache[name] = lt.dyadic(int(name[6:])) if name.startswith("dyadic") else lt.same_key(int(name[8:]))
        return _cache[name]
    return bo.flat_scene(name)


def lbvh(ctx, sc):
    """(records, reported depth) of the device LBVH of `sc`, with the evidence that it is one: the
    builder's number, and 64-B records only -- the converter to compact records refuses the LBVH's
    numbering.  With one or two triangles that numbering IS depth-first (a leaf; a root and its two
    leaves), so there, and only there, the converter takes the tree and adds its compact copy."""
    from mcrt import lib
    ds = lib.DeviceScene(ctx, sc, device_build=1)
    try:
        info = ds.info()
        n = sc.num_triangles
        assert ds.builder() == 1
        assert info["nodes"] == 2 * n - 1 and info["triangles"] == n, info
        assert info["bytes"] == 64 * info["nodes"] if n > 2 else info["bytes"] > 64 * info["nodes"], info
        return ds.records(), ds.layout()["depth"]
    finally:
        ds.close()


@pytest.mark.parametrize("name", STRUCTURE)
def test_structure(hip_ctx, name):
    sc = scene(name)
    rec, depth = lbvh(hip_ctx, sc)
    deepest = bo.leaf_depth(rec)
    print(f"\nLBVH {name}: n {sc.num_triangles}, distinct keys {len(np.unique(lt.morton_keys(sc)[0]))}, "
          f"deepest {deepest}, depth {depth}, spill blocks {ru.spill_blocks(depth)}, no packets {2 * depth > 64}")
    assert lt.check_lbvh(rec, sc, depth) == deepest
    if sc.num_triangles <= 2:                               # depth-first as well: the SAH builders' truth
        assert bo.check_tree(rec, sc) == deepest


@pytest.mark.parametrize("name", EXACT)
def test_exact_tree(hip_ctx, name):
    """Premise: the builder's fast division returns c exactly for the divisor 1.0 (dyadic), and is
    not reached at all where the extent is 0 (same_key).  A difference in the leaf order on dyadic
    is a finding about k_morton, not a tolerance to add."""
    sc = scene(name)
    n = sc.num_triangles
    rec, depth = lbvh(hip_ctx, sc)
    lt.check_lbvh(rec, sc, depth)
    keys, cells, _ = lt.morton_keys(sc)
    order = np.argsort(keys, kind="stable")
    ids = rec.view(np.int32)
    got = ids[n - 1:, 7]                                    # one shape: the primitive is the triangle
    assert (ids[n - 1:, 3] == 0).all()
    wrong = np.nonzero(got != order)[0]
    for j in wrong[:8]:
        print(f"leaf {j}: triangle {got[j]} cell {cells[got[j]].tolist()} key {int(keys[got[j]]):#x}, "
              f"expected {order[j]} cell {cells[order[j]].tolist()} key {int(keys[order[j]]):#x}")
    assert len(wrong) == 0, f"{len(wrong)} leaves out of the stable Morton order, first {wrong[:8].tolist()}"
    L, R, deepest = lt.radix_tree(keys[order])
    assert (ids[:n - 1, 12] == L).all() and (ids[:n - 1, 13] == R).all(), \
        np.nonzero((ids[:n - 1, 12] != L) | (ids[:n - 1, 13] != R))[0][:8].tolist()
    assert depth == deepest + 1


@pytest.mark.parametrize("name", ["clusters", "same_key257"])
def test_two_builds_give_the_same_bytes(hip_ctx, name):
    sc = scene(name)
    (a, da), (b, db) = lbvh(hip_ctx, sc), lbvh(hip_ctx, sc)
    assert a.tobytes() == b.tobytes() and da == db


# --- deep trees -------------------------------------------------------------------------------------

def test_deep_trees_turn_packets_off_and_need_spill_blocks(hip_ctx):
    """From the records, not from an emulation: geo_tame is too deep for the packet stack and needs
    at least three spill blocks, geo at least four."""
    for name, blocks in (("geo_tame", 3), ("geo", 4)):
        rec, depth = lbvh(hip_ctx, scene(name))
        assert depth == bo.leaf_depth(rec) + 1
        assert 2 * depth > 64, (name, depth)
        assert ru.spill_blocks(depth) >= blocks, (name, depth)


def test_deep_lbvh_walk_against_the_oracle(hip_ctx):
    """The 20 000 rays of test_gpu_build_opts.py's deep fixture through the LBVH of geo_tame, by that
    module's criteria against the oracle's walk of the host tree."""
    from mcrt import lib
    sc = scene("geo_tame")
    rays = random_rays(sc, 20000, seed=21)
    ds = lib.DeviceScene(hip_ctx, sc, device_build=1)
    try:
        assert ds.builder() == 1 and 2 * ds.layout()["depth"] > 64
        answers = _trace(hip_ctx, ds, rays)
    finally:
        ds.close()
    assert (answers[0]["shapeid"] >= 0).mean() > 0.05 and (answers[1] == 1).mean() > 0.05
    deep_answers_against_the_oracle(sc, rays, answers)


def test_deep_lbvh_frame_equals_the_default_trees(hip_ctx):
    """One 64 x 48 depth-3 PT frame of geo_tame: finite, not black, and test_gpu_build.py's criterion
    against the frame over the default tree (bit-identical on >= 99.9 % of pixels)."""
    from mcrt import lib
    sc = scene("geo_tame")
    W, H = 64, 48
    cam = deep_camera(W, H)
    out = []
    for device in (0, 1):
        ds = lib.DeviceScene(hip_ctx, sc, device_build=device)
        assert device == 0 or ds.builder() == 1
        fb = lib.FrameBuffer(hip_ctx, W, H)
        fb.render(ds, cam, frame=1, max_depth=3)
        out.append(fb.read(0))
        fb.close()
        ds.close()
    assert np.isfinite(out[1]).all() and out[1][..., :3].max() > 0
    eq = (out[0].view(np.uint32) == out[1].view(np.uint32)).all(-1)
    assert eq.mean() >= 0.999, eq.mean()
