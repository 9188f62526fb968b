"""tests/vertex_refit_util.py checked without a GPU: its deformations, and its structural check
against the host builders (mcrt_accel_build_host_records of the deformed scene: leaf words and exact
boxes of that tree), which a record one ulp off or a stale leaf must fail.  Also the premise of the
GPU walks against the float64 truth: the deformed edge scene keeps its generic and axis rays fully
determined (printed per family with -s)."""
import numpy as np
import pytest

import build_opts as bo
import ray_truth as rt
import vertex_refit_util as vu
from mcrt import lib

SCENES = ("grid", "clusters", "coplanar", "mixed", "root1", "root2", "root3", "root255", "root256", "root257", "root513")


def test_deform_is_deterministic_and_moves_by_an_edge_length():
    sc = bo.flat_scene("mixed")
    a = vu.mean_edge(sc)
    assert 0.01 < a < 10.0
    d0, d1 = vu.deformed(sc), vu.deformed(sc)
    assert d0.positions.dtype == np.float32 and d0.positions.shape == sc.positions.shape
    np.testing.assert_array_equal(d0.positions.view(np.uint32), d1.positions.view(np.uint32))
    np.testing.assert_array_equal(d0.positions[:, 3], sc.positions[:, 3])
    move = np.linalg.norm(d0.positions[:, :3].astype(np.float64) - sc.positions[:, :3], axis=1)
    assert move.max() <= np.sqrt(3.0) * a * (1 + 1e-6) and np.median(move) > 0.5 * a, (move.max(), np.median(move), a)
    assert d0.indices is sc.indices and d0.shapes is sc.shapes
    # a function of the position: vertices that coincide stay together
    _, inv = np.unique(sc.positions[:, :3], axis=0, return_inverse=True)
    order = np.argsort(inv.ravel(), kind="stable")
    same = inv.ravel()[order][1:] == inv.ravel()[order][:-1]
    assert same.any()
    assert (d0.positions[order][1:][same] == d0.positions[order][:-1][same]).all()
    # a second deformation is another one
    assert (vu.deformed(sc, k=2.9, phi=1.0).positions != d0.positions).any()


def test_partial_range_and_collapse():
    sc = bo.flat_scene("mixed")
    mid = len(sc.shapes) // 2
    first, count = vu.shape_vertex_range(sc, mid)
    d = vu.deformed(sc, first=first, count=count)
    changed = (d.positions != sc.positions).any(1)
    assert changed[first:first + count].mean() > 0.9 and not changed[:first].any() and not changed[first + count:].any()
    c = vu.with_vertices(sc, vu.collapse(sc.positions, first, count, (0.25, 1.5, -0.75)))
    tri, sid, _ = vu.builder_triangles(c)
    flat = tri[sid == mid]
    assert (flat == flat[:, :1]).all() and (flat[0, 0] == np.float32([0.25, 1.5, -0.75])).all()
    assert (tri[sid != mid] == vu.builder_triangles(sc)[0][sid != mid]).all()


def _variants(name):
    sc = bo.flat_scene(name)
    n = len(sc.positions)
    yield "deformed", vu.deformed(sc)
    yield "collapsed", vu.with_vertices(sc, vu.collapse(sc.positions, n // 3, max(n // 3, 1), (0.5, -0.25, 0.125)))


@pytest.mark.parametrize("name", SCENES)
def test_check_records_accepts_the_host_builders(name):
    for what, sc in _variants(name):
        for mode in (3, 4):
            rec, info = lib.build_host_records(sc, device_build=mode)
            deepest = vu.check_records(rec, sc)
            assert deepest == bo.check_tree(rec, sc, info["depth"]), (what, mode)


def test_check_records_under_transforms():
    """builder_triangles is the host's xformPoint: the leaves of a force_flat build of shapes that
    share a mesh under different transforms are its triangles word for word."""
    sc = vu.shared_mesh_scene()
    assert (sc.shapes["startIdx"][0] == sc.shapes["startIdx"][1]) and (sc.shapes["startVertex"][0] == sc.shapes["startVertex"][1])
    eye = np.eye(4, dtype=np.float32)
    assert all((s["toWorldTransform"] != eye).any() for s in sc.shapes)
    for s in (sc, vu.deformed(sc)):
        rec, info = lib.build_host_records(s, force_flat=True)
        assert info["two_level"] == 0
        vu.check_records(rec, s)


@pytest.mark.parametrize("name", ["coplanar", "mixed", "root3"])
def test_check_records_rejects_corrupted_records(name):
    sc = vu.deformed(bo.flat_scene(name))
    rec, _ = lib.build_host_records(sc, device_build=3)
    vu.check_records(rec, sc)
    ids = rec.view(np.int32)
    internal = np.nonzero(ids[:, 12] >= 0)[0]
    leaves = np.nonzero(ids[:, 12] < 0)[0]
    rng = np.random.default_rng(5)
    for node in rng.choice(internal, min(6, len(internal)), replace=False):
        for word in (0, 1, 6, 7, 9, 10):   # a lower and an upper bound of each child, one ulp outwards
            bad = rec.copy()
            toward = -np.inf if word in (0, 6, 10) else np.inf
            bad[node, word] = np.nextafter(bad[node, word], np.float32(toward))
            with pytest.raises(AssertionError, match="child boxes"):
                vu.check_records(bad, sc)
            bad[node, word] = np.nextafter(rec[node, word], np.float32(-toward))   # one ulp inwards
            with pytest.raises(AssertionError, match="child boxes"):
                vu.check_records(bad, sc)
    # a stale leaf: the triangle of the scene before the deformation
    old, _ = lib.build_host_records(bo.flat_scene(name), device_build=3)
    at_new, at_old = vu.leaves_by_triangle(rec, sc), vu.leaves_by_triangle(old, bo.flat_scene(name))
    moved = np.nonzero((rec[at_new, :11] != old[at_old, :11]).any(1))[0]
    assert len(moved)
    for t in moved[:4]:
        bad = rec.copy()
        bad[at_new[t], :11] = old[at_old[t], :11]
        with pytest.raises(AssertionError, match="a leaf's"):
            vu.check_records(bad, sc)
    # an edge recomputed from rounded sums instead of the builders' v1 - v0
    bad = rec.copy()
    bad[leaves[0], 4] = np.nextafter(bad[leaves[0], 4], np.float32(np.inf))
    with pytest.raises(AssertionError, match="first edge"):
        vu.check_records(bad, sc)
    # two parents for one record
    if len(internal) > 1:
        bad = rec.copy()
        bad.view(np.int32)[internal[1], 13] = ids[internal[0], 12]
        with pytest.raises(AssertionError):
            vu.check_records(bad, sc)


def test_leaf_words_are_keyed_by_triangle():
    sc = vu.deformed(bo.flat_scene("coplanar"))
    a, _ = lib.build_host_records(sc, device_build=3)
    b, _ = lib.build_host_records(sc, device_build=4)     # another tree over the same leaves
    assert a.shape == b.shape and (a.view(np.uint32) != b.view(np.uint32)).any()
    np.testing.assert_array_equal(vu.leaf_words(a, sc), vu.leaf_words(b, sc))


def test_deformed_edge_scene_keeps_determined_rays():
    """The walks on the GPU are judged on the deformed edge scene's own Case.  The deformation must
    leave a non-trivial share of determined rays; the generic and axis families stay fully
    determined, as they are for the undeformed scene."""
    base, case = vu.deformed_edge_case()
    moved = np.linalg.norm(case.scene.positions[:, :3].astype(np.float64) - base.positions[:, :3], axis=1)
    assert np.median(moved) > 0.05, np.median(moved)
    share = case.shares(rt.K)
    for f in rt.FAMILIES:
        print(f"deformed edge scene (a = {vu.EDGE_AMPLITUDE} mean edges) {f:14s} {int((case.fam == rt.FAMILIES.index(f)).sum()):5d} "
              f"rays, determined closest {share[f][0]:.3f} any {share[f][1]:.3f}")
    assert share["generic"] == (1.0, 1.0) and share["axis"] == (1.0, 1.0), share
    assert case.truth(rt.K).closest_det.mean() > 0.5


def test_python_binding_lists_the_new_entry_points():
    for name in ("mcrt_scene_update_vertices", "mcrt_scene_update_vertices_device", "mcrt_accel_refit"):
        assert name in lib.SIGNATURES and hasattr(lib.lib(), name)
    assert {"update_vertices", "refit"} <= set(dir(lib.DeviceScene))
