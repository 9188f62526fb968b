"""Host refit of the two-level structure (mcrt_accel_refit_host_records: RadeonRays' Refit branch,
RR/src/intersector/intersector_2level.cpp:495-660 -- the per-mesh trees stay, a new top-level Bvh
is built over the recomputed world boxes).  RR's Refit builds a fresh top Bvh over the same shape
order, so the refit must equal a fresh build of the moved scene bit for bit; the fresh host build
is pinned against RR's own bvh.cpp in tests/test_bvh2l_cpu.py."""
import numpy as np
import pytest

from mcrt import lib, scenes
from refit_util import (grid_place, power_of_two_line, similarity_transforms, spill_blocks, synthetic, translate,
                        with_transforms)


def _check(scene, moved, **opts):
    got, ginfo = lib.refit_host_records(scene, moved.shapes, **opts)
    want, winfo = lib.build_host_records(moved, **opts)
    assert ginfo == winfo
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    return ginfo


def test_one_instance_translated():
    sc = scenes.instances_test_scene()
    mats = [s["toWorldTransform"].copy() for s in sc.shapes]
    mats[4] = translate((1.5, 0.25, -2.0)) @ mats[4]
    info = _check(sc, with_transforms(sc, mats))
    assert info["two_level"] == 1
    # and the refit is not the identity: the moved scene's records differ from the built one's
    assert not np.array_equal(lib.build_host_records(sc)[0], lib.refit_host_records(sc, with_transforms(sc, mats).shapes)[0])


def test_every_instance_rotated_scaled_tilted():
    sc = scenes.instances_test_scene()
    _check(sc, with_transforms(sc, similarity_transforms(len(sc.shapes), 3, spread=8.0)))


def test_all_collapsed_takes_the_median_path():
    sc = synthetic(40)
    _check(sc, with_transforms(sc, [translate((1.0, 2.0, 3.0))] * 40), force_2level=True)


def test_grid_to_powers_of_two_deepens_the_tree():
    sc = synthetic(64)
    moved = with_transforms(sc, power_of_two_line(64))
    before = lib.build_host_records(sc, force_2level=True)[1]
    after = _check(sc, moved, force_2level=True)
    print("depth", before["depth"], "->", after["depth"])
    assert spill_blocks(before["depth"]) != spill_blocks(after["depth"])


def test_explicit_world_to_local():
    sc = synthetic(20)
    mats = similarity_transforms(20, 5)
    moved = with_transforms(sc, mats)
    w2l = np.stack([np.linalg.inv(M.astype(np.float64)).astype(np.float32) for M in mats])
    w2l[:, 0, 3] += np.float32(0.125)   # not the transpose of the inverse transpose: must be taken as given
    got, ginfo = lib.refit_host_records(sc, moved.shapes, world_to_local=w2l, force_2level=True)
    want, winfo = lib.build_host_records(moved, world_to_local=w2l, force_2level=True)
    assert ginfo == winfo
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, lib.build_host_records(moved, force_2level=True)[0])


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_top_levels(n):
    sc = synthetic(n)
    info = _check(sc, with_transforms(sc, similarity_transforms(n, 7)), force_2level=True)
    assert info["top_records"] == 2 * n - 1
    if n == 1:   # the root is an instance record
        rec = lib.refit_host_records(sc, sc.shapes, force_2level=True)[0]
        assert rec[0].view(np.int32)[12] == -2


def test_flat_scene_is_the_fresh_build():
    sc = scenes.test_scene()
    mats = [s["toWorldTransform"].copy() for s in sc.shapes]
    mats[1] = translate((0.3, 0.05, -0.2)) @ mats[1]
    info = _check(sc, with_transforms(sc, mats), device_build=3)
    assert info["two_level"] == 0


@pytest.mark.parametrize("field", ["numTriangles", "startVertex"])
def test_topology_change_is_rejected(field):
    sc = synthetic(6, grid_place)
    shapes = sc.shapes.copy()
    shapes[field][3] += 1
    with pytest.raises(lib.MCRTError, match="status 1"):
        lib.refit_host_records(sc, shapes, force_2level=True)
