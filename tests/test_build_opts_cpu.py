"""CPU tier of the builders under non-default mcrt_accel_opts (traversal_cost, num_bins, use_sah;
tests/build_opts.py GRID): the host builds are the ground truth of the device builders
(tests/test_gpu_build_opts.py), so they are pinned here

  * against the reference's own builders compiled into oracle/_ref/librrref.so: the flat Bvh2
    (RR/src/accelerator/bvh2.cpp) record for record -- internal / leaf pattern, child indices, all
    twelve child-box words bit for bit, the triangle of every leaf -- and the two-level structure
    (bvh.cpp + the translator, tests/test_bvh2l_cpu.compare_with_reference) with its bottom trees
    and instance leaves;
  * against build_opts.check_tree, a structural truth that shares no code with any builder;
  * and the device SAH build's algorithm (closed-form partition, median fallback, split arithmetic
    of mcrt_sah.h) is rehearsed on the host under the same options (tests/sah_emul)."""
import numpy as np
import pytest

import build_opts as bo
import refit_util as ru
from mcrt import lib, scenes
from oracle import pyoracle as po
from test_bvh2l_cpu import compare_with_reference
from test_sah_emul_cpu import emul, run_emul  # noqa: F401  (emul: the fixture that builds tests/sah_emul)

needs_ref = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/librrref.so not built")
GRID_IDS = [bo.tuple_id(t) for t in bo.GRID]

TWO_LEVEL_SCENES = {
    "instances_test": lambda: scenes.instances_test_scene(0),
    "similarity300": lambda: ru.with_transforms(ru.synthetic(300), ru.similarity_transforms(300, 400)),
    "pow2_line64": lambda: ru.with_transforms(ru.synthetic(64), ru.power_of_two_line(64)),
}


@pytest.fixture(scope="module")
def host_records():
    """Host flat build (device_build 3) of a scene under an option tuple, computed once."""
    cache = {}

    def get(name, t):
        if (name, t) not in cache:
            cache[name, t] = lib.build_host_records(bo.flat_scene(name), device_build=3, **bo.opts(t))
        return cache[name, t]
    return get


def compare_flat_with_reference(rec, ref):
    """Our flat records against the reference's Bvh2 nodes (mcrt.types.RRNODE_DTYPE): both number
    the tree in pre-order, so node j is record j."""
    assert rec.shape[0] == ref.shape[0]
    ids = rec.view(np.int32)
    internal = ids[:, 12] >= 0
    np.testing.assert_array_equal(ref["addr_left"] != 0xffffffff, internal)
    p = np.nonzero(internal)[0]
    np.testing.assert_array_equal(ids[p, 12], ref["addr_left"][p].astype(np.int64))
    np.testing.assert_array_equal(ids[p, 13], ref["addr_right"][p].astype(np.int64))
    R = ref[p]
    want = np.stack([R["lmin_v0"][:, 0], R["lmax_v1"][:, 0], R["lmin_v0"][:, 1], R["lmax_v1"][:, 1],
                     R["rmin_v2"][:, 0], R["rmax"][:, 0], R["rmin_v2"][:, 1], R["rmax"][:, 1],
                     R["lmin_v0"][:, 2], R["lmax_v1"][:, 2], R["rmin_v2"][:, 2], R["rmax"][:, 2]], 1)
    np.testing.assert_array_equal(rec[p, :12].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    lf = np.nonzero(~internal)[0]
    np.testing.assert_array_equal(ids[lf, 7], ref["prim_id"][lf].astype(np.int64))
    np.testing.assert_array_equal(ids[lf, 3], ref["mesh_id"][lf].astype(np.int64))


@needs_ref
@pytest.mark.parametrize("t", bo.GRID, ids=GRID_IDS)
def test_host_builds_equal_the_reference(host_records, t):
    o = bo.opts(t)
    for name in ("mixed", "grid", "clusters", "geo"):
        rec, info = host_records(name, t)
        assert info["two_level"] == 0
        compare_flat_with_reference(rec, po.ref_bvh_nodes(bo.flat_scene(name), **o))
    for name, make in TWO_LEVEL_SCENES.items():
        compare_with_reference(make(), **o)


@pytest.mark.parametrize("t", bo.GRID, ids=GRID_IDS)
def test_host_records_are_a_correct_tree(host_records, t):
    for name in bo.FLAT_SCENES:
        rec, info = host_records(name, t)
        bo.check_tree(rec, bo.flat_scene(name), depth=info["depth"])
        if len(rec) > 1:
            bo.check_nesting(rec)


def test_options_change_the_tree(host_records):
    """Every tuple but the default builds other records on the 3000-triangle soups and the geometric
    scene (a tuple that left the tree alone would test nothing), and the deep trees are deep: SAH
    off and 2 bins take the geometric scene past the 32 levels the packet walk's stack holds."""
    for name in ("grid", "clusters", "geo"):
        base = host_records(name, bo.GRID[0])[0]
        for t in bo.GRID[1:]:
            assert host_records(name, t)[0].tobytes() != base.tobytes(), (name, t)
    for n in bo.ROOT_SIZES:   # the root-size cases of the GPU tier (8 and 9 references: hardly a SAH node)
        base = host_records(f"root{n}", bo.GRID[0])[0]
        for t in ((5, 10.0, True), (64, 10.0, False)):
            assert (host_records(f"root{n}", t)[0].tobytes() != base.tobytes()) == (n >= 64), (n, t)
    assert host_records("geo", (64, 10.0, False))[1]["depth"] > 64
    assert host_records("geo", (2, 10.0, True))[1]["depth"] > 32
    d = host_records("geo_tame", (64, 10.0, False))[1]["depth"]
    assert 2 * d > 64 and ru.spill_blocks(d) == 3, d


@pytest.mark.parametrize("size", list(bo.LATTICE_SIZES))
@pytest.mark.parametrize("bins", bo.LATTICE_BINS)
def test_lattice_scenes(host_records, bins, size):
    """build_opts.lattice: the host build is a correct tree and (with the reference built) the
    reference's; its root splits on a lattice plane p_k, with triangles exactly on it and one ulp
    below; and for every inexact bin count the plane a step E * (1 / bins) would give sends another
    number of triangles left -- the premise under which a device build with a slightly different
    split plane cannot equal the host's on this scene."""
    name, t = f"lattice{bins}_{size}", (bins, 10.0, True)
    sc = bo.flat_scene(name)
    rec, info = host_records(name, t)
    bo.check_tree(rec, sc, depth=info["depth"])
    if po.ref_available():
        compare_flat_with_reference(rec, po.ref_bvh_nodes(sc, **bo.opts(t)))
    f32 = np.float32
    n = sc.num_triangles
    assert (9 <= n <= 256) if size == "wave" else n > 256
    x = sc.world_triangles()[..., 0]
    c = (x.min(1) + x.max(1)) * f32(0.5)
    nl = int(rec.view(np.int32)[0, 13]) // 2          # leaves under the root's first child
    E, k = f32(bo.LATTICE_EXTENT), np.arange(1, bins, dtype=f32)
    p = k * (E / f32(bins))
    won = [i for i in range(bins - 1) if int((c < p[i]).sum()) == nl]
    assert len(won) == 1, won
    i = won[0]
    assert (c == p[i]).any() and (c == np.nextafter(p[i], f32(-np.inf))).any()
    if bins not in (2, 64):
        wrong = k[i] * (E * (f32(1) / f32(bins)))
        assert int((c < wrong).sum()) != nl


@pytest.mark.parametrize("name", [c for c in ru.OPTION_CASES if c.startswith("lattice")])
def test_top_level_lattice_cases(name):
    """refit_util.lattice_line, the top level's counterpart of build_opts.lattice: the host build of
    the moved scene is the reference's; the world boxes' centroids are the intended floats but for a
    few next to a power of two; the root splits on a lattice plane; and the plane a step
    E * (1 / bins) would give parts the shapes elsewhere."""
    _, moved, _ = ru.forced_case(name)
    o = ru.case_opts(name)
    bins, n = o["bins"], len(moved.shapes)
    if po.ref_available():
        compare_with_reference(moved, **o)
    rec, info = lib.build_host_records(moved, force_2level=True, **o)
    f32 = np.float32
    tx = moved.shapes["toWorldTransform"][:, 0, 3].astype(f32)
    c = f32(0.5) * ((f32(0.5) + tx) + (f32(-0.5) + tx))        # transform_bbox of the unit box, then centre
    assert (c == tx).mean() > 0.9 and c.min() == 0 and c.max() == f32(ru.TOP_LATTICE_EXTENT)
    nl = int(rec.view(np.int32)[0, 13]) // 2
    E, k = f32(ru.TOP_LATTICE_EXTENT), np.arange(1, bins, dtype=f32)
    p, wrong = k * (E / f32(bins)), k * (E * (f32(1) / f32(bins)))
    # the reference's partition sends c < plane left or right by the parity of the range
    won = [i for i in range(bins - 1) if int((c < p[i]).sum()) in (nl, n - nl)]
    assert won
    for i in won:
        assert int((c < wrong[i]).sum()) != int((c < p[i]).sum())


@pytest.mark.parametrize("name", ru.OPTION_CASES)
def test_host_refit_keeps_its_options(name):
    """The two-level structure remembers cost / bins / SAH switch for its refits: the host refit of
    a scene built under options equals a fresh build of the moved scene under them, and that top
    tree is not the default options' (the case would test nothing otherwise)."""
    sc, moved, _ = ru.forced_case(name)
    o = ru.case_opts(name)
    want, info = lib.build_host_records(moved, force_2level=True, **o)
    got, ginfo = lib.refit_host_records(sc, moved.shapes, force_2level=True, **o)
    assert ginfo == info
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    top = info["top_records"]
    assert want[:top].tobytes() != lib.build_host_records(moved, force_2level=True)[0][:top].tobytes()


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("t", bo.GRID, ids=GRID_IDS)
def test_device_algorithm_matches_host_build_under_options(emul, t, kind):  # noqa: F811
    run_emul(emul, 20000, 1, kind, t)
