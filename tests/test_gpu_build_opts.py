"""The device builders under non-default mcrt_accel_opts (traversal_cost, num_bins, use_sah), on the
option tuples and scenes of tests/build_opts.py.

Ground truth is the host build under the same options, which tests/test_build_opts_cpu.py pins to
the reference's own builders for every tuple, and build_opts.check_tree, which shares no code with a
builder.  Every assertion is an equality: records as uint32 with +0 == -0 (the device reduces boxes
with order-free min / max), exact min / max boxes, equal depths, zero failures against the float64
ray truth (tests/ray_truth.py), bit-identical answers and frames -- or a criterion an existing test
fixed (tests/test_gpu_trace.py, against the oracle).

  * mcrt_sahbuild.hip (device_build 2, the default) against mcrt_bvh.cpp (device_build 3): bin counts
    whose step ext / bins is inexact, a masked lane of the wave-wide sweep (63), many equal prices
    (cost 1e6: the first minimum wins), no winning bin (cost FLT_MAX: plane = centroid minimum, then
    the median fallback), SAH off, and more bins than the device supports (the build must fall back
    to the host and say so); root sizes on each side of the builder's thresholds.
  * mcrt_accel_update_transforms keeps the options: the forced device / host top-level builds run
    the option cases of refit_util.FORCED_CASES in tests/test_gpu_refit.py; here the paths nothing
    forces (65 bins -> host, a flat scene -> a rebuild with the last options).
  * the walks over such trees: deeper ones (no packets, three spill blocks), other shapes.

What the record comparisons notice was checked once with a deliberately wrong library: the split
step of the one-wave path, of the level passes' sweep and of the top-level build computed as
ext * (1 / bins) instead of ext / bins (an ulp off at 3, 5, 7, 33 and 63 bins).  Of the 90 scene x
tuple cases of test_device_sah_equals_host_build only two then fail (7 and 63 bins on the mixed
scene) and no root-size case: an ulp of the plane rarely moves a triangle of a random scene.  The
lattice scenes (build_opts.lattice: centroids exactly on and one float below every plane the root
prices) fail at all five bin counts on both paths and pass at 2 and 64 bins, where the step is
exact; in tests/test_gpu_refit.py the four lattice cases fail on the device path and the other option
cases do not notice.  The lattice premise itself is asserted on the CPU (test_build_opts_cpu.py).
"""
import numpy as np
import pytest

import build_opts as bo
import ray_truth as rt
import refit_util as ru
from helpers import random_rays
from mcrt.camera import make_camera
from oracle import pyoracle as po
from test_gpu_ray_truth import _both_orders, _build, _trace, shared_case
from test_gpu_sah_build import _same_records
from test_gpu_trace import _no_unexplained_ray

pytestmark = pytest.mark.gpu
GRID_IDS = [bo.tuple_id(t) for t in bo.GRID]
MID = (64, 10.0, False)


def _first_difference(a, b):
    d = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(1))[0] if a.shape == b.shape else []
    return f"shapes {a.shape} {b.shape}, first differing records {list(d[:8])}"


def _device_against_host(ctx, sc, t):
    """Builds `sc` under tuple t on the device and on the host; asserts what the module's docstring
    says about the pair.  Returns the number of record sets compared."""
    from mcrt import lib
    o = bo.opts(t)
    host = lib.DeviceScene(ctx, sc, device_build=3, **o)
    dev = lib.DeviceScene(ctx, sc, device_build=2, **o)      # a fallback returns OK as well
    try:
        assert host.builder() == 0
        assert dev.builder() == (0 if t in bo.HOST_ONLY else 2), (t, dev.builder())
        a, b = host.records(), dev.records()
        assert _same_records(a, b), _first_difference(a, b)
        assert dev.layout()["depth"] == host.layout()["depth"]
        bo.check_tree(b, sc, depth=dev.layout()["depth"])
        bo.check_tree(a, sc, depth=host.layout()["depth"])
    finally:
        host.close()
        dev.close()
    return 2


@pytest.mark.parametrize("name", bo.FLAT_SCENES)
@pytest.mark.parametrize("t", bo.GRID, ids=GRID_IDS)
def test_device_sah_equals_host_build(hip_ctx, t, name):
    _device_against_host(hip_ctx, bo.flat_scene(name), t)


@pytest.mark.parametrize("n", bo.ROOT_SIZES)
def test_root_sizes(hip_ctx, n):
    """The root request on each side of the one-lane (8), one-wave (256) and chunk (4096) sizes."""
    for t in ((64, 10.0, True), (5, 10.0, True), MID):
        _device_against_host(hip_ctx, bo.flat_scene(f"root{n}"), t)


@pytest.mark.parametrize("size", list(bo.LATTICE_SIZES))
@pytest.mark.parametrize("bins", bo.LATTICE_BINS)
def test_centroids_on_the_candidate_planes(hip_ctx, bins, size):
    """build_opts.lattice: triangles exactly on and one ulp below every plane the root prices, so a
    split plane that is off by an ulp changes the partition (tests/test_build_opts_cpu.py checks
    that premise); one scene for the one-wave path, one for the level passes."""
    _device_against_host(hip_ctx, bo.flat_scene(f"lattice{bins}_{size}"), (bins, 10.0, True))


def test_explicit_default_options_equal_no_options(hip_ctx):
    """mcrt_accel_build(scene, NULL) and the explicit (10, 64, SAH) through device_build 0."""
    from mcrt import lib
    sc = bo.flat_scene("grid")
    plain = lib.DeviceScene(hip_ctx, sc, build=False)
    lib._check(lib.lib().mcrt_accel_build(plain.h, None), hip_ctx.h)
    explicit = lib.DeviceScene(hip_ctx, sc, cost=10.0, bins=64, sah=True, device_build=0)
    assert plain.builder() == 2 and explicit.builder() == 2
    np.testing.assert_array_equal(plain.records().view(np.uint32), explicit.records().view(np.uint32))
    assert plain.layout() == explicit.layout()
    plain.close()
    explicit.close()


# --- refits keep their options --------------------------------------------------------------------

def test_refit_with_65_bins_takes_the_host_path(hip_ctx):
    """More bins than the device top-level build supports: the refit runs on the host (path 2) with
    the remembered options, whatever the size of the top level."""
    from mcrt import lib
    sc, moved, _ = ru.forced_case("n300")
    ds = lib.DeviceScene(hip_ctx, sc, force_2level=True, bins=65)
    before = ds.records()
    ds.update_transforms(moved.shapes)
    assert ds.update_info()["path"] == 2
    want, info = lib.build_host_records(moved, force_2level=True, bins=65)
    top = info["top_records"]
    after = ds.records()
    assert ds.layout()["depth"] == info["depth"]
    assert after[top:].tobytes() == before[top:].tobytes()
    np.testing.assert_array_equal(ru.normalised(after[:top], top), ru.normalised(want[:top], top))
    assert want[:top].tobytes() != lib.build_host_records(moved, force_2level=True)[0][:top].tobytes()
    ds.close()


def test_flat_update_rebuilds_with_the_last_options(hip_ctx):
    from mcrt import lib
    sc = bo.flat_scene("grid")
    o = bo.opts((5, 1e6, False))
    moved = ru.with_transforms(sc, [ru.translate((0.5, -0.25, 2.0))] * len(sc.shapes))
    ds = lib.DeviceScene(hip_ctx, sc, **o)
    assert ds.builder() == 2
    ds.update_transforms(moved.shapes)
    assert ds.update_info()["path"] == 3 and ds.layout()["two_level"] == 0 and ds.builder() == 2
    want, info = lib.build_host_records(moved, device_build=3, **o)
    got = ds.records()
    # word 13 of a leaf on the device: its parent's index (the occluder hints); -1 as the host builds it
    leaf = got.view(np.int32)[:, 12] < 0
    got.view(np.int32)[leaf, 13] = -1
    assert _same_records(want, got), _first_difference(want, got)
    assert ds.layout()["depth"] == info["depth"]
    assert want.tobytes() != lib.build_host_records(moved, device_build=3)[0].tobytes()
    ds.close()


# --- the walks over such trees --------------------------------------------------------------------

WALK_OPTS = ((2, 10.0, True), (63, 10.0, True), (64, bo.FLT_MAX, True), MID)


@pytest.mark.parametrize("layout", ["compact", "plain64", "instanced"])
@pytest.mark.parametrize("t", WALK_OPTS, ids=[bo.tuple_id(t) for t in WALK_OPTS])
def test_walks_against_the_ray_truth(hip_ctx, t, layout):
    """Zero strong and zero weak failures against the float64 brute force, whose truths (and
    determined shares, tabulated in tests/test_gpu_ray_truth.py) do not depend on the tree."""
    from mcrt import lib
    o = bo.opts(t)
    if layout == "instanced":
        case, K = shared_case("instanced"), rt.K_2L
        ds = lib.DeviceScene(hip_ctx, case.scene, **o)
        assert ds.layout()["two_level"] == 1
    else:
        case, K = shared_case("edge0"), rt.K
        ds = _build(hip_ctx, case.scene, layout, opts=o)
        assert ds.builder() == 2
    try:
        bad = _both_orders(hip_ctx, ds, case, case.truth(K), f"{layout} {bo.tuple_id(t)}")
    finally:
        ds.close()
    assert not bad, "\n".join(bad)


@pytest.fixture(scope="module")
def deep(hip_ctx):
    """geo_tame with SAH off, as compact and as 64-B records, and 20 000 rays with both walks'
    answers.  Its levels span 2^40, so it is not judged with ray_truth (whose constants assume one
    scale) but by the criteria below."""
    sc = bo.flat_scene("geo_tame")
    rays = random_rays(sc, 20000, seed=21)
    out = {"scene": sc, "rays": rays}
    for layout in ("compact", "plain64"):
        ds = _build(hip_ctx, sc, layout, opts=bo.opts(MID))
        out[layout + "_depth"] = ds.layout()["depth"]
        out[layout] = _trace(hip_ctx, ds, rays)
        ds.close()
    return out


def test_deep_tree_compact_walk_equals_64b_walk(deep):
    d = deep["plain64_depth"]
    assert deep["compact_depth"] == d
    assert 2 * d > 64 and ru.spill_blocks(d) == 3, d        # no packets, three spill blocks
    (hc, ac), (hp, ap) = deep["compact"], deep["plain64"]
    assert (hp["shapeid"] >= 0).mean() > 0.05 and (ap == 1).mean() > 0.05
    np.testing.assert_array_equal(hc.view(np.uint8), hp.view(np.uint8))
    np.testing.assert_array_equal(ac, ap)


def deep_camera(W, H):
    """The camera of the deep-tree frames (here and in tests/test_gpu_lbvh.py)."""
    return make_camera((0.4, 0.05, -1.5), (0.4, 0.0, 0.0), W, H, fovy=45.0, near=0.1, far=30.0)


def deep_answers_against_the_oracle(sc, rays, answers):
    """tests/test_gpu_trace.py's test_closest_vs_oracle / test_any_vs_oracle criteria, unchanged, on
    `answers` (closest hits, any-hit answers of `rays`) against the oracle's walk of the host tree
    of `sc` with SAH off."""
    o = po.OracleScene(sc)
    o.build(10.0, 64, False)
    ho, hg = o.closest(rays), answers[0]
    same = (ho["shapeid"] == hg["shapeid"]) & (ho["primid"] == hg["primid"])
    assert same.mean() > 0.999, same.mean()
    hit = same & (ho["shapeid"] >= 0)
    np.testing.assert_allclose(hg["uvwt"][hit, 3], ho["uvwt"][hit, 3], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(hg["uvwt"][hit, :2], ho["uvwt"][hit, :2], atol=2e-3)
    diff = ~same & (ho["shapeid"] >= 0) & (hg["shapeid"] >= 0)
    if diff.any():
        np.testing.assert_allclose(hg["uvwt"][diff, 3], ho["uvwt"][diff, 3], rtol=1e-3)
    _no_unexplained_ray(sc, rays, ~same, "closest_det")
    a, g = o.any(rays), answers[1]
    assert (a == g).mean() > 0.999
    _no_unexplained_ray(sc, rays, a != g, "any_det")


def test_deep_tree_against_the_oracle(deep):
    """The 64-B walk's answers against the oracle's walk of the same tree."""
    deep_answers_against_the_oracle(deep["scene"], deep["rays"], deep["plain64"])


def test_deep_tree_frames_bit_identical(hip_ctx):
    """One 64 x 48 depth-3 PT frame of geo_tame (SAH off) over the device-built and the host-built
    records."""
    from mcrt import lib
    sc = bo.flat_scene("geo_tame")
    W, H = 64, 48
    cam = deep_camera(W, H)
    out = []
    for device in (3, 2):
        ds = lib.DeviceScene(hip_ctx, sc, device_build=device, **bo.opts(MID))
        fb = lib.FrameBuffer(hip_ctx, W, H)
        fb.render(ds, cam, frame=1, max_depth=3)
        out.append(fb.read(0))
        fb.close()
        ds.close()
    assert np.isfinite(out[0]).all() and out[0][..., :3].max() > 0
    np.testing.assert_array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
