"""mcrt_accel_update_transforms on the GPU: RTScene::updateDynamicEntities' SetTransform + Commit
(APP/raytracing/scene/RTScene.cpp:317-391), for which RadeonRays refits its two-level structure
(RR/src/intersector/intersector_2level.cpp:495-660: per-mesh trees kept, a fresh top-level Bvh over
the same shape order).  A refit therefore equals a fresh build of the moved scene; ground truth is
lib.build_host_records(moved scene), which tests/test_bvh2l_cpu.py pins against RR's own bvh.cpp
and tests/test_gpu_two_level.py against RR's two-level kernels.

Records are compared as uint32.  The device top-level builder (csrc/mcrt_topbuild.hip) reduces
boxes with order-free min / max, so the one permitted normalisation maps -0.0 to +0.0 in the 12
box words of internal top-level records (refit_util.normalised)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from clref_job import tl_rays
from mcrt import scenes
from mcrt import types as T
from mcrt.camera import scene_camera
from refit_util import (FORCED_CASES, case_opts, forced_case, normalised, similarity_transforms, spill_blocks,
                        synthetic, trace, translate, with_transforms)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PATH_OF = {"device": 1, "host": 2}


@pytest.fixture(scope="module")
def forced(hip_ctx, tmp_path_factory):
    """Results of tests/refit_job.py under MCRT_TOP_BUILD=device and =host, one fresh child
    process each."""
    out = {}
    for mode in PATH_OF:
        path = str(tmp_path_factory.mktemp("refit") / f"{mode}.npz")
        env = dict(os.environ, MCRT_TOP_BUILD=mode)
        r = subprocess.run([sys.executable, os.path.join(HERE, "refit_job.py"), path], env=env, capture_output=True,
                           text=True, timeout=300)
        if r.returncode != 0:
            pytest.fail(f"refit job ({mode}) failed:\n" + r.stdout + r.stderr)
        out[mode] = np.load(path, allow_pickle=False)
    return out


@pytest.fixture(scope="module")
def truth():
    """Fresh host build of each forced case's moved scene, computed once."""
    from mcrt import lib
    cache = {}

    def get(name):
        if name not in cache:
            _, moved, _ = forced_case(name)
            cache[name] = lib.build_host_records(moved, force_2level=True, **case_opts(name))
        return cache[name]
    return get


@pytest.mark.parametrize("mode", list(PATH_OF))
@pytest.mark.parametrize("name", FORCED_CASES)
def test_records_equal_a_fresh_build(forced, truth, name, mode):
    res = forced[mode]
    want, info = truth(name)
    top = info["top_records"]
    assert int(res[f"{name}_path"]) == PATH_OF[mode]
    assert int(res[f"{name}_depth"]) == info["depth"]
    assert bool(res[f"{name}_tail_kept"]), "records beyond the top level changed"
    got = res[f"{name}_top"]
    assert got.shape[0] == top
    np.testing.assert_array_equal(normalised(got, top), normalised(want[:top], top))


@pytest.mark.parametrize("mode", list(PATH_OF))
def test_degenerate_line_traces_like_a_fresh_scene(forced, truth, mode):
    """The 8 x 8 grid moved to x = 2^i: the top tree needs another spill block than the built one."""
    from mcrt import lib
    res = forced[mode]
    built = lib.build_host_records(forced_case("pow2")[0], force_2level=True)[1]
    assert spill_blocks(built["depth"]) != spill_blocks(truth("pow2")[1]["depth"])
    np.testing.assert_array_equal(res["pow2_upd_closest"], res["pow2_fresh_closest"])
    np.testing.assert_array_equal(res["pow2_upd_any"], res["pow2_fresh_any"])


def _moved_scene(name):
    if name == "instances_test":
        sc = scenes.instances_test_scene()
        cam = "instances_test"
    else:
        sc = scenes.instanced_proxy(grid_n=3, body_tris=2000)
        cam = "instanced_proxy"
    mats = [s["toWorldTransform"].copy() for s in sc.shapes]
    mats[2] = translate((0.75, 0.5, -1.0)) @ mats[2]
    mats[5] = translate((-1.0, 0.25, 0.5)) @ scenes._affine(1.3, 40.0, (0, 0, 0), 15.0) @ mats[5]
    return sc, with_transforms(sc, mats), cam


@pytest.mark.parametrize("name", ["instances_test", "instanced_small"])
def test_traces_and_frames_equal_a_fresh_scene(hip_ctx, name):
    from mcrt import lib
    sc, moved, camname = _moved_scene(name)
    ds = lib.DeviceScene(hip_ctx, sc)
    fresh = lib.DeviceScene(hip_ctx, moved)
    assert ds.layout()["two_level"] == 1
    rays = tl_rays(moved)
    before = trace(ds, rays)
    ds.update_transforms(moved.shapes)
    assert ds.update_info()["path"] in (1, 2)
    got, want = trace(ds, rays), trace(fresh, rays)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))
    assert (got.view(np.uint8) != before.view(np.uint8)).any()
    np.testing.assert_array_equal(trace(ds, rays, True), trace(fresh, rays, True))
    W, H = 96, 64
    cam = scene_camera(camname, W, H)
    fa, fb = lib.FrameBuffer(hip_ctx, W, H), lib.FrameBuffer(hip_ctx, W, H)
    for f in (0, 1):
        fa.render(ds, cam, frame=f, max_depth=3)
        fb.render(fresh, cam, frame=f, max_depth=3)
        a, b = fa.read(0), fb.read(0)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.nanmean(a[..., :3]) > 0
    # BDPT: the splat sums are order-nondeterministic (tests/test_gpu_two_level.py's bound)
    fa.render(ds, cam, frame=0, max_depth=2, integrator=T.INTEGRATOR_BDPT)
    fb.render(fresh, cam, frame=0, max_depth=2, integrator=T.INTEGRATOR_BDPT)
    g, ref = fa.read(0)[..., :3], fb.read(0)[..., :3]
    exact = (g.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(g) & np.isnan(ref))
    close = exact | (np.abs(g - ref) <= 4e-6 * (np.abs(g) + np.abs(ref)) + 1e-30)
    print(name, "BDPT bit-exact", exact.mean(), "within 4e-6", close.mean())
    assert close.all(-1).mean() >= 0.999, close.all(-1).mean()
    for o in (fa, fb, ds, fresh):
        o.close()


def test_three_updates_back_to_the_start(hip_ctx):
    from mcrt import lib
    sc = synthetic(70)
    ds = lib.DeviceScene(hip_ctx, sc, force_2level=True)
    original = ds.records()
    depth = ds.layout()["depth"]
    for seed in (1, 2):
        moved = with_transforms(sc, similarity_transforms(70, seed))
        ds.update_transforms(moved.shapes)
        want, info = lib.build_host_records(moved, force_2level=True)
        np.testing.assert_array_equal(normalised(ds.records(), 139), normalised(want, 139))
        assert ds.layout()["depth"] == info["depth"]
    ds.update_transforms(sc.shapes)
    np.testing.assert_array_equal(normalised(ds.records(), 139), normalised(original, 139))
    assert ds.layout()["depth"] == depth
    ds.close()


def test_update_with_frames_in_flight(hip_ctx):
    """No explicit synchronisation between the renders and the update: the call orders itself
    after the launches enqueued on the frame-slot streams."""
    from mcrt import lib
    sc, moved, camname = _moved_scene("instances_test")
    W, H = 96, 64
    cam = scene_camera(camname, W, H)
    ds = lib.DeviceScene(hip_ctx, sc)
    fresh = lib.DeviceScene(hip_ctx, moved)
    fa, fb = lib.FrameBuffer(hip_ctx, W, H), lib.FrameBuffer(hip_ctx, W, H)
    fa.set_frames_in_flight(2)
    fa.render(ds, cam, frame=0, max_depth=3)
    fa.render(ds, cam, frame=1, max_depth=3)
    ds.update_transforms(moved.shapes)
    for f in (0, 1):
        fa.render(ds, cam, frame=f, max_depth=3)
        fb.render(fresh, cam, frame=f, max_depth=3)
        np.testing.assert_array_equal(fa.read(0).view(np.uint32), fb.read(0).view(np.uint32))
    for o in (fa, fb, ds, fresh):
        o.close()


def test_flat_scene_is_rebuilt(hip_ctx):
    from mcrt import lib
    sc = scenes.test_scene()
    mats = [s["toWorldTransform"].copy() for s in sc.shapes]
    mats[1] = translate((0.3, 0.05, -0.2)) @ mats[1]
    moved = with_transforms(sc, mats)
    a, b = lib.DeviceScene(hip_ctx, sc), lib.DeviceScene(hip_ctx, sc)
    a.update_transforms(moved.shapes)
    assert a.update_info()["path"] == 3 and a.layout()["two_level"] == 0
    b.update_shapes(moved.shapes)
    b.build()
    np.testing.assert_array_equal(a.records().view(np.uint32), b.records().view(np.uint32))
    W, H = 96, 64
    cam = scene_camera("mixed", W, H)
    fa, fb = lib.FrameBuffer(hip_ctx, W, H), lib.FrameBuffer(hip_ctx, W, H)
    fa.render(a, cam, frame=0, max_depth=3)
    fb.render(b, cam, frame=0, max_depth=3)
    np.testing.assert_array_equal(fa.read(0).view(np.uint32), fb.read(0).view(np.uint32))
    for o in (fa, fb, a, b):
        o.close()


def test_errors(hip_ctx):
    from mcrt import lib
    sc = synthetic(6)
    ds = lib.DeviceScene(hip_ctx, sc, build=False)
    assert ds.update_info()["path"] == 0
    with pytest.raises(lib.MCRTError, match="status 4"):   # MCRT_ERROR_NOT_READY
        ds.update_transforms(sc.shapes)
    ds.build(force_2level=True)
    for field in ("numTriangles", "startVertex"):
        shapes = sc.shapes.copy()
        shapes[field][3] += 1
        with pytest.raises(lib.MCRTError, match="status 1"):   # MCRT_ERROR_INVALID_ARG
            ds.update_transforms(shapes)
    ds.update_transforms(sc.shapes)
    assert ds.update_info()["path"] in (1, 2) and ds.update_info()["ms"] > 0
    ds.close()
