"""Deforming meshes on the GPU: mcrt_scene_update_vertices(_device) + mcrt_accel_refit
(mcrt_refit.hip), through lib.DeviceScene.update_vertices / refit.

Records: after an update and a refit the records are a correct tree of the DEFORMED scene by
equality (build_opts.check_tree, lbvh_truth.check_lbvh, and vertex_refit_util.check_records, which
also takes shape transforms), words 12..15 of every record are the build's (the topology is kept),
and every leaf equals the leaf of the same (shape, primitive) in a fresh build of the deformed
scene by the same builder -- in 15 of its 16 words: word 13 of a leaf is the index of its parent
record (k_leaf_parents), which belongs to the tree and differs between two topologies; it is
covered by "words 12..15 keep their bits" and by check_records (it names the leaf's parent).

Walks: the refitted compact, 64-B and LBVH layouts against the float64 truth of the deformed edge
scene (0 strong, 0 weak failures; tests/test_vertex_refit_cpu.py holds the premise); one tree under
every walk gives bit-identical frames; against a fresh build the criteria of tests/test_gpu_build.py
for "another tree".

Shading: the guides and the albedo AOV of the updated scene equal a fresh scene's bit for bit at
every pixel whose primary hits agree.  The primary primitive is not exposed per pixel; where it
agrees the two walks return the same hit bit for bit, so the depth words |P - cam| agree too: the
pixels with equal depth words are a superset of those with equal primitives, and the equality is
asserted on that superset."""
import os

import numpy as np
import pytest

import build_opts as bo
import lbvh_truth
import ray_truth as rt
import refit_util as ru
import vertex_refit_util as vu
from helpers import random_rays
from mcrt import types as T
from mcrt.camera import scene_camera

pytestmark = pytest.mark.gpu

SCENES = ("grid", "clusters", "coplanar", "mixed", "root1", "root2", "root3", "root255", "root256", "root257", "root513")
BUILDERS = {"device_sah": {}, "host_sah": {"device_build": 3}, "perf_tree": {"device_build": 4}, "lbvh": {"device_build": 1}}
NOT_READY, INVALID_ARG = 4, 1
W, H = 96, 64


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(rec, scene, builder, depth):
    """The structural truths: the builder's own, then the numbering-free one."""
    if builder == "lbvh":
        lbvh_truth.check_lbvh(rec, scene, depth)
    else:
        bo.check_tree(rec, scene, depth)
    vu.check_records(rec, scene)


def _variants(sc):
    n = len(sc.positions)
    return (("deformed", vu.deformed(sc)),
            ("collapsed", vu.with_vertices(sc, vu.collapse(sc.positions, n // 3, max(n // 3, 1), (0.5, -0.25, 0.125)))))


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", SCENES)
def test_refitted_records_are_a_tree_of_the_deformed_scene(hip_ctx, name, builder):
    from mcrt import lib
    sc = bo.flat_scene(name)
    ds = lib.DeviceScene(hip_ctx, sc, **BUILDERS[builder])
    try:
        rec0, info0, depth = ds.records(), ds.info(), ds.layout()["depth"]
        _check(rec0, sc, builder, depth)
        for what, moved in _variants(sc):
            ds.update_vertices(moved.positions)
            ds.refit()
            assert ds.update_info()["path"] == 4, what
            rec = ds.records()
            assert ds.layout()["depth"] == depth and ds.info()["nodes"] == info0["nodes"], what
            _check(rec, moved, builder, depth)
            np.testing.assert_array_equal(_u32(rec)[:, 12:16], _u32(rec0)[:, 12:16], err_msg=f"{what}: topology words")
            fresh = lib.DeviceScene(hip_ctx, moved, **BUILDERS[builder])
            try:
                np.testing.assert_array_equal(vu.leaf_words(rec, moved), vu.leaf_words(fresh.records(), moved),
                                              err_msg=f"{what}: leaves against a fresh build")
            finally:
                fresh.close()
    finally:
        ds.close()


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["mixed", "root1", "root257"])
def test_idempotence_and_return(hip_ctx, name, builder):
    from mcrt import lib
    sc = bo.flat_scene(name)
    ds = lib.DeviceScene(hip_ctx, sc, **BUILDERS[builder])
    try:
        rec0, info0, depth = ds.records(), ds.info(), ds.layout()["depth"]
        ds.refit()                                   # unchanged vertices
        np.testing.assert_array_equal(_u32(ds.records()), _u32(rec0))
        assert ds.info()["bytes"] == info0["bytes"]
        ds.update_vertices(sc.positions)             # the same vertices again
        ds.refit()
        np.testing.assert_array_equal(_u32(ds.records()), _u32(rec0))
        a, b = vu.deformed(sc), vu.deformed(sc, 0.6, k=2.9, phi=1.0)
        ds.update_vertices(a.positions)
        ds.refit()
        ds.update_vertices(b.positions)              # two deformations in a row: the counters start at zero again
        ds.refit()
        _check(ds.records(), b, builder, depth)
        ds.update_vertices(sc.positions)             # and back
        ds.refit()
        np.testing.assert_array_equal(_u32(ds.records()), _u32(rec0))
        assert ds.info()["bytes"] == info0["bytes"]
    finally:
        ds.close()


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_partial_range(hip_ctx, builder):
    """Only the vertices of the middle shape of `mixed`, as a range."""
    from mcrt import lib
    sc = bo.flat_scene("mixed")
    first, count = vu.shape_vertex_range(sc, len(sc.shapes) // 2)
    moved = vu.deformed(sc, first=first, count=count)
    ds = lib.DeviceScene(hip_ctx, sc, **BUILDERS[builder])
    try:
        depth = ds.layout()["depth"]
        ds.update_vertices(moved.positions[first:first + count], first=first)
        ds.refit()
        _check(ds.records(), moved, builder, depth)
    finally:
        ds.close()


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_shared_mesh_under_transforms_and_transform_only_refit(hip_ctx, builder):
    """Two shapes with different transforms share one mesh (force_flat): a vertex update moves both.
    Then a transform-only refit: update_shapes + refit."""
    from mcrt import lib
    opts = dict(BUILDERS[builder], force_flat=True)
    sc = vu.shared_mesh_scene()
    ds = lib.DeviceScene(hip_ctx, sc, **opts)
    try:
        assert ds.layout()["two_level"] == 0
        rec0 = ds.records()
        vu.check_records(rec0, sc)
        moved = vu.deformed(sc)
        mats = [np.array(m, np.float32) for m in sc.shapes["toWorldTransform"]]
        mats[1] = ru.translate((0.4, -0.3, 0.2)) @ mats[1] @ np.diag([1.0, 1.5, 1.0, 1.0]).astype(np.float32)
        mats[2] = ru.translate((0.0, 0.25, 0.0)) @ mats[2]
        posed = ru.with_transforms(moved, mats)
        for what, now, step in (("vertices", moved, lambda: ds.update_vertices(moved.positions)),
                                ("transforms", posed, lambda: ds.update_shapes(posed.shapes))):
            step()
            ds.refit()
            assert ds.update_info()["path"] == 4, what
            rec = ds.records()
            vu.check_records(rec, now)               # leaves and exact boxes, by the numpy bottom-up
            np.testing.assert_array_equal(_u32(rec)[:, 12:16], _u32(rec0)[:, 12:16], err_msg=what)
            fresh = lib.DeviceScene(hip_ctx, now, **opts)
            try:
                np.testing.assert_array_equal(vu.leaf_words(rec, now), vu.leaf_words(fresh.records(), now), err_msg=what)
            finally:
                fresh.close()
    finally:
        ds.close()


def test_device_pointer_variant(hip_ctx):
    """Same records as the host variant; then a host build of that scene must see the vertices that
    only the device has."""
    import torch
    from mcrt import lib
    sc = bo.flat_scene("mixed")
    moved = vu.deformed(sc, normals=True)
    a, b = lib.DeviceScene(hip_ctx, sc), lib.DeviceScene(hip_ctx, sc)
    fresh = lib.DeviceScene(hip_ctx, moved, device_build=3)
    try:
        a.update_vertices(moved.positions, moved.normals)
        a.refit()
        dp = torch.from_numpy(moved.positions.copy()).cuda()
        dn = torch.from_numpy(moved.normals.copy()).cuda()
        torch.cuda.synchronize()
        b.update_vertices(dp.data_ptr(), dn.data_ptr(), count=len(moved.positions))
        b.refit()
        assert b.update_info()["path"] == 4
        np.testing.assert_array_equal(_u32(a.records()), _u32(b.records()))
        cam = scene_camera("mixed", W, H)
        fa, fb = lib.FrameBuffer(hip_ctx, W, H), lib.FrameBuffer(hip_ctx, W, H)
        fa.render(a, cam, frame=0, max_depth=2)
        fb.render(b, cam, frame=0, max_depth=2)
        np.testing.assert_array_equal(_u32(fa.read(0)), _u32(fb.read(0)))   # the normals arrived as well
        fa.close()
        fb.close()
        b.build(device_build=3)                      # reads the host copy: downloaded first
        np.testing.assert_array_equal(_u32(b.records()), _u32(fresh.records()))
        # a host update after a device update lands in both copies
        back = vu.deformed(sc, 0.5, k=2.9)
        b.update_vertices(dp.data_ptr(), count=len(moved.positions))
        b.update_vertices(back.positions[100:200], first=100)
        b.build(device_build=3)
        mix = moved.positions.copy()
        mix[100:200] = back.positions[100:200]
        want, _ = lib.build_host_records(vu.with_vertices(sc, mix), device_build=3)
        got = b.records()
        got.view(np.int32)[got.view(np.int32)[:, 12] < 0, 13] = -1
        np.testing.assert_array_equal(_u32(got), _u32(want))
    finally:
        for o in (a, b, fresh):
            o.close()


# --- walks -----------------------------------------------------------------------------------------

LAYOUTS = {"compact": ({}, {}), "plain64": ({"MCRT_QUANT_NODES": "0"}, {}), "lbvh": ({}, {"device_build": 1})}


def _trace(ctx, ds, rays, init=-7):
    import torch
    n = len(rays)
    r = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    h0 = np.zeros(n, T.ISECT_DTYPE)
    h0["shapeid"] = init
    h0["primid"] = init
    h = torch.from_numpy(h0.view(np.uint8).copy()).cuda()
    a = torch.full((n,), init, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ds.trace_closest(r.data_ptr(), n, h.data_ptr())
    ds.trace_any(r.data_ptr(), n, a.data_ptr())
    ctx.sync()
    return h.cpu().numpy().view(T.ISECT_DTYPE), a.cpu().numpy()


def _judge_both_orders(ctx, ds, case, tr, what):
    """Shuffled rays and whole 64-ray octant blocks against the truth; the failures as text."""
    rng = np.random.default_rng(7)
    blocks = rt.octant_blocks(case.rays)
    oc = rt.octant(case.rays[blocks]).reshape(-1, 64)
    assert (oc == oc[:, :1]).all() and set(oc[:, 0].tolist()) == set(range(8))
    out = []
    for order, index in (("shuffled", rng.permutation(len(case.rays))), ("octant blocks", blocks)):
        rays = case.rays[index]
        hits, occl = _trace(ctx, ds, rays)
        vc = rt.judge(tr, rays, hits=hits, index=index)
        va = rt.judge(tr, rays, occl=occl, index=index)
        print(f"{what} {order}: closest {vc.active} rays, {vc.determined} determined, {vc.weak_only} weak-only, "
              f"{len(vc.strong)}/{len(vc.weak)} failures; any {va.determined} determined, {va.weak_only} weak-only, "
              f"{len(va.strong)}/{len(va.weak)} failures")
        out += [f"{what} {order} {tag}: {v}" for tag, v in (("closest", vc), ("any", va)) if not v.ok()]
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_refitted_walks_against_the_float64_truth(hip_ctx, layout):
    from mcrt import lib
    base, case = vu.deformed_edge_case()
    if layout == "compact":
        for f, s in case.shares(rt.K).items():
            print(f"deformed edge scene {f:14s} determined closest {s[0]:.3f} any {s[1]:.3f}")
    env, opts = LAYOUTS[layout]
    ds = _with_env(env, lambda: lib.DeviceScene(hip_ctx, base, **opts))
    try:
        info = ds.info()
        ds.update_vertices(case.scene.positions)
        ds.refit()
        assert ds.update_info()["path"] == 4 and ds.info() == dict(info, build_ms=ds.info()["build_ms"])
        if layout == "compact":
            assert info["bytes"] > 64 * info["nodes"], info      # the compact records are still in use
        else:
            assert info["bytes"] == 64 * info["nodes"], info
        bad = _judge_both_orders(hip_ctx, ds, case, case.truth(rt.K), f"refitted {layout}")
    finally:
        ds.close()
    assert not bad, "\n".join(bad)


def _frames(ctx, ds, cam):
    from mcrt import lib
    fb = lib.FrameBuffer(ctx, W, H)
    try:
        fb.render(ds, cam, frame=0, max_depth=2)
        pt = fb.read(0).copy()
        fb.render(ds, cam, frame=0, max_depth=2, integrator=T.INTEGRATOR_BDPT)
        bd = {"rad": fb.read(0).copy(),
              "nosplat": (fb.read_bdpt("splat").view(np.float32).reshape(H, W, 4)[..., :3] == 0).all(-1)}
        for k in ("camera_vertices", "light_vertices", "camera_counts", "light_counts"):
            bd[k] = fb.read_bdpt(k).copy()
        return pt, bd
    finally:
        fb.close()


def test_same_refitted_tree_under_every_walk(hip_ctx):
    """64-B records, per-ray camera walks and no hints: the same tree in the same visit order, so the
    frames are the default's bit for bit.

    The PT frame: every word.  The BDPT frame: every word of the subpath vertices and counts, and
    every word of the radiance at the pixels no light-tracing splat landed on.  Where splats landed
    the radiance is a sum of float atomics whose order the hardware chooses anew in every run --
    measured on the MI355X: the default against MCRT_QUANT_NODES=0 differed in 29 of 24576 words, by
    one ulp each -- so no two BDPT frames are equal word for word there, with or without a refit;
    those pixels are held to the suite's bound for that order (tests/test_gpu_bdpt.py,
    tests/test_gpu_quant_nodes.py: 4e-6)."""
    from mcrt import lib
    sc = bo.flat_scene("mixed")
    moved = vu.deformed(sc)
    cam = scene_camera("mixed", W, H)

    def run():
        ds = lib.DeviceScene(hip_ctx, sc)
        try:
            ds.update_vertices(moved.positions)
            ds.refit()
            return _frames(hip_ctx, ds, cam), ds.info()
        finally:
            ds.close()

    (pt0, bd0), info0 = run()
    assert info0["bytes"] > 64 * info0["nodes"]
    assert (pt0[..., :3] > 0).mean() > 0.3
    for env in ({"MCRT_QUANT_NODES": "0"}, {"MCRT_CAMERA_PACKETS": "0"}, {"MCRT_SHADOW_HINTS": "0"}):
        (pt, bd), info = _with_env(env, run)
        if "MCRT_QUANT_NODES" in env:
            assert info["bytes"] == 64 * info["nodes"]
        np.testing.assert_array_equal(_u32(pt), _u32(pt0), err_msg=f"PT {env}")
        for k in ("camera_vertices", "light_vertices", "camera_counts", "light_counts", "nosplat"):
            np.testing.assert_array_equal(bd[k], bd0[k], err_msg=f"BDPT {k} {env}")
        quiet = bd0["nosplat"]
        differ = (_u32(bd["rad"]) != _u32(bd0["rad"])).any(-1)
        print(f"BDPT {env}: {int(quiet.sum())} of {quiet.size} pixels without splats, {int(differ.sum())} pixels differ")
        assert quiet.any() and not differ[quiet].any(), f"BDPT {env}"
        np.testing.assert_allclose(bd["rad"][..., :3], bd0["rad"][..., :3], rtol=4e-6, atol=4e-6, err_msg=f"BDPT {env}")


@pytest.fixture(scope="module")
def mixed_pair(hip_ctx):
    """`mixed` deformed (positions and normals): one scene updated and refitted, one created fresh."""
    from mcrt import lib
    sc = bo.flat_scene("mixed")
    moved = vu.deformed(sc, normals=True)
    ds = lib.DeviceScene(hip_ctx, sc)
    fresh = lib.DeviceScene(hip_ctx, moved)
    yield sc, moved, ds, fresh
    ds.close()
    fresh.close()


def test_shading_follows_the_update(hip_ctx, mixed_pair):
    from mcrt import lib
    sc, moved, ds, fresh = mixed_pair
    cam = scene_camera("mixed", W, H)
    fa, fb = lib.FrameBuffer(hip_ctx, W, H), lib.FrameBuffer(hip_ctx, W, H)
    try:
        fa.render_guides(ds, cam)
        before = fa.read_guides(T.GUIDE_NORMAL_PLANE).copy()
        ds.update_vertices(moved.positions, moved.normals)
        ds.refit()
        out = []
        for f, s in ((fa, ds), (fb, fresh)):
            f.render_guides(s, cam)
            out.append((f.read_guides(T.GUIDE_NORMAL_PLANE).copy(), f.read_guides(T.GUIDE_ALBEDO_DEPTH).copy(),
                        f.render_aov(s, cam, T.AOV_ALBEDO)))
        (na, aa, va), (nb, ab, vb) = out
        same = (_u32(aa)[..., 3] == _u32(ab)[..., 3]).reshape(-1)      # equal depth words: see the module docstring
        print(f"shading: primary depth agrees on {same.mean():.5f} of {same.size} pixels")
        assert same.mean() >= 0.999
        for what, x, y in (("normal plane", na, nb), ("albedo / depth", aa, ab), ("albedo AOV", va, vb)):
            eq = (_u32(x) == _u32(y)).reshape(same.size, -1).all(1)
            assert eq[same].all(), f"{what}: {int((~eq[same]).sum())} pixels differ from the fresh scene's"
        assert (_u32(na) != _u32(before)).any(-1).mean() > 0.3           # and the normals did change
    finally:
        fa.close()
        fb.close()


def test_refitted_against_a_fresh_build(hip_ctx, mixed_pair):
    """tests/test_gpu_build.py's criteria for another tree over the same triangles.  Runs after
    test_shading_follows_the_update; updates again all the same, so it stands alone too."""
    from mcrt import lib
    sc, moved, ds, fresh = mixed_pair
    ds.update_vertices(moved.positions, moved.normals)
    ds.refit()
    rays = random_rays(moved, 50000, seed=5)
    ha, hb = ru.trace(ds, rays), ru.trace(fresh, rays)
    same = (ha["shapeid"] == hb["shapeid"]) & (ha["primid"] == hb["primid"])
    print(f"refit vs fresh: same primitive on {same.mean():.6f} of {len(rays)} rays")
    assert same.mean() >= 0.9999, same.mean()
    hit = same & (ha["shapeid"] >= 0)
    assert hit.mean() > 0.3
    np.testing.assert_array_equal(_u32(ha["uvwt"][hit]), _u32(hb["uvwt"][hit]))
    np.testing.assert_array_equal(ru.trace(ds, rays, True), ru.trace(fresh, rays, True))
    cam = scene_camera("mixed", W, H)
    fa, fb = lib.FrameBuffer(hip_ctx, W, H), lib.FrameBuffer(hip_ctx, W, H)
    try:
        fa.render(ds, cam, frame=0, max_depth=2)
        fb.render(fresh, cam, frame=0, max_depth=2)
        eq = (_u32(fa.read(0)) == _u32(fb.read(0))).all(-1)
        print(f"refit vs fresh: frame equal on {eq.mean():.5f} of pixels")
        assert eq.mean() >= 0.999, eq.mean()
    finally:
        fa.close()
        fb.close()


def test_update_and_refit_with_frames_in_flight(hip_ctx):
    """render, update, refit, render with no synchronisation of the caller's in between: the first
    frame is the old vertices', the second the new ones'."""
    import torch
    from mcrt import lib
    sc = bo.flat_scene("mixed")
    moved = vu.deformed(sc)
    cam = scene_camera("mixed", W, H)
    ref, ds = lib.DeviceScene(hip_ctx, sc), lib.DeviceScene(hip_ctx, sc)
    fr, fa = lib.FrameBuffer(hip_ctx, W, H), lib.FrameBuffer(hip_ctx, W, H)
    try:
        fr.render(ref, cam, frame=0, max_depth=3)
        pre = fr.read(0).copy()
        ref.update_vertices(moved.positions)
        ref.refit()
        fr.render(ref, cam, frame=0, max_depth=3)
        post = fr.read(0).copy()
        assert (_u32(pre) != _u32(post)).any(-1).mean() > 0.2
        first = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        fa.set_frames_in_flight(2)
        fa.render(ds, cam, frame=0, max_depth=3)
        fa.copy_device(0, first.data_ptr())          # stream-ordered: no wait
        ds.update_vertices(moved.positions)
        ds.refit()
        fa.render(ds, cam, frame=0, max_depth=3)
        second = fa.read(0).copy()
        hip_ctx.sync()
        np.testing.assert_array_equal(_u32(first.cpu().numpy()), _u32(pre))
        np.testing.assert_array_equal(_u32(second), _u32(post))
    finally:
        for o in (fr, fa, ref, ds):
            o.close()


# --- errors and routes -----------------------------------------------------------------------------

def test_errors_leave_the_scene_untouched(hip_ctx):
    from mcrt import lib
    sc = bo.flat_scene("mixed")
    cam = scene_camera("mixed", W, H)
    nv = len(sc.positions)
    ds = lib.DeviceScene(hip_ctx, sc, build=False)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    try:
        with pytest.raises(lib.MCRTError, match=f"mcrt status {NOT_READY}:"):
            ds.refit()                               # before the first build
        ds.update_vertices(sc.positions)             # vertices may change before a build
        ds.build()
        rec0 = ds.records()
        fb.render(ds, cam, frame=0, max_depth=2)
        img0 = fb.read(0).copy()
        junk = np.full((8, 4), 1e6, np.float32)
        for first, count in ((nv - 7, 8), (nv + 1, 0), (0xffffffff, 2)):
            with pytest.raises(lib.MCRTError, match=f"mcrt status {INVALID_ARG}:.*vertex range"):
                ds.update_vertices(junk, first=first, count=count)
        L = lib.lib()
        assert L.mcrt_scene_update_vertices(ds.h, 1, 0xffffffff, junk.ctypes.data, None) == INVALID_ARG   # first + count wraps
        assert L.mcrt_scene_update_vertices(ds.h, 0, 8, None, None) == INVALID_ARG
        assert L.mcrt_scene_update_vertices_device(ds.h, 0, 8, None, None) == INVALID_ARG
        assert L.mcrt_scene_update_vertices(None, 0, 8, junk.ctypes.data, None) == INVALID_ARG
        assert L.mcrt_scene_update_vertices_device(None, 0, 8, None, None) == INVALID_ARG
        assert L.mcrt_accel_refit(None) == INVALID_ARG
        ds.update_vertices(junk, first=nv, count=0)  # an empty range at the end is inside the array
        ds.refit()
        np.testing.assert_array_equal(_u32(ds.records()), _u32(rec0))
        fb.render(ds, cam, frame=0, max_depth=2)
        np.testing.assert_array_equal(_u32(fb.read(0)), _u32(img0))
    finally:
        fb.close()
        ds.close()


def test_two_level_refit_is_a_rebuild(hip_ctx):
    """The instanced edge scene on its natural two-level path: refit rebuilds (path 3), and the
    walks of the deformed scene pass the truth with K_2L."""
    from mcrt import lib
    sc = rt.instanced_edge_scene()
    case = vu.Case(vu.deformed(sc, 0.25))
    ds = lib.DeviceScene(hip_ctx, sc)
    try:
        assert ds.layout()["two_level"] == 1
        ds.update_vertices(case.scene.positions)
        ds.refit()
        assert ds.update_info()["path"] == 3 and ds.layout()["two_level"] == 1
        want, _ = lib.build_host_records(case.scene)
        np.testing.assert_array_equal(_u32(ds.records()), _u32(want))
        bad = _judge_both_orders(hip_ctx, ds, case, case.truth(rt.K_2L), "two-level refit")
    finally:
        ds.close()
    assert not bad, "\n".join(bad)


def test_flat_update_transforms_keeps_its_rebuild(hip_ctx):
    from mcrt import lib
    sc = bo.flat_scene("mixed")
    ds = lib.DeviceScene(hip_ctx, sc)
    try:
        assert ds.update_info()["path"] == 0
        ds.refit()
        assert ds.update_info()["path"] == 4
        ds.update_transforms(sc.shapes)
        assert ds.update_info()["path"] == 3
        ds.refit()                                   # the new structure's first refit allocates again
        assert ds.update_info()["path"] == 4 and ds.update_info()["ms"] > 0.0
    finally:
        ds.close()
