"""The scene tables (mcrt_scene.hip), the ray queries (mcrt_query.hip) and mcrt_render_aov
(mcrt_aov.hip): what each entry point returns when it refuses, in the order it checks, and the
surface records two shapes of one mesh share.  The tests were written against the code while it
still lived in mcrt_capi.cpp and mcrt_kernels.hip and quote its messages; they use the `mixed`
scene and a small scene of their own at 96x64 and 24x40 (whole 8x8 tiles)."""
import ctypes

import numpy as np
import pytest

from clref_job import build_scene
from helpers import refused
from mcrt import scenes
from mcrt import types as T
from mcrt.camera import make_camera, scene_camera

pytestmark = pytest.mark.gpu
INVALID_ARG, NOT_READY = 1, 4
NAME, W, H = "mixed", 96, 64
NOT_BUILT = "mcrt_accel_build has not been called"


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _call(fn, *args, ctx=None):
    from mcrt import lib
    lib._check(fn(*args), ctx.h if ctx else None)


def _frame(hip_ctx, ds, w=W, h=H, cam=None):
    """One PT frame of depth 2."""
    from mcrt import lib
    fb = lib.FrameBuffer(hip_ctx, w, h)
    try:
        fb.render(ds, scene_camera(NAME, w, h) if cam is None else cam, frame=0, max_depth=2)
        hip_ctx.sync()
        return fb.read(0)
    finally:
        fb.close()


@pytest.fixture(scope="module")
def mixed():
    return build_scene(NAME)


@pytest.fixture(scope="module")
def scene(hip_ctx, mixed):
    from mcrt import lib
    ds = lib.DeviceScene(hip_ctx, mixed)
    yield ds
    ds.close()


def test_scene_refusals(hip_ctx, mixed, scene):
    """Status code and message of every refusal of the scene's entry points, in the order each
    checks: NULL arguments, a scene without shapes, the four required arrays, a counted table that
    is NULL, a texture outside the texel buffer (width 0; one byte past the end), then the update
    calls.  Without a scene there is no context to hold the message.  A refused update leaves the
    scene as it was: it renders the frame it rendered before, word for word."""
    from mcrt import lib
    L = lib.lib()
    sc = mixed
    before = _frame(hip_ctx, scene)
    assert np.isfinite(before).all() and before[..., :3].max() > 0

    out = ctypes.c_void_p()

    def create(ctx=hip_ctx, desc=True, handle=True, **over):
        d = sc.desc()
        for k, v in over.items():
            setattr(d, k, v)
        _call(L.mcrt_scene_create, ctx.h if ctx else None, ctypes.byref(d) if desc else None,
              ctypes.byref(out) if handle else None, ctx=ctx)

    # NULL arguments: one message
    refused(lambda: create(ctx=None), INVALID_ARG, "NULL argument")
    refused(lambda: create(desc=False), INVALID_ARG, "NULL argument")
    refused(lambda: create(handle=False), INVALID_ARG, "NULL argument")
    # no shapes, before the arrays are looked at
    empty = "scene has no shapes"
    refused(lambda: create(num_shapes=0), INVALID_ARG, empty)
    refused(lambda: create(shapes=None), INVALID_ARG, empty)
    refused(lambda: create(shapes=None, indices=None), INVALID_ARG, empty)
    # the four arrays every scene has (tangents, binormals and colours are not read)
    for field in ("indices", "positions", "uvs", "normals"):
        refused(lambda: create(**{field: None}), INVALID_ARG, "indices/positions/uvs/normals are required")
    # a table that has a count and no entries, before the entries are checked
    for field in ("materials", "lights", "textures"):
        assert getattr(sc.desc(), "num_" + field) > 0
        refused(lambda: create(**{field: None}), INVALID_ARG, "a table with a non-zero count is NULL")
    refused(lambda: create(normals=None, lights=None), INVALID_ARG, "indices/positions/uvs/normals are required")
    # textures: a width or height of 0, and level 0 ending one byte past the texel buffer
    tex = sc.textures.copy()
    assert len(tex) == 4 and (tex["numMipLevels"] == 1).all()
    ends = tex["memOffset"].astype(np.int64) + 4 * tex["width"].astype(np.int64) * tex["height"]
    assert ends.max() == sc.tex_data.nbytes and int(ends.argmax()) == 3   # the last texture ends the buffer
    tex["width"][1] = 0
    refused(lambda: create(textures=T.ptr(tex)), INVALID_ARG, "texture 1 is out of the texel buffer")
    tex = sc.textures.copy()
    tex["height"][2] = 0
    refused(lambda: create(textures=T.ptr(tex)), INVALID_ARG, "texture 2 is out of the texel buffer")
    refused(lambda: create(tex_data_bytes=sc.tex_data.nbytes - 1), INVALID_ARG, "texture 3 is out of the texel buffer")
    assert out.value is None
    assert L.mcrt_scene_destroy(None) == 0   # destroying nothing is not an error

    # the updates; a NULL scene leaves the message with the thread
    lights, mats, shapes = sc.lights.copy(), sc.materials.copy(), sc.shapes.copy()
    n = len(shapes)
    refused(lambda: _call(L.mcrt_scene_update_lights, None, lib._p(lights), len(lights)), INVALID_ARG, "invalid lights")
    refused(lambda: _call(L.mcrt_scene_update_lights, scene.h, None, 1, ctx=hip_ctx), INVALID_ARG, "invalid lights")
    refused(lambda: _call(L.mcrt_scene_update_materials, None, lib._p(mats), len(mats)), INVALID_ARG,
            "invalid materials")
    refused(lambda: _call(L.mcrt_scene_update_materials, scene.h, None, 1, ctx=hip_ctx), INVALID_ARG,
            "invalid materials")
    count = "shape count must not change"
    refused(lambda: _call(L.mcrt_scene_update_shapes, None, lib._p(shapes), n), INVALID_ARG, count)
    refused(lambda: _call(L.mcrt_scene_update_shapes, scene.h, None, n, ctx=hip_ctx), INVALID_ARG, count)
    refused(lambda: _call(L.mcrt_scene_update_shapes, scene.h, lib._p(shapes), n - 1, ctx=hip_ctx), INVALID_ARG, count)
    refused(lambda: _call(L.mcrt_scene_update_shapes, scene.h, lib._p(shapes), n + 1, ctx=hip_ctx), INVALID_ARG, count)
    topology = "shape topology must not change"
    moved = shapes.copy()
    moved["startIdx"][n - 1] += 3
    refused(lambda: scene.update_shapes(moved), INVALID_ARG, topology)
    moved = shapes.copy()
    moved["numTriangles"][0] -= 1
    refused(lambda: scene.update_shapes(moved), INVALID_ARG, topology)
    moved["materialId"][0] = len(mats)   # two faults: the topology is looked at first
    refused(lambda: scene.update_shapes(moved), INVALID_ARG, topology)
    # the vertex updates: the scene, the positions, then the range
    nv = len(sc.positions)
    pos = np.ascontiguousarray(sc.positions[:4], np.float32)
    for fn in (L.mcrt_scene_update_vertices, L.mcrt_scene_update_vertices_device):
        refused(lambda: _call(fn, None, 0, 4, lib._p(pos), None), INVALID_ARG, "scene is NULL")
        refused(lambda: _call(fn, scene.h, 0, 4, None, None, ctx=hip_ctx), INVALID_ARG, "positions is NULL")
        refused(lambda: _call(fn, scene.h, nv + 1, 0, None, None, ctx=hip_ctx), INVALID_ARG, "positions is NULL")
        refused(lambda: _call(fn, scene.h, nv - 3, 4, lib._p(pos), None, ctx=hip_ctx), INVALID_ARG,
                f"vertex range [{nv - 3}, {nv + 1}) is outside the scene's {nv} vertices")
        refused(lambda: _call(fn, scene.h, nv + 1, 0, lib._p(pos), None, ctx=hip_ctx), INVALID_ARG,
                f"vertex range [{nv + 1}, {nv + 1}) is outside the scene's {nv} vertices")
        refused(lambda: _call(fn, scene.h, 0xffffffff, 0xffffffff, lib._p(pos), None, ctx=hip_ctx), INVALID_ARG,
                f"vertex range [4294967295, 8589934590) is outside the scene's {nv} vertices")
        _call(fn, scene.h, nv, 0, lib._p(pos), None, ctx=hip_ctx)   # an empty range at the end is a no-op
    refused(lambda: _call(L.mcrt_scene_motion_snapshot, None), INVALID_ARG, "scene is NULL")

    # nothing was touched
    hip_ctx.sync()
    np.testing.assert_array_equal(_words(_frame(hip_ctx, scene)), _words(before))
    # ... and the good calls work: the same tables again give the same frame
    scene.update_lights(lights)
    scene.update_materials(mats)
    scene.update_shapes(shapes)
    scene.motion_snapshot()
    np.testing.assert_array_equal(_words(_frame(hip_ctx, scene)), _words(before))


def test_query_and_event_refusals(hip_ctx, mixed):
    """The refusals of the ray queries that test_gpu_trace.py::test_empty_query_and_errors leaves out:
    the counted queries without a count, the event calls without an event, and every query before a
    build -- which is looked at before the ray arguments, and after the done event was cleared."""
    import torch
    from mcrt import lib
    L = lib.lib()
    ds = lib.DeviceScene(hip_ctx, mixed, build=False)
    try:
        rays = torch.zeros(64 * T.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        hits = torch.zeros(64 * T.ISECT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        count = torch.full((1,), 64, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r, h, c = rays.data_ptr(), hits.data_ptr(), count.data_ptr()
        for fn in (L.mcrt_trace_closest_count, L.mcrt_trace_any_count):
            ev = ctypes.c_void_p(0x1234)
            refused(lambda: _call(fn, ds.h, r, None, 64, h, None, ctypes.byref(ev), ctx=hip_ctx), INVALID_ARG,
                    "d_numrays is NULL")
            assert ev.value == 0x1234   # refused before the event is touched
            refused(lambda: _call(fn, None, r, None, 64, h, None, None), INVALID_ARG, "d_numrays is NULL")
            refused(lambda: _call(fn, None, r, c, 64, h, None, ctypes.byref(ev)), INVALID_ARG, "scene is NULL")
            assert ev.value is None     # the done event is cleared first
            ev = ctypes.c_void_p(0x1234)
            refused(lambda: _call(fn, ds.h, r, c, 64, h, None, ctypes.byref(ev), ctx=hip_ctx), NOT_READY, NOT_BUILT)
            assert ev.value is None
            refused(lambda: _call(fn, ds.h, None, c, -1, None, None, None, ctx=hip_ctx), NOT_READY, NOT_BUILT)
        for fn in (L.mcrt_trace_closest, L.mcrt_trace_any):
            refused(lambda: _call(fn, None, r, 64, h), INVALID_ARG, "scene is NULL")
            refused(lambda: _call(fn, ds.h, r, 64, h, ctx=hip_ctx), NOT_READY, NOT_BUILT)
            refused(lambda: _call(fn, ds.h, r, 0, h, ctx=hip_ctx), NOT_READY, NOT_BUILT)
            refused(lambda: _call(fn, ds.h, None, -1, None, ctx=hip_ctx), NOT_READY, NOT_BUILT)   # two faults
        refused(lambda: lib.event_wait(None), INVALID_ARG, "event is NULL")
        assert L.mcrt_event_destroy(None) == 0   # destroying nothing is not an error
        # once built: the ray arguments, and a counted query's event works
        ds.build()
        bad = "invalid ray query arguments"
        refused(lambda: ds.trace_closest(r, -1, h), INVALID_ARG, bad)
        refused(lambda: ds.trace_closest(None, 64, h), INVALID_ARG, bad)
        refused(lambda: ds.trace_closest(r, 64, None), INVALID_ARG, bad)
        refused(lambda: ds.trace_any(r, 64, None), INVALID_ARG, bad)
        ev = ds.trace_count(False, r, c, 64, h, want_event=True)   # 64 inactive rays: nothing is written
        assert ev
        lib.event_wait(ev)
        lib.event_destroy(ev)
        hip_ctx.sync()
        assert not hits.cpu().numpy().any()
    finally:
        ds.close()


def test_render_aov_refusals(hip_ctx, mixed, scene):
    """mcrt_render_aov: NULL arguments, then the structure, then the aov, then the camera's size.
    After the refusals the albedo is the one from before, word for word."""
    from mcrt import lib
    L = lib.lib()
    w, h = 24, 40
    fb = lib.FrameBuffer(hip_ctx, w, h)
    unbuilt = lib.DeviceScene(hip_ctx, mixed, build=False)
    try:
        cam = np.ascontiguousarray(scene_camera(NAME, w, h))
        p = T.FrameParams(0, 1, T.SAMPLER_RANDOM, 0, 3, 8, 1, 0, T.INTEGRATOR_PT, 0)
        out = np.zeros((h, w, 4), np.float32)
        before = fb.render_aov(scene, cam)
        assert before[..., :3].max() > 0

        def aov(s=scene.h, f=fb.h, c=lib._p(cam), pp=ctypes.byref(p), which=T.AOV_ALBEDO, o=lib._p(out), ctx=hip_ctx):
            _call(L.mcrt_render_aov, s, f, c, pp, which, o, ctx=ctx)

        refused(lambda: aov(s=None, ctx=None), INVALID_ARG, "NULL argument")
        for missing in ("f", "c", "pp", "o"):
            refused(lambda: aov(**{missing: None}), INVALID_ARG, "NULL argument")
        refused(lambda: aov(o=None, which=7), INVALID_ARG, "NULL argument")        # two faults
        refused(lambda: aov(s=unbuilt.h), NOT_READY, NOT_BUILT)
        refused(lambda: aov(s=unbuilt.h, which=7), NOT_READY, NOT_BUILT)           # two faults
        for which in (-1, 2, 7):
            refused(lambda: aov(which=which), INVALID_ARG, "unknown aov")
        wide = np.ascontiguousarray(scene_camera(NAME, W, H))
        refused(lambda: aov(c=lib._p(wide)), INVALID_ARG, "camera size differs from the frame buffer")
        refused(lambda: aov(c=lib._p(wide), which=7), INVALID_ARG, "unknown aov")  # two faults
        bands = T.FrameParams(0, 1, T.SAMPLER_RANDOM, 0, 3, 12, 2, 0, T.INTEGRATOR_PT, 0)
        refused(lambda: aov(pp=ctypes.byref(bands)), INVALID_ARG, "band_rows must be a positive multiple of 8")
        assert not out.any()   # nothing was written
        np.testing.assert_array_equal(_words(fb.render_aov(scene, cam)), _words(before))
        lod = fb.render_aov(scene, cam, aov=T.AOV_TEXTURE_LOD)
        assert lod.shape == (h, w, 3, 4) and np.isfinite(lod).all()
    finally:
        unbuilt.close()
        fb.close()


def _shared_mesh_scene(shared):
    """A floor, a textured sphere, a box between, and the sphere again under another transform:
    as a second shape of the same mesh (`shared`) or with its vertices and indices stored twice.
    The same shapes in the same order either way, so the same world triangles."""
    rng = np.random.default_rng(scenes.SEED_BASE + 77)
    b = scenes.SceneBuilder("shared" if shared else "duplicated")
    checker = b.add_texture(scenes.tex_checker(32, (230, 230, 230), (40, 90, 160)))
    floor = b.add_material(kd=(0.7, 0.7, 0.7), ks=(0, 0, 0))
    ball = b.add_material(kd=(1, 1, 1), ks=(0.2, 0.2, 0.2), roughness=0.3, diffuseTexId=checker)
    other = b.add_material(kd=(0.6, 0.3, 0.2), ks=(0.3, 0.3, 0.3), roughness=0.2)
    b.add_mesh(*scenes.grid((-6, 0, -6), (12, 0, 0), (0, 0, 12), 3, 3, flip=True), floor)
    sphere = scenes.displaced_sphere(np.zeros(3), 1.0, 20, 10, rng, amp=0.1)
    first = b.add_mesh(*sphere, ball, transform=scenes._affine(1.0, 20.0, (-1.8, 1.0, 0.0)))
    b.add_mesh(*scenes.box((-0.5, 0.0, -0.5), (0.5, 1.2, 0.5), n=2), other)
    again = scenes._affine(0.7, -50.0, (1.9, 0.8, 0.6), 25.0)
    if shared:
        b.add_instance(first, again, material=other)
    else:
        b.add_mesh(*sphere, other, transform=again)
    b.add_directional_light(scenes.euler_forward(50.0, 30.0), (4.0, 4.0, 4.0))
    b.add_point_light((0.0, 4.0, -3.0), (8.0, 8.0, 8.0))
    return b.build()


@pytest.mark.parametrize("w,h", [(W, H), (24, 40)])
def test_shared_surface_records(hip_ctx, w, h):
    """Two shapes of one mesh share one range of surface records (mcrt_scene_create) and a vertex
    update rewrites it once, in place (mcrt_scene_update_vertices).  A PT frame of depth 2 over a
    flat structure is bit-identical to the frame of the same scene with the mesh stored twice, before
    and after the mesh's vertices move."""
    from mcrt import lib
    a, d = _shared_mesh_scene(True), _shared_mesh_scene(False)
    key = lambda s: [tuple(int(s.shapes[f][i]) for f in ("startIdx", "startVertex", "numTriangles")) for i in range(4)]  # noqa: E731
    assert key(a)[1] == key(a)[3] and len(set(key(a))) == 3 and len(set(key(d))) == 4
    np.testing.assert_array_equal(_words(a.world_triangles()), _words(d.world_triangles()))
    cam = make_camera((0.5, 2.6, -6.5), (0.0, 0.8, 0.0), w, h)
    dsa = lib.DeviceScene(hip_ctx, a, force_flat=True)
    dsd = lib.DeviceScene(hip_ctx, d, force_flat=True)
    try:
        assert dsa.layout()["two_level"] == 0 and dsd.layout()["two_level"] == 0
        np.testing.assert_array_equal(_words(dsa.records()), _words(dsd.records()))
        fa, fd = _frame(hip_ctx, dsa, w, h, cam), _frame(hip_ctx, dsd, w, h, cam)
        assert np.isfinite(fa).all() and (fa[..., :3].max(-1) > 0).mean() > 0.5
        np.testing.assert_array_equal(_words(fa), _words(fd))
        # the shared mesh's vertices move: once in the shared scene, both copies in the other
        sa, sd = a.shapes[1], d.shapes[3]
        nv = int(a.shapes[2]["startVertex"] - sa["startVertex"])
        pos = a.positions[sa["startVertex"]: sa["startVertex"] + nv].copy()
        pos[:, :3] *= np.float32(1.25)
        dsa.update_vertices(pos, first=int(sa["startVertex"]))
        dsd.update_vertices(pos, first=int(d.shapes[1]["startVertex"]))
        dsd.update_vertices(pos, first=int(sd["startVertex"]))
        dsa.build(force_flat=True)
        dsd.build(force_flat=True)
        np.testing.assert_array_equal(_words(dsa.records()), _words(dsd.records()))
        ma, md = _frame(hip_ctx, dsa, w, h, cam), _frame(hip_ctx, dsd, w, h, cam)
        np.testing.assert_array_equal(_words(ma), _words(md))
        assert not np.array_equal(_words(ma), _words(fa))   # the move is seen
    finally:
        dsa.close()
        dsd.close()
