"""GPU tests of the shape, material and light tables on the table-zoo scene
(mcrt.scenes.scene_table_zoo; its coverage conditions are tests/test_table_zoo_cpu.py): shapes
without a material, a material of another type with a normal map, emitters seen from behind, after
a specular and after a diffuse bounce, a lightID that names a point light, a six-triangle mesh
light under a scaled and rotated transform, unequal choicePdf, a black light, area samples taken
in the plane of the disk light -- and the scene boundary's checks of those tables.

  * whole PT and BDPT frames against the reference's own kernels run live (tests/clref_job.py
    ... table), judged as tests/test_gpu_reference.py and tests/test_gpu_bdpt.py judge theirs;
  * PT frames against the oracle, both samplers, with test_gpu_render.py::test_frame_parity's share;
  * light-count changes on one DeviceScene (7 -> 1 -> 0 -> 7 lights) against scenes created fresh;
  * every rule of the table check through mcrt_scene_create and the update calls: the status first,
    and only then a frame, equal bit for bit to the frame from before the rejected call.

Mutation check (done once by hand on scratch copies; the mutated code is not committed).  The
library was built with each single change -- none can index outside a table -- and this module was
run; the rule mutant ran on the CPU only, so that no wrongly accepted table reached a device:

  mutant                                                  caught by
  `materialId != -1` dropped from the NEE guard            nothing: equivalent in shadePath, whose `isUber`
    (mcrt_kernels.hip, `if (materialId != -1)` around      repeats the test, so the BSDF is 0 either way; no
    the BSDF evaluation)                                   valid table tells the two apart
  the -1 branch never taken (material 0 instead)           test_pt_frames_match_reference, test_pt_frames_match_oracle (both)
  `mat.type == 0` removed from `isUber`                    test_pt_frames_match_reference, test_pt_frames_match_oracle (both)
  emission test `> 0.0f` negated                           test_pt_frames_match_reference, test_pt_frames_match_oracle (both)
  `prevFlags` test inverted                                test_pt_frames_match_reference, test_pt_frames_match_oracle (both)
  `% numTriangles` and the `u.x` remap removed             test_pt_frames_match_reference, test_bdpt_frames_match_reference,
                                                           test_pt_frames_match_oracle (both)
  `light.choicePdf` replaced by `1.0f / numLights`         test_pt_frames_match_reference, test_pt_frames_match_oracle (both)
  `1 / light.area` replaced by the first triangle's area   test_pt_frames_match_reference, test_bdpt_frames_match_reference,
                                                           test_pt_frames_match_oracle (both)
  the texture-id rule removed from check_scene_tables      test_table_zoo_cpu.py::test_check_accepts_the_zoo_and_rejects_each_broken_table,
                                                           test_asan_cpu.py (host_asan's table_checks)
The other two places that test `materialId != -1` (the material fetch in shadePath and
k_bdpt_vertex) cannot be dropped without reading material -1, out of range, on the device; the
"never taken" mutant stands in for them.  `>` turned into `>=` in the emission test is equivalent for
every hit: a ray with gn . wo == 0 runs in the triangle's plane and cannot hit it.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import table_zoo as tz
from clref_job import TABLE_BDPT_CASES, TABLE_CASES, bdpt_key
from mcrt import types as T
from oracle import pyoracle as po
from test_gpu_bdpt import REL_TOL, compare_vertices, our_planes
from test_gpu_render import pixel_agreement

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = tz.W, tz.H
INVALID_ARG = 1   # MCRT_ERROR_INVALID_ARG
TEX_SLOTS = ("uber_normalMapId", "uber_diffuseTexId", "uber_glossyTexId", "uber_specReflectionTexId",
             "uber_transmissionTexId", "uber_opacityTexId", "uber_roughnessTexId", "uber_iorTexId")


def pt_frame(fb, ds, frame, D=tz.DEPTH, sampler=T.SAMPLER_RANDOM):
    fb.render(ds, tz.camera(), frame=frame, max_depth=D, sampler=sampler)
    return fb.read(0).copy()


def bdpt_frames(ctx, ds, D=2, frames=(0, 1)):
    """BDPT frames from a fresh frame buffer (its sampled-light state starts at zero): [(radiance, no-splat mask)]."""
    from mcrt import lib
    fb = lib.FrameBuffer(ctx, W, H)
    out = []
    for f in frames:
        fb.render(ds, tz.camera(), frame=f, max_depth=D, sampler=T.SAMPLER_RANDOM, integrator=T.INTEGRATOR_BDPT)
        g = fb.read(0)[..., :3].copy()
        nosplat = (fb.read_bdpt("splat").view(np.float32).reshape(H, W, 4)[..., :3] == 0).all(-1)
        out.append((g, nosplat))
    fb.close()
    return out


def bdpt_differences(got, ref, nosplat, label):
    """Splat-order criterion of tests/test_gpu_bdpt.py: bit-exact where no splat landed, within REL_TOL elsewhere."""
    exact = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    close = (np.abs(got - ref) <= REL_TOL * (np.abs(got) + np.abs(ref)) + 1e-30) | exact
    bad = []
    if not exact.all(-1)[nosplat].all():
        bad.append(f"{label}: {int((~exact.all(-1)[nosplat]).sum())} no-splat pixels outside bit-exactness")
    if not close.all():
        bad.append(f"{label}: {int((~close).sum())} values outside tolerance")
    return bad


# ---------------------------------------------------------------------------
# frames against the reference's kernels, live
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clref_table(tmp_path_factory):
    if not po.clref_available():
        pytest.skip("oracle/_ref/clref_runner.so not built")
    out = str(tmp_path_factory.mktemp("clref") / "clref_table.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "clref_job.py"), out, "ieee", "table"],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.fail("reference table-zoo job failed:\n" + r.stdout + r.stderr)
    return np.load(out, allow_pickle=False)


@pytest.mark.parametrize("case", TABLE_CASES, ids=[f"{c[0]}_d{c[4]}" for c in TABLE_CASES])
def test_pt_frames_match_reference(hip_ctx, clref_table, case):
    """Radiance bit for bit PathTracing.cl's, no tolerance."""
    from mcrt import lib
    name, w, h, frames, D = case
    assert (w, h, D) == (W, H, tz.DEPTH)
    ds = lib.DeviceScene(hip_ctx, tz.zoo())
    fb = lib.FrameBuffer(hip_ctx, W, H)
    try:
        for f in frames:
            g = pt_frame(fb, ds, f, D)
            ref = clref_table[f"{name}_{w}x{h}_d{D}_f{f}"]
            diff = (g[..., :3].view(np.uint32) != ref[..., :3].view(np.uint32)).any(-1)
            assert not diff.any(), (name, D, f, int(diff.sum()), np.argwhere(diff)[:8].tolist())
            assert np.isfinite(g).all() and g[..., :3].max() > 0
    finally:
        fb.close()
        ds.close()


@pytest.mark.parametrize("case", TABLE_BDPT_CASES, ids=[bdpt_key(c) for c in TABLE_BDPT_CASES])
def test_bdpt_frames_match_reference(hip_ctx, clref_table, case):
    """Vertex records and counts bit-exact, radiance bit-exact where no splat landed, within
    test_gpu_bdpt.py's REL_TOL elsewhere."""
    from mcrt import lib
    name, w, h, frames, D = case
    key = bdpt_key(case)
    N = w * h
    ds = lib.DeviceScene(hip_ctx, tz.zoo())
    fb = lib.FrameBuffer(hip_ctx, w, h)
    bad = []
    for f in frames:
        fb.render(ds, tz.camera(), frame=f, max_depth=D, sampler=T.SAMPLER_RANDOM, integrator=T.INTEGRATOR_BDPT)
        g = fb.read(0)[..., :3].copy()
        nosplat = (fb.read_bdpt("splat").view(np.float32).reshape(h, w, 4)[..., :3] == 0).all(-1)
        ref = np.ascontiguousarray(clref_table[f"{key}_f{f}"][..., :3])
        print(f"frame {f}: {int(nosplat.sum())} no-splat pixels, mean {np.nanmean(g):.6f} vs {np.nanmean(ref):.6f}")
        bad += bdpt_differences(g, ref, nosplat, f"frame {f}")
    cc = fb.read_bdpt("camera_counts").view(np.int32)
    lc = fb.read_bdpt("light_counts").view(np.int32)
    rcc = clref_table[f"{key}_camera_counts"].view(np.int32)
    rlc = clref_table[f"{key}_light_counts"].view(np.int32)
    if (cc != rcc).any():
        bad.append(f"camera counts differ at {int((cc != rcc).sum())} pixels")
    if (lc != rlc).any():
        bad.append(f"light counts differ at {int((lc != rlc).sum())} pixels")
    bad += compare_vertices(our_planes(fb.read_bdpt("camera_vertices"), D + 2, N),
                            clref_table[f"{key}_camera_vertices"].view(po.REF_VERTEX_DTYPE).reshape(N, D + 2),
                            cc, D + 2, N, "camera")
    bad += compare_vertices(our_planes(fb.read_bdpt("light_vertices"), D + 1, N),
                            clref_table[f"{key}_light_vertices"].view(po.REF_VERTEX_DTYPE).reshape(N, D + 1),
                            lc, D + 1, N, "light")
    fb.close()
    ds.close()
    assert not bad, bad


# ---------------------------------------------------------------------------
# frames against the oracle (no oracle/_ref needed)
# ---------------------------------------------------------------------------
ORACLE_AGREEMENT = 0.995


@pytest.mark.parametrize("sampler", [T.SAMPLER_RANDOM, T.SAMPLER_SOBOL], ids=["random", "sobol"])
def test_pt_frames_match_oracle(hip_ctx, sampler):
    """tests/test_gpu_render.py::test_frame_parity's criterion and share (0.995) at depth 3.  The
    ORACLE against the REFERENCE's kernels run live on this scene (never the product; both sampler
    builds) agrees on 0.99609 (frame 0) and 0.99707 (frame 1) of the pixels with the random sampler
    and on 0.99609 and 0.99674 with Sobol, so test_frame_parity's share holds for the frames compared."""
    from mcrt import lib
    o = po.OracleScene(tz.zoo())
    o.build()
    ds = lib.DeviceScene(hip_ctx, tz.zoo())
    fb = lib.FrameBuffer(hip_ctx, W, H)
    try:
        for frame in tz.FRAMES:
            g = pt_frame(fb, ds, frame, sampler=sampler)
            r, _ = o.render(tz.camera(), frame=frame, max_depth=tz.DEPTH, sampler=sampler)
            assert np.isfinite(g).all()
            frac = pixel_agreement(g, r)
            print(f"sampler {sampler} frame {frame}: pixel agreement {frac:.5f}")
            assert frac >= ORACLE_AGREEMENT, (frame, frac)
            np.testing.assert_allclose(g[..., :3].mean((0, 1)), r[..., :3].mean((0, 1)), rtol=2e-2)
    finally:
        fb.close()
        ds.close()


# ---------------------------------------------------------------------------
# light-count changes on one scene
# ---------------------------------------------------------------------------
def with_tables(sc, shapes, lights):
    from mcrt.scenes import Scene
    return Scene(shapes, sc.indices, sc.positions, sc.uvs, sc.normals, sc.tangents, sc.binormals, sc.colors,
                 sc.textures, sc.tex_data, lights, sc.materials, sobol=sc.sobol, name=sc.name)


def test_light_count_changes_equal_fresh_scenes(hip_ctx):
    """7 lights -> emitter 1 alone -> none -> 7 again on one DeviceScene; after each step PT and
    BDPT frames equal those of a scene created with the step's tables.  Without lights both
    integrators return MCRT_OK and zeros."""
    from mcrt import lib
    sc = tz.zoo()
    e1 = sc.zoo["shapes"]["emitter1"]
    one = sc.lights[sc.shapes["lightID"][e1]:][:1].copy()
    one["choicePdf"] = 1.0
    sh_one = sc.shapes.copy()
    sh_one["lightID"] = -1
    sh_one["lightID"][e1] = 0
    sh_none = sc.shapes.copy()
    sh_none["lightID"] = -1
    ds = lib.DeviceScene(hip_ctx, sc)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    steps = (("one light", [("shapes", sh_one), ("lights", one)], sh_one, one),       # ids first: legal in both tables
             ("no lights", [("shapes", sh_none), ("lights", sc.lights[:0].copy())], sh_none, sc.lights[:0].copy()),
             ("all lights", [("lights", sc.lights), ("shapes", sc.shapes)], sc.shapes, sc.lights))
    try:
        for label, updates, shapes, lights in steps:
            for kind, arr in updates:
                getattr(ds, "update_" + kind)(arr)
            fresh = lib.DeviceScene(hip_ctx, with_tables(sc, shapes, lights))
            fb2 = lib.FrameBuffer(hip_ctx, W, H)
            for f in tz.FRAMES:
                a, b = pt_frame(fb, ds, f), pt_frame(fb2, fresh, f)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label, f)
                assert np.isfinite(a).all() and (a[..., :3].any() == (len(lights) > 0)), (label, f)
            fb2.close()
            bad = []
            for f, ((a, ns), (b, _)) in enumerate(zip(bdpt_frames(hip_ctx, ds), bdpt_frames(hip_ctx, fresh))):
                bad += bdpt_differences(a, b, ns, f"{label} BDPT frame {f}")
                assert a.any() == (len(lights) > 0), (label, f)
            fresh.close()
            assert not bad, bad
    finally:
        fb.close()
        ds.close()


# ---------------------------------------------------------------------------
# rejections through the real boundary
# ---------------------------------------------------------------------------
def broken_tables(sc):
    """(label, shapes, materials, lights) per rule and side: the first rejected value below and above."""
    S = sc.zoo["shapes"]
    out = []
    for field, n in (("materialId", len(sc.materials)), ("lightID", len(sc.lights))):
        for v in (-2, n):
            sh = sc.shapes.copy()
            sh[field][S["glossy"]] = v
            out.append((f"{field}={v}", sh, sc.materials, sc.lights))
    for k in TEX_SLOTS:
        for v in (-2, len(sc.textures)):
            m = sc.materials.copy()
            m[k][sc.zoo["materials"]["type1"]] = v    # a material of another type: checked all the same
            out.append((f"{k}={v}", sc.shapes, m, sc.lights))
    for v in (-1, len(sc.shapes)):
        L = sc.lights.copy()
        L["shapeId"][sc.shapes["lightID"][S["emitter1"]]] = v
        out.append((f"mesh light shapeId={v}", sc.shapes, sc.materials, L))
    return out


def test_scene_create_rejects_every_rule(hip_ctx):
    """mcrt_scene_create through ctypes: MCRT_ERROR_INVALID_ARG, no scene handle, a message that
    names the entry.  Nothing is rendered with a rejected table."""
    from mcrt import lib
    sc = tz.zoo()
    for label, shapes, mats, lights in broken_tables(sc):
        bad = with_tables(sc, shapes, lights)
        bad.materials = mats
        desc = bad.desc()
        h = ctypes.c_void_p()
        st = lib.lib().mcrt_scene_create(hip_ctx.h, ctypes.byref(desc), ctypes.byref(h))
        assert st == INVALID_ARG and not h.value, (label, st)
        msg = lib.lib().mcrt_last_error(hip_ctx.h).decode()
        assert any(w in msg for w in ("shape ", "material ", "mesh light ")), (label, msg)
    # a moved startVertex one past the end
    sh = sc.shapes.copy()
    sh["startVertex"][int(np.argmax(sh["startVertex"]))] += 1
    desc = with_tables(sc, sh, sc.lights).desc()
    h = ctypes.c_void_p()
    assert lib.lib().mcrt_scene_create(hip_ctx.h, ctypes.byref(desc), ctypes.byref(h)) == INVALID_ARG and not h.value


def test_rejected_updates_leave_the_scene_as_it_was(hip_ctx):
    """Every rejected update raises (status first); only then a frame is rendered, and it equals the
    frame from before the call bit for bit.  The legal neighbours of the counts are accepted."""
    from mcrt import lib
    sc = tz.zoo()
    S = sc.zoo["shapes"]
    ds = lib.DeviceScene(hip_ctx, sc)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    try:
        before = pt_frame(fb, ds, 0)
        before_bdpt = bdpt_frames(hip_ctx, ds, frames=(0,))[0][0]
        calls = []
        for label, shapes, mats, lights in broken_tables(sc):
            if shapes is not sc.shapes:
                calls.append((label + " (update_shapes)", ds.update_shapes, (shapes,)))
                calls.append((label + " (update_transforms)", ds.update_transforms, (shapes,)))
            elif mats is not sc.materials:
                calls.append((label, ds.update_materials, (mats,)))
            else:
                calls.append((label, ds.update_lights, (lights,)))
        # counts that drop below an id a shape still holds; n = 0 materials while shapes name one
        calls.append(("5 lights", ds.update_lights, (sc.lights[:5],)))   # emitter 3 holds light 5
        calls.append(("0 lights", ds.update_lights, (sc.lights[:0],)))
        calls.append(("0 materials", ds.update_materials, (sc.materials[:0],)))
        calls.append((f"{len(sc.materials) - 1} materials", ds.update_materials, (sc.materials[:-1],)))
        moved = sc.shapes.copy()
        moved["startVertex"][int(np.argmax(moved["startVertex"]))] += 1
        calls.append(("startVertex one past the end (update_shapes)", ds.update_shapes, (moved,)))
        calls.append(("startVertex one past the end (update_transforms)", ds.update_transforms, (moved,)))
        for label, fn, args in calls:
            with pytest.raises(lib.MCRTError, match=f"status {INVALID_ARG}:"):
                fn(*args)
            after = pt_frame(fb, ds, 0)
            assert np.array_equal(before.view(np.uint32), after.view(np.uint32)), label
        after_bdpt, ns = bdpt_frames(hip_ctx, ds, frames=(0,))[0]
        assert not bdpt_differences(after_bdpt, before_bdpt, ns, "BDPT after the rejected updates")
        # the last accepted values pass: ids -1 and n - 1 through the shape update, and back
        ok = sc.shapes.copy()
        ok["materialId"][S["glossy"]] = len(sc.materials) - 1
        ok["lightID"][S["glossy"]] = -1
        ds.update_shapes(ok)
        ds.update_shapes(sc.shapes)
        ds.update_lights(sc.lights)
        ds.update_materials(sc.materials)
        after = pt_frame(fb, ds, 0)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    finally:
        fb.close()
        ds.close()
