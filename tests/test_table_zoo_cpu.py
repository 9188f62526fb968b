"""The table-zoo scene (mcrt.scenes.scene_table_zoo) on the CPU: its tables hold only values the
reference's kernels guard, the oracle's path log of the frames the GPU suite compares (96 x 64,
depth 3, frames 0 and 1) reaches every rare branch of the shape, material and light tables often
enough, a light-less copy renders to zeros, and the scene-table check of the host layer
(check_scene_tables, called by the stand-alone sanitizer program tests/asan/host_asan) accepts the
project's scenes and rejects each broken table with the rule that names it.  Run with -s for the
measured counts."""
import os
import struct
import subprocess
import zipfile

import numpy as np
import pytest

import table_zoo as tz
from clref_job import build_scene
from mcrt import scenes
from mcrt import types as T
from oracle import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
TEX_SLOTS = ("uber_normalMapId", "uber_diffuseTexId", "uber_glossyTexId", "uber_specReflectionTexId",
             "uber_transmissionTexId", "uber_opacityTexId", "uber_roughnessTexId", "uber_iorTexId")
# mcrt::TableRule (mcrt_internal.h)
OK, INDEX_RANGE, VERTEX_INDEX, MATERIAL_ID, LIGHT_ID, TEXTURE_ID, MESH_LIGHT = range(7)


@pytest.fixture(scope="module")
def counts():
    sc = tz.zoo()
    o = po.OracleScene(sc)
    o.build()
    frames, logs = tz.oracle_logs(o)
    c = tz.path_counts(sc, logs)
    print("\n" + tz.format_counts(c))
    return sc, c, frames


def test_tables_hold_guarded_values_only():
    sc = tz.zoo()
    for ids, n in ((sc.shapes["materialId"], len(sc.materials)), (sc.shapes["lightID"], len(sc.lights))):
        assert ((ids >= -1) & (ids < n)).all()
    for k in TEX_SLOTS:
        assert ((sc.materials[k] >= -1) & (sc.materials[k] < len(sc.textures))).all(), k
    assert len(sc.lights) >= 1 and np.isin(sc.lights["type"], (0, 1, 2, 3)).all()
    assert set(int(t) for t in sc.lights["type"]) == {0, 1, 2, 3}
    pdf = sc.lights["choicePdf"].astype(np.float64)
    assert len(np.unique(pdf)) == len(pdf) and abs(pdf.sum() - 1.0) < 1e-6
    assert (np.abs(pdf - 1.0 / len(pdf)) > 1e-3).all()
    assert sum(1 for L in sc.lights if not L["intensity"][:3].any()) == 1
    S = sc.zoo["shapes"]
    sh = sc.shapes
    assert sh["materialId"][S["no_material"]] == -1 and sh["lightID"][S["no_material"]] == -1
    assert sh["materialId"][S["emitter3"]] == -1 and sh["lightID"][S["emitter3"]] >= 0
    m = sc.materials[sh["materialId"][S["type1"]]]
    assert m["type"] == 1 and m["uber_normalMapId"] >= 0
    assert sc.lights["type"][sh["lightID"][S["point_light_id"]]] == T.POINT
    mirror, glass = (sc.materials[sh["materialId"][S[k]]] for k in ("mirror", "glass"))
    assert mirror["uber_kr"][:3].all() and not (mirror["uber_kd"][:3].any() or mirror["uber_ks"][:3].any()
                                                 or mirror["uber_kt"][:3].any())
    assert glass["uber_kt"][:3].all() and glass["uber_kt"][3] < 0.5


def test_emitter1_mesh_and_area():
    """At least 6 triangles of clearly unequal area under a non-uniform scale and a rotation; the
    shape's and the light's area are the world-space sum (MeshRenderer::computeSurfaceArea)."""
    sc = tz.zoo()
    e1 = sc.zoo["shapes"]["emitter1"]
    t = tz.world_triangles(sc, e1)
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    assert len(t) >= 6 and area.max() > 2.0 * area.min()
    assert np.abs(np.diff(np.sort(area))).min() > 0.02 * area.mean()
    M = sc.shapes["toWorldTransform"][e1][:3, :3].astype(np.float64)
    sv = np.linalg.svd(M, compute_uv=False)
    assert sv.max() > 1.5 * sv.min() and abs(M[0, 1]) > 0.1 and abs(M[1, 0]) > 0.1
    L = sc.lights[sc.shapes["lightID"][e1]]
    assert L["type"] == T.TRIANGLE_MESH_AREA and L["shapeId"] == e1
    np.testing.assert_allclose(sc.shapes["area"][e1], area.sum(), rtol=1e-6)
    np.testing.assert_allclose(L["area"], area.sum(), rtol=1e-6)
    assert abs(area.sum() - 4.0) > 0.5   # 4: the area of the untransformed mesh


def test_every_branch_is_reached(counts):
    sc, c, frames = counts
    assert not c["broken"], c["broken"]
    need = tz.required(sc, c)
    short = {k: v for k, v in need.items() if v < tz.MIN_PATHS}
    assert not short, short
    assert c["zero_light_query"] == 0
    for f in frames:
        assert np.isfinite(f).all() and f[..., :3].max() > 0


def test_every_triangle_of_emitter1_is_sampled(counts):
    sc, c, _ = counts
    assert (c["emitter1_triangle_rays"] >= tz.MIN_TRIANGLE_RAYS).all(), c["emitter1_triangle_rays"]


def test_emitter1_covers_four_tiles_and_tiles_mix(counts):
    sc, _, _ = counts
    o = po.OracleScene(sc)
    o.build()
    log = o.path_log(tz.W, tz.H, 1)
    o.render(tz.camera(), frame=0, max_depth=1)
    sid = log[:, 0, 0].view(np.int32).reshape(tz.H, tz.W).copy()
    o.path_log(None)
    tiles = sid.reshape(tz.H // 8, 8, tz.W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    assert sum(int((t == sc.zoo["shapes"]["emitter1"]).any()) for t in tiles) >= 4
    assert min(len(np.unique(t)) for t in tiles) >= 2
    assert (sid >= 0).all()


def test_lightless_copy_renders_zeros():
    sc = tz.dark_zoo()
    assert len(sc.lights) == 0 and (sc.shapes["lightID"] == -1).all()
    o = po.OracleScene(sc)
    o.build()
    cam = tz.camera()
    pt = np.full((tz.H, tz.W, 4), 7.0, np.float32)
    o.render(cam, frame=0, max_depth=tz.DEPTH, radiance=pt)
    assert not pt.any()
    rad, cc, lc, _ = po.OracleBDPT(o, tz.W, tz.H, 2).render(cam, frame=0)
    assert not rad.any()


# ---------------------------------------------------------------------------
# the host layer's table check, through the stand-alone sanitizer program
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_asan():
    d = os.path.join(HERE, "asan")
    subprocess.run(["make", "-C", d], check=True, capture_output=True)
    return os.path.join(d, "host_asan")


def run_check(prog, path, sc, expect, shapes=None, materials=None, lights=None, num_textures=None, num_vertices=None):
    shapes = sc.shapes if shapes is None else shapes
    materials = sc.materials if materials is None else materials
    lights = sc.lights if lights is None else lights
    nt = len(sc.textures) if num_textures is None else num_textures
    nv = len(sc.positions) if num_vertices is None else num_vertices
    with open(path, "wb") as f:
        f.write(struct.pack("<7I", len(shapes), len(materials), len(lights), nt, len(sc.indices), nv, expect))
        for a in (shapes, materials, lights, sc.indices):
            f.write(np.ascontiguousarray(a).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([prog, "--tables", str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (expect, r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def test_check_accepts_the_zoo_and_rejects_each_broken_table(host_asan, tmp_path):
    sc = tz.zoo()
    p = tmp_path / "tables.bin"
    run_check(host_asan, p, sc, OK)
    run_check(host_asan, p, tz.dark_zoo(), OK)
    S = sc.zoo["shapes"]
    for field, n, rule in (("materialId", len(sc.materials), MATERIAL_ID), ("lightID", len(sc.lights), LIGHT_ID)):
        for v, want in ((-2, rule), (n, rule), (-1, OK), (n - 1, OK)):
            sh = sc.shapes.copy()
            sh[field][S["plastic"]] = v
            out = run_check(host_asan, p, sc, want, shapes=sh)
            assert want == OK or f"shape {S['plastic']}" in out
    last = len(sc.materials) - 1
    for k in TEX_SLOTS:
        for v, want in ((-2, TEXTURE_ID), (len(sc.textures), TEXTURE_ID), (-1, OK), (len(sc.textures) - 1, OK)):
            m = sc.materials.copy()
            m[k][last] = v
            m["type"][last] = 1   # whatever the type
            out = run_check(host_asan, p, sc, want, materials=m)
            assert want == OK or f"material {last}" in out
    e1 = S["emitter1"]
    for v, want in ((-1, MESH_LIGHT), (len(sc.shapes), MESH_LIGHT), (0, OK), (len(sc.shapes) - 1, OK)):
        L = sc.lights.copy()
        L["shapeId"][sc.shapes["lightID"][e1]] = v
        run_check(host_asan, p, sc, want, lights=L)
    # a startVertex moved one past the end (the last shape's vertices end the vertex array)
    sh = sc.shapes.copy()
    k = int(np.argmax(sh["startVertex"]))
    sh["startVertex"][k] += 1
    assert f"shape {k}" in run_check(host_asan, p, sc, VERTEX_INDEX, shapes=sh)
    run_check(host_asan, p, sc, VERTEX_INDEX, num_vertices=len(sc.positions) - 1)
    # no materials while a shape names one; no lights while a shape names one
    run_check(host_asan, p, sc, MATERIAL_ID, materials=sc.materials[:0])
    run_check(host_asan, p, sc, LIGHT_ID, lights=sc.lights[:0])


def project_scenes(tmp):
    """Every generator of mcrt.scenes (the proxies at a reduced triangle budget: the budget moves
    triangle counts, not ids), the golden fixtures and the OBJ loaders' output."""
    from helpers import bunny_scene, rr_cornell_scene
    from mcrt import lib, objload
    for name in ("mixed", "cornell", "dragon_small", "lod_test", "tex_zoo", "table_zoo", "instances_test", "instanced_small"):
        yield name, build_scene(name)
    yield "table_zoo_dark", tz.dark_zoo()
    yield "san_miguel_proxy", scenes.san_miguel_proxy(tris=60000, tex_size=32)
    yield "sponza_proxy", scenes.sponza_proxy(tris=30000, tex_size=32)
    yield "bunny", bunny_scene()
    yield "rr_cornell", rr_cornell_scene()[0]
    with zipfile.ZipFile(os.path.join(HERE, "golden", "meshes.zip")) as z:
        z.extractall(tmp)
        objs = sorted(n for n in z.namelist() if n.endswith(".obj"))
    for n in objs:
        path = os.path.join(tmp, n)
        yield "capi:" + n, lib.load_obj(path, directional_lights=[((0.3, -1.0, 0.2), (4.0, 4.0, 4.0))])
        yield "python:" + n, objload.load_obj(path).build()


def test_check_accepts_the_projects_scenes(host_asan, tmp_path):
    p = tmp_path / "tables.bin"
    seen = 0
    for name, sc in project_scenes(str(tmp_path)):
        out = run_check(host_asan, p, sc, OK)
        seen += 1
        assert "rule 0" in out, (name, out)
    assert seen >= 15
