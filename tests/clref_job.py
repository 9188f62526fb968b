"""Runs the REFERENCE's OpenCL path tracer (oracle/_ref, GPU box only) in its own process
(keeps the OpenCL runtime out of the HIP test process) and saves its outputs.

usage: python tests/clref_job.py OUT.npz [variant]
Outputs: per-case radiance frames, accumulated images and RadeonRays query results, used by
tests/test_gpu_reference.py (and copied to tests/golden/clref_*.npz as committed fixtures).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monte-carlo-raytracer_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import bunny_scene, random_rays, rr_cornell_scene  # noqa: E402
from mcrt import scenes  # noqa: E402
from mcrt import types as T  # noqa: E402
from mcrt.camera import scene_camera  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

CASES = [  # (scene, W, H, frames, max_depth)
    ("mixed", 96, 64, (0, 1, 3), 2),
    ("mixed", 96, 64, (0, 2), 5),
    ("cornell", 64, 64, (0, 1), 2),
    ("dragon_small", 80, 60, (0,), 2),
]


BDPT_CASES = [  # (scene, W, H, frames rendered in order from fresh buffers, max_depth)
    ("mixed", 96, 64, (0, 1, 2), 2),
    ("cornell", 64, 64, (0, 1), 2),
    ("mixed", 64, 48, (0, 1), 4),
]


# The same, each frame with its TAA-jittered camera (scene_camera(..., frame=f, jitter=True)): frames
# 0..11 of the mixed scene cross frame 10, whose pixel (row 35, column 78) is NaN (BDPT.cl:310 divides
# 0 by 0 for a light ray leaving an area light at cos = 0; tests/test_oracle_bdpt_cpu.py)
BDPT_TAA_CASES = [
    ("mixed", 96, 64, tuple(range(12)), 2),
]
BDPT_NAN_FRAME, BDPT_NAN_PIXEL = 10, (35, 78)   # (row, column), as the oracle finds it


def bdpt_key(case):
    name, W, H, frames, D = case
    return f"bdpt_{name}_{W}x{H}_d{D}" + ("_taa" if case in BDPT_TAA_CASES else "")


def bdpt_camera(case, f):
    """Camera of frame f of a BDPT case: fixed, or the frame's TAA jitter for a BDPT_TAA_CASES case."""
    name, W, H, frames, D = case
    return scene_camera(name, W, H, frame=f, jitter=True) if case in BDPT_TAA_CASES else scene_camera(name, W, H)


def bdpt_job(out_path, variant):
    """RTBDPTPass frames (fresh buffers per case) + the last frame's vertex arrays and counts."""
    res = {}
    for case in BDPT_CASES + BDPT_TAA_CASES:
        name, W, H, frames, D = case
        cs = po.CLRefScene(build_scene(name), variant)
        key = bdpt_key(case)
        for f in frames:
            res[f"{key}_f{f}"] = cs.render_bdpt(bdpt_camera(case, f), frame=f, max_depth=D)
        for which in ("camera_vertices", "light_vertices", "camera_counts", "light_counts", "temp_radiance",
                      "visibility", "connection_rays"):
            res[f"{key}_{which}"] = cs.read_bdpt(which)
    np.savez_compressed(out_path, **res)
    print(f"clref bdpt job ({variant}): {len(res)} arrays -> {out_path}")


def strip_bdpt_golden(src, dst):
    """Keeps the radiance frames and the vertex counts of a bdpt_job output (the committed
    tests/golden/clref_bdpt_*.npz fixtures, BDPT_CASES only: the TAA case is compared live)."""
    z = np.load(src, allow_pickle=False)
    taa = tuple(bdpt_key(c) + "_" for c in BDPT_TAA_CASES)
    keep = {k: z[k] for k in z.files if k.endswith("_counts") or k.rsplit("_", 1)[-1][1:].isdigit()}
    keep = {k: v for k, v in keep.items() if not k.startswith(taa)}
    np.savez_compressed(dst, **keep)


# Two-level (instanced) scenes: RadeonRays' IntersectorTwoLevel kernels over the reference's own
# two-level build (oracle/_ref/librrref.so rr2l_build)
TL_CASES = [  # (scene, W, H, frames, max_depth)
    ("instances_test", 96, 64, (0, 1), 2),
    ("instances_test", 64, 48, (0,), 5),
    ("instanced_small", 80, 60, (0,), 2),
]
TL_BDPT_CASES = [("instances_test", 64, 48, (0, 1), 2)]


def tl_rays(scene, n=20000, seed=11):
    """Random rays; every 8th ray carries a shape id as its mask (RR_RAY_MASK at the instance)."""
    rays = random_rays(scene, n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    sel = np.arange(n) % 8 == 3
    rays["extra"][sel, 0] = rng.integers(0, len(scene.shapes), sel.sum())
    return rays


def tl_job(out_path, variant):
    res = {}
    cache = {}
    for case in TL_CASES:
        name, W, H, frames, D = case
        if name not in cache:
            cache[name] = po.CLRefScene(build_scene(name), variant, two_level=True)
        cs = cache[name]
        cam = scene_camera("instanced_proxy" if name == "instanced_small" else name, W, H)
        for f in frames:
            res[f"{name}_{W}x{H}_d{D}_f{f}"] = cs.render(cam, frame=f, max_depth=D)
    for name, cs in cache.items():
        rays = tl_rays(cs.scene)
        res[f"{name}_rays"] = rays
        res[f"{name}_closest"] = cs.trace(rays)
        res[f"{name}_any"] = cs.trace(rays, any_hit=True)
    for case in TL_BDPT_CASES:
        name, W, H, frames, D = case
        cs = po.CLRefScene(build_scene(name), variant, two_level=True)
        cam = scene_camera(name, W, H)
        for f in frames:
            res[f"bdpt_{name}_{W}x{H}_d{D}_f{f}"] = cs.render_bdpt(cam, frame=f, max_depth=D)
    np.savez_compressed(out_path, **res)
    print(f"clref two-level job ({variant}): {len(res)} arrays -> {out_path}")


# Texture zoo (mcrt.scenes.texture_zoo_scene): every material texture slot, wrap mode and a spread of
# texture sizes, against the reference's PathTracing.cl and BDPT.cl (tests/test_gpu_texture_zoo.py)
TEX_CASES = [("tex_zoo", 96, 64, (0, 1), 3)]
TEX_BDPT_CASES = [("tex_zoo", 96, 64, (0, 1), 2)]


def tex_job(out_path, variant):
    zoo_job(out_path, variant, TEX_CASES, TEX_BDPT_CASES, "texture-zoo")


def zoo_job(out_path, variant, pt_cases, bdpt_cases, what):
    res = {}
    for name, W, H, frames, D in pt_cases:
        cs = po.CLRefScene(build_scene(name), variant)
        cam = scene_camera(name, W, H)
        for f in frames:
            res[f"{name}_{W}x{H}_d{D}_f{f}"] = cs.render(cam, frame=f, max_depth=D)
    for case in bdpt_cases:
        name, W, H, frames, D = case
        cs = po.CLRefScene(build_scene(name), variant)
        cam = scene_camera(name, W, H)
        key = bdpt_key(case)
        for f in frames:
            res[f"{key}_f{f}"] = cs.render_bdpt(cam, frame=f, max_depth=D)
        for which in ("camera_vertices", "light_vertices", "camera_counts", "light_counts"):
            res[f"{key}_{which}"] = cs.read_bdpt(which)
    np.savez_compressed(out_path, **res)
    print(f"clref {what} job ({variant}): {len(res)} arrays -> {out_path}")


# Table zoo (mcrt.scenes.scene_table_zoo): the rare branches of the shape, material and light tables
# (tests/test_gpu_table_zoo.py).  Every table value is one the reference's kernels guard.
TABLE_CASES = [("table_zoo", 96, 64, (0, 1), 3)]
TABLE_BDPT_CASES = [("table_zoo", 96, 64, (0, 1), 2)]


def table_job(out_path, variant):
    zoo_job(out_path, variant, TABLE_CASES, TABLE_BDPT_CASES, "table-zoo")


LOD_CASES = [("lod_test", 160, 120), ("mixed", 96, 64), ("tex_zoo", 96, 64)]


def lod_job(out_path, variant):
    """The reference's texture-LOD functions at its own primary hits (clprobe_lod.cl)."""
    res = {}
    for name, W, H in LOD_CASES:
        cs = po.CLRefScene(build_scene(name), variant)
        res[f"lod_{name}_{W}x{H}"] = cs.probe_lod(scene_camera(name, W, H))
    np.savez_compressed(out_path, **res)
    print(f"clref lod job ({variant}): {len(res)} arrays -> {out_path}")


def build_scene(name):
    if name == "mixed":
        return scenes.test_scene()
    if name == "cornell":
        return scenes.cornell_box(os.path.join(ROOT, "tests", "golden", "cornell_original.npz"))
    if name == "dragon_small":
        return scenes.dragon_proxy(tris=20000)
    if name == "lod_test":
        return scenes.lod_test_scene()
    if name == "tex_zoo":
        return scenes.texture_zoo_scene()
    if name == "table_zoo":
        return scenes.scene_table_zoo()
    if name == "instances_test":
        return scenes.instances_test_scene()
    if name == "instanced_small":
        return scenes.instanced_proxy(grid_n=4, body_tris=6000)
    raise KeyError(name)


# bench.py's timed region at its defaults (--steps 20 --warmup 3): warmup = 4 x 32 frames, one
# untimed statistics frame, then ONE mcrt_render_frames call of frames 129 .. 148
TIMED_F0, TIMED_STEPS = 129, 20
TIMED_CHECK_FRAMES = tuple(TIMED_F0 + k for k in (1, 7, 19))


def taa_camera(name, W, H, f):
    """bench.py's camera of frame f: 64 precomputed TAA-jittered cameras, camera f % 64."""
    return scene_camera(name, W, H, frame=f % 64, jitter=True)


# BASELINE.json config 1 (the reference's CPU-device plumbing case): Dragon proxy 512x512, 4 spp
# (frames 0..3 accumulated with the box filter), PT, maxDepth 2.  "pt_acc": the frames are
# compared bit for bit and the product's accumulated image against the oracle's accumulation of
# the reference's frames (test_gpu_reference_scale.py); CONFIG1_ROWS of the reference frames are
# committed as tests/golden/config1_dragon512.npz (config1_job) for the CPU oracle test.
CONFIG1 = ("dragon_pt_512_4spp", "dragon_proxy", 512, 512, "pt_acc", (0, 1, 2, 3), 2)
CONFIG1_ROWS = tuple(range(3, 512, 64))


def config1_job(out_path, variant):
    key, name, W, H, _, frames, D = CONFIG1
    cs = po.CLRefScene(scale_scene(name), variant)
    cam = scene_camera(name, W, H)
    rows = np.asarray(CONFIG1_ROWS, np.int32)
    res = {"rows": rows}
    for f in frames:
        res[f"f{f}"] = np.ascontiguousarray(cs.render(cam, frame=f, max_depth=D)[rows, :, :3])
    np.savez_compressed(out_path, **res)


# BASELINE.json configs at full size against the reference kernels run live
# (tests/test_gpu_reference_scale.py): (key, scene, W, H, integrator, frames, max_depth).
# The sampler is the job's variant: "ieee" = random (the reference default), "sobol_ieee" = the
# reference rebuilt with RT_SAMPLER_SOBOL (oracle/refbuild/Makefile SOBOL_BUILD).
SCALE_CASES = {
    "ieee": [
        ("sm_pt_1080p", "san_miguel_proxy", 1920, 1080, "pt", (0, 1), 2),            # headline / config 4 scene
        # the bench's timed call: frames TIMED_F0 .. TIMED_F0 + 19 with TAA-jittered cameras
        # (camera of frame f = jitter of f % 64, bench.py cam_of); frames 1, 7, 19 of the batch
        ("sm_pt_1080p_taa", "san_miguel_proxy", 1920, 1080, "pt_taa", TIMED_CHECK_FRAMES, 2),
        ("sponza_pt_1080p", "sponza_proxy", 1920, 1080, "pt", (0, 1), 2),           # config 3
        ("dragon_pt_1080p", "dragon_proxy", 1920, 1080, "pt", (0, 1), 2),           # config 2
        ("sm_bdpt_1080p", "san_miguel_proxy", 1920, 1080, "bdpt", (0, 1), 2),       # config 4 integrator (bench size)
        # SURVEY §8(d)'s depth-5 sensitivity case (PathTracingSettings.h:81 allows maxDepth 1..10):
        # the regime where the wavefront's queues shrink bounce by bounce
        ("sm_pt_1080p_d5", "san_miguel_proxy", 1920, 1080, "pt", (0, 1), 5),
        ("sm_bdpt_540p_d5", "san_miguel_proxy", 960, 540, "bdpt", (0, 1), 5),
        # config 1: the Dragon proxy at 512x512, 4 spp accumulated (frames 0..3, box filter)
        CONFIG1,
    ],
    "sobol_ieee": [
        ("sm_sobol_4k", "san_miguel_proxy", 3840, 2160, "pt", (0, 600), 2),        # config 5; frame 600: Q6 wrap
        ("mixed_sobol_d5", "mixed", 96, 64, "pt", (0, 3), 5),
        ("mixed_sobol_bdpt", "mixed", 96, 64, "bdpt", (0, 1), 2),
    ],
}
BDPT_VERTEX_STRIDE = 17   # vertex records kept for every 17th pixel (the full arrays are ~0.5 GB at 960x540)
# cases whose FULL vertex arrays are also written (raw .npy beside the job's npz, ~3.5 GB at 1080p D = 2,
# ~1.6 GB at 960x540 D = 5), so every pixel's vertices are compared: config 4's integrator at the bench's
# size and the depth-5 case
FULL_VERTEX_CASES = ("sm_bdpt_1080p", "sm_bdpt_540p_d5")


def full_vertex_path(out_path, key, which):
    return f"{out_path}.{key}_{which}.npy"


def bdpt_vertex_sel(W, H):
    """Pixels whose BDPT vertex records the full-size comparison keeps: every 17th pixel, plus every
    pixel of three full rows (top, middle, bottom) and of a 64 x 64 block at the image centre, so
    neighbouring pixels (shared tiles, waves, splat targets) are compared without gaps too."""
    N = W * H
    rows = [np.arange(r * W, (r + 1) * W) for r in (0, H // 2, H - 1)]
    y0, x0 = H // 2 - 32, W // 2 - 32
    block = (np.arange(y0, y0 + 64)[:, None] * W + np.arange(x0, x0 + 64)[None, :]).ravel()
    return np.unique(np.concatenate([np.arange(0, N, BDPT_VERTEX_STRIDE), *rows, block]))


def scale_scene(name):
    from mcrt import sobol_matrices
    full = {"san_miguel_proxy": scenes.san_miguel_proxy, "sponza_proxy": scenes.sponza_proxy,
            "dragon_proxy": scenes.dragon_proxy}
    sc = full[name]() if name in full else build_scene(name)
    sc.sobol = sobol_matrices()
    return sc


def scale_job(out_path, variant):
    res = {}
    cache, nodes = {}, {}
    for key, name, W, H, integ, frames, D in SCALE_CASES[variant]:
        if name not in cache:
            cache.clear()
            nodes.clear()
            cache[name] = scale_scene(name)
        cam = scene_camera(name, W, H)
        cs = po.CLRefScene(cache[name], variant, nodes=nodes.get(name))   # Bvh2 nodes built once per scene
        nodes[name] = cs.nodes
        t0 = time.time()
        for f in frames:
            if integ == "pt_taa":
                res[f"{key}_f{f}"] = cs.render(taa_camera(name, W, H, f), frame=f, max_depth=D)
                continue
            res[f"{key}_f{f}"] = (cs.render_bdpt if integ == "bdpt" else cs.render)(cam, frame=f, max_depth=D)
        if integ == "bdpt":
            N = W * H
            sel = bdpt_vertex_sel(W, H)
            for which, depths in (("camera_vertices", D + 2), ("light_vertices", D + 1)):
                raw = cs.read_bdpt(which)
                v = raw.view(po.REF_VERTEX_DTYPE).reshape(N, depths)
                res[f"{key}_{which}"] = np.ascontiguousarray(v[sel])
                if key in FULL_VERTEX_CASES:
                    np.save(full_vertex_path(out_path, key, which), raw)
                del raw, v
            for which in ("camera_counts", "light_counts"):
                res[f"{key}_{which}"] = cs.read_bdpt(which).view(np.int32)
        print(f"{key}: {len(frames)} frames in {time.time() - t0:.1f}s", flush=True)
        del cs
    np.savez(out_path, **res)


def update_steps(sc):
    """Dynamic scene updates (RTScene::update, RTScene.cpp:317-391) applied cumulatively to the
    mixed scene: returns [(kind, new array)] -- materials edited, a shape moved (its transform and
    inverse transpose; the BVH is rebuilt, as RR's Commit does), lights re-scaled and re-aimed."""
    steps = []
    mats = sc.materials.copy()
    mats["uber_kd"][0, :3] *= 0.5
    mats["uber_roughness"][1] = (0.31, 0.07)
    mats["uber_ks"][2, :3] = (0.2, 0.6, 0.1)
    steps.append(("materials", mats))
    shapes = sc.shapes.copy()
    k = len(shapes) // 2
    M = shapes["toWorldTransform"][k].astype(np.float64)
    Tm = np.eye(4)
    Tm[:3, 3] = (0.3, 0.05, -0.2)
    M2 = (Tm @ M).astype(np.float32)
    shapes["toWorldTransform"][k] = M2
    shapes["toWorldInverseTranspose"][k] = np.linalg.inv(M2.astype(np.float64)).T.astype(np.float32)
    steps.append(("shapes", shapes))
    lights = sc.lights.copy()
    lights["intensity"][:, :3] *= np.float32(1.7)
    d = lights["d"][0, :3].astype(np.float64) + (0.1, -0.05, 0.2)
    lights["d"][0, :3] = (d / np.linalg.norm(d)).astype(np.float32)   # light 0 re-aimed
    steps.append(("lights", lights))
    return steps


def apply_step(sc, kind, arr):
    setattr(sc, kind, arr)
    sc._desc = None


def updates_job(out_path, variant):
    """The reference renders the mixed scene freshly built with each cumulative update."""
    res = {}
    sc = build_scene("mixed")
    cam = scene_camera("mixed", 96, 64)
    for i, (kind, arr) in enumerate(update_steps(sc)):
        apply_step(sc, kind, arr)
        cs = po.CLRefScene(sc, variant)
        for f in (0, 1):
            res[f"update{i}_{kind}_f{f}"] = cs.render(cam, frame=f, max_depth=3)
        del cs
    np.savez(out_path, **res)


def filter_table():
    """Reconstruction filters for tests/test_gpu_accumulate.py: every filter type at the reference's
    default settings (PathTracingSettings.h:55-66) and variations, each at TAA pixel offsets of
    frames 0..11 (PathTracingApp.cpp:208-215) plus hand-picked edge offsets."""
    from mcrt.camera import taa_jitter
    rows = []
    settings = [(T.BOX, {}), (T.TRIANGLE, {}), (T.TRIANGLE, dict(radius=(1.5, 3.0))),
                (T.GAUSSIAN, {}), (T.GAUSSIAN, dict(alpha=2.5, radius=(1.0, 2.0))),
                (T.MITCHELL, {}), (T.MITCHELL, dict(B=0.5, C=0.25)), (T.LANCZOS, {}), (T.LANCZOS, dict(tau=2.0))]
    for kind, kw in settings:
        r = kw.get("radius", (2.0, 2.0))
        offs = [taa_jitter(f, radius=r) for f in range(12)]
        offs += [(0.0, 0.0), (r[0], -r[1]), (0.5 * r[0], 1e-6), (-0.999 * r[0], 0.25)]
        for o in offs:
            rows.append(T.make_filter(kind, pixel_offset=o, **kw)[0])
    out = np.zeros(len(rows), T.FILTER_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def filters_job(out_path, variant):
    f = filter_table()
    np.savez(out_path, filters=f, weights=po.clref_filter_weights(f, variant))


def sm_job(out_path, variant, W, H, tris):
    """Two depth-2 frames of the San-Miguel proxy (test_san_miguel_proxy_bit_exact_vs_reference)."""
    cs = po.CLRefScene(scenes.san_miguel_proxy(tris=tris), variant)
    cam = scene_camera("san_miguel_proxy", W, H)
    np.savez_compressed(out_path, **{f"f{f}": cs.render(cam, frame=f, max_depth=2) for f in (0, 1)})


def main():
    out_path = sys.argv[1]
    variant = sys.argv[2] if len(sys.argv) > 2 else "ieee"
    if len(sys.argv) > 3 and sys.argv[3] == "bdpt":
        bdpt_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "lod":
        lod_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "tex":
        tex_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "table":
        table_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "2l":
        tl_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "updates":
        updates_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "filters":
        filters_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "config1":
        config1_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "scale":
        scale_job(out_path, variant)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "sm":
        sm_job(out_path, variant, int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
        return
    res = {}
    t0 = time.time()
    po.clref(variant)
    res["device"] = np.array(po.clref(variant).clref_device().decode())
    cache = {}
    for name, W, H, frames, D in CASES:
        if name not in cache:
            cache[name] = po.CLRefScene(build_scene(name), variant)
        cs = cache[name]
        cam_name = "dragon_proxy" if name == "dragon_small" else name
        cam = scene_camera(cam_name, W, H)
        for f in frames:
            res[f"{name}_{W}x{H}_d{D}_f{f}"] = cs.render(cam, frame=f, max_depth=D)
    # accumulation over 8 frames, box filter (ReconstructionPass)
    cs = cache["mixed"]
    cam = scene_camera("mixed", 64, 48)
    filt = T.make_filter(T.BOX)
    try:
        for f in range(8):
            cs.render(cam, frame=f, max_depth=2)
            img = cs.accumulate(f, filt, 48, 64)
        res["mixed_accum8_64x48"] = img
    except RuntimeError as e:   # no OpenCL image support on CDNA
        print("ReconstructionPass skipped:", e)
    # RadeonRays queries: conformance rays on orig.objm, random rays on bunny / mixed
    sc, z = rr_cornell_scene()
    rc = po.CLRefScene(sc, variant)
    res["rr_cornell_closest"] = rc.trace(z["rays_closest"])
    res["rr_cornell_any"] = rc.trace(z["rays_any"], any_hit=True)
    for nm, s in (("bunny", bunny_scene()), ("mixed", scenes.test_scene())):
        rays = random_rays(s, 20000, seed=11)
        c = po.CLRefScene(s, variant)
        res[f"{nm}_rays"] = rays
        res[f"{nm}_closest"] = c.trace(rays)
    np.savez_compressed(out_path, **res)
    print(f"clref_job ({variant}) on {res['device']}: {len(res)} arrays in {time.time() - t0:.1f}s -> {out_path}")


if __name__ == "__main__":
    main()
