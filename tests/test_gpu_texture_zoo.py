"""GPU tests of the texture path on the texture-zoo scene (mcrt.scenes.texture_zoo_scene): every
material texture slot, all four wrap modes, texture sizes 1x1 .. 100x60 (odd, non-square, one texel
wide), with and without mip chains, uvs from -1.75 to 2.5 and strips of pixels that sit on the
wrap branches' boundaries.

  * the product's texture read (MCRT_AOV_TEXTURE_LOD: the uv, the lod and the value the kernel
    read) and its albedo / opacity (MCRT_AOV_ALBEDO) against tests/tex_ref.py, the plain float64
    restatement of the reference's text, within the tolerance derived in that module;
  * whole PT and BDPT frames against the reference's own kernels run live (tests/clref_job.py
    ... tex), bit for bit as tests/test_gpu_reference.py and tests/test_gpu_bdpt.py judge theirs;
  * PT frames against the oracle with tests/test_gpu_render.py::test_frame_parity's criterion;
  * the coverage conditions of tests/tex_zoo.py, from the product's own AOV planes.
tests/test_gpu_texture_lod.py compares the same AOV planes bit for bit with the reference's
textures.cl compiled for this GPU (LOD_CASES holds the zoo).

Mutation check (done once by hand; the mutated code is not committed).  The library was built
with each single change to csrc/mcrt_shading.h -- none can index outside a texture, the final
clamps stay -- and this module plus test_gpu_texture_lod.py's footprint test were run:

  mutant                                              caught by
  mirror formula without its `1.0f -`                 test_texture_read_matches_tex_ref, test_albedo_matches_tex_ref
                                                      (both), test_pt_frames_match_reference, test_bdpt_frames_match_reference,
                                                      test_pt_frames_match_oracle (both), footprint[tex_zoo]
  cl_div in place of cr_div for 1 / w, 1 / h          test_texture_read_matches_tex_ref, test_albedo_matches_tex_ref (both),
                                                      test_pt_frames_match_reference, test_bdpt_frames_match_reference,
                                                      footprint[tex_zoo]  (footprint[lod_test] and [mixed], whose sizes are
                                                      powers of two, pass)
  Kr reading the glossy slot                          test_pt_frames_match_reference, test_bdpt_frames_match_reference,
                                                      test_pt_frames_match_oracle (both)
  roughness texture's .xy taken as .xx                test_pt_frames_match_reference, test_bdpt_frames_match_reference,
                                                      test_pt_frames_match_oracle (both)
  nonDelta opacity from the product, not the texture  test_bdpt_frames_match_reference
The unmutated library passes everything: the reciprocals 1 / w and 1 / h are correctly rounded in
the reference's compiled kernels for widths 3, 5, 7, 60 and 100 too, as readTexDesc's comment says.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import tex_ref
import tex_zoo as tz
from clref_job import TEX_BDPT_CASES, TEX_CASES, bdpt_key
from mcrt import types as T
from mcrt.camera import scene_camera
from oracle import pyoracle as po
from test_gpu_bdpt import REL_TOL, compare_vertices, our_planes
from test_gpu_render import pixel_agreement

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = tz.W, tz.H


@pytest.fixture(scope="module")
def zoo_gpu(hip_ctx):
    """The zoo on the device and its AOV planes: (scene, DeviceScene, FrameBuffer, camera, planes)."""
    from mcrt import lib
    sc = tz.zoo()
    ds = lib.DeviceScene(hip_ctx, sc)
    fb = lib.FrameBuffer(hip_ctx, W, H)
    cam = scene_camera("tex_zoo", W, H)
    planes = {"lod": fb.render_aov(ds, cam, T.AOV_TEXTURE_LOD),
              "albedo": fb.render_aov(ds, cam, T.AOV_ALBEDO),
              "albedo_lod": fb.render_aov(ds, cam, T.AOV_ALBEDO, texture_lod=True)}
    yield sc, ds, fb, cam, planes
    fb.close()
    ds.close()


def hit_planes(sc, planes):
    """(shape (H, W) int, -1 = miss; material; uv (H, W, 2); lod (H, W)) of the TEXTURE_LOD planes."""
    p = planes["lod"]
    shape = p[..., 1, 1].view(np.int32).copy()
    miss = (p[..., 0, :] == 0).all(-1) & (p[..., 1, :].view(np.uint32) == 0).all(-1)   # a miss writes zeros
    shape[miss] = -1
    mat = np.where(shape >= 0, sc.shapes["materialId"][np.maximum(shape, 0)], -1)
    return shape, mat, p[..., 1, 2:4], p[..., 1, 0]


def test_texture_read_matches_tex_ref(zoo_gpu):
    """For every hit pixel with a diffuse texture: tex_ref's read at the uv and lod the kernel used
    (plane 1) gives the value the kernel read (plane 2) within tex_ref's derived tolerance.  Plain
    textures take the bilinear path, mip-mapped ones all three of readTexture2Df_lod's paths."""
    sc, _, _, _, planes = zoo_gpu
    shape, mat, uv, lod = hit_planes(sc, planes)
    val = planes["lod"][..., 2, :].astype(np.float64)
    dtex = np.where(mat >= 0, sc.materials["uber_diffuseTexId"][np.maximum(mat, 0)], -1)
    assert not val[dtex < 0].any()
    paths = {False: np.zeros(3, int), True: np.zeros(3, int)}
    bad, worst, n = [], 0.0, 0
    for t in np.unique(dtex[dtex >= 0]):
        sel = dtex == t
        tex = sc.textures[t]
        want, tol, path = tex_ref.read_lod(tex, sc.tex_data, uv[sel], lod[sel])
        paths[int(tex["numMipLevels"]) > 1] += np.bincount(path, minlength=3)
        err = np.abs(val[sel] - want)
        n += int(sel.sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(tol > 0, err / tol, 0.0))))
        if not (err <= tol).all():
            k = int((err > tol).any(1).sum())
            bad.append((tuple(tex_ref.desc_fields(tex)[:4]), k, int(sel.sum()), float((err - tol).max())))
    print(f"{n} textured pixels; largest error / tolerance {worst:.3f}; paths (linear, last, trilinear): "
          f"plain {paths[False].tolist()}, mip-mapped {paths[True].tolist()}")
    assert not bad, bad
    assert n > 4000 and paths[False][0] > 1000 and not paths[False][1:].any()
    assert (paths[True] >= 50).all(), paths[True]


@pytest.mark.parametrize("with_lod", [False, True], ids=["level0", "mipmapped"])
def test_albedo_matches_tex_ref(zoo_gpu, with_lod):
    """MCRT_AOV_ALBEDO = (uber Kd, opacity.x) of every hit pixel against tex_ref's
    getUberMaterialProperties: diffuse texture times kd; opacity texture times the constant times
    the diffuse texture's alpha."""
    sc, _, _, _, planes = zoo_gpu
    shape, mat, uv, lod = hit_planes(sc, planes)
    got = planes["albedo_lod" if with_lod else "albedo"].astype(np.float64)
    assert not got[mat < 0].any()
    worst = 0.0
    for m in np.unique(mat[mat >= 0]):
        sel = mat == m
        rec = sc.materials[m]
        if with_lod:
            # plane 1's lod is the diffuse texture's; the opacity texture's is the same number when
            # it has as many levels (computeMipmapLOD depends on the level count alone) and is
            # unused when it has one level
            d, o = int(rec["uber_diffuseTexId"]), int(rec["uber_opacityTexId"])
            levels = {int(sc.textures[t]["numMipLevels"]) for t in (d, o) if t != -1} - {1}
            assert len(levels) <= 1 and (d != -1 or not levels), m
            plod = lod[sel]

            def reader(tex, data, q):
                v, tol, _ = tex_ref.read_lod(tex, data, q, plod)
                return v, tol
        else:
            reader = None
        want = tex_ref.uber_properties(rec, sc.textures, sc.tex_data, uv[sel], reader)
        ref = np.concatenate([want["Kd"], want["opacity"][:, :1]], 1)
        # the texture tolerance carried through the products, plus one float32 rounding per product
        tol = np.concatenate([want["tol_Kd"] + tex_ref.ulp32(want["Kd"]),
                              want["tol_opacity"][:, :1] + 2.0 * tex_ref.ulp32(want["opacity"][:, :1])], 1)
        err = np.abs(got[sel] - ref)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (m, int((err > tol).any(1).sum()), int(sel.sum()), float((err - tol).max()))
    print(f"albedo ({'mip-mapped' if with_lod else 'level 0'}): largest error / tolerance {worst:.3f}")


def test_coverage_from_product_planes(zoo_gpu):
    """The zoo's conditions (tests/tex_zoo.py) hold for the hits, uvs and materials the product
    itself reports: slots, wrap branches per mode and axis, sizes, uniform and divergent tiles."""
    sc, _, _, _, planes = zoo_gpu
    shape, mat, uv, lod = hit_planes(sc, planes)
    cov = tz.coverage(sc, shape, uv)
    print(tz.format_coverage(cov))
    assert not tz.check_coverage(sc, cov), tz.check_coverage(sc, cov)


# ---------------------------------------------------------------------------
# frames against the reference's kernels, live
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clref_tex(tmp_path_factory):
    if not po.clref_available():
        pytest.skip("oracle/_ref/clref_runner.so not built")
    out = str(tmp_path_factory.mktemp("clref") / "clref_tex.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "clref_job.py"), out, "ieee", "tex"],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.fail("reference texture-zoo job failed:\n" + r.stdout + r.stderr)
    return np.load(out, allow_pickle=False)


@pytest.mark.parametrize("case", TEX_CASES, ids=[f"{c[0]}_d{c[4]}" for c in TEX_CASES])
def test_pt_frames_match_reference(zoo_gpu, clref_tex, case):
    sc, ds, fb, cam, _ = zoo_gpu
    name, w, h, frames, D = case
    assert (w, h) == (W, H)
    for f in frames:
        fb.render(ds, cam, frame=f, max_depth=D, sampler=T.SAMPLER_RANDOM)
        g = fb.read(0)
        ref = clref_tex[f"{name}_{w}x{h}_d{D}_f{f}"]
        diff = (g[..., :3].view(np.uint32) != ref[..., :3].view(np.uint32)).any(-1)
        assert not diff.any(), (name, D, f, int(diff.sum()), np.argwhere(diff)[:8].tolist())
        assert np.isfinite(g).all() and g[..., :3].max() > 0


@pytest.mark.parametrize("case", TEX_BDPT_CASES, ids=[bdpt_key(c) for c in TEX_BDPT_CASES])
def test_bdpt_frames_match_reference(hip_ctx, clref_tex, case):
    """Judged as tests/test_gpu_bdpt.py::test_bdpt_matches_reference judges its cases: vertex records
    and counts bit-exact, radiance bit-exact where no splat landed, within REL_TOL elsewhere."""
    from mcrt import lib
    name, w, h, frames, D = case
    key = bdpt_key(case)
    N = w * h
    ds = lib.DeviceScene(hip_ctx, tz.zoo())
    fb = lib.FrameBuffer(hip_ctx, w, h)
    cam = scene_camera(name, w, h)
    report = []
    for f in frames:
        fb.render(ds, cam, frame=f, max_depth=D, sampler=T.SAMPLER_RANDOM, integrator=T.INTEGRATOR_BDPT)
        g = fb.read(0)[..., :3]
        ref = clref_tex[f"{key}_f{f}"][..., :3]
        exact = (g.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(g) & np.isnan(ref))
        close = np.abs(g - ref) <= REL_TOL * (np.abs(g) + np.abs(ref)) + 1e-30
        close |= exact
        nosplat = (fb.read_bdpt("splat").view(np.float32).reshape(h, w, 4)[..., :3] == 0).all(-1)
        ex_ns = exact.all(-1)[nosplat]
        report.append(f"frame {f}: bit-exact {exact.mean():.5f} (no-splat pixels {ex_ns.mean():.5f} of "
                      f"{int(nosplat.sum())}), within {REL_TOL:g} {close.mean():.5f}, mean {np.nanmean(g):.6f} vs {np.nanmean(ref):.6f}")
        if not ex_ns.all():
            report.append(f"frame {f}: {int((~ex_ns).sum())} no-splat pixels outside bit-exactness")
        if not close.all():
            report.append(f"frame {f}: {int((~close).sum())} pixels outside tolerance")
    cc = fb.read_bdpt("camera_counts").view(np.int32)
    lc = fb.read_bdpt("light_counts").view(np.int32)
    rcc = clref_tex[f"{key}_camera_counts"].view(np.int32)
    rlc = clref_tex[f"{key}_light_counts"].view(np.int32)
    bad = [r for r in report if "outside" in r]
    if (cc != rcc).any():
        bad.append(f"camera counts differ at {int((cc != rcc).sum())} pixels")
    if (lc != rlc).any():
        bad.append(f"light counts differ at {int((lc != rlc).sum())} pixels")
    bad += compare_vertices(our_planes(fb.read_bdpt("camera_vertices"), D + 2, N),
                           clref_tex[f"{key}_camera_vertices"].view(po.REF_VERTEX_DTYPE).reshape(N, D + 2),
                           cc, D + 2, N, "camera")
    bad += compare_vertices(our_planes(fb.read_bdpt("light_vertices"), D + 1, N),
                            clref_tex[f"{key}_light_vertices"].view(po.REF_VERTEX_DTYPE).reshape(N, D + 1),
                            lc, D + 1, N, "light")
    print(key, report)
    fb.close()
    ds.close()
    assert not bad, (bad, report)


# ---------------------------------------------------------------------------
# frames against the oracle (no oracle/_ref needed)
# ---------------------------------------------------------------------------
ORACLE_AGREEMENT = 0.98844 - 0.002


@pytest.fixture(scope="module")
def zoo_oracle():
    o = po.OracleScene(tz.zoo())
    o.build()
    return o


@pytest.mark.parametrize("sampler", [T.SAMPLER_RANDOM, T.SAMPLER_SOBOL], ids=["random", "sobol"])
def test_pt_frames_match_oracle(hip_ctx, zoo_oracle, sampler):
    """tests/test_gpu_render.py::test_frame_parity's criterion at depth 3, with the share of agreeing
    pixels the zoo allows.  The ORACLE against the REFERENCE's kernels run live on this scene (both
    sampler builds, frames 0, 1 and 3; never the product) agrees on 0.98844 .. 0.98975 of the pixels,
    below test_frame_parity's 0.995, for two reasons that are the scene's purpose: the edge strips
    put whole strips of pixels within an ulp of a wrap branch (the CPU's unfused uv blend lands on
    the other side of it), and the small quads run more than one uv unit -- 64 random texels -- per
    pixel, so the last bits of the CPU's and the GPU's hit barycentrics move the albedo by a few
    1e-4.  The bar is the lowest measured share minus 0.002."""
    from mcrt import lib
    ds = lib.DeviceScene(hip_ctx, tz.zoo())
    fb = lib.FrameBuffer(hip_ctx, W, H)
    cam = scene_camera("tex_zoo", W, H)
    for frame in (0, 3):
        fb.render(ds, cam, frame=frame, max_depth=3, sampler=sampler)
        g = fb.read(0)
        r, _ = zoo_oracle.render(cam, frame=frame, max_depth=3, sampler=sampler)
        assert np.isfinite(g).all()
        frac = pixel_agreement(g, r)
        print(f"sampler {sampler} frame {frame}: pixel agreement {frac:.5f}")
        assert frac >= ORACLE_AGREEMENT, (frame, frac)
        np.testing.assert_allclose(g[..., :3].mean((0, 1)), r[..., :3].mean((0, 1)), rtol=2e-2)
    fb.close()
    ds.close()
