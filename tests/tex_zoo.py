"""Shared by the CPU and GPU tests of the texture-zoo scene (mcrt.scenes.texture_zoo_scene): the
scene, the uv of a hit from its barycentrics, and the coverage conditions both suites assert --
the CPU suite from the oracle's primary hits, the GPU suite from the product's own AOV planes."""
import functools

import numpy as np

import tex_ref
from clref_job import build_scene

W, H = 96, 64
MIN_SLOT_PIXELS = 100
MIN_BRANCH_PIXELS = 50
MIN_TILES = 4
BRANCHES = ("below", "inside", "above", "around", "not_around")


@functools.lru_cache(maxsize=None)
def zoo():
    """The zoo scene, built once and shared (with the Sobol matrices the Sobol sampler reads)."""
    from mcrt import sobol_matrices
    sc = build_scene("tex_zoo")
    sc.sobol = sobol_matrices()
    return sc


def hit_uv(sc, shape, prim, bu, bv):
    """uv of hits (shape >= 0) as computeSurfaceInteraction blends it (geometry.cl:177-215), float32."""
    f32 = np.float32
    sh = sc.shapes[shape]
    i = sc.indices[(sh["startIdx"] + 3 * prim)[:, None] + np.arange(3)[None, :]].astype(np.int64) + sh["startVertex"][:, None]
    uv0, uv1, uv2 = sc.uvs[i[:, 0]], sc.uvs[i[:, 1]], sc.uvs[i[:, 2]]
    bu, bv = bu.astype(f32)[:, None], bv.astype(f32)[:, None]
    w0 = (f32(1.0) - bu - bv).astype(f32)
    return ((uv0 * w0).astype(f32) + (uv1 * bu).astype(f32) + (uv2 * bv).astype(f32)).astype(f32)


def coverage(sc, shape, uv):
    """Counts over an (H, W) int shape-id plane (< 0: miss) and the (H, W, 2) float32 uv plane:
      slots[name]                  pixels whose material binds the slot
      branches[(wrap, axis, b)]    pixels taking branch b of tex_ref's read of their DIFFUSE texture
                                   ('border' / 'not_border' for wrap 3 carry axis 'xy')
      one                          pixels where the wrapped coordinate reached the size (texel 0)
      sizes[(w, h, mips)]          pixels per diffuse texture
      uniform_tiles / divergent_tiles   8 x 8 tiles with one material / with three or more"""
    hit = shape >= 0
    mat = np.where(hit, sc.shapes["materialId"][np.maximum(shape, 0)], -1)
    out = {"slots": {}, "branches": {}, "sizes": {}, "one": 0}
    for name in tex_ref.SLOTS:
        out["slots"][name] = int((sc.materials[name][np.maximum(mat, 0)] != -1)[hit].sum())
    dtex = np.where(hit, sc.materials["uber_diffuseTexId"][np.maximum(mat, 0)], -1)
    for wr in range(4):
        for ax in "xy":
            for b in BRANCHES:
                out["branches"][(wr, ax, b)] = 0
    out["branches"][(3, "xy", "border")] = out["branches"][(3, "xy", "not_border")] = 0
    for t in np.unique(dtex[dtex >= 0]):
        sel = dtex == t
        tex = sc.textures[t]
        r = tex_ref.read_tex(tex, sc.tex_data, uv[sel])
        wr = int(tex["wrap"])
        key = (int(tex["width"]), int(tex["height"]), int(tex["numMipLevels"]) > 1)
        out["sizes"][key] = out["sizes"].get(key, 0) + int(sel.sum())
        for ax in "xy":
            br = r.branch[ax]
            for b in ("below", "inside", "above", "around"):
                out["branches"][(wr, ax, b)] += int(br[b].sum())
            out["branches"][(wr, ax, "not_around")] += int((~br["around"] & ~r.border).sum())
            out["one"] += int(br["one"].sum())
        if wr == 3:
            out["branches"][(3, "xy", "border")] += int(r.border.sum())
            out["branches"][(3, "xy", "not_border")] += int((~r.border).sum())
    Hh, Ww = shape.shape
    tiles = mat[:Hh - Hh % 8, :Ww - Ww % 8].reshape(Hh // 8, 8, Ww // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    nmat = np.array([np.unique(t[t >= 0]).size if (t >= 0).all() else -1 for t in tiles])
    out["uniform_tiles"] = int((nmat == 1).sum())
    out["divergent_tiles"] = int((nmat >= 3).sum())
    return out


def check_coverage(sc, cov):
    """The conditions the zoo must meet (the issue's part 3); returns the list of misses."""
    bad = []
    for name, n in cov["slots"].items():
        if n < MIN_SLOT_PIXELS:
            bad.append(f"slot {name}: {n} pixels")
    for key, n in cov["branches"].items():
        if n < MIN_BRANCH_PIXELS:
            bad.append(f"branch {key}: {n} pixels")
    if cov["one"] < MIN_BRANCH_PIXELS:
        bad.append(f"wrapped coordinate == size: {cov['one']} pixels")
    want = {(int(t["width"]), int(t["height"])) for t in sc.textures}
    seen = {(w, h) for (w, h, _), n in cov["sizes"].items() if n > 0}
    if want - seen:
        bad.append(f"sizes never read: {sorted(want - seen)}")
    for k in ("uniform_tiles", "divergent_tiles"):
        if cov[k] < MIN_TILES:
            bad.append(f"{k}: {cov[k]}")
    return bad


def format_coverage(cov):
    lines = ["slots: " + ", ".join(f"{k[5:-2] if k.endswith('Id') else k}={v}" for k, v in cov["slots"].items())]
    for wr in range(4):
        parts = [f"{ax}:{'/'.join(str(cov['branches'][(wr, ax, b)]) for b in BRANCHES)}" for ax in "xy"]
        extra = f" border {cov['branches'][(3, 'xy', 'border')]}/{cov['branches'][(3, 'xy', 'not_border')]}" if wr == 3 else ""
        lines.append(f"wrap {wr} ({'/'.join(BRANCHES)}) " + " ".join(parts) + extra)
    lines.append(f"coordinate == size: {cov['one']}; sizes: " + ", ".join(f"{w}x{h}{'m' if m else ''}={n}" for (w, h, m), n in sorted(cov["sizes"].items())))
    lines.append(f"tiles with one material: {cov['uniform_tiles']}, with >= 3: {cov['divergent_tiles']}")
    return "\n".join(lines)
