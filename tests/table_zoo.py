"""Shared by the CPU and GPU tests of the table-zoo scene (mcrt.scenes.scene_table_zoo): the scene,
and the branch counts of the oracle's path log (oracle/mcrt_oracle.h orc_set_pathlog) that the CPU
suite holds against the scene's coverage conditions."""
import functools

import numpy as np

from clref_job import build_scene
from mcrt import types as T
from mcrt.camera import scene_camera

W, H = 96, 64
DEPTH = 3
FRAMES = (0, 1)
MIN_PATHS = 32          # per branch
MIN_TRIANGLE_RAYS = 8   # shadow rays aimed at each triangle of emitter 1
SPECULAR, REFLECTION, TRANSMISSION = 16, 1, 2   # BxDFType bits (KRN/bxdfs.cl)


@functools.lru_cache(maxsize=None)
def zoo():
    """The zoo, built once and shared (with the Sobol matrices the Sobol sampler reads)."""
    from mcrt import sobol_matrices
    sc = build_scene("table_zoo")
    sc.sobol = sobol_matrices()
    return sc


@functools.lru_cache(maxsize=None)
def dark_zoo():
    """The same scene without lights and light ids."""
    from mcrt import scenes
    return scenes.scene_table_zoo(lights=False)


def camera():
    return scene_camera("table_zoo", W, H)


def world_triangles(sc, shape):
    """(numTriangles, 3, 3) float64 world-space vertices of one shape."""
    sh = sc.shapes[shape]
    i = sc.indices[sh["startIdx"]: sh["startIdx"] + 3 * sh["numTriangles"]].astype(np.int64) + int(sh["startVertex"])
    P = sc.positions[i, :3].astype(np.float64)
    M = sh["toWorldTransform"].astype(np.float64)
    return (P @ M[:3, :3].T + M[:3, 3]).reshape(-1, 3, 3)


def locate(tris, p, eps=1e-3):
    """Index of the triangle of `tris` (K, 3, 3) that holds each point of p (N, 3), -1: none."""
    out = np.full(len(p), -1)
    for k, (a, b, c) in enumerate(tris):
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        q = p - a
        off = np.abs(q @ n)
        v0, v1 = b - a, c - a
        d00, d01, d11 = v0 @ v0, v0 @ v1, v1 @ v1
        d20, d21 = q @ v0, q @ v1
        den = d00 * d11 - d01 * d01
        v = (d11 * d20 - d01 * d21) / den
        w = (d00 * d21 - d01 * d20) / den
        inside = (off < eps) & (v >= -eps) & (w >= -eps) & (v + w <= 1 + eps)
        out[inside & (out < 0)] = k
    return out


def path_counts(sc, logs):
    """Branch counts over the path logs [(H*W, DEPTH, 32) float32 per frame] of oracle PT frames."""
    sh = sc.shapes
    S = sc.zoo["shapes"]
    mat = sh["materialId"]
    nl = len(sc.lights)
    c = {"emitter_front_b0": 0, "emitter_back_b0": 0, "emitter_after_specular_reflection": 0,
         "emitter_after_specular_transmission": 0, "emitter_after_non_specular": 0,
         "emitter1_after_specular_reflection": 0, "emitter1_after_specular_transmission": 0,
         "emitter1_after_non_specular": 0,
         "no_material_b0": 0, "no_material_later": 0, "type1_b0": 0, "type1_later": 0, "non_area_light_id_b0": 0,
         "zero_light_no_query": 0, "zero_light_query": 0, "disk_in_plane_no_query": 0, "broken": []}
    for li in range(nl):
        c[f"light{li}_unoccluded"] = c[f"light{li}_occluded"] = 0
    e1 = S["emitter1"]
    tris1 = world_triangles(sc, e1)
    c["emitter1_triangle_rays"] = np.zeros(len(tris1), int)
    zero = [i for i in range(nl) if not sc.lights["intensity"][i, :3].any()]
    disk = [i for i in range(nl) if sc.lights["type"][i] == T.DISK_AREA]
    area = np.isin(sc.lights["type"], (T.DISK_AREA, T.TRIANGLE_MESH_AREA)) if nl else np.zeros(0, bool)
    is_type1 = np.zeros(len(sh), bool)
    ok = mat >= 0
    is_type1[ok] = sc.materials["type"][mat[ok]] != 0
    for log in logs:
        prev = None
        for b in range(log.shape[1]):
            rec = log[:, b]
            sid = rec[:, 0].view(np.int32)
            prim = rec[:, 1].view(np.int32)
            bx = rec[:, 5].view(np.int32)
            li = rec[:, 6].view(np.int32)
            occ = rec[:, 7].view(np.int32)
            live = sid >= 0
            s0 = np.maximum(sid, 0)
            light_id = np.where(live, sh["lightID"][s0], -1)
            em = light_id >= 0
            em_area = em & area[np.maximum(light_id, 0)] if nl else em
            # the side the ray met, from the logged ray and the triangle (gn = (p0 - p2) x (p1 - p2))
            front = np.zeros(len(sid), bool)
            for s in np.unique(sid[em]):
                sel = sid == s
                t = world_triangles(sc, s)[prim[sel]]
                gn = np.cross(t[:, 0] - t[:, 2], t[:, 1] - t[:, 2])
                front[sel] = np.einsum("ij,ij->i", gn, -rec[sel, 27:30].astype(np.float64)) > 0
            if b == 0:
                c["emitter_front_b0"] += int((em_area & front).sum())
                c["emitter_back_b0"] += int((em_area & ~front).sum())
                c["non_area_light_id_b0"] += int((em & ~em_area).sum())
                shaded = live & ~em
            else:
                spec = (prev & SPECULAR) == SPECULAR
                for name, bit in (("reflection", REFLECTION), ("transmission", TRANSMISSION)):
                    c[f"emitter_after_specular_{name}"] += int((em & spec & ((prev & bit) != 0)).sum())
                    c[f"emitter1_after_specular_{name}"] += int((em & spec & ((prev & bit) != 0) & (sid == e1) & front).sum())
                c["emitter_after_non_specular"] += int((em & ~spec & (prev > 0)).sum())
                c["emitter1_after_non_specular"] += int((em & ~spec & (prev > 0) & (sid == e1)).sum())
                shaded = live & ~(em & spec)
            # a shaded hit draws a light; an emission hit and a miss draw none
            if ((li >= 0) != shaded).any():
                c["broken"].append(f"bounce {b}: light drawn != shaded hit at {int(((li >= 0) != shaded).sum())} paths")
            nomat = shaded & (mat[s0] == -1)
            t1 = shaded & is_type1[s0]
            # no material: a light is drawn, no shadow query, no sampled type, no next ray.  Another
            # type: a light is drawn and no shadow query is made (it evaluates to 0), but the path
            # goes on -- the reference's compiled kernels sample every material as the uber one
            last = b + 1 == log.shape[1]
            for name, m, ends in (("no_material", nomat, True), ("type1", t1, last)):
                c[f"{name}_{'b0' if b == 0 else 'later'}"] += int(m.sum())
                bad = m & ((li < 0) | (occ != -2))
                bad |= m & ((bx != -1) | (rec[:, 21] != 0)) if ends else m & (bx <= 0)
                if bad.any():
                    c["broken"].append(f"bounce {b}: {name} hit with a shadow query or the wrong sampled type at {int(bad.sum())} paths")
            for i in range(nl):
                c[f"light{i}_unoccluded"] += int((shaded & (li == i) & (occ == -1)).sum())
                c[f"light{i}_occluded"] += int((shaded & (li == i) & (occ == 1)).sum())
            for i in zero:
                c["zero_light_no_query"] += int((shaded & (li == i) & (occ == -2)).sum())
                c["zero_light_query"] += int((shaded & (li == i) & (occ != -2)).sum())
            for i in disk:
                # in the plane of the disk, met from the side its normal points to: the hit point's
                # offset along the disk's normal is zero and both ends of the shadow ray are pushed
                # off the plane by the same trace offset
                p = rec[:, 24:27].astype(np.float64) + rec[:, 27:30].astype(np.float64) * rec[:, 4:5].astype(np.float64)
                off = (p - sc.lights["p"][i, :3].astype(np.float64)) @ sc.lights["d"][i, :3].astype(np.float64)
                side = rec[:, 27:30].astype(np.float64) @ sc.lights["d"][i, :3].astype(np.float64) < 0
                flat = np.abs(sh["toWorldTransform"][s0][:, 2, 3]) + np.abs(sc.positions[sh["startVertex"][s0], 2]) == 0
                inplane = shaded & (li == i) & (np.abs(off) < 1e-5) & side & flat & (mat[s0] >= 0) & ~is_type1[s0]
                c["disk_in_plane_no_query"] += int((inplane & (occ == -2)).sum())
                if (inplane & (occ != -2)).any():
                    c["broken"].append(f"bounce {b}: {int((inplane & (occ != -2)).sum())} in-plane disk samples with a shadow query")
            # shadow rays aimed at emitter 1: the target o + tmax d, located among its triangles
            m = shaded & (occ != -2) & (li == sh["lightID"][e1])
            tgt = rec[m, 8:11].astype(np.float64) + rec[m, 14:15].astype(np.float64) * rec[m, 11:14].astype(np.float64)
            k = locate(tris1, tgt)
            if (k < 0).any():
                c["broken"].append(f"bounce {b}: {int((k < 0).sum())} shadow rays to emitter 1 end off its triangles")
            c["emitter1_triangle_rays"] += np.bincount(k[k >= 0], minlength=len(tris1))
            prev = np.where(live, bx, -1)
    return c


def required(sc, c):
    """The counts that must reach MIN_PATHS (name -> count)."""
    need = {k: c[k] for k in ("emitter_front_b0", "emitter_back_b0", "emitter1_after_specular_reflection",
                              "emitter1_after_specular_transmission", "emitter1_after_non_specular", "no_material_b0",
                              "no_material_later", "type1_b0", "type1_later", "non_area_light_id_b0",
                              "zero_light_no_query", "disk_in_plane_no_query")}
    for i in range(len(sc.lights)):
        if sc.lights["intensity"][i, :3].any():
            need[f"light{i}_unoccluded"] = c[f"light{i}_unoccluded"]
            need[f"light{i}_occluded"] = c[f"light{i}_occluded"]
    return need


def format_counts(c):
    lines = [f"{k}: {v}" for k, v in c.items() if k not in ("broken", "emitter1_triangle_rays")]
    lines.append("shadow rays per triangle of emitter 1: " + " ".join(str(int(v)) for v in c["emitter1_triangle_rays"]))
    return "\n".join(lines)


def oracle_logs(o, sampler=T.SAMPLER_RANDOM):
    """Oracle PT frames FRAMES at DEPTH with their path logs: ([radiance], [log])."""
    cam = camera()
    frames, logs = [], []
    for f in FRAMES:
        log = o.path_log(W, H, DEPTH)
        r, _ = o.render(cam, frame=f, max_depth=DEPTH, sampler=sampler)
        frames.append(r)
        logs.append(log.copy())
        o.path_log(None)
    return frames, logs
