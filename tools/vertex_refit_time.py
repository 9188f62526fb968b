"""Times mcrt_scene_update_vertices and mcrt_accel_refit on the GPU (not bench.py: a one-off
measurement quoted in DESIGN.md 2j) and writes profiles/refit/vertex_refit_time.json.

Scene: the San-Miguel proxy at each of --sizes triangles, device SAH build, every vertex deformed
(P' = P + a sin(k P.yzx + phi), as tests/vertex_refit_util.py).  Per size:

  update_host_ms / update_device_ms   mcrt_scene_update_vertices(_device), all vertices
  refit_ms                            mcrt_accel_refit, wall; refit_kernel_ms / convert_kernel_ms:
                                      its two launches (k_refit, k_qnodes_convert) by
                                      mcrt_ctx_kernel_stats
  rebuild_ms                          the baseline on the same commit: destroy + create + build
  frames                              PT frame time, 1080p, depth 2: the refitted tree against a
                                      fresh tree of the same deformed scene, at a small and a large
                                      amplitude (fractions of the scene's diagonal)

Compulsory bytes of a refit: 2n - 1 records of 64 B read and written once; of the conversion: the
records read, their offsets read, the compact records written.  Both are set against
mcrt_ctx_stream_copy's rate.  Each figure is the median of --runs runs, synchronised before and after.
usage: python tools/vertex_refit_time.py [--runs 10] [--sizes 2000000,10000000] [--out FILE]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monte-carlo-raytracer_amd"))

AMPLITUDES = {"small": 0.001, "large": 0.02}   # of the scene's diagonal


def median_ms(ctx, fn, runs):
    ts = []
    for k in range(runs + 1):   # one untimed run first
        ctx.sync()
        t0 = time.perf_counter()
        fn(k)
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:]))


def deform(P, a, k=1.7, phi=0.3):
    out = P.copy()
    q = P[:, :3].astype(np.float64)
    out[:, :3] = (q + a * np.sin(k * q[:, [1, 2, 0]] + phi)).astype(np.float32)
    return out


def with_positions(scene, P):
    sc = copy.copy(scene)
    sc.positions = P
    sc._desc = None
    return sc


def frame_ms(ctx, lib, ds, cam, runs):
    fb = lib.FrameBuffer(ctx, 1920, 1080)
    ms = median_ms(ctx, lambda k: fb.render(ds, cam, frame=k, max_depth=2), runs)
    fb.close()
    return ms


def case(ctx, lib, scenes, scene_camera, tris, runs, copy_gbps):
    import torch
    sc = scenes.san_miguel_proxy(tris=tris)
    lo, hi = sc.bbox()
    diag = float(np.linalg.norm(hi - lo))
    variants = {k: deform(sc.positions, f * diag) for k, f in AMPLITUDES.items()}
    ds = lib.DeviceScene(ctx, sc)
    info = ds.info()
    built = ds.records()
    n = int(info["nodes"])
    row = {"triangles": int(info["triangles"]), "vertices": int(len(sc.positions)), "records": n,
           "structure_bytes": int(info["bytes"]), "build_ms": info["build_ms"], "diagonal": diag}
    cycle = [variants["small"], sc.positions]
    row["update_host_ms"] = median_ms(ctx, lambda k: ds.update_vertices(cycle[k % 2]), runs)
    dev = [torch.from_numpy(p).cuda() for p in cycle]
    torch.cuda.synchronize()
    row["update_device_ms"] = median_ms(ctx, lambda k: ds.update_vertices(dev[k % 2].data_ptr(), count=len(sc.positions)), runs)
    del dev
    ds.refit()   # the structure's first refit allocates: not timed

    def refit(k):
        ds.update_vertices(cycle[k % 2])
        ctx.sync()
        t0 = time.perf_counter()
        ds.refit()
        ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
    walls = []
    ctx.set_profiling(True)
    ctx.reset_stats()
    for k in range(runs):
        refit(k)
    stats = ctx.kernel_stats()
    ctx.set_profiling(False)
    assert ds.update_info()["path"] == 4 and ds.info()["bytes"] == info["bytes"]
    row["refit_ms"] = float(np.median(walls))
    row["refit_kernel_ms"] = stats["k_refit"]["ms"] / stats["k_refit"]["launches"]
    row["convert_kernel_ms"] = stats["k_refit_qnodes"]["ms"] / stats["k_refit_qnodes"]["launches"]
    refit_bytes = 2 * 64 * n
    convert_bytes = 64 * n + 4 * n + (info["bytes"] - 64 * n)
    row["refit_compulsory_bytes"] = refit_bytes
    row["convert_compulsory_bytes"] = int(convert_bytes)
    row["refit_gbps"] = refit_bytes / row["refit_kernel_ms"] / 1e6
    row["convert_gbps"] = convert_bytes / row["convert_kernel_ms"] / 1e6
    row["refit_share_of_stream_copy"] = row["refit_gbps"] / copy_gbps
    row["convert_share_of_stream_copy"] = row["convert_gbps"] / copy_gbps
    # quality: the refitted tree against a fresh one of the same deformed scene
    cam = scene_camera("san_miguel_proxy", 1920, 1080)
    row["frames"] = {"undeformed_ms": None}
    ds.update_vertices(sc.positions)
    ds.refit()
    # deformed and restored 2 x runs times by now: the records must be the build's again, word for word
    row["restored_records_equal_the_builds"] = bool(np.array_equal(ds.records().view(np.uint32), built.view(np.uint32)))
    del built
    row["frames"]["undeformed_ms"] = frame_ms(ctx, lib, ds, cam, runs)
    for name, P in variants.items():
        ds.update_vertices(P)
        ds.refit()
        refitted = frame_ms(ctx, lib, ds, cam, runs)
        fresh = lib.DeviceScene(ctx, with_positions(sc, P))
        row["frames"][name] = {"amplitude": AMPLITUDES[name] * diag, "refitted_ms": refitted,
                               "fresh_ms": frame_ms(ctx, lib, fresh, cam, runs)}
        row["frames"][name]["refitted_over_fresh"] = refitted / row["frames"][name]["fresh_ms"]
        fresh.close()
    # the baseline: what a host without the refit does per deformation
    state = {"ds": ds}

    def rebuild(k):
        state["ds"].close()
        state["ds"] = lib.DeviceScene(ctx, with_positions(sc, cycle[k % 2]))
    row["rebuild_ms"] = median_ms(ctx, rebuild, max(3, runs // 3))
    row["rebuild_over_update_and_refit"] = row["rebuild_ms"] / (row["update_host_ms"] + row["refit_ms"])
    state["ds"].close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sizes", default="2000000,10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit", "vertex_refit_time.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from mcrt import lib, scenes
    from mcrt.camera import scene_camera
    ctx = lib.Context(0)
    copy_gbps = ctx.stream_copy_gbps()
    res = {"gpu": torch.cuda.get_device_name(0), "runs": a.runs, "stream_copy_gbps": copy_gbps,
           "amplitudes_of_diagonal": AMPLITUDES, "cases": []}
    for tris in [int(x) for x in a.sizes.split(",")]:
        row = case(ctx, lib, scenes, scene_camera, tris, a.runs, copy_gbps)
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
