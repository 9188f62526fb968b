"""Times mcrt_accel_update_transforms on the GPU (not bench.py: a one-off measurement quoted in
DESIGN.md) and writes profiles/refit/refit_time.json.

1. Refit against full rebuild: instanced_proxy() at its defaults, one instance moved.  Baseline:
   mcrt_scene_update_shapes + mcrt_accel_build.  Against: mcrt_accel_update_transforms with the top
   level built on the host and on the device (MCRT_TOP_BUILD, set between calls: the library reads
   it at every update).
2. Device against host top build: synthetic top levels of single-triangle instances; "threshold" is
   the smallest measured count at which the device path wins (MCRT_TOP_DEVICE_MIN_SHAPES in
   csrc/mcrt_accel.cpp).

Each figure is the median of --runs runs, synchronised before and after.
usage: python tools/refit_time.py [--runs 10] [--sizes 1000,10000,100000,1000000] [--out FILE]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monte-carlo-raytracer_amd"))


def median_ms(ctx, fn, runs):
    ts = []
    for k in range(runs + 1):   # one untimed run first
        ctx.sync()
        t0 = time.perf_counter()
        fn(k)
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:]))


def translated(shapes, k, t):
    s = shapes.copy()
    M = s["toWorldTransform"][k].copy()
    M[:3, 3] += np.asarray(t, np.float32)
    s["toWorldTransform"][k] = M
    s["toWorldInverseTranspose"][k] = np.linalg.inv(M.astype(np.float64)).T.astype(np.float32)
    return s


def timed_update(ctx, ds, variants, mode, runs):
    os.environ["MCRT_TOP_BUILD"] = mode
    ms = median_ms(ctx, lambda k: ds.update_transforms(variants[k % 2]), runs)
    path = ds.update_info()["path"]
    del os.environ["MCRT_TOP_BUILD"]
    assert path == {"device": 1, "host": 2}[mode], (mode, path)
    return ms


def proxy_case(ctx, lib, scenes, runs):
    sc = scenes.instanced_proxy()
    variants = [translated(sc.shapes, 5, (0.4, 0.0, -0.3)), sc.shapes]
    ds = lib.DeviceScene(ctx, sc)

    def rebuild(k):
        ds.update_shapes(variants[k % 2])
        ds.build()
    out = {"shapes": len(sc.shapes), "triangles_effective": int(ds.info()["triangles"]),
           "rebuild_ms": median_ms(ctx, rebuild, runs)}
    for mode in ("host", "device"):
        out[f"{mode}_ms"] = timed_update(ctx, ds, variants, mode, runs)
        out[f"rebuild_over_{mode}"] = out["rebuild_ms"] / out[f"{mode}_ms"]
    ds.close()
    return out


def top_level_scene(scenes, n, seed):
    """n single-triangle shapes (one mesh + n - 1 instances), translated over a cube."""
    b = scenes.SceneBuilder(f"top_{n}")
    m = b.add_material(kd=(0.7, 0.7, 0.7))
    tri = b.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.tile([0, 0, 1], (3, 1)),
                     np.zeros((3, 2)), np.array([[0, 1, 2]]), m)
    b.add_instance(tri, np.eye(4, dtype=np.float32))
    sc = b.build()
    sc = copy.copy(sc)
    sc._desc = None
    sc.shapes = np.repeat(sc.shapes[1:2], n)
    place(sc.shapes, n, seed)
    return sc


def place(shapes, n, seed):
    t = np.random.default_rng(seed).uniform(0.0, 2.0 * n ** (1.0 / 3.0), (n, 3)).astype(np.float32)
    M = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    Mi = M.copy()
    M[:, :3, 3] = t
    Mi[:, 3, :3] = -t   # transpose of the inverse translation
    shapes["toWorldTransform"] = M
    shapes["toWorldInverseTranspose"] = Mi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sizes", default="1000,10000,100000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit", "refit_time.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from mcrt import lib, scenes
    ctx = lib.Context(0)
    res = {"gpu": torch.cuda.get_device_name(0), "runs": a.runs, "proxy": proxy_case(ctx, lib, scenes, a.runs),
           "top_levels": [], "threshold": None}
    print(json.dumps(res["proxy"]), flush=True)
    for n in [int(x) for x in a.sizes.split(",")]:
        sc = top_level_scene(scenes, n, 1)
        moved = sc.shapes.copy()
        place(moved, n, 2)
        ds = lib.DeviceScene(ctx, sc, force_2level=True)
        row = {"instances": n}
        for mode in ("host", "device"):
            row[f"{mode}_ms"] = timed_update(ctx, ds, [moved, sc.shapes], mode, a.runs)
        row["host_over_device"] = row["host_ms"] / row["device_ms"]
        ds.close()
        res["top_levels"].append(row)
        print(json.dumps(row), flush=True)
        if res["threshold"] is None and row["device_ms"] < row["host_ms"]:
            res["threshold"] = n
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
