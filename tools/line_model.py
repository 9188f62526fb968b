"""128-B line misses of the compact BVH records under three record orders (analysis tool, CPU).

Builds the San-Miguel proxy's tree with the oracle, traces camera rays in 8x8 tile order and one
diffuse bounce from their hits (tools/trav_sim.py's rays), keeps every ray's visit sequence, and
replays waves of 64 rays in queue order through a model of one CU's L1 (tools/line_model.c): an
LRU of 256 lines (32 KB) shared by 32 resident waves (8 per SIMD) that take turns one loop step
at a time; each of CUS model CUs walks a contiguous run of the queue.  The extension queue is the
camera hits' compacted order with each run of 512 rays grouped by octant x dominant axis, as
k_shade0 appends them.  Reports line misses per record visit for
  (a) dfs       the 64-B tree's depth-first order (32-B internal, 48-B leaf records back to back),
  (b) siblings  the two children of a node in one line,
  (c) treelets  a node and both its children in one line, pairs of treelets depth-first
and the compact copy's size in each order.

Usage: python tools/line_model.py [tris] [W] [H] [out.json]
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "monte-carlo-raytracer_amd"), os.path.join(ROOT, "tools")]
from mcrt import scenes  # noqa: E402
from mcrt.camera import scene_camera  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from trav_sim import bounce_rays, camera_rays  # noqa: E402

ORDERS = ("dfs", "siblings", "treelets")
CUS, SLOTS, LINES = 16, 32, 256


def lib():
    so = os.path.join(tempfile.gettempdir(), "line_model.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tools", "line_model.c"), "-o", so, "-lm"],
                   check=True)
    L = ctypes.CDLL(so)
    L.visit_seq.restype = ctypes.c_int64
    L.visit_seq.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.layout.restype = ctypes.c_uint64
    L.layout.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    L.lru_misses.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p] + \
        [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return L


def sequences(L, nodes, rays):
    n = len(rays)
    start = np.zeros(n + 1, np.int64)
    ht = np.zeros(n, np.float32)
    hn = np.zeros(n, np.int32)
    tot = L.visit_seq(nodes.ctypes.data, rays.ctypes.data, n, None, start.ctypes.data, ht.ctypes.data, hn.ctypes.data)
    seq = np.zeros(max(tot, 1), np.uint32)
    L.visit_seq(nodes.ctypes.data, rays.ctypes.data, n, seq.ctypes.data, start.ctypes.data, ht.ctypes.data, hn.ctypes.data)
    return seq, start, ht, hn


def queue_order(rays):
    """The extension queue: live rays only, each run of 512 grouped by octant x dominant axis."""
    live = np.flatnonzero(rays["extra"][:, 1] != 0)
    d = rays["d"][live, :3]
    octant = (d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4
    group = octant * 3 + np.abs(d).argmax(1)
    key = (np.arange(len(live)) // 512) * 24 + group
    return rays[live[np.argsort(key, kind="stable")]]


def replay(L, nodes, off, size, seq, start, nrays):
    waves = (nrays + 63) // 64
    out = np.zeros(4, np.int64)
    for cu in range(CUS):
        w0, w1 = waves * cu // CUS, waves * (cu + 1) // CUS
        L.lru_misses(nodes.ctypes.data, off.ctypes.data, size, seq.ctypes.data, start.ctypes.data, nrays, w0, w1, SLOTS,
                     LINES, out.ctypes.data)
    return {"visits": int(out[0]), "line_misses": int(out[1]), "line_accesses": int(out[2]),
            "misses_per_visit": round(float(out[1]) / max(int(out[0]), 1), 4)}


def main():
    tris = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 480
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 272
    t0 = time.time()
    sc = scenes.san_miguel_proxy(tris=tris)
    o = po.OracleScene(sc)
    o.build()
    nodes = o.nodes()
    print(f"scene {sc.num_triangles} tris, {len(nodes)} nodes, {time.time() - t0:.1f}s", flush=True)
    L = lib()
    cam = scene_camera("san_miguel_proxy", W, H)
    layouts = {}
    for k, name in enumerate(ORDERS):
        off = np.zeros(len(nodes), np.uint64)
        size = L.layout(nodes.ctypes.data, len(nodes), k, off.ctypes.data)
        layouts[name] = (off, int(size))
    res = {"scene": sc.name, "triangles": int(sc.num_triangles), "nodes": int(len(nodes)), "image": [W, H],
           "model": {"cus": CUS, "resident_waves": SLOTS, "l1_lines": LINES, "line_bytes": 128,
                     "interleaving": "resident waves take turns, one lock-step loop step each; LRU, fully associative"},
           "bytes": {name: layouts[name][1] for name in ORDERS}, "classes": {}}
    rays = camera_rays(cam, W, H)
    for cls in ("camera", "extension"):
        seq, start, ht, hn = sequences(L, nodes, rays)
        res["classes"][cls] = {"rays": int(len(rays))}
        for name in ORDERS:
            r = replay(L, nodes, layouts[name][0], layouts[name][1], seq, start, len(rays))
            res["classes"][cls][name] = r
            print(f"{cls:10s} {name:9s} visits/ray {r['visits'] / len(rays):6.1f} misses/visit {r['misses_per_visit']:.4f}",
                  flush=True)
        if cls == "camera":
            rays = queue_order(bounce_rays(nodes, rays, ht, hn, np.random.default_rng(1)))
    ext = res["classes"]["extension"]
    res["fewest_misses"] = min(ORDERS, key=lambda k: ext[k]["line_misses"])
    print(json.dumps(res["bytes"]), "fewest:", res["fewest_misses"], f"{time.time() - t0:.0f}s")
    if len(sys.argv) > 4:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
        with open(sys.argv[4], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
