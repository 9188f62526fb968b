"""Times the per-object-motion kernels on the GPU against the kernels they extend (not bench.py: a
one-off measurement quoted in DESIGN.md 2h) and writes profiles/denoise/temporal_motion_time.json.

The setup of tools/temporal_time.py: a 1080p San-Miguel-proxy frame at 1 spp, full history (the same
camera every call), per-kernel means from the library's profiling events (mcrt_ctx_kernel_stats).
Two states of the scene: nothing moved since the snapshot (every motion record static) and every
shape translated by 0.01 units since the snapshot (every hit pixel moved; the history still matches).
  k_guides vs k_guides_motion        alternating calls, static and moved
  k_temporal vs k_temporal_motion    alternating calls, static and moved, both load forms
Every comparison runs --rounds alternating blocks of --repeats calls after --warmup untimed calls;
the figure is the mean over the blocks and the spread their (max - min) / mean.
Compulsory bytes per pixel: k_temporal 144 (tools/temporal_time.py), k_temporal_motion 160 static
(+ the motion record) and 176 moved (+ the previous normal); k_guides_motion writes 32 more than
k_guides.  Floors are those bytes at mcrt_ctx_stream_copy's rate of this run.
usage: python tools/temporal_motion_time.py [--tris N] [--repeats 50] [--warmup 5] [--rounds 3] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monte-carlo-raytracer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from denoise_time import kernel_means   # noqa: E402

BYTES = {"k_temporal": 144, "k_temporal_motion_static": 160, "k_temporal_motion_moved": 176, "guides_added": 32}


def blocks(ctx, variants, warmup, repeats, rounds):
    """variants: {tag: (fn, [kernel names])}.  Alternating blocks; {tag: {kernel: {ms, spread}}}."""
    means = {tag: {k: [] for k in names} for tag, (_, names) in variants.items()}
    for r in range(rounds):
        for tag, (fn, names) in variants.items():
            m = kernel_means(ctx, fn, warmup if r == 0 else 1, repeats)
            for k in names:
                means[tag][k].append(m[k])
    out = {}
    for tag, per in means.items():
        out[tag] = {}
        for k, v in per.items():
            mean = sum(v) / len(v)
            out[tag][k] = {"ms": mean, "spread": (max(v) - min(v)) / mean, "blocks": v}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "temporal_motion_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from mcrt import lib, scenes
    from mcrt import types as T
    from mcrt.camera import scene_camera
    W, H = a.width, a.height
    ctx = lib.Context(0)
    sc = scenes.san_miguel_proxy(tris=a.tris)
    ds = lib.DeviceScene(ctx, sc)
    fb = lib.FrameBuffer(ctx, W, H)
    cam = scene_camera("san_miguel_proxy", W, H)
    fb.render(ds, cam, frame=0, max_depth=2)
    fb.accumulate(T.make_filter(T.BOX), 0)
    ctx.sync()
    ctx.set_profiling(True)
    res = {"gpu": torch.cuda.get_device_name(0), "width": W, "height": H, "triangles": a.tris, "repeats": a.repeats,
           "warmup": a.warmup, "rounds": a.rounds, "bytes_per_pixel": BYTES}
    gbps = ctx.stream_copy_gbps()
    res["stream_copy_gbps"] = gbps
    res["floor_ms"] = {k: b * W * H / (gbps * 1e9) * 1e3 for k, b in BYTES.items()}
    moved_shapes = sc.shapes.copy()
    moved_shapes["toWorldTransform"][:, 0, 3] += np.float32(0.01)

    for state in ("static", "moved"):
        ds.motion_snapshot()
        if state == "moved":
            ds.update_transforms(moved_shapes)
        fb.render_guides_motion(ds, cam)
        flag = fb.read_motion(0)[..., 3]
        hit = fb.read_guides(T.GUIDE_ALBEDO_DEPTH)[..., 3] > 0
        res[f"{state}_hit_fraction"] = float(hit.mean())
        res[f"{state}_moved_fraction"] = float((flag == 1).mean())
        assert ((flag == 1) == (hit if state == "moved" else np.zeros_like(hit))).all()
        row = blocks(ctx, {"k_guides": (lambda: fb.render_guides(ds, cam), ["k_guides"]),
                           "k_guides_motion": (lambda: fb.render_guides_motion(ds, cam), ["k_guides_motion"])},
                     a.warmup, a.repeats, a.rounds)
        res[f"guides_{state}"] = row
        print("guides", state, json.dumps(row), flush=True)
        fb.render_guides_motion(ds, cam)
        for loads in ("lazy", "eager"):
            os.environ["MCRT_TEMPORAL_LOADS"] = loads
            variants = {"k_temporal": (lambda: fb.temporal_accumulate(cam), ["k_temporal", "k_temporal_var"]),
                        "k_temporal_motion": (lambda: fb.temporal_accumulate_motion(cam),
                                              ["k_temporal_motion", "k_temporal_var"])}
            row = blocks(ctx, variants, a.warmup, a.repeats, a.rounds)
            base = row["k_temporal"]["k_temporal"]["ms"]
            for tag, per in row.items():
                per["over_k_temporal"] = per.get("k_temporal_motion", per.get("k_temporal"))["ms"] / base - 1.0
            res[f"temporal_{state}_{loads}"] = row
            print("temporal", state, loads, json.dumps(row), flush=True)
            N = fb.read_temporal(T.TEMPORAL_MOMENTS)[..., 2]
            res[f"temporal_{state}_{loads}_full_history_fraction"] = float((N[hit] > 1).mean())
    os.environ.pop("MCRT_TEMPORAL_LOADS", None)
    fb.close()
    ds.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
