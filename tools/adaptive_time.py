"""Times adaptive sampling on the GPU (not bench.py: one-off measurements quoted in DESIGN.md 2i)
and writes profiles/adaptive/adaptive_time.json.

  listed calls   San-Miguel proxy, 1080p, depth 2, calls of 16 frames (mcrt_render_frames +
                 mcrt_accumulate_frames, two frames in flight): wall time per call between two
                 synchronisations over --repeats back-to-back calls, with the mode off and with all,
                 half (a checkerboard) and a quarter (the top-left quadrant) of the tiles listed; per
                 kernel, ms and ns per item from the library's profiling events over 5 more calls
                 with one frame in flight, which shows whether the extension launch of a
                 checkerboard loses coherence.  --plain-only times only
                 the mode-off call (run it with MCRT_LIB_PATH on the parent commit's library and
                 hand the file to --parent: the yardstick).
  the update     mcrt_adaptive_update (k_tile_error + k_tile_list + the 4-byte read-back) on
                 installed moments at 1080p and 4K: wall time per call and the kernels' means; the
                 compulsory traffic is the 8 B per pixel of moments, stated against
                 mcrt_ctx_stream_copy's rate.
  equal quality  960x544, rounds of 16 frames: frames x tiles rendered until the list is empty at
                 one threshold (a multiple of the median tile error after the first round), against
                 the uniform run carried to the same worst-tile error: the threshold, or the adaptive
                 run's own worst tile where that one stopped at --max-samples.
usage: python tools/adaptive_time.py [--tris N] [--repeats 10] [--plain-only] [--parent FILE] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monte-carlo-raytracer_amd"))

BATCH = 16


def tile_lists(W, H):
    tx, ty = (W + 7) // 8, (H + 7) // 8
    t = np.arange(tx * ty)
    x, y = t % tx, t // tx
    return {"all": t, "half_checkerboard": t[(x + y) % 2 == 0], "quarter_quadrant": t[(x < tx // 2) & (y < ty // 2)]}


def timed_calls(ctx, fb, ds, cams, filts, first_frame, repeats, profile):
    """`repeats` calls of BATCH frames: wall ms per call and, with profile, the kernels' stats."""
    def call(f):
        fb.render_frames(ds, cams, frame=f, max_depth=2)
        fb.accumulate_frames(filts, f)

    f = first_frame
    for _ in range(2):   # warm-up
        call(f)
        f += BATCH
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(repeats):
        call(f)
        f += BATCH
    ctx.sync()
    res = {"ms_per_call": (time.perf_counter() - t0) * 1e3 / repeats}
    if profile:   # one frame in flight, so that no two calls' kernels share the GPU while they are timed
        fb.set_frames_in_flight(1)
        ctx.set_profiling(True)
        ctx.reset_stats()
        for _ in range(5):
            call(f)
            f += BATCH
        ctx.sync()
        fb.set_frames_in_flight(0)
        res["kernels"] = {k: {"ms": v["ms"] / v["launches"], "ns_per_item": 1e6 * v["ms"] / max(v["items"], 1)}
                          for k, v in ctx.kernel_stats().items()}
        ctx.set_profiling(False)
        ctx.reset_stats()
    return res, f


def listed_calls(ctx, ds, a, plain_only):
    from mcrt import lib
    from mcrt import types as T
    from mcrt.camera import scene_camera
    W, H = a.width, a.height
    cams = [scene_camera("san_miguel_proxy", W, H, frame=k, jitter=True) for k in range(BATCH)]
    filts = [T.make_filter(T.BOX)] * BATCH
    out = {"width": W, "height": H, "frames_per_call": BATCH, "repeats": a.repeats}
    fb = lib.FrameBuffer(ctx, W, H)
    res, f = timed_calls(ctx, fb, ds, cams, filts, 0, a.repeats, not plain_only)
    out["mode_off"] = res
    print("mode off", json.dumps(res["ms_per_call"]), flush=True)
    fb.close()
    if plain_only:
        return out
    fb = lib.FrameBuffer(ctx, W, H)
    fb.set_adaptive(error_threshold=0.0, min_samples=1 << 30)
    f = 0
    for name, ids in tile_lists(W, H).items():
        if name != "all":   # (frame 0 needs the full list, which the first case renders)
            fb.set_active_tiles(ids)
        res, f = timed_calls(ctx, fb, ds, cams, filts, f, a.repeats, True)
        res["tiles"] = int(len(ids))
        res["over_mode_off"] = res["ms_per_call"] / out["mode_off"]["ms_per_call"]
        out[name] = res
        print(name, len(ids), json.dumps(res["ms_per_call"]), flush=True)
    fb.close()
    return out


def update_time(ctx, a, gbps):
    import torch
    from mcrt import lib
    out = {}
    for W, H in ((1920, 1080), (3840, 2160)):
        fb = lib.FrameBuffer(ctx, W, H)
        rng = np.random.default_rng(W)
        m1 = (6 * rng.uniform(0.5, 3.0, (H, W))).astype(np.float32)
        mom = np.stack([m1, m1 * m1 / 6 + 6 * rng.uniform(0.0, 0.5, (H, W)).astype(np.float32)], -1).astype(np.float32)
        fb.set_adaptive(error_threshold=0.15, min_samples=2)
        dev = torch.from_numpy(mom.reshape(-1)).cuda()
        fb.set_moments(dev.data_ptr(), 6)
        for _ in range(3):
            n = fb.adaptive_update()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.repeats * 5):
            fb.adaptive_update()
        wall = (time.perf_counter() - t0) * 1e3 / (a.repeats * 5)
        ctx.set_profiling(True)
        ctx.reset_stats()
        for _ in range(a.repeats * 5):
            fb.adaptive_update()
        ks = {k: v["ms"] / v["launches"] for k, v in ctx.kernel_stats().items()}
        ctx.set_profiling(False)
        ctx.reset_stats()
        floor = 8.0 * W * H / (gbps * 1e9) * 1e3
        out[f"{W}x{H}"] = {"tiles": ((W + 7) // 8) * ((H + 7) // 8), "active": n, "update_wall_ms": wall,
                           "k_tile_error_ms": ks["k_tile_error"], "k_tile_list_ms": ks["k_tile_list"],
                           "moments_bytes": 8 * W * H, "moments_floor_ms": floor,
                           "k_tile_error_floor_share": floor / ks["k_tile_error"]}
        print(f"{W}x{H}", json.dumps(out[f"{W}x{H}"]), flush=True)
        fb.close()
    return out


def equal_quality(ctx, ds, a):
    from mcrt import lib
    from mcrt import types as T
    from mcrt.camera import scene_camera
    W, H, R = 960, 544, 16
    cam = scene_camera("san_miguel_proxy", W, H)
    filts = [T.make_filter(T.BOX)] * R
    tiles = ((W + 7) // 8) * ((H + 7) // 8)

    def run(adaptive, thr):
        fb = lib.FrameBuffer(ctx, W, H)
        # uniform: nobody is ever judged, every tile stays listed
        fb.set_adaptive(error_threshold=thr if adaptive else 0.0, min_samples=R if adaptive else 1 << 30,
                        max_samples=a.max_samples if adaptive else 0)
        f, listed, cost, errs = 0, tiles, 0, None
        first = None
        while f < a.max_samples:
            fb.render_frames(ds, [cam] * R, frame=f, max_depth=2)
            fb.accumulate_frames(filts, f)
            f += R
            cost += listed * R
            listed = fb.adaptive_update()
            errs = fb.read_adaptive(T.ADAPTIVE_TILE_ERROR)
            if first is None:
                first = errs.copy()
            if thr is None or (adaptive and listed == 0) or (not adaptive and errs.max() <= thr):
                break
        counts = fb.read_adaptive(T.ADAPTIVE_TILE_SAMPLES)
        fb.close()
        return dict(frames=f, tile_frames=cost, worst_error=float(errs.max()), first=first, counts=counts)

    probe = run(False, None)   # the first round's errors choose the threshold
    thr = float(a.threshold_scale * np.median(probe["first"]))
    ad = run(True, thr)
    target = max(thr, ad["worst_error"])
    un = run(False, target)
    c = ad["counts"]
    out = {"width": W, "height": H, "tiles": tiles, "round_frames": R, "max_samples": a.max_samples,
           "threshold": thr, "threshold_rule": f"{a.threshold_scale} x the median tile error after {R} frames",
           "errors_after_first_round": {"min": float(probe["first"].min()), "median": float(np.median(probe["first"])),
                                        "max": float(probe["first"].max())},
           "adaptive": {"rounds_frames": ad["frames"], "tile_frames": ad["tile_frames"], "worst_error": ad["worst_error"],
                        "tile_samples": {"min": int(c.min()), "median": float(np.median(c)), "max": int(c.max())},
                        "tiles_at_cap": int((c >= a.max_samples).sum())},
           "uniform": {"frames": un["frames"], "tile_frames": un["tile_frames"], "worst_error": un["worst_error"],
                       "target_error": target, "reached": bool(un["worst_error"] <= target)}}
    out["adaptive_over_uniform"] = ad["tile_frames"] / un["tile_frames"]
    print("equal quality", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--max-samples", type=int, default=1024)
    ap.add_argument("--threshold-scale", type=float, default=1.0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent", default=None, help="the --plain-only output of the parent commit's library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "adaptive_time.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from mcrt import lib, scenes
    ctx = lib.Context(0)
    ds = lib.DeviceScene(ctx, scenes.san_miguel_proxy(tris=a.tris))
    res = {"gpu": torch.cuda.get_device_name(0), "triangles": a.tris}
    res["listed_calls"] = listed_calls(ctx, ds, a, a.plain_only)
    if not a.plain_only:
        if a.parent:
            with open(a.parent) as f:
                parent = json.load(f)["listed_calls"]["mode_off"]["ms_per_call"]
            res["listed_calls"]["parent_full_call_ms"] = parent
            for k in ("mode_off", "all", "half_checkerboard", "quarter_quadrant"):
                res["listed_calls"][k]["over_parent"] = res["listed_calls"][k]["ms_per_call"] / parent
        res["stream_copy_gbps"] = ctx.stream_copy_gbps()
        res["update"] = update_time(ctx, a, res["stream_copy_gbps"])
        res["equal_quality"] = equal_quality(ctx, ds, a)
    ds.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
