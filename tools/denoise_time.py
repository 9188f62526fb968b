"""Times the guided a-trous denoiser on the GPU (not bench.py: a one-off measurement quoted in
DESIGN.md) and writes profiles/denoise/denoise_time.json.

1080p San-Miguel-proxy frames at 4 spp with moments, guides from mcrt_render_guides, then
mcrt_denoise_guided at its defaults (5 levels).  Per kernel, from the library's profiling events
(mcrt_ctx_kernel_stats) after --warmup untimed calls, the mean over --repeats calls:
  k_atrous_s1 .. s16   one entry per level, with the tile-staged kernel up to the default switch and
                       with MCRT_ATROUS_LDS_MAX_STEP = 0 / 4 (every level direct / staged where it
                       fits), the measurement the switch was chosen from
  k_atrous_prep, k_guides, k_moments
Each level's compulsory bytes come from the shapes: read 16 (colour) + 16 (normal-plane) + 4
(variance), write 16 + 4 per pixel, plus 16 once for the albedo-depth record; its floor is those
bytes at mcrt_ctx_stream_copy's attainable bandwidth.  Yardstick with the same 25 taps: k_denoise
(mcrt_postprocess) radius 2 on the same image, wall time of --repeats back-to-back launches.
usage: python tools/denoise_time.py [--tris N] [--repeats 50] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monte-carlo-raytracer_amd"))

LEVEL_BYTES = 16 + 16 + 4 + 16 + 4 + 16   # per pixel and level


def kernel_means(ctx, fn, warmup, repeats):
    """{kernel: mean ms per launch} over `repeats` calls of fn after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    ctx.sync()
    ctx.reset_stats()
    for _ in range(repeats):
        fn()
    ctx.sync()
    return {k: v["ms"] / v["launches"] for k, v in ctx.kernel_stats().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "denoise_time.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from mcrt import lib, scenes
    from mcrt import types as T
    from mcrt.camera import scene_camera
    W, H = a.width, a.height
    ctx = lib.Context(0)
    ds = lib.DeviceScene(ctx, scenes.san_miguel_proxy(tris=a.tris))
    fb = lib.FrameBuffer(ctx, W, H)
    cam = scene_camera("san_miguel_proxy", W, H)
    box = T.make_filter(T.BOX)
    fb.enable_moments()
    ctx.set_profiling(True)

    def frame(f):
        fb.render(ds, cam, frame=f, max_depth=2)
        fb.accumulate(box, f)

    for f in range(a.spp):   # the image the filter is timed on (and the warm-up of k_moments)
        frame(f)
    fb.render_guides(ds, cam)
    ctx.sync()
    res = {"gpu": torch.cuda.get_device_name(0), "width": W, "height": H, "triangles": a.tris, "spp": a.spp,
           "levels": a.levels, "repeats": a.repeats, "warmup": a.warmup}
    gbps = ctx.stream_copy_gbps()
    res["stream_copy_gbps"] = gbps
    level_bytes = LEVEL_BYTES * W * H
    floor_ms = level_bytes / (gbps * 1e9) * 1e3
    res["level_compulsory_bytes"] = level_bytes
    res["level_floor_ms"] = floor_ms

    ctx.reset_stats()
    for f in range(a.spp, a.spp + a.repeats):
        frame(f)
    ctx.sync()
    ks = ctx.kernel_stats()
    res["k_moments_ms"] = ks["k_moments"]["ms"] / ks["k_moments"]["launches"]
    res["k_accumulate_ms"] = ks["k_accumulate"]["ms"] / ks["k_accumulate"]["launches"]
    res["k_guides_ms"] = kernel_means(ctx, lambda: fb.render_guides(ds, cam), a.warmup, a.repeats)["k_guides"]

    names = [f"k_atrous_s{1 << i}" for i in range(a.levels)]
    for tag, env in (("default", None), ("all_direct", "0"), ("staged_to_4", "4")):
        if env is None:
            os.environ.pop("MCRT_ATROUS_LDS_MAX_STEP", None)
        else:
            os.environ["MCRT_ATROUS_LDS_MAX_STEP"] = env
        m = kernel_means(ctx, lambda: fb.denoise_guided(levels=a.levels), a.warmup, a.repeats)
        rows = [{"kernel": n, "ms": m[n], "floor_share": floor_ms / m[n]} for n in names]
        res[tag] = {"levels": rows, "k_atrous_prep_ms": m["k_atrous_prep"],
                    "total_ms": sum(r["ms"] for r in rows) + m["k_atrous_prep"]}
        print(tag, json.dumps(res[tag]), flush=True)
    os.environ.pop("MCRT_ATROUS_LDS_MAX_STEP", None)

    ctx.set_profiling(False)
    fb.postprocess(denoise=True, radius=2, sigma_spatial=1.5, sigma_range=0.3)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(a.repeats):
        fb.postprocess(denoise=True, radius=2, sigma_spatial=1.5, sigma_range=0.3)
    ctx.sync()
    # mcrt_postprocess = k_denoise + a device copy of the image into the display buffer
    res["k_denoise_r2_plus_copy_ms"] = (time.perf_counter() - t0) * 1e3 / a.repeats
    fb.close()
    ds.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
