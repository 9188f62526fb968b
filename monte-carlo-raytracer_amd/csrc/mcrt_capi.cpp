// mcrt_capi.cpp -- host runtime behind include/mcrt_capi.h: the context, and the helpers the other
// host files share (mcrt_host.h): the error text, the device flags, the environment's knobs, the
// frame slots' synchronisation, the frame arguments and DevBuf's way to the device.  Everything else
// has a file of its own: the scene tables (mcrt_scene.hip), the ray queries (mcrt_query.hip), the AOV
// pass (mcrt_aov.hip), the integrators' drivers (mcrt_pt_host.cpp, mcrt_bdpt_host.cpp), the frame
// buffer's planes (mcrt_film.hip), the roofline probes (mcrt_probe.hip).
//
// Replaces the reference's OpenCL host plumbing (PlatformManager / KernelManager /
// RTBufferManager, RTScene uploads, RadeonRays IntersectionApi, and the per-pass
// launch + clFinish sequence of RTPrimaryRaysPass / RTPathTracingPass /
// RTReconstructionPass) with: one HIP stream per context, all per-frame work enqueued
// without host synchronisation (queue sizes stay on the device), one memset per frame.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "mcrt_bands.h"
#include "mcrt_host.h"

namespace {

thread_local std::string g_lastError;
}  // namespace
namespace mcrt {
void set_last_error(const std::string& msg) { g_lastError = msg; }
// DevBuf's three ways to the device (mcrt_devbuf.h)
int dev_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
void dev_free(void* p) { (void)hipFree(p); }
int dev_sync(void* stream) { return (int)hipStreamSynchronize((hipStream_t)stream); }
}  // namespace mcrt
// the helpers mcrt_host.h declares for other host files; defined below among the file's own
using mcrt::fail, mcrt::env_int;
namespace {

const char* kKernelNames[K_COUNT] = {"k_primary",    "k_shade0",      "k_shadeN",       "k_shadow",   "k_extend",
                                     "k_accumulate", "k_trace_closest", "k_trace_any",  "k_bdpt_start",
                                     "k_bdpt_vertex", "k_bdpt_connect", "k_bdpt_vis",   "k_bdpt_gather",
                                     "k_shadow_extend", "k_guides",      "k_moments",    "k_atrous_prep",
                                     "k_atrous_s1",   "k_atrous_s2",   "k_atrous_s4",  "k_atrous_s8",
                                     "k_atrous_s16",  "k_atrous_s32",  "k_atrous_s64", "k_atrous_s128",
                                     "k_temporal",    "k_temporal_var", "k_guides_motion", "k_temporal_motion",
                                     "k_tile_error",  "k_tile_list",   "k_refit",      "k_refit_qnodes"};

}  // namespace

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------
mcrt_status mcrt::fail(mcrt_ctx ctx, mcrt_status code, const std::string& msg) {
    g_lastError = msg;
    if (ctx) ctx->error = msg;
    return code;
}

// Device-side error flags raised by kernels since the last check (call after a synchronisation):
// a traversal whose stack needed more entries than its spill column holds drops entries
// (mcrt_traverse.h), so its hits may be wrong -- reported, never silent.
mcrt_status mcrt::check_device_flags(mcrt_ctx ctx) {
    int f = 0;
    HIPCHK(ctx, hipMemcpy(&f, ctx->dFlags, sizeof(int), hipMemcpyDeviceToHost));
    if (f != 0) {
        HIPCHK(ctx, hipMemset(ctx->dFlags, 0, sizeof(int)));
        return fail(ctx, MCRT_ERROR_DEVICE,
                    "traversal stack overflow: a ray needed more stack entries than its spill column holds "
                    "(results of the affected launches are unreliable)");
    }
    return MCRT_OK;
}

static void drain_pending(mcrt_ctx ctx) {
    if (ctx->pending.empty()) return;
    for (auto& p : ctx->pending) {
        hipEventSynchronize(p.b);   // events may sit on frame-slot streams
        float ms = 0.0f;
        hipEventElapsedTime(&ms, p.a, p.b);
        ctx->totalMs[p.kernel] += ms;
        ctx->launches[p.kernel] += 1;
        int64_t it = p.items;
        if (p.countDev) {
            int v = 0, v2 = 0;
            hipMemcpy(&v, p.countDev, sizeof(int), hipMemcpyDeviceToHost);
            if (p.countDev2) hipMemcpy(&v2, p.countDev2, sizeof(int), hipMemcpyDeviceToHost);
            it = (int64_t)v + v2;
        }
        ctx->items[p.kernel] += it;
        hipEventDestroy(p.a);
        hipEventDestroy(p.b);
    }
    ctx->pending.clear();
}

int mcrt::env_int(const char* name, int def, int lo, int hi) {
    const char* e = std::getenv(name);
    return e ? (int)std::min<long>(hi, std::max<long>(lo, std::strtol(e, nullptr, 10))) : def;
}

// Stop rule of the extension rays' compact walks (TraceCtx::walkCap / walkLanes): a wave stops
// once it has taken MCRT_WALK_CAP steps (0 = never) and MCRT_WALK_LANES of its lanes or fewer are
// still walking (64: a fixed step limit).  Default 60 / 8: k_shadow_extend 0.643 -> 0.603 ms per
// frame on the headline (a fixed 130-step limit 0.609; profiles/r05/ab/README.txt item 20)
static int walk_cap() { return env_int("MCRT_WALK_CAP", 60, 0); }
// ... and only for calls of at least MCRT_WALK_MIN_PATHS paths (default 16 M): a rank's share of a
// strong-scaled frame (N = 8: 5 M paths per call) finishes the resumed walks in a launch too small
// to hide their tail (emulated N = 8 rank 0.175 -> 0.179 ms per frame with the rule; BDPT 0.649 ->
// 0.659).  The tests set it to 0 to run the rule on small frames.
static int64_t walk_min_paths() { return env_int("MCRT_WALK_MIN_PATHS", 16000000); }
static int walk_lanes() { return env_int("MCRT_WALK_LANES", 8, 0, 64); }

hipError_t mcrt::walk_rule(TraceCtx& c, int64_t paths, DevBuf<float4>& suspend, DevBuf<int>& suspended, int counts,
                           size_t entries, hipStream_t st) {
    const int wcap = c.qnodes && !c.twoLevel && paths >= walk_min_paths() ? walk_cap() : 0;
    if (wcap <= 0) return hipSuccess;
    hipError_t e = (hipError_t)suspend.grow(MCRT_SUSPEND_F4 * entries, st);
    if (e == hipSuccess && !suspended) e = (hipError_t)suspended.alloc(counts);
    if (e == hipSuccess) e = hipMemsetAsync(suspended.get(), 0, counts * sizeof(int), st);
    if (e != hipSuccess) return e;
    c.walkCap = wcap;
    c.walkLanes = walk_lanes();
    c.suspend = suspend.get();
    return hipSuccess;
}

hipError_t mcrt::fb_sync(mcrt_framebuffer fb) {
    hipError_t e = hipSuccess;
    for (auto& k : fb->slot)
        if (k.stream && e == hipSuccess) e = hipStreamSynchronize(k.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(fb->ctx->stream);
    return e;
}

void mcrt::ctx_wait_slots(mcrt_framebuffer fb) {
    for (auto& k : fb->slot)
        if (k.stream) hipStreamWaitEvent(fb->ctx->stream, k.done, 0);
}

bool mcrt::frame_args(mcrt_framebuffer fb, const mcrt_frame_params* p, FrameArgs& f, std::string& err) {
    f.W = fb->W;
    f.H = fb->H;
    f.frame = p->frame_index;
    f.maxDepth = p->max_depth;
    f.sampler = p->sampler;
    f.russianRoulette = p->russian_roulette;
    f.rrStartDepth = p->rr_start_depth;
    f.textureLod = p->texture_lod ? 1 : 0;
    // batched frames: workgroups of the camera / first-bounce launches walk (tile, frame) with the
    // frames of a tile adjacent, so one XCD traces a tile's batch of jittered frames back to back,
    // and a camera / first-shading wave holds 64 consecutive (pixel, frame) paths of one tile
    // (profiles/r02/ab/README.txt items 11, 14, 15); the order changes no result
    f.tileMajor = 1;
    f.primaryPack = 1;
    f.shadePack = 1;
    f.batch = 1;
    f.tileOrder = nullptr;   // set per call by pt_render (longest-first)
    f.tileCost = nullptr;
    f.numBands = p->num_bands <= 0 ? 1 : p->num_bands;
    f.bandIndex = p->band_index;
    f.bandRows = f.numBands == 1 ? 8 : p->band_rows;
    if (f.bandRows <= 0 || (f.bandRows & 7) != 0) { err = "band_rows must be a positive multiple of 8"; return false; }
    if (f.bandIndex < 0 || f.bandIndex >= f.numBands) { err = "band_index out of range"; return false; }
    f.tilesX = (int)((fb->W + 7) / 8);
    // row-blocks (8 rows) of this band set inside the image; tile ids are dealt in the kernel as
    // tb -> gb, over the band-local blocks that map inside
    f.numTiles = mcrt::band_blocks(fb->H, f.bandRows, f.numBands, f.bandIndex) * f.tilesX;
    return true;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" {

MCRT_API const char* mcrt_version(void) { return "mcrt-mi355x 0.1 (gfx950, HIP)"; }

MCRT_API const char* mcrt_last_error(mcrt_ctx ctx) { return ctx ? ctx->error.c_str() : g_lastError.c_str(); }

MCRT_API mcrt_status mcrt_ctx_create(int device, mcrt_ctx* out) {
    if (!out) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(nullptr, MCRT_ERROR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= n) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "device index out of range");
    auto* c = new mcrt_ctx_s();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return fail(nullptr, MCRT_ERROR_DEVICE, "hipSetDevice failed"); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->numCUs = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(nullptr, MCRT_ERROR_DEVICE, "hipStreamCreate failed");
    }
    c->stream = c->own;
    if (hipMalloc(&c->dFlags, 64 * sizeof(int)) != hipSuccess || hipMemset(c->dFlags, 0, 64 * sizeof(int)) != hipSuccess) {
        hipStreamDestroy(c->own);
        delete c;
        return fail(nullptr, MCRT_ERROR_OUT_OF_MEMORY, "device flags");
    }
    *out = c;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_destroy(mcrt_ctx ctx) {
    if (!ctx) return MCRT_OK;
    hipSetDevice(ctx->device);
    drain_pending(ctx);
    hipStreamSynchronize(ctx->stream);
    hipStreamDestroy(ctx->own);
    if (ctx->dFlags) hipFree(ctx->dFlags);
    delete ctx;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_synchronize(mcrt_ctx ctx) {
    if (!ctx) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "ctx is NULL");
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipDeviceSynchronize());   // frame-slot streams of the context's frame buffers
    return mcrt::check_device_flags(ctx);
}

MCRT_API mcrt_status mcrt_ctx_set_stream(mcrt_ctx ctx, void* stream) {
    if (!ctx) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "ctx is NULL");
    ctx->stream = stream ? (hipStream_t)stream : ctx->own;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_get_stream(mcrt_ctx ctx, void** stream) {
    if (!ctx || !stream) return fail(ctx, MCRT_ERROR_INVALID_ARG, "NULL argument");
    *stream = (void*)ctx->stream;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_set_profiling(mcrt_ctx ctx, int enable) {
    if (!ctx) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "ctx is NULL");
    ctx->profiling = enable != 0;
    ctx->countHints = enable >= 2;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_kernel_stats(mcrt_ctx ctx, int max, const char** names, double* total_ms,
                                           int64_t* launches, int64_t* items, int* count) {
    if (!ctx) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "ctx is NULL");
    hipSetDevice(ctx->device);
    drain_pending(ctx);
    int k = 0;
    for (int i = 0; i < K_COUNT && k < max; ++i) {
        if (ctx->launches[i] == 0) continue;
        if (names) names[k] = kKernelNames[i];
        if (total_ms) total_ms[k] = ctx->totalMs[i];
        if (launches) launches[k] = ctx->launches[i];
        if (items) items[k] = ctx->items[i];
        ++k;
    }
    if (count) *count = k;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_reset_stats(mcrt_ctx ctx) {
    if (!ctx) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "ctx is NULL");
    drain_pending(ctx);
    for (int i = 0; i < K_COUNT; ++i) { ctx->totalMs[i] = 0.0; ctx->launches[i] = 0; ctx->items[i] = 0; }
    return MCRT_OK;
}

// host camera helpers: mcrt_camera.cpp

}  // extern "C"
