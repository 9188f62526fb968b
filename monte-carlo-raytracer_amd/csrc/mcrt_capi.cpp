// mcrt_capi.cpp -- host runtime behind include/mcrt_capi.h.
//
// Replaces the reference's OpenCL host plumbing (PlatformManager / KernelManager /
// RTBufferManager, RTScene uploads, RadeonRays IntersectionApi, and the per-pass
// launch + clFinish sequence of RTPrimaryRaysPass / RTPathTracingPass /
// RTReconstructionPass) with: one HIP stream per context, all per-frame work enqueued
// without host synchronisation (queue sizes stay on the device), one memset per frame.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

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
using mcrt::fail, mcrt::env_int, mcrt::fb_sync, mcrt::ctx_wait_slots, mcrt::frame_args, mcrt::ensure_spill,
    mcrt::trace_ctx, mcrt::packet_ctx, mcrt::with_hints, mcrt::scene_args, mcrt::upload, mcrt::accel_ready;
namespace {

#define MCRT_MAX_BOUNCES 32

const char* kKernelNames[K_COUNT] = {"k_primary",    "k_shade0",      "k_shadeN",       "k_shadow",   "k_extend",
                                     "k_accumulate", "k_trace_closest", "k_trace_any",  "k_bdpt_start",
                                     "k_bdpt_vertex", "k_bdpt_connect", "k_bdpt_vis",   "k_bdpt_gather",
                                     "k_shadow_extend", "k_guides",      "k_moments",    "k_atrous_prep",
                                     "k_atrous_s1",   "k_atrous_s2",   "k_atrous_s4",  "k_atrous_s8",
                                     "k_atrous_s16",  "k_atrous_s32",  "k_atrous_s64", "k_atrous_s128",
                                     "k_temporal",    "k_temporal_var", "k_guides_motion", "k_temporal_motion"};

}  // namespace

// The set of the last BDPT call, as cur_slot (mcrt_host.h) is the slot of the last rendered frame
static BdptSet& cur_bset(mcrt_framebuffer fb) { return fb->bset[fb->bdptSet]; }

// BDPT queue counters (64 ints per frame set): [d] the subpath-ray queue of depth d (d <= 33;
// at depth 0 the light rays only), then these
enum { BDPT_CNT_CONN = 40, BDPT_CNT_CAM0 = 41, BDPT_CNT_SPLATS = 42 };
static int bdpt_max_connections(int D) { const int t = D + 2; return t * (t + 1) / 2 - 2; }   // RTBDPTPass.cpp:404-408

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------
mcrt_status mcrt::fail(mcrt_ctx ctx, mcrt_status code, const std::string& msg) {
    g_lastError = msg;
    if (ctx) ctx->error = msg;
    return code;
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
// PT: the stop rule for the extension launches of bounces <= MCRT_WALK_MAXB (default 0: the first,
// full-size one).  At depth 5 the later, smaller launches -- whose any-hit shadow blocks otherwise
// overlap the long walks' tail -- lost what the first gained: k_shadow_extend 2.951 ms per frame
// without the rule, 2.943 with it on every launch, 2.915 on the first only (item 20)
// ... and only for calls of at least MCRT_WALK_MIN_PATHS paths (default 16 M): a rank's share of a
// strong-scaled frame (N = 8: 5 M paths per call) finishes the resumed walks in a launch too small
// to hide their tail (emulated N = 8 rank 0.175 -> 0.179 ms per frame with the rule; BDPT 0.649 ->
// 0.659).  The tests set it to 0 to run the rule on small frames.
static int64_t walk_min_paths() { return env_int("MCRT_WALK_MIN_PATHS", 16000000); }
static int walk_max_bounce() { return env_int("MCRT_WALK_MAXB", 0); }
// BDPT: the light-tracing strategies (t = 1) evaluated by the vertex launches that create their
// light vertices instead of by a connection launch that re-reads them (MCRT_BDPT_LIGHT_IN_VERTEX)
static int bdpt_light_in_vertex() { return env_int("MCRT_BDPT_LIGHT_IN_VERTEX", 1) != 0; }
static int walk_lanes() { return env_int("MCRT_WALK_LANES", 8, 0, 64); }

SceneArgs mcrt::scene_args(mcrt_scene s) {
    SceneArgs a;
    a.shapes = s->dShapes.get();
    a.indices = s->dIndices.get();
    a.positions = s->dPositions.get();
    a.uvs = s->dUvs.get();
    a.normals = s->dNormals.get();
    a.textures = s->dTextures.get();
    a.texData = s->dTexData.get();
    a.sobol = s->dSobol.get();
    a.lights = s->dLights.get();
    a.materials = s->dMaterials.get();
    a.nodes = mcrt::accel_nodes(s);
    a.surf = s->dSurf.get();
    a.surfBase = s->dSurfBase.get();
    a.numLights = (int)s->numLights;
    return a;
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
    f.tileOrder = nullptr;   // set per call by render_frames (longest-first)
    f.tileCost = nullptr;
    f.numBands = p->num_bands <= 0 ? 1 : p->num_bands;
    f.bandIndex = p->band_index;
    f.bandRows = f.numBands == 1 ? 8 : p->band_rows;
    if (f.bandRows <= 0 || (f.bandRows & 7) != 0) { err = "band_rows must be a positive multiple of 8"; return false; }
    if (f.bandIndex < 0 || f.bandIndex >= f.numBands) { err = "band_index out of range"; return false; }
    f.tilesX = (int)((fb->W + 7) / 8);
    // row-blocks (8 rows) of this band set inside the image
    const int blocksTotal = (int)((fb->H + 7) / 8);
    const int bpb = f.bandRows / 8;
    int myBlocks = 0;
    for (int gb = 0; gb < blocksTotal; ++gb)
        if ((gb / bpb) % f.numBands == f.bandIndex) ++myBlocks;
    // tile ids are dealt in the kernel as tb -> gb; count the band-local blocks that map inside
    f.numTiles = myBlocks * f.tilesX;
    return true;
}

// Replaces a scene array once the context stream has finished with the old one.
template <class T>
static mcrt_status replace_array(mcrt_scene s, DevBuf<T>& dst, const T* src, size_t count) {
    mcrt_ctx ctx = s->ctx;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    dst.reset();
    if (count) {
        HIPCHK(ctx, dst.alloc(count));
        HIPCHK(ctx, hipMemcpy(dst.get(), src, sizeof(T) * count, hipMemcpyHostToDevice));
    }
    return MCRT_OK;
}

// An update's tables against the ones the scene keeps: `t` holds the replaced table and the counts
// after the update; the scene's current shapes are filled in here.  Nothing is changed.
static mcrt_status check_update(mcrt_scene s, mcrt::SceneTables t) {
    if (!t.shapes) {
        t.shapes = s->shapes.data();
        t.numShapes = s->shapes.size();
    }
    uint32_t at = 0, slot = 0;
    if (const int bad = mcrt::check_scene_tables(t, &at, &slot))
        return fail(s->ctx, MCRT_ERROR_INVALID_ARG, mcrt::scene_tables_message(bad, at, slot));
    return MCRT_OK;
}

mcrt_status mcrt::check_updated_shapes(mcrt_scene s, const mcrt_shape* sh, uint32_t n) {
    mcrt::SceneTables t;   // the new shapes against the current counts
    t.shapes = sh;
    t.numShapes = n;
    t.numMaterials = s->numMaterials;
    t.numLights = s->numLights;
    t.numTextures = s->numTextures;
    const mcrt_status st = check_update(s, t);
    if (st != MCRT_OK) return st;
    // the index ranges are the topology's and stay; a moved startVertex moves the vertices a shape names
    for (uint32_t i = 0; i < n; ++i) {
        if (sh[i].startVertex == s->shapes[i].startVertex) continue;
        if (mcrt::check_shape_ranges(&sh[i], 1, s->indices.data(), s->indices.size(), s->positions.size(), nullptr))
            return fail(s->ctx, MCRT_ERROR_INVALID_ARG, mcrt::scene_tables_message(mcrt::TABLE_VERTEX_INDEX, i, 0));
    }
    return MCRT_OK;
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

// Device-side error flags raised by kernels since the last check (call after a synchronisation):
// a traversal whose stack needed more entries than its spill column holds drops entries
// (mcrt_traverse.h), so its hits may be wrong -- reported, never silent.
static mcrt_status check_device_flags(mcrt_ctx ctx) {
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
    return check_device_flags(ctx);
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

MCRT_API mcrt_status mcrt_ctx_stream_copy(mcrt_ctx ctx, uint64_t bytes, int iters, double* gbps) {
    if (!ctx || !gbps || bytes < 4096 || iters < 1) return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad stream-copy args");
    hipSetDevice(ctx->device);
    const size_t n4 = (size_t)(bytes / 2 / 16);   // half the bytes read, half written
    float4 *a = nullptr, *b = nullptr;
    HIPCHK(ctx, hipMalloc(&a, n4 * 16));
    if (hipMalloc(&b, n4 * 16) != hipSuccess) { hipFree(a); return fail(ctx, MCRT_ERROR_OUT_OF_MEMORY, "stream copy"); }
    hipMemsetAsync(a, 0, n4 * 16, ctx->stream);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    float best = 1e30f;
    for (int i = 0; i < iters + 1; ++i) {
        hipEventRecord(e0, ctx->stream);
        mcrt::launch_stream_copy(a, b, n4, ctx->numCUs, ctx->stream);
        hipEventRecord(e1, ctx->stream);
        hipEventSynchronize(e1);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, e0, e1);
        if (i > 0 && ms < best) best = ms;   // launch 0 warms up
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(a);
    hipFree(b);
    HIPCHK(ctx, hipGetLastError());
    *gbps = (double)(2 * n4 * 16) / (best * 1e-3) / 1e9;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_gather_chase(mcrt_ctx ctx, uint64_t records, int steps, int iters, double* gsteps) {
    if (!ctx || !gsteps || records < 64 || records > 0xffffffffull || steps < 1 || iters < 1)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad gather-chase args");
    hipSetDevice(ctx->device);
    void* rec = nullptr;
    uint32_t* sink = nullptr;
    HIPCHK(ctx, hipMalloc(&rec, 64 * records));
    if (hipMalloc(&sink, 4) != hipSuccess) { hipFree(rec); return fail(ctx, MCRT_ERROR_OUT_OF_MEMORY, "gather chase"); }
    mcrt::launch_chase_init(rec, (uint32_t)records, ctx->stream);
    const int waves = ctx->numCUs * 32;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    float best = 1e30f;
    for (int i = 0; i < iters + 1; ++i) {
        hipEventRecord(e0, ctx->stream);
        mcrt::launch_chase(rec, (uint32_t)records, i == 0 ? std::max(1, steps / 4) : steps, waves, sink, ctx->stream);
        hipEventRecord(e1, ctx->stream);
        hipEventSynchronize(e1);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, e0, e1);
        if (i > 0 && ms < best) best = ms;   // launch 0 warms caches and translations
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(rec);
    hipFree(sink);
    HIPCHK(ctx, hipGetLastError());
    *gsteps = (double)waves * 64.0 * steps / (best * 1e-3) / 1e9;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_gather_chase_compact(mcrt_ctx ctx, uint64_t records, double leaf_frac, int steps,
                                                   int iters, double* gsteps) {
    if (!ctx || !gsteps || records < 64 || records > 0x3fffffffull || steps < 1 || iters < 1 || !(leaf_frac >= 0.0) ||
        leaf_frac > 1.0)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad gather-chase args");
    hipSetDevice(ctx->device);
    const int waves = ctx->numCUs * 32;
    float best = 0.0f;
    HIPCHK(ctx, mcrt::chase_compact((uint32_t)records, leaf_frac, steps, waves, iters, ctx->stream, &best));
    *gsteps = (double)waves * 64.0 * steps / (best * 1e-3) / 1e9;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_reset_stats(mcrt_ctx ctx) {
    if (!ctx) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "ctx is NULL");
    drain_pending(ctx);
    for (int i = 0; i < K_COUNT; ++i) { ctx->totalMs[i] = 0.0; ctx->launches[i] = 0; ctx->items[i] = 0; }
    return MCRT_OK;
}

// ---------------------------------------------------------------------------
// scene
// ---------------------------------------------------------------------------
// Surface records (SceneArgs::surf): shapes with the same (startIdx, startVertex, numTriangles)
// -- RTScene's instances of one mesh -- share one record range; the records are gathered on the
// device from the uploaded index/vertex arrays.  Rebuilt when shapes change.
static hipError_t build_surface_records(mcrt_scene s) {
    hipStream_t st = s->ctx->stream;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> meshOf;
    std::vector<uint32_t> mStart, mVert, mBase, shapeBase(s->shapes.size());
    uint32_t total = 0;
    for (size_t i = 0; i < s->shapes.size(); ++i) {
        const mcrt_shape& sh = s->shapes[i];
        auto key = std::make_tuple((uint32_t)sh.startIdx, (uint32_t)sh.startVertex, (uint32_t)sh.numTriangles);
        auto it = meshOf.find(key);
        if (it == meshOf.end()) {
            it = meshOf.emplace(key, total).first;
            if (sh.numTriangles > 0) {
                mStart.push_back(sh.startIdx);
                mVert.push_back(sh.startVertex);
                mBase.push_back(total);
            }
            total += sh.numTriangles;
        }
        shapeBase[i] = it->second;
    }
    hipError_t e = hipStreamSynchronize(st);   // the old records may still be read
    s->dSurf.reset();
    s->dSurfBase.reset();
    s->dSurfMeshes.reset();
    const int nm = (int)mBase.size();
    std::vector<uint32_t> meshes(3 * (size_t)std::max(nm, 1));
    std::copy(mStart.begin(), mStart.end(), meshes.begin());
    std::copy(mVert.begin(), mVert.end(), meshes.begin() + nm);
    std::copy(mBase.begin(), mBase.end(), meshes.begin() + 2 * nm);
    if (e == hipSuccess) e = (hipError_t)s->dSurf.alloc((size_t)std::max(total, 1u) * 8);   // 128 B per record
    if (e == hipSuccess) e = upload(s->dSurfBase, shapeBase.data(), shapeBase.size(), st);
    if (e == hipSuccess) e = upload(s->dSurfMeshes, meshes.data(), meshes.size(), st);
    if (e == hipSuccess && nm > 0) {
        const uint32_t* m = s->dSurfMeshes.get();
        mcrt::launch_surface_records(m, m + nm, m + 2 * nm, nm, total, s->dIndices.get(), s->dPositions.get(),
                                     s->dUvs.get(), s->dNormals.get(), s->dSurf.get(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

MCRT_API mcrt_status mcrt_scene_create(mcrt_ctx ctx, const mcrt_scene_desc* d, mcrt_scene* out) {
    if (!ctx || !d || !out) return fail(ctx, MCRT_ERROR_INVALID_ARG, "NULL argument");
    if (d->num_shapes == 0 || !d->shapes) return fail(ctx, MCRT_ERROR_INVALID_ARG, "scene has no shapes");
    if (!d->indices || !d->positions || !d->uvs || !d->normals)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "indices/positions/uvs/normals are required");
    if ((d->num_materials && !d->materials) || (d->num_lights && !d->lights) || (d->num_textures && !d->textures))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "a table with a non-zero count is NULL");
    {
        mcrt::SceneTables t;
        t.shapes = d->shapes;
        t.numShapes = d->num_shapes;
        t.materials = d->materials;
        t.numMaterials = d->num_materials;
        t.lights = d->lights;
        t.numLights = d->num_lights;
        t.numTextures = d->num_textures;
        t.indices = d->indices;
        t.numIndices = d->num_indices;
        t.numVertices = d->num_vertices;
        uint32_t at = 0, slot = 0;
        if (const int bad = mcrt::check_scene_tables(t, &at, &slot))
            return fail(ctx, MCRT_ERROR_INVALID_ARG, mcrt::scene_tables_message(bad, at, slot));
    }
    for (uint32_t i = 0; i < d->num_textures; ++i) {
        const mcrt_texture_desc& t = d->textures[i];
        if (t.width == 0 || t.height == 0 || (uint64_t)t.memOffset + 4ull * t.width * t.height > d->tex_data_bytes)
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "texture " + std::to_string(i) + " is out of the texel buffer");
    }
    hipSetDevice(ctx->device);
    auto* s = new mcrt_scene_s();
    s->ctx = ctx;
    s->shapes.assign(d->shapes, d->shapes + d->num_shapes);
    s->indices.assign(d->indices, d->indices + d->num_indices);
    s->positions.assign(d->positions, d->positions + d->num_vertices);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
#define UP(dst, src, cnt) if (e == hipSuccess) e = upload(s->dst, src, cnt, st)
    UP(dShapes, d->shapes, d->num_shapes);
    UP(dIndices, d->indices, d->num_indices);
    UP(dPositions, d->positions, d->num_vertices);
    UP(dUvs, d->uvs, d->num_vertices);
    UP(dNormals, d->normals, d->num_vertices);
    UP(dTextures, d->textures, d->num_textures);
    UP(dTexData, d->tex_data, d->tex_data_bytes);
    UP(dSobol, d->sobol_matrices, d->num_sobol_words);
    UP(dLights, d->lights, d->num_lights);
    UP(dMaterials, d->materials, d->num_materials);
#undef UP
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = build_surface_records(s);
    if (e != hipSuccess) {
        delete s;
        return fail(ctx, e == hipErrorOutOfMemory ? MCRT_ERROR_OUT_OF_MEMORY : MCRT_ERROR_DEVICE,
                    std::string("scene upload: ") + hipGetErrorString(e));
    }
    s->numLights = d->num_lights;
    s->numMaterials = d->num_materials;
    s->numTextures = d->num_textures;
    s->hasSobol = d->sobol_matrices != nullptr && d->num_sobol_words >= 1024u * 52u;
    *out = s;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_scene_destroy(mcrt_scene s) {
    if (!s) return MCRT_OK;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    delete s;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_scene_update_lights(mcrt_scene s, const mcrt_light* lights, uint32_t n) {
    if (!s || (n && !lights)) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "invalid lights");
    mcrt::SceneTables t;   // the new lights against the current shapes
    t.lights = lights;
    t.numLights = n;
    t.numMaterials = s->numMaterials;
    t.numTextures = s->numTextures;
    mcrt_status st = check_update(s, t);
    if (st != MCRT_OK) return st;
    st = replace_array(s, s->dLights, lights, n);
    if (st == MCRT_OK) s->numLights = n;
    return st;
}

MCRT_API mcrt_status mcrt_scene_update_materials(mcrt_scene s, const mcrt_material* m, uint32_t n) {
    if (!s || (n && !m)) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "invalid materials");
    mcrt::SceneTables t;   // the new materials against the current shapes and texture count
    t.materials = m;
    t.numMaterials = n;
    t.numLights = s->numLights;
    t.numTextures = s->numTextures;
    mcrt_status st = check_update(s, t);
    if (st != MCRT_OK) return st;
    st = replace_array(s, s->dMaterials, m, n);
    if (st == MCRT_OK) s->numMaterials = n;
    return st;
}

MCRT_API mcrt_status mcrt_scene_update_shapes(mcrt_scene s, const mcrt_shape* sh, uint32_t n) {
    if (!s || !sh || n != s->shapes.size())
        return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "shape count must not change");
    for (uint32_t i = 0; i < n; ++i)
        if (sh[i].startIdx != s->shapes[i].startIdx || sh[i].numTriangles != s->shapes[i].numTriangles)
            return fail(s->ctx, MCRT_ERROR_INVALID_ARG, "shape topology must not change");
    mcrt_status st = mcrt::check_updated_shapes(s, sh, n);
    if (st != MCRT_OK) return st;
    st = replace_array(s, s->dShapes, sh, n);
    if (st != MCRT_OK) return st;
    s->shapes.assign(sh, sh + n);   // after the last check: a rejected call leaves the scene as it was
    HIPCHK(s->ctx, build_surface_records(s));   // startVertex may have moved
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_scene_motion_snapshot(mcrt_scene s) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    mcrt_ctx ctx = s->ctx;
    const size_t n = s->shapes.size();
    if (n == 0 || !s->dShapes) return fail(ctx, MCRT_ERROR_INVALID_ARG, "scene has no shapes");
    hipSetDevice(ctx->device);
    if (!s->dPrevPose) HIPCHK(ctx, s->dPrevPose.alloc(n));
    mcrt::launch_pose_snapshot(s->dShapes.get(), s->dPrevPose.get(), (int)n, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

// ---------------------------------------------------------------------------
// RadeonRays-style queries
// ---------------------------------------------------------------------------
struct mcrt_event_s {
    hipEvent_t e = nullptr;
    int device = 0;
};

// n: the host count, or with countDev the grid's capacity (maxrays) and the device count
static mcrt_status trace_common(mcrt_scene s, const mcrt_ray* rays, int32_t n, const int32_t* countDev,
                                mcrt_intersection* hits, int32_t* occl, bool any, mcrt_event wait = nullptr,
                                mcrt_event* done = nullptr) {
    if (done) *done = nullptr;
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    mcrt_ctx ctx = s->ctx;
    if (!accel_ready(s)) return fail(ctx, MCRT_ERROR_NOT_READY, "mcrt_accel_build has not been called");
    if (n < 0 || (n > 0 && !rays) || (n > 0 && !any && !hits) || (n > 0 && any && !occl))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "invalid ray query arguments");
    hipSetDevice(ctx->device);
    if (wait) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, wait->e, 0));
    if (n > 0) {
        if (!ensure_spill(s, (size_t)n)) return fail(ctx, MCRT_ERROR_OUT_OF_MEMORY, "traversal spill buffer");
        Timed t(ctx, any ? K_TRACE_ANY : K_TRACE_CLOSEST, countDev, countDev ? 0 : n);
        mcrt::launch_trace_rays(any, trace_ctx(s), rays, n, countDev, hits, occl, ctx->stream);
    }
    HIPCHK(ctx, hipGetLastError());
    if (done) {
        auto* ev = new mcrt_event_s();
        ev->device = ctx->device;
        hipError_t e = hipEventCreateWithFlags(&ev->e, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ev->e, ctx->stream);
        if (e != hipSuccess) {
            if (ev->e) hipEventDestroy(ev->e);
            delete ev;
            return fail(ctx, MCRT_ERROR_DEVICE, std::string("query event: ") + hipGetErrorString(e));
        }
        *done = ev;
    }
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_trace_closest(mcrt_scene s, const mcrt_ray* d_rays, int32_t n, mcrt_intersection* d_hits) {
    return trace_common(s, d_rays, n, nullptr, d_hits, nullptr, false);
}

MCRT_API mcrt_status mcrt_trace_any(mcrt_scene s, const mcrt_ray* d_rays, int32_t n, int32_t* d_hits) {
    return trace_common(s, d_rays, n, nullptr, nullptr, d_hits, true);
}

MCRT_API mcrt_status mcrt_trace_closest_count(mcrt_scene s, const mcrt_ray* d_rays, const int32_t* d_numrays,
                                              int32_t maxrays, mcrt_intersection* d_hits, mcrt_event wait_event,
                                              mcrt_event* done_event) {
    if (!d_numrays) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "d_numrays is NULL");
    return trace_common(s, d_rays, maxrays, d_numrays, d_hits, nullptr, false, wait_event, done_event);
}

MCRT_API mcrt_status mcrt_trace_any_count(mcrt_scene s, const mcrt_ray* d_rays, const int32_t* d_numrays,
                                          int32_t maxrays, int32_t* d_hits, mcrt_event wait_event,
                                          mcrt_event* done_event) {
    if (!d_numrays) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "d_numrays is NULL");
    return trace_common(s, d_rays, maxrays, d_numrays, nullptr, d_hits, true, wait_event, done_event);
}

MCRT_API mcrt_status mcrt_event_wait(mcrt_event ev) {
    if (!ev) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "event is NULL");
    hipSetDevice(ev->device);
    const hipError_t e = hipEventSynchronize(ev->e);
    if (e != hipSuccess) return fail(nullptr, MCRT_ERROR_DEVICE, std::string("event wait: ") + hipGetErrorString(e));
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_event_destroy(mcrt_event ev) {
    if (!ev) return MCRT_OK;
    hipSetDevice(ev->device);
    hipEventDestroy(ev->e);
    delete ev;
    return MCRT_OK;
}

// ---------------------------------------------------------------------------
// frame buffer + integrator
// ---------------------------------------------------------------------------
static void fb_free_bdpt(mcrt_framebuffer fb) {
    for (auto& b : fb->bset) b = BdptSet();
    fb->sampLight.reset();
    if (fb->bdptConnect) hipEventDestroy(fb->bdptConnect);
    fb->bdptConnect = nullptr;
    fb->bdptDepth = 0;
}

static void slot_free(FrameSlot& k) {
    if (k.stream) hipStreamSynchronize(k.stream);
    if (k.done) hipEventDestroy(k.done);
    if (k.free) hipEventDestroy(k.free);
    if (k.stream) hipStreamDestroy(k.stream);
    k = FrameSlot();
}

// the slots' streams and events and every slot and set; the frame buffer's own planes go with it
static void fb_free(mcrt_framebuffer fb) {
    for (auto& k : fb->slot) slot_free(k);
    fb_free_bdpt(fb);
}

// Per-frame planes (radiance, primary hits) for `frames` frames of N pixels; ray queues of Q entries.
// N: pixels; T: the frame's 8x8 tiles x 64 (the packed hit slots, mcrt_kernels.hip hitSlot)
static hipError_t slot_alloc(FrameSlot& k, size_t N, size_t T, int frames = 1, size_t Q = 0) {
    hipError_t e = hipSuccess;
    if (Q < N) Q = N;
    auto A = [&](auto& buf, size_t count) {
        if (e == hipSuccess) e = (hipError_t)buf.alloc(count);
    };
    A(k.radiance, N * frames);
    A(k.hitsP, std::max(N, T) * frames);
    A(k.hitsE, Q);
    for (int i = 0; i < 2; ++i) { A(k.eO[i], Q); A(k.eD[i], Q); A(k.eT[i], Q); }
    A(k.sO, Q);
    A(k.sD, Q);
    A(k.sL, Q);
    A(k.counters, SLOT_COUNTER_BYTES / sizeof(int));
    k.frames = frames;
    k.queueCap = Q;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&k.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&k.done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&k.free, hipEventDisableTiming);
    // zero-fills on the slot's own stream, ahead of its first launch; `done` covers them for
    // readers on other streams (ctx_wait_slots) before the slot's first frame records it
    if (e == hipSuccess) e = hipMemsetAsync(k.radiance.get(), 0, 16 * N * frames, k.stream);
    if (e == hipSuccess) e = hipMemsetAsync(k.counters.get(), 0, SLOT_COUNTER_BYTES, k.stream);
    if (e == hipSuccess) e = hipEventRecord(k.done, k.stream);
    if (e != hipSuccess) slot_free(k);
    return e;
}

// NQ = the pixels of the whole 8x8 tiles covering the image (>= N): the start queues hold one slot
// per lane of the tile walk.  Ray queues and hits hold 2 x NQ (the depth-1 camera and light halves).
static hipError_t bset_alloc(BdptSet& b, size_t N, size_t NQ, int D, int frames, hipStream_t st) {
    const size_t C = (size_t)bdpt_max_connections(D);
    N *= frames;    // every per-frame array holds the batch's frames
    NQ *= frames;
    hipError_t e = hipSuccess;
    auto A = [&](auto& buf, size_t count) {
        if (e == hipSuccess) e = (hipError_t)buf.alloc(count);
    };
    A(b.camV, N * BDPT_VERTEX_PLANES * (D + 2));
    A(b.lightV, N * BDPT_VERTEX_PLANES * (D + 1));
    A(b.slots, N * (C - D));
    A(b.splat, N);
    A(b.camCount, N);
    A(b.lightCount, N);
    A(b.bdptCounters, 64);
    for (int i = 0; i < 2; ++i) { A(b.bqO[i], 2 * NQ); A(b.bqD[i], 2 * NQ); A(b.bqT[i], 2 * NQ); }
    A(b.bHits, 2 * NQ);
    A(b.cO, N * C);
    A(b.cD, N * C);
    A(b.cL, N * C);
    A(b.lkey, NQ);
    A(b.lkey2, NQ);
    A(b.lslot, NQ);
    A(b.lperm, NQ);
    A(b.ekey, 2 * N);
    A(b.ekey2, 2 * N);
    A(b.eslot, 2 * N);
    A(b.eperm, 2 * N);
    A(b.sortTmp, mcrt::bdpt_light_sort_temp_bytes((int)std::max(NQ, 2 * N)));
    // zero-fills on the stream of the set's frames (st, its slot's), ahead of the first launch
    // that writes the set: a 3 GB vertex-plane memset on another stream could still be running
    // under k_bdpt_start and zero its vertices
    if (e == hipSuccess) e = hipMemsetAsync(b.splat.get(), 0, 16 * N, st);
    if (e == hipSuccess) e = hipMemsetAsync(b.camV.get(), 0, 16 * N * BDPT_VERTEX_PLANES * (D + 2), st);
    if (e == hipSuccess) e = hipMemsetAsync(b.lightV.get(), 0, 16 * N * BDPT_VERTEX_PLANES * (D + 1), st);
    if (e != hipSuccess) b = BdptSet();
    else b.frames = frames;
    return e;
}

// RTBDPTPass::createBuffers (RTBDPTPass.cpp:442-479), sized for max depth D: set k of the
// per-frame arrays, plus the persistent sampled-light-vertex planes, which start zeroed (the
// reference's buffer starts with whatever the allocation holds; its clref runner zero-fills it too).
// (also the packed camera-hit slots per frame: every 8x8 tile of the frame x 64)
static size_t bdpt_queue_cap(mcrt_framebuffer fb) {
    return (size_t)((fb->W + 7) / 8) * ((fb->H + 7) / 8) * 64;
}
static hipError_t fb_ensure_bdpt(mcrt_framebuffer fb, int D, int k, int frames, hipStream_t st) {
    const size_t N = fb->N;
    if (fb->bdptDepth != D) {
        for (auto& sl : fb->slot)
            if (sl.stream) hipStreamSynchronize(sl.stream);
        hipStreamSynchronize(fb->ctx->stream);
        fb_free_bdpt(fb);
        hipError_t e = (hipError_t)fb->sampLight.alloc(N * D);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&fb->bdptConnect, hipEventDisableTiming);
        // zeroed on this frame's stream; every connect launch (the planes' only reader and writer)
        // waits for bdptConnect, recorded here first
        if (e == hipSuccess) e = hipMemsetAsync(fb->sampLight.get(), 0, 16 * N * D, st);
        if (e == hipSuccess) e = hipEventRecord(fb->bdptConnect, st);
        if (e != hipSuccess) { fb_free_bdpt(fb); return e; }
        fb->bdptDepth = D;
    }
    BdptSet& bs = fb->bset[k];
    if (bs.camV && bs.frames < frames) {   // a larger batch: the set's last frames must be done
        for (auto& sl : fb->slot)
            if (sl.stream) hipStreamSynchronize(sl.stream);
        hipStreamSynchronize(fb->ctx->stream);
        bs = BdptSet();
    }
    if (!bs.camV) return bset_alloc(bs, N, bdpt_queue_cap(fb), D, frames, st);
    return hipSuccess;
}

MCRT_API mcrt_status mcrt_framebuffer_create(mcrt_ctx ctx, uint32_t width, uint32_t height, mcrt_framebuffer* out) {
    if (!ctx || !out || width == 0 || height == 0 || (uint64_t)width * height > (1ull << 30))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "invalid frame buffer size");
    hipSetDevice(ctx->device);
    auto* fb = new mcrt_framebuffer_s();
    fb->ctx = ctx;
    fb->W = width;
    fb->H = height;
    fb->N = (size_t)width * height;
    const size_t N = fb->N;
    hipError_t e = hipSuccess;
    for (auto* img : {&fb->wsum, &fb->image, &fb->denoised, &fb->display})
        if (e == hipSuccess) e = (hipError_t)img->alloc(N);
    if (e == hipSuccess) e = (hipError_t)fb->wts.alloc(N);
    if (e == hipSuccess) e = (hipError_t)fb->hintPix.alloc(N);
    fb->slot.resize(MCRT_MAX_FRAMES_IN_FLIGHT);
    if (e == hipSuccess) e = slot_alloc(fb->slot[0], N, N);   // one frame: hits by pixel
    // zero-fills on slot 0's (private) stream, finished before the frame buffer is handed out:
    // only this buffer's work is waited for, not the device (other contexts, a captured caller stream)
    for (auto* img : {&fb->wsum, &fb->image, &fb->denoised, &fb->display})
        if (e == hipSuccess) e = hipMemsetAsync(img->get(), 0, 16 * N, fb->slot[0].stream);
    if (e == hipSuccess) e = hipMemsetAsync(fb->wts.get(), 0, 4 * N, fb->slot[0].stream);
    if (e == hipSuccess) e = mcrt::fill_hints(fb->hintPix.get(), N, 1u << 22, fb->slot[0].stream);   // no hints
    if (e == hipSuccess) e = hipStreamSynchronize(fb->slot[0].stream);
    if (e != hipSuccess) {
        fb_free(fb);
        delete fb;
        return fail(ctx, e == hipErrorOutOfMemory ? MCRT_ERROR_OUT_OF_MEMORY : MCRT_ERROR_DEVICE,
                    std::string("frame buffer: ") + hipGetErrorString(e));
    }
    *out = fb;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_set_frames_in_flight(mcrt_framebuffer fb, int32_t n) {
    if (!fb || n < 0 || n > MCRT_MAX_FRAMES_IN_FLIGHT)
        return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "frames in flight must be 0 (auto) .. 4");
    fb->framesInFlight = n;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_destroy(mcrt_framebuffer fb) {
    if (!fb) return MCRT_OK;
    hipSetDevice(fb->ctx->device);
    fb_sync(fb);
    fb_free(fb);
    delete fb;
    return MCRT_OK;
}

// Frames in flight for a render: the frame buffer's setting; auto = 2.  Each launch of a frame ends in a divergent tail of long rays that the next
// frame's launches fill (San-Miguel proxy 1080p: 2.33 -> 1.91 ms/frame with 2 slots, 2.06 with 4;
// tools/scale_emulate.py).  Small per-rank band shares are widened by batching frames
// (mcrt_render_frames) rather than by more slots: 4 slots of 1/8-image frames reach 0.49 ms per
// frame at N = 8, 2 slots of 16-frame batches 0.25.
// MCRT_WAVE_CLOCK=1: record per-workgroup clocks of launch `which` (grid of `blocks`) on stream st
static bool wave_clock_on() {
    static const bool on = env_int("MCRT_WAVE_CLOCK", 0) != 0;
    return on;
}
static uint32_t* wave_clock_buf(mcrt_framebuffer fb, int which, size_t blocks, hipStream_t st) {
    if (!wave_clock_on()) return nullptr;
    DevBuf<uint32_t>& clk = fb->waveClk[which];
    if (clk.grow(2 * blocks, st) != 0) { hipGetLastError(); return nullptr; }
    hipMemsetAsync(clk.get(), 0, 4 * clk.size(), st);
    return clk.get();
}

#define MCRT_LPT_SHADE_MAX_PATHS 16000000
// MCRT_LONGEST_FIRST=0: camera / first-shading tiles in plain tile order (A/B)
static bool longest_first() {
    static const bool on = env_int("MCRT_LONGEST_FIRST", 1) != 0;
    return on;
}

static int frames_in_flight(mcrt_framebuffer fb, const FrameArgs& f) {
    // MCRT_WAVE_CLOCK=1: one frame in flight -- the clock buffers are per frame buffer, so two slots'
    // launches in flight would write the same per-workgroup entries
    if (wave_clock_on()) return 1;
    int n = fb->framesInFlight;
    if (n <= 0) n = 2;
    return std::max(1, std::min(n, MCRT_MAX_FRAMES_IN_FLIGHT));
}

// RTBDPTPass::update (RTBDPTPass.cpp:67-128): start vertices, D+1 rounds of (trace, vertex),
// connections + MIS, visibility, gather.  Rays of both subpaths share one compacted queue.
static mcrt_status render_bdpt(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, const mcrt_frame_params* p,
                               const FrameArgs& f, int k, FrameSlot& slot) {
    // frame slot k on its stream: per-frame arrays of set k; the connect launch (the only reader
    // and writer of the shared sampled-light-vertex planes) waits for the previous frame's connect
    mcrt_ctx ctx = s->ctx;
    hipStream_t st = slot.stream;
    const int D = p->max_depth;
    const int B = f.batch;   // frames of this call (mcrt_render_frames): path = k * W*H + pixel
    HIPCHK(ctx, fb_ensure_bdpt(fb, D, k, B, st));
    BdptSet& bs = fb->bset[k];
    fb->bdptSet = k;
    slot.lastMaxDepth = D;
    slot.lastPixels = 0;
    fb->bands = f;
    fb->haveBands = true;
    fb->lastIntegrator = MCRT_INTEGRATOR_BDPT;
    fb->bdptBatch = B;
    mcrt_camera* dCam = slot.cameras();
    HIPCHK(ctx, hipMemcpyAsync(dCam, cam, sizeof(mcrt_camera) * B, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(bs.bdptCounters.get(), 0, 64 * sizeof(int), st));
    if (s->numLights == 0) {   // RTBDPTPass.cpp:69: no lights -> pass skipped
        HIPCHK(ctx, hipMemsetAsync(slot.radiance.get(), 0, 16 * fb->N * (size_t)B, st));
        return MCRT_OK;
    }
    const size_t N = fb->N * (size_t)B, C = (size_t)bdpt_max_connections(D);   // N: paths of the batch
    const size_t NQ = bdpt_queue_cap(fb) * (size_t)B;
    // spill columns: one per ray of the widest closest-hit launch (2 NQ) and one per wave of the
    // grid-stride visibility launch (mcrt::BDPT_VIS_MAX_WAVES)
    const size_t spillWords = (std::max(2 * NQ, (size_t)mcrt::BDPT_VIS_MAX_WAVES * 64) + 63) / 64 * 64 * (size_t)mcrt::accel_spill_cap(s);
    HIPCHK(ctx, bs.spill.grow(spillWords, st));
    TraceCtx tcs = trace_ctx(s);
    tcs.spill = bs.spill.get();
    const SceneArgs sa = scene_args(s);
    // the closest-hit launches' stop rule (TraceCtx::walkCap): a traced queue holds at most
    // max(bandQ, nSort) = nSort rays (below)
    const int wcap = tcs.qnodes && !tcs.twoLevel && (int64_t)f.numTiles * 64 * B >= walk_min_paths() ? walk_cap() : 0;
    TraceCtx tce = tcs;
    if (wcap > 0) {
        const size_t need = (size_t)std::min((size_t)2 * N, (size_t)2 * (size_t)f.numTiles * 64 * B);
        HIPCHK(ctx, bs.suspend.grow(MCRT_SUSPEND_F4 * need, st));
        if (!bs.suspendCnt) HIPCHK(ctx, bs.suspendCnt.alloc(64));
        HIPCHK(ctx, hipMemsetAsync(bs.suspendCnt.get(), 0, 64 * sizeof(int), st));
        tce.walkCap = wcap;
        tce.walkLanes = walk_lanes();
        tce.suspend = bs.suspend.get();
    }
    BdptArgs b{};
    b.camV = bs.camV.get();
    b.lightV = bs.lightV.get();
    b.camCount = bs.camCount.get();
    b.lightCount = bs.lightCount.get();
    b.sampLight = fb->sampLight.get();
    b.slots = bs.slots.get();
    b.splat = bs.splat.get();
    b.ownSlots = (int)C - D;
    // (planes at another stride hold other data; another band's paths were never written)
    // the light-start rays are traced in cell order (keys from k_bdpt_start, rocPRIM sort below):
    // k_extend 3.07 -> 2.82 ms per frame at 1080p (profiles/r04/ab/README.txt)
    b.lightKey = bs.lkey.get();
    b.lightSlot = bs.lslot.get();
    // the bounce queues that are traced (depths 1..D) in octant / origin-cell order: keys written by
    // k_bdpt_vertex, sorted below, walked through the permutation by k_extend
    b.extKey = nullptr;
    b.extSlot = nullptr;
    const float* box = mcrt::accel_world_box(s);
    for (int a = 0; a < 3; ++a) {
        const float ext = box[3 + a] - box[a];
        b.keyLo[a] = box[a];
        b.keyScale[a] = ext > 0.0f ? (a == 1 ? 8.0f : 32.0f) / ext : 0.0f;
    }
    b.cams = dCam;
    b.connCount = bs.bdptCounters.get() + BDPT_CNT_CONN;
    b.connO = bs.cO.get();
    b.connD = bs.cD.get();
    b.connL = bs.cL.get();
    b.lightInVertex = bdpt_light_in_vertex();
    BdptArgs bk = b;   // the vertex launches whose output queue is traced
    bk.extKey = bs.ekey.get();
    bk.extSlot = bs.eslot.get();
    // a bounce queue holds at most the band's camera + light rays (2 per path of this rank's tiles),
    // appended compactly from slot 0: sort (and clear) only that range, not the whole frame's -- a
    // rank of a band split would otherwise sort 8 x its own rays at N = 8
    const int bandQ = f.numTiles * 64 * B;   // this rank's paths: a start queue holds at most one ray each
    const int nSort = (int)std::min((size_t)2 * N, (size_t)2 * (size_t)bandQ);
    // the queue traced at round D + 1 holds camera rays only (the light subpaths end at depth D): at
    // most one per path, so it is sorted (and its keys cleared) over bandQ slots, not 2 x bandQ
    auto sortRange = [&](int tracedAt) { return tracedAt == D + 1 ? std::min(nSort, bandQ) : nSort; };
    auto clearKeys = [&](int n) {   // unwritten slots sort last (stable sort: after the written ones)
        return hipMemsetAsync(bs.ekey.get(), 0xFF, 4 * (size_t)n, st);
    };
    b.depth0Const = bs.constStride == N && bs.constBand[0] == f.bandRows && bs.constBand[1] == f.numBands &&
                    bs.constBand[2] == f.bandIndex ? 1 : 0;
    bs.constStride = N;
    bs.constBand[0] = f.bandRows;
    bs.constBand[1] = f.numBands;
    bs.constBand[2] = f.bandIndex;
    float4* const bHits = bs.bHits.get();
    int* cnt = bs.bdptCounters.get();   // [d] ray queue of depth d (d <= D + 1 <= 33), BDPT_CNT_* below
    auto queue = [&](int d) {
        BdptQueue q;
        q.count = cnt + d;
        q.o = bs.bqO[d & 1].get();
        q.d = bs.bqD[d & 1].get();
        q.t = bs.bqT[d & 1].get();
        return q;
    };
    const bool bandSplit = f.numBands > 1;
    const bool sparse = bandSplit && fb->splatExchange == MCRT_SPLAT_EXCHANGE_SPARSE;
    if (sparse) {
        // the splats landing in other ranks' rows go to a list (at most D per path: t = 1, s = 2..D+1);
        // the rank's own rows are zeroed by k_bdpt_start, the other rows of its plane stay unused
        const size_t cap = (size_t)D * (size_t)bandQ;
        HIPCHK(ctx, bs.splatList.grow(cap, st));
        if (!bs.splatAux) HIPCHK(ctx, bs.splatAux.alloc(128));
        b.splatList = bs.splatList.get();
        b.splatListCount = cnt + BDPT_CNT_SPLATS;
        b.splatListCap = (int)std::min(cap, (size_t)INT32_MAX);
        b.splatW = (int)f.W;
        b.splatN0 = (int)(f.W * f.H);
        b.splatBpb = f.bandRows / 8;
        b.splatBands = f.numBands;
        b.splatBand = f.bandIndex;
    } else if (bandSplit) {   // splats of this rank's light paths land in any pixel: clear the whole buffer
        mcrt::launch_bdpt_clear_splat((int)N, bs.splat.get(), st);
    }
    // depth 0: camera rays (coherent, 8x8 tiles in order) in the first half of queue 0's buffers
    // with their own count, light rays in the second half with count [0]; ONE launch traces both,
    // the camera rays as wave packets like PT's camera rays (packet_ctx); both
    // halves then feed the depth-1 vertex launches, which append to queue 1
    BdptQueue camQ = queue(0), lightQ = queue(0);
    camQ.count = cnt + BDPT_CNT_CAM0;
    lightQ.o += NQ;
    lightQ.d += NQ;
    lightQ.t += NQ;
    {
        Timed t(ctx, K_BDPT_START, nullptr, (int64_t)f.numTiles * 64 * B, st);
        mcrt::launch_bdpt_start(sa, f, b, dCam, camQ, lightQ, st);
    }
    {
        TraceCtx tcc = packet_ctx(s);
        tcc.spill = bs.spill.get();
        Timed t(ctx, K_EXTEND, camQ.count, 0, st);
        // exactly the slots k_bdpt_start wrote (the light queue's count, f.numTiles x 64 x B <= NQ)
        HIPCHK(ctx, mcrt::bdpt_light_sort(bs.lkey.get(), bs.lkey2.get(), bs.lslot.get(), bs.lperm.get(), f.numTiles * 64 * B,
                                          bs.sortTmp.get(), bs.sortTmp.size(), st));
        TraceCtx tl = tce;
        tl.suspendCount = wcap > 0 ? bs.suspendCnt.get() : nullptr;
        mcrt::launch_extend_pair(tcc, tl, camQ.count, camQ.o, camQ.d, bHits, lightQ.count, lightQ.o, lightQ.d,
                                 bHits + NQ, bandQ, bandQ, st, bs.lperm.get());   // grids sized to the band
        if (wcap > 0) mcrt::launch_walk_resume(tl, lightQ.o, lightQ.d, bHits + NQ, bandQ, st);
    }
    HIPCHK(ctx, clearKeys(sortRange(2)));   // queue 1 is traced (D >= 1), at round 2
    {
        Timed t(ctx, K_BDPT_VERTEX, camQ.count, 0, st);
        mcrt::launch_bdpt_vertex(sa, f, bk, 1, camQ, bHits, queue(1), bandQ, st);
    }
    {
        Timed t(ctx, K_BDPT_VERTEX, lightQ.count, 0, st);
        mcrt::launch_bdpt_vertex(sa, f, bk, 1, lightQ, bHits + NQ, queue(1), bandQ, st);
    }
    for (int d = 2; d <= D + 1; ++d) {
        const BdptQueue qIn = queue(d - 1), qOut = queue(d);
        {
            Timed t(ctx, K_EXTEND, qIn.count, 0, st);
            const int nQ = sortRange(d);
            HIPCHK(ctx, mcrt::bdpt_light_sort(bs.ekey.get(), bs.ekey2.get(), bs.eslot.get(), bs.eperm.get(), nQ,
                                              bs.sortTmp.get(), bs.sortTmp.size(), st, 16));
            TraceCtx te = tce;
            te.suspendCount = wcap > 0 ? bs.suspendCnt.get() + d : nullptr;
            mcrt::launch_extend(te, qIn.count, qIn.o, qIn.d, bHits, nQ, st, bs.eperm.get());
            if (wcap > 0) mcrt::launch_walk_resume(te, qIn.o, qIn.d, bHits, nQ, st);
        }
        const bool traced = d <= D;   // queue d is traced by the next round
        if (traced) HIPCHK(ctx, clearKeys(sortRange(d + 1)));
        Timed t(ctx, K_BDPT_VERTEX, qIn.count, 0, st);
        mcrt::launch_bdpt_vertex(sa, f, traced ? bk : b, d, qIn, bHits, qOut, nSort, st);
    }
    BdptQueue cq;
    cq.count = cnt + BDPT_CNT_CONN;
    cq.o = bs.cO.get();
    cq.d = bs.cD.get();
    cq.t = bs.cL.get();
    HIPCHK(ctx, hipStreamWaitEvent(st, fb->bdptConnect, 0));   // sampled-light planes in frame order
    {
        Timed t(ctx, K_BDPT_CONNECT, nullptr, (int64_t)f.numTiles * 64 * B, st);
        mcrt::launch_bdpt_connect(sa, f, b, dCam, cq, st);
    }
    HIPCHK(ctx, hipEventRecord(fb->bdptConnect, st));
    {
        Timed t(ctx, K_BDPT_VIS, cq.count, 0, st);
        TraceCtx tvis = tcs;
        with_hints(tvis, s, nullptr, 0);   // occluder hints by origin cell
        mcrt::launch_bdpt_vis(tvis, b, cq, (int)(C * N), st);
    }
    if (bandSplit) {   // completed by mcrt_bdpt_gather once the ranks' splats are summed
        fb->bdptPendingGather = true;
    } else {
        Timed t(ctx, K_BDPT_GATHER, nullptr, (int64_t)f.numTiles * 64 * B, st);
        mcrt::launch_bdpt_gather(f, b, slot.radiance.get(), nullptr, 0, st);
    }
    HIPCHK(ctx, hipGetLastError());
    slot.lastPixels = (int64_t)f.numTiles * 64 * B;
    return MCRT_OK;
}

static mcrt_status render_frames(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, int count,
                                 const mcrt_frame_params* p) {
    if (!s || !fb || !cam || !p) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = s->ctx;
    if (fb->ctx != ctx) return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame buffer belongs to another context");
    if (!accel_ready(s)) return fail(ctx, MCRT_ERROR_NOT_READY, "mcrt_accel_build has not been called");
    if (count < 1 || count > MCRT_MAX_BATCH_FRAMES)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame count must be 1 .. MCRT_MAX_BATCH_FRAMES (256)");
    if (p->integrator == MCRT_INTEGRATOR_BDPT && count > MCRT_MAX_BDPT_BATCH_FRAMES)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "BDPT frame count must be 1 .. MCRT_MAX_BDPT_BATCH_FRAMES (32)");
    for (int k = 0; k < count; ++k)
        if (cam[k].width != fb->W || cam[k].height != fb->H)
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "camera size differs from the frame buffer");
    if (p->integrator == MCRT_INTEGRATOR_BDPT) {   // slot codes (own strategy x paths) and ray tags are int32
        const uint64_t NB = (uint64_t)fb->N * count, C = (uint64_t)bdpt_max_connections(p->max_depth);
        if ((C - (uint64_t)p->max_depth) * NB >= (1ull << 31) || 2 * NB >= (1ull << 31))
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "BDPT: strategies x frames x pixels must stay below 2^31");
    }
    if ((uint64_t)fb->N * count >= (1ull << 31))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame count x pixels must stay below 2^31 (path ids are int32)");
    if (p->max_depth < 1 || p->max_depth > MCRT_MAX_BOUNCES) return fail(ctx, MCRT_ERROR_INVALID_ARG, "max_depth out of range");
    if (p->sampler != MCRT_SAMPLER_RANDOM && p->sampler != MCRT_SAMPLER_SOBOL)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "unknown sampler");
    if (p->sampler == MCRT_SAMPLER_SOBOL && !s->hasSobol)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "Sobol sampler requires the 1024x52 Sobol matrices in the scene");
    if (p->integrator != MCRT_INTEGRATOR_PT && p->integrator != MCRT_INTEGRATOR_BDPT)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "unknown integrator");
    if (fb->bdptPendingGather)
        return fail(ctx, MCRT_ERROR_NOT_READY, "band-split BDPT frame not completed (mcrt_bdpt_gather)");
    FrameArgs f;
    std::string err;
    if (!frame_args(fb, p, f, err)) return fail(ctx, MCRT_ERROR_INVALID_ARG, err);
    hipSetDevice(ctx->device);
    f.batch = count;
    // frame slot: its buffers are free once the accumulation of its previous frame has read them
    const bool bdpt = p->integrator == MCRT_INTEGRATOR_BDPT;
    const int S = bdpt && fb->bdptOneSet ? 1 : frames_in_flight(fb, f);
    int ks = fb->next % S;
    if (bdpt && ks != 0 && fb->bdptDepth == p->max_depth && !fb->bset[ks].camV) {
        // each BDPT set holds ~C x N x 48 B of connection rays (2.5 GB at 1080p, D = 2): when a
        // second one does not fit, fall back to one frame in flight instead of failing the frame
        // (zero-filled on slot ks's stream when it exists, else on slot 0's and finished here: set ks
        // is then first written on slot ks's stream)
        hipStream_t zs = fb->slot[ks].stream ? fb->slot[ks].stream : fb->slot[0].stream;
        hipError_t e = bset_alloc(fb->bset[ks], fb->N, bdpt_queue_cap(fb), p->max_depth, count, zs);
        if (e == hipSuccess && zs != fb->slot[ks].stream) e = hipStreamSynchronize(zs);
        if (e == hipErrorOutOfMemory) {
            hipGetLastError();
            fb->bdptOneSet = true;
            ks = 0;
        } else if (e != hipSuccess) {
            return fail(ctx, MCRT_ERROR_DEVICE, std::string("BDPT buffers: ") + hipGetErrorString(e));
        }
    }
    FrameSlot& slot = fb->slot[ks];
    if (bdpt) {   // BDPT frames overlap the same way (set ks)
        if (!slot.stream) {
            HIPCHK(ctx, slot_alloc(slot, fb->N, bdpt_queue_cap(fb), count));
        } else if (slot.frames < count) {   // radiance planes for a larger batch
            HIPCHK(ctx, hipEventSynchronize(slot.free));
            HIPCHK(ctx, hipStreamSynchronize(slot.stream));
            slot_free(slot);
            HIPCHK(ctx, slot_alloc(slot, fb->N, bdpt_queue_cap(fb), count));
        }
        HIPCHK(ctx, hipStreamWaitEvent(slot.stream, slot.free, 0));
        fb->cur = ks;
        fb->next = (ks + 1) % (fb->bdptOneSet ? 1 : S);
        slot.lastBatch = count;
        const mcrt_status r = render_bdpt(s, fb, cam, p, f, ks, slot);
        hipEventRecord(slot.done, slot.stream);
        return r;
    }
    // the queues hold at most the batch's paths of the band: size the ray grids to them
    const int bandPaths = f.numTiles * 64 * count;
    const size_t qNeed = std::max(fb->N, (size_t)bandPaths);
    if (!slot.stream) {
        HIPCHK(ctx, slot_alloc(slot, fb->N, bdpt_queue_cap(fb), count, qNeed));
    } else if (slot.frames < count || slot.queueCap < qNeed) {   // grow for a larger batch
        HIPCHK(ctx, hipEventSynchronize(slot.free));
        slot_free(slot);
        HIPCHK(ctx, slot_alloc(slot, fb->N, bdpt_queue_cap(fb), count, qNeed));
    }
    const int cap = mcrt::accel_spill_cap(s);
    const size_t spillRays = (std::max((size_t)bandPaths, 2 * qNeed + 64) + 63) / 64 * 64;
    HIPCHK(ctx, slot.spill.grow(spillRays * cap, slot.stream));
    hipStream_t st = slot.stream;
    HIPCHK(ctx, hipStreamWaitEvent(st, slot.free, 0));
    fb->cur = ks;
    fb->next = (ks + 1) % S;
    slot.lastMaxDepth = p->max_depth;
    slot.lastPixels = 0;
    slot.lastBatch = count;
    fb->bands = f;
    fb->haveBands = true;
    mcrt_camera* dCam = slot.cameras();
    int* const counters = slot.counters.get();
    float4 *const radiance = slot.radiance.get(), *const hitsP = slot.hitsP.get(), *const hitsE = slot.hitsE.get();
    float4 *const sO = slot.sO.get(), *const sD = slot.sD.get(), *const sL = slot.sL.get();
    HIPCHK(ctx, hipMemcpyAsync(dCam, cam, sizeof(mcrt_camera) * count, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(counters, 0, 128 * sizeof(int), st));
    int* shadowCnt = counters;          // [b]
    int* extCnt = counters + 32;        // [b]
    const SceneArgs sa = scene_args(s);
    fb->lastIntegrator = MCRT_INTEGRATOR_PT;
    if (s->numLights == 0) {   // RTPathTracingPass.cpp:42: no lights -> pass skipped; radiance = 0 here
        // every frame plane of the batch: accumulate reads `count` of them
        HIPCHK(ctx, hipMemsetAsync(radiance, 0, 16 * fb->N * (size_t)count, st));
        HIPCHK(ctx, hipEventRecord(slot.done, st));
        return MCRT_OK;
    }
    TraceCtx tcs = trace_ctx(s);
    tcs.spill = slot.spill.get();
    const int qCap = bandPaths;
    const int wcap = tcs.qnodes && !tcs.twoLevel && p->max_depth > 1 && bandPaths >= walk_min_paths() ? walk_cap() : 0;
    if (wcap > 0) {
        HIPCHK(ctx, slot.suspend.grow(MCRT_SUSPEND_F4 * (size_t)qCap, st));
        if (!slot.suspendCnt) HIPCHK(ctx, slot.suspendCnt.alloc(32));
        HIPCHK(ctx, hipMemsetAsync(slot.suspendCnt.get(), 0, 32 * sizeof(int), st));
    }
    if (longest_first()) {
        // the camera / first-shading tiles in descending cost of this slot's previous call (same
        // tiles), and this call's costs recorded for the next one -- all on the slot's stream
        if (slot.tileOrder.size() < (size_t)f.numTiles) {   // (the one allocated last)
            slot.costTiles = 0;
            HIPCHK(ctx, slot.tileCost.grow((size_t)f.numTiles, st));
            HIPCHK(ctx, slot.tileOrder.grow((size_t)f.numTiles, st));
        }
        if (slot.costTiles == f.numTiles) {
            mcrt::launch_tile_order(slot.tileCost.get(), f.numTiles, slot.tileOrder.get(), st);
            f.tileOrder = slot.tileOrder.get();
        }
        HIPCHK(ctx, hipMemsetAsync(slot.tileCost.get(), 0, 4 * (size_t)f.numTiles, st));
        f.tileCost = slot.tileCost.get();
        slot.costTiles = f.numTiles;
    }
    {
        Timed t(ctx, K_PRIMARY, nullptr, (int64_t)bandPaths, st);
        TraceCtx tcp = packet_ctx(s);   // coherent camera rays: wave packets
        tcp.spill = slot.spill.get();
        tcp.waveClock = wave_clock_buf(fb, 0, (size_t)f.numTiles * count, st);
        mcrt::launch_primary(tcp, f, dCam, hitsP, st);
    }
    for (int b = 0; b < p->max_depth; ++b) {
        QueueArgs q;
        q.shadowCount = shadowCnt + b;
        q.sO = sO; q.sD = sD; q.sL = sL;
        q.extCountOut = extCnt + b;
        q.eOout = slot.eO[b & 1].get(); q.eDout = slot.eD[b & 1].get(); q.eTout = slot.eT[b & 1].get();
        if (b == 0) {
            Timed t(ctx, K_SHADE0, nullptr, (int64_t)bandPaths, st);
            // the longest-first order also for the first shading (its extension queue then starts with
            // the expensive tiles' rays) only for small launches: at a rank's share of N >= 4 GPUs it
            // trims the extension launch's tail, on a whole 1080p image it costs the shading's
            // spatial locality (+2.8 % k_shade0, +1.2 % k_shadow_extend; profiles/r05/ab/longest_first)
            FrameArgs fs = f;
            if ((int64_t)bandPaths > MCRT_LPT_SHADE_MAX_PATHS) fs.tileOrder = nullptr;
            mcrt::launch_shade0(sa, fs, dCam, hitsP, radiance, q, st);
        } else {
            Timed t(ctx, K_SHADEN, extCnt + b - 1, 0, st);
            mcrt::launch_shadeN(sa, f, b, extCnt + b - 1, slot.eO[(b - 1) & 1].get(), slot.eD[(b - 1) & 1].get(),
                                slot.eT[(b - 1) & 1].get(), hitsE, radiance, q, qCap, st);
        }
        if (b + 1 < p->max_depth) {
            // shadow rays of bounce b + extension rays for bounce b+1 (both from this shading pass) in
            // one launch: separate k_extend + k_shadow launches cost 0.18 ms more per frame (r01)
            Timed t(ctx, K_SHADOW_EXTEND, extCnt + b, 0, st, shadowCnt + b);   // items: extension + shadow rays
            // bounce-0 shadow rays are coherent (a packed wave's paths share a pixel): wave packets
            TraceCtx tse = b == 0 ? packet_ctx(s) : tcs;
            tse.spill = slot.spill.get();
            with_hints(tse, s, b == 0 ? fb->hintPix.get() : nullptr, (uint32_t)fb->N);
            if (tse.hint && ctx->countHints) tse.hintHits = counters + 64 + b;
            if (tse.qnodes && ctx->countHints) tse.retraces = counters + 96 + b;
            if (b == 0) tse.waveClock = wave_clock_buf(fb, 1, 2 * (((size_t)qCap + 63) / 64), st);
            if (wcap > 0 && b <= walk_max_bounce()) {
                tse.walkCap = wcap;
                tse.walkLanes = walk_lanes();
                tse.suspend = slot.suspend.get();
                tse.suspendCount = slot.suspendCnt.get() + b;
            }
            mcrt::launch_shadow_extend(tse, extCnt + b, slot.eO[b & 1].get(), slot.eD[b & 1].get(), hitsE, shadowCnt + b,
                                       sO, sD, sL, radiance, qCap, qCap, st);
            if (tse.walkCap > 0) mcrt::launch_walk_resume(tse, slot.eO[b & 1].get(), slot.eD[b & 1].get(), hitsE, qCap, st);
        } else {
            Timed t(ctx, K_SHADOW, shadowCnt + b, 0, st);
            TraceCtx tsh = tcs;
            with_hints(tsh, s, b == 0 ? fb->hintPix.get() : nullptr, (uint32_t)fb->N);
            if (tsh.hint && ctx->countHints) tsh.hintHits = counters + 64 + b;
            tsh.waveClock = wave_clock_buf(fb, 2, ((size_t)qCap + 63) / 64, st);
            mcrt::launch_shadow(tsh, shadowCnt + b, sO, sD, sL, radiance, qCap, st);
        }
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(slot.done, st));
    slot.lastPixels = (int64_t)bandPaths;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_render_frame(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam,
                                       const mcrt_frame_params* p) {
    return render_frames(s, fb, cam, 1, p);
}

MCRT_API mcrt_status mcrt_render_frames(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cameras, int32_t count,
                                        const mcrt_frame_params* p) {
    return render_frames(s, fb, cameras, count, p);
}

MCRT_API mcrt_status mcrt_render_aov(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam,
                                     const mcrt_frame_params* p, int aov, float* host_out) {
    if (!s || !fb || !cam || !p || !host_out) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = s->ctx;
    if (!accel_ready(s)) return fail(ctx, MCRT_ERROR_NOT_READY, "mcrt_accel_build has not been called");
    if (aov != MCRT_AOV_ALBEDO && aov != MCRT_AOV_TEXTURE_LOD) return fail(ctx, MCRT_ERROR_INVALID_ARG, "unknown aov");
    if (cam->width != fb->W || cam->height != fb->H)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "camera size differs from the frame buffer");
    FrameArgs f;
    std::string err;
    if (!frame_args(fb, p, f, err)) return fail(ctx, MCRT_ERROR_INVALID_ARG, err);
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    FrameSlot& slot = cur_slot(fb);   // the AOV pass reuses the current slot's camera and primary-hit buffers
    if (!slot.counters) return fail(ctx, MCRT_ERROR_NOT_READY, kNoSlotBuffers);
    ctx_wait_slots(fb);
    mcrt_camera* dCam = slot.cameras();
    HIPCHK(ctx, hipMemcpyAsync(dCam, cam, sizeof(mcrt_camera), hipMemcpyHostToDevice, st));
    if (!ensure_spill(s, std::max((size_t)f.numTiles * 64, 2 * fb->N + 64)))
        return fail(ctx, MCRT_ERROR_OUT_OF_MEMORY, "traversal spill buffer");
    const TraceCtx tcs = packet_ctx(s);
    mcrt::launch_primary(tcs, f, dCam, slot.hitsP.get(), st);
    const size_t stride = aov == MCRT_AOV_TEXTURE_LOD ? 3 : 1;
    float4* dOut = nullptr;
    HIPCHK(ctx, hipMallocAsync((void**)&dOut, 16 * stride * fb->N, st));
    HIPCHK(ctx, hipMemsetAsync(dOut, 0, 16 * stride * fb->N, st));
    mcrt::launch_aov(scene_args(s), f, dCam, slot.hitsP.get(), aov, dOut, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, dOut, 16 * stride * fb->N, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFreeAsync(dOut, st);
    hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, MCRT_ERROR_DEVICE, std::string("aov: ") + hipGetErrorString(e));
    return MCRT_OK;
}

static mcrt_status accumulate(mcrt_framebuffer fb, const mcrt_filter* filters, int nfilters, int32_t frame_index) {
    if (!fb || !filters) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    if (fb->bdptPendingGather)
        return fail(ctx, MCRT_ERROR_NOT_READY, "band-split BDPT frame not completed (mcrt_bdpt_gather)");
    if (!fb->haveBands) {   // no frame rendered yet: whole image
        mcrt_frame_params p{};
        std::memset(&p, 0, sizeof(p));
        p.num_bands = 1;
        std::string err;
        frame_args(fb, &p, fb->bands, err);
        fb->haveBands = true;
    }
    hipSetDevice(ctx->device);
    FrameSlot& slot = cur_slot(fb);
    const int batch = slot.lastBatch;
    if (nfilters != 1 && nfilters != batch)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "one filter, or one per frame of the last mcrt_render_frames");
    if (!slot.counters) return fail(ctx, MCRT_ERROR_NOT_READY, kNoSlotBuffers);
    FrameArgs f = fb->bands;
    f.batch = batch;
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, slot.done, 0));   // the frame's render (its slot stream)
    // weights are evaluated on the device (k_accumulate, filters.cl); the filters go to the slot's
    // counter block, which its next render (after slot.free below) does not touch before this launch
    mcrt_filter* dFilt = slot.filters();
    HIPCHK(ctx, hipMemcpyAsync(dFilt, filters, sizeof(mcrt_filter) * nfilters, hipMemcpyHostToDevice, ctx->stream));
    {
        Timed t(ctx, K_ACCUM, nullptr, (int64_t)f.numTiles * 64 * batch);
        mcrt::launch_accumulate(f, frame_index, dFilt, nfilters == 1 ? 0 : 1, slot.radiance.get(), fb->wsum.get(), fb->wts.get(),
                                fb->image.get(), ctx->stream);
    }
    if (fb->dn.momentsOn) {   // the same frames' luminance moments, before the slot is released
        Timed t(ctx, K_MOMENTS, nullptr, (int64_t)f.numTiles * 64 * batch);
        mcrt::launch_moments(f, frame_index, slot.radiance.get(), fb->dn.moments.get(), ctx->stream);
        fb->dn.momentFrames = frame_index == 0 ? batch : fb->dn.momentFrames + batch;
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(slot.free, ctx->stream));   // the slot may take its next frame
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_accumulate(mcrt_framebuffer fb, const mcrt_filter* filter, int32_t frame_index) {
    return accumulate(fb, filter, 1, frame_index);
}

MCRT_API mcrt_status mcrt_accumulate_frames(mcrt_framebuffer fb, const mcrt_filter* filters, int32_t count,
                                            int32_t frame_index) {
    return accumulate(fb, filters, count, frame_index);
}

MCRT_API mcrt_status mcrt_framebuffer_device_ptrs(mcrt_framebuffer fb, void** radiance, void** weighted_sum,
                                                  void** weight_sum, void** image) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    if (radiance) *radiance = cur_slot(fb).radiance.get();
    if (weighted_sum) *weighted_sum = fb->wsum.get();
    if (weight_sum) *weight_sum = fb->wts.get();
    if (image) *image = fb->image.get();
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_postprocess(mcrt_framebuffer fb, const mcrt_postprocess_params* p) {
    if (!fb || !p) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    const int W = (int)fb->W, H = (int)fb->H;
    const float4* src = fb->image.get();
    if (p->use_denoise) {
        // RTDenoisePass (RTDenoisePass.cpp:21-60): the kernel writes nothing for a non-positive
        // radius or sigma (Denoise.cl:18-19), so the pass then shows its image's old content.
        if (p->denoise_radius > 16) return fail(ctx, MCRT_ERROR_INVALID_ARG, "denoise_radius > 16 (the GUI allows <= 10)");
        if (p->denoise_radius > 0 && p->sigma_spatial > 0.0f && p->sigma_range > 0.0f)
            mcrt::launch_denoise(W, H, p->denoise_radius, p->sigma_spatial, p->sigma_range, fb->image.get(), fb->denoised.get(),
                                 ctx->stream);
        src = fb->denoised.get();
    }
    if (p->use_tonemapping)   // RTToneMappingPass::applyReinhardToneMapping (RTToneMappingPass.cpp:38-72)
        mcrt::launch_tonemap(W * H, p->min_luminance, src, fb->display.get(), ctx->stream);
    else
        HIPCHK(ctx, hipMemcpyAsync(fb->display.get(), src, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_read(mcrt_framebuffer fb, int which, float* host_rgba) {
    if (!fb || !host_rgba || which < 0 || which > 3) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    const void* src = which == 0 ? (const void*)cur_slot(fb).radiance.get() : which == 1 ? (const void*)fb->wsum.get()
                      : which == 2 ? (const void*)fb->image.get() : (const void*)fb->display.get();
    HIPCHK(ctx, fb_sync(fb));
    HIPCHK(ctx, hipMemcpy(host_rgba, src, 16 * fb->N, hipMemcpyDeviceToHost));
    return check_device_flags(ctx);
}

MCRT_API mcrt_status mcrt_framebuffer_read_frame(mcrt_framebuffer fb, int32_t k, float* host_rgba) {
    if (!fb || !host_rgba) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    const int batch = cur_slot(fb).lastBatch;
    if (k < 0 || k >= std::max(batch, 1))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame index outside the last mcrt_render_frames batch");
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    HIPCHK(ctx, hipMemcpy(host_rgba, cur_slot(fb).radiance.get() + (size_t)k * fb->N, 16 * fb->N, hipMemcpyDeviceToHost));
    return check_device_flags(ctx);
}

MCRT_API mcrt_status mcrt_framebuffer_copy_device(mcrt_framebuffer fb, int which, void* d_dst) {
    if (!fb || !d_dst || which < 0 || which > 3) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    const void* src = which == 0 ? (const void*)cur_slot(fb).radiance.get() : which == 1 ? (const void*)fb->wsum.get()
                      : which == 2 ? (const void*)fb->image.get() : (const void*)fb->wts.get();
    if (which == 0) ctx_wait_slots(fb);
    HIPCHK(ctx, hipMemcpyAsync(d_dst, src, (which == 3 ? 4 : 16) * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    // the slot may take its next frame only after this copy has read its radiance
    if (which == 0) HIPCHK(ctx, hipEventRecord(cur_slot(fb).free, ctx->stream));
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_set_accumulation(mcrt_framebuffer fb, const void* d_wsum, const void* d_wts) {
    if (!fb || !d_wsum || !d_wts) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipMemcpyAsync(fb->wsum.get(), d_wsum, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(fb->wts.get(), d_wts, 4 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    mcrt::launch_resolve(fb->W, fb->H, fb->wsum.get(), fb->wts.get(), fb->image.get(), ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_bands_pack(mcrt_framebuffer fb, void* d_dst) {
    if (!fb || !d_dst) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    if (!fb->haveBands) return fail(fb->ctx, MCRT_ERROR_NOT_READY, "no frame rendered");
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    mcrt::launch_band_pack(fb->bands, fb->wsum.get(), fb->wts.get(), static_cast<float*>(d_dst), ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

// The largest rank's row count of a band split (whole 8-row blocks): the rows of one packed chunk.
static int band_max_rows(const FrameArgs& f) {
    const int blocks = (int)((f.H + 7) / 8), bpb = f.bandRows / 8;
    const int perCycle = bpb * f.numBands;
    return 8 * ((blocks / perCycle) * bpb + std::min(blocks % perCycle, bpb));
}

MCRT_API mcrt_status mcrt_framebuffer_band_layout(mcrt_framebuffer fb, int32_t* max_rows, int32_t* num_bands,
                                                  int32_t* band_index) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    if (!fb->haveBands) return fail(fb->ctx, MCRT_ERROR_NOT_READY, "no frame rendered");
    if (max_rows) *max_rows = band_max_rows(fb->bands);
    if (num_bands) *num_bands = fb->bands.numBands;
    if (band_index) *band_index = fb->bands.bandIndex;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_bands_unpack(mcrt_framebuffer fb, const void* d_recv, int32_t max_rows) {
    if (!fb || !d_recv) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    if (!fb->haveBands) return fail(fb->ctx, MCRT_ERROR_NOT_READY, "no frame rendered");
    const FrameArgs& f = fb->bands;
    // every chunk of d_recv must hold the largest rank's rows
    if (max_rows < band_max_rows(f))
        return fail(fb->ctx, MCRT_ERROR_INVALID_ARG, "max_rows below the largest rank's row count");
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    mcrt::launch_band_unpack(f, max_rows, static_cast<const float*>(d_recv), fb->wsum.get(), fb->wts.get(), fb->image.get(),
                             ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_stats(mcrt_framebuffer fb, int64_t* closest_rays, int64_t* any_rays,
                                            int64_t* shaded_paths) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    const FrameSlot& slot = cur_slot(fb);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    int c[64];
    if (fb->lastIntegrator == MCRT_INTEGRATOR_BDPT) {   // closest: all subpath rays; any: connection rays
        HIPCHK(ctx, hipMemcpy(c, cur_bset(fb).bdptCounters.get(), sizeof(c), hipMemcpyDeviceToHost));
        int64_t cl = 0;
        for (int d = 0; d <= slot.lastMaxDepth; ++d) cl += c[d];
        cl += c[BDPT_CNT_CAM0];
        if (closest_rays) *closest_rays = cl;
        if (any_rays) *any_rays = c[BDPT_CNT_CONN];
        if (shaded_paths) *shaded_paths = cl;
        return MCRT_OK;
    }
    HIPCHK(ctx, hipMemcpy(c, slot.counters.get(), sizeof(c), hipMemcpyDeviceToHost));
    int64_t cl = slot.lastPixels, an = 0, sh = slot.lastPixels;
    for (int b = 0; b < slot.lastMaxDepth; ++b) {
        an += c[b];
        if (b + 1 < slot.lastMaxDepth) { cl += c[32 + b]; sh += c[32 + b]; }
    }
    if (closest_rays) *closest_rays = cl;
    if (any_rays) *any_rays = an;
    if (shaded_paths) *shaded_paths = sh;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_queue_counts(mcrt_framebuffer fb, int32_t* shadow, int32_t* extension, int max) {
    if (!fb || max < 0) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    const FrameSlot& slot = cur_slot(fb);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    int c[64];
    HIPCHK(ctx, hipMemcpy(c, slot.counters.get(), sizeof(c), hipMemcpyDeviceToHost));
    for (int b = 0; b < max && b < 32; ++b) {
        const bool live = b < slot.lastMaxDepth && fb->lastIntegrator == MCRT_INTEGRATOR_PT;
        if (shadow) shadow[b] = live ? c[b] : 0;
        if (extension) extension[b] = live && b + 1 < slot.lastMaxDepth ? c[32 + b] : 0;
    }
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_hint_counts(mcrt_framebuffer fb, int32_t* hits, int max) {
    if (!fb || max < 0) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    const FrameSlot& slot = cur_slot(fb);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    int c[128];
    HIPCHK(ctx, hipMemcpy(c, slot.counters.get(), sizeof(c), hipMemcpyDeviceToHost));
    for (int b = 0; b < max && b < 32; ++b) {
        const bool live = b < slot.lastMaxDepth && fb->lastIntegrator == MCRT_INTEGRATOR_PT;
        if (hits) hits[b] = live ? c[64 + b] : 0;
    }
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_retrace_counts(mcrt_framebuffer fb, int32_t* retraces, int max) {
    if (!fb || max < 0) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    const FrameSlot& slot = cur_slot(fb);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    int c[128];
    HIPCHK(ctx, hipMemcpy(c, slot.counters.get(), sizeof(c), hipMemcpyDeviceToHost));
    for (int b = 0; b < max && b < 32; ++b) {
        const bool live = b + 1 < slot.lastMaxDepth && fb->lastIntegrator == MCRT_INTEGRATOR_PT;
        if (retraces) retraces[b] = live ? c[96 + b] : 0;
    }
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_wave_clock(mcrt_framebuffer fb, int which, uint32_t* host_out, int64_t max_blocks,
                                                 int64_t* blocks) {
    if (!fb || which < 0 || which > 2 || !blocks) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    *blocks = (int64_t)(fb->waveClk[which].size() / 2);
    if (!host_out || !fb->waveClk[which].get()) return MCRT_OK;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    const size_t n = std::min((size_t)std::max<int64_t>(max_blocks, 0), fb->waveClk[which].size() / 2);
    HIPCHK(ctx, hipMemcpy(host_out, fb->waveClk[which].get(), 8 * n, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_read_queue(mcrt_framebuffer fb, int which, void* host_dst,
                                                 int64_t max_records, int32_t* count) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    const FrameSlot& slot = cur_slot(fb);
    if (which != 0 && which != 1) return fail(ctx, MCRT_ERROR_INVALID_ARG, "which must be 0 (shadow) or 1 (extension)");
    if (max_records < 0 || (max_records > 0 && !host_dst)) return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad destination");
    if (slot.lastMaxDepth <= 0) return fail(ctx, MCRT_ERROR_INVALID_ARG, "nothing rendered yet");
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    int c[64];
    HIPCHK(ctx, hipMemcpy(c, slot.counters.get(), sizeof(c), hipMemcpyDeviceToHost));
    const int b = which == 0 ? slot.lastMaxDepth - 1 : slot.lastMaxDepth - 2;   // last shadow / last extension queue
    const int n = b < 0 ? 0 : (which == 0 ? c[b] : c[32 + b]);
    if (count) *count = n;
    const int64_t m = std::min<int64_t>(n, max_records);
    if (m == 0) return MCRT_OK;
    const float4* src[3];
    if (which == 0) { src[0] = slot.sO.get(); src[1] = slot.sD.get(); src[2] = slot.sL.get(); }
    else { src[0] = slot.eO[b & 1].get(); src[1] = slot.eD[b & 1].get(); src[2] = slot.eT[b & 1].get(); }   // b >= 0 here
    for (int k = 0; k < 3; ++k)
        HIPCHK(ctx, hipMemcpy(static_cast<char*>(host_dst) + (size_t)k * 16 * max_records, src[k], 16 * (size_t)m,
                              hipMemcpyDeviceToHost));
    return MCRT_OK;
}

// Rank-major splat layout of a band split of H rows into num_bands interleaved sets of band_rows
// rows: chunks = num_bands, each of (the largest rank's 8-row block count) x 8 rows x W pixels.
static size_t splat_chunk_pixels(const FrameArgs& f) {
    const int blocksTotal = (int)((f.H + 7) / 8), bpb = f.bandRows / 8;
    int maxBlocks = 0;
    for (int r = 0; r < f.numBands; ++r) {
        int nb = 0;
        for (int gb = 0; gb < blocksTotal; ++gb) nb += ((gb / bpb) % f.numBands == r) ? 1 : 0;
        maxBlocks = std::max(maxBlocks, nb);
    }
    return (size_t)maxBlocks * 8 * f.W;
}

MCRT_API mcrt_status mcrt_bdpt_splat_layout(mcrt_framebuffer fb, uint64_t* chunk_pixels, int32_t* chunks) {
    if (!fb || !chunk_pixels || !chunks) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    if (!fb->haveBands) return fail(fb->ctx, MCRT_ERROR_NOT_READY, "no frame rendered yet");
    *chunk_pixels = splat_chunk_pixels(fb->bands) * (size_t)std::max(fb->bands.batch, 1);   // batch frames per chunk
    *chunks = fb->bands.numBands;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_set_splat_exchange(mcrt_framebuffer fb, int32_t mode) {
    if (!fb || (mode != MCRT_SPLAT_EXCHANGE_DENSE && mode != MCRT_SPLAT_EXCHANGE_SPARSE))
        return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "unknown splat exchange mode");
    if (fb->bdptPendingGather) return fail(fb->ctx, MCRT_ERROR_NOT_READY, "band-split BDPT frame not completed");
    fb->splatExchange = mode;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_bdpt_splats_sparse(mcrt_framebuffer fb, void* d_dst, int64_t capacity, int64_t* counts,
                                             int32_t num_counts) {
    if (!fb || !counts) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    const int bands = fb->bands.numBands;
    if (num_counts < bands) return fail(ctx, MCRT_ERROR_INVALID_ARG, "counts must hold num_bands entries");
    for (int r = 0; r < num_counts; ++r) counts[r] = 0;
    if (!fb->bdptPendingGather) return MCRT_OK;   // nothing pending (light-less scene): no splats
    if (fb->splatExchange != MCRT_SPLAT_EXCHANGE_SPARSE)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame rendered with the dense splat exchange (mcrt_bdpt_splats_copy)");
    if (bands > 64) return fail(ctx, MCRT_ERROR_INVALID_ARG, "sparse splat exchange: at most 64 bands");
    hipSetDevice(ctx->device);
    BdptSet& bs = cur_bset(fb);
    hipStream_t st = cur_slot(fb).stream;
    BdptArgs b{};
    b.splatList = bs.splatList.get();
    b.splatListCount = bs.bdptCounters.get() + BDPT_CNT_SPLATS;
    b.splatListCap = (int)std::min(bs.splatList.size(), (size_t)INT32_MAX);
    b.splatW = (int)fb->bands.W;
    b.splatN0 = (int)(fb->bands.W * fb->bands.H);
    b.splatBpb = fb->bands.bandRows / 8;
    b.splatBands = bands;
    b.splatBand = fb->bands.bandIndex;
    int h[64];
    HIPCHK(ctx, hipMemsetAsync(bs.splatAux.get(), 0, 128 * sizeof(int), st));
    mcrt::launch_splat_hist(b, bs.splatAux.get(), st);
    HIPCHK(ctx, hipMemcpyAsync(h, bs.splatAux.get(), sizeof(int) * bands, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the sizes go to the host (an all-to-all's split sizes)
    mcrt::SplatOffsets off{};
    int64_t total = 0;
    for (int r = 0; r < bands; ++r) {
        off.off[r] = (int)total;
        counts[r] = h[r];
        total += h[r];
    }
    if (!d_dst || capacity < total) return MCRT_OK;   // sizes only (the caller grows its buffer and calls again)
    // the caller's send buffer may still be read by an earlier call's all-to-all on another frame
    // slot's stream (two frames in flight), and that call's unpack must read its receive buffer
    // before this call's all-to-all (ordered after this grouping on this stream) overwrites it: wait
    // for every other slot's completed frame, as mcrt_bdpt_splats_copy does
    for (auto& k : fb->slot)
        if (k.stream && k.stream != st) HIPCHK(ctx, hipStreamWaitEvent(st, k.done, 0));
    mcrt::launch_splat_group(b, off, bs.splatAux.get() + 64, (float4*)d_dst, st);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;   // grouping enqueued on the frame's stream
}

MCRT_API mcrt_status mcrt_bdpt_gather_sparse(mcrt_framebuffer fb, const void* d_recv, int64_t records) {
    if (!fb || (records > 0 && !d_recv)) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    if (!fb->bdptPendingGather) return MCRT_OK;
    if (fb->splatExchange != MCRT_SPLAT_EXCHANGE_SPARSE)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame rendered with the dense splat exchange (mcrt_bdpt_gather)");
    if (records < 0 || records > INT32_MAX) return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad record count");
    hipSetDevice(ctx->device);
    FrameSlot& slot = cur_slot(fb);
    const BdptSet& bs = cur_bset(fb);
    hipStream_t st = slot.stream;
    mcrt::launch_splat_unpack((const float4*)d_recv, (int)records, bs.splat.get(), st);
    BdptArgs b{};
    b.slots = bs.slots.get();
    b.splat = bs.splat.get();
    b.ownSlots = bdpt_max_connections(fb->bdptDepth) - fb->bdptDepth;
    {
        Timed t(ctx, K_BDPT_GATHER, nullptr, (int64_t)fb->bands.numTiles * 64 * fb->bands.batch, st);
        mcrt::launch_bdpt_gather(fb->bands, b, slot.radiance.get(), nullptr, 0, st);   // the rank's own plane
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(slot.done, st));
    fb->bdptPendingGather = false;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_bdpt_splats_copy(mcrt_framebuffer fb, void* d_dst) {
    if (!fb || !d_dst) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    if (fb->bdptPendingGather && fb->splatExchange == MCRT_SPLAT_EXCHANGE_SPARSE)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame rendered with the sparse splat exchange (mcrt_bdpt_splats_sparse)");
    if (!fb->haveBands) return fail(ctx, MCRT_ERROR_NOT_READY, "no frame rendered yet");
    hipSetDevice(ctx->device);
    const size_t chunk = splat_chunk_pixels(fb->bands);   // per frame; a rank's chunk holds batch of them
    const size_t total = chunk * (size_t)std::max(fb->bands.batch, 1) * (size_t)fb->bands.numBands;
    FrameSlot& slot = cur_slot(fb);
    hipStream_t st = slot.stream ? slot.stream : ctx->stream;
    // the caller's buffer may still be read by an earlier frame's gather on another slot's stream
    for (auto& k : fb->slot)
        if (k.stream && k.stream != st) HIPCHK(ctx, hipStreamWaitEvent(st, k.done, 0));
    HIPCHK(ctx, hipMemsetAsync(d_dst, 0, sizeof(float) * MCRT_SPLAT_CHANNELS * total, st));
    if (fb->bdptPendingGather)   // (else, e.g. a scene without lights: the frame is complete, no splats)
        mcrt::launch_bdpt_splat_pack(fb->bands, chunk, cur_bset(fb).splat.get(), (float*)d_dst, st);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;   // enqueued on the frame's stream (mcrt_framebuffer_stream): no host sync
}

MCRT_API mcrt_status mcrt_framebuffer_stream(mcrt_framebuffer fb, void** stream) {
    if (!fb || !stream) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    const FrameSlot& slot = cur_slot(fb);
    *stream = (void*)(slot.stream ? slot.stream : fb->ctx->stream);
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_bdpt_gather(mcrt_framebuffer fb, const void* d_own_chunk) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    if (!fb->bdptPendingGather) return MCRT_OK;   // nothing deferred (whole-image or light-less frame)
    if (fb->splatExchange == MCRT_SPLAT_EXCHANGE_SPARSE)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame rendered with the sparse splat exchange (mcrt_bdpt_gather_sparse)");
    hipSetDevice(ctx->device);
    FrameSlot& slot = cur_slot(fb);
    hipStream_t st = slot.stream;
    BdptArgs b{};
    b.slots = cur_bset(fb).slots.get();
    b.splat = cur_bset(fb).splat.get();
    b.ownSlots = bdpt_max_connections(fb->bdptDepth) - fb->bdptDepth;
    {
        Timed t(ctx, K_BDPT_GATHER, nullptr, (int64_t)fb->bands.numTiles * 64 * fb->bands.batch, st);
        mcrt::launch_bdpt_gather(fb->bands, b, slot.radiance.get(), (const float*)d_own_chunk,
                                 splat_chunk_pixels(fb->bands), st);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(slot.done, st));
    fb->bdptPendingGather = false;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_read_bdpt(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                uint64_t* needed) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    if (fb->bdptDepth <= 0) return fail(ctx, MCRT_ERROR_INVALID_ARG, "no BDPT frame rendered yet");
    // the planes of the last BDPT call's batch (plane stride N x batch)
    const size_t N = fb->N * (size_t)fb->bdptBatch, D = (size_t)fb->bdptDepth;
    const size_t C = (size_t)bdpt_max_connections(fb->bdptDepth);
    const BdptSet& bs = cur_bset(fb);
    const void* src = nullptr;
    size_t sz = 0;
    switch (which) {
    case 0: src = bs.camV.get(); sz = 16 * N * BDPT_VERTEX_PLANES * (D + 2); break;
    case 1: src = bs.lightV.get(); sz = 16 * N * BDPT_VERTEX_PLANES * (D + 1); break;
    case 2: src = bs.camCount.get(); sz = 4 * N; break;
    case 3: src = bs.lightCount.get(); sz = 4 * N; break;
    case 4: src = bs.slots.get(); sz = 16 * N * (C - D); break;
    case 5: src = fb->sampLight.get(); sz = 16 * fb->N * D; break;   // per pixel, carried across frames
    case 6: src = bs.splat.get(); sz = 16 * N; break;
    default: return fail(ctx, MCRT_ERROR_INVALID_ARG, "which must be 0..6");
    }
    if (needed) *needed = sz;
    if (!host_dst || bytes == 0) return MCRT_OK;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    HIPCHK(ctx, hipMemcpy(host_dst, src, std::min<size_t>(sz, bytes), hipMemcpyDeviceToHost));
    return MCRT_OK;
}

// host camera helpers: mcrt_camera.cpp

}  // extern "C"
