// mcrt_capi.cpp -- host runtime behind include/mcrt_capi.h: the context, the scene tables, the ray
// queries and mcrt_render_aov, and the helpers the other host files share (mcrt_host.h).  The
// integrators' drivers are mcrt_pt_host.cpp and mcrt_bdpt_host.cpp, the frame buffer's planes are
// mcrt_film.hip's, the roofline probes mcrt_probe.hip's.
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
using mcrt::fail, mcrt::env_int, mcrt::fb_sync, mcrt::ctx_wait_slots, mcrt::frame_args, mcrt::ensure_spill,
    mcrt::trace_ctx, mcrt::scene_args, mcrt::upload, mcrt::accel_ready;
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

const mcrt_float4* mcrt::host_positions(mcrt_scene s) {
    if (s->positionsStale) {   // the update that left it stale ended synchronised
        hipSetDevice(s->ctx->device);
        if (hipMemcpy(s->positions.data(), s->dPositions.get(), sizeof(float4) * s->positions.size(),
                      hipMemcpyDeviceToHost) != hipSuccess)
            return nullptr;
        s->positionsStale = false;
    }
    return s->positions.data();
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
    s->surfMeshes = e == hipSuccess ? (uint32_t)nm : 0;
    s->surfRecords = e == hipSuccess ? total : 0;
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

// The two vertex updates: `device` tells where positions / normals live.  Everything is checked
// before anything is touched; the copies and the surface records' relaunch run on the context
// stream after every launch already enqueued, and the call ends synchronised.
static mcrt_status update_vertices(mcrt_scene s, uint32_t first, uint32_t count, const void* positions,
                                   const void* normals, bool device) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    mcrt_ctx ctx = s->ctx;
    if (!positions) return fail(ctx, MCRT_ERROR_INVALID_ARG, "positions is NULL");
    const size_t nv = s->positions.size();
    if ((size_t)first > nv || (size_t)count > nv - first)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "vertex range [" + std::to_string(first) + ", " +
                                                     std::to_string((uint64_t)first + count) + ") is outside the scene's " +
                                                     std::to_string(nv) + " vertices");
    if (count == 0) return MCRT_OK;
    hipSetDevice(ctx->device);
    // as mcrt_accel_update_transforms: frames in flight finish on the old vertices
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipDeviceSynchronize());
    hipStream_t st = ctx->stream;
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t bytes = sizeof(float4) * (size_t)count;
    HIPCHK(ctx, hipMemcpyAsync(s->dPositions.get() + first, positions, bytes, kind, st));
    if (normals) HIPCHK(ctx, hipMemcpyAsync(s->dNormals.get() + first, normals, bytes, kind, st));
    if (device) {
        s->positionsStale = true;
    } else if (!s->positionsStale) {   // a stale copy is downloaded whole later, this range with it
        std::memcpy(s->positions.data() + first, positions, bytes);
    }
    if (s->surfMeshes > 0) {   // in place: the meshes, their bases and the records' count are the topology's
        const uint32_t* m = s->dSurfMeshes.get();
        const int nm = (int)s->surfMeshes;
        mcrt::launch_surface_records(m, m + nm, m + 2 * nm, nm, s->surfRecords, s->dIndices.get(), s->dPositions.get(),
                                     s->dUvs.get(), s->dNormals.get(), s->dSurf.get(), st);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipDeviceSynchronize());
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_scene_update_vertices(mcrt_scene s, uint32_t first, uint32_t count, const mcrt_float4* positions,
                                                const mcrt_float4* normals) {
    return update_vertices(s, first, count, positions, normals, false);
}

MCRT_API mcrt_status mcrt_scene_update_vertices_device(mcrt_scene s, uint32_t first, uint32_t count,
                                                       const void* d_positions, const void* d_normals) {
    return update_vertices(s, first, count, d_positions, d_normals, true);
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
// AOVs: a shading pass over borrowed camera hits (the frame buffer's planes: mcrt_film.hip)
// ---------------------------------------------------------------------------
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
    mcrt_camera* dCam = nullptr;   // the AOV pass reuses the current slot's camera and primary-hit buffers
    float4* hits = nullptr;
    const mcrt_status borrowed = mcrt::borrow_camera_hits(s, fb, cam, f, &dCam, &hits);
    if (borrowed != MCRT_OK) return borrowed;
    const size_t stride = aov == MCRT_AOV_TEXTURE_LOD ? 3 : 1;
    float4* dOut = nullptr;
    HIPCHK(ctx, hipMallocAsync((void**)&dOut, 16 * stride * fb->N, st));
    HIPCHK(ctx, hipMemsetAsync(dOut, 0, 16 * stride * fb->N, st));
    mcrt::launch_aov(scene_args(s), f, dCam, hits, aov, dOut, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, dOut, 16 * stride * fb->N, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFreeAsync(dOut, st);
    hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, MCRT_ERROR_DEVICE, std::string("aov: ") + hipGetErrorString(e));
    return MCRT_OK;
}

// host camera helpers: mcrt_camera.cpp

}  // extern "C"
