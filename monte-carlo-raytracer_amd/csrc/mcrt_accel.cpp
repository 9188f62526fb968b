// mcrt_accel.cpp -- the scene's acceleration structure on the device: mcrt_accel_build over the
// three builders (device SAH, device LBVH, the host layer's build_host_tree + upload) with one
// commit into AccelState (mcrt_host.h), the transform-only update, the refit, the read-back entry points and
// the traversal views the render and query paths take.  The options, input checks and the host
// build itself are mcrt_accel_host.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mcrt_host.h"

using mcrt::fail, mcrt::env_int;
using Clock = std::chrono::steady_clock;

static double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

// --- views and accessors ---
bool mcrt::accel_ready(mcrt_scene s) { return (bool)s->accel.dNodes; }
const float4* mcrt::accel_nodes(mcrt_scene s) { return s->accel.dNodes.get(); }
int mcrt::accel_spill_cap(mcrt_scene s) { return s->accel.spillCap; }
const float* mcrt::accel_world_box(mcrt_scene s) { return s->accel.tree.box; }

bool mcrt::ensure_spill(mcrt_scene s, size_t rays) {
    rays = (rays + 63) / 64 * 64;
    return s->accel.dSpill.grow(rays * (size_t)s->accel.spillCap, s->ctx->stream) == 0;
}

TraceCtx mcrt::trace_ctx(mcrt_scene s) {
    const AccelState& a = s->accel;
    TraceCtx c = {};
    c.nodes = a.dNodes.get();
    c.packet = 0;
    c.spill = a.dSpill.get();
    c.spillCap = a.spillCap;
    c.overflow = s->ctx->dFlags;
    c.twoLevel = a.tree.twoLevel ? 1 : 0;
    c.numNodes = (uint32_t)a.tree.numNodes;
    c.qnodes = a.dQNodes.get();
    c.qroot = a.qRoot;
    return c;
}

TraceCtx mcrt::packet_ctx(mcrt_scene s) {
    TraceCtx c = trace_ctx(s);
    c.packet = s->accel.packets ? 1 : 0;
    return c;
}

// Occluder hints (the leaf test of a two-level record would need the instance transform, so flat
// trees only).  The answers are the walk's with or without them; MCRT_SHADOW_HINTS=0 turns them
// off (A/B, tests).
static bool hints_enabled() { return env_int("MCRT_SHADOW_HINTS", 1) != 0; }
// test hook: MCRT_TEST_HINT_FILL=seed fills a new hint table with pseudo-random words below
// `range` instead of "no hint", so a test can check that arbitrary hints change no answer
hipError_t mcrt::fill_hints(uint32_t* d, size_t n, uint32_t range, hipStream_t st) {
    const char* e = std::getenv("MCRT_TEST_HINT_FILL");
    if (!e) return hipMemsetAsync(d, 0xff, 4 * n, st);
    std::vector<uint32_t> h(n);
    uint32_t x = 2463534242u + (uint32_t)std::atoi(e);
    for (auto& v : h) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        v = x % range;
    }
    hipError_t r = hipMemcpyAsync(d, h.data(), 4 * n, hipMemcpyHostToDevice, st);
    if (r == hipSuccess) r = hipStreamSynchronize(st);
    return r;
}
// Entries of the origin-cell table: 2^25 words (128 MB) for trees of more than 2^22 nodes (the
// headline scene: 20 M nodes), fewer for smaller trees (2 words per node, at least 2^18).  Any size
// is safe -- a slot is a hint, never an answer.
static int hint_bits_for(uint32_t numNodes) {
    int b = 18;
    while (b < MCRT_HINT_CELL_BITS && (1u << b) < 2u * numNodes) ++b;
    return b;
}
// The table is allocated (and emptied) on the first launch that uses it, on the context stream,
// which is finished before the launch's own stream reads it; if it does not fit, hints stay off.
static bool ensure_hint_cell(mcrt_scene s) {
    AccelState& a = s->accel;
    if (a.dHintCell) return true;
    if (a.hintAllocFailed) return false;
    mcrt_ctx ctx = s->ctx;
    const int bits = hint_bits_for((uint32_t)a.tree.numNodes);
    hipError_t e = (hipError_t)a.dHintCell.alloc((size_t)1 << bits);
    if (e == hipSuccess) e = mcrt::fill_hints(a.dHintCell.get(), (size_t)1 << bits, (uint32_t)a.tree.numNodes + 64, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        hipGetLastError();
        a.dHintCell.reset();
        a.hintAllocFailed = true;
        return false;
    }
    a.hintBits = bits;
    return true;
}
void mcrt::with_hints(TraceCtx& c, mcrt_scene s, uint32_t* pix, uint32_t n) {
    const AccelState& a = s->accel;
    if (a.tree.twoLevel || !hints_enabled() || !ensure_hint_cell(s)) return;
    c.hintCell = a.dHintCell.get();
    c.hintMask = (1u << a.hintBits) - 1;
    for (int k = 0; k < 3; ++k) {
        const float ext = a.tree.box[3 + k] - a.tree.box[k];
        c.hintLo[k] = a.tree.box[k];
        c.hintInvExt[k] = ext > 0.0f ? 1.0f / ext : 0.0f;
    }
    c.hint = pix ? pix : a.dHintCell.get();
    c.hintMode = pix ? MCRT_HINT_PIXEL : MCRT_HINT_CELL;
    c.hintPixels = n;
}

// --- build ---
// per-ray spill columns deep enough for the tree (allocated by ensure_spill for the largest launch)
static void apply_spill_cap(AccelState& a) {
    int needCap = ((a.tree.depth + 2 + 15) / 16) * 16;   // whole spill blocks of STACK_LDS entries
    // test hook: MCRT_TEST_SPILL_CAP=k caps the spill columns at k entries (0 = LDS stack only) so a
    // test can drive a traversal past its capacity and check that the overflow is reported
    if (const char* tc = std::getenv("MCRT_TEST_SPILL_CAP")) needCap = std::max(0, std::atoi(tc) / 16 * 16);
    if (needCap != a.spillCap) {
        a.dSpill.reset();
        a.spillCap = needCap;
    }
}

// No structure: what a build that fails after it touched the device leaves, and what commit
// starts from, so that nothing of the previous route survives the next one.  The spill columns,
// the scratch and the record of the last build's options and update are not the structure's.
static void drop(AccelState& a) {
    a.dNodes.reset();
    a.dQNodes.reset();
    a.dHintCell.reset();
    a.hintAllocFailed = false;
    mcrt::top_build_destroy(a.topDev);   // sized for the previous top level
    a.topDev = nullptr;
    a.top2l = mcrt::Bvh2lTop();
    a.refitParent.reset();   // the previous topology's
    a.refitArrive.reset();
    a.refitQOff.reset();
    a.refitFlag.reset();
    a.tree = mcrt::TreeInfo();
    a.qRoot = 0;
    a.packets = false;
}

// Everything that is derived from the records just put in place; boxFromRoot: a tree built on the
// device, whose world box is its root record's
static mcrt_status finish(mcrt_scene s, bool boxFromRoot) {
    mcrt_ctx ctx = s->ctx;
    AccelState& a = s->accel;
    mcrt::TreeInfo& t = a.tree;
    // wave packets for the coherent launches (mcrt_traverse.h traversePacket): flat trees whose
    // depth fits the packet stack (at most 2 entries per internal level: 2 x depth, the leaves'
    // level).  MCRT_CAMERA_PACKETS=0 walks them per ray (A/B and tests: the results are the same bit
    // for bit).
    a.packets = !t.twoLevel && 2 * t.depth <= MCRT_PK_STACK && t.numNodes < (1u << 26) &&   // 32-bit offsets
                env_int("MCRT_CAMERA_PACKETS", 1) != 0;
    if (!a.dScratch) HIPCHK(ctx, a.dScratch.alloc(256));
    HIPCHK(ctx, hipMemset(a.dScratch.get(), 0, 256 * sizeof(int)));
    if (!t.twoLevel) {
        // parent links of the leaves (occluder hints).  The origin-cell hint table is allocated on
        // its first use (ensure_hint_cell, sized for the tree); drop() freed the old one
        mcrt::launch_leaf_parents(a.dNodes.get(), (uint32_t)t.numNodes, ctx->stream);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    // compact records for the per-ray walks (mcrt_traverse.h traverseQOct): depth-first flat trees;
    // MCRT_QUANT_NODES=0 keeps the 64-B records everywhere (A/B, tests).  A tree the converter
    // cannot take (LBVH numbering) or a device without room for it (~0.8 GB at 10 M triangles)
    // keeps the 64-B walk: the same answers.
    // MCRT_QNODE_ORDER picks their order (A/B, tests: 1 sibling pairs, 2 treelets, the default; either
    // gives the same walks).
    if (!t.twoLevel && env_int("MCRT_QUANT_NODES", 1) != 0) {
        DevBuf<float4> q;
        const int order = env_int("MCRT_QNODE_ORDER", mcrt::QORDER_TREELETS);
        a.qOrder = order == mcrt::QORDER_SIBLINGS ? order : mcrt::QORDER_TREELETS;
        const hipError_t e = mcrt::build_qnodes(a.dNodes.get(), (uint32_t)t.numNodes, a.qOrder, q, ctx->stream);
        if (e == hipSuccess) {
            a.dQNodes = std::move(q);
        } else if (e != hipErrorNotSupported && e != hipErrorOutOfMemory) {
            return fail(ctx, MCRT_ERROR_DEVICE, std::string("compact records: ") + hipGetErrorString(e));
        } else {
            (void)hipGetLastError();
        }
    }
    apply_spill_cap(a);
    if (boxFromRoot) {
        float root[16];
        HIPCHK(ctx, hipMemcpy(root, a.dNodes.get(), sizeof(root), hipMemcpyDeviceToHost));
        mcrt::root_record_box(root, t.box);
    }
    // compact reference of the root: offset 0, and the leaf bit when the tree is one triangle
    a.qRoot = !t.twoLevel && t.numNodes == 1 ? 1u : 0u;
    return MCRT_OK;
}

// What every route ends in, once its records are on the device: the new structure in place of the
// old one.  host: the build the records were uploaded from, or NULL for a tree built on the device.
static mcrt_status commit(mcrt_scene s, const mcrt_accel_opts* opts, DevBuf<float4>& nodes, const mcrt::TreeInfo& info,
                          mcrt::HostTree* host, Clock::time_point t0) {
    AccelState& a = s->accel;
    drop(a);
    a.dNodes = std::move(nodes);
    a.tree = info;
    if (host) a.top2l = std::move(host->top);
    a.haveOpts = opts != nullptr;
    if (opts) a.lastOpts = *opts;
    a.lastOpts.world_to_local = nullptr;   // the caller's array, not kept
    const mcrt_status st = finish(s, host == nullptr);
    if (st != MCRT_OK) drop(a);
    a.buildMs = ms_since(t0);
    return st;
}

extern "C" {

MCRT_API mcrt_status mcrt_accel_build(mcrt_scene s, const mcrt_accel_opts* opts) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    mcrt_ctx ctx = s->ctx;
    AccelState& a = s->accel;
    const mcrt::SceneGeometry g = mcrt::scene_geometry(s);
    mcrt::AccelPlan plan;
    if (!mcrt::make_accel_plan(opts, g.shapes, g.numShapes, plan))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "num_bins out of range");
    const auto t0 = Clock::now();
    std::vector<uint32_t> first(g.numShapes);   // each shape's first triangle
    size_t n = 0;
    for (size_t si = 0; si < g.numShapes; ++si) { first[si] = (uint32_t)n; n += g.shapes[si].numTriangles; }
    if (n == 0) return fail(ctx, MCRT_ERROR_INVALID_ARG, "scene has no triangles (RR: Commit on empty scene throws)");
    if (n > (size_t)0x7fffffff) return fail(ctx, MCRT_ERROR_INVALID_ARG, "too many triangles");
    const int mode = plan.twoLevel ? -1 : plan.deviceBuild;
    DevBuf<float4> nodes;
    if (mode == 0 || mode == 1 || mode == 2) {
        // 0, 2: on-device SAH, node-identical to the host build; 1: on-device linear BVH (mcrt_gpubuild.hip)
        hipSetDevice(ctx->device);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        float4* built = nullptr;
        const char* why = nullptr;
        mcrt::TreeInfo info;
        info.numNodes = info.topNodes = 2 * n - 1;
        info.numTris = n;
        info.builder = mode == 1 ? 1 : 2;
        const hipError_t e =
            mode == 1 ? mcrt::gpu_build_bvh(g.dShapes, first, g.dIndices, g.dPositions, n, ctx->stream, &built, &info.depth)
                      : mcrt::gpu_build_sah(g.dShapes, first, g.dIndices, g.dPositions, n, plan.cost, plan.bins, plan.sah,
                                            ctx->stream, &built, &info.depth, &why);
        if (e == hipSuccess) {
            nodes.adopt(built, 4 * info.numNodes);
            return commit(s, opts, nodes, info, nullptr, t0);
        }
        // configurations the device SAH path does not reproduce (> 64 bins, a host whose rcpps the
        // table cannot model, pathological level counts) take the host build: same tree; so does a
        // device without room for the build's scratch (~230 B per triangle beyond the records)
        const bool hostInstead = mode != 1 && (e == hipErrorNotSupported || e == hipErrorInvalidValue || e == hipErrorOutOfMemory);
        if (!hostInstead) {
            drop(a);
            if (mode == 1)
                return fail(ctx, e == hipErrorOutOfMemory ? MCRT_ERROR_OUT_OF_MEMORY : MCRT_ERROR_DEVICE,
                            std::string("device LBVH build: ") + hipGetErrorString(e));
            return fail(ctx, MCRT_ERROR_DEVICE, std::string("device SAH build: ") + (why ? why : hipGetErrorString(e)));
        }
        (void)hipGetLastError();
        if (e == hipErrorOutOfMemory)
            std::fprintf(stderr, "mcrt: device SAH build out of memory, building the same tree on the host\n");
    }
    mcrt::HostTree t;
    const mcrt_float4* positions = mcrt::host_positions(s);   // downloaded after a device-side vertex update
    if (!positions) return fail(ctx, MCRT_ERROR_DEVICE, "download of the updated vertex positions failed");
    if (mcrt::build_host_tree(plan, g.shapes, g.numShapes, g.indices, positions, t) != MCRT_OK)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, plan.twoLevel ? "two-level BVH build failed" : "BVH build failed");
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    drop(a);   // room for the new records; a failed upload leaves no structure
    hipError_t e = (hipError_t)nodes.alloc(4 * t.numNodes);
    if (e == hipSuccess) e = hipMemcpy(nodes.get(), t.records, 64 * t.numNodes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, MCRT_ERROR_OUT_OF_MEMORY, std::string("BVH upload: ") + hipGetErrorString(e));
    return commit(s, opts, nodes, t, &t, t0);
}

// Shapes from which a top-level instance count the device builds the top tree when MCRT_TOP_BUILD
// is unset (tools/refit_time.py -> profiles/refit/refit_time.json, "threshold")
static constexpr size_t MCRT_TOP_DEVICE_MIN_SHAPES = 10000;

MCRT_API mcrt_status mcrt_accel_update_transforms(mcrt_scene s, const mcrt_shape* sh, uint32_t n,
                                                  const mcrt_mat4* world_to_local) {
    if (!s || !sh || n != mcrt::scene_geometry(s).numShapes)
        return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "shape count must not change");
    mcrt_ctx ctx = s->ctx;
    AccelState& a = s->accel;
    if (!a.dNodes) return fail(ctx, MCRT_ERROR_NOT_READY, "mcrt_accel_build has not been called");
    if (!mcrt::same_topology(sh, mcrt::scene_geometry(s).shapes, n, a.tree.twoLevel))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "shape topology must not change");
    if (const mcrt_status st = mcrt::check_updated_shapes(s, sh, n)) return st;   // before any state changes
    const auto t0 = Clock::now();
    hipSetDevice(ctx->device);
    // after every launch that reads the records or the shapes: the context stream and the
    // frame-slot streams of the context's frame buffers (as mcrt_ctx_synchronize reaches them)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipDeviceSynchronize());
    auto done = [&](int path) {
        a.updatePath = path;
        a.updateMs = ms_since(t0);
        return MCRT_OK;
    };
    if (!a.tree.twoLevel) {
        // RR's flat intersector rebuilds on every Commit: the last build's options again
        mcrt_status st = mcrt_scene_update_shapes(s, sh, n);
        if (st != MCRT_OK) return st;
        mcrt_accel_opts o = a.lastOpts;
        o.world_to_local = world_to_local;
        st = mcrt_accel_build(s, a.haveOpts ? &o : nullptr);
        if (st != MCRT_OK) return st;
        return done(3);
    }
    // the mesh keys are unchanged, so the surface records and their bases are too
    if (const mcrt_status st = mcrt::store_shapes(s, sh, n)) return st;
    const mcrt::SceneGeometry g = mcrt::scene_geometry(s);
    const mcrt::Bvh2lTop& top = a.top2l;
    const char* env = std::getenv("MCRT_TOP_BUILD");
    const bool forceHost = env && std::strcmp(env, "host") == 0;
    const bool forceDev = env && std::strcmp(env, "device") == 0;
    bool device = forceDev || (!forceHost && top.world.size() >= MCRT_TOP_DEVICE_MIN_SHAPES);
    std::string devWhy;
    if (device && top.bins > 64) {   // as mcrt_sahbuild.hip
        device = false;
        devWhy = "the device top-level build supports 2..64 bins";
    }
    int depth = 0, path = 2;
    float box[6];
    if (device) {
        hipError_t e = hipSuccess;
        const char* why = nullptr;
        DevBuf<mcrt_mat4> dW2l;
        if (!a.topDev) e = mcrt::top_build_create(top, &a.topDev);
        if (e == hipSuccess && world_to_local) e = mcrt::upload(dW2l, world_to_local, (size_t)n, ctx->stream);
        if (e == hipSuccess)
            e = mcrt::top_build_run(a.topDev, g.dShapes, dW2l.get(), a.dNodes.get(), ctx->stream, &depth, box, &why);
        if (dW2l) {
            (void)hipStreamSynchronize(ctx->stream);
            dW2l.reset();
        }
        if (e == hipSuccess) {
            path = 1;
        } else if (e == hipErrorNotSupported || e == hipErrorInvalidValue || e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            devWhy = why ? why : hipGetErrorString(e);   // the host path below rewrites the records
        } else {
            return fail(ctx, MCRT_ERROR_DEVICE, std::string("device top-level build: ") + hipGetErrorString(e));
        }
    }
    if (path == 2) {
        std::vector<float> rec(16 * a.tree.topNodes);
        mcrt::build_bvh2l_top(top, g.shapes, world_to_local, rec.data(), &depth, box);
        HIPCHK(ctx, hipMemcpy(a.dNodes.get(), rec.data(), 64 * a.tree.topNodes, hipMemcpyHostToDevice));
    }
    a.tree.depth = depth;
    std::memcpy(a.tree.box, box, sizeof(box));
    apply_spill_cap(a);
    done(path);
    if (forceDev && path != 1) return fail(ctx, MCRT_ERROR_DEVICE, "MCRT_TOP_BUILD=device: " + devWhy);
    return MCRT_OK;
}

// Refit of a flat structure (mcrt_refit.hip).  What the topology fixes stays as the
// build left it: depth, packets, the spill cap, qRoot, the compact records' offsets and size.  The
// occluder-hint table stays too: a hint is an exact leaf test plus the parent's stored box
// (mcrt_traverse.h hintOccludes: "any table content is safe"), and both were just rewritten.
MCRT_API mcrt_status mcrt_accel_refit(mcrt_scene s) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    mcrt_ctx ctx = s->ctx;
    AccelState& a = s->accel;
    if (!a.dNodes) return fail(ctx, MCRT_ERROR_NOT_READY, "mcrt_accel_build has not been called");
    const auto t0 = Clock::now();
    hipSetDevice(ctx->device);
    // as mcrt_accel_update_transforms: after every launch that reads the records
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipDeviceSynchronize());
    if (a.tree.twoLevel) {   // rebuilt: correct, not fast (refitting the per-mesh trees is DESIGN 2j's follow-up)
        mcrt_accel_opts o = a.lastOpts;
        const mcrt_status st = mcrt_accel_build(s, a.haveOpts ? &o : nullptr);
        if (st != MCRT_OK) return st;
        a.updatePath = 3;
        a.updateMs = ms_since(t0);
        return MCRT_OK;
    }
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)a.tree.numNodes;
    [[maybe_unused]] const int depth0 = a.tree.depth, cap0 = a.spillCap;
    [[maybe_unused]] const bool packets0 = a.packets;
    if (!a.refitParent) {   // the structure's first refit: everything a refit needs, once
        DevBuf<int> parent, arrive, flag;
        DevBuf<uint32_t> qoff;
        HIPCHK(ctx, parent.alloc(n));
        HIPCHK(ctx, arrive.alloc(n));
        HIPCHK(ctx, flag.alloc(4));
        HIPCHK(ctx, mcrt::launch_refit_parents(a.dNodes.get(), n, parent.get(), st));
        if (a.dQNodes) {
            size_t total = 0;
            HIPCHK(ctx, mcrt::refit_qnode_offsets(a.dNodes.get(), n, a.qOrder, qoff, &total, st));
            if (total != a.dQNodes.size()) return fail(ctx, MCRT_ERROR_DEVICE, "compact records: size changed without a build");
        }
        a.refitParent = std::move(parent);
        a.refitArrive = std::move(arrive);
        a.refitFlag = std::move(flag);
        a.refitQOff = std::move(qoff);
    }
    {
        Timed t(ctx, K_REFIT, nullptr, (int64_t)n);
        const mcrt::SceneGeometry g = mcrt::scene_geometry(s);
        HIPCHK(ctx, mcrt::launch_refit(a.dNodes.get(), n, g.dShapes, (uint32_t)g.numShapes, g.dIndices, g.dPositions,
                                       a.refitParent.get(), a.refitArrive.get(), st));
    }
    int unbounded = 0;
    if (a.dQNodes) {
        Timed t(ctx, K_REFIT_QNODES, nullptr, (int64_t)n);
        HIPCHK(ctx, mcrt::refit_qnodes(a.dNodes.get(), n, a.refitQOff.get(), a.dQNodes.get(), a.refitFlag.get(), st));
    }
    float root[16];
    if (a.dQNodes) HIPCHK(ctx, hipMemcpyAsync(&unbounded, a.refitFlag.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(root, a.dNodes.get(), sizeof(root), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (unbounded) {   // a box the bytes cannot bound: the 64-B walk answers the same, as after finish()
        a.dQNodes.reset();
        a.refitQOff.reset();
    }
    mcrt::root_record_box(root, a.tree.box);
    // the topology's, untouched by construction
    assert(a.tree.depth == depth0 && a.spillCap == cap0 && a.packets == packets0 && a.qRoot == (n == 1 ? 1u : 0u));
    a.updatePath = 4;
    a.updateMs = ms_since(t0);
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_accel_update_info(mcrt_scene s, int32_t* path, double* ms) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    if (path) *path = s->accel.updatePath;
    if (ms) *ms = s->accel.updateMs;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_accel_info(mcrt_scene s, uint64_t* num_nodes, uint64_t* device_bytes, double* build_ms,
                                     uint32_t* num_triangles) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    const AccelState& a = s->accel;
    if (num_nodes) *num_nodes = a.tree.numNodes;
    if (device_bytes) *device_bytes = 64ull * a.tree.numNodes + 16ull * a.dQNodes.size();
    if (build_ms) *build_ms = a.buildMs;
    if (num_triangles) *num_triangles = (uint32_t)a.tree.numTris;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_accel_layout(mcrt_scene s, int32_t* two_level, uint32_t* num_meshes,
                                       uint32_t* num_instances, int32_t* depth) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    const AccelState& a = s->accel;
    if (!a.dNodes) return fail(s->ctx, MCRT_ERROR_NOT_READY, "mcrt_accel_build has not been called");
    if (two_level) *two_level = a.tree.twoLevel ? 1 : 0;
    if (num_meshes) *num_meshes = (uint32_t)a.tree.numMeshes;
    if (num_instances) *num_instances = (uint32_t)a.tree.numInstances;
    if (depth) *depth = a.tree.depth;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_accel_read_records(mcrt_scene s, float* out, uint64_t max_records, uint64_t* num_records) {
    if (!s || !num_records) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    const AccelState& a = s->accel;
    if (!a.dNodes) return fail(s->ctx, MCRT_ERROR_INVALID_ARG, "scene has no acceleration structure");
    *num_records = a.tree.numNodes;
    if (!out) return MCRT_OK;
    mcrt_ctx ctx = s->ctx;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, a.dNodes.get(), 64 * std::min<uint64_t>(max_records, a.tree.numNodes), hipMemcpyDeviceToHost));
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_accel_read_compact(mcrt_scene s, void* out, uint64_t max_units, uint64_t* num_units,
                                             uint32_t* root_ref) {
    if (!s || !num_units) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    const AccelState& a = s->accel;
    if (!a.dNodes) return fail(s->ctx, MCRT_ERROR_INVALID_ARG, "scene has no acceleration structure");
    *num_units = a.dQNodes.size();
    if (root_ref) *root_ref = a.qRoot;
    if (!out || !a.dQNodes) return MCRT_OK;
    mcrt_ctx ctx = s->ctx;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, a.dQNodes.get(), 16 * std::min<uint64_t>(max_units, a.dQNodes.size()), hipMemcpyDeviceToHost));
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_accel_compact_order(const int32_t* kids, uint32_t n, int32_t order, uint32_t* off,
                                              uint64_t* num_units) {
    if (!kids || !off || !num_units || n == 0 || order < 1 || order > 2)
        return fail(nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument, no records or an unknown order");
    for (uint32_t i = 0; i < n; ++i) {   // parents before their children, every record some node's child once
        const int32_t l = kids[2 * (size_t)i], r = kids[2 * (size_t)i + 1];
        if (l < 0) continue;
        if ((uint32_t)l <= i || (uint32_t)l >= n || (uint32_t)r <= i || (uint32_t)r >= n || l == r)
            return fail(nullptr, MCRT_ERROR_INVALID_ARG, "child indices must lie above their parent's");
    }
    *num_units = mcrt::qnode_order_offsets(kids, n, order, off);
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_accel_builder(mcrt_scene s, int32_t* builder) {
    if (!s || !builder) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    *builder = s->accel.tree.builder;   // 0 for a two-level structure
    return MCRT_OK;
}

}  // extern "C"
