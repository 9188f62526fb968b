// mcrt_bdpt_host.cpp -- the bidirectional integrator's host side: its state (BdptState, held by the
// frame buffer as fb->bd), the driver of one BDPT call, the fall-back to one set when a second does
// not fit, and the band split's splat exchange (dense and sparse) with its entry points.  The
// kernels and their launchers are mcrt_bdpt.hip's; the rest of the runtime reaches this file
// through the five functions mcrt_host.h declares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <string>

#include "mcrt_bands.h"
#include "mcrt_host.h"

using mcrt::fail, mcrt::env_int, mcrt::fb_sync, mcrt::trace_ctx, mcrt::packet_ctx, mcrt::with_hints, mcrt::scene_args,
    mcrt::tile_lanes;

namespace {

// BDPT queue counters (64 ints per frame set): [d] the subpath-ray queue of depth d (d <= 33;
// at depth 0 the light rays only), then these
enum { BDPT_CNT_CONN = 40, BDPT_CNT_CAM0 = 41, BDPT_CNT_SPLATS = 42 };

// the light-tracing strategies (t = 1) evaluated by the vertex launches that create their
// light vertices instead of by a connection launch that re-reads them (MCRT_BDPT_LIGHT_IN_VERTEX)
int bdpt_light_in_vertex() { return env_int("MCRT_BDPT_LIGHT_IN_VERTEX", 1) != 0; }

// The set of the last BDPT call, as cur_slot (mcrt_host.h) is the slot of the last rendered frame
BdptSet& cur_set(mcrt_framebuffer fb) { return fb->bd.set[fb->bd.cur]; }

// N: pixels.  NQ = the pixels of the whole 8x8 tiles covering the image (>= N): the start queues hold
// one slot per lane of the tile walk.  Ray queues and hits hold 2 x NQ (the depth-1 camera and light halves).
hipError_t set_alloc(BdptSet& b, size_t N, size_t NQ, int D, int frames, hipStream_t st) {
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
hipError_t ensure_state(mcrt_framebuffer fb, int D, int k, int frames, hipStream_t st) {
    BdptState& bd = fb->bd;
    const size_t N = fb->N;
    if (bd.depth != D) {
        fb_sync(fb);
        bd.reset();
        hipError_t e = (hipError_t)bd.sampLight.alloc(N * D);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&bd.connect, hipEventDisableTiming);
        // zeroed on this frame's stream; every connect launch (the planes' only reader and writer)
        // waits for `connect`, recorded here first
        if (e == hipSuccess) e = hipMemsetAsync(bd.sampLight.get(), 0, 16 * N * D, st);
        if (e == hipSuccess) e = hipEventRecord(bd.connect, st);
        if (e != hipSuccess) { bd.reset(); return e; }
        bd.depth = D;
    }
    BdptSet& bs = bd.set[k];
    if (bs.camV && bs.frames < frames) {   // a larger batch: the set's last frames must be done
        fb_sync(fb);
        bs = BdptSet();
    }
    if (!bs.camV) return set_alloc(bs, N, tile_lanes(fb), D, frames, st);
    return hipSuccess;
}

// The launch arguments of a gather over the last call's set (also the head of a whole call's)
BdptArgs gather_args(mcrt_framebuffer fb) {
    const BdptSet& bs = cur_set(fb);
    BdptArgs b{};
    b.slots = bs.slots.get();
    b.splat = bs.splat.get();
    b.ownSlots = bdpt_max_connections(fb->bd.depth) - fb->bd.depth;
    return b;
}

// Sparse exchange: the splat list of set bs (cap records) and the band layout that names a row's owner
void splat_list_args(BdptArgs& b, mcrt_framebuffer fb, const BdptSet& bs, size_t cap) {
    const FrameArgs& f = fb->bands;
    b.splatList = bs.splatList.get();
    b.splatListCount = bs.bdptCounters.get() + BDPT_CNT_SPLATS;
    b.splatListCap = (int)std::min(cap, (size_t)INT32_MAX);
    b.splatW = (int)f.W;
    b.splatN0 = (int)(f.W * f.H);
    b.splatBpb = f.bandRows / 8;
    b.splatBands = f.numBands;
    b.splatBand = f.bandIndex;
}

// Makes st wait for every other slot's completed frame: a caller's exchange buffer may still be in
// use by an earlier call on another frame slot's stream
hipError_t wait_other_slots(mcrt_framebuffer fb, hipStream_t st) {
    for (auto& k : fb->slot)
        if (k.stream && k.stream != st) {
            const hipError_t e = hipStreamWaitEvent(st, k.done, 0);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// pixels of one frame's chunk of the rank-major splat layout: the largest rank's rows x W
size_t splat_chunk_pixels(const FrameArgs& f) {
    return (size_t)mcrt::band_max_rows(f.H, f.bandRows, f.numBands) * f.W;
}

// Completes a band-split frame: the gather over the rank's own rows, with its chunk of the summed
// splats (dense exchange) or its own plane (chunk NULL)
mcrt_status finish_gather(mcrt_framebuffer fb, FrameSlot& slot, const float* chunk, size_t chunkPixels) {
    mcrt_ctx ctx = fb->ctx;
    hipStream_t st = slot.stream;
    const BdptArgs b = gather_args(fb);
    {
        Timed t(ctx, K_BDPT_GATHER, nullptr, (int64_t)fb->bands.numTiles * 64 * fb->bands.batch, st);
        mcrt::launch_bdpt_gather(fb->bands, b, slot.radiance.get(), chunk, chunkPixels, st);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(slot.done, st));
    fb->bd.pendingGather = false;
    return MCRT_OK;
}

}  // namespace

void BdptState::reset() {
    for (auto& b : set) b = BdptSet();
    sampLight.reset();
    if (connect) hipEventDestroy(connect);
    connect = nullptr;
    depth = 0;
}

int mcrt::bdpt_sets(mcrt_framebuffer fb, int slots) { return fb->bd.oneSet ? 1 : slots; }
bool mcrt::bdpt_pending_gather(mcrt_framebuffer fb) { return fb->bd.pendingGather; }

mcrt_status mcrt::bdpt_reserve_set(mcrt_framebuffer fb, int k, int depth, int frames, bool* usable) {
    BdptState& bd = fb->bd;
    *usable = true;
    if (bd.depth != depth || bd.set[k].camV) return MCRT_OK;   // held already, or bdpt_render makes it
    // each BDPT set holds ~C x N x 48 B of connection rays (2.5 GB at 1080p, D = 2): when a
    // second one does not fit, fall back to one frame in flight instead of failing the frame
    // (zero-filled on slot k's stream when it exists, else on slot 0's and finished here: set k
    // is then first written on slot k's stream)
    hipStream_t zs = fb->slot[k].stream ? fb->slot[k].stream : fb->slot[0].stream;
    hipError_t e = set_alloc(bd.set[k], fb->N, tile_lanes(fb), depth, frames, zs);
    if (e == hipSuccess && zs != fb->slot[k].stream) e = hipStreamSynchronize(zs);
    if (e == hipErrorOutOfMemory) {
        hipGetLastError();
        bd.oneSet = true;
        *usable = false;
    } else if (e != hipSuccess) {
        return fail(fb->ctx, MCRT_ERROR_DEVICE, std::string("BDPT buffers: ") + hipGetErrorString(e));
    }
    return MCRT_OK;
}

hipError_t mcrt::bdpt_ray_counts(mcrt_framebuffer fb, int depth, int64_t* closest, int64_t* any) {
    int c[64];
    const hipError_t e = hipMemcpy(c, cur_set(fb).bdptCounters.get(), sizeof(c), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    int64_t cl = 0;
    for (int d = 0; d <= depth; ++d) cl += c[d];
    *closest = cl + c[BDPT_CNT_CAM0];
    *any = c[BDPT_CNT_CONN];
    return hipSuccess;
}

// RTBDPTPass::update (RTBDPTPass.cpp:67-128): start vertices, D+1 rounds of (trace, vertex),
// connections + MIS, visibility, gather.  Rays of both subpaths share one compacted queue.
mcrt_status mcrt::bdpt_render(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, const mcrt_frame_params* p,
                              const FrameArgs& f, int k, FrameSlot& slot) {
    // frame slot k on its stream: per-frame arrays of set k; the connect launch (the only reader
    // and writer of the shared sampled-light-vertex planes) waits for the previous frame's connect
    mcrt_ctx ctx = s->ctx;
    BdptState& bd = fb->bd;
    hipStream_t st = slot.stream;
    const int D = p->max_depth;
    const int B = f.batch;   // frames of this call (mcrt_render_frames): path = k * W*H + pixel
    HIPCHK(ctx, ensure_state(fb, D, k, B, st));
    BdptSet& bs = bd.set[k];
    bd.cur = k;
    slot.lastMaxDepth = D;
    slot.lastPixels = 0;
    fb->bands = f;
    fb->haveBands = true;
    fb->lastIntegrator = MCRT_INTEGRATOR_BDPT;
    bd.batch = B;
    mcrt_camera* dCam = slot.block.get()->cam;
    HIPCHK(ctx, hipMemcpyAsync(dCam, cam, sizeof(mcrt_camera) * B, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(bs.bdptCounters.get(), 0, 64 * sizeof(int), st));
    if (mcrt::scene_num_lights(s) == 0) {   // RTBDPTPass.cpp:69: no lights -> pass skipped
        HIPCHK(ctx, hipMemsetAsync(slot.radiance.get(), 0, 16 * fb->N * (size_t)B, st));
        return MCRT_OK;
    }
    const size_t N = fb->N * (size_t)B, C = (size_t)bdpt_max_connections(D);   // N: paths of the batch
    const size_t NQ = tile_lanes(fb) * (size_t)B;
    // spill columns: one per ray of the widest closest-hit launch (2 NQ) and one per wave of the
    // grid-stride visibility launch (mcrt::BDPT_VIS_MAX_WAVES)
    const size_t spillWords = (std::max(2 * NQ, (size_t)mcrt::BDPT_VIS_MAX_WAVES * 64) + 63) / 64 * 64 * (size_t)mcrt::accel_spill_cap(s);
    HIPCHK(ctx, bs.spill.grow(spillWords, st));
    TraceCtx tcs = trace_ctx(s);
    tcs.spill = bs.spill.get();
    const SceneArgs sa = scene_args(s);
    // a bounce queue holds at most the band's camera + light rays (2 per path of this rank's tiles),
    // appended compactly from slot 0: sort (and clear) only that range, not the whole frame's -- a
    // rank of a band split would otherwise sort 8 x its own rays at N = 8
    const int bandQ = f.numTiles * 64 * B;   // this rank's paths: a start queue holds at most one ray each
    const int nSort = (int)std::min((size_t)2 * N, (size_t)2 * (size_t)bandQ);
    // the closest-hit launches' stop rule (TraceCtx::walkCap): a traced queue holds at most
    // max(bandQ, nSort) = nSort rays; one suspend count per traced queue
    TraceCtx tce = tcs;
    HIPCHK(ctx, mcrt::walk_rule(tce, (int64_t)f.numTiles * 64 * B, bs.suspend, bs.suspendCnt, 64, (size_t)nSort, st));
    const int wcap = tce.walkCap;
    BdptArgs b = gather_args(fb);
    b.camV = bs.camV.get();
    b.lightV = bs.lightV.get();
    b.camCount = bs.camCount.get();
    b.lightCount = bs.lightCount.get();
    b.sampLight = bd.sampLight.get();
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
    const bool sparse = bandSplit && bd.splatExchange == MCRT_SPLAT_EXCHANGE_SPARSE;
    if (sparse) {
        // the splats landing in other ranks' rows go to a list (at most D per path: t = 1, s = 2..D+1);
        // the rank's own rows are zeroed by k_bdpt_start, the other rows of its plane stay unused
        const size_t cap = (size_t)D * (size_t)bandQ;
        HIPCHK(ctx, bs.splatList.grow(cap, st));
        if (!bs.splatAux) HIPCHK(ctx, bs.splatAux.alloc(128));
        splat_list_args(b, fb, bs, cap);
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
    HIPCHK(ctx, hipStreamWaitEvent(st, bd.connect, 0));   // sampled-light planes in frame order
    {
        Timed t(ctx, K_BDPT_CONNECT, nullptr, (int64_t)f.numTiles * 64 * B, st);
        mcrt::launch_bdpt_connect(sa, f, b, dCam, cq, st);
    }
    HIPCHK(ctx, hipEventRecord(bd.connect, st));
    {
        Timed t(ctx, K_BDPT_VIS, cq.count, 0, st);
        TraceCtx tvis = tcs;
        with_hints(tvis, s, nullptr, 0);   // occluder hints by origin cell
        mcrt::launch_bdpt_vis(tvis, b, cq, (int)(C * N), st);
    }
    if (bandSplit) {   // completed by mcrt_bdpt_gather once the ranks' splats are summed
        bd.pendingGather = true;
    } else {
        Timed t(ctx, K_BDPT_GATHER, nullptr, (int64_t)f.numTiles * 64 * B, st);
        mcrt::launch_bdpt_gather(f, b, slot.radiance.get(), nullptr, 0, st);
    }
    HIPCHK(ctx, hipGetLastError());
    slot.lastPixels = (int64_t)f.numTiles * 64 * B;
    return MCRT_OK;
}

extern "C" {

// Rank-major splat layout of a band split of H rows into num_bands interleaved sets of band_rows
// rows: chunks = num_bands, each of (the largest rank's 8-row block count) x 8 rows x W pixels.
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
    if (fb->bd.pendingGather) return fail(fb->ctx, MCRT_ERROR_NOT_READY, "band-split BDPT frame not completed");
    fb->bd.splatExchange = mode;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_bdpt_splats_sparse(mcrt_framebuffer fb, void* d_dst, int64_t capacity, int64_t* counts,
                                             int32_t num_counts) {
    if (!fb || !counts) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    const int bands = fb->bands.numBands;
    if (num_counts < bands) return fail(ctx, MCRT_ERROR_INVALID_ARG, "counts must hold num_bands entries");
    for (int r = 0; r < num_counts; ++r) counts[r] = 0;
    if (!fb->bd.pendingGather) return MCRT_OK;   // nothing pending (light-less scene): no splats
    if (fb->bd.splatExchange != MCRT_SPLAT_EXCHANGE_SPARSE)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame rendered with the dense splat exchange (mcrt_bdpt_splats_copy)");
    if (bands > 64) return fail(ctx, MCRT_ERROR_INVALID_ARG, "sparse splat exchange: at most 64 bands");
    hipSetDevice(ctx->device);
    BdptSet& bs = cur_set(fb);
    hipStream_t st = cur_slot(fb).stream;
    BdptArgs b{};
    splat_list_args(b, fb, bs, bs.splatList.size());
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
    // before this call's all-to-all (ordered after this grouping on this stream) overwrites it
    HIPCHK(ctx, wait_other_slots(fb, st));
    mcrt::launch_splat_group(b, off, bs.splatAux.get() + 64, (float4*)d_dst, st);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;   // grouping enqueued on the frame's stream
}

MCRT_API mcrt_status mcrt_bdpt_gather_sparse(mcrt_framebuffer fb, const void* d_recv, int64_t records) {
    if (!fb || (records > 0 && !d_recv)) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    if (!fb->bd.pendingGather) return MCRT_OK;
    if (fb->bd.splatExchange != MCRT_SPLAT_EXCHANGE_SPARSE)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame rendered with the dense splat exchange (mcrt_bdpt_gather)");
    if (records < 0 || records > INT32_MAX) return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad record count");
    hipSetDevice(ctx->device);
    FrameSlot& slot = cur_slot(fb);
    mcrt::launch_splat_unpack((const float4*)d_recv, (int)records, cur_set(fb).splat.get(), slot.stream);
    return finish_gather(fb, slot, nullptr, 0);   // the rank's own plane
}

MCRT_API mcrt_status mcrt_bdpt_splats_copy(mcrt_framebuffer fb, void* d_dst) {
    if (!fb || !d_dst) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    if (fb->bd.pendingGather && fb->bd.splatExchange == MCRT_SPLAT_EXCHANGE_SPARSE)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame rendered with the sparse splat exchange (mcrt_bdpt_splats_sparse)");
    if (!fb->haveBands) return fail(ctx, MCRT_ERROR_NOT_READY, "no frame rendered yet");
    hipSetDevice(ctx->device);
    const size_t chunk = splat_chunk_pixels(fb->bands);   // per frame; a rank's chunk holds batch of them
    const size_t total = chunk * (size_t)std::max(fb->bands.batch, 1) * (size_t)fb->bands.numBands;
    FrameSlot& slot = cur_slot(fb);
    hipStream_t st = slot.stream ? slot.stream : ctx->stream;
    // the caller's buffer may still be read by an earlier frame's gather on another slot's stream
    HIPCHK(ctx, wait_other_slots(fb, st));
    HIPCHK(ctx, hipMemsetAsync(d_dst, 0, sizeof(float) * MCRT_SPLAT_CHANNELS * total, st));
    if (fb->bd.pendingGather)   // (else, e.g. a scene without lights: the frame is complete, no splats)
        mcrt::launch_bdpt_splat_pack(fb->bands, chunk, cur_set(fb).splat.get(), (float*)d_dst, st);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;   // enqueued on the frame's stream (mcrt_framebuffer_stream): no host sync
}

MCRT_API mcrt_status mcrt_bdpt_gather(mcrt_framebuffer fb, const void* d_own_chunk) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    if (!fb->bd.pendingGather) return MCRT_OK;   // nothing deferred (whole-image or light-less frame)
    if (fb->bd.splatExchange == MCRT_SPLAT_EXCHANGE_SPARSE)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame rendered with the sparse splat exchange (mcrt_bdpt_gather_sparse)");
    hipSetDevice(ctx->device);
    return finish_gather(fb, cur_slot(fb), (const float*)d_own_chunk, splat_chunk_pixels(fb->bands));
}

MCRT_API mcrt_status mcrt_framebuffer_read_bdpt(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                uint64_t* needed) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    const BdptState& bd = fb->bd;
    if (bd.depth <= 0) return fail(ctx, MCRT_ERROR_INVALID_ARG, "no BDPT frame rendered yet");
    // the planes of the last BDPT call's batch (plane stride N x batch)
    const size_t N = fb->N * (size_t)bd.batch, D = (size_t)bd.depth;
    const size_t C = (size_t)bdpt_max_connections(bd.depth);
    const BdptSet& bs = cur_set(fb);
    const void* src = nullptr;
    size_t sz = 0;
    switch (which) {
    case 0: src = bs.camV.get(); sz = 16 * N * BDPT_VERTEX_PLANES * (D + 2); break;
    case 1: src = bs.lightV.get(); sz = 16 * N * BDPT_VERTEX_PLANES * (D + 1); break;
    case 2: src = bs.camCount.get(); sz = 4 * N; break;
    case 3: src = bs.lightCount.get(); sz = 4 * N; break;
    case 4: src = bs.slots.get(); sz = 16 * N * (C - D); break;
    case 5: src = bd.sampLight.get(); sz = 16 * fb->N * D; break;   // per pixel, carried across frames
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

}  // extern "C"
