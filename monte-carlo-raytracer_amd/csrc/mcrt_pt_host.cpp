// mcrt_pt_host.cpp -- the path tracer's host side and the frame slots it renders into: the slots'
// lifecycle (FrameSlot, mcrt_host.h), mcrt_render_frame(s) -- the argument checks, the slot choice and
// the hand-over to bdpt_render or to pt_render, the bounce driver -- mcrt_accumulate(_frames), and
// the read-backs of a PT call's counters and queues.  Only this file names a slot's queues, counter
// block, events and spill columns; the rest of the runtime borrows the current slot's camera hits
// through borrow_camera_hits / release_slot and reads its radiance, lastBatch and stream
// (mcrt_bdpt_host.cpp also the fields bdpt_render is handed).  The kernels and their launchers are
// mcrt_kernels.hip's; k_accumulate and its launcher are mcrt_film.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "mcrt_host.h"

using mcrt::fail, mcrt::env_int, mcrt::fb_sync, mcrt::frame_args, mcrt::trace_ctx, mcrt::packet_ctx, mcrt::with_hints,
    mcrt::scene_args, mcrt::accel_ready;

namespace {

const char* const kNoSlotBuffers = "the frame slot has no buffers (its last allocation failed)";

void slot_free(FrameSlot& k) {
    if (k.stream) hipStreamSynchronize(k.stream);
    if (k.done) hipEventDestroy(k.done);
    if (k.free) hipEventDestroy(k.free);
    if (k.stream) hipStreamDestroy(k.stream);
    k = FrameSlot();
}

// The slot with planes for `frames` frames and ray queues of qNeed entries (0: slot_alloc's least):
// allocated on first use; a smaller one is freed, once the accumulation of its last frame has read
// it and its stream has finished, and allocated again.  After a failure the slot is empty.
hipError_t slot_ensure(mcrt_framebuffer fb, FrameSlot& slot, int frames, size_t qNeed) {
    if (slot.stream) {
        if (slot.frames >= frames && slot.queueCap >= qNeed) return hipSuccess;
        const hipError_t e = hipEventSynchronize(slot.free);
        if (e != hipSuccess) return e;
        slot_free(slot);
    }
    return mcrt::slot_alloc(slot, fb->N, mcrt::tile_lanes(fb), frames, qNeed);
}

// MCRT_WAVE_CLOCK=1: record per-workgroup clocks of launch `which` (grid of `blocks`) on stream st
bool wave_clock_on() {
    static const bool on = env_int("MCRT_WAVE_CLOCK", 0) != 0;
    return on;
}
uint32_t* wave_clock_buf(mcrt_framebuffer fb, int which, size_t blocks, hipStream_t st) {
    if (!wave_clock_on()) return nullptr;
    DevBuf<uint32_t>& clk = fb->waveClk[which];
    if (clk.grow(2 * blocks, st) != 0) { hipGetLastError(); return nullptr; }
    hipMemsetAsync(clk.get(), 0, 4 * clk.size(), st);
    return clk.get();
}

#define MCRT_LPT_SHADE_MAX_PATHS 16000000
// MCRT_LONGEST_FIRST=0: camera / first-shading tiles in plain tile order (A/B)
bool longest_first() {
    static const bool on = env_int("MCRT_LONGEST_FIRST", 1) != 0;
    return on;
}

// The stop rule of the extension walks (mcrt::walk_rule) for the extension launches of bounces <=
// MCRT_WALK_MAXB (default 0: the first, full-size one).  At depth 5 the later, smaller launches --
// whose any-hit shadow blocks otherwise overlap the long walks' tail -- lost what the first gained:
// k_shadow_extend 2.951 ms per frame without the rule, 2.943 with it on every launch, 2.915 on the
// first only (profiles/r05/ab/README.txt item 20)
int walk_max_bounce() { return env_int("MCRT_WALK_MAXB", 0); }

// Frames in flight for a render: the frame buffer's setting; auto = 2.  Each launch of a frame ends
// in a divergent tail of long rays that the next frame's launches fill (San-Miguel proxy 1080p:
// 2.33 -> 1.91 ms/frame with 2 slots, 2.06 with 4; tools/scale_emulate.py).  Small per-rank band
// shares are widened by batching frames (mcrt_render_frames) rather than by more slots: 4 slots of
// 1/8-image frames reach 0.49 ms per frame at N = 8, 2 slots of 16-frame batches 0.25.
int frames_in_flight(mcrt_framebuffer fb) {
    // MCRT_WAVE_CLOCK=1: one frame in flight -- the clock buffers are per frame buffer, so two slots'
    // launches in flight would write the same per-workgroup entries
    if (wave_clock_on()) return 1;
    int n = fb->framesInFlight;
    if (n <= 0) n = 2;
    return std::max(1, std::min(n, MCRT_MAX_FRAMES_IN_FLIGHT));
}

// One PT call of f.batch frames in frame slot `slot`, enqueued on the slot's stream; the caller has
// made the slot ready (its buffers, spill columns and the wait for `free`).  Records the slot's `done`.
mcrt_status pt_render(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, const mcrt_frame_params* p,
                      FrameArgs f, FrameSlot& slot) {
    mcrt_ctx ctx = s->ctx;
    const int count = f.batch;
    // Adaptive sampling: the camera and first-shading launches cover the K tiles of the active list
    // (slot j takes tile list[j] through f.tileOrder, the table padded with numTiles so that a
    // surplus wave is invalid), and everything sized by the call's paths is sized by K.  The buffers
    // keep the whole image's capacity.
    const bool listed = mcrt::adaptive_on(fb);
    int tileSlots = f.numTiles;
    const uint32_t* const list = listed ? mcrt::adaptive_list(fb, &tileSlots) : nullptr;
    const int bandPaths = tileSlots * 64 * count;
    hipStream_t st = slot.stream;
    if (listed) mcrt::adaptive_rendered(fb, count);
    slot.lastMaxDepth = p->max_depth;
    slot.lastPixels = 0;
    fb->bands = f;
    fb->haveBands = true;
    SlotBlock* const blk = slot.block.get();
    mcrt_camera* dCam = blk->cam;
    float4 *const radiance = slot.radiance.get(), *const hitsP = slot.hitsP.get(), *const hitsE = slot.hitsE.get();
    float4 *const sO = slot.sO.get(), *const sD = slot.sD.get(), *const sL = slot.sL.get();
    HIPCHK(ctx, hipMemcpyAsync(dCam, cam, sizeof(mcrt_camera) * count, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(&blk->n, 0, sizeof(SlotCounts), st));
    int* const shadowCnt = blk->n.shadow;   // [b]
    int* const extCnt = blk->n.ext;         // [b]
    const SceneArgs sa = scene_args(s);
    fb->lastIntegrator = MCRT_INTEGRATOR_PT;
    if (mcrt::scene_num_lights(s) == 0) {   // RTPathTracingPass.cpp:42: no lights -> pass skipped; radiance = 0 here
        // every frame plane of the batch: accumulate reads `count` of them
        HIPCHK(ctx, hipMemsetAsync(radiance, 0, 16 * fb->N * (size_t)count, st));
        HIPCHK(ctx, hipEventRecord(slot.done, st));
        return MCRT_OK;
    }
    if (tileSlots == 0) {   // an empty list: no launch at all (never a zero-sized grid)
        HIPCHK(ctx, hipEventRecord(slot.done, st));
        return MCRT_OK;
    }
    TraceCtx tcs = trace_ctx(s);
    tcs.spill = slot.spill.get();
    const int qCap = bandPaths;
    TraceCtx tw = tcs;   // the extension walks' stop rule, when it applies: one suspend count per bounce
    if (p->max_depth > 1)
        HIPCHK(ctx, mcrt::walk_rule(tw, bandPaths, slot.suspend, slot.suspendCnt, MCRT_MAX_BOUNCES, (size_t)qCap, st));
    if (listed) {
        // the list takes the place of the longest-first order; no costs are recorded
        f.tileOrder = list;
    } else if (longest_first()) {
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
        if (listed && !(tcp.packet && !tcp.twoLevel)) {
            // the per-ray camera kernels take no tile table: every tile's camera ray, the hits of
            // the unlisted ones unused
            FrameArgs fc = f;
            fc.tileOrder = nullptr;
            mcrt::launch_primary(tcp, fc, dCam, hitsP, st);
        } else {
            mcrt::launch_primary(tcp, f, dCam, hitsP, st, listed ? tileSlots : -1);
        }
    }
    // a shadow launch's view for bounce b: this slot's spill columns, the occluder hints (bounce 0: by
    // pixel) and, at profiling level 2, their counter
    auto shadow_ctx = [&](TraceCtx t, int b) {
        t.spill = slot.spill.get();
        with_hints(t, s, b == 0 ? fb->hintPix.get() : nullptr, (uint32_t)fb->N);
        if (t.hint && ctx->countHints) t.hintHits = &blk->n.hintHits[b];
        return t;
    };
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
            if (!listed && (int64_t)bandPaths > MCRT_LPT_SHADE_MAX_PATHS) fs.tileOrder = nullptr;
            mcrt::launch_shade0(sa, fs, dCam, hitsP, radiance, q, st, listed ? tileSlots : -1);
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
            TraceCtx tse = shadow_ctx(b == 0 ? packet_ctx(s) : tcs, b);
            if (tse.qnodes && ctx->countHints) tse.retraces = &blk->n.retraces[b];
            if (b == 0) tse.waveClock = wave_clock_buf(fb, 1, 2 * (((size_t)qCap + 63) / 64), st);
            if (tw.walkCap > 0 && b <= walk_max_bounce()) {
                tse.walkCap = tw.walkCap;
                tse.walkLanes = tw.walkLanes;
                tse.suspend = tw.suspend;
                tse.suspendCount = slot.suspendCnt.get() + b;
            }
            mcrt::launch_shadow_extend(tse, extCnt + b, slot.eO[b & 1].get(), slot.eD[b & 1].get(), hitsE, shadowCnt + b,
                                       sO, sD, sL, radiance, qCap, qCap, st);
            if (tse.walkCap > 0) mcrt::launch_walk_resume(tse, slot.eO[b & 1].get(), slot.eD[b & 1].get(), hitsE, qCap, st);
        } else {
            Timed t(ctx, K_SHADOW, shadowCnt + b, 0, st);
            TraceCtx tsh = shadow_ctx(tcs, b);
            tsh.waveClock = wave_clock_buf(fb, 2, ((size_t)qCap + 63) / 64, st);
            mcrt::launch_shadow(tsh, shadowCnt + b, sO, sD, sL, radiance, qCap, st);
        }
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(slot.done, st));
    slot.lastPixels = (int64_t)bandPaths;
    return MCRT_OK;
}

mcrt_status render_frames(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, int count,
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
    if (p->sampler == MCRT_SAMPLER_SOBOL && !mcrt::scene_has_sobol(s))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "Sobol sampler requires the 1024x52 Sobol matrices in the scene");
    if (p->integrator != MCRT_INTEGRATOR_PT && p->integrator != MCRT_INTEGRATOR_BDPT)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "unknown integrator");
    if (mcrt::adaptive_on(fb)) {
        if (p->integrator == MCRT_INTEGRATOR_BDPT)   // its light-tracing splats land in any tile
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "adaptive mode renders with the path tracer only (no BDPT)");
        if (p->num_bands > 1) return fail(ctx, MCRT_ERROR_INVALID_ARG, "adaptive mode takes no band split (num_bands > 1)");
    }
    if (mcrt::bdpt_pending_gather(fb))
        return fail(ctx, MCRT_ERROR_NOT_READY, "band-split BDPT frame not completed (mcrt_bdpt_gather)");
    FrameArgs f;
    std::string err;
    if (!frame_args(fb, p, f, err)) return fail(ctx, MCRT_ERROR_INVALID_ARG, err);
    hipSetDevice(ctx->device);
    f.batch = count;
    // frame slot: its buffers are free once the accumulation of its previous frame has read them
    const bool bdpt = p->integrator == MCRT_INTEGRATOR_BDPT;
    int S = bdpt ? mcrt::bdpt_sets(fb, frames_in_flight(fb)) : frames_in_flight(fb);
    int ks = fb->next % S;
    if (bdpt && ks != 0) {   // a BDPT set that does not fit in device memory sends the frame to slot 0
        bool usable = true;
        const mcrt_status r = mcrt::bdpt_reserve_set(fb, ks, p->max_depth, count, &usable);
        if (r != MCRT_OK) return r;
        if (!usable) {   // ... as every BDPT frame from now on (bdpt_sets)
            ks = 0;
            S = 1;
        }
    }
    FrameSlot& slot = fb->slot[ks];
    // the queues hold at most the batch's paths of the band: size the ray grids to them (PT; BDPT's
    // queues are its set's)
    const int bandPaths = f.numTiles * 64 * count;
    const size_t qNeed = bdpt ? 0 : std::max(fb->N, (size_t)bandPaths);
    HIPCHK(ctx, slot_ensure(fb, slot, count, qNeed));
    if (!bdpt) {
        const int cap = mcrt::accel_spill_cap(s);
        const size_t spillRays = (std::max((size_t)bandPaths, 2 * qNeed + 64) + 63) / 64 * 64;
        HIPCHK(ctx, slot.spill.grow(spillRays * cap, slot.stream));
    }
    HIPCHK(ctx, hipStreamWaitEvent(slot.stream, slot.free, 0));
    fb->cur = ks;
    fb->next = (ks + 1) % S;
    slot.lastBatch = count;
    if (!bdpt) return pt_render(s, fb, cam, p, f, slot);
    const mcrt_status r = mcrt::bdpt_render(s, fb, cam, p, f, ks, slot);   // BDPT frames overlap the same way (set ks)
    hipEventRecord(slot.done, slot.stream);
    return r;
}

mcrt_status accumulate(mcrt_framebuffer fb, const mcrt_filter* filters, int nfilters, int32_t frame_index) {
    if (!fb || !filters) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    if (mcrt::bdpt_pending_gather(fb))
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
    if (!slot.block) return fail(ctx, MCRT_ERROR_NOT_READY, kNoSlotBuffers);
    // adaptive sampling: only the tiles of the list the call rendered with, each at its own count
    const bool listed = mcrt::adaptive_on(fb);
    int tiles = fb->bands.numTiles;
    const uint32_t *list = nullptr, *tileCount = nullptr;
    if (listed) {
        const mcrt_status ok = mcrt::adaptive_check_accumulate(fb, frame_index);
        if (ok != MCRT_OK) return ok;
        list = mcrt::adaptive_list(fb, &tiles);
        tileCount = mcrt::adaptive_counts(fb);
    }
    FrameArgs f = fb->bands;
    f.batch = batch;
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, slot.done, 0));   // the frame's render (its slot stream)
    // weights are evaluated on the device (k_accumulate, filters.cl); the filters go to the slot's
    // block, which its next render (after slot.free below) does not touch before this launch
    mcrt_filter* dFilt = slot.block.get()->filt;
    HIPCHK(ctx, hipMemcpyAsync(dFilt, filters, sizeof(mcrt_filter) * nfilters, hipMemcpyHostToDevice, ctx->stream));
    if (tiles > 0) {   // (an empty list: nothing to add)
        Timed t(ctx, K_ACCUM, nullptr, (int64_t)tiles * 64 * batch);
        mcrt::launch_accumulate(f, frame_index, dFilt, nfilters == 1 ? 0 : 1, slot.radiance.get(), fb->wsum.get(), fb->wts.get(),
                                fb->image.get(), ctx->stream, list, tiles, tileCount);
    }
    if (fb->dn.momentsOn) {   // the same frames' luminance moments, before the slot is released
        if (tiles > 0) {
            Timed t(ctx, K_MOMENTS, nullptr, (int64_t)tiles * 64 * batch);
            mcrt::launch_moments(f, frame_index, slot.radiance.get(), fb->dn.moments.get(), ctx->stream, list, tiles, tileCount);
        }
        fb->dn.momentFrames = frame_index == 0 ? batch : fb->dn.momentFrames + batch;
    }
    if (listed) mcrt::adaptive_accumulated(fb, batch, ctx->stream);   // after both: they read the counts
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(slot.free, ctx->stream));   // the slot may take its next frame
    return MCRT_OK;
}

// The counters of the current slot's last PT call, once every stream has finished.  Which entries are
// live is each caller's rule.
mcrt_status read_counts(mcrt_framebuffer fb, SlotCounts* n) {
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    HIPCHK(ctx, hipMemcpy(n, cur_slot(fb).block.get(), sizeof(SlotCounts), hipMemcpyDeviceToHost));   // the block's head
    return MCRT_OK;
}
// the same for the per-bounce read-backs, which take `max` entries
mcrt_status read_counts(mcrt_framebuffer fb, int max, SlotCounts* n) {
    if (!fb || max < 0) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    return read_counts(fb, n);
}
// bounces of the last call when it was a PT call, else none
int pt_bounces(mcrt_framebuffer fb) {
    return fb->lastIntegrator == MCRT_INTEGRATOR_PT ? cur_slot(fb).lastMaxDepth : 0;
}

}  // namespace

// Per-frame planes (radiance, primary hits) for `frames` frames of N pixels; ray queues of Q entries.
// N: pixels; T: the frame's 8x8 tiles x 64 (the packed hit slots, mcrt_shading.h hitSlot)
hipError_t mcrt::slot_alloc(FrameSlot& k, size_t N, size_t T, int frames, size_t Q) {
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
    A(k.block, 1);
    k.frames = frames;
    k.queueCap = Q;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&k.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&k.done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&k.free, hipEventDisableTiming);
    // zero-fills on the slot's own stream, ahead of its first launch; `done` covers them for
    // readers on other streams (ctx_wait_slots) before the slot's first frame records it
    if (e == hipSuccess) e = hipMemsetAsync(k.radiance.get(), 0, 16 * N * frames, k.stream);
    if (e == hipSuccess) e = hipMemsetAsync(k.block.get(), 0, sizeof(SlotBlock), k.stream);
    if (e == hipSuccess) e = hipEventRecord(k.done, k.stream);
    if (e != hipSuccess) slot_free(k);
    return e;
}

void mcrt::fb_free(mcrt_framebuffer fb) {
    for (auto& k : fb->slot) slot_free(k);
}

mcrt_status mcrt::borrow_camera_hits(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, const FrameArgs& f,
                                     mcrt_camera** dCamOut, float4** hitsOut) {
    mcrt_ctx ctx = s->ctx;
    hipStream_t st = ctx->stream;
    FrameSlot& slot = cur_slot(fb);
    if (!slot.block) return fail(ctx, MCRT_ERROR_NOT_READY, kNoSlotBuffers);
    ctx_wait_slots(fb);
    mcrt_camera* dCam = slot.block.get()->cam;
    HIPCHK(ctx, hipMemcpyAsync(dCam, cam, sizeof(mcrt_camera), hipMemcpyHostToDevice, st));
    if (!ensure_spill(s, std::max((size_t)f.numTiles * 64, 2 * fb->N + 64)))
        return fail(ctx, MCRT_ERROR_OUT_OF_MEMORY, "traversal spill buffer");
    const TraceCtx tcs = packet_ctx(s);
    launch_primary(tcs, f, dCam, slot.hitsP.get(), st);
    *dCamOut = dCam;
    *hitsOut = slot.hitsP.get();
    return MCRT_OK;
}

hipError_t mcrt::release_slot(mcrt_framebuffer fb, hipStream_t st) { return hipEventRecord(cur_slot(fb).free, st); }

extern "C" {

MCRT_API mcrt_status mcrt_framebuffer_set_frames_in_flight(mcrt_framebuffer fb, int32_t n) {
    if (!fb || n < 0 || n > MCRT_MAX_FRAMES_IN_FLIGHT)
        return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "frames in flight must be 0 (auto) .. 4");
    fb->framesInFlight = n;
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

MCRT_API mcrt_status mcrt_accumulate(mcrt_framebuffer fb, const mcrt_filter* filter, int32_t frame_index) {
    return accumulate(fb, filter, 1, frame_index);
}

MCRT_API mcrt_status mcrt_accumulate_frames(mcrt_framebuffer fb, const mcrt_filter* filters, int32_t count,
                                            int32_t frame_index) {
    return accumulate(fb, filters, count, frame_index);
}

MCRT_API mcrt_status mcrt_framebuffer_stats(mcrt_framebuffer fb, int64_t* closest_rays, int64_t* any_rays,
                                            int64_t* shaded_paths) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    const FrameSlot& slot = cur_slot(fb);
    if (fb->lastIntegrator == MCRT_INTEGRATOR_BDPT) {   // closest: all subpath rays; any: connection rays
        hipSetDevice(ctx->device);
        HIPCHK(ctx, fb_sync(fb));
        int64_t cl = 0, an = 0;
        HIPCHK(ctx, mcrt::bdpt_ray_counts(fb, slot.lastMaxDepth, &cl, &an));
        if (closest_rays) *closest_rays = cl;
        if (any_rays) *any_rays = an;
        if (shaded_paths) *shaded_paths = cl;
        return MCRT_OK;
    }
    SlotCounts n;
    const mcrt_status st = read_counts(fb, &n);
    if (st != MCRT_OK) return st;
    int64_t cl = slot.lastPixels, an = 0, sh = slot.lastPixels;
    for (int b = 0; b < slot.lastMaxDepth; ++b) {
        an += n.shadow[b];
        if (b + 1 < slot.lastMaxDepth) { cl += n.ext[b]; sh += n.ext[b]; }
    }
    if (closest_rays) *closest_rays = cl;
    if (any_rays) *any_rays = an;
    if (shaded_paths) *shaded_paths = sh;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_queue_counts(mcrt_framebuffer fb, int32_t* shadow, int32_t* extension, int max) {
    SlotCounts n;
    const mcrt_status st = read_counts(fb, max, &n);
    if (st != MCRT_OK) return st;
    for (int b = 0; b < max && b < MCRT_MAX_BOUNCES; ++b) {
        const bool live = b < pt_bounces(fb);
        if (shadow) shadow[b] = live ? n.shadow[b] : 0;
        if (extension) extension[b] = live && b + 1 < pt_bounces(fb) ? n.ext[b] : 0;
    }
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_hint_counts(mcrt_framebuffer fb, int32_t* hits, int max) {
    SlotCounts n;
    const mcrt_status st = read_counts(fb, max, &n);
    if (st != MCRT_OK) return st;
    for (int b = 0; b < max && b < MCRT_MAX_BOUNCES; ++b)
        if (hits) hits[b] = b < pt_bounces(fb) ? n.hintHits[b] : 0;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_retrace_counts(mcrt_framebuffer fb, int32_t* retraces, int max) {
    SlotCounts n;
    const mcrt_status st = read_counts(fb, max, &n);
    if (st != MCRT_OK) return st;
    for (int b = 0; b < max && b < MCRT_MAX_BOUNCES; ++b)
        if (retraces) retraces[b] = b + 1 < pt_bounces(fb) ? n.retraces[b] : 0;
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
    SlotCounts c;
    const mcrt_status st = read_counts(fb, &c);
    if (st != MCRT_OK) return st;
    const int b = which == 0 ? slot.lastMaxDepth - 1 : slot.lastMaxDepth - 2;   // last shadow / last extension queue
    const int n = b < 0 ? 0 : (which == 0 ? c.shadow[b] : c.ext[b]);
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

MCRT_API mcrt_status mcrt_framebuffer_stream(mcrt_framebuffer fb, void** stream) {
    if (!fb || !stream) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    const FrameSlot& slot = cur_slot(fb);
    *stream = (void*)(slot.stream ? slot.stream : fb->ctx->stream);
    return MCRT_OK;
}

}  // extern "C"
