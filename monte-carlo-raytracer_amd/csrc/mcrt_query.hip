// mcrt_query.hip -- the RadeonRays-style ray queries on AoS rays: k_trace_rays and, below it, the
// entry points mcrt_trace_closest / _any, their counted forms with events, mcrt_event_wait and
// mcrt_event_destroy.  Of the runtime it takes trace_ctx, ensure_spill, accel_ready and Timed
// (mcrt_host.h).  Built with mcrt_kernels.o's flags, where the kernel came from.
#include <string>

#include "mcrt_host.h"
#include "mcrt_device.h"
#include "mcrt_traverse.h"

using mcrt::fail, mcrt::ensure_spill, mcrt::trace_ctx, mcrt::accel_ready;

// ---------------------------------------------------------------------------
// RadeonRays-compatible queries on AoS rays (mcrt_trace_closest / mcrt_trace_any).
// One ray per lane, one wave per workgroup (LDS stack 4 KB): the hardware dispatcher keeps
// 8 waves per SIMD resident and refills them as they finish -- measured faster on MI355X
// than a persistent grid pulling work from an atomic queue.
// ---------------------------------------------------------------------------
template <bool ANY, int LAY>
__global__ __launch_bounds__(64) void k_trace_rays(TraceCtx c, const mcrt_ray* __restrict__ rays, int n,
                                                   const int* __restrict__ countDev,
                                                   mcrt_intersection* __restrict__ hits, int* __restrict__ occl) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[STACK_LDS * 64];
    if (countDev) n = min(n, *countDev);   // RR's numrays in remote memory (radeon_rays.h:272-277)
    const int lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;
    if (i >= n) return;
    const mcrt_ray rr = rays[i];
    if (rr.extra[1] == 0) return;   // inactive: output untouched (intersect_bvh2_lds.cl:88)
    TraceRay r;
    r.o = ld3(rr.o);
    r.d = ld3(rr.d);
    r.tmax = rr.o.w;
    r.mask = rr.extra[0];
    if (ANY) {
        occl[i] = traceAny<LAY>(c, r, lds + lane, raySpill(c, blockIdx.x, lane)) ? 1 : -1;
        return;
    }
    float t;
    const float4 h4 = traceClosest<LAY>(c, r, lds + lane, raySpill(c, blockIdx.x, lane), t);
    if (__float_as_int(h4.z) >= 0) {
        mcrt_intersection h;
        h.shapeid = __float_as_int(h4.z);
        h.primid = __float_as_int(h4.w);
        h.padding[0] = h.padding[1] = 0;
        h.uvwt.x = h4.x; h.uvwt.y = h4.y; h.uvwt.z = 0.0f; h.uvwt.w = t;
        hits[i] = h;
    } else {
        hits[i].shapeid = -1;
        hits[i].primid = -1;
    }
}

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
        const TraceCtx c = trace_ctx(s);
        const dim3 g((n + 63) / 64), b(64);
        if (any)
            hipLaunchKernelGGL(pickLayout(c, k_trace_rays<true, LAY_TWO_LEVEL>, k_trace_rays<true, LAY_QUANT>,
                                          k_trace_rays<true, LAY_PLAIN>),
                               g, b, 0, ctx->stream, c, rays, n, countDev, hits, occl);
        else
            hipLaunchKernelGGL(pickLayout(c, k_trace_rays<false, LAY_TWO_LEVEL>, k_trace_rays<false, LAY_QUANT>,
                                          k_trace_rays<false, LAY_PLAIN>),
                               g, b, 0, ctx->stream, c, rays, n, countDev, hits, occl);
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

extern "C" {

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

}  // extern "C"
