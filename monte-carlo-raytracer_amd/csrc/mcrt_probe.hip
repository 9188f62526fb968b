// mcrt_probe.hip -- the roofline probes behind bench.py's ceilings: kernels and their three entry
// points.  No renderer state; each call allocates its arrays, times its launches and frees them.
//
//   mcrt_ctx_stream_copy           attainable HBM bandwidth (k_stream_copy)
//   mcrt_ctx_gather_chase          dependent gathers over 64-B records (k_chase)
//   mcrt_ctx_gather_chase_compact  the same over the compact records' packed 32 / 48-B layout (k_chase_compact)
//
// Built with mcrt_kernels.o's flags, where the kernels came from.
#include <algorithm>

#include "mcrt_device.h"
#include "mcrt_host.h"

// Attainable-bandwidth probe (mcrt_ctx_stream_copy): a persistent grid (8 workgroups per CU)
// strides over the array; each lane keeps 4 independent 16-B nontemporal loads in flight.
__global__ __launch_bounds__(256) void k_stream_copy(const f4* __restrict__ src, f4* __restrict__ dst, size_t n) {
    const size_t step = (size_t)gridDim.x * 1024;
    for (size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x; base < n; base += step) {
        f4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (base + 256 * k < n) v[k] = __builtin_nontemporal_load(src + base + 256 * k);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (base + 256 * k < n) __builtin_nontemporal_store(v[k], dst + base + 256 * k);
    }
}

// Dependent-gather ceiling probe (mcrt_ctx_gather_chase): every lane follows a chain of 64-B
// records whose links are read from the record just fetched, fetched as four 16-B pieces -- the
// traversal's access pattern with none of its arithmetic.  The array size decides where the
// records come from (L2, Infinity Cache, HBM), so the traversal's node-visit rate can be set
// against the ceiling of its own access pattern (tools/probe/chase_probe.hip has more variants).
__global__ void k_chase_init(int4* rec, uint32_t n, uint32_t seed) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t h = (uint32_t)i * 2654435761u ^ seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    const uint32_t nxt = h % n;
    for (int q = 0; q < 4; ++q) rec[4 * i + q] = make_int4((int)nxt, (int)(nxt ^ 1u), (int)(nxt ^ 2u), (int)nxt);
}
__global__ __launch_bounds__(64) void k_chase(const int4* __restrict__ rec, uint32_t n, int steps, uint32_t* sink) {
    const uint32_t chain = blockIdx.x * 64 + threadIdx.x;
    uint32_t h = chain * 0x9E3779B9u + 12345u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13;
    uint32_t idx = h % n, acc = 0;
    for (int s = 0; s < steps; ++s) {
        const int4 a = rec[4 * (size_t)idx], b = rec[4 * (size_t)idx + 1];
        const int4 c = rec[4 * (size_t)idx + 2], d = rec[4 * (size_t)idx + 3];
        asm volatile("" ::"v"(a.y), "v"(b.y), "v"(c.y));
        acc += (uint32_t)(a.z ^ b.z ^ c.z);
        idx = (uint32_t)d.w;
    }
    if (acc == 0xdeadbeefu) sink[0] = idx;   // never true: keeps the loads live
}

// The chase over the compact records' layout: record i is 2 (internal, 32 B) or 3 (leaf, 48 B)
// 16-B units, packed back to back at off[i] (exclusive scan of chase_units); its link is the next
// record's reference (unit offset << 1 | leaf bit), so a leaf's third unit is fetched in the same
// round trip as in mcrt_traverse.h qwalk.
MCRT_DEV uint32_t chaseHash(uint32_t i, uint32_t seed) {
    uint32_t h = i * 2654435761u ^ seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    return h;
}
__global__ void k_chase_units(uint32_t* units, uint32_t n, uint32_t leaf16) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) units[i] = 2u + ((chaseHash((uint32_t)i, 99u) & 0xffffu) < leaf16 ? 1u : 0u);
}
__global__ void k_chase_init_compact(int4* rec, const uint32_t* off, const uint32_t* units, uint32_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t nxt = chaseHash((uint32_t)i, 777u) % n;
    const int ref = (int)((off[nxt] << 1) | (units[nxt] == 3u ? 1u : 0u));
    for (uint32_t q = 0; q < units[i]; ++q) rec[off[i] + q] = make_int4((int)nxt, (int)(nxt ^ 1u), (int)(nxt ^ 2u), ref);
}
__global__ __launch_bounds__(64) void k_chase_compact(const int4* __restrict__ rec, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ units, uint32_t n, int steps,
                                                      uint32_t* sink) {
    const uint32_t chain = blockIdx.x * 64 + threadIdx.x;
    uint32_t h = chain * 0x9E3779B9u + 12345u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13;
    const uint32_t i0 = h % n;
    uint32_t ref = (off[i0] << 1) | (units[i0] == 3u ? 1u : 0u), acc = 0;
    for (int s = 0; s < steps; ++s) {
        const int4* p = rec + (ref >> 1);
        const int4 a = p[0], b = p[1];
        int4 c;
        asm("" : "=v"(c.x), "=v"(c.y), "=v"(c.z), "=v"(c.w));
        if (ref & 1u) c = p[2];
        asm volatile("" ::"v"(a.y), "v"(b.y), "v"(c.y));
        acc += (uint32_t)(a.z ^ b.z ^ c.z);
        ref = (uint32_t)a.w;
    }
    if (acc == 0xdeadbeefu) sink[0] = ref;   // never true: keeps the loads live
}

// ---------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------
using mcrt::fail;

// The shortest of launches 1 .. iters in ms, by events on st; enqueue(i) puts launch i on the stream
// and launch 0 is not counted: it warms caches and translations.
template <class Enqueue>
static float best_ms(hipStream_t st, int iters, Enqueue enqueue) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    float best = 1e30f;
    for (int i = 0; i < iters + 1; ++i) {
        hipEventRecord(e0, st);
        enqueue(i);
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, e0, e1);
        if (i > 0 && ms < best) best = ms;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return best;
}
// a chase's warm-up launch is a quarter as long
static int chase_steps(int i, int steps) { return i == 0 ? std::max(1, steps / 4) : steps; }

extern "C" {

MCRT_API mcrt_status mcrt_ctx_stream_copy(mcrt_ctx ctx, uint64_t bytes, int iters, double* gbps) {
    if (!ctx || !gbps || bytes < 4096 || iters < 1) return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad stream-copy args");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t n4 = (size_t)(bytes / 2 / 16);   // half the bytes read, half written
    DevBuf<f4> a, b;
    HIPCHK(ctx, a.alloc(n4));
    if (b.alloc(n4) != 0) return fail(ctx, MCRT_ERROR_OUT_OF_MEMORY, "stream copy");
    hipMemsetAsync(a.get(), 0, n4 * 16, st);
    const size_t blocks = std::min((n4 + 1023) / 1024, (size_t)std::max(ctx->numCUs, 1) * 8);
    const float best = best_ms(st, iters, [&](int) {
        hipLaunchKernelGGL(k_stream_copy, dim3((unsigned)blocks), dim3(256), 0, st, a.get(), b.get(), n4);
    });
    HIPCHK(ctx, hipGetLastError());
    *gbps = (double)(2 * n4 * 16) / (best * 1e-3) / 1e9;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_gather_chase(mcrt_ctx ctx, uint64_t records, int steps, int iters, double* gsteps) {
    if (!ctx || !gsteps || records < 64 || records > 0xffffffffull || steps < 1 || iters < 1)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad gather-chase args");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)records;
    DevBuf<int4> rec;   // 64 B a record
    DevBuf<uint32_t> sink;
    HIPCHK(ctx, rec.alloc(4 * (size_t)n));
    if (sink.alloc(1) != 0) return fail(ctx, MCRT_ERROR_OUT_OF_MEMORY, "gather chase");
    hipLaunchKernelGGL(k_chase_init, dim3((n + 255) / 256), dim3(256), 0, st, rec.get(), n, 777u);
    const int waves = ctx->numCUs * 32;
    const float best = best_ms(st, iters, [&](int i) {
        hipLaunchKernelGGL(k_chase, dim3(waves), dim3(64), 0, st, rec.get(), n, chase_steps(i, steps), sink.get());
    });
    HIPCHK(ctx, hipGetLastError());
    *gsteps = (double)waves * 64.0 * steps / (best * 1e-3) / 1e9;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_ctx_gather_chase_compact(mcrt_ctx ctx, uint64_t records, double leaf_frac, int steps,
                                                   int iters, double* gsteps) {
    // a link is (unit offset << 1 | leaf) in 32 bits: the expected units, and below the scanned ones,
    // stay under 2^31
    if (!ctx || !gsteps || records < 64 || records > 0x3fffffffull || steps < 1 || iters < 1 || !(leaf_frac >= 0.0) ||
        leaf_frac > 1.0 || (double)records * (2.0 + leaf_frac) >= 2147483648.0)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad gather-chase args");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)records;
    const uint32_t leaf16 = (uint32_t)std::min(65536.0, std::max(0.0, leaf_frac * 65536.0));
    DevBuf<uint32_t> units, off, sink;
    DevBuf<int4> rec;
    HIPCHK(ctx, units.alloc(n));
    HIPCHK(ctx, off.alloc(n));
    HIPCHK(ctx, sink.alloc(1));
    hipLaunchKernelGGL(k_chase_units, dim3((n + 255) / 256), dim3(256), 0, st, units.get(), n, leaf16);
    size_t total = 0;
    const hipError_t scanned = mcrt::qnode_offsets(units.get(), off.get(), n, &total, st);
    if (scanned == hipErrorNotSupported) return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad gather-chase args");
    HIPCHK(ctx, scanned);
    HIPCHK(ctx, rec.alloc(total));
    hipLaunchKernelGGL(k_chase_init_compact, dim3((n + 255) / 256), dim3(256), 0, st, rec.get(), off.get(), units.get(), n);
    const int waves = ctx->numCUs * 32;
    const float best = best_ms(st, iters, [&](int i) {
        hipLaunchKernelGGL(k_chase_compact, dim3(waves), dim3(64), 0, st, rec.get(), off.get(), units.get(), n,
                           chase_steps(i, steps), sink.get());
    });
    HIPCHK(ctx, hipGetLastError());
    *gsteps = (double)waves * 64.0 * steps / (best * 1e-3) / 1e9;
    return MCRT_OK;
}

}  // extern "C"
