// mcrt_adaptive.hip -- adaptive sampling: the per-tile error of the accumulated image, the list of
// tiles still above the target, and the entry points that switch the mode, install a list and read
// the state back.  The path tracer renders over the list (mcrt_pt_host.cpp) and k_accumulate /
// k_moments take their tiles from it; what they need of this module they get through the adaptive_*
// functions of mcrt_host.h.  The state is fb->ad (AdaptiveState), named only here.
//
// Built like mcrt_denoise.hip, with -ffp-contract=off and IEEE division and square root, so every
// line of k_tile_error is one float32 operation in the written order and tests/adaptive_ref.py
// restates it in numpy.
#include <cmath>
#include <cstring>
#include <vector>

#include "mcrt_host.h"

namespace {

// The error of one 8x8 tile from the luminance moments (sum l, sum l*l) of its pixels, one wave per
// tile, lane l = pixel (l & 7, l >> 3) of the tile (tilePixel's mapping without a band split).
// n = the tile's sample count as a float.  Per lane inside the image
//   mean = m1 / n;  v = max(0, m2 / n - mean * mean) / (n - 1)          (k_atrous_prep's expression)
// and 0 for both outside it.  The order of the two sums is fixed: Sv = sum v and Sm = sum mean are
// each reduced by the butterfly  s = s + shfl_xor(s, d)  for d = 32, 16, 8, 4, 2, 1, in this order
// (float addition commutes, so every lane ends with the same bits).  With c the tile's pixels inside
// the image
//   err = sqrt(Sv / c) / (Sm / c + luminance_floor)
// written only when n >= 2; +inf otherwise.  The moments are finite (k_moments clamps as
// k_accumulate does) and the denominator is >= luminance_floor > 0, so err is never NaN.
__global__ __launch_bounds__(256) void k_tile_error(int W, int H, int tilesX, int numTiles,
                                                    const float2* __restrict__ moments,
                                                    const uint32_t* __restrict__ tileCount, float floorLum,
                                                    float* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int tile = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (tile >= numTiles) return;   // the whole wave
    const int ty = tile / tilesX, tx = tile - ty * tilesX;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const uint32_t cnt = tileCount[tile];
    if (cnt < 2u) {
        if (lane == 0) err[tile] = INFINITY;
        return;
    }
    const float n = (float)cnt;
    float v = 0.0f, mean = 0.0f;
    if (x < W && y < H) {
        const float2 m = moments[(size_t)y * W + x];
        mean = m.x / n;
        v = fmaxf(0.0f, m.y / n - mean * mean) / (n - 1.0f);
    }
    float sv = v, sm = mean;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sv = sv + __shfl_xor(sv, d, 64);
        sm = sm + __shfl_xor(sm, d, 64);
    }
    const float c = (float)(min(8, W - tx * 8) * min(8, H - ty * 8));
    if (lane == 0) err[tile] = sqrtf(sv / c) / (sm / c + floorLum);
}

// the decision of mcrt_adaptive_update for a tile of n samples
__device__ __forceinline__ bool tileActive(float err, uint32_t n, const mcrt_adaptive_params& p) {
    if (n < (uint32_t)p.min_samples) return true;
    if (p.max_samples > 0 && n >= (uint32_t)p.max_samples) return false;
    return err > p.error_threshold;
}

// The active tiles in ascending order, their count, and numTiles in every entry after them up to
// `cap`.  One workgroup walks the tiles in chunks of its width (as k_tile_order walks them): a
// chunk's flags are compacted by a ballot per wave and the waves' totals, the running base carries
// to the next chunk, so the order is the tile order whatever the schedule.
__global__ __launch_bounds__(1024) void k_tile_list(int numTiles, int cap, const float* __restrict__ err,
                                                    const uint32_t* __restrict__ tileCount, mcrt_adaptive_params p,
                                                    uint32_t* __restrict__ list, int* __restrict__ len) {
    __shared__ int waveSum[16];
    __shared__ int base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int t0 = 0; t0 < numTiles; t0 += 1024) {   // uniform trip count
        const int t = t0 + (int)threadIdx.x;
        const bool a = t < numTiles && tileActive(err[t], tileCount[t], p);
        const unsigned long long m = __ballot(a);
        if (lane == 0) waveSum[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += waveSum[w];
        if (a) list[off + __popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)t;   // < numTiles <= cap
        __syncthreads();
        if (threadIdx.x == 0) {
            int s = 0;
            for (int w = 0; w < 16; ++w) s += waveSum[w];
            base += s;
        }
        __syncthreads();
    }
    const int n = base;
    for (int i = n + (int)threadIdx.x; i < cap; i += 1024) list[i] = (uint32_t)numTiles;
    if (threadIdx.x == 0) *len = n;
}

// `batch` more samples in each listed tile: one lane per tile of the list
__global__ __launch_bounds__(256) void k_tile_count_add(const uint32_t* __restrict__ list, int len, uint32_t batch,
                                                        uint32_t* __restrict__ tileCount) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) tileCount[list[i]] += batch;
}

using mcrt::fail, mcrt::fb_sync;

int tile_count(mcrt_framebuffer fb) { return (int)(((fb->W + 7) / 8) * ((fb->H + 7) / 8)); }
// entries of the list buffer: every tile, rounded up to k_shade0's 8 waves per workgroup, and one
// workgroup more, so the surplus waves of any launch over the list read an entry (numTiles)
size_t list_cap(int numTiles) { return ((size_t)numTiles + 7) / 8 * 8 + 8; }

const char* const kModeOff = "adaptive mode is off (mcrt_framebuffer_set_adaptive)";
const char* const kPending = "a rendered frame has not been accumulated yet";

// the host list `ids` (n ascending tiles) into the device list, padded; every stream has finished
hipError_t install_list(mcrt_framebuffer fb, const uint32_t* ids, int n) {
    AdaptiveState& a = fb->ad;
    std::vector<uint32_t> h(a.list.size(), (uint32_t)a.numTiles);
    if (n > 0) std::memcpy(h.data(), ids, sizeof(uint32_t) * (size_t)n);
    const hipError_t e = hipMemcpy(a.list.get(), h.data(), sizeof(uint32_t) * h.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) a.listLen = n;
    return e;
}

mcrt_status reset(mcrt_framebuffer fb) {
    mcrt_ctx ctx = fb->ctx;
    AdaptiveState& a = fb->ad;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));   // a render in flight reads the list
    std::vector<uint32_t> all((size_t)a.numTiles);
    for (int t = 0; t < a.numTiles; ++t) all[(size_t)t] = (uint32_t)t;
    HIPCHK(ctx, install_list(fb, all.data(), a.numTiles));
    HIPCHK(ctx, hipMemsetAsync(a.tileCount.get(), 0, sizeof(uint32_t) * (size_t)a.numTiles, ctx->stream));
    HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)a.tileErr.get(), 0x7f800000, (size_t)a.numTiles, ctx->stream));   // +inf
    a.frames = 0;
    a.pending = 0;
    return MCRT_OK;
}

}  // namespace

const uint32_t* mcrt::adaptive_list(mcrt_framebuffer fb, int* len) {
    *len = fb->ad.listLen;
    return fb->ad.list.get();
}

const uint32_t* mcrt::adaptive_counts(mcrt_framebuffer fb) { return fb->ad.tileCount.get(); }

void mcrt::adaptive_rendered(mcrt_framebuffer fb, int batch) { fb->ad.pending = batch; }

mcrt_status mcrt::adaptive_check_accumulate(mcrt_framebuffer fb, int32_t frame_index) {
    const AdaptiveState& a = fb->ad;
    if (a.pending == 0) return fail(fb->ctx, MCRT_ERROR_NOT_READY, "adaptive mode: no rendered frame to accumulate");
    if (frame_index != a.frames)
        return fail(fb->ctx, MCRT_ERROR_INVALID_ARG,
                    "adaptive mode: frame_index must be the frames accumulated since the reset (" +
                        std::to_string(a.frames) + ")");
    if (frame_index == 0 && a.listLen != a.numTiles)
        return fail(fb->ctx, MCRT_ERROR_INVALID_ARG,
                    "adaptive mode: frame_index 0 needs every tile listed (mcrt_adaptive_reset)");
    return MCRT_OK;
}

void mcrt::adaptive_accumulated(mcrt_framebuffer fb, int batch, hipStream_t st) {
    AdaptiveState& a = fb->ad;
    if (a.listLen > 0)
        hipLaunchKernelGGL(k_tile_count_add, dim3((a.listLen + 255) / 256), dim3(256), 0, st, a.list.get(), a.listLen,
                           (uint32_t)batch, a.tileCount.get());
    a.frames += batch;
    a.pending = 0;
}

hipError_t mcrt::adaptive_set_counts(mcrt_framebuffer fb, int frames) {
    AdaptiveState& a = fb->ad;
    if (!a.on) return hipSuccess;
    const hipError_t e =
        hipMemsetD32Async((hipDeviceptr_t)a.tileCount.get(), frames, (size_t)a.numTiles, fb->ctx->stream);
    if (e == hipSuccess) a.frames = frames;
    return e;
}

extern "C" {

MCRT_API mcrt_status mcrt_framebuffer_set_adaptive(mcrt_framebuffer fb, const mcrt_adaptive_params* p) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    AdaptiveState& a = fb->ad;
    if (p) {
        if (!(p->error_threshold >= 0.0f)) return fail(ctx, MCRT_ERROR_INVALID_ARG, "error_threshold must be >= 0");
        if (p->min_samples < 2) return fail(ctx, MCRT_ERROR_INVALID_ARG, "min_samples must be >= 2");
        if (p->max_samples != 0 && p->max_samples < p->min_samples)
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "max_samples must be 0 (no cap) or >= min_samples");
        if (!(p->luminance_floor > 0.0f) || std::isinf(p->luminance_floor))
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "luminance_floor must be positive and finite");
    }
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    if (!p) {   // off: the state goes, the moments stay as they are
        a = AdaptiveState();
        return MCRT_OK;
    }
    if (!a.on) {
        AdaptiveState n;
        n.numTiles = tile_count(fb);
        HIPCHK(ctx, n.tileCount.alloc((size_t)n.numTiles));
        HIPCHK(ctx, n.tileErr.alloc((size_t)n.numTiles));
        HIPCHK(ctx, n.list.alloc(list_cap(n.numTiles)));
        HIPCHK(ctx, n.listLenDev.alloc(1));
        const mcrt_status st = mcrt_framebuffer_set_moments_enabled(fb, 1);
        if (st != MCRT_OK) return st;
        a = std::move(n);
        a.on = true;
    }
    a.p = *p;
    return reset(fb);
}

MCRT_API mcrt_status mcrt_adaptive_reset(mcrt_framebuffer fb) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    if (!fb->ad.on) return fail(fb->ctx, MCRT_ERROR_INVALID_ARG, kModeOff);
    return reset(fb);
}

MCRT_API mcrt_status mcrt_adaptive_update(mcrt_framebuffer fb, int32_t* active_tiles) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    AdaptiveState& a = fb->ad;
    if (!a.on) return fail(ctx, MCRT_ERROR_INVALID_ARG, kModeOff);
    if (a.pending != 0) return fail(ctx, MCRT_ERROR_NOT_READY, kPending);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));   // no render reads the list while it is rebuilt
    hipStream_t st = ctx->stream;
    {
        Timed t(ctx, K_TILE_ERROR, nullptr, (int64_t)a.numTiles * 64);
        hipLaunchKernelGGL(k_tile_error, dim3((a.numTiles + 3) / 4), dim3(256), 0, st, (int)fb->W, (int)fb->H,
                           (int)((fb->W + 7) / 8), a.numTiles, fb->dn.moments.get(), a.tileCount.get(), a.p.luminance_floor,
                           a.tileErr.get());
    }
    {
        Timed t(ctx, K_TILE_LIST, nullptr, (int64_t)a.numTiles);
        hipLaunchKernelGGL(k_tile_list, dim3(1), dim3(1024), 0, st, a.numTiles, (int)a.list.size(), a.tileErr.get(),
                           a.tileCount.get(), a.p, a.list.get(), a.listLenDev.get());
    }
    HIPCHK(ctx, hipGetLastError());
    int len = 0;
    HIPCHK(ctx, hipMemcpyAsync(&len, a.listLenDev.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    a.listLen = len;
    if (active_tiles) *active_tiles = len;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_set_active_tiles(mcrt_framebuffer fb, const uint32_t* tiles, int32_t n) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    AdaptiveState& a = fb->ad;
    if (!a.on) return fail(ctx, MCRT_ERROR_INVALID_ARG, kModeOff);
    if (n < 0 || n > a.numTiles || (n > 0 && !tiles)) return fail(ctx, MCRT_ERROR_INVALID_ARG, "bad tile list");
    for (int i = 0; i < n; ++i) {
        if (tiles[i] >= (uint32_t)a.numTiles)
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "tile " + std::to_string(tiles[i]) + " is past the image's tiles");
        if (i > 0 && tiles[i] <= tiles[i - 1]) return fail(ctx, MCRT_ERROR_INVALID_ARG, "the tile list must be strictly ascending");
    }
    if (a.pending != 0) return fail(ctx, MCRT_ERROR_NOT_READY, kPending);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    HIPCHK(ctx, install_list(fb, tiles, n));
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_read_adaptive(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                    uint64_t* needed) {
    if (!fb || which < 0 || which > 2) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    const AdaptiveState& a = fb->ad;
    if (!a.on) return fail(ctx, MCRT_ERROR_INVALID_ARG, kModeOff);
    const void* src = which == 0 ? (const void*)a.tileErr.get() : which == 1 ? (const void*)a.tileCount.get()
                                                                             : (const void*)a.list.get();
    const uint64_t need = 4 * (uint64_t)(which == 2 ? a.listLen : a.numTiles);
    if (needed) *needed = need;
    if (!host_dst) return MCRT_OK;
    if (bytes < need) return fail(ctx, MCRT_ERROR_INVALID_ARG, "destination too small");
    if (need == 0) return MCRT_OK;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    HIPCHK(ctx, hipMemcpy(host_dst, src, need, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

}  // extern "C"
