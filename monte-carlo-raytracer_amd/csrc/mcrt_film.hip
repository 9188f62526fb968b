// mcrt_film.hip -- the film: the frame buffer's own planes (wsum, wts, image, denoised, display),
// every kernel that writes `image` from wsum / wts, and below the kernels the entry points that create,
// zero-fill, read back, copy, install, pack for the band gather and post-process them.
//
//   k_accumulate         ReconstructionPass (clamp, weighted running mean); launched by mcrt_pt_host.cpp's
//                        accumulate() through launch_accumulate
//   k_resolve            image = wsum / wts after the accumulators were installed (a multi-GPU reduce)
//   k_band_pack/_unpack  a rank's rows of the accumulators for the end-of-job gather, and back
//   k_denoise, k_tonemap the reference's RTDenoisePass and RTToneMappingPass (mcrt_postprocess;
//                        mcrt_denoise.hip tone-maps through launch_tonemap)
//
// The planes are no state struct of this file's: the PT and BDPT hosts and the guided denoiser read
// them as the frame buffer's fields.  Built with mcrt_kernels.o's flags, where the kernels came from:
// the filter weights and every cl_div are pinned bit for bit against the reference under them.
#include <algorithm>
#include <string>

#include "mcrt_bands.h"
#include "mcrt_host.h"
#include "mcrt_shading.h"

// ---------------------------------------------------------------------------
// ReconstructionPass (KRN/reconstruction.cl:6-60) with the filters of KRN/filters.cl:12-69,
// evaluated on the device as the reference does (same expression shapes, so clang contracts the
// same products into fma; `/` is the OpenCL-default 2.5-ulp division, cl_div; exp and sin are the
// device library's, like OpenCL's).  The weight is uniform per frame (one pixelOffset per frame,
// RTReconstructionPass.cpp:71-123); pinned against the reference's filters.cl run live
// (oracle/refbuild/clprobe_filters.cl, tests/test_gpu_accumulate.py).  Band rows only.
// ---------------------------------------------------------------------------
MCRT_DEV float filterTriangle(f2 p, f2 radius) {   // filters.cl:17-20
    return fmaxf(0.0f, radius.x - fabsf(p.x)) * fmaxf(0.0f, radius.y - fabsf(p.y));
}
MCRT_DEV float filterGaussian1D(float d, float alpha, float expv) {   // filters.cl:22-25
    return fmaxf(0.0f, expf(-alpha * d * d) - expv);
}
MCRT_DEV float filterMitchell1D(float x, float B, float C) {   // filters.cl:32-39
    x = fabsf(2.0f * x);
    if (x > 1.0f)
        return ((-B - 6*C) * x*x*x + (6*B + 30*C) * x*x + (-12*B - 48*C) * x + (8*B + 24*C)) * (1.f/6.f);
    else
        return ((12 - 9*B - 6*C) * x*x*x + (-18 + 12*B + 6*C) * x*x + (6 - 2*B)) * (1.f/6.f);
}
MCRT_DEV float filterSinc(float x) {   // filters.cl:47-54 (1e-5 is a float literal: no cl_khr_fp64 pragma)
    x = fabsf(x);
    if (x < 1e-5f) return 1.0f;
    return cl_div(sinf(PI_F * x), (PI_F * x));
}
MCRT_DEV float filterWindowedSinc(float x, float radius, float tau) {   // filters.cl:56-64
    x = fabsf(x);
    if (x > radius) return 0.0f;
    const float lanczos = filterSinc(cl_div(x, tau));
    return filterSinc(x) * lanczos;
}
// the switch of reconstruction.cl:23-42
MCRT_DEV float filterWeight(const mcrt_filter& fp) {
    const f2 p = f2{fp.pixelOffset.x, fp.pixelOffset.y}, radius = f2{fp.radius.x, fp.radius.y};
    switch (fp.filterType) {
    case MCRT_TRIANGLE_FILTER: return filterTriangle(p, radius);
    case MCRT_GAUSSIAN_FILTER:
        return filterGaussian1D(p.x, fp.gaussianAlpha, fp.gaussianExpX) * filterGaussian1D(p.y, fp.gaussianAlpha, fp.gaussianExpY);
    case MCRT_MITCHELL_FILTER:
        return filterMitchell1D(cl_div(p.x, radius.x), fp.mitchellB, fp.mitchellC) *
               filterMitchell1D(cl_div(p.y, radius.y), fp.mitchellB, fp.mitchellC);
    case MCRT_LANCZOS_SINC_FILTER:
        return filterWindowedSinc(p.x, radius.x, fp.lanczosSincTau) * filterWindowedSinc(p.y, radius.y, fp.lanczosSincTau);
    default: return 1.0f;   // RT_BOX_FILTER
    }
}

// A batch of f.batch frames (mcrt_render_frames) is accumulated in frame order, frame + k with
// filter filters[k * fstride]: per pixel the same operations as f.batch single-frame launches.
// LIST (adaptive sampling): wave j takes tile list[j] (padded with numTiles past the list's end) and
// the tile's sample count stands for `frame`, so "first sample" is the count being 0; the pixels of
// other tiles are not touched.
template <bool LIST>
__global__ __launch_bounds__(256) void k_accumulate(FrameArgs f, int frame, const mcrt_filter* __restrict__ filters, int fstride,
                                                    const float4* __restrict__ radiance, float4* __restrict__ wsum,
                                                    float* __restrict__ wts, float4* __restrict__ image,
                                                    const uint32_t* __restrict__ list, const uint32_t* __restrict__ tileCount) {
    const int lane = threadIdx.x & 63;
    int tile = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (LIST) tile = (int)list[tile];
    int x, y;
    if (tile >= f.numTiles || !tilePixel(f, tile, lane, x, y)) return;
    if (LIST) frame = (int)tileCount[tile];
    const int pix = y * (int)f.W + x;
    f4 s;
    float ws;
    if (frame != 0) {
        const float4 o = wsum[pix];
        s = f4{o.x, o.y, o.z, o.w};
        ws = wts[pix];
    }
    for (int k = 0; k < f.batch; ++k) {
        const float4 r4 = radiance[(size_t)k * f.W * f.H + pix];
        const f4 radiance4 = f4{cl_clamp(r4.x, 0.0f, 1000.0f), cl_clamp(r4.y, 0.0f, 1000.0f),
                                cl_clamp(r4.z, 0.0f, 1000.0f), cl_clamp(r4.w, 0.0f, 1000.0f)};
        const float w = filterWeight(filters[k * fstride]);
        if (frame + k == 0) {
            s = radiance4 * w;
            ws = w;
        } else {
            s += radiance4 * w;   // contracted to fma, as reconstruction.cl:50
            ws = ws + w;
        }
    }
    wsum[pix] = make_float4(s.x, s.y, s.z, s.w);
    wts[pix] = ws;
    const f4 fin = cl_div(s, ws);
    image[pix] = make_float4(fin.x, fin.y, fin.z, fin.w);
}

// image = sum / weight after a multi-GPU reduce of the accumulators
__global__ __launch_bounds__(256) void k_resolve(int n, const float4* __restrict__ wsum, const float* __restrict__ wts,
                                                 float4* __restrict__ image) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 s = wsum[i];
    const float w = wts[i];
    image[i] = make_float4(cl_div(s.x, w), cl_div(s.y, w), cl_div(s.z, w), cl_div(s.w, w));
}

// Tile split, end of job: a rank's own rows of the accumulators in its band order (local 8-row
// block tb at rows 8 tb .. 8 tb + 7, tilePixel's numbering; mcrt.dist.band_rows_of), one packed row
// = W x (sum w*L as 4 floats) then W x sum w, straight from the frame buffer: no full-frame copy
// before the gather.  bpb = band_rows / 8.
__device__ __forceinline__ void bandOwner(int y, int bpb, int numBands, int& r, int& row) {
    const int gb = y >> 3;
    r = (gb / bpb) % numBands;
    row = ((gb / (bpb * numBands)) * bpb + gb % bpb) * 8 + (y & 7);
}

__global__ __launch_bounds__(256) void k_band_pack(int W, int H, int bpb, int numBands, int band,
                                                   const float4* __restrict__ wsum, const float* __restrict__ wts,
                                                   float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const int y = i / W, x = i - y * W;
    int r, row;
    bandOwner(y, bpb, numBands, r, row);
    if (r != band) return;
    float* o = out + (size_t)row * 5 * W;
    const float4 v = wsum[i];
    o[4 * x] = v.x;
    o[4 * x + 1] = v.y;
    o[4 * x + 2] = v.z;
    o[4 * x + 3] = v.w;
    o[4 * W + x] = wts[i];
}

// Rank dst after the gather: every other rank's rows (recv = numBands x maxRows packed rows) into
// the accumulators in place, then the image (k_resolve's division) in the same pass.
__global__ __launch_bounds__(256) void k_band_unpack(int W, int H, int bpb, int numBands, int band, int maxRows,
                                                     const float* __restrict__ recv, float4* __restrict__ wsum,
                                                     float* __restrict__ wts, float4* __restrict__ image) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const int y = i / W, x = i - y * W;
    int r, row;
    bandOwner(y, bpb, numBands, r, row);
    float4 s;
    float w;
    if (r == band) {
        s = wsum[i];
        w = wts[i];
    } else {
        const float* p = recv + ((size_t)r * maxRows + row) * 5 * W;
        s = make_float4(p[4 * x], p[4 * x + 1], p[4 * x + 2], p[4 * x + 3]);
        w = p[4 * W + x];
        wsum[i] = s;
        wts[i] = w;
    }
    image[i] = make_float4(cl_div(s.x, w), cl_div(s.y, w), cl_div(s.z, w), cl_div(s.w, w));
}

// ---------------------------------------------------------------------------
// Post-process (the reference's RTDenoisePass + RTToneMappingPass after reconstruction)
// ---------------------------------------------------------------------------
#define DENOISE_TILE 16
#define DENOISE_RMAX 16
// BilateralDenoise (KRN/Denoise.cl:6-47): a 16x16 tile plus its clamped apron staged in LDS
// once (the reference re-reads the (2r+1)^2 window through the image unit per pixel); the
// window is walked in the reference's order (x outer, y inner) so the sums round identically.
__global__ __launch_bounds__(DENOISE_TILE * DENOISE_TILE) void k_denoise(int W, int H, int r, float ss, float sr,
                                                                         const float4* __restrict__ in,
                                                                         float4* __restrict__ out) {
    __shared__ float4 tile[(DENOISE_TILE + 2 * DENOISE_RMAX) * (DENOISE_TILE + 2 * DENOISE_RMAX)];
    const int TW = DENOISE_TILE + 2 * r;
    const int x0 = blockIdx.x * DENOISE_TILE - r, y0 = blockIdx.y * DENOISE_TILE - r;
    const int tid = threadIdx.y * DENOISE_TILE + threadIdx.x;
    for (int i = tid; i < TW * TW; i += DENOISE_TILE * DENOISE_TILE) {
        const int gx = min(max(x0 + i % TW, 0), W - 1), gy = min(max(y0 + i / TW, 0), H - 1);
        tile[i] = in[(size_t)gy * W + gx];
    }
    __syncthreads();
    const int gx = blockIdx.x * DENOISE_TILE + threadIdx.x, gy = blockIdx.y * DENOISE_TILE + threadIdx.y;
    if (gx >= W || gy >= H) return;
    const float sdSq = ss * ss, srSq = sr * sr;
    const float4 oc = tile[(gy - y0) * TW + (gx - x0)];
    const f4 o = f4{oc.x, oc.y, oc.z, oc.w};
    f4 fc = f4{0.0f, 0.0f, 0.0f, 0.0f};
    float weightSum = 0.0f;
    for (int rx = -r; rx <= r; ++rx) {
        const int x = min(max(rx + gx, 0), W - 1);
        for (int ry = -r; ry <= r; ++ry) {
            const int y = min(max(ry + gy, 0), H - 1);
            const float4 kc = tile[(y - y0) * TW + (x - x0)];
            const f4 k = f4{kc.x, kc.y, kc.z, kc.w};
            const f4 cd = o - k;
            const float d2 = fmaf(cd.w, cd.w, fmaf(cd.z, cd.z, fmaf(cd.y, cd.y, cd.x * cd.x)));   // dot(float4)
            const int sp = (gx - x) * (gx - x) + (gy - y) * (gy - y);
            const float w = expf(cl_div((float)(-sp), (2.0f * sdSq)) - cl_div(d2, (2.0f * srSq)));
            weightSum += w;
            fc += w * k;
        }
    }
    fc = cl_div(fc, weightSum);
    out[(size_t)gy * W + gx] = make_float4(fc.x, fc.y, fc.z, fc.w);
}

// ReinhardToneMapping (KRN/ToneMapping.cl:42-63), luminance of KRN/colors.cl:19-22
__global__ __launch_bounds__(256) void k_tonemap(int n, float Lwhite, const float4* __restrict__ in,
                                                 float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    const float L = 0.212671f * p.x + 0.715160f * p.y + 0.072169f * p.z;
    const float tL = cl_div(L * (1.0f + cl_div(L, (Lwhite * Lwhite))), (1.0f + L));
    const float s = cl_div(tL, L);
    out[i] = make_float4(p.x * s, p.y * s, p.z * s, p.w);
}

// ---------------------------------------------------------------------------
// the two launchers other files call
// ---------------------------------------------------------------------------
void mcrt::launch_accumulate(const FrameArgs& f, int frame, const mcrt_filter* filters, int filterStride, const float4* radiance,
                             float4* wsum, float* wts, float4* image, hipStream_t st, const uint32_t* list, int listLen,
                             const uint32_t* tileCount) {
    if (list) {   // listLen > 0: whole workgroups of 4 waves, the surplus ones find numTiles in the table
        hipLaunchKernelGGL(k_accumulate<true>, dim3((listLen * 64 + 255) / 256), dim3(256), 0, st, f, frame, filters,
                           filterStride, radiance, wsum, wts, image, list, tileCount);
        return;
    }
    const int blocks = (f.numTiles * 64 + 255) / 256;
    hipLaunchKernelGGL(k_accumulate<false>, dim3(blocks), dim3(256), 0, st, f, frame, filters, filterStride, radiance, wsum,
                       wts, image, list, tileCount);
}

void mcrt::launch_tonemap(int n, float Lwhite, const float4* in, float4* out, hipStream_t st) {
    hipLaunchKernelGGL(k_tonemap, dim3((n + 255) / 256), dim3(256), 0, st, n, Lwhite, in, out);
}

// ---------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------
using mcrt::fail, mcrt::fb_sync, mcrt::ctx_wait_slots, mcrt::check_device_flags;

// one-dimensional launches over the frame buffer's pixels
static dim3 pixel_grid(mcrt_framebuffer fb) { return dim3((unsigned)((fb->N + 255) / 256)); }

// Plane `which` of mcrt_framebuffer_read and mcrt_framebuffer_copy_device: 0 the current slot's
// radiance (frame 0 of a batch), 1 wsum, 2 image.  Plane 3 is not the same for the two, on purpose:
// a host read shows `display`, what mcrt_postprocess made; a device copy hands out `wts`, the other
// half of the accumulators and 4 bytes a pixel, for the multi-GPU reduce.  The caller names its own.
static const void* film_plane(mcrt_framebuffer fb, int which, const void* plane3) {
    switch (which) {
    case 0: return cur_slot(fb).radiance.get();
    case 1: return fb->wsum.get();
    case 2: return fb->image.get();
    default: return plane3;
    }
}

static int band_max_rows(const FrameArgs& f) { return mcrt::band_max_rows(f.H, f.bandRows, f.numBands); }

extern "C" {

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
    if (e == hipSuccess) e = mcrt::slot_alloc(fb->slot[0], N, N);   // one frame: hits by pixel
    // zero-fills on slot 0's (private) stream, finished before the frame buffer is handed out:
    // only this buffer's work is waited for, not the device (other contexts, a captured caller stream)
    for (auto* img : {&fb->wsum, &fb->image, &fb->denoised, &fb->display})
        if (e == hipSuccess) e = hipMemsetAsync(img->get(), 0, 16 * N, fb->slot[0].stream);
    if (e == hipSuccess) e = hipMemsetAsync(fb->wts.get(), 0, 4 * N, fb->slot[0].stream);
    if (e == hipSuccess) e = mcrt::fill_hints(fb->hintPix.get(), N, 1u << 22, fb->slot[0].stream);   // no hints
    if (e == hipSuccess) e = hipStreamSynchronize(fb->slot[0].stream);
    if (e != hipSuccess) {
        mcrt::fb_free(fb);
        delete fb;
        return fail(ctx, e == hipErrorOutOfMemory ? MCRT_ERROR_OUT_OF_MEMORY : MCRT_ERROR_DEVICE,
                    std::string("frame buffer: ") + hipGetErrorString(e));
    }
    *out = fb;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_destroy(mcrt_framebuffer fb) {
    if (!fb) return MCRT_OK;
    hipSetDevice(fb->ctx->device);
    fb_sync(fb);
    mcrt::fb_free(fb);
    delete fb;
    return MCRT_OK;
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
            hipLaunchKernelGGL(k_denoise, dim3((W + DENOISE_TILE - 1) / DENOISE_TILE, (H + DENOISE_TILE - 1) / DENOISE_TILE),
                               dim3(DENOISE_TILE, DENOISE_TILE), 0, ctx->stream, W, H, p->denoise_radius, p->sigma_spatial,
                               p->sigma_range, fb->image.get(), fb->denoised.get());
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
    const void* src = film_plane(fb, which, fb->display.get());
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
    const void* src = film_plane(fb, which, fb->wts.get());
    if (which == 0) ctx_wait_slots(fb);
    HIPCHK(ctx, hipMemcpyAsync(d_dst, src, (which == 3 ? 4 : 16) * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    // the slot may take its next frame only after this copy has read its radiance
    if (which == 0) HIPCHK(ctx, mcrt::release_slot(fb, ctx->stream));
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_copy_device_frame(mcrt_framebuffer fb, int32_t k, void* d_dst) {
    if (!fb || !d_dst) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    FrameSlot& slot = cur_slot(fb);
    if (k < 0 || k >= std::max(slot.lastBatch, 1))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame index outside the last mcrt_render_frames batch");
    if (!slot.radiance) return fail(ctx, MCRT_ERROR_NOT_READY, "no frame rendered yet");
    hipSetDevice(ctx->device);
    ctx_wait_slots(fb);
    HIPCHK(ctx, hipMemcpyAsync(d_dst, slot.radiance.get() + (size_t)k * fb->N, 16 * fb->N, hipMemcpyDeviceToDevice,
                               ctx->stream));
    HIPCHK(ctx, mcrt::release_slot(fb, ctx->stream));   // as mcrt_framebuffer_copy_device 0
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_set_accumulation(mcrt_framebuffer fb, const void* d_wsum, const void* d_wts) {
    if (!fb || !d_wsum || !d_wts) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipMemcpyAsync(fb->wsum.get(), d_wsum, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(fb->wts.get(), d_wts, 4 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_resolve, pixel_grid(fb), dim3(256), 0, ctx->stream, (int)fb->N, fb->wsum.get(), fb->wts.get(),
                       fb->image.get());
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_bands_pack(mcrt_framebuffer fb, void* d_dst) {
    if (!fb || !d_dst) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    if (!fb->haveBands) return fail(fb->ctx, MCRT_ERROR_NOT_READY, "no frame rendered");
    mcrt_ctx ctx = fb->ctx;
    hipSetDevice(ctx->device);
    const FrameArgs& f = fb->bands;
    hipLaunchKernelGGL(k_band_pack, pixel_grid(fb), dim3(256), 0, ctx->stream, (int)f.W, (int)f.H, f.bandRows >> 3,
                       f.numBands, f.bandIndex, fb->wsum.get(), fb->wts.get(), static_cast<float*>(d_dst));
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
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
    hipLaunchKernelGGL(k_band_unpack, pixel_grid(fb), dim3(256), 0, ctx->stream, (int)f.W, (int)f.H, f.bandRows >> 3,
                       f.numBands, f.bandIndex, max_rows, static_cast<const float*>(d_recv), fb->wsum.get(), fb->wts.get(),
                       fb->image.get());
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

}  // extern "C"
