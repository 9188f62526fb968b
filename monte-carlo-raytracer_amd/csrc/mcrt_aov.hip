// mcrt_aov.hip -- the passes over borrowed camera hits: k_aov with its entry point mcrt_render_aov,
// and the denoiser's guide kernels, which mcrt_denoise.hip launches through launch_guides and
// launch_guides_motion (its own flags, -ffp-contract=off, would not give the guides MCRT_AOV_ALBEDO's
// Kd bit for bit).  Every pass reads the primary-hit buffer of the current frame slot
// (borrow_camera_hits, mcrt_host.h; hitSlot, mcrt_shading.h) in tile order, as k_shade0 does.  Built
// with mcrt_kernels.o's flags, where the kernels came from: the guides' Kd is k_aov's, and both are
// k_shade0's uberProps.
#include <string>

#include "mcrt_host.h"
#include "mcrt_shading.h"

using mcrt::fail, mcrt::frame_args, mcrt::scene_args, mcrt::accel_ready;

// ---------------------------------------------------------------------------
// Per-pixel outputs of the camera-ray hits (mcrt_render_aov), tile order as k_shade0.
//   MCRT_AOV_ALBEDO:     1 float4 = (uber Kd incl. texture, opacity.x); LOD per f.textureLod
//   MCRT_AOV_TEXTURE_LOD: 3 float4 = (duvdx, duvdy), (diffuse-texture LOD, shape, uv),
//                         the diffuse texture read mip-mapped (zeros where untextured)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_aov(SceneArgs s, FrameArgs f, const mcrt_camera* __restrict__ camp,
                                             const float4* __restrict__ hits, int which, float4* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int tile = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int x, y;
    if (tile >= f.numTiles || !tilePixel(f, tile, lane, x, y)) return;
    const int pix = y * (int)f.W + x;
    const int stride = which == MCRT_AOV_TEXTURE_LOD ? 3 : 1;
    float4* o = out + (size_t)pix * stride;
    for (int k = 0; k < stride; ++k) o[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 hit = hits[hitSlot(f, tile, lane, 0, x, y)];
    const int shapeIdx = __float_as_int(hit.z), primIdx = __float_as_int(hit.w);
    if (shapeIdx < 0) return;
    const mcrt_camera& cam = *camp;
    f3 dpdu, dpdv, dx, dy;
    const Frame si = computeSurfaceInteraction(s, shapeIdx, primIdx, f2{hit.x, hit.y}, &dpdu, &dpdv);
    cameraDiffDirs(cam, x, y, dx, dy);
    TexLod L = surfaceUVDifferentials(si, dpdu, dpdv, ld3(cam.pos), dx, dy);
    const int materialId = s.shapes[shapeIdx].materialId;
    if (which == MCRT_AOV_TEXTURE_LOD) {
        float lod = 0.0f;
        f4 c = f4{0.0f, 0.0f, 0.0f, 0.0f};
        if (materialId != -1 && s.materials[materialId].uber_diffuseTexId != -1) {
            const int t = s.materials[materialId].uber_diffuseTexId;
            const mcrt_texture_desc tex = s.textures[t];
            lod = mipLod(tex, L.duvdx, L.duvdy);
            c = readTexLodDesc(s, tex, si.uv, lod);
        }
        o[0] = make_float4(L.duvdx.x, L.duvdx.y, L.duvdy.x, L.duvdy.y);
        o[1] = make_float4(lod, __int_as_float(shapeIdx), si.uv.x, si.uv.y);
        o[2] = make_float4(c.x, c.y, c.z, c.w);
    } else {
        L.on = f.textureLod != 0;
        if (materialId != -1 && s.materials[materialId].type == 0) {
            const Uber u = uberProps(s, s.materials[materialId], si.uv, L);
            o[0] = make_float4(u.Kd.x, u.Kd.y, u.Kd.z, u.opacity.x);
        }
    }
}

// Denoiser guides of the camera-ray hits (mcrt_render_guides), tile order and albedo as k_aov:
//   normalPlane = (n, n . (P - cam.pos)), n = the interpolated shading normal before normal
//                 mapping, flipped to face the camera; the plane offset is camera-relative so a
//                 scene far from the origin keeps its precision
//   albedoDepth = (MCRT_AOV_ALBEDO's Kd, |P - cam.pos|)
// A miss writes (0, 0, 0, 0) and (0, 0, 0, -1).  Band rows only.
//
// MOTION (k_guides_motion, mcrt_render_guides_motion) writes the same two records and, from the
// shape's previous pose `prev` (mcrt_scene_motion_snapshot; NULL: none yet), two more:
//   motion     = (P_prev - P, flag).  flag 0: no table, or the table's 32 matrix words and mesh key
//                equal the shape's -- (0, 0, 0, 0) without evaluating anything.  flag 1: P_prev is
//                si.p's expression over the table's toWorldTransform (three transformPoint3 of the
//                same surface-record vertices, the same blend), d = P_prev - si.p per component.
//                flag -1: the mesh key differs, (0, 0, 0, -1).  A miss is (0, 0, 0, 0).
//   prevNormal = (n_prev, 0) where flag is 1, zeros otherwise: si.sn's expression over the table's
//                toWorldInverseTranspose, flipped when n was (the same physical side).
template <bool MOTION>
__device__ __forceinline__ void guidesPixel(const SceneArgs& s, const FrameArgs& f, const mcrt_camera* __restrict__ camp,
                                            const float4* __restrict__ hits, float4* __restrict__ normalPlane,
                                            float4* __restrict__ albedoDepth, const PrevPose* __restrict__ prev,
                                            float4* __restrict__ motion, float4* __restrict__ prevNormal) {
    const int lane = threadIdx.x & 63;
    const int tile = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int x, y;
    if (tile >= f.numTiles || !tilePixel(f, tile, lane, x, y)) return;
    const int pix = y * (int)f.W + x;
    const float4 hit = hits[hitSlot(f, tile, lane, 0, x, y)];
    const int shapeIdx = __float_as_int(hit.z), primIdx = __float_as_int(hit.w);
    if (shapeIdx < 0) {
        normalPlane[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        albedoDepth[pix] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (MOTION) {
            motion[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            prevNormal[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        return;
    }
    const mcrt_camera& cam = *camp;
    f3 dpdu, dpdv, dx, dy;
    const Frame si = computeSurfaceInteraction(s, shapeIdx, primIdx, f2{hit.x, hit.y}, &dpdu, &dpdv);
    cameraDiffDirs(cam, x, y, dx, dy);
    TexLod L = surfaceUVDifferentials(si, dpdu, dpdv, ld3(cam.pos), dx, dy);
    L.on = f.textureLod != 0;
    f3 kd = f3{0.0f, 0.0f, 0.0f};
    const int materialId = s.shapes[shapeIdx].materialId;
    if (materialId != -1 && s.materials[materialId].type == 0) kd = uberProps(s, s.materials[materialId], si.uv, L).Kd;
    const f3 v = si.p - ld3(cam.pos);
    f3 n = si.sn;
    float off = cl_dot(n, v);
    const bool flipped = off > 0.0f;
    if (flipped) {
        n = f3{-n.x, -n.y, -n.z};
        off = -off;
    }
    normalPlane[pix] = make_float4(n.x, n.y, n.z, off);
    albedoDepth[pix] = make_float4(kd.x, kd.y, kd.z, cl_length(v));
    if (MOTION) {
        float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pn = mv;
        if (prev) {
            const mcrt_shape shape = tableEntry(s.shapes, shapeIdx);
            const PrevPose pp = tableEntry(prev, shapeIdx);
            if (pp.startIdx != shape.startIdx || pp.startVertex != shape.startVertex ||
                pp.numTriangles != shape.numTriangles) {
                mv.w = -1.0f;
            } else {
                const uint32_t* a = reinterpret_cast<const uint32_t*>(&shape);
                const uint32_t* b = reinterpret_cast<const uint32_t*>(&pp);
                uint32_t diff = 0;
#pragma unroll
                for (int w = 0; w < 32; ++w) diff |= a[w] ^ b[w];
                if (diff) {
                    const float4* R = s.surf + 8 * ((size_t)tableEntry(s.surfBase, shapeIdx) + (uint32_t)primIdx);
                    const float4 r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3], r4 = R[4], r5 = R[5];
                    const f2 barycentrics = f2{hit.x, hit.y};
                    const f3 p0 = transformPoint3(pp.toWorldTransform, mk3(r0.x, r0.y, r0.z));
                    const f3 p1 = transformPoint3(pp.toWorldTransform, mk3(r0.w, r1.x, r1.y));
                    const f3 p2 = transformPoint3(pp.toWorldTransform, mk3(r1.z, r1.w, r2.x));
                    const f3 n0 = transformVector3(pp.toWorldInverseTranspose, mk3(r3.w, r4.x, r4.y));
                    const f3 n1 = transformVector3(pp.toWorldInverseTranspose, mk3(r4.z, r4.w, r5.x));
                    const f3 n2 = transformVector3(pp.toWorldInverseTranspose, mk3(r5.y, r5.z, r5.w));
                    const f3 pPrev = p0 * (1.0f - barycentrics.x - barycentrics.y) + p1 * barycentrics.x + p2 * barycentrics.y;
                    f3 nPrev = cl_normalize(n0 * (1.0f - barycentrics.x - barycentrics.y) + n1 * barycentrics.x + n2 * barycentrics.y);
                    if (flipped) nPrev = f3{-nPrev.x, -nPrev.y, -nPrev.z};
                    mv = make_float4(pPrev.x - si.p.x, pPrev.y - si.p.y, pPrev.z - si.p.z, 1.0f);
                    pn = make_float4(nPrev.x, nPrev.y, nPrev.z, 0.0f);
                }
            }
        }
        motion[pix] = mv;
        prevNormal[pix] = pn;
    }
}

__global__ __launch_bounds__(256) void k_guides(SceneArgs s, FrameArgs f, const mcrt_camera* __restrict__ camp,
                                                const float4* __restrict__ hits, float4* __restrict__ normalPlane,
                                                float4* __restrict__ albedoDepth) {
    guidesPixel<false>(s, f, camp, hits, normalPlane, albedoDepth, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void k_guides_motion(SceneArgs s, FrameArgs f, const mcrt_camera* __restrict__ camp,
                                                       const float4* __restrict__ hits,
                                                       float4* __restrict__ normalPlane,
                                                       float4* __restrict__ albedoDepth,
                                                       const PrevPose* __restrict__ prev, float4* __restrict__ motion,
                                                       float4* __restrict__ prevNormal) {
    guidesPixel<true>(s, f, camp, hits, normalPlane, albedoDepth, prev, motion, prevNormal);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace mcrt {

void launch_guides(const SceneArgs& s, const FrameArgs& f, const mcrt_camera* cam, const float4* hits,
                   float4* normalPlane, float4* albedoDepth, hipStream_t st) {
    const int blocks = (f.numTiles * 64 + 255) / 256;
    hipLaunchKernelGGL(k_guides, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, s, f, cam, hits, normalPlane,
                       albedoDepth);
}
void launch_guides_motion(const SceneArgs& s, const FrameArgs& f, const mcrt_camera* cam, const float4* hits,
                          float4* normalPlane, float4* albedoDepth, const PrevPose* prev, float4* motion,
                          float4* prevNormal, hipStream_t st) {
    const int blocks = (f.numTiles * 64 + 255) / 256;
    hipLaunchKernelGGL(k_guides_motion, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, s, f, cam, hits, normalPlane,
                       albedoDepth, prev, motion, prevNormal);
}

}  // namespace mcrt

static void launch_aov(const SceneArgs& s, const FrameArgs& f, const mcrt_camera* cam, const float4* hits, int which,
                       float4* out, hipStream_t st) {
    const int blocks = (f.numTiles * 64 + 255) / 256;
    hipLaunchKernelGGL(k_aov, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, s, f, cam, hits, which, out);
}

extern "C" {

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
    if (const hipError_t z = hipMemsetAsync(dOut, 0, 16 * stride * fb->N, st); z != hipSuccess) {
        hipFreeAsync(dOut, st);   // HIPCHK's status and text, after the free it has no room for
        return fail(ctx, z == hipErrorOutOfMemory ? MCRT_ERROR_OUT_OF_MEMORY : MCRT_ERROR_DEVICE,
                    std::string("hipMemsetAsync(dOut, 0, 16 * stride * fb->N, st): ") + hipGetErrorString(z));
    }
    launch_aov(scene_args(s), f, dCam, hits, aov, dOut, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, dOut, 16 * stride * fb->N, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFreeAsync(dOut, st);
    hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, MCRT_ERROR_DEVICE, std::string("aov: ") + hipGetErrorString(e));
    return MCRT_OK;
}

}  // extern "C"
