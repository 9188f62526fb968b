// mcrt_denoise.hip -- guide-driven edge-avoiding a-trous wavelet denoiser (mcrt_denoise_guided) and
// the per-pixel luminance moments that steer it (k_moments), its temporal history, and below the
// kernels the host entry points of all of it (each fills its kernel's argument struct and launches).
//
// Dammertz et al. 2010 ("Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination
// Filtering") weights on a normal, a plane-offset and a luminance edge-stopping term, the luminance
// term scaled by a filtered per-pixel variance as in SVGF (Schied et al. 2017).  This file is built
// with -ffp-contract=off and IEEE division, so every line below is one float32 operation in the
// written order and tests/atrous_ref.py restates it in numpy; only expf is the device library's.
//
// Planes (W*H each): colour float4, normal-plane float4 (n.xyz, n.(P - cam.pos)), albedo-depth
// float4 (Kd.rgb, |P - cam.pos|, -1 on a miss), variance float, moments float2 (sum l, sum l*l).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "mcrt_host.h"
#include "mcrt_shading.h"

namespace {

// k_tonemap's luminance, left to right
__device__ __forceinline__ float lum3(float r, float g, float b) {
    return (0.212671f * r + 0.715160f * g) + 0.072169f * b;
}

// Luminance moments of the frames k_accumulate has just added (same tiles, same clamp, frame order):
//   l = lum3(clamp(radiance.rgb, 0, 1000));  m1 += l;  m2 += l * l;   frame 0 overwrites.
// Unweighted on purpose: the reconstruction filter weight is one number per frame, and a variance
// of the samples, not of the weighted estimate, is what the edge-stopping term wants.
// LIST (adaptive sampling) as k_accumulate's: tile list[j], the tile's sample count for `frame`.
template <bool LIST>
__global__ __launch_bounds__(256) void k_moments(FrameArgs f, int frame, const float4* __restrict__ radiance,
                                                 float2* __restrict__ moments, const uint32_t* __restrict__ list,
                                                 const uint32_t* __restrict__ tileCount) {
    const int lane = threadIdx.x & 63;
    int tile = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (LIST) tile = (int)list[tile];
    int x, y;
    if (tile >= f.numTiles || !tilePixel(f, tile, lane, x, y)) return;
    if (LIST) frame = (int)tileCount[tile];
    const int pix = y * (int)f.W + x;
    float m1 = 0.0f, m2 = 0.0f;
    if (frame != 0) {
        const float2 o = moments[pix];
        m1 = o.x;
        m2 = o.y;
    }
    for (int k = 0; k < f.batch; ++k) {
        const float4 r4 = radiance[(size_t)k * f.W * f.H + pix];
        const float l = lum3(cl_clamp(r4.x, 0.0f, 1000.0f), cl_clamp(r4.y, 0.0f, 1000.0f), cl_clamp(r4.z, 0.0f, 1000.0f));
        const float ll = l * l;
        if (frame + k == 0) {
            m1 = l;
            m2 = ll;
        } else {
            m1 = m1 + l;
            m2 = m2 + ll;
        }
    }
    moments[pix] = make_float2(m1, m2);
}

// albedo channel a colour channel is divided by / multiplied back with
__device__ __forceinline__ float demodChannel(float a) { return a > 1e-3f ? a : 1.0f; }

// Level input 0:  c = image (rgb / demodChannel(albedo.rgb) with demodulation), alpha kept;
//   with moments of n >= 2 frames:  mean = m1 / n;  var = max(0, m2 / n - mean * mean) / (n - 1);
//   otherwise var = 1.
__global__ __launch_bounds__(256) void k_atrous_prep(int n, const float4* __restrict__ image,
                                                     const float4* __restrict__ albedoDepth,
                                                     const float2* __restrict__ moments, float frames, int demod,
                                                     float4* __restrict__ cOut, float* __restrict__ vOut) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 c = image[i];
    if (demod) {
        const float4 a = albedoDepth[i];
        c.x = c.x / demodChannel(a.x);
        c.y = c.y / demodChannel(a.y);
        c.z = c.z / demodChannel(a.z);
    }
    float v = 1.0f;
    if (moments) {
        const float2 m = moments[i];
        const float mean = m.x / frames;
        v = fmaxf(0.0f, m.y / frames - mean * mean) / (frames - 1.0f);
    }
    cOut[i] = c;
    vOut[i] = v;
}

// k_atrous_prep in adaptive mode: the same lines with n the sample count of the pixel's 8x8 tile
// (tiles differ); n < 2 gives var = 1.  `moments` NULL: var = 1 everywhere.
__global__ __launch_bounds__(256) void k_atrous_prep_tiles(int W, int H, const float4* __restrict__ image,
                                                           const float4* __restrict__ albedoDepth,
                                                           const float2* __restrict__ moments,
                                                           const uint32_t* __restrict__ tileCount, int demod,
                                                           float4* __restrict__ cOut, float* __restrict__ vOut) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    float4 c = image[i];
    if (demod) {
        const float4 a = albedoDepth[i];
        c.x = c.x / demodChannel(a.x);
        c.y = c.y / demodChannel(a.y);
        c.z = c.z / demodChannel(a.z);
    }
    float v = 1.0f;
    if (moments) {
        const int y = i / W, x = i - y * W;
        const uint32_t cnt = tileCount[(y >> 3) * ((W + 7) >> 3) + (x >> 3)];
        if (cnt >= 2u) {
            const float frames = (float)cnt;
            const float2 m = moments[i];
            const float mean = m.x / frames;
            v = fmaxf(0.0f, m.y / frames - mean * mean) / (frames - 1.0f);
        }
    }
    cOut[i] = c;
    vOut[i] = v;
}

struct AtrousArgs {
    int W, H, step;
    float isn2;       // 1 / (sigma_normal * sigma_normal)
    float sigmaD;     // sigma_depth
    float sl2;        // sigma_i * sigma_i (sigma_i of this level)
    int useVar;       // 1: v_p = 3x3 Gaussian of the variance plane, 0: v_p = 1
    int remodulate;   // last level with demodulation: rgb * demodChannel(albedo.rgb)
    const float4* cIn;
    const float4* normalPlane;
    const float4* albedoDepth;
    const float* vIn;
    float4* cOut;
    float* vOut;
};

#define ATROUS_TILE 16

// One level, step s, pixel p = (x, y); float32, each line one operation in this order:
//   z_p  = depth_p > 0 ? depth_p : 1                      (albedo-depth .w; -1 on a miss)
//   sdz  = sigmaD * z_p;  isd2 = 1 / (sdz * sdz);  isn2 = 1 / (sigma_normal * sigma_normal)
//   v_p  = useVar ? sum over (j, i) in -1..1 (j = row offset outer, i inner) of g[j] * g[i] * var at
//          the coordinates clamped to the image, g = [1/4, 1/2, 1/4], accumulated from 0 : 1
//   idl2 = 1 / (sl2 * v_p + 1e-8f)                       (sl2 = sigma_i * sigma_i)
//   l_p  = lum3(c_p.rgb)
//   for dy in -2..2 (outer), dx in -2..2 (inner), q = p + s * (dx, dy) inside the image:
//     dn  = n_p - n_q (xyz);  dn2 = (dn.x * dn.x + dn.y * dn.y) + dn.z * dn.z
//     dd  = d_p - d_q;        dl = l_p - lum3(c_q.rgb)
//     e   = (dn2 * isn2 + (dd * dd) * isd2) + (dl * dl) * idl2
//     w   = (h[dx] * h[dy]) * expf(-e),  h = [1/16, 1/4, 3/8, 1/4, 1/16]
//     sw += w;  sc.rgb += w * c_q.rgb;  sv += (w * w) * var_q        (sums start at 0)
//   c'.rgb = sc.rgb / sw;  c'.a = c_p.a;  var' = sv / (sw * sw)
//   remodulate: c'.rgb = c'.rgb * demodChannel(albedo_p.rgb)
// The three denominators belong to the centre pixel, so each is inverted once (an IEEE division)
// and the 25 taps multiply: with a division per term the kernel was bound by its 75 divisions per
// pixel, at 13-23 % of its bandwidth floor.
// LDS = true stages the 16x16 tile and its 2s halo -- colour with its luminance in .w, the
// normal-plane record and the variance, 36 B per pixel -- once per workgroup; LDS = false reads the
// taps from memory.  Both evaluate the lines above on the same values, so they agree bit for bit.
template <bool LDS>
__global__ __launch_bounds__(ATROUS_TILE * ATROUS_TILE) void k_atrous(AtrousArgs a) {
    extern __shared__ float4 smem[];
    const int W = a.W, H = a.H, s = a.step;
    const int tx = threadIdx.x & (ATROUS_TILE - 1), ty = threadIdx.x / ATROUS_TILE;
    const int x = blockIdx.x * ATROUS_TILE + tx, y = blockIdx.y * ATROUS_TILE + ty;
    const int TW = ATROUS_TILE + 4 * s;
    const int x0 = blockIdx.x * ATROUS_TILE - 2 * s, y0 = blockIdx.y * ATROUS_TILE - 2 * s;
    float4* sC = smem;
    float4* sN = smem + TW * TW;
    float* sV = reinterpret_cast<float*>(smem + 2 * TW * TW);
    if (LDS) {
        for (int i = threadIdx.x; i < TW * TW; i += ATROUS_TILE * ATROUS_TILE) {
            const int gy = y0 + i / TW, gx = x0 + i % TW;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = c;
            float v = 0.0f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {   // taps outside the image are never read
                const size_t g = (size_t)gy * W + gx;
                c = a.cIn[g];
                c.w = lum3(c.x, c.y, c.z);
                n = a.normalPlane[g];
                v = a.vIn[g];
            }
            sC[i] = c;
            sN[i] = n;
            sV[i] = v;
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 cp = a.cIn[p];
    const float4 np = a.normalPlane[p];
    const float4 ad = a.albedoDepth[p];
    const float zp = ad.w > 0.0f ? ad.w : 1.0f;
    const float sdz = a.sigmaD * zp;
    const float isd2 = 1.0f / (sdz * sdz);
    float vp = 1.0f;
    if (a.useVar) {
        vp = 0.0f;
        for (int j = -1; j <= 1; ++j) {
            const int yy = min(max(y + j, 0), H - 1);
            for (int i = -1; i <= 1; ++i) {
                const int xx = min(max(x + i, 0), W - 1);
                const float g = (j == 0 ? 0.5f : 0.25f) * (i == 0 ? 0.5f : 0.25f);
                vp = vp + g * a.vIn[(size_t)yy * W + xx];
            }
        }
    }
    const float idl2 = 1.0f / (a.sl2 * vp + 1e-8f);
    const float lp = lum3(cp.x, cp.y, cp.z);
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= H) continue;
        const float hy = dy == 0 ? 0.375f : (dy == -1 || dy == 1) ? 0.25f : 0.0625f;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= W) continue;
            const float hx = dx == 0 ? 0.375f : (dx == -1 || dx == 1) ? 0.25f : 0.0625f;
            float4 cq, nq;
            float vq, lq;
            if (LDS) {
                const int i = (qy - y0) * TW + (qx - x0);
                cq = sC[i];
                nq = sN[i];
                vq = sV[i];
                lq = cq.w;
            } else {
                const size_t q = (size_t)qy * W + qx;
                cq = a.cIn[q];
                nq = a.normalPlane[q];
                vq = a.vIn[q];
                lq = lum3(cq.x, cq.y, cq.z);
            }
            const float dnx = np.x - nq.x, dny = np.y - nq.y, dnz = np.z - nq.z;
            const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
            const float dd = np.w - nq.w;
            const float dl = lp - lq;
            const float e = (dn2 * a.isn2 + (dd * dd) * isd2) + (dl * dl) * idl2;
            const float w = (hx * hy) * expf(-e);
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            sv = sv + (w * w) * vq;
        }
    }
    float4 o = make_float4(sr / sw, sg / sw, sb / sw, cp.w);
    if (a.remodulate) {
        o.x = o.x * demodChannel(ad.x);
        o.y = o.y * demodChannel(ad.y);
        o.z = o.z * demodChannel(ad.z);
    }
    a.cOut[p] = o;
    a.vOut[p] = sv / (sw * sw);
}

// ---- temporal reprojection and history (mcrt_temporal_accumulate) -----------------------------
// History planes (W*H each, old read / new written): colour float4 in filter space, moments float4
// (mu1, mu2, N, z) = integrated luminance moments, history length, guide depth when written (-1 on
// a miss), and the normal-plane record the pixel had when written.

// One pixel p = (x, y) per lane; float32, each line one operation in this order (IEEE / and sqrtf):
//   c = image[p];  ad = albedoDepth[p];  g = normalPlane[p]
//   demodulate: c.rgb = c.rgb / demodChannel(ad.rgb);   l = lum3(c.rgb);  ll = l * l
//   have = false;  with a history and ad.w > 0:
//     u = (float)x / (float)W;  v = (float)y / (float)H
//     a = r00 + (r10 - r00) * u;  b = r01 + (r11 - r01) * u;  m = a + (b - a) * v      (per component)
//     k = ad.w / sqrtf((m.x * m.x + m.y * m.y) + m.z * m.z)
//     r = m * k + dpos            (dpos = cam.pos - prev.pos, one float32 subtraction on the host;
//                                  r = P - prev.pos, the world point itself is never formed)
//     cx = (M0.x * r.x + M0.y * r.y) + M0.z * r.z;  cy with M1;  cw with M3   (rows of prev.worldToClip,
//          xyz only: for a view-projection centred on prev.pos the dropped column cancels exactly)
//     cw > 0:  fx = ((cx / cw + 1) * 0.5f) * W;  fy = ((cy / cw + 1) * 0.5f) * H
//     fx > -1 && fx < W && fy > -1 && fy < H   (NaN and huge values never reach the int cast):
//       ix = (int)floorf(fx);  tx = fx - (float)ix;  iy, ty likewise
//       zr = sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z);  tol = planeThr * zr
//       for j in 0, 1 (outer), i in 0, 1, q = (ix + i, iy + j) inside the image:
//         hm = momentsOld[q];  pn = normalOld[q];  dn = g.xyz - pn.xyz
//         valid = hm.w > 0 && (dn.x * dn.x + dn.y * dn.y) + dn.z * dn.z <= normalThr
//                 && fabsf(((pn.x * r.x + pn.y * r.y) + pn.z * r.z) - pn.w) <= tol
//         w = (i ? tx : 1 - tx) * (j ? ty : 1 - ty)
//         valid:  sw += w;  sc.rgb += w * colourOld[q].rgb;  s1 += w * hm.x;  s2 += w * hm.y;  sn += w * hm.z
//       have = sw > 1e-4f
//   have:  N = fminf(sn / sw + 1, maxHistory);  al = fmaxf(alpha, 1 / N);  am = fmaxf(alphaMoments, 1 / N)
//          out.rgb = (sc.rgb / sw) * (1 - al) + c.rgb * al
//          mu1 = (s1 / sw) * (1 - am) + l * am;  mu2 = (s2 / sw) * (1 - am) + ll * am
//   else:  N = 1;  out.rgb = c.rgb;  mu1 = l;  mu2 = ll
//   colourNew[p] = (out.rgb, c.a);  momentsNew[p] = (mu1, mu2, N, ad.w);  normalNew[p] = g
// EAGER = true issues the four taps' twelve 16-B records together; EAGER = false fetches the eight
// validity records first and a tap's colour only when the tap is valid.  Same values, same bits.
//
// MOTION = true (mcrt_temporal_accumulate_motion) reprojects through the per-object motion of
// k_guides_motion's planes; the lines that change:
//   mv = motion[p]                                   (issued with image / albedoDepth / normalPlane)
//   r  = m * k + dpos                                as above
//   mv.w == 1:  r = r + mv.xyz (per component);  gp = prevNormal[p].xyz
//   mv.w == 0:  gp = g.xyz                           (any other mv.w >= 0 likewise)
//   mv.w <  0:  no taps are tested (have = false): N = 1, the current values, bit for bit
//   cx, cy, cw, fx, fy, zr, tol from r as above;  dn = gp - pn.xyz;  res from r as above
//   normalNew[p] = g                                 (the current record, as above)
// prevNormal[p] is fetched where mv.w == 1 only: issued with the first batch instead it cost 7.7 %
// more when nothing moved and the same when everything did.
// With an all-zero motion plane the three planes written are those of MOTION = false, bit for bit.
struct TemporalArgs {
    int W, H;
    int demod, haveHistory;
    float alpha, alphaMoments, maxHistory, normalThr, planeThr;
    float r00[3], r10[3], r11[3], r01[3];   // current camera's corner directions
    float dpos[3];                          // cam.pos - prev.pos
    float M0[3], M1[3], M3[3];              // prev.worldToClip rows 0, 1, 3 (xyz)
    const float4* image;
    const float4* albedoDepth;
    const float4* normalPlane;
    const float4* colourOld;
    const float4* momentsOld;
    const float4* normalOld;
    float4* colourNew;
    float4* momentsNew;
    float4* normalNew;
};
struct TemporalMotionArgs : TemporalArgs {
    const float4* motion;       // (P_prev - P, flag)
    const float4* prevNormal;   // (n_prev, 0) where flag is 1
};

template <bool EAGER, bool MOTION>
__device__ __forceinline__ void temporalPixel(const typename std::conditional<MOTION, TemporalMotionArgs, TemporalArgs>::type& a) {
    const int W = a.W, H = a.H;
    const int x = blockIdx.x * ATROUS_TILE + (threadIdx.x & (ATROUS_TILE - 1));
    const int y = blockIdx.y * ATROUS_TILE + threadIdx.x / ATROUS_TILE;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    float4 c = a.image[p];
    const float4 ad = a.albedoDepth[p];
    const float4 g = a.normalPlane[p];
    float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp = g;
    if constexpr (MOTION) {
        mv = a.motion[p];
    }
    if (a.demod) {
        c.x = c.x / demodChannel(ad.x);
        c.y = c.y / demodChannel(ad.y);
        c.z = c.z / demodChannel(ad.z);
    }
    const float l = lum3(c.x, c.y, c.z);
    const float ll = l * l;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f, sn = 0.0f;
    bool have = false;
    if (a.haveHistory && ad.w > 0.0f && !(MOTION && mv.w < 0.0f)) {
        const float u = (float)x / (float)W, v = (float)y / (float)H;
        float m[3], r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float ea = a.r00[k] + (a.r10[k] - a.r00[k]) * u;
            const float eb = a.r01[k] + (a.r11[k] - a.r01[k]) * u;
            m[k] = ea + (eb - ea) * v;
        }
        const float k = ad.w / sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = m[i] * k + a.dpos[i];
        if constexpr (MOTION) {
            if (mv.w == 1.0f) {
                r[0] = r[0] + mv.x;
                r[1] = r[1] + mv.y;
                r[2] = r[2] + mv.z;
                gp = a.prevNormal[p];
            }
        }
        const float cx = (a.M0[0] * r[0] + a.M0[1] * r[1]) + a.M0[2] * r[2];
        const float cy = (a.M1[0] * r[0] + a.M1[1] * r[1]) + a.M1[2] * r[2];
        const float cw = (a.M3[0] * r[0] + a.M3[1] * r[1]) + a.M3[2] * r[2];
        if (cw > 0.0f) {
            const float fx = ((cx / cw + 1.0f) * 0.5f) * (float)W;
            const float fy = ((cy / cw + 1.0f) * 0.5f) * (float)H;
            if (fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) {
                const int ix = (int)floorf(fx), iy = (int)floorf(fy);
                const float tx = fx - (float)ix, ty = fy - (float)iy;
                const float zr = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
                const float tol = a.planeThr * zr;
                float4 hm[4], pn[4], hc[4];
                bool in[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {   // t = 2 j + i; every in-image tap's loads are issued here
                    const int qx = ix + (t & 1), qy = iy + (t >> 1);
                    in[t] = qx >= 0 && qx < W && qy >= 0 && qy < H;
                    const size_t q = in[t] ? (size_t)qy * W + qx : p;
                    hm[t] = a.momentsOld[q];
                    pn[t] = a.normalOld[q];
                    if (EAGER) hc[t] = a.colourOld[q];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float dnx = gp.x - pn[t].x, dny = gp.y - pn[t].y, dnz = gp.z - pn[t].z;
                    const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
                    const float res = fabsf(((pn[t].x * r[0] + pn[t].y * r[1]) + pn[t].z * r[2]) - pn[t].w);
                    const bool valid = in[t] && hm[t].w > 0.0f && dn2 <= a.normalThr && res <= tol;
                    if (!valid) continue;
                    if (!EAGER) hc[t] = a.colourOld[(size_t)(iy + (t >> 1)) * W + (ix + (t & 1))];
                    const float w = ((t & 1) ? tx : 1.0f - tx) * ((t >> 1) ? ty : 1.0f - ty);
                    sw = sw + w;
                    sr = sr + w * hc[t].x;
                    sg = sg + w * hc[t].y;
                    sb = sb + w * hc[t].z;
                    s1 = s1 + w * hm[t].x;
                    s2 = s2 + w * hm[t].y;
                    sn = sn + w * hm[t].z;
                }
                have = sw > 1e-4f;
            }
        }
    }
    float N = 1.0f, mu1 = l, mu2 = ll;
    float4 o = c;
    if (have) {
        N = fminf(sn / sw + 1.0f, a.maxHistory);
        const float al = fmaxf(a.alpha, 1.0f / N), am = fmaxf(a.alphaMoments, 1.0f / N);
        o.x = (sr / sw) * (1.0f - al) + c.x * al;
        o.y = (sg / sw) * (1.0f - al) + c.y * al;
        o.z = (sb / sw) * (1.0f - al) + c.z * al;
        mu1 = (s1 / sw) * (1.0f - am) + l * am;
        mu2 = (s2 / sw) * (1.0f - am) + ll * am;
    }
    a.colourNew[p] = o;
    a.momentsNew[p] = make_float4(mu1, mu2, N, ad.w);
    a.normalNew[p] = g;
}

template <bool EAGER>
__global__ __launch_bounds__(ATROUS_TILE * ATROUS_TILE) void k_temporal(TemporalArgs a) {
    temporalPixel<EAGER, false>(a);
}

template <bool EAGER>
__global__ __launch_bounds__(ATROUS_TILE * ATROUS_TILE) void k_temporal_motion(TemporalMotionArgs a) {
    temporalPixel<EAGER, true>(a);
}

// The variance handed to the filter, from the planes k_temporal has just written; float32, each
// line one operation in this order:
//   (mu1, mu2, N, z) = moments[p];  n_p, d_p = normalPlane[p] (xyz, w)
//   N >= minHistory:  var = fmaxf(0, mu2 - mu1 * mu1)
//   else, over dy in -3..3 (outer), dx in -3..3, q = p + (dx, dy) inside the image and on p's surface:
//       s1 += mu1_q;  s2 += mu2_q;  cnt += 1                         (sums start at 0; q = p always counts)
//     p's surface: z_p <= 0 and z_q <= 0, or both > 0 with
//       dn = n_p - n_q;  (dn.x * dn.x + dn.y * dn.y) + dn.z * dn.z <= normalThr  and
//       dd = d_p - d_q;  t = planeThr * z_p;  dd * dd <= t * t
//     m1 = s1 / cnt;  m2 = s2 / cnt;  var = fmaxf(0, m2 - m1 * m1) * (minHistory / N)
// The variance of the samples (SVGF), not of the mean.  A workgroup with a pixel on the spatial
// path stages the moments and normal-plane records of its 16x16 tile and 3-pixel halo in LDS once
// (read from memory per tap, the 49 x 32 B of every pixel took 0.27 ms at 1080p after a reset);
// the values and the operations on them are the same either way.
__global__ __launch_bounds__(ATROUS_TILE * ATROUS_TILE) void k_temporal_var(int W, int H, float minHistory,
                                                                            float normalThr, float planeThr,
                                                                            const float4* __restrict__ moments,
                                                                            const float4* __restrict__ normalPlane,
                                                                            float* __restrict__ var) {
    constexpr int TW = ATROUS_TILE + 6;   // the tile and its 3-pixel halo: 2 x 7.6 KB of LDS
    __shared__ float4 sM[TW * TW];
    __shared__ float4 sN[TW * TW];
    const int x0 = blockIdx.x * ATROUS_TILE - 3, y0 = blockIdx.y * ATROUS_TILE - 3;
    const int x = blockIdx.x * ATROUS_TILE + (threadIdx.x & (ATROUS_TILE - 1));
    const int y = blockIdx.y * ATROUS_TILE + threadIdx.x / ATROUS_TILE;
    const bool inside = x < W && y < H;
    const size_t p = inside ? (size_t)y * W + x : 0;
    const float4 mp = moments[p];
    const bool spatial = inside && !(mp.z >= minHistory);
    // a workgroup none of whose pixels takes the spatial path (the steady state) stages nothing
    if (!__syncthreads_or(spatial)) {
        if (inside) var[p] = fmaxf(0.0f, mp.y - mp.x * mp.x);
        return;
    }
    for (int i = threadIdx.x; i < TW * TW; i += ATROUS_TILE * ATROUS_TILE) {
        const int gy = y0 + i / TW, gx = x0 + i % TW;
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = m;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {   // records outside the image are never read
            const size_t g = (size_t)gy * W + gx;
            m = moments[g];
            n = normalPlane[g];
        }
        sM[i] = m;
        sN[i] = n;
    }
    __syncthreads();
    if (!inside) return;
    if (!spatial) {
        var[p] = fmaxf(0.0f, mp.y - mp.x * mp.x);
        return;
    }
    const float4 np = sN[(y - y0) * TW + (x - x0)];
    const float t = planeThr * mp.w;
    const float t2 = t * t;
    float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const int q = (qy - y0) * TW + (qx - x0);
            const float4 mq = sM[q];
            const float4 nq = sN[q];
            bool same = dx == 0 && dy == 0;
            if (!same) {
                if (mp.w > 0.0f) {
                    const float dnx = np.x - nq.x, dny = np.y - nq.y, dnz = np.z - nq.z;
                    const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
                    const float dd = np.w - nq.w;
                    same = mq.w > 0.0f && dn2 <= normalThr && dd * dd <= t2;
                } else {
                    same = !(mq.w > 0.0f);
                }
            }
            if (same) {
                s1 = s1 + mq.x;
                s2 = s2 + mq.y;
                cnt = cnt + 1.0f;
            }
        }
    }
    const float m1 = s1 / cnt, m2 = s2 / cnt;
    var[p] = fmaxf(0.0f, m2 - m1 * m1) * (minHistory / mp.z);
}

}  // namespace

// called by mcrt_accumulate (mcrt_pt_host.cpp) while fb->dn.momentsOn
void mcrt::launch_moments(const FrameArgs& f, int frame, const float4* radiance, float2* moments, hipStream_t st,
                          const uint32_t* list, int listLen, const uint32_t* tileCount) {
    if (list) {
        hipLaunchKernelGGL(k_moments<true>, dim3((listLen * 64 + 255) / 256), dim3(256), 0, st, f, frame, radiance, moments,
                           list, tileCount);
        return;
    }
    const int blocks = (f.numTiles * 64 + 255) / 256;
    hipLaunchKernelGGL(k_moments<false>, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, f, frame, radiance, moments, list,
                       tileCount);
}

// ---------------------------------------------------------------------------
// Host entry points.  Their state is fb->dn (DenoiseState, mcrt_host.h); from the rest of the
// runtime they take the accumulated image, the display plane, the current slot's camera and
// primary-hit buffers and the context stream.
// ---------------------------------------------------------------------------
using mcrt::fail, mcrt::env_int, mcrt::ensure_plane, mcrt::fb_sync;

static const dim3 kTileBlock(ATROUS_TILE * ATROUS_TILE);
static dim3 tile_grid(int W, int H) { return dim3((W + ATROUS_TILE - 1) / ATROUS_TILE, (H + ATROUS_TILE - 1) / ATROUS_TILE); }

static hipError_t ensure_guides(mcrt_framebuffer fb) {
    hipError_t e = ensure_plane(fb, fb->dn.guideNormal);
    if (e == hipSuccess) e = ensure_plane(fb, fb->dn.guideAlbedo);
    return e;
}

static hipError_t ensure_motion(mcrt_framebuffer fb) {
    hipError_t e = ensure_plane(fb, fb->dn.motion);
    if (e == hipSuccess) e = ensure_plane(fb, fb->dn.motionNormal);
    return e;
}

// mcrt_render_guides and, with `motion`, mcrt_render_guides_motion: the same host path, one launch
// of k_guides or of k_guides_motion
static mcrt_status render_guides(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, const mcrt_frame_params* p,
                                 bool motion) {
    if (!s || !fb || !cam || !p) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = s->ctx;
    if (fb->ctx != ctx) return fail(ctx, MCRT_ERROR_INVALID_ARG, "frame buffer belongs to another context");
    if (!mcrt::accel_ready(s)) return fail(ctx, MCRT_ERROR_NOT_READY, "mcrt_accel_build has not been called");
    if (cam->width != fb->W || cam->height != fb->H)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "camera size differs from the frame buffer");
    FrameArgs f;
    std::string err;
    if (!mcrt::frame_args(fb, p, f, err)) return fail(ctx, MCRT_ERROR_INVALID_ARG, err);
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    DenoiseState& d = fb->dn;
    HIPCHK(ctx, ensure_guides(fb));
    if (motion) HIPCHK(ctx, ensure_motion(fb));
    mcrt_camera* dCam = nullptr;   // as mcrt_render_aov: the current slot's camera and primary-hit buffers are reused
    float4* hits = nullptr;
    const mcrt_status borrowed = mcrt::borrow_camera_hits(s, fb, cam, f, &dCam, &hits);
    if (borrowed != MCRT_OK) return borrowed;
    if (motion) {
        Timed t(ctx, K_GUIDES_MOTION, nullptr, (int64_t)f.numTiles * 64);
        mcrt::launch_guides_motion(mcrt::scene_args(s), f, dCam, hits, d.guideNormal.get(), d.guideAlbedo.get(),
                                   mcrt::scene_prev_poses(s), d.motion.get(), d.motionNormal.get(), st);
    } else {
        Timed t(ctx, K_GUIDES, nullptr, (int64_t)f.numTiles * 64);
        mcrt::launch_guides(mcrt::scene_args(s), f, dCam, hits, d.guideNormal.get(), d.guideAlbedo.get(), st);
    }
    HIPCHK(ctx, hipGetLastError());
    // the slot's next render (its own stream) may overwrite those buffers only after this pass
    HIPCHK(ctx, mcrt::release_slot(fb, st));
    d.haveGuides = true;
    d.haveMotion = motion;
    return MCRT_OK;
}

// The tail the plane read-backs share once `src` (NULL: not allocated yet) and its size are chosen:
// *needed, then a NULL destination (a size query), not ready, too small, in that order; the copy
// waits for every stream of the frame buffer
static mcrt_status read_plane(mcrt_framebuffer fb, const void* src, uint64_t need, void* host_dst, uint64_t bytes,
                              uint64_t* needed, const char* notReady) {
    mcrt_ctx ctx = fb->ctx;
    if (needed) *needed = need;
    if (!host_dst) return MCRT_OK;
    if (!src) return fail(ctx, MCRT_ERROR_NOT_READY, notReady);
    if (bytes < need) return fail(ctx, MCRT_ERROR_INVALID_ARG, "destination too small");
    hipSetDevice(ctx->device);
    HIPCHK(ctx, fb_sync(fb));
    HIPCHK(ctx, hipMemcpy(host_dst, src, need, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

// ---- temporal reprojection and history ----
static hipError_t ensure_temporal(mcrt_framebuffer fb) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = ensure_plane(fb, fb->dn.tColour[i]);
        if (e == hipSuccess) e = ensure_plane(fb, fb->dn.tMoments[i]);
        if (e == hipSuccess) e = ensure_plane(fb, fb->dn.tNormal[i]);
    }
    if (e == hipSuccess) e = ensure_plane(fb, fb->dn.tVar);
    return e;
}

// MCRT_TEMPORAL_LOADS selects k_temporal's load form for measurements and the test that both agree
// bit for bit: "eager" issues all twelve tap records together, anything else (the default, the
// form measured faster) fetches the eight validity records first and a tap's colour only when valid.
static bool temporal_eager_loads() {
    const char* e = std::getenv("MCRT_TEMPORAL_LOADS");
    return e && std::strcmp(e, "eager") == 0;
}

static void copy3(float* dst, float x, float y, float z) { dst[0] = x; dst[1] = y; dst[2] = z; }

// mcrt_temporal_accumulate and, with `motion`, mcrt_temporal_accumulate_motion: k_temporal (or
// k_temporal_motion) reprojects the old history planes of the history's camera into the pixels of
// `cam` and writes the new ones, k_temporal_var then derives the variance plane from them
static mcrt_status temporal_accumulate(mcrt_framebuffer fb, const mcrt_camera* cam, const mcrt_temporal_params* p,
                                       bool motion) {
    if (!fb || !cam || !p) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    DenoiseState& d = fb->dn;
    if (mcrt::adaptive_on(fb))   // the history integrates whole images of one sample count
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "mcrt_temporal_accumulate is not available in adaptive mode");
    if (!(p->alpha >= 0.0f && p->alpha <= 1.0f) || !(p->alpha_moments >= 0.0f && p->alpha_moments <= 1.0f))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "alpha and alpha_moments must be in 0 .. 1");
    if (p->max_history < 1 || p->min_history < 1)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "max_history and min_history must be >= 1");
    if (!(p->normal_threshold > 0.0f) || !(p->plane_threshold > 0.0f))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "thresholds must be positive");
    if (cam->width != fb->W || cam->height != fb->H)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "camera size differs from the frame buffer");
    if (!d.haveGuides) return fail(ctx, MCRT_ERROR_NOT_READY, "no guides (mcrt_render_guides / mcrt_framebuffer_set_guides)");
    if (motion && !d.haveMotion)
        return fail(ctx, MCRT_ERROR_NOT_READY,
                    "no motion planes for these guides (mcrt_render_guides_motion / mcrt_framebuffer_set_motion)");
    if (mcrt::bdpt_pending_gather(fb))
        return fail(ctx, MCRT_ERROR_NOT_READY, "band-split BDPT frame not completed (mcrt_bdpt_gather)");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, ensure_temporal(fb));
    const int old = d.tCur, now = old ^ 1;
    const mcrt_camera& c = *cam;
    const mcrt_camera& o = d.tHaveHistory ? d.tPrevCam : *cam;
    TemporalMotionArgs a;
    a.W = (int)fb->W;
    a.H = (int)fb->H;
    a.demod = p->demodulate_albedo ? 1 : 0;
    a.haveHistory = d.tHaveHistory ? 1 : 0;
    a.alpha = p->alpha;
    a.alphaMoments = p->alpha_moments;
    a.maxHistory = (float)p->max_history;
    a.normalThr = p->normal_threshold;
    a.planeThr = p->plane_threshold;
    copy3(a.r00, c.r00.x, c.r00.y, c.r00.z);
    copy3(a.r10, c.r10.x, c.r10.y, c.r10.z);
    copy3(a.r11, c.r11.x, c.r11.y, c.r11.z);
    copy3(a.r01, c.r01.x, c.r01.y, c.r01.z);
    copy3(a.dpos, c.pos.x - o.pos.x, c.pos.y - o.pos.y, c.pos.z - o.pos.z);
    copy3(a.M0, o.worldToClip.m0.x, o.worldToClip.m0.y, o.worldToClip.m0.z);
    copy3(a.M1, o.worldToClip.m1.x, o.worldToClip.m1.y, o.worldToClip.m1.z);
    copy3(a.M3, o.worldToClip.m3.x, o.worldToClip.m3.y, o.worldToClip.m3.z);
    a.image = fb->image.get();
    a.albedoDepth = d.guideAlbedo.get();
    a.normalPlane = d.guideNormal.get();
    a.colourOld = d.tColour[old].get();
    a.momentsOld = d.tMoments[old].get();
    a.normalOld = d.tNormal[old].get();
    a.colourNew = d.tColour[now].get();
    a.momentsNew = d.tMoments[now].get();
    a.normalNew = d.tNormal[now].get();
    a.motion = d.motion.get();
    a.prevNormal = d.motionNormal.get();
    const dim3 grid = tile_grid(a.W, a.H);
    const bool eager = temporal_eager_loads();
    {
        Timed tm(ctx, motion ? K_TEMPORAL_MOTION : K_TEMPORAL, nullptr, (int64_t)fb->N);
        const TemporalArgs& base = a;
        if (motion && eager)
            hipLaunchKernelGGL(k_temporal_motion<true>, grid, kTileBlock, 0, st, a);
        else if (motion)
            hipLaunchKernelGGL(k_temporal_motion<false>, grid, kTileBlock, 0, st, a);
        else if (eager)
            hipLaunchKernelGGL(k_temporal<true>, grid, kTileBlock, 0, st, base);
        else
            hipLaunchKernelGGL(k_temporal<false>, grid, kTileBlock, 0, st, base);
    }
    {
        Timed tm(ctx, K_TEMPORAL_VAR, nullptr, (int64_t)fb->N);
        hipLaunchKernelGGL(k_temporal_var, grid, kTileBlock, 0, st, a.W, a.H, (float)p->min_history, p->normal_threshold,
                           p->plane_threshold, a.momentsNew, a.normalNew, d.tVar.get());
    }
    HIPCHK(ctx, hipGetLastError());
    d.tCur = now;
    d.tHaveHistory = true;
    d.tAccumulated = true;
    d.tFedBack = false;
    d.tDemod = a.demod;
    d.tPrevCam = *cam;
    return MCRT_OK;
}

// Largest step whose level runs the tile-staged kernel (36 KB of LDS at step 4); larger steps read
// their taps from memory.  MCRT_ATROUS_LDS_MAX_STEP overrides it (0: never stage) for measurements
// and the test that both kernels agree bit for bit.
static int atrous_lds_max_step() {
    return env_int("MCRT_ATROUS_LDS_MAX_STEP", 4, 0, 8);   // step 8: 48 x 48 x 36 B = 81 KB does not fit 64 KB
}
static size_t atrous_lds_bytes(int step) {
    const size_t tw = ATROUS_TILE + 4 * (size_t)step;
    return tw * tw * 36;
}

// the two scratch colour / variance planes the levels ping-pong between
static hipError_t ensure_atrous(mcrt_framebuffer fb) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = ensure_plane(fb, fb->dn.atrousC[i]);
        if (e == hipSuccess) e = ensure_plane(fb, fb->dn.atrousV[i]);
    }
    return e;
}

// Level 0's input of an a-trous chain: colour in filter space and its variance plane.
struct AtrousIn {
    const float4* colour = nullptr;
    const float* var = nullptr;
    int useVar = 0;
};
using AtrousBegin = mcrt_status (*)(mcrt_framebuffer, const mcrt_guided_denoise_params*, AtrousIn&);

// The a-trous chain of mcrt_denoise_guided and mcrt_denoise_guided_temporal: the checks they share
// (in their order), then `begin` -- the caller's own checks and whatever makes level 0's input --
// then the levels, ping-ponging between the scratch planes, and the tone-map tail.  The output of
// level `feedback_level` (-1: none) becomes the colour history.
static mcrt_status atrous_chain(mcrt_framebuffer fb, const mcrt_guided_denoise_params* p, int feedback_level,
                                AtrousBegin begin) {
    mcrt_ctx ctx = fb->ctx;
    DenoiseState& d = fb->dn;
    const int demod = p->demodulate_albedo ? 1 : 0;
    if (p->levels < 1 || p->levels > MCRT_ATROUS_MAX_LEVELS)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "levels must be 1 .. 8");
    if (!(p->sigma_normal > 0.0f) || !(p->sigma_depth > 0.0f) || !(p->sigma_luminance > 0.0f))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "sigmas must be positive");
    if (feedback_level < -1 || feedback_level > p->levels - 2)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "feedback_level must be -1 .. levels - 2");
    if (!d.haveGuides) return fail(ctx, MCRT_ERROR_NOT_READY, "no guides (mcrt_render_guides / mcrt_framebuffer_set_guides)");
    if (mcrt::bdpt_pending_gather(fb))
        return fail(ctx, MCRT_ERROR_NOT_READY, "band-split BDPT frame not completed (mcrt_bdpt_gather)");
    hipSetDevice(ctx->device);
    AtrousIn in;
    const mcrt_status bs = begin(fb, p, in);
    if (bs != MCRT_OK) return bs;
    HIPCHK(ctx, ensure_atrous(fb));
    hipStream_t st = ctx->stream;
    const int ldsMax = atrous_lds_max_step();
    AtrousArgs a;
    a.W = (int)fb->W;
    a.H = (int)fb->H;
    a.isn2 = 1.0f / (p->sigma_normal * p->sigma_normal);
    a.sigmaD = p->sigma_depth;
    a.useVar = in.useVar;
    a.cIn = in.colour;
    a.normalPlane = d.guideNormal.get();
    a.albedoDepth = d.guideAlbedo.get();
    a.vIn = in.var;
    int dst = a.cIn == d.atrousC[0].get() ? 1 : 0;   // never the plane level 0 reads
    for (int i = 0; i < p->levels; ++i) {
        const bool last = i + 1 == p->levels;
        a.step = 1 << i;
        const float sigmaLevel = in.useVar ? p->sigma_luminance : p->sigma_luminance * std::ldexp(1.0f, -i);
        a.sl2 = sigmaLevel * sigmaLevel;
        a.remodulate = last && demod ? 1 : 0;
        // the last level writes the display image, or a scratch plane when k_tonemap follows
        a.cOut = last && !p->use_tonemapping ? fb->display.get() : d.atrousC[dst].get();
        a.vOut = d.atrousV[dst].get();
        {
            Timed t(ctx, K_ATROUS + i, nullptr, (int64_t)fb->N);
            if (a.step <= ldsMax && atrous_lds_bytes(a.step) <= 64 * 1024)
                hipLaunchKernelGGL(k_atrous<true>, tile_grid(a.W, a.H), kTileBlock, atrous_lds_bytes(a.step), st, a);
            else
                hipLaunchKernelGGL(k_atrous<false>, tile_grid(a.W, a.H), kTileBlock, 0, st, a);
        }
        if (i == feedback_level) {
            // this level's output (never the last level's: a scratch plane) becomes the colour history
            // by exchanging the two planes; the old history plane, which only level 0 read, is scratch
            // from now on, and no later level writes the new history plane
            std::swap(d.tColour[d.tCur], d.atrousC[dst]);
            d.tFedBack = true;
        }
        a.cIn = a.cOut;
        a.vIn = a.vOut;
        dst ^= 1;
    }
    d.filteredVar = dst ^ 1;
    if (p->use_tonemapping) mcrt::launch_tonemap(a.W * a.H, p->min_luminance, a.cIn, fb->display.get(), st);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

extern "C" {

MCRT_API mcrt_status mcrt_render_guides(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam,
                                        const mcrt_frame_params* p) {
    return render_guides(s, fb, cam, p, false);
}

MCRT_API mcrt_status mcrt_render_guides_motion(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam,
                                               const mcrt_frame_params* p) {
    return render_guides(s, fb, cam, p, true);
}

MCRT_API mcrt_status mcrt_framebuffer_set_guides(mcrt_framebuffer fb, const void* d_normal_plane,
                                                 const void* d_albedo_depth) {
    if (!fb || !d_normal_plane || !d_albedo_depth) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    DenoiseState& d = fb->dn;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, ensure_guides(fb));
    HIPCHK(ctx, hipMemcpyAsync(d.guideNormal.get(), d_normal_plane, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d.guideAlbedo.get(), d_albedo_depth, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    d.haveGuides = true;
    d.haveMotion = false;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_set_motion(mcrt_framebuffer fb, const void* d_motion, const void* d_prev_normal) {
    if (!fb || !d_motion || !d_prev_normal) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    DenoiseState& d = fb->dn;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, ensure_motion(fb));
    HIPCHK(ctx, hipMemcpyAsync(d.motion.get(), d_motion, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d.motionNormal.get(), d_prev_normal, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    d.haveMotion = true;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_read_motion(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                  uint64_t* needed) {
    if (!fb || which < 0 || which > 1) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    const void* src = which == 0 ? fb->dn.motion.get() : fb->dn.motionNormal.get();
    return read_plane(fb, src, 16 * (uint64_t)fb->N, host_dst, bytes, needed, "no motion planes yet");
}

MCRT_API mcrt_status mcrt_framebuffer_set_moments_enabled(mcrt_framebuffer fb, int on) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    mcrt_ctx ctx = fb->ctx;
    DenoiseState& d = fb->dn;
    if (!on && mcrt::adaptive_on(fb))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "adaptive mode needs the moments (mcrt_framebuffer_set_adaptive(fb, NULL) first)");
    hipSetDevice(ctx->device);
    if (on && !d.moments) {
        HIPCHK(ctx, ensure_plane(fb, d.moments));
        d.momentFrames = 0;
    }
    d.momentsOn = on != 0;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_set_moments(mcrt_framebuffer fb, const void* d_m1m2, int32_t frames) {
    if (!fb || !d_m1m2 || frames < 0) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    mcrt_ctx ctx = fb->ctx;
    DenoiseState& d = fb->dn;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, ensure_plane(fb, d.moments));
    HIPCHK(ctx, hipMemcpyAsync(d.moments.get(), d_m1m2, 8 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    d.momentFrames = frames;
    HIPCHK(ctx, mcrt::adaptive_set_counts(fb, frames));   // adaptive mode: every tile holds `frames` samples
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_read_guides(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                  uint64_t* needed) {
    if (!fb || which < 0 || which > 3) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    const DenoiseState& d = fb->dn;
    const void* src = which == 0 ? (const void*)d.guideNormal.get() : which == 1 ? (const void*)d.guideAlbedo.get()
                      : which == 2 ? (const void*)d.moments.get()
                      : d.filteredVar < 0 ? nullptr : (const void*)d.atrousV[d.filteredVar].get();
    const uint64_t need = (which < 2 ? 16 : which == 2 ? 8 : 4) * (uint64_t)fb->N;
    return read_plane(fb, src, need, host_dst, bytes, needed, "no such guide data yet");
}

MCRT_API mcrt_status mcrt_denoise_guided(mcrt_framebuffer fb, const mcrt_guided_denoise_params* p) {
    if (!fb || !p) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    return atrous_chain(fb, p, -1, [](mcrt_framebuffer fb, const mcrt_guided_denoise_params* p, AtrousIn& in) {
        mcrt_ctx ctx = fb->ctx;
        DenoiseState& d = fb->dn;
        HIPCHK(ctx, ensure_atrous(fb));   // k_atrous_prep writes level 0's input to the first scratch planes
        const int n = (int)fb->N;
        Timed t(ctx, K_ATROUS_PREP, nullptr, (int64_t)fb->N);
        const bool useVar = p->use_variance && d.moments && d.momentFrames >= 2;
        if (mcrt::adaptive_on(fb)) {   // n per pixel from its tile's count
            hipLaunchKernelGGL(k_atrous_prep_tiles, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (int)fb->W, (int)fb->H,
                               fb->image.get(), d.guideAlbedo.get(), useVar ? d.moments.get() : nullptr,
                               mcrt::adaptive_counts(fb), p->demodulate_albedo ? 1 : 0, d.atrousC[0].get(),
                               d.atrousV[0].get());
            in = {d.atrousC[0].get(), d.atrousV[0].get(), useVar ? 1 : 0};
            return MCRT_OK;
        }
        hipLaunchKernelGGL(k_atrous_prep, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, fb->image.get(),
                           d.guideAlbedo.get(), useVar ? d.moments.get() : nullptr, (float)d.momentFrames,
                           p->demodulate_albedo ? 1 : 0, d.atrousC[0].get(), d.atrousV[0].get());
        in = {d.atrousC[0].get(), d.atrousV[0].get(), useVar ? 1 : 0};
        return MCRT_OK;
    });
}

MCRT_API mcrt_status mcrt_temporal_accumulate(mcrt_framebuffer fb, const mcrt_camera* cam,
                                              const mcrt_temporal_params* p) {
    return temporal_accumulate(fb, cam, p, false);
}

MCRT_API mcrt_status mcrt_temporal_accumulate_motion(mcrt_framebuffer fb, const mcrt_camera* cam,
                                                     const mcrt_temporal_params* p) {
    return temporal_accumulate(fb, cam, p, true);
}

MCRT_API mcrt_status mcrt_temporal_reset(mcrt_framebuffer fb) {
    if (!fb) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "fb is NULL");
    fb->dn.tHaveHistory = false;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_set_temporal_history(mcrt_framebuffer fb, const void* d_colour,
                                                           const void* d_moments, const void* d_normal_plane,
                                                           const mcrt_camera* prev_camera) {
    if (!fb || !d_colour || !d_moments || !d_normal_plane || !prev_camera)
        return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    mcrt_ctx ctx = fb->ctx;
    DenoiseState& d = fb->dn;
    if (prev_camera->width != fb->W || prev_camera->height != fb->H)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "camera size differs from the frame buffer");
    hipSetDevice(ctx->device);
    HIPCHK(ctx, ensure_temporal(fb));
    const int cur = d.tCur;
    HIPCHK(ctx, hipMemcpyAsync(d.tColour[cur].get(), d_colour, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d.tMoments[cur].get(), d_moments, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d.tNormal[cur].get(), d_normal_plane, 16 * fb->N, hipMemcpyDeviceToDevice, ctx->stream));
    d.tPrevCam = *prev_camera;
    d.tHaveHistory = true;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_framebuffer_read_temporal(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                    uint64_t* needed) {
    if (!fb || which < 0 || which > 3) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "bad args");
    const DenoiseState& d = fb->dn;
    const int cur = d.tCur;
    const void* src = which == 0 ? (const void*)d.tColour[cur].get() : which == 1 ? (const void*)d.tMoments[cur].get()
                      : which == 2 ? (const void*)d.tVar.get() : (const void*)d.tNormal[cur].get();
    const uint64_t need = (which == 2 ? 4 : 16) * (uint64_t)fb->N;
    return read_plane(fb, src, need, host_dst, bytes, needed, "no temporal history yet");
}

MCRT_API mcrt_status mcrt_denoise_guided_temporal(mcrt_framebuffer fb, const mcrt_guided_denoise_params* p,
                                                  int32_t feedback_level) {
    if (!fb || !p) return fail(fb ? fb->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "NULL argument");
    return atrous_chain(fb, p, feedback_level, [](mcrt_framebuffer fb, const mcrt_guided_denoise_params* p, AtrousIn& in) {
        mcrt_ctx ctx = fb->ctx;
        const DenoiseState& d = fb->dn;
        const int demod = p->demodulate_albedo ? 1 : 0;
        if (!d.tAccumulated) return fail(ctx, MCRT_ERROR_NOT_READY, "no mcrt_temporal_accumulate yet");
        if (d.tFedBack)
            return fail(ctx, MCRT_ERROR_NOT_READY, "the colour history already holds a filtered level of this accumulate");
        if (demod != d.tDemod)
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "demodulate_albedo differs from the last mcrt_temporal_accumulate");
        // level 0 reads the colour history (already in filter space) and the variance plane
        in = {d.tColour[d.tCur].get(), d.tVar.get(), p->use_variance ? 1 : 0};
        return MCRT_OK;
    });
}

}  // extern "C"
