// mcrt_denoise.hip -- guide-driven edge-avoiding a-trous wavelet denoiser (mcrt_denoise_guided) and
// the per-pixel luminance moments that steer it (k_moments).
//
// Dammertz et al. 2010 ("Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination
// Filtering") weights on a normal, a plane-offset and a luminance edge-stopping term, the luminance
// term scaled by a filtered per-pixel variance as in SVGF (Schied et al. 2017).  This file is built
// with -ffp-contract=off and IEEE division, so every line below is one float32 operation in the
// written order and tests/atrous_ref.py restates it in numpy; only expf is the device library's.
//
// Planes (W*H each): colour float4, normal-plane float4 (n.xyz, n.(P - cam.pos)), albedo-depth
// float4 (Kd.rgb, |P - cam.pos|, -1 on a miss), variance float, moments float2 (sum l, sum l*l).
#include <type_traits>

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
__global__ __launch_bounds__(256) void k_moments(FrameArgs f, int frame, const float4* __restrict__ radiance,
                                                 float2* __restrict__ moments) {
    const int lane = threadIdx.x & 63;
    const int tile = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int x, y;
    if (tile >= f.numTiles || !tilePixel(f, tile, lane, x, y)) return;
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

namespace mcrt {

void launch_temporal(const TemporalParams& t, bool eager, hipStream_t st) {
    TemporalMotionArgs a;
    a.W = t.W;
    a.H = t.H;
    a.demod = t.demod;
    a.haveHistory = t.haveHistory;
    a.alpha = t.alpha;
    a.alphaMoments = t.alphaMoments;
    a.maxHistory = t.maxHistory;
    a.normalThr = t.normalThr;
    a.planeThr = t.planeThr;
    const mcrt_camera& c = *t.cam;
    const mcrt_camera& o = *t.prev;
    const float cp[3] = {c.pos.x, c.pos.y, c.pos.z}, op[3] = {o.pos.x, o.pos.y, o.pos.z};
    const mcrt_float3* corner[4] = {&c.r00, &c.r10, &c.r11, &c.r01};
    float* dst[4] = {a.r00, a.r10, a.r11, a.r01};
    for (int i = 0; i < 4; ++i) {
        dst[i][0] = corner[i]->x;
        dst[i][1] = corner[i]->y;
        dst[i][2] = corner[i]->z;
    }
    for (int i = 0; i < 3; ++i) a.dpos[i] = cp[i] - op[i];
    const mcrt_float4* row[3] = {&o.worldToClip.m0, &o.worldToClip.m1, &o.worldToClip.m3};
    float* rdst[3] = {a.M0, a.M1, a.M3};
    for (int i = 0; i < 3; ++i) {
        rdst[i][0] = row[i]->x;
        rdst[i][1] = row[i]->y;
        rdst[i][2] = row[i]->z;
    }
    a.image = t.image;
    a.albedoDepth = t.albedoDepth;
    a.normalPlane = t.normalPlane;
    a.colourOld = t.colourOld;
    a.momentsOld = t.momentsOld;
    a.normalOld = t.normalOld;
    a.colourNew = t.colourNew;
    a.momentsNew = t.momentsNew;
    a.normalNew = t.normalNew;
    const dim3 grid((t.W + ATROUS_TILE - 1) / ATROUS_TILE, (t.H + ATROUS_TILE - 1) / ATROUS_TILE);
    const dim3 block(ATROUS_TILE * ATROUS_TILE);
    if (t.motion) {
        a.motion = t.motion;
        a.prevNormal = t.prevNormal;
        if (eager)
            hipLaunchKernelGGL(k_temporal_motion<true>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(k_temporal_motion<false>, grid, block, 0, st, a);
        return;
    }
    const TemporalArgs& base = a;
    if (eager)
        hipLaunchKernelGGL(k_temporal<true>, grid, block, 0, st, base);
    else
        hipLaunchKernelGGL(k_temporal<false>, grid, block, 0, st, base);
}

void launch_temporal_var(int W, int H, int minHistory, float normalThr, float planeThr, const float4* moments,
                         const float4* normalPlane, float* var, hipStream_t st) {
    const dim3 grid((W + ATROUS_TILE - 1) / ATROUS_TILE, (H + ATROUS_TILE - 1) / ATROUS_TILE);
    hipLaunchKernelGGL(k_temporal_var, grid, dim3(ATROUS_TILE * ATROUS_TILE), 0, st, W, H, (float)minHistory, normalThr,
                       planeThr, moments, normalPlane, var);
}

void launch_moments(const FrameArgs& f, int frame, const float4* radiance, float2* moments, hipStream_t st) {
    const int blocks = (f.numTiles * 64 + 255) / 256;
    hipLaunchKernelGGL(k_moments, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, f, frame, radiance, moments);
}

void launch_atrous_prep(int n, const float4* image, const float4* albedoDepth, const float2* moments, int frames,
                        int demod, float4* cOut, float* vOut, hipStream_t st) {
    hipLaunchKernelGGL(k_atrous_prep, dim3((n + 255) / 256), dim3(256), 0, st, n, image, albedoDepth, moments,
                       (float)frames, demod, cOut, vOut);
}

size_t atrous_lds_bytes(int step) {
    const size_t tw = ATROUS_TILE + 4 * (size_t)step;
    return tw * tw * 36;
}

void launch_atrous(int W, int H, int step, bool lds, float sigmaNormal, float sigmaDepth, float sigmaLevel, int useVar,
                   int remodulate, const float4* cIn, const float4* normalPlane, const float4* albedoDepth,
                   const float* vIn, float4* cOut, float* vOut, hipStream_t st) {
    AtrousArgs a;
    a.W = W;
    a.H = H;
    a.step = step;
    a.isn2 = 1.0f / (sigmaNormal * sigmaNormal);
    a.sigmaD = sigmaDepth;
    a.sl2 = sigmaLevel * sigmaLevel;
    a.useVar = useVar;
    a.remodulate = remodulate;
    a.cIn = cIn;
    a.normalPlane = normalPlane;
    a.albedoDepth = albedoDepth;
    a.vIn = vIn;
    a.cOut = cOut;
    a.vOut = vOut;
    const dim3 grid((W + ATROUS_TILE - 1) / ATROUS_TILE, (H + ATROUS_TILE - 1) / ATROUS_TILE);
    if (lds)
        hipLaunchKernelGGL(k_atrous<true>, grid, dim3(ATROUS_TILE * ATROUS_TILE), atrous_lds_bytes(step), st, a);
    else
        hipLaunchKernelGGL(k_atrous<false>, grid, dim3(ATROUS_TILE * ATROUS_TILE), 0, st, a);
}

}  // namespace mcrt
