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

}  // namespace

namespace mcrt {

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
