// mcrt_qnodes.hip -- the acceleration structure's converter: the leaves' parent links and the compact
// records of a flat tree (mcrt_traverse.h traverseQOct has the format and the exactness argument).
// mcrt_accel.cpp's finish() is the only caller of launch_leaf_parents and build_qnodes; the layout's
// offset arithmetic (qnode_offsets) is shared with the probe that imitates it (mcrt_probe.hip).
//
// Built with mcrt_kernels.o's flags, where the kernels came from: quantBytes divides on the device.
#include <rocprim/device/device_scan.hpp>

#include "mcrt_devbuf.h"
#include "mcrt_device.h"
#include "mcrt_internal.h"
#include "mcrt_traverse.h"

using mcrt::DevBuf;

// Parent links of the flat tree's leaves (the occluder hints' box test, mcrt_traverse.h
// hintOccludes): every internal record writes its index into word 13 of each child that is a
// triangle leaf (mcrt_bvh.cpp leaves carry -1 there; the traversal never reads it for a leaf).
__global__ __launch_bounds__(256) void k_leaf_parents(float4* __restrict__ nodes, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 w = *reinterpret_cast<const int4*>(&nodes[4 * (size_t)i + 3]);
    if (w.x < 0) return;
    const int ch[2] = {w.x, w.y};
    for (int k = 0; k < 2; ++k) {
        if ((uint32_t)ch[k] >= n) continue;
        int* cw = reinterpret_cast<int*>(&nodes[4 * (size_t)ch[k] + 3]);
        if (cw[0] == -1) cw[1] = (int)i;
    }
}

// Compact records (mcrt_traverse.h traverseQOct has the format and the exactness argument).
// Sizes in 16-B units per 64-B record (internal 2, leaf 3); notDfs: a left child that is not the
// next record (the LBVH's numbering) -- the compact walk takes the left child as the next record.
__global__ __launch_bounds__(256) void k_qnodes_sizes(const float4* __restrict__ nodes, uint32_t n,
                                                      uint32_t* __restrict__ units, int* __restrict__ notDfs) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 w = *reinterpret_cast<const int4*>(&nodes[4 * (size_t)i + 3]);
    units[i] = w.x >= 0 ? 2u : 3u;
    if (w.x >= 0 && w.x != (int)i + 1) atomicOr(notDfs, 1);
}

// One axis of an internal record: its origin (the smaller lo) and the exponent byte e of its step,
// 2^(e - 127) >= extent / 250.  False for non-finite boxes.
MCRT_DEV bool quantExp(float lo0, float hi0, float lo1, float hi1, float& o, uint32_t& e) {
    o = fminf(lo0, lo1);
    const float ext = fmaxf(hi0, hi1) - o;
    if (!(ext >= 0.0f) || ext == __builtin_inff()) return false;
    int k = -126;
    if (ext > 0.0f) frexpf(ext * (1.0f / 250.0f), &k);   // ext / 250 <= 2^k
    e = (uint32_t)min(max(k + 127, 1), 254);
    return true;
}
// The two children's (lo, hi) on that axis as bytes q with fmaf(q, s, o) <= lo and >= hi exactly as
// the traversal decodes them; s = the walk's step (qScales: 2^(e - 127) times a mantissa the meta
// word's lower fields supply: 1 for x, about 1.24 for y and z), so 255 s covers the extent.
// False if no byte reaches.
MCRT_DEV bool quantBytes(float lo0, float hi0, float lo1, float hi1, float o, float sc, uint32_t& bytes) {
    const float b[4] = {lo0, hi0, lo1, hi1};
    bytes = 0;
    for (int j = 0; j < 4; ++j) {
        const bool up = (j & 1) != 0;   // hi bounds round up, lo bounds down
        int q = (int)(up ? ceilf((b[j] - o) / sc) : floorf((b[j] - o) / sc));
        q = min(max(q, 0), 255);
        if (up) {
            while (q < 255 && fmaf((float)q, sc, o) < b[j]) ++q;
            if (fmaf((float)q, sc, o) < b[j]) return false;
        } else {
            while (q > 0 && fmaf((float)q, sc, o) > b[j]) --q;
            if (fmaf((float)q, sc, o) > b[j]) return false;
        }
        bytes |= (uint32_t)q << (8 * j);
    }
    return true;
}

__global__ __launch_bounds__(256) void k_qnodes_convert(const float4* __restrict__ nodes, uint32_t n,
                                                        const uint32_t* __restrict__ off, float4* __restrict__ q,
                                                        int* __restrict__ fail) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 n0 = nodes[4 * (size_t)i], n1 = nodes[4 * (size_t)i + 1], n2 = nodes[4 * (size_t)i + 2];
    const int4 w = *reinterpret_cast<const int4*>(&nodes[4 * (size_t)i + 3]);
    float4* dst = q + off[i];
    if (w.x >= 0) {   // child 0 box (n0.x, n0.z, n2.x)-(n0.y, n0.w, n2.y), child 1 (n1.x, n1.z, n2.z)-(n1.y, n1.w, n2.w)
        float ox, oy, oz;
        uint32_t bx = 0, by = 0, bz = 0, ex = 0, ey = 0, ez = 0;
        bool ok = quantExp(n0.x, n0.y, n1.x, n1.y, ox, ex) && quantExp(n0.z, n0.w, n1.z, n1.w, oy, ey) &&
                  quantExp(n2.x, n2.y, n2.z, n2.w, oz, ez) && (uint32_t)w.y < n;
        const uint32_t leaf0 = ok && reinterpret_cast<const int4*>(&nodes[4 * (size_t)w.x + 3])->x < 0 ? 1u : 0u;
        const uint32_t leaf1 = ok && reinterpret_cast<const int4*>(&nodes[4 * (size_t)w.y + 3])->x < 0 ? 1u : 0u;
        // the y and z steps carry a mantissa from the fields below their exponent (qScales: 1 + e_x / 512
        // for y, 1 + e_y / 512 + e_x / 2^18 for z, about 1.24): one exponent less then often still covers
        // the extent, which gives those axes the x axis's step sizes (1.44 x the ideal step on average
        // instead of 1.79); quantBytes decides, y first (z's mantissa depends on e_y)
        uint32_t meta = ex | (ey << 9) | (ez << 18) | (leaf0 << 27);
        if (ok && ey > 1 && quantBytes(n0.z, n0.w, n1.z, n1.w, oy, qScales(meta - (1u << 9)).y, by)) meta -= 1u << 9;
        if (ok && ez > 1 && quantBytes(n2.x, n2.y, n2.z, n2.w, oz, qScales(meta - (1u << 18)).z, bz)) meta -= 1u << 18;
        const QScales sc = qScales(meta);
        ok = ok && quantBytes(n0.x, n0.y, n1.x, n1.y, ox, sc.x, bx) && quantBytes(n0.z, n0.w, n1.z, n1.w, oy, sc.y, by) &&
             quantBytes(n2.x, n2.y, n2.z, n2.w, oz, sc.z, bz);
        if (!ok) {
            atomicOr(fail, 1);
            return;
        }
        dst[0] = make_float4(ox, oy, oz, __uint_as_float((off[w.y] << 1) | leaf1));
        dst[1] = make_float4(__uint_as_float(bx), __uint_as_float(by), __uint_as_float(bz), __uint_as_float(meta));
        return;
    }
// leaf: its exact box (as the parent's record stores it) must be min / max of v0, v0 + e1, v0 + e2
    // for the compact walk to test it from the triangle; else bit 31 sends the walk to the parent
    bool slow = true;
    const int par = w.y;   // k_leaf_parents
    if (par >= 0 && (uint32_t)par < n) {
        const float4 p0 = nodes[4 * (size_t)par], p1 = nodes[4 * (size_t)par + 1], p2 = nodes[4 * (size_t)par + 2];
        const bool right = reinterpret_cast<const int4*>(&nodes[4 * (size_t)par + 3])->y == (int)i;
        const f3 lo = right ? f3{p1.x, p1.z, p2.z} : f3{p0.x, p0.z, p2.x};
        const f3 hi = right ? f3{p1.y, p1.w, p2.w} : f3{p0.y, p0.w, p2.y};
        const f3 v0 = ld3(n0), v1 = v0 + ld3(n1), v2 = v0 + ld3(n2);
        const f3 l = f3{fminf(fminf(v0.x, v1.x), v2.x), fminf(fminf(v0.y, v1.y), v2.y), fminf(fminf(v0.z, v1.z), v2.z)};
        const f3 h = f3{fmaxf(fmaxf(v0.x, v1.x), v2.x), fmaxf(fmaxf(v0.y, v1.y), v2.y), fmaxf(fmaxf(v0.z, v1.z), v2.z)};
        slow = __float_as_uint(l.x) != __float_as_uint(lo.x) || __float_as_uint(l.y) != __float_as_uint(lo.y) ||
               __float_as_uint(l.z) != __float_as_uint(lo.z) || __float_as_uint(h.x) != __float_as_uint(hi.x) ||
               __float_as_uint(h.y) != __float_as_uint(hi.y) || __float_as_uint(h.z) != __float_as_uint(hi.z);
    }
    dst[0] = n0;
    dst[1] = n1;
    dst[2] = make_float4(n2.x, n2.y, n2.z, __uint_as_float(i | (slow ? 0x80000000u : 0u)));
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace mcrt {

void launch_leaf_parents(float4* nodes, uint32_t n, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_leaf_parents, dim3((n + 255) / 256), dim3(256), 0, st, nodes, n);
}

hipError_t qnode_offsets(uint32_t* units, uint32_t* off, uint32_t n, size_t* total, hipStream_t st) {
    *total = 0;
    // 2 units a record at the least: 2^30 records cannot stay below 2^31 units, and fewer cannot
    // wrap the 32-bit scan (3 n < 2^32), so the total read back below is the true one
    if (n == 0 || n >= (1u << 30)) return hipErrorNotSupported;
    DevBuf<uint8_t> tmp;
    size_t tmpBytes = 0;
    uint32_t last[2] = {0, 0};   // the last record's offset and size
    hipError_t e = rocprim::exclusive_scan(nullptr, tmpBytes, units, off, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
    if (e == hipSuccess) e = (hipError_t)tmp.alloc(tmpBytes);
    if (e == hipSuccess) e = rocprim::exclusive_scan(tmp.get(), tmpBytes, units, off, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(&last[0], off + n - 1, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&last[1], units + n - 1, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // tmp is free to go
    if (e != hipSuccess) return e;
    *total = (size_t)last[0] + last[1];
    // a record reference is (offset << 1 | leaf) in 32 bits, here and in the probe
    return *total >= ((size_t)1 << 31) ? hipErrorNotSupported : hipSuccess;
}

hipError_t build_qnodes(const float4* nodes, uint32_t n, DevBuf<float4>& q, hipStream_t st) {
    q.reset();
    if (n == 0) return hipErrorNotSupported;
    DevBuf<uint32_t> units, off;
    DevBuf<int> flags;   // [0] not depth-first, [1] a box the bytes cannot bound
    int h[2] = {0, 0};
    size_t total = 0;
    hipError_t e = (hipError_t)units.alloc(n);
    if (e == hipSuccess) e = (hipError_t)off.alloc(n);
    if (e == hipSuccess) e = (hipError_t)flags.alloc(2);
    if (e == hipSuccess) e = hipMemsetAsync(flags.get(), 0, 2 * sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_qnodes_sizes, dim3((n + 255) / 256), dim3(256), 0, st, nodes, n, units.get(), flags.get());
    e = hipMemcpyAsync(h, flags.get(), sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = qnode_offsets(units.get(), off.get(), n, &total, st);   // finishes st: h[0] is there
    if (e == hipSuccess && h[0] != 0) e = hipErrorNotSupported;
    if (e == hipSuccess) e = (hipError_t)q.alloc(total);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_qnodes_convert, dim3((n + 255) / 256), dim3(256), 0, st, nodes, n, off.get(), q.get(),
                           flags.get() + 1);
        e = hipMemcpyAsync(h + 1, flags.get() + 1, sizeof(int), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h[1] != 0) e = hipErrorNotSupported;
    if (e != hipSuccess) q.reset();
    return e;
}

hipError_t refit_qnode_offsets(const float4* nodes, uint32_t n, DevBuf<uint32_t>& off, size_t* total, hipStream_t st) {
    off.reset();
    *total = 0;
    if (n == 0) return hipErrorNotSupported;
    DevBuf<uint32_t> units;
    DevBuf<int> flag;   // not depth-first: such a tree has no compact records, and the caller knows
    hipError_t e = (hipError_t)units.alloc(n);
    if (e == hipSuccess) e = (hipError_t)off.alloc(n);
    if (e == hipSuccess) e = (hipError_t)flag.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(flag.get(), 0, sizeof(int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_qnodes_sizes, dim3((n + 255) / 256), dim3(256), 0, st, nodes, n, units.get(), flag.get());
        e = qnode_offsets(units.get(), off.get(), n, total, st);   // finishes st
    }
    if (e != hipSuccess) off.reset();
    return e;
}

hipError_t refit_qnodes(const float4* nodes, uint32_t n, const uint32_t* off, float4* q, int* flag, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_qnodes_convert, dim3((n + 255) / 256), dim3(256), 0, st, nodes, n, off, q, flag);
    return hipGetLastError();
}

}  // namespace mcrt
