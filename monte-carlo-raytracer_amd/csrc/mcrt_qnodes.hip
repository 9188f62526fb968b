// mcrt_qnodes.hip -- the acceleration structure's converter: the leaves' parent links and the compact
// records of a flat tree (mcrt_traverse.h traverseQOct has the format and the exactness argument).
// mcrt_accel.cpp's finish() is the only caller of launch_leaf_parents and build_qnodes.  The records'
// order by cache line is qnode_order_offsets' (host); the back-to-back offset arithmetic
// (qnode_offsets) serves the probe that imitates the walk's fetches (mcrt_probe.hip).
//
// Built with mcrt_kernels.o's flags, where the kernels came from: quantBytes divides on the device.
#include <rocprim/device/device_scan.hpp>

#include <vector>

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
// The child words of every record for the host's ordering pass (qnode_order_offsets): (left, right),
// (-1, -1) for a leaf; notDfs: a left child that is not the next record (the LBVH's numbering) --
// the ordering pass takes parents before their children, which the depth-first numbering gives.
__global__ __launch_bounds__(256) void k_qnodes_kids(const float4* __restrict__ nodes, uint32_t n,
                                                     int2* __restrict__ kids, int* __restrict__ notDfs) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 w = *reinterpret_cast<const int4*>(&nodes[4 * (size_t)i + 3]);
    kids[i] = w.x >= 0 ? make_int2(w.x, w.y) : make_int2(-1, -1);
    if (w.x >= 0 && (w.x != (int)i + 1 || (uint32_t)w.y >= n || w.y <= w.x)) atomicOr(notDfs, 1);
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
        // bits 27..31: what the right child's reference is above the left child's, 2 x the 16-B units
        // between the two records + the leaf bits' difference (3..17: siblings are at most a line apart)
        const uint32_t step = ok ? 2u * (off[w.y] - off[w.x]) + leaf1 - leaf0 : 0u;
        uint32_t meta = ex | (ey << 9) | (ez << 18) | (step << 27);
        if (ok && ey > 1 && quantBytes(n0.z, n0.w, n1.z, n1.w, oy, qScales(meta - (1u << 9)).y, by)) meta -= 1u << 9;
        if (ok && ez > 1 && quantBytes(n2.x, n2.y, n2.z, n2.w, oz, qScales(meta - (1u << 18)).z, bz)) meta -= 1u << 18;
        const QScales sc = qScales(meta);
        ok = ok && quantBytes(n0.x, n0.y, n1.x, n1.y, ox, sc.x, bx) && quantBytes(n0.z, n0.w, n1.z, n1.w, oy, sc.y, by) &&
             quantBytes(n2.x, n2.y, n2.z, n2.w, oz, sc.z, bz);
        if (!ok) {
            atomicOr(fail, 1);
            return;
        }
        dst[0] = make_float4(ox, oy, oz, __uint_as_float((off[w.x] << 1) | leaf0));
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

// The order of the compact copy: off[i] = the 16-B unit at which record i starts, for
// a tree whose parents come before their children.  A 128-B line is 8 units; internal records take
// 2, leaves 3.
//   QORDER_SIBLINGS  the two children of a node side by side in one line, pairs in depth-first order;
//   QORDER_TREELETS  a node and both its children in one line (a treelet); each of the two children's
//                    own children starts a treelet, the two treelets of a sibling pair side by side
//                    (in one line where both fit), pairs in depth-first order.
// Siblings are never more than a line apart, so the walk reaches the right child from the left
// child's reference and the 5-bit step of the parent's meta word (which the 64-B tree's own order,
// the right child a whole subtree away, would not fit).
size_t qnode_order_offsets(const int* kids, uint32_t n, int order, uint32_t* off) {
    auto leaf = [&](uint32_t i) { return kids[2 * (size_t)i] < 0; };
    auto units = [&](uint32_t i) { return leaf(i) ? 3u : 2u; };
    auto fit = [](size_t cur, uint32_t u) { return (cur & 7u) + u > 8u ? (cur + 7u) & ~(size_t)7u : cur; };
    size_t cur = 0;
    auto place = [&](uint32_t i) { off[i] = (uint32_t)cur; cur += units(i); };
    place(0);
    if (order == QORDER_SIBLINGS) {
        for (uint32_t i = 0; i < n; ++i) {
            if (leaf(i)) continue;
            const uint32_t l = (uint32_t)kids[2 * (size_t)i], r = (uint32_t)kids[2 * (size_t)i + 1];
            cur = fit(cur, units(l) + units(r));
            place(l);
            place(r);
        }
        return cur;
    }
    std::vector<uint8_t> inner(n, 0);   // 1: a treelet's child member, whose children start treelets
    auto treelet = [&](uint32_t g) {    // g and its children, in one line
        if (leaf(g)) { cur = fit(cur, 3u); place(g); return; }
        const uint32_t l = (uint32_t)kids[2 * (size_t)g], r = (uint32_t)kids[2 * (size_t)g + 1];
        cur = fit(cur, 2u + units(l) + units(r));
        place(g);
        place(l);
        place(r);
        inner[l] = inner[r] = 1;
    };
    cur = 0;
    treelet(0);
    for (uint32_t i = 1; i < n; ++i) {
        if (!inner[i] || leaf(i)) continue;
        treelet((uint32_t)kids[2 * (size_t)i]);
        treelet((uint32_t)kids[2 * (size_t)i + 1]);
    }
    return cur;
}

// The offsets of a structure's compact records on the device, and *total = their units.  Finishes st.
// hipErrorNotSupported for a tree that is not depth-first and for a total >= 2^31 (a record
// reference is off << 1 | leaf).
static hipError_t order_offsets(const float4* nodes, uint32_t n, int order, DevBuf<uint32_t>& off, size_t* total,
                                hipStream_t st) {
    off.reset();
    *total = 0;
    if (n == 0 || n >= (1u << 30)) return hipErrorNotSupported;
    DevBuf<int2> kids;
    DevBuf<int> flag;
    int notDfs = 0;
    hipError_t e = (hipError_t)kids.alloc(n);
    if (e == hipSuccess) e = (hipError_t)flag.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(flag.get(), 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    std::vector<int> hk(2 * (size_t)n);
    hipLaunchKernelGGL(k_qnodes_kids, dim3((n + 255) / 256), dim3(256), 0, st, nodes, n, kids.get(), flag.get());
    e = hipMemcpyAsync(hk.data(), kids.get(), 2 * sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&notDfs, flag.get(), sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    if (notDfs) return hipErrorNotSupported;
    kids.reset();
    std::vector<uint32_t> ho(n);
    const size_t units = qnode_order_offsets(hk.data(), n, order, ho.data());
    if (units >= ((size_t)1 << 31)) return hipErrorNotSupported;
    e = (hipError_t)off.alloc(n);
    if (e == hipSuccess) e = hipMemcpyAsync(off.get(), ho.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // ho is free to go
    if (e != hipSuccess) off.reset();
    else *total = units;
    return e;
}

hipError_t build_qnodes(const float4* nodes, uint32_t n, int order, DevBuf<float4>& q, hipStream_t st) {
    q.reset();
    DevBuf<uint32_t> off;
    DevBuf<int> flag;   // a box the bytes cannot bound
    int h = 0;
    size_t total = 0;
    hipError_t e = order_offsets(nodes, n, order, off, &total, st);
    if (e == hipSuccess) e = (hipError_t)flag.alloc(1);
    if (e == hipSuccess) e = (hipError_t)q.alloc(total);
    // the padding between treelets is never read; zeroed so that the copy is a function of the tree
    if (e == hipSuccess) e = hipMemsetAsync(q.get(), 0, 16 * total, st);
    if (e == hipSuccess) e = refit_qnodes(nodes, n, off.get(), q.get(), flag.get(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h, flag.get(), sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h != 0) e = hipErrorNotSupported;
    if (e != hipSuccess) q.reset();
    return e;
}

hipError_t refit_qnode_offsets(const float4* nodes, uint32_t n, int order, DevBuf<uint32_t>& off, size_t* total,
                               hipStream_t st) {
    return order_offsets(nodes, n, order, off, total, st);
}

hipError_t refit_qnodes(const float4* nodes, uint32_t n, const uint32_t* off, float4* q, int* flag, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_qnodes_convert, dim3((n + 255) / 256), dim3(256), 0, st, nodes, n, off, q, flag);
    return hipGetLastError();
}

}  // namespace mcrt
