// mcrt_refit.hip -- refit of a flat structure on the device (mcrt_accel_refit): the
// topology of the last build stays, every leaf is recomputed from the scene's current vertices and
// shape transforms, and every box above it bottom-up.  mcrt_accel.cpp is the only caller.
//
// Exactness.  A leaf is what the builders write for its (shape, primitive): the world transform
// with xrow's separately rounded products and sums (mcrt_gpubuild.hip k_prims, the host's
// xformPoint), the edges as v1 - v0 and v2 - v0, the box with k_prims' selects.  A box above is
// fminf / fmaxf of its two children, which do not round, so the order in which the two children
// arrive changes no bit (but the sign of a zero).  Built with -ffp-contract=off, as
// mcrt_topbuild.hip is.
//
// The numbering does not matter: the kernels read the child words only (pre-order for the SAH
// builders, internal records first for the LBVH).
#include <hip/hip_runtime.h>

#include "mcrt_internal.h"

namespace {

constexpr int BLOCK = 256;

// RR transform_point (mathutils.h:111-118), as mcrt_gpubuild.hip xrow
__device__ __forceinline__ float xrow(const mcrt_float4& r, float x, float y, float z) {
    float acc = 0.0f;
    acc = __fadd_rn(acc, __fmul_rn(r.x, x));
    acc = __fadd_rn(acc, __fmul_rn(r.y, y));
    acc = __fadd_rn(acc, __fmul_rn(r.z, z));
    acc = __fadd_rn(acc, __fmul_rn(r.w, 0.0f));
    return __fadd_rn(acc, r.w);
}

// Once per structure: every internal record names itself the parent of its two children; the root
// (the one record nobody names) keeps the -1 the array was filled with.
__global__ __launch_bounds__(BLOCK) void k_refit_parents(const float4* __restrict__ nodes, uint32_t n,
                                                         int* __restrict__ parent) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int4 w = *reinterpret_cast<const int4*>(&nodes[4 * (size_t)i + 3]);
    if (w.x < 0) return;
    if ((uint32_t)w.x < n) parent[w.x] = (int)i;
    if ((uint32_t)w.y < n) parent[w.y] = (int)i;
}

// One thread per record; the leaves' threads work.  A leaf rewrites its triangle, then carries its
// box in registers up the tree: at each parent it writes the box into the parent's slot for this
// child and arrives at the parent's counter.  The first arrival is done; the second reads its
// sibling's slot, merges and goes on.  Release/acquire through the arrival counter, k_bottom_up's
// shape (mcrt_gpubuild.hip): publish the slot, add, acquire, read the sibling's.  No thread waits
// for another.  arrive is zero on entry.
__global__ __launch_bounds__(BLOCK) void k_refit(float4* nodes, uint32_t n, const mcrt_shape* __restrict__ shapes,
                                                 uint32_t numShapes, const uint32_t* __restrict__ indices,
                                                 const float4* __restrict__ positions, const int* __restrict__ parent,
                                                 int* arrive) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float4* rec = &nodes[4 * (size_t)i];
    if (reinterpret_cast<const int4*>(rec + 3)->x >= 0) return;
    float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];   // the id words 3 and 7 and word 11 go back as they are
    const uint32_t shapeId = __float_as_uint(r0.w), primId = __float_as_uint(r1.w);
    if (shapeId >= numShapes) return;   // not a triangle of this scene: left alone
    const mcrt_shape& sh = shapes[shapeId];
    if (primId >= (uint32_t)sh.numTriangles) return;
    float p[9];
    for (int k = 0; k < 3; ++k) {
        const float4 v = positions[sh.startVertex + indices[sh.startIdx + 3 * primId + k]];
        p[3 * k + 0] = xrow(sh.toWorldTransform.m0, v.x, v.y, v.z);
        p[3 * k + 1] = xrow(sh.toWorldTransform.m1, v.x, v.y, v.z);
        p[3 * k + 2] = xrow(sh.toWorldTransform.m2, v.x, v.y, v.z);
    }
    rec[0] = make_float4(p[0], p[1], p[2], r0.w);
    rec[1] = make_float4(p[3] - p[0], p[4] - p[1], p[5] - p[2], r1.w);
    rec[2] = make_float4(p[6] - p[0], p[7] - p[1], p[8] - p[2], r2.w);
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {   // k_prims' selects
        const float x = p[a], y = p[3 + a], z = p[6 + a];
        const float m0 = (y < x) ? y : x, x0 = (x < y) ? y : x;
        lo[a] = (z < m0) ? z : m0;
        hi[a] = (x0 < z) ? z : x0;
    }
    int child = (int)i;
    int node = parent[i];
    while (node >= 0) {
        float4* pr = &nodes[4 * (size_t)node];
        // internal record: c0 x/y slabs, c1 x/y slabs, z slabs of both, children
        const int right = reinterpret_cast<const int4*>(pr + 3)->y == child ? 1 : 0;
        // the slot as three (lo, hi) pairs: x, y at float2 2 right, 2 right + 1; z at 4 + right
        unsigned long long* slab = reinterpret_cast<unsigned long long*>(pr);
        const int mine[3] = {2 * right, 2 * right + 1, 4 + right};
        const int other[3] = {2 * (right ^ 1), 2 * (right ^ 1) + 1, 4 + (right ^ 1)};
        // release: the slot is stored write-through at agent scope and has left this wave before the
        // arrival counts (in place of k_bottom_up's release fence, which writes the whole L2 back
        // per wave and level: DESIGN.md 2j has both measured)
        for (int a = 0; a < 3; ++a)
            __hip_atomic_store(&slab[mine[a]], ((unsigned long long)__float_as_uint(hi[a]) << 32) | __float_as_uint(lo[a]),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(&arrive[node], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            return;   // the sibling's thread finishes the node
        // acquire: this CU's L1 may hold the record's line from before the sibling wrote its slot
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        for (int a = 0; a < 3; ++a) {
            const unsigned long long s = __hip_atomic_load(&slab[other[a]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lo[a] = fminf(lo[a], __uint_as_float((uint32_t)s));
            hi[a] = fmaxf(hi[a], __uint_as_float((uint32_t)(s >> 32)));
        }
        child = node;
        node = parent[node];
    }
}

}  // namespace

namespace mcrt {

hipError_t launch_refit_parents(const float4* nodes, uint32_t n, int* parent, hipStream_t st) {
    hipError_t e = hipMemsetAsync(parent, 0xff, sizeof(int) * (size_t)n, st);   // -1: the root has no parent
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_refit_parents, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, nodes, n, parent);
    return hipGetLastError();
}

hipError_t launch_refit(float4* nodes, uint32_t n, const mcrt_shape* dShapes, uint32_t numShapes, const uint32_t* dIndices,
                        const float4* dPositions, const int* parent, int* arrive, hipStream_t st) {
    hipError_t e = hipMemsetAsync(arrive, 0, sizeof(int) * (size_t)n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_refit, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, nodes, n, dShapes, numShapes, dIndices,
                       dPositions, parent, arrive);
    return hipGetLastError();
}

}  // namespace mcrt
