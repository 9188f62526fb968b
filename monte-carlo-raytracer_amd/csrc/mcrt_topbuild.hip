// mcrt_topbuild.hip -- on-device build of the two-level structure's top tree for gfx950
// (mcrt_accel_update_transforms, path 1).
//
// When only transforms change RadeonRays keeps every per-mesh tree, recomputes the world boxes
// with transform_bbox and builds a new top-level Bvh over them (the Refit branch,
// RR/src/intersector/intersector_2level.cpp:495-660).  This file restates that Bvh
// (RR/src/accelerator/bvh.cpp:73-437) the way ObjBvh does on the host (mcrt_bvh2l.cpp), node for
// node, and writes the records straight into the scene's array:
//
//   * world box of a top-level shape = transformBox's operation order (corners lo + (0|ext),
//     xform's add sequence); compiled -ffp-contract=off, divisions through double (exactly the
//     correctly rounded float quotient);
//   * split = binned SAH over all three axes, the first best (axis, bin) wins (strict <); empty
//     bins keep the host's +-FLT_MAX boxes, so their NaN prices lose the same way;
//   * the two-sided partition in its closed form (mcrt_sahbuild.hip's header): with nL references
//     going left, the k-th misplaced reference left of nL swaps with the k-th misplaced one counted
//     from the end, so the order inside a range -- which later median splits read -- is the host's;
//   * a one-sided partition falls back to the median and keeps the boxes the partition grew
//     (bvh.cpp:198-212);
//   * pre-order numbering (left p + 1, right p + 2 nLeft), one shape per leaf.
// Box reductions are order-free min/max: only the sign of a zero bound can differ from the host.
//
// Schedule: a request of more than SMALL references is split by one workgroup, level by level
// (the host reads the next level's request count); every request of at most SMALL references is
// finished by one wave that walks its subtree with a stack in LDS (smaller child next, so the
// stack stays O(log SMALL)).  Both run the same splitNode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "mcrt_internal.h"

namespace {

constexpr int MAXB = 64;        // bins supported on the device path (as mcrt_sahbuild.hip)
constexpr int SMALL = 256;      // requests up to this many references finish in one wave
constexpr int BT = 256;         // threads of a large request's workgroup
constexpr int MAX_LEVELS = 1024;   // levels of large requests; beyond: the host path
constexpr int SMALL_STACK = 16;

struct Req {   // one BuildNode call (bvh.cpp:73): its range, record and the boxes its parent grew
    float b[6], cb[6];
    uint32_t start, num, index, level;
};
struct Counters {
    uint32_t big, small, height, error;
    int root[12];   // ordered ints: box lo, box hi, centroid lo, centroid hi
};
struct TopEnt {
    int32_t shape, meshBase, mesh, pad;
};
struct Params {
    const mcrt_shape* shapes;
    const mcrt_mat4* w2l;   // NULL: transpose of toWorldInverseTranspose
    const TopEnt* top;      // per top-level shape, world order
    const float* meshBox;
    float4 *lo, *hi, *cen;  // world box and centroid of each top-level shape
    uint32_t *refs, *slots;
    float4* nodes;
    Req *bigA, *bigB, *small;
    uint32_t capBig, capSmall;
    uint32_t n, nb;
    float cost;
    int sahOn;
    Counters* ctr;
};

__device__ __forceinline__ int oi(float f) {   // monotonic float -> int
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float of(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }
__device__ __forceinline__ float fdiv(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float ax3(const float4& v, int a) { return a == 0 ? v.x : a == 1 ? v.y : v.z; }
// bbox::surface_area (bbox.h): 2 (xy + xz + yz)
__device__ __forceinline__ float area6(const float* b) {
    const float x = b[3] - b[0], y = b[4] - b[1], z = b[5] - b[2];
    return 2.f * (x * y + x * z + y * z);
}
// std::min / std::max as the host's Box::grow applies them
__device__ __forceinline__ float smin(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float smax(float a, float b) { return a < b ? b : a; }

// ---------------------------------------------------------------------------
// world boxes (transform_bbox, mathutils.h:142-158) and the root request's bounds
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_boxes(Params P) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    float v[12];
    for (int k = 0; k < 12; ++k) v[k] = ((k / 3) & 1) ? -FLT_MAX : FLT_MAX;
    if (i < P.n) {
        const TopEnt t = P.top[i];
        const float* mb = &P.meshBox[6 * t.mesh];
        const mcrt_mat4& M = P.shapes[t.shape].toWorldTransform;
        const mcrt_float4 rows[3] = {M.m0, M.m1, M.m2};
        const float e[3] = {mb[3] - mb[0], mb[4] - mb[1], mb[5] - mb[2]};
        const int sel[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}, {0, 0, 1}};
        float lo[3], hi[3];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float p[3], q[3];
            for (int a = 0; a < 3; ++a) p[a] = mb[a] + (sel[c][a] ? e[a] : 0.0f);
            for (int r = 0; r < 3; ++r) {
                float acc = 0.0f;
                acc += rows[r].x * p[0];
                acc += rows[r].y * p[1];
                acc += rows[r].z * p[2];
                acc += rows[r].w * 0.0f;
                q[r] = acc + rows[r].w;
            }
            for (int a = 0; a < 3; ++a) {
                lo[a] = c == 0 ? q[a] : smin(lo[a], q[a]);
                hi[a] = c == 0 ? q[a] : smax(hi[a], q[a]);
            }
        }
        float cn[3];
        for (int a = 0; a < 3; ++a) cn[a] = 0.5f * (hi[a] + lo[a]);
        P.lo[i] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        P.hi[i] = make_float4(hi[0], hi[1], hi[2], 0.0f);
        P.cen[i] = make_float4(cn[0], cn[1], cn[2], 0.0f);
        P.refs[i] = i;
        for (int a = 0; a < 3; ++a) {
            v[a] = lo[a];
            v[3 + a] = hi[a];
            v[6 + a] = v[9 + a] = cn[a];
        }
    }
    for (int k = 0; k < 12; ++k) {
        const bool isMax = (k / 3) & 1;
        float x = v[k];
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(x, off);
            x = isMax ? fmaxf(x, o) : fminf(x, o);
        }
        if ((threadIdx.x & 63) == 0) {
            if (isMax) atomicMax(&P.ctr->root[k], oi(x));
            else atomicMin(&P.ctr->root[k], oi(x));
        }
    }
}

// instance record (mcrt_bvh2l.cpp): world -> object rows + (-2, bottom root, shape id, 0)
__device__ void writeInstance(const Params& P, uint32_t node, uint32_t ref) {
    const TopEnt t = P.top[ref];
    float4 r0, r1, r2;
    if (P.w2l) {
        const mcrt_mat4& m = P.w2l[t.shape];
        r0 = make_float4(m.m0.x, m.m0.y, m.m0.z, m.m0.w);
        r1 = make_float4(m.m1.x, m.m1.y, m.m1.z, m.m1.w);
        r2 = make_float4(m.m2.x, m.m2.y, m.m2.z, m.m2.w);
    } else {   // inverse = transpose(inverse transpose)
        const mcrt_mat4& m = P.shapes[t.shape].toWorldInverseTranspose;
        r0 = make_float4(m.m0.x, m.m1.x, m.m2.x, m.m3.x);
        r1 = make_float4(m.m0.y, m.m1.y, m.m2.y, m.m3.y);
        r2 = make_float4(m.m0.z, m.m1.z, m.m2.z, m.m3.z);
    }
    float4* o = &P.nodes[4 * (size_t)node];
    o[0] = r0;
    o[1] = r1;
    o[2] = r2;
    o[3] = make_float4(__int_as_float(-2), __int_as_float(t.meshBase), __int_as_float(t.shape), 0.0f);
}

// the root request, or the single instance record of a one-shape top level
__global__ void k_root(Params P) {
    Counters& c = *P.ctr;
    if (P.n == 1) {
        writeInstance(P, 0, 0);
        return;
    }
    Req r;
    for (int k = 0; k < 6; ++k) {
        r.b[k] = of(c.root[k]);
        r.cb[k] = of(c.root[6 + k]);
    }
    r.start = 0;
    r.num = P.n;
    r.index = 0;
    r.level = 0;
    if (P.n > (uint32_t)SMALL) {
        P.bigA[0] = r;
        c.big = 1;
    } else {
        P.small[0] = r;
        c.small = 1;
    }
}

// ---------------------------------------------------------------------------
// one BuildNode: split, partition, record, child requests
// ---------------------------------------------------------------------------
struct Shared {
    int bins[3 * MAXB * 7];   // per axis and bin: count, box lo xyz, box hi xyz (ordered ints)
    int child[24];            // left box lo, hi, left centroid lo, hi, then the right side's
    uint32_t wsum[BT / 64];
    uint32_t cnt;
    float bestVal[BT / 64];
    int bestIdx[BT / 64];
};

// exclusive count of the flag over the workgroup's threads, and its total
template <int T>
__device__ __forceinline__ uint32_t flagScan(bool f, Shared& S, uint32_t& total) {
    const uint64_t m = __ballot(f);
    const int lane = threadIdx.x & 63;
    const uint32_t before = __popcll(m & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
    if (T == 64) {
        total = __popcll(m);
        return before;
    }
    const int w = threadIdx.x >> 6;
    if (lane == 0) S.wsum[w] = __popcll(m);
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    for (int q = 0; q < T / 64; ++q) {
        if (q < w) base += S.wsum[q];
        total += S.wsum[q];
    }
    __syncthreads();
    return base + before;
}

// child bounds of the references j in [0, num) by side into S.child (min / max on what is there)
template <int T, class Side>
__device__ __forceinline__ void growChildren(const Params& P, uint32_t start, uint32_t num, Shared& S, Side left) {
    float b[24];
    for (int k = 0; k < 24; ++k) b[k] = ((k / 3) & 1) ? -FLT_MAX : FLT_MAX;
    for (uint32_t j = threadIdx.x; j < num; j += T) {
        const uint32_t id = P.refs[start + j];
        const float4 lo = P.lo[id], hi = P.hi[id], c = P.cen[id];
        const bool L = left(j, c);
        const float v[12] = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, c.x, c.y, c.z, c.x, c.y, c.z};
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const bool isMax = (k / 3) & 1;
            const float l = isMax ? fmaxf(b[k], v[k]) : fminf(b[k], v[k]);
            const float r = isMax ? fmaxf(b[12 + k], v[k]) : fminf(b[12 + k], v[k]);
            b[k] = L ? l : b[k];
            b[12 + k] = L ? b[12 + k] : r;
        }
    }
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        const bool isMax = (k / 3) & 1;
        float x = b[k];
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(x, off);
            x = isMax ? fmaxf(x, o) : fminf(x, o);
        }
        if ((threadIdx.x & 63) == 0) {
            if (isMax) atomicMax(&S.child[k], oi(x));
            else atomicMin(&S.child[k], oi(x));
        }
    }
}

// Splits request nd (num >= 2): writes its record and the instance records of single-reference
// children, returns the child requests.  Every thread of the workgroup calls it and gets the same
// L and R.
template <int T>
__device__ void splitNode(const Params& P, const Req& nd, Shared& S, Req& L, Req& R) {
    const int tid = threadIdx.x;
    const uint32_t start = nd.start, num = nd.num, nb = P.nb;
    const float ce[3] = {nd.cb[3] - nd.cb[0], nd.cb[4] - nd.cb[1], nd.cb[5] - nd.cb[2]};
    for (int k = tid; k < 24; k += T) S.child[k] = oi(((k / 3) & 1) ? -FLT_MAX : FLT_MAX);
    if (tid == 0) S.cnt = 0;
    // split axis and plane: FindSahSplit (bvh.cpp:253-361), else the centroid box's largest axis
    int axis = -1;
    float border = 0.0f;
    if (P.sahOn && !(ce[0] * ce[0] + ce[1] * ce[1] + ce[2] * ce[2] == 0.f)) {
        for (uint32_t k = tid; k < 3 * nb; k += T) {
            S.bins[7 * k] = 0;
            for (int a = 0; a < 3; ++a) {
                S.bins[7 * k + 1 + a] = oi(FLT_MAX);
                S.bins[7 * k + 4 + a] = oi(-FLT_MAX);
            }
        }
        __syncthreads();
        float invr[3];
        for (int a = 0; a < 3; ++a) invr[a] = ce[a] == 0.f ? 0.0f : fdiv(1.f, ce[a]);
        const float nbf = (float)nb, top = (float)(nb - 1);
        for (uint32_t j = tid; j < num; j += T) {
            const uint32_t id = P.refs[start + j];
            const float4 lo = P.lo[id], hi = P.hi[id], c = P.cen[id];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (ce[a] == 0.f) continue;
                const float x = nbf * ((ax3(c, a) - nd.cb[a]) * invr[a]);
                int bi = (int)(top < x ? top : x);
                bi = min(max(bi, 0), (int)nb - 1);
                int* B = &S.bins[7 * (a * nb + bi)];
                atomicAdd(&B[0], 1);
                atomicMin(&B[1], oi(lo.x));
                atomicMin(&B[2], oi(lo.y));
                atomicMin(&B[3], oi(lo.z));
                atomicMax(&B[4], oi(hi.x));
                atomicMax(&B[5], oi(hi.y));
                atomicMax(&B[6], oi(hi.z));
            }
        }
        __syncthreads();
        // candidate t = axis * (nb - 1) + i prices the split after bin i; ascending t is the
        // host's loop order, so the lowest t among equal minima is its strict-< winner
        const float invarea = fdiv(1.f, area6(nd.b));
        float bs = INFINITY;
        int bt = 0x7fffffff;
        for (uint32_t t = tid; t < 3 * (nb - 1); t += T) {
            const uint32_t a = t / (nb - 1), i = t % (nb - 1);
            if (ce[a] == 0.f) continue;
            float lb[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
            float rb[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
            int lc = 0;
            for (uint32_t k = 0; k <= i; ++k) {
                const int* B = &S.bins[7 * (a * nb + k)];
                lc += B[0];
                for (int q = 0; q < 3; ++q) {
                    lb[q] = fminf(lb[q], of(B[1 + q]));
                    lb[3 + q] = fmaxf(lb[3 + q], of(B[4 + q]));
                }
            }
            for (uint32_t k = i + 1; k < nb; ++k) {
                const int* B = &S.bins[7 * (a * nb + k)];
                for (int q = 0; q < 3; ++q) {
                    rb[q] = fminf(rb[q], of(B[1 + q]));
                    rb[3 + q] = fmaxf(rb[3 + q], of(B[4 + q]));
                }
            }
            const int rc = (int)num - lc;
            const float price = P.cost + ((float)lc * area6(lb) + (float)rc * area6(rb)) * invarea;
            if (price < FLT_MAX && price < bs) {
                bs = price;
                bt = (int)t;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(bs, off);
            const int ot = __shfl_xor(bt, off);
            if (os < bs || (os == bs && ot < bt)) {
                bs = os;
                bt = ot;
            }
        }
        if (T > 64) {
            if ((tid & 63) == 0) {
                S.bestVal[tid >> 6] = bs;
                S.bestIdx[tid >> 6] = bt;
            }
            __syncthreads();
            bs = S.bestVal[0];
            bt = S.bestIdx[0];
            for (int q = 1; q < T / 64; ++q) {
                const float os = S.bestVal[q];
                const int ot = S.bestIdx[q];
                if (os < bs || (os == bs && ot < bt)) {
                    bs = os;
                    bt = ot;
                }
            }
        }
        if (bt != 0x7fffffff) {
            const int a = bt / (int)(nb - 1), i = bt % (int)(nb - 1);
            const float split = nd.cb[a] + (float)(i + 1) * fdiv(ce[a], nbf);
            if (!(split != split)) {
                axis = a;
                border = split;
            }
        }
    }
    if (axis < 0) {   // bbox::maxdim (bbox.h:191-203) and the centre of that axis
        const float x = ce[0], y = ce[1], z = ce[2];
        axis = (x >= y && x >= z) ? 0 : (y >= x && y >= z) ? 1 : (z >= x && z >= y) ? 2 : 0;
        border = 0.5f * (nd.cb[3 + axis] + nd.cb[axis]);
    }
    __syncthreads();   // S.child / S.cnt are initialised
    const bool near2far = (num + start) & 1u;
    const int A = axis;
    const float bd = border;
    auto goesLeft = [=](const float4& c) { return near2far ? ax3(c, A) < bd : ax3(c, A) >= bd; };
    uint32_t nl = 0;
    if (ce[axis] > 0.f) {
        // the partition's boxes: every reference grows the side its predicate names
        uint32_t mine = 0;
        for (uint32_t j = tid; j < num; j += T) mine += goesLeft(P.cen[P.refs[start + j]]) ? 1u : 0u;
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
        if ((tid & 63) == 0) atomicAdd(&S.cnt, mine);
        growChildren<T>(P, start, num, S, [=](uint32_t, const float4& c) { return goesLeft(c); });
        __syncthreads();
        nl = S.cnt;
        if (nl > 0 && nl < num) {
            // misplaced lefts (positions >= nl), numbered from the end
            uint32_t run = 0;
            for (uint32_t r0 = 0; r0 < num - nl; r0 += T) {
                const uint32_t r = r0 + tid;
                const bool in = r < num - nl;
                const uint32_t j = num - 1 - (in ? r : 0);
                const bool Lf = in && goesLeft(P.cen[P.refs[start + j]]);
                uint32_t total;
                const uint32_t k = run + flagScan<T>(Lf, S, total);
                if (Lf) P.slots[start + k] = j;
                run += total;
            }
            __syncthreads();
            // misplaced rights (positions < nl) swap with them in order
            run = 0;
            for (uint32_t j0 = 0; j0 < nl; j0 += T) {
                const uint32_t j = j0 + tid;
                const bool in = j < nl;
                const uint32_t id = in ? P.refs[start + j] : 0u;
                const bool Lf = in && goesLeft(P.cen[id]);
                uint32_t total;
                const uint32_t Lb = run + flagScan<T>(Lf, S, total);
                if (in && !Lf) {
                    const uint32_t q = P.slots[start + (j - Lb)];
                    if (q >= nl && q < num) {
                        P.refs[start + j] = P.refs[start + q];
                        P.refs[start + q] = id;
                    }
                }
                run += total;
            }
            __syncthreads();
        }
    }
    if (nl == 0 || nl == num) {
        // median of the current order; the boxes grown above stay (bvh.cpp:198-212)
        nl = num >> 1;
        const uint32_t half = nl;
        growChildren<T>(P, start, num, S, [=](uint32_t j, const float4&) { return j < half; });
    }
    __syncthreads();
    for (int k = 0; k < 6; ++k) {
        L.b[k] = of(S.child[k]);
        L.cb[k] = of(S.child[6 + k]);
        R.b[k] = of(S.child[12 + k]);
        R.cb[k] = of(S.child[18 + k]);
    }
    L.start = start;
    L.num = nl;
    L.index = nd.index + 1;
    R.start = start + nl;
    R.num = num - nl;
    R.index = nd.index + 2 * nl;
    L.level = R.level = nd.level + 1;
    if (tid == 0) {
        float4* o = &P.nodes[4 * (size_t)nd.index];
        o[0] = make_float4(L.b[0], L.b[3], L.b[1], L.b[4]);
        o[1] = make_float4(R.b[0], R.b[3], R.b[1], R.b[4]);
        o[2] = make_float4(L.b[2], L.b[5], R.b[2], R.b[5]);
        o[3] = make_float4(__int_as_float((int)L.index), __int_as_float((int)R.index), 0.0f, 0.0f);
        if (L.num == 1) writeInstance(P, L.index, P.refs[L.start]);
        if (R.num == 1) writeInstance(P, R.index, P.refs[R.start]);
    }
    __syncthreads();   // S is reused by the next call
}

// a level of large requests: one workgroup each
__global__ __launch_bounds__(BT) void k_big(Params P, const Req* __restrict__ cur, Req* __restrict__ next) {
    __shared__ Shared S;
    const Req nd = cur[blockIdx.x];
    Req c[2];
    splitNode<BT>(P, nd, S, c[0], c[1]);
    if (threadIdx.x != 0) return;
    atomicMax(&P.ctr->height, nd.level + 1);
    for (int k = 0; k < 2; ++k) {
        if (c[k].num < 2) continue;
        if (c[k].num > (uint32_t)SMALL) {
            const uint32_t slot = atomicAdd(&P.ctr->big, 1u);
            if (slot >= P.capBig) atomicOr(&P.ctr->error, 1u);
            else next[slot] = c[k];
        } else {
            const uint32_t slot = atomicAdd(&P.ctr->small, 1u);
            if (slot >= P.capSmall) atomicOr(&P.ctr->error, 2u);
            else P.small[slot] = c[k];
        }
    }
}

// one wave finishes a request of at most SMALL references
__global__ __launch_bounds__(64) void k_small(Params P) {
    __shared__ Shared S;
    __shared__ Req stack[SMALL_STACK];
    int sp = 1;
    if (threadIdx.x == 0) stack[0] = P.small[blockIdx.x];
    __syncthreads();
    uint32_t height = 0;
    while (sp > 0) {
        const Req nd = stack[--sp];
        __syncthreads();
        Req L, R;
        splitNode<64>(P, nd, S, L, R);
        height = max(height, nd.level + 1);
        // the larger child first, so the smaller one is split next
        const bool leftFirst = L.num >= R.num;
        const Req& a = leftFirst ? L : R;
        const Req& b = leftFirst ? R : L;
        const int push = (a.num > 1 ? 1 : 0) + (b.num > 1 ? 1 : 0);
        if (sp + push > SMALL_STACK) {   // not reached: depth O(log SMALL)
            if (threadIdx.x == 0) atomicOr(&P.ctr->error, 4u);
            break;
        }
        if (threadIdx.x == 0) {
            int q = sp;
            if (a.num > 1) stack[q++] = a;
            if (b.num > 1) stack[q++] = b;
        }
        sp += push;
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(&P.ctr->height, height);
}

}  // namespace

namespace mcrt {

struct TopBuildDev {
    Params P{};
    char* blob = nullptr;
    int maxBottom = 0;
};

hipError_t top_build_create(const Bvh2lTop& top, TopBuildDev** out) {
    *out = nullptr;
    const size_t n = top.world.size();
    if (n == 0 || n > 0x3fffffffull || top.bins < 2 || top.bins > MAXB) return hipErrorInvalidValue;
    auto* d = new TopBuildDev();
    const size_t numMeshes = top.meshBase.size();
    const uint32_t capBig = (uint32_t)(n / SMALL + 2), capSmall = (uint32_t)(n / 2 + 2);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    const size_t oTop = take(sizeof(TopEnt) * n), oBox = take(sizeof(float) * 6 * numMeshes);
    const size_t oLo = take(sizeof(float4) * n), oHi = take(sizeof(float4) * n), oCen = take(sizeof(float4) * n);
    const size_t oRefs = take(sizeof(uint32_t) * n), oSlots = take(sizeof(uint32_t) * n);
    const size_t oBigA = take(sizeof(Req) * capBig), oBigB = take(sizeof(Req) * capBig);
    const size_t oSmall = take(sizeof(Req) * capSmall), oCtr = take(sizeof(Counters));
    hipError_t e = hipMalloc((void**)&d->blob, off);
    if (e != hipSuccess) {
        delete d;
        return e;
    }
    std::vector<TopEnt> ents(n);
    for (size_t i = 0; i < n; ++i)
        ents[i] = TopEnt{top.world[i], (int32_t)top.meshBase[top.meshOf[i]], top.meshOf[i], 0};
    e = hipMemcpy(d->blob + oTop, ents.data(), sizeof(TopEnt) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(d->blob + oBox, top.meshBox.data(), sizeof(float) * 6 * numMeshes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d->blob);
        delete d;
        return e;
    }
    Params& P = d->P;
    P.top = (const TopEnt*)(d->blob + oTop);
    P.meshBox = (const float*)(d->blob + oBox);
    P.lo = (float4*)(d->blob + oLo);
    P.hi = (float4*)(d->blob + oHi);
    P.cen = (float4*)(d->blob + oCen);
    P.refs = (uint32_t*)(d->blob + oRefs);
    P.slots = (uint32_t*)(d->blob + oSlots);
    P.bigA = (Req*)(d->blob + oBigA);
    P.bigB = (Req*)(d->blob + oBigB);
    P.small = (Req*)(d->blob + oSmall);
    P.ctr = (Counters*)(d->blob + oCtr);
    P.capBig = capBig;
    P.capSmall = capSmall;
    P.n = (uint32_t)n;
    P.nb = (uint32_t)top.bins;
    P.cost = top.cost;
    P.sahOn = top.sah ? 1 : 0;
    d->maxBottom = top.maxBottom;
    *out = d;
    return hipSuccess;
}

void top_build_destroy(TopBuildDev* d) {
    if (!d) return;
    if (d->blob) (void)hipFree(d->blob);
    delete d;
}

hipError_t top_build_run(TopBuildDev* d, const mcrt_shape* dShapes, const mcrt_mat4* dWorldToLocal, float4* nodes,
                         hipStream_t st, int* depth, float* topBox, const char** why) {
    *why = nullptr;
    Params P = d->P;
    P.shapes = dShapes;
    P.w2l = dWorldToLocal;
    P.nodes = nodes;
    Counters hc{};
    for (int k = 0; k < 12; ++k) hc.root[k] = ((k / 3) & 1) ? (int)0x80000000 : 0x7fffffff;
    hipError_t e = hipMemcpyAsync(P.ctr, &hc, sizeof(Counters), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_boxes, dim3((P.n + 255) / 256), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_root, dim3(1), dim3(1), 0, st, P);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t numBig = P.n > (uint32_t)SMALL ? 1u : 0u;
    int levels = 0;
    while (numBig > 0) {
        if (++levels > MAX_LEVELS) {
            *why = "device top-level build: too many levels of large requests";
            (void)hipStreamSynchronize(st);
            return hipErrorNotSupported;
        }
        if ((e = hipMemsetAsync(&P.ctr->big, 0, sizeof(uint32_t), st)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_big, dim3(numBig), dim3(BT), 0, st, P, P.bigA, P.bigB);
        if ((e = hipMemcpyAsync(&hc, P.ctr, sizeof(Counters), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        if (hc.error) {
            *why = "device top-level build: capacity exceeded";
            return hipErrorNotSupported;
        }
        numBig = hc.big;
        std::swap(P.bigA, P.bigB);
    }
    const uint32_t numSmall = P.n > (uint32_t)SMALL ? hc.small : (P.n > 1 ? 1u : 0u);
    if (numSmall > 0) hipLaunchKernelGGL(k_small, dim3(numSmall), dim3(64), 0, st, P);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&hc, P.ctr, sizeof(Counters), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (hc.error) {
        *why = "device top-level build: stack or capacity exceeded";
        return hipErrorNotSupported;
    }
    *depth = (int)hc.height + d->maxBottom + 1;   // + the return marker
    for (int k = 0; k < 6; ++k) {
        const int i = hc.root[k];
        const int bits = i >= 0 ? i : i ^ 0x7fffffff;
        std::memcpy(&topBox[k], &bits, 4);
    }
    return hipSuccess;
}

}  // namespace mcrt
