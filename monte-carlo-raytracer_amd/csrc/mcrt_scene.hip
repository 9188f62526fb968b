// mcrt_scene.hip -- the scene tables: the arrays a scene holds on the device and the host copies the
// builders read, the surface records gathered from them, the previous poses; on top the two kernels,
// below them the entry points that create, replace and move them and the few views the rest of the
// runtime takes (mcrt_host.h).  Only this file names the fields of mcrt_scene_s, apart from `ctx` and
// `accel` (mcrt_accel.cpp's).
//
//   k_surface_records    one 128-B record per triangle of each distinct mesh (SceneArgs::surf)
//   k_pose_snapshot      the shapes' poses into the previous-pose table (mcrt_scene_motion_snapshot)
//
// Built with mcrt_kernels.o's flags, where the kernels came from.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mcrt_host.h"

using mcrt::fail, mcrt::upload;

// Surface records (SceneArgs::surf): record r of mesh m (meshBase[m] <= r < meshBase[m+1]) is
// triangle p = r - meshBase[m] of the (startIdx, startVertex) range, packed as
// (p0 p1.x | p1.yz p2.xy | p2.z uv0 uv1.x | uv1.y uv2 n0.x | n0.yz n1.xy | n1.z n2) + 2 pad float4.
__global__ void k_surface_records(const uint32_t* __restrict__ meshStartIdx, const uint32_t* __restrict__ meshStartVertex,
                                  const uint32_t* __restrict__ meshBase, int numMeshes, uint32_t numRecords,
                                  const uint32_t* __restrict__ indices, const float4* __restrict__ positions,
                                  const float2* __restrict__ uvs, const float4* __restrict__ normals,
                                  float4* __restrict__ surf) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= numRecords) return;
    int lo = 0, hi = numMeshes - 1;   // last mesh with meshBase <= r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (meshBase[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const uint32_t p = r - meshBase[lo];
    const uint32_t* ix = indices + meshStartIdx[lo] + 3 * p;
    const uint32_t sv = meshStartVertex[lo];
    const float4 a = positions[sv + ix[0]], b = positions[sv + ix[1]], c = positions[sv + ix[2]];
    const float2 ta = uvs[sv + ix[0]], tb = uvs[sv + ix[1]], tc = uvs[sv + ix[2]];
    const float4 na = normals[sv + ix[0]], nb = normals[sv + ix[1]], nc = normals[sv + ix[2]];
    float4* R = surf + 8 * (size_t)r;
    R[0] = make_float4(a.x, a.y, a.z, b.x);
    R[1] = make_float4(b.y, b.z, c.x, c.y);
    R[2] = make_float4(c.z, ta.x, ta.y, tb.x);
    R[3] = make_float4(tb.y, tc.x, tc.y, na.x);
    R[4] = make_float4(na.y, na.z, nb.x, nb.y);
    R[5] = make_float4(nb.z, nc.x, nc.y, nc.z);
    R[6] = make_float4(0.f, 0.f, 0.f, 0.f);
    R[7] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// The previous-pose table (mcrt_scene_motion_snapshot): the first 35 words of every mcrt_shape --
// both matrices and the mesh key -- and a zero, one word per thread.
__global__ __launch_bounds__(256) void k_pose_snapshot(const mcrt_shape* __restrict__ shapes, PrevPose* __restrict__ out,
                                                       int n) {
    constexpr int WORDS = (int)(sizeof(PrevPose) / 4), SHAPE_WORDS = (int)(sizeof(mcrt_shape) / 4);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * WORDS) return;
    const int k = i / WORDS, w = i - k * WORDS;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(shapes);
    reinterpret_cast<uint32_t*>(out)[i] = w < WORDS - 1 ? src[(size_t)k * SHAPE_WORDS + w] : 0u;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// The records of the scene's distinct meshes (dSurfMeshes, surfMeshes, surfRecords) from its current
// vertex arrays into dSurf, on st: the build's launch and, in place, every vertex update's.
static void launch_surface_records(mcrt_scene s, hipStream_t st) {
    if (s->surfRecords == 0) return;
    const uint32_t* m = s->dSurfMeshes.get();
    const int nm = (int)s->surfMeshes;
    k_surface_records<<<(s->surfRecords + 255) / 256, 256, 0, st>>>(m, m + nm, m + 2 * nm, nm, s->surfRecords,
                                                                    s->dIndices.get(), s->dPositions.get(),
                                                                    s->dUvs.get(), s->dNormals.get(), s->dSurf.get());
}

// Surface records (SceneArgs::surf): shapes of one mesh -- RTScene's instances -- share one record
// range (mcrt::surface_meshes); the records are gathered on the device from the uploaded
// index/vertex arrays.  Rebuilt when shapes change.
static hipError_t build_surface_records(mcrt_scene s) {
    hipStream_t st = s->ctx->stream;
    std::vector<uint32_t> meshes, shapeBase;
    const uint32_t total = mcrt::surface_meshes(s->shapes.data(), s->shapes.size(), meshes, shapeBase);
    const uint32_t nm = (uint32_t)(meshes.size() / 3);
    hipError_t e = hipStreamSynchronize(st);   // the old records may still be read
    s->dSurf.reset();
    s->dSurfBase.reset();
    s->dSurfMeshes.reset();
    if (nm == 0) meshes.assign(3, 0u);   // never an empty table
    if (e == hipSuccess) e = (hipError_t)s->dSurf.alloc((size_t)std::max(total, 1u) * 8);   // 128 B per record
    if (e == hipSuccess) e = upload(s->dSurfBase, shapeBase.data(), shapeBase.size(), st);
    if (e == hipSuccess) e = upload(s->dSurfMeshes, meshes.data(), meshes.size(), st);
    s->surfMeshes = nm;
    s->surfRecords = total;
    if (e == hipSuccess && nm > 0) {
        launch_surface_records(s, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) s->surfMeshes = s->surfRecords = 0;
    return e;
}

// Replaces a scene array once the context stream has finished with the old one.
template <class T>
static mcrt_status replace_array(mcrt_scene s, DevBuf<T>& dst, const T* src, size_t count) {
    mcrt_ctx ctx = s->ctx;
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    dst.reset();
    if (count) {
        HIPCHK(ctx, dst.alloc(count));
        HIPCHK(ctx, hipMemcpy(dst.get(), src, sizeof(T) * count, hipMemcpyHostToDevice));
    }
    return MCRT_OK;
}

// The scene's shapes and the counts of its other tables, as check_scene_tables takes them: what
// every check starts from.  The caller puts in the table it brings, with its count.
static mcrt::SceneTables current_tables(mcrt_scene s) {
    mcrt::SceneTables t;
    t.shapes = s->shapes.data();
    t.numShapes = s->shapes.size();
    t.numMaterials = s->numMaterials;
    t.numLights = s->numLights;
    t.numTextures = s->numTextures;
    return t;
}

// An update's tables (current_tables with the replaced table put in) checked.  Nothing is changed.
static mcrt_status check_update(mcrt_scene s, const mcrt::SceneTables& t) {
    uint32_t at = 0, slot = 0;
    if (const int bad = mcrt::check_scene_tables(t, &at, &slot))
        return fail(s->ctx, MCRT_ERROR_INVALID_ARG, mcrt::scene_tables_message(bad, at, slot));
    return MCRT_OK;
}

mcrt_status mcrt::check_updated_shapes(mcrt_scene s, const mcrt_shape* sh, uint32_t n) {
    mcrt::SceneTables t = current_tables(s);   // the new shapes against the current counts
    t.shapes = sh;
    t.numShapes = n;
    const mcrt_status st = check_update(s, t);
    if (st != MCRT_OK) return st;
    // the index ranges are the topology's and stay; a moved startVertex moves the vertices a shape names
    for (uint32_t i = 0; i < n; ++i) {
        if (sh[i].startVertex == s->shapes[i].startVertex) continue;
        if (mcrt::check_shape_ranges(&sh[i], 1, s->indices.data(), s->indices.size(), s->positions.size(), nullptr))
            return fail(s->ctx, MCRT_ERROR_INVALID_ARG, mcrt::scene_tables_message(mcrt::TABLE_VERTEX_INDEX, i, 0));
    }
    return MCRT_OK;
}

const mcrt_float4* mcrt::host_positions(mcrt_scene s) {
    if (s->positionsStale) {   // the update that left it stale ended synchronised
        hipSetDevice(s->ctx->device);
        if (hipMemcpy(s->positions.data(), s->dPositions.get(), sizeof(float4) * s->positions.size(),
                      hipMemcpyDeviceToHost) != hipSuccess)
            return nullptr;
        s->positionsStale = false;
    }
    return s->positions.data();
}

mcrt::SceneGeometry mcrt::scene_geometry(mcrt_scene s) {
    return {s->shapes.data(), s->shapes.size(), s->indices.data(), s->dShapes.get(), s->dIndices.get(),
            s->dPositions.get()};
}

mcrt_status mcrt::store_shapes(mcrt_scene s, const mcrt_shape* sh, uint32_t n) {
    HIPCHK(s->ctx, hipMemcpy(s->dShapes.get(), sh, sizeof(mcrt_shape) * n, hipMemcpyHostToDevice));
    s->shapes.assign(sh, sh + n);
    return MCRT_OK;
}

int mcrt::scene_num_lights(mcrt_scene s) { return (int)s->numLights; }
bool mcrt::scene_has_sobol(mcrt_scene s) { return s->hasSobol; }
const PrevPose* mcrt::scene_prev_poses(mcrt_scene s) { return s->dPrevPose.get(); }

SceneArgs mcrt::scene_args(mcrt_scene s) {
    SceneArgs a;
    a.shapes = s->dShapes.get();
    a.indices = s->dIndices.get();
    a.positions = s->dPositions.get();
    a.uvs = s->dUvs.get();
    a.normals = s->dNormals.get();
    a.textures = s->dTextures.get();
    a.texData = s->dTexData.get();
    a.sobol = s->dSobol.get();
    a.lights = s->dLights.get();
    a.materials = s->dMaterials.get();
    a.nodes = mcrt::accel_nodes(s);
    a.surf = s->dSurf.get();
    a.surfBase = s->dSurfBase.get();
    a.numLights = (int)s->numLights;
    return a;
}

// The two vertex updates: `device` tells where positions / normals live.  Everything is checked
// before anything is touched; the copies and the surface records' relaunch run on the context
// stream after every launch already enqueued, and the call ends synchronised.
static mcrt_status update_vertices(mcrt_scene s, uint32_t first, uint32_t count, const void* positions,
                                   const void* normals, bool device) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    mcrt_ctx ctx = s->ctx;
    if (!positions) return fail(ctx, MCRT_ERROR_INVALID_ARG, "positions is NULL");
    const size_t nv = s->positions.size();
    if ((size_t)first > nv || (size_t)count > nv - first)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "vertex range [" + std::to_string(first) + ", " +
                                                     std::to_string((uint64_t)first + count) + ") is outside the scene's " +
                                                     std::to_string(nv) + " vertices");
    if (count == 0) return MCRT_OK;
    hipSetDevice(ctx->device);
    // as mcrt_accel_update_transforms: frames in flight finish on the old vertices
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipDeviceSynchronize());
    hipStream_t st = ctx->stream;
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t bytes = sizeof(float4) * (size_t)count;
    HIPCHK(ctx, hipMemcpyAsync(s->dPositions.get() + first, positions, bytes, kind, st));
    if (normals) HIPCHK(ctx, hipMemcpyAsync(s->dNormals.get() + first, normals, bytes, kind, st));
    if (device) {
        s->positionsStale = true;
    } else if (!s->positionsStale) {   // a stale copy is downloaded whole later, this range with it
        std::memcpy(s->positions.data() + first, positions, bytes);
    }
    if (s->surfMeshes > 0) {   // in place: the meshes, their bases and the records' count are the topology's
        launch_surface_records(s, st);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipDeviceSynchronize());
    return MCRT_OK;
}

extern "C" {

MCRT_API mcrt_status mcrt_scene_create(mcrt_ctx ctx, const mcrt_scene_desc* d, mcrt_scene* out) {
    if (!ctx || !d || !out) return fail(ctx, MCRT_ERROR_INVALID_ARG, "NULL argument");
    if (d->num_shapes == 0 || !d->shapes) return fail(ctx, MCRT_ERROR_INVALID_ARG, "scene has no shapes");
    if (!d->indices || !d->positions || !d->uvs || !d->normals)
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "indices/positions/uvs/normals are required");
    if ((d->num_materials && !d->materials) || (d->num_lights && !d->lights) || (d->num_textures && !d->textures))
        return fail(ctx, MCRT_ERROR_INVALID_ARG, "a table with a non-zero count is NULL");
    auto s = std::make_unique<mcrt_scene_s>();   // the counts first: the tables are checked against them
    s->ctx = ctx;
    s->numLights = d->num_lights;
    s->numMaterials = d->num_materials;
    s->numTextures = d->num_textures;
    s->hasSobol = d->sobol_matrices != nullptr && d->num_sobol_words >= 1024u * 52u;
    {
        mcrt::SceneTables t = current_tables(s.get());   // every table is the description's
        t.shapes = d->shapes;
        t.numShapes = d->num_shapes;
        t.materials = d->materials;
        t.lights = d->lights;
        t.indices = d->indices;
        t.numIndices = d->num_indices;
        t.numVertices = d->num_vertices;
        const mcrt_status st = check_update(s.get(), t);
        if (st != MCRT_OK) return st;
    }
    for (uint32_t i = 0; i < d->num_textures; ++i) {
        const mcrt_texture_desc& t = d->textures[i];
        if (t.width == 0 || t.height == 0 || (uint64_t)t.memOffset + 4ull * t.width * t.height > d->tex_data_bytes)
            return fail(ctx, MCRT_ERROR_INVALID_ARG, "texture " + std::to_string(i) + " is out of the texel buffer");
    }
    hipSetDevice(ctx->device);
    s->shapes.assign(d->shapes, d->shapes + d->num_shapes);
    s->indices.assign(d->indices, d->indices + d->num_indices);
    s->positions.assign(d->positions, d->positions + d->num_vertices);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
#define UP(dst, src, cnt) if (e == hipSuccess) e = upload(s->dst, src, cnt, st)
    UP(dShapes, d->shapes, d->num_shapes);
    UP(dIndices, d->indices, d->num_indices);
    UP(dPositions, d->positions, d->num_vertices);
    UP(dUvs, d->uvs, d->num_vertices);
    UP(dNormals, d->normals, d->num_vertices);
    UP(dTextures, d->textures, d->num_textures);
    UP(dTexData, d->tex_data, d->tex_data_bytes);
    UP(dSobol, d->sobol_matrices, d->num_sobol_words);
    UP(dLights, d->lights, d->num_lights);
    UP(dMaterials, d->materials, d->num_materials);
#undef UP
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = build_surface_records(s.get());
    if (e != hipSuccess)
        return fail(ctx, e == hipErrorOutOfMemory ? MCRT_ERROR_OUT_OF_MEMORY : MCRT_ERROR_DEVICE,
                    std::string("scene upload: ") + hipGetErrorString(e));
    *out = s.release();
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_scene_destroy(mcrt_scene s) {
    if (!s) return MCRT_OK;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    delete s;
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_scene_update_lights(mcrt_scene s, const mcrt_light* lights, uint32_t n) {
    if (!s || (n && !lights)) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "invalid lights");
    mcrt::SceneTables t = current_tables(s);   // the new lights against the current shapes
    t.lights = lights;
    t.numLights = n;
    mcrt_status st = check_update(s, t);
    if (st != MCRT_OK) return st;
    st = replace_array(s, s->dLights, lights, n);
    if (st == MCRT_OK) s->numLights = n;
    return st;
}

MCRT_API mcrt_status mcrt_scene_update_materials(mcrt_scene s, const mcrt_material* m, uint32_t n) {
    if (!s || (n && !m)) return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "invalid materials");
    mcrt::SceneTables t = current_tables(s);   // the new materials against the current shapes and texture count
    t.materials = m;
    t.numMaterials = n;
    mcrt_status st = check_update(s, t);
    if (st != MCRT_OK) return st;
    st = replace_array(s, s->dMaterials, m, n);
    if (st == MCRT_OK) s->numMaterials = n;
    return st;
}

MCRT_API mcrt_status mcrt_scene_update_shapes(mcrt_scene s, const mcrt_shape* sh, uint32_t n) {
    if (!s || !sh || n != s->shapes.size())
        return fail(s ? s->ctx : nullptr, MCRT_ERROR_INVALID_ARG, "shape count must not change");
    for (uint32_t i = 0; i < n; ++i)
        if (sh[i].startIdx != s->shapes[i].startIdx || sh[i].numTriangles != s->shapes[i].numTriangles)
            return fail(s->ctx, MCRT_ERROR_INVALID_ARG, "shape topology must not change");
    mcrt_status st = mcrt::check_updated_shapes(s, sh, n);
    if (st != MCRT_OK) return st;
    st = replace_array(s, s->dShapes, sh, n);
    if (st != MCRT_OK) return st;
    s->shapes.assign(sh, sh + n);   // after the last check: a rejected call leaves the scene as it was
    HIPCHK(s->ctx, build_surface_records(s));   // startVertex may have moved
    return MCRT_OK;
}

MCRT_API mcrt_status mcrt_scene_update_vertices(mcrt_scene s, uint32_t first, uint32_t count, const mcrt_float4* positions,
                                                const mcrt_float4* normals) {
    return update_vertices(s, first, count, positions, normals, false);
}

MCRT_API mcrt_status mcrt_scene_update_vertices_device(mcrt_scene s, uint32_t first, uint32_t count,
                                                       const void* d_positions, const void* d_normals) {
    return update_vertices(s, first, count, d_positions, d_normals, true);
}

MCRT_API mcrt_status mcrt_scene_motion_snapshot(mcrt_scene s) {
    if (!s) return fail(nullptr, MCRT_ERROR_INVALID_ARG, "scene is NULL");
    mcrt_ctx ctx = s->ctx;
    const size_t n = s->shapes.size();
    if (n == 0 || !s->dShapes) return fail(ctx, MCRT_ERROR_INVALID_ARG, "scene has no shapes");
    hipSetDevice(ctx->device);
    if (!s->dPrevPose) HIPCHK(ctx, s->dPrevPose.alloc(n));
    const int words = (int)n * (int)(sizeof(PrevPose) / 4);
    hipLaunchKernelGGL(k_pose_snapshot, dim3((words + 255) / 256), dim3(256), 0, ctx->stream, s->dShapes.get(),
                       s->dPrevPose.get(), (int)n);
    HIPCHK(ctx, hipGetLastError());
    return MCRT_OK;
}

}  // extern "C"
