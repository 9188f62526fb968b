// mcrt_accel_host.cpp -- the acceleration structure's host layer: the parsed build options, the
// input checks (the scene tables' among them, and the surface records' mesh ranges), the world-space
// triangles and the one host build that mcrt_accel_build (mcrt_accel.cpp) uploads and
// mcrt_accel_build_host_records returns.  No device, no context: it links into host-only programs
// (tests/asan) with mcrt_bvh.cpp and mcrt_bvh2l.cpp.
#include <algorithm>
#include <cstring>
#include <map>
#include <thread>
#include <tuple>

#include "mcrt_internal.h"

namespace mcrt {

static mcrt_status invalid(const std::string& msg) {
    set_last_error(msg);
    return MCRT_ERROR_INVALID_ARG;
}

bool make_accel_plan(const mcrt_accel_opts* opts, const mcrt_shape* shapes, std::size_t n, AccelPlan& plan) {
    plan = AccelPlan();
    if (opts) {
        plan.cost = opts->traversal_cost;
        plan.bins = opts->num_bins;
        plan.sah = opts->use_sah != 0;
        plan.deviceBuild = opts->device_build;
        plan.worldToLocal = opts->world_to_local;
    }
    if (plan.bins < 2 || plan.bins > 4096) {
        set_last_error("num_bins out of range");
        return false;
    }
    plan.twoLevel = (opts && opts->force_2level) || (!(opts && opts->force_flat) && shapes_are_instanced(shapes, n));
    return true;
}

int check_shape_ranges(const mcrt_shape* shapes, std::size_t n, const uint32_t* indices, uint64_t numIndices,
                       uint64_t numVertices, uint32_t* badShape) {
    uint32_t none;
    uint32_t& bad = badShape ? *badShape : none;
    for (bad = 0; bad < n; ++bad)   // every index range before the first index is read
        if ((uint64_t)shapes[bad].startIdx + 3ull * shapes[bad].numTriangles > numIndices) return 1;
    for (bad = 0; bad < n; ++bad) {
        const mcrt_shape& sh = shapes[bad];
        for (uint64_t k = 0; k < 3ull * sh.numTriangles; ++k)
            if ((uint64_t)sh.startVertex + indices[sh.startIdx + k] >= numVertices) return 2;
    }
    return 0;
}

int check_scene_tables(const SceneTables& t, uint32_t* entry, uint32_t* slot) {
    uint32_t none;
    uint32_t& at = entry ? *entry : none;
    uint32_t& sl = slot ? *slot : none;
    at = sl = 0;
    auto outside = [](int32_t id, std::size_t n) { return id < -1 || (id >= 0 && (std::size_t)id >= n); };
    if (t.indices)
        if (const int bad = check_shape_ranges(t.shapes, t.numShapes, t.indices, t.numIndices, t.numVertices, &at)) return bad;
    for (at = 0; at < t.numShapes; ++at) {
        if (outside(t.shapes[at].materialId, t.numMaterials)) return TABLE_MATERIAL_ID;
        if (outside(t.shapes[at].lightID, t.numLights)) return TABLE_LIGHT_ID;
    }
    for (at = 0; t.materials && at < t.numMaterials; ++at) {   // whatever the type: normal mapping runs before the type test
        const mcrt_material& m = t.materials[at];
        const int32_t ids[8] = {m.uber_normalMapId, m.uber_diffuseTexId, m.uber_glossyTexId, m.uber_specReflectionTexId,
                                m.uber_transmissionTexId, m.uber_opacityTexId, m.uber_roughnessTexId, m.uber_iorTexId};
        for (sl = 0; sl < 8; ++sl)
            if (outside(ids[sl], t.numTextures)) return TABLE_TEXTURE_ID;
    }
    sl = 0;
    for (at = 0; t.lights && at < t.numLights; ++at) {
        const mcrt_light& L = t.lights[at];
        if (L.type == MCRT_TRIANGLE_MESH_AREA_LIGHT &&
            (L.shapeId < 0 || (std::size_t)L.shapeId >= t.numShapes || t.shapes[L.shapeId].numTriangles == 0))
            return TABLE_MESH_LIGHT;
    }
    at = 0;
    return TABLE_OK;
}

std::string scene_tables_message(int rule, uint32_t entry, uint32_t slot) {
    static const char* const slots[8] = {"normal map", "diffuse", "glossy", "specular reflection",
                                         "transmission", "opacity", "roughness", "ior"};
    const std::string e = std::to_string(entry);
    switch (rule) {
    case TABLE_OK: return "";
    case TABLE_INDEX_RANGE: return "shape " + e + " indexes past the index array";
    case TABLE_VERTEX_INDEX: return "vertex index out of range in shape " + e;
    case TABLE_MATERIAL_ID: return "shape " + e + " has an invalid material id";
    case TABLE_LIGHT_ID: return "shape " + e + " has an invalid light id";
    case TABLE_TEXTURE_ID: return "material " + e + " has an invalid " + slots[slot & 7] + " texture id";
    case TABLE_MESH_LIGHT: return "mesh light " + e + " has an invalid shape";
    }
    return "invalid scene tables";
}

uint32_t surface_meshes(const mcrt_shape* shapes, std::size_t n, std::vector<uint32_t>& meshes,
                        std::vector<uint32_t>& shapeBase) {
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> meshOf;
    std::vector<uint32_t> mStart, mVert, mBase;
    shapeBase.resize(n);
    uint32_t total = 0;
    for (std::size_t i = 0; i < n; ++i) {
        const mcrt_shape& sh = shapes[i];
        auto key = std::make_tuple((uint32_t)sh.startIdx, (uint32_t)sh.startVertex, (uint32_t)sh.numTriangles);
        auto it = meshOf.find(key);
        if (it == meshOf.end()) {
            it = meshOf.emplace(key, total).first;
            if (sh.numTriangles > 0) {
                mStart.push_back(sh.startIdx);
                mVert.push_back(sh.startVertex);
                mBase.push_back(total);
            }
            total += sh.numTriangles;
        }
        shapeBase[i] = it->second;
    }
    meshes = mStart;
    meshes.insert(meshes.end(), mVert.begin(), mVert.end());
    meshes.insert(meshes.end(), mBase.begin(), mBase.end());
    return total;
}

bool same_topology(const mcrt_shape* a, const mcrt_shape* b, std::size_t n, bool twoLevel) {
    for (std::size_t i = 0; i < n; ++i)
        if (a[i].startIdx != b[i].startIdx || a[i].numTriangles != b[i].numTriangles ||
            (twoLevel && a[i].startVertex != b[i].startVertex))
            return false;
    return true;
}

// RR transform_point (RR/include/math/mathutils.h:111-118) for the BVH's world-space triangles
static inline void xformPoint(const mcrt_mat4& m, const mcrt_float4& p, float* o) {
    const mcrt_float4* r[3] = {&m.m0, &m.m1, &m.m2};
    for (int i = 0; i < 3; ++i) {
        float acc = 0.0f;
        acc += r[i]->x * p.x;
        acc += r[i]->y * p.y;
        acc += r[i]->z * p.z;
        acc += r[i]->w * 0.0f;
        o[i] = acc + r[i]->w;
    }
}

// World-space triangles of all shapes in shape order, 9 floats each, with each one's shape and primitive
static void flatten_triangles(const mcrt_shape* shapes, std::size_t n, const uint32_t* indices, const mcrt_float4* positions,
                       std::vector<float>& tri, std::vector<int32_t>& shapeOf, std::vector<int32_t>& primOf) {
    std::size_t total = 0;
    for (std::size_t si = 0; si < n; ++si) total += shapes[si].numTriangles;
    tri.resize(9 * total);
    shapeOf.resize(total);
    primOf.resize(total);
    std::size_t k = 0;
    for (std::size_t si = 0; si < n; ++si) {
        const mcrt_shape& sh = shapes[si];
        for (uint32_t f = 0; f < sh.numTriangles; ++f, ++k) {
            for (int c = 0; c < 3; ++c)
                xformPoint(sh.toWorldTransform, positions[sh.startVertex + indices[sh.startIdx + 3 * f + c]],
                           &tri[9 * k + 3 * c]);
            shapeOf[k] = (int32_t)si;
            primOf[k] = (int32_t)f;
        }
    }
}

void root_record_box(const float* r, float* box) {
    int32_t mark;
    std::memcpy(&mark, &r[12], 4);
    if (mark >= 0) {
        const float lo[3] = {std::min(r[0], r[4]), std::min(r[2], r[6]), std::min(r[8], r[10])};
        const float hi[3] = {std::max(r[1], r[5]), std::max(r[3], r[7]), std::max(r[9], r[11])};
        for (int a = 0; a < 3; ++a) { box[a] = lo[a]; box[3 + a] = hi[a]; }
        return;
    }
    for (int a = 0; a < 3; ++a) {
        const float v0 = r[a], v1 = r[a] + r[4 + a], v2 = r[a] + r[8 + a];
        box[a] = std::min(v0, std::min(v1, v2));
        box[3 + a] = std::max(v0, std::max(v1, v2));
    }
}

mcrt_status build_host_tree(const AccelPlan& plan, const mcrt_shape* shapes, std::size_t n, const uint32_t* indices,
                            const mcrt_float4* positions, HostTree& out) {
    const int threads = (int)std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
    out.twoLevel = plan.twoLevel;
    if (plan.twoLevel) {
        Bvh2lOut b2;
        if (!build_bvh2l(shapes, n, indices, positions, plan.worldToLocal, plan.cost, plan.bins, plan.sah, threads, b2))
            return invalid("two-level BVH build failed");
        out.two = std::move(b2.records);
        out.records = out.two.data();
        out.numNodes = b2.numNodes;
        out.topNodes = b2.topNodes;
        for (std::size_t i = 0; i < n; ++i) out.numTris += shapes[i].numTriangles;
        out.depth = b2.depth;
        out.numMeshes = b2.numMeshes;
        out.numInstances = b2.numInstances;
        std::memcpy(out.box, b2.topBox, sizeof(out.box));
        out.top = std::move(b2.top);
        return MCRT_OK;
    }
    std::vector<float> tri;
    std::vector<int32_t> shapeOf, primOf;
    flatten_triangles(shapes, n, indices, positions, tri, shapeOf, primOf);
    if (shapeOf.empty()) return invalid("scene has no triangles (RR: Commit on empty scene throws)");
    const bool axes3 = plan.deviceBuild == 4;   // the perf tree (3-axis SAH), not the reference's
    if (!build_bvh(tri.data(), shapeOf.data(), primOf.data(), shapeOf.size(), plan.cost, plan.bins, plan.sah, threads,
                   out.flat, axes3))
        return invalid("BVH build failed");
    out.records = out.flat.nodes;
    out.numNodes = out.topNodes = out.flat.numNodes;
    out.numTris = out.flat.numTris;
    out.depth = out.flat.depth;
    out.builder = axes3 ? 4 : 0;
    root_record_box(out.records, out.box);
    return MCRT_OK;
}

static mcrt_status host_records(const mcrt_scene_desc* d, const mcrt_accel_opts* opts, const mcrt_shape* moved,
                                const mcrt_mat4* movedW2l, float* out_records, uint64_t max_records,
                                uint64_t* num_records, int32_t* info) {
    if (!d || !d->shapes || !d->indices || !d->positions || !num_records) return invalid("invalid arguments");
    AccelPlan plan;
    if (!make_accel_plan(opts, d->shapes, d->num_shapes, plan)) return MCRT_ERROR_INVALID_ARG;
    if (moved && !same_topology(moved, d->shapes, d->num_shapes, plan.twoLevel))
        return invalid("shape topology must not change");
    const mcrt_shape* shapes = d->shapes;
    if (moved && !plan.twoLevel) {   // a flat structure is rebuilt: the fresh build of the moved shapes
        shapes = moved;
        make_accel_plan(opts, moved, d->num_shapes, plan);
        plan.worldToLocal = movedW2l;
        moved = nullptr;
    }
    const int bad = check_shape_ranges(shapes, d->num_shapes, d->indices, d->num_indices, d->num_vertices, nullptr);
    if (bad) return invalid(bad == 1 ? "shape indices out of range" : "vertex index out of range");
    HostTree t;
    const mcrt_status st = build_host_tree(plan, shapes, d->num_shapes, d->indices, d->positions, t);
    if (st != MCRT_OK) return st;
    // mcrt_accel_refit_host_records: the refit's top level over the built one, as the host path of
    // mcrt_accel_update_transforms uploads it
    if (moved) build_bvh2l_top(t.top, moved, movedW2l, t.two.data(), &t.depth, t.box);
    *num_records = t.numNodes;
    if (out_records) std::memcpy(out_records, t.records, 64 * std::min<uint64_t>(max_records, t.numNodes));
    const int32_t inf[4] = {t.twoLevel ? 1 : 0, (int32_t)t.topNodes, t.depth, t.numMeshes};
    if (info) std::memcpy(info, inf, sizeof(inf));
    return MCRT_OK;
}

}  // namespace mcrt

extern "C" {

MCRT_API mcrt_status mcrt_accel_build_host_records(const mcrt_scene_desc* d, const mcrt_accel_opts* opts,
                                                   float* out_records, uint64_t max_records, uint64_t* num_records,
                                                   int32_t* info) {
    return mcrt::host_records(d, opts, nullptr, nullptr, out_records, max_records, num_records, info);
}

MCRT_API mcrt_status mcrt_accel_refit_host_records(const mcrt_scene_desc* d, const mcrt_accel_opts* opts,
                                                   const mcrt_shape* moved_shapes, const mcrt_mat4* moved_world_to_local,
                                                   float* out_records, uint64_t max_records, uint64_t* num_records,
                                                   int32_t* info) {
    if (!moved_shapes) {
        mcrt::set_last_error("invalid arguments");
        return MCRT_ERROR_INVALID_ARG;
    }
    return mcrt::host_records(d, opts, moved_shapes, moved_world_to_local, out_records, max_records, num_records, info);
}

}  // extern "C"
