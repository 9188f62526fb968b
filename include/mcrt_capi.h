/*
 * mcrt_capi.h -- C ABI of the MI355X-native Monte-Carlo path-tracing core.
 *
 * This is the drop-in boundary for the reference's hot path
 * (compix/Monte-Carlo-Raytracer).  Every entry point names the reference
 * interface it replaces (paths relative to the reference repo root):
 *
 *   RR  = third_party/RadeonRays/RadeonRays
 *   APP = source/application/PathTracer
 *   KRN = assets/kernels
 *
 * Plain C: opaque handles, plain pointers and sizes, no C++ or torch types.
 * Every call returns an mcrt_status; mcrt_last_error() gives the message
 * (the reference threw std::exception / Calc::Exception and the passes caught
 * them: APP/raytracing/renderPasses/RTPathTracingPass.cpp:89-104).
 *
 * All structs below are byte-identical to the OpenCL device structs of
 * KRN/kernel_data.h (sizes/offsets: SURVEY.md Appendix B), so the scene
 * arrays the reference's RTScene builds (APP/raytracing/scene/RTScene.cpp)
 * can be passed unchanged.
 */
#ifndef MCRT_CAPI_H
#define MCRT_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCRT_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------ */
/* Status codes                                                             */
/* ------------------------------------------------------------------------ */
typedef int mcrt_status;
#define MCRT_OK                   0
#define MCRT_ERROR_INVALID_ARG    1
#define MCRT_ERROR_OUT_OF_MEMORY  2
#define MCRT_ERROR_DEVICE         3
#define MCRT_ERROR_NOT_READY      4  /* e.g. trace before mcrt_accel_build */
#define MCRT_ERROR_NO_DEVICE      5

/* ------------------------------------------------------------------------ */
/* Device-layout value types (OpenCL float3 = 16 B, float2 = 8 B)           */
/* ------------------------------------------------------------------------ */
typedef struct __attribute__((aligned(16))) { float x, y, z, w; } mcrt_float4;
typedef mcrt_float4 mcrt_float3;                      /* OpenCL float3: 16 B */
typedef struct __attribute__((aligned(8))) { float x, y; } mcrt_float2;
typedef struct __attribute__((aligned(16))) { mcrt_float4 m0, m1, m2, m3; } mcrt_mat4; /* row major, KRN/matrix.cl:4-11 */

/* RTShape, KRN/kernel_data.h:36-52 (160 B) */
typedef struct __attribute__((aligned(16))) {
    mcrt_mat4 toWorldTransform;
    mcrt_mat4 toWorldInverseTranspose;
    uint32_t  startIdx;
    uint32_t  startVertex;
    uint32_t  numTriangles;
    int32_t   materialId;   /* -1 = none */
    int32_t   lightID;      /* -1 = not an emitter */
    float     area;
    int32_t   pad[2];
} mcrt_shape;

/* RTMaterial (uber material), KRN/kernel_data.h:87-113 (128 B) */
typedef struct __attribute__((aligned(16))) {
    mcrt_float3 uber_kd;
    mcrt_float3 uber_ks;
    mcrt_float3 uber_kr;
    mcrt_float4 uber_kt;        /* w >= 0.5: glossy, else perfect specular transmission */
    mcrt_float3 uber_opacity;
    mcrt_float2 uber_roughness;
    float       uber_eta;
    int32_t     type;           /* 0 = RT_UBER_MATERIAL */
    int32_t     uber_normalMapId;
    int32_t     uber_diffuseTexId;
    int32_t     uber_glossyTexId;
    int32_t     uber_specReflectionTexId;
    int32_t     uber_transmissionTexId;
    int32_t     uber_opacityTexId;
    int32_t     uber_roughnessTexId;
    int32_t     uber_iorTexId;
} mcrt_material;

/* RTLight, KRN/kernel_data.h:137-152 (80 B) */
#define MCRT_DIRECTIONAL_LIGHT        0
#define MCRT_POINT_LIGHT              1
#define MCRT_DISK_AREA_LIGHT          2
#define MCRT_TRIANGLE_MESH_AREA_LIGHT 3
#define MCRT_LIGHT_FLAG_DELTA_POSITION  (1 << 1)
#define MCRT_LIGHT_FLAG_DELTA_DIRECTION (1 << 2)
#define MCRT_LIGHT_FLAG_AREA            (1 << 3)
typedef struct __attribute__((aligned(16))) {
    mcrt_float3 d;
    mcrt_float3 p;
    mcrt_float3 intensity;
    float   radius;
    float   area;
    float   choicePdf;
    int32_t shapeId;
    int32_t type;
    int32_t flags;
    int32_t pad[2];
} mcrt_light;

/* RTPinholeCamera, KRN/kernel_data.h:246-264 (176 B) */
typedef struct __attribute__((aligned(16))) {
    mcrt_mat4   worldToClip;
    mcrt_float3 r00, r10, r11, r01;   /* corner directions, APP/.../RTPrimaryRaysPass.cpp:96-99 */
    mcrt_float3 pos;
    mcrt_float3 direction;
    uint32_t    width;
    uint32_t    height;
    float       area;
    int32_t     padding;
} mcrt_camera;

/* TextureDesc2D, KRN/kernel_data.h:317-326 (16 B); texels are RGBA8 */
typedef struct {
    uint16_t width, height, numMipLevels, format, wrap, pad;
    uint32_t memOffset;       /* byte offset into tex_data */
} mcrt_texture_desc;

/* RadeonRays ray, RR/src/kernels/CL/common.cl:53-60 and KRN/kernel_data.h:407-417 (48 B) */
typedef struct __attribute__((aligned(16))) {
    mcrt_float4 o;            /* xyz origin, w = max range */
    mcrt_float4 d;            /* xyz direction, w = time (unused) */
    int32_t extra[2];         /* [0] = mask (-1: all shapes), [1] = active flag (0: inactive) */
    int32_t doBackfaceCulling;
    int32_t padding;
} mcrt_ray;

/* RadeonRays Intersection, RR/src/kernels/CL/common.cl:63-70 (32 B) */
typedef struct __attribute__((aligned(16))) {
    int32_t shapeid;          /* -1 on miss */
    int32_t primid;           /* -1 on miss */
    int32_t padding[2];
    mcrt_float4 uvwt;         /* (u, v, 0, t); left untouched on miss */
} mcrt_intersection;

/* RTFilterProperties with the DEVICE layout (56 B): KRN/kernel_data.h:63-80.
 * The reference host struct is 48 B (RadeonRays::float2 is 4-byte aligned),
 * so the reference device read shifted fields; this ABI
 * uses the explicit, correctly laid-out device struct. */
#define MCRT_BOX_FILTER          0
#define MCRT_TRIANGLE_FILTER     1
#define MCRT_GAUSSIAN_FILTER     2
#define MCRT_MITCHELL_FILTER     3
#define MCRT_LANCZOS_SINC_FILTER 4
typedef struct __attribute__((aligned(8))) {
    int32_t     filterType;
    int32_t     _align0;
    mcrt_float2 radius;
    float       mitchellB;
    float       mitchellC;
    float       lanczosSincTau;
    float       gaussianAlpha;
    float       gaussianExpX;
    float       gaussianExpY;
    mcrt_float2 pixelOffset;
    float       pad;
    int32_t     _align1;
} mcrt_filter;

/* ------------------------------------------------------------------------ */
/* Scene description = the 15 SCENE_PARAMS arrays (KRN/kernel_data.h:338-352,
 * filled by RTScene::setSceneArgs, APP/raytracing/scene/RTScene.cpp:178-197).
 * Host pointers; they are COPIED to HBM and may be freed after the call.     */
/* ------------------------------------------------------------------------ */
typedef struct {
    const mcrt_shape*        shapes;        uint32_t num_shapes;
    const uint32_t*          indices;       uint32_t num_indices;   /* per-shape local vertex indices */
    const mcrt_float3*       positions;     uint32_t num_vertices;  /* all per-vertex arrays have num_vertices */
    const mcrt_float2*       uvs;
    const mcrt_float3*       normals;
    const mcrt_float3*       tangents;
    const mcrt_float3*       binormals;
    const mcrt_float3*       colors;        /* may be NULL */
    const mcrt_texture_desc* textures;      uint32_t num_textures;
    const uint8_t*           tex_data;      uint64_t tex_data_bytes;
    const uint32_t*          sobol_matrices; uint32_t num_sobol_words; /* 1024 x 52 (APP/raytracing/sampling/sobol.h:34); may be NULL for the random sampler */
    const mcrt_light*        lights;        uint32_t num_lights;
    const mcrt_material*     materials;     uint32_t num_materials;
} mcrt_scene_desc;

/* BVH build options: RTScene::commit SetOption calls (APP/raytracing/scene/RTScene.cpp:203-238)
 * and IntersectorLDS::Process (RR/src/intersector/intersector_lds.cpp:176-196). */
typedef struct {
    float traversal_cost;   /* "bvh.sah.traversal_cost", default 10 */
    int   num_bins;         /* "bvh.sah.num_bins", default 64 */
    int   use_sah;          /* "bvh.builder" == "sah", default 1 */
    /* Which builder makes the flat structure.  0 (default) / 2: RadeonRays' Bvh2 node for node
     * (bit-exact parity), built on the device (mcrt_sahbuild.hip: the reference's split
     * arithmetic incl. this host's _mm_rcp_ps, its partition order in closed form; ~0.2 s for
     * 10 M triangles); falls back to 3 for num_bins > 64.  3: the same tree built on the host
     * (mcrt_bvh.cpp; ~2 s for 10 M triangles).  1: on-device linear BVH (Morton order, rocPRIM
     * radix sort), same record format and triangle data, different tree (equal-t hit ties may
     * resolve differently from the reference); ignores the three SAH fields.  4: perf tree (A/B
     * option, not the parity default): host binned SAH over all three axes, the cheapest split
     * wins (RR bins the largest centroid axis only); same records and traversal, another tree. */
    int   device_build;
    /* Two-level (instanced) structure: RadeonRays' IntersectorTwoLevel, which RR selects when a
     * shape is an instance (RTScene::attachMesh -> CreateInstance for every further entity that
     * shares a mesh, APP/raytracing/scene/RTScene.cpp:572-596) unless "bvh.forceflat"; forced by
     * "bvh.force2level" (RR/src/device/calc_intersection_device.cpp:68-105, defaults off,
     * PathTracingSettings.h:239-240).  Shapes with equal (startIdx, startVertex, numTriangles)
     * are instances of the first one; each keeps its own transform, shape id and material.
     * Host-built (device_build applies to the flat structure only); after a transform change its top
     * level alone is rebuilt, on the device or the host (mcrt_accel_update_transforms). */
    int   force_2level;
    int   force_flat;
    /* Per-shape world-to-local matrices (Shape::SetTransform's minv, RR/include/radeon_rays.h;
     * the reference passes Transform::getWorldToLocalMatrix).  NULL: the transpose of each
     * shape's toWorldInverseTranspose.  Used by the two-level structure only. */
    const mcrt_mat4* world_to_local;
} mcrt_accel_opts;

#define MCRT_SAMPLER_SOBOL  0   /* KRN/samplers.cl:16 */
#define MCRT_SAMPLER_RANDOM 1   /* KRN/samplers.cl:17 (reference default) */

/* Integrators: RTPathTracingPass (KRN/PathTracing.cl) and RTBDPTPass (KRN/BDPT.cl). */
#define MCRT_INTEGRATOR_PT   0
#define MCRT_INTEGRATOR_BDPT 1

/* One frame = one sample per pixel (RTPathTracingPass::update, APP/.../RTPathTracingPass.cpp:40-114). */
typedef struct {
    int32_t frame_index;        /* integrator_frameNum */
    int32_t max_depth;          /* PathTracerSettings::GI.maxDepth (default 2) */
    int32_t sampler;            /* MCRT_SAMPLER_* */
    int32_t russian_roulette;   /* 0 = off (parity mode; the reference has none) */
    int32_t rr_start_depth;     /* first bounce at which RR may terminate */
    /* Tile split for multi-GPU: rows y with (y / band_rows) % num_bands == band_index
     * are rendered; others are left untouched.  num_bands = 1 renders everything. */
    int32_t band_rows;
    int32_t num_bands;
    int32_t band_index;
    /* MCRT_INTEGRATOR_PT (0, default) or MCRT_INTEGRATOR_BDPT (RTBDPTPass::update,
     * APP/.../RTBDPTPass.cpp:67-128).  BDPT with num_bands > 1 renders the band's camera and
     * light subpaths; its light-tracing strategies splat into any pixel, so the frame stops after
     * the visibility pass: the caller sums the ranks' splats (mcrt_bdpt_splats_copy + a
     * reduce-scatter) and completes it with mcrt_bdpt_gather. */
    int32_t integrator;
    /* 1: textures at camera-ray hits are read mip-mapped over the pixel footprint (ray
     * differentials, computeSurfaceInteractionWithDifferentials + readTexture2Df_lod +
     * computeMipmapLOD: KRN/geometry.cl:92-175, KRN/textures.cl:148-202).  The reference carries
     * this path switched off (KRN/textures.cl:204-209); 0 (default) = its bilinear level-0
     * reads.  PT only; needs the textures' mip chains (mcrt_texture_desc.numMipLevels). */
    int32_t texture_lod;
} mcrt_frame_params;

typedef struct mcrt_ctx_s*         mcrt_ctx;
typedef struct mcrt_scene_s*       mcrt_scene;
typedef struct mcrt_framebuffer_s* mcrt_framebuffer;

/* ------------------------------------------------------------------------ */
/* Context (replaces PlatformManager/KernelManager/RTBufferManager,
 * APP/raytracing/system/{Kernel,Platform}Manager.cpp, and RadeonRays::CreateFromOpenClContext,
 * RR/src/api/radeon_rays.cpp:288-318).  One context per GPU.               */
/* ------------------------------------------------------------------------ */
MCRT_API mcrt_status mcrt_ctx_create(int device, mcrt_ctx* out);
MCRT_API mcrt_status mcrt_ctx_destroy(mcrt_ctx ctx);
MCRT_API const char* mcrt_last_error(mcrt_ctx ctx);   /* ctx may be NULL: last global error */
MCRT_API mcrt_status mcrt_ctx_synchronize(mcrt_ctx ctx);
/* stream: a hipStream_t (as void*) all work of this context is enqueued on; NULL = the context's own stream. */
MCRT_API mcrt_status mcrt_ctx_set_stream(mcrt_ctx ctx, void* stream);
/* The context stream (hipStream_t) that accumulation and the frame-buffer copies are enqueued on:
 * a caller orders its own work (e.g. an RCCL collective) after them with it. */
MCRT_API mcrt_status mcrt_ctx_get_stream(mcrt_ctx ctx, void** stream);
/* Per-kernel HIP-event timing (replaces QueryManager GPU timers, source/engine/util/QueryManager.h:141-164).
 * enable = 2 also counts the shadow rays answered by their occluder hint (mcrt_framebuffer_hint_counts);
 * those counters are device atomics that slow the shadow launches by a few per cent, so timing runs use 1. */
MCRT_API mcrt_status mcrt_ctx_set_profiling(mcrt_ctx ctx, int enable);
/* Synchronizes, then fills up to max entries: kernel name, summed HIP-event time (ms),
 * launch count and items processed (pixels / rays / paths); *count = kernels with stats. */
MCRT_API mcrt_status mcrt_ctx_kernel_stats(mcrt_ctx ctx, int max, const char** names,
                                           double* total_ms, int64_t* launches,
                                           int64_t* items, int* count);
MCRT_API mcrt_status mcrt_ctx_reset_stats(mcrt_ctx ctx);
/* Attainable HBM bandwidth: a float4 stream-copy kernel over `bytes` (>= 1 GiB recommended,
 * well above the 256 MB Infinity Cache), best of `iters` launches; *gbps = (read + write)
 * bytes / time.  The roofline's "attainable" figure next to the 8 TB/s spec peak. */
MCRT_API mcrt_status mcrt_ctx_stream_copy(mcrt_ctx ctx, uint64_t bytes, int iters, double* gbps);
/* Dependent-gather ceiling of the traversal's access pattern: every lane of 32 waves per CU
 * follows a chain of 64-B records over an array of `records` records (uniformly random links
 * read from the record just fetched, four 16-B loads per step), `steps` steps, best of `iters`
 * launches; *gsteps = dependent record fetches per second / 1e9.  The roofline's reference for
 * the node-visit rate of the latency-bound traversal kernels (records ~ the tree's node count:
 * served from HBM; ~2 M: Infinity Cache; ~32 K: L2). */
MCRT_API mcrt_status mcrt_ctx_gather_chase(mcrt_ctx ctx, uint64_t records, int steps, int iters, double* gsteps);
/* The same probe over the compact records' layout (the per-ray walks, mcrt_traverse.h qwalk):
 * records of 32 B (an internal node: 2 x 16-B loads) or 48 B (a leaf: 3 loads in the same round
 * trip, its type carried in the link) packed back to back, a share leaf_frac of them leaves. */
MCRT_API mcrt_status mcrt_ctx_gather_chase_compact(mcrt_ctx ctx, uint64_t records, double leaf_frac, int steps,
                                                   int iters, double* gsteps);

/* ------------------------------------------------------------------------ */
/* Scene (replaces RTScene upload + RadeonRays CreateMesh/AttachShape/SetId/
 * SetTransform/Commit: APP/raytracing/scene/RTScene.cpp:28-56,199-267,564-809;
 * RR/include/radeon_rays.h:214-237).                                        */
/* ------------------------------------------------------------------------ */
/* Accepted ranges, checked on the host before anything is uploaded: a shape's materialId in
 * -1 .. num_materials-1 (-1: no material) and lightID in -1 .. num_lights-1 (-1: not an emitter);
 * each of a material's eight texture ids in -1 .. num_textures-1 (-1: none), whatever its type; a
 * mesh light's shapeId names a shape with triangles; every index range inside the index array and
 * every vertex it names inside the vertex array.  MCRT_ERROR_INVALID_ARG otherwise, with a message
 * that names the entry.  num_lights = 0 is legal: both integrators return zeros. */
MCRT_API mcrt_status mcrt_scene_create(mcrt_ctx ctx, const mcrt_scene_desc* desc, mcrt_scene* out);
MCRT_API mcrt_status mcrt_scene_destroy(mcrt_scene scene);
/* Dynamic updates (RTScene::update, APP/raytracing/scene/RTScene.cpp:317-391). Shapes
 * whose transforms change go through mcrt_accel_update_transforms (below), which replaces the
 * shapes and brings the acceleration structure up to date in one call. */
/* Each update is checked against the tables the scene holds before any state changes, with the
 * ranges of mcrt_scene_create; a rejected call (MCRT_ERROR_INVALID_ARG) leaves the scene as it was.
 * _lights: every shape's lightID in -1 .. n-1, mesh lights name a shape with triangles; n = 0 is
 * legal while no shape holds a light id.  _materials: every shape's materialId in -1 .. n-1, the
 * new materials' texture ids in -1 .. num_textures-1; n = 0 is legal while no shape names a
 * material.  _shapes (and mcrt_accel_update_transforms): same count, startIdx and numTriangles;
 * materialId and lightID in the current tables' ranges; a moved startVertex keeps every vertex
 * the shape names inside the vertex array. */
MCRT_API mcrt_status mcrt_scene_update_lights(mcrt_scene scene, const mcrt_light* lights, uint32_t n);
MCRT_API mcrt_status mcrt_scene_update_materials(mcrt_scene scene, const mcrt_material* m, uint32_t n);
MCRT_API mcrt_status mcrt_scene_update_shapes(mcrt_scene scene, const mcrt_shape* s, uint32_t n);
/* Deforming meshes (skinning, cloth, morph targets, a simulation's output): replaces the positions
 * -- and the normals, unless `normals` is NULL: they are kept -- of vertices [first, first + count)
 * of the scene's vertex array.  Indices, uvs and the shapes stay.  MCRT_ERROR_INVALID_ARG for a NULL
 * scene, a NULL position pointer or a range that does not lie inside the vertex array; a rejected
 * call changes nothing.  The call runs after every launch already enqueued (it finishes the context
 * stream, then the device, as mcrt_accel_update_transforms does), so frames in flight finish on the
 * old vertices; it returns synchronised.  The surface records are regenerated in place: shading
 * sees the new positions and normals from the next launch on.
 * The acceleration structure is STALE afterwards, as after mcrt_scene_update_shapes, until
 * mcrt_accel_refit (same topology, fast) or mcrt_accel_build (a new tree) has run.
 * `area` of mcrt_shape and mcrt_light stays what the caller gave at creation: a deformed emitter
 * wants mcrt_scene_update_shapes / mcrt_scene_update_lights with its new area too.
 * _device: the same from device memory (a skinning kernel's output; float4 per vertex), copied on
 * the context stream.  The host copy of the positions that the host builders read is then
 * downloaded by the next call that needs it (mcrt_accel_build with a host builder, which the flat
 * route of mcrt_accel_update_transforms ends in). */
MCRT_API mcrt_status mcrt_scene_update_vertices(mcrt_scene scene, uint32_t first, uint32_t count,
                                                const mcrt_float4* positions, const mcrt_float4* normals);
MCRT_API mcrt_status mcrt_scene_update_vertices_device(mcrt_scene scene, uint32_t first, uint32_t count,
                                                       const void* d_positions, const void* d_normals);
/* BVH build over all shapes in world space (IntersectionApi::Commit ->
 * IntersectorLDS::Process -> Bvh2::Build, RR/src/accelerator/bvh2.h:206-315).
 * Hit shapeid = index into the shapes array (RTScene assigns SetId(nextShapeId++)
 * in shape order, RTScene.cpp:592,668). opts may be NULL (defaults). */
MCRT_API mcrt_status mcrt_accel_build(mcrt_scene scene, const mcrt_accel_opts* opts);
/* Moved shapes: RTScene::updateDynamicEntities' SetTransform on each moved shape + Commit
 * (APP/raytracing/scene/RTScene.cpp:317-391) in one call.  `shapes` replaces the scene's shape
 * array as mcrt_scene_update_shapes does (same count, startIdx and numTriangles; surface records
 * included) and the structure of the last mcrt_accel_build is brought up to date:
 *  - two-level: RadeonRays' Refit branch (RR/src/intersector/intersector_2level.cpp:495-660):
 *    every per-mesh tree stays, the world boxes are recomputed (transform_bbox) and a new
 *    top-level Bvh (RR/src/accelerator/bvh.cpp:73-437) is built over them with the build's
 *    traversal cost, bins and SAH switch.  Only records [0, top-level records) are rewritten, in
 *    place; the result equals a fresh mcrt_accel_build of the moved shapes.  startVertex must be
 *    unchanged too (the mesh key is (startIdx, startVertex, numTriangles)).  world_to_local: per
 *    shape as in mcrt_accel_opts; NULL = the transpose of each toWorldInverseTranspose.
 *    The top tree is built on the device (mcrt_topbuild.hip) from a threshold shape count upward
 *    and on the host below it; the environment variable MCRT_TOP_BUILD=host / =device forces one
 *    (=device fails with MCRT_ERROR_DEVICE where the device path cannot take the input, e.g. more
 *    than 64 bins; the structure is then still brought up to date on the host).
 *  - flat: RR's flat intersector rebuilds on every Commit: mcrt_scene_update_shapes +
 *    mcrt_accel_build with the options of the last build.
 * Ordered after every launch already enqueued on the context stream and on the frame-slot
 * streams.  MCRT_ERROR_NOT_READY before the first mcrt_accel_build, MCRT_ERROR_INVALID_ARG on a
 * topology change. */
MCRT_API mcrt_status mcrt_accel_update_transforms(mcrt_scene scene, const mcrt_shape* shapes, uint32_t n,
                                                  const mcrt_mat4* world_to_local /* may be NULL */);
/* Refit: brings the structure of the last mcrt_accel_build up to date with the scene's current
 * vertex positions (mcrt_scene_update_vertices) AND current shape transforms
 * (mcrt_scene_update_shapes), keeping the tree's topology.
 *  - flat (every builder: device SAH, host SAH, the perf tree, the LBVH): on the device
 *    (mcrt_refit.hip).  Every leaf becomes what the builder would write for its triangle, bit for
 *    bit; every box above becomes the exact union of its children; the compact records are
 *    converted again in place.  Depth, record count and device bytes do not change, and after the
 *    structure's first refit nothing is allocated.  Reported as path 4.
 *  - two-level: rebuilt with the options of the last build; correct, not fast.  Reported as path 3.
 * The tree's quality decays as the mesh leaves the pose it was built for: the caller decides when
 * to call mcrt_accel_build again.  mcrt_accel_update_transforms on a flat scene keeps its full
 * rebuild (path 3); a host that wants the fast path calls mcrt_scene_update_shapes and then this.
 * Synchronises as mcrt_accel_update_transforms does.  MCRT_ERROR_NOT_READY before the first
 * mcrt_accel_build. */
MCRT_API mcrt_status mcrt_accel_refit(mcrt_scene scene);
/* The last mcrt_accel_update_transforms or mcrt_accel_refit: *path 0 none yet, 1 top level built on
 * the device, 2 top level built on the host, 3 full rebuild (flat update_transforms, two-level
 * refit), 4 flat refit on the device; *ms its wall time including its synchronisation. */
MCRT_API mcrt_status mcrt_accel_update_info(mcrt_scene scene, int32_t* path, double* ms);
/* Build statistics: node count, bytes on device, host build milliseconds. */
MCRT_API mcrt_status mcrt_accel_info(mcrt_scene scene, uint64_t* num_nodes, uint64_t* device_bytes,
                                     double* build_ms, uint32_t* num_triangles);
/* Which structure mcrt_accel_build made: two_level 0 (flat Bvh2) / 1 (instanced), distinct
 * meshes and instances of the two-level one, deepest traversal path. */
MCRT_API mcrt_status mcrt_accel_layout(mcrt_scene scene, int32_t* two_level, uint32_t* num_meshes,
                                       uint32_t* num_instances, int32_t* depth);
/* Copy of the device records (64 B each, the mcrt_accel_build_host_records layout) into out
 * (up to max_records; out may be NULL to query *num_records).  In a flat structure a triangle
 * leaf's int word 13 holds its parent record's index on the device (the occluder hints' box test)
 * where the host build leaves -1. */
MCRT_API mcrt_status mcrt_accel_read_records(mcrt_scene scene, float* out, uint64_t max_records,
                                             uint64_t* num_records);
/* Copy of the flat structure's compact records (the per-ray walks' copy of the tree)
 * in 16-B units into out (up to max_units; out may be NULL to query).  *num_units is 0 where the
 * structure has none; *root_ref (may be NULL) is the root's reference, unit offset << 1 | leaf bit. */
MCRT_API mcrt_status mcrt_accel_read_compact(mcrt_scene scene, void* out, uint64_t max_units, uint64_t* num_units,
                                             uint32_t* root_ref);
/* The order of the compact records, on the host (no device needed): kids = n x (left, right) record
 * indices, (-1, -1) for a leaf, every child index above its parent's; order 1 sibling pairs, 2
 * treelets; off[i] = the 16-B unit at which record i starts (internal records take 2 units,
 * leaves 3; a 128-B line is 8), *num_units the copy's size. */
MCRT_API mcrt_status mcrt_accel_compact_order(const int32_t* kids, uint32_t n, int32_t order, uint32_t* off,
                                              uint64_t* num_units);
/* ------------------------------------------------------------------------ */
/* Scene ingestion for C/C++ hosts (mcrt_objload.cpp): OBJ + MTL + PNG into the
 * SCENE_PARAMS arrays, replacing the reference's assimp import + RTScene mesh,
 * material and texture conversion (source/engine/resource/AssetImporter.cpp:40,
 * APP/raytracing/scene/RTScene.cpp:564-766, 826-880).  Left-handed (z negated,
 * winding flipped), fan triangulation, face normals where vn is missing,
 * uber materials from Kd/Ks/Ns + map_Kd/map_bump/map_d/map_Ks, RGBA8 textures.  */
/* ------------------------------------------------------------------------ */
typedef struct mcrt_obj_scene_s* mcrt_obj_scene;
#define MCRT_OBJ_MIPS            1   /* store each texture's glGenerateMipmap chain (uploadTextures) */
#define MCRT_OBJ_EMISSIVE_LIGHTS 2   /* materials with Ke > 0 become triangle-mesh area lights */
MCRT_API mcrt_status mcrt_obj_load(const char* path, uint32_t flags, mcrt_obj_scene* out);
/* Extra lights (the demo's sun: PathTracingApp.cpp:395-401).  Directional lights are placed on
 * the scene's bounding sphere like RTScene::setLight (RTScene.cpp:482-494). */
MCRT_API mcrt_status mcrt_obj_add_directional_light(mcrt_obj_scene s, const float dir[3], const float intensity[3]);
MCRT_API mcrt_status mcrt_obj_add_point_light(mcrt_obj_scene s, const float pos[3], const float intensity[3]);
/* The arrays as a mcrt_scene_desc for mcrt_scene_create (pointers owned by s, valid until the
 * next add_* call or mcrt_obj_free; sobol_matrices left NULL for the caller to set). */
MCRT_API mcrt_status mcrt_obj_scene_desc(mcrt_obj_scene s, mcrt_scene_desc* desc);
MCRT_API const char* mcrt_obj_warnings(mcrt_obj_scene s);   /* missing MTL / skipped textures */
MCRT_API void mcrt_obj_free(mcrt_obj_scene s);

/* Which builder made the flat structure: 0 host (or two-level), 1 device LBVH, 2 device SAH
 * (mcrt_accel_opts.device_build 0 and 2), 4 the host 3-axis SAH perf tree (device_build 4). */
MCRT_API mcrt_status mcrt_accel_builder(mcrt_scene scene, int32_t* builder);
/* Host-only build of the structure mcrt_accel_build would upload (no device needed): 64-B
 * records (mcrt_bvh.cpp / mcrt_bvh2l.cpp layouts) into out_records (up to max_records; may be
 * NULL to query *num_records); info[4] = {two_level, top-level records, depth, meshes}.
 * For tools and tests (e.g. pinning the trees against the reference builders). */
MCRT_API mcrt_status mcrt_accel_build_host_records(const mcrt_scene_desc* desc, const mcrt_accel_opts* opts,
                                                   float* out_records, uint64_t max_records,
                                                   uint64_t* num_records, int32_t* info);

/* Host-only twin of mcrt_accel_update_transforms (no device needed): builds `desc` as it stands,
 * applies the refit for moved_shapes (RR's Refit branch, intersector_2level.cpp:495-660) through
 * the function the device scene's host path uses, and returns the records and info as above.  For
 * a flat structure: the fresh build of the moved shapes. */
MCRT_API mcrt_status mcrt_accel_refit_host_records(const mcrt_scene_desc* desc, const mcrt_accel_opts* opts,
                                                   const mcrt_shape* moved_shapes,
                                                   const mcrt_mat4* moved_world_to_local,
                                                   float* out_records, uint64_t max_records,
                                                   uint64_t* num_records, int32_t* info);

/* ------------------------------------------------------------------------ */
/* Ray queries on DEVICE buffers (IntersectionApi::QueryIntersection /
 * QueryOcclusion, RR/include/radeon_rays.h:267-277 -> IntersectorLDS::Intersect/
 * Occluded, RR/src/intersector/intersector_lds.cpp:266-326).
 * Semantics of intersect_main/occluded_main (RR/src/kernels/CL/intersect_bvh2_lds.cl):
 *  - rays with extra[1] == 0 leave their output untouched;
 *  - a leaf is skipped when ray mask (extra[0]) == shape id (RR_RAY_MASK);
 *  - closest: miss -> shapeid = primid = -1 (uvwt untouched), hit -> uvwt = (u,v,0,t);
 *  - any: 1 = occluded, -1 = not occluded.                                 */
/* ------------------------------------------------------------------------ */
MCRT_API mcrt_status mcrt_trace_closest(mcrt_scene scene, const mcrt_ray* d_rays, int32_t n,
                                        mcrt_intersection* d_hits);
MCRT_API mcrt_status mcrt_trace_any(mcrt_scene scene, const mcrt_ray* d_rays, int32_t n,
                                    int32_t* d_hits);
/* The variants with the ray count in device memory (QueryIntersection / QueryOcclusion with
 * `Buffer const* numrays, int maxrays`, RR/include/radeon_rays.h:272-277; the count a previous
 * kernel wrote, read by the query kernel itself, so no host round trip): min(*d_numrays, maxrays)
 * rays are traced, the grid covers maxrays.  Asynchronous on the context stream, as RR's queries:
 * the query waits for wait_event (NULL: none) and, when done_event is not NULL, *done_event
 * receives a new event recorded after it (RR's `Event** event`; mcrt_event_wait = Event::Wait,
 * mcrt_event_destroy = IntersectionApi::DeleteEvent). */
typedef struct mcrt_event_s* mcrt_event;
MCRT_API mcrt_status mcrt_trace_closest_count(mcrt_scene scene, const mcrt_ray* d_rays, const int32_t* d_numrays,
                                              int32_t maxrays, mcrt_intersection* d_hits, mcrt_event wait_event,
                                              mcrt_event* done_event);
MCRT_API mcrt_status mcrt_trace_any_count(mcrt_scene scene, const mcrt_ray* d_rays, const int32_t* d_numrays,
                                          int32_t maxrays, int32_t* d_hits, mcrt_event wait_event,
                                          mcrt_event* done_event);
MCRT_API mcrt_status mcrt_event_wait(mcrt_event event);
MCRT_API mcrt_status mcrt_event_destroy(mcrt_event event);

/* ------------------------------------------------------------------------ */
/* Frame buffer + integrator (RTPrimaryRaysPass, RTPathTracingPass,
 * RTReconstructionPass: APP/raytracing/renderPasses/RT*Pass.cpp; kernels
 * KRN/PathTracing.cl, KRN/reconstruction.cl).                              */
/* ------------------------------------------------------------------------ */
MCRT_API mcrt_status mcrt_framebuffer_create(mcrt_ctx ctx, uint32_t width, uint32_t height,
                                             mcrt_framebuffer* out);
MCRT_API mcrt_status mcrt_framebuffer_destroy(mcrt_framebuffer fb);
/* Frames in flight (PT): mcrt_render_frame for frame i uses buffer slot i mod n on its own HIP
 * stream and returns at once; mcrt_accumulate runs on the context stream in call order, after
 * that frame's render, so n frames overlap on the GPU and the image is unchanged bit for bit
 * (the reference's pass sequence per frame, RTPathTracingPass::update then
 * RTReconstructionPass::updateReconstruction, is kept; only its clFinish after every launch is
 * gone).  0 = auto = 2: each launch's divergent tail of long rays is filled by the next
 * frame's launches (small band shares are better widened by mcrt_render_frames).  Reads of the frame
 * buffer synchronise every slot.  No reference counterpart (its passes are synchronous). */
#define MCRT_MAX_FRAMES_IN_FLIGHT 4
MCRT_API mcrt_status mcrt_framebuffer_set_frames_in_flight(mcrt_framebuffer fb, int32_t n);
/* Renders one 1-spp frame: PrimaryRays + maxDepth x (shade, shadow, extend).
 * Result: per-pixel frame radiance ("RadianceBufferCL"). */
MCRT_API mcrt_status mcrt_render_frame(mcrt_scene scene, mcrt_framebuffer fb, const mcrt_camera* camera,
                                       const mcrt_frame_params* params);
/* ReconstructionPass (KRN/reconstruction.cl:6-60): clamp [0,1000] (NaN->0),
 * frame_index 0 overwrites, else accumulates sum(w*L), sum(w); image = ratio.
 * After mcrt_render_frames it accumulates every frame of that batch in frame order
 * (frame_index = the batch's first frame), all with this filter. */
MCRT_API mcrt_status mcrt_accumulate(mcrt_framebuffer fb, const mcrt_filter* filter, int32_t frame_index);
/* Batched frames (PT and BDPT): renders the `count` (PT 1..256, BDPT 1..32: its per-frame arrays
 * are whole-frame sized) consecutive 1-spp frames
 * params->frame_index + k, k < count, with cameras[k] (per-frame TAA jitter), in ONE pass --
 * every launch (camera rays, shading, shadow + extension rays) covers all count frames' paths,
 * so a small per-rank band share (tile split over N GPUs) still fills the 256 CUs and the
 * divergent tail of each launch is paid once per batch (1/8 of the bands x 160 frames = the
 * paths of one GPU's 20-frame call).  Per frame the arithmetic, the RNG
 * streams (keyed by pixel, frame_index + k, bounce) and the radiance are exactly those of
 * mcrt_render_frame; mcrt_accumulate_frames (or mcrt_accumulate) then sums them in frame order,
 * so the image equals count x (mcrt_render_frame + mcrt_accumulate) bit for bit.  Radiance read
 * back (mcrt_framebuffer_read 0) is the batch's first frame.  The reference renders one frame
 * per RTPathTracingPass::update; this is the same sequence, launched wider.
 * BDPT (RTBDPTPass::update per frame): every launch covers the batch's (tile, frame) paths; the
 * s = 1 strategies walk the batch's frames in order, so the sampled-light-vertex slot each frame
 * reads is the one the previous frame wrote (BDPT.cl:585-586), as in count single calls; vertices
 * and own strategies are those of count single calls bit for bit, splat sums up to atomic order.
 * With a band split, mcrt_bdpt_splat_layout's chunk then holds the batch's frames.
 * Memory (PT): each frame slot (2 in flight) holds about 0.8 KB per path of the call (ray queues,
 * hit records, the per-ray traversal stack spill and, for calls of >= 16 M paths, the stopped
 * walks' state) plus 32 B per pixel and frame: 1080p x 20 frames ~ 34 GB per slot.  A call that does not fit fails with the hipMalloc error (nothing is
 * rendered; smaller calls still work), e.g. 256 whole 1080p frames; 256 band-frames of a 1/8
 * band share fit. */
MCRT_API mcrt_status mcrt_render_frames(mcrt_scene scene, mcrt_framebuffer fb, const mcrt_camera* cameras,
                                        int32_t count, const mcrt_frame_params* params);
/* filters: `count` filters (one per frame of the last mcrt_render_frames; the per-frame filter
 * props of RTReconstructionPass) or 1 shared by all; frame_index = the batch's first frame. */
MCRT_API mcrt_status mcrt_accumulate_frames(mcrt_framebuffer fb, const mcrt_filter* filters, int32_t count,
                                            int32_t frame_index);
/* Device pointers of the frame buffer's arrays (float4 x W*H, float x W*H).  The radiance
 * pointer is the plane of the LAST rendered frame: frames rotate through the frame slots
 * (mcrt_framebuffer_set_frames_in_flight), so it is valid only until the next render call on this
 * frame buffer, and work on another stream must first synchronise with the frame (e.g.
 * mcrt_ctx_synchronize).  The accumulator and image pointers are fixed for the frame buffer's life. */
MCRT_API mcrt_status mcrt_framebuffer_device_ptrs(mcrt_framebuffer fb, void** radiance, void** weighted_sum,
                                                  void** weight_sum, void** image);
/* Post-process of the accumulated image, the passes after RTReconstructionPass in the
 * reference pipeline (PathTracingApp.cpp:240-254): RTDenoisePass (BilateralDenoise,
 * KRN/Denoise.cl:6-47, RTDenoisePass.cpp) then RTToneMappingPass (ReinhardToneMapping,
 * KRN/ToneMapping.cl:42-63, RTToneMappingPass.cpp; the pass passes GI.minLuminance as Lwhite).
 * Result: the display image (mcrt_framebuffer_read which = 3), = the image when both are off. */
typedef struct {
    int32_t use_denoise;        /* GI.useDenoise (default 0) */
    int32_t denoise_radius;     /* GI.denoiseKernelRadius (default 1) */
    float   sigma_spatial;      /* GI.bilateralDenoiseSigmaSpatial (default 1.0) */
    float   sigma_range;        /* GI.bilateralDenoiseSigmaRange (default 0.1) */
    int32_t use_tonemapping;    /* GI.useTonemapping (default 0) */
    float   min_luminance;      /* GI.minLuminance (default 2.0), Reinhard's Lwhite */
} mcrt_postprocess_params;
MCRT_API mcrt_status mcrt_postprocess(mcrt_framebuffer fb, const mcrt_postprocess_params* params);
/* Per-pixel outputs at the camera-ray hits (camera rays traced by this call; no shading):
 *  MCRT_AOV_ALBEDO:      float4 per pixel = (uber diffuse Kd incl. texture, opacity.x), zero on
 *                        a miss; mip-mapped when params->texture_lod (an albedo guide for denoisers)
 *  MCRT_AOV_TEXTURE_LOD: 3 float4 per pixel = (duvdx, duvdy), (diffuse-texture LOD, shape index
 *                        bits, uv), the diffuse texture read at that LOD (zeros where untextured).
 * host_out: W*H*{1|3}*4 floats.  Band fields of params select the rows as in mcrt_render_frame. */
#define MCRT_AOV_ALBEDO      0
#define MCRT_AOV_TEXTURE_LOD 1
MCRT_API mcrt_status mcrt_render_aov(mcrt_scene scene, mcrt_framebuffer fb, const mcrt_camera* camera,
                                     const mcrt_frame_params* params, int aov, float* host_out);
/* ---- Guide-buffer-driven denoiser (opt-in; nothing below changes any other call's output) ----
 *
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the accumulated image,
 * steered by geometry guides captured at the camera-ray hits and, optionally, by a per-pixel
 * variance estimated from luminance moments accumulated next to the image (as in SVGF).
 *
 * Guides: two float4 planes of W*H records owned by the frame buffer (allocated on first use).
 *   normal-plane  (n.x, n.y, n.z, n . (P - cam.pos)): n the interpolated shading normal before
 *                 normal mapping, flipped to face the camera, P the hit point; the plane offset
 *                 is camera-relative so that a scene far from the origin loses nothing
 *   albedo-depth  (Kd.rgb, |P - cam.pos|): Kd exactly MCRT_AOV_ALBEDO's (honours texture_lod)
 * A miss holds (0,0,0,0) and (0,0,0,-1).
 *
 * mcrt_render_guides traces the camera rays of `camera` (mcrt_render_aov's path: it waits for the
 * frame slots and reuses the bound slot's camera and primary-hit buffers) and writes the guides of
 * the rows the band fields of params select; other rows keep their content.  Everything stays on
 * the device, enqueued on the context stream.  mcrt_framebuffer_set_guides installs both planes
 * from device memory instead (tests, other renderers). */
MCRT_API mcrt_status mcrt_render_guides(mcrt_scene scene, mcrt_framebuffer fb, const mcrt_camera* camera,
                                        const mcrt_frame_params* params);
MCRT_API mcrt_status mcrt_framebuffer_set_guides(mcrt_framebuffer fb, const void* d_normal_plane,
                                                 const void* d_albedo_depth);
/* Luminance moments.  While enabled, mcrt_accumulate / mcrt_accumulate_frames also update, for
 * the pixels of the band and per frame of the batch in frame order,
 *   l = (0.212671f*r + 0.715160f*g) + 0.072169f*b,  m1 += l,  m2 += l*l
 * with r, g, b the radiance clamped to [0, 1000] as the accumulation clamps it; frame_index 0
 * overwrites both and restarts the frame count.  The moments are UNWEIGHTED: the reconstruction
 * filter weight (one number per frame) is deliberately not applied, they describe the samples.
 * Enabling allocates and zeroes the plane (0 frames); disabling keeps it.
 * mcrt_framebuffer_set_moments installs (m1, m2) float2 records of `frames` frames from device
 * memory. */
MCRT_API mcrt_status mcrt_framebuffer_set_moments_enabled(mcrt_framebuffer fb, int on);
MCRT_API mcrt_status mcrt_framebuffer_set_moments(mcrt_framebuffer fb, const void* d_m1m2, int32_t frames);
/* Reads guide data back: which 0 normal-plane (float4), 1 albedo-depth (float4), 2 moments
 * (float2), 3 the filtered variance of the last mcrt_denoise_guided (float).  *needed (may be
 * NULL) receives the byte size; host_dst may be NULL to query it; otherwise bytes must be >= it.
 * MCRT_ERROR_NOT_READY when the plane does not exist yet. */
MCRT_API mcrt_status mcrt_framebuffer_read_guides(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                  uint64_t* needed);
/* The filter: image -> display image (mcrt_framebuffer_read which = 3), enqueued on the context
 * stream after the last accumulate.  Level i = 0 .. levels-1 has step s = 2^i and the 25 taps
 * q = p + s*(dx, dy), dx, dy in -2..2 (taps outside the image are skipped), h = [1/16, 1/4, 3/8, 1/4, 1/16]:
 *   e  = |n_p - n_q|^2 / sigma_normal^2 + (d_p - d_q)^2 / (sigma_depth * z_p)^2
 *        + (l_p - l_q)^2 / (sigma_i^2 * v_p + 1e-8)
 *   w  = h[dx] h[dy] expf(-e);   c' = sum w c_q / sum w;   var' = sum w^2 var_q / (sum w)^2
 * d the plane offset, z_p the centre's depth (1 on a miss), l the luminance of the level's input.
 * With use_variance and moments of n >= 2 frames: var0 = max(0, m2/n - (m1/n)^2) / (n - 1),
 * v_p = the 3x3 Gaussian of var around p, sigma_i = sigma_luminance; otherwise var = 1, v_p = 1 and
 * sigma_i = sigma_luminance * 2^-i.  With demodulate_albedo the filter runs on image / albedo
 * (channels with albedo <= 1e-3 are left alone) and multiplies the albedo back after the last
 * level.  Alpha passes through.  mcrt_postprocess and its denoised image are not touched.
 * MCRT_ERROR_NOT_READY without guides or with a band-split BDPT frame pending; under a band split
 * run it on the gathering rank after mcrt_framebuffer_bands_unpack, with guides that rank renders
 * whole-image (moments are not gathered: var = 1). */
typedef struct {
    int32_t levels;             /* 1..8; default 5 (steps 1,2,4,8,16) */
    float   sigma_normal;       /* default 0.1 */
    float   sigma_depth;        /* default 0.02, relative to the centre pixel's depth */
    float   sigma_luminance;    /* default 4.0 (in standard deviations when variance is used) */
    int32_t use_variance;       /* 1: guide the luminance weight by the moments when >= 2 frames are in them */
    int32_t demodulate_albedo;  /* 1: filter image / albedo, multiply back after the last level */
    int32_t use_tonemapping;    /* then k_tonemap, as mcrt_postprocess */
    float   min_luminance;
} mcrt_guided_denoise_params;
MCRT_API mcrt_status mcrt_denoise_guided(mcrt_framebuffer fb, const mcrt_guided_denoise_params* params);

/* ---- Temporal reprojection and history for the guided denoiser ---------------------------------
 * The temporal half of SVGF (Schied et al. 2017) for an interactive caller that shows 1..k samples
 * per displayed frame while the camera moves.  All of it is opt-in: without these calls nothing
 * else launches, allocates or changes.  Per displayed frame:
 *   1. render 1..k frames and accumulate them starting at frame_index 0,
 *   2. mcrt_render_guides(camera),
 *   3. mcrt_temporal_accumulate(fb, camera, params)   -- the camera those guides were made with,
 *   4. mcrt_denoise_guided_temporal(fb, params, feedback_level)  -> display image.
 *
 * History planes, owned by the frame buffer, W*H records each, allocated on first use:
 *   colour   float4  the integrated colour in filter space (image / albedo with demodulate_albedo,
 *                    channels with albedo <= 1e-3 left alone), alpha of the current image
 *   moments  float4  (mu1, mu2, N, z): the integrated luminance moments, the history length N (a
 *                    float), the pixel's guide depth when the record was written (-1 on a miss)
 *   previous normal-plane float4: the guide record the pixel had when written
 *   variance float   the variance handed to the filter
 * and a host copy of the camera they belong to.  The first three exist twice (read / written) and
 * swap per accumulate; the guide planes themselves are never swapped or written.
 *
 * mcrt_temporal_accumulate, pixel p = (x, y), c = image (demodulated), l its luminance:
 *   P - prev.pos = m * (depth_p / |m|) + (camera.pos - prev.pos), m the bilinear blend of camera's
 *   corner directions at (x / W, y / H); the world point itself is never formed, so a scene far
 *   from the origin loses nothing.  Its clip coordinates are rows 0, 1 and 3 of prev.worldToClip
 *   applied to that offset, xyz only, the translation column dropped:
 *     REQUIREMENT: camera.worldToClip must be a view-projection centred on camera.pos (then
 *     worldToClip * (pos, 1) has zero x, y and w and the dropped column cancels exactly).
 *     mcrt_make_pinhole_camera and mcrt.camera.make_camera make such cameras.
 *   worldToClip carries no TAA jitter while the corner directions do, so history is resampled at the
 *   unjittered projection.  With f = ((clip.xy / clip.w + 1) / 2) * (W, H), the four history
 *   records around f (bilinear weights w) are tested: a tap q counts when it was a hit,
 *   |n_p - n_q|^2 <= normal_threshold, and the plane it stored passes through the point,
 *   |n_q . (P - prev.pos) - d_q| <= plane_threshold * |P - prev.pos|.  The test is on the plane, not
 *   on a depth difference: a floor seen at a grazing angle is not rejected.
 *   With valid weight above 1e-4:  N = min(sum w N_q / sum w + 1, max_history),
 *     a = max(alpha, 1 / N), colour = lerp(history, c, a); the moments likewise with alpha_moments.
 *   Otherwise (disocclusion, miss, off screen, no history):  N = 1, colour = c, moments = (l, l*l).
 * Then the variance:  N >= min_history: max(0, mu2 - mu1^2);  otherwise the same expression of the
 * moments averaged over the 7x7 neighbours on p's surface (both misses, or both hits whose
 * normals and plane offsets agree within the thresholds, the offsets relative to p's depth), times
 * min_history / N.  This is the variance of the samples, not of the mean: sigma_luminance keeps
 * its default.  The float32 operation order of both kernels is fixed in mcrt_denoise.hip and
 * restated in tests/temporal_ref.py.
 *
 * mcrt_denoise_guided_temporal runs mcrt_denoise_guided's levels with the colour history as the
 * level-0 colour (no demodulation pass: it is in filter space already), the variance plane as var0
 * and use_variance as given (no moments of mcrt_accumulate are needed); remodulation, tone mapping
 * and the display image as there.  feedback_level = k >= 0 makes the output of level k the colour
 * history the next accumulate integrates (SVGF: k = 0) by exchanging plane pointers, no copy;
 * -1 feeds nothing back.  params->demodulate_albedo must equal the last accumulate's flag.
 *
 * mcrt_temporal_reset: the next accumulate starts without history (planes are kept).
 * mcrt_framebuffer_set_temporal_history installs colour, moments and previous normal-plane (float4
 * planes in device memory) and the camera they belong to (tests, other renderers).
 * mcrt_framebuffer_read_temporal reads the planes as the NEXT accumulate will read them: which 0
 * colour history, 1 moments history, 2 variance (float), 3 previous normal-plane; needed / host_dst
 * / bytes as mcrt_framebuffer_read_guides.
 *
 * MCRT_ERROR_INVALID_ARG: NULL arguments, alpha or alpha_moments outside [0, 1], max_history or
 * min_history < 1, non-positive thresholds, a camera whose size differs from the frame buffer,
 * feedback_level outside -1 .. levels - 2, demodulate_albedo differing from the last accumulate.
 * MCRT_ERROR_NOT_READY: no guides, a band-split BDPT frame pending, mcrt_denoise_guided_temporal
 * before any accumulate or a second time after the same accumulate when the first call fed back.
 * Everything is enqueued on the context stream after the last accumulate and the guides, as
 * mcrt_denoise_guided; mcrt_framebuffer_read_temporal synchronises.
 *
 * mcrt_temporal_accumulate assumes a static world: a moved instance's history is rejected by the
 * plane test, or ghosts when the instance slides within its own plane.  The per-object motion
 * section below reprojects through each shape's own motion.  Band-split or multi-rank history is
 * not kept: run this on the gathering rank. */
typedef struct {
    float   alpha;              /* weight floor of the new frame's colour, 0..1, default 0.2 */
    float   alpha_moments;      /* same for the luminance moments, default 0.2 */
    int32_t max_history;        /* cap of the history length N, >= 1, default 32 */
    int32_t min_history;        /* N below which the variance is estimated spatially, >= 1, default 4 */
    float   normal_threshold;   /* a history tap is valid when |n_p - n_q|^2 <= this, > 0, default 0.1 */
    float   plane_threshold;    /* ... and its plane passes P within this * |P - prev.pos|, > 0, default 0.01 */
    int32_t demodulate_albedo;  /* 1: the history lives in image / albedo space (as mcrt_denoise_guided's flag) */
} mcrt_temporal_params;
MCRT_API mcrt_status mcrt_temporal_accumulate(mcrt_framebuffer fb, const mcrt_camera* camera,
                                              const mcrt_temporal_params* params);
MCRT_API mcrt_status mcrt_temporal_reset(mcrt_framebuffer fb);
MCRT_API mcrt_status mcrt_denoise_guided_temporal(mcrt_framebuffer fb, const mcrt_guided_denoise_params* params,
                                                  int32_t feedback_level);
MCRT_API mcrt_status mcrt_framebuffer_set_temporal_history(mcrt_framebuffer fb, const void* d_colour,
                                                           const void* d_moments, const void* d_normal_plane,
                                                           const mcrt_camera* prev_camera);
MCRT_API mcrt_status mcrt_framebuffer_read_temporal(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                    uint64_t* needed);

/* ---- Per-object motion for the temporal history -------------------------------------------------
 * Reprojects the history through the motion of the shape each pixel sees, so that an object moved
 * with mcrt_accel_update_transforms (or mcrt_scene_update_shapes + mcrt_accel_build) keeps its
 * history.  Opt-in like the sections above: without these calls no launch, buffer, kernel argument
 * or output of any other call changes.  Per displayed frame:
 *   1. mcrt_scene_motion_snapshot(scene)          -- the poses of the frame just shown,
 *   2. mcrt_accel_update_transforms(scene, ...)   -- this frame's poses,
 *   3. render 1..k frames and accumulate them starting at frame_index 0,
 *   4. mcrt_render_guides_motion(scene, fb, camera, params),
 *   5. mcrt_temporal_accumulate_motion(fb, camera, params),
 *   6. mcrt_denoise_guided_temporal(fb, params, feedback_level)   -- unchanged.
 *
 * mcrt_scene_motion_snapshot records, for every shape, the current toWorldTransform,
 * toWorldInverseTranspose and mesh key (startIdx, startVertex, numTriangles) as its previous pose:
 * a device table owned by the scene, 144 B per shape, allocated by the first snapshot and copied
 * out of the scene's shape array on the context stream.  It sees every mcrt_scene_update_shapes /
 * mcrt_accel_update_transforms made before it and none made after, and needs no mcrt_accel_build.
 *
 * mcrt_render_guides_motion is mcrt_render_guides (the same host path, the same two guide planes,
 * bit for bit) whose one guide launch also writes two more float4 planes owned by the frame buffer
 * (allocated on first use), for the rows the band fields select:
 *   motion           (P_prev - P, flag), P the hit point, P_prev the same surface point under the
 *                    shape's previous pose: the hit's three object-space vertices through the
 *                    table's toWorldTransform and the same barycentric blend, then one subtraction
 *                    per component.
 *                    flag  0: static -- no snapshot yet, or all 32 matrix floats (compared as
 *                             uint32) and the mesh key equal the table's; the record is exactly
 *                             (0, 0, 0, 0).  A miss holds the same.
 *                    flag  1: moved.
 *                    flag -1: no previous pose -- the mesh key differs; the record is (0, 0, 0, -1).
 *   previous normal  (n_prev, 0) where flag is 1, (0, 0, 0, 0) elsewhere: the interpolated shading
 *                    normal formed from the object-space normals through the table's
 *                    toWorldInverseTranspose (so non-uniform scales and mirrors need no case),
 *                    flipped exactly when the guide normal was: the same physical side.
 * mcrt_framebuffer_set_motion installs both planes from device memory (tests, other renderers).
 * The motion planes belong to one set of guides: mcrt_render_guides and mcrt_framebuffer_set_guides
 * make them stale.  mcrt_framebuffer_read_motion: which 0 motion, 1 previous normal; needed /
 * host_dst / bytes as mcrt_framebuffer_read_guides.
 *
 * mcrt_temporal_accumulate_motion is mcrt_temporal_accumulate (parameters, validation, plane swap,
 * variance) with, per pixel, mv = motion[p]:
 *   flag  1:  P - prev.pos becomes (P - prev.pos) + mv.xyz, and the normal test compares the
 *             history tap with n_prev instead of the guide normal; the plane test, the clip
 *             coordinates and the tolerance use the moved offset,
 *   flag  0:  as mcrt_temporal_accumulate (with an all-zero motion plane every plane written is
 *             bit-identical to it),
 *   flag -1:  no tap is tested: N = 1 and the current values.
 * The record written to the previous normal-plane history is the current guide record either way.
 * A background pixel an object has uncovered (flag 0) reprojects onto where the object was and is
 * rejected by the plane test, like a camera-move disocclusion.
 *
 * MCRT_ERROR_NOT_READY in addition to the calls they extend: mcrt_temporal_accumulate_motion without
 * motion planes belonging to the current guides.
 * Not covered: deforming geometry (a changed mesh key gives flag -1), moving lights and the shading
 * lag of moved shadows and reflections, motion under a band split or across ranks. */
MCRT_API mcrt_status mcrt_scene_motion_snapshot(mcrt_scene scene);
MCRT_API mcrt_status mcrt_render_guides_motion(mcrt_scene scene, mcrt_framebuffer fb, const mcrt_camera* camera,
                                               const mcrt_frame_params* params);
MCRT_API mcrt_status mcrt_framebuffer_set_motion(mcrt_framebuffer fb, const void* d_motion, const void* d_prev_normal);
MCRT_API mcrt_status mcrt_framebuffer_read_motion(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                  uint64_t* needed);
MCRT_API mcrt_status mcrt_temporal_accumulate_motion(mcrt_framebuffer fb, const mcrt_camera* camera,
                                                     const mcrt_temporal_params* params);

/* ---- Adaptive sampling: render only the tiles above an error target (opt-in) --------------------
 * Without these calls nothing else launches, allocates or changes.  In adaptive mode a path-tracing
 * call renders, and the accumulate after it touches, only the tiles of an active list; every other
 * pixel keeps its accumulators, image and moments.  A tile is 8x8 pixels (one wave); tile t is
 * column-block t % ceil(W/8) of row-block t / ceil(W/8).  The loop of a host:
 *   mcrt_framebuffer_set_adaptive(fb, &params);            -- mode on, moments on, reset
 *   do { render + accumulate a round of frames (frame_index counts on from 0);
 *        mcrt_adaptive_update(fb, &active); } while (active > 0);
 * A tile holds n samples (its own count: tiles differ).  mcrt_adaptive_update judges every tile from
 * the luminance moments (m1, m2) of its pixels, in float32 and in this order (IEEE division and
 * square root, no contraction; tests/adaptive_ref.py restates it):
 *   per pixel inside the image:  mean = m1 / n;  v = max(0, m2 / n - mean * mean) / (n - 1)
 *   Sv = sum v, Sm = sum mean over the tile's 64 lanes (lane l = pixel (l & 7, l >> 3), 0 outside
 *        the image), each by the butterfly s = s + s[lane ^ d], d = 32, 16, 8, 4, 2, 1
 *   err = sqrt(Sv / c) / (Sm / c + luminance_floor),  c = the tile's pixels inside the image;
 *         +inf while n < 2
 *   active = n < min_samples ? 1 : (max_samples > 0 && n >= max_samples) ? 0 : err > error_threshold
 * and rebuilds the list: the active tiles in ascending order.  It waits for the frame slots and the
 * context stream -- the one host synchronisation per round -- and returns the list's length.
 *
 * mcrt_framebuffer_set_adaptive: non-NULL params turn the mode on, turn the moments on (allocating
 *   the plane as mcrt_framebuffer_set_moments_enabled does) and reset; NULL turns the mode off and
 *   frees its state (moments stay as they are).
 * mcrt_adaptive_reset: zeroes the tile counts and the frame count, lists every tile and drops a
 *   rendered frame that was not accumulated.  The host calls it when it restarts the accumulation.
 * mcrt_framebuffer_set_active_tiles: installs a host list of n tile ids, strictly ascending and below
 *   the tile count; n = 0 is legal.  This is region rendering; the next update replaces the list.
 * mcrt_framebuffer_read_adaptive: which 0 the tile errors (float), 1 the tile sample counts
 *   (uint32), one per tile; 2 the active list (uint32, its current length).  needed / host_dst /
 *   bytes as mcrt_framebuffer_read_guides.
 *
 * In adaptive mode:
 *  - mcrt_render_frame(s) launches over the list only; with an empty list it launches nothing.  The
 *    radiance of an unlisted tile is NOT written: mcrt_framebuffer_read 0, mcrt_framebuffer_read_frame
 *    and the device copies of the radiance are defined only on the tiles of the list the call
 *    rendered with.  mcrt_framebuffer_stats counts the listed tiles' paths.
 *  - mcrt_accumulate(_frames) needs a rendered frame; frame_index must equal the frames accumulated
 *    since the reset, and frame_index 0 needs the full list (mcrt_adaptive_reset).  Per listed pixel
 *    it runs the operations of the plain call in the same order; "first sample" is the tile's count
 *    being 0.  Then every listed tile's count grows by the batch.
 *  - mcrt_denoise_guided with use_variance takes n per pixel from its tile's count (n < 2: var = 1).
 *  - mcrt_framebuffer_set_moments also sets every tile's count and the frame count to `frames`.
 * MCRT_ERROR_INVALID_ARG, before anything changes: parameters out of range; a BDPT render (its
 * light-tracing splats land in any tile); num_bands > 1; mcrt_temporal_accumulate(_motion); turning
 * the moments off; a wrong frame_index; a list that is not strictly ascending or names a tile past
 * the image; mcrt_adaptive_reset / _update / mcrt_framebuffer_set_active_tiles with the mode off.
 * MCRT_ERROR_NOT_READY: mcrt_adaptive_update or mcrt_framebuffer_set_active_tiles with a rendered
 * frame not yet accumulated; mcrt_accumulate without one. */
typedef struct {
    float   error_threshold;   /* a tile is done when its error <= this; >= 0 */
    int32_t min_samples;       /* a tile is not judged before it has this many; >= 2 */
    int32_t max_samples;       /* a tile stops at this many whatever its error; 0 = no cap, else >= min_samples */
    float   luminance_floor;   /* added to the tile's mean luminance in the denominator; > 0, default 1e-3 */
} mcrt_adaptive_params;
MCRT_API mcrt_status mcrt_framebuffer_set_adaptive(mcrt_framebuffer fb, const mcrt_adaptive_params* params);
MCRT_API mcrt_status mcrt_adaptive_reset(mcrt_framebuffer fb);
MCRT_API mcrt_status mcrt_adaptive_update(mcrt_framebuffer fb, int32_t* active_tiles);
MCRT_API mcrt_status mcrt_framebuffer_set_active_tiles(mcrt_framebuffer fb, const uint32_t* tiles, int32_t n);
MCRT_API mcrt_status mcrt_framebuffer_read_adaptive(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                    uint64_t* needed);
/* Copies device -> host (RGBA32F, W*H*4 floats).  which: 0 radiance, 1 weighted sum, 2 image,
 * 3 display image (mcrt_postprocess, mcrt_denoise_guided). */
MCRT_API mcrt_status mcrt_framebuffer_read(mcrt_framebuffer fb, int which, float* host_rgba);
/* Radiance of frame k (0 <= k < count) of the last mcrt_render_frames call (k = 0: the same as
 * mcrt_framebuffer_read 0): the reference's RadianceBufferCL of that frame
 * (RTPathTracingPass.cpp:106), RGBA32F, W*H*4 floats. */
MCRT_API mcrt_status mcrt_framebuffer_read_frame(mcrt_framebuffer fb, int32_t k, float* host_rgba);
/* Device-to-device copy of one frame-buffer array into caller memory (e.g. a torch/RCCL
 * buffer for the multi-GPU reduce): which 0 radiance (float4), 1 weighted sum (float4),
 * 2 image (float4), 3 weight sum (float).  Enqueued on the context stream, ordered after the
 * last render; the radiance copy keeps that frame's slot from taking a new frame until read. */
MCRT_API mcrt_status mcrt_framebuffer_copy_device(mcrt_framebuffer fb, int which, void* d_dst);
/* mcrt_framebuffer_copy_device 0 for frame k (0 <= k < count) of the last mcrt_render_frames call:
 * W*H float4, enqueued on the context stream with the same ordering and slot hold. */
MCRT_API mcrt_status mcrt_framebuffer_copy_device_frame(mcrt_framebuffer fb, int32_t k, void* d_dst);
/* Inverse for multi-GPU: overwrite the weighted sums (float4) and weights (float) from device
 * memory (after a reduce) and recompute the image = sum / weight on the device. */
MCRT_API mcrt_status mcrt_framebuffer_set_accumulation(mcrt_framebuffer fb, const void* d_wsum, const void* d_wts);
/* Tile split (mcrt_frame_params.num_bands > 1), end of job, without full-frame copies: pack this
 * rank's own rows of the accumulators (its bands of the last render, local 8-row block tb at rows
 * 8 tb .. 8 tb + 7) into d_dst, one row = W x float4 weighted sum then W x float weight (5 W
 * floats), straight from the frame buffer.  Rows past the rank's last row are left untouched.
 * Enqueued on the context stream after the last accumulate.  Replaces the all-reduce of the two
 * accumulation buffers the reference would need (RTPathTracingPass.cpp:99-117 accumulates on one
 * device) with the gather of mcrt.dist.gather_bands_fb. */
MCRT_API mcrt_status mcrt_framebuffer_bands_pack(mcrt_framebuffer fb, void* d_dst);
/* On the gathering rank: d_recv = num_bands chunks of max_rows packed rows (chunk r = rank r's
 * mcrt_framebuffer_bands_pack output); every other rank's rows are written into this frame
 * buffer's accumulators in place and the image = sum / weight is recomputed (the same division
 * as mcrt_framebuffer_set_accumulation).  Enqueued on the context stream. */
MCRT_API mcrt_status mcrt_framebuffer_bands_unpack(mcrt_framebuffer fb, const void* d_recv, int32_t max_rows);
/* Band geometry of the last render, for a C++ host sizing the gather of the packed rows:
 * max_rows = the largest rank's row count (whole 8-row blocks; one packed chunk = max_rows x 5 W
 * floats, the max_rows argument of mcrt_framebuffer_bands_unpack), and the num_bands / band_index
 * the frame was rendered with.  Any output pointer may be NULL. */
MCRT_API mcrt_status mcrt_framebuffer_band_layout(mcrt_framebuffer fb, int32_t* max_rows, int32_t* num_bands,
                                                  int32_t* band_index);
/* Per-frame path statistics of the last render (paths, closest rays, any rays, ...). */
MCRT_API mcrt_status mcrt_framebuffer_stats(mcrt_framebuffer fb, int64_t* closest_rays, int64_t* any_rays,
                                            int64_t* shaded_paths);
/* Queue sizes of the last PT render, per bounce b < max: shadow[b] = shadow rays queued by
 * bounce b's shading, extension[b] = extension rays queued for bounce b+1. */
MCRT_API mcrt_status mcrt_framebuffer_queue_counts(mcrt_framebuffer fb, int32_t* shadow, int32_t* extension, int max);
/* Shadow rays of the last PT render answered by their occluder hint, per bounce b < max (the rest
 * walked the tree; the reference walks every one, intersect_bvh2_lds.cl:229-363, with the same
 * answers).  Counted while mcrt_ctx_set_profiling(ctx, 2) is on; zero otherwise, when the hints are
 * off (MCRT_SHADOW_HINTS=0) or the structure is two-level. */
MCRT_API mcrt_status mcrt_framebuffer_hint_counts(mcrt_framebuffer fb, int32_t* hits, int max);
/* Extension rays of the last PT render whose closest-hit walk over the compact records ended on a
 * near tie and was repeated on the exact 64-B records (so the reference's visit order resolves it),
 * per bounce b < max (rays traced for bounce b + 1).  Counted while mcrt_ctx_set_profiling(ctx, 2)
 * is on; zero otherwise and with MCRT_QUANT_NODES=0. */
MCRT_API mcrt_status mcrt_framebuffer_retrace_counts(mcrt_framebuffer fb, int32_t* retraces, int max);
/* Diagnostics: with MCRT_WAVE_CLOCK=1 in the environment, the last PT call's launches record each
 * workgroup's (start, end) on the constant 100-MHz clock (s_memrealtime, low 32 bits); which = 0
 * camera launch, 1 bounce-0 shadow + extension launch (extension workgroups), 2 last-bounce shadow
 * launch.  Copies min(max_blocks, *blocks) pairs; (0, 0) = a workgroup that had no work.  While
 * MCRT_WAVE_CLOCK is set every render keeps ONE frame in flight (the buffers are per frame buffer). */
MCRT_API mcrt_status mcrt_framebuffer_wave_clock(mcrt_framebuffer fb, int which, uint32_t* host_out, int64_t max_blocks,
                                                 int64_t* blocks);
/* Host copy of a ray queue of the last render (the state the reference keeps in its
 * per-pixel trace_shadowRays / trace_rays / throughput buffers):
 *   which 0: shadow queue of the last bounce    -- origin.xyz|tmax, dir.xyz|pixel(int bits), throughput*L
 *   which 1: last extension queue (bounce D-2)  -- origin.xyz|pixel(int bits), dir.xyz|bsdf flags, throughput
 * Writes min(count, max_records) records as three float4 arrays back to back
 * (dst = [a0..a(n-1) | b0.. | c0..], 48 * max_records bytes) and the full count.
 * The ORDER of the records is not deterministic: the shading kernels append them per workgroup
 * through LDS atomics (grouped by octant x dominant axis), so two runs hold the same set of
 * records in different orders.  Every record carries its pixel, and the radiance does not depend
 * on the order; compare queues as sets (e.g. sorted by pixel). */
MCRT_API mcrt_status mcrt_framebuffer_read_queue(mcrt_framebuffer fb, int which, void* host_dst,
                                                 int64_t max_records, int32_t* count);
/* Host copy of the BDPT state of the last BDPT frame (the reference keeps it in RTBDPTPass's
 * m_cameraVertices / m_lightVertices / vertex-count buffers, RTBDPTPass.cpp:456-470):
 *   which 0: camera vertices, (D+2) depths x 8 planes of float4 x W*H (layout: mcrt_bdpt.hip)
 *         1: light vertices, (D+1) depths x 8 planes     2/3: camera / light vertex counts (int32 x W*H)
 *         4: own-strategy contributions ((C-D) planes)   5: persistent s=1 sampled light vertices (D planes)
 *         6: light-tracing (t=1) splat sums of the frame (float4 x W*H)
 * Copies min(bytes, size) bytes; *needed = the array's size (host_dst may be NULL to query it). */
/* Band-split BDPT (num_bands > 1): the frame's light-tracing splats land in any pixel, so the ranks
 * exchange them once per frame (the reference's ConnectVertices atomics + CopyBuffer,
 * BDPT.cl:671-913).  The splats are laid out RANK-MAJOR: `chunks` (= num_bands) chunks of
 * `chunk_pixels` pixels of MCRT_SPLAT_CHANNELS (3) floats -- r, g, b, as the reference's splat
 * buffer (BDPT.cl:654-669, 888-899) -- chunk r holding the rows of rank r's bands in its own tile order (zero
 * past its last row), so ONE reduce-scatter hands each rank exactly its rows' sums:
 *   mcrt_bdpt_splat_layout   the chunk geometry of the last frame's band split;
 *   mcrt_bdpt_splats_copy    this rank's splats, rank-major, into d_dst (chunks x chunk_pixels
 *                            x 3 floats of device memory), ENQUEUED on the frame's stream
 *                            (mcrt_framebuffer_stream): order the collective after it there (no
 *                            host synchronisation, so frames in flight keep overlapping);
 *   mcrt_bdpt_gather         completes the rank's bands with d_own_chunk = chunk band_index of the
 *                            ranks' summed buffers (chunk_pixels x 3 floats; NULL: the rank's own splats
 *                            in its natural layout -- a 1-rank check).  It reads d_own_chunk on the
 *                            frame's stream; a later mcrt_bdpt_splats_copy waits for it.
 * Rendering or accumulating in between fails with MCRT_ERROR_NOT_READY.  With no frame pending (a
 * light-less scene, a whole-image frame) the copy writes zeros and the gather does nothing. */
#define MCRT_SPLAT_CHANNELS 3
MCRT_API mcrt_status mcrt_bdpt_splat_layout(mcrt_framebuffer fb, uint64_t* chunk_pixels, int32_t* chunks);
/* The HIP stream (hipStream_t) the last frame of fb was enqueued on (its frame slot's). */
MCRT_API mcrt_status mcrt_framebuffer_stream(mcrt_framebuffer fb, void** stream);
MCRT_API mcrt_status mcrt_bdpt_splats_copy(mcrt_framebuffer fb, void* d_dst);
MCRT_API mcrt_status mcrt_bdpt_gather(mcrt_framebuffer fb, const void* d_own_chunk);
/* Sparse splat exchange (the band split's alternative to the dense rank-major buffer above): only a
 * few per cent of a rank's paths splat into another rank's rows (San-Miguel proxy: ~2.6 %), so the
 * ranks exchange those splats as records -- 4 floats: the target path index (k * W*H + pixel, int
 * bits), r, g, b -- with one all-to-all instead of reducing whole frames:
 *   mcrt_framebuffer_set_splat_exchange  MCRT_SPLAT_EXCHANGE_SPARSE before rendering (DENSE: default);
 *                            k_bdpt_vis then adds the rank's own-row splats in place and lists the rest;
 *   mcrt_bdpt_splats_sparse  counts[r] = records for rank r (counts[band_index] = 0), SYNCHRONOUS up to
 *                            the frame's visibility pass (the sizes are host data for the all-to-all);
 *                            when d_dst holds capacity >= sum(counts) records of device memory it also
 *                            groups the records by rank into it, enqueued on the frame's stream (else
 *                            counts only: grow the buffer and call again);
 *   mcrt_bdpt_gather_sparse  adds the `records` received records (targets in this rank's rows) and
 *                            completes the rank's bands, on the frame's stream.
 * The frame equals the dense exchange's (and one GPU's) up to the order of the splat sums. */
#define MCRT_SPLAT_EXCHANGE_DENSE 0
#define MCRT_SPLAT_EXCHANGE_SPARSE 1
MCRT_API mcrt_status mcrt_framebuffer_set_splat_exchange(mcrt_framebuffer fb, int32_t mode);
MCRT_API mcrt_status mcrt_bdpt_splats_sparse(mcrt_framebuffer fb, void* d_dst, int64_t capacity, int64_t* counts,
                                             int32_t num_counts);
MCRT_API mcrt_status mcrt_bdpt_gather_sparse(mcrt_framebuffer fb, const void* d_recv, int64_t records);
MCRT_API mcrt_status mcrt_framebuffer_read_bdpt(mcrt_framebuffer fb, int which, void* host_dst, uint64_t bytes,
                                                uint64_t* needed);

/* ------------------------------------------------------------------------ */
/* Host helpers                                                              */
/* ------------------------------------------------------------------------ */
/* The reference host's RTPinholeCamera (kernel_data.h:246-264), bit for bit: CameraComponent
 * (source/engine/camera/CameraComponent.cpp:61-134: glm::perspective -- left-handed, the vendored
 * glm forces GLM_FORCE_LEFT_HANDED -- and the view matrix from the transform's rotation columns
 * right / up / look), RTUtil::screenToRay for the four image corners at the near plane
 * (APP/raytracing/util/RTUtil.cpp:9-41, RTPrimaryRaysPass.cpp:81-104) with pixel_offset = the
 * TAA jitter in pixels (GI.filterSettings.curPixelOffset), worldToClip = viewProj (row major) and
 * the z = 1 image-plane area of RTBDPTPass.cpp:158-166.  fov_y is the value the reference hands to
 * glm::perspective, i.e. RADIANS (note: PathTracingApp.cpp:387 passes 45.0f, so the reference
 * app's vertical field of view is 45 rad mod pi ~ 58.3 degrees).  float32 in glm's operation
 * order (mcrt_camera.cpp), pinned against the reference's own glm (tests/test_camera_cpu.py). */
MCRT_API mcrt_status mcrt_make_pinhole_camera_axes(const float pos[3], const float right[3], const float up[3],
                                                   const float look[3], float fov_y, float near_z, float far_z,
                                                   uint32_t width, uint32_t height, const float pixel_offset[2],
                                                   mcrt_camera* out);
/* Convenience form: a look-at camera (Camera::lookAt, source/engine/camera/Camera.cpp:58-63, with
 * forward = target - position) and the field of view in DEGREES (glm::radians); otherwise
 * mcrt_make_pinhole_camera_axes. */
MCRT_API mcrt_status mcrt_make_pinhole_camera(const float pos[3], const float forward[3], const float up[3],
                                              float fov_y_deg, float near_z, float far_z,
                                              uint32_t width, uint32_t height,
                                              const float pixel_offset[2], mcrt_camera* out);
/* TAA jitter of frame `frame` (PathTracingApp.cpp:208-215): pixel offset =
 * (lerp(-rx, rx, sobol(frame, 0)), lerp(-ry, ry, sobol(frame, 1))), Sampler::sobolSample with
 * scramble 0 over the 1024 x 52 g_SobolMatrices32 (the scene's sobol_matrices); radius = the
 * reconstruction filter radius (GI.filterSettings.radius). */
MCRT_API mcrt_status mcrt_taa_pixel_offset(const uint32_t* sobol_matrices, uint32_t frame, float radius_x,
                                           float radius_y, float out[2]);
/* Library version / build string. */
MCRT_API const char* mcrt_version(void);

#ifdef __cplusplus
}
#endif

#ifdef __cplusplus
static_assert(sizeof(mcrt_shape) == 160, "RTShape is 160 B");
static_assert(sizeof(mcrt_material) == 128, "RTMaterial is 128 B");
static_assert(sizeof(mcrt_light) == 80, "RTLight is 80 B");
static_assert(sizeof(mcrt_camera) == 176, "RTPinholeCamera is 176 B");
static_assert(sizeof(mcrt_texture_desc) == 16, "TextureDesc2D is 16 B");
static_assert(sizeof(mcrt_ray) == 48, "RR ray is 48 B");
static_assert(sizeof(mcrt_intersection) == 32, "RR Intersection is 32 B");
static_assert(sizeof(mcrt_filter) == 56, "RTFilterProperties (device) is 56 B");
static_assert(offsetof(mcrt_material, uber_roughness) == 80, "roughness @80");
static_assert(offsetof(mcrt_material, uber_normalMapId) == 96, "normalMapId @96");
static_assert(offsetof(mcrt_material, uber_iorTexId) == 96 + 28, "the eight texture ids are consecutive: iorTexId @124");
static_assert(offsetof(mcrt_camera, width) == 160, "width @160");
static_assert(offsetof(mcrt_filter, radius) == 8, "radius @8 (device)");
static_assert(offsetof(mcrt_filter, mitchellB) == 16, "B @16 (device)");
static_assert(offsetof(mcrt_filter, pixelOffset) == 40, "pixelOffset @40 (device)");
#else
_Static_assert(sizeof(mcrt_shape) == 160, "RTShape is 160 B");
_Static_assert(sizeof(mcrt_material) == 128, "RTMaterial is 128 B");
_Static_assert(sizeof(mcrt_light) == 80, "RTLight is 80 B");
_Static_assert(sizeof(mcrt_camera) == 176, "RTPinholeCamera is 176 B");
_Static_assert(sizeof(mcrt_ray) == 48, "RR ray is 48 B");
_Static_assert(sizeof(mcrt_intersection) == 32, "RR Intersection is 32 B");
_Static_assert(sizeof(mcrt_filter) == 56, "RTFilterProperties (device) is 56 B");
#endif

#endif /* MCRT_CAPI_H */
