// mcrt_host.h -- the host runtime's objects behind the opaque handles of include/mcrt_capi.h, and
// the few helpers that host code in another file may call.  Not part of the ABI.
//
// This is the boundary between the host files.  mcrt_capi.cpp holds the context and the helpers
// declared below.  A subsystem with entry points of its own (mcrt_denoise.hip, mcrt_adaptive.hip,
// mcrt_accel.cpp, mcrt_bdpt_host.cpp, mcrt_pt_host.cpp, mcrt_film.hip, mcrt_probe.hip,
// mcrt_scene.hip, mcrt_query.hip, mcrt_aov.hip) includes this header, reaches the rest of the
// runtime through what is declared here and nothing else, and keeps its state in one struct that
// only it names the fields of: DenoiseState, AdaptiveState, BdptState and the frame slots (FrameSlot,
// mcrt_pt_host.cpp) held by the frame buffer, AccelState held by the scene, and the scene itself
// (mcrt_scene_s, mcrt_scene.hip; its `ctx` is everyone's, `accel` mcrt_accel.cpp's).  Four have none:
// the probes, the ray queries and the AOV pass keep no state, and the film's planes (wsum, wts,
// image, denoised, display, bands) are plain fields of the frame buffer, which the integrators'
// hosts and the denoiser read; mcrt_film.hip creates, zero-fills, reads back, packs and
// post-processes them.  It compiles as plain C++ (-x c++ -D__HIP_PLATFORM_AMD__) and inside a .hip
// translation unit.
#pragma once
#include <climits>
#include <cstddef>
#include <string>
#include <vector>

#include "mcrt_devbuf.h"
#include "mcrt_internal.h"

using mcrt::DevBuf;

#define MCRT_ATROUS_MAX_LEVELS 8

enum KernelId {
    K_PRIMARY, K_SHADE0, K_SHADEN, K_SHADOW, K_EXTEND, K_ACCUM, K_TRACE_CLOSEST, K_TRACE_ANY,
    K_BDPT_START, K_BDPT_VERTEX, K_BDPT_CONNECT, K_BDPT_VIS, K_BDPT_GATHER, K_SHADOW_EXTEND,
    K_GUIDES, K_MOMENTS, K_ATROUS_PREP,
    K_ATROUS,   // one entry per level: K_ATROUS + i is the launch of step 2^i
    K_TEMPORAL = K_ATROUS + MCRT_ATROUS_MAX_LEVELS, K_TEMPORAL_VAR, K_GUIDES_MOTION, K_TEMPORAL_MOTION,
    K_TILE_ERROR, K_TILE_LIST,
    K_REFIT, K_REFIT_QNODES,   // mcrt_accel_refit: the refit launch, the compact conversion
    K_COUNT
};

struct mcrt_ctx_s {
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    int numCUs = 256;
    bool profiling = false;
    bool countHints = false;   // mcrt_ctx_set_profiling(2): occluder-hint counters (one atomic per wave)
    int* dFlags = nullptr;          // device flags: [0] traversal-stack overflow (mcrt_traverse.h), set by any launch
    std::string error;
    struct Pending {
        int kernel;
        hipEvent_t a, b;
        const int* countDev;   // device counter holding the item count (or nullptr)
        const int* countDev2;  // a second counter added to it (fused launches), or nullptr
        int64_t items;
    };
    std::vector<Pending> pending;
    double totalMs[K_COUNT] = {};
    int64_t launches[K_COUNT] = {};
    int64_t items[K_COUNT] = {};
};

// The acceleration structure of a scene (mcrt_accel.cpp), written by mcrt_accel_build's commit and
// mcrt_accel_update_transforms.  Only mcrt_accel.cpp names its fields; the rest of the runtime
// goes through the views and accessors declared below.
struct AccelState {
    DevBuf<float4> dNodes;     // 4 float4 per record; empty: no structure
    mcrt::TreeInfo tree;       // counts, depth, layout, builder, world box
    // compact records of the flat tree (TraceCtx::qnodes; mcrt::build_qnodes), empty when not built
    DevBuf<float4> dQNodes;
    int qOrder = 0;   // their order (QORDER_*), for the refit's offsets
    uint32_t qRoot = 0;
    bool packets = false;      // coherent launches as wave packets
    double buildMs = 0.0;
    // traversal scratch
    DevBuf<uint32_t> dSpill;   // spillCap words per ray (ensure_spill)
    int spillCap = 0;
    DevBuf<int> dScratch;      // work counters for API queries
    // occluder hints of the shadow rays after bounce 0, by origin cell (TraceCtx::hint, flat trees):
    // allocated on the first shadow launch that uses hints (ensure_hint_cell), 2^hintBits words
    DevBuf<uint32_t> dHintCell;
    int hintBits = 0;
    bool hintAllocFailed = false;   // no memory for the table: hints stay off for this structure
    // transform updates (mcrt_accel_update_transforms): the options of the last mcrt_accel_build
    // (without its world_to_local pointer), the two-level build's refit state, the device top-level
    // builder's arrays (made by the first update that takes the device path)
    mcrt_accel_opts lastOpts = {};
    bool haveOpts = false;
    mcrt::Bvh2lTop top2l;
    mcrt::TopBuildDev* topDev = nullptr;
    int updatePath = 0;
    double updateMs = 0.0;
    // refit of a flat structure (mcrt_accel_refit): made by the structure's first refit, freed by
    // drop(); refits after the first allocate nothing
    DevBuf<int> refitParent;       // per record: its parent, -1 for the root
    DevBuf<int> refitArrive;       // per record: arrivals of the running refit
    DevBuf<uint32_t> refitQOff;    // per record: offset of its compact record (with dQNodes only)
    DevBuf<int> refitFlag;         // the converter's "a box the bytes cannot bound"
    ~AccelState() { mcrt::top_build_destroy(topDev); }   // the buffers free themselves
};

// The scene tables (mcrt_scene.hip).  Only mcrt_scene.hip names the fields, apart from `ctx` and
// `accel`; the rest of the runtime goes through the views and readers declared below.
struct mcrt_scene_s {
    mcrt_ctx ctx = nullptr;
    // host copies needed for the BVH build and dynamic updates
    std::vector<mcrt_shape> shapes;
    std::vector<uint32_t> indices;
    std::vector<mcrt_float4> positions;
    // device arrays
    DevBuf<mcrt_shape> dShapes;
    DevBuf<uint32_t> dIndices;
    DevBuf<float4> dPositions;
    DevBuf<float2> dUvs;
    DevBuf<float4> dNormals;
    DevBuf<mcrt_texture_desc> dTextures;
    DevBuf<uint8_t> dTexData;
    DevBuf<uint32_t> dSobol;
    DevBuf<mcrt_light> dLights;
    DevBuf<mcrt_material> dMaterials;
    DevBuf<float4> dSurf;           // surface records (SceneArgs::surf), 128 B per distinct mesh triangle
    DevBuf<uint32_t> dSurfBase;     // per shape: its first surface record
    DevBuf<uint32_t> dSurfMeshes;   // startIdx | startVertex | base per distinct mesh (kept: vertex updates relaunch over it)
    uint32_t surfMeshes = 0, surfRecords = 0;   // distinct meshes with triangles, and the records of all
    // mcrt_scene_update_vertices_device wrote dPositions alone: `positions` is downloaded by the
    // next route that reads it (mcrt::host_positions)
    bool positionsStale = false;
    uint32_t numLights = 0, numMaterials = 0, numTextures = 0;
    bool hasSobol = false;
    AccelState accel;   // the acceleration structure and what is sized by it (mcrt_accel.cpp)
    // previous poses (mcrt_scene_motion_snapshot): one record per shape, allocated by the first
    // snapshot; only k_guides_motion receives it
    DevBuf<PrevPose> dPrevPose;
};

// The small device block of a frame slot.  Its head, the per-bounce counters of a PT call, is what
// the call zeroes and the read-backs copy; the batch's cameras (mcrt_render_frames) and filters
// (mcrt_accumulate_frames) follow.  The kernels see these addresses, so the byte layout is pinned.
struct SlotCounts {
    int shadow[MCRT_MAX_BOUNCES];     // shadow rays queued by bounce b
    int ext[MCRT_MAX_BOUNCES];        // extension rays queued by bounce b, traced for bounce b + 1
    int hintHits[MCRT_MAX_BOUNCES];   // of shadow[b], answered by their occluder hint (profiling level 2)
    int retraces[MCRT_MAX_BOUNCES];   // of ext[b], walks repeated on the exact records (profiling level 2)
};
struct SlotBlock {
    SlotCounts n;
    mcrt_camera cam[MCRT_MAX_BATCH_FRAMES];
    mcrt_filter filt[MCRT_MAX_BATCH_FRAMES];
    char slack[1536];
};
static_assert(MCRT_MAX_BOUNCES == 32 && sizeof(SlotCounts::shadow) == sizeof(int) * MCRT_MAX_BOUNCES, "one count per bounce");
static_assert(offsetof(SlotCounts, shadow) == 0 && offsetof(SlotCounts, ext) == 128 && offsetof(SlotCounts, hintHits) == 256 &&
                  offsetof(SlotCounts, retraces) == 384 && offsetof(SlotBlock, n) == 0,
              "the four counter arrays");
static_assert(offsetof(SlotBlock, cam) == 512 && sizeof(SlotCounts) == 512, "cameras from byte 512 (176 B each)");
static_assert(offsetof(SlotBlock, filt) == 512 + 176 * MCRT_MAX_BATCH_FRAMES, "then the filters");
static_assert(sizeof(SlotBlock) == 512 + 176 * MCRT_MAX_BATCH_FRAMES + sizeof(mcrt_filter) * MCRT_MAX_BATCH_FRAMES + 1536,
              "the block's size");

// One frame in flight: the per-frame buffers of mcrt_render_frame(s), its own stream and
// spill columns.  Frame i renders in slot i mod S on that slot's stream while mcrt_accumulate
// runs on the context stream in frame order (it waits for the slot's `done` event and records
// `free` after reading the slot's radiance), so S frames overlap on the GPU -- each frame's
// arithmetic and the per-pixel accumulation order are unchanged, so the image is the same bit
// for bit.  Small per-rank frames (tile split over many GPUs) do not fill 256 CUs alone.
// The slots are mcrt_pt_host.cpp's: it allocates and frees them, chooses one per call, and alone
// names the queues, the block, the spill columns, the tile order, the suspended walks and -- apart
// from ctx_wait_slots -- the events.  mcrt_film.hip reads radiance and lastBatch, mcrt_capi.cpp stream;
// mcrt_bdpt_host.cpp, handed a ready slot by the entry function, also writes radiance, the block's
// cameras, lastMaxDepth and lastPixels and records `done` after a gather; everything else borrows
// the current slot through borrow_camera_hits and release_slot below.
struct FrameSlot {
    DevBuf<float4> radiance;
    DevBuf<float4> hitsP;        // primary hits (mcrt_shading.h hitSlot)
    DevBuf<float4> hitsE;        // extension hits by queue slot
    DevBuf<float4> eO[2], eD[2], eT[2];
    DevBuf<float4> sO, sD, sL;
    DevBuf<SlotBlock> block;     // one: counters, cameras, filters
    DevBuf<uint32_t> spill;      // per-ray traversal spill columns of this slot's launches
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;   // recorded after the slot's last render
    hipEvent_t free = nullptr;   // recorded on the context stream after the slot's buffers were last read
    int lastMaxDepth = 0;
    int64_t lastPixels = 0;
    int lastBatch = 1;           // frames of the slot's last render (mcrt_render_frames)
    int frames = 1;              // radiance / primary-hit planes of W*H allocated (batch capacity)
    size_t queueCap = 0;         // entries of each ray-queue buffer
    // longest-first tile order (FrameArgs::tileOrder): the camera-wave cost of each tile recorded by
    // this slot's last call, and the order made from it; stream-ordered on the slot's stream
    DevBuf<uint32_t> tileCost, tileOrder;   // the same size
    int costTiles = 0;           // tiles of the recorded costs (0: none)
    // suspended extension walks (TraceCtx::walkCap): MCRT_SUSPEND_F4 float4 per queue entry, and
    // one count per bounce (zeroed per call)
    DevBuf<float4> suspend;
    DevBuf<int> suspendCnt;
};

// Per-frame BDPT arrays (RTBDPTPass::createBuffers, RTBDPTPass.cpp:442-479), one set per frame
// slot so BDPT frames overlap like PT frames; layouts in mcrt_bdpt.hip.
struct BdptSet {
    DevBuf<float4> camV, lightV, slots, splat;
    DevBuf<int> camCount, lightCount;
    DevBuf<int> bdptCounters;    // 64 ints: the queue counters (BDPT_CNT_*)
    DevBuf<float4> bqO[2], bqD[2], bqT[2], bHits;
    DevBuf<float4> cO, cD, cL;   // connection queue
    DevBuf<uint32_t> spill;      // traversal spill columns of this set's launches
    // the light-start queue's sort (mcrt::bdpt_light_sort): keys, sorted keys, slots, permutation
    DevBuf<uint32_t> lkey, lkey2, lslot, lperm;
    // the traced bounce queues' sort (same routine; k_bdpt_vertex's keys over 2 N slots)
    DevBuf<uint32_t> ekey, ekey2, eslot, eperm;
    DevBuf<uint8_t> sortTmp;
    int frames = 0;              // batch frames the per-frame arrays hold (plane stride N x frames)
    // plane stride and band (rows, count, index) whose depth-0 frame-invariant planes k_bdpt_start
    // wrote for every path of the band
    size_t constStride = 0;
    int constBand[3] = {0, 0, -1};
    // band split, sparse splat exchange: the splats landing in other ranks' rows (BdptArgs::splatList)
    // and 128 ints of grouping scratch (per-owner counts, cursors)
    DevBuf<float4> splatList;
    DevBuf<int> splatAux;
    // suspended closest-hit walks (TraceCtx::walkCap): MCRT_SUSPEND_F4 float4 per queue entry, one
    // count per traced queue (zeroed per call)
    DevBuf<float4> suspend;
    DevBuf<int> suspendCnt;
};

// The bidirectional integrator's host state (mcrt_bdpt_host.cpp), allocated by the first BDPT frame
// of a max depth.  Only mcrt_bdpt_host.cpp names its fields; the rest of the runtime goes through
// the functions declared below.  The per-frame arrays exist once per frame slot; the
// sampled-light-vertex planes carry state from frame to frame (BDPT.cl:585), so they are shared and
// the connect launches stay in frame order.
struct BdptState {
    int depth = 0;                 // max depth the arrays are sized for (0: none)
    BdptSet set[MCRT_MAX_FRAMES_IN_FLIGHT];
    hipEvent_t connect = nullptr;  // recorded after the last enqueued frame's connect launch
    DevBuf<float4> sampLight;      // the sampled-light-vertex planes (D x N)
    int batch = 1;                 // frames of the last BDPT call (plane stride N x batch)
    bool oneSet = false;           // a second set did not fit in HBM: BDPT frames use slot 0 only
    bool pendingGather = false;    // band-split frame waiting for the ranks' summed splats
    int splatExchange = MCRT_SPLAT_EXCHANGE_DENSE;   // mcrt_framebuffer_set_splat_exchange
    int cur = 0;                   // the set of the last BDPT call, as mcrt_framebuffer_s::cur is its slot
    // frees the sets, the shared planes and the event (the next frame allocates for its depth);
    // the caller has finished every stream that may use them
    void reset();
    ~BdptState() { reset(); }
};
// strategies (s, t) of a path of max depth D (RTBDPTPass.cpp:404-408)
inline int bdpt_max_connections(int D) { const int t = D + 2; return t * (t + 1) / 2 - 2; }

// The denoiser's state (mcrt_denoise.hip), every plane allocated on first use.
struct DenoiseState {
    // Guided denoiser (mcrt_denoise_guided): the guides of the camera-ray hits, the luminance
    // moments k_moments keeps next to the image, and two scratch colour / variance planes the
    // levels ping-pong between (fb->denoised stays mcrt_postprocess's)
    DevBuf<float4> guideNormal;      // (n, n . (P - cam.pos))
    DevBuf<float4> guideAlbedo;      // (Kd, |P - cam.pos|), -1 on a miss
    bool haveGuides = false;
    DevBuf<float2> moments;          // (sum l, sum l*l)
    bool momentsOn = false;
    int momentFrames = 0;            // frames in the moments (host side; restarts at frame_index 0)
    DevBuf<float4> atrousC[2];
    DevBuf<float> atrousV[2];
    int filteredVar = -1;            // which of atrousV holds the last level's variance, -1 before a denoise
    // Temporal history (mcrt_temporal_accumulate).  Colour, moments and the previous normal-plane
    // exist twice: k_temporal reads set tCur and writes the other, then tCur flips, so set tCur is
    // always what the next accumulate (and mcrt_framebuffer_read_temporal) reads.
    DevBuf<float4> tColour[2];       // integrated colour in filter space, alpha of the current image
    DevBuf<float4> tMoments[2];      // (mu1, mu2, N, z)
    DevBuf<float4> tNormal[2];       // the guide record the pixel had when written
    DevBuf<float> tVar;              // the variance handed to the filter
    int tCur = 0;
    bool tHaveHistory = false;       // false: the next accumulate starts without history
    bool tAccumulated = false;       // an accumulate has run: the planes feed mcrt_denoise_guided_temporal
    bool tFedBack = false;           // the colour history already holds a filtered level of this accumulate
    int tDemod = 0;                  // demodulate_albedo of the last accumulate
    mcrt_camera tPrevCam = {};       // camera of the history planes
    // Per-object motion (mcrt_render_guides_motion); the planes belong to one set of guides, so
    // whatever replaces the guides alone clears haveMotion
    DevBuf<float4> motion;           // (P_prev - P, flag)
    DevBuf<float4> motionNormal;     // (n_prev, 0) where flag is 1
    bool haveMotion = false;
};

// Adaptive sampling (mcrt_adaptive.hip): the tiles a PT call renders and an accumulate touches.  A
// tile is 8x8 pixels, tile t = row-block (t / tilesX), column-block (t % tilesX) of the whole image
// (tilePixel's numbering without a band split).  Only mcrt_adaptive.hip names the fields; the path
// tracer and the denoiser go through the adaptive_* functions declared below.
struct AdaptiveState {
    bool on = false;
    mcrt_adaptive_params p = {};
    int numTiles = 0;
    DevBuf<uint32_t> tileCount;   // samples accumulated per tile
    DevBuf<float> tileErr;        // k_tile_error's result per tile (+inf below 2 samples)
    // the active tiles, ascending; entries from listLen to the buffer's end hold numTiles, so a launch
    // rounded up to whole workgroups (k_shade0: 8 waves) finds no real tile in its surplus waves
    DevBuf<uint32_t> list;        // numTiles rounded up to 8, and 8 more
    DevBuf<int> listLenDev;       // k_tile_list's count, read back by mcrt_adaptive_update
    int listLen = 0;
    int frames = 0;               // frames accumulated since the last reset
    int pending = 0;              // frames rendered and not yet accumulated
};

struct mcrt_framebuffer_s {
    mcrt_ctx ctx = nullptr;
    uint32_t W = 0, H = 0;
    size_t N = 0;
    std::vector<FrameSlot> slot;   // slot[0] always allocated; others on first use
    int cur = 0, next = 0;         // slot of the last rendered frame / of the next one
    int framesInFlight = 0;        // 0 = auto (mcrt_framebuffer_set_frames_in_flight)
    DevBuf<float4> wsum;
    DevBuf<float> wts;
    DevBuf<float4> image;
    DevBuf<float4> denoised;     // RTDenoisePass output (persistent: the reference keeps its image)
    DevBuf<float4> display;      // post-processed image (mcrt_postprocess)
    DevBuf<uint32_t> hintPix;    // occluder hint of each pixel's bounce-0 shadow ray (TraceCtx::hint)
    FrameArgs bands{};      // band layout of the last mcrt_render_frame (used by mcrt_accumulate)
    bool haveBands = false;
    // diagnostics (MCRT_WAVE_CLOCK=1): per-workgroup (start, end) clocks of the last PT call's camera,
    // shadow+extension and last shadow launches (mcrt_framebuffer_wave_clock)
    DevBuf<uint32_t> waveClk[3];   // 2 words per workgroup
    int lastIntegrator = MCRT_INTEGRATOR_PT;
    BdptState bd;
    DenoiseState dn;
    AdaptiveState ad;
};
// The slot of the last rendered frame: what the read-back entry points show.  After a failed
// regrow its buffers are empty, never stale.
inline FrameSlot& cur_slot(mcrt_framebuffer fb) { return fb->slot[fb->cur]; }

// What host code in another file may call.  First mcrt_capi.cpp's helpers
namespace mcrt {
// records msg as the thread's and the context's (may be NULL) last error; returns code
mcrt_status fail(mcrt_ctx ctx, mcrt_status code, const std::string& msg);
// Reports and clears the device-side error flags kernels raised since the last check (a traversal
// stack overflow); call after a synchronisation
mcrt_status check_device_flags(mcrt_ctx ctx);
// An integer environment variable clamped to lo .. hi, or `def` when it is not set.
int env_int(const char* name, int def, int lo = INT_MIN, int hi = INT_MAX);
// Host reads and context-stream work that touch the slots: all slot streams first.
hipError_t fb_sync(mcrt_framebuffer fb);
// Makes the context stream wait for every slot's last render (work on the context stream
// that reads or rewrites slot buffers: BDPT, AOVs, device copies).
void ctx_wait_slots(mcrt_framebuffer fb);
bool frame_args(mcrt_framebuffer fb, const mcrt_frame_params* p, FrameArgs& f, std::string& err);
// Lanes of the 8x8 tiles covering the image (>= N): the packed camera-hit slots of a frame and one
// start-queue entry per lane of BDPT's tile walk
inline size_t tile_lanes(mcrt_framebuffer fb) { return (size_t)((fb->W + 7) / 8) * ((fb->H + 7) / 8) * 64; }
// Stop rule of the extension rays' compact walks (TraceCtx::walkCap) for a call of `paths` paths:
// when the tree has compact records and the call is large enough (MCRT_WALK_CAP, MCRT_WALK_MIN_PATHS),
// sizes `suspend` for `entries` queue entries, zeroes the `counts` suspend counters on st and fills
// c.walkCap / walkLanes / suspend; otherwise c.walkCap stays 0.  Whether the rule is wanted at all,
// and for which launches, is the caller's.
hipError_t walk_rule(TraceCtx& c, int64_t paths, DevBuf<float4>& suspend, DevBuf<int>& suspended, int counts,
                     size_t entries, hipStream_t st);
// mcrt_scene.hip: the scene tables, as the rest of the runtime reads them
// The geometry the builders and the refit read (mcrt_accel.cpp): the host shapes and indices, the
// device shapes, indices and positions.  The host pointers hold until the next call that replaces shapes.
struct SceneGeometry {
    const mcrt_shape* shapes;
    size_t numShapes;
    const uint32_t* indices;
    const mcrt_shape* dShapes;
    const uint32_t* dIndices;
    const float4* dPositions;
};
SceneGeometry scene_geometry(mcrt_scene s);
// A new shape table (same count, same mesh keys: checked by the caller) on the device, with a
// blocking copy, and on the host; the surface records and their bases stay as they are
mcrt_status store_shapes(mcrt_scene s, const mcrt_shape* shapes, uint32_t n);
int scene_num_lights(mcrt_scene s);
bool scene_has_sobol(mcrt_scene s);                // a Sobol matrix table of the full size was uploaded
const PrevPose* scene_prev_poses(mcrt_scene s);    // mcrt_scene_motion_snapshot's table, NULL before the first
SceneArgs scene_args(mcrt_scene s);                // the kernels' view
// The shapes of an update (same count and topology as the scene's, checked by the caller) against
// the scene's current table counts (check_scene_tables), and a moved startVertex against the host
// copies of the indices and the vertex count.  Changes nothing; MCRT_ERROR_INVALID_ARG names the shape.
mcrt_status check_updated_shapes(mcrt_scene s, const mcrt_shape* shapes, uint32_t n);
// The host copy of the positions, for a host builder: downloaded first when a device-side vertex
// update left it stale (the caller has finished the context stream).  NULL after a failed download.
const mcrt_float4* host_positions(mcrt_scene s);
// mcrt_pt_host.cpp: the frame slots and the path tracer
// A slot's buffers, stream and events: planes for `frames` frames of N pixels (T: the lanes of the
// frame's tiles) and ray queues of Q entries (at least N).  After a failure the slot is empty.
hipError_t slot_alloc(FrameSlot& k, size_t N, size_t T, int frames = 1, size_t Q = 0);
// the slots' streams, events and buffers; the frame buffer's own planes and its BDPT state go with it
void fb_free(mcrt_framebuffer fb);
// The current slot's camera record and primary-hit buffer, borrowed for a pass on the context
// stream: waits for every slot's last render, uploads `cam`, sizes the scene's spill columns and
// traces the camera rays of `f` (wave packets).  MCRT_ERROR_NOT_READY when the slot has no buffers.
// The slot's next render may overwrite both, so a pass that leaves work on the stream ends with
// release_slot.
mcrt_status borrow_camera_hits(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, const FrameArgs& f,
                               mcrt_camera** dCam, float4** hits);
// records on st that the current slot's buffers were read: the slot may take its next frame after it
hipError_t release_slot(mcrt_framebuffer fb, hipStream_t st);
// mcrt_bdpt_host.cpp: the bidirectional integrator
// One BDPT call of f.batch frames in frame slot `slot` with set k, enqueued on the slot's stream
// (the caller has made the slot ready and records its `done`).
mcrt_status bdpt_render(mcrt_scene s, mcrt_framebuffer fb, const mcrt_camera* cam, const mcrt_frame_params* p,
                        const FrameArgs& f, int k, FrameSlot& slot);
// Set k > 0 for a call of `frames` frames at this depth, allocated here if the frame buffer's arrays
// are of that depth and lack it.  *usable = false: it did not fit in device memory, and BDPT frames
// of this frame buffer use set 0 alone from now on (bdpt_sets).
mcrt_status bdpt_reserve_set(mcrt_framebuffer fb, int k, int depth, int frames, bool* usable);
int bdpt_sets(mcrt_framebuffer fb, int slots);   // sets BDPT frames rotate over, of `slots` frame slots: 1 or `slots`
bool bdpt_pending_gather(mcrt_framebuffer fb);   // a band-split frame waits for mcrt_bdpt_gather(_sparse)
// rays of the last BDPT call (max depth `depth`), read from its set: all subpath rays, connection rays
hipError_t bdpt_ray_counts(mcrt_framebuffer fb, int depth, int64_t* closest, int64_t* any);
// mcrt_adaptive.hip: adaptive sampling, as the path tracer and the denoiser see it
inline bool adaptive_on(mcrt_framebuffer fb) { return fb->ad.on; }
// the active-tile table of the next PT call (padded, see AdaptiveState::list) and its length
const uint32_t* adaptive_list(mcrt_framebuffer fb, int* len);
const uint32_t* adaptive_counts(mcrt_framebuffer fb);   // samples per tile
void adaptive_rendered(mcrt_framebuffer fb, int batch);   // a PT call of `batch` frames was enqueued over the list
// mcrt_accumulate's checks in adaptive mode, before anything is enqueued: a rendered frame is
// waiting, frame_index is the frame count since the reset, and frame 0 covers every tile
mcrt_status adaptive_check_accumulate(mcrt_framebuffer fb, int32_t frame_index);
// after k_accumulate and k_moments over the list: `batch` more samples in each listed tile (on st)
void adaptive_accumulated(mcrt_framebuffer fb, int batch, hipStream_t st);
// mcrt_framebuffer_set_moments: every tile holds `frames` samples (on the context stream)
hipError_t adaptive_set_counts(mcrt_framebuffer fb, int frames);
// mcrt_accel.cpp: the views of the scene's acceleration structure and the little else of it that
// the rest of the runtime reads
bool accel_ready(mcrt_scene s);            // mcrt_accel_build has made a structure
const float4* accel_nodes(mcrt_scene s);   // its records (SceneArgs::nodes)
int accel_spill_cap(mcrt_scene s);         // spill entries per ray the tree's depth asks for
const float* accel_world_box(mcrt_scene s);   // lo xyz, hi xyz
// Per-ray spill columns for `rays` rays (rounded up to whole waves); grown on demand.
bool ensure_spill(mcrt_scene s, size_t rays);
// the per-ray walks' view
TraceCtx trace_ctx(mcrt_scene s);
// the coherent launches' view (camera rays, bounce-0 shadow rays): wave packets when the tree allows
TraceCtx packet_ctx(mcrt_scene s);
// Occluder hints for a shadow launch (mcrt_traverse.h hintOccludes; flat trees only): bounce-0 rays
// by pixel (table `pix`, n pixels), later ones by origin cell; MCRT_SHADOW_HINTS=0 turns them off
void with_hints(TraceCtx& c, mcrt_scene s, uint32_t* pix, uint32_t n);
// a new hint table (the scene's by cell, a frame buffer's by pixel) filled with "no hint"
hipError_t fill_hints(uint32_t* d, size_t n, uint32_t range, hipStream_t st);
// `count` host elements into the (empty) buffer; S is T or the C ABI's name for it
template <class T, class S>
hipError_t upload(DevBuf<T>& dst, const S* src, size_t count, hipStream_t st) {
    static_assert(sizeof(S) == sizeof(T), "same element");
    if (!src || count == 0) return hipSuccess;
    hipError_t e = (hipError_t)dst.alloc(count);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(dst.get(), src, sizeof(T) * count, hipMemcpyHostToDevice, st);
}
// Allocates the plane (one T per pixel, zero-filled on the context stream) when it does not exist yet.
template <class T>
hipError_t ensure_plane(mcrt_framebuffer fb, DevBuf<T>& p) {
    if (p) return hipSuccess;
    hipError_t e = (hipError_t)p.alloc(fb->N);
    if (e == hipSuccess) e = hipMemsetAsync(p.get(), 0, sizeof(T) * fb->N, fb->ctx->stream);
    return e;
}
}  // namespace mcrt

#define HIPCHK(ctx, expr)                                                                                   \
    do {                                                                                                    \
        hipError_t e_ = (hipError_t)(expr);   /* DevBuf reports the runtime's codes as int */               \
        if (e_ != hipSuccess)                                                                               \
            return mcrt::fail(ctx, e_ == hipErrorOutOfMemory ? MCRT_ERROR_OUT_OF_MEMORY : MCRT_ERROR_DEVICE, \
                              std::string(#expr) + ": " + hipGetErrorString(e_));                           \
    } while (0)

struct Timed {
    mcrt_ctx c;
    int k;
    hipEvent_t a = nullptr, b = nullptr;
    const int* countDev;
    int64_t items;
    hipStream_t st;
    const int* countDev2;
    Timed(mcrt_ctx ctx, int kernel, const int* countDev_, int64_t items_, hipStream_t stream = nullptr,
          const int* countDev2_ = nullptr)
        : c(ctx), k(kernel), countDev(countDev_), items(items_), st(stream ? stream : ctx->stream),
          countDev2(countDev2_) {
        if (c->profiling) {
            hipEventCreate(&a);
            hipEventCreate(&b);
            hipEventRecord(a, st);
        }
    }
    ~Timed() {
        if (c->profiling) {
            hipEventRecord(b, st);
            c->pending.push_back({k, a, b, countDev, countDev2, items});
        }
    }
};
