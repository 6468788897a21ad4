// lrc_internal.h -- what the translation units of liblidarcast share and include/lidarcast.h does not declare: the
// handles behind the opaque types, the error plumbing, the HIP status macro, the owning device buffers and the small
// host helpers.  Everything in here is hidden: only the C ABI of include/lidarcast.h and the lrc_internal_* test hooks
// are dynamic symbols of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lidarcast.h"
#include "lrc_bvh_device.h"
#include "lrc_noise.h"
#include "lrc_echo.h"
#include "lrc_material.h"
#include "lrc_movers.h"
#include "lrc_flow.h"
#include "lrc_deform.h"

// sets lrc_last_error() (lidarcast.hip).  Exported: lrc_nprandom.cpp, built without HIP headers, reports through it.
extern "C" int lrc_internal_fail(int code, const char* msg);

#pragma GCC visibility push(hidden)

int fail(int code, const std::string& msg);      // lidarcast.hip: sets the thread's lrc_last_error() text, returns code

// LRC_HIP_WHERE is read where LRC_HIP is used, not here: a unit that names the stage its HIP calls belong to in front of
// the call text redefines it after this include (lrc_bvh_device.hip)
#define LRC_HIP_WHERE ""
#define LRC_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            (void)hipGetLastError();                                                       \
            return fail(e__ == hipErrorOutOfMemory ? LRC_ERR_OOM : LRC_ERR_HIP,            \
                        std::string(LRC_HIP_WHERE #call) + ": " + hipGetErrorString(e__)); \
        }                                                                                  \
    } while (0)

constexpr int kBlock = 256;          // compaction kernels
#ifndef LRC_TRACE_BLOCK
#define LRC_TRACE_BLOCK 64
#endif
constexpr int kTBlock = LRC_TRACE_BLOCK;   // trace kernel workgroup (rays per tile)

enum PoolSlot { kPoolRays = 0, kPoolT, kPoolPrim, kPoolNormal, kPoolPoint, kPoolSem, kPoolIns, kPoolInc, kPoolInten,
                kPoolPoses, kPoolDirs, kPoolOffs, kPoolCen, kPoolNoise,
                // *_compact entry points: scan angles in, per-wave keep counts, compacted frame arrays out
                kPoolAngles, kPoolKeep, kPoolTile, kPoolCounts, kPoolOutPoint, kPoolOutSem, kPoolOutIns, kPoolOutInc,
                kPoolOutIdx, kPoolOutXyzl, kPoolOutRange, kPoolStats, kPoolFrameStats, kPoolSlots };

// triangle records fetched per leaf round trip by the product kernels.  With edge records the pair fits 64 VGPRs, i.e. 8
// waves per SIMD: -2...-4 % trace time on all benchmark scenes against one record per round trip.
constexpr int kLeafW = 2;

struct lrc_ctx {
    int device = 0;
    // staging buffers of the host-pointer entry points, grown on demand and reused (a per-waypoint caller
    // such as the reference loop, s3dis_simulator.py:254-264, would otherwise pay hipMalloc/hipFree per pose)
    void* pool[kPoolSlots] = {};
    size_t pool_cap[kPoolSlots] = {};
    // compaction scratch (grown on demand, reused): per-tile counts and exclusive offsets.  Two sets: the
    // cloud rebuild of the multi-GPU path runs on its own stream next to the compaction of the local scan.
    struct TileScratch {
        uint32_t* d_tile_off = nullptr;     // offset of a tile inside its super tile (1024 tiles)
        uint32_t* d_tile_cnt = nullptr;
        uint32_t* d_super_total = nullptr;  // kept entries per super tile
        uint64_t* d_super_base = nullptr;   // exclusive prefix of d_super_total (+ grand total)
        uint64_t tile_cap = 0;
        double* d_dirs_soa = nullptr;       // direction table transposed to x[N] y[N] z[N] (cloud rebuild only)
        uint64_t dirs_cap = 0;
        // Frees every array and returns to the empty state.  A plain method, not a destructor: the owner makes the handle's
        // device current first (hipSetDevice) and says so where it calls this.
        void release() {
            for (void* p : {(void*)d_tile_off, (void*)d_tile_cnt, (void*)d_super_total, (void*)d_super_base, (void*)d_dirs_soa})
                if (p) (void)hipFree(p);
            *this = TileScratch{};
        }
    };
    TileScratch cloud_scratch;
    // lrc_compact_dev: one scratch set per caller stream (a caller that keeps two scans in flight on two streams compacts on
    // both); a set handed on to another stream is first ordered behind its last use (scratch_for)
    static constexpr int kCompactSets = 4;
    TileScratch compact_scratch[kCompactSets];
    hipStream_t compact_stream[kCompactSets] = {};
    hipEvent_t compact_done[kCompactSets] = {};
    bool compact_used[kCompactSets] = {};
    int compact_next = 0;
    // Dispatch chaining of trace launches ("the launch tail"): the LAST workgroup of every trace launch writes the
    // launch's sequence number to this signal word at its first instruction; a trace launch on ANOTHER stream than the
    // previous one is held behind hipStreamWaitValue64(word >= previous sequence number), i.e. it starts the moment the
    // previous launch has handed out its last workgroup -- its waves fill the slots the previous launch's tail leaves empty,
    // and launches that a caller keeps in flight on two streams run staggered instead of falling into phase.
    uint64_t* chain_word = nullptr;     // hipMallocSignalMemory; NULL: not supported here, launches are never chained
    uint64_t chain_seq = 0;             // sequence number of the last chained trace launch
    hipStream_t chain_stream = nullptr; // ... and the stream it went to
    bool chain_enabled = false;         // lrc_ctx_set_launch_chaining (opt-in: measured equal to what the dispatcher does itself)
    // *_compact entry points: kernels on one stream, the transfers of finished pose chunks on another
    hipStream_t s_compute = nullptr, s_copy = nullptr, s_stats = nullptr;
    hipEvent_t ev_chunk[8] = {}, ev_compact[8] = {};
    uint64_t* h_counts = nullptr;       // page-locked landing area of the per-pose counts and statistics (async copies
    uint64_t h_counts_cap = 0;          // need one): counts (P u64) | 4 x P doubles of per-pose statistics
    lrc::DeviceArena build_arena;       // scratch of the device scene build, reused from scene to scene
    float* stat_scratch = nullptr;      // chunk sums of lrc_cloud_range_stats_dev (calls of one context must not overlap
    uint64_t stat_scratch_cap = 0;      // on different streams: handles are not thread-safe)
    float* d_noise_tab = nullptr;       // lrc_scan_noisy_*: the normal quantile table (lrc_noise.h), uploaded on first use
};

struct lrc_table {            // a sensor's direction table resident in HBM (lrc_table_create)
    lrc_ctx* ctx = nullptr;
    double* d_dirs3 = nullptr;
    uint64_t n = 0;
    double* d_fire = nullptr;   // optional (lrc_table_set_fire): per ray the fraction of the sweep at which it fires
};

struct lrc_material_table {   // a material table resident in HBM (lrc_material_table_create): num_classes records and the model
    lrc_ctx* ctx = nullptr;
    lrcmat::Record* d_records = nullptr;
    lrc_material_model model{};
};

struct lrc_scene {
    lrc_ctx* ctx = nullptr;
    void* slab = nullptr;             // device-built scenes: ONE allocation holds every array below except d_slot_sphere / *4
    float4* d_nodes = nullptr;
    float4* d_tris = nullptr;
    uint32_t* d_slot_prim = nullptr;
    uint32_t* d_slot_label = nullptr;
    float* d_slot_box = nullptr;      // per leaf slot the triangle's exact vertex box (lo xyz, hi xyz)
    float4* d_prim_plane = nullptr;   // per caller's triangle row: (v0, label bits), (Ng, 0): lrc_cloud_from_prims_dev
    std::mutex plane_mutex;           // ... built on first use, published complete (ensure_prim_plane)
    float4* d_slot_sphere = nullptr;  // per leaf slot: centre of the triangle's box + bounding radius (sector_kernel)
    // quantised node images of the SAME tree ("32-byte nodes"): child boxes on a 15-bit grid
    // per axis, rounded outward (margin 1/16 cell).  d_nodes_q: 32 B per node for the per-lane fetches; d_nodes_n: the same
    // boxes as normalised float32 (64 B per node) for the scalar fetches.  NULL when the grid does not fit the scene.
    uint4* d_nodes_q = nullptr;
    float4* d_nodes_n = nullptr;
    // the same tree collapsed to four children per node (every second level removed), on the same grid:
    // d_nodes_q4 64 B per node (per child lo|hi<<16 x, y, z + reference), d_nodes_n4 128 B (per child lo, hi, ref, pad)
    uint4* d_nodes_q4 = nullptr;
    float4* d_nodes_n4 = nullptr;
    uint64_t num_nodes4 = 0;
    float qbase[3] = {0, 0, 0}, qW[3] = {1, 1, 1}, qinvW[3] = {1, 1, 1};
    const lrc_grid* cur_grid = nullptr;   // set around a grid scan (launch_trace, kGenGrid)
    lrc_scene_info info{};
    lrc_scan_options opts{};          // sticky opt-in options (lrc_scene_set_options)
    uint64_t launches = 0, rays = 0;
    lrc_deform* deform = nullptr;     // the deformable that owns this scene (lrc_deform_create); NULL for an ordinary scene
    void* flow_scratch = nullptr;     // flow_scan_dev without a mover set: grown on demand (a set brings its own scratch)
    uint64_t flow_scratch_cap = 0;
};

struct lrc_movers {           // a mover set (lrc_movers_create): the caller's scenes, not owned, and the scan's scratch
    lrc_ctx* ctx = nullptr;
    std::vector<lrc_scene*> scenes;
    void* scratch = nullptr;      // movers_scan_dev and flow_scan_dev: grown on demand, the same size whatever M is
    uint64_t scratch_cap = 0;
};

// device buffer of a host-pointer entry point: its own allocation, or a slot of the context's staging pool
struct DevBuf {
    void* p = nullptr;
    bool pooled = false;
    ~DevBuf() { if (p && !pooled) (void)hipFree(p); }
    // buffer of the context's staging pool (kept for the next call)
    int get(lrc_ctx* ctx, int slot, size_t bytes) {
        if (ctx->pool_cap[slot] < bytes) {
            if (ctx->pool[slot]) { (void)hipFree(ctx->pool[slot]); ctx->pool[slot] = nullptr; ctx->pool_cap[slot] = 0; }
            const size_t cap = bytes + bytes / 8;
            LRC_HIP(hipMalloc(&ctx->pool[slot], cap));
            ctx->pool_cap[slot] = cap;
        }
        p = ctx->pool[slot];
        pooled = true;
        return LRC_OK;
    }
};
// plain owning device allocation
struct Buf {
    void* p = nullptr;
    ~Buf() { if (p) (void)hipFree(p); }
};

inline uint64_t blocks_of(uint64_t n, uint64_t per) { return (n + per - 1) / per; }
inline int env_int(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }

// the mesh checks of lrc_coverage_create and lrc_frameobj_create (non-finite vertex, triangle index out of range); `who`
// prefixes the message.  Defined in lidarcast.hip, beside fail(): host code with no unit of its own.
// lrc_scene_create with the node images chosen by the caller (qmode as LRC_QNODES; lidarcast.hip): lrc_deform_create asks for
// float32 nodes whatever the environment says
int scene_create_mode(lrc_ctx* ctx, const float* verts3, uint64_t V, const uint32_t* tris3, uint64_t T, const uint16_t* tri_sem,
                      const uint16_t* tri_ins, int qmode, lrc_scene** out_scene);

int check_mesh(const char* who, const double* verts3, uint64_t V, const int32_t* tris3, uint64_t T);

// lrc_noise.hip: checks an lrc_noise for a table of N rays (LRC_ERR_INVALID_ARG, `who` prefixes the message), makes the
// context's quantile table resident and fills the kernel's parameter block
int noise_params(lrc_ctx* ctx, const char* who, const lrc_noise* nz, uint64_t N, lrcnoise::Params* out);
// the same checks and the same block with the HOST copy of the table, for the host twins of the generators (no context, no GPU)
int noise_params_host(const char* who, const lrc_noise* nz, uint64_t N, lrcnoise::Params* out);

// beam footprint and multi-echo returns.  lrc_echo.hip checks the arguments of lrc_scan_echoes_* and fills an lrcecho::Params;
// lidarcast.hip, which owns the trace kernel and the frame path, launches (echo_scan_dev) and scans to frames
// (echo_scan_compact: host poses and offsets, ep.offsets2 / ep.weight are filled there; the weights of the kept rows are gathered
// there from the fixed-stride weights by the compacted index column).
int echo_scan_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N, const lrcecho::Params& ep,
                  double max_range, const lrc_hits* d_out, hipStream_t st);
int echo_scan_compact(lrc_scene* s, const double* poses16, uint64_t P, const lrc_table* table, const double* offsets2,
                      lrcecho::Params ep, double max_range, const lrc_frames* out, uint8_t* weight_rows, uint64_t capacity,
                      uint64_t* out_total);

// surface materials.  lrc_material.hip checks the arguments of lrc_scan_materials_* and fills an lrcmat::Params from the resident
// table; lidarcast.hip, which owns the trace kernel and the frame path, launches (material_scan_dev) and scans to frames
// (material_scan_compact: host poses; mp.bounces / mp.surface3 and the intensity column are its own device buffers, gathered
// there for the kept rows by the compacted index column; a NULL destination is skipped).
int material_scan_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N, const lrcmat::Params& mp,
                      double max_range, const lrc_hits* d_out, hipStream_t st);
int material_scan_compact(lrc_scene* s, const double* poses16, uint64_t P, const lrc_table* table, lrcmat::Params mp,
                          double max_range, const lrc_frames* out, float* intensity_rows, uint8_t* bounces_rows, float* surface_rows,
                          uint64_t capacity, uint64_t* out_total);

// moving objects: the four scans lrc_scan_movers_*, lrc_scan_noisy_movers_*, lrc_scan_mover_sweeps_* and
// lrc_scan_noisy_mover_sweeps_* are one scan under two switches.  lrc_movers.hip checks their arguments, fills the
// lrcnoise::Params (noise_params) and owns the handle and the host functions; lidarcast.hip, which owns the trace launch,
// write_back and the frame path, holds the two kernel templates and enqueues the passes.
struct MoverScan {                   // one call of the family: device pointers
    const double* sensor;            // (P,16) poses, or with `fire` the sensor's (P,24) motion records
    const double* dirs3;             // (N,3)
    const double* fire;              // (N) firing fractions; non-NULL: the scan is under moving-sensor sweeps
    const float* movers;             // (P,M,12) mover poses, or with `fire` the (P,M,24) mover sweep records; unread without a set
    const lrcnoise::Params* noise;   // non-NULL: the scan is under seeded sensor noise
    uint64_t P, N;
    double max_range;
};
// movers_scan_dev: everything on `st`, no host synchronisation; set == NULL: the variant's plain scan (lrc_scan_poses_dev,
// lrc_scan_noisy_dev, lrc_scan_sweeps_dev, lrc_scan_noisy_sweeps_dev) and a zero mover column.  movers_scan_compact: host
// records (`sensor`, `movers` as in MoverScan, by `sweep`), the table with its directions and under `sweep` its fire table, all
// poses in one call (pose p is frame first_frame + p of `noise`), the mover column gathered for the kept rows by the compacted
// index column; `flow`: flow_scan_compact's columns beside it.
struct FlowCompact;
int movers_scan_dev(lrc_scene* s, lrc_movers* set, const MoverScan& scan, const lrc_hits* d_out, uint8_t* d_mover, hipStream_t st);
int movers_scan_compact(lrc_scene* s, lrc_movers* set, const double* sensor, uint64_t P, const lrc_table* table, const float* movers,
                        double max_range, bool sweep, const lrcnoise::Params* noise, const lrc_frames* out, uint8_t* mover_rows,
                        uint64_t capacity, uint64_t* out_total, const FlowCompact* flow = nullptr);

// the checks lrc_scan_movers_* and lrc_scan_flow_* share (lrc_movers.hip).  check_call: NULL scene or output, a set of another
// context or one that holds the static scene, a range_noise option; `set` may be NULL.  check_poses12: `count` host mover poses,
// every entry finite and max |R^T R - I| <= 2^-16 in float64.  check_motion (lidarcast.hip): the host check of (P,24) sensor
// records every *_sweeps_compact call makes.
int check_call(const char* who, const lrc_scene* s, const lrc_movers* set, const void* out);
int check_poses12(const char* who, const float* m, uint64_t count);
int check_motion(const char* who, const double* m, uint64_t P);

// scene flow under movers.  lrc_flow.hip checks the arguments of lrc_scan_flow_* and owns the host functions; lidarcast.hip holds
// the kernels and enqueues the passes (flow_scan_dev: everything on `st`, no host synchronisation; d_status == NULL: the flow
// alone, nothing cast) and scans to frames (flow_scan_compact: the mover scan and the flow at the fixed stride, then the frame
// path of movers_scan_compact with the flow and status columns gathered beside the mover column).
struct FlowNext {             // what pairs every frame of a call with its next one: device pointers for flow_scan_dev, host
    const float* next_mover_poses12;      // pointers for flow_scan_compact
    const double* next_poses16;
    const uint8_t* has_next;              // nullable: all ones
};
struct FlowCompact {          // what flow_scan_compact adds to movers_scan_compact
    FlowNext next;                        // host pointers
    float* flow_rows;                     // nullable
    uint8_t* status_rows;                 // nullable: flow only, nothing cast
};
// non-rigid scene flow (lrc_scan_nonrigid_flow_dev): the surface pairs of one call as the kernel takes them, by value in its
// arguments.  Entry k serves the rows of mover mover[k] (w - 1) whose prim is below T[k]; vb is never NULL here (lrc_flow.hip
// has put the deformable's current vertices in).  count == 0, or a NULL pointer: the rigid ray kernel.
struct FlowPairs {
    uint32_t count;
    uint32_t mover[16];
    uint32_t T[16];
    const float* va[16];
    const float* vb[16];
    const uint32_t* tris3[16];
    const uint32_t* prim;                 // the records' prim column
};
int flow_scan_dev(lrc_scene* s, lrc_movers* set, const lrc_hits* d_rec, const uint8_t* d_mover, uint64_t P, uint64_t N,
                  const float* d_mover_poses12, const FlowNext& next, double max_range, float* d_flow3, uint8_t* d_status,
                  hipStream_t st, const FlowPairs* pairs = nullptr);
// what a deformable keeps resident (lrc_deform.hip): its current vertices and its triangles
struct DeformMesh { const float* d_verts3; const uint32_t* d_tris3; uint64_t V, T; };
DeformMesh deform_mesh(const lrc_deform* d);

// a deformable (lrc_deform_create: keyframes; lrc_deform_create_skinned: a rest shape, bone influences and K key poses).  Both
// routes write d_verts and refit the scene from it; every other call on the handle does not know which route made it.
struct lrc_deform {
    lrc_ctx* ctx = nullptr;
    lrc_scene* scene = nullptr;       // owned
    uint32_t K = 0;
    uint64_t V = 0, T = 0;
    float* d_keys = nullptr;          // (K, V, 3); NULL for a skinned deformable
    float* d_verts = nullptr;         // (V, 3): the current shape
    uint32_t* d_tris3 = nullptr;      // (T, 3)
    uint32_t* d_order = nullptr;      // inner nodes grouped by height, height 0 first
    std::vector<uint32_t> level_off;  // level_off[h] .. level_off[h + 1]: the nodes of height h in d_order
    uint32_t tail_first = 0;          // heights >= tail_first are finished by k_tail (== number of heights: no tail)
    // skinned deformables (lrc_skin.hip); B == 0: the keyframe route
    uint32_t B = 0;                   // bones per key pose
    float* d_rest = nullptr;          // (V, 3) rest positions
    uint32_t* d_idx4 = nullptr;       // (V) four uint8 bone indices, influence j in bits 8 j .. 8 j + 7
    float4* d_wgt4 = nullptr;         // (V) four weights
    float* d_poses = nullptr;         // (K, B, 12) bone poses
    // animated movers under sweeps (lrc_span.hip); allocated by the first lrc_deform_span_dev
    bool spanned = false;             // the node boxes hold both shapes of a span: set by lrc_deform_span_dev, cleared by lrc_deform_set_dev
    float* d_verts_b = nullptr;       // (V, 3): shape B of the span (d_verts holds shape A)
    float* d_span_box = nullptr;      // per leaf slot the span box (lo xyz, hi xyz)
    float* d_span_rec = nullptr;      // per leaf slot lrcspan::kRecFloats floats: v0, v1, v2 of A, then of B, two of padding
};
// lrc_deform.hip, for both routes.  deform_coordinate_ok: the bit test of scene_create_host, finite and |f| <= 1e6.
// deform_build: what creation does after the route's own checks -- the scene from `verts0_3` (float32 nodes), the fixed bounds
// (enc'ed lo / hi planes of the union box the caller has gathered), the height table, the vertex, triangle and height arrays;
// on failure the caller destroys `d`.  deform_refit_enqueue: k_slots, k_level per height and k_tail on `st`, from d_verts; its two
// halves are deform_slots_enqueue (k_slots) and deform_nodes_enqueue (k_level / k_tail from `slot_box`: the scene's exact slot
// boxes, or the span boxes of lrc_span.hip).  deform_shape_enqueue: the vertices of shape (k0, k1, w) into `out` (V, 3) by the
// handle's route -- keyframe copy, k_blend or k_skin -- arguments checked by the caller.  deform_height_table: the inner nodes of
// `nodes` grouped by height, height 0 first (false: no tree over the slots), for the host refits.
inline bool deform_coordinate_ok(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x7FFFFFFFu) <= 0x49742400u;
}
int deform_build(lrc_deform* d, const char* who, const float* verts0_3, const uint32_t* tris3, const uint16_t* tri_sem,
                 const uint16_t* tri_ins, const int lo[3], const int hi[3]);
int deform_refit_enqueue(lrc_deform* d, hipStream_t st);
int deform_slots_enqueue(lrc_deform* d, hipStream_t st);
int deform_nodes_enqueue(lrc_deform* d, const float* d_slot_box, hipStream_t st);
int deform_shape_enqueue(lrc_deform* d, uint32_t k0, uint32_t k1, float w, float* d_out, hipStream_t st);
bool deform_height_table(const float* nodes, uint64_t num_nodes, uint64_t num_slots, std::vector<uint32_t>& order);
// lrc_span.hip: the per-ray-shape cast of a spanned deformable's scene in the place of cast_plain (lidarcast.hip,
// movers_scan_dev under sweeps): ray g of `n` has the firing fraction d_fire[g % rays_per_pose]; the five columns of `out` the merge reads
int span_cast(lrc_deform* d, const float* d_rays6, const uint8_t* d_keep, const double* d_fire, uint64_t rays_per_pose, uint64_t n,
              const lrc_hits& out, hipStream_t st);
// lrc_skin.hip: the k_skin launch of deform_shape_enqueue on a skinned deformable, into `d_out` (V, 3)
int skin_enqueue(lrc_deform* d, uint32_t k0, uint32_t k1, float w, float* d_out, hipStream_t st);
int flow_scan_compact(lrc_scene* s, lrc_movers* set, const double* poses16, uint64_t P, const lrc_table* table,
                      const float* mover_poses12, const FlowNext& next, double max_range, const lrc_frames* out, uint8_t* mover_rows,
                      float* flow_rows, uint8_t* status_rows, uint64_t capacity, uint64_t* out_total);

#pragma GCC visibility pop
