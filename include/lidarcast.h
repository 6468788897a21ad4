/*
 * lidarcast.h -- C ABI of liblidarcast, the MI355X (gfx950) LiDAR ray-cast scan engine.
 *
 * The reference has no FFI on this path: its engine boundary is the Python ABC
 * RaycastEngineBase (raycast_engine/raycast_engine.py:16-61) whose concrete classes call
 * open3d.t.geometry.RaycastingScene (raycast_engine/raycast_engine_cpu.py:46-51,
 * raycast_engine/raycast_engine_gpu_simple.py:41-46).  The entry points below are what a
 * ctypes binding of that boundary needs ("Suggested C exports"); each
 * one names the reference call it stands in for.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every function returns an int status: 0 (LRC_OK) or a negative LRC_ERR_* code;
 *     lrc_last_error() returns a thread-local, NUL-terminated description of the last failure.
 *   - no exception, abort() or longjmp crosses this boundary.
 *   - the caller allocates inputs and outputs; the library owns only the opaque handles.
 *   - "host" entry points take host pointers, copy, run the HIP kernels and copy back
 *     (synchronous on return).  "_dev" entry points take DEVICE pointers and a hipStream_t
 *     (passed as void*; NULL = the null stream) and only enqueue work.
 *   - handles are not thread-safe; use one context per thread.
 *   - finite-ray contract: a ray with a NaN or infinite origin or direction component is never cast; it is reported
 *     as a miss (t = +inf, prim = LRC_INVALID_PRIM, zeros elsewhere), as Embree reports a ray it cannot intersect.
 *     Mesh vertices must be finite and within 1e6 (lrc_scene_create rejects others).
 *
 * Hit definition (oracle/lrc_oracle.c restates it on the CPU)
 *   Two-sided closest hit, t in (0, +inf), t parametric along the GIVEN direction (the direction
 *   is not normalised, as in Open3D), miss = +inf / prim 0xFFFFFFFF, ties broken by the smaller
 *   triangle row index.  float32 throughout with a fixed fused-multiply-add expression tree.
 */
#ifndef LIDARCAST_H
#define LIDARCAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRC_OK                 0
#define LRC_ERR_INVALID_ARG  (-1)   /* NULL pointer, bad size, triangle index out of range      */
#define LRC_ERR_NO_DEVICE    (-2)   /* no HIP device / device ordinal out of range              */
#define LRC_ERR_HIP          (-3)   /* a HIP runtime call failed; text in lrc_last_error()      */
#define LRC_ERR_OOM          (-4)   /* host or device allocation failed                         */
#define LRC_ERR_INTERNAL     (-5)

#define LRC_INVALID_PRIM  0xFFFFFFFFu

typedef struct lrc_ctx   lrc_ctx;     /* one HIP device + scratch buffers                       */
typedef struct lrc_scene lrc_scene;   /* one triangle mesh + its BVH, resident in HBM           */

/* Per-ray hit attributes, structure-of-arrays.  Every pointer may be NULL (attribute skipped).
 * Arrays hold one entry per ray (cast) or P*N entries, pose-major (scan).
 * Replaces the result dict of RaycastingScene.cast_rays (raycast_engine_cpu.py:51-53:
 * t_hit, primitive_ids, primitive_normals) plus the numpy post-processing that follows it. */
typedef struct lrc_hits {
    float*    t;             /* (n)    parametric range; +inf = miss or removed by the range filter */
    uint32_t* prim;          /* (n)    triangle row index in the caller's array; LRC_INVALID_PRIM   */
    float*    normal3;       /* (n,3)  unit geometric normal normalize((v1-v0)x(v2-v0)); 0 on miss   */
    float*    point3;        /* (n,3)  o + (d/|d|)*t in float32, mul then add
                                       (raycast_engine_cpu.py:57-62); 0 on miss                      */
    uint16_t* sem;           /* (n)    semantic label of the hit triangle; 0 on miss                 */
    uint16_t* ins;           /* (n)    instance label of the hit triangle; 0 on miss                 */
    double*   incident_deg;  /* (n)    degrees(arccos(|((p-c)/|p-c|)_z|)) in float64
                                       (raycast_engine_cpu.py:100-107); 0 on miss                    */
    void*     t_label;       /* (n) x 8 B  DEVICE entry points only: packed {float t; uint32 sem|ins<<16}, the
                                       pair lrc_cloud_from_ranges_dev needs to rebuild a hit point          */
    uint32_t* tile_count;    /* (ceil(n/64)) DEVICE entry points only: number of kept entries in each
                                       aligned run of 64 outputs; lets lrc_compact_dev skip its counting
                                       pass (lrc_compact_io.tile_count).  Ignored by the host entry points */
    float*    intensity;     /* (n)    opt-in (the reference computes no intensity; its noise model expects one
                                       in [0,1], lidar/lidar_intrinsics.py:364-377): Lambertian return
                                       |cos(angle between the ray and the unit geometric normal)|, float32;
                                       0 on miss                                                        */
} lrc_hits;

typedef struct lrc_scene_info {
    uint64_t num_vertices;
    uint64_t num_triangles;
    uint64_t num_nodes;        /* inner nodes of the binary BVH (64 B each)                      */
    uint64_t num_leaves;
    uint64_t num_slots;        /* triangle records in leaf order (48 B each), == num_triangles   */
    uint32_t max_depth;        /* root = depth 0; bounded by LRC_MAX_BVH_DEPTH                   */
    uint32_t max_leaf_size;
    uint64_t device_bytes;     /* HBM held by this scene                                         */
    double   build_ms;         /* host BVH build time                                            */
    double   upload_ms;
    float    bounds_lo[3];
    float    bounds_hi[3];
    uint32_t quantised_nodes;  /* 1: the trace kernels walk the 32-byte quantised node images of this tree   */
    float    leaf_inflation;   /* mean half perimeter of a leaf box on the 15-bit grid / of its float32 box  */
    uint32_t device_build;     /* 1: the BVH was built on the GPU (build_ms = hierarchy + layout kernels,
                                  upload_ms = mesh transfer + validation); 0: host builder                     */
    uint32_t reserved_;
} lrc_scene_info;

#define LRC_MAX_BVH_DEPTH 32

/* Library version string, e.g. "lidarcast 0.1.0 (gfx950)". */
const char* lrc_version(void);

/* Thread-local text of the last error raised on this thread ("" if none). */
const char* lrc_last_error(void);

/* Number of visible HIP devices (0 when there is none); never fails. */
int lrc_device_count(void);

/* Bind a context to HIP device `device`.  Fails with LRC_ERR_NO_DEVICE on a box without a GPU so
 * that RaycastEngineGPU() raises and the caller's try/except (s3dis_simulator.py:66-74) can act. */
int lrc_ctx_create(int device, lrc_ctx** out_ctx);
int lrc_ctx_destroy(lrc_ctx* ctx);
int lrc_ctx_synchronize(lrc_ctx* ctx);

/* Launch chaining (opt-in; available where the device supports stream memory operations).
 * The poses of a trajectory are independent (s3dis_simulator.py:254-288 carries no state from one waypoint to the
 * next), so a caller may keep two scans in flight: lrc_scan_poses_dev / lrc_scan_angles_dev / lrc_cast*_dev on two
 * streams with two record sets.  A scan launch ends in a tail -- a few long-running waves on an emptying chip -- and what
 * two unordered launches make of it is luck: side by side they end together (nothing gained) or staggered (+12 %).
 * With chaining the library orders them: a scan enqueued on ANOTHER stream than the previous scan of this context is held
 * (hipStreamWaitValue64 on a signal word the previous launch's last workgroup writes when it starts) until that launch
 * has no workgroup left to hand out, and then fills the slots its tail leaves empty.  Consecutive scans on ONE stream
 * are untouched (stream order already serialises them).  The only semantic effect is an extra ordering edge from the
 * earlier-enqueued scan to the later one; results are unaffected.  Off by default: on MI355X the workgroup dispatcher
 * serves one launch of one-wave workgroups at a time anyway, so two bare trace launches on two
 * streams already overlap this way and the explicit order measured equal (tools/pipe_time.py, tools/two_in_flight.py);
 * it is kept for callers whose streams carry other kernels between the scans. */
int lrc_ctx_set_launch_chaining(lrc_ctx* ctx, int enabled);
int lrc_ctx_get_launch_chaining(const lrc_ctx* ctx, int* out_enabled, int* out_supported);

/* Build the scene once per mesh: float32 vertices (V,3) and uint32 triangle rows (T,3) in, binned-SAH
 * BVH (leaves <= 4 triangles, bounded depth), triangle records, id / label / plane tables and the
 * quantised node images out, all resident in HBM.  tri_sem / tri_ins are optional per-triangle labels.
 * The build runs ON THE GPU (csrc/lrc_bvh_device.hip; milliseconds for a 10^6-triangle mesh); the
 * host builder (csrc/bvh_build.cpp) produces the same tree and the same bytes and serves meshes of a
 * handful of triangles and LRC_DEVICE_BUILD=0.
 * Replaces RaycastingScene() + TriangleMesh.from_legacy + add_triangles, which the reference
 * repeats on every call (raycast_engine_cpu.py:46-47, raycast_engine.py:20-24).
 * T == 0 is allowed (every ray misses). */
int lrc_scene_create(lrc_ctx* ctx,
                     const float* verts3, uint64_t num_vertices,
                     const uint32_t* tris3, uint64_t num_triangles,
                     const uint16_t* tri_sem, const uint16_t* tri_ins,
                     lrc_scene** out_scene);
/* The same for a mesh that is already in HBM (DEVICE pointers; labels may be NULL): nothing crosses
 * PCIe.  Synchronous like lrc_scene_create; the input arrays may be released on return. */
int lrc_scene_create_dev(lrc_ctx* ctx,
                         const float* d_verts3, uint64_t num_vertices,
                         const uint32_t* d_tris3, uint64_t num_triangles,
                         const uint16_t* d_tri_sem, const uint16_t* d_tri_ins,
                         lrc_scene** out_scene);
int lrc_scene_destroy(lrc_scene* scene);
int lrc_scene_get_info(const lrc_scene* scene, lrc_scene_info* out_info);

/* Copy the BVH back to host arrays (tests check its invariants).  Any pointer may be NULL.
 *   nodes16 : num_nodes * 16 floats  (lo0 xyz, hi0 xyz, lo1 xyz, hi1 xyz, ref0, ref1, 0, 0; refs are
 *             int32 bit patterns: >=0 inner node index, <0 leaf: ~ref = first_slot*8 + count)
 *   slot_prim: num_slots uint32 (triangle row index stored in each leaf slot) */
int lrc_scene_export_bvh(const lrc_scene* scene, float* nodes16, uint32_t* slot_prim);

/* Copy one of the scene's device arrays back (tests compare the device builder's bytes with the host builder's).
 * dst may be NULL to ask for the size only (*out_bytes; 0 for an array this scene does not have). */
#define LRC_ARRAY_NODES       0   /* num_nodes x 64 B                                      */
#define LRC_ARRAY_TRIS        1   /* num_slots x 48 B: v0 v1 v2 Ng                         */
#define LRC_ARRAY_SLOT_PRIM   2   /* num_slots x u32                                       */
#define LRC_ARRAY_SLOT_LABEL  3   /* num_slots x u32: sem | ins << 16                      */
#define LRC_ARRAY_PRIM_PLANE  4   /* num_triangles x 32 B: (v0, label bits), (Ng, 0)       */
#define LRC_ARRAY_NODES_Q     5   /* num_nodes x 32 B quantised image                      */
#define LRC_ARRAY_NODES_N     6   /* num_nodes x 64 B normalised float32 image             */
int lrc_scene_export_array(const lrc_scene* scene, int which, void* dst, uint64_t dst_bytes, uint64_t* out_bytes);

/* ---- cast: explicit rays --------------------------------------------------------------------
 * rays6 is (N,6) float32 rows [ox,oy,oz,dx,dy,dz] (raycast_engine_cpu.py:24-38).
 * center3 (3 doubles, may be NULL) and max_range implement lidar_intersect_mesh's range filter
 * (raycast_engine_cpu.py:95-97): a hit is kept iff |float64(point) - center| < max_range (strict);
 * removed hits are reported exactly like misses.  With center3 == NULL nothing is filtered and
 * incident_deg is measured from the ray origin.
 * Replaces RaycastingScene.cast_rays + the numpy block raycast_engine_cpu.py:50-73. */
int lrc_cast(lrc_scene* scene, const float* rays6, uint64_t num_rays,
             const double* center3, double max_range, const lrc_hits* out);
int lrc_cast_dev(lrc_scene* scene, const float* d_rays6, uint64_t num_rays,
                 const double* center3 /* HOST pointer, 3 doubles or NULL */, double max_range,
                 const lrc_hits* d_out, void* stream);

/* ---- cast: explicit rays of several poses in one launch ------------------------------------------
 * rays6 holds the rays of S poses back to back (ragged: the dual-axis sensor drops ~2 % of its rays per
 * pose, lidar/indoor_lidar.py:292-294); seg_offsets (S+1 entries, first 0, last num_rays) delimits them
 * and centers3 (S,3) gives each pose's range-filter centre.  Per ray exactly lrc_cast with its pose's
 * centre.  Replaces the per-waypoint loop body (s3dis_simulator.py:254-264) for sensors whose rays are
 * generated on the host. */
int lrc_cast_segments(lrc_scene* scene, const float* rays6, uint64_t num_rays,
                      const uint64_t* seg_offsets, uint64_t num_segments, const double* centers3,
                      double max_range, const lrc_hits* out);
int lrc_cast_segments_dev(lrc_scene* scene, const float* d_rays6, uint64_t num_rays,
                          const uint64_t* d_seg_offsets, uint64_t num_segments,
                          const double* d_centers3, double max_range, const lrc_hits* d_out,
                          void* stream);

/* ---- scan: pose-batched, rays generated in the kernel -------------------------------------------
 * poses16: (P,16) float64 row-major 4x4 sensor poses (Waypoint.to_pose_matrix,
 *          trajectory/trajectory_generator.py:30-44).
 * dirs3  : (N,3) float64 sensor-frame unit directions, line-major/azimuth-minor
 *          (IndoorLidar._gen_lidar_rays_with_vertical_degrees, lidar/indoor_lidar.py:108-126).
 * Ray (p,i): origin = float32(pose[:3,3]); direction = float32(dirs3[i] @ R^T) evaluated in float64 as the
 * fused chain fma(c,R[j][2], fma(b,R[j][1], a*R[j][0])) -- what numpy's BLAS product gives bit for bit
 * (lidar/indoor_lidar.py:127-131); then exactly lrc_cast with
 * center = pose[:3,3] and max_range.  Output index = p*N + i.
 * Replaces the per-waypoint loop body s3dis_simulator.py:254-264. */
int lrc_scan_poses(lrc_scene* scene, const double* poses16, uint64_t num_poses,
                   const double* dirs3, uint64_t rays_per_pose, double max_range,
                   const lrc_hits* out);
int lrc_scan_poses_dev(lrc_scene* scene, const double* d_poses16, uint64_t num_poses,
                       const double* d_dirs3, uint64_t rays_per_pose, double max_range,
                       const lrc_hits* d_out, void* stream);

/* ---- compaction: fixed-stride records -> the reference's variable-length frames ----------------
 * Stable compaction, in (segment, ray) order, of the entries whose t is finite.  `t` holds
 * num_segments * seg_len entries.  counts[s] receives the number kept in segment s;
 * the kept entries of all segments are packed back to back, which is the order of
 * np.vstack over frames (containers/s3dis_sim_scene.py:326,362).  Optional gathers (NULL = skip):
 * point3 -> out_point3 (K,3), sem/ins -> out_sem/out_ins (K), incident -> out_incident (K),
 * out_index (K) = index of the kept entry inside its segment, out_xyzl (K,4) = point + packed labels.
 * Host variant returns the total K in *out_total. */
typedef struct lrc_compact_io {
    const float*    t;
    const float*    point3;
    const uint16_t* sem;
    const uint16_t* ins;
    const double*   incident_deg;
    const uint32_t* tile_count;    /* optional, device entry point only: lrc_hits.tile_count of the scan
                                      that produced t (used when seg_len % 64 == 0)                   */
    uint64_t*       counts;        /* (num_segments)                                  */
    float*          out_point3;
    uint16_t*       out_sem;
    uint16_t*       out_ins;
    double*         out_incident_deg;
    uint32_t*       out_index;
    float*          out_xyzl;      /* (K,4) packed rows x, y, z, label bits (sem | ins<<16): the 16-byte
                                      row the multi-GPU all-gather moves                              */
    float*          out_range_origin; /* (K) |point| from the WORLD origin in float32, formed as numpy's
                                      np.linalg.norm(points, axis=1) forms it: the quantity the reference takes its
                                      ScanQuality range statistics over (s3dis_simulator.py:283-284)  */
} lrc_compact_io;

int lrc_compact(lrc_ctx* ctx, uint64_t num_segments, uint64_t seg_len,
                const lrc_compact_io* io, uint64_t* out_total);
int lrc_compact_dev(lrc_ctx* ctx, uint64_t num_segments, uint64_t seg_len,
                    const lrc_compact_io* d_io, void* stream);

/* ---- the scan pipeline: consecutive pose batches of one scene, launches overlapped inside the library ---------------
 * The poses of a trajectory are independent (s3dis_simulator.py:254-288), and so are consecutive trajectories over one
 * mesh (the reference's batch driver, s3dis_simulator.py:594-726, runs them one after the other).  A caller that stays on
 * the device -- dataset generation, the multi-GPU step, bench.py -- submits batch after batch; each submit is one pose-batched
 * scan (lrc_scan_poses_dev, into one of four record sets the pipeline owns) plus the stable compaction (lrc_compact_dev) into
 * the CALLER's rows / counts.  With rays_per_pose % 64 == 0 a set holds per ray 12 bytes -- (t, label, triangle slot) -- and per
 * 64 rays the keep mask.  The compaction forms the (x, y, z, label) row of a ray from that record, the unit vector of its row
 * in the submit's ray table (lrc_pipe_set_ray_table; the pipeline keeps one table per set) and the pose's float32 origin, with
 * the arithmetic the scan itself forms the point with; rays of a pose that does not take the table (its rotation is not pose
 * 0's, or the table is off) have their packed row stored beside the record instead.  The complete 36-byte record is formed from
 * the same only when lrc_pipe_records asks for it, out of nothing but what the pipeline and the scene own.  The pipeline
 * arranges the launches so that the trace
 * of submit k+1 fills the wave slots the trace of submit k leaves empty while its last, long-running waves finish, and the
 * rows of submit k are scattered by the first workgroups of the trace launch of submit k+2 (DESIGN.md "the launch tail":
 * a 64-pose launch alone loses a sixth of its time to that tail).  Same arithmetic, same bytes as lrc_scan_poses_dev +
 * lrc_compact_dev called one after the other.
 *   lrc_pipe_submit   enqueues only.  Inputs and the output buffers are taken as of `stream`'s current position; nothing
 *                     is ordered after it on `stream` -- that is the point -- until
 *   lrc_pipe_wait     scatters the rows still in the pipeline and makes `stream` wait for every submit so far (event
 *                     waits, no host synchronisation).  Outputs of a submit are complete once `stream` has passed it.
 *   d_out             the out_* members and counts of lrc_compact_io (device pointers); the input members are ignored.
 *                     The buffers of a submit are written up to two submits later: rotate at least three output buffers
 *                     between lrc_pipe_wait calls.  rays_per_pose % 64 != 0 falls back to scan + compaction per stream.
 *   d_poses16, d_dirs3  are read by the submit's trace on an internal stream, which `stream` does not wait for: leave
 *                     them unchanged until `stream` has passed lrc_pipe_wait, or rotate them like the output buffers.
 *                     The same holds for the inputs of lrc_pipe_submit_sharded.
 *   lrc_pipe_records  the fixed-stride records (lrc_hits, device pointers, tile_count included) of submit `ticket`;
 *                     valid while at most three further submits have been made (four sets rotate; the fourth rewrites
 *                     them).  For a submit that kept only the 12-byte records (rays_per_pose % 64 == 0) the complete records
 *                     are rebuilt first, behind that submit's trace, and the host waits for them: the same bytes
 *                     lrc_scan_poses_dev writes.  The rebuild reads the set, its ray table and the scene, never d_poses16 or
 *                     d_dirs3: it is valid after lrc_pipe_wait, when the caller may have changed them.  A verification surface.
 *   lrc_pipe_trace_ms the time the trace launch of submit `ticket` spent between its stream reaching it and its last wave
 *                     (HIP events on the launch stream; inside the pipeline launches overlap, so this is longer than the
 *                     launch's share of the step).  Synchronises the host with that launch.
 *   lrc_pipe_set_line_width  a hint for submits with rays_per_pose % 64 == 0: the rays of a pose come in scan lines of
 *                     `line_width` consecutive table rows (one elevation each).  A tracing wave then takes 32 columns of two
 *                     adjacent lines instead of 64 columns of one, which keeps its rays together for longer.  0 (the default):
 *                     automatic -- the length of the first run of equal z in the table, read once per table address the
 *                     pipeline has not seen (the first such submit synchronises the host with `stream` for an 8-byte
 *                     read-back; later submits add nothing -- so that first submit must not be made while `stream` is being
 *                     captured into a graph: give the width as a hint there, a hinted pipeline never synchronises).  A width is used when it is a multiple of 64 that divides
 *                     rays_per_pose into at least two lines; otherwise waves take 64 consecutive rays as before.  The width
 *                     only regroups rays into waves, and the regrouping is a bijection of the pose's rays for ANY width: a
 *                     wrong or stale one (another table at a recycled address, a table edited in place) can cost speed,
 *                     never a byte of the rows, counts or records.
 *   lrc_pipe_set_tile_lines  how many adjacent scan lines a tracing wave takes when a line width is in use: 4 (16 columns of
 *                     four lines), 2 (32 columns of two), 1 (64 consecutive rays, whatever the width), or 0 (the default):
 *                     automatic.  Lines are grouped from line 0 and again from the first line whose direction has another z
 *                     sign than line 0's (found with the automatic line width, in the same read-back; a hinted width has no
 *                     such split), so that no wave holds lines above and below the horizon: by fours, then a pair if two or
 *                     three lines remain, then an odd last line as 64 consecutive rays.  Like the width, this only regroups rays
 *                     into waves, bijectively for any value: it never changes a byte.
 *   lrc_pipe_set_ray_table  1 (the default) or 0.  The ray table holds, per row of the direction table, the float32 world
 *                     direction, its guarded reciprocal and its unit vector for the rotation of pose 0 of a submit, so that
 *                     the tracing waves load them instead of forming them per ray in float64.  It is rebuilt on the device for
 *                     every submit with rays_per_pose % 64 == 0 from that submit's own poses and table (nothing is cached by
 *                     address).  A pose whose nine rotation entries are not bit for bit those of pose 0 is traced as without
 *                     a table, pose by pose inside one launch: mixed rotations cost the gain for those poses, never a byte.
 * Destroy the pipeline before its scene. */
typedef struct lrc_pipe lrc_pipe;
int lrc_pipe_create(lrc_scene* scene, uint64_t max_poses, uint64_t rays_per_pose, lrc_pipe** out_pipe);
int lrc_pipe_destroy(lrc_pipe* pipe);
int lrc_pipe_submit(lrc_pipe* pipe, const double* d_poses16, uint64_t num_poses, const double* d_dirs3, double max_range,
                    const lrc_compact_io* d_out, void* stream, uint64_t* out_ticket);
int lrc_pipe_wait(lrc_pipe* pipe, void* stream);
int lrc_pipe_records(lrc_pipe* pipe, uint64_t ticket, lrc_hits* out_records);
int lrc_pipe_trace_ms(lrc_pipe* pipe, uint64_t ticket, float* out_ms);
int lrc_pipe_set_line_width(lrc_pipe* pipe, uint64_t line_width);
int lrc_pipe_set_tile_lines(lrc_pipe* pipe, uint32_t lines);
int lrc_pipe_set_ray_table(lrc_pipe* pipe, int enable);

/* The pipeline on N ranks (one process per GPU; the collective itself is the caller's: RCCL all-gather of the send slabs).
 *   lrc_pipe_submit_sharded  traces this rank's pose block like lrc_pipe_submit, with the triangle ids and per-wave keep counts
 *                            written straight into the caller's send slab (d_send_prim: P * rays_per_pose words,
 *                            d_send_tile_count: one word per 64 rays); `assemble` (nullable) describes an EARLIER scan whose
 *                            slabs of ALL ranks have been gathered: its assembly -- the other ranks' rows rebuilt from their
 *                            ids (lrc_cloud_from_prims_own_dev's arithmetic, bit-identical), this rank's own rows scattered
 *                            from the records of submit `own_ticket` -- rides in the leading workgroups of this trace launch,
 *                            i.e. it runs when the previous launch's tail begins instead of waiting, as a separate kernel of
 *                            4-wave workgroups does, until a trace launch has no workgroup left.  `stream` must already wait
 *                            for the collective that produced the gathered slabs.  At most two submits may lie between
 *                            `own_ticket` and this one (own_ticket >= this submit's ticket - 3): one more, and this
 *                            submit's own trace would rewrite the records the assembly reads.
 *   lrc_pipe_trace_done      `stream` waits for the trace of that submit (the send slab is complete: start the collective).
 *   lrc_pipe_scan_gathered   the scan over the gathered keep counts of ALL ranks and a transposed copy of d_dirs3 (read as it is
 *                            at this point of `stream`), into the offset table of gathered->scan_slot: to be enqueued on the
 *                            communication stream right behind the collective (two small kernels; the launch that carries the
 *                            assembly must wait for them through `stream` of lrc_pipe_submit_sharded).
 *   lrc_pipe_assemble        the same assembly with the plain kernels on `stream` (the last scans of a run), after the scan;
 *                            up to three submits may lie between `own_ticket` and the call.
 * Rows and counts of an assembled scan are complete once the stream has passed lrc_pipe_wait (or lrc_pipe_assemble). */
typedef struct lrc_gathered {
    const double*   d_all_poses16;     /* (num_poses_all,16) the poses of ALL ranks, slab after slab                    */
    uint64_t        num_poses_all;     /* = slabs * poses_per_slab (a rank with fewer poses pads its slab with invalid ids) */
    const uint32_t* d_all_prims;       /* entry 0 of slab 0 of the gathered triangle ids                                 */
    const uint32_t* d_all_tile_counts; /* entry 0 of slab 0 of the gathered per-wave keep counts                         */
    uint64_t        poses_per_slab;
    uint64_t        slab_stride_bytes; /* distance between slabs (ids and counts share it)                               */
    uint64_t        own_slab;          /* this rank's slab                                                               */
    uint64_t        own_ticket;        /* the submit that scanned it; its records must still be there: at most 2 submits
                                          after it for lrc_pipe_submit_sharded, 3 for lrc_pipe_assemble / _scan_gathered  */
    uint64_t        scan_slot;         /* 0 / 1: which of the pipeline's two offset tables lrc_pipe_scan_gathered fills for
                                          this scan (alternate with the gather buffers)                                  */
    float*          d_out_xyzl;        /* (K,4) the assembled rows, np.vstack order                                      */
    uint64_t*       d_counts;          /* (num_poses_all) kept rays per pose, nullable                                   */
} lrc_gathered;
int lrc_pipe_submit_sharded(lrc_pipe* pipe, const double* d_poses16, uint64_t num_poses, const double* d_dirs3, double max_range,
                            uint32_t* d_send_prim, uint32_t* d_send_tile_count, const lrc_gathered* assemble, void* stream,
                            uint64_t* out_ticket);
int lrc_pipe_trace_done(lrc_pipe* pipe, uint64_t ticket, void* stream);
int lrc_pipe_scan_gathered(lrc_pipe* pipe, const double* d_dirs3, const lrc_gathered* gathered, void* stream);
int lrc_pipe_assemble(lrc_pipe* pipe, const double* d_dirs3, const lrc_gathered* gathered, void* stream);

/* ---- scan straight to the reference's variable-length frames ---------------------------------------
 * What S3DISSimulator.run_simulation needs from a whole trajectory (s3dis_simulator.py:254-288): per pose the kept
 * points and their attributes, in ray order.  One call = pose-batched scan (lrc_scan_poses_dev) + stable compaction
 * (lrc_compact_dev) in HBM + the per-pose counts + ONE transfer per requested array of exactly the K kept rows.
 * Frame p is rows [sum(counts[:p]), sum(counts[:p+1])) of every array: np.vstack order
 * (containers/s3dis_sim_scene.py:326).  All pointers are HOST pointers the caller allocated, `capacity` rows each
 * (num_poses * rays_per_pose always suffices; a smaller buffer fails with LRC_ERR_INVALID_ARG and *out_total = K, so
 * that the caller can retry).  counts is required, every other array may be NULL.  Buffers from lrc_host_alloc are
 * page-locked: the transfers then run as DMA at PCIe rate instead of through the runtime's staging copies. */
typedef struct lrc_frames {
    uint64_t* counts;        /* (num_poses) kept rays per pose                                       */
    float*    point3;        /* (K,3)                                                                */
    uint16_t* sem;           /* (K)                                                                  */
    uint16_t* ins;           /* (K)                                                                  */
    double*   incident_deg;  /* (K)                                                                  */
    uint32_t* index;         /* (K) index of the kept ray inside its pose (the surviving-ray list)   */
    float*    xyzl;          /* (K,4) x, y, z, label bits (sem | ins<<16)                            */
    float*    range_origin;  /* (K) see lrc_compact_io.out_range_origin                              */
    /* per-pose statistics, (num_poses) each, computed on the device with numpy's own arithmetic (pairwise summation in
     * 8192-element buffer chunks, every operation in the column's type: csrc/lrc_stats.h), so that they carry the bits
     * np.mean / np.std give on the same frame -- what the reference's ScanQuality records hold
     * (s3dis_simulator.py:276-286); 0 for a pose that kept nothing.  The column itself need not be requested. */
    float*    range_origin_mean;   /* np.mean(np.linalg.norm(points, axis=1)), float32               */
    float*    range_origin_std;    /* np.std(...)                                                    */
    double*   incident_mean;       /* np.mean(incident_angles), float64                              */
    double*   incident_std;        /* np.std(incident_angles)                                        */
} lrc_frames;
int lrc_scan_poses_compact(lrc_scene* scene, const double* poses16, uint64_t num_poses,
                           const double* dirs3, uint64_t rays_per_pose, double max_range,
                           const lrc_frames* out, uint64_t capacity, uint64_t* out_total);

/* ---- scan of a GRID sensor: one wavefront per packet of rays ------------------------------------------------
 * The multi-line sensor's rays form a grid: dirs3[j * width + i] = (cos a_j cos b_i, cos a_j sin b_i, sin a_j) with one
 * elevation a_j per scan line and b_i = az0 + i * az_step covering one turn (IndoorLidar with listed elevations,
 * lidar/indoor_lidar.py:94-131: az0 = pi, az_step = -2 pi / width).  Telling the library so lets it trace a whole packet
 * of rays (one pose x up to 8 lines x 64 azimuths) per wavefront -- the tree is walked once per packet for the
 * packet's frustum, and each surviving triangle runs the exact ray/triangle test only on the few rays whose direction
 * its bounding sphere can contain (csrc/lrc_sector.h) -- instead of once per ray.  Same hit definition, same result
 * BYTES as lrc_scan_poses_dev on the same table (tests assert it); the table itself still supplies the exact float64
 * directions.  Needs width % 64 == 0, width >= 256 and |az_step| * width = 2 pi; the caller vouches that dirs3 HAS
 * this structure (the Python engine derives az0 / az_step from the table and verifies every entry). */
typedef struct lrc_grid {
    uint32_t lines;      /* scan lines H                               */
    uint32_t width;      /* azimuths per line W                        */
    double   az0;        /* azimuth of column 0, radians               */
    double   az_step;    /* azimuth increment per column, radians      */
} lrc_grid;
int lrc_scan_grid_dev(lrc_scene* scene, const double* d_poses16, uint64_t num_poses, const double* d_dirs3,
                      const lrc_grid* grid, double max_range, const lrc_hits* d_out, void* stream);
int lrc_scan_grid_compact(lrc_scene* scene, const double* poses16, uint64_t num_poses, const double* dirs3,
                          const lrc_grid* grid, double max_range, const lrc_frames* out, uint64_t capacity,
                          uint64_t* out_total);

/* ---- a sensor's direction table resident in HBM -------------------------------------------------------------
 * A caller that scans pose after pose with the same sensor (the reference's per-waypoint loop,
 * s3dis_simulator.py:254-264) would upload the same (N,3) float64 table with every call; a table handle uploads it
 * once.  lrc_scan_table_compact is lrc_scan_poses_compact (grid == NULL) or lrc_scan_grid_compact (grid != NULL) on
 * that resident table. */
typedef struct lrc_table lrc_table;
int lrc_table_create(lrc_ctx* ctx, const double* dirs3, uint64_t rays_per_pose, lrc_table** out_table);
int lrc_table_destroy(lrc_table* table);
int lrc_scan_table_compact(lrc_scene* scene, const double* poses16, uint64_t num_poses, const lrc_table* table,
                           const lrc_grid* grid /* nullable */, double max_range, const lrc_frames* out,
                           uint64_t capacity, uint64_t* out_total);

/* ---- moving-sensor sweeps (opt-in) -------------------------------------------------------
 * A spinning sensor on a moving robot fires its rays one after the other during one sweep (0.1 s at 10 Hz), so every ray
 * is cast from its own pose.  Sweep k is described by one MOTION RECORD, 24 float64:
 *   [0..11]  the start pose: the first three rows of the 4x4 matrix, exactly as poses16 holds them
 *   [12..15] dq = (w, x, y, z), unit, w >= cos(pi/4): the world-frame rotation from the start to the end orientation,
 *            R_end = R(dq) R_start (a rotation of at most pi/2 per sweep)
 *   [16..18] dc = c_end - c_start
 *   [19..23] zero
 * and ray i by its FIRING FRACTION fire[i] in [0, 1): the fraction of the sweep at which it fires ((i mod W) / W for a
 * sensor that fires column after column; any table for a sensor that staggers its lasers).  With s = fire[i], ray (k, i) is,
 * every step a separate float64 operation in this order (csrc/lrc_device.h restates it, the tests restate it in numpy):
 *   v    = gen_ray's float64 world direction of dirs3[i] under the start rotation (the dgemm FMA chain of lrc_scan_poses)
 *   qw   = (1 - s) + s*dq.w;   u = (s*dq.x, s*dq.y, s*dq.z)                       nlerp, NOT normalised
 *   n    = ((qw*qw + ux*ux) + uy*uy) + uz*uz;   k = 2/n
 *   t    = u x v  (tx = uy*vz - uz*vy, ty = uz*vx - ux*vz, tz = ux*vy - uy*vx);   w = u x t (same form)
 *   v'_j = v_j + k*(qw*t_j + w_j)                                                 rotation by q/|q|, no square root
 *   c_j  = (s*dc_j == 0) ? c0_j : c0_j + s*dc_j                                   c0 = the start translation
 * direction = float32(v'), origin = float32(c), range-filter centre = c in float64; then exactly lrc_cast.
 * Output index = k*N + i, as lrc_scan_poses_dev.  Properties:
 *   - s = 0 (or dq = (1, 0, 0, 0) and dc = 0) adds signed zeros only: the static ray of lrc_scan_poses, bit for bit.
 *   - no transcendental function anywhere: bit-exact against a host restatement.
 *   - the nlerp angle differs from constant-rate slerp by at most (computed, not measured)
 *         rotation per sweep   0.05 rad   0.1 rad   0.2 rad   0.5 rad   pi/2
 *         max angle error      5.1e-7     4.1e-6    3.3e-5    5.1e-4    1.7e-2  rad
 *   (max over s of |2 atan2(s sin(a/2), 1 - s + s cos(a/2)) - s a| for a rotation a per sweep, rounded up)
 *   lrc_scan_sweeps_dev      device pointers: d_motion24 (P,24), d_dirs3 (N,3), d_fire (N).  The caller vouches for the
 *                            records and the fire table (lrc_scan_sweeps_compact and lrc_table_set_fire check them).
 *   lrc_table_set_fire       attaches a resident fire table (N values in [0, 1), checked) to a direction table; NULL
 *                            detaches it.  Uploaded once, like the direction table.
 *   lrc_scan_sweeps_compact  host records, the resident table with its fire table: compacted in HBM exactly like
 *                            lrc_scan_table_compact (same lrc_frames, counts, index, range_origin, per-pose statistics).
 *                            Rejects non-finite records, dq.w < cos(pi/4) and a non-unit dq with LRC_ERR_INVALID_ARG
 *                            before any launch.
 * lrc_scene_set_options applies unchanged (range_noise_len = num_poses * rays_per_pose). */
int lrc_scan_sweeps_dev(lrc_scene* scene, const double* d_motion24, uint64_t num_poses, const double* d_dirs3,
                        const double* d_fire, uint64_t rays_per_pose, double max_range, const lrc_hits* d_out,
                        void* stream);
int lrc_table_set_fire(lrc_table* table, const double* fire, uint64_t rays_per_pose);
int lrc_scan_sweeps_compact(lrc_scene* scene, const double* motion24, uint64_t num_poses, const lrc_table* table,
                            double max_range, const lrc_frames* out, uint64_t capacity, uint64_t* out_total);

/* ---- seeded sensor noise (opt-in) ------------------------------------------------------------
 * A pose-batched scan whose range noise, angle jitter and dropout are drawn in the kernel, where the ray is made, from a
 * counter-based generator: the noise of ray i of pose p is a pure function of (seed, first_frame + p, i).  It does not
 * depend on call order or chunking, nothing is uploaded, and any frame can be scanned again with its exact noise (P = 6
 * in one call = P = 2 and then P = 4 with first_frame + 2).  The reference declares range_noise_std, angle_noise_std and
 * dropout_probability for the multi-line sensor and never applies them; this is the project's model:
 *   words     Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85),
 *             key = (seed lo, seed hi), counter = (i, frame lo, frame hi, 0), frame = first_frame + p in 64 bits.
 *             w0: range, w1: azimuth jitter, w2: elevation jitter, w3: dropout.  rays_per_pose < 2^32.
 *   normal    z of ONE word w: sign = w >> 31 (set: negative), r = w & 0x7FFFFFFF.  r < 128: |z| = B[23][0] (5.42).  Else
 *             L = leading one of r (7..30), e = 30 - L, below = r - 2^L, c = below >> (L-6),
 *             f = float32(below & (2^(L-6) - 1)) * 2^-(L-6), |z| = fmaf(f, D[e][c], B[e][c]) in float32, with
 *             B[e][c] = float32(Phi^-1(1 - q/2)) at q = 2^-(e+1) (1 + c/64), D[e][c] = (next cell's B) - B[e][c] in float32
 *             (behind c = 63 comes B[e-1][0]; 0 for e = 0).  |z - exact quantile| <= 4.6e-5 + rounding.  Integer and
 *             float32 operations only: the same bits on the host (lrc_noise_draws) and in the kernel.
 *   dropout   the ray is dropped iff w3 < min(floor(dropout * 2^32), 2^32 - 1): never cast, reported as a miss.
 *   jitter    on the float64 table row (a, b, c) in the sensor frame, before the rotation into the world, one float64
 *             operation per step: dp = angle_std*z(w1), dt = angle_std*z(w2), h = sqrt(a*a + b*b), ca = (c*a)/h,
 *             cb = (c*b)/h, a1 = (a - dp*b) - dt*ca, b1 = (b + dp*a) - dt*cb, c1 = c + dt*h,
 *             n = sqrt((a1*a1 + b1*b1) + c1*c1), row = (a1/n, b1/n, c1/n).  A row with h == 0 is left as it is.
 *   range     t' = t + float32(range_std) * z(w0), a float32 multiply then an add; t' <= 0 drops the return; point, range
 *             filter, min_range and incident angle use t' -- the semantics of lrc_scan_options.range_noise.
 * A zero range_std, angle_std or dropout skips its step: the all-zero model returns the bytes of lrc_scan_poses_dev.
 * Negative or non-finite standard deviations, dropout outside [0, 1) and rays_per_pose >= 2^32 fail with
 * LRC_ERR_INVALID_ARG before any launch, and so does a call while a range_noise option is set (one noise source per
 * call); min_range and incident_mode apply unchanged.
 *   lrc_scan_noisy_dev      device pointers, fixed-stride records, as lrc_scan_poses_dev
 *   lrc_scan_noisy_compact  host poses and a resident table: compacted in HBM exactly like lrc_scan_table_compact (same
 *                           lrc_frames, counts, index, range_origin, per-pose statistics)
 *   lrc_noise_draws         host, no GPU: the variates and the keep flags (1 = not dropped) of P x N rays; any output
 *                           may be NULL
 *   lrc_noise_table         host: the table in use, base B and slope D, entry [e*64 + c] */
typedef struct lrc_noise {
    uint64_t seed;
    uint64_t first_frame;   /* frame id of pose 0 of the call */
    double   range_std;     /* metres */
    double   angle_std;     /* radians, azimuth and elevation alike */
    double   dropout;       /* probability in [0, 1) */
} lrc_noise;
int lrc_scan_noisy_dev(lrc_scene* scene, const double* d_poses16, uint64_t num_poses, const double* d_dirs3,
                       uint64_t rays_per_pose, double max_range, const lrc_noise* noise, const lrc_hits* d_out,
                       void* stream);
int lrc_scan_noisy_compact(lrc_scene* scene, const double* poses16, uint64_t num_poses, const lrc_table* table,
                           double max_range, const lrc_noise* noise, const lrc_frames* out, uint64_t capacity,
                           uint64_t* out_total);
int lrc_noise_draws(const lrc_noise* noise, uint64_t num_poses, uint64_t rays_per_pose, float* z_range, float* z_az,
                    float* z_el, uint8_t* keep);
int lrc_noise_table(float* base1536, float* slope1536);

/* ---- noisy moving-sensor sweeps (opt-in) -----------------------------------------------------
 * The two sensor-side effects above in one scan: every ray is cast from the pose of the sensor at the moment it fires AND
 * carries the seeded noise of (seed, first_frame + k, i).  Motion records, firing fractions and lrc_noise are those of the
 * two sections above.  For ray i of sweep k, frame = first_frame + k in 64 bits, every step a separate float64 operation
 * in this order (csrc/lrc_device.h gen_ray_noisy_sweep; tests/test_noisy_sweep_host.py restates it in numpy):
 *   1 words    w = the Philox block of (seed, frame, i), formed only if angle_std != 0 or dropout != 0.  The ray is dropped
 *              iff dropout != 0 and w3 < threshold: never cast, reported as a miss            (the seeded noise's rule)
 *   2 jitter   angle_std != 0: the jitter step on the float64 table row (a, b, c) with dp = angle_std*z(w1),
 *              dt = angle_std*z(w2); a row with h == 0 is left as it is                        (the seeded noise's step)
 *   3 static   v = the dgemm FMA chain of the (jittered) row under the START rotation of motion record k
 *   4 sweep    s = fire[i]: v' = v rotated by q(s)/|q(s)|, c = c(s) with the -0.0-keeping select; direction =
 *              float32(v'), origin = float32(c)                                                (the sweep's steps from v on)
 *   5 range    behind the traversal: the range-filter centre is c(s) in float64, and where range_std != 0 and the ray hit,
 *              t' = t + float32(range_std) * z(w0); t' <= 0 is no return; point, range filter, min_range and incident
 *              angle use t' and c(s)
 *   6 a zero range_std, angle_std or dropout skips its step.
 * Properties, bit for bit: the all-zero model returns the bytes of lrc_scan_sweeps_*; records whose end is their start, and a
 * zero fire table, return the bytes of lrc_scan_noisy_* under the start poses (the sweep then adds signed zeros only to a
 * direction that is never -0.0); P = 6 in one call = P = 2 and then P = 4 with first_frame + 2.
 *   lrc_scan_noisy_sweeps_dev      device pointers.  The caller vouches for the records and the fire table, as in
 *                                  lrc_scan_sweeps_dev; the lrc_noise is checked as in lrc_scan_noisy_dev; a call while a
 *                                  range_noise option is set fails with LRC_ERR_INVALID_ARG.
 *   lrc_scan_noisy_sweeps_compact  host records and the resident table with its fire table: compacted in HBM exactly like
 *                                  lrc_scan_table_compact.  Checks the records as lrc_scan_sweeps_compact and the lrc_noise
 *                                  (for an empty call too); a table without a fire table is refused.
 *   lrc_noisy_sweep_rays           host, no GPU, compiled from the kernel's own generator: per ray the float32 origin and
 *                                  direction (rays6; a dropped ray's direction is NaN), the float64 centre c(s) (centres3),
 *                                  float32(range_std) * z(w0) (range_term; 0 when range_std == 0) and the keep flag (1 = not
 *                                  dropped).  Any output may be NULL.  Checks the lrc_noise, the records and the fire table
 *                                  (values in [0, 1)).
 * min_range and incident_mode apply unchanged. */
int lrc_scan_noisy_sweeps_dev(lrc_scene* scene, const double* d_motion24, uint64_t num_poses, const double* d_dirs3,
                              uint64_t rays_per_pose, const double* d_fire, double max_range, const lrc_noise* noise,
                              const lrc_hits* d_out, void* stream);
int lrc_scan_noisy_sweeps_compact(lrc_scene* scene, const double* motion24, uint64_t num_poses, const lrc_table* table,
                                  double max_range, const lrc_noise* noise, const lrc_frames* out, uint64_t capacity,
                                  uint64_t* out_total);
int lrc_noisy_sweep_rays(const lrc_noise* noise, const double* motion24, uint64_t num_poses, const double* dirs3,
                         const double* fire, uint64_t rays_per_pose, float* rays6, double* centres3, float* range_term,
                         uint8_t* keep);

/* ---- beam footprint and multi-echo returns (opt-in) ------------------------------------------
 * Every other scan casts an infinitely thin ray.  A real beam diverges by a few milliradians; at a table edge or a door
 * frame its footprint straddles two surfaces and the sensor reports two echoes, or one placed on the beam axis.  Here a
 * BEAM is K sub-rays, 1 <= K <= 16, cast in neighbouring lanes of one wave and reduced to at most E echoes, 1 <= E <= 4,
 * behind the traversal; no per-sub-ray record reaches memory.  The reference has nothing of the kind.
 *   offsets   offsets2 is (K, 2) float64 (du_k, dv_k) in radians, supplied by the caller: the library builds no pattern.
 *   sub-ray   k of table row (a, b, c), one float64 operation per step: h = sqrt(a*a + b*b), dp = du_k / h (du is an arc, so
 *             the footprint stays round at high elevation), dt = dv_k, then the jitter step of the seeded noise above on
 *             (a, b, c, dp, dt), then the dgemm chain and the float32 narrowing of lrc_scan_poses_dev.  A sub-ray with
 *             du_k == 0 and dv_k == 0 passes the row through bit for bit; a row with h == 0 is left as it is for every k
 *             (its K sub-rays coincide).
 *   reduce    on the closest-hit distances t_k (float32, before any range filter) of the sub-rays that hit, ordered by
 *             (t_k, k) ascending, s_0 <= s_1 <= ...: a new cluster starts at m = 0 and wherever (s_m - s_(m-1)) > separation
 *             (one float32 subtraction, one compare), so a surface seen at a grazing angle chains into ONE cluster.  A
 *             cluster has weight n_c (its member count), a representative (the member with the smallest k) and a range
 *             (the representative's t).  Clusters with n_c < min_count are discarded; the first E of the rest, ascending,
 *             are echoes 0..E-1; slots that stay empty are miss records.
 *   record    echo e of beam (p, i) is record (p * N + i) * E + e: the record lrc_scan_poses_dev would write for the AXIS
 *             ray (origin and direction of the unjittered row) had it hit the representative's triangle at the echo's
 *             range.  point3 = o + unit(d_axis) * t; the range filter, min_range, incident_deg and intensity use that
 *             point and direction; prim, normal3, sem and ins are the representative's.  d_weight, (P * N * E) uint8 or
 *             NULL, receives n_c, 0 for an empty slot (also where the range filter then drops the record).
 * Properties (tests/test_echo_gpu.py):
 *   P1  K = 1 with offset (0, 0) and E = 1 gives the bytes of lrc_scan_poses_dev.
 *   P2  with offsets2[0] == (0, 0), the echo whose representative is k = 0 equals the clean scan's record of that beam in
 *       every column, incident_deg included.
 *   P3  the result does not depend on pose order or chunking (P = 6 in one call = P = 2 and then P = 4).
 * LRC_ERR_INVALID_ARG before any launch: K or E out of range, min_count outside [1, K], a non-finite offset, a separation
 * that is not finite or <= 0, d_out->tile_count != NULL (a wave no longer writes 64 consecutive records) and a call while
 * a range_noise option is set.  min_range and incident_mode apply unchanged.
 *   lrc_scan_echoes_dev      device pointers; d_out holds P * N * E records.  The offsets are in device memory: the caller
 *                            vouches that they are finite (lrc_scan_echoes_compact checks its host table)
 *   lrc_scan_echoes_compact  host poses and offsets, a resident table: compacted like lrc_scan_table_compact as P poses
 *                            of N * E records, so index = i * E + e; weight_rows, `capacity` bytes or NULL, receives
 *                            the weights of the kept rows, aligned with them (gathered on the device)
 *   lrc_echo_reduce          host, no GPU: the reduction alone.  t is (num_beams, K) float32 with +inf for a sub-ray
 *                            without a hit; out_rep (num_beams, E) int32 receives the representative k of each echo
 *                            (-1: empty slot), out_weight (num_beams, E) uint8 its weight.  Checks the beam as the scans
 *                            do.  The restatement the tests and DESIGN.md point at (csrc/lrc_echo.h). */
typedef struct lrc_beam {
    uint32_t subrays;       /* K */
    uint32_t max_echoes;    /* E */
    uint32_t min_count;     /* clusters of fewer sub-rays are discarded; 1 keeps all */
    float    separation;    /* metres */
} lrc_beam;
int lrc_scan_echoes_dev(lrc_scene* scene, const double* d_poses16, uint64_t num_poses, const double* d_dirs3,
                        uint64_t rays_per_pose, const double* d_offsets2, const lrc_beam* beam, double max_range,
                        const lrc_hits* d_out, uint8_t* d_weight /* nullable */, void* stream);
int lrc_scan_echoes_compact(lrc_scene* scene, const double* poses16, uint64_t num_poses, const lrc_table* table,
                            const double* offsets2, const lrc_beam* beam, double max_range, const lrc_frames* out,
                            uint8_t* weight_rows /* nullable */, uint64_t capacity, uint64_t* out_total);
int lrc_echo_reduce(const float* t, uint64_t num_beams, const lrc_beam* beam, int32_t* out_rep, uint8_t* out_weight);

/* ---- surface materials: glass, mirrors and return intensity (opt-in) ---------------------------
 * Every other scan treats every surface as an opaque, matte sheet.  Here each semantic class has a MATERIAL, and a ray that
 * meets glass or a mirror is continued from its hit point inside the trace kernel: a window is seen only near normal
 * incidence and looked through otherwise, a mirror puts ghost points behind the wall, and the intensity column depends on
 * the surface.  The reference has nothing of the kind.
 *   record    lrc_material, 16 bytes, one per semantic class: kind (0 diffuse, 1 glass, 2 mirror), albedo (the strength of
 *             the surface's own return), pass (the gain kept by a pulse that goes on: transmission of glass, specular
 *             reflectance of a mirror, two-way), retro_cos (the surface answers itself when c >= retro_cos; a value above
 *             1: never).  A semantic id >= num_classes is diffuse with albedo 1.
 *   chain     a ray is a chain of SEGMENTS (o_k, d_k), k = 0, 1, ...; segment 0 is the ray of lrc_scan_poses_dev, bit for
 *             bit.  State: T = +0 (path length), g = 1 (gain), b = 0 (bounces).  All arithmetic is float32 with one
 *             rounding per operation except the fused expression named below.  Per segment:
 *             1 hit       the closest hit of (o_k, d_k) under the library's hit definition: t_k and a triangle -- exactly
 *                         what lrc_cast_dev returns for that ray without centre or filter.  A miss: no return.
 *             2 geometry  h_k = d_k / |d_k| and pp_k = o_k + h_k * t_k as every record's point3 is formed; n the unit
 *                         normal of the record (normal3); c = |fma(hz, nz, fma(hy, ny, hx * nx))| (the intensity
 *                         expression of lrc_hits); T = T + t_k.
 *             3 own       m = the record of the triangle's semantic id.  m.kind == 0 or c >= m.retro_cos: the surface
 *                         returns, the chain ends, I = (g * m.albedo) * c.
 *             4 go on     otherwise b == max_bounces: no return.  Otherwise b = b + 1, g = g * m.pass,
 *                         glass: d_(k+1) = d_k; mirror: dn = (hx * nx + hy * ny) + hz * nz, s = dn + dn,
 *                         d_(k+1) = h_k - s * n per component (not normalised); h_(k+1) = d_(k+1) / |d_(k+1)|,
 *                         o_(k+1) = pp_k + h_(k+1) * skin with skin = 2^-10 m, T = T + skin.
 *             5 record    a return with I < min_intensity is no return.  A return's record is the one lrc_scan_poses_dev
 *                         would write for (o_0, d_0) had it hit the FINAL triangle at range T: point3 lies on the original
 *                         beam at the total path length, where the sensor believes the surface to be; the range filter,
 *                         min_range and incident_deg use that point; prim, normal3, sem and ins are the final surface's;
 *                         intensity is I.  bounces (uint8) receives b and surface_point3 (float32 x 3) the last pp_k, where
 *                         the return physically came from.  A ray without a return (also one the range filter drops) has
 *                         the miss record, bounces = 0 and surface_point3 = 0.
 *             The skin stands in the place of a "skip the triangle I stand on" rule: every segment is an ordinary ray, so
 *             the explicit-ray cast and the CPU oracle trace the chain unchanged.
 * Properties (tests/test_material_gpu.py): an all-diffuse table with albedo 1 gives the bytes of lrc_scan_poses_dev in
 * every column, intensity included; the result does not depend on how the poses are split into calls.
 * LRC_ERR_INVALID_ARG before any launch: num_classes outside [1, 256], max_bounces > 8, a min_intensity that is not finite
 * or outside [0, 1], a kind > 2, an albedo or pass that is not finite or outside [0, 1], a retro_cos that is not finite or
 * negative, a table of another context than the scene's, a call while a range_noise option is set, and a call while
 * incident_mode is 1: the angle between the original beam and the final surface's normal means nothing behind a mirror.
 * min_range applies unchanged; incident_deg (mode 0) is the angle of the reported point, on the original beam, as in every scan.
 * Lifetime: a material table belongs to the context it was created on and must be destroyed BEFORE that context
 * (lrc_material_table_destroy makes the context's device current); the library keeps no list of a context's tables.
 *   lrc_material_table_create   validates `records` (model->num_classes of them, host) and makes them resident
 *   lrc_scan_materials_dev      device pointers; d_out, d_bounces (nullable) and d_surface_point3 (nullable) hold P * N
 *                               entries
 *   lrc_scan_materials_compact  host poses, a resident direction table: compacted like lrc_scan_table_compact;
 *                               intensity_rows (float32), bounces_rows (uint8) and surface_rows (float32 x 3), `capacity`
 *                               rows each or NULL, receive those columns of the kept rows, aligned with them (gathered on
 *                               the device)
 *   lrc_material_step           host, no GPU: step 2 to 5 of ONE segment for n rays, by the inline functions the kernel calls
 *                               (csrc/lrc_material.h).  In: this segment's closest hit per ray (t, +inf or any value that is
 *                               not < +inf for a miss; sem; normal3).  In and out: origin3, dir3, path (T), gain (g), bounces
 *                               (b) and status -- 0 pending, 1 returned, 2 no return; rays that are not pending are left
 *                               alone.  Out for a ray that returns: intensity (I) and surface_point3; a ray that goes on has
 *                               its next segment in origin3 / dir3.  min_intensity is applied to a return. */
typedef struct lrc_material {
    uint32_t kind;          /* 0 diffuse, 1 glass, 2 mirror */
    float    albedo;
    float    pass;
    float    retro_cos;
} lrc_material;
typedef struct lrc_material_model {
    uint32_t num_classes;   /* 1..256 */
    uint32_t max_bounces;   /* 0..8 */
    float    min_intensity;
    uint32_t reserved_;
} lrc_material_model;
typedef struct lrc_material_table lrc_material_table;
int lrc_material_table_create(lrc_ctx* ctx, const lrc_material_model* model, const lrc_material* records,
                              lrc_material_table** out_table);
int lrc_material_table_destroy(lrc_material_table* table);
int lrc_scan_materials_dev(lrc_scene* scene, const double* d_poses16, uint64_t num_poses, const double* d_dirs3,
                           uint64_t rays_per_pose, const lrc_material_table* materials, double max_range,
                           const lrc_hits* d_out, uint8_t* d_bounces /* nullable */, float* d_surface_point3 /* nullable */,
                           void* stream);
int lrc_scan_materials_compact(lrc_scene* scene, const double* poses16, uint64_t num_poses, const lrc_table* table,
                               const lrc_material_table* materials, double max_range, const lrc_frames* out,
                               float* intensity_rows /* nullable */, uint8_t* bounces_rows /* nullable */,
                               float* surface_rows /* nullable */, uint64_t capacity, uint64_t* out_total);
int lrc_material_step(const lrc_material_model* model, const lrc_material* records, uint64_t n, const float* t,
                      const uint16_t* sem, const float* normal3, float* origin3, float* dir3, float* path, float* gain,
                      uint8_t* bounces, uint8_t* status, float* intensity, float* surface_point3);

/* ---- moving objects: rigid movers traced per frame (opt-in) -----------------------------------------
 * Every other scan is of a frozen scene.  Here people, doors and carts stand at a different pose in every frame: a mover
 * occludes the room behind it, the room occludes the mover, and every return says which mover it came from.  The static scene
 * is built once; a frame costs one cast per mover, not a rebuild.  The reference has nothing of the kind.
 *   mover     a rigid triangle mesh with per-triangle sem / ins, modelled around its own origin and held as an ordinary
 *             lrc_scene of the same context.  A mover SET is 1 <= M <= 255 such scenes (lrc_movers_create; the set does not
 *             own them: they must outlive it).
 *   pose      per scan pose p and mover m a MOVER POSE: 12 float32, the row-major 3 x 4 [R | c] from object to world;
 *             mover_poses12 is shaped (P, M, 12).  A mover stands still during a frame.
 *   ray (p, i)   (o, d) is the ray of lrc_scan_poses_dev, bit for bit.  All arithmetic is float32 with one rounding per
 *             operation, nothing fused.
 *             1 static    t_s and a triangle: exactly what lrc_cast_dev returns for (o, d) without centre or filter.  A miss:
 *                         +inf.
 *             2 frame     per mover e = o - c (three subtractions), o'_j = (R[0][j] * e_x + R[1][j] * e_y) + R[2][j] * e_z,
 *                         d'_j the same expression on d, not normalised.  t_m and a triangle: what lrc_cast_dev returns for
 *                         (o', d') on mover m's scene without centre or filter; the finite-ray contract applies to (o', d').
 *             3 merge     both kinds of range are taken before any range filter.  The winner is the smallest of t_s, t_0,
 *                         ..., t_(M-1), compared as float32; on an exact tie the static scene wins over any mover and the
 *                         smaller m wins among movers.
 *             4 record    the record lrc_scan_poses_dev would write for (o, d) had it hit the winner at range t: point3 =
 *                         o + unit(d) * t as every record forms it; the range filter, min_range, incident_deg (both modes)
 *                         and intensity use that point, d and the normal3 that is written.  prim, sem and ins are the
 *                         winner's; prim is the row in the winner's OWN mesh.  For a mover normal3_j = (R[j][0] * n_x +
 *                         R[j][1] * n_y) + R[j][2] * n_z of the mover record's normal, not renormalised.  mover (uint8)
 *                         receives 0 for the static scene and m + 1 for a mover, and 0 where there is no return or the
 *                         filter drops it.  A static hit that the range filter or min_range removes does not uncover a
 *                         mover behind it.
 *   culling   a ray is left out of a mover's cast only when it cannot meet a sphere around the mover's box, enlarged by a
 *             margin far above float32 rounding (csrc/lrc_movers.h): a test the traversal's own root-box test also fails.
 *             It never changes a byte; a ray left out writes no ray record and is not cast (the keep mask of the
 *             explicit-ray launch).
 * Properties (tests/test_movers_gpu.py): a mover that is a copy of the room at the identity pose gives the clean scan's
 * bytes and mover == 0; the result does not depend on how the poses are split into calls.
 * LRC_ERR_INVALID_ARG before any launch: M = 0 or M > 255 in lrc_movers_create, a mover scene of another context, the static
 * scene used as one of its movers, d_out->tile_count != NULL (the merge writes no per-tile keep counts), a call while a
 * range_noise option is set and, in lrc_scan_movers_compact, a mover pose with an entry that is not finite or with
 * max |R^T R - I| > 2^-16 evaluated in float64.  lrc_scan_movers_dev cannot read device poses: its caller vouches for them.
 * A NULL set is allowed in both scan calls: the bytes of lrc_scan_poses_dev and a zero mover column.  min_range and
 * incident_mode of the STATIC scene apply to the merged record; options of the mover scenes are ignored.
 * Lifetime: a set belongs to the context it was created on and must be destroyed BEFORE that context and before its scenes'
 * last use; it holds the scan's scratch (one ray set, one keep column, two record sets: 98 bytes per ray whatever M is), so
 * calls on one set must not overlap on different streams.
 *   lrc_movers_create        `scenes`: num_movers scene handles (host array)
 *   lrc_scan_movers_dev      device pointers; d_out and d_mover (nullable) hold P * N entries; everything is enqueued on
 *                            `stream`, nothing is waited for
 *   lrc_scan_movers_compact  host poses and mover poses, a resident direction table: compacted like lrc_scan_table_compact;
 *                            mover_rows (uint8, `capacity` rows, nullable) receives the mover column of the kept rows,
 *                            aligned with them (gathered on the device)
 *   lrc_mover_rays           host, no GPU: step 2 for n rays and ONE mover pose, by the inline functions the kernels call
 *   lrc_mover_merge          host, no GPU: step 3 and the mover's world normal for n rays of ONE frame.  In: (t, normal3) of
 *                            the static cast, (M, n) ranges and (M, n, 3) normals of the mover casts (+inf or any value that
 *                            is not < the winner's for a miss), (M, 12) poses.  Out: the winner's t, normal3 and mover id. */
typedef struct lrc_movers lrc_movers;
int lrc_movers_create(lrc_ctx* ctx, lrc_scene* const* scenes, uint32_t num_movers, lrc_movers** out_set);
int lrc_movers_destroy(lrc_movers* set);
int lrc_scan_movers_dev(lrc_scene* scene, lrc_movers* set /* nullable */, const double* d_poses16, uint64_t num_poses,
                        const double* d_dirs3, uint64_t rays_per_pose, const float* d_mover_poses12, double max_range,
                        const lrc_hits* d_out, uint8_t* d_mover /* nullable */, void* stream);
int lrc_scan_movers_compact(lrc_scene* scene, lrc_movers* set /* nullable */, const double* poses16, uint64_t num_poses,
                            const lrc_table* table, const float* mover_poses12, double max_range, const lrc_frames* out,
                            uint8_t* mover_rows /* nullable */, uint64_t capacity, uint64_t* out_total);
int lrc_mover_rays(const float* rays6, uint64_t num_rays, const float* pose12, float* out_rays6);
int lrc_mover_merge(uint64_t num_rays, uint32_t num_movers, const float* t_static, const float* normal3_static,
                    const float* t_movers, const float* normal3_movers, const float* poses12, float* out_t,
                    float* out_normal3, uint8_t* out_mover);

/* ---- movers under moving-sensor sweeps: per-ray mover pose (opt-in) ----------------------------------
 * The two features above, composed: ray i of sweep k fires at s = fire[i], is cast from the sensor pose at s (exactly the ray of
 * lrc_scan_sweeps_dev, bit for bit) and meets every mover at THAT MOVER'S pose at s.  A person who walks through a 0.1 s sweep is
 * sheared and stretched as in real data; a mover that stands still gives the bytes of lrc_scan_movers_*.
 *   record    per sweep k and mover m a MOVER SWEEP RECORD: 24 float32, shaped (P, M, 24)
 *               [0..11]  the mover's pose12 at the START of the sweep
 *               [12..15] dq = (w, x, y, z), w >= cos(pi/4): R_end = R(dq) R_start
 *               [16..18] dc = c_end - c_start
 *               [19..23] zero
 *             The mover moves between the two poses as the sensor does between its own: the centre straight, the rotation by
 *             nlerp (the error table of the moving-sensor sweeps applies).
 *   ray (k, i)  s = (float)fire[i].  All mover arithmetic is float32, one rounding per operation, nothing fused, in this order:
 *               c_j = c0_j + s*dc_j;   qw = (1 - s) + s*dq.w;   u = (s*dq.x, s*dq.y, s*dq.z)
 *               n = ((qw*qw + ux*ux) + uy*uy) + uz*uz;   k = 2/n
 *               for a vector v:  t = u x v, w = u x t  (tx = uy*vz - uz*vy, ty = uz*vx - ux*vz, tz = ux*vy - uy*vx; w alike)
 *                                forward R(q) v:   v'_j = v_j + k*(qw*t_j + w_j)
 *                                inverse R(q)^T v: v'_j = v_j + k*(w_j - qw*t_j)
 *             2 frame   e = o - c;  o' = R_start^T inverse(e),  d' = R_start^T inverse(d)  (R_start^T as step 2 of the moving
 *                       objects forms it)
 *             4 record  normal3 = forward(R_start n) of the mover record's normal n (R_start n as step 4 there), not renormalised;
 *                       the record is the one lrc_scan_sweeps_dev would write for (o, d) had it hit the winner: point3 on the world
 *                       ray, the range filter about the sensor's centre c(s) in float64
 *             Steps 1 and 3, the tie rule, the culling and the options are those of the moving objects, unchanged.
 *   still     a record whose word 12 has the bits of 1.0f and whose words 13..18 are all +0.0f takes steps 2 and 4 of the moving
 *             objects with its pose12: the same bytes as lrc_scan_movers_dev when the sensor stands still too.
 * The record interpolates between the poses at the two ends of the sweep and nothing else: a path that turns a corner inside a
 * sweep is cut straight.
 * LRC_ERR_INVALID_ARG before any launch: what lrc_scan_movers_* refuse (a range_noise option among it), d_out->tile_count != NULL
 * and, in lrc_scan_mover_sweeps_compact, what lrc_scan_sweeps_compact refuses (no fire table, a bad sensor record) and a mover
 * sweep record with an entry that is not finite, a start pose with max |R^T R - I| > 2^-16 or dq.w < cos(pi/4) (as float32).
 * A NULL set: the bytes of lrc_scan_sweeps_dev and a zero mover column.  Scratch: the set's, 122 bytes per ray whatever M is.
 *   lrc_scan_mover_sweeps_dev      device pointers, as lrc_scan_sweeps_dev and lrc_scan_movers_dev take them; enqueued on `stream`
 *   lrc_scan_mover_sweeps_compact  host records, the resident table with its fire table; frames and mover_rows as
 *                                  lrc_scan_movers_compact (the index column gives each point's firing fraction)
 *   lrc_mover_sweep_rays           host, no GPU: step 2 for n world rays with their own fire[i] and ONE record
 *   lrc_mover_sweep_normals        host, no GPU: step 4's normal for n normals with their own fire[i] and ONE record */
int lrc_scan_mover_sweeps_dev(lrc_scene* scene, lrc_movers* set /* nullable */, const double* d_motion24, uint64_t num_poses,
                              const double* d_dirs3, const double* d_fire, uint64_t rays_per_pose, const float* d_mover_motion24,
                              double max_range, const lrc_hits* d_out, uint8_t* d_mover /* nullable */, void* stream);
int lrc_scan_mover_sweeps_compact(lrc_scene* scene, lrc_movers* set /* nullable */, const double* motion24, uint64_t num_poses,
                                  const lrc_table* table, const float* mover_motion24, double max_range, const lrc_frames* out,
                                  uint8_t* mover_rows /* nullable */, uint64_t capacity, uint64_t* out_total);
int lrc_mover_sweep_rays(const float* rays6, const double* fire, uint64_t num_rays, const float* motion24, float* out_rays6);
int lrc_mover_sweep_normals(const float* normal3, const double* fire, uint64_t num_rays, const float* motion24,
                            float* out_normal3);

/* ---- seeded sensor noise under movers (opt-in) ---------------------------------------------------------
 * The moving objects and the seeded sensor noise, composed: a frame with people in it that has range noise, angle jitter and
 * dropped returns, drawn in the kernels and reproducible bit for bit.  The noise cannot be added afterwards: the jitter decides
 * which surface a ray meets, the room or a mover; a dropped ray is never cast; the range filter and min_range act on the noisy
 * range.  float32 with one rounding per operation and nothing fused, except where the seeded sensor noise fuses (the quantile's
 * one fmaf).  The noise of ray i of pose p is the Philox block of (seed, first_frame + p, i): the words w0..w3 of the seeded
 * sensor noise.
 *   1 dropout   dropout != 0 and w3 < thr: the ray is dropped.  It is cast against neither the room nor any mover; its record is a
 *               miss and its mover byte is 0.
 *   2 jitter    angle_std != 0: the table row is jittered in the sensor frame before the rotation into the world, as there.  (o, d)
 *               is the ray of lrc_scan_noisy_dev, bit for bit.  That ray is taken into every mover's frame and culled: steps 1-3
 *               of the moving objects, unchanged, on the jittered ray.
 *   3 winner    decided on the CLEAN ranges: the smallest float32 t of t_s, t_0, ..., t_(M-1) wins; on an exact tie the static
 *               scene, then the smaller m.  The range draw is one measurement error per ray: it does not reorder surfaces.
 *   4 range     range_std != 0: t' = t_winner + float32(range_std) * z(w0), a float32 multiply, then an add; t' <= 0 is no
 *               return.  The record is step 4 of the moving objects at t': the point, the range filter, min_range, incident_deg
 *               (both modes) and intensity use t', the jittered d and the winner's written normal; prim, sem and ins are the
 *               winner's; the mover byte is the winner's where the record is kept and 0 elsewhere.
 *   5 zeros     a zero parameter skips its step (wave-uniform branches on kernel arguments).  The all-zero model gives the bytes
 *               of lrc_scan_movers_dev; a NULL set gives the bytes of lrc_scan_noisy_dev and a zero mover column.
 * The result does not depend on how the poses are split into calls when each call brings its own first_frame.
 * LRC_ERR_INVALID_ARG before any launch, the offender named: what lrc_scan_noisy_dev refuses (a NULL model, a negative or
 * non-finite standard deviation, dropout outside [0, 1), rays_per_pose >= 2^32, a range_noise option) and what lrc_scan_movers_*
 * refuse (the static scene among the movers, a set or table of another context, d_out->tile_count != NULL and, in the compact
 * call, a bad mover pose).  min_range and incident_mode of the STATIC scene apply, as there.
 * Scratch: the set's, grown under the same rule: what lrc_scan_movers_dev holds there plus the world ray set and the live
 * column, 123 bytes per ray whatever M is.
 *   lrc_scan_noisy_movers_dev      device pointers, as lrc_scan_movers_dev takes them, and the model; enqueued on `stream`,
 *                                  nothing is waited for
 *   lrc_scan_noisy_movers_compact  lrc_scan_movers_compact with the model: pose p of the call is frame first_frame + p; frames
 *                                  and mover_rows as there */
int lrc_scan_noisy_movers_dev(lrc_scene* scene, lrc_movers* set /* nullable */, const double* d_poses16, uint64_t num_poses,
                              const double* d_dirs3, uint64_t rays_per_pose, const float* d_mover_poses12, double max_range,
                              const lrc_noise* noise, const lrc_hits* d_out, uint8_t* d_mover /* nullable */, void* stream);
int lrc_scan_noisy_movers_compact(lrc_scene* scene, lrc_movers* set /* nullable */, const double* poses16, uint64_t num_poses,
                                  const lrc_table* table, const float* mover_poses12, double max_range, const lrc_noise* noise,
                                  const lrc_frames* out, uint8_t* mover_rows /* nullable */, uint64_t capacity,
                                  uint64_t* out_total);

/* ---- scene flow under movers: per-point flow and visibility at the next frame (opt-in) ----------------
 * For every return of a frame scanned with movers: where the surface the point lies on will be at a NEXT frame, and whether
 * that place can be seen from the next sensor pose (the occlusion mask of scene-flow benchmarks).  "Next" is given per frame,
 * so a caller pairs frames as it likes (k -> k + 1, backward flow, k -> k + 2) and the result does not depend on how frames are
 * split into calls.  The reference has nothing of the kind.
 * Row (p, i) is a record of lrc_scan_movers_dev: x = point3 (float32), w = mover (0: the room, m + 1: mover m; a w above M is
 * read as 0).  Per frame p: A = mover_poses12[p] (the poses the row was scanned with), B = next_mover_poses12[p], the sensor
 * pose next_poses16[p] to be seen from, has_next[p] (uint8; a NULL pointer means all ones).
 *   1 target  w == 0, or the 48 bytes of A[w-1] and B[w-1] are equal: y = x.  Otherwise in float64, one rounding per operation,
 *             nothing fused: e = x - c_A; q_j = (R_A[0][j] e_x + R_A[1][j] e_y) + R_A[2][j] e_z;
 *             y_j = ((R_B[j][0] q_x + R_B[j][1] q_y) + R_B[j][2] q_z) + c_B,j
 *   2 flow    flow3_j = float32(y_j - x_j); a room point or a mover that stands still gives +0 in all three components
 *   3 sight   y32 = float32(y); o = float32(next_pose[:3,3]); d = y32 - o, L = sqrt((d_x^2 + d_y^2) + d_z^2), h = d / L, all
 *             float32.  dist = the float64 distance of y32 from the float64 translation of the next pose, as the scan's range
 *             filter forms it: sqrt((e_x^2 + e_y^2) + e_z^2), e = float64(y32) - c.  Unless dist < max_range (and, with the
 *             static scene's min_range > 0, dist >= min_range) the row is OUT OF RANGE (3) and not cast.
 *   4 ranges  t_s = what lrc_cast_dev returns for (o, h) on the room without centre or filter; per mover t_m = what it returns
 *             on mover m's scene for the ray taken into its frame with B[m] (step 2 of the moving objects).  Culling as there:
 *             it never changes a byte.  A ray that is not finite is not cast (the finite-ray contract): a miss.
 *   5 status  thr = L - 2^-12 * max(L, 1) in float32 (the product is exact: one rounding).  OCCLUDED (2) iff
 *             min(t_s, t_0, ..., t_(M-1)) < thr compared as float32, else VISIBLE (1).  The surface the point lies on is itself
 *             met at about L; the margin keeps it from counting (measured: DESIGN.md section 5m).
 *   6 a row without a return (t = +inf), or of a frame with has_next[p] == 0: +0 flow and status NONE (0).
 * Status 1 means line of sight and range, not that a scan line of the next frame lands there (no field-of-view test).
 * LRC_ERR_INVALID_ARG before any launch: what lrc_scan_movers_* refuse (a set of another context, the static scene among its
 * movers, a range_noise option, NULL scene or records), a NULL flow3 / flow_rows, records without t or point3, a NULL mover
 * column with a set, NULL next sensor poses, NULL mover poses (either table) with a set and, in lrc_scan_flow_compact, what
 * lrc_scan_movers_compact refuses, applied to both mover pose tables.
 *   lrc_scan_flow_dev      device pointers; everything is enqueued on `stream`, nothing is waited for.  d_records: t and point3
 *                          of P * N records; d_flow3 (P * N, 3) float32; d_status (P * N) uint8, NULL: the flow alone, nothing
 *                          is cast.  A NULL set: zero flow and line of sight against the room alone.  Scratch lives in the set
 *                          (in the scene without one) and does not grow with M; calls that share it must share a stream.
 *   lrc_scan_flow_compact  what lrc_scan_movers_compact takes plus the next sensor poses (P, 16), the next mover poses
 *                          (P, M, 12) and has_next (P, nullable), all on the host: the mover scan and the flow at the fixed
 *                          stride, compacted; flow_rows (capacity, 3) float32 and status_rows (capacity) uint8 (nullable: the
 *                          flow alone) receive the two columns of the kept rows, gathered like mover_rows.
 *   lrc_flow_rays          host, no GPU: steps 1 to 3 for P frames of N rows by the inline functions the kernels call.  Out per
 *                          row: flow3, the ray (o, h) as rays6, keep (1: to be cast), thr and the status so far (0, 3, or 1 for
 *                          a row that is cast); the ray and thr of a row that is not cast are zero.
 *   lrc_flow_status        host, no GPU: step 5 for n rows.  In: the static cast's ranges (n), the mover casts' (M, n) (+inf for
 *                          a miss or a ray not cast), thr and the status of lrc_flow_rays.  Out: rows of status 1 judged, every
 *                          other row's status unchanged. */
#define LRC_FLOW_NONE 0
#define LRC_FLOW_VISIBLE 1
#define LRC_FLOW_OCCLUDED 2
#define LRC_FLOW_OUT_OF_RANGE 3
int lrc_scan_flow_dev(lrc_scene* scene, lrc_movers* set /* nullable */, const lrc_hits* d_records, const uint8_t* d_mover,
                      uint64_t num_poses, uint64_t rays_per_pose, const float* d_mover_poses12, const float* d_next_mover_poses12,
                      const double* d_next_poses16, const uint8_t* d_has_next /* nullable */, double max_range, float* d_flow3,
                      uint8_t* d_status /* nullable */, void* stream);
int lrc_scan_flow_compact(lrc_scene* scene, lrc_movers* set /* nullable */, const double* poses16, uint64_t num_poses,
                          const lrc_table* table, const float* mover_poses12, const double* next_poses16,
                          const float* next_mover_poses12, const uint8_t* has_next /* nullable */, double max_range,
                          const lrc_frames* out, uint8_t* mover_rows /* nullable */, float* flow_rows,
                          uint8_t* status_rows /* nullable */, uint64_t capacity, uint64_t* out_total);
int lrc_flow_rays(const float* t, const float* point3, const uint8_t* mover, uint64_t num_poses, uint64_t rays_per_pose,
                  uint32_t num_movers, const float* mover_poses12, const float* next_mover_poses12, const double* next_poses16,
                  const uint8_t* has_next /* nullable */, double max_range, double min_range, float* out_flow3, float* out_rays6,
                  uint8_t* out_keep, float* out_thr, uint8_t* out_status);
int lrc_flow_status(uint64_t num_rows, uint32_t num_movers, const float* t_static, const float* t_movers, const float* thr,
                    const uint8_t* status, uint8_t* out_status);

/* ---- deforming movers: keyframed meshes blended and refitted on the device (opt-in) -----------------
 * A DEFORMABLE is one topology (tris3) with K keyframes of its V vertices.  lrc_deform_create builds an ordinary lrc_scene from
 * keyframe 0 by the builders of lrc_scene_create (device or host as that call chooses), always with float32 nodes whatever
 * LRC_QNODES says (the quantisation grid is tied to bounds that a deformation moves): its arrays for keyframe 0 are the bytes
 * of lrc_scene_create under LRC_QNODES=0.  Creation is synchronous.  The deformable keeps the keyframes, tris3, the current
 * vertices and a height table of the tree resident, and owns the scene: lrc_deform_scene hands it out, lrc_scene_destroy on
 * it is refused, lrc_deform_destroy frees it.
 *
 * lrc_deform_set_dev ENQUEUES on `stream`, without a host synchronisation, the next shape and the refit of the scene to it:
 *   blend    per coordinate v = a + w * (b - a) of keyframes k0 (a) and k1 (b), then clamped into [min(a, b), max(a, b)]
 *            (float32, one rounding per operation, nothing fused): a blended vertex lies in the box of its two keyframes
 *            exactly.  w == 0 or k0 == k1 copies the bits of keyframe k0, w == 1 those of k1.
 *   refit    per leaf slot the 48-byte record (v0, e1, e2, Ng) and the slot box of its triangle from the current vertices, by
 *            the builders' own expressions; then per inner node, height by height from the leaves up, both child boxes: a
 *            leaf child's box is the min / max over its <= 4 slot boxes, an inner child's the min / max of that node's two
 *            boxes, in the builders' total order (-0 below +0).  An empty leaf keeps its all-zero box.  References, slot_prim,
 *            slot_label and the three padding records are not touched; the tree keeps the splits of keyframe 0.
 * Any tree whose child boxes are the exact vertex min / max below them gives the same hits bit for bit, so every cast and
 * scan call takes the scene as the ordinary scene it is, as the static scene or as a mover of a set, and returns what a fresh
 * lrc_scene_create of the current vertices returns.  A scan enqueued on the SAME stream after lrc_deform_set_dev sees the new
 * shape and needs no wait; calls on other streams, and the host-pointer calls (they run on streams of the library), are the
 * caller's to order (synchronise the stream of the set first).
 * info.bounds_lo / bounds_hi of the scene are the union of ALL keyframes' boxes and never change; the movers' cull sphere is
 * made from them.  Entry points that cache per-triangle geometry of a scene refuse a deformable scene (LRC_ERR_INVALID_ARG):
 * the plane table behind lrc_cloud_from_prims_dev / _own_dev, the gathered rebuild of a pipe and LRC_ARRAY_PRIM_PLANE.  lrc_coverage_create
 * and lrc_frameobj_create take a mesh, not a scene: their tables describe the vertices they were given and nothing else.
 *
 * LRC_ERR_INVALID_ARG before any launch: K = 0, T = 0, a keyframe entry that is not finite or above 1e6 in magnitude, a
 * triangle index >= V (lrc_deform_create); k0 or k1 >= K, w outside [0, 1] or not finite (lrc_deform_set_dev).
 *
 *   lrc_deform_create    keyframes3: host (K, V, 3) float32; tris3, tri_sem, tri_ins as lrc_scene_create takes them
 *   lrc_deform_vertices  synchronous read-back of the current (V, 3) vertices (waits for the device)
 *   lrc_deform_launches  kernel launches one lrc_deform_set_dev enqueues: with a blend, and with a keyframe copy instead
 * Host functions, no GPU, by the inline functions the kernels call:
 *   lrc_deform_blend     out3 = blend of a3 and b3 ((num_vertices, 3) float32 each); a3 == b3, w == 0 and w == 1 copy
 *   lrc_deform_refit     nodes16 in: the topology (references), out: the boxes; out_tri_rec12 (num_slots, 12) and
 *                        out_slot_box6 (num_slots, 6) are written.  LRC_ERR_INVALID_ARG for nodes that are no tree over the
 *                        slots, a slot_prim entry >= T or a triangle index >= V. */
typedef struct lrc_deform lrc_deform;
int lrc_deform_create(lrc_ctx* ctx, const float* keyframes3, uint32_t K, uint64_t V, const uint32_t* tris3, uint64_t T,
                      const uint16_t* tri_sem, const uint16_t* tri_ins, lrc_deform** out);
int lrc_deform_destroy(lrc_deform* deform);
lrc_scene* lrc_deform_scene(lrc_deform* deform);
int lrc_deform_set_dev(lrc_deform* deform, uint32_t k0, uint32_t k1, float w, void* stream);
int lrc_deform_vertices(lrc_deform* deform, float* out_verts3);
int lrc_deform_launches(const lrc_deform* deform, uint32_t* blended, uint32_t* copied);
int lrc_deform_blend(const float* a3, const float* b3, uint64_t num_vertices, float w, float* out3);
int lrc_deform_refit(float* nodes16, uint64_t num_nodes, const uint32_t* slot_prim, uint64_t num_slots, const uint32_t* tris3,
                     uint64_t T, const float* verts3, uint64_t V, float* out_tri_rec12, float* out_slot_box6);

/* ---- skinned deforming movers: bone poses skinned and refitted on the device (opt-in) ----------------
 * A SKINNED deformable keeps no keyframes.  It keeps a REST shape (V, 3), up to four bone influences per vertex -- idx4 (V, 4)
 * uint8 bone indices and wgt4 (V, 4) float32 weights; an unused influence carries weight +0 and any valid index -- and K KEY
 * POSES of B bones, poses12 (K, B, 12) float32: a bone pose is the row-major 3 x 4 [A | c] of a mover pose, any affine map (no
 * orthonormality is demanded).  Key pose k is "keyframe k": the vertices of key pose k are, per vertex at rest position
 * (x, y, z), with all four influences always evaluated in index order and m = bones + 12 * idx[j],
 *   p_j.i = ((m[4i] * x + m[4i+1] * y) + m[4i+2] * z) + m[4i+3]
 *   v.i   = ((wgt0 * p_0.i + wgt1 * p_1.i) + wgt2 * p_2.i) + wgt3 * p_3.i
 * (float32, one rounding per operation, nothing fused), and lrc_deform_set_dev(k0, k1, w) gives blend(skin(pose k0),
 * skin(pose k1), w) by the blend above; for w == 0, w == 1 or k0 == k1 it is the skin of the one pose and nothing is blended.
 * Those are the bytes a keyframe deformable made from the host-skinned keyframes (lrc_skin_apply per key pose) holds after the
 * same call, so everything said above about the refit, the scans, the bounds and the refusing entry points holds as it stands.
 * The handle IS an lrc_deform: lrc_deform_scene, lrc_deform_set_dev (one skinning launch in place of the blend or the copy),
 * lrc_deform_vertices, lrc_deform_snapshot_dev, lrc_deform_launches (both counts are 1 + the refit's) and lrc_deform_destroy
 * take it.  It keeps resident 12 + 4 + 16 = 32 bytes per vertex and 48 bytes per bone and key pose, counted in
 * info.device_bytes, where the keyframe route keeps 12 bytes per vertex and keyframe.
 *
 * lrc_deform_create_skinned skins the K key poses on the host, one at a time, keeping none but key pose 0, from which the scene
 * is built; the scene's fixed bounds are the union box of all key poses over the vertices triangles use.  Synchronous.
 * LRC_ERR_INVALID_ARG before any launch, the message naming the offender: B outside 1 .. 255, K = 0, T = 0, a triangle index
 * >= V, a bone index >= B, a weight that is not finite or is negative, a vertex whose weights (summed in float64) lie further
 * than 2^-10 from 1, a pose entry that is not finite, a key pose that puts a vertex at a coordinate that is not finite or
 * exceeds 1e6 (the key pose is named).  The arrays are checked before the context, so all of this is refused without a GPU.
 *   lrc_skin_apply  host, no GPU, by the inline function the kernel calls: out3 (V, 3) = the vertices under ONE pose's
 *                   bones12 (B, 12).  Refuses B outside 1 .. 255 and a bone index >= B; weights are taken as they are.
 * Not built: a shape from a pose that is not in the clip (a set_pose_dev): the scene's bounds and the movers' cull sphere
 * would need a bound on vertices the host has never seen. */
int lrc_skin_apply(const float* rest3, uint64_t V, const uint8_t* idx4, const float* wgt4, const float* bones12, uint32_t B,
                   float* out3);
int lrc_deform_create_skinned(lrc_ctx* ctx, const float* rest3, uint64_t V, const uint8_t* idx4, const float* wgt4,
                              const float* poses12, uint32_t K, uint32_t B, const uint32_t* tris3, uint64_t T,
                              const uint16_t* tri_sem, const uint16_t* tri_ins, lrc_deform** out);

/* ---- non-rigid scene flow: the flow of deforming movers (opt-in) -----------------------------------------
 * The scene flow above for a set with deformables: a row on a deforming triangle flows to where ITS point of the triangle is in
 * the next shape at the next pose, not to the rigid step.  A row has x = point3, w = mover, j = prim (a mover scan's prim is the
 * row in the winner's own mesh).  A SURFACE PAIR for mover m = w - 1 is two vertex arrays of that mover's deformable: VA (the
 * shape the row was scanned with) and VB (the next shape), (V, 3) float32 each, with the deformable's tris3 and T.  A row has no
 * pair if its mover has none, if j >= T, or if w == 0 or w > M: it takes steps 1 and 2 of the scene flow unchanged.  A row with
 * a pair, in float64, one rounding per operation, nothing fused:
 *   1  q = R_A^T (x - c_A), by the expressions of step 1 there
 *   2  (i0, i1, i2) = tris3[j]; a_k = float64(VA[i_k])
 *   3  e1 = a1 - a0, e2 = a2 - a0, r = q - a0
 *   4  dot products as (p_x q_x + p_y q_y) + p_z q_z: d11 = e1.e1, d12 = e1.e2, d22 = e2.e2, r1 = r.e1, r2 = r.e2
 *   5  den = d11 * d22 - d12 * d12
 *   6  u = (d22 * r1 - d12 * r2) / den, v = (d11 * r2 - d12 * r1) / den; unless den > 0, u = v = 0 (a triangle without area
 *      yields no NaN)
 *   7  s = (1 - u) - v; no clamp
 *   8  D_k = float64(VB[i_k]) - a_k.  If all nine components compare equal to zero, z = q with no addition: a triangle that keeps
 *      its shape gives the rigid step's bytes.  Otherwise z_c = q_c + ((s * D0_c + u * D1_c) + v * D2_c): the DISPLACEMENT is
 *      interpolated, not the position, so what the float32 point lies off its plane by is carried along, not lost
 *   9  y = R_B z + c_B, by the expressions of step 1 there
 *  10  y = x, and +0 flow, if and only if the two poses have the same 48 bytes AND all D_k are zero
 * From y on, steps 2 to 6 of the scene flow apply as they stand.  The status is cast against the movers' scenes AS THEY STAND on
 * `stream`: the caller has set the next shape (lrc_deform_set_dev) before the call, on the same stream.
 *   lrc_deform_snapshot_dev     enqueues on `stream` a copy of the deformable's current (V, 3) vertices into a caller's device
 *                               buffer, with no wait: what a caller keeps as VA before it sets the next shape.  Refuses NULL.
 *   lrc_scan_nonrigid_flow_dev  lrc_scan_flow_dev plus `pairs`: at most 16 per call, handed to the kernel in its arguments (no
 *                               table upload, no host synchronisation); all P frames of a call share them, so a caller whose
 *                               shapes change every frame calls it per frame.  A NULL d_verts_b3 means the deformable's current
 *                               vertices.  The records need prim as well as t and point3.  num_pairs == 0 gives
 *                               lrc_scan_flow_dev's bytes.  LRC_ERR_INVALID_ARG before any launch: what lrc_scan_flow_dev
 *                               refuses; num_pairs > 16, or NULL pairs with num_pairs > 0; a pair whose mover >= M or whose
 *                               mover is not a deformable's scene; a mover listed twice; a NULL d_verts_a3; records without prim.
 *   lrc_nonrigid_flow_rays      host, no GPU: lrc_flow_rays plus prim and host pairs, by the inline functions the kernel calls.
 *                               LRC_ERR_INVALID_ARG for more than 16 pairs, a mover >= M or listed twice, a NULL array of a pair
 *                               or a triangle index >= V.  lrc_flow_status serves as it is. */
typedef struct lrc_surface_pair {
    uint32_t mover;                /* m: the rows with w == m + 1 */
    const float* d_verts_a3;       /* (V, 3) device: the shape the rows were scanned with */
    const float* d_verts_b3;       /* (V, 3) device: the next shape; NULL: the deformable's current vertices */
} lrc_surface_pair;
typedef struct lrc_surface_pair_host {
    uint32_t mover;
    const float* verts_a3;         /* (V, 3) host */
    const float* verts_b3;         /* (V, 3) host */
    const uint32_t* tris3;         /* (T, 3) host */
    uint64_t T, V;
} lrc_surface_pair_host;
int lrc_deform_snapshot_dev(lrc_deform* deform, float* d_out_verts3, void* stream);
int lrc_scan_nonrigid_flow_dev(lrc_scene* scene, lrc_movers* set /* nullable */, const lrc_hits* d_records, const uint8_t* d_mover,
                               uint64_t num_poses, uint64_t rays_per_pose, const float* d_mover_poses12,
                               const float* d_next_mover_poses12, const double* d_next_poses16,
                               const uint8_t* d_has_next /* nullable */, double max_range, const lrc_surface_pair* pairs,
                               uint32_t num_pairs, float* d_flow3, uint8_t* d_status /* nullable */, void* stream);
int lrc_nonrigid_flow_rays(const float* t, const float* point3, const uint8_t* mover, const uint32_t* prim, uint64_t num_poses,
                           uint64_t rays_per_pose, uint32_t num_movers, const float* mover_poses12,
                           const float* next_mover_poses12, const double* next_poses16, const uint8_t* has_next /* nullable */,
                           double max_range, double min_range, const lrc_surface_pair_host* pairs, uint32_t num_pairs,
                           float* out_flow3, float* out_rays6, uint8_t* out_keep, float* out_thr, uint8_t* out_status);

/* ---- animated movers under sweeps: a per-ray shape traced on the device (opt-in) ------------------------
 * Under lrc_scan_mover_sweeps_* a mover has a per-ray POSE; a deformable that was merely set keeps ONE shape for the whole
 * sweep.  A SPANNED deformable has a per-ray SHAPE as well.  lrc_deform_span_dev gives it two end shapes, A = (k0a, k1a, wa)
 * and B = (k0b, k1b, wb), each the vertices lrc_deform_set_dev of that triple gives (VA, VB; keyframe and skinned route alike),
 * and ray i of a sweep, with s = (float)fire[i] -- the fraction the mover's pose is taken at -- meets the mover at the vertices
 *   span_vertex(a, b, s) = a                    if s == 0 or a and b have the same bits
 *                          b                    if s == 1
 *                          blend(a, b, s)       otherwise: v = a + s * (b - a), clamped into [min(a, b), max(a, b)]
 * per coordinate (float32, one rounding per operation, nothing fused; the blend of the deforming movers above, whose copy rule
 * the three cases are).  The hit is the library's own, unchanged: with the 48-byte record and the vertex box the builders form
 * from the ray's own three blended vertices, the Moeller-Trumbore conditions and the box clause against that box, the smallest
 * t, and on an exact tie the smaller triangle row.  So a ray's t, prim, normal3, sem and ins are, bit for bit, what lrc_cast_dev
 * returns for that ray on a fresh lrc_scene_create of span_vertex(VA, VB, s); the mover's pose per ray, the merge with the room
 * and the other movers, the filter and the record are those of the movers under moving-sensor sweeps, untouched.  A shape that
 * does not change (A == B), or a fire table of zeros, gives the bytes of the scan with the deformable set to A.
 *
 * lrc_deform_span_dev ENQUEUES on `stream`, with no host wait: shape A into the deformable's vertices and the slot refit of
 * lrc_deform_set_dev for it (records and exact slot boxes are A's: every OTHER entry point that takes the scene returns shape
 * A's bytes, only its node boxes are larger than need be); shape B into a second vertex array; per leaf slot the SPAN BOX, the
 * min / max of the triangle's vertex boxes at A and at B, and the slot's six vertices gathered side by side; the node refit
 * of lrc_deform_set_dev from the span boxes.  The tree is never rebuilt.  Every blended coordinate lies between its two ends
 * exactly, so every blended triangle's box lies inside its slot's span box and no box test prunes a hit.  The call marks the
 * deformable SPANNED; lrc_deform_set_dev clears the mark and restores the one-shape scan.  lrc_scan_mover_sweeps_dev / _compact
 * trace a spanned deformable of the set per ray and everything else as before.  The extra arrays (12 bytes per vertex, 104
 * bytes per leaf slot) are allocated by the first call, counted in info.device_bytes and freed by lrc_deform_destroy.
 * LRC_ERR_INVALID_ARG before any launch: what lrc_deform_set_dev refuses, for either shape (the message names it).
 *   lrc_deform_span_launches  kernel launches one lrc_deform_span_dev enqueues: with both shapes blended, and with both copied
 * Host functions, no GPU, by the inline functions the kernels call:
 *   lrc_span_vertices      out3 = span_vertex(a3, b3, s) per coordinate ((num_vertices, 3) float32 each); s in [0, 1]
 *   lrc_deform_span_refit  nodes16: the topology (references; not written); out_nodes16 receives the nodes with every child box
 *                          refitted to the span, out_span_box6 (num_slots, 6) the span boxes, out_span_rec18 (num_slots, 18;
 *                          nullable) the slots' vertices, A's three then B's.  Refuses what lrc_deform_refit refuses. */
int lrc_deform_span_dev(lrc_deform* deform, uint32_t k0a, uint32_t k1a, float wa, uint32_t k0b, uint32_t k1b, float wb,
                        void* stream);
int lrc_deform_span_launches(const lrc_deform* deform, uint32_t* blended, uint32_t* copied);
int lrc_span_vertices(const float* a3, const float* b3, uint64_t num_vertices, float s, float* out3);
int lrc_deform_span_refit(const float* nodes16, uint64_t num_nodes, const uint32_t* slot_prim, uint64_t num_slots,
                          const uint32_t* tris3, uint64_t T, const float* verts_a3, const float* verts_b3, uint64_t V,
                          float* out_nodes16, float* out_span_box6, float* out_span_rec18 /* nullable */);

/* ---- seeded sensor noise under movers in sweeps (opt-in) ----------------------------------------------
 * The movers under moving-sensor sweeps and the seeded sensor noise, composed: a walking person seen from a moving robot, with
 * range noise, angle jitter and dropped returns, drawn in the kernels and reproducible bit for bit.  The noise cannot be added
 * afterwards: the jitter decides whether a ray meets the room or a mover; a dropped ray is never cast, not against a spanned
 * deformable either; the range filter and min_range act on the noisy range.  float32 with one rounding per operation and
 * nothing fused, beyond what the reused functions already fuse (the quantile's one fmaf).  For ray i of sweep k:
 * frame = first_frame + k in 64 bits, s = (float)fire[i], and the noise is the Philox block of (seed, frame, i), words w0..w3.
 *   1 ray       (o, d, live) is the ray of lrc_scan_noisy_sweeps_dev, bit for bit: dropout != 0 and w3 < thr drops the ray; the
 *               jitter is applied to the table row in front of the rotation, the sweep behind it.  A ray that is not live is cast
 *               against neither the room nor any mover: its record is the miss lrc_scan_noisy_sweeps_dev writes for a dropped
 *               ray and its mover byte is 0.
 *   2 movers    THAT ray is taken into every mover's frame at s (step 2 of the movers under moving-sensor sweeps; a still record
 *               takes the shortcut there) and culled, unchanged.  The scene of a spanned deformable is cast per ray at the shape
 *               of the same s: the jitter does not touch s.
 *   3 winner    decided on the CLEAN ranges: the smallest float32 t of t_s, t_0, ..., t_(M-1) wins; on an exact tie the static
 *               scene, then the smaller m.  The winner's normal is turned into the world by the mover's pose at s.
 *   4 range     range_std != 0 and something was hit: t' = t_winner + float32(range_std) * z(w0), a float32 multiply, then an
 *               add; t' <= 0 is no return.  The point, the range filter, min_range, incident_deg (both modes) and the record use
 *               t', the jittered swept d and the sensor's centre c(s) of the moving-sensor sweeps in float64; prim, sem and ins
 *               are the winner's; the mover byte is the winner's where the record is kept and 0 elsewhere.
 *   5 zeros     a zero parameter skips its step (wave-uniform branches on kernel arguments).  The all-zero model gives the bytes
 *               of lrc_scan_mover_sweeps_dev; a NULL set gives the bytes of lrc_scan_noisy_sweeps_dev and a zero mover column;
 *               a sensor and movers that all stand still give the bytes of lrc_scan_noisy_movers_dev.
 * The result does not depend on how the sweeps are split into calls when each call brings its own first_frame.
 * LRC_ERR_INVALID_ARG before any launch, the call and the offender named: what lrc_scan_noisy_sweeps_dev refuses (a NULL model, a
 * negative or non-finite standard deviation, dropout outside [0, 1), rays_per_pose >= 2^32, a range_noise option; in the compact
 * call no fire table and a bad sensor record) and what lrc_scan_mover_sweeps_* refuse (the static scene among the movers, a set
 * or table of another context, d_out->tile_count != NULL and, in the compact call, a bad mover sweep record).  min_range and
 * incident_mode of the STATIC scene apply.  Scratch: the set's, laid out as under the seeded sensor noise under movers, 123 bytes
 * per ray whatever M is.
 *   lrc_scan_noisy_mover_sweeps_dev      device pointers, as lrc_scan_mover_sweeps_dev takes them, and the model; enqueued on
 *                                        `stream`, nothing is waited for
 *   lrc_scan_noisy_mover_sweeps_compact  lrc_scan_mover_sweeps_compact with the model: all sweeps are traced in one call, so sweep
 *                                        p of the call is frame first_frame + p; frames and mover_rows as there */
int lrc_scan_noisy_mover_sweeps_dev(lrc_scene* scene, lrc_movers* set /* nullable */, const double* d_motion24, uint64_t num_poses,
                                    const double* d_dirs3, const double* d_fire, uint64_t rays_per_pose,
                                    const float* d_mover_motion24, double max_range, const lrc_noise* noise, const lrc_hits* d_out,
                                    uint8_t* d_mover /* nullable */, void* stream);
int lrc_scan_noisy_mover_sweeps_compact(lrc_scene* scene, lrc_movers* set /* nullable */, const double* motion24,
                                        uint64_t num_poses, const lrc_table* table, const float* mover_motion24, double max_range,
                                        const lrc_noise* noise, const lrc_frames* out, uint8_t* mover_rows /* nullable */,
                                        uint64_t capacity, uint64_t* out_total);

/* Page-locked host memory for the frame buffers above (hipHostMalloc / hipHostFree).  The caller owns it. */
int lrc_host_alloc(lrc_ctx* ctx, uint64_t bytes, void** out_ptr);
int lrc_host_free(lrc_ctx* ctx, void* ptr);

/* ---- dual-axis sensor: rays generated in the kernel from host-drawn scan angles (opt-in) ---------------
 * The reference's DualAxisLidar draws, per ray, a noisy azimuth phi and elevation theta from the global numpy stream
 * and drops ~2 % of the rays with one more uniform draw (lidar/indoor_lidar.py:262-294); that stream is what "seeded
 * identically" means, so the draws stay on the host.  What moves to the device is everything after them: sin/cos,
 * the rotation into the world frame (un-fused, as numpy evaluates it, :283-287) and the float32 narrowing.
 *   angles2 : (num_poses * rays_per_pose, 2) float64 (phi, theta), pose-major
 *   keep    : nullable (num_poses * rays_per_pose) bytes, 0 = ray dropped by the sensor: never cast, reported as a
 *             miss, so the compacted frames equal those of casting only the kept rays
 * Output index = p * rays_per_pose + i; range filter centre = pose[:3,3].  NOT bit-guaranteed against the host
 * generator: the device's double-precision sin/cos need not round like the host's libm (the tests count the rays
 * whose float32 direction differs).  The default path (host generator + lrc_cast_segments) stays bit-exact. */
int lrc_scan_angles_dev(lrc_scene* scene, const double* d_poses16, uint64_t num_poses, const double* d_angles2,
                        const uint8_t* d_keep, uint64_t rays_per_pose, double max_range, const lrc_hits* d_out,
                        void* stream);
int lrc_scan_angles_compact(lrc_scene* scene, const double* poses16, uint64_t num_poses, const double* angles2,
                            const uint8_t* keep, uint64_t rays_per_pose, double max_range, const lrc_frames* out,
                            uint64_t capacity, uint64_t* out_total);

/* ---- explicit rays of several poses straight to frames --------------------------------------------------------
 * The frame-producing form of lrc_cast_segments for sensors whose rays come from the host generator (the dual-axis
 * sensor's bit-exact default path): every pose contributes rays_per_pose rays at a fixed stride,
 *   rays6    : (num_poses * rays_per_pose, 6) float32, pose-major
 *   keep     : nullable (num_poses * rays_per_pose) bytes, 0 = ray dropped by the sensor (lidar/indoor_lidar.py:292-294):
 *              never cast, reported as a miss -- the frames equal those of casting only the kept rays
 *   centers3 : (num_poses, 3) float64 range-filter centres (pose[:3,3])
 * and the result is compacted in HBM exactly like lrc_scan_poses_compact's (same lrc_frames, same ordering, per-pose
 * statistics included).  `index` is then the ray's index among ALL rays_per_pose rays of its pose. */
int lrc_scan_rays_compact(lrc_scene* scene, const float* rays6, const uint8_t* keep, const double* centers3,
                          uint64_t num_poses, uint64_t rays_per_pose, double max_range, const lrc_frames* out,
                          uint64_t capacity, uint64_t* out_total);

/* ---- numpy's legacy seeded stream (row a7: the BLK2GO generator draws its noise from np.random) --------------------
 * The reference draws, per pose, two normals per ray and then one uniform per ray from the GLOBAL numpy stream
 * (lidar/indoor_lidar.py:257-296).  lrc_rng_scan_draws produces exactly the doubles RandomState.normal(loc, scale,
 * normals_per_pose) followed by RandomState.random_sample(uniforms_per_pose) would return, pose after pose, for
 * num_poses poses, and leaves *state where numpy's generator would stand (np.random.get_state() / set_state()
 * tuples map to this struct field by field): MT19937 words, random_sample doubles, polar-method normals with the
 * cached second value.  Host code, multi-threaded (threads <= 0: the cores of the host, at most 16); no GPU involved. */
typedef struct lrc_mt19937_state {
    uint32_t key[624];
    int32_t  pos;          /* 0..624, next word of key[] (624: the block is used up)              */
    int32_t  has_gauss;
    double   gauss;        /* the cached normal when has_gauss                                   */
} lrc_mt19937_state;
int lrc_rng_scan_draws(lrc_mt19937_state* state, uint64_t num_poses, uint64_t normals_per_pose,
                       uint64_t uniforms_per_pose, double loc, double scale, double* out_normals,
                       double* out_uniforms, int threads);

/* The rays of one dual-axis pose from the sines and cosines of its scan angles (numpy's own, which only numpy reproduces):
 * d = (cos(theta) cos(phi), cos(theta) sin(phi), sin(theta)) rotated as the reference rotates it, ray by ray and un-fused,
 * (d0 R[j][0] + d1 R[j][1]) + d2 R[j][2], narrowed to float32 beside the pose's origin (lidar/indoor_lidar.py:274-291).
 * pose16: row-major 4x4 float64; out_rays6: (n, 6) float32.  Host code: the dozen numpy passes this replaces were what
 * bounded the BLK2GO trajectory once the draws were native. */
int lrc_rays_from_trig(const double* cos_theta, const double* sin_theta, const double* cos_phi, const double* sin_phi,
                       uint64_t n, const double* pose16, float* out_rays6);

/* ---- diagnostics ---------------------------------------------------------------------------------------
 * Per-ray traversal counters of a pose-batched scan from an instrumented build of the trace kernel, host arrays.
 * stats: (num_poses * rays_per_pose, LRC_STATS_WORDS) uint32: [0] inner-node steps, [1] triangle tests, [2] node steps
 * taken wave-uniformly (scalar fetch), [3] node steps with no child hit, [4] triangles that pass every
 * Moeller-Trumbore condition and are rejected only by the hit definition's box clause -- the one
 * clause Embree does not have; the tests assert a total of 0 on the BASELINE configurations. */
#define LRC_STATS_WORDS 5
int lrc_debug_scan_stats(lrc_scene* scene, const double* poses16, uint64_t num_poses, const double* dirs3,
                         uint64_t rays_per_pose, double max_range, uint32_t* stats);

/* ---- opt-in sensor-realism options --------------------------------
 * The reference DECLARES these sensor parameters but never applies them (SURVEY.md F6, F7:
 * Indoor8LineLidarIntrinsics.add_noise has no caller, lidar/lidar_intrinsics.py:364-389; min_range is never
 * read by the engines; the "incident angle" ignores the surface, raycast_engine_cpu.py:100-107).  Everything
 * is OFF by default, which is the reference's behaviour and what the parity tests pin.  Options are sticky
 * on the scene handle until changed; pass NULL to reset.
 *   min_range      > 0: a hit is kept only if its float64 distance from the centre is >= min_range
 *   range_noise    additive noise in metres, one float per ray of the NEXT calls (drawn by the caller, e.g.
 *                  from a seeded numpy stream, so that seeded runs are reproducible bit for bit):
 *                  t' = t + noise (float32); t' <= 0 drops the return; point, range filter and incident
 *                  angle use t'.  Host entry points take a host array, _dev entry points a device array;
 *                  range_noise_len must equal the number of rays of the call.
 *                  (Noise drawn in the kernel from a seed, with angle jitter and dropout: lrc_scan_noisy_dev.)
 *   incident_mode  0: reference (angle between centre->point and the vertical axis)
 *                  1: angle between the ray and the hit triangle's normal, acos(|d^.n|) in degrees */
typedef struct lrc_scan_options {
    double       min_range;
    const float* range_noise;
    uint64_t     range_noise_len;
    int          incident_mode;
} lrc_scan_options;
int lrc_scene_set_options(lrc_scene* scene, const lrc_scan_options* opts);

/* ---- scene cloud from per-ray (t, label) pairs of a pose-batched scan ------------------------------
 * A pose-batched scan is a pure function of (poses16, dirs3): whoever holds those can rebuild the hit point of
 * ray (p,i) from its t alone, with the same float32 arithmetic as the scan itself (bit-identical rows).  The
 * multi-GPU assembly therefore all-gathers 8-byte (t, label) pairs (lrc_hits.t_label) instead of 16-byte rows
 * and every rank runs this function over the gathered pairs of all poses:
 *   d_t_label : (P*N) x {float t; uint32 label}, +inf = no return
 *   d_out_xyzl: (K,4) rows x, y, z, label bits, stable pose-major order (np.vstack of the frames,
 *               containers/s3dis_sim_scene.py:326); d_counts (P), nullable: kept rays per pose. */
int lrc_cloud_from_ranges_dev(lrc_ctx* ctx, const double* d_poses16, uint64_t num_poses,
                              const double* d_dirs3, uint64_t rays_per_pose, const void* d_t_label,
                              float* d_out_xyzl, uint64_t* d_counts, void* stream);

/* The same rebuild from 4 bytes per ray: the hit triangle's row (lrc_hits.prim, Open3D's primitive_ids of
 * raycast_engine_cpu.py:51; LRC_INVALID_PRIM = no return).  A closest hit is a pure function of (pose, direction,
 * triangle), so a rank that holds the scene replica recomputes t with the scan's own ray/triangle test, bit for
 * bit, and the point and the triangle's labels from it.  This is what the multi-GPU all-gather moves (DESIGN.md
 * section 6): xGMI links, not the kernels, bound the multi-GPU job.  Not available while a range_noise option is
 * set (the noise is not a function of the triangle): use lrc_cloud_from_ranges_dev then.
 *   d_prim       : entry (pose p, ray i) at word (p / poses_per_slab) * slab_stride_bytes/4
 *                  + (p % poses_per_slab) * rays_per_pose + i -- the gathered send slabs of several ranks in place;
 *                  poses_per_slab = 0 means one contiguous (num_poses * rays_per_pose) array
 *   d_tile_count : nullable; the senders' lrc_hits.tile_count (kept rays per aligned run of 64), laid out in the
 *                  same slabs: tile k of slab r at d_tile_count[r * slab_stride_bytes/4 + k].  Saves the counting
 *                  pass; needs rays_per_pose % 64 == 0
 *   ranks that own fewer poses than poses_per_slab pad their slab with LRC_INVALID_PRIM entries (zero counts); the
 *   pose table then has num_poses = slabs * poses_per_slab rows, padded ones arbitrary.
 * Scratch (tile offsets, transposed direction table) belongs to the scene's context: lrc_cloud_from_prims_dev and
 * lrc_cloud_from_ranges_dev share one set, lrc_compact_dev has its own, so a rebuild may run on one stream beside a
 * compaction on another, but two rebuilds (or two compactions) of one context must not overlap in time. */
int lrc_cloud_from_prims_dev(lrc_scene* scene, const double* d_poses16, uint64_t num_poses,
                             const double* d_dirs3, uint64_t rays_per_pose, const uint32_t* d_prim,
                             const uint32_t* d_tile_count, uint64_t poses_per_slab, uint64_t slab_stride_bytes,
                             float* d_out_xyzl, uint64_t* d_counts, void* stream);

/* The same when the caller's own slab of poses does not need rebuilding: its rows come from the local records the trace
 * kernel wrote (own->t, own->point3, own->sem, own->ins: fixed-stride arrays of poses_per_slab x rays_per_pose entries),
 * scattered to their place in the assembled cloud; only the other slabs are rebuilt from ids.  Same output bytes.
 * Needs the senders' per-wave keep counts (d_tile_count, rays_per_pose % 64 == 0). */
int lrc_cloud_from_prims_own_dev(lrc_scene* scene, const double* d_poses16, uint64_t num_poses, const double* d_dirs3,
                                 uint64_t rays_per_pose, const uint32_t* d_prim, const uint32_t* d_tile_count,
                                 uint64_t poses_per_slab, uint64_t slab_stride_bytes, uint64_t own_slab,
                                 const lrc_compact_io* own, float* d_out_xyzl, uint64_t* d_counts, void* stream);

/* Per-pose mean / std of |p| (float32, from the WORLD origin, numpy's arithmetic: lrc_stats.h) over the assembled
 * (x, y, z, label) rows of a scan: the ScanQuality range statistics (s3dis_simulator.py:283-286) of a cloud that was
 * assembled on the device.  d_range: scratch of max_rows floats (receives |p| per row). */
int lrc_cloud_range_stats_dev(lrc_ctx* ctx, const float* d_xyzl, const uint64_t* d_counts, uint64_t num_poses,
                              uint64_t max_rows, float* d_range, float* d_mean, float* d_std, void* stream);

/* ---- nearest annotated point --------------------------------------
 * Exact 1-nearest-neighbour lookup of float32 query points in a float64 annotated cloud, float64 distances,
 * ties to the smaller row.  Replaces sklearn NearestNeighbors(n_neighbors=1, algorithm='ball_tree')
 * .fit(annotated).kneighbors(points) at containers/s3dis_sim_scene.py:416-418, which the reference runs on
 * every frame's hit points at export time to attach colour / semantic / instance labels; also used once per
 * mesh to bake per-triangle labels (triangle centroid -> nearest annotated point) that the trace kernel then
 * writes back per ray.  cell_size <= 0 picks a grid spacing from the point density. */
typedef struct lrc_nn lrc_nn;
int lrc_nn_create(lrc_ctx* ctx, const double* points3, uint64_t num_points, double cell_size, lrc_nn** out_nn);
int lrc_nn_destroy(lrc_nn* nn);
int lrc_nn_query(lrc_nn* nn, const float* query3, uint64_t num_queries, uint32_t* out_index,
                 double* out_dist /* nullable */);
int lrc_nn_query_dev(lrc_nn* nn, const float* d_query3, uint64_t num_queries, uint32_t* d_out_index,
                     double* d_out_dist /* nullable */, void* stream);

/* ---- validation metrics ---------------------------------------------
 * The O(n*m) parts of the reference's sampled cloud metrics (evaluate_single_scene.py:55-111), host arrays:
 *   lrc_min_distances : out_min[i] = min_j |a_i - b_j| in float32 (sum of squares, one sqrt): the directed
 *                       term of compute_chamfer_distance (:81-96) and compute_hausdorff_distance (:98-111)
 *   lrc_rbf_kernel_sum: sum_ij exp(-gamma * max(|a_i|^2 + |b_j|^2 - 2 a_i.b_j, 0)), float64: one of the
 *                       three kernel sums of compute_mmd_sampled (:55-79)
 * Non-finite coordinates answer as numpy's min, maximum and exp do: a distance or a kernel term that is NaN there
 * (a NaN coordinate, inf - inf, 0 * inf) makes the row's minimum, or the sum, NaN. */
int lrc_min_distances(lrc_ctx* ctx, const float* a3, uint64_t n, const float* b3, uint64_t m, float* out_min);
int lrc_rbf_kernel_sum(lrc_ctx* ctx, const float* a3, uint64_t n, const float* b3, uint64_t m, double gamma,
                       double* out_sum);

/* ---- detection boxes ---------------------------------------------------------------------------------
 * Axis-aligned boxes of the object instances of a labelled cloud after a k-nearest-neighbour statistical outlier
 * filter: lidar_net_bbox_visualizer.py:163-249 of the reference (instances by class and instance id, Open3D's
 * remove_statistical_outlier(nb_neighbors=k, std_ratio), min / max of what is left), all instances in one call.
 *   instance : (index of sem in class_ids, ins) with ins != 0; rows of other classes or with ins == 0 are ignored;
 *              an instance of fewer than min_points rows is dropped, one of fewer than k rows keeps every row.
 *   avg      : per row of an instance of n >= k rows, (sum of the square roots of the k smallest float64 squared
 *              distances (dx*dx + dy*dy) + dz*dz to rows of the same instance, itself included, ascending, one after
 *              the other) / k.
 *   filter   : mean = sum_{avg>0} avg / n, std = sqrt(sum_{avg>0} (avg - mean)^2 / (n - 1)), threshold = mean +
 *              std_ratio * std; a row is kept iff avg > 0 && avg < threshold (k or more coincident rows go).  An
 *              instance of one row with k == 1 (and min_points <= 1) is filtered: mean = 0, 0 / 0 under the root makes
 *              the threshold a NaN (sign and payload unspecified), and the row is removed.
 *   box      : min3 / max3 are the float32 minimum / maximum of the kept rows as numpy's points.min(axis=0) /
 *              .max(axis=0) return them: an extreme that equals zero has the sign of the last kept row (ascending row
 *              order) whose coordinate on that axis is +0 or -0; every other extreme is the plain minimum / maximum.
 * One lrc_box per instance of min_points rows or more, ordered by (position of the class in class_ids, ins); the
 * call writes min(total, capacity) of them and the total to *out_num_boxes.  The optional per-row outputs (num_rows
 * entries, input order): avg (-1 where the filter did not run) and keep (1 = the row is in its instance's box).
 * 1 <= k <= 32, at most 64 distinct class ids, num_rows < 2^31; cell_size <= 0 picks a grid spacing per instance
 * (results do not depend on it).  Rows are (K,4) x, y, z, label bits (sem | ins<<16) on the device, as the scan
 * pipeline leaves them, or host float32 xyz plus uint16 sem and ins.  Boxes and the count are HOST memory in both
 * entry points: lrc_instance_boxes_dev returns after the work it enqueued on `stream` has finished. */
typedef struct lrc_box {
    uint16_t sem;
    uint16_t ins;
    uint32_t num_points;     /* rows of the instance                                               */
    uint32_t num_kept;       /* rows inside the box (0: the filter removed all; min3 = +inf, max3 = -inf) */
    uint32_t filtered;       /* 1: num_points >= k and the filter ran; 0: every row kept             */
    float    min3[3];        /* float32 minimum of the kept rows (a zero: the last kept zero row's) */
    float    max3[3];
    double   mean;           /* filter statistics; 0 and +inf when filtered == 0                    */
    double   threshold;
} lrc_box;                   /* 56 bytes */

int lrc_instance_boxes(lrc_ctx* ctx, const float* points3, const uint16_t* sem, const uint16_t* ins, uint64_t num_rows,
                       const uint16_t* class_ids, uint32_t num_classes, uint32_t min_points, uint32_t k, double std_ratio,
                       double cell_size, lrc_box* out_boxes, uint64_t capacity, uint64_t* out_num_boxes,
                       double* out_avg /* nullable */, uint8_t* out_keep /* nullable */);
int lrc_instance_boxes_dev(lrc_ctx* ctx, const float* d_xyzl, uint64_t num_rows, const uint16_t* class_ids,
                           uint32_t num_classes, uint32_t min_points, uint32_t k, double std_ratio, double cell_size,
                           lrc_box* out_boxes, uint64_t capacity, uint64_t* out_num_boxes,
                           double* d_out_avg /* nullable */, uint8_t* d_out_keep /* nullable */, void* stream);

/* ---- cloud preprocessing ----------------------------------------------------------------------------
 * The reference's preprocessing stage (s3dis_data_loader.py:85-158): Open3D's remove_statistical_outlier over a whole
 * float64 room cloud, then estimate_normals with a hybrid (radius, max_nn) search on the kept rows, in one call.
 *   avg      : per input row, (sum of the square roots of the min(nb_neighbors, n) smallest float64 squared distances
 *              (dx*dx + dy*dy) + dz*dz to the rows of the cloud, itself included, ascending, one after the other) /
 *              min(nb_neighbors, n).
 *   filter   : mean = sum_{avg>0} avg / n, std = sqrt(sum_{avg>0} (avg - mean)^2 / (n - 1)), threshold = mean +
 *              std_ratio * std, both reduced in an order fixed by n; a row is kept iff avg > 0 && avg < threshold
 *              (nb_neighbors or more coincident rows all go; n == 1 keeps nothing).  Kept rows are listed in
 *              ascending row order (Open3D's `ind`).  remove_outliers == 0 keeps every row (avg = -1, mean = 0,
 *              threshold = +inf).
 *   normals  : per kept row, in kept order.  Neighbours are the kept rows with d2 < radius^2 (strict), itself
 *              included, ordered by (d2, kept index), the first max_nn of them; nn_count is their number.  Fewer than
 *              3 give (0, 0, 1).  Otherwise Open3D's nine cumulants are summed in neighbour order and divided by the
 *              count, cov = E[x x^T] - E[x] E[x]^T, and the normal is the unit eigenvector of the smallest eigenvalue
 *              from the closed-form robust symmetric 3x3 solver (Eberly; Open3D's fast_normal_computation path); a
 *              zero covariance gives (0, 0, 1).  An exactly diagonal covariance gives the axis of its smallest entry,
 *              and among equal smallest entries z before x before y (diag(s, s, L) with s < L gives (1, 0, 0)).  The
 *              sign is the solver's: no orientation is applied.
 * 1 <= nb_neighbors <= 32 and 1 <= max_nn <= 32 (the lists live in registers; the reference uses 20 and 30), finite
 * std_ratio > 0 and radius > 0, n < 2^31; a non-finite coordinate fails with LRC_ERR_INVALID_ARG.  cell_size <= 0
 * picks the grid spacing (about max(nb_neighbors, max_nn) rows per cell); no result depends on it.
 * out_kept needs n entries; out_normals3 (3 per kept row) is required when estimate_normals != 0; out_avg (n
 * entries), out_nn_count (one per kept row) and out_stats2 (mean, threshold; HOST memory in both entry points) are
 * optional.  *out_num_kept is HOST memory; lrc_cloud_preprocess_dev returns after the work it enqueued on `stream`
 * has finished. */
typedef struct lrc_preprocess_opts {
    uint32_t remove_outliers;    /* 1: statistical outlier filter                                      */
    uint32_t nb_neighbors;       /* k of the filter                                                    */
    double   std_ratio;
    uint32_t estimate_normals;   /* 1: PCA normals of the kept rows                                    */
    uint32_t max_nn;             /* neighbour cap of the hybrid search                                 */
    double   radius;             /* search radius of the hybrid search                                 */
    double   cell_size;          /* <= 0: automatic                                                    */
} lrc_preprocess_opts;           /* 40 bytes */

int lrc_cloud_preprocess(lrc_ctx* ctx, const double* points3, uint64_t n, const lrc_preprocess_opts* opts,
                         uint32_t* out_kept, uint64_t* out_num_kept, double* out_normals3 /* nullable */,
                         double* out_avg /* nullable */, uint8_t* out_nn_count /* nullable */,
                         double* out_stats2 /* nullable */);
int lrc_cloud_preprocess_dev(lrc_ctx* ctx, const double* d_points3, uint64_t n, const lrc_preprocess_opts* opts,
                             uint32_t* d_out_kept, uint64_t* out_num_kept, double* d_out_normals3 /* nullable */,
                             double* d_out_avg /* nullable */, uint8_t* d_out_nn_count /* nullable */,
                             double* out_stats2 /* nullable */, void* stream);

/* ---- object boxes -----------------------------------------------------------------------------------
 * The reference's ground-truth boxes of S3DIS rooms (s3dis_bbox_visualizer.py:70-116): per Annotations/<class>_<k>.txt
 * object, Open3D's remove_statistical_outlier(nb_neighbors=k, std_ratio) on float64 points and the min / max of the
 * kept rows; every object of a room or of an area in one call, with a number of launches and host synchronisations
 * that does not depend on the number of objects.  Objects are runs of the concatenated rows: object s is rows
 * [offsets[s], offsets[s+1]) (num_objects + 1 HOST entries, offsets[0] == 0, offsets[num_objects] == n, never
 * decreasing; empty objects are allowed).
 *   m < k    : no filter (the reference returns such points as they are): every row is kept, avg = -1, mean = 0,
 *              threshold = +inf, filtered = 0.
 *   m >= k   : exactly the outlier stage of lrc_cloud_preprocess(nb_neighbors = k, std_ratio) run on the object's rows
 *              alone, bit for bit: neighbours come only from the same object, avg = (sum of the square roots of the k
 *              smallest float64 squared distances (dx*dx + dy*dy) + dz*dz, itself included, ascending) / k, mean and
 *              std reduced in the order lrc_cloud_preprocess fixes for m rows, keep = avg > 0 && avg < threshold.  An
 *              object of one row with k == 1 is filtered: mean = 0, 0 / 0 under the root makes the threshold a NaN
 *              (sign and payload unspecified), and the row is removed.
 *   box      : min3 / max3 are the float64 minimum / maximum of the kept rows as numpy's points.min(axis=0) /
 *              .max(axis=0) return them: an extreme that equals zero has the sign of the last kept row whose coordinate
 *              on that axis is +0 or -0; every other extreme is the plain minimum / maximum.
 * One lrc_objbox per object, in object order (HOST memory in both entry points).  The optional per-row outputs: out_kept
 * (n entries; the kept rows' indices, ascending, so object s's kept rows start at the sum of num_kept over the objects
 * before it), avg and keep (n entries, input order).  1 <= k <= 32, finite std_ratio > 0, n < 2^31 and num_objects <
 * 2^31, checked on the host before any launch; a non-finite coordinate fails with LRC_ERR_INVALID_ARG.  cell_size <= 0
 * picks a grid spacing per object (about k rows per cell); no result depends on it.  lrc_object_boxes_dev takes device
 * points and device per-row outputs and returns after the work it enqueued on `stream` has finished. */
typedef struct lrc_objbox {
    uint64_t num_points;     /* rows of the object                                                  */
    uint64_t num_kept;       /* rows inside the box (0: the filter removed all; min3 = +inf, max3 = -inf) */
    uint32_t filtered;       /* 1: num_points >= k and the filter ran; 0: every row kept             */
    uint32_t reserved_;
    double   min3[3];        /* float64 minimum of the kept rows (a zero: the last kept zero row's) */
    double   max3[3];
    double   mean;           /* filter statistics; 0 and +inf when filtered == 0                    */
    double   threshold;
} lrc_objbox;                /* 88 bytes */

int lrc_object_boxes(lrc_ctx* ctx, const double* points3, uint64_t n, const uint64_t* offsets, uint64_t num_objects,
                     uint32_t k, double std_ratio, double cell_size, lrc_objbox* out_boxes,
                     uint32_t* out_kept /* nullable */, double* out_avg /* nullable */, uint8_t* out_keep /* nullable */);
int lrc_object_boxes_dev(lrc_ctx* ctx, const double* d_points3, uint64_t n, const uint64_t* offsets, uint64_t num_objects,
                         uint32_t k, double std_ratio, double cell_size, lrc_objbox* out_boxes,
                         uint32_t* d_out_kept /* nullable */, double* d_out_avg /* nullable */,
                         uint8_t* d_out_keep /* nullable */, void* stream);

/* ---- robot-cube occupancy for the trajectory planner ----------------
 * out_flags[q] = 1 iff some mesh vertex lies inside the axis-aligned cube [p_q - half, p_q + half] (float64,
 * inclusive; a NaN coordinate is inside nothing), for all Q positions at once, any number of them.  Replaces
 * AutoTrajectoryGenerator._is_point_inside_mesh
 * (trajectory/auto_trajectory_generator.py:219-238), which the reference evaluates position by position over
 * every vertex for the free-space grid (:129-139) and for every waypoint of every candidate (:345-356). */
typedef struct lrc_occ lrc_occ;
int lrc_occ_create(lrc_ctx* ctx, const double* verts3, uint64_t num_vertices, lrc_occ** out_occ);
int lrc_occ_destroy(lrc_occ* occ);
int lrc_occ_query(lrc_occ* occ, const double* points3, uint64_t num_points, double half, uint8_t* out_flags);

/* ---- surface coverage of scans ------------------------------------------------------------
 * Which triangles of a mesh did a set of scans return points from, how much area is that, per semantic class, and which
 * few pose sets cover the most.  Definitions:
 *   returned ray   : a ray returns a point iff its t is finite after the range filter (exactly the rows compaction keeps).
 *                    A ray with a valid prim but t = +inf (removed by the range filter) returns nothing, nor does
 *                    prim == LRC_INVALID_PRIM.  A prim >= num_triangles is ignored as well.
 *   seen triangle  : triangle j is seen by a set of poses iff at least one returned ray of those poses has prim == j.
 *   hits[j]        : the number of returned rays with prim == j, over all sets (uint32, wraps past 2^32 - 1).
 *   area           : float64, 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = (v1 - v0) x (v2 - v0) component by component as
 *                    a*b - c*d; no fused multiply-add anywhere, correctly rounded sqrt (computed on the device).
 *   quantised area : q[j] = uint64(rint(area * 2^32)); every area sum is an exact uint64 sum of q (order-free, bit-
 *                    reproducible).  A mesh whose total q would exceed 2^63 is refused with LRC_ERR_INVALID_ARG.
 *   covered area   = covered_q * 2^-32 m^2, ratio = covered_q / total_q, redundancy = returned rays / covered area.
 * Sampling caveat: a tiny triangle can lie between two scan lines of every pose, so "seen" means "received at least one
 * return"; the sampled result converges on the visible area as the number of poses grows.  No dilation is applied.
 *
 * A coverage object holds num_sets bitsets of ceil(T/32) uint32 words each (bit j of word j/32, LSB first), hits and the
 * returned-ray count of every set; they start at zero and repeated accumulations add up.  Per-class sums are kept per
 * distinct tri_sem value (at most 4096), indexed densely in ascending label order (lrc_coverage_classes); without
 * tri_sem there are no classes.  Vertices (V,3) float64 must be finite, triangles (T,3) int32 in [0, V), 0 < T < 2^32-1.
 * The object is not thread-safe; "_dev" entry points enqueue on `stream`, the others return after the work finished. */
typedef struct lrc_coverage lrc_coverage;

typedef struct lrc_coverage_info {
    uint64_t num_triangles;
    uint64_t num_sets;
    uint64_t words_per_set;    /* ceil(num_triangles / 32)                                         */
    uint64_t total_q;          /* sum of q over the mesh                                           */
    uint32_t num_classes;      /* distinct tri_sem values (0 without tri_sem)                     */
    uint32_t reserved_;
} lrc_coverage_info;           /* 40 bytes */

typedef struct lrc_coverage_stats {
    uint64_t covered_q;        /* sum of q over the seen triangles                                 */
    uint64_t total_q;
    uint64_t seen_triangles;
    uint64_t returns;          /* returned rays accumulated into the set(s)                        */
} lrc_coverage_stats;          /* 32 bytes; the _dev summary writes these four words in this order */

int lrc_coverage_create(lrc_ctx* ctx, const double* verts3, uint64_t num_vertices, const int32_t* tris3,
                        uint64_t num_triangles, const uint16_t* tri_sem /* nullable */, uint64_t num_sets,
                        lrc_coverage** out_cov);
int lrc_coverage_destroy(lrc_coverage* cov);
int lrc_coverage_get_info(const lrc_coverage* cov, lrc_coverage_info* out);
/* num_classes label values (ascending) and their total q; either pointer may be NULL. */
int lrc_coverage_classes(const lrc_coverage* cov, uint16_t* out_class_ids, uint64_t* out_total_q);
/* Zero every bitset, hits and the returned-ray counts. */
int lrc_coverage_reset(lrc_coverage* cov, void* stream);
/* d_t (float32) and d_prim (uint32) of num_poses x rays_per_pose rays, pose-major as lrc_scan_poses_dev writes them.
 * Pose p goes to set d_set_of_pose[p] (device, num_poses entries; an entry >= num_sets drops that pose's rays) or, with
 * NULL, to set p (then num_poses <= num_sets is required).  Integer atomics only: the result does not depend on order. */
int lrc_coverage_accumulate_dev(lrc_coverage* cov, const float* d_t, const uint32_t* d_prim, uint64_t num_poses,
                                uint64_t rays_per_pose, const uint32_t* d_set_of_pose /* nullable */, void* stream);
/* Summary of set `set_index`, or of the union of all sets for set_index < 0: the stats, the per-class covered q
 * (num_classes entries; may be NULL only without classes) and, optionally, the set's (or the union's) bitset
 * (words_per_set words).  The _dev form writes the four stats words, the classes and the bits to device memory. */
int lrc_coverage_summary(lrc_coverage* cov, int64_t set_index, lrc_coverage_stats* out, uint64_t* out_class_q,
                         uint32_t* out_bits /* nullable */);
int lrc_coverage_summary_dev(lrc_coverage* cov, int64_t set_index, uint64_t* d_out4, uint64_t* d_out_class_q,
                             uint32_t* d_out_bits /* nullable */, void* stream);
/* Greedy view selection over the object's sets.  covered starts as initial_bits (words_per_set words; NULL = empty);
 * each round picks the set k with the largest gain_k = sum of q over the bits of (bits_k & ~covered), ties to the
 * smallest k, and ORs it into covered.  Selection stops after `budget` picks, at a gain of 0, or as soon as
 * float64(covered_q) / float64(total_q) >= target_ratio: both uint64 sums are converted to float64 (round to nearest
 * even), then divided once in float64, the arithmetic of `ratio` above (target_ratio <= 0: no target; an initial
 * cover that already reaches it picks nothing).  Writes the picks (uint32) and their gains (uint64 q units) in pick order and their number.  The rounds
 * run on the device, the pick of round r read by the launches of round r + 1; the host form synchronises once. */
int lrc_coverage_select(lrc_coverage* cov, uint32_t budget, double target_ratio, const uint32_t* initial_bits,
                        uint32_t* out_picks, uint64_t* out_gains, uint32_t* out_num_picks);
int lrc_coverage_select_dev(lrc_coverage* cov, uint32_t budget, double target_ratio, const uint32_t* d_initial_bits,
                            uint32_t* d_out_picks, uint64_t* d_out_gains, uint32_t* d_out_num_picks, void* stream);
/* Copy out every set's bitset (num_sets * words_per_set words), hits (num_triangles), the returned rays per set
 * (num_sets) and the quantised area table q (num_triangles); NULL skips one. */
int lrc_coverage_export(lrc_coverage* cov, uint32_t* out_bits, uint32_t* out_hits, uint64_t* out_returns,
                        uint64_t* out_q);

/* ---- semantic occupancy grids from scans --------------------------------------------------
 * Three states per voxel, as semantic scene completion ground truth needs them: OCCUPIED (a return ended in it), FREE
 * (a ray passed through it), UNKNOWN (no ray reached it).  Only the scan knows "free": it needs the poses and the
 * per-ray ranges, which a stacked cloud no longer holds.  Not to be confused with lrc_occ_* (the planner's robot-cube
 * test).  Definitions:
 *   grid       origin g (3 float64, finite), voxel size s (float64, finite, > 0), dims (nx, ny, nz), each >= 1,
 *              nx*ny*nz <= 2^31 - 1.  The voxel of a float64 point x is i_a = floor((x_a - g_a) / s) per axis (an f64
 *              subtract, then an f64 divide, then floor); it is inside iff 0 <= i < n on every axis.  Its linear
 *              index is (i*ny + j)*nz + k: arrays have shape (nx, ny, nz) in C order, z fastest.
 *   rays       pose-batched static scans only.  Ray (p, i), entry p*N + i, has origin o, float32 exactly as the scan
 *              forms it, and end point e, the float32 hit point o + (d/|d|)*t: the row the scene cloud holds.  A ray
 *              contributes only if its t is finite (it RETURNS: exactly the rows compaction keeps).  Rays without a
 *              return carve nothing.
 *   walk       float64, no contraction, o and e widened exactly: a = voxel of o, b = voxel of e, D = e - o.  For each
 *              axis with b_a != a_a: n_a = |b_a - a_a| steps, step_a = sign(b_a - a_a),
 *              tMax_a = ((g_a + (a_a + 1)*s) - o_a) / D_a stepping up, ((g_a + a_a*s) - o_a) / D_a stepping down,
 *              tDelta_a = s / |D_a|; axes with n_a = 0 take no part.  Visit a; then, while any n_a > 0, take the axis
 *              with the smallest tMax among those with n_a > 0 (ties x, then y, then z), step it, tMax_a += tDelta_a,
 *              n_a -= 1, and visit the new voxel.  The walk ends in b: 6-connected, Manhattan + 1 voxels.  Every
 *              visited voxel except b that lies in the grid gets its FREE bit; b, if in the grid, gets one RETURN with
 *              the ray's (sem, ins) (label bits sem | ins << 16).  a == b carves nothing.  Voxels outside the grid are
 *              ignored, but the walk is defined over the whole segment.
 *   limits     a returned ray whose o or e is not finite, whose voxel coordinates leave [-2^31, 2^31) or whose walk
 *              has more than 2^24 - 1 steps is REJECTED: it carves nothing, records no return, and is counted.
 *   accumulate additive over calls until reset; the result depends neither on pose order, nor on chunking, nor on the
 *              order of atomics: free bits are an OR, returns are integer counts.
 *   finalize   (min_returns >= 1) returns[v] = number of returns in v (uint32).  v is OCCUPIED iff returns[v] >=
 *              min_returns, else FREE iff its free bit is set, else UNKNOWN (a few returns below min_returns and no
 *              free bit stay unknown).  sem[v] = most frequent semantic label among v's returns, ties to the smallest;
 *              ins[v] = most frequent instance among the returns whose sem equals sem[v], ties to the smallest; both 0
 *              without returns.  Outputs: the sparse list, ascending by linear index, of every voxel with >= 1 return
 *              (idx u32, sem u16, ins u16, returns u32); an optional dense state u8 array (0 unknown, 1 free,
 *              2 occupied); the counts.
 * Every returned ray reserves one 8-byte key slot until the next reset (the key buffer grows, no return is dropped;
 * at most 2^31 - 1 rays between resets).  The object is not thread-safe and its calls must be ordered on one stream;
 * "_dev" entry points enqueue on `stream`, the others return after the work finished. */
typedef struct lrc_voxgrid lrc_voxgrid;

typedef struct lrc_voxgrid_info {
    double   origin[3];
    double   voxel_size;
    int64_t  dims[3];
    uint64_t num_voxels;       /* nx*ny*nz                                                         */
    uint64_t words;            /* free bitset words, ceil(num_voxels / 32)                         */
    uint64_t reserved_keys;    /* rays accumulated since the last reset (key slots)                */
    uint64_t sparse_bound;     /* min(num_voxels, reserved_keys): capacity the sparse outputs need */
} lrc_voxgrid_info;            /* 88 bytes */

typedef struct lrc_voxgrid_counts {
    uint64_t num_sparse;       /* voxels with >= 1 return                                          */
    uint64_t num_free;
    uint64_t num_occupied;
    uint64_t num_unknown;
    uint64_t rejected_rays;    /* returned rays refused by the limits above                        */
    uint64_t returns;          /* returns recorded in the grid (the sum of returns[v])             */
} lrc_voxgrid_counts;          /* 48 bytes; the _dev finalize writes these six words in this order */

/* Rejects a non-finite origin, a voxel size that is not finite and > 0, a dim < 1 and more than 2^31 - 1 voxels with
 * LRC_ERR_INVALID_ARG. */
int lrc_voxgrid_create(lrc_ctx* ctx, const double* origin3, double voxel_size, const int64_t* dims3,
                       lrc_voxgrid** out_vg);
int lrc_voxgrid_destroy(lrc_voxgrid* vg);
int lrc_voxgrid_get_info(const lrc_voxgrid* vg, lrc_voxgrid_info* out);
/* Clear the free bits, the returns and the counters. */
int lrc_voxgrid_reset(lrc_voxgrid* vg, void* stream);
/* Walk the rays of a pose-batched scan: d_poses16 (num_poses x 16 float64, row-major 4x4) and d_dirs3
 * (rays_per_pose x 3 float64) as lrc_scan_poses_dev took them, d_t_label its (num_poses * rays_per_pose) x 8 B
 * lrc_hits.t_label pairs {float t; uint32 sem | ins << 16}. */
int lrc_voxgrid_accumulate_dev(lrc_voxgrid* vg, const double* d_poses16, uint64_t num_poses, const double* d_dirs3,
                               uint64_t rays_per_pose, const void* d_t_label, void* stream);
/* The sparse list (capacity >= sparse_bound entries each; unused tail entries are left as they were), the dense
 * state (num_voxels bytes; NULL skips it) and the counts.  The _dev form writes the six count words to d_counts6 and
 * needs no host synchronisation; the host form synchronises once and copies num_sparse entries. */
int lrc_voxgrid_finalize_dev(lrc_voxgrid* vg, uint32_t min_returns, uint32_t* d_idx, uint16_t* d_sem, uint16_t* d_ins,
                             uint32_t* d_returns, uint64_t capacity, uint8_t* d_state /* nullable */,
                             uint64_t* d_counts6, void* stream);
int lrc_voxgrid_finalize(lrc_voxgrid* vg, uint32_t min_returns, uint32_t* out_idx, uint16_t* out_sem, uint16_t* out_ins,
                         uint32_t* out_returns, uint64_t capacity, uint8_t* out_state /* nullable */,
                         lrc_voxgrid_counts* out_counts);
/* Copy out the free bitset (words uint32; bit v of word v/32, least significant bit first). */
int lrc_voxgrid_export_bits(lrc_voxgrid* vg, uint32_t* out_bits);

/* ---- dynamic occupancy: per-frame grids under movers ------------------------------------------
 * An occupancy SEQUENCE is F frame slots of one grid geometry.  lrc_voxgrid ORs the free space of all poses into one grid,
 * which is wrong as soon as something moves: a pedestrian smears into a corridor of occupied voxels that the free space
 * carved while they stood elsewhere contradicts.  A sequence keeps one grid per frame (4D occupancy, single-sweep scene
 * completion) and, with LRC_VOXSEQ_STATIC_ONLY and every pose mapped to one slot, the static map with the movers' returns
 * left out.  Definitions:
 *   grid       origin, voxel size, dims, the voxel of a point and the linear index exactly as lrc_voxgrid defines them
 *              above.  F >= 1 slots; each slot's free bits start on a word boundary (words_per_frame = ceil(V / 32) words
 *              per slot, V = nx*ny*nz).  Create refuses F * 32 * words_per_frame > 2^31 - 1 and everything
 *              lrc_voxgrid_create refuses.
 *   segments   ray (p, i), entry r = p*N + i of the records, contributes iff t[r] is finite.  Its segment runs from o to e:
 *              o = d_origins3[p] when origin_per_ray == 0 (a float32 triple; for every pose-batched scan the float32 of the
 *              pose's translation, as the scan forms its ray origin), o = d_origins3[r] when origin_per_ray == 1 (taken as
 *              given); e = point3[r].  Its labels are sem[r], ins[r]; its mover id d_mover[r] (NULL: all zero; 0 is the
 *              room, m + 1 mover m, the column the mover scans write).  Its slot is f = d_frame_of_pose[p] (uint32), or
 *              first_frame + p when that array is NULL.  With a NULL array first_frame + num_poses > F is refused before
 *              any launch; with an array a pose whose f >= F contributes nothing, its returned rays are counted in
 *              `skipped`, and no access is made with that f.
 *   walk       the walk, the limits and the rejection of lrc_voxgrid, verbatim: float64 without contraction, ties x, then
 *              y, then z, a == b carves nothing, rejected rays are counted (per slot).  Free bits and returns go to slot f
 *              only.
 *   flags      LRC_VOXSEQ_STATIC_ONLY: a returned ray with mover id != 0 carves its free voxels as usual but records no
 *              return; its end voxel gets neither a free bit nor a return from it.
 *   accumulate additive over calls until reset; the result depends neither on pose order, nor on chunking, nor on the order
 *              of atomics: free bits are an OR, returns and the counters are integer counts.
 *   finalize   (min_returns >= 1) per slot, returns, the state, sem and ins exactly as lrc_voxgrid_finalize defines them.
 *              Two more columns come from a SECOND, INDEPENDENT vote over the same returns: mover[v] (uint8) = the most
 *              frequent mover id among all of v's returns, ties to the smallest id; mover_returns[v] (uint32) = the number
 *              of v's returns with id != 0.  sem / ins and mover are voted separately: in a voxel shared by a mover and the
 *              room they can name different surfaces (sem / ins of the mover's majority class beside mover == 0, or the
 *              reverse).  Outputs (lrc_voxseq_out): ONE sparse list of every (slot, voxel) with >= 1 return, ascending by
 *              (slot, idx), idx within the slot; frame_offsets (F + 1 uint64): slot f owns entries
 *              [frame_offsets[f], frame_offsets[f + 1]), frame_offsets[F] is the list's length; an optional dense state of
 *              F * V bytes, slot-major (0 unknown, 1 free, 2 occupied); counts, F x 6 uint64 in the order of
 *              lrc_voxgrid_counts; one `skipped` word.
 * Every ray of an accumulate call reserves two 8-byte key slots until the next reset (the key buffers grow, no return is
 * dropped; at most 2^31 - 1 rays between resets).  The object is not thread-safe and its calls must be ordered on one
 * stream; "_dev" entry points enqueue on `stream`, the others return after the work finished. */
#define LRC_VOXSEQ_STATIC_ONLY 1u

typedef struct lrc_voxseq lrc_voxseq;

typedef struct lrc_voxseq_info {
    double   origin[3];
    double   voxel_size;
    int64_t  dims[3];
    uint64_t num_voxels;       /* V = nx*ny*nz, per slot                                           */
    uint64_t words_per_frame;  /* ceil(V / 32): the free bitset holds num_frames * this many words */
    uint64_t num_frames;       /* F                                                                */
    uint64_t reserved_keys;    /* rays accumulated since the last reset (key slots)                */
    uint64_t sparse_bound;     /* min(F * V, reserved_keys): capacity the sparse outputs need      */
} lrc_voxseq_info;             /* 96 bytes */

/* The outputs of finalize: device pointers for the _dev form, host pointers for the host form. */
typedef struct lrc_voxseq_out {
    uint32_t* idx;             /* (capacity)  linear index within the slot                         */
    uint16_t* sem;             /* (capacity)                                                       */
    uint16_t* ins;             /* (capacity)                                                       */
    uint32_t* returns;         /* (capacity)                                                       */
    uint8_t*  mover;           /* (capacity)  the mover vote                                       */
    uint32_t* mover_returns;   /* (capacity)  returns with mover id != 0                           */
    uint64_t* frame_offsets;   /* (F + 1)     required                                             */
    uint8_t*  state;           /* (F * V)     nullable                                             */
    uint64_t* counts;          /* (F, 6)      required; rows in the order of lrc_voxgrid_counts    */
    uint64_t* skipped;         /* (1)         required                                             */
} lrc_voxseq_out;              /* 80 bytes */

int lrc_voxseq_create(lrc_ctx* ctx, const double* origin3, double voxel_size, const int64_t* dims3, uint64_t num_frames,
                      lrc_voxseq** out_seq);
int lrc_voxseq_destroy(lrc_voxseq* seq);
int lrc_voxseq_get_info(const lrc_voxseq* seq, lrc_voxseq_info* out);
/* Clear the free bits, the returns and the counters (skipped and rejected included). */
int lrc_voxseq_reset(lrc_voxseq* seq, void* stream);
/* Walk the segments of num_poses * rays_per_pose records (pose-major, as every pose-batched scan writes them).  d_records is
 * a host struct of DEVICE pointers; its t, point3, sem and ins are required (LRC_ERR_INVALID_ARG otherwise), the other
 * columns are not read.  d_origins3: num_poses (origin_per_ray == 0) or num_poses * rays_per_pose (== 1) float32 triples. */
int lrc_voxseq_accumulate_dev(lrc_voxseq* seq, const float* d_origins3, int origin_per_ray, uint64_t num_poses,
                              uint64_t rays_per_pose, const uint32_t* d_frame_of_pose /* nullable */, uint64_t first_frame,
                              const lrc_hits* d_records, const uint8_t* d_mover /* nullable */, uint32_t flags,
                              void* stream);
/* The sparse columns need capacity >= sparse_bound entries each (unused tail entries are left as they were).  The _dev form
 * needs no host synchronisation; the host form synchronises and copies frame_offsets[F] entries. */
int lrc_voxseq_finalize_dev(lrc_voxseq* seq, uint32_t min_returns, const lrc_voxseq_out* d_out, uint64_t capacity,
                            void* stream);
int lrc_voxseq_finalize(lrc_voxseq* seq, uint32_t min_returns, const lrc_voxseq_out* out, uint64_t capacity);
/* Copy out the free bitset (num_frames * words_per_frame uint32; bit v of slot f is bit v % 32 of word
 * f * words_per_frame + v / 32). */
int lrc_voxseq_export_bits(lrc_voxseq* seq, uint32_t* out_bits);
/* Host step, no GPU: the walk of n segments o3[r] -> e3[r] (float32 triples) on a grid, compiled from the very functions the
 * kernel calls.  ORs the free bits into io_free_bits (ceil(V / 32) words), writes b = the voxel of e3[r] to out_end3 (n x 3
 * int64; inside the grid or not; zeros where o, e or a voxel coordinate was refused) and out_rejected[r] = 1 for a segment
 * the limits refuse.  A segment is walked whatever its range: the caller selects the returned rays. */
int lrc_voxseq_walk(const double* origin3, double voxel_size, const int64_t* dims3, const float* o3, const float* e3,
                    uint64_t n, uint32_t* io_free_bits, int64_t* out_end3, uint8_t* out_rejected);

/* ---- per-frame object annotations of scans ----------------------------------------------------
 * What a detector that trains on one sweep at a time needs, per (frame, object), in the SENSOR's frame: how many returns
 * the object got, how much of it is visible and where the visible part lies.  Definitions:
 *   object        object k is the k-th distinct label word key = sem | ins << 16 among the mesh's triangles, ascending
 *                 (the label-bit layout of lrc_hits.t_label).  Without label arrays there is one object, key 0; a NULL
 *                 tri_sem or tri_ins counts as all zero.  More than 4096 objects are refused (LRC_ERR_INVALID_ARG).
 *   static table  per object: key, tri_count (uint32), total_q (uint64: the sum of the quantised areas q of section 5e,
 *                 the same numbers lrc_coverage_export returns), wmin[3] / wmax[3] (float64: the AABB of the vertices of
 *                 the object's triangles, as given).  Built on the device at create; input checks as lrc_coverage_create.
 *   returned ray  as in section 5e: t finite and prim < num_triangles.  A returned ray whose point3 row has a non-finite
 *                 coordinate is ignored and counted in rejected_rays.  Rows of rays that do not return are never read.
 *   sensor frame  pose M (row-major 4x4 float64), R = M[:3,:3], c = M[:3,3], x = the ray's float32 point3 row widened
 *                 exactly: e = x - c, s_a = (R[0][a]*e_0 + R[1][a]*e_1) + R[2][a]*e_2, float64, no fused multiply-add.
 *   accumulators  returns (uint32): returned rays whose triangle belongs to k.  seen_tris (uint32): triangles of k with
 *                 at least one return in the frame.  seen_q (uint64): the sum of q over those triangles, each once per
 *                 frame however many rays hit it and however many calls deliver them.  vmin[3] / vmax[3] (float64): min
 *                 and max of s over the returns in the IEEE total order on finite values (-0.0 below +0.0); +inf / -inf
 *                 while returns == 0.
 *   accumulate    pose p of a call goes to frame first_frame + p; calls add up until reset.  Accumulating a frame twice
 *                 doubles returns and leaves seen_tris, seen_q, vmin and vmax as they were.  The result depends neither on
 *                 pose order, nor on chunking, nor on the order of atomics (integer counts and sums, an OR-ed bitset of
 *                 words_per_frame = ceil(T/32) words per frame, integer min / max on an order-preserving image).
 * The object is not thread-safe and its calls must be ordered on one stream; "_dev" entry points enqueue on `stream`,
 * the others return after the work finished. */
typedef struct lrc_frameobj lrc_frameobj;

typedef struct lrc_frameobj_info {
    uint64_t num_triangles;
    uint64_t num_frames;
    uint64_t num_objects;
    uint64_t words_per_frame;  /* ceil(num_triangles / 32)                                         */
    uint64_t rejected_rays;    /* returned rays with a non-finite point since the last reset       */
} lrc_frameobj_info;           /* 40 bytes */

int lrc_frameobj_create(lrc_ctx* ctx, const double* verts3, uint64_t num_vertices, const int32_t* tris3,
                        uint64_t num_triangles, const uint16_t* tri_sem /* nullable */,
                        const uint16_t* tri_ins /* nullable */, uint64_t num_frames, lrc_frameobj** out_fo);
int lrc_frameobj_destroy(lrc_frameobj* fo);
/* Synchronises the device (rejected_rays is read back). */
int lrc_frameobj_get_info(const lrc_frameobj* fo, lrc_frameobj_info* out);
/* The static table, num_objects rows: key, tri_count, total_q, wmin (K,3), wmax (K,3); any pointer may be NULL. */
int lrc_frameobj_objects(const lrc_frameobj* fo, uint32_t* out_key, uint32_t* out_tri_count, uint64_t* out_total_q,
                         double* out_wmin, double* out_wmax);
/* Zero the counts, the bitsets and rejected_rays; vmin / vmax back to +inf / -inf. */
int lrc_frameobj_reset(lrc_frameobj* fo, void* stream);
/* d_poses16 (num_poses x 16 float64, row-major 4x4) and the d_t / d_prim / d_point3 records of num_poses x rays_per_pose
 * rays, pose-major as lrc_scan_poses_dev writes them.  first_frame + num_poses > num_frames and NULL pointers are
 * refused with LRC_ERR_INVALID_ARG before anything is launched. */
int lrc_frameobj_accumulate_dev(lrc_frameobj* fo, const double* d_poses16, uint64_t num_poses, uint64_t rays_per_pose,
                                const float* d_t, const uint32_t* d_prim, const float* d_point3, uint64_t first_frame,
                                void* stream);
/* The per-(frame, object) arrays in C order: returns, seen_tris, seen_q (F, K); vmin, vmax (F, K, 3).  NULL skips one.
 * The host form waits for the device, then copies (blocking; rejected_rays is a separate lrc_frameobj_get_info call, which
 * waits again); the _dev form writes device memory on `stream`. */
int lrc_frameobj_export(lrc_frameobj* fo, uint32_t* out_returns, uint32_t* out_seen_tris, uint64_t* out_seen_q,
                        double* out_vmin, double* out_vmax);
int lrc_frameobj_export_dev(lrc_frameobj* fo, uint32_t* d_returns, uint32_t* d_seen_tris, uint64_t* d_seen_q,
                            double* d_vmin, double* d_vmax, void* stream);

/* Resident waves per CU the runtime grants the pose-batched trace kernel on this scene (its LDS stack is sized by
 * the tree depth), its VGPR count and LDS bytes per wave: the occupancy figure bench.py reports. */
int lrc_scene_get_occupancy(const lrc_scene* scene, int* waves_per_cu, int* vgprs, int* lds_bytes);

/* Number of traversal-kernel launches and rays issued on this scene so far (bench bookkeeping). */
int lrc_scene_get_counters(const lrc_scene* scene, uint64_t* launches, uint64_t* rays);

#ifdef __cplusplus
}
#endif
#endif /* LIDARCAST_H */
