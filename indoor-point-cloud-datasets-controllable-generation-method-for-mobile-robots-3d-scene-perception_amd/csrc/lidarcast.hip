// lidarcast.hip -- HIP kernels and C ABI of liblidarcast (gfx950 / MI355X only).
//
// Implements include/lidarcast.h.  Replaces, behind the reference's engine boundary
// (raycast_engine/raycast_engine.py:16-61), the Open3D/Embree work of
// raycast_engine/raycast_engine_cpu.py:46-73 and the numpy post-processing of :95-107,
// and, for pose batches, the per-waypoint loop body of s3dis_simulator.py:254-264.
//
// Kernels
//   trace_kernel<GEN,..> one lane per ray, one wave per workgroup; while-while BVH2 traversal with the per-lane
//                        stack in LDS ([depth][lane], conflict free); wave-uniform nodes fetched through the
//                        scalar cache (s_load); fused hit write-back (t, prim, normal, point, labels, range
//                        filter, incident angle, packed (t,label) pair, per-wave keep count).
//                        GEN = the ray generator (lrc_gen.h): explicit rays, or rays formed inside the kernel.
//                        QN = per-lane node fetches from the 32-byte quantised node images (15-bit grid per axis,
//                        one v_perm_b32 per plane); float32 world-space nodes for the rays the grid is not proven for.
//   compact_*            stable stream compaction of the fixed-stride records into frame order.
//   cloud_*              the same compaction with the hit point rebuilt from (t, label) pairs (multi-GPU assembly).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "lrc_internal.h"
#include "lrc_bvh.h"
#include "lrc_qnodes.h"
#include "lrc_device.h"
#include "lrc_gen.h"

using namespace lrcdev;

// ------------------------------------------------------------------------------------------------
// error plumbing (declared in lrc_internal.h)
// ------------------------------------------------------------------------------------------------
namespace {
thread_local std::string g_err;
}  // namespace

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// ------------------------------------------------------------------------------------------------
// argument checks shared with other units (declared in lrc_internal.h)
// ------------------------------------------------------------------------------------------------
// The mesh checks of lrc_coverage_create and lrc_frameobj_create; `who` is the entry point's name, the message's prefix.
int check_mesh(const char* who, const double* verts3, uint64_t V, const int32_t* tris3, uint64_t T) {
    for (uint64_t i = 0; i < 3 * V; ++i)
        if (!__builtin_isfinite(verts3[i])) return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": non-finite vertex");
    for (uint64_t i = 0; i < 3 * T; ++i)
        if (tris3[i] < 0 || (uint64_t)tris3[i] >= V)
            return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": triangle index out of range");
    return LRC_OK;
}

#ifndef LRC_REBUILD_R
#define LRC_REBUILD_R 2      // tiles (of 64 entries) one wave of the cloud rebuild handles (1, 2, 4, 8 measured equal)
#endif

// ------------------------------------------------------------------------------------------------
// device code
// ------------------------------------------------------------------------------------------------
namespace {

// A cloud rebuild from gathered triangle ids (lrc_cloud_from_prims_dev), as a kernel argument block.
struct RebuildParams {
    const double* __restrict__ poses16;
    const double* __restrict__ dirs_soa;     // direction table transposed to x[N] y[N] z[N]
    const uint32_t* __restrict__ prims;      // entry (pose p, ray i): slab p / pps, word (p % pps) * seg_len + i
    uint32_t pps;
    uint64_t stride;                         // words between slabs
    uint32_t seg_len, tps, ntiles, nseg;
    const float4* __restrict__ plane;
    uint32_t num_prims;
    const uint32_t* __restrict__ tile_off;
    const uint64_t* __restrict__ super_base;
    float4* __restrict__ out_xyzl;
    uint64_t* __restrict__ counts;
    uint32_t skip_slab;                      // tiles of this slab are not rebuilt (the caller scatters its own records); ~0u: none
};

// The lean record set of a pipeline submit (lrc_pipe_submit), as its consumers read it: per ray the 12-byte record
// (t bits, label, slot), per 64-ray tile the keep mask (bit l: lane l kept).  Only for segments of a multiple of 64 rays: tile t
// holds rays 64 t ... 64 t + 63 of ONE pose.  The tile's form is the trace wave's own decision, read where the trace read it:
// tab != NULL (the submit's launch carried this ray table) and the flag `same` of the tile's pose record in it -> RECORD form,
// the output row is pair_row(pose record's origin, table row's h, t, label) and `row` was not written; otherwise ROW form, `row`
// holds the packed row (x, y, z, label bits) exactly as it goes to lrc_compact_io::out_xyzl (zeros for a ray that is not kept).
struct LeanIn {
    const uint32_t* rec;       // three words per ray
    const float4* row;
    const uint64_t* keep_mask;
    const float4* tab;         // the set's own ray table (RayPose below: rows of seg_len, then the pose records), or NULL
};

struct TraceParams {
    const float4* nodes;
    const float4* tris;
    const uint32_t* slot_prim;
    const uint32_t* slot_label;
    const float* slot_box;     // per slot lo xyz, hi xyz of the triangle's vertices
    const float4* prim_plane;  // per caller's triangle row: (v0, label bits), (Ng, 0)
    uint32_t num_nodes;
    // kGenPoses with rays_per_pose % 64 == 0: tiles (workgroups) per pose -- a tile then lies in one pose, and the pose and the
    // tile's first in-pose index are scalar arithmetic on the 32-bit tile number.  0: per-lane 64-bit division, as for every other
    // generator.  (Placed in the padding behind num_nodes: the argument block keeps its size.)
    uint32_t tiles_per_pose;
    const uint4* nodes_q;      // QN kernels: 32-byte quantised nodes (per-lane fetches) ...
    const float4* nodes_n;     // ... and the same boxes as normalised float32 (scalar fetches)
    const uint4* nodes_q4;     // QN = 2: the tree collapsed to four children per node, 64 B per node ...
    const float4* nodes_n4;    // ... and 128 B per node as normalised float32
    uint32_t stack_cap;        // entries of the per-lane LDS stack
    uint32_t tile_chunk_log2;  // 0: eight contiguous tile ranges, one per XCD; k + 1: chunks of 2^k tiles round robin
    uint32_t force_redo;       // test hook (LRC_DEBUG_FORCE_REDO=m): rays with gid % m == 0 take the redo path as well
    // lean record set with tiles_per_pose != 0 only (lrc_pipe_submit): lines of the scan pattern are 64 * line_tiles rays long
    // and a tile takes 64 / L columns of L = 2 or 4 adjacent lines (lrc_device.h, tile_ray; line_group below).  0: 64
    // consecutive rays.  (In the padding behind force_redo.)
    uint32_t line_tiles;
    uint64_t* chain_word;      // launch chain (lrc_ctx::chain_word): the last workgroup stores chain_seq here when it starts
    uint64_t chain_seq;
    // scan pipeline (lrc_pipe): the first pre.blocks workgroups of the launch do not trace -- each compacts one 64-entry
    // tile of an EARLIER scan's records (whose offsets a scan pass has tabulated).  They are handed out first, i.e. into the
    // wave slots the previous launch's long last waves leave empty, and are gone in microseconds; the trace tiles follow in
    // the same grid with no barrier in between.
    struct Pre {
        uint32_t blocks;           // leading workgroups in all; each scatter workgroup takes kPreTiles tiles
        uint32_t rows_only;        // only the packed (x, y, z, label) rows (+ counts) are asked for: the batched form
        // sharded form (lrc_pipe_submit_sharded): the assembly of an EARLIER scan of all ranks rides here -- the first
        // own_blocks workgroups scatter this rank's own rows from its records at the offsets of the assembled cloud
        // (tile_base, super_base: the scan over ALL ranks' keep counts), the others rebuild the other ranks' rows from their
        // gathered triangle ids (rebuild_tiles, LRC_REBUILD_R tiles each; tiles of the own slab are skipped)
        uint32_t sharded, own_blocks;
        uint64_t tile_base;
        const uint64_t* super_base;
        RebuildParams rq;
        uint64_t seg_len, tps, ntiles, nseg;
        const uint32_t* tile_off;
        const uint32_t* super_total;
        lrc_compact_io io;
        LeanIn lean;               // plain form: the earlier scan's lean record set (io's t / point3 / sem / ins are not read)
    } pre;
    // lean record set (scan pipeline): row != NULL -> write_back stores per ray the 12-byte record, per wave the keep mask, and
    // no column of `out`.  Wave-uniform: a run-time branch.  A wave that did not take the prepared path
    // (no ray table, or its pose turns relative to pose 0) stores the packed row into `row` as well: see LeanIn.
    struct Lean {
        float4* row;
        uint32_t* rec;             // (t bits, label, slot): t after range noise; (inf, 0, 0xFFFFFFFF) for a ray that is not kept
        uint64_t* keep_mask;
    } lean;
    float qbase[3], qW[3], qinvW[3];   // normalised coordinate n = (x - qbase) * qinvW in [2, 4); qW = 1 / qinvW = 2^k
    // inputs
    const float* rays6;        // explicit rays (kGenRays)
    const uint64_t* seg_offsets;   // explicit rays in S segments (poses): (S+1) ray offsets, or NULL
    const double* seg_centers3;    // (S,3) range-filter centres of the segments
    uint32_t num_segments;
    // with line_tiles != 0: the line grouping of the tiles (lrc_device.h, tile_ray: bit 31 = groups of four lines, bits 0-30 =
    // the first line of the other elevation sign).  0: groups of two from line 0.  (In the padding behind num_segments.)
    uint32_t line_group;
    const double* poses16;     // kGenPoses, kGenAngles and every generator that scans from poses
    const double* dirs3;       // kGenPoses: (N,3) sensor-frame direction table
    // kGenAngles: (P*N,2) noisy (phi, theta) of the dual-axis sensor.  kGenPoses never reads them, and only kGenPoses reads the ray
    // table of a prepared pipeline submit (RayPose below; NULL: none), so the two share one slot: the argument block keeps its
    // size, on which the register allocation of the product kernel has depended before.
    union {
        const double* angles2;
        const float4* ray_tab;
    };
    const uint8_t* keep_mask;  // kGenAngles, nullable: 0 = ray dropped by the sensor (never cast, reported as a miss)
    uint32_t* stats;           // STATS build only: kStatsWords counters per ray
    uint64_t rays_per_pose;
    uint64_t total;
    int has_center;
    double cx, cy, cz;
    double max_range;
    // opt-in sensor-realism options (lrc_scan_options; all off by default = the reference's behaviour)
    double min_range;
    const float* range_noise;
    int incident_mode;
    lrc_hits out;
    // kGenSweeps (moving-sensor sweeps, lrc_scan_sweeps_*): (P,24) motion records and the (N) firing fractions of the table
    const double* motion24;
    const double* fire;
    // kGenNoisy (seeded sensor noise, lrc_scan_noisy_*): generator parameters and the resident quantile table
    lrcnoise::Params noise;
    // kGenEchoes (beam footprint and multi-echo returns, lrc_scan_echoes_*): the offset table and the reduction's parameters.  For
    // this generator rays_per_pose and total count LANES (G per beam, lrc_echo.h) in the kernel; launch_trace converts them
    lrcecho::Params echo;
    // kGenMaterials (surface materials, lrc_scan_materials_*): the resident table, the model's limits and the two per-ray outputs that
    // travel beside the record set (lrc_material.h)
    lrcmat::Params mat;
};

// workgroup -> tile remap: consecutive tiles land on the same XCD (blocks b, b+8, ... share an L2),
// so each XCD's 4 MiB L2 keeps the part of the scene its run of poses/scanlines looks at.
// klog > 0: the tiles are dealt to the XCDs in chunks of 2^(klog-1) consecutive tiles, round robin (chunk c -> XCD c % 8),
// instead of eight contiguous ranges.  Tiles beyond the last full round of eight chunks keep their own number.  Shifts
// and masks of wave-uniform values only: the scalar unit does it.
__device__ __forceinline__ uint32_t xcd_tile_chunked(uint32_t b, uint32_t nwg, uint32_t klog) {
    const uint32_t k = klog - 1u;
    const uint32_t full = (nwg >> (k + 3u)) << (k + 3u);
    if (b >= full) return b;
    const uint32_t x = b & 7u, j = b >> 3;
    return ((((j >> k) << 3) + x) << k) | (j & ((1u << k) - 1u));
}

__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t nwg) {
#ifdef LRC_NO_XCD_REMAP
    return b;      // A/B build only
#endif
    uint32_t q = nwg >> 3, r = nwg & 7u, x = b & 7u;
    uint32_t base = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (b >> 3);
}

struct alignas(16) F4 { float x, y, z, w; };                       // plain 16-byte record (loads as dwordx4)
// the 12-byte record of a lean record set (LeanIn) and its first two words, as the compiler's vector types at the alignment the
// packed array gives them: one dwordx3 store, one dwordx2 load
typedef uint32_t u32x3_ __attribute__((ext_vector_type(3)));
typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));
typedef u32x3_ rec3 __attribute__((aligned(4)));
typedef u32x2_ rec2 __attribute__((aligned(4)));
typedef __attribute__((address_space(4))) const float cfloat;      // constant address space: uniform loads become s_load
__device__ __forceinline__ F4 ld_uniform(const float4* gp) {
    cfloat* c = (cfloat*)gp;
    return F4{c[0], c[1], c[2], c[3]};
}

// ---- cloud rebuild from triangle ids: the device part ----
// R independent entries per lane: all ids are fetched first, then all plane records, then the arithmetic -- a chain
// of dependent gathers wants loads in flight per wave.  plane: 2 x float4 per triangle row: (v0, label bits), (Ng, 0)
// -- all a known hit needs to give t again.  Tiles [tile0, tile0 + R) below `limit` are processed.
template <int R>
__device__ __forceinline__ void rebuild_tiles(const RebuildParams& q, uint32_t tile0, uint32_t limit, uint32_t lane) {
    uint32_t seg[R], idx[R], prim[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t tile = tile0 + k;
        prim[k] = LRC_INVALID_PRIM;
        seg[k] = 0; idx[k] = 0;
        if (tile < limit) {
            seg[k] = tile / q.tps;
            const uint32_t chunk = tile - seg[k] * q.tps, sb = seg[k] / q.pps;
            idx[k] = chunk * 64u + lane;
            if (idx[k] < q.seg_len && sb != q.skip_slab)     // read once: streaming load
                prim[k] = __builtin_nontemporal_load(q.prims + (uint64_t)sb * q.stride +
                                                     (uint64_t)(seg[k] - sb * q.pps) * q.seg_len + idx[k]);
        }
    }
    float4 pa[R], pb[R];
    double da[R], db[R], dc[R];
    uint64_t dst[R];
    bool keep[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        keep[k] = prim[k] != LRC_INVALID_PRIM;
        const unsigned long long m = __ballot(keep[k]);
        pa[k] = pb[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        da[k] = db[k] = dc[k] = 0.0;
        dst[k] = 0;
        if (keep[k]) {
            const uint32_t tile = tile0 + k;
            // the tile's offset is wave-uniform too (written by the scan kernel before this launch): scalar loads
            typedef __attribute__((address_space(4))) const uint64_t cu64;
            typedef __attribute__((address_space(4))) const uint32_t cu32;
            dst[k] = ((cu64*)q.super_base)[tile >> 10] + ((cu32*)q.tile_off)[tile] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
            da[k] = q.dirs_soa[idx[k]];
            db[k] = q.dirs_soa[(size_t)q.seg_len + idx[k]];
            dc[k] = q.dirs_soa[2 * (size_t)q.seg_len + idx[k]];
        }
        if (keep[k] && prim[k] < q.num_prims) {   // an id that is not a triangle of this scene: zero plane, never a wild read
            pa[k] = q.plane[(size_t)prim[k] * 2];
            pb[k] = q.plane[(size_t)prim[k] * 2 + 1];
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (!keep[k]) continue;
        // the tile's pose is wave-uniform: its matrix comes through the scalar cache (constant address space), not as twelve
        // 64-lane loads of one address through the vector memory path, which is what bounds this kernel
        typedef __attribute__((address_space(4))) const double cdouble;
        cdouble* M = (cdouble*)(q.poses16 + (size_t)seg[k] * 16);
        // gen_ray, with the direction already in registers (same FMA chain, lrc_device.h)
        V3 o, d, h, pt;
        d.x = (float)dgemm_row(da[k], db[k], dc[k], M[0], M[1], M[2]);
        d.y = (float)dgemm_row(da[k], db[k], dc[k], M[4], M[5], M[6]);
        d.z = (float)dgemm_row(da[k], db[k], dc[k], M[8], M[9], M[10]);
        o.x = (float)M[3]; o.y = (float)M[7]; o.z = (float)M[11];
        // the sender's scan established that this ray hits this triangle; t is the expression tri_hit evaluates
        // (T/|den| with T = Ng.(v0-O), den = Ng.D, sign-corrected), so v0 and Ng are all that is needed
        const V3 v0{pa[k].x, pa[k].y, pa[k].z}, ng{pb[k].x, pb[k].y, pb[k].z};
        const float den = dot3(ng, d);
        const uint32_t sgn = __float_as_uint(den) & 0x80000000u;
        const float t = xorsign(dot3(ng, sub3(v0, o)), sgn) / __builtin_fabsf(den);
        hit_point(o, d, t, h, pt);
        // streaming store: the rows are never read back here, and must not push the plane table out of the L2
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f row = {pt.x, pt.y, pt.z, pa[k].w};
        __builtin_nontemporal_store(row, (v4f*)(q.out_xyzl + dst[k]));
    }
}

// per-pose (segment) row counts from the scanned tile offsets: thread sg writes counts[sg]
__device__ __forceinline__ void rebuild_counts(const RebuildParams& q, uint32_t first, uint32_t step) {
    if (!q.counts) return;
    const uint32_t nsuper = (q.ntiles + 1023u) / 1024u;
    for (uint32_t sg = first; sg < q.nseg; sg += step) {
        const uint64_t g0 = (uint64_t)sg * q.tps, g1 = g0 + q.tps;
        const uint64_t o0 = g0 >= q.ntiles ? q.super_base[nsuper] : q.super_base[g0 >> 10] + q.tile_off[g0];
        const uint64_t o1 = g1 >= q.ntiles ? q.super_base[nsuper] : q.super_base[g1 >> 10] + q.tile_off[g1];
        q.counts[sg] = o1 - o0;
    }
}

// the unit normal of the record from the third float4 of a triangle slot (Ng in y, z, w): write_back and the expansion of a
// lean pipeline record set (expand_lean_kernel) both form it here, so the two cannot drift by a bit
__device__ __forceinline__ void slot_normal(float4 c, float& nx, float& ny, float& nz) {
    const float len = __builtin_sqrtf(fma_(c.w, c.w, fma_(c.z, c.z, c.y * c.y)));
    nx = c.y / len; ny = c.z / len; nz = c.w / len;
}

// The range filter of a ray that has a hit, shared by the lean and the plain write-back: keep &= sqrt(s) < max_range (and >=
// min_range, opt-in), s the squared float64 distance to the filter centre.  Where the launch has bounds around max_range^2
// (lrc_device.h, range_band), no opt-in needs the distance itself and no ray of the wave falls between the bounds, s is compared
// with the lower bound and the float64 square root (v_rsq_f64 and its Newton steps, at half rate) is never formed; otherwise the
// whole wave takes the square root.  Returns the distance, or 0 where it was not formed (then no output reads it).
template <bool FILTER>
__device__ __forceinline__ double range_filter(const TraceParams& p, double s, bool& keep) {
    const bool filter = FILTER || p.has_center;
    const RangeBand rb = range_band(p.max_range);      // wave-uniform: a handful of instructions on a kernel argument
    const bool need_dist = !rb.fast | !filter | (p.min_range > 0.0) | (p.out.incident_deg != nullptr);   // wave-uniform
    if (!need_dist && __builtin_amdgcn_ballot_w64(range_in_band(s, rb.lo, rb.hi)) == 0ull) {
        keep = range_below(s, rb.lo);
        return 0.0;
    }
    const double dist = __builtin_sqrt(s);
    if (filter) keep = dist < p.max_range;
    if (p.min_range > 0.0) keep = keep & (dist >= p.min_range);     // opt-in; the reference never applies it
    return dist;
}

// ---- fused write-back: everything after the closest hit is known (shared by the trace kernels) ------------------
// best_slot = 0xFFFFFFFF: no hit.  FILTER: apply the max_range filter (scans and casts with a centre).
// BY_PRIM: `best_slot` is the caller's triangle ROW (sector_kernel keys rays by (t, row)); labels and the normal then
// come from the per-row plane table instead of the per-slot arrays -- same values.
// HAVE_LABEL: the caller has slot_label[best_slot] already (trace_kernel issues the load together with the box clause's).
// MAT: the intensity column receives the caller's value (the material chain's I, trace_kernel kGenMaterials) in the place of |h.n|.
// GIVEN: the hit was found elsewhere (mover_merge_kernel: the winner among the static scene and the movers): `best_slot` is
// the triangle ROW to report, slot_label_in its label and n_in the normal to write and to use; no scene array is read.
// Returns whether the ray is kept.
template <bool FILTER_ALWAYS, bool BY_PRIM = false, bool HAVE_LABEL = false, bool MAT = false, bool GIVEN = false>
__device__ __forceinline__ bool write_back(const TraceParams& p, uint64_t gid, uint32_t tid, V3 o, V3 d, double cx,
                                           double cy, double cz, float tbest, uint32_t best_slot, uint32_t slot_label_in = 0u,
                                           bool have_h = false, V3 h_in = V3{0.f, 0.f, 0.f}, float inten_in = 0.f,
                                           V3 n_in = V3{0.f, 0.f, 0.f}) {
    const bool lean = FILTER_ALWAYS && !BY_PRIM && p.lean.row != nullptr;    // a kernel argument: wave-uniform
    bool keep = best_slot != 0xFFFFFFFFu;
    float t_out = __builtin_inff();
    uint32_t prim = LRC_INVALID_PRIM;
    float nx = 0.f, ny = 0.f, nz = 0.f, px = 0.f, py = 0.f, pz = 0.f;
    uint32_t label = 0;
    double inc = 0.0;
    float inten = 0.f;
    if (keep && p.range_noise) {
        // opt-in range noise (the reference declares range_noise_std but never applies it, lidar_intrinsics.py:
        // 364-389 has no caller): host-drawn additive noise on the range; a non-positive range drops the return
        tbest = tbest + p.range_noise[gid];
        keep = tbest > 0.0f;
    }
    if (keep) {
        // p = o + (d/|d|)*t : numpy float32, one rounding per operation (raycast_engine_cpu.py:57-62)
        // have_h (wave-uniform): the unit direction comes from the ray table of a prepared submit -- unit_dir's own bits
        V3 hh, pp;
        if (have_h) {
            hh = h_in;
            const PairRow r = pair_row(o, hh, tbest, 0u);      // what the consumers of the record form again (LeanIn)
            pp.x = r.x; pp.y = r.y; pp.z = r.z;
        } else {
            hit_point(o, d, tbest, hh, pp);
        }
        const float hx = hh.x, hy = hh.y, hz = hh.z;
        px = pp.x; py = pp.y; pz = pp.z;
        // range filter + incident angle in float64 (raycast_engine_cpu.py:95-107)
        const double ex = (double)px - cx, ey = (double)py - cy, ez = (double)pz - cz;
        const double dist = range_filter<FILTER_ALWAYS>(p, (ex * ex + ey * ey) + ez * ez, keep);
        if (keep && lean) {           // the lean record: no triangle id, no normal
            t_out = tbest;
            label = HAVE_LABEL ? slot_label_in : p.slot_label[best_slot];
        } else if (keep) {
            t_out = tbest;
            if (GIVEN) {
                prim = best_slot;
                label = slot_label_in;
            } else if (BY_PRIM) {
                prim = best_slot;
                label = __float_as_uint(p.prim_plane[(size_t)best_slot * 2].w);
            } else {
                prim = p.slot_prim[best_slot];
                label = HAVE_LABEL ? slot_label_in : p.slot_label[best_slot];
            }
            if (p.out.normal3 || p.out.intensity || (p.out.incident_deg && p.incident_mode == 1)) {
                if (GIVEN) {
                    nx = n_in.x; ny = n_in.y; nz = n_in.z;
                } else {
                    float4 c;
                    if (BY_PRIM) { const float4 g = p.prim_plane[(size_t)best_slot * 2 + 1]; c = make_float4(0.f, g.x, g.y, g.z); }
                    else c = p.tris[(size_t)best_slot * 3 + 2];
                    slot_normal(c, nx, ny, nz);
                }
            }
            if (p.out.incident_deg) {
                if (p.incident_mode == 1) {   // opt-in: angle between the ray and the surface normal
                    const double cs = __builtin_fabs(((double)hx * (double)nx + (double)hy * (double)ny) +
                                                     (double)hz * (double)nz);
                    inc = acos(cs < 1.0 ? cs : 1.0) * kRadToDeg;
                } else {
                    inc = acos(__builtin_fabs(ez / dist)) * kRadToDeg;
                }
            }
            if (p.out.intensity)      // opt-in: Lambertian return |h.n|, float32 (same FMA order as every dot product here)
                inten = MAT ? inten_in : __builtin_fabsf(fma_(hz, nz, fma_(hy, ny, hx * nx)));
            if (!p.out.normal3) { nx = ny = nz = 0.f; }
        } else {
            px = py = pz = 0.f;
        }
    }
    if (lean) {
        // one 12-byte store per ray: all a consumer needs to form the row of a prepared wave again (pair_row) and the expansion
        // for lrc_pipe_records to find triangle id and normal.  A wave that did not take the prepared path (have_h is
        // wave-uniform: one pose per tile) has no table row to form its point from later and stores the packed row beside it.
        // The keep mask goes as four 16-bit words: each quarter of the wave is a quarter of a 1-D tile (of four different ones in a
        // four-line tile, lrc_device.h tile_ray), so up to four waves fill one mask, no atomics, nothing to zero.  The per-tile
        // counts of a lean set are the scan pass's to form (popcount of the masks, compact_scan_masks_kernel).
        const unsigned long long m = __ballot(keep);
        if ((tid & 15u) == 0) ((uint16_t*)p.lean.keep_mask)[gid >> 4] = (uint16_t)(m >> (tid & 48u));
        const rec3 r = {__float_as_uint(t_out), label, keep ? best_slot : 0xFFFFFFFFu};
        *(rec3*)(p.lean.rec + gid * 3) = r;
        if (!have_h) p.lean.row[gid] = make_float4(px, py, pz, __uint_as_float(label));
        return keep;
    }
    if (p.out.tile_count) {   // kept rays of this wave's 64 consecutive outputs (feeds lrc_compact_dev)
        const unsigned long long m = __ballot(keep);
        if ((tid & 63u) == 0) p.out.tile_count[gid >> 6] = (uint32_t)__popcll(m);
    }
    if (p.out.t) p.out.t[gid] = t_out;
    if (p.out.t_label) ((uint2*)p.out.t_label)[gid] = make_uint2(__float_as_uint(t_out), label);
    if (p.out.prim) p.out.prim[gid] = prim;
    if (p.out.normal3) { float* q = p.out.normal3 + gid * 3; q[0] = nx; q[1] = ny; q[2] = nz; }
    if (p.out.point3) { float* q = p.out.point3 + gid * 3; q[0] = px; q[1] = py; q[2] = pz; }
    if (p.out.sem) p.out.sem[gid] = (uint16_t)(label & 0xFFFFu);
    if (p.out.ins) p.out.ins[gid] = (uint16_t)(label >> 16);
    if (p.out.incident_deg) p.out.incident_deg[gid] = inc;
    if (p.out.intensity) p.out.intensity[gid] = inten;
    return keep;
}

// ---- moving objects: the mover scan family (lrc_scan_movers_*, lrc_scan_noisy_movers_*, lrc_scan_mover_sweeps_*,
// lrc_scan_noisy_mover_sweeps_*; the arithmetic is lrc_movers.h's and the generators', the orchestration movers_scan_dev's;
// DESIGN.md sections 5k, 5n, 5r, 5t) -------------------------------------------------------------------------------------------
// One algorithm under two switches.  SWEEP: the sensor's records are (P,24) motion records and a mover is met at the pose its
// (P,M,24) record has at the ray's firing fraction s = (float)fire[i] (to_object_at / to_world_at), not at its (P,M,12) pose.
// NOISY: the ray is the noisy generator's, with a live byte (0: dropped, never cast), and the last merge draws the winner's range.
//
// Pose of ray gid and, with `uniform` (rays_per_pose % 64 == 0: a wave lies in one pose), the same value as a scalar, so that what
// is read per pose comes through the scalar cache.
__device__ __forceinline__ uint32_t mover_pose_of(uint64_t gid, uint64_t rays_per_pose, int uniform) {
    uint32_t pose = (uint32_t)(gid / rays_per_pose);
    if (uniform) pose = (uint32_t)__builtin_amdgcn_readfirstlane((int)pose);
    return pose;
}
// The WORDS words that are read of record (pose, m) of a (P, M, STRIDE) float32 table -- a pose12 (12 of 12) or a mover sweep
// record (19 of 24) --: through the scalar cache where a wave lies in one pose.
template <int WORDS, int STRIDE>
__device__ __forceinline__ void mover_record_load(const float* records, uint32_t pose, uint32_t M, uint32_t m, int uniform, float* out) {
    const float* mp = records + ((size_t)pose * M + m) * STRIDE;
    if (uniform) {
        cfloat* c = (cfloat*)mp;
#pragma unroll
        for (int k = 0; k < WORDS; ++k) out[k] = c[k];
    } else {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) out[k] = mp[k];
    }
}
template <bool SWEEP> constexpr int kMoverWords = SWEEP ? 19 : 12;
template <bool SWEEP> constexpr int kMoverStride = SWEEP ? 24 : 12;

// Ray gid of a ray set as three float2 (24-byte records: 8-byte aligned).  T: V3 or lrcmov::Vec.
template <class T>
__device__ __forceinline__ void store_ray6(float* rays6, uint64_t gid, T o, T d) {
    float2* r = (float2*)(rays6 + gid * 6);
    r[0] = make_float2(o.x, o.y);
    r[1] = make_float2(o.z, d.x);
    r[2] = make_float2(d.y, d.z);
}
template <class T>
__device__ __forceinline__ void load_ray6(const float* rays6, uint64_t gid, T& o, T& d) {
    const float2* r = (const float2*)(rays6 + gid * 6);
    const float2 a = r[0], b = r[1], c = r[2];
    o = T{a.x, a.y, b.x};
    d = T{b.y, c.x, c.y};
}

// The ray kernel: one thread per (pose, i).  The static pass (q.records == NULL) forms the variant's generator's bits and stores
// them: the clean non-sweep variant straight as the rays to cast, the other three as the world ray set (world6), the noisy ones
// with the ray's live byte -- the one Philox block for the jitter and the dropout, the one float64 chain.  A mover's pass takes
// the world ray into the mover's frame and stores it with the keep byte of the explicit-ray launch (0: dropped, or left out by
// lrcmov::culled; no ray stored).  The three variants that stored the world ray read it back (no float64 chain, no division per
// mover); the clean non-sweep variant has no world6 and forms gen_ray's bits again.  The zero tests are on kernel arguments.
// Side by side, and kept: only the noisy sweep static pass zeroes a dropped ray's stored ray; the noisy non-sweep one stores
// what the generator left.
template <bool SWEEP, bool NOISY>
__global__ __launch_bounds__(kBlock) void mover_rays_kernel(const double* __restrict__ sensor, const double* __restrict__ dirs3,
                                                            const double* __restrict__ fire, const lrcnoise::Params np,
                                                            uint64_t rays_per_pose, uint64_t total, const lrcmov::RayPass q,
                                                            int uniform, float* __restrict__ world6, uint8_t* __restrict__ live,
                                                            float* __restrict__ rays6, uint8_t* __restrict__ keep) {
    constexpr bool STORED = SWEEP || NOISY;
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= total) return;
    const uint32_t pose = mover_pose_of(gid, rays_per_pose, uniform);
    const uint64_t i = gid - (uint64_t)pose * rays_per_pose;
    const bool first = q.records == nullptr;
    V3 o, d;
    if (first || !STORED) {
        double cx, cy, cz;
        bool alive = true;
        if constexpr (SWEEP && NOISY) gen_ray_noisy_sweep(sensor, dirs3, fire, np, pose, i, o, d, alive);
        else if constexpr (SWEEP) gen_ray_sweep(sensor, dirs3, fire, pose, i, o, d);
        else if constexpr (NOISY) gen_ray_noisy(sensor, dirs3, np, pose, i, o, d, cx, cy, cz, alive);
        else gen_ray(sensor, dirs3, pose, i, o, d, cx, cy, cz);
        if (first) {
            if constexpr (SWEEP && NOISY) { if (!alive) o = d = V3{0.f, 0.f, 0.f}; }
            store_ray6(STORED ? world6 : rays6, gid, o, d);
            if constexpr (NOISY) live[gid] = alive ? (uint8_t)1 : (uint8_t)0;
            return;
        }
    }
    if constexpr (NOISY) {
        if (live[gid] == 0) {      // dropped: cast against no mover either
            keep[gid] = 0;
            return;
        }
    }
    float rec[kMoverWords<SWEEP>];
    mover_record_load<kMoverWords<SWEEP>, kMoverStride<SWEEP>>(q.records, pose, q.M, q.m, uniform, rec);
    lrcmov::Vec wo, wd, ro, rd;
    if constexpr (STORED) {
        load_ray6(world6, gid, wo, wd);
    } else {
        wo = lrcmov::Vec{o.x, o.y, o.z};
        wd = lrcmov::Vec{d.x, d.y, d.z};
    }
    if constexpr (SWEEP) lrcmov::to_object_at(rec, (float)fire[i], wo, wd, ro, rd);
    else lrcmov::to_object(rec, wo, wd, ro, rd);
    const bool out = lrcmov::culled(q.sphere, ro, rd);
    keep[gid] = out ? (uint8_t)0 : (uint8_t)1;
    if (out) return;
    store_ray6(rays6, gid, ro, rd);
}

// The merge kernel's view of one mover's pass: the running winner (the static cast's record set to begin with), this mover's
// cast, and -- in the last pass -- the caller's record set (p.out) and mover column.  p brings the sensor's records, the firing
// fractions and the model (p.noise).
struct MoverMerge {
    const float* records;      // (P, M, 12) poses, or (P, M, 24) mover sweep records
    const float* world6;       // the static pass's world rays; unused by the clean non-sweep variant, which stores none
    uint32_t M, m;
    int uniform, last;
    float* w_t; uint32_t* w_prim; float* w_n3; uint16_t* w_sem; uint16_t* w_ins; uint8_t* w_who;
    const float* m_t; const uint32_t* m_prim; const float* m_n3; const uint16_t* m_sem; const uint16_t* m_ins;
    uint8_t* d_mover;          // nullable
};
struct MoverWinner { float t; uint32_t prim, label; V3 n; uint32_t who; };

// The running winner of ray gid against mover q.m (lrcmov::takes: on the CLEAN ranges; a dropped ray was cast nowhere, +inf
// throughout), the mover's normal turned into the world by its pose, or by the pose it has at s (`fire`: the firing fractions).
template <bool SWEEP>
__device__ __forceinline__ MoverWinner mover_take(const MoverMerge& q, const double* fire, uint64_t gid, uint32_t pose, uint64_t i) {
    MoverWinner w{q.w_t[gid], q.w_prim[gid], (uint32_t)q.w_sem[gid] | ((uint32_t)q.w_ins[gid] << 16),
                  V3{q.w_n3[gid * 3], q.w_n3[gid * 3 + 1], q.w_n3[gid * 3 + 2]}, q.w_who[gid]};
    const float tm = q.m_t[gid];
    if (lrcmov::takes(tm, w.t)) {
        float rec[kMoverWords<SWEEP>];
        mover_record_load<kMoverWords<SWEEP>, kMoverStride<SWEEP>>(q.records, pose, q.M, q.m, q.uniform, rec);
        const lrcmov::Vec mn{q.m_n3[gid * 3], q.m_n3[gid * 3 + 1], q.m_n3[gid * 3 + 2]};
        lrcmov::Vec n;
        if constexpr (SWEEP) n = lrcmov::to_world_at(rec, (float)fire[i], mn);
        else n = lrcmov::to_world(rec, mn);
        w.t = tm;
        w.prim = q.m_prim[gid];
        w.label = (uint32_t)q.m_sem[gid] | ((uint32_t)q.m_ins[gid] << 16);
        w.n = V3{n.x, n.y, n.z};
        w.who = q.m + 1u;
    }
    return w;
}
__device__ __forceinline__ void winner_store(const MoverMerge& q, uint64_t gid, const MoverWinner& w) {
    q.w_t[gid] = w.t;
    q.w_prim[gid] = w.prim;
    q.w_n3[gid * 3] = w.n.x; q.w_n3[gid * 3 + 1] = w.n.y; q.w_n3[gid * 3 + 2] = w.n.z;
    q.w_sem[gid] = (uint16_t)(w.label & 0xFFFFu);
    q.w_ins[gid] = (uint16_t)(w.label >> 16);
    q.w_who[gid] = (uint8_t)w.who;
}

// One thread per (pose, i): mover_take; every pass but the last stores the winner.  The last pass writes the record the
// variant's plain scan (lrc_scan_poses_dev, lrc_scan_noisy_dev, lrc_scan_sweeps_dev, lrc_scan_noisy_sweeps_dev) would write had
// the ray hit the winner (write_back, GIVEN), filter included, and the mover column.  Its ray and filter centre, side by side and
// kept as they are: the clean non-sweep variant forms gen_ray's bits again; the others read the stored world ray back, the
// noisy non-sweep one with the centre from the pose (poses16[3], [7], [11]), the sweep ones with sweep_centre of the sensor's
// record.  NOISY draws the winner's range (noisy_range of frame first_frame + pose: the ray's second Philox block, only where
// range_std != 0 and something was hit; a non-positive range is no return).
template <bool SWEEP, bool NOISY>
__global__ __launch_bounds__(kBlock) void mover_merge_kernel(const TraceParams p, const MoverMerge q) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= p.total) return;
    const uint32_t pose = mover_pose_of(gid, p.rays_per_pose, q.uniform);
    const uint64_t i = gid - (uint64_t)pose * p.rays_per_pose;
    MoverWinner w = mover_take<SWEEP>(q, p.fire, gid, pose, i);
    if (!q.last) {
        winner_store(q, gid, w);
        return;
    }
    V3 o, d;
    double cx, cy, cz;
    if constexpr (!SWEEP && !NOISY) {
        gen_ray(p.poses16, p.dirs3, pose, i, o, d, cx, cy, cz);
    } else {
        load_ray6(q.world6, gid, o, d);
        if constexpr (SWEEP) {
            sweep_centre(p.motion24 + (size_t)pose * 24, p.fire[i], cx, cy, cz);
        } else {
            const double* Mp = p.poses16 + (size_t)pose * 16;
            cx = Mp[3]; cy = Mp[7]; cz = Mp[11];
        }
    }
    bool hit = w.t < __builtin_inff();
    if constexpr (NOISY) {
        if (p.noise.range_std != 0.0f && hit) {
            w.t = noisy_range(p.noise, p.noise.first_frame + pose, (uint32_t)i, w.t);
            hit = w.t > 0.0f;
        }
    }
    const bool kept = write_back<true, false, true, false, true>(p, gid, threadIdx.x, o, d, cx, cy, cz, w.t, hit ? w.prim : 0xFFFFFFFFu,
                                                                 w.label, false, V3{0.f, 0.f, 0.f}, 0.f, w.n);
    if (q.d_mover) q.d_mover[gid] = kept ? (uint8_t)w.who : (uint8_t)0;
}

// ---- scene flow under movers (lrc_scan_flow_*; the arithmetic is lrc_flow.h's, the orchestration flow_scan_dev's) -------------
// What the flow's ray kernel reads and writes.  The four line-of-sight columns are NULL together (flow only).
struct FlowRays {
    const float* t; const float* point3; const uint8_t* mover;       // the records of lrc_scan_movers_dev; mover nullable (all room)
    const float* A; const float* B;                                  // (P, M, 12) each; unread with M == 0
    const double* next16; const uint8_t* has_next;                   // (P, 16); (P) nullable: all ones
    uint32_t M;
    uint64_t rays_per_pose, total;
    double max_range, min_range;
    float* flow3;
    float* rays6; uint8_t* keep; float* thr; uint8_t* status;
};

// One thread per record: steps 1 to 3 of the header.  The row's own pose pair is a per-lane fetch by w; most lanes have w == 0
// and fetch nothing.
__global__ __launch_bounds__(kBlock) void flow_rays_kernel(const FlowRays q) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= q.total) return;
    const uint32_t pose = (uint32_t)(gid / q.rays_per_pose);
    const bool live = (q.t[gid] < __builtin_inff()) & (q.has_next == nullptr || q.has_next[pose] != 0);
    const uint32_t w = (live && q.mover) ? q.mover[gid] : 0u;
    float x[3] = {0.f, 0.f, 0.f}, A[12], B[12];
    bool moved = false;
    if (live) {
        x[0] = q.point3[gid * 3]; x[1] = q.point3[gid * 3 + 1]; x[2] = q.point3[gid * 3 + 2];
    }
    if (w != 0u && w <= q.M) {
        const size_t row = ((size_t)pose * q.M + (w - 1u)) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) { A[k] = q.A[row + k]; B[k] = q.B[row + k]; }
        moved = !lrcflow::same_pose(A, B);
    }
    const lrcflow::Ray r = lrcflow::ray(live, moved, x, A, B, q.next16 + (size_t)pose * 16, q.max_range, q.min_range);
    q.flow3[gid * 3] = r.flow[0]; q.flow3[gid * 3 + 1] = r.flow[1]; q.flow3[gid * 3 + 2] = r.flow[2];
    if (!q.status) return;
    const bool cast = r.status == lrcflow::kVisible;
    q.status[gid] = r.status;
    q.keep[gid] = cast ? (uint8_t)1 : (uint8_t)0;
    if (!cast) return;
    q.thr[gid] = r.thr;
    float2* o = (float2*)(q.rays6 + gid * 6);      // 24-byte records: 8-byte aligned
    o[0] = make_float2(r.o.x, r.o.y);
    o[1] = make_float2(r.o.z, r.h.x);
    o[2] = make_float2(r.h.y, r.h.z);
}

// The ray kernel of lrc_scan_nonrigid_flow_dev: flow_rays_kernel whose mover rows look their mover up among
// the call's surface pairs (at most 16, in the kernel arguments: a wave-uniform walk of scalars) and, with a pair and prim < T,
// fetch the triangle's three indices and its three vertices in both shapes per lane.  Every other row takes the rigid step.
__global__ __launch_bounds__(kBlock) void nonrigid_target_kernel(const FlowRays q, const FlowPairs pp) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= q.total) return;
    const uint32_t pose = (uint32_t)(gid / q.rays_per_pose);
    const bool live = (q.t[gid] < __builtin_inff()) & (q.has_next == nullptr || q.has_next[pose] != 0);
    const uint32_t w = (live && q.mover) ? q.mover[gid] : 0u;
    float x[3] = {0.f, 0.f, 0.f}, A[12], B[12];
    bool moved = false, paired = false;
    if (live) {
        x[0] = q.point3[gid * 3]; x[1] = q.point3[gid * 3 + 1]; x[2] = q.point3[gid * 3 + 2];
    }
    const float* va = nullptr;
    const float* vb = nullptr;
    const uint32_t* tris = nullptr;
    uint32_t T = 0u;
    if (w != 0u && w <= q.M) {
        const size_t row = ((size_t)pose * q.M + (w - 1u)) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) { A[k] = q.A[row + k]; B[k] = q.B[row + k]; }
        moved = !lrcflow::same_pose(A, B);
#pragma unroll
        for (uint32_t k = 0; k < lrcflow::kMaxPairs; ++k)
            if (k < pp.count && pp.mover[k] == w - 1u) { va = pp.va[k]; vb = pp.vb[k]; tris = pp.tris3[k]; T = pp.T[k]; }
    }
    lrcflow::Ray r;
    if (T != 0u) {
        const uint32_t j = pp.prim[gid];
        if (j < T) {                                     // before any fetch: a miss's prim is 0xFFFFFFFF, a stale one anything
            float a9[9], b9[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t i = (size_t)tris[(size_t)j * 3 + c] * 3;
#pragma unroll
                for (int e = 0; e < 3; ++e) { a9[3 * c + e] = va[i + e]; b9[3 * c + e] = vb[i + e]; }
            }
            r = lrcflow::nonrigid_ray(x, A, B, a9, b9, q.next16 + (size_t)pose * 16, q.max_range, q.min_range);
            paired = true;
        }
    }
    if (!paired) r = lrcflow::ray(live, moved, x, A, B, q.next16 + (size_t)pose * 16, q.max_range, q.min_range);
    q.flow3[gid * 3] = r.flow[0]; q.flow3[gid * 3 + 1] = r.flow[1]; q.flow3[gid * 3 + 2] = r.flow[2];
    if (!q.status) return;
    const bool cast = r.status == lrcflow::kVisible;
    q.status[gid] = r.status;
    q.keep[gid] = cast ? (uint8_t)1 : (uint8_t)0;
    if (!cast) return;
    q.thr[gid] = r.thr;
    float2* o = (float2*)(q.rays6 + gid * 6);      // 24-byte records: 8-byte aligned
    o[0] = make_float2(r.o.x, r.o.y);
    o[1] = make_float2(r.o.z, r.h.x);
    o[2] = make_float2(r.h.y, r.h.z);
}

// A mover's pass: the world ray of every row that is cast, taken into mover q.m's frame with its NEXT pose, and the keep byte of
// the explicit-ray launch (0: not cast at all, or left out by lrcmov::culled).
__global__ __launch_bounds__(kBlock) void flow_object_rays_kernel(const float* __restrict__ world6, const uint8_t* __restrict__ cast,
                                                                 uint64_t rays_per_pose, uint64_t total, const lrcmov::RayPass q,
                                                                 int uniform, float* __restrict__ rays6, uint8_t* __restrict__ keep) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= total) return;
    const uint32_t pose = mover_pose_of(gid, rays_per_pose, uniform);
    float m12[12];
    mover_record_load<12, 12>(q.records, pose, q.M, q.m, uniform, m12);
    bool out = cast[gid] == 0;
    lrcmov::Vec ro{0.f, 0.f, 0.f}, rd{0.f, 0.f, 0.f};
    if (!out) {
        const float2* r = (const float2*)(world6 + gid * 6);
        const float2 a = r[0], b = r[1], c = r[2];
        lrcmov::to_object(m12, lrcmov::Vec{a.x, a.y, b.x}, lrcmov::Vec{b.y, c.x, c.y}, ro, rd);
        out = lrcmov::culled(q.sphere, ro, rd);
    }
    keep[gid] = out ? (uint8_t)0 : (uint8_t)1;
    if (out) return;
    float2* w = (float2*)(rays6 + gid * 6);
    w[0] = make_float2(ro.x, ro.y);
    w[1] = make_float2(ro.z, rd.x);
    w[2] = make_float2(rd.y, rd.z);
}

// The running float32 minimum of the ranges met along the line of sight (t_min holds the static cast's to begin with) against
// one mover's cast (t_mover; NULL: no mover, only the verdict).  The last pass writes the status of the rows that were cast.
__global__ __launch_bounds__(kBlock) void flow_merge_kernel(float* __restrict__ t_min, const float* __restrict__ t_mover,
                                                            const float* __restrict__ thr, const uint8_t* __restrict__ cast,
                                                            uint64_t total, int last, uint8_t* __restrict__ status) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= total) return;
    float t = t_min[gid];
    if (t_mover) t = lrcflow::nearer(t_mover[gid], t);
    if (!last) {
        t_min[gid] = t;
        return;
    }
    if (cast[gid]) status[gid] = lrcflow::judge(t, thr[gid]);
}

constexpr int kStatsWords = 5;   // node steps, triangle tests, wave-uniform node steps, dead node steps, pad-clause rejections

// ---- stable compaction, one tile (64 consecutive entries of one segment) per wave ---------------------------------------
// exclusive prefix of the super-tile totals at super tile s, formed on the spot: a wave sums at most a few hundred
// numbers, which is cheaper than the launch of a kernel that would tabulate them (compact_base_kernel)
__device__ __forceinline__ uint64_t super_prefix_wave(const uint32_t* __restrict__ total, uint64_t s, uint32_t lane) {
    uint64_t acc = 0;
    for (uint64_t j = lane; j < s; j += 64) acc += total[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    return acc;
}
__device__ __forceinline__ uint64_t super_prefix_thread(const uint32_t* __restrict__ total, uint64_t s) {
    uint64_t acc = 0;
    for (uint64_t j = 0; j < s; ++j) acc += total[j];
    return acc;
}

// one thread per segment: count = global offset of its end tile - global offset of its first tile
__device__ __forceinline__ void segment_count(const lrc_compact_io& io, uint64_t tps, uint64_t ntiles, uint64_t nseg, uint64_t sg,
                                              const uint32_t* tile_off, const uint64_t* super_base, const uint32_t* super_total) {
    if (sg >= nseg) return;
    const uint64_t nsuper = (ntiles + 1023) / 1024;
    const uint64_t g0 = sg * tps, g1 = g0 + tps;
    auto at = [&](uint64_t g) -> uint64_t {
        if (super_total) return g >= ntiles ? super_prefix_thread(super_total, nsuper)
                                            : super_prefix_thread(super_total, g >> 10) + tile_off[g];
        return g >= ntiles ? super_base[nsuper] : super_base[g >> 10] + tile_off[g];
    };
    io.counts[sg] = at(g1) - at(g0);
}

// the kept entries of tile `tile` go to their rows; called by all 64 lanes of one wave
__device__ __forceinline__ void scatter_tile(const lrc_compact_io& io, uint64_t seg_len, uint64_t tps, uint64_t tile, uint32_t lane,
                                             const uint32_t* tile_off, const uint64_t* super_base, uint64_t tile_base,
                                             const uint32_t* super_total) {
    const uint64_t seg = tile / tps, chunk = tile - seg * tps;
    const uint64_t i = chunk * 64 + lane;
    const uint64_t src = seg * seg_len + i;
    bool keep = false;
    if (i < seg_len) keep = io.t[src] < __builtin_inff();
    const unsigned long long m = __ballot(keep);
    if (m == 0ull) return;
    const uint64_t gt = tile_base + tile;
    const uint64_t sbase = super_total ? super_prefix_wave(super_total, gt >> 10, lane) : super_base[gt >> 10];
    if (!keep) return;
    const uint64_t tbase = sbase + tile_off[gt];
    const uint64_t dst = tbase + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (io.out_xyzl) {
        const float* sp = io.point3 + src * 3;
        const uint32_t lab = (io.sem ? (uint32_t)io.sem[src] : 0u) | ((io.ins ? (uint32_t)io.ins[src] : 0u) << 16);
        ((float4*)io.out_xyzl)[dst] = make_float4(sp[0], sp[1], sp[2], __uint_as_float(lab));
    }
    if (io.out_point3) {
        const float* sp = io.point3 + src * 3;
        float* q = io.out_point3 + dst * 3;
        q[0] = sp[0]; q[1] = sp[1]; q[2] = sp[2];
    }
    if (io.out_sem) io.out_sem[dst] = io.sem[src];
    if (io.out_ins) io.out_ins[dst] = io.ins[src];
    if (io.out_incident_deg) io.out_incident_deg[dst] = io.incident_deg[src];
    if (io.out_index) io.out_index[dst] = (uint32_t)i;
    if (io.out_range_origin) {
        // |p| from the WORLD origin in float32 exactly as np.linalg.norm(points, axis=1) forms it: squares, the
        // 3-element add.reduce left to right, one sqrt -- the quantity the reference's ScanQuality range statistics are
        // taken over (s3dis_simulator.py:283-284)
        const float* sp = io.point3 + src * 3;
        io.out_range_origin[dst] = __builtin_sqrtf((sp[0] * sp[0] + sp[1] * sp[1]) + sp[2] * sp[2]);
    }
}

// R consecutive tiles by one wave, packed (x, y, z, label) rows only, tiles aligned with the segments (seg_len % 64 == 0) and R
// dividing 1024 (the tiles of a call lie in one super tile).  This is the form the trace launch of the scan pipeline runs in
// its leading workgroups: a wave there holds a trace wave's registers and LDS, so few waves with many loads in flight each --
// all keep flags first, then all payloads, then the stores: two memory round trips per R tiles instead of per tile.
// super_base != NULL: the offsets are those of a scan over MORE tiles than this call's (all ranks' scans): tile t of the call is
// tile tile_base + t of that scan and its super tile's base is tabulated (compact_base_kernel); else the bases are summed here
// from the totals and the R tiles lie in one super tile.
template <int R>
__device__ __forceinline__ void scatter_tiles_xyzl(const lrc_compact_io& io, uint64_t ntiles, uint64_t tile0, uint32_t lane,
                                                   const uint32_t* tile_off, const uint32_t* super_total,
                                                   uint64_t tile_base = 0, const uint64_t* super_base = nullptr) {
    float t[R];
    uint64_t off[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t tile = tile0 + r;
        const bool valid = tile < ntiles;
        t[r] = valid ? io.t[tile * 64 + lane] : __builtin_inff();
        off[r] = valid ? (uint64_t)tile_off[tile_base + tile] : 0u;
        if (super_base && valid) off[r] += super_base[(tile_base + tile) >> 10];
    }
    const uint64_t sbase = super_base ? 0ull : super_prefix_wave(super_total, tile0 >> 10, lane);
    float px[R], py[R], pz[R];
    uint32_t lab[R];
    unsigned long long m[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool keep = t[r] < __builtin_inff();
        m[r] = __ballot(keep);
        px[r] = py[r] = pz[r] = 0.0f;
        lab[r] = 0u;
        if (keep) {
            const uint64_t src = (tile0 + r) * 64 + lane;
            const float* sp = io.point3 + src * 3;
            px[r] = sp[0]; py[r] = sp[1]; pz[r] = sp[2];
            lab[r] = (io.sem ? (uint32_t)io.sem[src] : 0u) | ((io.ins ? (uint32_t)io.ins[src] : 0u) << 16);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (t[r] < __builtin_inff()) {
            const uint64_t dst = sbase + off[r] + (uint64_t)__popcll(m[r] & ((1ull << lane) - 1ull));
            ((float4*)io.out_xyzl)[dst] = make_float4(px[r], py[r], pz[r], __uint_as_float(lab[r]));
        }
    }
}
// ---- the ray table of a prepared pipeline submit (lrc_pipe_submit; lrc_device.h ray_row) -------------
// One buffer behind TraceParams::ray_tab, for a table of N rows and P poses, in units of 16 bytes:
//   [0, 2N)        per row i two records: (d.x, d.y, d.z, 0) and (inv.x, inv.y, inv.z, 0)      -- the prologue's two loads
//   [2N, 3N)       per row i (h.x, h.y, h.z, 0)                      -- the epilogue's one load, and every record consumer's
//   [3N, 3N + 4P)  per pose p a RayPose: whether its rotation block is pose 0's bit for bit (then the rows are its rays'),
//                  its float32 origin and its float64 range-filter centre; read through the scalar cache
// All of it is rebuilt for every submit from that submit's poses and table (ray_table_kernel): nothing is keyed on an
// address, so a table edited in place or a new one at a recycled address cannot leave stale rows behind.  A pipeline holds
// one table per record set: the consumers of a set's records (LeanIn) read the table its trace read.
struct alignas(64) RayPose {
    double cx, cy, cz;
    uint32_t same;             // 1: the nine rotation doubles equal pose 0's as bit patterns (-0.0 != +0.0; a NaN equals only a NaN of the same bits)
    float ox, oy, oz;          // (the flag between the two: centre + flag are one 32-byte load, flag + origin one of 16)
    uint32_t pad[6];
};
static_assert(sizeof(RayPose) == 64, "RayPose: four 16-byte units");
// (the trace kernel derives the offsets 2N and 3N from tiles_per_pose as N = 64 * tiles_per_pose: a pipeline allocates its
// tables, and hence carries one, only in a build with kTBlock == 64 -- lrc_pipe_create)
constexpr uint64_t kRayTabMaxRows = 1ull << 24;     // rows a pipeline prepares a table for (the offsets stay in 32 bits)
__host__ __device__ inline uint64_t ray_tab_bytes(uint64_t N, uint64_t P) { return N * 48u + P * sizeof(RayPose); }

// Streaming accesses of the scan pipeline's scatter: a record of a lean record set is read once, two launches after it was
// written, and the caller's output row is written once and not read again by the library.  With non-temporal loads and stores
// the pipelined step is 3-4 % faster on every scene (profiles/pipe_fused_scatter.txt, items 4-6) -- presumably because the
// bytes no longer pass through L2 and the Infinity Cache in front of the tracing waves, which want the scene's nodes
// there.  The trace's own stores of the set stay ordinary: streaming them measured slower.  The table's h rows are NOT
// streamed: 1 MB that all poses of a submit share, and the trace of the same launch reads its own table's likewise.
typedef float nt_float4 __attribute__((ext_vector_type(4)));       // the builtins take the compiler's vector types
__device__ __forceinline__ void store_streaming(float4* q, float4 v) {
    const nt_float4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, (nt_float4*)q);
}
__device__ __forceinline__ float4 load_streaming(const float4* q) {
    const nt_float4 w = __builtin_nontemporal_load((const nt_float4*)q);
    return make_float4(w.x, w.y, w.z, w.w);
}

// The form of the tiles of pose `seg` (wave-uniform) of a lean record set, decided where the trace wave decided it: the launch
// carried a table and the pose record's flag `same` is set (trace_kernel: have_h).  One 16-byte scalar load, flag + origin.
struct LeanPose { bool rec; V3 o; };
__device__ __forceinline__ LeanPose lean_pose(const LeanIn& in, uint32_t seg_len, uint32_t seg) {
    typedef __attribute__((address_space(4))) const RayPose cpose;
    LeanPose q{false, V3{0.f, 0.f, 0.f}};
    if (in.tab != nullptr) {
        cpose* rp = (cpose*)(in.tab + (size_t)seg_len * 3u) + seg;
        q.rec = rp->same != 0u;
        q.o = V3{rp->ox, rp->oy, rp->oz};
    }
    return q;
}
// (t bits, label) of ray `ray` of the set and the unit vector of table row i, as the loads of a record-form tile
template <bool STREAMING>      // (a template argument: two loads merged behind a run-time flag lose the hint)
__device__ __forceinline__ rec2 lean_pair(const LeanIn& in, uint64_t ray) {
    const rec2* q = (const rec2*)(in.rec + ray * 3);
    if (STREAMING) return __builtin_nontemporal_load(q);
    return *q;
}
__device__ __forceinline__ V3 lean_h(const LeanIn& in, uint32_t seg_len, uint32_t i) {
    typedef float f32x3_ __attribute__((ext_vector_type(3)));
    const f32x3_ h = *(const f32x3_*)(in.tab + (size_t)seg_len * 2u + i);
    return V3{h.x, h.y, h.z};
}
__device__ __forceinline__ float4 lean_row(const LeanPose& ps, V3 h, rec2 a) {
    const PairRow r = pair_row(ps.o, h, __uint_as_float(a.x), a.y);
    return make_float4(r.x, r.y, r.z, __uint_as_float(r.label));
}

// scatter_tile from a lean record set (LeanIn): the tile's keep mask is one scalar load, a kept lane loads its record and
// the table's unit vector (or, row form, its row: one 16-byte load) and every output is a function of that row and the lane --
// the same values scatter_tile forms from the 36-byte record.  seg_len % 64 == 0 (a lean set exists only then).
__device__ __forceinline__ void scatter_tile_lean(const lrc_compact_io& io, const LeanIn& in, uint64_t seg_len, uint64_t tps,
                                                  uint64_t tile, uint32_t lane, const uint32_t* tile_off,
                                                  const uint32_t* super_total) {
    typedef __attribute__((address_space(4))) const uint64_t cu64;
    const unsigned long long m = ((cu64*)in.keep_mask)[tile];
    if (m == 0ull) return;
    const uint64_t sbase = super_prefix_wave(super_total, tile >> 10, lane);
    const uint64_t seg = tile / tps, i = (tile - seg * tps) * 64 + lane;
    const LeanPose ps = lean_pose(in, (uint32_t)seg_len, (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)seg));
    if (!((m >> lane) & 1ull)) return;
    const float4 r = ps.rec ? lean_row(ps, lean_h(in, (uint32_t)seg_len, (uint32_t)i), lean_pair<false>(in, seg * seg_len + i))
                            : in.row[seg * seg_len + i];
    const uint64_t dst = sbase + tile_off[tile] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    const uint32_t lab = __float_as_uint(r.w);
    if (io.out_xyzl) ((float4*)io.out_xyzl)[dst] = r;
    if (io.out_point3) {
        float* q = io.out_point3 + dst * 3;
        q[0] = r.x; q[1] = r.y; q[2] = r.z;
    }
    if (io.out_sem) io.out_sem[dst] = (uint16_t)(lab & 0xFFFFu);
    if (io.out_ins) io.out_ins[dst] = (uint16_t)(lab >> 16);
    if (io.out_index) io.out_index[dst] = (uint32_t)i;
    if (io.out_range_origin) io.out_range_origin[dst] = __builtin_sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z);   // as scatter_tile
}

// scatter_tiles_xyzl from a lean record set: scalar loads of the keep masks instead of per-lane t loads, then per lane 8 bytes
// of its record and the 12 of the table's unit vector -- or, row form, the 16-byte row, which IS the output row -- instead of
// five loads per kept lane.  Four tiles at a time: eight rows in flight per lane (32 registers) pushed the trace kernel, whose
// registers this wave holds, into scratch.  Four tiles of ONE pose share the form and the origin (one pose record load, one
// branch around all their loads); a group that straddles two poses (tables of fewer than four tiles, or not a multiple of
// four) goes tile by tile.  tile0 < 2^31 (the launch's grid).
template <int R>
__device__ __forceinline__ void scatter_tiles_xyzl_lean(const lrc_compact_io& io, const LeanIn& in, uint64_t ntiles, uint64_t tile0,
                                                        uint32_t lane, const uint32_t* tile_off, const uint32_t* super_total,
                                                        uint32_t seg_len, uint32_t tps) {
    typedef __attribute__((address_space(4))) const uint64_t cu64;
    typedef __attribute__((address_space(4))) const uint32_t cu32;
    constexpr int H = R < 4 ? R : 4;
    static_assert(R % H == 0, "R: a multiple of four, or below four");
    const uint64_t sbase = super_prefix_wave(super_total, tile0 >> 10, lane);
    const unsigned long long below = (1ull << lane) - 1ull;
    float4* const out = (float4*)io.out_xyzl;
    // pose and in-pose tile of the run's first tile by one division, of the others by counting (all wave-uniform)
    uint32_t seg = (uint32_t)tile0 / tps, u = (uint32_t)tile0 - seg * tps;
#pragma unroll
    for (int h = 0; h < R; h += H) {
        const uint64_t t0 = tile0 + h;
        if (u + (uint32_t)H > tps) {
            for (int r = 0; r < H; ++r) {
                const uint64_t tile = t0 + r;
                if (tile < ntiles) {
                    const unsigned long long m = ((cu64*)in.keep_mask)[tile];
                    const uint32_t off = ((cu32*)tile_off)[tile];
                    const LeanPose ps = lean_pose(in, seg_len, seg);
                    if ((m >> lane) & 1ull)
                        store_streaming(&out[sbase + off + (uint64_t)__popcll(m & below)],
                                        ps.rec ? lean_row(ps, lean_h(in, seg_len, u * 64u + lane), lean_pair<true>(in, tile * 64 + lane))
                                               : load_streaming(&in.row[tile * 64 + lane]));
                }
                if (++u == tps) { u = 0u; ++seg; }
            }
            continue;
        }
        unsigned long long m[H];
        uint32_t off[H];
#pragma unroll
        for (int r = 0; r < H; ++r) {
            const bool valid = t0 + r < ntiles;          // wave-uniform
            m[r] = valid ? ((cu64*)in.keep_mask)[t0 + r] : 0ull;
            off[r] = valid ? ((cu32*)tile_off)[t0 + r] : 0u;
        }
        // (a group wholly past the last tile may be past the last pose record too: it loads nothing)
        const LeanPose ps = t0 < ntiles ? lean_pose(in, seg_len, seg) : LeanPose{false, V3{0.f, 0.f, 0.f}};
        // every lane of a tile with a kept ray loads: coalesced reads and no divergent branch between the loads, so all of
        // them are in flight at once (what a ray that is not kept loads is never stored)
        if (ps.rec) {
            rec2 a[H];
            V3 hv[H];
#pragma unroll
            for (int r = 0; r < H; ++r) {
                a[r] = m[r] != 0ull ? lean_pair<true>(in, (t0 + r) * 64 + lane) : rec2{0u, 0u};
                hv[r] = m[r] != 0ull ? lean_h(in, seg_len, (u + r) * 64u + lane) : V3{0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int r = 0; r < H; ++r)
                if ((m[r] >> lane) & 1ull) store_streaming(&out[sbase + off[r] + (uint64_t)__popcll(m[r] & below)], lean_row(ps, hv[r], a[r]));
        } else {
            float4 row[H];
#pragma unroll
            for (int r = 0; r < H; ++r)
                row[r] = m[r] != 0ull ? load_streaming(&in.row[(t0 + r) * 64 + lane]) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int r = 0; r < H; ++r)
                if ((m[r] >> lane) & 1ull) store_streaming(&out[sbase + off[r] + (uint64_t)__popcll(m[r] & below)], row[r]);
        }
        u += (uint32_t)H;
        if (u == tps) { u = 0u; ++seg; }
    }
}
#ifndef LRC_PRE_TILES
#define LRC_PRE_TILES 8
#endif
constexpr int kPreTiles = LRC_PRE_TILES;      // tiles per leading workgroup of a pipelined trace launch (4 / 8 / 16 measured)

template <int I> struct IntTag { static constexpr int value = I; };

// The kernel that fills a ray table (its layout: RayPose, in front of the lean scatters, which read it too).  One-wave
// workgroups, like the scan pass: beside the other stream's running trace launch they are handed wave slots one by one.
// Lane-strided over the rows, then over the poses.
__global__ __launch_bounds__(64) void ray_table_kernel(const double* __restrict__ poses16, uint32_t P,
                                                       const double* __restrict__ dirs3, uint32_t N, float4* __restrict__ tab) {
    const uint32_t first = blockIdx.x * 64u + threadIdx.x, step = gridDim.x * 64u;
    const double R[9] = {poses16[0], poses16[1], poses16[2], poses16[4], poses16[5], poses16[6], poses16[8], poses16[9], poses16[10]};
    for (uint32_t i = first; i < N; i += step) {
        const double* dv = dirs3 + (size_t)i * 3;
        const RayRow r = ray_row(R, dv[0], dv[1], dv[2]);
        tab[(size_t)i * 2] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
        tab[(size_t)i * 2 + 1] = make_float4(r.inv.x, r.inv.y, r.inv.z, 0.0f);
        tab[(size_t)N * 2 + i] = make_float4(r.h.x, r.h.y, r.h.z, 0.0f);
    }
    RayPose* rp = (RayPose*)(tab + (size_t)N * 3);
    const uint64_t* B = (const uint64_t*)poses16;
    for (uint32_t q = first; q < P; q += step) {
        const double* M = poses16 + (size_t)q * 16;
        const uint64_t* A = (const uint64_t*)M;
        bool same = true;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if ((k & 3) != 3) same = same & (A[k] == B[k]);
        RayPose o{};
        o.cx = M[3]; o.cy = M[7]; o.cz = M[11];
        o.ox = (float)M[3]; o.oy = (float)M[7]; o.oz = (float)M[11];
        o.same = same ? 1u : 0u;
        rp[q] = o;
    }
}

// GEN: the ray generator, one of the names of lrc_gen.h (which also states what each implies for the launch and the tail).
// QN: 1 = walk the quantised node images (32-byte nodes for the per-lane fetches), 2 = walk their
//     four-wide collapse (64-byte nodes, half the steps); a wave with a ray outside the bound the quantisation margin is
//     proven for walks the float32 world-space nodes instead
template <int GEN, int LEAFW, bool UNI, bool SPEC, bool STATS = false, int QN = 0>
__global__ __launch_bounds__(kTBlock, gen_min_waves(GEN, QN, STATS)) void trace_kernel(const TraceParams p) {
    extern __shared__ int s_stack[];   // [stack depth][kTBlock]: one column per lane, conflict free
    constexpr bool kCentreFromMotion = gen_centre_from_motion(GEN), kDrawsNoise = gen_draws_noise(GEN);
    const uint32_t tid = threadIdx.x;
    if (GEN == kGenPoses && p.pre.blocks != 0u && p.pre.sharded != 0u) {
        if (blockIdx.x < p.pre.blocks) {
            // per-pose counts of the assembled cloud (one thread per pose of ALL ranks), then this workgroup's share
            rebuild_counts(p.pre.rq, blockIdx.x * kTBlock + tid, p.pre.blocks * kTBlock);
            if (blockIdx.x < p.pre.own_blocks) {
                const uint64_t tile0 = (uint64_t)blockIdx.x * kPreTiles;
                if (tile0 < p.pre.ntiles)
                    scatter_tiles_xyzl<kPreTiles>(p.pre.io, p.pre.ntiles, tile0, tid, p.pre.tile_off, nullptr, p.pre.tile_base,
                                                  p.pre.super_base);
            } else {
                const uint32_t tile0 = (blockIdx.x - p.pre.own_blocks) * (uint32_t)LRC_REBUILD_R;
                if (tile0 < p.pre.rq.ntiles) rebuild_tiles<LRC_REBUILD_R>(p.pre.rq, tile0, p.pre.rq.ntiles, tid);
            }
            return;
        }
    } else
    if (GEN == kGenPoses && p.pre.blocks != 0u) {          // wave-uniform; only the pose-batched scan is ever pipelined
        if (blockIdx.x < p.pre.blocks) {
            if (p.pre.io.counts) segment_count(p.pre.io, p.pre.tps, p.pre.ntiles, p.pre.nseg, (uint64_t)blockIdx.x * kTBlock + tid,
                                               p.pre.tile_off, nullptr, p.pre.super_total);
            const uint64_t tile0 = (uint64_t)blockIdx.x * kPreTiles;
            if (tile0 < p.pre.ntiles) {      // the earlier scan's records are a lean set (only fused submits ride here)
                if (p.pre.rows_only) {
                    scatter_tiles_xyzl_lean<kPreTiles>(p.pre.io, p.pre.lean, p.pre.ntiles, tile0, tid, p.pre.tile_off,
                                                       p.pre.super_total, (uint32_t)p.pre.seg_len, (uint32_t)p.pre.tps);
                } else {
                    for (int r = 0; r < kPreTiles; ++r)
                        if (tile0 + r < p.pre.ntiles)
                            scatter_tile_lean(p.pre.io, p.pre.lean, p.pre.seg_len, p.pre.tps, tile0 + r, tid, p.pre.tile_off,
                                              p.pre.super_total);
                }
            }
            return;
        }
    }
    const uint32_t tile = p.tile_chunk_log2 ? xcd_tile_chunked(blockIdx.x - p.pre.blocks, gridDim.x - p.pre.blocks, p.tile_chunk_log2)
                                            : xcd_tile(blockIdx.x - p.pre.blocks, gridDim.x - p.pre.blocks);
    const uint64_t gid = (uint64_t)tile * kTBlock + tid;
    // launch chain: workgroups are handed out in blockIdx order, so when the last one starts the launch has no workgroup
    // left to dispatch -- the next trace launch (held on another stream behind this word) may start filling the freed slots
    if (p.chain_word != nullptr && blockIdx.x == gridDim.x - 1 && tid == 0)
        __hip_atomic_store(p.chain_word, p.chain_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (gid >= p.total) return;

    // ---- the ray ----
    V3 o, d;
    V3 inv;                    // safe_inv of d per axis: formed with the ray (kGenPoses may take it from a prepared table)
    double cx, cy, cz;
    bool live = true;          // false: not cast at all (dropped by the sensor, or a non-finite ray)
    uint32_t pose32 = 0;
    if (GEN == kGenPoses) {
        uint64_t pose, i;
        if (p.tiles_per_pose != 0u) {
            // a tile lies in one pose: pose and in-pose index from the 32-bit tile number, one 32-bit division of
            // workgroup-uniform values instead of a 64-bit division per lane
            const uint32_t pu = tile / p.tiles_per_pose;
            pose = pu;
            const uint32_t u = tile - pu * p.tiles_per_pose;
            i = p.line_tiles != 0u ? tile_ray(u, tid, p.line_tiles, p.tiles_per_pose, p.line_group) : u * (uint32_t)kTBlock + tid;
        } else {
            pose = gid / p.rays_per_pose;
            i = gid - pose * p.rays_per_pose;
        }
        // prepared submit (ray_table_kernel): a wave whose pose has pose 0's rotation takes d and 1/d from the table and its
        // origin from the pose record -- no pose matrix, no float64, no division.  Wave-uniform: a tile lies in one pose.
        typedef __attribute__((address_space(4))) const RayPose cpose;
        bool prepared = false;
        if (p.tiles_per_pose != 0u && p.ray_tab != nullptr) {
            cpose* rp = (cpose*)(p.ray_tab + (size_t)p.tiles_per_pose * 192u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pose);
            // the row's records are fetched beside the pose record, not behind its flag: one round trip, and a wave that
            // falls back (a turning trajectory) merely drops them
            const uint32_t same = rp->same;
            const float ox = rp->ox, oy = rp->oy, oz = rp->oz;
            const float4 ta = p.ray_tab[(size_t)(uint32_t)i * 2], tb = p.ray_tab[(size_t)(uint32_t)i * 2 + 1];
            prepared = same != 0u;
            if (prepared) {
                o.x = ox; o.y = oy; o.z = oz;
                d.x = ta.x; d.y = ta.y; d.z = ta.z;
                inv.x = tb.x; inv.y = tb.y; inv.z = tb.z;
            } else {
                // a use on this side as well, or the compiler sinks the loads behind the flag's branch: two round trips
                asm volatile("" :: "v"(ta.x), "v"(ta.y), "v"(ta.z), "v"(tb.x), "v"(tb.y), "v"(tb.z), "s"(ox), "s"(oy), "s"(oz));
            }
        }
        if (!prepared) {
            double ux, uy, uz;      // the centre is fetched again behind the traversal
            gen_ray(p.poses16, p.dirs3, pose, i, o, d, ux, uy, uz);
            inv = V3{safe_inv(d.x), safe_inv(d.y), safe_inv(d.z)};
        }
        pose32 = (uint32_t)pose;
    } else if (GEN == kGenAngles) {
        const uint64_t pose = gid / p.rays_per_pose;
        const double2 a = ((const double2*)p.angles2)[gid];
        gen_ray_angles(p.poses16, pose, a.x, a.y, o, d, cx, cy, cz);
        if (p.keep_mask) live = p.keep_mask[gid] != 0;
        pose32 = (uint32_t)pose;
    } else if (GEN == kGenSweeps) {
        const uint64_t pose = gid / p.rays_per_pose;
        const uint64_t i = gid - pose * p.rays_per_pose;
        gen_ray_sweep(p.motion24, p.dirs3, p.fire, pose, i, o, d);
        pose32 = (uint32_t)pose;
    } else if (GEN == kGenNoisy) {
        const uint64_t pose = gid / p.rays_per_pose;
        const uint64_t i = gid - pose * p.rays_per_pose;
        gen_ray_noisy(p.poses16, p.dirs3, p.noise, pose, i, o, d, cx, cy, cz, live);
        pose32 = (uint32_t)pose;
    } else if (GEN == kGenNoisySweeps) {
        const uint64_t pose = gid / p.rays_per_pose;
        const uint64_t i = gid - pose * p.rays_per_pose;
        gen_ray_noisy_sweep(p.motion24, p.dirs3, p.fire, p.noise, pose, i, o, d, live);
        pose32 = (uint32_t)pose;
    } else if (GEN == kGenMaterials) {
        const uint64_t pose = gid / p.rays_per_pose;
        double ux, uy, uz;          // the centre is fetched again behind the traversal
        gen_ray(p.poses16, p.dirs3, pose, gid - pose * p.rays_per_pose, o, d, ux, uy, uz);
        pose32 = (uint32_t)pose;
    } else if (GEN == kGenEchoes) {
        // lane gid = beam * G + k.  64 % G == 0 and a pose is a whole number of groups, so k is the lane's place in its group of
        // the wave, no group straddles a wave, and the `gid >= total` exit above removes whole groups only.  Lanes k >= K are
        // not live: they cast nothing and take part in the reduction as sub-rays without a hit.
        const uint64_t pose = gid / p.rays_per_pose;
        const uint64_t r = gid - pose * p.rays_per_pose;
        const uint32_t k = tid & ((1u << p.echo.group_log2) - 1u);
        live = k < p.echo.subrays;
        gen_ray_beam(p.poses16, p.dirs3, p.echo.offsets2, pose, r >> p.echo.group_log2, live ? k : 0u, o, d, cx, cy, cz);
        pose32 = (uint32_t)pose;
    } else {
        const float* r = p.rays6 + gid * 6;
        o.x = r[0]; o.y = r[1]; o.z = r[2];
        d.x = r[3]; d.y = r[4]; d.z = r[5];
        if (p.keep_mask) live = p.keep_mask[gid] != 0;          // rays the sensor dropped: never cast
        if (!p.seg_offsets && p.seg_centers3) {
            // explicit rays of several poses at a FIXED stride (rays_per_pose each, dropped ones masked): pose = gid / N
            pose32 = (uint32_t)(gid / p.rays_per_pose);
        } else if (p.seg_offsets) {
            // rays of several poses back to back: find this ray's pose (largest s with off[s] <= gid)
            uint32_t lo = 0, hi = p.num_segments;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (p.seg_offsets[mid] <= gid) lo = mid; else hi = mid;
            }
            pose32 = lo;
        }
    }

    // ---- closest hit ----
    float tbest = __builtin_inff();
    uint32_t best_slot = 0xFFFFFFFFu;
    uint32_t best_prim = 0xFFFFFFFFu;   // loaded lazily, only to break exact ties
    uint32_t best_label = 0u;           // slot_label[best_slot], fetched together with the box of the deferred clause

    uint32_t st_nodes = 0, st_tris = 0, st_uni = 0, st_dead = 0, st_pad = 0;   // STATS build only (lrc_debug_scan_stats)
    live = live & finite_ray(o, d);
    if (GEN != kGenPoses) inv = V3{safe_inv(d.x), safe_inv(d.y), safe_inv(d.z)};

    // The traversal, once per node image: Q = false walks the float32 world-space nodes with the ray's world-space slab
    // constants; Q = true walks the quantised images with the slab constants in normalised coordinates.  Which boxes
    // are visited differs (the quantised boxes are a little larger), what is found does not: every box test is
    // conservative with respect to the hit definition (lrc_device.h), the closest hit is order independent.
    // qtag 0: float32 world-space nodes.  1: quantised images; all rays of the wave point into one direction octant, so
    // the plane selectors are wave-uniform and live in SGPRs.  2: the same on the four-wide collapse of the tree.
    bool redo = false;         // quantised paths: this ray must be redone on qtag 0 (its closest candidate failed the box
                               // clause, or -- qtag 2 -- its stack would not have held a step's pushes)
    auto traverse = [&](auto qtag, auto ctag) {
        constexpr int QM = decltype(qtag)::value;
        constexpr bool Q = QM != 0;
        constexpr bool INLINE_CLAUSE = decltype(ctag)::value != 0;    // the redo route tests the clause per test
        (void)INLINE_CLAUSE;
        RaySlab sl;
        uint32_t sel_nx = 0, sel_ny = 0, sel_nz = 0, sel_fx = 0, sel_fy = 0, sel_fz = 0;
        uint32_t oct = 0;     // quantised paths: the wave's direction octant (wave-uniform, SGPR)
        if (Q) {
            // normalised coordinates: n = (x - base) / W per axis, W a power of two (scaling by it is exact)
            const float ix = inv.x, iy = inv.y, iz = inv.z;
            sl.ix = ix * p.qW[0]; sl.iy = iy * p.qW[1]; sl.iz = iz * p.qW[2];
            sl.ox = ((o.x - p.qbase[0]) * p.qinvW[0]) * sl.ix;
            sl.oy = ((o.y - p.qbase[1]) * p.qinvW[1]) * sl.iy;
            sl.oz = ((o.z - p.qbase[2]) * p.qinvW[2]) * sl.iz;
            // v_perm_b32 selectors: the plane the rays enter / leave through on each axis, picked by the sign of the
            // direction (for ix > 0 fma(lo, ix, -ox) <= fma(hi, ix, -ox) by monotone rounding, so picking by sign IS
            // the min / max of slab_interval, bit for bit)
            constexpr uint32_t kLo = 0x0701000Cu, kHi = 0x0703020Cu;   // {0x40, half word, 0x00}
            oct = (uint32_t)__builtin_amdgcn_readfirstlane((int)sign_octant(d));
            sel_nx = (oct & 1u) ? kHi : kLo; sel_fx = (oct & 1u) ? kLo : kHi;
            sel_ny = (oct & 2u) ? kHi : kLo; sel_fy = (oct & 2u) ? kLo : kHi;
            sel_nz = (oct & 4u) ? kHi : kLo; sel_fz = (oct & 4u) ? kLo : kHi;
        } else if (INLINE_CLAUSE) {
            // the redo route forms 1/d again, from a copy of d the compiler cannot connect with the prologue's: neither `inv` nor
            // an intermediate of safe_inv is held through the first traversal (they were spilled to scratch)
            V3 dd = d;
            asm volatile("" : "+v"(dd.x), "+v"(dd.y), "+v"(dd.z));
            sl = make_slab(o, dd);
        } else {
            sl.ix = inv.x; sl.iy = inv.y; sl.iz = inv.z;      // make_slab with safe_inv already taken
            sl.ox = o.x * sl.ix; sl.oy = o.y * sl.iy; sl.oz = o.z * sl.iz;
        }
        int sp = 0;
        int ref = 0;   // root
        // descend into the nearer hit child, push the other; nothing hit -> pop, or (stack empty) continue with the
        // empty leaf so that the outer loop ends
        auto choose = [&](float n0, float f0, float n1, float f1, int r0, int r1) {
            if (STATS) st_nodes += 1u;
            const bool h0 = (n0 <= f0) & (n0 <= tbest);
            const bool h1 = (n1 <= f1) & (n1 <= tbest);
            if (h0 & h1) {
                const bool first0 = n0 <= n1;
                s_stack[sp * kTBlock + tid] = first0 ? r1 : r0;
                ++sp;
                ref = first0 ? r0 : r1;
            } else if (h0) {
                ref = r0;
            } else if (h1) {
                ref = r1;
            } else if (sp == 0) {
                if (STATS) st_dead += 1u;
                ref = ~0;   // empty leaf
            } else {
                if (STATS) st_dead += 1u;
                --sp;
                ref = s_stack[sp * kTBlock + tid];
            }
        };
        // one inner-node step on a float32 node (world space, or the normalised image on the scalar path)
        auto step = [&](const F4 q0, const F4 q1, const F4 q2, const F4 q3) {
            float n0, f0, n1, f1;
            slab_interval(sl, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, n0, f0);
            slab_interval(sl, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, n1, f1);
            choose(n0, f0, n1, f1, __float_as_int(q3.x), __float_as_int(q3.y));
        };
        // the same on a wave-uniform node (SGPRs).  Quantised path: the normalised image, entry / exit planes picked by
        // the wave's octant with scalar selects (slab_interval2_oct: slab_interval's bits, twelve vector min / max less)
        auto step_u = [&](const F4 q0, const F4 q1, const F4 q2, const F4 q3) {
            if (QM == 1) {
                const float c0[6] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y}, c1[6] = {q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
                float n0, f0, n1, f1;
                slab_interval2_oct(sl, oct, c0, c1, n0, f0, n1, f1);
                choose(n0, f0, n1, f1, __float_as_int(q3.x), __float_as_int(q3.y));
            } else {
                step(q0, q1, q2, q3);
            }
        };
        // one inner-node step on a 32-byte quantised node: per child (lo|hi << 16) x, y, z and the reference
        auto step_q = [&](const uint4 a, const uint4 b) {
            auto plane = [](uint32_t w, uint32_t sel) { return __uint_as_float(__builtin_amdgcn_perm(0x40000000u, w, sel)); };
            auto interval = [&](const uint4 c, float& tn, float& tf) {
                const float nx = fma_(plane(c.x, sel_nx), sl.ix, -sl.ox), fx = fma_(plane(c.x, sel_fx), sl.ix, -sl.ox);
                const float ny = fma_(plane(c.y, sel_ny), sl.iy, -sl.oy), fy = fma_(plane(c.y, sel_fy), sl.iy, -sl.oy);
                const float nz = fma_(plane(c.z, sel_nz), sl.iz, -sl.oz), fz = fma_(plane(c.z, sel_fz), sl.iz, -sl.oz);
                const float n = max2(max2(nx, ny), max2(nz, 0.0f));
                const float f = min2(min2(fx, fy), fz);
                tn = fma_(n, kPadRelLo, -kPadAbs);
                tf = fma_(f, kPadRelHi, kPadAbs);
            };
            float n0, f0, n1, f1;
            interval(a, n0, f0);
            interval(b, n1, f1);
            choose(n0, f0, n1, f1, (int)a.w, (int)b.w);
        };
#ifdef LRC_VARIANTS
        // four-wide step: descend into the nearest hit child, push the other hit children; nothing hit -> pop
        auto choose4 = [&](float t0, float f0, float t1, float f1, float t2, float f2, float t3, float f3,
                           int r0, int r1, int r2, int r3) {
            if (STATS) st_nodes += 1u;
            const bool h0 = (t0 <= f0) & (t0 <= tbest), h1 = (t1 <= f1) & (t1 <= tbest);
            const bool h2 = (t2 <= f2) & (t2 <= tbest), h3 = (t3 <= f3) & (t3 <= tbest);
            const float inf = __builtin_inff();
            const float d0 = h0 ? t0 : inf, d1 = h1 ? t1 : inf, d2 = h2 ? t2 : inf, d3 = h3 ? t3 : inf;
            const float dm = min2(min2(d0, d1), min2(d2, d3));
            if (dm < inf) {
                if (sp + 3 > (int)p.stack_cap) {      // cannot happen on a tree whose depth the stack was sized for
                    redo = true; ref = ~0; sp = 0;    // ... unless three children stay pending level after level
                } else {
                    const int near = d0 == dm ? 0 : d1 == dm ? 1 : d2 == dm ? 2 : 3;
                    if (h3 & (near != 3)) { s_stack[sp * kTBlock + tid] = r3; ++sp; }
                    if (h2 & (near != 2)) { s_stack[sp * kTBlock + tid] = r2; ++sp; }
                    if (h1 & (near != 1)) { s_stack[sp * kTBlock + tid] = r1; ++sp; }
                    if (h0 & (near != 0)) { s_stack[sp * kTBlock + tid] = r0; ++sp; }
                    ref = near == 0 ? r0 : near == 1 ? r1 : near == 2 ? r2 : r3;
                }
            } else if (sp == 0) {
                if (STATS) st_dead += 1u;
                ref = ~0;
            } else {
                if (STATS) st_dead += 1u;
                --sp;
                ref = s_stack[sp * kTBlock + tid];
            }
        };
        auto step_q4 = [&](const uint4 a, const uint4 b, const uint4 c, const uint4 e) {
            auto plane = [](uint32_t w, uint32_t sel) { return __uint_as_float(__builtin_amdgcn_perm(0x40000000u, w, sel)); };
            auto interval = [&](const uint4 k, float& tn, float& tf) {
                const float nx = fma_(plane(k.x, sel_nx), sl.ix, -sl.ox), fx = fma_(plane(k.x, sel_fx), sl.ix, -sl.ox);
                const float ny = fma_(plane(k.y, sel_ny), sl.iy, -sl.oy), fy = fma_(plane(k.y, sel_fy), sl.iy, -sl.oy);
                const float nz = fma_(plane(k.z, sel_nz), sl.iz, -sl.oz), fz = fma_(plane(k.z, sel_fz), sl.iz, -sl.oz);
                const float n = max2(max2(nx, ny), max2(nz, 0.0f));
                const float f = min2(min2(fx, fy), fz);
                tn = fma_(n, kPadRelLo, -kPadAbs);
                tf = fma_(f, kPadRelHi, kPadAbs);
            };
            float t0, f0, t1, f1, t2, f2, t3, f3;
            interval(a, t0, f0); interval(b, t1, f1); interval(c, t2, f2); interval(e, t3, f3);
            choose4(t0, f0, t1, f1, t2, f2, t3, f3, (int)a.w, (int)b.w, (int)c.w, (int)e.w);
        };
        // the same on a wave-uniform node of the normalised float32 image (128 B: per child lo, hi, reference, pad)
        auto step_n4 = [&](const F4 a0, const F4 a1, const F4 b0, const F4 b1, const F4 c0, const F4 c1, const F4 e0,
                           const F4 e1) {
            float t0, f0, t1, f1, t2, f2, t3, f3;
            slab_interval(sl, a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, t0, f0);
            slab_interval(sl, b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, t1, f1);
            slab_interval(sl, c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, t2, f2);
            slab_interval(sl, e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, t3, f3);
            choose4(t0, f0, t1, f1, t2, f2, t3, f3, __float_as_int(a1.z), __float_as_int(b1.z), __float_as_int(c1.z),
                    __float_as_int(e1.z));
        };
#endif
        // one leaf: test its 1..4 triangles, keep the lexicographically smallest (t, triangle row)
        auto leaf = [&](const int lref) {
            const uint32_t enc = (uint32_t)(~lref);
            const uint32_t first = enc >> 3, cnt = enc & 7u;
            // LEAFW records are fetched at once (one memory round trip per LEAFW triangles);
            // the triangle array is padded so that reading past a short leaf stays in bounds
            for (uint32_t k0 = 0; k0 < cnt; k0 += LEAFW) {
                float4 ra[LEAFW], rb[LEAFW], rc[LEAFW];
#pragma unroll
                for (int j = 0; j < LEAFW; ++j) {
                    const float4* tr = p.tris + (size_t)(first + k0 + j) * 3;
#ifdef LRC_TRI36
                    // A/B only (profiles/r04_trace_levers.txt): 36 of the record's 48 bytes come back, Ng = cross(e2, e1) is
                    // formed again (the builder's own expression: same bits) -- one dwordx4 return per test for six VALU
                    ra[j] = tr[0]; rb[j] = tr[1]; rc[j].x = ((const float*)tr)[8];
#else
                    ra[j] = tr[0]; rb[j] = tr[1]; rc[j] = tr[2];
#endif
                }
#pragma unroll
                for (int j = 0; j < LEAFW; ++j) {
                    if (k0 + j < cnt) {
                        if (STATS) st_tris += 1u;
                        const uint32_t slot = first + k0 + j;
                        const float4 a = ra[j], b = rb[j], c = rc[j];
#ifdef LRC_TRI36
                        const V3 v0{a.x, a.y, a.z}, v1{a.w, b.x, b.y}, v2{b.z, b.w, c.x}, ng = cross3(v2, v1);
#else
                        const V3 v0{a.x, a.y, a.z}, v1{a.w, b.x, b.y}, v2{b.z, b.w, c.x}, ng{c.y, c.z, c.w};
#endif
                        float t;
                        bool hit;
                        // edge records (v0, e1, e2, Ng): v1 / v2 above ARE e1 / e2.  Candidates are ranked by the
                        // Moeller-Trumbore conditions on every node image; the box clause is tested once, after the
                        // traversal (below), and inline only on the redo route (INLINE_CLAUSE, float32 nodes).
                        hit = tri_mt(o, d, v0, v1, v2, ng, t);
                        if (INLINE_CLAUSE) {
                            if (hit) {
                                const float* bx = p.slot_box + (size_t)slot * 6;
                                hit = box_clause(sl, bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], t);
                                if (STATS) { if (!hit) st_pad += 1u; }
                            }
                        }
                        if (hit) {
                            if (t < tbest) {
                                tbest = t; best_slot = slot; best_prim = 0xFFFFFFFFu;
                            } else if (t == tbest) {
                                if (best_prim == 0xFFFFFFFFu) best_prim = p.slot_prim[best_slot];
                                const uint32_t pr = p.slot_prim[slot];
                                if (pr < best_prim) { best_slot = slot; best_prim = pr; }
                            }
                        }
                    }
                }
            }
        };
        auto fetch_step = [&]() {         // per-lane fetch of node `ref`
#ifdef LRC_VARIANTS
            if (QM == 2) {
                const uint4* n = p.nodes_q4 + (size_t)ref * 4;
                step_q4(n[0], n[1], n[2], n[3]);
            } else
#endif
            if (Q) {
                const uint4* n = p.nodes_q + (size_t)ref * 2;
                step_q(n[0], n[1]);
            } else {
                const F4* n = (const F4*)(p.nodes + (size_t)ref * 4);
                step(n[0], n[1], n[2], n[3]);
            }
        };
        while (true) {
            // descend inner nodes
            int pending = ~0;   // SPEC: one postponed leaf (empty = ~0)
            while (ref >= 0) {
                if (UNI) {
                    // Neighbouring rays walk the top of the tree in lock step.  When every active lane
                    // of the wave wants the same node, fetch it once through the scalar cache into
                    // SGPRs (s_load) instead of 64 identical vector loads through the L1.
                    const int uref = __builtin_amdgcn_readfirstlane(ref);
                    if (__builtin_amdgcn_ballot_w64(ref != uref) == 0ull) {
                        if (STATS) st_uni += 1u;
#ifdef LRC_VARIANTS
                        if (QM == 2) {
                            const float4* n = p.nodes_n4 + (size_t)uref * 8;
                            step_n4(ld_uniform(n), ld_uniform(n + 1), ld_uniform(n + 2), ld_uniform(n + 3),
                                    ld_uniform(n + 4), ld_uniform(n + 5), ld_uniform(n + 6), ld_uniform(n + 7));
                        } else
#endif
                        {
                            const float4* n = (Q ? p.nodes_n : p.nodes) + (size_t)uref * 4;
                            step_u(ld_uniform(n), ld_uniform(n + 1), ld_uniform(n + 2), ld_uniform(n + 3));
                        }
                    } else {
                        fetch_step();
                    }
                } else {
                    fetch_step();
                }
                if (SPEC) {
                    // speculative traversal: park the first leaf and keep descending from the stack, so
                    // that this lane stays busy while its neighbours are still in inner nodes
                    if ((ref < 0) & (ref != ~0) & (pending == ~0) & (sp > 0)) {
                        pending = ref;
                        --sp;
                        ref = s_stack[sp * kTBlock + tid];
                    }
                }
            }
            if (SPEC) leaf(pending);
            leaf(ref);
            if (sp == 0) break;
            --sp;
            ref = s_stack[sp * kTBlock + tid];
        }
        if (!INLINE_CLAUSE) {
            if (best_slot != 0xFFFFFFFFu) {       // the box clause of the closest candidate, in world coordinates
                const float* bx = p.slot_box + (size_t)best_slot * 6;
                // the label the write-back needs has the same index: issued here, it comes back with the box instead of
                // costing a second dependent round trip after the redo ballot (unused if the ray is dropped or redone)
                best_label = p.slot_label[best_slot];
                RaySlab w = sl;
                if (Q) {        // ix = ix' / W exactly (W a power of two); ox = o * ix as make_slab forms it
                    w.ix = sl.ix * p.qinvW[0]; w.iy = sl.iy * p.qinvW[1]; w.iz = sl.iz * p.qinvW[2];
                    w.ox = o.x * w.ix; w.oy = o.y * w.iy; w.oz = o.z * w.iz;
                }
                if (!box_clause(w, bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], tbest)) {
                    redo = true;
                    if (STATS) st_pad += 1u;
                }
            }
#ifdef LRC_VARIANTS
            if (p.force_redo) redo |= (((uint64_t)blockIdx.x * kTBlock + tid) % p.force_redo) == 0;   // test hook (LRC_DEBUG_FORCE_REDO=m)
#endif
        }
    };
    using FirstPass = IntTag<0>;      // edge records: every first pass defers the box clause
    if (p.num_nodes) {
        if (QN) {
            // outside this bound the margin of the quantised boxes is not proven to cover the difference
            // between the two slab arithmetics: such a wave walks the float32 nodes
            auto far1 = [](float oa, float da, float base, float W) {
                return !(__builtin_fabsf(oa - base) <= lrc::kQnodeNearBase * W) | !(__builtin_fabsf(oa) <= lrc::kQnodeNearOrigin * W) |
                       !(__builtin_fabsf(da) <= 0x1p60f);
            };
            const bool far = live & (far1(o.x, d.x, p.qbase[0], p.qW[0]) | far1(o.y, d.y, p.qbase[1], p.qW[1]) |
                                     far1(o.z, d.z, p.qbase[2], p.qW[2]));
            const uint32_t oct = sign_octant(d);
            // octant of the first ACTIVE lane (which may be a ray that is not cast: the wave then merely takes the float32
            // nodes; results do not depend on the choice)
            const uint32_t oct0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)oct);
            // a wave whose rays point into different octants (it straddles an axis direction) walks the float32 nodes too
            if (__builtin_amdgcn_ballot_w64(far | (live & (oct != oct0))) != 0ull) { if (live) traverse(IntTag<0>{}, FirstPass{}); }
            else if (live) {
#ifdef LRC_VARIANTS
                if (QN == 2) traverse(IntTag<2>{}, IntTag<0>{});
                else
#endif
                traverse(IntTag<1>{}, IntTag<0>{});
            }
        } else if (live) {
            traverse(IntTag<0>{}, FirstPass{});
        }
        // a ray whose closest candidate failed the box clause (or, four-wide nodes, whose stack was too short) is redone
        // on the float32 nodes with the clause tested per triangle
        if (__builtin_amdgcn_ballot_w64(redo) != 0ull) {
            if (redo) {
                tbest = __builtin_inff(); best_slot = 0xFFFFFFFFu; best_prim = 0xFFFFFFFFu;
                traverse(IntTag<0>{}, IntTag<1>{});
            }
            // every lane of such a wave loads its label again: the one fetched with the box is not held through the redo
            // traversal, which has no register for it
            best_label = best_slot != 0xFFFFFFFFu ? p.slot_label[best_slot] : 0u;
        }
    }

    // ---- fused write-back ----
    // prepared submit (kGenPoses with a ray table): flag and float64 centre come from the pose record again (scalar loads) and the
    // row's unit direction from the table, in the place of the per-lane fetch of the pose's translation.  Pointer and divisor
    // are made opaque so that nothing of the prologue (the division's reciprocal) is held through the traversal.
    const float4* tab = nullptr;
    uint32_t tpp = 0u;
    if (GEN == kGenPoses) {
        tab = p.ray_tab; tpp = p.tiles_per_pose;
        asm volatile("" : "+s"(tab));
        asm volatile("" : "+s"(tpp));
    }
    const bool tabbed = GEN == kGenPoses && tpp != 0u && tab != nullptr;      // a kernel argument: uniform over the launch
    if (GEN != kGenRays && !kCentreFromMotion && !tabbed) {
        // the range-filter centre (the pose's translation, float64) is fetched again here instead of being held in six
        // registers through the traversal; the pointer is made opaque so that the fetch is not merged with gen_ray's
        const double* M = p.poses16;
        asm volatile("" : "+s"(M));
        M += (size_t)pose32 * 16;
        cx = M[3]; cy = M[7]; cz = M[11];
    } else if (GEN != kGenRays) {
        // formed below: kGenSweeps and kGenNoisySweeps from the record and the firing fraction, a prepared submit from its pose record
    } else if (p.seg_centers3) {
        const double* c = p.seg_centers3 + (size_t)pose32 * 3;      // the centre of this ray's pose (segment)
        cx = c[0]; cy = c[1]; cz = c[2];
    } else if (p.has_center) { cx = p.cx; cy = p.cy; cz = p.cz; }
    else { cx = (double)o.x; cy = (double)o.y; cz = (double)o.z; }
    // the ray's index is formed again from the workgroup number (scalar arithmetic) instead of being carried through the
    // traversal in two registers the kernel does not have (the compiler spilled them to scratch: 8 B per ray each way);
    // the workgroup number is made opaque so that the two computations are not merged
    uint32_t wg = blockIdx.x;
    asm volatile("" : "+s"(wg));
    const uint32_t tile_w = p.tile_chunk_log2 ? xcd_tile_chunked(wg - p.pre.blocks, gridDim.x - p.pre.blocks, p.tile_chunk_log2)
                                              : xcd_tile(wg - p.pre.blocks, gridDim.x - p.pre.blocks);
    uint64_t gid_w = (uint64_t)tile_w * kTBlock + tid;
    uint32_t pu_w = 0u;
    if (GEN == kGenPoses && tpp != 0u && (p.line_tiles != 0u || tabbed)) pu_w = tile_w / tpp;
    if (GEN == kGenPoses && tpp != 0u && p.line_tiles != 0u)      // line-group tile: the same mapping as in front of the traversal
        gid_w = (uint64_t)pu_w * p.rays_per_pose + tile_ray(tile_w - pu_w * tpp, tid, p.line_tiles, tpp, p.line_group);
    bool have_h = false;
    V3 h_tab{0.f, 0.f, 0.f};
    if (tabbed) {
        typedef __attribute__((address_space(4))) const RayPose cpose;
        cpose* rp = (cpose*)(tab + (size_t)tpp * 192u) + pu_w;
        // record and row are fetched side by side (one round trip); a wave that falls back drops the row
        const uint32_t same = rp->same;
        const double rx = rp->cx, ry = rp->cy, rz = rp->cz;
        typedef __attribute__((address_space(1))) const nt_float4 gfloat4;      // a global load: the opaque pointer lost its address space
        const nt_float4 th = ((gfloat4*)tab)[(size_t)tpp * 128u + ((uint32_t)gid_w - pu_w * (uint32_t)p.rays_per_pose)];
        have_h = same != 0u;
        if (have_h) {
            h_tab.x = th.x; h_tab.y = th.y; h_tab.z = th.z;
            cx = rx; cy = ry; cz = rz;
        } else {
            asm volatile("" :: "v"(th.x), "v"(th.y), "v"(th.z), "s"(rx), "s"(ry), "s"(rz));      // keeps the loads in front of the branch
            const double* M = p.poses16;      // as above
            asm volatile("" : "+s"(M));
            M += (size_t)pose32 * 16;
            cx = M[3]; cy = M[7]; cz = M[11];
        }
    }
    if (kCentreFromMotion) {
        // the range-filter centre c(s), float64, formed again from the record and fire[i] (as kGenPoses fetches the pose's
        // translation again) instead of being held through the traversal; opaque pointers keep the loads from merging
        const double* M = p.motion24;
        const double* F = p.fire;
        asm volatile("" : "+s"(M));
        asm volatile("" : "+s"(F));
        M += (size_t)pose32 * 24;
        sweep_centre(M, F[gid_w - (uint64_t)pose32 * p.rays_per_pose], cx, cy, cz);
    }
    if (kDrawsNoise && p.noise.range_std != 0.0f && best_slot != 0xFFFFFFFFu) {
        // the range draw: the ray's Philox block is formed again here instead of z0 being held through the traversal; a
        // non-positive range is no return
        tbest = noisy_range(p.noise, p.noise.first_frame + pose32, (uint32_t)(gid_w - (uint64_t)pose32 * p.rays_per_pose), tbest);
        if (!(tbest > 0.0f)) best_slot = 0xFFFFFFFFu;
    }
    if (GEN == kGenEchoes) {
        // the beam's K closest hits -> at most E echoes, across the G lanes of the group.  Every lane of the wave is here: no
        // lane has left since the `gid >= total` exit, which takes whole groups.  The record is the AXIS ray's: gen_ray's bits
        // of the unjittered row (the origin is every sub-ray's)
        lrcecho::reduce_lanes(p.echo, tid, gid_w, tbest, best_slot, best_label,
                              [&](uint64_t beam, uint64_t rec, float t_e, uint32_t slot_e, uint32_t label_e) {
            const double* M = p.poses16;
            asm volatile("" : "+s"(M));
            double ux, uy, uz;
            gen_ray(M, p.dirs3, pose32, beam - (uint64_t)pose32 * (p.rays_per_pose >> p.echo.group_log2), o, d, ux, uy, uz);
            write_back<true, false, true>(p, rec, tid, o, d, cx, cy, cz, t_e, slot_e, label_e, false, h_tab);
        });
        return;
    }
    if (GEN == kGenMaterials) {
        // the chain of segments behind the first traversal.  The record is the ORIGINAL ray's at the total path length:
        // gen_ray's bits again, not held through the loop.  A wave none of whose lanes took the step still has it in (o, d), the
        // registers of the current segment: nothing to form.
        lrcmat::chain_lanes(p, gid_w, o, d, tbest, best_slot, best_label,
                            [&](uint32_t slot, float& nx, float& ny, float& nz) { slot_normal(p.tris[(size_t)slot * 3 + 2], nx, ny, nz); },
                            [&] { best_prim = 0xFFFFFFFFu; traverse(IntTag<0>{}, IntTag<1>{}); },
                            [&](bool touched, float T, uint32_t slot, uint32_t label, float I) {
            if (__builtin_amdgcn_ballot_w64(touched) != 0ull) {
                const double* M = p.poses16;
                asm volatile("" : "+s"(M));
                double ux, uy, uz;
                gen_ray(M, p.dirs3, pose32, gid_w - (uint64_t)pose32 * p.rays_per_pose, o, d, ux, uy, uz);
            }
            return write_back<true, false, true, true>(p, gid_w, tid, o, d, cx, cy, cz, T, slot, label, false, h_tab, I);
        });
        return;
    }
    write_back<GEN != kGenRays, false, true>(p, gid_w, tid, o, d, cx, cy, cz, tbest, best_slot, best_label, have_h, h_tab);
    if (STATS) {
        if (p.stats) {
            uint32_t* q = p.stats + gid_w * kStatsWords;
            q[0] = st_nodes; q[1] = st_tris; q[2] = st_uni; q[3] = st_dead; q[4] = st_pad;
        }
    }

}

#include "lrc_stats.h"

// ---- compaction -------------------------------------------------------------------------------
// tile = 64 consecutive entries of one segment = one wave; tile index = seg * tps + chunk.

__global__ __launch_bounds__(kBlock) void compact_count_kernel(const float* t, uint64_t seg_len,
                                                               uint64_t tps, uint64_t ntiles,
                                                               uint32_t* tile_cnt) {
    const uint64_t tile = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const uint64_t seg = tile / tps, chunk = tile - seg * tps;
    const uint64_t i = chunk * 64 + (threadIdx.x & 63u);
    bool keep = false;
    if (i < seg_len) keep = t[seg * seg_len + i] < __builtin_inff();
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) tile_cnt[tile] = (uint32_t)__popcll(m);
}

// Pass A: one WAVE scans a run of 1024 tile counts (a "super tile" = 65536 entries):
// tile_off[tile] = exclusive offset inside the super tile, super_total[b] = its sum.
// The counts may sit in slabs (the gathered send buffers of several ranks): tiles_per_slab consecutive tiles, then the
// next slab slab_stride words further on; a plain array is one slab.
// One-wave workgroups on purpose: this kernel runs beside the trace launch of the caller's other stream, which takes every
// wave slot the moment it is freed.  As a 1024-thread workgroup (16 waves that must start together on ONE CU) the scan
// was not scheduled until that launch had no workgroup left -- 150-170 us for a 5 us kernel, and with it the whole chain
// trace -> scan -> scatter -> next trace fell into phase with the other stream's (profiles/r04_chain_timeline.txt).
constexpr int kScanRows = 16;           // 64 lanes x 16 rows = 1024 tiles per wave and super tile
// MASKS: tile_cnt is an array of 64-bit keep masks (one slab), a tile's count the popcount of its mask, written to cnt_out too
template <bool MASKS = false>
__device__ __forceinline__ void scan_super_tiles(const uint32_t* tile_cnt, uint64_t tiles_per_slab, uint64_t slab_stride,
                                                 uint32_t* tile_off, uint64_t ntiles, uint32_t* super_total,
                                                 uint32_t* cnt_out = nullptr) {
    const uint32_t lane = threadIdx.x;
    const uint64_t nsuper = (ntiles + 1023) / 1024;
    const bool one_slab = tiles_per_slab >= ntiles;          // a plain array: no slab arithmetic (a 64-bit division per entry)
    // grid-stride over the super tiles: the scan pipeline launches FEW waves on purpose (each must find a free wave slot
    // beside a running trace launch, and they arrive at a trickle), stand-alone callers one wave per super tile
    for (uint64_t sup = blockIdx.x; sup < nsuper; sup += gridDim.x) {
        const uint64_t first = sup * 1024;
        uint32_t c[kScanRows];
#pragma unroll
        for (int r = 0; r < kScanRows; ++r) {          // all loads first (coalesced rows of 64), then the arithmetic
            const uint64_t tile = first + (uint64_t)r * 64 + lane;
            c[r] = 0u;
            if (tile < ntiles) {
                uint64_t idx = tile;
                if (!one_slab) {
                    const uint64_t sb = tile / tiles_per_slab;
                    idx = sb * slab_stride + (tile - sb * tiles_per_slab);
                }
                if (MASKS) {
                    c[r] = (uint32_t)__popcll(((const unsigned long long*)tile_cnt)[tile]);
                    cnt_out[tile] = c[r];
                } else {
                    c[r] = tile_cnt[idx];
                }
            }
        }
        uint32_t carry = 0u;
#pragma unroll
        for (int r = 0; r < kScanRows; ++r) {
            uint32_t incl = c[r];                     // inclusive scan of the row inside the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, 64);
                if (lane >= (uint32_t)d) incl += up;
            }
            const uint64_t tile = first + (uint64_t)r * 64 + lane;
            if (tile < ntiles) tile_off[tile] = carry + incl - c[r];
            carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        if (lane == 0) super_total[sup] = carry;
    }
}
__global__ __launch_bounds__(64) void compact_scan_kernel(const uint32_t* tile_cnt, uint64_t tiles_per_slab,
                                                          uint64_t slab_stride, uint32_t* tile_off,
                                                          uint64_t ntiles, uint32_t* super_total) {
    scan_super_tiles(tile_cnt, tiles_per_slab, slab_stride, tile_off, ntiles, super_total);
}
// Length of the first run of equal z in a direction table of n rows: the scan line width of a sensor whose table is laid
// out line by line at constant elevation (lrc_pipe_submit, automatic line width).  One wave, once per table.
__global__ __launch_bounds__(64) void first_line_kernel(const double* __restrict__ dirs3, uint64_t n, uint32_t* out) {
    const uint32_t lane = threadIdx.x;
    const double z0 = dirs3[2];
    uint64_t w = n;
    for (uint64_t base = 0; base < n; base += 64) {
        const uint64_t i = base + lane;
        const unsigned long long m = __ballot(i < n && dirs3[i * 3 + 2] != z0);
        if (m != 0ull) { w = base + (uint64_t)__builtin_ctzll(m); break; }
    }
    // out[1]: the first line (of w rays) whose z has another sign than line 0's -- the split of the line groups (lrc_device.h,
    // tile_ray); the number of whole lines if there is none
    const uint64_t h = w != 0 ? n / w : 0;
    uint64_t sp = h;
    for (uint64_t base = 0; base < h; base += 64) {
        const uint64_t j = base + lane;
        const unsigned long long m = __ballot(j < h && (dirs3[j * w * 3 + 2] < 0.0) != (z0 < 0.0));
        if (m != 0ull) { sp = base + (uint64_t)__builtin_ctzll(m); break; }
    }
    if (lane == 0) {
        out[0] = w > 0xFFFFFFFFull ? 0u : (uint32_t)w;
        out[1] = sp > 0x7FFFFFFFull ? 0u : (uint32_t)sp;
    }
}

// the scan pass of a lean record set (lrc_pipe_submit): the counts are the popcounts of the tiles' keep masks -- the tracing
// waves of a line-group tile each hold halves or quarters of several tiles and write no counts -- and go to tile_cnt_out as a by-product (what
// lrc_pipe_records hands out as lrc_hits.tile_count)
__global__ __launch_bounds__(64) void compact_scan_masks_kernel(const uint64_t* keep_mask, uint32_t* tile_cnt_out, uint32_t* tile_off,
                                                                uint64_t ntiles, uint32_t* super_total) {
    scan_super_tiles<true>((const uint32_t*)keep_mask, ntiles, 0, tile_off, ntiles, super_total, tile_cnt_out);
}
// the same scan over the gathered counts of all ranks (lrc_pipe_scan_gathered), and in the same waves the direction table
// (N,3) -> x[N] y[N] z[N] for the rebuild (as dirs_transpose_kernel): one kernel less to find wave slots for beside a running
// trace launch
__global__ __launch_bounds__(64) void gathered_scan_kernel(const uint32_t* tile_cnt, uint64_t tiles_per_slab,
                                                           uint64_t slab_stride, uint32_t* tile_off, uint64_t ntiles,
                                                           uint32_t* super_total, const double* __restrict__ dirs3, uint32_t n,
                                                           double* __restrict__ soa) {
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u) {
        soa[i] = dirs3[(size_t)i * 3];
        soa[(size_t)n + i] = dirs3[(size_t)i * 3 + 1];
        soa[2 * (size_t)n + i] = dirs3[(size_t)i * 3 + 2];
    }
    scan_super_tiles(tile_cnt, tiles_per_slab, slab_stride, tile_off, ntiles, super_total);
}

// Pass A2: one wave turns the super-tile totals into exclusive bases (base[nsuper] = grand total).  One wave for the same
// reason as above: a 1024-thread workgroup waits for sixteen free wave slots on one CU while a trace launch is running.
__global__ __launch_bounds__(64) void compact_base_kernel(const uint32_t* super_total, uint64_t* super_base,
                                                          uint64_t nsuper) {
    const uint32_t lane = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nsuper; base += 64) {
        const uint64_t i = base + lane;
        const uint64_t v = i < nsuper ? super_total[i] : 0;
        uint64_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t up = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (i < nsuper) super_base[i] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) super_base[nsuper] = carry;
}

// Pass B: scatter the kept entries; the first workgroups also write the per-segment counts (scatter_tile / segment_count,
// defined in front of the trace kernel, which runs them too: TraceParams::pre).
// tile_base: index of this call's tile 0 in tile_off / super_base (non-zero when the offsets come from a scan over the
// tiles of several ranks and this call scatters one rank's records into the assembled cloud).
// super_total != NULL: the bases of the super tiles are summed here from the totals (super_base is not read).
__global__ __launch_bounds__(kBlock) void compact_scatter_kernel(const lrc_compact_io io,
                                                                 uint64_t seg_len, uint64_t tps,
                                                                 uint64_t ntiles, uint64_t nseg,
                                                                 const uint32_t* tile_off,
                                                                 const uint64_t* super_base, uint64_t tile_base,
                                                                 const uint32_t* super_total) {
    if (io.counts) segment_count(io, tps, ntiles, nseg, (uint64_t)blockIdx.x * kBlock + threadIdx.x, tile_off, super_base, super_total);
    const uint64_t tile = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    scatter_tile(io, seg_len, tps, tile, threadIdx.x & 63u, tile_off, super_base, tile_base, super_total);
}

// Pass B of the scan pipeline's plain form (lrc_pipe_wait) for a lean record set: as compact_scatter_kernel, tile_base = 0 and
// the super tile bases summed from the totals
__global__ __launch_bounds__(kBlock) void compact_scatter_lean_kernel(const lrc_compact_io io, const LeanIn in,
                                                                      uint64_t seg_len, uint64_t tps,
                                                                      uint64_t ntiles, uint64_t nseg,
                                                                      const uint32_t* tile_off,
                                                                      const uint32_t* super_total) {
    if (io.counts) segment_count(io, tps, ntiles, nseg, (uint64_t)blockIdx.x * kBlock + threadIdx.x, tile_off, nullptr, super_total);
    const uint64_t tile = (uint64_t)blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tile >= ntiles) return;
    scatter_tile_lean(io, in, seg_len, tps, tile, threadIdx.x & 63u, tile_off, super_total);
}

// lrc_pipe_records of a lean set: the 36-byte record of every ray rebuilt from its 12-byte record (t, label, slot) -- the
// triangle id through the scene's slot table, the normal by the helper write_back forms it with, the point by pair_row from the
// set's own table (or, a tile in the row form, from its row: LeanIn); a ray that is not kept gets the miss record.  Reads nothing
// of the caller's: its poses and table may have changed since the submit.  seg_len % 64 == 0: a wave lies in one pose.
__global__ __launch_bounds__(kBlock) void expand_lean_kernel(const LeanIn in, uint64_t seg_len,
                                                             const uint32_t* __restrict__ slot_prim, const float4* __restrict__ tris,
                                                             lrc_hits out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t seg = i / seg_len;
    const LeanPose ps = lean_pose(in, (uint32_t)seg_len, (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)seg));
    const rec3 a = *(const rec3*)(in.rec + i * 3);
    uint32_t prim = LRC_INVALID_PRIM;
    float nx = 0.f, ny = 0.f, nz = 0.f, px = 0.f, py = 0.f, pz = 0.f;
    if (a.z != 0xFFFFFFFFu) {
        prim = slot_prim[a.z];
        slot_normal(tris[(size_t)a.z * 3 + 2], nx, ny, nz);
        const float4 r = ps.rec ? lean_row(ps, lean_h(in, (uint32_t)seg_len, (uint32_t)(i - seg * seg_len)), rec2{a.x, a.y}) : in.row[i];
        px = r.x; py = r.y; pz = r.z;
    }
    out.t[i] = __uint_as_float(a.x);
    out.prim[i] = prim;
    out.normal3[i * 3] = nx; out.normal3[i * 3 + 1] = ny; out.normal3[i * 3 + 2] = nz;
    out.point3[i * 3] = px; out.point3[i * 3 + 1] = py; out.point3[i * 3 + 2] = pz;
    out.sem[i] = (uint16_t)(a.y & 0xFFFFu);
    out.ins[i] = (uint16_t)(a.y >> 16);
}

// |p| of assembled (x, y, z, label) rows from the WORLD origin, float32, as np.linalg.norm(points, axis=1) forms it
// (the quantity the reference's ScanQuality range statistics are taken over, s3dis_simulator.py:283-284)
__global__ __launch_bounds__(kBlock) void rows_range_kernel(const float4* __restrict__ rows, uint64_t n, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 r = rows[i];
    out[i] = __builtin_sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z);
}

// ---- scene cloud from per-ray (t, label) pairs -------------------------------------------------------
// A pose-batched scan is a pure function of (pose, direction table), so a rank that holds the poses and the
// table can rebuild any other rank's hit points from the 8-byte pair alone: this is what the multi-GPU
// all-gather moves instead of 16-byte rows.  Same arithmetic as the trace epilogue (gen_ray + hit_point).

__global__ __launch_bounds__(kBlock) void cloud_count_kernel(const uint2* tl, uint64_t seg_len, uint64_t tps,
                                                             uint64_t ntiles, uint32_t* tile_cnt) {
    const uint64_t tile = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const uint64_t seg = tile / tps, chunk = tile - seg * tps;
    const uint64_t i = chunk * 64 + (threadIdx.x & 63u);
    bool keep = false;
    if (i < seg_len) keep = __uint_as_float(tl[seg * seg_len + i].x) < __builtin_inff();
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) tile_cnt[tile] = (uint32_t)__popcll(m);
}

__global__ __launch_bounds__(kBlock) void cloud_scatter_kernel(const double* poses16, const double* dirs3,
                                                               const uint2* tl, uint64_t seg_len, uint64_t tps,
                                                               uint64_t ntiles, uint64_t nseg,
                                                               const uint32_t* tile_off, const uint64_t* super_base,
                                                               float4* out_xyzl, uint64_t* counts) {
    const uint32_t lane = threadIdx.x & 63u;
    if (counts) {
        const uint64_t sg = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
        if (sg < nseg) {
            const uint64_t nsuper = (ntiles + 1023) / 1024;
            const uint64_t g0 = sg * tps, g1 = g0 + tps;
            const uint64_t o0 = g0 >= ntiles ? super_base[nsuper] : super_base[g0 >> 10] + tile_off[g0];
            const uint64_t o1 = g1 >= ntiles ? super_base[nsuper] : super_base[g1 >> 10] + tile_off[g1];
            counts[sg] = o1 - o0;
        }
    }
    const uint64_t tile = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const uint64_t seg = tile / tps, chunk = tile - seg * tps;
    const uint64_t i = chunk * 64 + lane;
    uint2 rec = make_uint2(0x7F800000u, 0u);
    if (i < seg_len) rec = tl[seg * seg_len + i];
    const float t = __uint_as_float(rec.x);
    const bool keep = t < __builtin_inff();
    const unsigned long long m = __ballot(keep);
    if (!keep) return;
    const uint64_t dst = super_base[tile >> 10] + tile_off[tile] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    V3 o, d, h, pt;
    double cx, cy, cz;
    gen_ray(poses16, dirs3, seg, i, o, d, cx, cy, cz);
    hit_point(o, d, t, h, pt);
    out_xyzl[dst] = make_float4(pt.x, pt.y, pt.z, __uint_as_float(rec.y));
}

// ---- scene cloud from per-ray triangle ids ---------------------------------------------------------------
// The hit of a pose-batched scan is a pure function of (pose, direction, triangle): a rank that holds the scene,
// the poses and the direction table rebuilds t with the scan's own ray/triangle test (tri_hit, bit-identical) and
// the point and label from it.  So the multi-GPU all-gather moves the 4-byte primitive id per ray -- Open3D's
// primitive_ids -- and nothing else.  Rays the sender dropped (miss, range filter) carry LRC_INVALID_PRIM.
// Entry (pose p, ray i) lives in slab p / pps at word (p % pps) * seg_len + i; slabs are `stride` words apart.

__global__ __launch_bounds__(kBlock) void prim_count_kernel(const uint32_t* prims, uint64_t pps, uint64_t stride,
                                                            uint64_t seg_len, uint64_t tps, uint64_t ntiles,
                                                            uint32_t* tile_cnt) {
    const uint64_t tile = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const uint64_t seg = tile / tps, chunk = tile - seg * tps;
    const uint64_t i = chunk * 64 + (threadIdx.x & 63u);
    const uint64_t sb = seg / pps;
    bool keep = false;
    if (i < seg_len) keep = prims[sb * stride + (seg - sb * pps) * seg_len + i] != LRC_INVALID_PRIM;
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) tile_cnt[tile] = (uint32_t)__popcll(m);
}

// (N,3) -> x[N] y[N] z[N]: the rebuild reads one direction per lane, and a 24-byte stride costs the vector L1 three
// times the transactions of three unit-stride reads
__global__ __launch_bounds__(kBlock) void dirs_transpose_kernel(const double* __restrict__ dirs3, uint32_t n,
                                                                double* __restrict__ soa) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    soa[i] = dirs3[(size_t)i * 3];
    soa[(size_t)n + i] = dirs3[(size_t)i * 3 + 1];
    soa[2 * (size_t)n + i] = dirs3[(size_t)i * 3 + 2];
}

// Stand-alone rebuild: one wave per R consecutive tiles.
// No XCD-contiguous remap of the tiles here: eight write streams a power of two apart land on the same HBM channels
// in lock step -- measured 540 us against 330 us for round-robin workgroups.
template <int R>
__global__ __launch_bounds__(kBlock) void prim_scatter_kernel(const RebuildParams q) {
    rebuild_counts(q, blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
    // everything that depends on the tile alone is wave-uniform: keep it on the scalar unit
    const uint32_t tile0 = __builtin_amdgcn_readfirstlane((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * R);
    if (tile0 >= q.ntiles) return;
    rebuild_tiles<R>(q, tile0, q.ntiles, threadIdx.x & 63u);
}

// Per caller's triangle ROW: (v0, label bits), (Ng, 0) -- all a known hit needs to give t again.  Read by the multi-GPU
// cloud rebuild only (lrc_cloud_from_prims_dev), so it is built from the slot arrays the first time that is called.
__global__ __launch_bounds__(kBlock) void prim_plane_kernel(const float4* __restrict__ tris, const uint32_t* __restrict__ slot_prim,
                                                            const uint32_t* __restrict__ slot_label, uint32_t num_slots,
                                                            uint32_t num_prims, float4* __restrict__ plane) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= num_slots) return;
    const uint32_t row = slot_prim[k];
    if (row >= num_prims) return;
    const float4 a = tris[(size_t)k * 3], c = tris[(size_t)k * 3 + 2];
    plane[(size_t)row * 2] = make_float4(a.x, a.y, a.z, __uint_as_float(slot_label[k]));
    plane[(size_t)row * 2 + 1] = make_float4(c.y, c.z, c.w, 0.0f);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

// shared with the other translation units of the library (not part of the public ABI)
int lrc_internal_fail(int code, const char* msg) { return fail(code, msg ? msg : ""); }
// test hook (tests/test_tile_mapping.py): the ray of every (tile, lane) of a pose of tpp tiles for a line width hint (in rays)
// and the line width in tiles the pipeline would use for it -- the host compilation of the kernel's mapping (lrc_device.h)
uint32_t lrc_internal_tile_map(uint64_t line_width, uint32_t tpp, uint32_t* out_ray) {
    const uint32_t wt = line_tiles_for(line_width, (uint64_t)tpp * 64u);
    if (out_ray)
        for (uint32_t u = 0; u < tpp; ++u)
            for (uint32_t l = 0; l < 64u; ++l) out_ray[(size_t)u * 64u + l] = tile_ray(u, l, wt, tpp);
    return wt;
}
// ... and its line-group form (tests/test_tile_groups.py): `lines` (1, 2, 4) lines per tile, groups kept on either side of line
// `split`.  Returns the lines per tile of the widest group the mapping forms.
uint32_t lrc_internal_tile_map_groups(uint64_t line_width, uint32_t tpp, uint32_t split, uint32_t lines, uint32_t* out_ray) {
    const uint32_t wt = lines >= 2u ? line_tiles_for(line_width, (uint64_t)tpp * 64u) : 0u;
    const uint32_t grp = line_group_for(split, lines);
    if (out_ray)
        for (uint32_t u = 0; u < tpp; ++u)
            for (uint32_t l = 0; l < 64u; ++l) out_ray[(size_t)u * 64u + l] = tile_ray(u, l, wt, tpp, grp);
    return tile_lines_of(wt, tpp, grp);
}
// test hook (tests/test_range_band.py): the range filter's decision for squared distances s[0..n) against max_range, made by the
// host compilation of the very functions the kernel calls (lrc_device.h, range_band): keep[i] = the filter keeps s[i];
// in_band[i] = the square root decided (also when the bounds are not used at all).  bounds3: lo, hi, fast.
void lrc_internal_range_decide(double max_range, const double* s, uint64_t n, uint8_t* keep, uint8_t* in_band, double* bounds3) {
    const RangeBand rb = range_band(max_range);
    if (bounds3) { bounds3[0] = rb.lo; bounds3[1] = rb.hi; bounds3[2] = (double)rb.fast; }
    for (uint64_t i = 0; i < n; ++i) {
        const bool band = !rb.fast || range_in_band(s[i], rb.lo, rb.hi);
        keep[i] = band ? (uint8_t)(std::sqrt(s[i]) < max_range) : (uint8_t)range_below(s[i], rb.lo);
        if (in_band) in_band[i] = (uint8_t)band;
    }
}

// test hook (tests/test_ray_table_host.py): rows of the ray table of a prepared pipeline submit for the rotation block rot9 (row
// major), made by the host compilation of the very function ray_table_kernel calls (lrc_device.h, ray_row): per row 9 floats
// d, inv, h
void lrc_internal_ray_table_rows(const double* rot9, const double* dirs3, uint64_t n, float* out9) {
    for (uint64_t i = 0; i < n; ++i) {
        const RayRow r = ray_row(rot9, dirs3[3 * i], dirs3[3 * i + 1], dirs3[3 * i + 2]);
        float* q = out9 + 9 * i;
        q[0] = r.d.x; q[1] = r.d.y; q[2] = r.d.z; q[3] = r.inv.x; q[4] = r.inv.y; q[5] = r.inv.z; q[6] = r.h.x; q[7] = r.h.y; q[8] = r.h.z;
    }
}

// test hook (tests/test_pipe_pair_rows_host.py): the output rows of n rays from origin, unit vector, t and label, made by the host
// compilation of the very function the trace's write-back and the consumers of a lean record set call (lrc_device.h, pair_row):
// per ray 4 words x, y, z, label
void lrc_internal_pair_rows(const float* o3, const float* h3, const float* t, const uint32_t* label, uint64_t n, uint32_t* out4) {
    for (uint64_t i = 0; i < n; ++i) {
        const PairRow r = pair_row(V3{o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]}, V3{h3[3 * i], h3[3 * i + 1], h3[3 * i + 2]}, t[i], label[i]);
        std::memcpy(out4 + 4 * i, &r, 16);
    }
}

const char* lrc_version(void) { return "lidarcast 0.1.0 (gfx950)"; }

const char* lrc_last_error(void) { return g_err.c_str(); }

int lrc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int lrc_ctx_create(int device, lrc_ctx** out_ctx) {
    if (!out_ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_ctx_create: out_ctx is NULL");
    *out_ctx = nullptr;
    int n = lrc_device_count();
    if (n <= 0) return fail(LRC_ERR_NO_DEVICE, "lrc_ctx_create: no HIP device is visible");
    if (device < 0 || device >= n)
        return fail(LRC_ERR_NO_DEVICE, "lrc_ctx_create: device ordinal out of range");
    LRC_HIP(hipSetDevice(device));
    lrc_ctx* c = new (std::nothrow) lrc_ctx();
    if (!c) return fail(LRC_ERR_OOM, "lrc_ctx_create: out of host memory");
    c->device = device;
    // the signal word of the launch chain; where stream memory operations are not available launches are simply not chained
    int can_wait = 0;
    if (hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, device) == hipSuccess && can_wait) {
        void* w = nullptr;
        if (hipExtMallocWithFlags(&w, 8, hipMallocSignalMemory) == hipSuccess && w) {
            if (hipStreamWriteValue64(nullptr, w, 0, 0) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess) {
                c->chain_word = (uint64_t*)w;
            } else {
                (void)hipFree(w);
            }
        }
    }
    (void)hipGetLastError();
    *out_ctx = c;
    return LRC_OK;
}

int lrc_ctx_set_launch_chaining(lrc_ctx* ctx, int enabled) {
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_ctx_set_launch_chaining: ctx is NULL");
    ctx->chain_enabled = enabled != 0;
    return LRC_OK;
}

int lrc_ctx_get_launch_chaining(const lrc_ctx* ctx, int* enabled, int* supported) {
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_ctx_get_launch_chaining: ctx is NULL");
    if (enabled) *enabled = ctx->chain_enabled ? 1 : 0;
    if (supported) *supported = ctx->chain_word ? 1 : 0;
    return LRC_OK;
}

int lrc_ctx_destroy(lrc_ctx* ctx) {
    if (!ctx) return LRC_OK;
    (void)hipSetDevice(ctx->device);
    for (int k = 0; k < kPoolSlots; ++k)
        if (ctx->pool[k]) (void)hipFree(ctx->pool[k]);
    if (ctx->h_counts) (void)hipHostFree(ctx->h_counts);
    lrc::arena_release(&ctx->build_arena);
    if (ctx->s_compute) (void)hipStreamDestroy(ctx->s_compute);
    if (ctx->s_copy) (void)hipStreamDestroy(ctx->s_copy);
    if (ctx->s_stats) (void)hipStreamDestroy(ctx->s_stats);
    for (hipEvent_t e : ctx->ev_chunk) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_compact) if (e) (void)hipEventDestroy(e);
    if (ctx->chain_word) (void)hipFree(ctx->chain_word);
    if (ctx->stat_scratch) (void)hipFree(ctx->stat_scratch);
    if (ctx->d_noise_tab) (void)hipFree(ctx->d_noise_tab);
    for (hipEvent_t e : ctx->compact_done) if (e) (void)hipEventDestroy(e);
    for (lrc_ctx::TileScratch& sc : ctx->compact_scratch) sc.release();      // (the context's device is current: above)
    ctx->cloud_scratch.release();
    delete ctx;
    return LRC_OK;
}

int lrc_ctx_synchronize(lrc_ctx* ctx) {
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_ctx_synchronize: ctx is NULL");
    LRC_HIP(hipSetDevice(ctx->device));
    LRC_HIP(hipDeviceSynchronize());
    return LRC_OK;
}

int lrc_scene_destroy(lrc_scene* s) {
    if (!s) return LRC_OK;
    if (s->deform)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scene_destroy: the scene belongs to a deformable (lrc_deform_destroy frees it)");
    if (s->ctx) (void)hipSetDevice(s->ctx->device);
    if (s->slab) {
        (void)hipFree(s->slab);
    } else {
        if (s->d_nodes) (void)hipFree(s->d_nodes);
        if (s->d_tris) (void)hipFree(s->d_tris);
        if (s->d_slot_prim) (void)hipFree(s->d_slot_prim);
        if (s->d_slot_label) (void)hipFree(s->d_slot_label);
        if (s->d_slot_box) (void)hipFree(s->d_slot_box);
        if (s->d_nodes_q) (void)hipFree(s->d_nodes_q);
        if (s->d_nodes_n) (void)hipFree(s->d_nodes_n);
    }
    if (s->d_prim_plane) (void)hipFree(s->d_prim_plane);
    if (s->d_slot_sphere) (void)hipFree(s->d_slot_sphere);
    if (s->d_nodes_q4) (void)hipFree(s->d_nodes_q4);
    if (s->d_nodes_n4) (void)hipFree(s->d_nodes_n4);
    if (s->flow_scratch) (void)hipFree(s->flow_scratch);
    delete s;
    return LRC_OK;
}

}  // extern "C"

namespace {

void build_options_from_env(lrc::BuildOptions& opt) {
    opt.max_leaf = env_int("LRC_MAX_LEAF", opt.max_leaf);
    opt.bfs_nodes = env_int("LRC_BFS_NODES", opt.bfs_nodes);
    opt.depth_slack = env_int("LRC_DEPTH_SLACK", opt.depth_slack);
    opt.median_only = env_int("LRC_BUILD_MEDIAN_ONLY", 0);      // test hook: every split takes the median fallback
    opt.subtrees = env_int("LRC_BUILD_SUBTREES", opt.subtrees);  // 0: the device builder goes level by level to the bottom (A/B)
}

// LRC_QNODES: 0 = float32 nodes only, 1 (default) = quantised images when the grid is fine enough for the scene's
// triangles, 2 = whenever the grid fits.  The grid has 2^15 cells along each axis of the scene; where the cells are
// not small against the leaf boxes (a very large scene of small triangles) the widened boxes cost more triangle tests
// than the smaller nodes save (measured: DESIGN.md section 4.1).
int qnodes_mode() { return env_int("LRC_QNODES", 1); }      // read at every scene creation

void qnodes_report(const lrc_scene* s, double infl) {
    if (std::getenv("LRC_QNODES_VERBOSE"))
        std::fprintf(stderr, "[qnodes] leaf box inflation %.3f, W = %g %g %g -> %s\n", infl, (double)s->qW[0],
                     (double)s->qW[1], (double)s->qW[2], s->d_nodes_q ? "quantised images" : "float32 nodes");
}

// The scene build on the device (lrc_bvh_device.hip): the same tree, the same bytes as the host builder below, in
// milliseconds.  Returns lrc::kDevBuildUnsupported (1) for a mesh the device path does not take (<= max_leaf triangles).
int scene_create_device(lrc_ctx* ctx, const float* verts3, uint64_t V, const uint32_t* tris3, uint64_t T,
                        const uint16_t* tri_sem, const uint16_t* tri_ins, bool on_device, int qmode, lrc_scene** out_scene) {
    lrc_scene* s = new (std::nothrow) lrc_scene();
    if (!s) return fail(LRC_ERR_OOM, "lrc_scene_create: out of host memory");
    s->ctx = ctx;
    lrc::DeviceScene d;
    lrc::BuildOptions opt;
    build_options_from_env(opt);
    const int rc = lrc::build_bvh_device(&ctx->build_arena, verts3, V, tris3, T, tri_sem, tri_ins, on_device, opt,
                                         qmode, &d);
    if (rc != lrc::kDevBuildOk) {
        delete s;
        return rc;
    }
    s->slab = d.slab;
    s->d_nodes = (float4*)d.nodes;
    s->d_tris = (float4*)d.tris;
    s->d_slot_prim = d.slot_prim;
    s->d_slot_label = d.slot_label;
    s->d_slot_box = d.slot_box;
    s->d_nodes_q = (uint4*)d.nodes_q;
    s->d_nodes_n = (float4*)d.nodes_n;
    for (int a = 0; a < 3; ++a) { s->qbase[a] = d.qbase[a]; s->qW[a] = d.qW[a]; s->qinvW[a] = d.qinvW[a]; }
    lrc_scene_info& in = s->info;
    in.num_vertices = V;
    in.num_triangles = T;
    in.num_nodes = d.num_nodes;
    in.num_leaves = d.num_leaves;
    in.num_slots = d.num_slots;
    in.max_depth = d.max_depth;
    in.max_leaf_size = d.max_leaf_size;
    for (int k = 0; k < 3; ++k) { in.bounds_lo[k] = d.bounds_lo[k]; in.bounds_hi[k] = d.bounds_hi[k]; }
    in.device_bytes = d.slab_bytes;
    in.build_ms = d.ms_hierarchy + d.ms_emit;
    in.upload_ms = d.ms_upload;
    in.quantised_nodes = s->d_nodes_q ? 1u : 0u;
    in.leaf_inflation = (float)d.leaf_inflation;
    in.device_build = 1u;
    qnodes_report(s, d.leaf_inflation);
    *out_scene = s;
    return LRC_OK;
}

int scene_create_host(lrc_ctx* ctx, const float* verts3, uint64_t V, const uint32_t* tris3, uint64_t T,
                      const uint16_t* tri_sem, const uint16_t* tri_ins, int qmode, lrc_scene** out_scene) {
    for (uint64_t i = 0; i < 3 * T; ++i)
        if (tris3[i] >= V)
            return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create: triangle index out of range");
    for (uint64_t i = 0; i < 3 * V; ++i) {
        uint32_t u;   // bit test: immune to any finite-math assumption of the compiler
        std::memcpy(&u, &verts3[i], 4);
        if ((u & 0x7FFFFFFFu) > 0x49742400u /* 1e6f */)
            return fail(LRC_ERR_INVALID_ARG,
                        "lrc_scene_create: vertex coordinate is not finite or exceeds 1e6");
    }
    lrc_scene* s = new (std::nothrow) lrc_scene();
    if (!s) return fail(LRC_ERR_OOM, "lrc_scene_create: out of host memory");
    s->ctx = ctx;

    lrc::HostBVH h;
    lrc::BuildOptions opt;
    build_options_from_env(opt);
    auto t0 = std::chrono::steady_clock::now();
    try {
        lrc::build_bvh(verts3, V, tris3, T, tri_sem, tri_ins, opt, &h);
    } catch (const std::bad_alloc&) {
        delete s;
        return fail(LRC_ERR_OOM, "lrc_scene_create: out of host memory during the BVH build");
    } catch (...) {
        delete s;
        return fail(LRC_ERR_INTERNAL, "lrc_scene_create: BVH build failed");
    }
    auto t1 = std::chrono::steady_clock::now();

    lrc_scene_info& in = s->info;
    in.num_vertices = V;
    in.num_triangles = T;
    in.num_nodes = h.num_nodes;
    in.num_leaves = h.num_leaves;
    in.num_slots = h.num_slots;
    in.max_depth = h.max_depth;
    in.max_leaf_size = h.max_leaf_size;
    for (int k = 0; k < 3; ++k) { in.bounds_lo[k] = h.bounds_lo[k]; in.bounds_hi[k] = h.bounds_hi[k]; }
    in.build_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();

    auto upload = [&](void** dptr, const void* src, size_t bytes) -> int {
        if (!bytes) return LRC_OK;
        LRC_HIP(hipMalloc(dptr, bytes));
        LRC_HIP(hipMemcpy(*dptr, src, bytes, hipMemcpyHostToDevice));
        in.device_bytes += bytes;
        return LRC_OK;
    };
    int rc;
    if ((rc = upload((void**)&s->d_nodes, h.nodes.data(), h.nodes.size() * 4)) ||
        (rc = upload((void**)&s->d_tris, h.tri_rec.data(), h.tri_rec.size() * 4)) ||
        (rc = upload((void**)&s->d_slot_prim, h.slot_prim.data(), h.slot_prim.size() * 4)) ||
        (rc = upload((void**)&s->d_slot_label, h.slot_label.data(), h.slot_label.size() * 4)) ||
        (rc = upload((void**)&s->d_slot_box, h.slot_box.data(), h.slot_box.size() * 4))) {
        std::string keep = g_err;
        lrc_scene_destroy(s);
        g_err = keep;
        return rc;
    }
    {
        std::vector<uint32_t> q8, q16;
        std::vector<float> n16, n32;
        double infl = 1.0;
        const int mode = qmode;
        lrc::QGrid g;
        if (mode != 0 && lrc::make_qgrid(h, s->qbase, s->qW, s->qinvW, g) && lrc::build_qnodes(h, g, q8, n16, &infl) &&
            (mode >= 2 || infl <= lrc::kQnodeMaxInflation)) {
#ifdef LRC_VARIANTS
            if (env_int("LRC_WIDE", 0) != 0 && !lrc::build_q4nodes(h, g, q16, n32, &s->num_nodes4)) { q16.clear(); n32.clear(); }
#endif
            if ((rc = upload((void**)&s->d_nodes_q, q8.data(), q8.size() * 4)) ||
                (rc = upload((void**)&s->d_nodes_n, n16.data(), n16.size() * 4)) ||
                (rc = upload((void**)&s->d_nodes_q4, q16.data(), q16.size() * 4)) ||
                (rc = upload((void**)&s->d_nodes_n4, n32.data(), n32.size() * 4))) {
                std::string keep = g_err;
                lrc_scene_destroy(s);
                g_err = keep;
                return rc;
            }
        }
        in.quantised_nodes = s->d_nodes_q ? 1u : 0u;
        in.leaf_inflation = (float)infl;
        qnodes_report(s, infl);
    }
    auto t2 = std::chrono::steady_clock::now();
    in.upload_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    *out_scene = s;
    return LRC_OK;
}

// LRC_DEVICE_BUILD: 1 (default) = build the scene on the GPU, 0 = host builder (same tree, same bytes; the reference
// for the device builder in the tests).  The four-wide images of the laboratory build exist on the host path only.
bool want_device_build() {
#ifdef LRC_VARIANTS
    if (env_int("LRC_WIDE", 0) != 0) return false;
#endif
    return env_int("LRC_DEVICE_BUILD", 1) != 0;
}

}  // namespace

#ifdef LRC_VARIANTS
#include "lrc_lab.h"
#endif

extern "C" {

int lrc_scene_create(lrc_ctx* ctx, const float* verts3, uint64_t V, const uint32_t* tris3, uint64_t T,
                     const uint16_t* tri_sem, const uint16_t* tri_ins, lrc_scene** out_scene) {
    return scene_create_mode(ctx, verts3, V, tris3, T, tri_sem, tri_ins, qnodes_mode(), out_scene);
}

}  // extern "C"

// lrc_scene_create with the node images chosen by the caller (qmode as LRC_QNODES): lrc_deform_create asks for 0
int scene_create_mode(lrc_ctx* ctx, const float* verts3, uint64_t V, const uint32_t* tris3, uint64_t T,
                      const uint16_t* tri_sem, const uint16_t* tri_ins, int qmode, lrc_scene** out_scene) {
    if (!out_scene) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create: out_scene is NULL");
    *out_scene = nullptr;
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create: ctx is NULL");
    if ((V && !verts3) || (T && !tris3))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create: NULL vertex or triangle array");
    if (T >= (1ull << 28) || V >= (1ull << 32))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create: mesh too large (T < 2^28, V < 2^32)");
    LRC_HIP(hipSetDevice(ctx->device));
    if (want_device_build()) {
        const int rc = scene_create_device(ctx, verts3, V, tris3, T, tri_sem, tri_ins, false, qmode, out_scene);
        if (rc != lrc::kDevBuildUnsupported) return rc;
    }
    return scene_create_host(ctx, verts3, V, tris3, T, tri_sem, tri_ins, qmode, out_scene);
}

extern "C" {

int lrc_scene_create_dev(lrc_ctx* ctx, const float* d_verts3, uint64_t V, const uint32_t* d_tris3, uint64_t T,
                         const uint16_t* d_tri_sem, const uint16_t* d_tri_ins, lrc_scene** out_scene) {
    if (!out_scene) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create_dev: out_scene is NULL");
    *out_scene = nullptr;
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create_dev: ctx is NULL");
    if ((V && !d_verts3) || (T && !d_tris3))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create_dev: NULL vertex or triangle array");
    if (T >= (1ull << 28) || V >= (1ull << 32))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scene_create_dev: mesh too large (T < 2^28, V < 2^32)");
    LRC_HIP(hipSetDevice(ctx->device));
    if (want_device_build()) {
        const int rc = scene_create_device(ctx, d_verts3, V, d_tris3, T, d_tri_sem, d_tri_ins, true, qnodes_mode(), out_scene);
        if (rc != lrc::kDevBuildUnsupported) return rc;
    }
    // a mesh the device builder does not take (a handful of triangles), or LRC_DEVICE_BUILD=0: build on the host
    std::vector<float> hv(3 * V);
    std::vector<uint32_t> ht(3 * T);
    std::vector<uint16_t> hs(d_tri_sem ? T : 0), hi(d_tri_ins ? T : 0);
    if (V) LRC_HIP(hipMemcpy(hv.data(), d_verts3, 3 * V * 4, hipMemcpyDeviceToHost));
    if (T) LRC_HIP(hipMemcpy(ht.data(), d_tris3, 3 * T * 4, hipMemcpyDeviceToHost));
    if (d_tri_sem && T) LRC_HIP(hipMemcpy(hs.data(), d_tri_sem, T * 2, hipMemcpyDeviceToHost));
    if (d_tri_ins && T) LRC_HIP(hipMemcpy(hi.data(), d_tri_ins, T * 2, hipMemcpyDeviceToHost));
    return scene_create_host(ctx, hv.data(), V, ht.data(), T, d_tri_sem ? hs.data() : nullptr,
                             d_tri_ins ? hi.data() : nullptr, qnodes_mode(), out_scene);
}

int lrc_scene_get_info(const lrc_scene* scene, lrc_scene_info* out_info) {
    if (!scene || !out_info) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_get_info: NULL argument");
    *out_info = scene->info;
    return LRC_OK;
}

int lrc_scene_set_options(lrc_scene* scene, const lrc_scan_options* opts) {
    if (!scene) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_set_options: scene is NULL");
    if (!opts) { scene->opts = lrc_scan_options{}; return LRC_OK; }
    if (!(opts->min_range >= 0.0) || (opts->incident_mode != 0 && opts->incident_mode != 1))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scene_set_options: min_range < 0 or unknown incident_mode");
    scene->opts = *opts;
    return LRC_OK;
}

int lrc_scene_get_counters(const lrc_scene* scene, uint64_t* launches, uint64_t* rays) {
    if (!scene) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_get_counters: scene is NULL");
    if (launches) *launches = scene->launches;
    if (rays) *rays = scene->rays;
    return LRC_OK;
}

int lrc_scene_export_bvh(const lrc_scene* s, float* nodes16, uint32_t* slot_prim) {
    if (!s) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_export_bvh: scene is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    if (nodes16 && s->info.num_nodes)
        LRC_HIP(hipMemcpy(nodes16, s->d_nodes, s->info.num_nodes * 64, hipMemcpyDeviceToHost));
    if (slot_prim && s->info.num_slots)
        LRC_HIP(hipMemcpy(slot_prim, s->d_slot_prim, s->info.num_slots * 4, hipMemcpyDeviceToHost));
    return LRC_OK;
}

// the plane table of the cloud rebuild, built on first use.  The table is complete before the pointer is published (one
// synchronisation, once per scene): a second caller -- another host thread, or another non-blocking stream -- either sees
// NULL and waits for the mutex, or sees a finished table; it can never read a zeroed or half-written one.
static int ensure_prim_plane(lrc_scene* s, hipStream_t st) {
    if (s->deform)
        return fail(LRC_ERR_INVALID_ARG, "the plane table caches per-triangle geometry: not available on a deformable scene");
    if (s->info.num_triangles == 0) return LRC_OK;
    if (__atomic_load_n(&s->d_prim_plane, __ATOMIC_ACQUIRE)) return LRC_OK;
    std::lock_guard<std::mutex> lock(s->plane_mutex);
    if (s->d_prim_plane) return LRC_OK;
    const uint64_t T = s->info.num_triangles;
    float4* table = nullptr;
    LRC_HIP(hipMalloc((void**)&table, T * 32));
    hipError_t e = hipMemsetAsync(table, 0, T * 32, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(prim_plane_kernel, dim3((uint32_t)blocks_of(s->info.num_slots, kBlock)), dim3(kBlock), 0, st,
                           (const float4*)s->d_tris, (const uint32_t*)s->d_slot_prim, (const uint32_t*)s->d_slot_label,
                           (uint32_t)s->info.num_slots, (uint32_t)T, table);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(table);
        (void)hipGetLastError();
        return fail(LRC_ERR_HIP, std::string("plane table of the cloud rebuild: ") + hipGetErrorString(e));
    }
    s->info.device_bytes += T * 32;
    __atomic_store_n(&s->d_prim_plane, table, __ATOMIC_RELEASE);
    return LRC_OK;
}

int lrc_scene_export_array(const lrc_scene* cs, int which, void* dst, uint64_t dst_bytes, uint64_t* out_bytes) {
    if (!cs) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_export_array: scene is NULL");
    lrc_scene* s = const_cast<lrc_scene*>(cs);
    if (which == LRC_ARRAY_PRIM_PLANE) {
        LRC_HIP(hipSetDevice(s->ctx->device));
        int rc = ensure_prim_plane(s, nullptr);
        if (rc) return rc;
        LRC_HIP(hipStreamSynchronize(nullptr));
    }
    const void* src = nullptr;
    uint64_t bytes = 0;
    const lrc_scene_info& in = s->info;
    switch (which) {
        case LRC_ARRAY_NODES: src = s->d_nodes; bytes = in.num_nodes * 64; break;
        case LRC_ARRAY_TRIS: src = s->d_tris; bytes = in.num_slots * 48; break;
        case LRC_ARRAY_SLOT_PRIM: src = s->d_slot_prim; bytes = in.num_slots * 4; break;
        case LRC_ARRAY_SLOT_LABEL: src = s->d_slot_label; bytes = in.num_slots * 4; break;
        case LRC_ARRAY_PRIM_PLANE: src = s->d_prim_plane; bytes = in.num_triangles * 32; break;
        case LRC_ARRAY_NODES_Q: src = s->d_nodes_q; bytes = s->d_nodes_q ? in.num_nodes * 32 : 0; break;
        case LRC_ARRAY_NODES_N: src = s->d_nodes_n; bytes = s->d_nodes_n ? in.num_nodes * 64 : 0; break;
        default: return fail(LRC_ERR_INVALID_ARG, "lrc_scene_export_array: unknown array");
    }
    if (out_bytes) *out_bytes = bytes;
    if (!dst || !bytes) return LRC_OK;
    if (dst_bytes < bytes) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_export_array: destination too small");
    LRC_HIP(hipSetDevice(s->ctx->device));
    LRC_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return LRC_OK;
}

// stack entries a trace needs = deepest leaf depth (one pending sibling per inner level above it), and the LDS that holds them
static uint32_t trace_stack_depth(const lrc_scene* s) { return s->info.max_depth < 1 ? 1 : s->info.max_depth; }
static size_t trace_lds_bytes(uint32_t depth) { return (size_t)depth * kTBlock * sizeof(int); }

// One launch of the trace kernel over p.total rays.  gen: the generator by its name in lrc_gen.h.  kGenGrid is a grid scan
// (lrc_scan_grid_*): the per-ray kernel of kGenPoses here, the packet kernel in the laboratory build.  kGenEchoes: p.total and
// p.rays_per_pose count echo records on entry.
static int launch_trace(lrc_scene* s, TraceParams& p, int gen, hipStream_t st, bool stats = false) {
    p.nodes = s->d_nodes;
    p.tris = s->d_tris;
    p.slot_prim = s->d_slot_prim;
    p.slot_label = s->d_slot_label;
    p.slot_box = s->d_slot_box;
    p.prim_plane = s->d_prim_plane;
    p.num_nodes = (uint32_t)s->info.num_nodes;
    p.nodes_q = s->d_nodes_q;
    p.nodes_n = s->d_nodes_n;
    p.nodes_q4 = s->d_nodes_q4;
    p.nodes_n4 = s->d_nodes_n4;
    for (int a = 0; a < 3; ++a) { p.qbase[a] = s->qbase[a]; p.qW[a] = s->qW[a]; p.qinvW[a] = s->qinvW[a]; }
    const bool qn = s->d_nodes_q != nullptr;
    if (gen == kGenEchoes) {      // the caller counts echo RECORDS (E per beam), the kernel LANES (G per beam, lrc_echo.h)
        const uint64_t E = p.echo.max_echoes;
        p.rays_per_pose = (p.rays_per_pose / E) << p.echo.group_log2;
        p.total = (p.total / E) << p.echo.group_log2;
    }
    p.min_range = s->opts.min_range;
    p.incident_mode = s->opts.incident_mode;
    if (!p.range_noise && s->opts.range_noise) {      // device entry points: the pointer is a device pointer
        if (s->opts.range_noise_len != p.total)
            return fail(LRC_ERR_INVALID_ARG, "range_noise_len does not match the number of rays of this call");
        p.range_noise = s->opts.range_noise;
    }
    if (p.total == 0) return LRC_OK;
    const uint64_t nblk = (p.total + kTBlock - 1) / kTBlock;
    if (nblk + p.pre.blocks > 0x7FFFFFFFull) return fail(LRC_ERR_INVALID_ARG, "too many rays for one launch");
    // pose-batched scans whose poses are whole tiles: the kernel forms pose and in-pose index from the tile number (in 32 bits:
    // poses of less than 2^32 rays)
    p.tiles_per_pose = (gen_pose_is_tiles(gen) && p.rays_per_pose % kTBlock == 0 && p.rays_per_pose <= 0xFFFFFFFFull)
                           ? (uint32_t)(p.rays_per_pose / kTBlock) : 0u;
    // two-line tiles: lean record sets only (the serial calls' tile_count is per 64 consecutive outputs), and the counters of
    // the instrumented kernel, which has no tile_count
    if (p.tiles_per_pose == 0u || (p.lean.row == nullptr && !stats)) p.line_tiles = 0u;
    if (p.line_tiles == 0u) p.line_group = 0u;
    const uint32_t depth = trace_stack_depth(s);
    const size_t lds = trace_lds_bytes(depth);
    p.stack_cap = depth;
    // Workgroup -> tile order.  A pose-batched scan deals every pose's tiles to the 8 XCDs in 16 chunks: each XCD works on
    // every pose (the poses of a trajectory cost differently: balance) but always on the same sixteenth-pairs of the scan
    // pattern, so what its L2 holds after one pose is what the next pose needs.  Other launches, and
    // scans whose pose is not 16 chunks of a power-of-two >= 16 tiles, keep the eight contiguous tile ranges.
    p.tile_chunk_log2 = 0;
    // ... while the scene is resident in the 256 MiB Infinity Cache.  Past it (synth_hall: 0.3 GB) an L2 miss costs an HBM
    // round trip and the XCD-local pose run -- neighbouring scan lines of ONE pose share their subtrees in the XCD's L2 --
    // is worth more than the balance: measured +1...+16 % for the striped order there, -1...-10 % on the cache-resident
    // scenes (profiles/r03_xcd_striping_sweep.txt).
    constexpr uint64_t kStripeSceneBytes = 192ull << 20;
    if (gen_table_order(gen) && p.rays_per_pose % 64 == 0 && s->info.device_bytes <= kStripeSceneBytes) {
        const uint64_t tpp = p.rays_per_pose / 64;
        if (tpp % 16 == 0) {
            const uint64_t chunk = tpp / 16;
            if (chunk >= 16 && (chunk & (chunk - 1)) == 0) { uint32_t k = 0; while ((1ull << k) < chunk) ++k; p.tile_chunk_log2 = k + 1; }
        }
    }
#ifdef LRC_VARIANTS
    {
        const int rc = launch_trace_lab(s, p, gen, st, stats, nblk, lds, depth);
        if (rc <= 0) {
            if (rc == LRC_OK) { LRC_HIP(hipGetLastError()); s->launches += 1; s->rays += p.total; }
            return rc;
        }
    }
#endif
    if (gen == kGenGrid) gen = kGenPoses;
    // Launch chain.  Every product trace launch signs the context's signal word when its last workgroup starts.  A launch
    // that goes to ANOTHER stream than the previous one is held until that signature is there: the caller keeps two scans
    // in flight (two streams, two record sets), so instead of both launches dispatching side by side and ending together --
    // or, by chance, not -- this one starts exactly when the previous one has no workgroup left to hand out, and its waves
    // fill the slots the previous launch's long-running last waves leave empty.  Same stream as before: stream order already
    // serialises the two launches, nothing is added.  The wait only ever refers to a launch enqueued earlier, so it cannot
    // close a cycle with the caller's own events.
    lrc_ctx* const cx_ = s->ctx;
    if (cx_->chain_word && cx_->chain_enabled) {
        if (cx_->chain_seq > 0 && st != cx_->chain_stream && st != nullptr && cx_->chain_stream != nullptr)
            LRC_HIP(hipStreamWaitValue64(st, cx_->chain_word, cx_->chain_seq, hipStreamWaitValueGte, ~0ull));
        p.chain_word = cx_->chain_word;
        p.chain_seq = cx_->chain_seq + 1;
    } else {
        p.chain_word = nullptr;
        p.chain_seq = 0;
    }
#define LRC_LAUNCH_Q(G, S, Q) \
    hipLaunchKernelGGL((trace_kernel<G, kLeafW, true, false, S, Q>), dim3((uint32_t)(nblk + p.pre.blocks)), dim3(kTBlock), lds, st, p)
#define LRC_LAUNCH(G, S) case G: if (qn) LRC_LAUNCH_Q(G, S, 1); else LRC_LAUNCH_Q(G, S, 0); break      // quantised or float32 nodes
    if (stats) {   // per-ray traversal counters (lrc_debug_scan_stats)
        switch (gen) {
            LRC_LAUNCH(kGenPoses, true);
            LRC_LAUNCH(kGenRays, true);
            default: return fail(LRC_ERR_INVALID_ARG, "traversal statistics are not available for the scan-angle generator");
        }
    } else {
        switch (gen) {
            LRC_LAUNCH(kGenRays, false);
            LRC_LAUNCH(kGenPoses, false);
            LRC_LAUNCH(kGenAngles, false);
            LRC_LAUNCH(kGenSweeps, false);
            LRC_LAUNCH(kGenNoisy, false);
            LRC_LAUNCH(kGenEchoes, false);
            LRC_LAUNCH(kGenMaterials, false);
            LRC_LAUNCH(kGenNoisySweeps, false);
            default: return fail(LRC_ERR_INTERNAL, "launch_trace: unknown ray generator");
        }
    }
#undef LRC_LAUNCH
#undef LRC_LAUNCH_Q
    LRC_HIP(hipGetLastError());
    if (p.chain_word) { cx_->chain_seq = p.chain_seq; cx_->chain_stream = st; }
    s->launches += 1;
    s->rays += gen == kGenEchoes ? (p.total >> p.echo.group_log2) * p.echo.subrays : p.total;      // echoes: the sub-rays cast, not the lanes
    return LRC_OK;
}

int lrc_scene_get_occupancy(const lrc_scene* s, int* waves_per_cu, int* vgprs, int* lds_bytes) {
    if (!s) return fail(LRC_ERR_INVALID_ARG, "lrc_scene_get_occupancy: scene is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    const size_t lds = trace_lds_bytes(trace_stack_depth(s));
    // the pose-batched product kernel this scene's scans run: over quantised nodes, or float32 ones
    const void* const kernel = s->d_nodes_q ? reinterpret_cast<const void*>(&trace_kernel<kGenPoses, kLeafW, true, false, false, 1>)
                                            : reinterpret_cast<const void*>(&trace_kernel<kGenPoses, kLeafW, true, false, false>);
    int blocks = 0;
    hipFuncAttributes attr;
    LRC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, kTBlock, lds));
    LRC_HIP(hipFuncGetAttributes(&attr, kernel));
    if (waves_per_cu) *waves_per_cu = blocks * (kTBlock / 64);
    if (vgprs) *vgprs = attr.numRegs;
    if (lds_bytes) *lds_bytes = (int)lds;
    return LRC_OK;
}

// The TraceParams fields every scan fills alike: `total` rays in poses of `rays_per_pose` (at least 1: the kernel divides by
// it), the range filter about the pose centres and, where the caller has one, the record set to write.
static void scan_fields(TraceParams& p, uint64_t rays_per_pose, uint64_t total, double max_range, const lrc_hits* out,
                        bool has_center = true) {
    p.rays_per_pose = rays_per_pose ? rays_per_pose : 1;
    p.total = total;
    p.has_center = has_center;
    p.max_range = max_range;
    if (out) p.out = *out;
}

int lrc_cast_dev(lrc_scene* s, const float* d_rays6, uint64_t n, const double* center3,
                 double max_range, const lrc_hits* d_out, void* stream) {
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_cast_dev: NULL scene or output");
    if (n && !d_rays6) return fail(LRC_ERR_INVALID_ARG, "lrc_cast_dev: rays6 is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    p.rays6 = d_rays6;
    scan_fields(p, n, n, max_range, d_out, center3 != nullptr);
    if (center3) { p.cx = center3[0]; p.cy = center3[1]; p.cz = center3[2]; }
    return launch_trace(s, p, kGenRays, (hipStream_t)stream);
}

int lrc_cast_segments_dev(lrc_scene* s, const float* d_rays6, uint64_t n, const uint64_t* d_seg_offsets,
                          uint64_t num_segments, const double* d_centers3, double max_range,
                          const lrc_hits* d_out, void* stream) {
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_cast_segments_dev: NULL scene or output");
    if (n && (!d_rays6 || !d_seg_offsets || !d_centers3 || num_segments == 0))
        return fail(LRC_ERR_INVALID_ARG, "lrc_cast_segments_dev: NULL rays, offsets or centres");
    if (num_segments > 0x7FFFFFFFull) return fail(LRC_ERR_INVALID_ARG, "lrc_cast_segments_dev: too many segments");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    p.rays6 = d_rays6;
    p.seg_offsets = d_seg_offsets;
    p.seg_centers3 = d_centers3;
    p.num_segments = (uint32_t)num_segments;
    scan_fields(p, n, n, max_range, d_out);
    return launch_trace(s, p, kGenRays, (hipStream_t)stream);
}

int lrc_scan_poses_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3,
                       uint64_t N, double max_range, const lrc_hits* d_out, void* stream) {
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_poses_dev: NULL scene or output");
    if (P && N && (!d_poses16 || !d_dirs3))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_poses_dev: poses16 or dirs3 is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    p.poses16 = d_poses16;
    p.dirs3 = d_dirs3;
    scan_fields(p, N, P * N, max_range, d_out);
    return launch_trace(s, p, kGenPoses, (hipStream_t)stream);
}

int lrc_scan_sweeps_dev(lrc_scene* s, const double* d_motion24, uint64_t P, const double* d_dirs3, const double* d_fire,
                        uint64_t N, double max_range, const lrc_hits* d_out, void* stream) {
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_sweeps_dev: NULL scene or output");
    if (P && N && (!d_motion24 || !d_dirs3 || !d_fire))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_sweeps_dev: motion24, dirs3 or fire is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    p.motion24 = d_motion24;
    p.dirs3 = d_dirs3;
    p.fire = d_fire;
    scan_fields(p, N, P * N, max_range, d_out);
    return launch_trace(s, p, kGenSweeps, (hipStream_t)stream);
}

int lrc_scan_noisy_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N, double max_range,
                       const lrc_noise* noise, const lrc_hits* d_out, void* stream) {
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_dev: NULL scene or output");
    if (P && N && (!d_poses16 || !d_dirs3))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_dev: poses16 or dirs3 is NULL");
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_dev: a range_noise option is set (one noise source per call)");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    int rc = noise_params(s->ctx, "lrc_scan_noisy_dev", noise, N, &p.noise);
    if (rc) return rc;
    p.poses16 = d_poses16;
    p.dirs3 = d_dirs3;
    scan_fields(p, N, P * N, max_range, d_out);
    return launch_trace(s, p, kGenNoisy, (hipStream_t)stream);
}

int lrc_scan_noisy_sweeps_dev(lrc_scene* s, const double* d_motion24, uint64_t P, const double* d_dirs3, uint64_t N,
                              const double* d_fire, double max_range, const lrc_noise* noise, const lrc_hits* d_out, void* stream) {
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_sweeps_dev: NULL scene or output");
    if (P && N && (!d_motion24 || !d_dirs3 || !d_fire))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_sweeps_dev: motion24, dirs3 or fire is NULL");
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_sweeps_dev: a range_noise option is set (one noise source per call)");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    int rc = noise_params(s->ctx, "lrc_scan_noisy_sweeps_dev", noise, N, &p.noise);
    if (rc) return rc;
    p.motion24 = d_motion24;
    p.dirs3 = d_dirs3;
    p.fire = d_fire;
    scan_fields(p, N, P * N, max_range, d_out);
    return launch_trace(s, p, kGenNoisySweeps, (hipStream_t)stream);
}

int lrc_scan_angles_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_angles2,
                        const uint8_t* d_keep, uint64_t N, double max_range, const lrc_hits* d_out, void* stream) {
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_angles_dev: NULL scene or output");
    if (P && N && (!d_poses16 || !d_angles2))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_angles_dev: poses16 or angles2 is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    p.poses16 = d_poses16;
    p.angles2 = d_angles2;
    p.keep_mask = d_keep;
    scan_fields(p, N, P * N, max_range, d_out);
    return launch_trace(s, p, kGenAngles, (hipStream_t)stream);
}

static int check_grid(const char* who, const lrc_grid* g, uint64_t N) {
    auto bad = [&](const char* m) { return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + m); };
    if (!g) return bad("grid is NULL");
    if (g->lines == 0 || g->width == 0 || (uint64_t)g->lines * g->width != N) return bad("lines * width != rays_per_pose");
    if (g->width % 64 || g->width < 256) return bad("the packet kernel needs width % 64 == 0 and width >= 256");
    if (!(std::fabs(g->az_step) > 0.0) || std::fabs(std::fabs(g->az_step) * g->width - 6.283185307179586) > 1e-6)
        return bad("az_step must cover one turn: |az_step| * width = 2 pi");
    return LRC_OK;
}

int lrc_scan_grid_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, const lrc_grid* grid,
                      double max_range, const lrc_hits* d_out, void* stream) {
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_grid_dev: NULL scene or output");
    if (!grid) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_grid_dev: grid is NULL");
    const uint64_t N = (uint64_t)grid->lines * grid->width;
    int rc = check_grid("lrc_scan_grid_dev", grid, N);
    if (rc) return rc;
    if (P && (!d_poses16 || !d_dirs3)) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_grid_dev: poses16 or dirs3 is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    p.poses16 = d_poses16;
    p.dirs3 = d_dirs3;
    scan_fields(p, N, P * N, max_range, d_out);
    s->cur_grid = grid;
    rc = launch_trace(s, p, kGenGrid, (hipStream_t)stream);
    s->cur_grid = nullptr;
    return rc;
}

}  // extern "C"

// The trace launch of lrc_scan_echoes_dev, whose arguments lrc_echo.hip has checked (declared in lrc_internal.h): ep.offsets2 and
// ep.weight are device pointers, d_out holds P * N * E records.
int echo_scan_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N, const lrcecho::Params& ep,
                  double max_range, const lrc_hits* d_out, hipStream_t st) {
    TraceParams p{};
    p.poses16 = d_poses16;
    p.dirs3 = d_dirs3;
    p.echo = ep;
    scan_fields(p, N * ep.max_echoes, P * N * ep.max_echoes, max_range, d_out);
    return launch_trace(s, p, kGenEchoes, st);
}

// The trace launch of lrc_scan_materials_dev, whose arguments lrc_material.hip has checked (declared in lrc_internal.h): mp.table,
// mp.bounces and mp.surface3 are device pointers, d_out holds P * N records.
int material_scan_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N, const lrcmat::Params& mp,
                      double max_range, const lrc_hits* d_out, hipStream_t st) {
    TraceParams p{};
    p.poses16 = d_poses16;
    p.dirs3 = d_dirs3;
    p.mat = mp;
    scan_fields(p, N, P * N, max_range, d_out);
    return launch_trace(s, p, kGenMaterials, st);
}

// ---- host-pointer convenience wrappers ---------------------------------------------------------
namespace {
// The per-ray columns of lrc_hits that the host-pointer entry points stage, listed ONCE: f(member, elements per ray, slot of
// the context's staging pool).  The element size is the member's pointer type's.  (t_label and tile_count exist on the
// device entry points only.)
template <class F>
int hits_columns(F&& f) {
    int rc;
    if ((rc = f(&lrc_hits::t, 1, kPoolT)) || (rc = f(&lrc_hits::prim, 1, kPoolPrim)) ||
        (rc = f(&lrc_hits::normal3, 3, kPoolNormal)) || (rc = f(&lrc_hits::point3, 3, kPoolPoint)) ||
        (rc = f(&lrc_hits::sem, 1, kPoolSem)) || (rc = f(&lrc_hits::ins, 1, kPoolIns)) ||
        (rc = f(&lrc_hits::incident_deg, 1, kPoolInc)) || (rc = f(&lrc_hits::intensity, 1, kPoolInten)))
        return rc;
    return LRC_OK;
}
// The columns a compaction reads, listed ONCE: f(record array of lrc_hits, input array of lrc_compact_io, elements per ray).
template <class F>
int record_columns(F&& f) {
    int rc;
    if ((rc = f(&lrc_hits::t, &lrc_compact_io::t, 1)) || (rc = f(&lrc_hits::point3, &lrc_compact_io::point3, 3)) ||
        (rc = f(&lrc_hits::sem, &lrc_compact_io::sem, 1)) || (rc = f(&lrc_hits::ins, &lrc_compact_io::ins, 1)) ||
        (rc = f(&lrc_hits::incident_deg, &lrc_compact_io::incident_deg, 1)))
        return rc;
    return LRC_OK;
}
// The compacted columns of a frame, listed ONCE: f(array of lrc_frames, output array of lrc_compact_io, elements per row).
// A new column is a line here, its allocation in FrameStage::alloc and its store in the scatter kernels.
template <class F>
int frame_columns(F&& f) {
    int rc;
    if ((rc = f(&lrc_frames::point3, &lrc_compact_io::out_point3, 3)) || (rc = f(&lrc_frames::sem, &lrc_compact_io::out_sem, 1)) ||
        (rc = f(&lrc_frames::ins, &lrc_compact_io::out_ins, 1)) ||
        (rc = f(&lrc_frames::incident_deg, &lrc_compact_io::out_incident_deg, 1)) ||
        (rc = f(&lrc_frames::index, &lrc_compact_io::out_index, 1)) || (rc = f(&lrc_frames::xyzl, &lrc_compact_io::out_xyzl, 4)) ||
        (rc = f(&lrc_frames::range_origin, &lrc_compact_io::out_range_origin, 1)))
        return rc;
    return LRC_OK;
}
// device arrays (context pool) for the columns of `h` the caller asked for, and their way home
struct HitsStage {
    lrc_hits d{};
    int alloc(lrc_ctx* ctx, const lrc_hits& h, uint64_t n) {
        if (!n) return LRC_OK;
        return hits_columns([&](auto col, size_t per_ray, int slot) -> int {
            if (!(h.*col)) return LRC_OK;
            DevBuf b;      // a pool slot: the context keeps it
            int rc = b.get(ctx, slot, n * per_ray * sizeof(*(h.*col)));
            if (rc) return rc;
            d.*col = static_cast<std::remove_reference_t<decltype(d.*col)>>(b.p);
            return LRC_OK;
        });
    }
    int download(const lrc_hits& h, uint64_t n) {
        if (!n) return LRC_OK;
        return hits_columns([&](auto col, size_t per_ray, int) -> int {
            if (h.*col) LRC_HIP(hipMemcpy(h.*col, d.*col, n * per_ray * sizeof(*(h.*col)), hipMemcpyDeviceToHost));
            return LRC_OK;
        });
    }
};
// host entry points: lrc_scan_options.range_noise is a HOST array; stage it in HBM for the call
struct NoiseStage {
    lrc_scene* s = nullptr;
    const float* host = nullptr;
    DevBuf buf;
    int begin(lrc_scene* scene, uint64_t n) {
        if (!scene->opts.range_noise) return LRC_OK;
        if (scene->opts.range_noise_len != n)
            return fail(LRC_ERR_INVALID_ARG, "range_noise_len does not match the number of rays of this call");
        int rc = buf.get(scene->ctx, kPoolNoise, n * 4);
        if (rc) return rc;
        LRC_HIP(hipMemcpy(buf.p, scene->opts.range_noise, n * 4, hipMemcpyHostToDevice));
        s = scene;
        host = scene->opts.range_noise;
        scene->opts.range_noise = (const float*)buf.p;
        return LRC_OK;
    }
    ~NoiseStage() { if (s) s->opts.range_noise = host; }
};
// An input array of a host-pointer entry point: `count` elements into slot `slot` of the context's staging pool, copied
// there before this returns or, with `async`, on that stream (the one that consumes them).
template <class T>
int stage_input(lrc_ctx* ctx, int slot, const T* host, size_t count, const T** dev, const hipStream_t* async = nullptr) {
    DevBuf b;      // a pool slot: the context keeps it
    int rc = b.get(ctx, slot, count * sizeof(T));
    if (rc) return rc;
    if (async) LRC_HIP(hipMemcpyAsync(b.p, host, count * sizeof(T), hipMemcpyHostToDevice, *async));
    else LRC_HIP(hipMemcpy(b.p, host, count * sizeof(T), hipMemcpyHostToDevice));
    *dev = static_cast<const T*>(b.p);
    return LRC_OK;
}
// What lrc_cast, lrc_cast_segments and lrc_scan_poses share around their *_dev call: device arrays for the columns asked
// for and the scene's host noise array staged for the call (restored on every exit), then -- when the call went through --
// one synchronisation and the columns brought home.
struct HostScan {
    HitsStage st;
    NoiseStage ns;
    int begin(lrc_scene* s, const lrc_hits& out, uint64_t n) {
        int rc = st.alloc(s->ctx, out, n);
        return rc ? rc : ns.begin(s, n);
    }
    int finish(int rc, const lrc_hits& out, uint64_t n) {
        if (rc) return rc;
        LRC_HIP(hipDeviceSynchronize());
        return st.download(out, n);
    }
};
}  // namespace

extern "C" {

int lrc_cast(lrc_scene* s, const float* rays6, uint64_t n, const double* center3, double max_range,
             const lrc_hits* out) {
    if (!s || !out) return fail(LRC_ERR_INVALID_ARG, "lrc_cast: NULL scene or output");
    if (n && !rays6) return fail(LRC_ERR_INVALID_ARG, "lrc_cast: rays6 is NULL");
    if (!n) return LRC_OK;
    LRC_HIP(hipSetDevice(s->ctx->device));
    const float* d_rays = nullptr;
    int rc = stage_input(s->ctx, kPoolRays, rays6, n * 6, &d_rays);
    if (rc) return rc;
    HostScan hs;
    if ((rc = hs.begin(s, *out, n))) return rc;
    return hs.finish(lrc_cast_dev(s, d_rays, n, center3, max_range, &hs.st.d, nullptr), *out, n);
}

int lrc_cast_segments(lrc_scene* s, const float* rays6, uint64_t n, const uint64_t* seg_offsets,
                      uint64_t num_segments, const double* centers3, double max_range, const lrc_hits* out) {
    if (!s || !out) return fail(LRC_ERR_INVALID_ARG, "lrc_cast_segments: NULL scene or output");
    if (!n) return LRC_OK;
    if (!rays6 || !seg_offsets || !centers3 || num_segments == 0)
        return fail(LRC_ERR_INVALID_ARG, "lrc_cast_segments: NULL rays, offsets or centres");
    if (seg_offsets[0] != 0 || seg_offsets[num_segments] != n)
        return fail(LRC_ERR_INVALID_ARG, "lrc_cast_segments: offsets must start at 0 and end at num_rays");
    for (uint64_t k = 0; k < num_segments; ++k)
        if (seg_offsets[k] > seg_offsets[k + 1])
            return fail(LRC_ERR_INVALID_ARG, "lrc_cast_segments: offsets must be non-decreasing");
    LRC_HIP(hipSetDevice(s->ctx->device));
    const float* d_rays = nullptr;
    const uint64_t* d_offs = nullptr;
    const double* d_cen = nullptr;
    int rc;
    if ((rc = stage_input(s->ctx, kPoolRays, rays6, n * 6, &d_rays)) ||
        (rc = stage_input(s->ctx, kPoolOffs, seg_offsets, num_segments + 1, &d_offs)) ||
        (rc = stage_input(s->ctx, kPoolCen, centers3, num_segments * 3, &d_cen)))
        return rc;
    HostScan hs;
    if ((rc = hs.begin(s, *out, n))) return rc;
    return hs.finish(lrc_cast_segments_dev(s, d_rays, n, d_offs, num_segments, d_cen, max_range, &hs.st.d, nullptr), *out, n);
}

int lrc_scan_poses(lrc_scene* s, const double* poses16, uint64_t P, const double* dirs3, uint64_t N,
                   double max_range, const lrc_hits* out) {
    if (!s || !out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_poses: NULL scene or output");
    if (P && N && (!poses16 || !dirs3))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_poses: poses16 or dirs3 is NULL");
    const uint64_t n = P * N;
    if (!n) return LRC_OK;
    LRC_HIP(hipSetDevice(s->ctx->device));
    const double *d_poses = nullptr, *d_dirs = nullptr;
    int rc;
    if ((rc = stage_input(s->ctx, kPoolPoses, poses16, P * 16, &d_poses)) ||
        (rc = stage_input(s->ctx, kPoolDirs, dirs3, N * 3, &d_dirs)))
        return rc;
    HostScan hs;
    if ((rc = hs.begin(s, *out, n))) return rc;
    return hs.finish(lrc_scan_poses_dev(s, d_poses, P, d_dirs, N, max_range, &hs.st.d, nullptr), *out, n);
}

// ---- compaction: tile scratch, the scan chain, lrc_compact_dev ---------------------------------------------------------
// the grid of a kBlock kernel that gives every tile of 64 entries one wave
static uint64_t tile_blocks(uint64_t ntiles) { return blocks_of(ntiles, kBlock / 64); }

// Scratch for `ntiles` tiles.  Growing frees the old arrays -- the transposed direction table too: both its users make it
// again behind this call -- so the caller has made the device current and nothing may still read them.
static int ensure_tile_scratch(lrc_ctx::TileScratch& sc, uint64_t ntiles) {
    if (sc.tile_cap >= ntiles + 1) return LRC_OK;
    sc.release();
    const uint64_t nsuper = blocks_of(ntiles, 1024);
    LRC_HIP(hipMalloc((void**)&sc.d_tile_off, (ntiles + 1) * 4));
    LRC_HIP(hipMalloc((void**)&sc.d_tile_cnt, (ntiles + 1) * 4));
    LRC_HIP(hipMalloc((void**)&sc.d_super_total, (nsuper + 1) * 4));
    LRC_HIP(hipMalloc((void**)&sc.d_super_base, (nsuper + 1) * 8));
    sc.tile_cap = ntiles + 1;
    return LRC_OK;
}

// The scratch set of a compaction on stream `st`: the one that stream used last; otherwise the next set in turn, ordered
// behind whatever another stream may still be doing with it (an event wait; free when that work is long done).
static int compact_scratch_for(lrc_ctx* ctx, hipStream_t st, uint64_t ntiles, int* out_set) {
    int set = -1;
    for (int k = 0; k < lrc_ctx::kCompactSets; ++k)
        if (ctx->compact_used[k] && ctx->compact_stream[k] == st) { set = k; break; }
    if (set < 0) {
        set = ctx->compact_next;
        ctx->compact_next = (ctx->compact_next + 1) % lrc_ctx::kCompactSets;
        if (!ctx->compact_done[set]) LRC_HIP(hipEventCreateWithFlags(&ctx->compact_done[set], hipEventDisableTiming));
        else if (ctx->compact_used[set]) LRC_HIP(hipStreamWaitEvent(st, ctx->compact_done[set], 0));
        ctx->compact_stream[set] = st;
        ctx->compact_used[set] = true;
    }
    lrc_ctx::TileScratch& sc = ctx->compact_scratch[set];
    if (sc.tile_cap < ntiles + 1 && sc.d_tile_off) {
        // growing frees the old arrays: whatever still reads them must be done first
        LRC_HIP(hipEventSynchronize(ctx->compact_done[set]));
    }
    *out_set = set;
    return ensure_tile_scratch(sc, ntiles);
}

// The scan chain on `st`: per-tile keep counts `cnt` (tiles_per_slab of them every slab_stride words; stride 0: one run) ->
// sc's offsets inside super tiles of 1024 tiles and the super tiles' totals, and, with `bases`, the totals' exclusive prefix
// (a scatter over few super tiles sums the totals in front of it itself).
static void launch_scan_chain(lrc_ctx::TileScratch& sc, const uint32_t* cnt, uint64_t tiles_per_slab, uint64_t slab_stride,
                              uint64_t ntiles, bool bases, hipStream_t st) {
    const uint64_t nsuper = blocks_of(ntiles, 1024);
    hipLaunchKernelGGL(compact_scan_kernel, dim3((uint32_t)nsuper), dim3(64), 0, st, cnt, tiles_per_slab, slab_stride,
                       sc.d_tile_off, ntiles, sc.d_super_total);
    if (bases)
        hipLaunchKernelGGL(compact_base_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)sc.d_super_total,
                           sc.d_super_base, nsuper);
}

// the launches of a compaction on stream `st` with scratch set `sc` (sized by the caller for nseg * ceil(seg_len / 64) tiles)
static int enqueue_compaction(lrc_ctx::TileScratch& sc, uint64_t nseg, uint64_t seg_len, const lrc_compact_io* io, hipStream_t st) {
    const uint64_t tps = blocks_of(seg_len, 64);
    const uint64_t ntiles = nseg * tps;
    const uint64_t nblocks = tile_blocks(ntiles);
    // the trace kernel can hand over its per-wave keep counts (lrc_hits.tile_count) when tiles line up
    const uint32_t* cnt = (io->tile_count && seg_len % 64 == 0) ? io->tile_count : nullptr;
    if (!cnt) {
        hipLaunchKernelGGL(compact_count_kernel, dim3((uint32_t)nblocks), dim3(kBlock), 0, st, io->t, seg_len,
                           tps, ntiles, sc.d_tile_cnt);
        cnt = sc.d_tile_cnt;
    }
    // few super tiles (a C3 scan has 64): every scatter wave sums the totals in front of it itself, one launch less
    const bool inline_bases = blocks_of(ntiles, 1024) <= 512;
    launch_scan_chain(sc, cnt, ntiles, 0, ntiles, !inline_bases, st);
    // the scatter grid must also cover the threads that write the per-segment counts (one per segment)
    const uint64_t need = io->counts ? blocks_of(nseg, kBlock) : 0;
    const uint64_t grid = nblocks > need ? nblocks : need;
    hipLaunchKernelGGL(compact_scatter_kernel, dim3((uint32_t)grid), dim3(kBlock), 0, st, *io, seg_len, tps,
                       ntiles, nseg, (const uint32_t*)sc.d_tile_off, (const uint64_t*)sc.d_super_base, (uint64_t)0,
                       inline_bases ? (const uint32_t*)sc.d_super_total : (const uint32_t*)nullptr);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

// The rebuild of a gathered scan's rows from its triangle ids: one wave per LRC_REBUILD_R tiles.
static void launch_prim_scatter(const RebuildParams& q, hipStream_t st) {
    constexpr int kR = LRC_REBUILD_R;
    const uint64_t wblocks = tile_blocks(blocks_of(q.ntiles, kR));
    hipLaunchKernelGGL(prim_scatter_kernel<kR>, dim3((uint32_t)(wblocks ? wblocks : 1)), dim3(kBlock), 0, st, q);
}
// ... and the rows of the rank's own poses (own_tiles tiles, tps per pose), straight from its local records `io` to the
// offsets the rebuild's scan gave them; tile_base: the own slab's first tile in the assembled cloud.
static void launch_own_rows(const lrc_compact_io& io, uint64_t N, uint64_t tps, uint64_t own_tiles, const RebuildParams& q,
                            uint64_t tile_base, hipStream_t st) {
    const uint64_t nblocks = tile_blocks(own_tiles);
    if (nblocks)
        hipLaunchKernelGGL(compact_scatter_kernel, dim3((uint32_t)nblocks), dim3(kBlock), 0, st, io, N, tps, own_tiles, own_tiles / tps,
                           (const uint32_t*)q.tile_off, (const uint64_t*)q.super_base, tile_base, (const uint32_t*)nullptr);
}

int lrc_compact_dev(lrc_ctx* ctx, uint64_t nseg, uint64_t seg_len, const lrc_compact_io* io,
                    void* stream) {
    if (!ctx || !io) return fail(LRC_ERR_INVALID_ARG, "lrc_compact_dev: NULL argument");
    if (nseg == 0 || seg_len == 0) return LRC_OK;
    if (!io->t) return fail(LRC_ERR_INVALID_ARG, "lrc_compact_dev: t is NULL");
    if (((io->out_point3 || io->out_xyzl || io->out_range_origin) && !io->point3) || (io->out_sem && !io->sem) ||
        (io->out_ins && !io->ins) || (io->out_incident_deg && !io->incident_deg))
        return fail(LRC_ERR_INVALID_ARG, "lrc_compact_dev: an output is requested without its input");
    LRC_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const uint64_t ntiles = nseg * blocks_of(seg_len, 64);
    if (tile_blocks(ntiles) > 0x7FFFFFFFull) return fail(LRC_ERR_INVALID_ARG, "lrc_compact_dev: too many entries");
    int set = -1;
    int rc = compact_scratch_for(ctx, st, ntiles, &set);
    if (rc) return rc;
    if ((rc = enqueue_compaction(ctx->compact_scratch[set], nseg, seg_len, io, st))) return rc;
    LRC_HIP(hipEventRecord(ctx->compact_done[set], st));
    return LRC_OK;
}

// ---- the scan pipeline (include/lidarcast.h: lrc_pipe_*) ---------------------------------------------------------------------
// Consecutive pose batches of one scene, scanned and compacted with the launches overlapped INSIDE the library.
// What the measurements of round 4 say about this chip (DESIGN.md "the launch tail"; profiles/r04_chain_timeline_before.txt,
// r04_queue_share.txt, r04_pipe_arrangements.txt):
//   * a trace launch -- 65 536 one-wave workgroups that take a wave slot the moment it is freed -- keeps the dispatcher to
//     itself while it has workgroups left: another stream's kernel gets a trickle of slots if its workgroups are one wave
//     (a 32-workgroup kernel: 30-160 us) and none at all if they are 4 or 16 waves.  When the launch has handed out its
//     last workgroup the next READY kernel of any stream takes over, into the slots the launch's long last waves leave
//     empty (a 64-pose launch alone loses 50-60 us to that tail).
//   * so two trace launches on two streams with NOTHING between two launches of a stream overlap perfectly (+12 %), and
//     the moment a compaction sits between them (trace -> scan -> scatter -> trace per stream) it waits for the OTHER
//     stream's whole dispatch phase, the trace behind it waits too, and the two chains run in lock step (+0...6 %).
// Hence: trace launches of consecutive submits alternate between two streams; the 32-workgroup scan pass of submit k sits
// behind its trace (it trickles in during the other stream's launch, nothing waits for it); and the scatter of submit k is not
// a launch at all: it rides at the FRONT of the trace launch of submit k+2 (same stream, TraceParams::pre: one tile per
// one-wave workgroup), so it is handed out exactly when the previous launch's tail begins and is gone in microseconds.  Four
// record sets: set k is read by launch k+2 and written again by launch k+4, both on its own stream.
// A fused submit writes a set's LEAN form: per ray the record (t, label, slot), 12 B, per tile the keep mask -- one store
// per ray instead of ten, no triangle id and no normal in the trace, and no point: the consumers form the output row from the
// record and the set's ray table (LeanIn; a wave that did not take the table stores its 16-byte row as well; DESIGN.md section
// 5.2).  The complete 36-byte record, in arrays of its own beside the lean ones, is what the plain fallback and the sharded
// submits write, and what lrc_pipe_records expands a lean set into on demand.
#ifndef LRC_PIPE_TILE_LINES
#define LRC_PIPE_TILE_LINES 4      // lines per tile of an automatic submit (profiles/trace_line_group_tiles.txt)
#endif
#ifndef LRC_PIPE_SCAN_WAVES
#define LRC_PIPE_SCAN_WAVES 64     // waves of a submit's scan pass: one per super tile up to this (lrc_pipe_submit says why)
#endif
struct lrc_pipe {
    lrc_scene* scene = nullptr;
    int device = 0;
    uint64_t max_poses = 0, rays_per_pose = 0, cap = 0;      // cap = max_poses * rays_per_pose records per set
    static constexpr int kSets = 4;
    void* slab[kSets] = {};                                  // one allocation per record set
    lrc_hits rec[kSets] = {};
    uint32_t* rec3[kSets] = {};                              // the lean form (rec3, row, keep_mask; tile_count is rec's)
    float4* row[kSets] = {};                                 // ... its rows: written by the waves that took no table row only
    uint64_t* keep_mask[kSets] = {};
    bool lean[kSets] = {};                                   // the set holds its last submit in the lean form ...
    bool expanded[kSets] = {};                               // ... and lrc_pipe_records has rebuilt rec from it
    lrc_compact_io out[kSets] = {};                          // the caller's output buffers of the submit that used the set
    uint64_t poses[kSets] = {};                              // its pose count
    bool pending[kSets] = {};                                // scanned, scan pass enqueued, rows not yet scattered
    lrc_ctx::TileScratch scratch[2];                         // per trace stream: offsets of the scan waiting for its scatter
    hipStream_t s_trace[2] = {};
    hipEvent_t ev_in[kSets] = {}, ev_t0[kSets] = {}, ev_trace[kSets] = {}, ev_flush[2] = {}, ev_expand = nullptr;
    bool fused = true;                                       // false: N % 64 != 0 or > 512 super tiles: plain chain per stream
    uint64_t ticket = 0;                                     // submits so far; submit k uses set k % 4, trace stream k % 2
    // sharded submits (lrc_pipe_submit_sharded): per scan slot the scan over ALL ranks' keep counts and the direction table
    // transposed for the rebuild (TileScratch::d_dirs_soa, written by every lrc_pipe_scan_gathered of that slot)
    lrc_ctx::TileScratch gscratch[2];
    // per set: the ticket of the last trace launch that read the set's records as the own rows of an assembly (0: none).  The
    // submit that writes the set again waits for that launch when it runs on the other trace stream.
    uint64_t read_by[kSets] = {};
    // two-line tiles (lrc_pipe_set_line_width; lrc_device.h, tile_ray): the caller's hint, or, automatic, the width detected on
    // the first submit of a table address the pipeline has not seen (one one-wave kernel and a 4-byte read-back, then nothing)
    uint64_t line_hint = 0;                                  // 0: automatic
    const double* line_table = nullptr;                      // the table line_auto was detected on
    uint32_t line_auto = 0;                                  // its line width in tiles, 0: 1-D tiles
    uint32_t* d_line = nullptr;
    uint32_t line_last = 0;                                  // line width in tiles the last submit's launch ran with
    // line-group tiles (lrc_pipe_set_tile_lines): lines per tile asked for (0: automatic = 4 where the table has a group of
    // four), the split line detected with line_auto, and what the last launch ran with
    uint32_t lines_hint = 0, split_auto = 0, lines_last = 1, group_last = 0;
    // prepared submits (lrc_pipe_set_ray_table; ray_table_kernel): one ray table per record set, because the set's records are
    // read against it.  Table k % 4 is written by the ray_table_kernel of submit k, read by trace k, by the leading workgroups
    // of launch k + 2, by lrc_pipe_wait's plain scatter and by lrc_pipe_records' expansion, and written again by submit k + 4.
    // Every one of these is enqueued on trace stream k % 2 (k, k + 2 and k + 4 share it), in this order, so stream order alone
    // keeps the table from being rewritten while anything reads it.  NULL: not a fused pipeline, or more rows than kRayTabMaxRows.
    float4* ray_tab[kSets] = {};
    bool tabbed[kSets] = {};                                 // the set's last submit carried its table (LeanIn::tab)
    bool use_ray_tab = true;
    bool ray_tab_last = false;                               // the last submit's launch carried a table
};

int lrc_pipe_destroy(lrc_pipe* pp) {
    if (!pp) return LRC_OK;
    (void)hipSetDevice(pp->device);
    for (hipStream_t st : {pp->s_trace[0], pp->s_trace[1]})
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (int k = 0; k < lrc_pipe::kSets; ++k) {
        if (pp->slab[k]) (void)hipFree(pp->slab[k]);
        for (hipEvent_t e : {pp->ev_in[k], pp->ev_t0[k], pp->ev_trace[k]}) if (e) (void)hipEventDestroy(e);
    }
    if (pp->ev_expand) (void)hipEventDestroy(pp->ev_expand);
    if (pp->d_line) (void)hipFree(pp->d_line);
    for (int k = 0; k < lrc_pipe::kSets; ++k)
        if (pp->ray_tab[k]) (void)hipFree(pp->ray_tab[k]);
    for (int k = 0; k < 2; ++k) {
        if (pp->ev_flush[k]) (void)hipEventDestroy(pp->ev_flush[k]);
        pp->scratch[k].release();        // (the pipeline's device is current: above)
        pp->gscratch[k].release();
    }
    delete pp;
    return LRC_OK;
}

int lrc_pipe_create(lrc_scene* s, uint64_t max_poses, uint64_t rays_per_pose, lrc_pipe** out_pipe) {
    if (!out_pipe) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_create: out_pipe is NULL");
    *out_pipe = nullptr;
    if (!s) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_create: scene is NULL");
    if (max_poses == 0 || rays_per_pose == 0) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_create: max_poses and rays_per_pose must be positive");
    if (max_poses > 0x7FFFFFFFull || max_poses * rays_per_pose / rays_per_pose != max_poses || max_poses * rays_per_pose > (1ull << 36))
        return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_create: batch too large");
    LRC_HIP(hipSetDevice(s->ctx->device));
    lrc_pipe* pp = new (std::nothrow) lrc_pipe();
    if (!pp) return fail(LRC_ERR_OOM, "lrc_pipe_create: out of host memory");
    pp->scene = s;
    pp->device = s->ctx->device;
    pp->max_poses = max_poses;
    pp->rays_per_pose = rays_per_pose;
    const uint64_t n = pp->cap = max_poses * rays_per_pose;
    const uint64_t tiles = max_poses * blocks_of(rays_per_pose, 64);
    pp->fused = rays_per_pose % 64 == 0 && blocks_of(tiles, 1024) <= 512;
    auto bail = [&](int rc) { (void)lrc_pipe_destroy(pp); return rc; };
    auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
    // a record set: t | prim | normal3 | point3 | sem | ins | tile_count, 36 B per ray + 4 B per 64 rays, and for a fused
    // pipeline beside it the lean form row | rec3 | keep_mask, 16 + 12 B per ray + 8 B per 64 rays
    const uint64_t off_t = 0, off_prim = off_t + up(4 * n), off_nrm = off_prim + up(4 * n), off_pt = off_nrm + up(12 * n),
                   off_sem = off_pt + up(12 * n), off_ins = off_sem + up(2 * n), off_tc = off_ins + up(2 * n),
                   off_row = off_tc + up(4 * ((n + 63) / 64)), off_rec3 = off_row + (pp->fused ? up(16 * n) : 0),
                   off_km = off_rec3 + (pp->fused ? up(12 * n) : 0), bytes = off_km + (pp->fused ? up(8 * ((n + 63) / 64)) : 0);
    for (int k = 0; k < lrc_pipe::kSets; ++k) {
        hipError_t e = hipMalloc(&pp->slab[k], bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); return bail(fail(LRC_ERR_OOM, "lrc_pipe_create: out of device memory for the record sets")); }
        char* b = (char*)pp->slab[k];
        lrc_hits& h = pp->rec[k];
        h.t = (float*)(b + off_t); h.prim = (uint32_t*)(b + off_prim); h.normal3 = (float*)(b + off_nrm);
        h.point3 = (float*)(b + off_pt); h.sem = (uint16_t*)(b + off_sem); h.ins = (uint16_t*)(b + off_ins);
        h.tile_count = (uint32_t*)(b + off_tc);
        if (pp->fused) {
            pp->row[k] = (float4*)(b + off_row); pp->rec3[k] = (uint32_t*)(b + off_rec3); pp->keep_mask[k] = (uint64_t*)(b + off_km);
        }
    }
    // The two trace streams must reach the hardware on queues of their own, or their launches cannot overlap.  The runtime
    // shares a bounded pool of hardware queues per stream priority among all of the process's streams (GPU_MAX_HW_QUEUES,
    // 2 on some systems: then both trace streams landed on one queue behind each other and the pipelined step was 2-4 %
    // SLOWER than the two calls, profiles/pipe_two_hw_queues.txt).  At the least priority they draw from a pool the
    // process's normal-priority streams do not use, and everything else the caller submits keeps precedence.
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) return bail(fail(LRC_ERR_HIP, "lrc_pipe_create: stream priorities"));
    for (int k = 0; k < 2; ++k) {
        if (hipStreamCreateWithPriority(&pp->s_trace[k], hipStreamNonBlocking, prio_least) != hipSuccess) return bail(fail(LRC_ERR_HIP, "lrc_pipe_create: stream"));
        if (hipEventCreateWithFlags(&pp->ev_flush[k], hipEventDisableTiming) != hipSuccess) return bail(fail(LRC_ERR_HIP, "lrc_pipe_create: event"));
        int rc = ensure_tile_scratch(pp->scratch[k], tiles);
        if (rc) return bail(rc);
    }
    for (int k = 0; k < lrc_pipe::kSets; ++k) {
        if (hipEventCreateWithFlags(&pp->ev_in[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreate(&pp->ev_t0[k]) != hipSuccess || hipEventCreate(&pp->ev_trace[k]) != hipSuccess)
            return bail(fail(LRC_ERR_HIP, "lrc_pipe_create: event"));
    }
    if (hipEventCreateWithFlags(&pp->ev_expand, hipEventDisableTiming) != hipSuccess) return bail(fail(LRC_ERR_HIP, "lrc_pipe_create: event"));
    if (pp->fused && hipMalloc((void**)&pp->d_line, 2 * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); return bail(fail(LRC_ERR_OOM, "lrc_pipe_create: out of device memory")); }
    if (pp->fused && kTBlock == 64 && rays_per_pose <= kRayTabMaxRows)
        for (int k = 0; k < lrc_pipe::kSets; ++k)
            if (hipMalloc((void**)&pp->ray_tab[k], ray_tab_bytes(rays_per_pose, max_poses)) != hipSuccess) { (void)hipGetLastError(); return bail(fail(LRC_ERR_OOM, "lrc_pipe_create: out of device memory for the ray tables")); }
    *out_pipe = pp;
    return LRC_OK;
}

}  // extern "C"

namespace {
// the compaction input of the records in set `set`
lrc_compact_io pipe_io(const lrc_pipe* pp, int set) {
    lrc_compact_io io = pp->out[set];
    const lrc_hits& h = pp->rec[set];
    io.t = h.t; io.point3 = h.point3; io.sem = h.sem; io.ins = h.ins; io.incident_deg = nullptr; io.tile_count = h.tile_count;
    return io;
}
// ... and its lean form (row == NULL: the set holds complete records)
LeanIn pipe_lean(const lrc_pipe* pp, int set) {
    if (!pp->lean[set]) return LeanIn{nullptr, nullptr, nullptr, nullptr};
    return LeanIn{pp->rec3[set], pp->row[set], pp->keep_mask[set], pp->tabbed[set] ? pp->ray_tab[set] : nullptr};
}
// before the launch of a submit overwrites `set` on stream T: an assembly that read the set's own records in a launch on the
// OTHER trace stream (lag 1 or 3) is ordered before this launch only by dispatch, so T waits for that launch's event.  Lag 2
// shares T and is ordered already.  ev_trace of the reader is still its own: the reader came at most three submits earlier.
int wait_for_readers(lrc_pipe* pp, int set, hipStream_t T) {
    const uint64_t r = pp->read_by[set];
    if (r != 0 && pp->s_trace[(r - 1) % 2] != T) LRC_HIP(hipStreamWaitEvent(T, pp->ev_trace[(r - 1) % lrc_pipe::kSets], 0));
    pp->read_by[set] = 0;
    return LRC_OK;
}
}  // namespace

extern "C" {

// test hook (tests/test_pipe_two_line_gpu.py): the line width, in tiles of 64 rays, the trace launch of the pipeline's last
// lrc_pipe_submit ran with (0: 1-D tiles) -- the regrouping changes no byte, so no output can tell whether it happened
uint32_t lrc_internal_pipe_line_tiles(const lrc_pipe* pp) { return pp ? pp->line_last : 0u; }

// ... and its lines per tile (4, 2, or 1 for 1-D tiles) and line grouping word (lrc_device.h, tile_ray)
uint32_t lrc_internal_pipe_tile_lines(const lrc_pipe* pp) { return pp ? pp->lines_last : 0u; }
uint32_t lrc_internal_pipe_line_group(const lrc_pipe* pp) { return pp ? pp->group_last : 0u; }

int lrc_pipe_set_tile_lines(lrc_pipe* pp, uint32_t lines) {
    if (!pp) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_set_tile_lines: pipe is NULL");
    if (lines != 0u && lines != 1u && lines != 2u && lines != 4u) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_set_tile_lines: lines must be 0, 1, 2 or 4");
    pp->lines_hint = lines;
    return LRC_OK;
}

int lrc_pipe_set_ray_table(lrc_pipe* pp, int enable) {
    if (!pp) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_set_ray_table: pipe is NULL");
    if (enable != 0 && enable != 1) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_set_ray_table: enable must be 0 or 1");
    pp->use_ray_tab = enable != 0;
    return LRC_OK;
}

// test hook (tests/test_pipe_ray_table_gpu.py): the ray table the trace launch of the last lrc_pipe_submit carried (device
// pointer: 48 bytes per table row, then 64 per pose, see RayPose), or NULL -- the table changes no byte of the outputs, so only
// its own content can tell whether it was there and which poses took it
const void* lrc_internal_pipe_ray_table(const lrc_pipe* pp) {
    return pp && pp->ray_tab_last ? (const void*)pp->ray_tab[(pp->ticket - 1) % lrc_pipe::kSets] : nullptr;
}

int lrc_pipe_set_line_width(lrc_pipe* pp, uint64_t line_width) {
    if (!pp) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_set_line_width: pipe is NULL");
    pp->line_hint = line_width;
    pp->line_table = nullptr;      // a return to automatic detects again on the next submit
    return LRC_OK;
}

int lrc_pipe_submit(lrc_pipe* pp, const double* d_poses16, uint64_t P, const double* d_dirs3, double max_range,
                    const lrc_compact_io* d_out, void* stream, uint64_t* out_ticket) {
    if (!pp || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit: NULL pipe or output");
    if (P == 0) { if (out_ticket) *out_ticket = pp->ticket; return LRC_OK; }
    if (P > pp->max_poses) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit: more poses than the pipeline was created for");
    if (!d_poses16 || !d_dirs3) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit: poses16 or dirs3 is NULL");
    if (d_out->out_incident_deg) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit: the pipeline's records carry no incident angle");
    lrc_scene* s = pp->scene;
    LRC_HIP(hipSetDevice(s->ctx->device));
    const uint64_t k = pp->ticket;
    const int set = (int)(k % lrc_pipe::kSets), lane = (int)(k % 2);
    hipStream_t T = pp->s_trace[lane];
    // inputs (poses, table) and outputs (the caller's rows and counts) are the caller's as of this point of its stream
    LRC_HIP(hipEventRecord(pp->ev_in[set], (hipStream_t)stream));
    LRC_HIP(hipStreamWaitEvent(T, pp->ev_in[set], 0));
    int rc = wait_for_readers(pp, set, T);
    if (rc) return rc;
    const uint64_t N = pp->rays_per_pose;
    TraceParams p{};
    p.poses16 = d_poses16;
    p.dirs3 = d_dirs3;
    scan_fields(p, N, P * N, max_range, &pp->rec[set]);
    if (pp->fused) {           // the lean form: only what the scatter reads (the plain fallback below reads the full record)
        p.lean.row = pp->row[set]; p.lean.rec = pp->rec3[set]; p.lean.keep_mask = pp->keep_mask[set];
        // line-group tiles: the hinted line width, or the table's own, detected once per table address -- on the caller's
        // stream, whose position the table is valid at, with a 4-byte read-back; nothing afterwards.  A stale width (a new
        // table at a recycled address, a table edited in place) maps the rays as well as the right one: same bytes.
        if (pp->line_hint == 0 && pp->line_table != d_dirs3) {
            uint32_t w[2] = {0, 0};
            hipLaunchKernelGGL(first_line_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_dirs3, N, pp->d_line);
            LRC_HIP(hipGetLastError());
            LRC_HIP(hipMemcpyAsync(w, pp->d_line, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
            LRC_HIP(hipStreamSynchronize((hipStream_t)stream));
            pp->line_auto = line_tiles_for(w[0], N);
            pp->split_auto = w[1];
            pp->line_table = d_dirs3;
        }
        p.line_tiles = kTBlock == 64 && pp->lines_hint != 1u ? (pp->line_hint ? line_tiles_for(pp->line_hint, N) : pp->line_auto) : 0u;
        // line groups: of four lines unless two are asked for, on either side of the split detected with the width (a hinted
        // width has no detection behind it -- a hinted pipeline never synchronises -- and no split).  Where the table has no
        // group of four the word yields the two-line mapping.
        if (p.line_tiles != 0u)
            p.line_group = line_group_for(pp->line_hint == 0 ? pp->split_auto : 0u,
                                          pp->lines_hint == 0u ? (uint32_t)LRC_PIPE_TILE_LINES : pp->lines_hint);
    }
    // prepared submit: this set's ray table is rebuilt from THIS submit's poses and table, behind the scan pass of submit
    // k - 2 and in front of the trace (at most 64 one-wave workgroups: a few microseconds on an idle GPU, and beside the other
    // stream's launch they trickle in during a step that has nothing else for this stream to do)
    pp->ray_tab_last = false;
    if (pp->fused && pp->use_ray_tab && pp->ray_tab[set]) {
        const uint64_t rows = N > P ? N : P, waves = blocks_of(rows, 64);
        hipLaunchKernelGGL(ray_table_kernel, dim3((uint32_t)(waves < 64 ? waves : 64)), dim3(64), 0, T, d_poses16, (uint32_t)P, d_dirs3,
                           (uint32_t)N, pp->ray_tab[set]);
        LRC_HIP(hipGetLastError());
        p.ray_tab = pp->ray_tab[set];
        pp->ray_tab_last = true;
    }
    // the rows of submit k - 2 (this stream's previous scan; its scan pass was enqueued behind its trace) ride in front
    const int prev = (int)((k + lrc_pipe::kSets - 2) % lrc_pipe::kSets);
    lrc_compact_io pio{};
    if (pp->fused && k >= 2 && pp->pending[prev]) {
        pio = pipe_io(pp, prev);
        const uint64_t tps = N / 64, ntiles = pp->poses[prev] * tps;
        const uint64_t need = pio.counts ? blocks_of(pp->poses[prev], kTBlock) : 0;
        const uint64_t pre_blocks = blocks_of(ntiles, kPreTiles);
        p.pre.blocks = (uint32_t)(pre_blocks > need ? pre_blocks : need);
        p.pre.rows_only = (pio.out_xyzl && !pio.out_point3 && !pio.out_sem && !pio.out_ins && !pio.out_index && !pio.out_range_origin) ? 1u : 0u;
        p.pre.seg_len = N; p.pre.tps = tps; p.pre.ntiles = ntiles; p.pre.nseg = pp->poses[prev];
        p.pre.tile_off = pp->scratch[lane].d_tile_off;
        p.pre.super_total = pp->scratch[lane].d_super_total;
        p.pre.io = pio;
        p.pre.lean = pipe_lean(pp, prev);
    }
    LRC_HIP(hipEventRecord(pp->ev_t0[set], T));
    rc = launch_trace(s, p, kGenPoses, T);
    if (rc) return rc;
    LRC_HIP(hipEventRecord(pp->ev_trace[set], T));
    pp->line_last = p.line_tiles;
    pp->group_last = p.line_group;
    pp->lines_last = tile_lines_of(p.line_tiles, (uint32_t)(N / 64), p.line_group);
    if (p.pre.blocks) pp->pending[prev] = false;
    pp->out[set] = *d_out;
    pp->poses[set] = P;
    pp->lean[set] = p.lean.row != nullptr;
    // what the trace kernel calls `tabbed`: with it, the pose records of the set's table say which tiles are in the record form
    // (read back from the launch's own argument block: launch_trace fills tiles_per_pose, and a laboratory kernel that takes
    // no table drops the pointer)
    pp->tabbed[set] = p.lean.row != nullptr && p.ray_tab != nullptr && p.tiles_per_pose != 0u;
    pp->ray_tab_last = p.ray_tab != nullptr;
    pp->expanded[set] = false;
    if (pp->fused) {
        // the scan pass over this scan's per-wave keep counts: 32-64 one-wave workgroups behind the trace; the rows follow
        // with this stream's next launch (or with lrc_pipe_wait)
        const uint64_t ntiles = P * (N / 64), nsuper = blocks_of(ntiles, 1024);
        // One wave per super tile.  Beside the other stream's running launch a kernel of this stream is handed a wave slot
        // every few microseconds at best, so in a long run four waves (in within 20 us, 80 us of work each) are 0.4 % ahead of
        // 64 (arriving over 300 us: the next launch of this stream waits behind them) -- but a run ENDS with this pass alone on
        // the GPU, where four waves take 80 us and 64 take 10: over blocks of 20 submits the wide pass is 2.4 % faster, over 300
        // submits 0.4 % slower (profiles/r04_pipe_scan_width.txt).  Callers synchronise more often than every 300 batches.
        // (a lean set's counts are the popcounts of its keep masks; rec's tile_count is filled on the way for lrc_pipe_records)
        hipLaunchKernelGGL(compact_scan_masks_kernel, dim3((uint32_t)(nsuper < LRC_PIPE_SCAN_WAVES ? nsuper : LRC_PIPE_SCAN_WAVES)), dim3(64), 0, T,
                           (const uint64_t*)pp->keep_mask[set], pp->rec[set].tile_count, pp->scratch[lane].d_tile_off, ntiles,
                           pp->scratch[lane].d_super_total);
        LRC_HIP(hipGetLastError());
        pp->pending[set] = true;
    } else {
        lrc_compact_io io = pipe_io(pp, set);
        rc = enqueue_compaction(pp->scratch[lane], P, N, &io, T);
        if (rc) return rc;
    }
    pp->ticket = k + 1;
    if (out_ticket) *out_ticket = k + 1;
    return LRC_OK;
}

}  // extern "C"

// ---- the pipeline on N ranks: the trace writes triangle ids + keep counts into the caller's send slab, the assembly of an
// EARLIER scan of all ranks (its gathered slabs) rides in the leading workgroups of this trace launch ----------------------
namespace {
// max_back: how many submits may have followed own_ticket.  3 where the work runs on the caller's stream, ahead of every later
// submit (lrc_pipe_assemble, lrc_pipe_scan_gathered); 2 where the assembly rides in the launch of the next submit, which must not
// be own_ticket + 4: that launch's own trace writes the set the assembly reads (lrc_pipe_submit_sharded).
int check_gathered(const lrc_pipe* pp, const lrc_gathered* g, const char* who, uint64_t max_back) {
    auto bad = [&](const char* m) { return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + m); };
    if (!g->d_all_poses16 || !g->d_all_prims || !g->d_all_tile_counts || !g->d_out_xyzl) return bad("NULL member of lrc_gathered");
    if (g->poses_per_slab == 0 || g->poses_per_slab > pp->max_poses || g->num_poses_all == 0 || g->num_poses_all % g->poses_per_slab)
        return bad("num_poses_all must be a multiple of poses_per_slab (<= the pipeline's max_poses)");
    if (g->own_slab >= g->num_poses_all / g->poses_per_slab) return bad("own_slab outside the gathered slabs");
    if (g->slab_stride_bytes % 4 || g->slab_stride_bytes < g->poses_per_slab * pp->rays_per_pose * 4) return bad("slab stride smaller than a slab");
    if (g->own_ticket == 0 || g->own_ticket > pp->ticket || pp->ticket - g->own_ticket > max_back)
        return bad(max_back < 3 ? "the own records of that scan are rewritten by this submit: carry the assembly at most three "
                                  "submits after own_ticket, or use lrc_pipe_assemble"
                                : "the own records of that scan are gone (four sets rotate): assemble within three submits");
    if (pp->lean[(g->own_ticket - 1) % lrc_pipe::kSets]) return bad("own_ticket is not a submit of lrc_pipe_submit_sharded");
    const uint64_t ntiles = g->num_poses_all * (pp->rays_per_pose / 64);
    if (ntiles > 0x7FFFFFFFull) return bad("too many entries");
    return LRC_OK;
}

// the scan over all ranks' keep counts (two one-wave kernels on `st`; the first also transposes the direction table for the
// rebuild) into the scratch set of g->scan_slot: the launch that reads them waits for `st` as it must for the offsets; also what
// a first use needs: the plane table
int scan_gathered(lrc_pipe* pp, const lrc_gathered* g, const double* d_dirs3, hipStream_t st, int scan_waves) {
    lrc_scene* s = pp->scene;
    lrc_ctx::TileScratch& sc = pp->gscratch[g->scan_slot & 1u];
    const uint64_t N = pp->rays_per_pose, tps = N / 64, ntiles = g->num_poses_all * tps;
    int rc = ensure_tile_scratch(sc, ntiles);
    if (rc) return rc;
    if ((rc = ensure_prim_plane(s, st))) return rc;
    // every call: the table may have been edited in place, or be a new one at a recycled address
    if (!sc.d_dirs_soa) {
        LRC_HIP(hipMalloc((void**)&sc.d_dirs_soa, N * 24));
        sc.dirs_cap = N;
    }
    const uint64_t stride = g->slab_stride_bytes / 4, nsuper = blocks_of(ntiles, 1024);
    // one wave per super tile, at least one per 1024 directions (16 rows of the table per lane), at most scan_waves
    uint64_t grid = nsuper > blocks_of(N, 1024) ? nsuper : blocks_of(N, 1024);
    if (scan_waves > 0 && grid > (uint64_t)scan_waves) grid = (uint64_t)scan_waves;
    hipLaunchKernelGGL(gathered_scan_kernel, dim3((uint32_t)grid), dim3(64), 0, st, g->d_all_tile_counts, g->poses_per_slab * tps, stride,
                       sc.d_tile_off, ntiles, sc.d_super_total, d_dirs3, (uint32_t)N, sc.d_dirs_soa);
    hipLaunchKernelGGL(compact_base_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)sc.d_super_total, sc.d_super_base, nsuper);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

// the rebuild's argument block and the own rows' compaction input, for a gathered scan whose counts have been scanned
int prepare_gathered(lrc_pipe* pp, const lrc_gathered* g, RebuildParams* q, lrc_compact_io* own_io, uint64_t* own_tiles,
                     uint64_t* tile_base) {
    lrc_scene* s = pp->scene;
    lrc_ctx::TileScratch& sc = pp->gscratch[g->scan_slot & 1u];
    const uint64_t N = pp->rays_per_pose, tps = N / 64, ntiles = g->num_poses_all * tps;
    if (sc.tile_cap < ntiles + 1 || !sc.d_dirs_soa || !s->d_prim_plane)
        return fail(LRC_ERR_INVALID_ARG, "lrc_pipe: the gathered scan has not been through lrc_pipe_scan_gathered");
    const uint64_t stride = g->slab_stride_bytes / 4;
    q->poses16 = g->d_all_poses16; q->dirs_soa = sc.d_dirs_soa; q->prims = g->d_all_prims;
    q->pps = (uint32_t)g->poses_per_slab; q->stride = stride; q->seg_len = (uint32_t)N; q->tps = (uint32_t)tps;
    q->ntiles = (uint32_t)ntiles; q->nseg = (uint32_t)g->num_poses_all; q->plane = s->d_prim_plane;
    q->num_prims = (uint32_t)s->info.num_triangles; q->tile_off = sc.d_tile_off; q->super_base = sc.d_super_base;
    q->out_xyzl = (float4*)g->d_out_xyzl; q->counts = g->d_counts; q->skip_slab = (uint32_t)g->own_slab;
    const lrc_hits& h = pp->rec[(g->own_ticket - 1) % lrc_pipe::kSets];
    *own_io = lrc_compact_io{};
    own_io->t = h.t; own_io->point3 = h.point3; own_io->sem = h.sem; own_io->ins = h.ins;
    own_io->out_xyzl = g->d_out_xyzl;
    *own_tiles = pp->poses[(g->own_ticket - 1) % lrc_pipe::kSets] * tps;
    *tile_base = g->own_slab * g->poses_per_slab * tps;
    return LRC_OK;
}
}  // namespace

extern "C" {

int lrc_pipe_submit_sharded(lrc_pipe* pp, const double* d_poses16, uint64_t P, const double* d_dirs3, double max_range,
                            uint32_t* d_send_prim, uint32_t* d_send_tile_count, const lrc_gathered* assemble, void* stream,
                            uint64_t* out_ticket) {
    if (!pp) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit_sharded: pipe is NULL");
    if (!pp->fused) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit_sharded: needs rays_per_pose % 64 == 0");
    if (P == 0 || P > pp->max_poses) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit_sharded: pose count outside (0, max_poses]");
    if (!d_poses16 || !d_dirs3 || !d_send_prim || !d_send_tile_count)
        return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit_sharded: NULL poses, table or send slab");
    lrc_scene* s = pp->scene;
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_submit_sharded: a scan with range noise cannot be rebuilt from triangle ids");
    LRC_HIP(hipSetDevice(s->ctx->device));
    int rc;
    if (assemble && (rc = check_gathered(pp, assemble, "lrc_pipe_submit_sharded", 2))) return rc;
    const uint64_t k = pp->ticket;
    const int set = (int)(k % lrc_pipe::kSets), lane = (int)(k % 2);
    hipStream_t T = pp->s_trace[lane];
    // inputs, the send slab and -- for the assembly -- the gathered slabs are the caller's as of this point of its stream
    LRC_HIP(hipEventRecord(pp->ev_in[set], (hipStream_t)stream));
    LRC_HIP(hipStreamWaitEvent(T, pp->ev_in[set], 0));
    if ((rc = wait_for_readers(pp, set, T))) return rc;
    const uint64_t N = pp->rays_per_pose;
    TraceParams p{};
    p.poses16 = d_poses16; p.dirs3 = d_dirs3;
    scan_fields(p, N, P * N, max_range, &pp->rec[set]);
    p.out.prim = d_send_prim;                  // the 36-byte record stays complete: its id column IS the send slab
    p.out.tile_count = d_send_tile_count;
    lrc_compact_io own_io{};
    if (assemble) {
        uint64_t own_tiles = 0, tile_base = 0;
        if ((rc = prepare_gathered(pp, assemble, &p.pre.rq, &own_io, &own_tiles, &tile_base))) return rc;
        p.pre.sharded = 1;
        p.pre.io = own_io;
        p.pre.ntiles = own_tiles;
        p.pre.seg_len = N; p.pre.tps = N / 64;
        p.pre.tile_off = pp->gscratch[assemble->scan_slot & 1u].d_tile_off;
        p.pre.super_base = pp->gscratch[assemble->scan_slot & 1u].d_super_base;
        p.pre.tile_base = tile_base;
        p.pre.own_blocks = (uint32_t)blocks_of(own_tiles, kPreTiles);
        const uint64_t rb = blocks_of(p.pre.rq.ntiles, LRC_REBUILD_R);
        const uint64_t need = blocks_of(p.pre.rq.nseg, kTBlock);        // threads for the per-pose counts
        uint64_t blocks = p.pre.own_blocks + rb;
        if (blocks < need) blocks = need;
        p.pre.blocks = (uint32_t)blocks;
    }
    LRC_HIP(hipEventRecord(pp->ev_t0[set], T));
    rc = launch_trace(s, p, kGenPoses, T);
    if (rc) return rc;
    LRC_HIP(hipEventRecord(pp->ev_trace[set], T));
    if (assemble) pp->read_by[(assemble->own_ticket - 1) % lrc_pipe::kSets] = k + 1;
    pp->out[set] = lrc_compact_io{};
    pp->poses[set] = P;
    pp->lean[set] = false;                     // the complete record (its id column is the send slab)
    pp->expanded[set] = false;
    pp->pending[set] = false;                  // nothing local to scatter: the rows appear when the gathered scan is assembled
    pp->ticket = k + 1;
    if (out_ticket) *out_ticket = k + 1;
    return LRC_OK;
}

int lrc_pipe_trace_done(lrc_pipe* pp, uint64_t ticket, void* stream) {
    if (!pp) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_trace_done: pipe is NULL");
    if (ticket == 0 || ticket > pp->ticket || pp->ticket - ticket >= (uint64_t)lrc_pipe::kSets)
        return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_trace_done: the events of that submit have been reused");
    LRC_HIP(hipSetDevice(pp->scene->ctx->device));
    LRC_HIP(hipStreamWaitEvent((hipStream_t)stream, pp->ev_trace[(ticket - 1) % lrc_pipe::kSets], 0));
    return LRC_OK;
}

// the scan over the gathered keep counts, on the caller's COMMUNICATION stream right behind the collective: two one-wave kernels
// that trickle in beside the running trace launch and have a whole step before the launch that carries the assembly needs them
// (between two trace launches of one stream they would hold the second back: DESIGN.md section 5.2)
int lrc_pipe_scan_gathered(lrc_pipe* pp, const double* d_dirs3, const lrc_gathered* g, void* stream) {
    if (!pp || !g || !d_dirs3) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_scan_gathered: NULL argument");
    int rc = check_gathered(pp, g, "lrc_pipe_scan_gathered", 3);
    if (rc) return rc;
    LRC_HIP(hipSetDevice(pp->device));
    return scan_gathered(pp, g, d_dirs3, (hipStream_t)stream, LRC_PIPE_SCAN_WAVES * 4);
}

// the assembly of a gathered (and scanned) scan with the plain kernels, on `stream` (the end of a run: no later launch to ride on)
int lrc_pipe_assemble(lrc_pipe* pp, const double* d_dirs3, const lrc_gathered* g, void* stream) {
    if (!pp || !g || !d_dirs3) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_assemble: NULL argument");
    int rc = check_gathered(pp, g, "lrc_pipe_assemble", 3);
    if (rc) return rc;
    LRC_HIP(hipSetDevice(pp->scene->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    // the own records were written by a trace on an internal stream
    LRC_HIP(hipStreamWaitEvent(st, pp->ev_trace[(g->own_ticket - 1) % lrc_pipe::kSets], 0));
    RebuildParams q{};
    lrc_compact_io io{};
    uint64_t own_tiles = 0, tile_base = 0;
    if ((rc = prepare_gathered(pp, g, &q, &io, &own_tiles, &tile_base))) return rc;
    launch_prim_scatter(q, st);
    launch_own_rows(io, pp->rays_per_pose, pp->rays_per_pose / 64, own_tiles, q, tile_base, st);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_pipe_wait(lrc_pipe* pp, void* stream) {
    if (!pp) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_wait: pipe is NULL");
    if (pp->ticket == 0) return LRC_OK;
    LRC_HIP(hipSetDevice(pp->scene->ctx->device));
    // the rows still waiting for a launch to ride on (the last two submits) are scattered by the plain kernel
    for (uint64_t back = 2; back >= 1; --back) {
        if (pp->ticket < back) continue;
        const uint64_t k = pp->ticket - back;
        const int set = (int)(k % lrc_pipe::kSets), lane = (int)(k % 2);
        if (!pp->pending[set]) continue;
        lrc_compact_io io = pipe_io(pp, set);
        const uint64_t N = pp->rays_per_pose, tps = N / 64, ntiles = pp->poses[set] * tps;
        const uint64_t nblocks = tile_blocks(ntiles);
        const uint64_t need = io.counts ? blocks_of(pp->poses[set], kBlock) : 0;
        const dim3 grid((uint32_t)(nblocks > need ? nblocks : need));
        if (pp->lean[set])
            hipLaunchKernelGGL(compact_scatter_lean_kernel, grid, dim3(kBlock), 0, pp->s_trace[lane], io, pipe_lean(pp, set), N, tps,
                               ntiles, pp->poses[set], (const uint32_t*)pp->scratch[lane].d_tile_off,
                               (const uint32_t*)pp->scratch[lane].d_super_total);
        else
            hipLaunchKernelGGL(compact_scatter_kernel, grid, dim3(kBlock), 0, pp->s_trace[lane],
                               io, N, tps, ntiles, pp->poses[set], (const uint32_t*)pp->scratch[lane].d_tile_off,
                               (const uint64_t*)nullptr, (uint64_t)0, (const uint32_t*)pp->scratch[lane].d_super_total);
        LRC_HIP(hipGetLastError());
        pp->pending[set] = false;
    }
    for (int lane = 0; lane < 2; ++lane) {
        LRC_HIP(hipEventRecord(pp->ev_flush[lane], pp->s_trace[lane]));
        LRC_HIP(hipStreamWaitEvent((hipStream_t)stream, pp->ev_flush[lane], 0));
    }
    return LRC_OK;
}

// the complete 36-byte records of a submit (a verification surface: bench.py and the pipeline never read them).  A lean set is
// expanded into its full arrays once per submit, behind its trace, and the host waits as lrc_pipe_trace_ms does.
int lrc_pipe_records(lrc_pipe* pp, uint64_t ticket, lrc_hits* out_records) {
    if (!pp || !out_records) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_records: NULL argument");
    if (ticket == 0 || ticket > pp->ticket || pp->ticket - ticket >= (uint64_t)lrc_pipe::kSets)
        return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_records: the records of that submit are gone (four sets rotate)");
    const int set = (int)((ticket - 1) % lrc_pipe::kSets);
    if (pp->lean[set] && !pp->expanded[set]) {
        // a lean set: rebuild the complete records on the set's trace stream behind its trace, and wait for them
        lrc_scene* s = pp->scene;
        LRC_HIP(hipSetDevice(s->ctx->device));
        hipStream_t T = pp->s_trace[(ticket - 1) % 2];
        const uint64_t n = pp->poses[set] * pp->rays_per_pose;
        hipLaunchKernelGGL(expand_lean_kernel, dim3((uint32_t)blocks_of(n, kBlock)), dim3(kBlock), 0, T,
                           pipe_lean(pp, set), pp->rays_per_pose, (const uint32_t*)s->d_slot_prim,
                           (const float4*)s->d_tris, pp->rec[set], n);
        LRC_HIP(hipGetLastError());
        LRC_HIP(hipEventRecord(pp->ev_expand, T));
        LRC_HIP(hipEventSynchronize(pp->ev_expand));
        pp->expanded[set] = true;
    }
    *out_records = pp->rec[set];
    return LRC_OK;
}

int lrc_pipe_trace_ms(lrc_pipe* pp, uint64_t ticket, float* out_ms) {
    if (!pp || !out_ms) return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_trace_ms: NULL argument");
    if (ticket == 0 || ticket > pp->ticket || pp->ticket - ticket >= (uint64_t)lrc_pipe::kSets)
        return fail(LRC_ERR_INVALID_ARG, "lrc_pipe_trace_ms: the events of that submit have been reused");
    const int set = (int)((ticket - 1) % lrc_pipe::kSets);
    LRC_HIP(hipSetDevice(pp->scene->ctx->device));
    LRC_HIP(hipEventSynchronize(pp->ev_trace[set]));
    LRC_HIP(hipEventElapsedTime(out_ms, pp->ev_t0[set], pp->ev_trace[set]));
    return LRC_OK;
}

int lrc_cloud_from_ranges_dev(lrc_ctx* ctx, const double* d_poses16, uint64_t P, const double* d_dirs3,
                              uint64_t N, const void* d_t_label, float* d_out_xyzl, uint64_t* d_counts,
                              void* stream) {
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_from_ranges_dev: ctx is NULL");
    if (P == 0 || N == 0) return LRC_OK;
    if (!d_poses16 || !d_dirs3 || !d_t_label || !d_out_xyzl)
        return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_from_ranges_dev: NULL argument");
    LRC_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const uint64_t tps = blocks_of(N, 64), ntiles = P * tps;
    const uint64_t nblocks = tile_blocks(ntiles);
    if (nblocks > 0x7FFFFFFFull) return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_from_ranges_dev: too many entries");
    lrc_ctx::TileScratch& sc = ctx->cloud_scratch;
    int rc = ensure_tile_scratch(sc, ntiles);
    if (rc) return rc;
    hipLaunchKernelGGL(cloud_count_kernel, dim3((uint32_t)nblocks), dim3(kBlock), 0, st, (const uint2*)d_t_label, N,
                       tps, ntiles, sc.d_tile_cnt);
    launch_scan_chain(sc, sc.d_tile_cnt, ntiles, 0, ntiles, true, st);
    const uint64_t need = d_counts ? blocks_of(P, kBlock) : 0;
    const uint64_t grid = nblocks > need ? nblocks : need;
    hipLaunchKernelGGL(cloud_scatter_kernel, dim3((uint32_t)grid), dim3(kBlock), 0, st, d_poses16, d_dirs3,
                       (const uint2*)d_t_label, N, tps, ntiles, P, (const uint32_t*)sc.d_tile_off,
                       (const uint64_t*)sc.d_super_base, (float4*)d_out_xyzl, d_counts);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

// Checks the arguments of a rebuild from triangle ids, enqueues its preparation on `st` (tile offsets from the senders'
// counts or from a counting pass, transposed direction table) and fills the kernel argument block.
static int prepare_rebuild(lrc_scene* s, const char* who, const double* d_poses16, uint64_t P, const double* d_dirs3,
                           uint64_t N, const uint32_t* d_prim, const uint32_t* d_tile_count, uint64_t poses_per_slab,
                           uint64_t slab_stride_bytes, float* d_out_xyzl, uint64_t* d_counts, hipStream_t st,
                           RebuildParams* q) {
    auto bad = [&](const char* msg) { return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + msg); };
    if (!d_poses16 || !d_dirs3 || !d_prim || !d_out_xyzl) return bad("NULL argument");
    if (s->opts.range_noise)
        return bad("a scan with range noise cannot be rebuilt from triangle ids; gather (t,label) pairs "
                   "(lrc_cloud_from_ranges_dev)");
    const uint64_t tps = blocks_of(N, 64), ntiles = P * tps;
    if (poses_per_slab == 0 || poses_per_slab >= P) { poses_per_slab = P; slab_stride_bytes = 0; }
    else if (slab_stride_bytes % 4 || slab_stride_bytes < poses_per_slab * N * 4)
        return bad("slab stride smaller than a slab or not a multiple of 4");
    if (d_tile_count && N % 64) return bad("tile counts need rays_per_pose % 64 == 0");
    if (ntiles > 0x7FFFFFFFull || N > 0x7FFFFFFFull) return bad("too many entries");
    lrc_ctx* ctx = s->ctx;
    lrc_ctx::TileScratch& sc = ctx->cloud_scratch;
    int rc = ensure_tile_scratch(sc, ntiles);
    if (rc) return rc;
    if ((rc = ensure_prim_plane(s, st))) return rc;
    if (sc.dirs_cap < N) {
        if (sc.d_dirs_soa) { (void)hipFree(sc.d_dirs_soa); sc.d_dirs_soa = nullptr; }
        sc.dirs_cap = 0;
        LRC_HIP(hipMalloc((void**)&sc.d_dirs_soa, N * 24));
        sc.dirs_cap = N;
    }
    const uint64_t stride = slab_stride_bytes / 4;
    if (d_tile_count) {
        // the senders' trace kernels already counted (lrc_hits.tile_count travels in the slab): no counting pass
        launch_scan_chain(sc, d_tile_count, poses_per_slab * tps, stride, ntiles, true, st);
    } else {
        hipLaunchKernelGGL(prim_count_kernel, dim3((uint32_t)tile_blocks(ntiles)), dim3(kBlock), 0, st, d_prim, poses_per_slab,
                           stride, N, tps, ntiles, sc.d_tile_cnt);
        launch_scan_chain(sc, sc.d_tile_cnt, ntiles, 0, ntiles, true, st);
    }
    hipLaunchKernelGGL(dirs_transpose_kernel, dim3((uint32_t)blocks_of(N, kBlock)), dim3(kBlock), 0, st,
                       d_dirs3, (uint32_t)N, sc.d_dirs_soa);
    q->poses16 = d_poses16;
    q->dirs_soa = sc.d_dirs_soa;
    q->prims = d_prim;
    q->pps = (uint32_t)poses_per_slab;
    q->stride = stride;
    q->seg_len = (uint32_t)N;
    q->tps = (uint32_t)tps;
    q->ntiles = (uint32_t)ntiles;
    q->nseg = (uint32_t)P;
    q->plane = s->d_prim_plane;
    q->num_prims = (uint32_t)s->info.num_triangles;
    q->tile_off = sc.d_tile_off;
    q->super_base = sc.d_super_base;
    q->out_xyzl = (float4*)d_out_xyzl;
    q->counts = d_counts;
    q->skip_slab = 0xFFFFFFFFu;
    return LRC_OK;
}

int lrc_cloud_from_prims_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N,
                             const uint32_t* d_prim, const uint32_t* d_tile_count, uint64_t poses_per_slab,
                             uint64_t slab_stride_bytes, float* d_out_xyzl, uint64_t* d_counts, void* stream) {
    if (!s) return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_from_prims_dev: scene is NULL");
    if (P == 0 || N == 0) return LRC_OK;
    LRC_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    RebuildParams q{};
    int rc = prepare_rebuild(s, "lrc_cloud_from_prims_dev", d_poses16, P, d_dirs3, N, d_prim, d_tile_count,
                             poses_per_slab, slab_stride_bytes, d_out_xyzl, d_counts, st, &q);
    if (rc) return rc;
    launch_prim_scatter(q, st);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_cloud_from_prims_own_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N,
                                 const uint32_t* d_prim, const uint32_t* d_tile_count, uint64_t poses_per_slab,
                                 uint64_t slab_stride_bytes, uint64_t own_slab, const lrc_compact_io* own,
                                 float* d_out_xyzl, uint64_t* d_counts, void* stream) {
    if (!s) return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_from_prims_own_dev: scene is NULL");
    if (P == 0 || N == 0) return LRC_OK;
    if (!own || !own->t || !own->point3)
        return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_from_prims_own_dev: the own records need t and point3");
    if (!d_tile_count || N % 64 || poses_per_slab == 0 || poses_per_slab > P || own_slab * poses_per_slab >= P)
        return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_from_prims_own_dev: needs per-wave keep counts (rays_per_pose % 64 == 0), "
                                         "slabs and an own slab inside the scan");
    LRC_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    RebuildParams q{};
    int rc = prepare_rebuild(s, "lrc_cloud_from_prims_own_dev", d_poses16, P, d_dirs3, N, d_prim, d_tile_count,
                             poses_per_slab, slab_stride_bytes, d_out_xyzl, d_counts, st, &q);
    if (rc) return rc;
    q.skip_slab = (uint32_t)own_slab;
    launch_prim_scatter(q, st);
    // the own poses: rows straight from the local record (what the trace wrote), at the offsets of the assembled cloud
    const uint64_t first_pose = own_slab * poses_per_slab;
    const uint64_t own_poses = first_pose + poses_per_slab <= P ? poses_per_slab : P - first_pose;
    const uint64_t tps = N / 64, own_tiles = own_poses * tps;
    lrc_compact_io io = *own;
    io.counts = nullptr;                 // the per-pose counts of ALL poses come from the rebuild's scan
    io.out_point3 = nullptr; io.out_sem = nullptr; io.out_ins = nullptr; io.out_incident_deg = nullptr;
    io.out_index = nullptr; io.out_range_origin = nullptr;
    io.out_xyzl = d_out_xyzl;
    launch_own_rows(io, N, tps, own_tiles, q, first_pose * tps, st);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_cloud_range_stats_dev(lrc_ctx* ctx, const float* d_xyzl, const uint64_t* d_counts, uint64_t num_poses,
                              uint64_t max_rows, float* d_range, float* d_mean, float* d_std, void* stream) {
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_range_stats_dev: ctx is NULL");
    if (num_poses == 0) return LRC_OK;
    if (!d_xyzl || !d_counts || !d_range || !d_mean || !d_std)
        return fail(LRC_ERR_INVALID_ARG, "lrc_cloud_range_stats_dev: NULL argument");
    LRC_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (max_rows)
        hipLaunchKernelGGL(rows_range_kernel, dim3((uint32_t)blocks_of(max_rows, kBlock)), dim3(kBlock), 0, st,
                           (const float4*)d_xyzl, max_rows, d_range);
    const uint64_t need = segment_stats_scratch_values(num_poses, max_rows);
    if (ctx->stat_scratch_cap < need) {
        if (ctx->stat_scratch) { LRC_HIP(hipDeviceSynchronize()); (void)hipFree(ctx->stat_scratch); ctx->stat_scratch = nullptr; ctx->stat_scratch_cap = 0; }
        LRC_HIP(hipMalloc((void**)&ctx->stat_scratch, (need + need / 4) * 4));
        ctx->stat_scratch_cap = need + need / 4;
    }
    launch_segment_stats<float>(st, (const float*)d_range, d_counts, (uint64_t)0, num_poses, ctx->stat_scratch, d_mean, d_std);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_compact(lrc_ctx* ctx, uint64_t nseg, uint64_t seg_len, const lrc_compact_io* io,
                uint64_t* out_total) {
    if (!ctx || !io) return fail(LRC_ERR_INVALID_ARG, "lrc_compact: NULL argument");
    if (out_total) *out_total = 0;
    const uint64_t n = nseg * seg_len;
    if (!n) return LRC_OK;
    if (!io->t) return fail(LRC_ERR_INVALID_ARG, "lrc_compact: t is NULL");
    LRC_HIP(hipSetDevice(ctx->device));
    DevBuf bufs[13];          // allocations of this call: 5 inputs, the counts, 7 outputs
    int used = 0;
    lrc_compact_io d{};
    // `rows` rows of a column of io in HBM, for d's member `col`
    auto device_column = [&](auto col, uint64_t rows, size_t per_row, bool upload) -> int {
        DevBuf& b = bufs[used++];
        const size_t bytes = rows * per_row * sizeof(*(d.*col));
        LRC_HIP(hipMalloc(&b.p, bytes));
        if (upload) LRC_HIP(hipMemcpy(b.p, io->*col, bytes, hipMemcpyHostToDevice));
        d.*col = static_cast<std::remove_reference_t<decltype(d.*col)>>(b.p);
        return LRC_OK;
    };
    int rc;
    if ((rc = record_columns([&](auto, auto col, size_t per_ray) -> int { return io->*col ? device_column(col, n, per_ray, true) : LRC_OK; })) ||
        (rc = device_column(&lrc_compact_io::counts, nseg, 1, false)) ||
        (rc = frame_columns([&](auto, auto col, size_t per_row) -> int { return io->*col ? device_column(col, n, per_row, false) : LRC_OK; })))
        return rc;
    if ((rc = lrc_compact_dev(ctx, nseg, seg_len, &d, nullptr))) return rc;
    LRC_HIP(hipDeviceSynchronize());
    std::vector<uint64_t> counts(nseg);
    LRC_HIP(hipMemcpy(counts.data(), d.counts, nseg * 8, hipMemcpyDeviceToHost));
    uint64_t K = 0;
    for (uint64_t c : counts) K += c;
    if (io->counts) std::memcpy(io->counts, counts.data(), nseg * 8);
    if (out_total) *out_total = K;
    if (!K) return LRC_OK;
    return frame_columns([&](auto, auto col, size_t per_row) -> int {
        if (io->*col) LRC_HIP(hipMemcpy(io->*col, d.*col, K * per_row * sizeof(*(d.*col)), hipMemcpyDeviceToHost));
        return LRC_OK;
    });
}


}  // extern "C"

// ---- scan straight to the reference's variable-length frames ----------------------------------------------------
namespace {
// The *_compact entry points enqueue their input copies (on the context's compute stream, which consumes them) before
// anything can fail: an error return must not leave such a copy in flight over staging buffers the next call reuses.
struct SyncUnlessOk {
    bool armed = true;
    ~SyncUnlessOk() { if (armed) (void)hipDeviceSynchronize(); }
    int done(int rc) { if (rc == LRC_OK) armed = false; return rc; }
};

// compacted frame arrays in HBM (context pool) and the record set they are compacted from
struct FrameStage {
    DevBuf t, p3, sem, ins, inc, tile;                     // fixed-stride records
    DevBuf cnt, op3, osem, oins, oinc, oidx, oxyzl, orng;   // compacted outputs
    DevBuf fstat;                                           // per-pose statistics: 4 x P doubles
    lrc_hits rec{};
    lrc_compact_io io{};
    double* d_stats = nullptr;
    uint64_t stat_partial = 0;                                // values of chunk-sum scratch per column, behind the 4 P results
    int alloc(lrc_ctx* ctx, const lrc_frames& f, uint64_t P, uint64_t n) {
        int rc;
        const bool rstats = f.range_origin_mean || f.range_origin_std, istats = f.incident_mean || f.incident_std;
        const bool want_pt = f.point3 || f.xyzl || f.range_origin || rstats;
        const bool want_sem = f.sem || f.xyzl, want_ins = f.ins || f.xyzl;
        if ((rc = t.get(ctx, kPoolT, n * 4))) return rc;
        rec.t = (float*)t.p;
        if (want_pt) { if ((rc = p3.get(ctx, kPoolPoint, n * 12))) return rc; rec.point3 = (float*)p3.p; }
        if (want_sem) { if ((rc = sem.get(ctx, kPoolSem, n * 2))) return rc; rec.sem = (uint16_t*)sem.p; }
        if (want_ins) { if ((rc = ins.get(ctx, kPoolIns, n * 2))) return rc; rec.ins = (uint16_t*)ins.p; }
        if (f.incident_deg || istats) { if ((rc = inc.get(ctx, kPoolInc, n * 8))) return rc; rec.incident_deg = (double*)inc.p; }
        if (rstats || istats) {
            // 4 x P doubles of results, then the chunk sums of the two columns (segment_chunk_sums_kernel)
            stat_partial = segment_stats_scratch_values(P, n);
            if ((rc = fstat.get(ctx, kPoolFrameStats, (P * 4 + 2 * stat_partial) * 8))) return rc;
            d_stats = (double*)fstat.p;
        }
        if ((rc = tile.get(ctx, kPoolTile, (blocks_of(n, 64) + 1) * 4))) return rc;
        rec.tile_count = (uint32_t*)tile.p;
        io.t = rec.t; io.point3 = rec.point3; io.sem = rec.sem; io.ins = rec.ins; io.incident_deg = rec.incident_deg;
        io.tile_count = rec.tile_count;
        if ((rc = cnt.get(ctx, kPoolCounts, P * 8))) return rc;
        io.counts = (uint64_t*)cnt.p;
        if (f.point3) { if ((rc = op3.get(ctx, kPoolOutPoint, n * 12))) return rc; io.out_point3 = (float*)op3.p; }
        if (f.sem) { if ((rc = osem.get(ctx, kPoolOutSem, n * 2))) return rc; io.out_sem = (uint16_t*)osem.p; }
        if (f.ins) { if ((rc = oins.get(ctx, kPoolOutIns, n * 2))) return rc; io.out_ins = (uint16_t*)oins.p; }
        if (f.incident_deg || istats) { if ((rc = oinc.get(ctx, kPoolOutInc, n * 8))) return rc; io.out_incident_deg = (double*)oinc.p; }
        if (f.index) { if ((rc = oidx.get(ctx, kPoolOutIdx, n * 4))) return rc; io.out_index = (uint32_t*)oidx.p; }
        if (f.xyzl) { if ((rc = oxyzl.get(ctx, kPoolOutXyzl, n * 16))) return rc; io.out_xyzl = (float*)oxyzl.p; }
        if (f.range_origin || rstats) { if ((rc = orng.get(ctx, kPoolOutRange, n * 4))) return rc; io.out_range_origin = (float*)orng.p; }
        return LRC_OK;
    }
};

int ensure_streams(lrc_ctx* ctx) {
    if (!ctx->s_compute) LRC_HIP(hipStreamCreateWithFlags(&ctx->s_compute, hipStreamNonBlocking));
    if (!ctx->s_copy) LRC_HIP(hipStreamCreateWithFlags(&ctx->s_copy, hipStreamNonBlocking));
    if (!ctx->s_stats) LRC_HIP(hipStreamCreateWithFlags(&ctx->s_stats, hipStreamNonBlocking));
    for (hipEvent_t& e : ctx->ev_chunk)
        if (!e) LRC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (hipEvent_t& e : ctx->ev_compact)
        if (!e) LRC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return LRC_OK;
}

// bytes of one row of the columns the caller asked for
size_t frame_row_bytes(const lrc_frames& out) {
    size_t bytes = 0;
    (void)frame_columns([&](auto host, auto, size_t per_row) -> int {
        if (out.*host) bytes += per_row * sizeof(*(out.*host));
        return LRC_OK;
    });
    return bytes;
}

// `rows` rows of every column the caller asked for, from device row r0 of the compacted arrays to host row K, on stream `st`
int copy_frame_rows(const lrc_frames& out, const lrc_compact_io& io, uint64_t r0, uint64_t K, uint64_t rows, hipStream_t st) {
    return frame_columns([&](auto host, auto dev, size_t per_row) -> int {
        if (out.*host)
            LRC_HIP(hipMemcpyAsync(out.*host + K * per_row, io.*dev + r0 * per_row, rows * per_row * sizeof(*(out.*host)),
                                   hipMemcpyDeviceToHost, st));
        return LRC_OK;
    });
}

// The statistics of poses [p0, p0 + np), whose compacted rows start at device row r0, enqueued on stream `ss` behind those
// poses' compaction: numpy's arithmetic (lrc_stats.h) over the compacted columns, results into the page-locked area behind
// the counts.  Floats in the first two blocks of P doubles' worth of space, doubles in the last two.
int enqueue_frame_stats(lrc_ctx* ctx, const FrameStage& st, const lrc_frames* out, uint64_t P, uint64_t p0, uint64_t np_,
                        uint64_t r0, hipStream_t ss) {
    float* rm = (float*)st.d_stats;            float* rs = (float*)(st.d_stats + P);
    double* im = st.d_stats + 2 * P;           double* is = st.d_stats + 3 * P;
    double* hs = (double*)(ctx->h_counts + ctx->h_counts_cap);
    if (out->range_origin_mean || out->range_origin_std) {
        launch_segment_stats<float>(ss, (const float*)st.io.out_range_origin, (const uint64_t*)(st.io.counts + p0), r0, np_,
                                    (float*)(st.d_stats + 4 * P) + r0 / 8192 + p0, rm + p0, rs + p0);
        LRC_HIP(hipMemcpyAsync((float*)hs + p0, rm + p0, np_ * 4, hipMemcpyDeviceToHost, ss));
        LRC_HIP(hipMemcpyAsync((float*)(hs + ctx->h_counts_cap) + p0, rs + p0, np_ * 4, hipMemcpyDeviceToHost, ss));
    }
    if (out->incident_mean || out->incident_std) {
        launch_segment_stats<double>(ss, (const double*)st.io.out_incident_deg, (const uint64_t*)(st.io.counts + p0), r0, np_,
                                     st.d_stats + 4 * P + st.stat_partial + r0 / 8192 + p0, im + p0, is + p0);
        LRC_HIP(hipMemcpyAsync(hs + 2 * ctx->h_counts_cap + p0, im + p0, np_ * 8, hipMemcpyDeviceToHost, ss));
        LRC_HIP(hipMemcpyAsync(hs + 3 * ctx->h_counts_cap + p0, is + p0, np_ * 8, hipMemcpyDeviceToHost, ss));
    }
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

// ... and, once their stream is idle, the P statistics from that area to the caller's arrays
void publish_frame_stats(const lrc_ctx* ctx, const lrc_frames* out, uint64_t P) {
    const double* hs = (const double*)(ctx->h_counts + ctx->h_counts_cap);
    for (uint64_t k = 0; k < P; ++k) {
        if (out->range_origin_mean) out->range_origin_mean[k] = ((const float*)hs)[k];
        if (out->range_origin_std) out->range_origin_std[k] = ((const float*)(hs + ctx->h_counts_cap))[k];
        if (out->incident_mean) out->incident_mean[k] = hs[2 * ctx->h_counts_cap + k];
        if (out->incident_std) out->incident_std[k] = hs[3 * ctx->h_counts_cap + k];
    }
}

// Trace -> compaction -> kept rows to the host, pipelined over contiguous chunks of poses: while chunk c's rows cross
// PCIe on the copy stream, chunk c+1 is traced and compacted on the compute stream.  Each chunk compacts into its own
// worst-case region of the device arrays (rows [p0*N, ...)); the host destination offset is the running row count, so
// the host arrays come out packed in pose order (np.vstack order) without a second pass.  Pinned destinations
// (lrc_host_alloc) make the transfers true DMA.  `p` describes the whole scan (inputs already in HBM).
int frames_finish(lrc_scene* s, TraceParams& p, int gen, FrameStage& st, uint64_t P, uint64_t N, const lrc_frames* out,
                  uint64_t capacity, uint64_t* out_total) {
    lrc_ctx* ctx = s->ctx;
    int rc = ensure_streams(ctx);
    if (rc) return rc;
    // Every exit -- the error returns below too -- leaves the three streams idle: the caller's stage buffers go back to
    // the context pool and its pinned destinations to Python as soon as this function returns.
    struct Drain {
        lrc_ctx* c;
        ~Drain() {
            (void)hipStreamSynchronize(c->s_compute);
            (void)hipStreamSynchronize(c->s_copy);
            (void)hipStreamSynchronize(c->s_stats);
        }
    } drain{ctx};
    if (ctx->h_counts_cap < P) {
        if (ctx->h_counts) { (void)hipHostFree(ctx->h_counts); ctx->h_counts = nullptr; ctx->h_counts_cap = 0; }
        LRC_HIP(hipHostMalloc((void**)&ctx->h_counts, (P + P / 4 + 64) * 8 * 5, hipHostMallocDefault));
        ctx->h_counts_cap = P + P / 4 + 64;
    }
    // chunks only pay when there is enough to overlap, and need pose boundaries on 64-ray tiles (fused keep counts)
    uint64_t chunks = (P * N >= (1u << 20) && N % 64 == 0) ? (P < 4 ? P : 4) : 1;
    // Graded chunks: an eighth of the poses, then up to the half, then the rest.  The transfer of the rows is the longest
    // stage (67 MB at 50-56 GB/s for C3): it starts as soon as a few poses are traced, and the later, larger chunks are ready
    // before the copy engine asks for them (C3: 1.48 ms against 1.53 for four equal chunks; tools/chunk_scheme_sweep.sh,
    // profiles/r03_chunk_schemes.txt).  Equal chunks for short trajectories.
    // echoes: the weight rows are gathered from ONE packed run of compacted rows (echo_scan_compact); materials: likewise for
    // intensity, bounces and surface points (material_scan_compact)
    if (gen_frames_one_chunk(gen)) chunks = 1;
    bool graded = chunks == 4 && P >= 8;
    uint32_t ends32[8] = {4, 16, 32, 32, 32, 32, 32, 32};       // chunk ends in 32nds of the trajectory
    if (graded) chunks = 3;
#ifdef LRC_VARIANTS
    {   // A/B knob: LRC_CHUNK_SCHEME = "a,b,...,32" chunk ends in 32nds; "0" = four equal chunks
        const char* e = std::getenv("LRC_CHUNK_SCHEME");
        if (e && graded) {
            if (e[0] == '0') { graded = false; chunks = 4; }
            else {
                uint64_t k = 0;
                for (const char* q = e; *q && k < 8; ++k) { ends32[k] = (uint32_t)std::strtoul(q, (char**)&q, 10); if (*q == ',') ++q; }
                if (k && ends32[k - 1] == 32) chunks = k;
            }
        }
    }
#endif
    auto chunk_end = [&](uint64_t c) -> uint64_t {
        if (!graded) return P * (c + 1) / chunks;
        return c + 1 == chunks ? P : P * ends32[c] / 32;
    };
    const float* noise = p.range_noise ? p.range_noise : s->opts.range_noise;   // staged in HBM by NoiseStage
    // (the callers enqueue their input copies on the compute stream: nothing to wait for here)
    const uint64_t n_all = P * N;
    if (chunks == 1 && capacity >= n_all && n_all * frame_row_bytes(*out) <= (4u << 20)) {
        // A small call -- the reference's own loop asks for ONE pose per call (s3dis_simulator.py:254-264): everything on
        // one stream and ONE synchronisation.  The rows are copied at their worst-case length together with the counts
        // (a pose's rows are ~1 MB: cheaper than a second round trip to learn the exact length first).
        hipStream_t cs = ctx->s_compute;
        TraceParams q = p;
        q.out = st.rec;
        lrc_scan_options saved = s->opts;
        q.range_noise = nullptr;
        if (noise) { s->opts.range_noise = noise; s->opts.range_noise_len = q.total; }
        rc = launch_trace(s, q, gen, cs);
        s->opts = saved;
        if (rc) return rc;
        if ((rc = lrc_compact_dev(ctx, P, N, &st.io, cs))) return rc;
        LRC_HIP(hipMemcpyAsync(ctx->h_counts, st.io.counts, P * 8, hipMemcpyDeviceToHost, cs));
        if (st.d_stats && (rc = enqueue_frame_stats(ctx, st, out, P, 0, P, 0, cs))) return rc;
        if ((rc = copy_frame_rows(*out, st.io, 0, 0, n_all, cs))) return rc;
        LRC_HIP(hipStreamSynchronize(cs));
        uint64_t K1 = 0;
        for (uint64_t k = 0; k < P; ++k) {
            out->counts[k] = ctx->h_counts[k];
            K1 += ctx->h_counts[k];
        }
        publish_frame_stats(ctx, out, P);
        if (out_total) *out_total = K1;
        return LRC_OK;
    }
    uint64_t p0 = 0;
    for (uint64_t c = 0; c < chunks; ++c) {
        const uint64_t p1 = chunk_end(c), np_ = p1 - p0, r0 = p0 * N;
        TraceParams q = p;
        if (q.poses16) q.poses16 = p.poses16 + p0 * 16;
        if (q.motion24) q.motion24 = p.motion24 + p0 * 24;
        q.noise.first_frame = p.noise.first_frame + p0;      // the generators that draw noise: the chunk's first frame id
        // (angles2 shares its slot with ray_tab: only lrc_pipe_submit sets a table and it never comes through this chunked
        // path -- a launch with a table must not be given an offset here)
        if (q.angles2) q.angles2 = p.angles2 + r0 * 2;
        if (q.rays6) q.rays6 = p.rays6 + r0 * 6;
        if (q.seg_centers3) q.seg_centers3 = p.seg_centers3 + p0 * 3;
        if (q.keep_mask) q.keep_mask = p.keep_mask + r0;
        q.total = np_ * N;
        q.range_noise = nullptr;
        lrc_scan_options saved = s->opts;
        if (noise) { s->opts.range_noise = noise + r0; s->opts.range_noise_len = q.total; }
        // the chunk's part of the record set, which is also what its compaction reads, and of the compacted arrays
        q.out = st.rec;
        lrc_compact_io io = st.io;
        (void)record_columns([&](auto hit, auto in, size_t per_ray) -> int {
            if (st.rec.*hit) q.out.*hit = st.rec.*hit + r0 * per_ray;
            io.*in = q.out.*hit;
            return LRC_OK;
        });
        q.out.tile_count = st.rec.tile_count + blocks_of(r0, 64);
        io.tile_count = q.out.tile_count;
        io.counts = st.io.counts + p0;
        (void)frame_columns([&](auto, auto dev, size_t per_row) -> int {
            if (io.*dev) io.*dev = st.io.*dev + r0 * per_row;
            return LRC_OK;
        });
        rc = launch_trace(s, q, gen, ctx->s_compute);
        s->opts = saved;
        if (rc) return rc;
        if ((rc = lrc_compact_dev(ctx, np_, N, &io, ctx->s_compute))) return rc;
        LRC_HIP(hipMemcpyAsync(ctx->h_counts + p0, st.io.counts + p0, np_ * 8, hipMemcpyDeviceToHost, ctx->s_compute));
        LRC_HIP(hipEventRecord(ctx->ev_chunk[c], ctx->s_compute));
        if (st.d_stats) {
            // on a stream of their own: the statistics need this chunk's compaction and nothing else, so they run beside
            // the next chunk's trace and the row transfers
            LRC_HIP(hipStreamWaitEvent(ctx->s_stats, ctx->ev_chunk[c], 0));
            if ((rc = enqueue_frame_stats(ctx, st, out, P, p0, np_, r0, ctx->s_stats))) return rc;
        }
        p0 = p1;
    }
    uint64_t K = 0;
    int status = LRC_OK;
    p0 = 0;
    for (uint64_t c = 0; c < chunks; ++c) {
        const uint64_t p1 = chunk_end(c), r0 = p0 * N;
        LRC_HIP(hipEventSynchronize(ctx->ev_chunk[c]));
        uint64_t Kc = 0;
        for (uint64_t k = p0; k < p1; ++k) { out->counts[k] = ctx->h_counts[k]; Kc += ctx->h_counts[k]; }
        if (K + Kc > capacity) status = LRC_ERR_INVALID_ARG;        // keep counting: the caller learns the size needed
        if (status == LRC_OK && Kc && (rc = copy_frame_rows(*out, st.io, r0, K, Kc, ctx->s_copy))) return rc;
        K += Kc;
        p0 = p1;
    }
    LRC_HIP(hipStreamSynchronize(ctx->s_copy));
    LRC_HIP(hipStreamSynchronize(ctx->s_compute));
    if (st.d_stats) {
        LRC_HIP(hipStreamSynchronize(ctx->s_stats));
        publish_frame_stats(ctx, out, P);
    }
    if (out_total) *out_total = K;
    if (status != LRC_OK)
        return fail(LRC_ERR_INVALID_ARG, "frame buffers too small: capacity " + std::to_string(capacity) +
                                             " rows, the scan kept " + std::to_string(K));
    return LRC_OK;
}

// What the *_compact entry points share from their SyncUnlessOk guard on.  The entry point has checked its arguments, made
// the device current and filled what is its own in `p`; `inputs(up)` stages its input arrays with up(pool slot, host array,
// elements, &device pointer in p), on the compute stream, which consumes them.  Here: the frame stage, the scene's host
// noise array, the common TraceParams fields and frames_finish.  gen: the generator (launch_trace); `grid`: a grid scan.
template <class Inputs>
int scan_compact(lrc_scene* s, TraceParams& p, int gen, uint64_t P, uint64_t N, double max_range, const lrc_frames* out,
                 uint64_t capacity, uint64_t* out_total, Inputs&& inputs, const lrc_grid* grid = nullptr) {
    SyncUnlessOk guard;      // constructed before the first asynchronous upload, destroyed after everything below
    lrc_ctx* const ctx = s->ctx;
    const uint64_t n = P * N;
    int rc;
    if ((rc = ensure_streams(ctx))) return rc;
    const hipStream_t in = ctx->s_compute;
    if ((rc = inputs([&](int slot, auto* host, size_t count, auto** dev) { return stage_input(ctx, slot, host, count, dev, &in); })))
        return rc;
    FrameStage st;
    if ((rc = st.alloc(ctx, *out, P, n))) return rc;
    NoiseStage ns;           // restores the scene's host pointer on every exit
    if (!gen_draws_noise(gen) && (rc = ns.begin(s, n))) return rc;      // (those draw their own noise and have refused a range_noise option)
    scan_fields(p, N, n, max_range, nullptr);
    s->cur_grid = grid;
    rc = frames_finish(s, p, gen, st, P, N, out, capacity, out_total);
    s->cur_grid = nullptr;
    return guard.done(rc);
}

// lrc_scan_poses_compact, and behind their own checks lrc_scan_table_compact (d_dirs3: the resident table, nothing to upload)
// and lrc_scan_grid_compact.  The messages say lrc_scan_poses_compact for all three callers: callers match on them.
int scan_compact_impl(lrc_scene* s, const double* poses16, uint64_t P, const double* dirs3, uint64_t N,
                      const lrc_grid* grid, double max_range, const lrc_frames* out, uint64_t capacity,
                      uint64_t* out_total, const double* d_dirs3 = nullptr) {
    if (out_total) *out_total = 0;
    if (!s || !out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_poses_compact: NULL scene or output");
    if (!(P * N)) return LRC_OK;
    if (!poses16 || (!dirs3 && !d_dirs3) || !out->counts)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_poses_compact: poses16, dirs3 or counts is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    p.dirs3 = d_dirs3;
    return scan_compact(s, p, grid ? kGenGrid : kGenPoses, P, N, max_range, out, capacity, out_total, [&](auto up) {
        int rc = up(kPoolPoses, poses16, P * 16, &p.poses16);
        if (rc || d_dirs3) return rc;
        return up(kPoolDirs, dirs3, N * 3, &p.dirs3);
    }, grid);
}
}  // namespace

// ---- per-ray columns beside the record set, for the kept rows ----------------------------------------------------------------
// A scan family whose records carry a column a frame has no place for (the echo weight; intensity, bounces and surface points
// of the material scan) keeps it at the fixed stride and gathers it for the kept rows by the compacted index column: row r of
// the compacted arrays belongs to the pose whose run [prefix[p], prefix[p + 1]) holds it; its record is that pose's
// index[r]-th.  One thread per row; the prefix is small (P + 1 values) and searched by bisection.  W: the column's word
// (uint8_t or a 4-byte word), `words` of them per record.
namespace {
template <class W>
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint64_t* __restrict__ prefix, uint32_t P,
                                                          const uint32_t* __restrict__ index, const W* __restrict__ src,
                                                          uint32_t words, uint64_t records_per_pose, uint64_t rows,
                                                          W* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= rows) return;
    uint32_t lo = 0, hi = P;           // prefix[lo] <= r < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= r) lo = mid; else hi = mid;
    }
    const uint32_t i = index[r];
    const bool ok = i < records_per_pose;
    const uint64_t from = ((uint64_t)lo * records_per_pose + (ok ? i : 0u)) * words;
    for (uint32_t w = 0; w < words; ++w) out[r * words + w] = ok ? src[from + w] : (W)0;
}

struct GatherColumn {
    const void* d_src;       // device: the column at the fixed stride; NULL: skipped
    void* host_dst;          // host: `rows` records; NULL: skipped
    uint32_t word_bytes;     // 1 or 4
    uint32_t words;          // per record
};

// `who` prefixes the messages; counts: host, per pose, adding up to `rows`
int gather_rows_by_index(const char* who, const uint64_t* counts, uint64_t P, const uint32_t* d_index, uint64_t records_per_pose,
                         uint64_t rows, const GatherColumn* cols, int ncols) {
    if (!rows) return LRC_OK;
    if (P > 0x7FFFFFFFull || blocks_of(rows, 256) > 0x7FFFFFFFull)
        return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": too many poses or rows for the gather of the per-ray columns");
    std::vector<uint64_t> prefix(P + 1, 0);
    for (uint64_t p = 0; p < P; ++p) prefix[p + 1] = prefix[p] + counts[p];
    if (prefix[P] != rows) return fail(LRC_ERR_INTERNAL, std::string(who) + ": counts do not add up to the kept rows");
    Buf d_prefix;
    LRC_HIP(hipMalloc(&d_prefix.p, (P + 1) * 8));
    LRC_HIP(hipMemcpy(d_prefix.p, prefix.data(), (P + 1) * 8, hipMemcpyHostToDevice));
    const dim3 grid((uint32_t)blocks_of(rows, 256));
    for (int c = 0; c < ncols; ++c) {
        const GatherColumn& g = cols[c];
        if (!g.d_src || !g.host_dst) continue;
        const size_t bytes = (size_t)rows * g.word_bytes * g.words;
        Buf d_out;
        LRC_HIP(hipMalloc(&d_out.p, bytes));
        if (g.word_bytes == 1)
            hipLaunchKernelGGL(gather_rows_kernel<uint8_t>, grid, dim3(256), 0, nullptr, (const uint64_t*)d_prefix.p, (uint32_t)P, d_index,
                               (const uint8_t*)g.d_src, g.words, records_per_pose, rows, (uint8_t*)d_out.p);
        else
            hipLaunchKernelGGL(gather_rows_kernel<uint32_t>, grid, dim3(256), 0, nullptr, (const uint64_t*)d_prefix.p, (uint32_t)P, d_index,
                               (const uint32_t*)g.d_src, g.words, records_per_pose, rows, (uint32_t*)d_out.p);
        LRC_HIP(hipGetLastError());
        LRC_HIP(hipMemcpy(g.host_dst, d_out.p, bytes, hipMemcpyDeviceToHost));
    }
    return LRC_OK;
}
}  // namespace

// lrc_scan_echoes_compact behind its checks (lrc_echo.hip; declared in lrc_internal.h).  The echo records are compacted by the
// path every *_compact entry point takes, as P poses of N * E records: `index` comes out as i * E + e.  No wave of the echo
// kernel writes 64 consecutive records, so the record set carries no per-tile keep counts and lrc_compact_dev counts itself.  The
// weights of the kept rows are gathered on the device by the compacted index column (gather_rows_by_index above).
int echo_scan_compact(lrc_scene* s, const double* poses16, uint64_t P, const lrc_table* table, const double* offsets2,
                      lrcecho::Params ep, double max_range, const lrc_frames* out, uint8_t* weight_rows, uint64_t capacity,
                      uint64_t* out_total) {
    SyncUnlessOk guard;
    lrc_ctx* const ctx = s->ctx;
    const uint64_t NE = table->n * ep.max_echoes, n = P * NE;
    int rc;
    if ((rc = ensure_streams(ctx))) return rc;
    const hipStream_t in = ctx->s_compute;
    TraceParams p{};
    p.dirs3 = table->d_dirs3;
    if ((rc = stage_input(ctx, kPoolPoses, poses16, P * 16, &p.poses16, &in)) ||
        (rc = stage_input(ctx, kPoolOffs, offsets2, (size_t)ep.subrays * 2, &ep.offsets2, &in)))
        return rc;
    FrameStage st;
    if ((rc = st.alloc(ctx, *out, P, n))) return rc;
    st.rec.tile_count = nullptr;
    st.io.tile_count = nullptr;
    DevBuf wbuf;
    ep.weight = nullptr;
    if (weight_rows) {
        if (!st.io.out_index) {       // the gather reads the index column whether or not the caller asked for it
            if ((rc = st.oidx.get(ctx, kPoolOutIdx, n * 4))) return rc;
            st.io.out_index = (uint32_t*)st.oidx.p;
        }
        if ((rc = wbuf.get(ctx, kPoolKeep, n))) return rc;
        ep.weight = (uint8_t*)wbuf.p;
    }
    p.echo = ep;
    scan_fields(p, NE, n, max_range, nullptr);
    uint64_t total = 0;
    rc = frames_finish(s, p, kGenEchoes, st, P, NE, out, capacity, &total);
    if (out_total) *out_total = total;
    if (rc == LRC_OK && weight_rows && total) {
        const GatherColumn col{ep.weight, weight_rows, 1, 1};
        rc = gather_rows_by_index("lrc_scan_echoes_compact", out->counts, P, st.io.out_index, NE, total, &col, 1);
    }
    return guard.done(rc);
}

// lrc_scan_materials_compact behind its checks (lrc_material.hip; declared in lrc_internal.h): the path every *_compact entry
// point takes, with three per-ray columns a frame has no place for -- the intensity of the record set, bounces and surface points
// -- in buffers of their own (pool slots), gathered for the kept rows on the device by the compacted index column
// (gather_rows_by_index above).
int material_scan_compact(lrc_scene* s, const double* poses16, uint64_t P, const lrc_table* table, lrcmat::Params mp,
                          double max_range, const lrc_frames* out, float* intensity_rows, uint8_t* bounces_rows, float* surface_rows,
                          uint64_t capacity, uint64_t* out_total) {
    SyncUnlessOk guard;
    lrc_ctx* const ctx = s->ctx;
    const uint64_t N = table->n, n = P * N;
    int rc;
    if ((rc = ensure_streams(ctx))) return rc;
    const hipStream_t in = ctx->s_compute;
    TraceParams p{};
    p.dirs3 = table->d_dirs3;
    if ((rc = stage_input(ctx, kPoolPoses, poses16, P * 16, &p.poses16, &in))) return rc;
    FrameStage st;
    if ((rc = st.alloc(ctx, *out, P, n))) return rc;
    const bool gather = intensity_rows || bounces_rows || surface_rows;
    if (gather && !st.io.out_index) {       // the gather reads the index column whether or not the caller asked for it
        if ((rc = st.oidx.get(ctx, kPoolOutIdx, n * 4))) return rc;
        st.io.out_index = (uint32_t*)st.oidx.p;
    }
    DevBuf ibuf, bbuf, sbuf;
    mp.bounces = nullptr;
    mp.surface3 = nullptr;
    if (intensity_rows) {
        if ((rc = ibuf.get(ctx, kPoolInten, n * 4))) return rc;
        st.rec.intensity = (float*)ibuf.p;
    }
    if (bounces_rows) {
        if ((rc = bbuf.get(ctx, kPoolKeep, n))) return rc;
        mp.bounces = (uint8_t*)bbuf.p;
    }
    if (surface_rows) {
        if ((rc = sbuf.get(ctx, kPoolNormal, n * 12))) return rc;      // no frame column lives in the normals' slot
        mp.surface3 = (float*)sbuf.p;
    }
    p.mat = mp;
    scan_fields(p, N, n, max_range, nullptr);
    uint64_t total = 0;
    rc = frames_finish(s, p, kGenMaterials, st, P, N, out, capacity, &total);
    if (out_total) *out_total = total;
    if (rc == LRC_OK && gather && total) {
        const GatherColumn cols[3] = {{st.rec.intensity, intensity_rows, 4, 1}, {mp.bounces, bounces_rows, 1, 1}, {mp.surface3, surface_rows, 4, 3}};
        rc = gather_rows_by_index("lrc_scan_materials_compact", out->counts, P, st.io.out_index, N, total, cols, 3);
    }
    return guard.done(rc);
}

// ---- moving objects: the four lrc_scan_*movers*_dev calls behind their checks (lrc_movers.hip; declared in lrc_internal.h) ----
namespace {
// The explicit-ray launch as lrc_cast_dev makes it with no centre and no filter, whatever options the scene carries: the
// ranges the merge compares are taken before any filter.  d_keep: nullable, 0 = the ray is not cast (a miss).
int cast_plain(lrc_scene* sc, const float* d_rays6, const uint8_t* d_keep, uint64_t n, const lrc_hits& out, hipStream_t st) {
    TraceParams p{};
    p.rays6 = d_rays6;
    p.keep_mask = d_keep;
    scan_fields(p, n, n, (double)__builtin_inff(), &out, false);
    const lrc_scan_options saved = sc->opts;
    sc->opts = lrc_scan_options{};
    const int rc = launch_trace(sc, p, kGenRays, st);
    sc->opts = saved;
    return rc;
}

// The scratch of the mover and flow scans: `count` columns of width[k] bytes per ray for n rays, each 256-byte aligned, column k
// at off[k].  A block that is too small is replaced by one an eighth larger than is needed.
int scratch_columns(void*& block, uint64_t& cap, uint64_t n, const uint32_t* width, int count, uint64_t* off) {
    uint64_t end = 0;
    for (int k = 0; k < count; ++k) {
        off[k] = end;
        end += (n * width[k] + 255u) & ~(uint64_t)255u;
    }
    if (cap < end) {
        // (hipFree waits for the device: nothing enqueued earlier still reads the old block)
        if (block) { (void)hipFree(block); block = nullptr; cap = 0; }
        LRC_HIP(hipMalloc(&block, end + end / 8));
        cap = end + end / 8;
    }
    return LRC_OK;
}
}  // namespace

// All on `st`, nothing waited for.  c.fire selects SWEEP and c.noise NOISY (the kernels' two switches).  A NULL set: the launch of
// the variant's plain scan (lrc_scan_poses_dev, lrc_scan_noisy_dev, lrc_scan_sweeps_dev, lrc_scan_noisy_sweeps_dev) and a zero
// mover column.  Otherwise
//   the static pass    mover_rays_kernel (the world rays; NOISY: and the live bytes) and the explicit-ray launch on the scene
//                      (NOISY: under the live bytes, a dropped ray is never cast), into the winner's columns
//   per mover m        mover_rays_kernel (object-frame rays + keep bytes), the explicit-ray launch on the mover's scene -- or,
//                      under SWEEP for the scene of a spanned deformable, the per-ray-shape cast of lrc_span.hip (span_cast: the
//                      same five columns, the same firing fractions) --, and mover_merge_kernel, whose
//                      last pass writes the caller's records
// in the set's scratch, which holds one ray set, one keep column and two record sets (winner, mover) whatever M is: 74 bytes per
// ray, and in front of them the stored world ray set unless the scan is neither SWEEP nor NOISY (+24) and NOISY's live column (+1).
int movers_scan_dev(lrc_scene* s, lrc_movers* set, const MoverScan& c, const lrc_hits* d_out, uint8_t* d_mover, hipStream_t st) {
    const bool sweep = c.fire != nullptr, noisy = c.noise != nullptr, stored = sweep || noisy;
    const uint64_t N = c.N, n = c.P * N;
    if (!n) return LRC_OK;
    const lrcnoise::Params np = noisy ? *c.noise : lrcnoise::Params{};
    TraceParams p{};       // what the plain scan, write_back and the range draw read: the scan's inputs, the model, the filter, the caller's records
    p.noise = np;
    (sweep ? p.motion24 : p.poses16) = c.sensor;
    p.dirs3 = c.dirs3;
    p.fire = c.fire;
    scan_fields(p, N, n, c.max_range, d_out);
    int rc;
    if (!set) {
        if ((rc = launch_trace(s, p, sweep ? (noisy ? kGenNoisySweeps : kGenSweeps) : (noisy ? kGenNoisy : kGenPoses), st))) return rc;
        if (d_mover) LRC_HIP(hipMemsetAsync(d_mover, 0, n, st));
        return LRC_OK;
    }
    if (c.P > 0xFFFFFFFFull || blocks_of(n, kBlock) > 0x7FFFFFFFull)
        return fail(LRC_ERR_INVALID_ARG, std::string("lrc_scan_") + (noisy ? "noisy_" : "") +
                                             (sweep ? "mover_sweeps: too many sweeps" : "movers: too many poses") + " or rays for one call");
    // scratch columns: [world6] | [live] | rays6 | keep | winner (t, prim, normal3, sem, ins, who) | mover (t, prim, normal3, sem, ins)
    uint32_t width[15];
    int cols = 0;
    if (stored) width[cols++] = 24;
    if (noisy) width[cols++] = 1;
    const int first = cols;
    for (uint32_t bytes : {24u, 1u, 4u, 4u, 12u, 2u, 2u, 1u, 4u, 4u, 12u, 2u, 2u}) width[cols++] = bytes;
    uint64_t off[15];
    if ((rc = scratch_columns(set->scratch, set->scratch_cap, n, width, cols, off))) return rc;
    uint8_t* const b = (uint8_t*)set->scratch;
    float* const world6 = stored ? (float*)(b + off[0]) : nullptr;
    uint8_t* const live = noisy ? b + off[1] : nullptr;
    const uint64_t* const o = off + first;
    float* const rays6 = (float*)(b + o[0]);
    uint8_t* const keep = b + o[1];
    lrc_hits w{}, mv{};
    w.t = (float*)(b + o[2]); w.prim = (uint32_t*)(b + o[3]); w.normal3 = (float*)(b + o[4]);
    w.sem = (uint16_t*)(b + o[5]); w.ins = (uint16_t*)(b + o[6]);
    uint8_t* const who = b + o[7];
    mv.t = (float*)(b + o[8]); mv.prim = (uint32_t*)(b + o[9]); mv.normal3 = (float*)(b + o[10]);
    mv.sem = (uint16_t*)(b + o[11]); mv.ins = (uint16_t*)(b + o[12]);
    auto* const rays_kernel = sweep ? (noisy ? mover_rays_kernel<true, true> : mover_rays_kernel<true, false>)
                                    : (noisy ? mover_rays_kernel<false, true> : mover_rays_kernel<false, false>);
    auto* const merge_kernel = sweep ? (noisy ? mover_merge_kernel<true, true> : mover_merge_kernel<true, false>)
                                     : (noisy ? mover_merge_kernel<false, true> : mover_merge_kernel<false, false>);
    const dim3 grid((uint32_t)blocks_of(n, kBlock));
    const int uniform = N % 64 == 0;
    const uint32_t M = (uint32_t)set->scenes.size();
    lrcmov::RayPass rp{};
    hipLaunchKernelGGL(rays_kernel, grid, dim3(kBlock), 0, st, c.sensor, c.dirs3, c.fire, np, N, n, rp, uniform, world6, live, rays6, keep);
    LRC_HIP(hipGetLastError());
    if ((rc = cast_plain(s, stored ? world6 : rays6, live, n, w, st))) return rc;
    LRC_HIP(hipMemsetAsync(who, 0, n, st));
    p.min_range = s->opts.min_range;       // the scene's options, as launch_trace would set them
    p.incident_mode = s->opts.incident_mode;
    for (uint32_t m = 0; m < M; ++m) {
        lrc_scene* const ms = set->scenes[m];
        rp.records = c.movers;
        rp.M = M;
        rp.m = m;
        rp.sphere = lrcmov::bounding_sphere(ms->info.bounds_lo, ms->info.bounds_hi);
        hipLaunchKernelGGL(rays_kernel, grid, dim3(kBlock), 0, st, c.sensor, c.dirs3, c.fire, np, N, n, rp, uniform, world6, live, rays6, keep);
        LRC_HIP(hipGetLastError());
        // under SWEEP a spanned deformable (lrc_deform_span_dev) is met per ray at the shape of the ray's own s (lrc_span.hip)
        if ((rc = (sweep && ms->deform && ms->deform->spanned) ? span_cast(ms->deform, rays6, keep, c.fire, N, n, mv, st)
                                                                : cast_plain(ms, rays6, keep, n, mv, st)))
            return rc;
        MoverMerge q{};
        q.records = c.movers; q.world6 = world6; q.M = M; q.m = m; q.uniform = uniform; q.last = m + 1 == M;
        q.w_t = w.t; q.w_prim = w.prim; q.w_n3 = w.normal3; q.w_sem = w.sem; q.w_ins = w.ins; q.w_who = who;
        q.m_t = mv.t; q.m_prim = mv.prim; q.m_n3 = mv.normal3; q.m_sem = mv.sem; q.m_ins = mv.ins;
        q.d_mover = d_mover;
        hipLaunchKernelGGL(merge_kernel, grid, dim3(kBlock), 0, st, p, q);
        LRC_HIP(hipGetLastError());
    }
    return LRC_OK;
}

// lrc_scan_flow_dev behind its checks (lrc_flow.hip).  All on `st`, nothing waited for:
//   the ray kernel     flow_rays_kernel: the flow and, with d_status, the world line of sight, its cast byte, thr, the first status
//                      (nonrigid_target_kernel instead when the call brings surface pairs)
//   the static pass    the explicit-ray launch on the scene, straight into the running minimum
//   per mover m        flow_object_rays_kernel (object-frame rays by the NEXT pose + keep bytes), the explicit-ray launch on the
//                      mover's scene, flow_merge_kernel; the last merge writes the status
// in the set's scratch (the scene's own without a set): two ray sets, two byte columns and three float columns whatever M is.
int flow_scan_dev(lrc_scene* s, lrc_movers* set, const lrc_hits* d_rec, const uint8_t* d_mover, uint64_t P, uint64_t N,
                  const float* d_mover_poses12, const FlowNext& next, double max_range, float* d_flow3, uint8_t* d_status,
                  hipStream_t st, const FlowPairs* pairs) {
    const uint64_t n = P * N;
    if (!n) return LRC_OK;
    if (P > 0xFFFFFFFFull || blocks_of(n, kBlock) > 0x7FFFFFFFull)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_flow: too many poses or rays for one call");
    const dim3 grid((uint32_t)blocks_of(n, kBlock));
    const uint32_t M = set ? (uint32_t)set->scenes.size() : 0u;
    FlowRays fr{};
    fr.t = d_rec->t; fr.point3 = d_rec->point3; fr.mover = set ? d_mover : nullptr;
    fr.A = d_mover_poses12; fr.B = next.next_mover_poses12;
    fr.next16 = next.next_poses16; fr.has_next = next.has_next;
    fr.M = M; fr.rays_per_pose = N; fr.total = n;
    fr.max_range = max_range; fr.min_range = s->opts.min_range;
    fr.flow3 = d_flow3;
    // with surface pairs (lrc_scan_nonrigid_flow_dev) the non-rigid ray kernel stands in for the rigid one; the passes behind it
    // are the same
    auto ray_kernel = [&]() {
        if (pairs && pairs->count) hipLaunchKernelGGL(nonrigid_target_kernel, grid, dim3(kBlock), 0, st, fr, *pairs);
        else hipLaunchKernelGGL(flow_rays_kernel, grid, dim3(kBlock), 0, st, fr);
    };
    if (!d_status) {
        ray_kernel();
        LRC_HIP(hipGetLastError());
        return LRC_OK;
    }
    // scratch columns: world rays6 | object rays6 | cast | keep | thr | t_min | t_mover
    const uint32_t width[7] = {24, 24, 1, 1, 4, 4, 4};
    uint64_t off[7];
    void*& block = set ? set->scratch : s->flow_scratch;
    int rc;
    if ((rc = scratch_columns(block, set ? set->scratch_cap : s->flow_scratch_cap, n, width, 7, off))) return rc;
    uint8_t* const b = (uint8_t*)block;
    float* const world6 = (float*)(b + off[0]);
    float* const obj6 = (float*)(b + off[1]);
    uint8_t* const cast = b + off[2];
    uint8_t* const keep = b + off[3];
    float* const thr = (float*)(b + off[4]);
    lrc_hits w{}, mv{};
    w.t = (float*)(b + off[5]);
    mv.t = (float*)(b + off[6]);
    fr.rays6 = world6; fr.keep = cast; fr.thr = thr; fr.status = d_status;
    ray_kernel();
    LRC_HIP(hipGetLastError());
    if ((rc = cast_plain(s, world6, cast, n, w, st))) return rc;
    const int uniform = N % 64 == 0;
    for (uint32_t m = 0; m < M; ++m) {
        lrc_scene* const ms = set->scenes[m];
        lrcmov::RayPass rp{};
        rp.records = next.next_mover_poses12;
        rp.M = M;
        rp.m = m;
        rp.sphere = lrcmov::bounding_sphere(ms->info.bounds_lo, ms->info.bounds_hi);
        hipLaunchKernelGGL(flow_object_rays_kernel, grid, dim3(kBlock), 0, st, world6, cast, N, n, rp, uniform, obj6, keep);
        LRC_HIP(hipGetLastError());
        if ((rc = cast_plain(ms, obj6, keep, n, mv, st))) return rc;
        hipLaunchKernelGGL(flow_merge_kernel, grid, dim3(kBlock), 0, st, w.t, mv.t, thr, cast, n, (int)(m + 1 == M), d_status);
        LRC_HIP(hipGetLastError());
    }
    if (!M) {
        hipLaunchKernelGGL(flow_merge_kernel, grid, dim3(kBlock), 0, st, w.t, (const float*)nullptr, thr, cast, n, 1, d_status);
        LRC_HIP(hipGetLastError());
    }
    return LRC_OK;
}

// Host sensor records, a resident direction table: the records at the fixed stride by movers_scan_dev on the context's compute
// stream, compacted by lrc_compact_dev (which counts itself: the merge kernel writes no per-tile keep counts); the counts come
// home first, then exactly the kept rows.  The mover column stays at the fixed stride and is gathered for the kept rows by the
// compacted index column (gather_rows_by_index above).
// With `sweep`: `sensor` holds P (P,24) motion records (else (P,16) poses), `movers` the (P, M, 24) mover sweep records (else
// (P, M, 12) poses), and the table brings its fire table.  With `noise` the scan is noisy: the one call traces every pose at once
// (no pose chunks), pose or sweep p of the call is frame first_frame + p throughout.
// With `flow` (flow_scan_compact): the flow and its status at the fixed stride behind the mover scan, gathered like the mover column.
int movers_scan_compact(lrc_scene* s, lrc_movers* set, const double* sensor, uint64_t P, const lrc_table* table, const float* movers,
                        double max_range, bool sweep, const lrcnoise::Params* noise, const lrc_frames* out, uint8_t* mover_rows,
                        uint64_t capacity, uint64_t* out_total, const FlowCompact* flow) {
    const std::string who = flow ? "lrc_scan_flow_compact"
                                 : std::string("lrc_scan_") + (noise ? "noisy_" : "") + (sweep ? "mover_sweeps_compact" : "movers_compact");
    SyncUnlessOk guard;
    lrc_ctx* const ctx = s->ctx;
    const uint64_t N = table->n, n = P * N;
    int rc;
    if ((rc = ensure_streams(ctx))) return rc;
    const hipStream_t cs = ctx->s_compute;
    struct Drain {
        hipStream_t st;
        ~Drain() { (void)hipStreamSynchronize(st); }
    } drain{cs};
    const double* d_poses = nullptr;
    const float* d_mp = nullptr;
    if ((rc = stage_input(ctx, kPoolPoses, sensor, P * (sweep ? 24 : 16), &d_poses, &cs))) return rc;
    if (set && (rc = stage_input(ctx, kPoolNoise, movers, P * set->scenes.size() * (sweep ? 24 : 12), &d_mp, &cs))) return rc;
    FrameStage st;
    if ((rc = st.alloc(ctx, *out, P, n))) return rc;
    st.rec.tile_count = nullptr;
    st.io.tile_count = nullptr;
    const bool want_flow = flow && (flow->flow_rows || flow->status_rows);
    if ((mover_rows || want_flow) && !st.io.out_index) {       // the gather reads the index column whether or not the caller asked for it
        if ((rc = st.oidx.get(ctx, kPoolOutIdx, n * 4))) return rc;
        st.io.out_index = (uint32_t*)st.oidx.p;
    }
    DevBuf mbuf, p3buf, fbuf, sbuf;
    if ((mover_rows || (want_flow && set)) && (rc = mbuf.get(ctx, kPoolKeep, n))) return rc;
    FlowNext d_next{};
    if (want_flow) {
        // the flow reads point3 whether or not a frame column needs it; no frame column lives in the slots of the two flow columns
        if (!st.rec.point3) {
            if ((rc = p3buf.get(ctx, kPoolPoint, n * 12))) return rc;
            st.rec.point3 = (float*)p3buf.p;
        }
        if ((rc = fbuf.get(ctx, kPoolNormal, n * 12))) return rc;
        if (flow->status_rows && (rc = sbuf.get(ctx, kPoolAngles, n))) return rc;
        if ((rc = stage_input(ctx, kPoolCen, flow->next.next_poses16, P * 16, &d_next.next_poses16, &cs))) return rc;
        if (set && (rc = stage_input(ctx, kPoolOffs, flow->next.next_mover_poses12, P * set->scenes.size() * 12,
                                     &d_next.next_mover_poses12, &cs)))
            return rc;
        if (flow->next.has_next && (rc = stage_input(ctx, kPoolRays, flow->next.has_next, P, &d_next.has_next, &cs))) return rc;
    }
    if (ctx->h_counts_cap < P) {
        if (ctx->h_counts) { (void)hipHostFree(ctx->h_counts); ctx->h_counts = nullptr; ctx->h_counts_cap = 0; }
        LRC_HIP(hipHostMalloc((void**)&ctx->h_counts, (P + P / 4 + 64) * 8 * 5, hipHostMallocDefault));
        ctx->h_counts_cap = P + P / 4 + 64;
    }
    const MoverScan scan{d_poses, table->d_dirs3, sweep ? table->d_fire : nullptr, d_mp, noise, P, N, max_range};
    if ((rc = movers_scan_dev(s, set, scan, &st.rec, (uint8_t*)mbuf.p, cs))) return rc;
    if (want_flow && (rc = flow_scan_dev(s, set, &st.rec, (const uint8_t*)mbuf.p, P, N, d_mp, d_next, max_range, (float*)fbuf.p,
                                         (uint8_t*)sbuf.p, cs)))
        return rc;
    if ((rc = lrc_compact_dev(ctx, P, N, &st.io, cs))) return rc;
    LRC_HIP(hipMemcpyAsync(ctx->h_counts, st.io.counts, P * 8, hipMemcpyDeviceToHost, cs));
    if (st.d_stats && (rc = enqueue_frame_stats(ctx, st, out, P, 0, P, 0, cs))) return rc;
    LRC_HIP(hipStreamSynchronize(cs));
    uint64_t K = 0;
    for (uint64_t k = 0; k < P; ++k) { out->counts[k] = ctx->h_counts[k]; K += ctx->h_counts[k]; }
    if (out_total) *out_total = K;
    if (K > capacity)
        return guard.done(fail(LRC_ERR_INVALID_ARG, "frame buffers too small: capacity " + std::to_string(capacity) +
                                                        " rows, the scan kept " + std::to_string(K)));
    if (K && (rc = copy_frame_rows(*out, st.io, 0, 0, K, cs))) return rc;
    LRC_HIP(hipStreamSynchronize(cs));
    publish_frame_stats(ctx, out, P);
    if ((mover_rows || want_flow) && K) {
        const GatherColumn cols[3] = {{mbuf.p, mover_rows, 1, 1},
                                      {fbuf.p, flow ? flow->flow_rows : nullptr, 4, 3},
                                      {sbuf.p, flow ? flow->status_rows : nullptr, 1, 1}};
        rc = gather_rows_by_index(who.c_str(), out->counts, P, st.io.out_index, N, K, cols, 3);
    }
    return guard.done(rc);
}

// Host check of (P,24) motion records (lrc_scan_sweeps_compact): finite, dq.w >= cos(pi/4) (a rotation of at most pi/2 per
// sweep, where the nlerp error table of include/lidarcast.h holds), |dq| = 1 to 1e-6.  Declared in lrc_internal.h: the checks of
// lrc_scan_mover_sweeps_compact (lrc_movers.hip) make it too.
int check_motion(const char* who, const double* m, uint64_t P) {
    constexpr double kCosQuarterPi = 0.70710678118654752440;
    for (uint64_t k = 0; k < P; ++k) {
        const double* r = m + k * 24;
        for (int j = 0; j < 24; ++j)
            if (!std::isfinite(r[j]))
                return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": record " + std::to_string(k) + " is not finite");
        if (r[12] < kCosQuarterPi)
            return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": record " + std::to_string(k) +
                                                 " rotates by more than pi/2 per sweep (dq.w < cos(pi/4))");
        const double n = ((r[12] * r[12] + r[13] * r[13]) + r[14] * r[14]) + r[15] * r[15];
        if (!(std::fabs(n - 1.0) <= 1e-6))
            return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": record " + std::to_string(k) + " has a non-unit dq");
    }
    return LRC_OK;
}

int flow_scan_compact(lrc_scene* s, lrc_movers* set, const double* poses16, uint64_t P, const lrc_table* table,
                      const float* mover_poses12, const FlowNext& next, double max_range, const lrc_frames* out, uint8_t* mover_rows,
                      float* flow_rows, uint8_t* status_rows, uint64_t capacity, uint64_t* out_total) {
    const FlowCompact flow{next, flow_rows, status_rows};
    return movers_scan_compact(s, set, poses16, P, table, mover_poses12, max_range, false, nullptr, out, mover_rows, capacity, out_total, &flow);
}

extern "C" {

int lrc_host_alloc(lrc_ctx* ctx, uint64_t bytes, void** out_ptr) {
    if (!ctx || !out_ptr) return fail(LRC_ERR_INVALID_ARG, "lrc_host_alloc: NULL argument");
    *out_ptr = nullptr;
    if (!bytes) return LRC_OK;
    LRC_HIP(hipSetDevice(ctx->device));
    LRC_HIP(hipHostMalloc(out_ptr, bytes, hipHostMallocDefault));
    return LRC_OK;
}

int lrc_host_free(lrc_ctx* ctx, void* ptr) {
    if (!ptr) return LRC_OK;
    if (ctx) (void)hipSetDevice(ctx->device);
    LRC_HIP(hipHostFree(ptr));
    return LRC_OK;
}

int lrc_table_create(lrc_ctx* ctx, const double* dirs3, uint64_t N, lrc_table** out_table) {
    if (!out_table) return fail(LRC_ERR_INVALID_ARG, "lrc_table_create: out_table is NULL");
    *out_table = nullptr;
    if (!ctx || !dirs3 || !N) return fail(LRC_ERR_INVALID_ARG, "lrc_table_create: NULL context / table or empty table");
    LRC_HIP(hipSetDevice(ctx->device));
    lrc_table* t = new (std::nothrow) lrc_table();
    if (!t) return fail(LRC_ERR_OOM, "lrc_table_create: out of host memory");
    t->ctx = ctx;
    t->n = N;
    hipError_t e = hipMalloc((void**)&t->d_dirs3, N * 24);
    if (e == hipSuccess) e = hipMemcpy(t->d_dirs3, dirs3, N * 24, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (t->d_dirs3) (void)hipFree(t->d_dirs3);
        delete t;
        return fail(e == hipErrorOutOfMemory ? LRC_ERR_OOM : LRC_ERR_HIP, std::string("lrc_table_create: ") + hipGetErrorString(e));
    }
    *out_table = t;
    return LRC_OK;
}

int lrc_table_destroy(lrc_table* t) {
    if (!t) return LRC_OK;
    if (t->ctx) (void)hipSetDevice(t->ctx->device);
    if (t->d_dirs3) (void)hipFree(t->d_dirs3);
    if (t->d_fire) (void)hipFree(t->d_fire);
    delete t;
    return LRC_OK;
}

int lrc_scan_table_compact(lrc_scene* s, const double* poses16, uint64_t P, const lrc_table* table, const lrc_grid* grid,
                           double max_range, const lrc_frames* out, uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    if (!table) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_table_compact: table is NULL");
    if (s && table->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_table_compact: table and scene belong to different contexts");
    if (grid) {
        int rc = check_grid("lrc_scan_table_compact", grid, table->n);
        if (rc) return rc;
    }
    return scan_compact_impl(s, poses16, P, nullptr, table->n, grid, max_range, out, capacity, out_total, table->d_dirs3);
}

int lrc_table_set_fire(lrc_table* t, const double* fire, uint64_t N) {
    if (!t) return fail(LRC_ERR_INVALID_ARG, "lrc_table_set_fire: table is NULL");
    if (!fire) {
        if (t->d_fire) { (void)hipSetDevice(t->ctx->device); (void)hipFree(t->d_fire); t->d_fire = nullptr; }
        return LRC_OK;
    }
    if (N != t->n) return fail(LRC_ERR_INVALID_ARG, "lrc_table_set_fire: the fire table must have one entry per ray of the table");
    for (uint64_t i = 0; i < N; ++i)
        if (!(fire[i] >= 0.0 && fire[i] < 1.0))     // NaN fails both
            return fail(LRC_ERR_INVALID_ARG, "lrc_table_set_fire: fire[" + std::to_string(i) + "] is outside [0, 1)");
    LRC_HIP(hipSetDevice(t->ctx->device));
    if (!t->d_fire) LRC_HIP(hipMalloc((void**)&t->d_fire, N * 8));
    LRC_HIP(hipMemcpy(t->d_fire, fire, N * 8, hipMemcpyHostToDevice));
    return LRC_OK;
}

int lrc_scan_sweeps_compact(lrc_scene* s, const double* motion24, uint64_t P, const lrc_table* table, double max_range,
                            const lrc_frames* out, uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    if (!s || !out || !table) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_sweeps_compact: NULL scene, table or output");
    if (table->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_sweeps_compact: table and scene belong to different contexts");
    if (!table->d_fire) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_sweeps_compact: the table has no fire table (lrc_table_set_fire)");
    const uint64_t N = table->n;
    if (!(P * N)) return LRC_OK;      // before motion24 is looked at
    if (!motion24 || !out->counts) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_sweeps_compact: motion24 or counts is NULL");
    int rc = check_motion("lrc_scan_sweeps_compact", motion24, P);
    if (rc) return rc;
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    p.dirs3 = table->d_dirs3;
    p.fire = table->d_fire;
    return scan_compact(s, p, kGenSweeps, P, N, max_range, out, capacity, out_total,
                        [&](auto up) { return up(kPoolPoses, motion24, P * 24, &p.motion24); });
}

int lrc_scan_noisy_compact(lrc_scene* s, const double* poses16, uint64_t P, const lrc_table* table, double max_range,
                           const lrc_noise* noise, const lrc_frames* out, uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    if (!s || !out || !table) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_compact: NULL scene, table or output");
    if (table->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_compact: table and scene belong to different contexts");
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_compact: a range_noise option is set (one noise source per call)");
    const uint64_t N = table->n;
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    int rc = noise_params(s->ctx, "lrc_scan_noisy_compact", noise, N, &p.noise);      // checked for an empty call too
    if (rc) return rc;
    if (!(P * N)) return LRC_OK;
    if (!poses16 || !out->counts) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_compact: poses16 or counts is NULL");
    p.dirs3 = table->d_dirs3;
    return scan_compact(s, p, kGenNoisy, P, N, max_range, out, capacity, out_total,
                        [&](auto up) { return up(kPoolPoses, poses16, P * 16, &p.poses16); });
}

int lrc_scan_noisy_sweeps_compact(lrc_scene* s, const double* motion24, uint64_t P, const lrc_table* table, double max_range,
                                  const lrc_noise* noise, const lrc_frames* out, uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    if (!s || !out || !table) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_sweeps_compact: NULL scene, table or output");
    if (table->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_sweeps_compact: table and scene belong to different contexts");
    if (!table->d_fire) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_sweeps_compact: the table has no fire table (lrc_table_set_fire)");
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_sweeps_compact: a range_noise option is set (one noise source per call)");
    const uint64_t N = table->n;
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    int rc = noise_params(s->ctx, "lrc_scan_noisy_sweeps_compact", noise, N, &p.noise);      // checked for an empty call too
    if (rc) return rc;
    if (!(P * N)) return LRC_OK;      // before motion24 is looked at
    if (!motion24 || !out->counts) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_noisy_sweeps_compact: motion24 or counts is NULL");
    if ((rc = check_motion("lrc_scan_noisy_sweeps_compact", motion24, P))) return rc;
    p.dirs3 = table->d_dirs3;
    p.fire = table->d_fire;
    return scan_compact(s, p, kGenNoisySweeps, P, N, max_range, out, capacity, out_total,
                        [&](auto up) { return up(kPoolPoses, motion24, P * 24, &p.motion24); });
}

// Host, no GPU: what trace_kernel<kGenNoisySweeps> casts and uses, from the very gen_ray_noisy_sweep, sweep_centre and normal_of it runs.
int lrc_noisy_sweep_rays(const lrc_noise* noise, const double* motion24, uint64_t P, const double* dirs3, const double* fire,
                         uint64_t N, float* rays6, double* centres3, float* range_term, uint8_t* keep) {
    lrcnoise::Params np{};
    int rc = noise_params_host("lrc_noisy_sweep_rays", noise, N, &np);
    if (rc) return rc;
    if (!(P * N)) return LRC_OK;
    if (!motion24 || !dirs3 || !fire) return fail(LRC_ERR_INVALID_ARG, "lrc_noisy_sweep_rays: motion24, dirs3 or fire is NULL");
    if ((rc = check_motion("lrc_noisy_sweep_rays", motion24, P))) return rc;
    for (uint64_t i = 0; i < N; ++i)
        if (!(fire[i] >= 0.0 && fire[i] < 1.0))     // NaN fails both
            return fail(LRC_ERR_INVALID_ARG, "lrc_noisy_sweep_rays: fire[" + std::to_string(i) + "] is outside [0, 1)");
    const float nan32 = lrcnoise::bits_float(0x7FC00000u);
    for (uint64_t k = 0; k < P; ++k)
        for (uint64_t i = 0; i < N; ++i) {
            const uint64_t r = k * N + i;
            V3 o, d;
            bool live = true;
            gen_ray_noisy_sweep(motion24, dirs3, fire, np, k, i, o, d, live);
            if (rays6) {
                float* q = rays6 + r * 6;
                q[0] = o.x; q[1] = o.y; q[2] = o.z;
                q[3] = live ? d.x : nan32; q[4] = live ? d.y : nan32; q[5] = live ? d.z : nan32;      // a dropped ray has no direction
            }
            if (centres3) sweep_centre(motion24 + k * 24, fire[i], centres3[r * 3], centres3[r * 3 + 1], centres3[r * 3 + 2]);
            if (range_term)      // noisy_range's term: t' = t + range_term
                range_term[r] = np.range_std != 0.0f
                                    ? np.range_std * lrcnoise::normal_of(lrcnoise::ray_words(np.seed, np.first_frame + k, (uint32_t)i).w0, np.tab)
                                    : 0.0f;
            if (keep) keep[r] = (uint8_t)live;
        }
    return LRC_OK;
}

int lrc_scan_poses_compact(lrc_scene* s, const double* poses16, uint64_t P, const double* dirs3, uint64_t N,
                           double max_range, const lrc_frames* out, uint64_t capacity, uint64_t* out_total) {
    return scan_compact_impl(s, poses16, P, dirs3, N, nullptr, max_range, out, capacity, out_total);
}

int lrc_scan_grid_compact(lrc_scene* s, const double* poses16, uint64_t P, const double* dirs3, const lrc_grid* grid,
                          double max_range, const lrc_frames* out, uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    if (!grid) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_grid_compact: grid is NULL");
    const uint64_t N = (uint64_t)grid->lines * grid->width;
    int rc = check_grid("lrc_scan_grid_compact", grid, N);
    if (rc) return rc;
    return scan_compact_impl(s, poses16, P, dirs3, N, grid, max_range, out, capacity, out_total);
}

int lrc_scan_angles_compact(lrc_scene* s, const double* poses16, uint64_t P, const double* angles2,
                            const uint8_t* keep, uint64_t N, double max_range, const lrc_frames* out,
                            uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    if (!s || !out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_angles_compact: NULL scene or output");
    const uint64_t n = P * N;
    if (!n) return LRC_OK;
    if (!poses16 || !angles2 || !out->counts)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_angles_compact: poses16, angles2 or counts is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    return scan_compact(s, p, kGenAngles, P, N, max_range, out, capacity, out_total, [&](auto up) {
        int rc;
        if ((rc = up(kPoolPoses, poses16, P * 16, &p.poses16)) || (rc = up(kPoolAngles, angles2, n * 2, &p.angles2))) return rc;
        return keep ? up(kPoolKeep, keep, n, &p.keep_mask) : LRC_OK;
    });
}

int lrc_scan_rays_compact(lrc_scene* s, const float* rays6, const uint8_t* keep, const double* centers3, uint64_t P,
                          uint64_t N, double max_range, const lrc_frames* out, uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    if (!s || !out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_rays_compact: NULL scene or output");
    const uint64_t n = P * N;
    if (!n) return LRC_OK;
    if (!rays6 || !centers3 || !out->counts)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_rays_compact: rays6, centers3 or counts is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    return scan_compact(s, p, kGenRays, P, N, max_range, out, capacity, out_total, [&](auto up) {
        int rc;
        if ((rc = up(kPoolRays, rays6, n * 6, &p.rays6)) || (rc = up(kPoolCen, centers3, P * 3, &p.seg_centers3))) return rc;
        return keep ? up(kPoolKeep, keep, n, &p.keep_mask) : LRC_OK;
    });
}

int lrc_debug_scan_stats(lrc_scene* s, const double* poses16, uint64_t P, const double* dirs3, uint64_t N,
                         double max_range, uint32_t* stats) {
    if (!s || !stats) return fail(LRC_ERR_INVALID_ARG, "lrc_debug_scan_stats: NULL scene or output");
    const uint64_t n = P * N;
    if (!n) return LRC_OK;
    if (!poses16 || !dirs3) return fail(LRC_ERR_INVALID_ARG, "lrc_debug_scan_stats: poses16 or dirs3 is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    TraceParams p{};
    DevBuf ds;
    int rc;
    if ((rc = stage_input(s->ctx, kPoolPoses, poses16, P * 16, &p.poses16)) ||
        (rc = stage_input(s->ctx, kPoolDirs, dirs3, N * 3, &p.dirs3)) || (rc = ds.get(s->ctx, kPoolStats, n * kStatsWords * 4)))
        return rc;
    scan_fields(p, N, n, max_range, nullptr);
    p.stats = (uint32_t*)ds.p;
    // LRC_STATS_LINE_WIDTH=W: the waves grouped as the scan pipeline groups them for lines of W rays (tools/trav_stats.py);
    // the counters stay indexed by ray
    // LRC_STATS_TILE_LINES=4 with LRC_STATS_LINE_SPLIT=s: groups of four lines on either side of line s
    p.line_tiles = kTBlock == 64 ? line_tiles_for((uint64_t)env_int("LRC_STATS_LINE_WIDTH", 0), N) : 0u;
    p.line_group = line_group_for((uint32_t)env_int("LRC_STATS_LINE_SPLIT", 0), (uint32_t)env_int("LRC_STATS_TILE_LINES", 2));
    if ((rc = launch_trace(s, p, kGenPoses, nullptr, true))) return rc;
    LRC_HIP(hipDeviceSynchronize());
    LRC_HIP(hipMemcpy(stats, ds.p, n * kStatsWords * 4, hipMemcpyDeviceToHost));
    return LRC_OK;
}

}  // extern "C"
