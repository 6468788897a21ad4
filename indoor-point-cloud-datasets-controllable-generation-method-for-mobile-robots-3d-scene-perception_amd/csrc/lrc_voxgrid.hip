// lrc_voxgrid.hip -- semantic occupancy grids from pose-batched scans: ray-carved free space (gfx950).
//
// Definition (include/lidarcast.h, DESIGN.md section 5f, tests/voxgrid_restate.py): the grid, the walk and its limits are
// lrc_voxwalk.h's, the keys, their runs and the sem / ins vote lrc_voxruns.h's.  This unit's own:
//   Rays    ray (p, i), entry p*N + i: origin o = float32 as gen_ray forms it, end point e = hit_point(o, d, t), the
//           float32 row of the scene cloud.  A ray contributes only if its t is finite (it returns).  Its end voxel b, if
//           in the grid, gets one RETURN with the ray's (sem, ins); a rejected ray records none and is counted.
//   Finalize  returns[v] = returns in v; occupied iff returns >= min_returns, else free iff the free bit is set, else
//           unknown.
//
// Kernels
//   walk       one thread per ray: walk_segment into a FreeSink on the grid's bitset, then one 64-bit key
//              (idx << 32) | (sem << 16) | ins per returned ray, appended with one atomic per wave.
//   finalize   the runs of the keys (KeyRuns), then one thread per voxel votes over its few (sem, ins) runs.  Dense state
//              from the bitset plus the sparse list.  Integer work only after the walk.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "lrc_internal.h"
#include "lrc_device.h"
#include "lrc_voxwalk.h"
#include "lrc_voxruns.h"

namespace {

using namespace lrcdev;
using namespace lrcwalk;

// accumulator words (uint64): [0] keys appended, [1] rejected rays, [2] key slots overflowed (never expected),
// finalize: [3] free bits, [4] occupied voxels, [5] occupied voxels whose free bit is set
enum { kAccKeys = 0, kAccRejected = 1, kAccOverflow = 2, kAccFree = 3, kAccOcc = 4, kAccOverlap = 5, kAccWords = 8 };

// ---- walk -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void walk_kernel(const double* __restrict__ poses16, const double* __restrict__ dirs3,
                                                      const uint2* __restrict__ tl, uint64_t N, uint64_t total, Grid g,
                                                      uint32_t* __restrict__ bits, unsigned long long* __restrict__ keys,
                                                      uint64_t key_cap, unsigned long long* __restrict__ acc) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool ret = false, rejected = false;
    unsigned long long key = 0;
    if (gid < total) {
        const uint2 rec = tl[gid];
        const float t = __uint_as_float(rec.x);
        if (finite_f(t)) {
            const uint64_t p = gid / N, i = gid - p * N;
            V3 o, d, h, e;
            double cx, cy, cz;
            gen_ray(poses16, dirs3, p, i, o, d, cx, cy, cz);
            hit_point(o, d, t, h, e);
            FreeSink sink{bits};
            uint32_t end = 0;
            int32_t b3[3];
            const int rc = walk_segment(g, o.x, o.y, o.z, e.x, e.y, e.z, sink, end, b3);
            rejected = rc == kWalkRejected;
            if (rc == kWalkEnd) {
                ret = true;
                key = ((unsigned long long)end << 32) | ((unsigned long long)(rec.y & 0xFFFFu) << 16) |
                      (unsigned long long)(rec.y >> 16);
            }
        }
    }
    const unsigned long long rm = __ballot(rejected);
    if (rm && __lane_id() == (uint32_t)__ffsll((long long)rm) - 1)
        atomicAdd(&acc[kAccRejected], (unsigned long long)__popcll(rm));
    const unsigned long long pos = wave_append(ret, &acc[kAccKeys], &acc[kAccOverflow], key_cap);
    if (pos != kNoSlot) keys[pos] = key;
}

// ---- finalize ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void dense_kernel(const uint32_t* __restrict__ bits, uint32_t V,
                                                       uint8_t* __restrict__ state) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v < V) state[v] = (uint8_t)((bits[v >> 5] >> (v & 31u)) & 1u);
}

// one thread per voxel head: count its returns and vote sem, then ins within the winning sem
__global__ __launch_bounds__(kBlock) void vote_kernel(const unsigned long long* __restrict__ ukeys,
                                                      const uint32_t* __restrict__ counts, const uint32_t* __restrict__ nruns,
                                                      const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                      uint64_t R, uint32_t min_returns, const uint32_t* __restrict__ bits,
                                                      uint32_t* __restrict__ o_idx, uint16_t* __restrict__ o_sem,
                                                      uint16_t* __restrict__ o_ins, uint32_t* __restrict__ o_ret,
                                                      uint8_t* __restrict__ state, unsigned long long* __restrict__ acc) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool occ = false, overlap = false;
    if (j < R && flag[j]) {
        const LabelVote v = label_vote(ukeys, counts, *nruns, j);
        const uint32_t idx = (uint32_t)(ukeys[j] >> 32), o = pos[j];
        o_idx[o] = idx;
        o_sem[o] = (uint16_t)v.sem;
        o_ins[o] = (uint16_t)v.ins;
        o_ret[o] = v.total;
        occ = v.total >= min_returns;
        if (occ) {
            overlap = (bits[idx >> 5] >> (idx & 31u)) & 1u;
            if (state) state[idx] = 2;
        }
    }
    const unsigned long long om = __ballot(occ), vm = __ballot(overlap);
    if (__lane_id() == 0) {
        if (om) atomicAdd(&acc[kAccOcc], (unsigned long long)__popcll(om));
        if (vm) atomicAdd(&acc[kAccOverlap], (unsigned long long)__popcll(vm));
    }
}

__global__ __launch_bounds__(kBlock) void popcount_kernel(const uint32_t* __restrict__ bits, uint64_t W, uint32_t V,
                                                          unsigned long long* __restrict__ acc) {
    __shared__ uint32_t s_part[kBlock / 64];
    const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t c = 0;
    if (w < W) {
        uint32_t x = bits[w];
        const uint64_t lo = w * 32;
        if ((uint64_t)V - lo < 32) x &= (1u << (uint32_t)((uint64_t)V - lo)) - 1u;
        c = (uint32_t)__popc(x);
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if (__lane_id() == 0) s_part[threadIdx.x / 64] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t n = 0;
        for (int i = 0; i < kBlock / 64; ++i) n += s_part[i];
        if (n) atomicAdd(&acc[kAccFree], (unsigned long long)n);
    }
}

// counts: [0] sparse entries, [1] free, [2] occupied, [3] unknown, [4] rejected rays, [5] returns recorded
__global__ void counts_kernel(const uint32_t* __restrict__ pos, uint64_t R, uint64_t V,
                              const unsigned long long* __restrict__ acc, uint64_t* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const uint64_t occ = acc[kAccOcc], fr = acc[kAccFree] - acc[kAccOverlap];
    out[0] = R ? pos[R] : 0;
    out[1] = fr;
    out[2] = occ;
    out[3] = V - fr - occ;
    out[4] = acc[kAccRejected];
    out[5] = acc[kAccKeys];
}

}  // namespace

struct lrc_voxgrid {
    int device = 0;
    Grid g{};
    uint64_t V = 0, W = 0;
    uint32_t* d_bits = nullptr;                 // W words
    unsigned long long* d_keys = nullptr;       // key_cap slots; [0, reserved) valid or all-ones
    uint64_t key_cap = 0, reserved = 0;
    unsigned long long* d_acc = nullptr;        // kAccWords
    KeyRuns runs;                               // finalize scratch; runs.G = V
};

namespace {

void release(lrc_voxgrid* v) {
    v->runs.release();
    void* ps[] = {v->d_bits, v->d_keys, v->d_acc};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    v->d_bits = nullptr;
    v->d_keys = nullptr;
    v->d_acc = nullptr;
}

}  // namespace

extern "C" {

int lrc_voxgrid_destroy(lrc_voxgrid* vg) {
    if (!vg) return LRC_OK;
    (void)hipSetDevice(vg->device);
    release(vg);
    delete vg;
    return LRC_OK;
}

int lrc_voxgrid_create(lrc_ctx* ctx, const double* origin3, double voxel_size, const int64_t* dims3,
                       lrc_voxgrid** out_vg) {
    if (!out_vg) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_create: out_vg is NULL");
    *out_vg = nullptr;
    if (!ctx || !origin3 || !dims3) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_create: NULL argument");
    for (int a = 0; a < 3; ++a)
        if (!__builtin_isfinite(origin3[a]))
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_create: origin must be finite");
    if (!__builtin_isfinite(voxel_size) || !(voxel_size > 0.0))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_create: voxel_size must be finite and > 0");
    uint64_t V = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims3[a] < 1 || dims3[a] > 0x7FFFFFFFll)
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_create: every dim must be >= 1");
        V *= (uint64_t)dims3[a];
        if (V > 0x7FFFFFFFull)
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_create: nx*ny*nz must not exceed 2^31 - 1");
    }
    lrc_voxgrid* v = new (std::nothrow) lrc_voxgrid();
    if (!v) return lrc_internal_fail(LRC_ERR_OOM, "lrc_voxgrid_create: out of host memory");
    v->device = ctx->device;
    v->g.gx = origin3[0];
    v->g.gy = origin3[1];
    v->g.gz = origin3[2];
    v->g.s = voxel_size;
    v->g.nx = (int32_t)dims3[0];
    v->g.ny = (int32_t)dims3[1];
    v->g.nz = (int32_t)dims3[2];
    v->g.V = (uint32_t)V;
    v->V = v->runs.G = V;
    v->W = (V + 31) / 32;
    auto run = [&]() -> int {
        LRC_HIP(hipSetDevice(v->device));
        LRC_HIP(hipMalloc((void**)&v->d_bits, v->W * 4));
        LRC_HIP(hipMalloc((void**)&v->d_acc, kAccWords * 8));
        LRC_HIP(hipMemset(v->d_bits, 0, v->W * 4));
        LRC_HIP(hipMemset(v->d_acc, 0, kAccWords * 8));
        return LRC_OK;
    };
    const int rc = run();
    if (rc != LRC_OK) {
        lrc_voxgrid_destroy(v);
        return rc;
    }
    *out_vg = v;
    return LRC_OK;
}

int lrc_voxgrid_get_info(const lrc_voxgrid* vg, lrc_voxgrid_info* out) {
    if (!vg || !out) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_get_info: NULL argument");
    out->origin[0] = vg->g.gx;
    out->origin[1] = vg->g.gy;
    out->origin[2] = vg->g.gz;
    out->voxel_size = vg->g.s;
    out->dims[0] = vg->g.nx;
    out->dims[1] = vg->g.ny;
    out->dims[2] = vg->g.nz;
    out->num_voxels = vg->V;
    out->words = vg->W;
    out->reserved_keys = vg->reserved;
    out->sparse_bound = vg->reserved < vg->V ? vg->reserved : vg->V;
    return LRC_OK;
}

int lrc_voxgrid_reset(lrc_voxgrid* vg, void* stream) {
    if (!vg) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_reset: NULL argument");
    const hipStream_t st = (hipStream_t)stream;
    LRC_HIP(hipSetDevice(vg->device));
    LRC_HIP(hipMemsetAsync(vg->d_bits, 0, vg->W * 4, st));
    LRC_HIP(hipMemsetAsync(vg->d_acc, 0, kAccWords * 8, st));
    vg->reserved = 0;
    return LRC_OK;
}

int lrc_voxgrid_accumulate_dev(lrc_voxgrid* vg, const double* d_poses16, uint64_t num_poses, const double* d_dirs3,
                               uint64_t rays_per_pose, const void* d_t_label, void* stream) {
    if (!vg) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_accumulate_dev: NULL argument");
    if (num_poses == 0 || rays_per_pose == 0) return LRC_OK;
    if (!d_poses16 || !d_dirs3 || !d_t_label)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_accumulate_dev: NULL argument");
    if (num_poses > kMaxKeys || rays_per_pose > kMaxKeys || num_poses * rays_per_pose > kMaxKeys - vg->reserved)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG,
                                 "lrc_voxgrid_accumulate_dev: more than 2^31 - 1 rays between resets");
    const uint64_t total = num_poses * rays_per_pose;
    const hipStream_t st = (hipStream_t)stream;
    LRC_HIP(hipSetDevice(vg->device));
    const uint64_t need = vg->reserved + total;
    const int rc = grow_key_columns(&vg->d_keys, nullptr, &vg->key_cap, vg->reserved, need, st);      // no return is ever dropped
    if (rc != LRC_OK) return rc;
    LRC_HIP(hipMemsetAsync(vg->d_keys + vg->reserved, 0xFF, total * 8, st));   // unfilled slots sort last
    vg->reserved = need;
    hipLaunchKernelGGL(walk_kernel, dim3((uint32_t)blocks_of(total, kBlock)), dim3(kBlock), 0, st, d_poses16, d_dirs3,
                       (const uint2*)d_t_label, rays_per_pose, total, vg->g, vg->d_bits, vg->d_keys, vg->reserved,
                       vg->d_acc);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_voxgrid_finalize_dev(lrc_voxgrid* vg, uint32_t min_returns, uint32_t* d_idx, uint16_t* d_sem, uint16_t* d_ins,
                             uint32_t* d_returns, uint64_t capacity, uint8_t* d_state, uint64_t* d_counts6, void* stream) {
    if (!vg || !d_counts6) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_finalize_dev: NULL argument");
    if (min_returns < 1) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_finalize_dev: min_returns must be >= 1");
    const uint64_t R = vg->reserved;
    const uint64_t bound = R < vg->V ? R : vg->V;
    if (bound && (!d_idx || !d_sem || !d_ins || !d_returns))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_finalize_dev: NULL sparse output");
    if (capacity < bound)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_finalize_dev: capacity below sparse_bound");
    const hipStream_t st = (hipStream_t)stream;
    LRC_HIP(hipSetDevice(vg->device));
    LRC_HIP(hipMemsetAsync(vg->d_acc + kAccFree, 0, 3 * 8, st));
    if (d_state)
        hipLaunchKernelGGL(dense_kernel, dim3((uint32_t)blocks_of(vg->V, kBlock)), dim3(kBlock), 0, st,
                           (const uint32_t*)vg->d_bits, vg->g.V, d_state);
    if (R) {
        const KeyColumn col{vg->d_keys, 32};
        int rc = vg->runs.ensure(R, {col}, st);
        if (rc == LRC_OK) rc = vg->runs.runs_of(col, R, st);
        if (rc != LRC_OK) return rc;
        const KeyRuns& r = vg->runs;
        hipLaunchKernelGGL(vote_kernel, dim3((uint32_t)blocks_of(R, kBlock)), dim3(kBlock), 0, st,
                           (const unsigned long long*)r.d_ukeys, (const uint32_t*)r.d_counts,
                           (const uint32_t*)r.d_nruns, (const uint32_t*)r.d_flag, (const uint32_t*)r.d_pos, R,
                           min_returns, (const uint32_t*)vg->d_bits, d_idx, d_sem, d_ins, d_returns, d_state, vg->d_acc);
    }
    hipLaunchKernelGGL(popcount_kernel, dim3((uint32_t)blocks_of(vg->W, kBlock)), dim3(kBlock), 0, st,
                       (const uint32_t*)vg->d_bits, vg->W, vg->g.V, vg->d_acc);
    hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)vg->runs.d_pos, R, vg->V,
                       (const unsigned long long*)vg->d_acc, d_counts6);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_voxgrid_finalize(lrc_voxgrid* vg, uint32_t min_returns, uint32_t* out_idx, uint16_t* out_sem, uint16_t* out_ins,
                         uint32_t* out_returns, uint64_t capacity, uint8_t* out_state, lrc_voxgrid_counts* out_counts) {
    if (!vg || !out_counts) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_finalize: NULL argument");
    const uint64_t R = vg->reserved, bound = R < vg->V ? R : vg->V;
    if (bound && (!out_idx || !out_sem || !out_ins || !out_returns))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_finalize: NULL sparse output");
    if (capacity < bound)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_finalize: capacity below sparse_bound");
    LRC_HIP(hipSetDevice(vg->device));
    LRC_HIP(hipDeviceSynchronize());                      // work the caller enqueued on other streams
    void* buf = nullptr;
    const uint64_t n = bound ? bound : 1;
    const size_t bytes = 6 * 8 + n * 12 + (out_state ? vg->V : 0);
    LRC_HIP(hipMalloc(&buf, bytes));
    struct Free {
        void* p;
        ~Free() { (void)hipFree(p); }
    } guard{buf};
    uint64_t* dc = (uint64_t*)buf;
    uint32_t* di = (uint32_t*)(dc + 6);
    uint32_t* dr = di + n;
    uint16_t* ds = (uint16_t*)(dr + n);
    uint16_t* dn = ds + n;
    uint8_t* dst = out_state ? (uint8_t*)(dn + n) : nullptr;
    int rc = lrc_voxgrid_finalize_dev(vg, min_returns, di, ds, dn, dr, n, dst, dc, nullptr);
    if (rc != LRC_OK) return rc;
    uint64_t c[6];
    LRC_HIP(hipMemcpy(c, dc, sizeof(c), hipMemcpyDeviceToHost));     // the one synchronisation
    out_counts->num_sparse = c[0];
    out_counts->num_free = c[1];
    out_counts->num_occupied = c[2];
    out_counts->num_unknown = c[3];
    out_counts->rejected_rays = c[4];
    out_counts->returns = c[5];
    if (c[0]) {
        LRC_HIP(hipMemcpy(out_idx, di, c[0] * 4, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out_sem, ds, c[0] * 2, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out_ins, dn, c[0] * 2, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out_returns, dr, c[0] * 4, hipMemcpyDeviceToHost));
    }
    if (out_state) LRC_HIP(hipMemcpy(out_state, dst, vg->V, hipMemcpyDeviceToHost));
    return LRC_OK;
}

int lrc_voxgrid_export_bits(lrc_voxgrid* vg, uint32_t* out_bits) {
    if (!vg || !out_bits) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxgrid_export_bits: NULL argument");
    LRC_HIP(hipSetDevice(vg->device));
    LRC_HIP(hipDeviceSynchronize());
    LRC_HIP(hipMemcpy(out_bits, vg->d_bits, vg->W * 4, hipMemcpyDeviceToHost));
    return LRC_OK;
}

}  // extern "C"
