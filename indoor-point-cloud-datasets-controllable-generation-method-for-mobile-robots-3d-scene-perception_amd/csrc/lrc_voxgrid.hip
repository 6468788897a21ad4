// lrc_voxgrid.hip -- semantic occupancy grids from pose-batched scans: ray-carved free space (gfx950).
//
// Definition (include/lidarcast.h, DESIGN.md section 5f, tests/voxgrid_restate.py):
//   Grid    origin g (3 float64), voxel size s (float64 > 0), dims (nx, ny, nz), nx*ny*nz <= 2^31 - 1.  The voxel of a
//           float64 point x is i_a = floor((x_a - g_a) / s) (an f64 subtract, then an f64 divide, then floor); it is
//           inside iff 0 <= i < n on every axis; linear index (i*ny + j)*nz + k (C order, z fastest).
//   Rays    ray (p, i), entry p*N + i: origin o = float32 as gen_ray forms it, end point e = hit_point(o, d, t), the
//           float32 row of the scene cloud.  A ray contributes only if its t is finite (it returns).
//   Walk    float64, no contraction, o and e widened exactly: a = voxel(o), b = voxel(e), D = e - o.  Per axis with
//           b_a != a_a: n_a = |b_a - a_a|, step_a = sign(b_a - a_a), tMax_a = ((g_a + (a_a + 1)*s) - o_a) / D_a stepping
//           up, ((g_a + a_a*s) - o_a) / D_a stepping down, tDelta_a = s / |D_a|; axes with n_a = 0 take no part.  Visit a;
//           while any n_a > 0: take the axis with the smallest tMax among those with n_a > 0 (ties x, then y, then z),
//           step it, tMax_a += tDelta_a, n_a -= 1, visit the new voxel.  The walk ends in b (Manhattan + 1 voxels).
//           Every visited in-grid voxel except b gets its FREE bit; b, if in the grid, gets one RETURN with the ray's
//           (sem, ins).  a == b carves nothing.
//   Limits  a returned ray whose o or e is not finite, whose voxel coordinates leave [-2^31, 2^31), or whose walk is
//           2^24 or more steps long is REJECTED: it carves nothing, records no return and is counted.
//   Finalize  returns[v] = returns in v; occupied iff returns >= min_returns, else free iff the free bit is set, else
//           unknown.  sem[v] = most frequent sem among v's returns (ties to the smallest), ins[v] = most frequent ins
//           among the returns with that sem (ties to the smallest).
//
// Kernels
//   walk       one thread per ray.  The walk is exact as defined; it stops early once it has left the grid on an axis in
//              that axis' direction of travel (no later voxel, b included, can be inside again) and skips rays that
//              never enter.  Free bits: the voxels of one bitset word are gathered per ray, then a plain load first and
//              an atomicOr only when a bit is still clear -- all rays of a pose start in the sensor's voxel, and after
//              the first wave those words are set.  Returns: one 64-bit
//              key (idx << 32) | (sem << 16) | ins per returned ray, appended with one atomic per wave.
//   finalize   rocprim radix sort of the keys (unused reserved slots hold all-ones keys that sort last), run-length
//              encoding of equal keys, a head flag per voxel and an exclusive scan for its slot, then one thread per
//              voxel votes over its few (sem, ins) runs.  Dense state from the bitset plus the sparse list.  Integer
//              work only after the walk.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <new>
#include <string>

#include "lrc_internal.h"
#include "lrc_device.h"

namespace {

using namespace lrcdev;

constexpr int64_t kMaxWalk = 1ll << 24;                      // steps per ray (the Manhattan distance) refused
constexpr uint64_t kMaxKeys = 0x7FFFFFFFull;                // reserved key slots between resets
constexpr double kCoordLimit = 2147483648.0;                // voxel coordinates in [-2^31, 2^31)

struct GridDesc {
    double gx, gy, gz, s;
    int32_t nx, ny, nz;
    uint32_t V;
};

// accumulator words (uint64): [0] keys appended, [1] rejected rays, [2] key slots overflowed (never expected),
// finalize: [3] free bits, [4] occupied voxels, [5] occupied voxels whose free bit is set
enum { kAccKeys = 0, kAccRejected = 1, kAccOverflow = 2, kAccFree = 3, kAccOcc = 4, kAccOverlap = 5, kAccWords = 8 };

// ---- walk -------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

__device__ inline bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// voxel coordinate of one axis; false when it leaves [-2^31, 2^31) (o, e finite, g finite, s > 0: no NaN here)
__device__ inline bool vox_coord(double x, double g, double s, int32_t& out) {
    const double f = __builtin_floor((x - g) / s);
    if (!(f >= -kCoordLimit && f < kCoordLimit)) return false;
    out = (int32_t)f;                                      // exact: an integer in int32's range
    return true;
}

// the rest of the walk is outside the grid on this axis: c is past the grid in the direction of travel (or the axis
// does not move and c is outside)
__device__ inline bool gone(int32_t c, int32_t step, int32_t n) { return (step >= 0 && c >= n) || (step <= 0 && c < 0); }

// Free bits of one ray: consecutive voxels in one bitset word (steps along z, the fastest axis) are gathered into one
// mask; a word is written when the walk leaves it, with a plain load first and an atomicOr only when a bit is still clear.
// (An L1-bypassing check load measured 2x slower: the plain load's stale answer costs at most an idempotent atomic.)
struct FreeSink {
    uint32_t w = 0xFFFFFFFFu, m = 0;
    __device__ void flush(uint32_t* __restrict__ bits) {
        if (m && (bits[w] & m) != m) atomicOr(&bits[w], m);
    }
    __device__ void add(uint32_t* __restrict__ bits, uint32_t idx) {
        const uint32_t nw = idx >> 5;
        if (nw != w) {
            flush(bits);
            w = nw;
            m = 0;
        }
        m |= 1u << (idx & 31u);
    }
};

__global__ __launch_bounds__(kBlock) void walk_kernel(const double* __restrict__ poses16, const double* __restrict__ dirs3,
                                                      const uint2* __restrict__ tl, uint64_t N, uint64_t total, GridDesc g,
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
            int32_t a0, a1, a2, b0, b1, b2;
            rejected = !(finite_f(o.x) && finite_f(o.y) && finite_f(o.z) && finite_f(e.x) && finite_f(e.y) && finite_f(e.z));
            if (!rejected)
                rejected = !(vox_coord(o.x, g.gx, g.s, a0) && vox_coord(o.y, g.gy, g.s, a1) && vox_coord(o.z, g.gz, g.s, a2) &&
                             vox_coord(e.x, g.gx, g.s, b0) && vox_coord(e.y, g.gy, g.s, b1) && vox_coord(e.z, g.gz, g.s, b2));
            if (!rejected) {
                const int64_t d0 = (int64_t)b0 - a0, d1 = (int64_t)b1 - a1, d2 = (int64_t)b2 - a2;
                int32_t n0 = 0, n1 = 0, n2 = 0;
                const int64_t m0 = d0 < 0 ? -d0 : d0, m1 = d1 < 0 ? -d1 : d1, m2 = d2 < 0 ? -d2 : d2;
                rejected = m0 + m1 + m2 >= kMaxWalk;
                if (!rejected) {
                    n0 = (int32_t)m0; n1 = (int32_t)m1; n2 = (int32_t)m2;
                    const int32_t s0 = d0 > 0 ? 1 : (d0 < 0 ? -1 : 0);
                    const int32_t s1 = d1 > 0 ? 1 : (d1 < 0 ? -1 : 0);
                    const int32_t s2 = d2 > 0 ? 1 : (d2 < 0 ? -1 : 0);
                    int32_t c0 = a0, c1 = a1, c2 = a2;
                    bool inside = !(gone(c0, s0, g.nx) || gone(c1, s1, g.ny) || gone(c2, s2, g.nz));
                    if (inside) {
                        const double ox = o.x, oy = o.y, oz = o.z;
                        const double D0 = (double)e.x - ox, D1 = (double)e.y - oy, D2 = (double)e.z - oz;
                        double t0 = 0.0, t1 = 0.0, t2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
                        if (s0) {
                            t0 = ((g.gx + ((double)a0 + (s0 > 0 ? 1.0 : 0.0)) * g.s) - ox) / D0;
                            q0 = g.s / __builtin_fabs(D0);
                        }
                        if (s1) {
                            t1 = ((g.gy + ((double)a1 + (s1 > 0 ? 1.0 : 0.0)) * g.s) - oy) / D1;
                            q1 = g.s / __builtin_fabs(D1);
                        }
                        if (s2) {
                            t2 = ((g.gz + ((double)a2 + (s2 > 0 ? 1.0 : 0.0)) * g.s) - oz) / D2;
                            q2 = g.s / __builtin_fabs(D2);
                        }
                        FreeSink sink;
                        while (n0 + n1 + n2 > 0) {
                            if ((uint32_t)c0 < (uint32_t)g.nx && (uint32_t)c1 < (uint32_t)g.ny && (uint32_t)c2 < (uint32_t)g.nz)
                                sink.add(bits, ((uint32_t)c0 * (uint32_t)g.ny + (uint32_t)c1) * (uint32_t)g.nz + (uint32_t)c2);
                            bool out;
                            if (n0 > 0 && (n1 == 0 || t0 <= t1) && (n2 == 0 || t0 <= t2)) {
                                c0 += s0; t0 = t0 + q0; --n0;
                                out = gone(c0, s0, g.nx);
                            } else if (n1 > 0 && (n2 == 0 || t1 <= t2)) {
                                c1 += s1; t1 = t1 + q1; --n1;
                                out = gone(c1, s1, g.ny);
                            } else {
                                c2 += s2; t2 = t2 + q2; --n2;
                                out = gone(c2, s2, g.nz);
                            }
                            if (out) {
                                inside = false;
                                break;
                            }
                        }
                        sink.flush(bits);
                        // the walk ended in b (or left the grid for good: b is outside then)
                        if (inside && (uint32_t)c0 < (uint32_t)g.nx && (uint32_t)c1 < (uint32_t)g.ny &&
                            (uint32_t)c2 < (uint32_t)g.nz) {
                            const uint32_t idx = ((uint32_t)c0 * (uint32_t)g.ny + (uint32_t)c1) * (uint32_t)g.nz + (uint32_t)c2;
                            ret = true;
                            key = ((unsigned long long)idx << 32) | ((unsigned long long)(rec.y & 0xFFFFu) << 16) |
                                  (unsigned long long)(rec.y >> 16);
                        }
                    }
                }
            }
        }
    }
    const uint32_t lane = __lane_id();
    const unsigned long long rm = __ballot(rejected);
    if (rm && lane == (uint32_t)__ffsll((long long)rm) - 1) atomicAdd(&acc[kAccRejected], (unsigned long long)__popcll(rm));
    const unsigned long long m = __ballot(ret);
    if (m) {                                                   // wave-uniform: one atomic per wave for the slots
        const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(&acc[kAccKeys], (unsigned long long)__popcll(m));
        base = __shfl(base, (int)leader);
        if (ret) {
            const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (pos < key_cap) keys[pos] = key;
            else atomicOr(&acc[kAccOverflow], 1ull);
        }
    }
}

// ---- finalize ---------------------------------------------------------------------------------------------------
// head of a voxel's runs among the unique keys
__global__ __launch_bounds__(kBlock) void head_kernel(const unsigned long long* __restrict__ ukeys,
                                                      const uint32_t* __restrict__ nruns, uint64_t R, uint32_t V,
                                                      uint32_t* __restrict__ flag) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j > R) return;
    uint32_t f = 0;
    if (j < *nruns) {
        const uint32_t idx = (uint32_t)(ukeys[j] >> 32);
        f = idx < V && (j == 0 || (uint32_t)(ukeys[j - 1] >> 32) != idx);
    }
    flag[j] = f;
}

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
        const uint64_t nr = *nruns;
        const unsigned long long k0 = ukeys[j];
        const uint32_t idx = (uint32_t)(k0 >> 32);
        uint32_t total = 0, best_cnt = 0, best_sem = 0, best_ins = 0;
        uint64_t k = j;
        while (k < nr && (uint32_t)(ukeys[k] >> 32) == idx) {
            const unsigned long long top = ukeys[k] >> 16;           // (idx, sem)
            uint32_t sem_cnt = 0, ins_cnt = 0, ins = 0;
            while (k < nr && (ukeys[k] >> 16) == top) {
                const uint32_t c = counts[k];
                sem_cnt += c;
                if (c > ins_cnt) { ins_cnt = c; ins = (uint32_t)(ukeys[k] & 0xFFFFull); }   // ascending ins: ties keep the smallest
                ++k;
            }
            total += sem_cnt;
            if (sem_cnt > best_cnt) { best_cnt = sem_cnt; best_sem = (uint32_t)(top & 0xFFFFull); best_ins = ins; }
        }
        const uint32_t o = pos[j];
        o_idx[o] = idx;
        o_sem[o] = (uint16_t)best_sem;
        o_ins[o] = (uint16_t)best_ins;
        o_ret[o] = total;
        occ = total >= min_returns;
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
    GridDesc g{};
    uint64_t V = 0, W = 0;
    uint32_t* d_bits = nullptr;                 // W words
    unsigned long long* d_keys = nullptr;       // key_cap slots; [0, reserved) valid or all-ones
    uint64_t key_cap = 0, reserved = 0;
    unsigned long long* d_acc = nullptr;        // kAccWords
    // finalize scratch, sized for fin_cap keys
    uint64_t fin_cap = 0;
    unsigned long long* d_sorted = nullptr;
    unsigned long long* d_ukeys = nullptr;
    uint32_t* d_counts = nullptr;
    uint32_t* d_flag = nullptr;                 // fin_cap + 1
    uint32_t* d_pos = nullptr;                  // fin_cap + 1
    uint32_t* d_nruns = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
};

namespace {

void release_fin(lrc_voxgrid* v) {
    void* ps[] = {v->d_sorted, v->d_ukeys, v->d_counts, v->d_flag, v->d_pos, v->d_nruns, v->d_tmp};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    v->d_sorted = v->d_ukeys = nullptr;
    v->d_counts = v->d_flag = v->d_pos = v->d_nruns = nullptr;
    v->d_tmp = nullptr;
    v->fin_cap = 0;
    v->tmp_bytes = 0;
}

void release(lrc_voxgrid* v) {
    release_fin(v);
    void* ps[] = {v->d_bits, v->d_keys, v->d_acc};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    v->d_bits = nullptr;
    v->d_keys = nullptr;
    v->d_acc = nullptr;
}

uint32_t key_end_bit(uint64_t V) {                   // V < 2^b: every valid key's idx field is below all ones
    uint32_t b = 0;
    while (b < 32 && (1ull << b) <= V) ++b;
    return 32 + b;
}

int ensure_fin(lrc_voxgrid* v, uint64_t R, hipStream_t st) {
    if (R <= v->fin_cap) return LRC_OK;
    LRC_HIP(hipStreamSynchronize(st));                  // the old scratch may still be read by enqueued work
    release_fin(v);
    const uint64_t cap = R;
    LRC_HIP(hipMalloc((void**)&v->d_sorted, cap * 8));
    LRC_HIP(hipMalloc((void**)&v->d_ukeys, cap * 8));
    LRC_HIP(hipMalloc((void**)&v->d_counts, cap * 4));
    LRC_HIP(hipMalloc((void**)&v->d_flag, (cap + 1) * 4));
    LRC_HIP(hipMalloc((void**)&v->d_pos, (cap + 1) * 4));
    LRC_HIP(hipMalloc((void**)&v->d_nruns, 4));
    size_t a = 0, b = 0, c = 0;
    const uint32_t eb = key_end_bit(v->V);
    LRC_HIP(rocprim::radix_sort_keys(nullptr, a, (const unsigned long long*)v->d_keys, v->d_sorted, (size_t)cap, 0, eb, st));
    LRC_HIP(rocprim::run_length_encode(nullptr, b, (const unsigned long long*)v->d_sorted, (unsigned int)cap, v->d_ukeys,
                                     v->d_counts, v->d_nruns, st));
    LRC_HIP(rocprim::exclusive_scan(nullptr, c, (const uint32_t*)v->d_flag, v->d_pos, 0u, (size_t)(cap + 1),
                                  rocprim::plus<uint32_t>(), st));
    v->tmp_bytes = a > b ? a : b;
    if (c > v->tmp_bytes) v->tmp_bytes = c;
    LRC_HIP(hipMalloc(&v->d_tmp, v->tmp_bytes ? v->tmp_bytes : 1));
    v->fin_cap = cap;
    return LRC_OK;
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
    v->V = V;
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
    if (need > vg->key_cap) {                            // grow: no return is ever dropped
        uint64_t cap = vg->key_cap * 2;
        if (cap < need) cap = need;
        if (cap > kMaxKeys) cap = kMaxKeys;
        unsigned long long* nk = nullptr;
        LRC_HIP(hipMalloc((void**)&nk, cap * 8));
        if (vg->reserved) {
            hipError_t e = hipMemcpyAsync(nk, vg->d_keys, vg->reserved * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                (void)hipFree(nk);
                LRC_HIP(e);
            }
        }
        if (vg->d_keys) LRC_HIP(hipFree(vg->d_keys));
        vg->d_keys = nk;
        vg->key_cap = cap;
    }
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
        int rc = ensure_fin(vg, R, st);
        if (rc != LRC_OK) return rc;
        size_t tb = vg->tmp_bytes;
        LRC_HIP(rocprim::radix_sort_keys(vg->d_tmp, tb, (const unsigned long long*)vg->d_keys, vg->d_sorted, (size_t)R, 0,
                                       key_end_bit(vg->V), st));
        tb = vg->tmp_bytes;
        LRC_HIP(rocprim::run_length_encode(vg->d_tmp, tb, (const unsigned long long*)vg->d_sorted, (unsigned int)R,
                                         vg->d_ukeys, vg->d_counts, vg->d_nruns, st));
        hipLaunchKernelGGL(head_kernel, dim3((uint32_t)blocks_of(R + 1, kBlock)), dim3(kBlock), 0, st,
                           (const unsigned long long*)vg->d_ukeys, (const uint32_t*)vg->d_nruns, R, vg->g.V, vg->d_flag);
        LRC_HIP(hipGetLastError());
        tb = vg->tmp_bytes;
        LRC_HIP(rocprim::exclusive_scan(vg->d_tmp, tb, (const uint32_t*)vg->d_flag, vg->d_pos, 0u, (size_t)(R + 1),
                                      rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL(vote_kernel, dim3((uint32_t)blocks_of(R, kBlock)), dim3(kBlock), 0, st,
                           (const unsigned long long*)vg->d_ukeys, (const uint32_t*)vg->d_counts,
                           (const uint32_t*)vg->d_nruns, (const uint32_t*)vg->d_flag, (const uint32_t*)vg->d_pos, R,
                           min_returns, (const uint32_t*)vg->d_bits, d_idx, d_sem, d_ins, d_returns, d_state, vg->d_acc);
    }
    hipLaunchKernelGGL(popcount_kernel, dim3((uint32_t)blocks_of(vg->W, kBlock)), dim3(kBlock), 0, st,
                       (const uint32_t*)vg->d_bits, vg->W, vg->g.V, vg->d_acc);
    hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)vg->d_pos, R, vg->V,
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
