// lrc_frameobj.hip -- per-frame object annotations of scans: returns, visible area and visible box of every object in
// every frame, in the sensor's frame (gfx950).
//
// Definitions (include/lidarcast.h).  Object k is the k-th distinct label word key = sem | ins << 16
// among the mesh's triangles, ascending.  A ray RETURNS iff its t is finite and its prim < T (section 5e); a returned ray
// with a non-finite point3 coordinate is ignored and counted in rejected_rays; rows of rays that do not return are never
// loaded.  The sensor-frame coordinate of a returned ray of pose M (row-major 4x4 float64), with x its float32 point3 row
// widened exactly, e = x - M[:3,3]:   s_a = (M[0][a]*e_0 + M[1][a]*e_1) + M[2][a]*e_2   in float64, no contraction.
// Per (frame, object): returns (u32), seen_tris (u32), seen_q (u64, each triangle once per frame, q of lrc_area.h),
// vmin / vmax (f64, IEEE total order on finite values: -0.0 below +0.0; +inf / -inf while returns == 0).
//
// Every accumulator is an integer that is added, OR-ed or min / max-ed: doubles are held as their order-preserving 64-bit
// image (img_of), so the result depends neither on pose order, nor on chunking, nor on the order of atomics.
//
// Kernels
//   static_kernel      q[j] and the per-object table (tri_count, total_q, world AABB) with the reduction below, straight to
//                      global atomics (once, at create).
//   accumulate_kernel  one workgroup per (pose, run of kRaysPerBlock rays): pose and frame are uniform over the workgroup.
//                      N that is no multiple of the tile leaves the last workgroup of each pose partly idle: lanes past N
//                      load nothing and take no part.  Inside a wave, runs of equal prim are merged as in lrc_coverage:
//                      the head lane of a run tests the frame's triangle bit and, if a plain load does not show it, issues
//                      ONE returning atomicOr; the lane whose OR newly set the bit carries q[prim] and one seen triangle
//                      (exactly once across calls).  Then the wave loops over its distinct objects (ballot + shuffle of the
//                      first remaining lane's object): count by popcount, q by a butterfly sum, the six box coordinates by
//                      butterfly min / max.  Lanes 0..8 add the wave's partial to the workgroup's LDS table: kSlots rows,
//                      direct-mapped by object index, claimed with an LDS compare-and-swap on the row's tag.  A partial
//                      whose row is owned by another object goes straight to the global row instead (same commutative
//                      operations: only slower), so more distinct objects than rows cost time, never correctness.
//                      After a barrier one thread per claimed row flushes it with global integer atomics.
//   export_kernel      one thread per (frame, object): counts as they are, boxes decoded from their images.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "lrc_internal.h"
#include "lrc_area.h"

namespace {

typedef unsigned long long u64;

constexpr int kRaysPerThread = 4;
constexpr uint64_t kRaysPerBlock = (uint64_t)kBlock * kRaysPerThread;
constexpr uint32_t kMaxObjects = 4096;
constexpr uint32_t kSlots = 128;             // LDS rows per workgroup (68 B each: 8.5 KB of the 160 KB)
constexpr uint32_t kEmpty = 0xFFFFFFFFu;     // tag of an unclaimed row (object indices are < 4096)
constexpr u64 kImgPosInf = 0xFFF0000000000000ull;   // img_of(+inf): the identity of min
constexpr u64 kImgNegInf = 0x000FFFFFFFFFFFFFull;   // img_of(-inf): the identity of max

// Order-preserving image of a double: unsigned comparison of images is the IEEE total order (-0.0 below +0.0).
__host__ __device__ inline u64 img_of(double x) {
    u64 b;
    __builtin_memcpy(&b, &x, 8);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}

__host__ __device__ inline double dbl_of(u64 i) {
    const u64 b = (i >> 63) ? i ^ (1ull << 63) : ~i;
    double x;
    __builtin_memcpy(&x, &b, 8);
    return x;
}

__device__ inline bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

__device__ inline uint32_t next_boundary(u64 boundary, uint32_t lane) {
    const u64 above = lane == 63 ? 0ull : (boundary >> (lane + 1)) << (lane + 1);
    return above ? (uint32_t)__ffsll((long long)above) - 1 : 64u;
}

struct Part {            // one wave's partial of one object, the same in every lane (scalars: they stay in registers)
    uint32_t cnt, tris;
    u64 q, l0, l1, l2, h0, h1, h2;
};

__device__ inline u64 min_u64(u64 a, u64 b) { return b < a ? b : a; }
__device__ inline u64 max_u64(u64 a, u64 b) { return b > a ? b : a; }

// Loop over the distinct objects of the wave's ok lanes; commit(k, part) runs wave-uniformly once per object.
// Returns true in every lane if a q sum wrapped.
template <class Commit>
__device__ inline bool object_runs(bool ok, uint32_t obj, bool tri_new, u64 q, const u64 (&lo)[3], const u64 (&hi)[3],
                                   Commit&& commit) {
    bool ovf = false;
    u64 rem = __ballot(ok);
    while (rem) {
        const int first = __ffsll((long long)rem) - 1;
        const uint32_t k = (uint32_t)__shfl((int)obj, first);
        const bool mine = ok && obj == k;
        const u64 m = __ballot(mine);
        rem &= ~m;
        Part p;
        p.cnt = (uint32_t)__popcll(m);
        p.tris = (uint32_t)__popcll(__ballot(mine && tri_new));
        p.q = mine ? q : 0ull;
        p.l0 = mine ? lo[0] : kImgPosInf;
        p.l1 = mine ? lo[1] : kImgPosInf;
        p.l2 = mine ? lo[2] : kImgPosInf;
        p.h0 = mine ? hi[0] : kImgNegInf;
        p.h1 = mine ? hi[1] : kImgNegInf;
        p.h2 = mine ? hi[2] : kImgNegInf;
        for (int o = 32; o > 0; o >>= 1) {
            p.l0 = min_u64(p.l0, __shfl_xor(p.l0, o));
            p.l1 = min_u64(p.l1, __shfl_xor(p.l1, o));
            p.l2 = min_u64(p.l2, __shfl_xor(p.l2, o));
            p.h0 = max_u64(p.h0, __shfl_xor(p.h0, o));
            p.h1 = max_u64(p.h1, __shfl_xor(p.h1, o));
            p.h2 = max_u64(p.h2, __shfl_xor(p.h2, o));
        }
        if (__ballot(mine && q != 0ull)) {
            for (int o = 32; o > 0; o >>= 1) {
                const u64 s = p.q + __shfl_xor(p.q, o);
                ovf |= s < p.q;
                p.q = s;
            }
        }
        commit(k, p);
    }
    return __ballot(ovf) != 0ull;
}

// Lanes 0..8 of the wave add `p` to one row (LDS or global: the same integer atomics).
__device__ __forceinline__ void commit_row(uint32_t lane, uint32_t* ret, uint32_t* tris, u64* q, u64* lo3, u64* hi3, const Part& p) {
    if (lane == 0) {
        atomicAdd(ret, p.cnt);
    } else if (lane == 1) {
        if (p.tris) atomicAdd(tris, p.tris);
    } else if (lane == 2) {
        if (p.q) atomicAdd(q, p.q);
    } else if (lane == 3) {          // one branch per coordinate: a lane-indexed pick would put the partial in scratch
        atomicMin(lo3, p.l0);
    } else if (lane == 4) {
        atomicMin(lo3 + 1, p.l1);
    } else if (lane == 5) {
        atomicMin(lo3 + 2, p.l2);
    } else if (lane == 6) {
        atomicMax(hi3, p.h0);
    } else if (lane == 7) {
        atomicMax(hi3 + 1, p.h1);
    } else if (lane == 8) {
        atomicMax(hi3 + 2, p.h2);
    }
}

// ---- static table -----------------------------------------------------------------------------------------------
// flag bit 0: a triangle's q reaches 2^63 or a sum of q wrapped
__global__ __launch_bounds__(kBlock) void static_kernel(const double* __restrict__ v, const int32_t* __restrict__ f,
                                                        uint64_t T, const uint16_t* __restrict__ obj_of_tri,
                                                        uint64_t* __restrict__ qtab, uint32_t* __restrict__ tri_count,
                                                        u64* __restrict__ total_q, u64* __restrict__ wlo,
                                                        u64* __restrict__ whi, uint32_t* __restrict__ flag) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = __lane_id();
    const bool ok = j < T;
    uint32_t k = 0;
    u64 q = 0, lo[3] = {kImgPosInf, kImgPosInf, kImgPosInf}, hi[3] = {kImgNegInf, kImgNegInf, kImgNegInf};
    bool bad = false;
    if (ok) {
        uint64_t qq;
        bad = !lrc_area_q(v, f, j, &qq);
        qtab[j] = qq;
        q = qq;
        k = obj_of_tri[j];
        for (int c = 0; c < 3; ++c) {
            const uint64_t vi = (uint32_t)f[3 * j + c];
            for (int a = 0; a < 3; ++a) {
                const u64 im = img_of(v[3 * vi + a]);
                lo[a] = im < lo[a] ? im : lo[a];
                hi[a] = im > hi[a] ? im : hi[a];
            }
        }
    }
    uint32_t* tris_unused = nullptr;
    bool ovf = object_runs(ok, k, false, q, lo, hi, [&](uint32_t kk, const Part& p) {
        if (lane == 2) {
            if (p.q) {
                const u64 old = atomicAdd(&total_q[kk], p.q);
                if (old + p.q < old) atomicOr(flag, 1u);
            }
        } else {
            commit_row(lane, &tri_count[kk], tris_unused, nullptr, wlo + 3 * (uint64_t)kk, whi + 3 * (uint64_t)kk, p);
        }
    });
    if (__ballot(bad) != 0ull) ovf = true;
    if (ovf && lane == 0) atomicOr(flag, 1u);
}

// ---- accumulate -------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
__global__ __launch_bounds__(kBlock) void accumulate_kernel(
    const double* __restrict__ poses, const float* __restrict__ t, const uint32_t* __restrict__ prim,
    const uint32_t* __restrict__ point3, uint64_t N, uint64_t blocks_per_pose, uint64_t first_frame, uint64_t T, uint64_t W,
    uint32_t K, const uint16_t* __restrict__ obj_of_tri, const uint64_t* __restrict__ qtab, uint32_t* __restrict__ bits,
    uint32_t* __restrict__ g_ret, uint32_t* __restrict__ g_tris, u64* __restrict__ g_q, u64* __restrict__ g_lo,
    u64* __restrict__ g_hi, u64* __restrict__ g_rejected) {
    __shared__ uint32_t s_tag[kSlots], s_ret[kSlots], s_tris[kSlots], s_rej;
    __shared__ u64 s_q[kSlots], s_lo[kSlots * 3], s_hi[kSlots * 3];
    for (uint32_t s = threadIdx.x; s < kSlots; s += kBlock) {
        s_tag[s] = kEmpty;
        s_ret[s] = 0;
        s_tris[s] = 0;
        s_q[s] = 0;
    }
    for (uint32_t s = threadIdx.x; s < kSlots * 3; s += kBlock) {
        s_lo[s] = kImgPosInf;
        s_hi[s] = kImgNegInf;
    }
    if (threadIdx.x == 0) s_rej = 0;
    __syncthreads();

    const uint64_t pose = blockIdx.x / blocks_per_pose;            // uniform: a workgroup never spans two poses
    const uint64_t r0 = (blockIdx.x % blocks_per_pose) * kRaysPerBlock;
    const uint64_t frame = first_frame + pose;                     // < num_frames (checked on the host)
    const uint64_t row0 = frame * K;
    const double* __restrict__ M = poses + pose * 16;
    const double r00 = M[0], r01 = M[1], r02 = M[2], c0 = M[3];
    const double r10 = M[4], r11 = M[5], r12 = M[6], c1 = M[7];
    const double r20 = M[8], r21 = M[9], r22 = M[10], c2 = M[11];
    uint32_t* __restrict__ fbits = bits + frame * W;
    const uint32_t lane = __lane_id();
    uint32_t rejected = 0;                                         // wave-uniform

    for (int it = 0; it < kRaysPerThread; ++it) {
        const uint64_t i = r0 + (uint64_t)it * kBlock + threadIdx.x;
        uint32_t p = LRC_INVALID_PRIM, obj = 0;
        bool ok = false, rej = false;
        u64 im[3] = {kImgPosInf, kImgPosInf, kImgPosInf};
        if (i < N) {
            const uint64_t g = pose * N + i;
            const uint32_t tb = __float_as_uint(t[g]);
            p = prim[g];
            ok = finite_bits(tb) && (uint64_t)p < T;               // a returned ray; other rows are not loaded
            if (ok) {
                const uint32_t b0 = point3[3 * g], b1 = point3[3 * g + 1], b2 = point3[3 * g + 2];
                if (finite_bits(b0) && finite_bits(b1) && finite_bits(b2)) {
                    const double e0 = (double)__uint_as_float(b0) - c0;
                    const double e1 = (double)__uint_as_float(b1) - c1;
                    const double e2 = (double)__uint_as_float(b2) - c2;
                    im[0] = img_of((r00 * e0 + r10 * e1) + r20 * e2);
                    im[1] = img_of((r01 * e0 + r11 * e1) + r21 * e2);
                    im[2] = img_of((r02 * e0 + r12 * e1) + r22 * e2);
                    obj = obj_of_tri[p];
                } else {
                    ok = false;
                    rej = true;
                }
            }
        }
        rejected += (uint32_t)__popcll(__ballot(rej));
        const u64 okm = __ballot(ok);
        if (!okm) continue;                                        // uniform
        // runs of equal prim: the head lane of a run owns the triangle's bit of this frame
        const uint32_t prev = (uint32_t)__shfl_up((int)p, 1);
        const bool prev_ok = lane > 0 && ((okm >> (lane - 1)) & 1ull);
        const bool head = ok && !(prev_ok && prev == p);
        bool tri_new = false;
        u64 q = 0;
        if (head) {
            const uint32_t word = p >> 5, m = 1u << (p & 31u);
            if (!(fbits[word] & m)) tri_new = !(atomicOr(&fbits[word], m) & m);
            if (tri_new) q = qtab[p];
        }
        object_runs(ok, obj, tri_new, q, im, im, [&](uint32_t k, const Part& part) {
            const uint32_t slot = k & (kSlots - 1);
            uint32_t owner = 0;
            if (lane == 0) {
                owner = __atomic_load_n(&s_tag[slot], __ATOMIC_RELAXED);
                if (owner == kEmpty) {
                    owner = atomicCAS(&s_tag[slot], kEmpty, k);
                    if (owner == kEmpty) owner = k;
                }
            }
            owner = (uint32_t)__shfl((int)owner, 0);
            if (owner == k) {
                commit_row(lane, &s_ret[slot], &s_tris[slot], &s_q[slot], &s_lo[3 * slot], &s_hi[3 * slot], part);
            } else {                                               // the row belongs to another object: global row
                const uint64_t r = row0 + k;
                commit_row(lane, &g_ret[r], &g_tris[r], &g_q[r], &g_lo[3 * r], &g_hi[3 * r], part);
            }
        });
    }
    if (lane == 0 && rejected) atomicAdd(&s_rej, rejected);
    __syncthreads();
    if (threadIdx.x < kSlots) {
        const uint32_t s = threadIdx.x, k = s_tag[s];
        if (k != kEmpty && s_ret[s]) {                             // a claimed row has at least one return
            const uint64_t r = row0 + k;
            atomicAdd(&g_ret[r], s_ret[s]);
            if (s_tris[s]) atomicAdd(&g_tris[r], s_tris[s]);
            if (s_q[s]) atomicAdd(&g_q[r], s_q[s]);
            for (int a = 0; a < 3; ++a) {
                atomicMin(&g_lo[3 * r + a], s_lo[3 * s + a]);
                atomicMax(&g_hi[3 * r + a], s_hi[3 * s + a]);
            }
        }
    } else if (threadIdx.x == kSlots && s_rej) {
        atomicAdd(g_rejected, (u64)s_rej);
    }
}

// ---- reset / export ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fill_boxes_kernel(u64* __restrict__ lo, u64* __restrict__ hi, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        lo[i] = kImgPosInf;
        hi[i] = kImgNegInf;
    }
}

__global__ __launch_bounds__(kBlock) void export_kernel(uint64_t rows, const uint32_t* __restrict__ g_ret,
                                                        const uint32_t* __restrict__ g_tris, const u64* __restrict__ g_q,
                                                        const u64* __restrict__ g_lo, const u64* __restrict__ g_hi,
                                                        uint32_t* __restrict__ o_ret, uint32_t* __restrict__ o_tris,
                                                        uint64_t* __restrict__ o_q, double* __restrict__ o_lo,
                                                        double* __restrict__ o_hi) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    if (o_ret) o_ret[r] = g_ret[r];
    if (o_tris) o_tris[r] = g_tris[r];
    if (o_q) o_q[r] = g_q[r];
    for (int a = 0; a < 3; ++a) {
        if (o_lo) o_lo[3 * r + a] = dbl_of(g_lo[3 * r + a]);
        if (o_hi) o_hi[3 * r + a] = dbl_of(g_hi[3 * r + a]);
    }
}

}  // namespace

struct lrc_frameobj {
    int device = 0;
    uint64_t T = 0, F = 0, W = 0;
    uint32_t K = 0;
    std::vector<uint32_t> keys, tri_count;     // the static table, host copies
    std::vector<uint64_t> total_q;
    std::vector<double> wmin, wmax;            // K * 3
    uint64_t* d_q = nullptr;                   // T
    uint16_t* d_obj = nullptr;                 // T: object index of every triangle
    uint32_t* d_bits = nullptr;                // F * W
    uint32_t* d_ret = nullptr;                 // F * K
    uint32_t* d_tris = nullptr;                // F * K
    u64* d_sq = nullptr;                       // F * K
    u64* d_lo = nullptr;                       // F * K * 3, images
    u64* d_hi = nullptr;
    u64* d_rej = nullptr;                      // 1
};

namespace {

void release(lrc_frameobj* o) {
    void* ps[] = {o->d_q, o->d_obj, o->d_bits, o->d_ret, o->d_tris, o->d_sq, o->d_lo, o->d_hi, o->d_rej};
    for (void* p : ps)
        if (p) (void)hipFree(p);
}

int enqueue_reset(lrc_frameobj* o, hipStream_t st) {
    const uint64_t rows = o->F * o->K;
    LRC_HIP(hipMemsetAsync(o->d_bits, 0, o->F * o->W * 4, st));
    LRC_HIP(hipMemsetAsync(o->d_ret, 0, rows * 4, st));
    LRC_HIP(hipMemsetAsync(o->d_tris, 0, rows * 4, st));
    LRC_HIP(hipMemsetAsync(o->d_sq, 0, rows * 8, st));
    LRC_HIP(hipMemsetAsync(o->d_rej, 0, 8, st));
    hipLaunchKernelGGL(fill_boxes_kernel, dim3((uint32_t)blocks_of(rows * 3, kBlock)), dim3(kBlock), 0, st, o->d_lo,
                       o->d_hi, rows * 3);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

}  // namespace

extern "C" {

int lrc_frameobj_destroy(lrc_frameobj* fo) {
    if (!fo) return LRC_OK;
    (void)hipSetDevice(fo->device);
    release(fo);
    delete fo;
    return LRC_OK;
}

int lrc_frameobj_create(lrc_ctx* ctx, const double* verts3, uint64_t V, const int32_t* tris3, uint64_t T,
                        const uint16_t* tri_sem, const uint16_t* tri_ins, uint64_t num_frames, lrc_frameobj** out_fo) {
    if (!out_fo) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_create: out_fo is NULL");
    *out_fo = nullptr;
    if (!ctx || !verts3 || !tris3) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_create: NULL argument");
    if (T == 0 || T >= (1ull << 32) - 1 || V == 0)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_create: need 0 < num_triangles < 2^32 - 1 and vertices");
    if (num_frames == 0 || num_frames >= (1ull << 31))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_create: need 0 < num_frames < 2^31");
    if (int rc = check_mesh("lrc_frameobj_create", verts3, V, tris3, T)) return rc;
    const uint64_t W = (T + 31) / 32;
    if (num_frames > (~0ull / 4) / W) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_create: too many frames");
    // objects: the distinct label words, ascending
    std::vector<uint32_t> key(T, 0u);
    if (tri_sem || tri_ins)
        for (uint64_t j = 0; j < T; ++j)
            key[j] = (tri_sem ? (uint32_t)tri_sem[j] : 0u) | ((tri_ins ? (uint32_t)tri_ins[j] : 0u) << 16);
    std::vector<uint32_t> keys = key;
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (keys.size() > kMaxObjects)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_create: more than 4096 distinct objects");
    std::vector<uint16_t> obj(T);
    for (uint64_t j = 0; j < T; ++j)
        obj[j] = (uint16_t)(std::lower_bound(keys.begin(), keys.end(), key[j]) - keys.begin());
    lrc_frameobj* o = new (std::nothrow) lrc_frameobj();
    if (!o) return lrc_internal_fail(LRC_ERR_OOM, "lrc_frameobj_create: out of host memory");
    o->device = ctx->device;
    o->T = T;
    o->F = num_frames;
    o->W = W;
    o->K = (uint32_t)keys.size();
    o->keys = keys;
    const uint64_t K = o->K, rows = o->F * K;
    auto run = [&]() -> int {
        LRC_HIP(hipSetDevice(o->device));
        LRC_HIP(hipMalloc((void**)&o->d_q, T * 8));
        LRC_HIP(hipMalloc((void**)&o->d_obj, T * 2));
        LRC_HIP(hipMalloc((void**)&o->d_bits, o->F * W * 4));
        LRC_HIP(hipMalloc((void**)&o->d_ret, rows * 4));
        LRC_HIP(hipMalloc((void**)&o->d_tris, rows * 4));
        LRC_HIP(hipMalloc((void**)&o->d_sq, rows * 8));
        LRC_HIP(hipMalloc((void**)&o->d_lo, rows * 24));
        LRC_HIP(hipMalloc((void**)&o->d_hi, rows * 24));
        LRC_HIP(hipMalloc((void**)&o->d_rej, 8));
        Buf dv, df, dtab;
        LRC_HIP(hipMalloc(&dv.p, V * 24));
        LRC_HIP(hipMalloc(&df.p, T * 12));
        // the static table: tri_count (K u32, padded to 8 B), total_q (K), wlo / whi (3 K each), flag
        const uint64_t kpad = (K + 1) / 2;
        LRC_HIP(hipMalloc(&dtab.p, (kpad + K + 6 * K + 1) * 8));
        u64* base = (u64*)dtab.p;
        uint32_t* d_cnt = (uint32_t*)base;
        u64 *d_tq = base + kpad, *d_wlo = d_tq + K, *d_whi = d_wlo + 3 * K;
        uint32_t* d_flag = (uint32_t*)(d_whi + 3 * K);
        LRC_HIP(hipMemcpy(dv.p, verts3, V * 24, hipMemcpyHostToDevice));
        LRC_HIP(hipMemcpy(df.p, tris3, T * 12, hipMemcpyHostToDevice));
        LRC_HIP(hipMemcpy(o->d_obj, obj.data(), T * 2, hipMemcpyHostToDevice));
        LRC_HIP(hipMemset(dtab.p, 0, (kpad + K + 6 * K + 1) * 8));
        hipLaunchKernelGGL(fill_boxes_kernel, dim3((uint32_t)blocks_of(3 * K, kBlock)), dim3(kBlock), 0, nullptr, d_wlo,
                           d_whi, 3 * K);
        hipLaunchKernelGGL(static_kernel, dim3((uint32_t)blocks_of(T, kBlock)), dim3(kBlock), 0, nullptr,
                           (const double*)dv.p, (const int32_t*)df.p, T, (const uint16_t*)o->d_obj, o->d_q, d_cnt, d_tq,
                           d_wlo, d_whi, d_flag);
        LRC_HIP(hipGetLastError());
        int rc = enqueue_reset(o, nullptr);
        if (rc != LRC_OK) return rc;
        LRC_HIP(hipDeviceSynchronize());
        std::vector<u64> host(kpad + 7 * K + 1);
        LRC_HIP(hipMemcpy(host.data(), dtab.p, host.size() * 8, hipMemcpyDeviceToHost));
        const uint32_t* h_cnt = (const uint32_t*)host.data();
        const u64 *h_tq = host.data() + kpad, *h_wlo = h_tq + K, *h_whi = h_wlo + 3 * K;
        bool over = (host[kpad + 7 * K] & 0xFFFFFFFFull) != 0;
        u64 sum = 0;
        for (uint64_t k = 0; k < K && !over; ++k) {
            over = sum + h_tq[k] < sum;
            sum += h_tq[k];
        }
        if (over || sum > (1ull << 63))
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_create: total quantised area exceeds 2^63");
        o->tri_count.assign(h_cnt, h_cnt + K);
        o->total_q.assign(h_tq, h_tq + K);
        o->wmin.resize(3 * K);
        o->wmax.resize(3 * K);
        for (uint64_t i = 0; i < 3 * K; ++i) {
            o->wmin[i] = dbl_of(h_wlo[i]);
            o->wmax[i] = dbl_of(h_whi[i]);
        }
        return LRC_OK;
    };
    const int rc = run();
    if (rc != LRC_OK) {
        lrc_frameobj_destroy(o);
        return rc;
    }
    *out_fo = o;
    return LRC_OK;
}

int lrc_frameobj_get_info(const lrc_frameobj* fo, lrc_frameobj_info* out) {
    if (!fo || !out) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_get_info: NULL argument");
    LRC_HIP(hipSetDevice(fo->device));
    LRC_HIP(hipDeviceSynchronize());
    u64 rej = 0;
    LRC_HIP(hipMemcpy(&rej, fo->d_rej, 8, hipMemcpyDeviceToHost));
    out->num_triangles = fo->T;
    out->num_frames = fo->F;
    out->num_objects = fo->K;
    out->words_per_frame = fo->W;
    out->rejected_rays = rej;
    return LRC_OK;
}

int lrc_frameobj_objects(const lrc_frameobj* fo, uint32_t* out_key, uint32_t* out_tri_count, uint64_t* out_total_q,
                         double* out_wmin, double* out_wmax) {
    if (!fo) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_objects: NULL argument");
    const size_t K = fo->K;
    if (out_key) std::copy(fo->keys.begin(), fo->keys.end(), out_key);
    if (out_tri_count) std::copy(fo->tri_count.begin(), fo->tri_count.end(), out_tri_count);
    if (out_total_q) std::copy(fo->total_q.begin(), fo->total_q.end(), out_total_q);
    if (out_wmin) std::copy(fo->wmin.begin(), fo->wmin.begin() + 3 * K, out_wmin);
    if (out_wmax) std::copy(fo->wmax.begin(), fo->wmax.begin() + 3 * K, out_wmax);
    return LRC_OK;
}

int lrc_frameobj_reset(lrc_frameobj* fo, void* stream) {
    if (!fo) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_reset: NULL argument");
    LRC_HIP(hipSetDevice(fo->device));
    return enqueue_reset(fo, (hipStream_t)stream);
}

int lrc_frameobj_accumulate_dev(lrc_frameobj* fo, const double* d_poses16, uint64_t num_poses, uint64_t rays_per_pose,
                                const float* d_t, const uint32_t* d_prim, const float* d_point3, uint64_t first_frame,
                                void* stream) {
    if (!fo || !d_poses16 || !d_t || !d_prim || !d_point3)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_accumulate_dev: NULL argument");
    if (first_frame > fo->F || num_poses > fo->F - first_frame)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_accumulate_dev: first_frame + num_poses > num_frames");
    if (num_poses == 0 || rays_per_pose == 0) return LRC_OK;
    const uint64_t bpp = blocks_of(rays_per_pose, kRaysPerBlock);
    if (num_poses > 0x7FFFFFFFull / bpp)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_accumulate_dev: too many rays for one call");
    LRC_HIP(hipSetDevice(fo->device));
    hipLaunchKernelGGL(accumulate_kernel, dim3((uint32_t)(num_poses * bpp)), dim3(kBlock), 0, (hipStream_t)stream,
                       d_poses16, d_t, d_prim, (const uint32_t*)d_point3, rays_per_pose, bpp, first_frame, fo->T, fo->W,
                       fo->K, (const uint16_t*)fo->d_obj, (const uint64_t*)fo->d_q, fo->d_bits, fo->d_ret, fo->d_tris,
                       fo->d_sq, fo->d_lo, fo->d_hi, fo->d_rej);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_frameobj_export_dev(lrc_frameobj* fo, uint32_t* d_returns, uint32_t* d_seen_tris, uint64_t* d_seen_q,
                            double* d_vmin, double* d_vmax, void* stream) {
    if (!fo) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_export_dev: NULL argument");
    LRC_HIP(hipSetDevice(fo->device));
    const uint64_t rows = fo->F * fo->K;
    hipLaunchKernelGGL(export_kernel, dim3((uint32_t)blocks_of(rows, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, rows,
                       (const uint32_t*)fo->d_ret, (const uint32_t*)fo->d_tris, (const u64*)fo->d_sq, (const u64*)fo->d_lo,
                       (const u64*)fo->d_hi, d_returns, d_seen_tris, d_seen_q, d_vmin, d_vmax);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_frameobj_export(lrc_frameobj* fo, uint32_t* out_returns, uint32_t* out_seen_tris, uint64_t* out_seen_q,
                        double* out_vmin, double* out_vmax) {
    if (!fo) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_frameobj_export: NULL argument");
    LRC_HIP(hipSetDevice(fo->device));
    const uint64_t rows = fo->F * fo->K;
    Buf dlo, dhi;
    if (out_vmin) LRC_HIP(hipMalloc(&dlo.p, rows * 24));
    if (out_vmax) LRC_HIP(hipMalloc(&dhi.p, rows * 24));
    LRC_HIP(hipDeviceSynchronize());          // work the caller enqueued on other streams
    if (out_vmin || out_vmax) {
        const int rc = lrc_frameobj_export_dev(fo, nullptr, nullptr, nullptr, (double*)dlo.p, (double*)dhi.p, nullptr);
        if (rc != LRC_OK) return rc;
    }
    // the copies on the null stream follow the decode kernel
    if (out_returns) LRC_HIP(hipMemcpy(out_returns, fo->d_ret, rows * 4, hipMemcpyDeviceToHost));
    if (out_seen_tris) LRC_HIP(hipMemcpy(out_seen_tris, fo->d_tris, rows * 4, hipMemcpyDeviceToHost));
    if (out_seen_q) LRC_HIP(hipMemcpy(out_seen_q, fo->d_sq, rows * 8, hipMemcpyDeviceToHost));
    if (out_vmin) LRC_HIP(hipMemcpy(out_vmin, dlo.p, rows * 24, hipMemcpyDeviceToHost));
    if (out_vmax) LRC_HIP(hipMemcpy(out_vmax, dhi.p, rows * 24, hipMemcpyDeviceToHost));
    return LRC_OK;
}

}  // extern "C"
