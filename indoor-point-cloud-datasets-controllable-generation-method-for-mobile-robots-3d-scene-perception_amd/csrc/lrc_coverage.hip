// lrc_coverage.hip -- surface coverage of scans: which triangles returned points, per pose set (gfx950).
//
// Definition (include/lidarcast.h): a ray RETURNS a point iff its t is finite; triangle j is SEEN
// by a set of poses iff one returned ray of those poses has prim == j.  Areas are quantised once, q[j] = rint(area_j *
// 2^32) in uint64, so every area sum below is an exact integer sum that does not depend on the order of the additions.
//
// Kernels
//   area_kernel     q[j] from float64 vertices, no contraction (the pragma below), correctly rounded sqrt.
//   accumulate      one workgroup per (pose, run of kRaysPerBlock rays): the pose -> set map is uniform over the
//                   workgroup.  Inside a wave, runs of equal prim are merged: the head lane of a run issues one atomicOr
//                   into the set's bitset (skipped when a plain load already shows the bit) and one atomicAdd of the run
//                   length into hits.  Returned rays are counted per workgroup and added once to returns[set].
//   summary         one thread per bitset word: the bits of one set, of the OR of all sets, or of every triangle (the
//                   totals), summed into a workgroup partial (plus per-class partials in LDS) and added with one 64-bit
//                   atomic per workgroup and class.  Wrap-around of any uint64 sum is detected and reported.
//   gain / pick / or  the greedy selection, entirely on the device: the pick of round r is read by the launches of
//                   round r + 1 through a small state record, one host synchronisation at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "lrc_internal.h"
#include "lrc_area.h"

namespace {

constexpr int kRaysPerThread = 4;
constexpr uint64_t kRaysPerBlock = (uint64_t)kBlock * kRaysPerThread;
constexpr int kWordsPerThread = 4;           // gain kernel
constexpr uint32_t kMaxClasses = 4096;       // distinct tri_sem values (per-class partials live in LDS)
constexpr uint32_t kNoPick = 0xFFFFFFFFu;

struct SelectState {
    uint32_t done;           // 1: no further round picks
    uint32_t win;            // set picked by the current round, kNoPick if none
    uint32_t round;
    uint32_t reserved_;
};

// ---- area table -------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
__global__ __launch_bounds__(kBlock) void area_kernel(const double* __restrict__ v, const int32_t* __restrict__ f,
                                                      uint64_t T, uint64_t* __restrict__ q, uint32_t* __restrict__ flag) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= T) return;
    if (!lrc_area_q(v, f, j, &q[j])) atomicOr(flag, 1u);  // lrc_area.h: the one definition of q
}

// ---- accumulate -------------------------------------------------------------------------------------------------
__device__ inline uint32_t next_boundary(unsigned long long boundary, uint32_t lane) {
    const unsigned long long above = lane == 63 ? 0ull : (boundary >> (lane + 1)) << (lane + 1);
    return above ? (uint32_t)__ffsll((long long)above) - 1 : 64u;
}

__global__ __launch_bounds__(kBlock) void accumulate_kernel(const float* __restrict__ t, const uint32_t* __restrict__ prim,
                                                            uint64_t N, uint64_t blocks_per_pose,
                                                            const uint32_t* __restrict__ set_of_pose, uint64_t S, uint64_t T,
                                                            uint64_t W, uint32_t* __restrict__ bits,
                                                            uint32_t* __restrict__ hits, unsigned long long* __restrict__ returns) {
    __shared__ uint32_t s_ret[kBlock / 64];
    const uint64_t pose = blockIdx.x / blocks_per_pose;
    const uint64_t r0 = (blockIdx.x % blocks_per_pose) * kRaysPerBlock;
    const uint64_t set = set_of_pose ? (uint64_t)set_of_pose[pose] : pose;
    if (set >= S) return;                                // uniform over the workgroup: out-of-range sets are ignored
    uint32_t* __restrict__ sbits = bits + set * W;
    const uint32_t lane = __lane_id();
    uint32_t returned = 0;                               // wave-uniform
    for (int it = 0; it < kRaysPerThread; ++it) {
        const uint64_t i = r0 + (uint64_t)it * kBlock + threadIdx.x;
        uint32_t p = LRC_INVALID_PRIM;
        bool ok = false;
        if (i < N) {
            const uint64_t g = pose * N + i;
            const uint32_t tb = __float_as_uint(t[g]);
            p = prim[g];
            ok = (tb & 0x7f800000u) != 0x7f800000u && (uint64_t)p < T;      // finite t, valid triangle
        }
        const unsigned long long okm = __ballot(ok);
        returned += (uint32_t)__popcll(okm);
        const uint32_t prev = (uint32_t)__shfl_up((int)p, 1);
        const bool prev_ok = lane > 0 && ((okm >> (lane - 1)) & 1ull);
        const bool head = ok && !(prev_ok && prev == p);
        const unsigned long long boundary = __ballot(head) | ~okm;
        if (head) {
            const uint32_t len = next_boundary(boundary, lane) - lane;
            const uint32_t word = p >> 5, m = 1u << (p & 31u);
            if (!(sbits[word] & m)) atomicOr(&sbits[word], m);
            atomicAdd(&hits[p], len);
        }
    }
    if (lane == 0) s_ret[threadIdx.x / 64] = returned;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t n = 0;
        for (int w = 0; w < kBlock / 64; ++w) n += s_ret[w];
        if (n) atomicAdd(&returns[set], (unsigned long long)n);
    }
}

// ---- summaries --------------------------------------------------------------------------------------------------
__device__ inline uint32_t tail_mask(uint64_t w, uint64_t T) {
    const uint64_t lo = w * 32;
    return T - lo >= 32 ? 0xFFFFFFFFu : ((1u << (uint32_t)(T - lo)) - 1u);
}

// out: [0] covered_q, [1] total_q (written by workgroup 0), [2] seen triangles, [3] returned rays (workgroup 0)
__global__ __launch_bounds__(kBlock) void summary_kernel(const uint32_t* __restrict__ bits, uint64_t nsets, uint64_t W,
                                                         uint64_t T, const uint64_t* __restrict__ q,
                                                         const uint16_t* __restrict__ cls, uint32_t C,
                                                         const unsigned long long* __restrict__ returns, uint64_t nret,
                                                         const unsigned long long* __restrict__ total_q,
                                                         uint32_t* __restrict__ out_bits, unsigned long long* __restrict__ out,
                                                         unsigned long long* __restrict__ out_cls, uint32_t* __restrict__ flag) {
    extern __shared__ unsigned long long s_cls[];
    __shared__ unsigned long long s_sum[kBlock], s_cnt[kBlock];
    __shared__ uint32_t s_ovf;
    for (uint32_t c = threadIdx.x; c < C; c += kBlock) s_cls[c] = 0;
    if (threadIdx.x == 0) s_ovf = 0;
    __syncthreads();
    const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long sum = 0, cnt = 0;
    uint32_t ovf = 0;
    if (w < W) {
        uint32_t x = 0xFFFFFFFFu;
        if (bits) {
            x = 0;
            for (uint64_t k = 0; k < nsets; ++k) x |= bits[k * W + w];
        }
        x &= tail_mask(w, T);
        if (out_bits) out_bits[w] = x;
        cnt = (unsigned long long)__popc(x);
        while (x) {
            const uint32_t b = (uint32_t)__ffs((int)x) - 1;
            x &= x - 1;
            const uint64_t j = w * 32 + b;
            const unsigned long long qj = q[j];
            ovf |= (sum + qj < sum);
            sum += qj;
            if (C) atomicAdd(&s_cls[cls[j]], qj);
        }
    }
    s_sum[threadIdx.x] = sum;
    s_cnt[threadIdx.x] = cnt;
    if (ovf) s_ovf = 1;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            const unsigned long long a = s_sum[threadIdx.x], b = s_sum[threadIdx.x + h];
            if (a + b < a) s_ovf = 1;
            s_sum[threadIdx.x] = a + b;
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long a = s_sum[0];
        if (a) {
            const unsigned long long old = atomicAdd(&out[0], a);
            if (old + a < old) s_ovf = 1;
        }
        if (s_cnt[0]) atomicAdd(&out[2], s_cnt[0]);
        if (s_ovf && flag) atomicOr(flag, 1u);
    }
    for (uint32_t c = threadIdx.x; c < C; c += kBlock)
        if (s_cls[c]) atomicAdd(&out_cls[c], s_cls[c]);
    if (blockIdx.x == 0) {                                 // returned rays of the chosen sets, and the mesh total
        __syncthreads();
        unsigned long long r = 0;
        for (uint64_t k = threadIdx.x; k < nret; k += kBlock) r += returns[k];
        s_cnt[threadIdx.x] = r;
        __syncthreads();
        for (int h = kBlock / 2; h > 0; h >>= 1) {
            if (threadIdx.x < h) s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            out[3] = s_cnt[0];
            out[1] = total_q ? *total_q : 0ull;
        }
    }
}

// ---- greedy selection -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gain_kernel(const uint32_t* __restrict__ bits, uint64_t W, uint64_t T,
                                                      uint64_t blocks_per_set, const uint32_t* __restrict__ covered,
                                                      const uint64_t* __restrict__ q, const uint32_t* __restrict__ picked,
                                                      const SelectState* __restrict__ st,
                                                      unsigned long long* __restrict__ gains) {
    __shared__ unsigned long long s_sum[kBlock / 64];
    if (st->done) return;
    const uint64_t k = blockIdx.x / blocks_per_set;
    if (picked[k]) return;                                 // its bits are all covered: gain 0
    const uint64_t w0 = (blockIdx.x % blocks_per_set) * (uint64_t)(kBlock * kWordsPerThread);
    const uint32_t* __restrict__ sb = bits + k * W;
    unsigned long long g = 0;
    for (int it = 0; it < kWordsPerThread; ++it) {
        const uint64_t w = w0 + (uint64_t)it * kBlock + threadIdx.x;
        if (w >= W) break;
        uint32_t x = sb[w];
        if (!x) continue;
        x &= ~covered[w] & tail_mask(w, T);
        while (x) {
            const uint32_t b = (uint32_t)__ffs((int)x) - 1;
            x &= x - 1;
            g += q[w * 32 + b];
        }
    }
    for (int o = 32; o > 0; o >>= 1) g += __shfl_down(g, o);
    if (__lane_id() == 0) s_sum[threadIdx.x / 64] = g;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < kBlock / 64; ++w) s += s_sum[w];
        if (s) atomicAdd(&gains[k], s);
    }
}

// One workgroup: the largest gain, ties to the smallest set index; gains are zeroed for the next round.
__global__ __launch_bounds__(1024) void pick_kernel(unsigned long long* __restrict__ gains, uint64_t S, uint32_t budget,
                                                    double target, unsigned long long* __restrict__ covered_q,
                                                    const unsigned long long* __restrict__ total_q,
                                                    uint32_t* __restrict__ picked, SelectState* __restrict__ st,
                                                    uint32_t* __restrict__ out_picks, unsigned long long* __restrict__ out_gains,
                                                    uint32_t* __restrict__ out_num) {
    __shared__ unsigned long long s_g[1024];
    __shared__ uint32_t s_k[1024];
    __shared__ uint32_t s_done;
    if (threadIdx.x == 0) {
        uint32_t done = st->done;
        // already at the target before this round (an initial cover, or the previous pick reached it)
        if (!done && target > 0.0 && *total_q && (double)*covered_q / (double)*total_q >= target) done = 1;
        if (!done && st->round >= budget) done = 1;
        st->done = done;
        st->win = kNoPick;
        s_done = done;
    }
    __syncthreads();
    if (s_done) return;
    unsigned long long bg = 0;
    uint32_t bk = kNoPick;
    for (uint64_t k = threadIdx.x; k < S; k += 1024) {
        const unsigned long long g = gains[k];
        if (g > bg) { bg = g; bk = (uint32_t)k; }          // k ascends per thread: the first maximum is kept
        gains[k] = 0;
    }
    s_g[threadIdx.x] = bg;
    s_k[threadIdx.x] = bk;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            const unsigned long long g2 = s_g[threadIdx.x + h];
            const uint32_t k2 = s_k[threadIdx.x + h];
            if (g2 > s_g[threadIdx.x] || (g2 == s_g[threadIdx.x] && k2 < s_k[threadIdx.x])) {
                s_g[threadIdx.x] = g2;
                s_k[threadIdx.x] = k2;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long g = s_g[0];
        if (g == 0) {
            st->done = 1;
            return;
        }
        const uint32_t r = st->round;
        out_picks[r] = s_k[0];
        out_gains[r] = g;
        *out_num = r + 1;
        *covered_q += g;
        picked[s_k[0]] = 1;
        st->win = s_k[0];
        st->round = r + 1;
    }
}

__global__ __launch_bounds__(kBlock) void or_kernel(const uint32_t* __restrict__ bits, uint64_t W,
                                                    const SelectState* __restrict__ st, uint32_t* __restrict__ covered) {
    const uint32_t k = st->win;
    if (k == kNoPick) return;
    const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w < W) covered[w] |= bits[(uint64_t)k * W + w];
}

}  // namespace

struct lrc_coverage {
    int device = 0;
    uint64_t T = 0, S = 0, W = 0;
    uint32_t C = 0;
    std::vector<uint16_t> class_ids;       // dense class index -> tri_sem value
    std::vector<uint64_t> class_total_q;
    uint64_t total_q = 0;
    uint64_t* d_q = nullptr;
    uint16_t* d_cls = nullptr;
    uint32_t* d_bits = nullptr;            // S * W
    uint32_t* d_hits = nullptr;            // T
    unsigned long long* d_returns = nullptr;   // S
    unsigned long long* d_scratch = nullptr;   // [0..3] summary, [4] total_q, [5] flag, [8 .. 8 + C) per-class
    uint32_t* d_covered = nullptr;         // W, selection
    unsigned long long* d_gains = nullptr; // S
    uint32_t* d_picked = nullptr;          // S
    SelectState* d_state = nullptr;
};

namespace {

void release(lrc_coverage* c) {
    void* ps[] = {c->d_q, c->d_cls, c->d_bits, c->d_hits, c->d_returns, c->d_scratch, c->d_covered, c->d_gains,
                  c->d_picked, c->d_state};
    for (void* p : ps)
        if (p) (void)hipFree(p);
}

// summary of (bits, nsets) into out (4 words) and out_cls (C words), both zeroed here; stream-ordered
int launch_summary(lrc_coverage* c, const uint32_t* bits, uint64_t nsets, const unsigned long long* returns,
                   uint64_t nret, const unsigned long long* total_q, uint32_t* out_bits, unsigned long long* out,
                   unsigned long long* out_cls, uint32_t* flag, hipStream_t st) {
    LRC_HIP(hipMemsetAsync(out, 0, 32, st));
    if (c->C) LRC_HIP(hipMemsetAsync(out_cls, 0, (size_t)c->C * 8, st));
    hipLaunchKernelGGL(summary_kernel, dim3((uint32_t)blocks_of(c->W, kBlock)), dim3(kBlock), (size_t)c->C * 8, st, bits,
                       nsets, c->W, c->T, (const uint64_t*)c->d_q, (const uint16_t*)c->d_cls, c->C, returns, nret, total_q,
                       out_bits, out, out_cls, flag);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int check_set(const lrc_coverage* c, int64_t set_index, const char* who) {
    if (set_index >= 0 && (uint64_t)set_index >= c->S)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, (std::string(who) + ": set_index >= num_sets").c_str());
    return LRC_OK;
}

}  // namespace

extern "C" {

int lrc_coverage_destroy(lrc_coverage* cov) {
    if (!cov) return LRC_OK;
    (void)hipSetDevice(cov->device);
    release(cov);
    delete cov;
    return LRC_OK;
}

int lrc_coverage_create(lrc_ctx* ctx, const double* verts3, uint64_t V, const int32_t* tris3, uint64_t T,
                        const uint16_t* tri_sem, uint64_t num_sets, lrc_coverage** out_cov) {
    if (!out_cov) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_create: out_cov is NULL");
    *out_cov = nullptr;
    if (!ctx || !verts3 || !tris3) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_create: NULL argument");
    if (T == 0 || T >= (1ull << 32) - 1 || V == 0)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_create: need 0 < num_triangles < 2^32 - 1 and vertices");
    if (num_sets == 0 || num_sets >= (1ull << 31))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_create: need 0 < num_sets < 2^31");
    if (int rc = check_mesh("lrc_coverage_create", verts3, V, tris3, T)) return rc;
    const uint64_t W = (T + 31) / 32;
    if (num_sets > (~0ull / 4) / W) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_create: too many sets");
    lrc_coverage* c = new (std::nothrow) lrc_coverage();
    if (!c) return lrc_internal_fail(LRC_ERR_OOM, "lrc_coverage_create: out of host memory");
    c->device = ctx->device;
    c->T = T;
    c->S = num_sets;
    c->W = W;
    std::vector<uint16_t> dense;
    if (tri_sem) {
        std::vector<int32_t> slot(65536, -1);
        dense.resize(T);
        for (uint64_t j = 0; j < T; ++j) {
            int32_t& s = slot[tri_sem[j]];
            if (s < 0) {
                if (c->class_ids.size() >= kMaxClasses) {
                    delete c;
                    return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_create: more than 4096 distinct labels");
                }
                s = (int32_t)c->class_ids.size();
                c->class_ids.push_back(tri_sem[j]);
            }
            dense[j] = (uint16_t)s;
        }
        // dense indices follow ascending label values
        std::vector<uint16_t> sorted = c->class_ids;
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 0; i < sorted.size(); ++i) slot[sorted[i]] = (int32_t)i;
        for (uint64_t j = 0; j < T; ++j) dense[j] = (uint16_t)slot[tri_sem[j]];
        c->class_ids = sorted;
        c->C = (uint32_t)sorted.size();
    }
    int rc = LRC_OK;
    auto run = [&]() -> int {
        LRC_HIP(hipSetDevice(c->device));
        LRC_HIP(hipMalloc((void**)&c->d_q, T * 8));
        if (c->C) LRC_HIP(hipMalloc((void**)&c->d_cls, T * 2));
        LRC_HIP(hipMalloc((void**)&c->d_bits, c->S * W * 4));
        LRC_HIP(hipMalloc((void**)&c->d_hits, T * 4));
        LRC_HIP(hipMalloc((void**)&c->d_returns, c->S * 8));
        LRC_HIP(hipMalloc((void**)&c->d_scratch, (8 + (size_t)c->C) * 8));
        LRC_HIP(hipMalloc((void**)&c->d_covered, W * 4));
        LRC_HIP(hipMalloc((void**)&c->d_gains, c->S * 8));
        LRC_HIP(hipMalloc((void**)&c->d_picked, c->S * 4));
        LRC_HIP(hipMalloc((void**)&c->d_state, sizeof(SelectState)));
        Buf dv, df;
        LRC_HIP(hipMalloc(&dv.p, V * 24));
        LRC_HIP(hipMalloc(&df.p, T * 12));
        LRC_HIP(hipMemcpy(dv.p, verts3, V * 24, hipMemcpyHostToDevice));
        LRC_HIP(hipMemcpy(df.p, tris3, T * 12, hipMemcpyHostToDevice));
        if (c->C) LRC_HIP(hipMemcpy(c->d_cls, dense.data(), T * 2, hipMemcpyHostToDevice));
        LRC_HIP(hipMemset(c->d_bits, 0, c->S * W * 4));
        LRC_HIP(hipMemset(c->d_hits, 0, T * 4));
        LRC_HIP(hipMemset(c->d_returns, 0, c->S * 8));
        LRC_HIP(hipMemset(c->d_scratch, 0, (8 + (size_t)c->C) * 8));
        uint32_t* flag = (uint32_t*)(c->d_scratch + 5);
        hipLaunchKernelGGL(area_kernel, dim3((uint32_t)blocks_of(T, kBlock)), dim3(kBlock), 0, nullptr,
                           (const double*)dv.p, (const int32_t*)df.p, T, c->d_q, flag);
        LRC_HIP(hipGetLastError());
        int r = launch_summary(c, nullptr, 0, c->d_returns, 0, nullptr, nullptr, c->d_scratch, c->d_scratch + 8, flag,
                               nullptr);
        if (r != LRC_OK) return r;
        LRC_HIP(hipDeviceSynchronize());
        std::vector<unsigned long long> host(8 + c->C);
        LRC_HIP(hipMemcpy(host.data(), c->d_scratch, host.size() * 8, hipMemcpyDeviceToHost));
        if (host[5] || host[0] > (1ull << 63))
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_create: total quantised area exceeds 2^63");
        c->total_q = host[0];
        c->class_total_q.assign(host.begin() + 8, host.end());
        LRC_HIP(hipMemcpy(c->d_scratch + 4, &c->total_q, 8, hipMemcpyHostToDevice));
        return LRC_OK;
    };
    rc = run();
    if (rc != LRC_OK) {
        lrc_coverage_destroy(c);
        return rc;
    }
    *out_cov = c;
    return LRC_OK;
}

int lrc_coverage_get_info(const lrc_coverage* cov, lrc_coverage_info* out) {
    if (!cov || !out) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_get_info: NULL argument");
    out->num_triangles = cov->T;
    out->num_sets = cov->S;
    out->words_per_set = cov->W;
    out->total_q = cov->total_q;
    out->num_classes = cov->C;
    out->reserved_ = 0;
    return LRC_OK;
}

int lrc_coverage_classes(const lrc_coverage* cov, uint16_t* out_class_ids, uint64_t* out_total_q) {
    if (!cov) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_classes: NULL argument");
    for (uint32_t i = 0; i < cov->C; ++i) {
        if (out_class_ids) out_class_ids[i] = cov->class_ids[i];
        if (out_total_q) out_total_q[i] = cov->class_total_q[i];
    }
    return LRC_OK;
}

int lrc_coverage_reset(lrc_coverage* cov, void* stream) {
    if (!cov) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_reset: NULL argument");
    const hipStream_t st = (hipStream_t)stream;
    LRC_HIP(hipSetDevice(cov->device));
    LRC_HIP(hipMemsetAsync(cov->d_bits, 0, cov->S * cov->W * 4, st));
    LRC_HIP(hipMemsetAsync(cov->d_hits, 0, cov->T * 4, st));
    LRC_HIP(hipMemsetAsync(cov->d_returns, 0, cov->S * 8, st));
    return LRC_OK;
}

int lrc_coverage_accumulate_dev(lrc_coverage* cov, const float* d_t, const uint32_t* d_prim, uint64_t num_poses,
                                uint64_t rays_per_pose, const uint32_t* d_set_of_pose, void* stream) {
    if (!cov || ((!d_t || !d_prim) && num_poses && rays_per_pose))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_accumulate_dev: NULL argument");
    if (!d_set_of_pose && num_poses > cov->S)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG,
                                 "lrc_coverage_accumulate_dev: without set_of_pose, num_poses must not exceed num_sets");
    if (num_poses == 0 || rays_per_pose == 0) return LRC_OK;
    const uint64_t bpp = blocks_of(rays_per_pose, kRaysPerBlock);
    if (num_poses > 0x7FFFFFFFull / bpp)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_accumulate_dev: too many rays for one call");
    LRC_HIP(hipSetDevice(cov->device));
    hipLaunchKernelGGL(accumulate_kernel, dim3((uint32_t)(num_poses * bpp)), dim3(kBlock), 0, (hipStream_t)stream, d_t,
                       d_prim, rays_per_pose, bpp, d_set_of_pose, cov->S, cov->T, cov->W, cov->d_bits, cov->d_hits,
                       cov->d_returns);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_coverage_summary_dev(lrc_coverage* cov, int64_t set_index, uint64_t* d_out4, uint64_t* d_out_class_q,
                             uint32_t* d_out_bits, void* stream) {
    if (!cov || !d_out4 || (cov->C && !d_out_class_q))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_summary_dev: NULL argument");
    int rc = check_set(cov, set_index, "lrc_coverage_summary_dev");
    if (rc != LRC_OK) return rc;
    LRC_HIP(hipSetDevice(cov->device));
    const bool all = set_index < 0;
    const uint64_t k = all ? 0 : (uint64_t)set_index;
    return launch_summary(cov, cov->d_bits + k * cov->W, all ? cov->S : 1, cov->d_returns + k, all ? cov->S : 1,
                          cov->d_scratch + 4, d_out_bits, (unsigned long long*)d_out4, (unsigned long long*)d_out_class_q,
                          nullptr, (hipStream_t)stream);
}

int lrc_coverage_summary(lrc_coverage* cov, int64_t set_index, lrc_coverage_stats* out, uint64_t* out_class_q,
                         uint32_t* out_bits) {
    if (!cov || !out || (cov->C && !out_class_q))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_summary: NULL argument");
    int rc = check_set(cov, set_index, "lrc_coverage_summary");
    if (rc != LRC_OK) return rc;
    LRC_HIP(hipSetDevice(cov->device));
    Buf db;
    if (out_bits) LRC_HIP(hipMalloc(&db.p, cov->W * 4));
    LRC_HIP(hipDeviceSynchronize());          // work the caller enqueued on other streams
    // the object's scratch holds the per-class totals of the mesh: summaries go to a buffer of their own
    Buf dout;
    LRC_HIP(hipMalloc(&dout.p, (4 + (size_t)cov->C) * 8));
    uint64_t* d4 = (uint64_t*)dout.p;
    rc = lrc_coverage_summary_dev(cov, set_index, d4, d4 + 4, (uint32_t*)db.p, nullptr);
    if (rc != LRC_OK) return rc;
    std::vector<uint64_t> host(4 + cov->C);
    LRC_HIP(hipMemcpy(host.data(), d4, host.size() * 8, hipMemcpyDeviceToHost));
    out->covered_q = host[0];
    out->total_q = host[1];
    out->seen_triangles = host[2];
    out->returns = host[3];
    for (uint32_t i = 0; i < cov->C; ++i) out_class_q[i] = host[4 + i];
    if (out_bits) LRC_HIP(hipMemcpy(out_bits, db.p, cov->W * 4, hipMemcpyDeviceToHost));
    return LRC_OK;
}

int lrc_coverage_select_dev(lrc_coverage* cov, uint32_t budget, double target_ratio, const uint32_t* d_initial_bits,
                            uint32_t* d_out_picks, uint64_t* d_out_gains, uint32_t* d_out_num_picks, void* stream) {
    if (!cov || !d_out_num_picks || (budget && (!d_out_picks || !d_out_gains)))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_select_dev: NULL argument");
    if (!(target_ratio == target_ratio))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_select_dev: target_ratio is NaN");
    const hipStream_t st = (hipStream_t)stream;
    LRC_HIP(hipSetDevice(cov->device));
    const uint64_t W = cov->W, S = cov->S;
    if (d_initial_bits) LRC_HIP(hipMemcpyAsync(cov->d_covered, d_initial_bits, W * 4, hipMemcpyDeviceToDevice, st));
    else LRC_HIP(hipMemsetAsync(cov->d_covered, 0, W * 4, st));
    LRC_HIP(hipMemsetAsync(cov->d_gains, 0, S * 8, st));
    LRC_HIP(hipMemsetAsync(cov->d_picked, 0, S * 4, st));
    LRC_HIP(hipMemsetAsync(cov->d_state, 0, sizeof(SelectState), st));
    LRC_HIP(hipMemsetAsync(d_out_num_picks, 0, 4, st));
    // covered_q of the initial cover (masked to the mesh's triangles) -> d_scratch[0]; the caller's bits stay as given
    unsigned long long* cq = cov->d_scratch;
    if (d_initial_bits) {
        int rc = launch_summary(cov, cov->d_covered, 1, cov->d_returns, 0, cov->d_scratch + 4, nullptr, cq,
                                cov->d_scratch + 8, nullptr, st);
        if (rc != LRC_OK) return rc;
    } else {
        LRC_HIP(hipMemsetAsync(cq, 0, 8, st));
    }
    const uint64_t per_set = blocks_of(W, (uint64_t)kBlock * kWordsPerThread);
    if (S > 0x7FFFFFFFull / per_set) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_select_dev: too many sets");
    const uint64_t rounds = budget < S ? budget : S;
    for (uint64_t r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(gain_kernel, dim3((uint32_t)(S * per_set)), dim3(kBlock), 0, st, (const uint32_t*)cov->d_bits,
                           W, cov->T, per_set, (const uint32_t*)cov->d_covered, (const uint64_t*)cov->d_q,
                           (const uint32_t*)cov->d_picked, (const SelectState*)cov->d_state, cov->d_gains);
        hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(1024), 0, st, cov->d_gains, S, budget, target_ratio, cq,
                           (const unsigned long long*)(cov->d_scratch + 4), cov->d_picked, cov->d_state, d_out_picks,
                           (unsigned long long*)d_out_gains, d_out_num_picks);
        hipLaunchKernelGGL(or_kernel, dim3((uint32_t)blocks_of(W, kBlock)), dim3(kBlock), 0, st,
                           (const uint32_t*)cov->d_bits, W, (const SelectState*)cov->d_state, cov->d_covered);
        LRC_HIP(hipGetLastError());
    }
    return LRC_OK;
}

int lrc_coverage_select(lrc_coverage* cov, uint32_t budget, double target_ratio, const uint32_t* initial_bits,
                        uint32_t* out_picks, uint64_t* out_gains, uint32_t* out_num_picks) {
    if (!cov || !out_num_picks || (budget && (!out_picks || !out_gains)))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_select: NULL argument");
    LRC_HIP(hipSetDevice(cov->device));
    LRC_HIP(hipDeviceSynchronize());
    Buf di, dp, dg, dn;
    if (initial_bits) {
        LRC_HIP(hipMalloc(&di.p, cov->W * 4));
        LRC_HIP(hipMemcpy(di.p, initial_bits, cov->W * 4, hipMemcpyHostToDevice));
    }
    const uint64_t m = budget ? budget : 1;
    LRC_HIP(hipMalloc(&dp.p, m * 4));
    LRC_HIP(hipMalloc(&dg.p, m * 8));
    LRC_HIP(hipMalloc(&dn.p, 4));
    int rc = lrc_coverage_select_dev(cov, budget, target_ratio, (const uint32_t*)di.p, (uint32_t*)dp.p, (uint64_t*)dg.p,
                                     (uint32_t*)dn.p, nullptr);
    if (rc != LRC_OK) return rc;
    LRC_HIP(hipMemcpy(out_num_picks, dn.p, 4, hipMemcpyDeviceToHost));      // the one synchronisation
    if (*out_num_picks) {
        LRC_HIP(hipMemcpy(out_picks, dp.p, (size_t)*out_num_picks * 4, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out_gains, dg.p, (size_t)*out_num_picks * 8, hipMemcpyDeviceToHost));
    }
    return LRC_OK;
}

int lrc_coverage_export(lrc_coverage* cov, uint32_t* out_bits, uint32_t* out_hits, uint64_t* out_returns,
                        uint64_t* out_q) {
    if (!cov) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_coverage_export: NULL argument");
    LRC_HIP(hipSetDevice(cov->device));
    LRC_HIP(hipDeviceSynchronize());
    if (out_bits) LRC_HIP(hipMemcpy(out_bits, cov->d_bits, cov->S * cov->W * 4, hipMemcpyDeviceToHost));
    if (out_hits) LRC_HIP(hipMemcpy(out_hits, cov->d_hits, cov->T * 4, hipMemcpyDeviceToHost));
    if (out_returns) LRC_HIP(hipMemcpy(out_returns, cov->d_returns, cov->S * 8, hipMemcpyDeviceToHost));
    if (out_q) LRC_HIP(hipMemcpy(out_q, cov->d_q, cov->T * 8, hipMemcpyDeviceToHost));
    return LRC_OK;
}

}  // extern "C"
