// lrc_objboxes.hip -- S3DIS annotation boxes: Open3D's statistical outlier filter inside each of many float64 objects
// and the axis-aligned box of what is left, every object of a room or an area in one call (gfx950).
//
// The reference's s3dis_bbox_visualizer.py loads every Annotations/<class>_<k>.txt of a room, runs
// remove_statistical_outlier(nb_neighbors=20, std_ratio=2.0) on each object of 20 rows or more (:70-94) and takes the
// min / max of the kept rows (:96-116).  An object here is a run of rows [off[s], off[s+1]) of one concatenated cloud;
// an object of m >= k rows gets exactly the outlier stage of lrc_cloud_preprocess run on its rows alone (the walk,
// avg and the reduction order come from lrc_knn64.h), an object of m < k rows keeps every row (avg = -1).
//   1. bounds: an (object, chunk) grid of workgroups folds each object's float64 bounds into order-preserving integer
//      keys with 64-bit atomic min / max (min / max are order-free) and flags non-finite coordinates; one host sync;
//   2. grid: per object a cell size of about k rows per cell of a sheet over the largest face of its box, at most m
//      cells; each object owns the cell range [base[s], base[s] + m) of one global table (base: a host prefix sum),
//      so one stable radix sort of all rows by global cell key and one counting table serve every object;
//   3. k-NN: one lane per row in cell order; a wavefront walks one object at a time (readfirstlane over the objects of
//      its lanes), so the object's grid stays in scalar registers as the single-cloud kernel's does;
//   4. mean / threshold: an (object, chunk) grid of workgroups reduces each chunk exactly as pp_sum_kernel does for a
//      cloud of m rows, one workgroup per object folds the chunks as pp_final_kernel does; keep = avg > 0 && avg < thr;
//   5. a scan of the keep flags compacts the kept rows (ascending, object after object), and a second bounds pass over
//      the kept rows gives each box.
// Launches and host synchronisations do not depend on the number of objects.  Results depend on distances only, so the
// bytes do not change with the cell size or with the order of the objects.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "lrc_knn64.h"

namespace {

constexpr uint32_t kMaxRowsY = 65535;   // objects per grid row of the (object, chunk) launches; blocks stride beyond

// float64 -> uint64 with the same order for finite values (and -0 < +0)
__device__ __forceinline__ uint64_t ord_key(uint64_t b) { return (b >> 63) ? ~b : (b | (1ull << 63)); }
__device__ __forceinline__ double ord_val(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// object of row i: the last s with off[s] <= i (empty objects share their offset with the next one)
__device__ __forceinline__ uint32_t object_of(const uint64_t* __restrict__ off, uint32_t S, uint64_t i) {
    uint32_t lo = 0, hi = S;                    // off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// (chunk, object) workgroups: order keys of each object's min / max over its rows (flag == nullptr) or over its kept
// rows; keys[6 s .. 6 s + 6) = lo x y z, hi x y z.  The first pass also flags non-finite coordinates, which it skips.
// zrow (kept pass): per object and axis, 1 + the last kept row whose coordinate is +0 or -0.  numpy's min / max over
// the rows (a running np.minimum / np.maximum, row after row) keeps the later of two equal values, so a zero extreme
// takes the sign of the last zero row, not the -0 < +0 order of the keys.
__global__ __launch_bounds__(kBlock) void ob_bounds_kernel(const double* __restrict__ p, const uint64_t* __restrict__ off,
                                                          uint32_t S, const uint32_t* __restrict__ flag,
                                                          unsigned long long* __restrict__ keys, uint32_t* __restrict__ bad,
                                                          unsigned long long* __restrict__ zrow) {
    __shared__ unsigned long long red[9][kBlock];
    const uint32_t t = threadIdx.x;
    for (uint32_t s = blockIdx.y; s < S; s += gridDim.y) {
        const uint64_t a0 = off[s], m = off[s + 1] - a0;
        const uint64_t chunk = (m + kRedBlocks - 1) / kRedBlocks;
        if ((uint64_t)blockIdx.x * chunk >= m) continue;            // the whole workgroup: same s, same chunk
        const uint64_t a = a0 + (uint64_t)blockIdx.x * chunk, e = min(a + chunk, a0 + m);
        unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0}, zr[3] = {0, 0, 0};
        uint32_t nf = 0;
        for (uint64_t i = a + t; i < e; i += kBlock) {
            if (flag && !flag[i]) continue;
            for (int c = 0; c < 3; ++c) {
                const uint64_t b = reinterpret_cast<const uint64_t*>(p)[3 * i + c];
                if (non_finite_bits(b)) { nf = 1; continue; }
                const unsigned long long kb = ord_key(b);
                lo[c] = min(lo[c], kb);
                hi[c] = max(hi[c], kb);
                if ((b << 1) == 0) zr[c] = i + 1;                 // rows ascend in a lane: the last one wins
            }
        }
        if (nf) atomicOr(bad, 1u);
        __syncthreads();
        for (int c = 0; c < 3; ++c) { red[c][t] = lo[c]; red[3 + c][t] = hi[c]; red[6 + c][t] = zr[c]; }
        __syncthreads();
        for (int w = kBlock / 2; w > 0; w >>= 1) {
            if (t < (uint32_t)w)
                for (int c = 0; c < 3; ++c) {
                    red[c][t] = min(red[c][t], red[c][t + w]);
                    red[3 + c][t] = max(red[3 + c][t], red[3 + c][t + w]);
                    red[6 + c][t] = max(red[6 + c][t], red[6 + c][t + w]);
                }
            __syncthreads();
        }
        if (t < 3 && red[t][0] != ~0ull) atomicMin(&keys[6 * (uint64_t)s + t], red[t][0]);
        else if (t >= 3 && t < 6 && red[t - 3][0] != ~0ull) atomicMax(&keys[6 * (uint64_t)s + t], red[t][0]);
        else if (zrow && t >= 6 && t < 9 && red[t][0]) atomicMax(&zrow[3 * (uint64_t)s + t - 6], red[t][0]);
    }
}

// one lane per object: its grid (the preprocess rule, capped at max(m, 1) cells); an object of fewer than k rows gets
// one cell (no walk reads it)
__global__ __launch_bounds__(kBlock) void ob_grid_kernel(const unsigned long long* __restrict__ keys,
                                                        const uint64_t* __restrict__ off, uint32_t S, int k,
                                                        double cell_size, Grid* __restrict__ grids) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const uint64_t m = off[s + 1] - off[s];
    Grid g;
    g.h = 1.0;
    g.inv_h = 1.0;
    for (int c = 0; c < 3; ++c) { g.lo[c] = 0.0; g.n[c] = 1; }
    if (m >= (uint64_t)k) {
        double ext[3], emax = 0.0;
        for (int c = 0; c < 3; ++c) {
            g.lo[c] = ord_val(keys[6 * (uint64_t)s + c]);
            ext[c] = ord_val(keys[6 * (uint64_t)s + 3 + c]) - g.lo[c];
            emax = fmax(emax, ext[c]);
        }
        double h = cell_size;
        if (!(h > 0.0)) {
            // annotated objects are surfaces: about k rows per cell of a sheet spanning the largest face of the box
            const double area = fmax(fmax(ext[0] * ext[1], ext[1] * ext[2]), ext[0] * ext[2]);
            if (area > 0.0) h = sqrt(area * (double)k / (double)m);
            else if (emax > 0.0) h = emax * (double)k / (double)m;
            else h = 1.0;
        }
        h = fmax(h, emax / 1024.0);                             // at most 1024 cells per axis
        if (!(h > 0.0)) h = 1.0;
        for (;;) {
            double cd = 1.0;
            for (int c = 0; c < 3; ++c) {
                g.n[c] = max(1, (int)floor(ext[c] / h) + 1);
                cd *= (double)g.n[c];
            }
            if (cd <= (double)m) break;
            h *= 1.26;
        }
        g.h = h;
        g.inv_h = 1.0 / h;
    }
    grids[s] = g;
}

// per row: its object and its global cell key base[s] + local cell
__global__ __launch_bounds__(kBlock) void ob_key_kernel(const double* __restrict__ p, uint64_t n,
                                                       const uint64_t* __restrict__ off, uint32_t S,
                                                       const Grid* __restrict__ grids, const uint32_t* __restrict__ base,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                       uint32_t* __restrict__ seg) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = object_of(off, S, i);
    const Grid g = grids[s];
    const int cx = cell_of(p[3 * i], g.lo[0], g.inv_h, g.n[0]);
    const int cy = cell_of(p[3 * i + 1], g.lo[1], g.inv_h, g.n[1]);
    const int cz = cell_of(p[3 * i + 2], g.lo[2], g.inv_h, g.n[2]);
    keys[i] = base[s] + ((uint32_t)cz * (uint32_t)g.n[1] + (uint32_t)cy) * (uint32_t)g.n[0] + (uint32_t)cx;
    vals[i] = (uint32_t)i;
    seg[i] = s;
}

// cell populations and the rows in cell order, each with its object in pad
__global__ __launch_bounds__(kBlock) void ob_gather_kernel(const double* __restrict__ p, const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals,
                                                          const uint32_t* __restrict__ seg, uint64_t n,
                                                          uint32_t* __restrict__ counts, SPt* __restrict__ pts) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    atomicAdd(&counts[keys[j]], 1u);
    const uint32_t v = vals[j];
    SPt s;
    s.x = p[3 * (uint64_t)v];
    s.y = p[3 * (uint64_t)v + 1];
    s.z = p[3 * (uint64_t)v + 2];
    s.idx = v;
    s.pad = seg[v];
    pts[j] = s;
}

// one lane per row in cell order.  The lanes of a wavefront take their objects one at a time (the first active lane's
// object, then the next), so the object's grid and cell table are wave-uniform.
template <int KC>
__global__ __launch_bounds__(kBlock) void ob_knn_kernel(const SPt* __restrict__ pts, uint64_t n,
                                                       const uint64_t* __restrict__ off, const Grid* __restrict__ grids,
                                                       const uint32_t* __restrict__ base, const uint32_t* __restrict__ start,
                                                       int k, double* __restrict__ avg) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const SPt q = pts[i];
    for (;;) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(q.pad);
        if (q.pad != s) continue;
        if (off[s + 1] - off[s] < (uint64_t)k) {
            avg[q.idx] = -1.0;
        } else {
            const Grid g = grids[s];
            avg[q.idx] = knn_avg<KC>(pts, g, start + base[s], q.x, q.y, q.z, k, k);
        }
        break;
    }
}

// (chunk, object) workgroups over the objects of k rows or more: pp_sum_kernel's chunk b of a cloud of m rows, into
// part[256 s + b]; stats == nullptr: sum_{avg>0} avg, otherwise sum_{avg>0} (avg - stats[2 s])^2
__global__ __launch_bounds__(kBlock) void ob_sum_kernel(const double* __restrict__ avg, const uint64_t* __restrict__ off,
                                                       uint32_t S, int k, const double* __restrict__ stats,
                                                       double* __restrict__ part) {
    __shared__ double red[kBlock];
    for (uint32_t s = blockIdx.y; s < S; s += gridDim.y) {
        const uint64_t a0 = off[s], m = off[s + 1] - a0;
        if (m < (uint64_t)k) continue;
        const uint64_t chunk = (m + kRedBlocks - 1) / kRedBlocks;
        double* out = part + (uint64_t)kRedBlocks * s + blockIdx.x;
        if ((uint64_t)blockIdx.x * chunk >= m) {                     // an empty chunk sums to +0
            if (threadIdx.x == 0) *out = 0.0;
            continue;
        }
        const uint64_t a = a0 + (uint64_t)blockIdx.x * chunk, e = min(a + chunk, a0 + m);
        const double acc = chunk_partial(avg, a, e, stats ? stats + 2 * (uint64_t)s : nullptr);
        const double v = block_sum(acc, red);
        if (threadIdx.x == 0) *out = v;
    }
}

// one workgroup per object of k rows or more: pp_final_kernel's fold of its chunks; phase 0 -> stats[2 s] = mean,
// phase 1 -> stats[2 s + 1] = mean + std_ratio * std
__global__ __launch_bounds__(kRedBlocks) void ob_final_kernel(const double* __restrict__ part,
                                                             const uint64_t* __restrict__ off, uint32_t S, int k,
                                                             int phase, double std_ratio, double* __restrict__ stats) {
    __shared__ double red[kBlock];
    for (uint32_t s = blockIdx.x; s < S; s += gridDim.x) {
        const uint64_t m = off[s + 1] - off[s];
        if (m < (uint64_t)k) continue;
        const double v = block_sum(part[(uint64_t)kRedBlocks * s + threadIdx.x], red);
        if (threadIdx.x != 0) continue;
        if (phase == 0) stats[2 * (uint64_t)s] = v / (double)m;
        else stats[2 * (uint64_t)s + 1] = stats[2 * (uint64_t)s] + std_ratio * sqrt(v / (double)(m - 1));
    }
}

__global__ __launch_bounds__(kBlock) void ob_keep_kernel(const double* __restrict__ avg, const uint32_t* __restrict__ seg,
                                                        const uint64_t* __restrict__ off, uint64_t n, int k,
                                                        const double* __restrict__ stats, uint32_t* __restrict__ flag,
                                                        uint8_t* __restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = seg[i];
    const double v = avg[i];
    const uint32_t f = off[s + 1] - off[s] < (uint64_t)k ? 1u : ((v > 0.0 && v < stats[2 * (uint64_t)s + 1]) ? 1u : 0u);
    flag[i] = f;
    if (keep) keep[i] = (uint8_t)f;
}

__global__ __launch_bounds__(kBlock) void ob_compact_kernel(uint64_t n, const uint32_t* __restrict__ flag,
                                                           const uint32_t* __restrict__ pos, uint32_t* __restrict__ kept) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !flag[i]) return;
    kept[pos[i]] = (uint32_t)i;
}

// one lane per object: its lrc_objbox
__global__ __launch_bounds__(kBlock) void ob_box_kernel(const double* __restrict__ p, const uint64_t* __restrict__ off,
                                                       uint32_t S, int k,
                                                       const unsigned long long* __restrict__ zrow,
                                                       const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                       const unsigned long long* __restrict__ kkeys,
                                                       const double* __restrict__ stats, lrc_objbox* __restrict__ boxes) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const uint64_t a = off[s], m = off[s + 1] - a;
    lrc_objbox b;
    b.num_points = m;
    b.num_kept = m ? (uint64_t)pos[a + m - 1] + flag[a + m - 1] - pos[a] : 0;
    b.filtered = m >= (uint64_t)k ? 1u : 0u;
    b.reserved_ = 0;
    for (int c = 0; c < 3; ++c) {
        b.min3[c] = b.num_kept ? ord_val(kkeys[6 * (uint64_t)s + c]) : INFINITY;
        b.max3[c] = b.num_kept ? ord_val(kkeys[6 * (uint64_t)s + 3 + c]) : -INFINITY;
        const unsigned long long z = zrow[3 * (uint64_t)s + c];
        if (z && b.min3[c] == 0.0) b.min3[c] = p[3 * (z - 1) + c];
        if (z && b.max3[c] == 0.0) b.max3[c] = p[3 * (z - 1) + c];
    }
    b.mean = b.filtered ? stats[2 * (uint64_t)s] : 0.0;
    b.threshold = b.filtered ? stats[2 * (uint64_t)s + 1] : INFINITY;
    boxes[s] = b;
}

template <int KC>
hipError_t launch_knn(uint64_t n, hipStream_t st, const SPt* pts, const uint64_t* off, const Grid* grids,
                      const uint32_t* base, const uint32_t* start, int k, double* avg) {
    hipLaunchKernelGGL(ob_knn_kernel<KC>, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, pts, n, off,
                       grids, base, start, k, avg);
    return hipGetLastError();
}

hipError_t dispatch_knn(uint64_t n, hipStream_t st, const SPt* pts, const uint64_t* off, const Grid* grids,
                        const uint32_t* base, const uint32_t* start, int k, double* avg) {
    if (k <= 1) return launch_knn<1>(n, st, pts, off, grids, base, start, k, avg);
    if (k <= 2) return launch_knn<2>(n, st, pts, off, grids, base, start, k, avg);
    if (k <= 4) return launch_knn<4>(n, st, pts, off, grids, base, start, k, avg);
    if (k <= 8) return launch_knn<8>(n, st, pts, off, grids, base, start, k, avg);
    if (k <= 16) return launch_knn<16>(n, st, pts, off, grids, base, start, k, avg);
    if (k <= 20) return launch_knn<20>(n, st, pts, off, grids, base, start, k, avg);
    if (k <= 24) return launch_knn<24>(n, st, pts, off, grids, base, start, k, avg);
    return launch_knn<32>(n, st, pts, off, grids, base, start, k, avg);
}

// host checks, before any launch: offsets from 0 to n without a step back, n and the object count below 2^31,
// 1 <= k <= 32, a finite std_ratio > 0
int check_args(const char* fn, uint64_t n, const uint64_t* offsets, uint64_t S, uint32_t k, double std_ratio) {
    const std::string f(fn);
    if (n >= (1ull << 31) || S >= (1ull << 31))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, (f + ": need n < 2^31 and num_objects < 2^31").c_str());
    if (k < 1 || k > 32) return lrc_internal_fail(LRC_ERR_INVALID_ARG, (f + ": need 1 <= k <= 32").c_str());
    if (!finite_positive(std_ratio))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, (f + ": need a finite std_ratio > 0").c_str());
    if (offsets[0] != 0 || offsets[S] != n)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, (f + ": need offsets[0] == 0 and offsets[num_objects] == n").c_str());
    for (uint64_t s = 0; s < S; ++s)
        if (offsets[s + 1] < offsets[s])
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, (f + ": offsets must not decrease").c_str());
    return LRC_OK;
}

}  // namespace

extern "C" {

int lrc_object_boxes_dev(lrc_ctx* ctx, const double* d_points3, uint64_t n, const uint64_t* offsets, uint64_t num_objects,
                         uint32_t k, double std_ratio, double cell_size, lrc_objbox* out_boxes, uint32_t* d_out_kept,
                         double* d_out_avg, uint8_t* d_out_keep, void* stream) {
    if (!ctx || !offsets || (n && !d_points3) || (num_objects && !out_boxes))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_object_boxes_dev: NULL argument");
    if (int rc = check_args("lrc_object_boxes_dev", n, offsets, num_objects, k, std_ratio)) return rc;
    const uint32_t S = (uint32_t)num_objects;
    if (S == 0) return LRC_OK;
    LRC_HIP(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    Arena arena(st);

    // cell ranges: max(m, 1) cells for an object of k rows or more, one for a smaller non-empty one (total <= n)
    std::vector<uint32_t> h_base(S + 1);
    uint64_t cells = 0;
    for (uint32_t s = 0; s < S; ++s) {
        h_base[s] = (uint32_t)cells;
        const uint64_t m = offsets[s + 1] - offsets[s];
        cells += m >= k ? m : (m ? 1 : 0);
    }
    h_base[S] = (uint32_t)cells;

    // per object: offsets, cell bases, bound keys (all rows, kept rows), grid, statistics, box; the chunk partials
    uint64_t* off;
    uint32_t *base, *bad;
    unsigned long long *keys, *kkeys, *zrow;
    Grid* grids;
    double *stats, *part;
    lrc_objbox* boxes;
    {
        const size_t o_base = align256((S + 1) * 8), o_keys = o_base + align256((S + 1) * 4),
                     o_kkeys = o_keys + align256((size_t)S * 48), o_zrow = o_kkeys + align256((size_t)S * 48),
                     o_grid = o_zrow + align256((size_t)S * 24),
                     o_stats = o_grid + align256((size_t)S * sizeof(Grid)), o_box = o_stats + align256((size_t)S * 16),
                     o_bad = o_box + align256((size_t)S * sizeof(lrc_objbox)), o_part = o_bad + 256,
                     total = o_part + align256((size_t)S * kRedBlocks * 8);
        void* q;
        LRC_HIP(arena.get(total, &q));
        char* c = (char*)q;
        off = (uint64_t*)c; base = (uint32_t*)(c + o_base); keys = (unsigned long long*)(c + o_keys);
        kkeys = (unsigned long long*)(c + o_kkeys); zrow = (unsigned long long*)(c + o_zrow); grids = (Grid*)(c + o_grid); stats = (double*)(c + o_stats);
        boxes = (lrc_objbox*)(c + o_box); bad = (uint32_t*)(c + o_bad); part = (double*)(c + o_part);
    }
    LRC_HIP(hipMemcpyAsync(off, offsets, (S + 1) * 8, hipMemcpyHostToDevice, st));
    LRC_HIP(hipMemcpyAsync(base, h_base.data(), (S + 1) * 4, hipMemcpyHostToDevice, st));
    // lo keys start at all ones, hi keys at zero: 6 words per object, three of each
    {
        std::vector<unsigned long long> init((size_t)S * 6);
        for (size_t j = 0; j < init.size(); ++j) init[j] = (j % 6) < 3 ? ~0ull : 0ull;
        LRC_HIP(hipMemcpyAsync(keys, init.data(), init.size() * 8, hipMemcpyHostToDevice, st));
        LRC_HIP(hipMemcpyAsync(kkeys, init.data(), init.size() * 8, hipMemcpyHostToDevice, st));
        LRC_HIP(hipMemsetAsync(zrow, 0, (size_t)S * 24, st));
        LRC_HIP(hipMemsetAsync(bad, 0, 4, st));
        const dim3 og(kRedBlocks, std::min(S, kMaxRowsY));
        if (n) hipLaunchKernelGGL(ob_bounds_kernel, og, dim3(kBlock), 0, st, d_points3, (const uint64_t*)off, S,
                                  (const uint32_t*)nullptr, keys, bad, (unsigned long long*)nullptr);
        LRC_HIP(hipGetLastError());
        uint32_t h_bad = 0;
        LRC_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st));
        LRC_HIP(hipStreamSynchronize(st));          // `init` stays alive until the copies above have run
        if (h_bad) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_object_boxes: non-finite coordinate");
    }
    const uint32_t sblk = (S + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ob_grid_kernel, dim3(sblk), dim3(kBlock), 0, st, (const unsigned long long*)keys,
                       (const uint64_t*)off, S, (int)k, cell_size, grids);
    LRC_HIP(hipGetLastError());

    if (n) {
        const uint32_t nblk = (uint32_t)((n + kBlock - 1) / kBlock);
        uint32_t *keys_a, *keys_b, *vals_a, *vals_b, *seg, *counts, *start, *flag, *pos;
        SPt* pts;
        double* avg;
        {
            const size_t sz = align256(n * 4), o_cnt = 7 * sz, o_start = o_cnt + align256((cells + 1) * 4),
                         o_pts = o_start + align256((cells + 1) * 4), o_avg = o_pts + align256(n * sizeof(SPt)),
                         total = o_avg + (d_out_avg ? 0 : align256(n * 8));
            void* q;
            LRC_HIP(arena.get(total, &q));
            char* c = (char*)q;
            keys_a = (uint32_t*)c; keys_b = (uint32_t*)(c + sz); vals_a = (uint32_t*)(c + 2 * sz);
            vals_b = (uint32_t*)(c + 3 * sz); seg = (uint32_t*)(c + 4 * sz); flag = (uint32_t*)(c + 5 * sz);
            pos = (uint32_t*)(c + 6 * sz); counts = (uint32_t*)(c + o_cnt); start = (uint32_t*)(c + o_start);
            pts = (SPt*)(c + o_pts);
            avg = d_out_avg ? d_out_avg : (double*)(c + o_avg);
        }
        hipLaunchKernelGGL(ob_key_kernel, dim3(nblk), dim3(kBlock), 0, st, d_points3, n, (const uint64_t*)off, S,
                           (const Grid*)grids, (const uint32_t*)base, keys_a, vals_a, seg);
        LRC_HIP(hipGetLastError());
        LRC_HIP(hipMemsetAsync(counts, 0, (cells + 1) * 4, st));
        const int end_bit = std::max(1, bit_width(cells));
        size_t tmp_sort = 0, tmp_scan = 0, tmp_flag = 0;
        LRC_HIP(rocprim::radix_sort_pairs(nullptr, tmp_sort, keys_a, keys_b, vals_a, vals_b, (size_t)n, 0, end_bit, st));
        LRC_HIP(rocprim::exclusive_scan(nullptr, tmp_scan, counts, start, 0u, (size_t)(cells + 1),
                                          rocprim::plus<uint32_t>(), st));
        LRC_HIP(rocprim::exclusive_scan(nullptr, tmp_flag, flag, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
        void* tmp;
        LRC_HIP(arena.get(std::max(tmp_sort, std::max(tmp_scan, tmp_flag)), &tmp));
        LRC_HIP(rocprim::radix_sort_pairs(tmp, tmp_sort, keys_a, keys_b, vals_a, vals_b, (size_t)n, 0, end_bit, st));
        hipLaunchKernelGGL(ob_gather_kernel, dim3(nblk), dim3(kBlock), 0, st, d_points3, keys_b, vals_b,
                           (const uint32_t*)seg, n, counts, pts);
        LRC_HIP(hipGetLastError());
        LRC_HIP(rocprim::exclusive_scan(tmp, tmp_scan, counts, start, 0u, (size_t)(cells + 1),
                                          rocprim::plus<uint32_t>(), st));

        LRC_HIP(dispatch_knn(n, st, pts, off, grids, base, start, (int)k, avg));
        const dim3 og(kRedBlocks, std::min(S, kMaxRowsY));
        const dim3 fg(std::min(S, kMaxRowsY));
        hipLaunchKernelGGL(ob_sum_kernel, og, dim3(kBlock), 0, st, (const double*)avg, (const uint64_t*)off, S, (int)k,
                           (const double*)nullptr, part);
        hipLaunchKernelGGL(ob_final_kernel, fg, dim3(kRedBlocks), 0, st, (const double*)part, (const uint64_t*)off, S,
                           (int)k, 0, std_ratio, stats);
        hipLaunchKernelGGL(ob_sum_kernel, og, dim3(kBlock), 0, st, (const double*)avg, (const uint64_t*)off, S, (int)k,
                           (const double*)stats, part);
        hipLaunchKernelGGL(ob_final_kernel, fg, dim3(kRedBlocks), 0, st, (const double*)part, (const uint64_t*)off, S,
                           (int)k, 1, std_ratio, stats);
        hipLaunchKernelGGL(ob_keep_kernel, dim3(nblk), dim3(kBlock), 0, st, (const double*)avg, (const uint32_t*)seg,
                           (const uint64_t*)off, n, (int)k, (const double*)stats, flag, d_out_keep);
        LRC_HIP(hipGetLastError());
        LRC_HIP(rocprim::exclusive_scan(tmp, tmp_flag, flag, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
        if (d_out_kept)
            hipLaunchKernelGGL(ob_compact_kernel, dim3(nblk), dim3(kBlock), 0, st, n, (const uint32_t*)flag,
                               (const uint32_t*)pos, d_out_kept);
        hipLaunchKernelGGL(ob_bounds_kernel, og, dim3(kBlock), 0, st, d_points3, (const uint64_t*)off, S,
                           (const uint32_t*)flag, kkeys, bad, zrow);
        hipLaunchKernelGGL(ob_box_kernel, dim3(sblk), dim3(kBlock), 0, st, d_points3, (const uint64_t*)off, S, (int)k,
                           (const unsigned long long*)zrow,
                           (const uint32_t*)flag, (const uint32_t*)pos, (const unsigned long long*)kkeys,
                           (const double*)stats, boxes);
        LRC_HIP(hipGetLastError());
    } else {
        // every object is empty: the box kernel reads no row
        hipLaunchKernelGGL(ob_box_kernel, dim3(sblk), dim3(kBlock), 0, st, d_points3, (const uint64_t*)off, S, (int)k,
                           (const unsigned long long*)zrow, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const unsigned long long*)kkeys,
                           (const double*)stats, boxes);
        LRC_HIP(hipGetLastError());
    }
    LRC_HIP(hipMemcpyAsync(out_boxes, boxes, (size_t)S * sizeof(lrc_objbox), hipMemcpyDeviceToHost, st));
    LRC_HIP(hipStreamSynchronize(st));
    return LRC_OK;
}

int lrc_object_boxes(lrc_ctx* ctx, const double* points3, uint64_t n, const uint64_t* offsets, uint64_t num_objects,
                     uint32_t k, double std_ratio, double cell_size, lrc_objbox* out_boxes, uint32_t* out_kept,
                     double* out_avg, uint8_t* out_keep) {
    if (!ctx || !offsets || (n && !points3) || (num_objects && !out_boxes))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_object_boxes: NULL argument");
    if (int rc = check_args("lrc_object_boxes", n, offsets, num_objects, k, std_ratio)) return rc;
    if (num_objects == 0) return LRC_OK;
    LRC_HIP(hipSetDevice(ctx->device));
    double *d_p = nullptr, *d_avg = nullptr;
    uint32_t* d_kept = nullptr;
    uint8_t* d_keep = nullptr;
    int rc = LRC_OK;
    if (n && (hipMalloc((void**)&d_p, n * 24) != hipSuccess || (out_kept && hipMalloc((void**)&d_kept, n * 4) != hipSuccess) ||
              (out_avg && hipMalloc((void**)&d_avg, n * 8) != hipSuccess) ||
              (out_keep && hipMalloc((void**)&d_keep, n) != hipSuccess))) {
        rc = lrc_internal_fail(LRC_ERR_OOM, "lrc_object_boxes: out of device memory");
    } else if (n && hipMemcpy(d_p, points3, n * 24, hipMemcpyHostToDevice) != hipSuccess) {
        rc = lrc_internal_fail(LRC_ERR_HIP, "lrc_object_boxes: upload failed");
    } else if ((rc = lrc_object_boxes_dev(ctx, d_p, n, offsets, num_objects, k, std_ratio, cell_size, out_boxes, d_kept,
                                          d_avg, d_keep, nullptr)) == LRC_OK && n) {
        uint64_t kept = 0;
        for (uint64_t s = 0; s < num_objects; ++s) kept += out_boxes[s].num_kept;
        if ((out_kept && kept && hipMemcpy(out_kept, d_kept, kept * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
            (out_avg && hipMemcpy(out_avg, d_avg, n * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
            (out_keep && hipMemcpy(out_keep, d_keep, n, hipMemcpyDeviceToHost) != hipSuccess))
            rc = lrc_internal_fail(LRC_ERR_HIP, "lrc_object_boxes: download failed");
    }
    if (d_p) (void)hipFree(d_p);
    if (d_kept) (void)hipFree(d_kept);
    if (d_avg) (void)hipFree(d_avg);
    if (d_keep) (void)hipFree(d_keep);
    return rc;
}

}  // extern "C"
