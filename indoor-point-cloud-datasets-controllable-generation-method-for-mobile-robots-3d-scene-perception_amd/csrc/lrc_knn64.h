// lrc_knn64.h -- float64 cell grids, the exact k-nearest walk over expanding cube shells and the fixed-order reduction
// pieces shared by lrc_preprocess.hip (one cloud per call) and lrc_objboxes.hip (many objects per call).
//
// Both files compute Open3D's remove_statistical_outlier on float64 rows with the same arithmetic, so that an object
// filtered by lrc_object_boxes gives the bytes lrc_cloud_preprocess gives for that object alone:
//   avg  = (sum of the square roots of the `found` smallest squared distances (dx*dx + dy*dy) + dz*dz, ascending, one
//          after the other) / found;
//   sums = kRedBlocks contiguous chunks of ceil(n / kRedBlocks) rows in row order, lanes strided by kBlock inside a
//          chunk, block_sum's tree over the lanes, block_sum's tree over the chunks.
// Everything here lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "lrc_internal.h"

namespace {

constexpr int kRedBlocks = 256;        // chunks of the fixed-order reductions (bounds, mean, std)

struct Grid {
    double lo[3];
    double h, inv_h;
    int n[3];
};

// a row in cell order: coordinates and its index in the set the grid was built over (pad: free for the caller)
struct alignas(16) SPt {
    double x, y, z;
    uint32_t idx, pad;
};

__device__ __forceinline__ int cell_of(double x, double lo, double inv_h, int n) {
    const double f = floor((x - lo) * inv_h);
    return f < 0.0 ? 0 : (f >= (double)n ? n - 1 : (int)f);
}

// exponent bits all ones: inf or nan.  The test runs on the integer bits as loaded, never on a double: the device code
// is built with -fno-honor-nans, and a class test on a double value may be folded to "never nan".
__device__ __forceinline__ bool non_finite_bits(uint64_t b) { return (b << 1) >= (0xFFEull << 52); }

__device__ __forceinline__ double sq3(double qx, double qy, double qz, double px, double py, double pz) {
    const double dx = qx - px, dy = qy - py, dz = qz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

// rows m of the cells on the surface of the cube of cells [c-r, c+r]^3, clipped to the grid; the statement that follows
// is the body.  On a z- or y-face of the shell the whole x-run belongs to it; otherwise only its two ends.  (A macro,
// not a function taking a lambda: a list captured by reference would be kept in scratch.)
#define PP_SHELL_CELL(x, y, z) (((uint32_t)(z) * (uint32_t)g.n[1] + (uint32_t)(y)) * (uint32_t)g.n[0] + (uint32_t)(x))
#define PP_FOR_SHELL_ROWS(m)                                                                                        \
    for (int z = max(cz - r, 0), z1_ = min(cz + r, g.n[2] - 1); z <= z1_; ++z)                                      \
        for (int y = max(cy - r, 0), y1_ = min(cy + r, g.n[1] - 1); y <= y1_; ++y)                                  \
            for (int x = cx - r, step_ = ((z == cz - r) | (z == cz + r) | (y == cy - r) | (y == cy + r)) ? 1 : max(2 * r, 1); \
                 x <= cx + r; x += step_)                                                                           \
                if (x >= 0 && x < g.n[0])                                                                           \
                    for (uint32_t m = start[PP_SHELL_CELL(x, y, z)], e_ = start[PP_SHELL_CELL(x, y, z) + 1]; m < e_; ++m)

// everything inside the cube of cells [c-r, c+r]^3 has been searched: a row outside it lies farther from q than this
// (the distance to the nearest face, shrunk by 1e-6 cell: a row binned by floor((p-lo)/h) may sit one rounding below
// its cell's edge)
__device__ __forceinline__ double cube_margin(const Grid& g, double qx, double qy, double qz, int cx, int cy, int cz, int r) {
    const double mx = fmin(qx - (g.lo[0] + (double)(cx - r) * g.h), (g.lo[0] + (double)(cx + r + 1) * g.h) - qx);
    const double my = fmin(qy - (g.lo[1] + (double)(cy - r) * g.h), (g.lo[1] + (double)(cy + r + 1) * g.h) - qy);
    const double mz = fmin(qz - (g.lo[2] + (double)(cz - r) * g.h), (g.lo[2] + (double)(cz + r + 1) * g.h) - qz);
    return fmin(mx, fmin(my, mz)) - 1.0e-6 * g.h;
}

// insert v into the ascending list best[0..KC): compile-time indices only
template <int KC, class T>
__device__ __forceinline__ void insert_sorted(T (&best)[KC], T v) {
    if (!(v < best[KC - 1])) return;
#pragma unroll
    for (int j = KC - 1; j > 0; --j) {
        const T prev = best[j - 1];
        best[j] = v < prev ? prev : (v < best[j] ? v : best[j]);
    }
    best[0] = v < best[0] ? v : best[0];
}

// avg of the row q of a grid over pts / start: the k smallest squared distances to the grid's rows, itself included,
// found by expanding cube shells until the k-th cannot be beaten; the first `found` of them (found = min(k, rows))
// are square-rooted and summed in ascending order
template <int KC>
__device__ __forceinline__ double knn_avg(const SPt* __restrict__ pts, const Grid& g, const uint32_t* __restrict__ start,
                                          double qx, double qy, double qz, int k, int found) {
    const int cx = cell_of(qx, g.lo[0], g.inv_h, g.n[0]);
    const int cy = cell_of(qy, g.lo[1], g.inv_h, g.n[1]);
    const int cz = cell_of(qz, g.lo[2], g.inv_h, g.n[2]);
    // the k-best list is right-aligned in best[KC-k, KC): the slots below hold -inf and never move, so the k-th
    // smallest is best[KC-1] and every index stays a compile-time constant (a run-time index would put the list in
    // scratch)
    double best[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) best[j] = j < KC - k ? -INFINITY : INFINITY;
    const int rmax = max(max(max(cx, g.n[0] - 1 - cx), max(cy, g.n[1] - 1 - cy)), max(cz, g.n[2] - 1 - cz));
    for (int r = 0; r <= rmax; ++r) {
        PP_FOR_SHELL_ROWS(m) {
            const SPt p = pts[m];
            insert_sorted<KC>(best, sq3(qx, qy, qz, p.x, p.y, p.z));
        }
        const double kth = best[KC - 1];
        if (kth < INFINITY) {
            const double margin = cube_margin(g, qx, qy, qz, cx, cy, cz, r);
            if (margin > 0.0 && kth <= margin * margin) break;
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < KC; ++j)
        if (j >= KC - k && j < KC - k + found) sum += sqrt(best[j]);
    return sum / (double)found;
}

__device__ double block_sum(double v, double* red) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (t < (uint32_t)w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}

// this lane's share of one reduction chunk, rows [a, e) strided by kBlock: sum_{avg>0} avg (stats == nullptr) or
// sum_{avg>0} (avg - stats[0])^2
__device__ __forceinline__ double chunk_partial(const double* __restrict__ avg, uint64_t a, uint64_t e,
                                                const double* __restrict__ stats) {
    const double mean = stats ? stats[0] : 0.0;
    double acc = 0.0;
    for (uint64_t j = a + threadIdx.x; j < e; j += kBlock) {
        const double v = avg[j];
        if (v > 0.0) {
            if (stats) { const double d = v - mean; acc += d * d; }
            else acc += v;
        }
    }
    return acc;
}

int bit_width(uint64_t v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// stream-ordered workspace: one block per phase, freed on every exit path
struct Arena {
    hipStream_t st;
    std::vector<void*> blocks;
    explicit Arena(hipStream_t s) : st(s) {}
    ~Arena() {
        for (void* p : blocks) (void)hipFreeAsync(p, st);
    }
    hipError_t get(size_t bytes, void** out) {
        *out = nullptr;
        hipError_t e = hipMallocAsync(out, bytes ? bytes : 256, st);
        if (e == hipSuccess) blocks.push_back(*out);
        return e;
    }
};

bool finite_positive(double v) { return v > 0.0 && v < INFINITY; }

}  // namespace
