// lrc_preprocess.hip -- room preprocessing of a float64 cloud: statistical outlier filter and PCA normals (gfx950).
//
// The reference's first stage (s3dis_data_loader.py, S3DISPreprocessor.preprocess_pointcloud :85-158) runs Open3D's
// remove_statistical_outlier(nb_neighbors, std_ratio) over the whole room and then estimate_normals with
// KDTreeSearchParamHybrid(radius, max_nn) on what is left.  One call here does both:
//   1. grid: float64 bounds of the cloud (non-finite coordinates are rejected), a cell size of about max(k, max_nn)
//      rows per cell of a sheet spanning the largest face of the box, a stable radix sort of the rows by cell and a
//      table of cell starts;
//   2. outliers: one lane per row finds the k smallest float64 squared distances (dx*dx + dy*dy) + dz*dz, itself
//      included, over expanding cube shells until the k-th cannot be beaten (lrc_nn.hip's exactness argument);
//      avg = (sum of the min(k, n) square roots, ascending, one after the other) / min(k, n).  mean = sum_{avg>0} avg / n
//      and std = sqrt(sum_{avg>0} (avg-mean)^2 / (n-1)) are reduced in an order fixed by n alone (kRedBlocks contiguous
//      chunks in row order, lanes strided inside a chunk, a fixed tree over lanes and chunks); a row is kept iff
//      avg > 0 && avg < mean + std_ratio * std; the kept rows are compacted in ascending row order (Open3D's `ind`);
//   3. normals on the kept rows, on a grid of their own: the neighbours of a row are the rows with d2 < radius^2, itself
//      included, ordered by (d2, index), the first max_nn of them.  Walk A keeps only distances and yields the cut-off
//      D (the count-th smallest d2); walk B, over the same shells, keeps the indices of the rows with d2 < D and the
//      lowest-index rows with d2 == D (one uint32 key per neighbour); the d2 < D part is then stably sorted by d2.  The
//      nine cumulants are accumulated in that order, cov = E[xx^T] - E[x]E[x]^T, and the unit eigenvector of the
//      smallest eigenvalue comes from the closed-form robust symmetric 3x3 solver (Eberly), as Open3D's default
//      fast_normal_computation path computes it.  Fewer than 3 neighbours, or a zero covariance, give (0, 0, 1).
// Every list lives in registers: one instantiation per list length, compile-time indices only (no scratch).  Results
// depend on distances and indices only, never on the grid, so the bytes do not change with the cell size.
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

constexpr uint32_t kTie = 0x80000000u; // walk B key bit: d2 == D (indices are < 2^31)

// per-block float64 bounds and a non-finite flag; the host folds the blocks (min / max: order-free)
__global__ __launch_bounds__(kBlock) void pp_bounds_kernel(const double* __restrict__ p, uint64_t n,
                                                          double* __restrict__ part, uint32_t* __restrict__ bad) {
    __shared__ double red[6][kBlock];
    const uint32_t t = threadIdx.x;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nf = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + t; i < n; i += (uint64_t)gridDim.x * kBlock)
        for (int c = 0; c < 3; ++c) {
            const uint64_t b = reinterpret_cast<const uint64_t*>(p)[3 * i + c];
            if (non_finite_bits(b)) { nf = 1; continue; }
            const double v = __longlong_as_double((long long)b);
            lo[c] = fmin(lo[c], v);
            hi[c] = fmax(hi[c], v);
        }
    if (nf) atomicOr(bad, 1u);
    for (int c = 0; c < 3; ++c) { red[c][t] = lo[c]; red[3 + c][t] = hi[c]; }
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (t < (uint32_t)w)
            for (int c = 0; c < 3; ++c) {
                red[c][t] = fmin(red[c][t], red[c][t + w]);
                red[3 + c][t] = fmax(red[3 + c][t], red[3 + c][t + w]);
            }
        __syncthreads();
    }
    if (t < 6) part[6 * blockIdx.x + t] = red[t][0];
}

__global__ __launch_bounds__(kBlock) void pp_key_kernel(const double* __restrict__ p, uint64_t n, const Grid g,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int cx = cell_of(p[3 * i], g.lo[0], g.inv_h, g.n[0]);
    const int cy = cell_of(p[3 * i + 1], g.lo[1], g.inv_h, g.n[1]);
    const int cz = cell_of(p[3 * i + 2], g.lo[2], g.inv_h, g.n[2]);
    keys[i] = ((uint32_t)cz * (uint32_t)g.n[1] + (uint32_t)cy) * (uint32_t)g.n[0] + (uint32_t)cx;
    vals[i] = (uint32_t)i;
}

// cell populations (counts only: their values do not depend on the order of the atomics) and the rows in cell order
__global__ __launch_bounds__(kBlock) void pp_gather_kernel(const double* __restrict__ p, const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals, uint64_t n,
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
    s.pad = 0;
    pts[j] = s;
}

// ---- 2. outlier filter ----------------------------------------------------------------------------------------------

template <int KC>
__global__ __launch_bounds__(kBlock) void pp_knn_kernel(const SPt* __restrict__ pts, uint64_t n, const Grid g,
                                                       const uint32_t* __restrict__ start, int k, double* __restrict__ avg) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const SPt q = pts[i];
    const int found = (uint64_t)k < n ? k : (int)n;
    avg[q.idx] = knn_avg<KC>(pts, g, start, q.x, q.y, q.z, k, found);
}

// kRedBlocks blocks, chunk b = rows [b*ceil(n/kRedBlocks), ...) in row order: sum_{avg>0} avg (stats == nullptr) or
// sum_{avg>0} (avg - stats[0])^2
__global__ __launch_bounds__(kBlock) void pp_sum_kernel(const double* __restrict__ avg, uint64_t n,
                                                       const double* __restrict__ stats, double* __restrict__ part) {
    __shared__ double red[kBlock];
    const uint64_t chunk = (n + kRedBlocks - 1) / kRedBlocks;
    const uint64_t a = (uint64_t)blockIdx.x * chunk, e = min(a + chunk, n);
    const double acc = chunk_partial(avg, a, e, stats);
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one block: phase 0 -> stats[0] = mean; phase 1 -> stats[1] = mean + std_ratio * std
__global__ __launch_bounds__(kRedBlocks) void pp_final_kernel(const double* __restrict__ part, uint64_t n, int phase,
                                                             double std_ratio, double* __restrict__ stats) {
    __shared__ double red[kBlock];
    const double s = block_sum(part[threadIdx.x], red);
    if (threadIdx.x != 0) return;
    if (phase == 0) stats[0] = s / (double)n;
    else stats[1] = stats[0] + std_ratio * sqrt(s / (double)(n - 1));
}

__global__ __launch_bounds__(kBlock) void pp_keep_kernel(const double* __restrict__ avg, uint64_t n,
                                                        const double* __restrict__ stats, uint32_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double v = avg[i];
    flag[i] = (v > 0.0 && v < stats[1]) ? 1u : 0u;
}

// kept rows in ascending row order: their indices and coordinates (the normals' input)
__global__ __launch_bounds__(kBlock) void pp_compact_kernel(const double* __restrict__ p, uint64_t n,
                                                           const uint32_t* __restrict__ flag,
                                                           const uint32_t* __restrict__ pos, uint32_t* __restrict__ kept,
                                                           double* __restrict__ pk) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint32_t o = pos[i];
    kept[o] = (uint32_t)i;
    if (!pk) return;
    pk[3 * (uint64_t)o] = p[3 * i];
    pk[3 * (uint64_t)o + 1] = p[3 * i + 1];
    pk[3 * (uint64_t)o + 2] = p[3 * i + 2];
}

__global__ __launch_bounds__(kBlock) void pp_fill_kernel(uint64_t n, uint32_t* __restrict__ kept, double* __restrict__ avg) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (kept) kept[i] = (uint32_t)i;
    if (avg) avg[i] = -1.0;
}

// ---- 3. normals -----------------------------------------------------------------------------------------------------

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// eigenvector of the eigenvalue e0 of the symmetric A (a00 a01 a02 a11 a12 a22) that is far from the others: the
// longest cross product of two rows of A - e0 I
__device__ V3 eigvec0(const double (&a)[6], double e0) {
    const V3 r0 = {a[0] - e0, a[1], a[2]}, r1 = {a[1], a[3] - e0, a[4]}, r2 = {a[2], a[4], a[5] - e0};
    const V3 c01 = cross(r0, r1), c02 = cross(r0, r2), c12 = cross(r1, r2);
    const double d0 = dot(c01, c01), d1 = dot(c02, c02), d2 = dot(c12, c12);
    double dmax = d0;
    int imax = 0;
    if (d1 > dmax) { dmax = d1; imax = 1; }
    if (d2 > dmax) imax = 2;
    const V3 c = imax == 0 ? c01 : (imax == 1 ? c02 : c12);
    const double s = sqrt(imax == 0 ? d0 : (imax == 1 ? d1 : d2));
    return {c.x / s, c.y / s, c.z / s};
}

// eigenvector of e1 in the plane orthogonal to the unit v0 (a 2x2 problem in the basis U, V of that plane)
__device__ V3 eigvec1(const double (&a)[6], V3 v0, double e1) {
    V3 u;
    if (fabs(v0.x) > fabs(v0.y)) {
        const double il = 1.0 / sqrt(v0.x * v0.x + v0.z * v0.z);
        u = {-v0.z * il, 0.0, v0.x * il};
    } else {
        const double il = 1.0 / sqrt(v0.y * v0.y + v0.z * v0.z);
        u = {0.0, v0.z * il, -v0.y * il};
    }
    const V3 v = cross(v0, u);
    const V3 au = {a[0] * u.x + a[1] * u.y + a[2] * u.z, a[1] * u.x + a[3] * u.y + a[4] * u.z,
                   a[2] * u.x + a[4] * u.y + a[5] * u.z};
    const V3 av = {a[0] * v.x + a[1] * v.y + a[2] * v.z, a[1] * v.x + a[3] * v.y + a[4] * v.z,
                   a[2] * v.x + a[4] * v.y + a[5] * v.z};
    double m00 = u.x * au.x + u.y * au.y + u.z * au.z - e1;
    double m01 = u.x * av.x + u.y * av.y + u.z * av.z;
    double m11 = v.x * av.x + v.y * av.y + v.z * av.z - e1;
    const double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
    if (a00 >= a11) {
        if (fmax(a00, a01) > 0.0) {
            if (a00 >= a01) { m01 /= m00; m00 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m00; }
            else { m00 /= m01; m01 = 1.0 / sqrt(1.0 + m00 * m00); m00 *= m01; }
            return {m01 * u.x - m00 * v.x, m01 * u.y - m00 * v.y, m01 * u.z - m00 * v.z};
        }
        return u;
    }
    if (fmax(a11, a01) > 0.0) {
        if (a11 >= a01) { m01 /= m11; m11 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m11; }
        else { m11 /= m01; m01 = 1.0 / sqrt(1.0 + m11 * m11); m11 *= m01; }
        return {m11 * u.x - m01 * v.x, m11 * u.y - m01 * v.y, m11 * u.z - m01 * v.z};
    }
    return u;
}

// unit eigenvector of the smallest eigenvalue of the symmetric c (c00 c01 c02 c11 c12 c22); (0,0,0) for c == 0.
// Eberly, "A Robust Eigensolver for 3x3 Symmetric Matrices": scale by the largest coefficient, eigenvalues from the
// trigonometric form of the shifted, normalised matrix, the well-separated eigenvector first.
__device__ V3 smallest_eigvec(const double (&c)[6]) {
    double mc = c[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) mc = fmax(mc, c[j]);
    if (mc == 0.0) return {0.0, 0.0, 0.0};
    double a[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = c[j] / mc;
    const double norm = a[1] * a[1] + a[2] * a[2] + a[4] * a[4];
    if (!(norm > 0.0)) {
        if (a[0] < a[3] && a[0] < a[5]) return {1.0, 0.0, 0.0};
        if (a[3] < a[0] && a[3] < a[5]) return {0.0, 1.0, 0.0};
        if (a[0] < a[5]) return {1.0, 0.0, 0.0};          // a[0] == a[3]: the smallest twice, x of its plane
        return {0.0, 0.0, 1.0};
    }
    const double q = (a[0] + a[3] + a[5]) / 3.0;
    const double b00 = a[0] - q, b11 = a[3] - q, b22 = a[5] - q;
    const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2.0) / 6.0);
    const double c00 = b11 * b22 - a[4] * a[4];
    const double c01 = a[1] * b22 - a[4] * a[2];
    const double c02 = a[1] * a[4] - b11 * a[2];
    const double det = (b00 * c00 - a[1] * c01 + a[2] * c02) / (p * p * p);
    const double half_det = fmin(fmax(det * 0.5, -1.0), 1.0);
    const double angle = acos(half_det) / 3.0;
    const double two_thirds_pi = 2.09439510239319549;
    const double beta2 = cos(angle) * 2.0;
    const double beta0 = cos(angle + two_thirds_pi) * 2.0;
    const double beta1 = -(beta0 + beta2);
    const double e0 = q + p * beta0, e1 = q + p * beta1, e2 = q + p * beta2;
    if (half_det >= 0.0) {
        const V3 v2 = eigvec0(a, e2);
        if (e2 < e0 && e2 < e1) return v2;
        const V3 v1 = eigvec1(a, v2, e1);
        if (e1 < e0 && e1 < e2) return v1;
        return cross(v1, v2);
    }
    const V3 v0 = eigvec0(a, e0);
    if (e0 < e1 && e0 < e2) return v0;
    const V3 v1 = eigvec1(a, v0, e1);
    if (e1 < e0 && e1 < e2) return v1;
    return cross(v0, v1);
}

template <int KC>
__global__ __launch_bounds__(kBlock) void pp_nbr_kernel(const SPt* __restrict__ pts, uint64_t m, const Grid g,
                                                       const uint32_t* __restrict__ start, int max_nn, double radius,
                                                       uint32_t* __restrict__ nbr) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const SPt q = pts[i];
    const double r2 = radius * radius;
    const int cx = cell_of(q.x, g.lo[0], g.inv_h, g.n[0]);
    const int cy = cell_of(q.y, g.lo[1], g.inv_h, g.n[1]);
    const int cz = cell_of(q.z, g.lo[2], g.inv_h, g.n[2]);
    const int rmax = max(max(max(cx, g.n[0] - 1 - cx), max(cy, g.n[1] - 1 - cy)), max(cz, g.n[2] - 1 - cz));

    // walk A: the max_nn smallest d2 < r2 -> the cut-off D and the number of neighbours
    int r_end = rmax;
    int cnt = 0, less = 0;
    double D;
    {
        double best[KC];                                  // right-aligned, as in pp_knn_kernel
#pragma unroll
        for (int j = 0; j < KC; ++j) best[j] = j < KC - max_nn ? -INFINITY : INFINITY;
        for (int r = 0; r <= rmax; ++r) {
            PP_FOR_SHELL_ROWS(m) {
                const SPt p = pts[m];
                const double d2 = sq3(q.x, q.y, q.z, p.x, p.y, p.z);
                if (d2 < r2) insert_sorted<KC>(best, d2);
            }
            const double kth = best[KC - 1];
            const double margin = cube_margin(g, q.x, q.y, q.z, cx, cy, cz, r);
            // strict: every row with d2 == kth lies inside the cube too (walk B needs them all for the index tie-break)
            if (margin > 0.0 && (kth < margin * margin || margin >= radius)) { r_end = r; break; }
        }
        D = -INFINITY;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j >= KC - max_nn && best[j] < INFINITY) { ++cnt; D = fmax(D, best[j]); }   // cnt >= 1: the row itself
#pragma unroll
        for (int j = 0; j < KC; ++j) less += (j >= KC - max_nn && best[j] < D) ? 1 : 0;
    }

    // walk B: the rows with d2 < D in index order, then the rows with d2 == D in index order
    uint32_t key[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) key[j] = 0xFFFFFFFFu;
    for (int r = 0; r <= r_end; ++r)
        PP_FOR_SHELL_ROWS(m) {
            const SPt p = pts[m];
            const double d2 = sq3(q.x, q.y, q.z, p.x, p.y, p.z);
            if (d2 <= D) insert_sorted<KC>(key, (d2 == D ? kTie : 0u) | p.idx);
        }
    uint32_t* o = nbr + (uint64_t)q.idx * (uint32_t)max_nn;
#pragma unroll
    for (int j = 0; j < KC; ++j)
        if (j < max_nn) o[j] = j < cnt ? key[j] : 0xFFFFFFFFu;
}

// one lane per kept row: its neighbour list (pp_nbr_kernel) in (d2, index) order, the cumulants, the normal.  Kernels of
// their own: the list's distances and indices together do not fit beside the walk state in 128 registers.  The d2 < D
// part (already in index order) gets its stable rank by d2 from the distances alone (ranks packed four to a register),
// and the row's keys are permuted in place in global memory.
template <int KC>
__global__ __launch_bounds__(kBlock) void pp_pca_kernel(const double* __restrict__ pk, uint64_t m, int max_nn,
                                                       uint32_t* nbr, double* __restrict__ normals,
                                                       uint8_t* __restrict__ nn_count) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    uint32_t* row = nbr + i * (uint32_t)max_nn;
    const double qx = pk[3 * i], qy = pk[3 * i + 1], qz = pk[3 * i + 2];
    int cnt = 0, less = 0;
    double d[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        const uint32_t key = j < max_nn ? row[j] : 0xFFFFFFFFu;
        cnt += key != 0xFFFFFFFFu ? 1 : 0;
        d[j] = INFINITY;
        if (!(key & kTie)) {
            ++less;
            const uint64_t o = 3 * (uint64_t)key;
            d[j] = sq3(qx, qy, qz, pk[o], pk[o + 1], pk[o + 2]);
        }
    }
    if (nn_count) nn_count[i] = (uint8_t)cnt;
    double* out = normals + 3 * i;
    if (cnt < 3) { out[0] = 0.0; out[1] = 0.0; out[2] = 1.0; return; }

    uint32_t rank[(KC + 3) / 4];
#pragma unroll
    for (int w = 0; w < (KC + 3) / 4; ++w) rank[w] = 0;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        uint32_t rj = 0;
#pragma unroll
        for (int t = 0; t < KC; ++t)
            if (t != j) rj += (d[t] < d[j] || (d[t] == d[j] && t < j)) ? 1u : 0u;
        rank[j >> 2] |= rj << (8 * (j & 3));
    }
    uint32_t key[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) key[j] = j < less ? row[j] : 0u;
#pragma unroll
    for (int j = 0; j < KC; ++j)
        if (j < less) row[(rank[j >> 2] >> (8 * (j & 3))) & 0xFFu] = key[j];

    // Open3D's cumulants in neighbour order, then the covariance
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        if (j < cnt) {
            const uint64_t o = 3 * (uint64_t)(row[j] & ~kTie);
            const double x = pk[o], y = pk[o + 1], z = pk[o + 2];
            s[0] += x; s[1] += y; s[2] += z;
            s[3] += x * x; s[4] += x * y; s[5] += x * z;
            s[6] += y * y; s[7] += y * z; s[8] += z * z;
        }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) s[j] /= (double)cnt;
    const double cov[6] = {s[3] - s[0] * s[0], s[4] - s[0] * s[1], s[5] - s[0] * s[2],
                           s[6] - s[1] * s[1], s[7] - s[1] * s[2], s[8] - s[2] * s[2]};
    const V3 nv = smallest_eigvec(cov);
    if (nv.x == 0.0 && nv.y == 0.0 && nv.z == 0.0) { out[0] = 0.0; out[1] = 0.0; out[2] = 1.0; return; }
    out[0] = nv.x; out[1] = nv.y; out[2] = nv.z;
}

template <int KC>
hipError_t launch_knn(uint64_t n, hipStream_t st, const SPt* pts, const Grid& g, const uint32_t* start, int k, double* avg) {
    hipLaunchKernelGGL(pp_knn_kernel<KC>, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, pts, n, g,
                       start, k, avg);
    return hipGetLastError();
}

hipError_t dispatch_knn(uint64_t n, hipStream_t st, const SPt* pts, const Grid& g, const uint32_t* start, int k, double* avg) {
    if (k <= 1) return launch_knn<1>(n, st, pts, g, start, k, avg);
    if (k <= 2) return launch_knn<2>(n, st, pts, g, start, k, avg);
    if (k <= 4) return launch_knn<4>(n, st, pts, g, start, k, avg);
    if (k <= 8) return launch_knn<8>(n, st, pts, g, start, k, avg);
    if (k <= 16) return launch_knn<16>(n, st, pts, g, start, k, avg);
    if (k <= 20) return launch_knn<20>(n, st, pts, g, start, k, avg);
    if (k <= 24) return launch_knn<24>(n, st, pts, g, start, k, avg);
    return launch_knn<32>(n, st, pts, g, start, k, avg);
}

template <int KC>
hipError_t launch_normal(uint64_t m, hipStream_t st, const SPt* pts, const double* pk, const Grid& g, const uint32_t* start,
                         int max_nn, double radius, uint32_t* nbr, double* normals, uint8_t* nn) {
    const dim3 grid((uint32_t)((m + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(pp_nbr_kernel<KC>, grid, dim3(kBlock), 0, st, pts, m, g, start, max_nn, radius, nbr);
    hipLaunchKernelGGL(pp_pca_kernel<KC>, grid, dim3(kBlock), 0, st, pk, m, max_nn, nbr, normals, nn);
    return hipGetLastError();
}

hipError_t dispatch_normal(uint64_t m, hipStream_t st, const SPt* pts, const double* pk, const Grid& g,
                           const uint32_t* start, int max_nn, double radius, uint32_t* nbr, double* normals, uint8_t* nn) {
    if (max_nn <= 4) return launch_normal<4>(m, st, pts, pk, g, start, max_nn, radius, nbr, normals, nn);
    if (max_nn <= 8) return launch_normal<8>(m, st, pts, pk, g, start, max_nn, radius, nbr, normals, nn);
    if (max_nn <= 16) return launch_normal<16>(m, st, pts, pk, g, start, max_nn, radius, nbr, normals, nn);
    if (max_nn <= 24) return launch_normal<24>(m, st, pts, pk, g, start, max_nn, radius, nbr, normals, nn);
    return launch_normal<32>(m, st, pts, pk, g, start, max_nn, radius, nbr, normals, nn);
}

// the rows of p (m of them) in cell order and the table of cell starts; LRC_ERR_INVALID_ARG for a non-finite coordinate
int build_grid(const double* p, uint64_t m, double cell_size, int per_cell, hipStream_t st, Arena& arena, Grid* out_g,
               SPt** out_pts, uint32_t** out_start) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>((m + kBlock - 1) / kBlock, kRedBlocks);
    double* part;
    uint32_t* bad;
    {
        void* q;
        LRC_HIP(arena.get(align256(nb * 6 * 8) + 256, &q));
        part = (double*)q;
        bad = (uint32_t*)((char*)q + align256(nb * 6 * 8));
    }
    LRC_HIP(hipMemsetAsync(bad, 0, 4, st));
    hipLaunchKernelGGL(pp_bounds_kernel, dim3(nb), dim3(kBlock), 0, st, p, m, part, bad);
    LRC_HIP(hipGetLastError());
    std::vector<double> h_part((size_t)nb * 6);
    uint32_t h_bad = 0;
    LRC_HIP(hipMemcpyAsync(h_part.data(), part, h_part.size() * 8, hipMemcpyDeviceToHost, st));
    LRC_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st));
    LRC_HIP(hipStreamSynchronize(st));
    if (h_bad) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_cloud_preprocess: non-finite coordinate");
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t b = 0; b < nb; ++b)
        for (int c = 0; c < 3; ++c) {
            lo[c] = std::min(lo[c], h_part[6 * b + c]);
            hi[c] = std::max(hi[c], h_part[6 * b + 3 + c]);
        }
    Grid g{};
    double ext[3], emax = 0.0;
    for (int c = 0; c < 3; ++c) {
        g.lo[c] = lo[c];
        ext[c] = hi[c] - lo[c];
        emax = std::max(emax, ext[c]);
    }
    double h = cell_size;
    if (!(h > 0.0)) {
        // scan points lie on surfaces: about per_cell rows per cell of a sheet spanning the largest face of the box
        const double area = std::max(std::max(ext[0] * ext[1], ext[1] * ext[2]), ext[0] * ext[2]);
        if (area > 0.0) h = std::sqrt(area * (double)per_cell / (double)m);
        else if (emax > 0.0) h = emax * (double)per_cell / (double)m;
        else h = 1.0;
    }
    h = std::max(h, emax / 1024.0);                         // at most 1024 cells per axis
    if (!(h > 0.0)) h = 1.0;
    const double cap = 2.0 * (double)m + 64.0;
    uint64_t cells;
    for (;;) {
        double cd = 1.0;
        for (int c = 0; c < 3; ++c) {
            g.n[c] = std::max(1, (int)std::floor(ext[c] / h) + 1);
            cd *= (double)g.n[c];
        }
        if (cd <= cap) { cells = (uint64_t)cd; break; }
        h *= 1.26;
    }
    g.h = h;
    g.inv_h = 1.0 / h;

    uint32_t *keys_a, *keys_b, *vals_a, *vals_b, *counts, *start;
    SPt* pts;
    {
        const size_t sz = align256(m * 4), o_cnt = 4 * sz, o_start = o_cnt + align256((cells + 1) * 4),
                     o_pts = o_start + align256((cells + 1) * 4), total = o_pts + align256(m * sizeof(SPt));
        void* q;
        LRC_HIP(arena.get(total, &q));
        char* c = (char*)q;
        keys_a = (uint32_t*)c; keys_b = (uint32_t*)(c + sz); vals_a = (uint32_t*)(c + 2 * sz);
        vals_b = (uint32_t*)(c + 3 * sz); counts = (uint32_t*)(c + o_cnt); start = (uint32_t*)(c + o_start);
        pts = (SPt*)(c + o_pts);
    }
    const uint32_t mblk = (uint32_t)((m + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pp_key_kernel, dim3(mblk), dim3(kBlock), 0, st, p, m, g, keys_a, vals_a);
    LRC_HIP(hipGetLastError());
    LRC_HIP(hipMemsetAsync(counts, 0, (cells + 1) * 4, st));
    const int end_bit = std::max(1, bit_width(cells));
    size_t tmp_sort = 0, tmp_scan = 0;
    LRC_HIP(rocprim::radix_sort_pairs(nullptr, tmp_sort, keys_a, keys_b, vals_a, vals_b, (size_t)m, 0, end_bit, st));
    LRC_HIP(rocprim::exclusive_scan(nullptr, tmp_scan, counts, start, 0u, (size_t)(cells + 1), rocprim::plus<uint32_t>(), st));
    void* tmp;
    LRC_HIP(arena.get(std::max(tmp_sort, tmp_scan), &tmp));
    LRC_HIP(rocprim::radix_sort_pairs(tmp, tmp_sort, keys_a, keys_b, vals_a, vals_b, (size_t)m, 0, end_bit, st));
    hipLaunchKernelGGL(pp_gather_kernel, dim3(mblk), dim3(kBlock), 0, st, p, keys_b, vals_b, m, counts, pts);
    LRC_HIP(hipGetLastError());
    LRC_HIP(rocprim::exclusive_scan(tmp, tmp_scan, counts, start, 0u, (size_t)(cells + 1), rocprim::plus<uint32_t>(), st));
    *out_g = g;
    *out_pts = pts;
    *out_start = start;
    return LRC_OK;
}

int check_opts(uint64_t n, const lrc_preprocess_opts* o) {
    if (n >= (1ull << 31)) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_cloud_preprocess: need n < 2^31");
    if (o->remove_outliers) {
        if (o->nb_neighbors < 1 || o->nb_neighbors > 32)
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_cloud_preprocess: need 1 <= nb_neighbors <= 32");
        if (!finite_positive(o->std_ratio))
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_cloud_preprocess: need a finite std_ratio > 0");
    }
    if (o->estimate_normals) {
        if (o->max_nn < 1 || o->max_nn > 32)
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_cloud_preprocess: need 1 <= max_nn <= 32");
        if (!finite_positive(o->radius))
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_cloud_preprocess: need a finite radius > 0");
    }
    return LRC_OK;
}

}  // namespace

extern "C" {

int lrc_cloud_preprocess_dev(lrc_ctx* ctx, const double* d_points3, uint64_t n, const lrc_preprocess_opts* opts,
                             uint32_t* d_out_kept, uint64_t* out_num_kept, double* d_out_normals3, double* d_out_avg,
                             uint8_t* d_out_nn_count, double* out_stats2, void* stream) {
    if (!ctx || !opts || !out_num_kept || (n && (!d_points3 || !d_out_kept)) ||
        (opts->estimate_normals && n && !d_out_normals3))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_cloud_preprocess_dev: NULL argument");
    *out_num_kept = 0;
    if (out_stats2) { out_stats2[0] = 0.0; out_stats2[1] = INFINITY; }
    if (int rc = check_opts(n, opts)) return rc;
    if (n == 0) return LRC_OK;
    LRC_HIP(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    Arena arena(st);
    const int per_cell = std::max(opts->remove_outliers ? (int)opts->nb_neighbors : 1,
                                  opts->estimate_normals ? (int)opts->max_nn : 1);
    const uint32_t nblk = (uint32_t)((n + kBlock - 1) / kBlock);

    Grid g;
    SPt* pts;
    uint32_t* start;
    // the first grid also rejects non-finite input, whichever stages run
    if (int rc = build_grid(d_points3, n, opts->cell_size, per_cell, st, arena, &g, &pts, &start)) return rc;

    uint64_t m = n;
    const double* pk = d_points3;                     // the normals' input rows, in kept order
    if (opts->remove_outliers) {
        double *avg, *part, *stats, *pkb;
        uint32_t *flag, *pos;
        {
            const size_t o_part = align256(n * 8), o_stats = o_part + align256(kRedBlocks * 8),
                         o_flag = o_stats + 256, o_pos = o_flag + align256(n * 4), o_pk = o_pos + align256(n * 4),
                         total = o_pk + (opts->estimate_normals ? align256(n * 24) : 0);
            void* q;
            LRC_HIP(arena.get(total, &q));
            char* c = (char*)q;
            avg = (double*)c; part = (double*)(c + o_part); stats = (double*)(c + o_stats);
            flag = (uint32_t*)(c + o_flag); pos = (uint32_t*)(c + o_pos); pkb = (double*)(c + o_pk);
        }
        LRC_HIP(dispatch_knn(n, st, pts, g, start, (int)opts->nb_neighbors, avg));
        hipLaunchKernelGGL(pp_sum_kernel, dim3(kRedBlocks), dim3(kBlock), 0, st, avg, n, (const double*)nullptr, part);
        hipLaunchKernelGGL(pp_final_kernel, dim3(1), dim3(kRedBlocks), 0, st, part, n, 0, opts->std_ratio, stats);
        hipLaunchKernelGGL(pp_sum_kernel, dim3(kRedBlocks), dim3(kBlock), 0, st, avg, n, (const double*)stats, part);
        hipLaunchKernelGGL(pp_final_kernel, dim3(1), dim3(kRedBlocks), 0, st, part, n, 1, opts->std_ratio, stats);
        hipLaunchKernelGGL(pp_keep_kernel, dim3(nblk), dim3(kBlock), 0, st, avg, n, stats, flag);
        LRC_HIP(hipGetLastError());
        size_t tmp_scan = 0;
        LRC_HIP(rocprim::exclusive_scan(nullptr, tmp_scan, flag, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
        void* tmp;
        LRC_HIP(arena.get(tmp_scan, &tmp));
        LRC_HIP(rocprim::exclusive_scan(tmp, tmp_scan, flag, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL(pp_compact_kernel, dim3(nblk), dim3(kBlock), 0, st, d_points3, n, flag, pos, d_out_kept,
                           opts->estimate_normals ? pkb : nullptr);
        LRC_HIP(hipGetLastError());
        if (d_out_avg) LRC_HIP(hipMemcpyAsync(d_out_avg, avg, n * 8, hipMemcpyDeviceToDevice, st));
        uint32_t last[2];
        double h_stats[2];
        LRC_HIP(hipMemcpyAsync(&last[0], pos + (n - 1), 4, hipMemcpyDeviceToHost, st));
        LRC_HIP(hipMemcpyAsync(&last[1], flag + (n - 1), 4, hipMemcpyDeviceToHost, st));
        LRC_HIP(hipMemcpyAsync(h_stats, stats, 16, hipMemcpyDeviceToHost, st));
        LRC_HIP(hipStreamSynchronize(st));
        m = (uint64_t)last[0] + last[1];
        if (out_stats2) { out_stats2[0] = h_stats[0]; out_stats2[1] = h_stats[1]; }
        pk = pkb;
    } else {
        hipLaunchKernelGGL(pp_fill_kernel, dim3(nblk), dim3(kBlock), 0, st, n, d_out_kept, d_out_avg);
        LRC_HIP(hipGetLastError());
    }

    if (opts->estimate_normals && m > 0) {
        if (opts->remove_outliers) {
            // Open3D builds a new tree on the kept cloud: a grid of their own (the neighbours do not depend on it)
            if (int rc = build_grid(pk, m, opts->cell_size, per_cell, st, arena, &g, &pts, &start)) return rc;
        }
        void* nbr;                                    // max_nn neighbour keys per kept row
        LRC_HIP(arena.get(m * opts->max_nn * 4, &nbr));
        LRC_HIP(dispatch_normal(m, st, pts, pk, g, start, (int)opts->max_nn, opts->radius, (uint32_t*)nbr, d_out_normals3,
                               d_out_nn_count));
    }
    LRC_HIP(hipStreamSynchronize(st));
    *out_num_kept = m;
    return LRC_OK;
}

int lrc_cloud_preprocess(lrc_ctx* ctx, const double* points3, uint64_t n, const lrc_preprocess_opts* opts,
                         uint32_t* out_kept, uint64_t* out_num_kept, double* out_normals3, double* out_avg,
                         uint8_t* out_nn_count, double* out_stats2) {
    if (!ctx || !opts || !out_num_kept || (n && (!points3 || !out_kept)) || (opts->estimate_normals && n && !out_normals3))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_cloud_preprocess: NULL argument");
    *out_num_kept = 0;
    if (out_stats2) { out_stats2[0] = 0.0; out_stats2[1] = INFINITY; }
    if (int rc = check_opts(n, opts)) return rc;
    if (n == 0) return LRC_OK;
    LRC_HIP(hipSetDevice(ctx->device));
    const bool normals = opts->estimate_normals != 0;
    double *d_p = nullptr, *d_normals = nullptr, *d_avg = nullptr;
    uint32_t* d_kept = nullptr;
    uint8_t* d_nn = nullptr;
    int rc = LRC_OK;
    uint64_t m = 0;
    if (hipMalloc((void**)&d_p, n * 24) != hipSuccess || hipMalloc((void**)&d_kept, n * 4) != hipSuccess ||
        (normals && hipMalloc((void**)&d_normals, n * 24) != hipSuccess) ||
        (out_avg && hipMalloc((void**)&d_avg, n * 8) != hipSuccess) ||
        (normals && out_nn_count && hipMalloc((void**)&d_nn, n) != hipSuccess)) {
        rc = lrc_internal_fail(LRC_ERR_OOM, "lrc_cloud_preprocess: out of device memory");
    } else if (hipMemcpy(d_p, points3, n * 24, hipMemcpyHostToDevice) != hipSuccess) {
        rc = lrc_internal_fail(LRC_ERR_HIP, "lrc_cloud_preprocess: upload failed");
    } else if ((rc = lrc_cloud_preprocess_dev(ctx, d_p, n, opts, d_kept, &m, d_normals, d_avg, d_nn, out_stats2,
                                              nullptr)) == LRC_OK) {
        if (hipMemcpy(out_kept, d_kept, m * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            (normals && m && hipMemcpy(out_normals3, d_normals, m * 24, hipMemcpyDeviceToHost) != hipSuccess) ||
            (out_avg && hipMemcpy(out_avg, d_avg, n * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
            (d_nn && m && hipMemcpy(out_nn_count, d_nn, m, hipMemcpyDeviceToHost) != hipSuccess))
            rc = lrc_internal_fail(LRC_ERR_HIP, "lrc_cloud_preprocess: download failed");
        else
            *out_num_kept = m;
    }
    if (d_p) (void)hipFree(d_p);
    if (d_kept) (void)hipFree(d_kept);
    if (d_normals) (void)hipFree(d_normals);
    if (d_avg) (void)hipFree(d_avg);
    if (d_nn) (void)hipFree(d_nn);
    return rc;
}

}  // extern "C"
