// lrc_boxes.hip -- detection boxes from a labelled scan cloud: per-instance k-NN statistical outlier filter and AABB
// (gfx950).
//
// The reference turns the labelled cloud into 3-D detection annotations in lidar_net_bbox_visualizer.py: the points of
// every (class, instance) pair with instance != 0 and at least min_points rows (:163-201), Open3D's
// remove_statistical_outlier(nb_neighbors=k, std_ratio) inside each instance of k rows or more (:203-225), and the
// axis-aligned box of what is left (:227-249).  All instances of a cloud go through one call here:
//   1. key every row (class index << 16 | ins, or "ignored") and radix-sort the keys: one segment per instance,
//      rows in ascending row order inside it (the sort is stable);
//   2. one workgroup per segment: float32 AABB, a cell size for the instance (surfaces: about k rows per cell of the
//      sheet), each row's (segment, cell) key; a second stable sort by that key and a counting table of cell starts;
//   3. one lane per row: the k smallest float64 squared distances (dx*dx + dy*dy) + dz*dz among the rows of its
//      instance, itself included, over expanding cube shells of cells until the k-th cannot be beaten (lrc_nn.hip's
//      exactness argument); avg = (sum of the k square roots, ascending, one after the other) / k;
//   4. one workgroup per segment: mean = sum_{avg>0} avg / n and std = sqrt(sum_{avg>0} (avg-mean)^2 / (n-1)) in a
//      fixed reduction order, thr = mean + std_ratio * std, keep = avg > 0 && avg < thr, min / max of the kept rows
//      (as numpy's min / max over the rows: a zero extreme has the sign of the last kept zero row).
// The k-best list lives in registers: one instantiation per list length, compile-time indices only (no scratch).
// Only distances are used, so ties and the cell size cannot change a result.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "lrc_internal.h"

namespace {

constexpr uint32_t kIgnored = 0xFFFFFFFFu;
constexpr int kMaxClasses = 64;

struct ClassList {
    uint32_t n;
    uint16_t id[kMaxClasses];
};

// grid of one instance; cells = 1 and filtered = 0 for instances the filter does not run on
struct SegGrid {
    double lo[3];
    double h, inv_h;
    uint64_t table;          // first entry of the instance's cell table
    int n[3];
    uint32_t filtered;
};

__device__ __forceinline__ int cell_of(double x, double lo, double inv_h, int n) {
    const double f = floor((x - lo) * inv_h);
    return f < 0.0 ? 0 : (f >= (double)n ? n - 1 : (int)f);
}

__device__ __forceinline__ uint32_t bits_of(float f) { return __float_as_uint(f); }

__global__ __launch_bounds__(kBlock) void box_key_kernel(const float4* __restrict__ xyzl, uint64_t K, const ClassList cl,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ rows,
                                                         double* __restrict__ out_avg, uint8_t* __restrict__ out_keep) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const uint32_t lab = bits_of(xyzl[i].w);
    const uint32_t sem = lab & 0xFFFFu, ins = lab >> 16;
    uint32_t key = kIgnored;
    if (ins != 0)
        for (uint32_t c = 0; c < cl.n; ++c)
            if (cl.id[c] == sem) { key = (c << 16) | ins; break; }
    keys[i] = key;
    rows[i] = (uint32_t)i;
    if (out_avg) out_avg[i] = -1.0;
    if (out_keep) out_keep[i] = 0;
}

// one workgroup per segment: AABB, grid, (segment, cell) key of every row
__global__ __launch_bounds__(kBlock) void box_grid_kernel(const float4* __restrict__ xyzl, const uint32_t* __restrict__ rows,
                                                          const uint32_t* __restrict__ seg_start,
                                                          const uint32_t* __restrict__ seg_count,
                                                          const uint64_t* __restrict__ seg_table, uint32_t min_points,
                                                          uint32_t k, double cell_size, SegGrid* __restrict__ grids,
                                                          uint64_t* __restrict__ key64, uint32_t* __restrict__ pos) {
    __shared__ float red[6][kBlock];
    __shared__ SegGrid sg;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const uint32_t a = seg_start[s], n = seg_count[s];
    const bool filtered = n >= min_points && n >= k;
    if (!filtered) {
        if (t == 0) {
            SegGrid g{};
            g.h = g.inv_h = 1.0;
            g.n[0] = g.n[1] = g.n[2] = 1;
            g.table = seg_table[s];
            g.filtered = 0;
            grids[s] = g;
        }
        for (uint32_t j = t; j < n; j += kBlock) { key64[a + j] = (uint64_t)s << 32; pos[a + j] = a + j; }
        return;
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t j = t; j < n; j += kBlock) {
        const float4 p = xyzl[rows[a + j]];
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
    for (int c = 0; c < 3; ++c) { red[c][t] = lo[c]; red[3 + c][t] = hi[c]; }
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (t < (uint32_t)w)
            for (int c = 0; c < 3; ++c) {
                red[c][t] = fminf(red[c][t], red[c][t + w]);
                red[3 + c][t] = fmaxf(red[3 + c][t], red[3 + c][t + w]);
            }
        __syncthreads();
    }
    if (t == 0) {
        double ext[3], emax = 0.0;
        for (int c = 0; c < 3; ++c) {
            sg.lo[c] = (double)red[c][0];
            ext[c] = (double)red[3 + c][0] - (double)red[c][0];
            emax = fmax(emax, ext[c]);
        }
        double h = cell_size;
        if (!(h > 0.0)) {
            // scan points lie on surfaces: about k rows per cell of a sheet spanning the largest face of the box
            const double area = fmax(fmax(ext[0] * ext[1], ext[1] * ext[2]), ext[0] * ext[2]);
            if (area > 0.0) h = sqrt(area * (double)k / (double)n);
            else if (emax > 0.0) h = emax * (double)k / (double)n;
            else h = 1.0;
        }
        h = fmax(h, emax / 1024.0);                          // at most 1024 cells per axis
        if (!(h > 0.0)) h = 1.0;
        const double cap = 2.0 * (double)n + 64.0;           // the host sized the cell table for this
        for (;;) {
            double cells = 1.0;
            for (int c = 0; c < 3; ++c) {
                sg.n[c] = max(1, (int)floor(ext[c] / h) + 1);
                cells *= (double)sg.n[c];
            }
            if (cells <= cap) break;
            h *= 1.26;
        }
        sg.h = h;
        sg.inv_h = 1.0 / h;
        sg.table = seg_table[s];
        sg.filtered = 1;
        grids[s] = sg;
    }
    __syncthreads();
    const SegGrid g = sg;
    for (uint32_t j = t; j < n; j += kBlock) {
        const float4 p = xyzl[rows[a + j]];
        const int cx = cell_of((double)p.x, g.lo[0], g.inv_h, g.n[0]);
        const int cy = cell_of((double)p.y, g.lo[1], g.inv_h, g.n[1]);
        const int cz = cell_of((double)p.z, g.lo[2], g.inv_h, g.n[2]);
        key64[a + j] = ((uint64_t)s << 32) | (uint64_t)(((uint32_t)cz * (uint32_t)g.n[1] + (uint32_t)cy) * (uint32_t)g.n[0] + (uint32_t)cx);
        pos[a + j] = a + j;
    }
}

// cell populations (counts only: their values do not depend on the order of the atomics) and the points in cell
// order, each carrying its position in instance order (pos: the second sort's values; rows: the first sort's)
__global__ __launch_bounds__(kBlock) void box_count_kernel(const float4* __restrict__ xyzl, const uint64_t* __restrict__ key64,
                                                           const uint32_t* __restrict__ pos,
                                                           const uint32_t* __restrict__ rows, uint64_t M,
                                                           const SegGrid* __restrict__ grids, uint32_t* __restrict__ table,
                                                           float4* __restrict__ pts) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= M) return;
    const uint64_t key = key64[j];
    atomicAdd(&table[grids[key >> 32].table + (key & 0xFFFFFFFFull)], 1u);
    const uint32_t q = pos[j];
    const float4 p = xyzl[rows[q]];
    pts[j] = make_float4(p.x, p.y, p.z, __uint_as_float(q));
}

// insert d2 into the ascending list best[0..KC): compile-time indices only
template <int KC>
__device__ __forceinline__ void insert_sorted(double (&best)[KC], double d2) {
    if (!(d2 < best[KC - 1])) return;
#pragma unroll
    for (int j = KC - 1; j > 0; --j) {
        const double prev = best[j - 1];
        best[j] = d2 < prev ? prev : (d2 < best[j] ? d2 : best[j]);
    }
    best[0] = d2 < best[0] ? d2 : best[0];
}

template <int KC>
__global__ __launch_bounds__(kBlock) void box_knn_kernel(const float4* __restrict__ pts, const uint64_t* __restrict__ key64,
                                                         uint64_t M, const SegGrid* __restrict__ grids,
                                                         const uint32_t* __restrict__ start, int k,
                                                         double* __restrict__ avg) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    const SegGrid g = grids[key64[i] >> 32];
    const float4 q = pts[i];
    const uint32_t qi = __float_as_uint(q.w);          // avg is stored in instance order
    if (!g.filtered) { avg[qi] = -1.0; return; }
    const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
    const int cx = cell_of(qx, g.lo[0], g.inv_h, g.n[0]);
    const int cy = cell_of(qy, g.lo[1], g.inv_h, g.n[1]);
    const int cz = cell_of(qz, g.lo[2], g.inv_h, g.n[2]);
    double best[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) best[j] = INFINITY;
    const uint32_t* tab = start + g.table;
    const int rmax = max(max(max(cx, g.n[0] - 1 - cx), max(cy, g.n[1] - 1 - cy)), max(cz, g.n[2] - 1 - cz));
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.n[2] - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, g.n[1] - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.n[0] - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool zface = (z == cz - r) | (z == cz + r);
            for (int y = y0; y <= y1; ++y) {
                const bool yface = (y == cy - r) | (y == cy + r);
                // on a z- or y-face of the shell the whole x-run belongs to it; otherwise only the two ends
                const int step = (zface | yface) ? 1 : max(2 * r, 1);
                for (int x = cx - r; x <= cx + r; x += step) {
                    if (x < x0 || x > x1) continue;
                    const uint32_t c = ((uint32_t)z * (uint32_t)g.n[1] + (uint32_t)y) * (uint32_t)g.n[0] + (uint32_t)x;
                    const uint32_t b0 = tab[c], b1 = tab[c + 1];
                    for (uint32_t m = b0; m < b1; ++m) {
                        const float4 p = pts[m];
                        const double dx = qx - (double)p.x, dy = qy - (double)p.y, dz = qz - (double)p.z;
                        insert_sorted<KC>(best, (dx * dx + dy * dy) + dz * dz);
                    }
                }
            }
        }
        double kth = best[0];
#pragma unroll
        for (int j = 1; j < KC; ++j) kth = (j == k - 1) ? best[j] : kth;
        if (kth < INFINITY) {
            // everything inside the cube of cells [c-r, c+r]^3 has been searched: a closer row would have to lie
            // outside it, i.e. farther than the distance from q to the nearest face of that cube
            const double mx = fmin(qx - (g.lo[0] + (double)(cx - r) * g.h), (g.lo[0] + (double)(cx + r + 1) * g.h) - qx);
            const double my = fmin(qy - (g.lo[1] + (double)(cy - r) * g.h), (g.lo[1] + (double)(cy + r + 1) * g.h) - qy);
            const double mz = fmin(qz - (g.lo[2] + (double)(cz - r) * g.h), (g.lo[2] + (double)(cz + r + 1) * g.h) - qz);
            // (shrunk by 1e-6 cell: a row binned by floor((p-lo)/h) may sit one rounding below its cell's edge)
            const double margin = fmin(mx, fmin(my, mz)) - 1.0e-6 * g.h;
            if (margin > 0.0 && kth <= margin * margin) break;
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < KC; ++j)
        if (j < k) sum += sqrt(best[j]);
    avg[qi] = sum / (double)k;
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

// one workgroup per segment: statistics, keep flags, box of the kept rows.  Every sum has one fixed order, whatever the
// grid: each lane accumulates rows t, t+256, ... of the instance (ascending row order) in turn, then a fixed tree over
// the lanes.
// zr: per axis, 1 + the position in the instance of the last kept row whose coordinate is +0 or -0.  numpy's min / max
// over the rows (a running np.minimum / np.maximum, row after row) keeps the later of two equal values, so a zero
// extreme takes the sign of the last kept zero row; fminf / fmaxf and the tree over the lanes cannot know which that is.
__global__ __launch_bounds__(kBlock) void box_stats_kernel(const float4* __restrict__ xyzl, const uint32_t* __restrict__ rows,
                                                           const double* __restrict__ avg,
                                                           const uint32_t* __restrict__ seg_start,
                                                           const uint32_t* __restrict__ seg_count,
                                                           const SegGrid* __restrict__ grids, uint32_t min_points,
                                                           double std_ratio, lrc_box* __restrict__ boxes,
                                                           double* __restrict__ out_avg, uint8_t* __restrict__ out_keep) {
    __shared__ double red[kBlock];
    __shared__ float fred[6][kBlock];
    __shared__ uint32_t cred[kBlock];
    __shared__ uint32_t zred[3][kBlock];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const uint32_t a = seg_start[s], n = seg_count[s];
    if (n < min_points) {
        if (t == 0) { boxes[s].num_points = n; boxes[s].num_kept = 0; boxes[s].filtered = 0; }
        return;
    }
    const bool filtered = grids[s].filtered != 0;
    double mean = 0.0, thr = INFINITY;
    if (filtered) {
        double acc = 0.0;
        for (uint32_t j = t; j < n; j += kBlock) {
            const double v = avg[a + j];
            if (v > 0.0) acc += v;
        }
        mean = block_sum(acc, red) / (double)n;
        acc = 0.0;
        for (uint32_t j = t; j < n; j += kBlock) {
            const double v = avg[a + j];
            if (v > 0.0) { const double d = v - mean; acc += d * d; }
        }
        const double sq = block_sum(acc, red);
        const double sd = sqrt(sq / (double)(n - 1));
        thr = mean + std_ratio * sd;
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t kept = 0, zr[3] = {0, 0, 0};
    for (uint32_t j = t; j < n; j += kBlock) {
        const double v = filtered ? avg[a + j] : -1.0;
        const bool keep = !filtered || (v > 0.0 && v < thr);
        const uint32_t r = rows[a + j];
        const float4 p = xyzl[r];
        if (keep) {
            ++kept;
            lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
            hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
            // positions ascend in a lane: the last one wins
            if ((bits_of(p.x) << 1) == 0) zr[0] = j + 1;
            if ((bits_of(p.y) << 1) == 0) zr[1] = j + 1;
            if ((bits_of(p.z) << 1) == 0) zr[2] = j + 1;
        }
        if (out_avg) out_avg[r] = v;
        if (out_keep) out_keep[r] = keep ? 1 : 0;
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c) { fred[c][t] = lo[c]; fred[3 + c][t] = hi[c]; zred[c][t] = zr[c]; }
    cred[t] = kept;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (t < (uint32_t)w) {
            for (int c = 0; c < 3; ++c) {
                fred[c][t] = fminf(fred[c][t], fred[c][t + w]);
                fred[3 + c][t] = fmaxf(fred[3 + c][t], fred[3 + c][t + w]);
                zred[c][t] = max(zred[c][t], zred[c][t + w]);
            }
            cred[t] += cred[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        lrc_box& b = boxes[s];
        b.num_points = n;
        b.num_kept = cred[0];
        b.filtered = filtered ? 1 : 0;
        for (int c = 0; c < 3; ++c) {
            b.min3[c] = fred[c][0];
            b.max3[c] = fred[3 + c][0];
            const uint32_t z = zred[c][0];
            if (z) {
                const float zero = reinterpret_cast<const float*>(xyzl)[4 * (uint64_t)rows[a + z - 1] + c];
                if (b.min3[c] == 0.0f) b.min3[c] = zero;
                if (b.max3[c] == 0.0f) b.max3[c] = zero;
            }
        }
        b.mean = mean;
        b.threshold = thr;
    }
}

template <int KC>
hipError_t launch_knn(uint64_t M, hipStream_t st, const float4* pts, const uint64_t* key64, const SegGrid* grids,
                      const uint32_t* start, int k, double* avg) {
    const uint64_t nblk = (M + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(box_knn_kernel<KC>, dim3((uint32_t)nblk), dim3(kBlock), 0, st, pts, key64, M, grids, start, k, avg);
    return hipGetLastError();
}

hipError_t dispatch_knn(uint64_t M, hipStream_t st, const float4* pts, const uint64_t* key64, const SegGrid* grids,
                        const uint32_t* start, int k, double* avg) {
    if (k <= 1) return launch_knn<1>(M, st, pts, key64, grids, start, k, avg);
    if (k <= 2) return launch_knn<2>(M, st, pts, key64, grids, start, k, avg);
    if (k <= 4) return launch_knn<4>(M, st, pts, key64, grids, start, k, avg);
    if (k <= 8) return launch_knn<8>(M, st, pts, key64, grids, start, k, avg);
    if (k <= 16) return launch_knn<16>(M, st, pts, key64, grids, start, k, avg);
    if (k <= 20) return launch_knn<20>(M, st, pts, key64, grids, start, k, avg);
    if (k <= 24) return launch_knn<24>(M, st, pts, key64, grids, start, k, avg);
    return launch_knn<32>(M, st, pts, key64, grids, start, k, avg);
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

int check_params(uint64_t K, const uint16_t* class_ids, uint32_t num_classes, uint32_t k, ClassList* cl) {
    if (K >= (1ull << 31)) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_instance_boxes: need num_rows < 2^31");
    if (k < 1 || k > 32) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_instance_boxes: need 1 <= k <= 32");
    if (num_classes > (uint32_t)kMaxClasses)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_instance_boxes: at most 64 classes");
    if (num_classes && !class_ids) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_instance_boxes: NULL class_ids");
    std::memset(cl, 0, sizeof(*cl));
    cl->n = num_classes;
    for (uint32_t c = 0; c < num_classes; ++c) {
        for (uint32_t d = 0; d < c; ++d)
            if (class_ids[d] == class_ids[c])
                return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_instance_boxes: repeated class id");
        cl->id[c] = class_ids[c];
    }
    return LRC_OK;
}

}  // namespace

extern "C" {

int lrc_instance_boxes_dev(lrc_ctx* ctx, const float* d_xyzl, uint64_t num_rows, const uint16_t* class_ids,
                           uint32_t num_classes, uint32_t min_points, uint32_t k, double std_ratio, double cell_size,
                           lrc_box* out_boxes, uint64_t capacity, uint64_t* out_num_boxes, double* d_out_avg,
                           uint8_t* d_out_keep, void* stream) {
    if (!ctx || !out_num_boxes || (num_rows && !d_xyzl) || (capacity && !out_boxes))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_instance_boxes_dev: NULL argument");
    *out_num_boxes = 0;
    ClassList cl;
    if (int rc = check_params(num_rows, class_ids, num_classes, k, &cl)) return rc;
    if (num_rows == 0) return LRC_OK;
    LRC_HIP(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const uint64_t K = num_rows;
    const float4* xyzl = reinterpret_cast<const float4*>(d_xyzl);
    Arena arena(st);

    // ---- 1. key, sort, segments ----
    uint32_t *keys_a, *keys_b, *rows_a, *rows_b, *ukeys, *counts, *nruns;
    {
        void* p;
        const size_t sz = align256(K * 4);
        LRC_HIP(arena.get(6 * sz + 256, &p));
        char* c = (char*)p;
        keys_a = (uint32_t*)c; keys_b = (uint32_t*)(c + sz); rows_a = (uint32_t*)(c + 2 * sz);
        rows_b = (uint32_t*)(c + 3 * sz); ukeys = (uint32_t*)(c + 4 * sz); counts = (uint32_t*)(c + 5 * sz);
        nruns = (uint32_t*)(c + 6 * sz);
    }
    const uint32_t nblk = (uint32_t)((K + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(box_key_kernel, dim3(nblk), dim3(kBlock), 0, st, xyzl, K, cl, keys_a, rows_a, d_out_avg, d_out_keep);
    LRC_HIP(hipGetLastError());
    const int end_bit1 = 16 + bit_width(num_classes);        // the ignored key's bits above all class indices
    size_t tmp1 = 0, tmp_rle = 0;
    LRC_HIP(rocprim::radix_sort_pairs(nullptr, tmp1, keys_a, keys_b, rows_a, rows_b, (size_t)K, 0, end_bit1, st));
    LRC_HIP(rocprim::run_length_encode(nullptr, tmp_rle, keys_b, (unsigned int)K, ukeys, counts, nruns, st));
    void* tmp;
    LRC_HIP(arena.get(std::max(tmp1, tmp_rle), &tmp));
    LRC_HIP(rocprim::radix_sort_pairs(tmp, tmp1, keys_a, keys_b, rows_a, rows_b, (size_t)K, 0, end_bit1, st));
    LRC_HIP(rocprim::run_length_encode(tmp, tmp_rle, keys_b, (unsigned int)K, ukeys, counts, nruns, st));
    uint32_t runs = 0;
    LRC_HIP(hipMemcpyAsync(&runs, nruns, 4, hipMemcpyDeviceToHost, st));
    LRC_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> h_ukeys(runs), h_counts(runs);
    if (runs) {
        LRC_HIP(hipMemcpyAsync(h_ukeys.data(), ukeys, (size_t)runs * 4, hipMemcpyDeviceToHost, st));
        LRC_HIP(hipMemcpyAsync(h_counts.data(), counts, (size_t)runs * 4, hipMemcpyDeviceToHost, st));
        LRC_HIP(hipStreamSynchronize(st));
    }
    const uint32_t S = (runs && h_ukeys[runs - 1] == kIgnored) ? runs - 1 : runs;
    if (S == 0) return LRC_OK;
    std::vector<uint32_t> h_start(S);
    std::vector<uint64_t> h_table(S);
    uint64_t M = 0, T = 0;
    for (uint32_t s = 0; s < S; ++s) {
        h_start[s] = (uint32_t)M;
        h_table[s] = T;
        M += h_counts[s];
        const bool filtered = h_counts[s] >= min_points && h_counts[s] >= k;
        T += filtered ? 2ull * h_counts[s] + 64 : 1;         // box_grid_kernel's cap on the instance's cells
    }

    // ---- 2. grids, second sort, cell table ----
    uint32_t *seg_start, *seg_count, *table, *starts;
    uint64_t *seg_table, *key_a, *key_b;
    SegGrid* grids;
    float4* pts;
    double* avg;
    lrc_box* boxes;
    {
        const size_t o_count = align256(S * 4), o_tab = o_count + align256(S * 4), o_grid = o_tab + align256(S * 8),
                     o_box = o_grid + align256(S * sizeof(SegGrid)), o_ka = o_box + align256(S * sizeof(lrc_box)),
                     o_kb = o_ka + align256(M * 8), o_pts = o_kb + align256(M * 8), o_avg = o_pts + align256(M * 16),
                     o_table = o_avg + align256(M * 8), o_starts = o_table + align256((T + 1) * 4),
                     total = o_starts + align256((T + 1) * 4);
        void* p;
        LRC_HIP(arena.get(total, &p));
        char* c = (char*)p;
        seg_start = (uint32_t*)c; seg_count = (uint32_t*)(c + o_count); seg_table = (uint64_t*)(c + o_tab);
        grids = (SegGrid*)(c + o_grid); boxes = (lrc_box*)(c + o_box); key_a = (uint64_t*)(c + o_ka);
        key_b = (uint64_t*)(c + o_kb); pts = (float4*)(c + o_pts); avg = (double*)(c + o_avg); table = (uint32_t*)(c + o_table);
        starts = (uint32_t*)(c + o_starts);
    }
    LRC_HIP(hipMemcpyAsync(seg_start, h_start.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
    LRC_HIP(hipMemcpyAsync(seg_count, h_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
    LRC_HIP(hipMemcpyAsync(seg_table, h_table.data(), (size_t)S * 8, hipMemcpyHostToDevice, st));
    LRC_HIP(hipMemsetAsync(table, 0, (T + 1) * 4, st));
    hipLaunchKernelGGL(box_grid_kernel, dim3(S), dim3(kBlock), 0, st, xyzl, rows_b, seg_start, seg_count, seg_table,
                       min_points, k, cell_size, grids, key_a, rows_a);
    LRC_HIP(hipGetLastError());
    const int end_bit2 = 32 + bit_width(S);
    size_t tmp2 = 0, tmp_scan = 0;
    // values: positions in instance order (rows_a, written by box_grid_kernel) -> keys_a (free since the first sort)
    LRC_HIP(rocprim::radix_sort_pairs(nullptr, tmp2, key_a, key_b, rows_a, keys_a, (size_t)M, 0, end_bit2, st));
    LRC_HIP(rocprim::exclusive_scan(nullptr, tmp_scan, table, starts, 0u, (size_t)(T + 1), rocprim::plus<uint32_t>(), st));
    void* tmpb;
    LRC_HIP(arena.get(std::max(tmp2, tmp_scan), &tmpb));
    LRC_HIP(rocprim::radix_sort_pairs(tmpb, tmp2, key_a, key_b, rows_a, keys_a, (size_t)M, 0, end_bit2, st));
    const uint32_t mblk = (uint32_t)((M + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(box_count_kernel, dim3(mblk), dim3(kBlock), 0, st, xyzl, key_b, keys_a, rows_b, M, grids, table, pts);
    LRC_HIP(hipGetLastError());
    LRC_HIP(rocprim::exclusive_scan(tmpb, tmp_scan, table, starts, 0u, (size_t)(T + 1), rocprim::plus<uint32_t>(), st));

    // ---- 3. neighbours, 4. statistics and boxes ----
    LRC_HIP(dispatch_knn(M, st, pts, key_b, grids, starts, (int)k, avg));
    hipLaunchKernelGGL(box_stats_kernel, dim3(S), dim3(kBlock), 0, st, xyzl, rows_b, avg, seg_start, seg_count, grids, min_points,
                       std_ratio, boxes, d_out_avg, d_out_keep);
    LRC_HIP(hipGetLastError());
    std::vector<lrc_box> h_boxes(S);
    LRC_HIP(hipMemcpyAsync(h_boxes.data(), boxes, (size_t)S * sizeof(lrc_box), hipMemcpyDeviceToHost, st));
    LRC_HIP(hipStreamSynchronize(st));
    uint64_t nb = 0;
    for (uint32_t s = 0; s < S; ++s) {
        if (h_counts[s] < min_points) continue;
        if (nb < capacity) {
            lrc_box b = h_boxes[s];
            b.sem = cl.id[h_ukeys[s] >> 16];
            b.ins = (uint16_t)(h_ukeys[s] & 0xFFFFu);
            out_boxes[nb] = b;
        }
        ++nb;
    }
    *out_num_boxes = nb;
    return LRC_OK;
}

int lrc_instance_boxes(lrc_ctx* ctx, const float* points3, const uint16_t* sem, const uint16_t* ins, uint64_t num_rows,
                       const uint16_t* class_ids, uint32_t num_classes, uint32_t min_points, uint32_t k, double std_ratio,
                       double cell_size, lrc_box* out_boxes, uint64_t capacity, uint64_t* out_num_boxes, double* out_avg,
                       uint8_t* out_keep) {
    if (!ctx || !out_num_boxes || (num_rows && (!points3 || !sem || !ins)) || (capacity && !out_boxes))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_instance_boxes: NULL argument");
    *out_num_boxes = 0;
    ClassList cl;
    if (int rc = check_params(num_rows, class_ids, num_classes, k, &cl)) return rc;
    if (num_rows == 0) return LRC_OK;
    std::vector<float> rows;
    try {
        rows.resize(4 * num_rows);
    } catch (const std::bad_alloc&) {
        return lrc_internal_fail(LRC_ERR_OOM, "lrc_instance_boxes: out of host memory");
    }
    for (uint64_t i = 0; i < num_rows; ++i) {
        std::memcpy(&rows[4 * i], &points3[3 * i], 12);
        const uint32_t lab = (uint32_t)sem[i] | ((uint32_t)ins[i] << 16);
        std::memcpy(&rows[4 * i + 3], &lab, 4);
    }
    LRC_HIP(hipSetDevice(ctx->device));
    float* d_rows = nullptr;
    double* d_avg = nullptr;
    uint8_t* d_keep = nullptr;
    int rc = LRC_OK;
    if (hipMalloc((void**)&d_rows, num_rows * 16) != hipSuccess ||
        (out_avg && hipMalloc((void**)&d_avg, num_rows * 8) != hipSuccess) ||
        (out_keep && hipMalloc((void**)&d_keep, num_rows) != hipSuccess)) {
        rc = lrc_internal_fail(LRC_ERR_OOM, "lrc_instance_boxes: out of device memory");
    } else if (hipMemcpy(d_rows, rows.data(), num_rows * 16, hipMemcpyHostToDevice) != hipSuccess) {
        rc = lrc_internal_fail(LRC_ERR_HIP, "lrc_instance_boxes: upload failed");
    } else if ((rc = lrc_instance_boxes_dev(ctx, d_rows, num_rows, class_ids, num_classes, min_points, k, std_ratio,
                                            cell_size, out_boxes, capacity, out_num_boxes, d_avg, d_keep, nullptr)) ==
               LRC_OK) {
        if (hipDeviceSynchronize() != hipSuccess ||
            (out_avg && hipMemcpy(out_avg, d_avg, num_rows * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
            (out_keep && hipMemcpy(out_keep, d_keep, num_rows, hipMemcpyDeviceToHost) != hipSuccess))
            rc = lrc_internal_fail(LRC_ERR_HIP, "lrc_instance_boxes: kernel or download failed");
    }
    if (d_rows) (void)hipFree(d_rows);
    if (d_avg) (void)hipFree(d_avg);
    if (d_keep) (void)hipFree(d_keep);
    return rc;
}

}  // extern "C"
