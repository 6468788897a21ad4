// lrc_metrics.hip -- point-cloud similarity metrics of the validation stage (gfx950).
//
// SURVEY.md section 8(f) row N3.  The reference evaluates generated clouds with three sampled metrics
// (evaluate_single_scene.py:55-111): Chamfer = mean(min_j |x_i - y_j|) + mean(min_i |x_i - y_j|) on 5 000-point
// samples, Hausdorff = max of the two directed maxima on 3 000-point samples, and MMD with an RBF kernel
// exp(-gamma |x-y|^2) on up to 10 000-point samples -- all as dense numpy distance matrices.  The two kernels
// below are the O(n*m) parts:
//   min_dist_kernel : for every row of A the distance to the nearest row of B   (Chamfer, Hausdorff)
//   rbf_sum_kernel  : sum_ij exp(-gamma * max(|a_i|^2 + |b_j|^2 - 2 a_i.b_j, 0))  (one term of the MMD)
// B is streamed through LDS in tiles; float32 distances as numpy computes them for float32 clouds, float64
// accumulation of the kernel sum.
// A NaN distance or kernel term reaches the result as np.min / np.maximum / np.exp carry it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "lrc_internal.h"

namespace {

constexpr int kTile = 1024;

// NaN is carried as numpy's min, maximum and exp carry it.  The device code is built with -fno-honor-nans: x != x is
// false there, min and max return their other operand and exp(NaN) is 0, so NaN is asked of the bits.  Finite
// coordinates (and a finite gamma) cannot give one, so the pair loops come in two forms: the plain one, and a checked one
// that a thread takes for a tile only if its own row of A or some row of B seen so far holds an infinity or a NaN.
constexpr uint32_t kInfBits = 0x7F800000u, kNanBits = 0x7FC00000u, kInfHi = 0x7FF00000u;
// Exponent all ones, asked with the sign shifted out: the masked form `(bits & inf) == inf` is read back by the
// compiler as a float class test, from which -fno-honor-nans then drops the NaN.
__device__ inline bool non_finite(float x) { return (__float_as_uint(x) << 1) >= (kInfBits << 1); }
// |x|'s high word: above kInfHi for a NaN (every NaN that float32 inputs and arithmetic on them give has a mantissa bit
// in this word), kInfHi for an infinity.
__device__ inline uint32_t abs_hi(double x) { return (uint32_t)__double2hiint(x) & 0x7FFFFFFFu; }

// kChecked: d2 is a sum of squares (+0, positive, +inf or NaN), on which the unsigned order of the bit patterns is the
// float order with every NaN above +inf.  The largest pattern seen is the sticky flag of np.min's NaN.
template <bool kChecked>
__device__ inline void min_dist_tile(const float* sb, uint32_t cnt, float ax, float ay, float az, float& best,
                                     uint32_t& worst) {
    for (uint32_t k = 0; k < cnt; ++k) {
        const float dx = ax - sb[3 * k], dy = ay - sb[3 * k + 1], dz = az - sb[3 * k + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;     // numpy: sum of squares, then one sqrt
        if (kChecked) {
            const uint32_t u = __float_as_uint(d2), b = __float_as_uint(best);
            best = __uint_as_float(u < b ? u : b);
            worst = u > worst ? u : worst;
        } else {
            best = d2 < best ? d2 : best;
        }
    }
}

__global__ __launch_bounds__(256) void min_dist_kernel(const float* A, uint64_t n, const float* B, uint64_t m,
                                                       float* out) {
    __shared__ float sb[kTile * 3];
    __shared__ uint32_t s_bad;                              // some row of B so far is not finite
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (i < n) { ax = A[3 * i]; ay = A[3 * i + 1]; az = A[3 * i + 2]; }
    const bool a_bad = non_finite(ax) | non_finite(ay) | non_finite(az);
    if (threadIdx.x == 0) s_bad = 0u;
    float best = __builtin_inff();
    uint32_t worst = 0u;
    for (uint64_t base = 0; base < m; base += kTile) {
        const uint32_t cnt = (uint32_t)((m - base) < (uint64_t)kTile ? (m - base) : (uint64_t)kTile);
        __syncthreads();
        bool b_bad = false;
        for (uint32_t k = threadIdx.x; k < cnt * 3; k += 256) {
            const float v = B[3 * base + k];
            sb[k] = v;
            b_bad |= non_finite(v);
        }
        if (b_bad) s_bad = 1u;                              // benign race: every writer stores 1
        __syncthreads();
        if (a_bad || s_bad) min_dist_tile<true>(sb, cnt, ax, ay, az, best, worst);
        else min_dist_tile<false>(sb, cnt, ax, ay, az, best, worst);
    }
    if (i < n) out[i] = worst > kInfBits ? __uint_as_float(kNanBits) : __builtin_sqrtf(best);
}

// kChecked: np.maximum(d2, 0) and np.exp carry a NaN into the sum, and -gamma * d2 is one more for 0 * inf; the largest
// |.| high word of both is the sticky flag.
template <bool kChecked>
__device__ inline void rbf_tile(const float* sb, uint32_t cnt, double ax, double ay, double az, double an, double gamma,
                                double& acc, uint32_t& worst) {
    for (uint32_t k = 0; k < cnt; ++k) {
        const double bx = sb[4 * k], by = sb[4 * k + 1], bz = sb[4 * k + 2];
        const double bn = (bx * bx + by * by) + bz * bz;
        double d2 = an + bn - 2.0 * ((ax * bx + ay * by) + az * bz);
        if (kChecked) {
            const uint32_t h = abs_hi(d2);
            worst = h > worst ? h : worst;
        }
        d2 = d2 > 0.0 ? d2 : 0.0;
        if (kChecked) {
            const uint32_t h = abs_hi(-gamma * d2);
            worst = h > worst ? h : worst;
        }
        acc += exp(-gamma * d2);
    }
}

__global__ __launch_bounds__(256) void rbf_sum_kernel(const float* A, uint64_t n, const float* B, uint64_t m,
                                                      double gamma, uint32_t gamma_bad, double* out_partial) {
    __shared__ float sb[kTile * 4];
    __shared__ double red[256];
    __shared__ uint32_t s_bad;                              // gamma, or some row of B so far, is not finite
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    double ax = 0, ay = 0, az = 0, an = 0;
    bool a_bad = false;
    if (i < n) {
        const float x = A[3 * i], y = A[3 * i + 1], z = A[3 * i + 2];
        a_bad = non_finite(x) | non_finite(y) | non_finite(z);
        ax = x; ay = y; az = z;
        an = (ax * ax + ay * ay) + az * az;
    }
    if (threadIdx.x == 0) s_bad = gamma_bad;
    double acc = 0.0;
    uint32_t worst = 0u;
    for (uint64_t base = 0; base < m; base += kTile) {
        const uint32_t cnt = (uint32_t)((m - base) < (uint64_t)kTile ? (m - base) : (uint64_t)kTile);
        __syncthreads();
        bool b_bad = false;
        for (uint32_t k = threadIdx.x; k < cnt; k += 256) {
            const float x = B[3 * (base + k)], y = B[3 * (base + k) + 1], z = B[3 * (base + k) + 2];
            sb[4 * k] = x; sb[4 * k + 1] = y; sb[4 * k + 2] = z;
            b_bad |= non_finite(x) | non_finite(y) | non_finite(z);
        }
        if (b_bad) s_bad = 1u;                              // benign race: every writer stores 1
        __syncthreads();
        if (i < n) {
            if (a_bad || s_bad) rbf_tile<true>(sb, cnt, ax, ay, az, an, gamma, acc, worst);
            else rbf_tile<false>(sb, cnt, ax, ay, az, an, gamma, acc, worst);
        }
    }
    red[threadIdx.x] = worst > kInfHi ? __longlong_as_double(0x7FF8000000000000ll) : acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out_partial[blockIdx.x] = red[0];
}

}  // namespace

extern "C" {

int lrc_min_distances(lrc_ctx* ctx, const float* a3, uint64_t n, const float* b3, uint64_t m, float* out_min) {
    if (!ctx || (n && (!a3 || !out_min)) || (m && !b3))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_min_distances: NULL argument");
    if (n == 0) return LRC_OK;
    if (m == 0) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_min_distances: the target cloud is empty");
    LRC_HIP(hipSetDevice(ctx->device));
    Buf da, db, dout;
    LRC_HIP(hipMalloc(&da.p, n * 12));
    LRC_HIP(hipMalloc(&db.p, m * 12));
    LRC_HIP(hipMalloc(&dout.p, n * 4));
    LRC_HIP(hipMemcpy(da.p, a3, n * 12, hipMemcpyHostToDevice));
    LRC_HIP(hipMemcpy(db.p, b3, m * 12, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(min_dist_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, nullptr, (const float*)da.p, n,
                       (const float*)db.p, m, (float*)dout.p);
    LRC_HIP(hipGetLastError());
    LRC_HIP(hipDeviceSynchronize());
    LRC_HIP(hipMemcpy(out_min, dout.p, n * 4, hipMemcpyDeviceToHost));
    return LRC_OK;
}

int lrc_rbf_kernel_sum(lrc_ctx* ctx, const float* a3, uint64_t n, const float* b3, uint64_t m, double gamma,
                       double* out_sum) {
    if (!ctx || !out_sum || (n && !a3) || (m && !b3))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_rbf_kernel_sum: NULL argument");
    *out_sum = 0.0;
    if (n == 0 || m == 0) return LRC_OK;
    LRC_HIP(hipSetDevice(ctx->device));
    const uint32_t nblk = (uint32_t)((n + 255) / 256);
    Buf da, db, dp;
    LRC_HIP(hipMalloc(&da.p, n * 12));
    LRC_HIP(hipMalloc(&db.p, m * 12));
    LRC_HIP(hipMalloc(&dp.p, (size_t)nblk * 8));
    LRC_HIP(hipMemcpy(da.p, a3, n * 12, hipMemcpyHostToDevice));
    LRC_HIP(hipMemcpy(db.p, b3, m * 12, hipMemcpyHostToDevice));
    // asked on the host: the device build drops the NaN from its own float class tests
    const uint32_t gamma_bad = std::isfinite(gamma) ? 0u : 1u;
    hipLaunchKernelGGL(rbf_sum_kernel, dim3(nblk), dim3(256), 0, nullptr, (const float*)da.p, n, (const float*)db.p, m,
                       gamma, gamma_bad, (double*)dp.p);
    LRC_HIP(hipGetLastError());
    LRC_HIP(hipDeviceSynchronize());
    double* part = new (std::nothrow) double[nblk];
    if (!part) return lrc_internal_fail(LRC_ERR_OOM, "lrc_rbf_kernel_sum: out of host memory");
    hipError_t e = hipMemcpy(part, dp.p, (size_t)nblk * 8, hipMemcpyDeviceToHost);
    double s = 0.0;
    for (uint32_t k = 0; k < nblk; ++k) s += part[k];
    delete[] part;
    if (e != hipSuccess) return lrc_internal_fail(LRC_ERR_HIP, "lrc_rbf_kernel_sum: download failed");
    *out_sum = s;
    return LRC_OK;
}

}  // extern "C"
