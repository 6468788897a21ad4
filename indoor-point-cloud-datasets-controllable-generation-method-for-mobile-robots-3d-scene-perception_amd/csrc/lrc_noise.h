// lrc_noise.h -- the seeded sensor noise of lrc_scan_noisy_* (include/lidarcast.h "seeded sensor noise", DESIGN.md
// section 5h): a counter-based generator and a table-driven normal quantile, the same integer and float32 operations on
// the host and in the trace kernel, no transcendental function.  The noise of a ray is a pure function of
// (seed, frame id, ray index): nothing is drawn in call order, nothing crosses PCIe.
//
//   words   Philox4x32-10, key = (seed lo, seed hi), counter = (ray index, frame lo, frame hi, 0) with
//           frame = first_frame + pose (64 bit).  One block per ray: w0 range, w1 azimuth jitter, w2 elevation jitter,
//           w3 dropout.
//   normal  from ONE word: sign = w >> 31, r = w & 0x7FFFFFFF is the two-sided tail probability q = r / 2^31 of |z|.
//           r < 128: |z| = B[23][0] (the clamp, 5.42).  Else with L the leading one of r (7..30): e = 30 - L the octave of
//           q, below = r - 2^L, c = below >> (L - 6) the cell (64 per octave), f = (below mod 2^(L-6)) * 2^-(L-6) the place
//           in the cell (exact in float32: at most 24 bits), |z| = fmaf(f, D[e][c], B[e][c]).
//           B[e][c] = float32(Phi^-1(1 - q/2)) at q = 2^-(e+1) (1 + c/64); D[e][c] = (next cell's B) - B[e][c] in float32,
//           the cell behind c = 63 being B[e-1][0] (0 for e = 0).  Linear interpolation in q over a cell of relative width
//           1/64: the error is at most h^2/8 max|g''| <= (1/64)^2 / 8 * 1.5 = 4.6e-5 with g(u) = Phi^-1(1 - 2^(u-1)).
//   table   built on the host in float64 (lrc_noise.hip), 2 x 1536 float32 = 12 KB, uploaded once per context.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LRC_NHD __host__ __device__ __forceinline__
#else
#define LRC_NHD inline
#endif

namespace lrcnoise {

constexpr int kOctaves = 24, kCells = 64, kTable = kOctaves * kCells;   // 1536 entries each of base and slope

struct Words { uint32_t w0, w1, w2, w3; };

// what the trace kernel needs of an lrc_noise (kGenNoisy, kGenNoisySweeps): a zero range_std, angle_std or drop_thr skips its step
struct Params {
    uint64_t seed, first_frame;
    double angle_std;        // radians
    const float* tab;        // device: base[kTable] | slope[kTable]
    float range_std;         // metres, float32(lrc_noise::range_std)
    uint32_t drop_thr;       // drop_threshold(lrc_noise::dropout)
};

LRC_NHD Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Words{c0, c1, c2, c3};
}

// the block of ray i of frame `frame` under `seed`
LRC_NHD Words ray_words(uint64_t seed, uint64_t frame, uint32_t i) {
    return philox4x32_10(i, (uint32_t)frame, (uint32_t)(frame >> 32), 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

LRC_NHD float bits_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    union { uint32_t u; float f; } v; v.u = u; return v.f;
#endif
}

LRC_NHD uint32_t float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    union { uint32_t u; float f; } v; v.f = f; return v.u;
#endif
}

// standard normal variate of one word; tab = base[kTable] followed by slope[kTable]
LRC_NHD float normal_of(uint32_t w, const float* tab) {
    const uint32_t r = w & 0x7FFFFFFFu;
    float a;
    if (r < 128u) {
        a = tab[(kOctaves - 1) * kCells];
    } else {
        const uint32_t L = 31u - (uint32_t)__builtin_clz(r), sh = L - 6u;
        const uint32_t below = r - (1u << L);
        const uint32_t idx = (30u - L) * kCells + (below >> sh);
        const float f = (float)(below & ((1u << sh) - 1u)) * bits_float((127u - sh) << 23);
        a = __builtin_fmaf(f, tab[kTable + idx], tab[idx]);
    }
    return bits_float((w & 0x80000000u) | float_bits(a));       // the word's top bit is the sign
}

// dropout threshold of probability p in [0, 1): a ray is dropped iff w3 < thr
inline uint32_t drop_threshold(double p) {
    const double v = p * 4294967296.0;
    return v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
}

// Angle jitter in the sensor frame on a float64 table row (a, b, c): dp, dt the azimuth and elevation offsets in radians.
// The row moves along its azimuth tangent (-b, a, 0) and its elevation tangent (-c a/h, -c b/h, h), h = sqrt(a^2 + b^2), and
// is normalised again.  One float64 operation per step in exactly this order (built with -ffp-contract=off; numpy restates
// it in tests/noise_restate.py).  A row with h == 0 (straight up or down: no azimuth) is left as it is.
LRC_NHD void jitter_row(double& a, double& b, double& c, double dp, double dt) {
    const double h = __builtin_sqrt(a * a + b * b);
    if (h == 0.0) return;
    const double ca = (c * a) / h, cb = (c * b) / h;
    const double a1 = (a - dp * b) - dt * ca;
    const double b1 = (b + dp * a) - dt * cb;
    const double c1 = c + dt * h;
    const double n = __builtin_sqrt((a1 * a1 + b1 * b1) + c1 * c1);
    a = a1 / n; b = b1 / n; c = c1 / n;
}

}  // namespace lrcnoise
