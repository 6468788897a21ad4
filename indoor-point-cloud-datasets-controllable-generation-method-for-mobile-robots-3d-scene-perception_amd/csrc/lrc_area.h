// lrc_area.h -- the quantised triangle area of DESIGN.md section 5e, one definition for every table that sums areas
// (lrc_coverage.hip, lrc_frameobj.hip): q = uint64(rint(area * 2^32)), area = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz),
// c = (v1 - v0) x (v2 - v0) component by component as a*b - c*d, float64, no contraction, correctly rounded sqrt.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// false (and q = 0) when area * 2^32 reaches 2^63; vertices are finite (checked on the host).
__device__ inline bool lrc_area_q(const double* __restrict__ v, const int32_t* __restrict__ f, uint64_t j, uint64_t* q) {
#pragma clang fp contract(off)                            // this body only: an including file keeps its own setting
    const uint64_t a = (uint32_t)f[3 * j], b = (uint32_t)f[3 * j + 1], c = (uint32_t)f[3 * j + 2];
    const double ux = v[3 * b] - v[3 * a], uy = v[3 * b + 1] - v[3 * a + 1], uz = v[3 * b + 2] - v[3 * a + 2];
    const double wx = v[3 * c] - v[3 * a], wy = v[3 * c + 1] - v[3 * a + 1], wz = v[3 * c + 2] - v[3 * a + 2];
    const double cx = uy * wz - uz * wy;
    const double cy = uz * wx - ux * wz;
    const double cz = ux * wy - uy * wx;
    const double area = 0.5 * __builtin_sqrt((cx * cx + cy * cy) + cz * cz);
    const double s = area * 4294967296.0;                 // exact: a power of two
    if (s < 9223372036854775808.0) {                      // 2^63
        *q = (uint64_t)__builtin_rint(s);
        return true;
    }
    *q = 0;
    return false;
}
