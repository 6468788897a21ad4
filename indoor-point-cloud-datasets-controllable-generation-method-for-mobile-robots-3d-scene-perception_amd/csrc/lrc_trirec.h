// lrc_trirec.h -- the arithmetic the two scene builders (bvh_build.cpp on the host, lrc_bvh_device.hip on the device) and the
// refit of a deformable scene (lrc_deform.h) share, written once: the order-preserving float32 <-> int32 encoding that makes
// box min / max associative and commutative, and the 48-byte triangle record with its slot box.
//
//   enc / dec   float32 bits <-> int32 with the same order, -0.0 below +0.0 (an involution on all bit patterns)
//   tmin / tmax min / max of two float32 under that total order: a box plane does not depend on the order its members arrive in
//   tri_record  v0, e1 = v0 - v1, e2 = v2 - v0, Ng = cross(e2, e1) with component = fma(a_j, b_k, -(a_k * b_j)), and the
//               triangle's exact vertex box (lo xyz, hi xyz)
// float32, one rounding per operation (the build is -ffp-contract=off); the fma of Ng is asked for by name.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LRC_THD __host__ __device__ __forceinline__
#else
#define LRC_THD inline
#endif

namespace lrctri {

LRC_THD int enc(float f) { int i; __builtin_memcpy(&i, &f, 4); return i ^ ((i >> 31) & 0x7FFFFFFF); }
LRC_THD float dec(int i) { i ^= (i >> 31) & 0x7FFFFFFF; float f; __builtin_memcpy(&f, &i, 4); return f; }
LRC_THD int imin(int a, int b) { return a < b ? a : b; }
LRC_THD int imax(int a, int b) { return a > b ? a : b; }
LRC_THD float tmin(float a, float b) { return dec(imin(enc(a), enc(b))); }
LRC_THD float tmax(float a, float b) { return dec(imax(enc(a), enc(b))); }

// rec: 12 floats (v0, e1, e2, Ng); box: 6 floats (lo xyz, hi xyz)
LRC_THD void tri_record(const float* v0, const float* v1, const float* v2, float* rec, float* box) {
    float a[3], b[3], c[3], e1[3], e2[3];
    for (int k = 0; k < 3; ++k) { a[k] = v0[k]; b[k] = v1[k]; c[k] = v2[k]; e1[k] = a[k] - b[k]; e2[k] = c[k] - a[k]; }
    for (int k = 0; k < 3; ++k) { rec[k] = a[k]; rec[3 + k] = e1[k]; rec[6 + k] = e2[k]; }
    rec[9] = __builtin_fmaf(e2[1], e1[2], -(e2[2] * e1[1]));
    rec[10] = __builtin_fmaf(e2[2], e1[0], -(e2[0] * e1[2]));
    rec[11] = __builtin_fmaf(e2[0], e1[1], -(e2[1] * e1[0]));
    for (int k = 0; k < 3; ++k) {
        box[k] = dec(imin(imin(enc(a[k]), enc(b[k])), enc(c[k])));
        box[3 + k] = dec(imax(imax(enc(a[k]), enc(b[k])), enc(c[k])));
    }
}

}  // namespace lrctri
