// lrc_noise.hip -- host side of the seeded sensor noise (lrc_noise.h): the quantile table, the argument checks, the
// resident copy of the table, the host evaluation of the draws (lrc_noise_draws: what the kernel draws, without a GPU) and
// the two test hooks that put a chosen counter, key or word in front of the generator: lrc_internal_noise_words on the host,
// lrc_internal_noise_words_dev on the device.
#include <cmath>

#include "lrc_internal.h"
#include "lrc_noise.h"

namespace {

// z with P(Z > z) = t for 0 < t < 0.5, float64: Newton's iteration on 0.5 erfc(z / sqrt 2) - t from z = 0.  The function is
// convex and decreasing on z >= 0, so the iterates rise monotonically to the root; the last steps are rounding noise.
double upper_quantile(double t) {
    constexpr double kInvSqrt2 = 0.70710678118654752440, kInvSqrt2Pi = 0.39894228040143267794;
    double z = 0.0;
    for (int it = 0; it < 200; ++it) {
        const double f = 0.5 * std::erfc(z * kInvSqrt2) - t;
        const double dz = f / (kInvSqrt2Pi * std::exp(-0.5 * z * z));
        z += dz;
        if (std::fabs(dz) <= 1e-16 * z) break;
    }
    return z;
}

struct Table {
    float v[2 * lrcnoise::kTable];      // base | slope
    Table() {
        using namespace lrcnoise;
        for (int e = 0; e < kOctaves; ++e)
            for (int c = 0; c < kCells; ++c)
                v[e * kCells + c] = (float)upper_quantile(0.5 * std::ldexp(1.0 + c / 64.0, -(e + 1)));
        for (int e = 0; e < kOctaves; ++e)
            for (int c = 0; c < kCells; ++c) {
                const float next = c + 1 < kCells ? v[e * kCells + c + 1] : (e > 0 ? v[(e - 1) * kCells] : 0.0f);
                v[kTable + e * kCells + c] = next - v[e * kCells + c];
            }
    }
};

const float* host_table() {
    static const Table t;      // built on first use, thread-safe
    return t.v;
}

int check_noise(const char* who, const lrc_noise* nz, uint64_t N) {
    auto bad = [&](const char* m) { return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + m); };
    if (!nz) return bad("noise is NULL");
    if (!(nz->range_std >= 0.0) || !std::isfinite(nz->range_std)) return bad("range_std must be finite and not negative");
    if (!(nz->angle_std >= 0.0) || !std::isfinite(nz->angle_std)) return bad("angle_std must be finite and not negative");
    if (!(nz->dropout >= 0.0 && nz->dropout < 1.0)) return bad("dropout must lie in [0, 1)");
    if (N > 0xFFFFFFFFull) return bad("at most 2^32 - 1 rays per pose (the ray index is one counter word)");
    return LRC_OK;
}

// the context's resident copy of the table, uploaded on first use
int resident_table(lrc_ctx* ctx) {
    if (!ctx->d_noise_tab) {
        float* d = nullptr;
        LRC_HIP(hipMalloc((void**)&d, sizeof(float) * 2 * lrcnoise::kTable));
        const hipError_t e = hipMemcpy(d, host_table(), sizeof(float) * 2 * lrcnoise::kTable, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); LRC_HIP(e); }
        ctx->d_noise_tab = d;
    }
    return LRC_OK;
}

// lrc_internal_noise_words_dev: block j of n -- philox4x32_10 of the caller's counter and key (ctr4 != NULL: words4 is written)
// or the caller's words (ctr4 == NULL: words4 is read), and the variate of each of its four words from the resident table
__global__ __launch_bounds__(kBlock) void noise_words_kernel(const uint32_t* __restrict__ ctr4, const uint32_t* __restrict__ key2,
                                                             uint64_t n, uint32_t* words4, float* __restrict__ z4,
                                                             const float* __restrict__ tab) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    uint32_t* w4 = words4 + j * 4;
    lrcnoise::Words w;
    if (ctr4) {
        const uint32_t* c = ctr4 + j * 4;
        w = lrcnoise::philox4x32_10(c[0], c[1], c[2], c[3], key2[j * 2], key2[j * 2 + 1]);
        w4[0] = w.w0; w4[1] = w.w1; w4[2] = w.w2; w4[3] = w.w3;
    } else {
        w = lrcnoise::Words{w4[0], w4[1], w4[2], w4[3]};
    }
    if (z4) {
        float* z = z4 + j * 4;
        z[0] = lrcnoise::normal_of(w.w0, tab);
        z[1] = lrcnoise::normal_of(w.w1, tab);
        z[2] = lrcnoise::normal_of(w.w2, tab);
        z[3] = lrcnoise::normal_of(w.w3, tab);
    }
}

}  // namespace

#pragma GCC visibility push(hidden)
int noise_params(lrc_ctx* ctx, const char* who, const lrc_noise* nz, uint64_t N, lrcnoise::Params* out) {
    int rc = check_noise(who, nz, N);
    if (rc) return rc;
    rc = resident_table(ctx);
    if (rc) return rc;
    out->seed = nz->seed;
    out->first_frame = nz->first_frame;
    out->angle_std = nz->angle_std;
    out->tab = ctx->d_noise_tab;
    out->range_std = (float)nz->range_std;
    out->drop_thr = lrcnoise::drop_threshold(nz->dropout);
    return LRC_OK;
}

int noise_params_host(const char* who, const lrc_noise* nz, uint64_t N, lrcnoise::Params* out) {
    int rc = check_noise(who, nz, N);
    if (rc) return rc;
    out->seed = nz->seed;
    out->first_frame = nz->first_frame;
    out->angle_std = nz->angle_std;
    out->tab = host_table();
    out->range_std = (float)nz->range_std;
    out->drop_thr = lrcnoise::drop_threshold(nz->dropout);
    return LRC_OK;
}
#pragma GCC visibility pop

extern "C" {

int lrc_noise_table(float* base1536, float* slope1536) {
    const float* t = host_table();
    for (int k = 0; k < lrcnoise::kTable; ++k) {
        if (base1536) base1536[k] = t[k];
        if (slope1536) slope1536[k] = t[lrcnoise::kTable + k];
    }
    return LRC_OK;
}

int lrc_noise_draws(const lrc_noise* nz, uint64_t P, uint64_t N, float* z_range, float* z_az, float* z_el, uint8_t* keep) {
    int rc = check_noise("lrc_noise_draws", nz, N);
    if (rc) return rc;
    const float* t = host_table();
    const uint32_t thr = lrcnoise::drop_threshold(nz->dropout);
    for (uint64_t p = 0; p < P; ++p)
        for (uint64_t i = 0; i < N; ++i) {
            const lrcnoise::Words w = lrcnoise::ray_words(nz->seed, nz->first_frame + p, (uint32_t)i);
            const uint64_t k = p * N + i;
            if (z_range) z_range[k] = lrcnoise::normal_of(w.w0, t);
            if (z_az) z_az[k] = lrcnoise::normal_of(w.w1, t);
            if (z_el) z_el[k] = lrcnoise::normal_of(w.w2, t);
            if (keep) keep[k] = (uint8_t)(w.w3 >= thr);
        }
    return LRC_OK;
}

// test hook: one Philox4x32-10 block for any counter and key (the known answers), and the variate of any word
int lrc_internal_noise_words(const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4, float* z4) {
    if (!ctr4 || !key2 || !out4) return fail(LRC_ERR_INVALID_ARG, "lrc_internal_noise_words: NULL argument");
    const lrcnoise::Words w = lrcnoise::philox4x32_10(ctr4[0], ctr4[1], ctr4[2], ctr4[3], key2[0], key2[1]);
    out4[0] = w.w0; out4[1] = w.w1; out4[2] = w.w2; out4[3] = w.w3;
    if (z4) for (int k = 0; k < 4; ++k) z4[k] = lrcnoise::normal_of(out4[k], host_table());
    return LRC_OK;
}

// test hook: the device twin of lrc_internal_noise_words for n blocks.  d_ctr4 (n, 4) and d_key2 (n, 2): d_words4 (n, 4)
// receives the Philox blocks; d_ctr4 NULL: d_words4 is the input (any word can be put in front of normal_of).  d_z4 (n, 4),
// nullable: the variates of the words from the context's resident table.  Enqueued on `stream`, no host synchronisation.
int lrc_internal_noise_words_dev(lrc_ctx* ctx, const uint32_t* d_ctr4, const uint32_t* d_key2, uint64_t n, uint32_t* d_words4,
                                 float* d_z4, void* stream) {
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_internal_noise_words_dev: ctx is NULL");
    if (!n) return LRC_OK;
    if (!d_words4 || (d_ctr4 && !d_key2)) return fail(LRC_ERR_INVALID_ARG, "lrc_internal_noise_words_dev: NULL argument");
    if (n > 0x7FFFFFFFull * kBlock) return fail(LRC_ERR_INVALID_ARG, "lrc_internal_noise_words_dev: too many blocks for one launch");
    LRC_HIP(hipSetDevice(ctx->device));
    int rc = resident_table(ctx);
    if (rc) return rc;
    noise_words_kernel<<<dim3((unsigned)blocks_of(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream>>>(
        d_ctr4, d_key2, n, d_words4, d_z4, ctx->d_noise_tab);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

}  // extern "C"
