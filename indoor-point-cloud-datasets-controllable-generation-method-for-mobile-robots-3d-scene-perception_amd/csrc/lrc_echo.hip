// lrc_echo.hip -- host side of the beam footprint and multi-echo returns (lrc_echo.h): the argument checks, the entry points
// lrc_scan_echoes_dev / lrc_scan_echoes_compact (the trace launch and the frame path are lidarcast.hip's: echo_scan_dev,
// echo_scan_compact), the gather of the kept rows' weights and the host reduction lrc_echo_reduce.
#include <cmath>
#include <vector>

#include "lrc_internal.h"
#include "lrc_echo.h"

namespace {

// checks an lrc_beam (LRC_ERR_INVALID_ARG, `who` prefixes the message) and fills what the kernel needs of it
int check_beam(const char* who, const lrc_beam* b, lrcecho::Params* out) {
    auto bad = [&](const char* m) { return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + m); };
    if (!b) return bad("beam is NULL");
    if (b->subrays < 1 || b->subrays > lrcecho::kMaxSubrays) return bad("subrays must lie in [1, 16]");
    if (b->max_echoes < 1 || b->max_echoes > lrcecho::kMaxEchoes) return bad("max_echoes must lie in [1, 4]");
    if (b->min_count < 1 || b->min_count > b->subrays) return bad("min_count must lie in [1, subrays]");
    if (!std::isfinite(b->separation) || !(b->separation > 0.0f)) return bad("separation must be finite and positive");
    if (out) {
        *out = lrcecho::Params{};
        out->separation = b->separation;
        out->subrays = (uint8_t)b->subrays;
        out->group_log2 = (uint8_t)lrcecho::group_log2_of(b->subrays, b->max_echoes);
        out->max_echoes = (uint8_t)b->max_echoes;
        out->min_count = (uint8_t)b->min_count;
    }
    return LRC_OK;
}

// row r of the compacted arrays belongs to the pose whose run [prefix[p], prefix[p + 1]) holds it; its record is that pose's
// index[r]-th.  One thread per row; the prefix is small (P + 1 values) and searched by bisection.
__global__ __launch_bounds__(256) void echo_gather_kernel(const uint64_t* __restrict__ prefix, uint32_t P,
                                                          const uint32_t* __restrict__ index, const uint8_t* __restrict__ weight,
                                                          uint64_t records_per_pose, uint64_t rows, uint8_t* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= rows) return;
    uint32_t lo = 0, hi = P;           // prefix[lo] <= r < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= r) lo = mid; else hi = mid;
    }
    const uint32_t i = index[r];
    out[r] = i < records_per_pose ? weight[(uint64_t)lo * records_per_pose + i] : (uint8_t)0;
}

}  // namespace

#pragma GCC visibility push(hidden)
int echo_gather_rows(lrc_ctx* ctx, const uint64_t* counts, uint64_t P, const uint32_t* d_index, const uint8_t* d_weight,
                     uint64_t records_per_pose, uint64_t rows, uint8_t* weight_rows) {
    (void)ctx;
    if (!rows) return LRC_OK;
    if (P > 0x7FFFFFFFull || blocks_of(rows, 256) > 0x7FFFFFFFull)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_compact: too many poses or rows for the weight gather");
    std::vector<uint64_t> prefix(P + 1, 0);
    for (uint64_t p = 0; p < P; ++p) prefix[p + 1] = prefix[p] + counts[p];
    if (prefix[P] != rows) return fail(LRC_ERR_INTERNAL, "lrc_scan_echoes_compact: counts do not add up to the kept rows");
    Buf d_prefix, d_out;
    LRC_HIP(hipMalloc(&d_prefix.p, (P + 1) * 8));
    LRC_HIP(hipMalloc(&d_out.p, rows));
    LRC_HIP(hipMemcpy(d_prefix.p, prefix.data(), (P + 1) * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(echo_gather_kernel, dim3((uint32_t)blocks_of(rows, 256)), dim3(256), 0, nullptr,
                       (const uint64_t*)d_prefix.p, (uint32_t)P, d_index, d_weight, records_per_pose, rows, (uint8_t*)d_out.p);
    LRC_HIP(hipGetLastError());
    LRC_HIP(hipMemcpy(weight_rows, d_out.p, rows, hipMemcpyDeviceToHost));
    return LRC_OK;
}
#pragma GCC visibility pop

extern "C" {

int lrc_scan_echoes_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N,
                        const double* d_offsets2, const lrc_beam* beam, double max_range, const lrc_hits* d_out,
                        uint8_t* d_weight, void* stream) {
    // what needs no scene is checked first
    lrcecho::Params ep;
    int rc = check_beam("lrc_scan_echoes_dev", beam, &ep);
    if (rc) return rc;
    if (d_out && d_out->tile_count)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_dev: tile_count must be NULL (a wave does not write 64 consecutive records)");
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_dev: NULL scene or output");
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_dev: a range_noise option is set");
    if (P && N && (!d_poses16 || !d_dirs3 || !d_offsets2))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_dev: poses16, dirs3 or offsets2 is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    ep.offsets2 = d_offsets2;
    ep.weight = d_weight;
    return echo_scan_dev(s, d_poses16, P, d_dirs3, N, ep, max_range, d_out, (hipStream_t)stream);
}

int lrc_scan_echoes_compact(lrc_scene* s, const double* poses16, uint64_t P, const lrc_table* table, const double* offsets2,
                            const lrc_beam* beam, double max_range, const lrc_frames* out, uint8_t* weight_rows,
                            uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    // what needs no scene is checked first, and for an empty call too
    lrcecho::Params ep;
    int rc = check_beam("lrc_scan_echoes_compact", beam, &ep);
    if (rc) return rc;
    if (!offsets2) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_compact: offsets2 is NULL");
    for (uint32_t k = 0; k < 2u * beam->subrays; ++k)
        if (!std::isfinite(offsets2[k])) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_compact: non-finite offset");
    if (!s || !out || !table) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_compact: NULL scene, table or output");
    if (table->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_compact: table and scene belong to different contexts");
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_compact: a range_noise option is set");
    if (!(P * table->n)) return LRC_OK;
    if (!poses16 || !out->counts) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_compact: poses16 or counts is NULL");
    if (table->n * (uint64_t)beam->max_echoes > 0xFFFFFFFFull)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_echoes_compact: rays_per_pose * max_echoes must stay below 2^32 (the index column)");
    LRC_HIP(hipSetDevice(s->ctx->device));
    return echo_scan_compact(s, poses16, P, table, offsets2, ep, max_range, out, weight_rows, capacity, out_total);
}

int lrc_echo_reduce(const float* t, uint64_t num_beams, const lrc_beam* beam, int32_t* out_rep, uint8_t* out_weight) {
    int rc = check_beam("lrc_echo_reduce", beam, nullptr);
    if (rc) return rc;
    if (num_beams && (!t || !out_rep || !out_weight)) return fail(LRC_ERR_INVALID_ARG, "lrc_echo_reduce: NULL argument");
    const uint32_t K = beam->subrays, E = beam->max_echoes;
    for (uint64_t b = 0; b < num_beams; ++b)
        lrcecho::reduce_beam(t + b * K, K, E, beam->min_count, beam->separation, out_rep + b * E, out_weight + b * E);
    return LRC_OK;
}

}  // extern "C"
