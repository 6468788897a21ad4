// lrc_echo.hip -- host side of the beam footprint and multi-echo returns (lrc_echo.h): the argument checks, the entry points
// lrc_scan_echoes_dev / lrc_scan_echoes_compact (the trace launch and the frame path are lidarcast.hip's: echo_scan_dev,
// echo_scan_compact, which also gathers the kept rows' weights), the host reduction lrc_echo_reduce and the device test hook
// lrc_internal_echo_lanes_dev (reduce_lanes on the caller's rows, without a traversal in front of it).
#include <cmath>

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

constexpr int kLanesBlock = 256;      // whole waves

// lrc_internal_echo_lanes_dev: lrcecho::reduce_lanes on rows of the caller's, in the trace kernel's lane layout -- lane
// gid = beam * G + k, the `gid >= lanes` exit takes whole groups (lanes = num_beams * G), every other lane of the wave reaches
// the reduction.  Lane k < K with t < +inf holds a hit of slot k and label beam * K + k; every other lane is a sub-ray without
// a hit, whose range (0 for the lanes k >= K) must not count.
__global__ __launch_bounds__(kLanesBlock) void echo_lanes_kernel(const float* __restrict__ t, uint64_t lanes, lrcecho::Params q,
                                                                 int32_t* __restrict__ rep, float* __restrict__ range,
                                                                 uint32_t* __restrict__ label) {
    const uint64_t gid = (uint64_t)blockIdx.x * kLanesBlock + threadIdx.x;
    if (gid >= lanes) return;
    const uint32_t tid = threadIdx.x & 63u, K = q.subrays;
    const uint32_t k = tid & ((1u << q.group_log2) - 1u);
    const uint64_t beam = gid >> q.group_log2;
    const float tk = k < K ? t[beam * K + k] : 0.0f;
    const bool hit = (k < K) & (tk < __builtin_inff());
    lrcecho::reduce_lanes(q, tid, gid, tk, hit ? k : 0xFFFFFFFFu, (uint32_t)(beam * K + k),
                          [&](uint64_t, uint64_t rec, float t_e, uint32_t slot_e, uint32_t label_e) {
        rep[rec] = slot_e == 0xFFFFFFFFu ? -1 : (int32_t)slot_e;
        range[rec] = t_e;
        label[rec] = label_e;
    });
}

}  // namespace

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

// test hook: the device reduction alone.  d_t (num_beams, K) float32; d_rep / d_range / d_label (num_beams, E): the representative
// sub-ray of echo e (-1: empty slot), its range (+inf) and its label beam * K + rep (an empty slot's label is not specified);
// d_weight (num_beams, E), nullable as lrcecho::Params::weight is.  Enqueued on `stream`, no host synchronisation.
int lrc_internal_echo_lanes_dev(lrc_ctx* ctx, const float* d_t, uint64_t num_beams, const lrc_beam* beam, int32_t* d_rep,
                                float* d_range, uint32_t* d_label, uint8_t* d_weight, void* stream) {
    lrcecho::Params ep;
    int rc = check_beam("lrc_internal_echo_lanes_dev", beam, &ep);
    if (rc) return rc;
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_internal_echo_lanes_dev: ctx is NULL");
    if (num_beams && (!d_t || !d_rep || !d_range || !d_label))
        return fail(LRC_ERR_INVALID_ARG, "lrc_internal_echo_lanes_dev: NULL argument");
    if (num_beams > 0xFFFFFFFFull / beam->subrays)
        return fail(LRC_ERR_INVALID_ARG, "lrc_internal_echo_lanes_dev: num_beams * subrays must stay below 2^32 (the label)");
    if (!num_beams) return LRC_OK;
    LRC_HIP(hipSetDevice(ctx->device));
    ep.weight = d_weight;
    const uint64_t lanes = num_beams << ep.group_log2;
    echo_lanes_kernel<<<dim3((unsigned)blocks_of(lanes, kLanesBlock)), dim3(kLanesBlock), 0, (hipStream_t)stream>>>(
        d_t, lanes, ep, d_rep, d_range, d_label);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

}  // extern "C"
