// lrc_movers.hip -- host side of the moving objects (lrc_movers.h): the mover set, the checks of the eight scan entry points
// lrc_scan_movers_*, lrc_scan_noisy_movers_*, lrc_scan_mover_sweeps_* and lrc_scan_noisy_mover_sweeps_* (the kernels, the launches
// and the frame path are lidarcast.hip's: movers_scan_dev, movers_scan_compact) and the host functions lrc_mover_rays,
// lrc_mover_merge, lrc_mover_sweep_rays and lrc_mover_sweep_normals, which run the inline functions the kernels call on arrays.
#include <cmath>

#include "lrc_internal.h"
#include "lrc_movers.h"

// the checks lrc_scan_movers_* and lrc_scan_flow_* share (declared in lrc_internal.h); `set` may be NULL
int check_call(const char* who, const lrc_scene* s, const lrc_movers* set, const void* out) {
    auto bad = [&](const char* t) { return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + t); };
    if (!s || !out) return bad("NULL scene or output");
    if (set) {
        if (set->ctx != s->ctx) return bad("movers and scene belong to different contexts");
        for (const lrc_scene* m : set->scenes)
            if (m == s) return bad("the static scene is one of its own movers");
    }
    if (s->opts.range_noise) return bad("a range_noise option is set");
    return LRC_OK;
}

// one host pose12 `q`, named `what` k in the message: every entry finite, max |R^T R - I| <= 2^-16 in float64
static int check_pose12(const char* who, const char* what, uint64_t k, const float* q) {
    for (int e = 0; e < 12; ++e)
        if (!std::isfinite(q[e]))
            return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + what + " " + std::to_string(k) + " has an entry that is not finite");
    double worst = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double dot = 0.0;
            for (int r = 0; r < 3; ++r) dot += (double)q[4 * r + a] * (double)q[4 * r + b];
            worst = std::fmax(worst, std::fabs(dot - (a == b ? 1.0 : 0.0)));
        }
    if (worst > lrcmov::kOrthoTol)
        return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + what + " " + std::to_string(k) + " is no rotation: max |R^T R - I| = " +
                                             std::to_string(worst) + " > 2^-16");
    return LRC_OK;
}

// host-pose entry point: every entry finite, max |R^T R - I| <= 2^-16 in float64
int check_poses12(const char* who, const float* m, uint64_t count) {
    for (uint64_t k = 0; k < count; ++k) {
        const int rc = check_pose12(who, "mover pose", k, m + k * 12);
        if (rc) return rc;
    }
    return LRC_OK;
}

// host mover sweep records (count x 24 float32): every entry finite, the start pose a rotation as check_poses12 asks, dq.w >=
// cos(pi/4) (at most pi/2 per sweep, where the nlerp error table of include/lidarcast.h holds)
static int check_motion24(const char* who, const float* m, uint64_t count) {
    constexpr double kCosQuarterPi = 0.70710678118654752440;
    for (uint64_t k = 0; k < count; ++k) {
        const float* r = m + k * 24;
        for (int e = 12; e < 24; ++e)
            if (!std::isfinite(r[e]))
                return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": mover sweep record " + std::to_string(k) + " has an entry that is not finite");
        const int rc = check_pose12(who, "mover sweep record", k, r);
        if (rc) return rc;
        if (r[12] < (float)kCosQuarterPi)      // the float32 nearest cos(pi/4): a quarter turn narrowed from float64 passes
            return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": mover sweep record " + std::to_string(k) +
                                                 " rotates by more than pi/2 per sweep (dq.w < cos(pi/4))");
    }
    return LRC_OK;
}

// ---- the eight scan entry points behind two checkers ---------------------------------------------------------------------------
// `sweep`: the sensor's records are motion24 with a fire table, the movers' are mover sweep records.  `noisy`: the call brings an
// lrc_noise.  Every refusal comes before the first device call, in this order: the mover calls' own (check_call, tile_count or the
// table, NULL inputs, bad host records), among them the model's (noise_params_host: the checks of lrc_scan_noisy_dev /
// lrc_scan_noisy_sweeps_dev with no context, N >= 2^32 among them) where each call has always made them.  noise_params then
// makes the quantile table resident.
static int scan_dev(const char* name, bool sweep, bool noisy, lrc_scene* s, lrc_movers* set, const double* d_sensor, uint64_t P,
                    const double* d_dirs3, const double* d_fire, uint64_t N, const float* d_movers, double max_range,
                    const lrc_noise* noise, const lrc_hits* d_out, uint8_t* d_mover, void* stream) {
    const std::string who = name;
    int rc = check_call(name, s, set, d_out);
    if (rc) return rc;
    if (d_out->tile_count)
        return fail(LRC_ERR_INVALID_ARG, who + ": tile_count is not written by this scan (lrc_compact_dev counts itself)");
    if (P && N && (!d_sensor || !d_dirs3 || (sweep && !d_fire)))
        return fail(LRC_ERR_INVALID_ARG, who + (sweep ? ": motion24, dirs3 or fire is NULL" : ": poses16 or dirs3 is NULL"));
    if (P && N && set && !d_movers) return fail(LRC_ERR_INVALID_ARG, who + (sweep ? ": mover_motion24 is NULL" : ": mover_poses12 is NULL"));
    lrcnoise::Params np{};
    if (noisy && (rc = noise_params_host(name, noise, N, &np))) return rc;
    LRC_HIP(hipSetDevice(s->ctx->device));
    if (noisy && (rc = noise_params(s->ctx, name, noise, N, &np))) return rc;
    const MoverScan scan{d_sensor, d_dirs3, sweep ? d_fire : nullptr, d_movers, noisy ? &np : nullptr, P, N, max_range};
    return movers_scan_dev(s, set, scan, d_out, d_mover, (hipStream_t)stream);
}

// An empty call (P * table->n == 0) returns after the table's checks -- under `sweep` the fire table among them -- and the
// model's, before the sensor's records are looked at.  Only the calls without a model have a rays_per_pose message of their own:
// the model's checks refuse N >= 2^32 before it.
static int scan_compact(const char* name, bool sweep, bool noisy, lrc_scene* s, lrc_movers* set, const double* sensor, uint64_t P,
                        const lrc_table* table, const float* movers, double max_range, const lrc_noise* noise, const lrc_frames* out,
                        uint8_t* mover_rows, uint64_t capacity, uint64_t* out_total) {
    const std::string who = name;
    if (out_total) *out_total = 0;
    int rc = check_call(name, s, set, out);
    if (rc) return rc;
    if (!table) return fail(LRC_ERR_INVALID_ARG, who + ": table is NULL");
    if (table->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, who + ": table and scene belong to different contexts");
    if (sweep && !table->d_fire) return fail(LRC_ERR_INVALID_ARG, who + ": the table has no fire table (lrc_table_set_fire)");
    lrcnoise::Params np{};
    if (noisy && (rc = noise_params_host(name, noise, table->n, &np))) return rc;
    if (!(P * table->n)) return LRC_OK;
    if (!sensor || !out->counts) return fail(LRC_ERR_INVALID_ARG, who + (sweep ? ": motion24 or counts is NULL" : ": poses16 or counts is NULL"));
    if (!noisy && table->n > 0xFFFFFFFFull)
        return fail(LRC_ERR_INVALID_ARG, who + ": rays_per_pose must stay below 2^32 (the index column)");
    if (sweep && (rc = check_motion(name, sensor, P))) return rc;
    if (set) {
        if (!movers) return fail(LRC_ERR_INVALID_ARG, who + (sweep ? ": mover_motion24 is NULL" : ": mover_poses12 is NULL"));
        const uint64_t count = P * set->scenes.size();
        if ((rc = sweep ? check_motion24(name, movers, count) : check_poses12(name, movers, count))) return rc;
    }
    LRC_HIP(hipSetDevice(s->ctx->device));
    if (noisy && (rc = noise_params(s->ctx, name, noise, table->n, &np))) return rc;
    return movers_scan_compact(s, set, sensor, P, table, movers, max_range, sweep, noisy ? &np : nullptr, out, mover_rows, capacity,
                               out_total);
}

extern "C" {

int lrc_movers_create(lrc_ctx* ctx, lrc_scene* const* scenes, uint32_t num_movers, lrc_movers** out_set) {
    if (out_set) *out_set = nullptr;
    // what needs no context is checked first
    if (num_movers < 1 || num_movers > lrcmov::kMaxMovers)
        return fail(LRC_ERR_INVALID_ARG, "lrc_movers_create: the number of movers must lie in [1, 255]");
    if (!ctx || !out_set) return fail(LRC_ERR_INVALID_ARG, "lrc_movers_create: NULL context or output");
    if (!scenes) return fail(LRC_ERR_INVALID_ARG, "lrc_movers_create: scenes is NULL");
    for (uint32_t m = 0; m < num_movers; ++m) {
        if (!scenes[m]) return fail(LRC_ERR_INVALID_ARG, "lrc_movers_create: mover " + std::to_string(m) + " is NULL");
        if (scenes[m]->ctx != ctx)
            return fail(LRC_ERR_INVALID_ARG, "lrc_movers_create: mover " + std::to_string(m) + " belongs to another context");
    }
    lrc_movers* set = new lrc_movers;
    set->ctx = ctx;
    set->scenes.assign(scenes, scenes + num_movers);
    *out_set = set;
    return LRC_OK;
}

int lrc_movers_destroy(lrc_movers* set) {
    if (!set) return LRC_OK;
    if (set->scratch) {
        (void)hipSetDevice(set->ctx->device);
        (void)hipFree(set->scratch);
    }
    delete set;
    return LRC_OK;
}

int lrc_scan_movers_dev(lrc_scene* s, lrc_movers* set, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N,
                        const float* d_mover_poses12, double max_range, const lrc_hits* d_out, uint8_t* d_mover, void* stream) {
    return scan_dev("lrc_scan_movers_dev", false, false, s, set, d_poses16, P, d_dirs3, nullptr, N, d_mover_poses12, max_range, nullptr,
                    d_out, d_mover, stream);
}

int lrc_scan_movers_compact(lrc_scene* s, lrc_movers* set, const double* poses16, uint64_t P, const lrc_table* table,
                            const float* mover_poses12, double max_range, const lrc_frames* out, uint8_t* mover_rows,
                            uint64_t capacity, uint64_t* out_total) {
    return scan_compact("lrc_scan_movers_compact", false, false, s, set, poses16, P, table, mover_poses12, max_range, nullptr, out,
                        mover_rows, capacity, out_total);
}

int lrc_mover_rays(const float* rays6, uint64_t n, const float* pose12, float* out_rays6) {
    if (!pose12 || (n && (!rays6 || !out_rays6))) return fail(LRC_ERR_INVALID_ARG, "lrc_mover_rays: NULL argument");
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = rays6 + i * 6;
        lrcmov::Vec oo, od;
        lrcmov::to_object(pose12, lrcmov::Vec{r[0], r[1], r[2]}, lrcmov::Vec{r[3], r[4], r[5]}, oo, od);
        float* w = out_rays6 + i * 6;
        w[0] = oo.x; w[1] = oo.y; w[2] = oo.z; w[3] = od.x; w[4] = od.y; w[5] = od.z;
    }
    return LRC_OK;
}

int lrc_mover_merge(uint64_t n, uint32_t M, const float* t_static, const float* normal3_static, const float* t_movers,
                    const float* normal3_movers, const float* poses12, float* out_t, float* out_normal3, uint8_t* out_mover) {
    if (M > lrcmov::kMaxMovers) return fail(LRC_ERR_INVALID_ARG, "lrc_mover_merge: the number of movers must not exceed 255");
    if (n && (!t_static || !normal3_static || !out_t || !out_normal3 || !out_mover || (M && (!t_movers || !normal3_movers || !poses12))))
        return fail(LRC_ERR_INVALID_ARG, "lrc_mover_merge: NULL argument");
    for (uint64_t i = 0; i < n; ++i) {
        float t = t_static[i];
        lrcmov::Vec nn{normal3_static[i * 3], normal3_static[i * 3 + 1], normal3_static[i * 3 + 2]};
        uint8_t who = 0;
        for (uint32_t m = 0; m < M; ++m) {
            const float tm = t_movers[(uint64_t)m * n + i];
            if (!lrcmov::takes(tm, t)) continue;
            const float* q = normal3_movers + ((uint64_t)m * n + i) * 3;
            nn = lrcmov::to_world(poses12 + (uint64_t)m * 12, lrcmov::Vec{q[0], q[1], q[2]});
            t = tm;
            who = (uint8_t)(m + 1u);
        }
        out_t[i] = t;
        out_normal3[i * 3] = nn.x; out_normal3[i * 3 + 1] = nn.y; out_normal3[i * 3 + 2] = nn.z;
        out_mover[i] = who;
    }
    return LRC_OK;
}

// ---- movers under moving-sensor sweeps ---------------------------------------------------------------------------------------

int lrc_scan_mover_sweeps_dev(lrc_scene* s, lrc_movers* set, const double* d_motion24, uint64_t P, const double* d_dirs3,
                              const double* d_fire, uint64_t N, const float* d_mover_motion24, double max_range,
                              const lrc_hits* d_out, uint8_t* d_mover, void* stream) {
    return scan_dev("lrc_scan_mover_sweeps_dev", true, false, s, set, d_motion24, P, d_dirs3, d_fire, N, d_mover_motion24, max_range,
                    nullptr, d_out, d_mover, stream);
}

int lrc_scan_mover_sweeps_compact(lrc_scene* s, lrc_movers* set, const double* motion24, uint64_t P, const lrc_table* table,
                                  const float* mover_motion24, double max_range, const lrc_frames* out, uint8_t* mover_rows,
                                  uint64_t capacity, uint64_t* out_total) {
    return scan_compact("lrc_scan_mover_sweeps_compact", true, false, s, set, motion24, P, table, mover_motion24, max_range, nullptr,
                        out, mover_rows, capacity, out_total);
}

int lrc_mover_sweep_rays(const float* rays6, const double* fire, uint64_t n, const float* motion24, float* out_rays6) {
    if (!motion24 || (n && (!rays6 || !fire || !out_rays6))) return fail(LRC_ERR_INVALID_ARG, "lrc_mover_sweep_rays: NULL argument");
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = rays6 + i * 6;
        lrcmov::Vec oo, od;
        lrcmov::to_object_at(motion24, (float)fire[i], lrcmov::Vec{r[0], r[1], r[2]}, lrcmov::Vec{r[3], r[4], r[5]}, oo, od);
        float* w = out_rays6 + i * 6;
        w[0] = oo.x; w[1] = oo.y; w[2] = oo.z; w[3] = od.x; w[4] = od.y; w[5] = od.z;
    }
    return LRC_OK;
}

int lrc_mover_sweep_normals(const float* normal3, const double* fire, uint64_t n, const float* motion24, float* out_normal3) {
    if (!motion24 || (n && (!normal3 || !fire || !out_normal3))) return fail(LRC_ERR_INVALID_ARG, "lrc_mover_sweep_normals: NULL argument");
    for (uint64_t i = 0; i < n; ++i) {
        const float* q = normal3 + i * 3;
        const lrcmov::Vec w = lrcmov::to_world_at(motion24, (float)fire[i], lrcmov::Vec{q[0], q[1], q[2]});
        out_normal3[i * 3] = w.x; out_normal3[i * 3 + 1] = w.y; out_normal3[i * 3 + 2] = w.z;
    }
    return LRC_OK;
}

// ---- seeded sensor noise under movers, and under movers in sweeps --------------------------------------------------------------

int lrc_scan_noisy_movers_dev(lrc_scene* s, lrc_movers* set, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N,
                              const float* d_mover_poses12, double max_range, const lrc_noise* noise, const lrc_hits* d_out,
                              uint8_t* d_mover, void* stream) {
    return scan_dev("lrc_scan_noisy_movers_dev", false, true, s, set, d_poses16, P, d_dirs3, nullptr, N, d_mover_poses12, max_range,
                    noise, d_out, d_mover, stream);
}

int lrc_scan_noisy_movers_compact(lrc_scene* s, lrc_movers* set, const double* poses16, uint64_t P, const lrc_table* table,
                                  const float* mover_poses12, double max_range, const lrc_noise* noise, const lrc_frames* out,
                                  uint8_t* mover_rows, uint64_t capacity, uint64_t* out_total) {
    return scan_compact("lrc_scan_noisy_movers_compact", false, true, s, set, poses16, P, table, mover_poses12, max_range, noise, out,
                        mover_rows, capacity, out_total);
}

int lrc_scan_noisy_mover_sweeps_dev(lrc_scene* s, lrc_movers* set, const double* d_motion24, uint64_t P, const double* d_dirs3,
                                    const double* d_fire, uint64_t N, const float* d_mover_motion24, double max_range,
                                    const lrc_noise* noise, const lrc_hits* d_out, uint8_t* d_mover, void* stream) {
    return scan_dev("lrc_scan_noisy_mover_sweeps_dev", true, true, s, set, d_motion24, P, d_dirs3, d_fire, N, d_mover_motion24,
                    max_range, noise, d_out, d_mover, stream);
}

int lrc_scan_noisy_mover_sweeps_compact(lrc_scene* s, lrc_movers* set, const double* motion24, uint64_t P, const lrc_table* table,
                                        const float* mover_motion24, double max_range, const lrc_noise* noise, const lrc_frames* out,
                                        uint8_t* mover_rows, uint64_t capacity, uint64_t* out_total) {
    return scan_compact("lrc_scan_noisy_mover_sweeps_compact", true, true, s, set, motion24, P, table, mover_motion24, max_range, noise,
                        out, mover_rows, capacity, out_total);
}

}  // extern "C"
