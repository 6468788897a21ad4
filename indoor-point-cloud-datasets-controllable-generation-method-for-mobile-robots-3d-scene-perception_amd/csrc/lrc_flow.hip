// lrc_flow.hip -- host side of the scene flow under movers (lrc_flow.h): the checks of lrc_scan_flow_dev / lrc_scan_flow_compact
// (the kernels, the launches and the frame path are lidarcast.hip's: flow_scan_dev, flow_scan_compact) and the two host functions
// lrc_flow_rays and lrc_flow_status, which run the inline functions the kernels call on arrays.
// The same for the non-rigid flow of deforming movers: the checks of lrc_scan_nonrigid_flow_dev, which
// turn the caller's surface pairs into the kernel's argument block, and the host function lrc_nonrigid_flow_rays.
#include <cmath>

#include "lrc_internal.h"
#include "lrc_flow.h"

static_assert(sizeof(FlowPairs::mover) / sizeof(uint32_t) == lrcflow::kMaxPairs, "the kernel's pair block holds kMaxPairs entries");

extern "C" {

int lrc_scan_flow_dev(lrc_scene* s, lrc_movers* set, const lrc_hits* d_records, const uint8_t* d_mover, uint64_t P, uint64_t N,
                      const float* d_mover_poses12, const float* d_next_mover_poses12, const double* d_next_poses16,
                      const uint8_t* d_has_next, double max_range, float* d_flow3, uint8_t* d_status, void* stream) {
    auto bad = [&](const char* t) { return fail(LRC_ERR_INVALID_ARG, std::string("lrc_scan_flow_dev: ") + t); };
    int rc = check_call("lrc_scan_flow_dev", s, set, d_records);
    if (rc) return rc;
    if (!d_flow3) return bad("flow3 is NULL");
    if (!d_records->t || !d_records->point3) return bad("the records need t and point3");
    if (set && !d_mover) return bad("the mover column is NULL");
    if (!d_next_poses16) return bad("next_poses16 is NULL");
    if (set && (!d_mover_poses12 || !d_next_mover_poses12)) return bad("mover_poses12 or next_mover_poses12 is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    const FlowNext next{d_next_mover_poses12, d_next_poses16, d_has_next};
    return flow_scan_dev(s, set, d_records, d_mover, P, N, d_mover_poses12, next, max_range, d_flow3, d_status, (hipStream_t)stream);
}

int lrc_scan_flow_compact(lrc_scene* s, lrc_movers* set, const double* poses16, uint64_t P, const lrc_table* table,
                          const float* mover_poses12, const double* next_poses16, const float* next_mover_poses12,
                          const uint8_t* has_next, double max_range, const lrc_frames* out, uint8_t* mover_rows, float* flow_rows,
                          uint8_t* status_rows, uint64_t capacity, uint64_t* out_total) {
    auto bad = [&](const char* t) { return fail(LRC_ERR_INVALID_ARG, std::string("lrc_scan_flow_compact: ") + t); };
    if (out_total) *out_total = 0;
    int rc = check_call("lrc_scan_flow_compact", s, set, out);
    if (rc) return rc;
    if (!table) return bad("table is NULL");
    if (table->ctx != s->ctx) return bad("table and scene belong to different contexts");
    if (!flow_rows) return bad("flow_rows is NULL");
    if (!next_poses16) return bad("next_poses16 is NULL");
    if (set && (!mover_poses12 || !next_mover_poses12)) return bad("mover_poses12 or next_mover_poses12 is NULL");
    if (!(P * table->n)) return LRC_OK;
    if (!poses16 || !out->counts) return bad("poses16 or counts is NULL");
    if (table->n > 0xFFFFFFFFull) return bad("rays_per_pose must stay below 2^32 (the index column)");
    if (set) {
        if ((rc = check_poses12("lrc_scan_flow_compact", mover_poses12, P * set->scenes.size()))) return rc;
        if ((rc = check_poses12("lrc_scan_flow_compact (next)", next_mover_poses12, P * set->scenes.size()))) return rc;
    }
    LRC_HIP(hipSetDevice(s->ctx->device));
    const FlowNext next{next_mover_poses12, next_poses16, has_next};
    return flow_scan_compact(s, set, poses16, P, table, mover_poses12, next, max_range, out, mover_rows, flow_rows, status_rows,
                             capacity, out_total);
}

int lrc_flow_rays(const float* t, const float* point3, const uint8_t* mover, uint64_t P, uint64_t N, uint32_t M,
                  const float* mover_poses12, const float* next_mover_poses12, const double* next_poses16, const uint8_t* has_next,
                  double max_range, double min_range, float* out_flow3, float* out_rays6, uint8_t* out_keep, float* out_thr,
                  uint8_t* out_status) {
    if (M > lrcmov::kMaxMovers) return fail(LRC_ERR_INVALID_ARG, "lrc_flow_rays: the number of movers must not exceed 255");
    const uint64_t n = P * N;
    if (n && (!t || !point3 || !next_poses16 || !out_flow3 || !out_rays6 || !out_keep || !out_thr || !out_status ||
              (M && (!mover || !mover_poses12 || !next_mover_poses12))))
        return fail(LRC_ERR_INVALID_ARG, "lrc_flow_rays: NULL argument");
    for (uint64_t p = 0; p < P; ++p)
        for (uint64_t i = 0; i < N; ++i) {
            const uint64_t g = p * N + i;
            const bool live = (t[g] < INFINITY) & (has_next == nullptr || has_next[p] != 0);
            const uint32_t w = (live && M) ? mover[g] : 0u;
            const float* A = nullptr;
            const float* B = nullptr;
            bool moved = false;
            if (w != 0u && w <= M) {
                A = mover_poses12 + (p * M + (w - 1u)) * 12;
                B = next_mover_poses12 + (p * M + (w - 1u)) * 12;
                moved = !lrcflow::same_pose(A, B);
            }
            const lrcflow::Ray r = lrcflow::ray(live, moved, point3 + g * 3, A, B, next_poses16 + p * 16, max_range, min_range);
            const bool cast = r.status == lrcflow::kVisible;
            for (int j = 0; j < 3; ++j) out_flow3[g * 3 + j] = r.flow[j];
            float* w6 = out_rays6 + g * 6;
            w6[0] = cast ? r.o.x : 0.f; w6[1] = cast ? r.o.y : 0.f; w6[2] = cast ? r.o.z : 0.f;
            w6[3] = cast ? r.h.x : 0.f; w6[4] = cast ? r.h.y : 0.f; w6[5] = cast ? r.h.z : 0.f;
            out_keep[g] = cast ? 1 : 0;
            out_thr[g] = cast ? r.thr : 0.f;
            out_status[g] = r.status;
        }
    return LRC_OK;
}

// Non-rigid scene flow: lrc_scan_flow_dev's checks, then the pairs become the kernel's argument block --
// the triangles, T and a NULL next shape come from the deformable that owns the mover's scene.
int lrc_scan_nonrigid_flow_dev(lrc_scene* s, lrc_movers* set, const lrc_hits* d_records, const uint8_t* d_mover, uint64_t P,
                               uint64_t N, const float* d_mover_poses12, const float* d_next_mover_poses12,
                               const double* d_next_poses16, const uint8_t* d_has_next, double max_range,
                               const lrc_surface_pair* pairs, uint32_t num_pairs, float* d_flow3, uint8_t* d_status, void* stream) {
    auto bad = [&](const std::string& t) { return fail(LRC_ERR_INVALID_ARG, "lrc_scan_nonrigid_flow_dev: " + t); };
    int rc = check_call("lrc_scan_nonrigid_flow_dev", s, set, d_records);
    if (rc) return rc;
    if (!d_flow3) return bad("flow3 is NULL");
    if (!d_records->t || !d_records->point3 || !d_records->prim) return bad("the records need t, point3 and prim");
    if (set && !d_mover) return bad("the mover column is NULL");
    if (!d_next_poses16) return bad("next_poses16 is NULL");
    if (set && (!d_mover_poses12 || !d_next_mover_poses12)) return bad("mover_poses12 or next_mover_poses12 is NULL");
    if (num_pairs > lrcflow::kMaxPairs) return bad("at most 16 surface pairs per call");
    if (num_pairs && !pairs) return bad("pairs is NULL");
    const uint32_t M = set ? (uint32_t)set->scenes.size() : 0u;
    FlowPairs fp{};
    fp.count = num_pairs;
    fp.prim = d_records->prim;
    for (uint32_t k = 0; k < num_pairs; ++k) {
        const lrc_surface_pair& p = pairs[k];
        if (p.mover >= M) return bad("pair " + std::to_string(k) + " names mover " + std::to_string(p.mover) + " of " + std::to_string(M));
        const lrc_deform* d = set->scenes[p.mover]->deform;
        if (!d) return bad("pair " + std::to_string(k) + ": mover " + std::to_string(p.mover) + " is not a deformable's scene");
        for (uint32_t e = 0; e < k; ++e)
            if (pairs[e].mover == p.mover) return bad("mover " + std::to_string(p.mover) + " is listed twice");
        if (!p.d_verts_a3) return bad("pair " + std::to_string(k) + ": verts_a3 is NULL");
        const DeformMesh mesh = deform_mesh(d);
        fp.mover[k] = p.mover;
        fp.T[k] = (uint32_t)mesh.T;           // T < 2^28 (lrc_deform_create)
        fp.va[k] = p.d_verts_a3;
        fp.vb[k] = p.d_verts_b3 ? p.d_verts_b3 : mesh.d_verts3;
        fp.tris3[k] = mesh.d_tris3;
    }
    LRC_HIP(hipSetDevice(s->ctx->device));
    const FlowNext next{d_next_mover_poses12, d_next_poses16, d_has_next};
    return flow_scan_dev(s, set, d_records, d_mover, P, N, d_mover_poses12, next, max_range, d_flow3, d_status, (hipStream_t)stream,
                         &fp);
}

int lrc_nonrigid_flow_rays(const float* t, const float* point3, const uint8_t* mover, const uint32_t* prim, uint64_t P, uint64_t N,
                           uint32_t M, const float* mover_poses12, const float* next_mover_poses12, const double* next_poses16,
                           const uint8_t* has_next, double max_range, double min_range, const lrc_surface_pair_host* pairs,
                           uint32_t num_pairs, float* out_flow3, float* out_rays6, uint8_t* out_keep, float* out_thr,
                           uint8_t* out_status) {
    auto bad = [&](const std::string& w) { return fail(LRC_ERR_INVALID_ARG, "lrc_nonrigid_flow_rays: " + w); };
    if (M > lrcmov::kMaxMovers) return bad("the number of movers must not exceed 255");
    const uint64_t n = P * N;
    if (n && (!t || !point3 || !next_poses16 || !out_flow3 || !out_rays6 || !out_keep || !out_thr || !out_status ||
              (M && (!mover || !mover_poses12 || !next_mover_poses12))))
        return bad("NULL argument");
    if (num_pairs > lrcflow::kMaxPairs) return bad("at most 16 surface pairs per call");
    if (num_pairs && (!pairs || !prim)) return bad("pairs or prim is NULL");
    for (uint32_t k = 0; k < num_pairs; ++k) {
        const lrc_surface_pair_host& p = pairs[k];
        if (p.mover >= M) return bad("pair " + std::to_string(k) + " names mover " + std::to_string(p.mover) + " of " + std::to_string(M));
        for (uint32_t e = 0; e < k; ++e)
            if (pairs[e].mover == p.mover) return bad("mover " + std::to_string(p.mover) + " is listed twice");
        if (!p.verts_a3 || !p.verts_b3 || (p.T && !p.tris3)) return bad("pair " + std::to_string(k) + " has a NULL array");
        for (uint64_t i = 0; i < 3 * p.T; ++i)
            if (p.tris3[i] >= p.V) return bad("pair " + std::to_string(k) + ": triangle index out of range");
    }
    for (uint64_t p = 0; p < P; ++p)
        for (uint64_t i = 0; i < N; ++i) {
            const uint64_t g = p * N + i;
            const bool live = (t[g] < INFINITY) & (has_next == nullptr || has_next[p] != 0);
            const uint32_t w = (live && M) ? mover[g] : 0u;
            const float* A = nullptr;
            const float* B = nullptr;
            const lrc_surface_pair_host* pair = nullptr;
            bool moved = false;
            if (w != 0u && w <= M) {
                A = mover_poses12 + (p * M + (w - 1u)) * 12;
                B = next_mover_poses12 + (p * M + (w - 1u)) * 12;
                moved = !lrcflow::same_pose(A, B);
                for (uint32_t k = 0; k < num_pairs; ++k)
                    if (pairs[k].mover == w - 1u) pair = pairs + k;
            }
            lrcflow::Ray r;
            if (pair && prim[g] < pair->T) {
                float a9[9], b9[9];
                for (int c = 0; c < 3; ++c) {
                    const uint64_t v = (uint64_t)pair->tris3[(uint64_t)prim[g] * 3 + c] * 3;
                    for (int e = 0; e < 3; ++e) { a9[3 * c + e] = pair->verts_a3[v + e]; b9[3 * c + e] = pair->verts_b3[v + e]; }
                }
                r = lrcflow::nonrigid_ray(point3 + g * 3, A, B, a9, b9, next_poses16 + p * 16, max_range, min_range);
            } else {
                r = lrcflow::ray(live, moved, point3 + g * 3, A, B, next_poses16 + p * 16, max_range, min_range);
            }
            const bool cast = r.status == lrcflow::kVisible;
            for (int j = 0; j < 3; ++j) out_flow3[g * 3 + j] = r.flow[j];
            float* w6 = out_rays6 + g * 6;
            w6[0] = cast ? r.o.x : 0.f; w6[1] = cast ? r.o.y : 0.f; w6[2] = cast ? r.o.z : 0.f;
            w6[3] = cast ? r.h.x : 0.f; w6[4] = cast ? r.h.y : 0.f; w6[5] = cast ? r.h.z : 0.f;
            out_keep[g] = cast ? 1 : 0;
            out_thr[g] = cast ? r.thr : 0.f;
            out_status[g] = r.status;
        }
    return LRC_OK;
}

int lrc_flow_status(uint64_t n, uint32_t M, const float* t_static, const float* t_movers, const float* thr, const uint8_t* status,
                    uint8_t* out_status) {
    if (M > lrcmov::kMaxMovers) return fail(LRC_ERR_INVALID_ARG, "lrc_flow_status: the number of movers must not exceed 255");
    if (n && (!t_static || !thr || !status || !out_status || (M && !t_movers)))
        return fail(LRC_ERR_INVALID_ARG, "lrc_flow_status: NULL argument");
    for (uint64_t i = 0; i < n; ++i) {
        float t = t_static[i];
        for (uint32_t m = 0; m < M; ++m) t = lrcflow::nearer(t_movers[(uint64_t)m * n + i], t);
        out_status[i] = status[i] == lrcflow::kVisible ? lrcflow::judge(t, thr[i]) : status[i];
    }
    return LRC_OK;
}

}  // extern "C"
