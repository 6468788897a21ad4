// lrc_material.hip -- host side of the surface materials (lrc_material.h): the checks of a model and its records, the resident
// table, the entry points lrc_scan_materials_dev / lrc_scan_materials_compact (the trace launch and the frame path are
// lidarcast.hip's: material_scan_dev, material_scan_compact, which also gathers the kept rows' intensity, bounces and surface
// points) and the host step lrc_material_step.
#include <cmath>

#include "lrc_internal.h"
#include "lrc_material.h"

static_assert(sizeof(lrc_material) == sizeof(lrcmat::Record) && sizeof(lrc_material) == 16, "lrc_material is the kernel's record");

namespace {

// checks an lrc_material_model and, when given, its num_classes records (LRC_ERR_INVALID_ARG, `who` prefixes the message)
int check_model(const char* who, const lrc_material_model* m, const lrc_material* rec) {
    auto bad = [&](const std::string& t) { return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": " + t); };
    if (!m) return bad("model is NULL");
    if (m->num_classes < 1 || m->num_classes > lrcmat::kMaxClasses) return bad("num_classes must lie in [1, 256]");
    if (m->max_bounces > lrcmat::kMaxBounces) return bad("max_bounces must lie in [0, 8]");
    if (!std::isfinite(m->min_intensity) || !(m->min_intensity >= 0.0f && m->min_intensity <= 1.0f))
        return bad("min_intensity must be finite and lie in [0, 1]");
    if (!rec) return bad("records is NULL");
    for (uint32_t k = 0; k < m->num_classes; ++k) {
        const lrc_material& r = rec[k];
        const std::string at = "class " + std::to_string(k) + ": ";
        if (r.kind > lrcmat::kMirror) return bad(at + "kind must be 0 (diffuse), 1 (glass) or 2 (mirror)");
        if (!std::isfinite(r.albedo) || !(r.albedo >= 0.0f && r.albedo <= 1.0f)) return bad(at + "albedo must be finite and lie in [0, 1]");
        if (!std::isfinite(r.pass) || !(r.pass >= 0.0f && r.pass <= 1.0f)) return bad(at + "pass must be finite and lie in [0, 1]");
        if (!std::isfinite(r.retro_cos) || !(r.retro_cos >= 0.0f)) return bad(at + "retro_cos must be finite and not negative");
    }
    return LRC_OK;
}

lrcmat::Params params_of(const lrc_material_table* t) {
    lrcmat::Params mp{};
    mp.table = t->d_records;
    mp.min_intensity = t->model.min_intensity;
    mp.num_classes = t->model.num_classes;
    mp.max_bounces = t->model.max_bounces;
    return mp;
}

}  // namespace

extern "C" {

int lrc_material_table_create(lrc_ctx* ctx, const lrc_material_model* model, const lrc_material* records,
                              lrc_material_table** out_table) {
    if (out_table) *out_table = nullptr;
    // what needs no context is checked first
    int rc = check_model("lrc_material_table_create", model, records);
    if (rc) return rc;
    if (!ctx || !out_table) return fail(LRC_ERR_INVALID_ARG, "lrc_material_table_create: NULL context or output");
    LRC_HIP(hipSetDevice(ctx->device));
    lrcmat::Record* d = nullptr;
    const size_t bytes = sizeof(lrcmat::Record) * model->num_classes;
    LRC_HIP(hipMalloc((void**)&d, bytes));
    const hipError_t e = hipMemcpy(d, records, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); LRC_HIP(e); }
    lrc_material_table* t = new lrc_material_table;
    t->ctx = ctx;
    t->d_records = d;
    t->model = *model;
    *out_table = t;
    return LRC_OK;
}

int lrc_material_table_destroy(lrc_material_table* t) {
    if (!t) return LRC_OK;
    (void)hipSetDevice(t->ctx->device);
    if (t->d_records) (void)hipFree(t->d_records);
    delete t;
    return LRC_OK;
}

int lrc_scan_materials_dev(lrc_scene* s, const double* d_poses16, uint64_t P, const double* d_dirs3, uint64_t N,
                           const lrc_material_table* mat, double max_range, const lrc_hits* d_out, uint8_t* d_bounces,
                           float* d_surface_point3, void* stream) {
    if (!mat) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_dev: materials is NULL");
    if (!s || !d_out) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_dev: NULL scene or output");
    if (mat->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_dev: materials and scene belong to different contexts");
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_dev: a range_noise option is set");
    if (s->opts.incident_mode == 1)      // the angle between the ORIGINAL beam and the final surface's normal means nothing behind a mirror
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_dev: incident_mode 1 (angle to the surface normal) is not defined for a continued ray");
    if (P && N && (!d_poses16 || !d_dirs3))
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_dev: poses16 or dirs3 is NULL");
    LRC_HIP(hipSetDevice(s->ctx->device));
    lrcmat::Params mp = params_of(mat);
    mp.bounces = d_bounces;
    mp.surface3 = d_surface_point3;
    return material_scan_dev(s, d_poses16, P, d_dirs3, N, mp, max_range, d_out, (hipStream_t)stream);
}

int lrc_scan_materials_compact(lrc_scene* s, const double* poses16, uint64_t P, const lrc_table* table,
                               const lrc_material_table* mat, double max_range, const lrc_frames* out, float* intensity_rows,
                               uint8_t* bounces_rows, float* surface_rows, uint64_t capacity, uint64_t* out_total) {
    if (out_total) *out_total = 0;
    if (!mat) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_compact: materials is NULL");
    if (!s || !out || !table) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_compact: NULL scene, table or output");
    if (table->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_compact: table and scene belong to different contexts");
    if (mat->ctx != s->ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_compact: materials and scene belong to different contexts");
    if (s->opts.range_noise)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_compact: a range_noise option is set");
    if (s->opts.incident_mode == 1)      // the angle between the ORIGINAL beam and the final surface's normal means nothing behind a mirror
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_compact: incident_mode 1 (angle to the surface normal) is not defined for a continued ray");
    if (!(P * table->n)) return LRC_OK;
    if (!poses16 || !out->counts) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_compact: poses16 or counts is NULL");
    if (table->n > 0xFFFFFFFFull)
        return fail(LRC_ERR_INVALID_ARG, "lrc_scan_materials_compact: rays_per_pose must stay below 2^32 (the index column)");
    LRC_HIP(hipSetDevice(s->ctx->device));
    return material_scan_compact(s, poses16, P, table, params_of(mat), max_range, out, intensity_rows, bounces_rows, surface_rows,
                                 capacity, out_total);
}

int lrc_material_step(const lrc_material_model* model, const lrc_material* records, uint64_t n, const float* t,
                      const uint16_t* sem, const float* normal3, float* origin3, float* dir3, float* path, float* gain,
                      uint8_t* bounces, uint8_t* status, float* intensity, float* surface_point3) {
    int rc = check_model("lrc_material_step", model, records);
    if (rc) return rc;
    if (n && (!t || !sem || !normal3 || !origin3 || !dir3 || !path || !gain || !bounces || !status || !intensity || !surface_point3))
        return fail(LRC_ERR_INVALID_ARG, "lrc_material_step: NULL argument");
    const lrcmat::Record* tab = reinterpret_cast<const lrcmat::Record*>(records);
    for (uint64_t i = 0; i < n; ++i) {
        if (status[i] != lrcmat::kContinue) continue;
        if (!(t[i] < __builtin_inff())) { status[i] = (uint8_t)lrcmat::kNoReturn; continue; }
        lrcmat::Seg sg{origin3[i * 3], origin3[i * 3 + 1], origin3[i * 3 + 2], dir3[i * 3], dir3[i * 3 + 1], dir3[i * 3 + 2],
                       path[i], gain[i], bounces[i]};
        float I = 0.0f, px, py, pz;
        int st = lrcmat::step(sg, t[i], normal3[i * 3], normal3[i * 3 + 1], normal3[i * 3 + 2],
                              lrcmat::record_of(tab, model->num_classes, sem[i]), model->max_bounces, I, px, py, pz);
        if (st == lrcmat::kReturn && I < model->min_intensity) st = lrcmat::kNoReturn;
        path[i] = sg.T; gain[i] = sg.g; bounces[i] = (uint8_t)sg.b;
        status[i] = (uint8_t)st;
        if (st == lrcmat::kReturn) {
            intensity[i] = I;
            surface_point3[i * 3] = px; surface_point3[i * 3 + 1] = py; surface_point3[i * 3 + 2] = pz;
        } else if (st == lrcmat::kContinue) {
            origin3[i * 3] = sg.ox; origin3[i * 3 + 1] = sg.oy; origin3[i * 3 + 2] = sg.oz;
            dir3[i * 3] = sg.dx; dir3[i * 3 + 1] = sg.dy; dir3[i * 3 + 2] = sg.dz;
        }
    }
    return LRC_OK;
}

}  // extern "C"
