// lrc_span.hip -- animated movers under sweeps (include/lidarcast.h "animated movers under sweeps"): a
// deformable that stands between two shapes A and B for the length of a sweep, and the cast in which every ray meets it at the
// shape it has at the ray's own firing fraction s -- the vertices lrcspan::span_vertex(A, B, s).  The tree is the deformable's
// own: its node boxes are refitted to hold both shapes, and since span_vertex never leaves [min(a, b), max(a, b)] every blended
// triangle's box lies inside its slot's span box, so no box test prunes a hit ("containment").
//
//   k_span_slots       one thread per leaf slot: the span box and the slot's vertex record, v0 v1 v2 of A then of B
//                      (lrcspan::slot_span).  A leaf's <= 4 slots are consecutive, so a leaf test reads 80 consecutive bytes per
//                      triangle in five 16-byte loads where a gather through tris3 would issue 18 scattered 4-byte loads.
//   node refit         k_level / k_tail of lrc_deform.hip with the span boxes in the place of slot_box (deform_nodes_enqueue)
//   span_trace_kernel  one lane per explicit ray, 64-lane workgroups.  Plain stack traversal of the float32 nodes (a deformable
//                      scene has no quantised images), nearer child first, the other pushed; the stack lies in LDS as
//                      [depth][lane], one column per lane.  Leaf test: blend the nine coordinates, lrctri::tri_record (the
//                      builders' record and vertex box), tri_mt, box_clause against that box, then (t, triangle row) order: the
//                      hit of DESIGN.md section 3 on a fresh scene of the blended vertices.  Writes the five columns the sweep merge
//                      reads (t, prim, normal3, sem, ins), a miss as write_back writes it.
// The host functions lrc_span_vertices and lrc_deform_span_refit run the same inline functions on arrays, without a GPU.
#include <cmath>
#include <cstring>

#include "lrc_internal.h"
#include "lrc_device.h"
#include "lrc_span.h"

namespace {

using namespace lrcdev;

constexpr int kSpanBlock = 256;      // k_span_slots
constexpr int kSpanTrace = 64;       // span_trace_kernel: one wave per workgroup

__global__ __launch_bounds__(kSpanBlock) void k_span_slots(const float* va3, const float* vb3, const uint32_t* tris3,
                                                           const uint32_t* slot_prim, uint32_t num_slots, float4* out_rec,
                                                           float* span_box) {
    const uint32_t s = blockIdx.x * kSpanBlock + threadIdx.x;
    if (s >= num_slots) return;
    float r[lrcspan::kRecFloats], bx[6];
    r[18] = 0.f; r[19] = 0.f;
    lrcspan::slot_span(va3, vb3, tris3, slot_prim[s], r, bx);
    float4* o = out_rec + (size_t)s * (lrcspan::kRecFloats / 4);
#pragma unroll
    for (int k = 0; k < lrcspan::kRecFloats / 4; ++k) o[k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
#pragma unroll
    for (int k = 0; k < 6; ++k) span_box[(size_t)s * 6 + k] = bx[k];
}

struct SpanTrace {
    const float4* nodes;           // the deformable's float32 nodes, boxes refitted to the span
    const float4* rec;             // kRecFloats / 4 float4 per leaf slot
    const uint32_t* slot_prim;
    const uint32_t* slot_label;
    const float* rays6;
    const uint8_t* keep;           // nullable: 0 = the ray is not cast
    const double* fire;            // (rays_per_pose)
    uint64_t rays_per_pose, total;
    float* t; uint32_t* prim; float* normal3; uint16_t* sem; uint16_t* ins;     // each nullable
};

// the 48-byte record and the vertex box of slot `slot` at fraction s, by the builders' own expressions on the blended vertices
__device__ __forceinline__ void span_record(const float4* rec, uint32_t slot, float s, float* r12, float* bx6) {
    const float4* p = rec + (size_t)slot * (lrcspan::kRecFloats / 4);
    const float4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
    const float va[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x};
    const float vb[9] = {c.y, c.z, c.w, d.x, d.y, d.z, d.w, e.x, e.y};
    float v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = lrcspan::span_vertex(va[k], vb[k], s);
    lrctri::tri_record(v, v + 3, v + 6, r12, bx6);
}

__global__ __launch_bounds__(kSpanTrace) void span_trace_kernel(const SpanTrace q) {
    __shared__ int s_stack[lrc::kMaxDepth][kSpanTrace];     // [depth][lane]: one column per lane, conflict free
    const uint64_t gid = (uint64_t)blockIdx.x * kSpanTrace + threadIdx.x;
    if (gid >= q.total) return;
    const uint32_t lane = threadIdx.x;
    bool live = q.keep ? q.keep[gid] != 0 : true;
    V3 o{0.f, 0.f, 0.f}, d{0.f, 0.f, 0.f};
    if (live) {                                   // a culled ray's row was never stored
        const float2* w = (const float2*)(q.rays6 + gid * 6);
        const float2 a = w[0], b = w[1], c = w[2];
        o = V3{a.x, a.y, b.x};
        d = V3{b.y, c.x, c.y};
        live = finite_ray(o, d);
    }
    float tbest = __builtin_inff();
    uint32_t best_slot = 0xFFFFFFFFu, best_prim = 0xFFFFFFFFu;
    float s = 0.f;
    if (live) {
        s = (float)q.fire[gid % q.rays_per_pose];
        const RaySlab sl = make_slab(o, d);
        int ref = 0, sp = 0;
        while (true) {
            if (ref >= 0) {
                const float4* n = q.nodes + (size_t)ref * 4;
                const float4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3];
                float n0, f0, n1, f1;
                slab_interval(sl, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, n0, f0);
                slab_interval(sl, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, n1, f1);
                const bool h0 = (n0 <= f0) & (n0 <= tbest), h1 = (n1 <= f1) & (n1 <= tbest);
                const int r0 = __float_as_int(q3.x), r1 = __float_as_int(q3.y);
                if (h0 & h1) {
                    const bool swap = n1 < n0;
                    s_stack[sp++][lane] = swap ? r0 : r1;
                    ref = swap ? r1 : r0;
                    continue;
                }
                if (h0 | h1) { ref = h0 ? r0 : r1; continue; }
            } else {
                const uint32_t code = (uint32_t)(~ref), first = code >> 3, cnt = code & 7u;
                for (uint32_t k = 0; k < cnt; ++k) {
                    const uint32_t slot = first + k;
                    float r[12], bx[6], t;
                    span_record(q.rec, slot, s, r, bx);
                    if (!tri_mt(o, d, V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, V3{r[6], r[7], r[8]}, V3{r[9], r[10], r[11]}, t)) continue;
                    if (!box_clause(sl, bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], t)) continue;
                    if (t < tbest) {
                        tbest = t; best_slot = slot; best_prim = 0xFFFFFFFFu;
                    } else if (t == tbest) {                       // an exact tie: the smaller triangle row
                        if (best_prim == 0xFFFFFFFFu) best_prim = q.slot_prim[best_slot];
                        const uint32_t pr = q.slot_prim[slot];
                        if (pr < best_prim) { best_slot = slot; best_prim = pr; }
                    }
                }
            }
            if (sp == 0) break;
            ref = s_stack[--sp][lane];
        }
    }
    // the miss record of write_back: +inf, LRC_INVALID_PRIM, zeros
    uint32_t prim = LRC_INVALID_PRIM, label = 0u;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (best_slot != 0xFFFFFFFFu) {
        prim = q.slot_prim[best_slot];
        label = q.slot_label[best_slot];
        if (q.normal3) {
            float r[12], bx[6];
            span_record(q.rec, best_slot, s, r, bx);
            // slot_normal's expression (lidarcast.hip) on the blended Ng
            const float len = __builtin_sqrtf(fma_(r[11], r[11], fma_(r[10], r[10], r[9] * r[9])));
            nx = r[9] / len; ny = r[10] / len; nz = r[11] / len;
        }
    }
    if (q.t) q.t[gid] = tbest;
    if (q.prim) q.prim[gid] = prim;
    if (q.normal3) { float* w = q.normal3 + gid * 3; w[0] = nx; w[1] = ny; w[2] = nz; }
    if (q.sem) q.sem[gid] = (uint16_t)(label & 0xFFFFu);
    if (q.ins) q.ins[gid] = (uint16_t)(label >> 16);
}

int check_shape(const lrc_deform* d, const char* which, uint32_t k0, uint32_t k1, float w) {
    if (k0 >= d->K || k1 >= d->K) return fail(LRC_ERR_INVALID_ARG, std::string("lrc_deform_span_dev: keyframe index of shape ") + which + " out of range");
    if (!(w >= 0.0f && w <= 1.0f)) return fail(LRC_ERR_INVALID_ARG, std::string("lrc_deform_span_dev: w of shape ") + which + " must lie in [0, 1]");
    return LRC_OK;
}

}  // namespace

int span_cast(lrc_deform* d, const float* d_rays6, const uint8_t* d_keep, const double* d_fire, uint64_t rays_per_pose, uint64_t n,
              const lrc_hits& out, hipStream_t st) {
    if (!n) return LRC_OK;
    lrc_scene* s = d->scene;
    if (!d->spanned || !d->d_span_rec || !s->info.num_nodes || !rays_per_pose)
        return fail(LRC_ERR_INTERNAL, "span_cast: the deformable holds no span");
    if (blocks_of(n, kSpanTrace) > 0x7FFFFFFFull) return fail(LRC_ERR_INVALID_ARG, "lrc_scan_mover_sweeps: too many rays for one call");
    SpanTrace q{};
    q.nodes = s->d_nodes; q.rec = (const float4*)d->d_span_rec; q.slot_prim = s->d_slot_prim; q.slot_label = s->d_slot_label;
    q.rays6 = d_rays6; q.keep = d_keep; q.fire = d_fire; q.rays_per_pose = rays_per_pose; q.total = n;
    q.t = out.t; q.prim = out.prim; q.normal3 = out.normal3; q.sem = out.sem; q.ins = out.ins;
    hipLaunchKernelGGL(span_trace_kernel, dim3((uint32_t)blocks_of(n, kSpanTrace)), dim3(kSpanTrace), 0, st, q);
    LRC_HIP(hipGetLastError());
    s->launches += 1;
    s->rays += n;
    return LRC_OK;
}

extern "C" {

int lrc_deform_span_dev(lrc_deform* d, uint32_t k0a, uint32_t k1a, float wa, uint32_t k0b, uint32_t k1b, float wb, void* stream) {
    if (!d) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_span_dev: deform is NULL");
    int rc;
    if ((rc = check_shape(d, "A", k0a, k1a, wa)) || (rc = check_shape(d, "B", k0b, k1b, wb))) return rc;
    LRC_HIP(hipSetDevice(d->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    lrc_scene* s = d->scene;
    const uint32_t S = (uint32_t)s->info.num_slots;
    if (!d->d_span_rec) {                 // the first span of this deformable: the three extra arrays
        const size_t vert_bytes = (size_t)d->V * 12, box_bytes = (size_t)S * 24, rec_bytes = (size_t)S * lrcspan::kRecFloats * 4;
        LRC_HIP(hipMalloc((void**)&d->d_verts_b, vert_bytes ? vert_bytes : 4));
        LRC_HIP(hipMalloc((void**)&d->d_span_box, box_bytes ? box_bytes : 4));
        LRC_HIP(hipMalloc((void**)&d->d_span_rec, rec_bytes ? rec_bytes : 16));
        s->info.device_bytes += vert_bytes + box_bytes + rec_bytes;
    }
    // shape A as lrc_deform_set_dev leaves it in the vertices, the records and the exact slot boxes; B beside it; the node boxes
    // from the span boxes
    if ((rc = deform_shape_enqueue(d, k0a, k1a, wa, d->d_verts, st))) return rc;
    if ((rc = deform_slots_enqueue(d, st))) return rc;
    if ((rc = deform_shape_enqueue(d, k0b, k1b, wb, d->d_verts_b, st))) return rc;
    hipLaunchKernelGGL(k_span_slots, dim3((uint32_t)blocks_of(S, kSpanBlock)), dim3(kSpanBlock), 0, st, (const float*)d->d_verts,
                       (const float*)d->d_verts_b, (const uint32_t*)d->d_tris3, (const uint32_t*)s->d_slot_prim, S,
                       (float4*)d->d_span_rec, d->d_span_box);
    LRC_HIP(hipGetLastError());
    if ((rc = deform_nodes_enqueue(d, d->d_span_box, st))) return rc;
    d->spanned = true;
    return LRC_OK;
}

int lrc_deform_span_launches(const lrc_deform* d, uint32_t* blended, uint32_t* copied) {
    if (!d) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_span_launches: deform is NULL");
    uint32_t set_blended = 0, set_copied = 0;
    const int rc = lrc_deform_launches(d, &set_blended, &set_copied);
    if (rc) return rc;
    // one set's launches (shape, k_slots, the node refit) plus the second shape and k_span_slots
    if (blended) *blended = set_blended + 2u;
    if (copied) *copied = set_copied + (d->B ? 2u : 1u);
    return LRC_OK;
}

int lrc_span_vertices(const float* a3, const float* b3, uint64_t num_vertices, float s, float* out3) {
    if (num_vertices && (!a3 || !b3 || !out3)) return fail(LRC_ERR_INVALID_ARG, "lrc_span_vertices: NULL argument");
    if (!(s >= 0.0f && s <= 1.0f)) return fail(LRC_ERR_INVALID_ARG, "lrc_span_vertices: s must lie in [0, 1]");
    for (uint64_t i = 0; i < num_vertices * 3; ++i) out3[i] = lrcspan::span_vertex(a3[i], b3[i], s);
    return LRC_OK;
}

int lrc_deform_span_refit(const float* nodes16, uint64_t num_nodes, const uint32_t* slot_prim, uint64_t num_slots, const uint32_t* tris3,
                          uint64_t T, const float* va3, const float* vb3, uint64_t V, float* out_nodes16, float* out_span_box6,
                          float* out_span_rec18) {
    if ((num_nodes && (!nodes16 || !out_nodes16)) || (num_slots && (!slot_prim || !tris3 || !va3 || !vb3 || !out_span_box6)))
        return fail(LRC_ERR_INVALID_ARG, "lrc_deform_span_refit: NULL argument");
    for (uint64_t s = 0; s < num_slots; ++s)
        if (slot_prim[s] >= T) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_span_refit: a slot names a triangle row >= T");
    for (uint64_t i = 0; i < 3 * T; ++i)
        if (tris3[i] >= V) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_span_refit: triangle index out of range");
    std::vector<uint32_t> order;
    if (!deform_height_table(nodes16, num_nodes, num_slots, order))
        return fail(LRC_ERR_INVALID_ARG, "lrc_deform_span_refit: the nodes are no tree over the slots (a reference out of range, a leaf "
                                         "past the slots or above 4 entries, or a node reached twice)");
    if (num_nodes && out_nodes16 != nodes16) std::memmove(out_nodes16, nodes16, num_nodes * 64);
    for (uint64_t s = 0; s < num_slots; ++s)
        lrcspan::slot_span(va3, vb3, tris3, slot_prim[s], out_span_rec18 ? out_span_rec18 + 18 * s : nullptr, out_span_box6 + 6 * s);
    for (uint32_t n : order) lrcdef::node_refit(out_nodes16 + 16 * (uint64_t)n, out_nodes16, out_span_box6);     // height by height
    return LRC_OK;
}

}  // extern "C"
