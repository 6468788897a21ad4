// lrc_deform.hip -- deforming movers (include/lidarcast.h "deforming movers"): a scene built once from
// keyframe 0 whose vertices are blended between two keyframes and whose triangle records, slot boxes and node boxes are
// refitted on the device, in stream order, without rebuilding the tree.  DESIGN.md section 4 ("BVH result == brute force")
// holds for ANY tree whose child boxes are the exact vertex min / max below them, so the refitted tree gives the hits of a
// fresh build bit for bit.
//
//   k_blend   one thread per coordinate: lrcdef::blend1
//   k_slots   one thread per leaf slot: the 48-byte record and the slot box of triangle slot_prim[s] (lrcdef::slot_refit)
//   k_level   one thread per inner node of ONE height: both child boxes (lrcdef::node_refit).  A node reads only nodes of a
//             smaller height, written by an earlier launch: the kernel boundary is the only ordering between heights.
//   k_tail    ONE workgroup finishes every height from `first` up, __syncthreads() between heights: the writer and the
//             reader of a box sit on one CU, so no other workgroup's cache is involved.
// The host functions lrc_deform_blend and lrc_deform_refit run the same inline functions on arrays, without a GPU.
// A skinned deformable (lrc_skin.hip) is the same handle: its vertices come from k_skin instead of k_blend
// or the keyframe copy, and creation (deform_build) and the refit launches (deform_refit_enqueue) are shared with it.
// A span between two shapes (lrc_span.hip) takes the same pieces apart: the shape of a triple into any
// vertex array (deform_shape_enqueue), k_slots alone (deform_slots_enqueue), and k_level / k_tail from slot boxes of the
// caller's choice (deform_nodes_enqueue).
#include <cmath>
#include <cstring>

#include "lrc_internal.h"
#include "lrc_deform.h"

// struct lrc_deform: lrc_internal.h (lrc_skin.hip makes skinned ones)

namespace {

constexpr int kDefBlock = 256;
constexpr uint32_t kTailMax = 256;    // the tail takes over from the first height that holds at most this many nodes

__global__ __launch_bounds__(kDefBlock) void k_blend(const float* a, const float* b, float w, float* out, uint64_t n3) {
    const uint64_t i = (uint64_t)blockIdx.x * kDefBlock + threadIdx.x;
    if (i < n3) out[i] = lrcdef::blend1(a[i], b[i], w);
}

__global__ __launch_bounds__(kDefBlock) void k_slots(const float* verts3, const uint32_t* tris3, const uint32_t* slot_prim,
                                                     uint32_t num_slots, float4* out_tris, float* slot_box) {
    const uint32_t s = blockIdx.x * kDefBlock + threadIdx.x;
    if (s >= num_slots) return;
    float r[12], bx[6];
    lrcdef::slot_refit(verts3, tris3, slot_prim[s], r, bx);
    float4* o = out_tris + (size_t)s * 3;
    o[0] = make_float4(r[0], r[1], r[2], r[3]);
    o[1] = make_float4(r[4], r[5], r[6], r[7]);
    o[2] = make_float4(r[8], r[9], r[10], r[11]);
#pragma unroll
    for (int k = 0; k < 6; ++k) slot_box[(size_t)s * 6 + k] = bx[k];
}

__global__ __launch_bounds__(kDefBlock) void k_level(float* nodes, const float* slot_box, const uint32_t* order, uint32_t n) {
    const uint32_t i = blockIdx.x * kDefBlock + threadIdx.x;
    if (i < n) lrcdef::node_refit(nodes + 16 * (size_t)order[i], nodes, slot_box);
}

struct TailArgs { uint32_t off[lrc::kMaxDepth + 2]; uint32_t first, heights; };

__global__ __launch_bounds__(kDefBlock) void k_tail(float* nodes, const float* slot_box, const uint32_t* order, const TailArgs a) {
    for (uint32_t h = a.first; h < a.heights; ++h) {
        for (uint32_t i = a.off[h] + threadIdx.x; i < a.off[h + 1]; i += kDefBlock)
            lrcdef::node_refit(nodes + 16 * (size_t)order[i], nodes, slot_box);
        __syncthreads();
    }
}

// Every inner node's height (0 when both children are leaves, else 1 + the larger height of its inner children) and the node
// indices grouped by height, from the 16-float nodes; walks from node 0.  false: a reference out of range, a leaf that runs
// past the slots, or a node reached twice (no tree).
bool height_table(const float* nodes, uint64_t num_nodes, uint64_t num_slots, std::vector<uint32_t>& order,
                  std::vector<uint32_t>& level_off) {
    order.clear();
    level_off.assign(1, 0u);
    if (num_nodes == 0) return true;
    if (num_nodes > 0x7FFFFFFFull) return false;
    std::vector<int32_t> height(num_nodes, -1);
    std::vector<uint8_t> seen(num_nodes, 0);
    std::vector<std::pair<uint32_t, int>> stack;       // (node, next child to visit)
    stack.emplace_back(0u, 0);
    seen[0] = 1;
    int32_t top = 0;
    while (!stack.empty()) {
        const uint32_t n = stack.back().first;
        const int c = stack.back().second;
        if (c < 2) {
            stack.back().second = c + 1;
            int32_t ref;
            std::memcpy(&ref, &nodes[16 * (uint64_t)n + 12 + c], 4);
            if (ref < 0) {
                const uint32_t code = (uint32_t)(~ref), first = code >> 3, cnt = code & 7u;
                if (cnt > (uint32_t)lrc::kMaxLeaf || (uint64_t)first + cnt > num_slots) return false;
            } else {
                if ((uint64_t)ref >= num_nodes || seen[ref]) return false;
                seen[ref] = 1;
                stack.emplace_back((uint32_t)ref, 0);
            }
            continue;
        }
        int32_t h = 0;
        for (int k = 0; k < 2; ++k) {
            int32_t ref;
            std::memcpy(&ref, &nodes[16 * (uint64_t)n + 12 + k], 4);
            if (ref >= 0) h = std::max(h, height[ref] + 1);
        }
        height[n] = h;
        top = std::max(top, h);
        stack.pop_back();
    }
    level_off.assign((size_t)top + 2, 0u);
    for (uint64_t n = 0; n < num_nodes; ++n)
        if (height[n] >= 0) ++level_off[(size_t)height[n] + 1];
    for (size_t h = 0; h + 1 < level_off.size(); ++h) level_off[h + 1] += level_off[h];
    order.resize(level_off.back());
    std::vector<uint32_t> cur(level_off.begin(), level_off.end() - 1);
    for (uint64_t n = 0; n < num_nodes; ++n)
        if (height[n] >= 0) order[cur[(size_t)height[n]]++] = (uint32_t)n;
    return true;
}

}  // namespace

DeformMesh deform_mesh(const lrc_deform* d) { return DeformMesh{d->d_verts, d->d_tris3, d->V, d->T}; }

int deform_build(lrc_deform* d, const char* who, const float* verts0_3, const uint32_t* tris3, const uint16_t* tri_sem,
                 const uint16_t* tri_ins, const int lo[3], const int hi[3]) {
    lrc_ctx* ctx = d->ctx;
    const uint64_t V = d->V, T = d->T;
    // float32 nodes whatever LRC_QNODES says: the quantisation grid is tied to bounds that a deformation moves
    int rc = scene_create_mode(ctx, verts0_3, V, tris3, T, tri_sem, tri_ins, 0, &d->scene);
    if (rc) return rc;
    lrc_scene* s = d->scene;
    s->deform = d;
    for (int a = 0; a < 3; ++a) { s->info.bounds_lo[a] = lrctri::dec(lo[a]); s->info.bounds_hi[a] = lrctri::dec(hi[a]); }

    // the height table, on the host from the exported nodes
    std::vector<float> nodes(s->info.num_nodes * 16);
    std::vector<uint32_t> order;
    auto hip = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return LRC_OK;
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? LRC_ERR_OOM : LRC_ERR_HIP, std::string(who) + ": " + what + ": " + hipGetErrorString(e));
    };
    if ((rc = hip(hipMemcpy(nodes.data(), s->d_nodes, nodes.size() * 4, hipMemcpyDeviceToHost), "node read-back"))) return rc;
    if (!height_table(nodes.data(), s->info.num_nodes, s->info.num_slots, order, d->level_off) || order.size() != s->info.num_nodes ||
        d->level_off.size() > (size_t)lrc::kMaxDepth + 2)
        return fail(LRC_ERR_INTERNAL, std::string(who) + ": the built tree has no height table");
    const uint32_t heights = (uint32_t)d->level_off.size() - 1;
    d->tail_first = heights;
    if (env_int("LRC_DEFORM_TAIL", 1) != 0)        // 0: one launch per height to the top (the A/B of tools/deform_time.py)
        for (uint32_t h = 0; h < heights; ++h)
            if (d->level_off[h + 1] - d->level_off[h] <= kTailMax) { d->tail_first = h; break; }

    const size_t vert_bytes = (size_t)V * 12, tri_bytes = (size_t)T * 12, ord_bytes = order.size() * 4;
    if ((rc = hip(hipMalloc((void**)&d->d_verts, vert_bytes ? vert_bytes : 4), "vertices")) ||
        (rc = hip(hipMalloc((void**)&d->d_tris3, tri_bytes), "triangles")) ||
        (rc = hip(hipMalloc((void**)&d->d_order, ord_bytes ? ord_bytes : 4), "height table")) ||
        (rc = hip(hipMemcpy(d->d_verts, verts0_3, vert_bytes, hipMemcpyHostToDevice), "vertex upload")) ||
        (rc = hip(hipMemcpy(d->d_tris3, tris3, tri_bytes, hipMemcpyHostToDevice), "triangle upload")) ||
        (rc = hip(hipMemcpy(d->d_order, order.data(), ord_bytes, hipMemcpyHostToDevice), "height table upload")))
        return rc;
    s->info.device_bytes += vert_bytes + tri_bytes + ord_bytes;
    return LRC_OK;
}

int deform_slots_enqueue(lrc_deform* d, hipStream_t st) {
    lrc_scene* s = d->scene;
    const uint32_t S = (uint32_t)s->info.num_slots;
    hipLaunchKernelGGL(k_slots, dim3((uint32_t)blocks_of(S, kDefBlock)), dim3(kDefBlock), 0, st, (const float*)d->d_verts,
                       (const uint32_t*)d->d_tris3, (const uint32_t*)s->d_slot_prim, S, s->d_tris, s->d_slot_box);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int deform_nodes_enqueue(lrc_deform* d, const float* d_slot_box, hipStream_t st) {
    lrc_scene* s = d->scene;
    const uint32_t heights = (uint32_t)d->level_off.size() - 1;
    for (uint32_t h = 0; h < d->tail_first; ++h) {
        const uint32_t n = d->level_off[h + 1] - d->level_off[h];
        hipLaunchKernelGGL(k_level, dim3((uint32_t)blocks_of(n, kDefBlock)), dim3(kDefBlock), 0, st, (float*)s->d_nodes,
                           d_slot_box, (const uint32_t*)(d->d_order + d->level_off[h]), n);
    }
    if (d->tail_first < heights) {
        TailArgs a{};
        for (uint32_t h = 0; h <= heights; ++h) a.off[h] = d->level_off[h];
        a.first = d->tail_first; a.heights = heights;
        hipLaunchKernelGGL(k_tail, dim3(1), dim3(kDefBlock), 0, st, (float*)s->d_nodes, d_slot_box, (const uint32_t*)d->d_order, a);
    }
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int deform_refit_enqueue(lrc_deform* d, hipStream_t st) {
    const int rc = deform_slots_enqueue(d, st);
    return rc ? rc : deform_nodes_enqueue(d, d->scene->d_slot_box, st);
}

int deform_shape_enqueue(lrc_deform* d, uint32_t k0, uint32_t k1, float w, float* d_out, hipStream_t st) {
    const uint64_t n3 = d->V * 3;
    if (d->B) return skin_enqueue(d, k0, k1, w, d_out, st);     // a skinned deformable: k_skin writes the vertices (lrc_skin.hip)
    if (!n3) return LRC_OK;
    if (w == 0.0f || w == 1.0f || k0 == k1) {              // the bits of one keyframe
        const uint32_t k = (w == 1.0f) ? k1 : k0;
        LRC_HIP(hipMemcpyAsync(d_out, d->d_keys + (uint64_t)k * n3, n3 * 4, hipMemcpyDeviceToDevice, st));
    } else {
        hipLaunchKernelGGL(k_blend, dim3((uint32_t)blocks_of(n3, kDefBlock)), dim3(kDefBlock), 0, st,
                           (const float*)(d->d_keys + (uint64_t)k0 * n3), (const float*)(d->d_keys + (uint64_t)k1 * n3), w, d_out, n3);
        LRC_HIP(hipGetLastError());
    }
    return LRC_OK;
}

bool deform_height_table(const float* nodes, uint64_t num_nodes, uint64_t num_slots, std::vector<uint32_t>& order) {
    std::vector<uint32_t> level_off;
    return height_table(nodes, num_nodes, num_slots, order, level_off);
}

extern "C" {

int lrc_deform_destroy(lrc_deform* d) {
    if (!d) return LRC_OK;
    if (d->ctx) (void)hipSetDevice(d->ctx->device);
    for (void* p : {(void*)d->d_keys, (void*)d->d_verts, (void*)d->d_tris3, (void*)d->d_order, (void*)d->d_rest, (void*)d->d_idx4,
                    (void*)d->d_wgt4, (void*)d->d_poses, (void*)d->d_verts_b, (void*)d->d_span_box, (void*)d->d_span_rec})
        if (p) (void)hipFree(p);
    if (d->scene) {
        d->scene->deform = nullptr;
        lrc_scene_destroy(d->scene);
    }
    delete d;
    return LRC_OK;
}

int lrc_deform_create(lrc_ctx* ctx, const float* keyframes3, uint32_t K, uint64_t V, const uint32_t* tris3, uint64_t T,
                      const uint16_t* tri_sem, const uint16_t* tri_ins, lrc_deform** out) {
    if (!out) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_create: out is NULL");
    *out = nullptr;
    // everything is checked before the first launch
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_create: ctx is NULL");
    if (K == 0 || T == 0) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_create: a deformable needs at least one keyframe and one triangle");
    if (!keyframes3 || !tris3) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_create: NULL keyframe or triangle array");
    if (T >= (1ull << 28) || V >= (1ull << 32)) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_create: mesh too large (T < 2^28, V < 2^32)");
    for (uint64_t i = 0; i < 3 * T; ++i)
        if (tris3[i] >= V) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_create: triangle index out of range");
    for (uint64_t i = 0; i < (uint64_t)K * V * 3; ++i)
        if (!deform_coordinate_ok(keyframes3[i]))
            return fail(LRC_ERR_INVALID_ARG, "lrc_deform_create: keyframe " + std::to_string(i / (V * 3)) +
                                                 " has a coordinate that is not finite or exceeds 1e6");
    // bounds: the union of every keyframe's box over the vertices triangles use, fixed for the deformable's life.  A blended
    // vertex lies in the box of its two keyframes (the clamp of blend1), so the movers' cull sphere made from these bounds at
    // every scan stays valid without a read-back.
    int lo[3] = {0x7F7FFFFF, 0x7F7FFFFF, 0x7F7FFFFF}, hi[3] = {(int)0x80800000u, (int)0x80800000u, (int)0x80800000u};
    {
        std::vector<uint8_t> used(V, 0);
        for (uint64_t i = 0; i < 3 * T; ++i) used[tris3[i]] = 1;
        for (uint32_t k = 0; k < K; ++k)
            for (uint64_t v = 0; v < V; ++v) {
                if (!used[v]) continue;
                const float* p = keyframes3 + ((uint64_t)k * V + v) * 3;
                for (int a = 0; a < 3; ++a) { lo[a] = lrctri::imin(lo[a], lrctri::enc(p[a])); hi[a] = lrctri::imax(hi[a], lrctri::enc(p[a])); }
            }
    }
    LRC_HIP(hipSetDevice(ctx->device));

    lrc_deform* d = new (std::nothrow) lrc_deform();
    if (!d) return fail(LRC_ERR_OOM, "lrc_deform_create: out of host memory");
    d->ctx = ctx; d->K = K; d->V = V; d->T = T;
    auto bail = [&](int rc) { const std::string keep = lrc_last_error(); lrc_deform_destroy(d); return fail(rc, keep); };
    int rc = deform_build(d, "lrc_deform_create", keyframes3, tris3, tri_sem, tri_ins, lo, hi);
    if (rc) return bail(rc);
    auto hip = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return LRC_OK;
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? LRC_ERR_OOM : LRC_ERR_HIP, std::string("lrc_deform_create: ") + what + ": " + hipGetErrorString(e));
    };
    const size_t key_bytes = (size_t)K * V * 12;
    if ((rc = hip(hipMalloc((void**)&d->d_keys, key_bytes ? key_bytes : 4), "keyframes")) ||
        (rc = hip(hipMemcpy(d->d_keys, keyframes3, key_bytes, hipMemcpyHostToDevice), "keyframe upload")))
        return bail(rc);
    d->scene->info.device_bytes += key_bytes;
    *out = d;
    return LRC_OK;
}

lrc_scene* lrc_deform_scene(lrc_deform* d) { return d ? d->scene : nullptr; }

int lrc_deform_launches(const lrc_deform* d, uint32_t* blended, uint32_t* copied) {
    if (!d) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_launches: deform is NULL");
    const uint32_t heights = (uint32_t)d->level_off.size() - 1;
    const uint32_t refit = 1u + d->tail_first + (d->tail_first < heights ? 1u : 0u);
    if (blended) *blended = 1u + refit;
    if (copied) *copied = d->B ? 1u + refit : refit;     // a skinned deformable skins where a keyframe is copied
    return LRC_OK;
}

int lrc_deform_set_dev(lrc_deform* d, uint32_t k0, uint32_t k1, float w, void* stream) {
    if (!d) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_set_dev: deform is NULL");
    if (k0 >= d->K || k1 >= d->K) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_set_dev: keyframe index out of range");
    if (!(w >= 0.0f && w <= 1.0f)) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_set_dev: w must lie in [0, 1]");
    LRC_HIP(hipSetDevice(d->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int rc = deform_shape_enqueue(d, k0, k1, w, d->d_verts, st);
    if (rc) return rc;
    d->spanned = false;
    return deform_refit_enqueue(d, st);
}

int lrc_deform_vertices(lrc_deform* d, float* out_verts3) {
    if (!d || (d->V && !out_verts3)) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_vertices: NULL argument");
    LRC_HIP(hipSetDevice(d->ctx->device));
    LRC_HIP(hipDeviceSynchronize());
    if (d->V) LRC_HIP(hipMemcpy(out_verts3, d->d_verts, d->V * 12, hipMemcpyDeviceToHost));
    return LRC_OK;
}

int lrc_deform_snapshot_dev(lrc_deform* d, float* d_out_verts3, void* stream) {
    if (!d || !d_out_verts3) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_snapshot_dev: NULL argument");
    LRC_HIP(hipSetDevice(d->ctx->device));
    if (d->V) LRC_HIP(hipMemcpyAsync(d_out_verts3, d->d_verts, d->V * 12, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LRC_OK;
}

int lrc_deform_blend(const float* a3, const float* b3, uint64_t num_vertices, float w, float* out3) {
    if (num_vertices && (!a3 || !b3 || !out3)) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_blend: NULL argument");
    if (!(w >= 0.0f && w <= 1.0f)) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_blend: w must lie in [0, 1]");
    const uint64_t n3 = num_vertices * 3;
    if (w == 0.0f || w == 1.0f || a3 == b3) {
        if (n3) std::memmove(out3, w == 1.0f ? b3 : a3, n3 * 4);
        return LRC_OK;
    }
    for (uint64_t i = 0; i < n3; ++i) out3[i] = lrcdef::blend1(a3[i], b3[i], w);
    return LRC_OK;
}

int lrc_deform_refit(float* nodes16, uint64_t num_nodes, const uint32_t* slot_prim, uint64_t num_slots, const uint32_t* tris3,
                     uint64_t T, const float* verts3, uint64_t V, float* out_tri_rec12, float* out_slot_box6) {
    if ((num_nodes && !nodes16) || (num_slots && (!slot_prim || !tris3 || !verts3 || !out_tri_rec12 || !out_slot_box6)))
        return fail(LRC_ERR_INVALID_ARG, "lrc_deform_refit: NULL argument");
    for (uint64_t s = 0; s < num_slots; ++s)
        if (slot_prim[s] >= T) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_refit: a slot names a triangle row >= T");
    for (uint64_t i = 0; i < 3 * T; ++i)
        if (tris3[i] >= V) return fail(LRC_ERR_INVALID_ARG, "lrc_deform_refit: triangle index out of range");
    std::vector<uint32_t> order, level_off;
    if (!height_table(nodes16, num_nodes, num_slots, order, level_off))
        return fail(LRC_ERR_INVALID_ARG, "lrc_deform_refit: the nodes are no tree over the slots (a reference out of range, a leaf "
                                         "past the slots or above 4 entries, or a node reached twice)");
    for (uint64_t s = 0; s < num_slots; ++s)
        lrcdef::slot_refit(verts3, tris3, slot_prim[s], out_tri_rec12 + 12 * s, out_slot_box6 + 6 * s);
    for (uint32_t n : order) lrcdef::node_refit(nodes16 + 16 * (uint64_t)n, nodes16, out_slot_box6);     // height by height
    return LRC_OK;
}

}  // extern "C"
