// lrc_skin.hip -- skinned deforming movers (include/lidarcast.h "skinned deforming movers"): a
// deformable whose shapes are not K whole vertex arrays but a rest shape, up to four bone influences per vertex and K key
// poses of B bones.  Key pose k is "keyframe k": lrc_deform_set_dev skins the two key poses and blends them into d_verts, the
// bytes a keyframe deformable of the host-skinned keyframes holds, and the refit of lrc_deform.hip follows unchanged.
//
//   k_skin<TWO>   one thread per vertex, 256-wide blocks.  Every vertex of a block reads the pose's bone table with its own
//                 lane's bone indices, so the block first stages the table (two for TWO) in LDS: a strided cooperative load of
//                 12 * B floats per pose, one __syncthreads(), then per lane lrcskin::skin1 on LDS operands (and
//                 lrcdef::blend1 for TWO).  Dynamic LDS, 48 * B bytes per pose: a six-bone rig takes 288 B, the largest table
//                 (B = 255) 12 240 B per pose.
// The host functions run the same inline functions on arrays, without a GPU: lrc_skin_apply, and the pass of
// lrc_deform_create_skinned that skins every key pose once for the checks, the bounds and the scene of key pose 0.
#include <cmath>
#include <cstring>

#include "lrc_internal.h"
#include "lrc_skin.h"

namespace {

constexpr int kSkinBlock = 256;

template <bool TWO>
__global__ __launch_bounds__(kSkinBlock) void k_skin(const float* rest3, const uint32_t* idx4, const float4* wgt4, const float* bones_a,
                                                     const float* bones_b, uint32_t n12, float w, float* out3, uint64_t V) {
    extern __shared__ float s_bones[];          // n12 floats of pose a, then (TWO) n12 floats of pose b
    for (uint32_t i = threadIdx.x; i < n12; i += kSkinBlock) {
        s_bones[i] = bones_a[i];
        if (TWO) s_bones[n12 + i] = bones_b[i];
    }
    __syncthreads();
    const uint64_t v = (uint64_t)blockIdx.x * kSkinBlock + threadIdx.x;
    if (v >= V) return;
    const uint32_t packed = idx4[v];
    const float4 wg = wgt4[v];
    const uint8_t idx[4] = {(uint8_t)(packed & 255u), (uint8_t)((packed >> 8) & 255u), (uint8_t)((packed >> 16) & 255u),
                            (uint8_t)(packed >> 24)};
    const float wgt[4] = {wg.x, wg.y, wg.z, wg.w};
    const float p[3] = {rest3[3 * v], rest3[3 * v + 1], rest3[3 * v + 2]};
    float a[3];
    lrcskin::skin1(s_bones, idx, wgt, p, a);
    if (TWO) {
        float b[3];
        lrcskin::skin1(s_bones + n12, idx, wgt, p, b);
#pragma unroll
        for (int i = 0; i < 3; ++i) a[i] = lrcdef::blend1(a[i], b[i], w);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) out3[3 * v + i] = a[i];
}

}  // namespace

int skin_enqueue(lrc_deform* d, uint32_t k0, uint32_t k1, float w, float* d_out, hipStream_t st) {
    if (!d->V) return LRC_OK;
    const uint32_t n12 = 12u * d->B;
    const dim3 grid((uint32_t)blocks_of(d->V, kSkinBlock)), block(kSkinBlock);
    if (w == 0.0f || w == 1.0f || k0 == k1) {              // one key pose: skinned, nothing blended
        const float* bones = d->d_poses + (uint64_t)((w == 1.0f) ? k1 : k0) * n12;
        hipLaunchKernelGGL(k_skin<false>, grid, block, n12 * sizeof(float), st, (const float*)d->d_rest, (const uint32_t*)d->d_idx4,
                           (const float4*)d->d_wgt4, bones, bones, n12, w, d_out, d->V);
    } else {
        hipLaunchKernelGGL(k_skin<true>, grid, block, 2 * n12 * sizeof(float), st, (const float*)d->d_rest, (const uint32_t*)d->d_idx4,
                           (const float4*)d->d_wgt4, (const float*)(d->d_poses + (uint64_t)k0 * n12),
                           (const float*)(d->d_poses + (uint64_t)k1 * n12), n12, w, d_out, d->V);
    }
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

extern "C" {

int lrc_skin_apply(const float* rest3, uint64_t V, const uint8_t* idx4, const float* wgt4, const float* bones12, uint32_t B,
                   float* out3) {
    if (B < 1 || B > lrcskin::kMaxBones) return fail(LRC_ERR_INVALID_ARG, "lrc_skin_apply: B = " + std::to_string(B) + " bones (1 <= B <= 255)");
    if (!bones12 || (V && (!rest3 || !idx4 || !wgt4 || !out3))) return fail(LRC_ERR_INVALID_ARG, "lrc_skin_apply: NULL argument");
    for (uint64_t i = 0; i < 4 * V; ++i)
        if (idx4[i] >= B)
            return fail(LRC_ERR_INVALID_ARG, "lrc_skin_apply: vertex " + std::to_string(i / 4) + " names bone " + std::to_string(idx4[i]) +
                                                 " of " + std::to_string(B));
    for (uint64_t v = 0; v < V; ++v) lrcskin::skin1(bones12, idx4 + 4 * v, wgt4 + 4 * v, rest3 + 3 * v, out3 + 3 * v);
    return LRC_OK;
}

int lrc_deform_create_skinned(lrc_ctx* ctx, const float* rest3, uint64_t V, const uint8_t* idx4, const float* wgt4,
                              const float* poses12, uint32_t K, uint32_t B, const uint32_t* tris3, uint64_t T, const uint16_t* tri_sem,
                              const uint16_t* tri_ins, lrc_deform** out) {
    const std::string who = "lrc_deform_create_skinned";
    if (!out) return fail(LRC_ERR_INVALID_ARG, who + ": out is NULL");
    *out = nullptr;
    // everything is checked before the first launch, the arrays before the context
    if (B < 1 || B > lrcskin::kMaxBones) return fail(LRC_ERR_INVALID_ARG, who + ": B = " + std::to_string(B) + " bones (1 <= B <= 255)");
    if (K == 0 || T == 0) return fail(LRC_ERR_INVALID_ARG, who + ": a deformable needs at least one key pose and one triangle");
    if (!rest3 || !idx4 || !wgt4 || !poses12 || !tris3) return fail(LRC_ERR_INVALID_ARG, who + ": NULL rest, influence, pose or triangle array");
    if (T >= (1ull << 28) || V >= (1ull << 32)) return fail(LRC_ERR_INVALID_ARG, who + ": mesh too large (T < 2^28, V < 2^32)");
    for (uint64_t i = 0; i < 3 * T; ++i)
        if (tris3[i] >= V) return fail(LRC_ERR_INVALID_ARG, who + ": triangle index out of range");
    for (uint64_t v = 0; v < V; ++v) {
        double sum = 0.0;
        for (int j = 0; j < 4; ++j) {
            if (idx4[4 * v + j] >= B)
                return fail(LRC_ERR_INVALID_ARG, who + ": vertex " + std::to_string(v) + " names bone " + std::to_string(idx4[4 * v + j]) +
                                                     " of " + std::to_string(B));
            const float wj = wgt4[4 * v + j];
            if (!(std::isfinite(wj) && wj >= 0.0f))
                return fail(LRC_ERR_INVALID_ARG, who + ": vertex " + std::to_string(v) + " has a weight that is not finite or is negative");
            sum += (double)wj;
        }
        if (!(std::fabs(sum - 1.0) <= 0x1p-10))
            return fail(LRC_ERR_INVALID_ARG, who + ": the weights of vertex " + std::to_string(v) + " sum to " + std::to_string(sum) +
                                                 " (1 within 2^-10)");
    }
    for (uint64_t i = 0; i < (uint64_t)K * B * 12; ++i)
        if (!std::isfinite(poses12[i]))
            return fail(LRC_ERR_INVALID_ARG, who + ": key pose " + std::to_string(i / ((uint64_t)B * 12)) + ", bone " +
                                                 std::to_string(i / 12 % B) + " has an entry that is not finite");
    // the host skins the K key poses one at a time with the kernel's own skin1 and keeps only key pose 0: every coordinate is
    // checked, and the union box over the vertices triangles use becomes the scene's fixed bounds.  A blended vertex lies in
    // the box of its two skinned ends (the clamp of blend1) and the device skins with the same skin1, so the movers' cull
    // sphere made from these bounds stays valid without a read-back.
    std::vector<float> first((size_t)V * 3), work;
    int lo[3] = {0x7F7FFFFF, 0x7F7FFFFF, 0x7F7FFFFF}, hi[3] = {(int)0x80800000u, (int)0x80800000u, (int)0x80800000u};
    {
        std::vector<uint8_t> used(V, 0);
        for (uint64_t i = 0; i < 3 * T; ++i) used[tris3[i]] = 1;
        if (K > 1) work.resize((size_t)V * 3);
        for (uint32_t k = 0; k < K; ++k) {
            float* dst = k == 0 ? first.data() : work.data();
            const float* bones = poses12 + (uint64_t)k * B * 12;
            for (uint64_t v = 0; v < V; ++v) {
                float* q = dst + 3 * v;
                lrcskin::skin1(bones, idx4 + 4 * v, wgt4 + 4 * v, rest3 + 3 * v, q);
                for (int a = 0; a < 3; ++a)
                    if (!deform_coordinate_ok(q[a]))
                        return fail(LRC_ERR_INVALID_ARG, who + ": key pose " + std::to_string(k) + " puts vertex " + std::to_string(v) +
                                                             " at a coordinate that is not finite or exceeds 1e6");
                if (!used[v]) continue;
                for (int a = 0; a < 3; ++a) { lo[a] = lrctri::imin(lo[a], lrctri::enc(q[a])); hi[a] = lrctri::imax(hi[a], lrctri::enc(q[a])); }
            }
        }
    }
    if (!ctx) return fail(LRC_ERR_INVALID_ARG, who + ": ctx is NULL");
    LRC_HIP(hipSetDevice(ctx->device));

    lrc_deform* d = new (std::nothrow) lrc_deform();
    if (!d) return fail(LRC_ERR_OOM, who + ": out of host memory");
    d->ctx = ctx; d->K = K; d->V = V; d->T = T; d->B = B;
    auto bail = [&](int rc) { const std::string keep = lrc_last_error(); lrc_deform_destroy(d); return fail(rc, keep); };
    int rc = deform_build(d, who.c_str(), first.data(), tris3, tri_sem, tri_ins, lo, hi);
    if (rc) return bail(rc);
    auto hip = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return LRC_OK;
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? LRC_ERR_OOM : LRC_ERR_HIP, who + ": " + what + ": " + hipGetErrorString(e));
    };
    const size_t rest_bytes = (size_t)V * 12, idx_bytes = (size_t)V * 4, wgt_bytes = (size_t)V * 16, pose_bytes = (size_t)K * B * 48;
    if ((rc = hip(hipMalloc((void**)&d->d_rest, rest_bytes ? rest_bytes : 4), "rest shape")) ||
        (rc = hip(hipMalloc((void**)&d->d_idx4, idx_bytes ? idx_bytes : 4), "bone indices")) ||
        (rc = hip(hipMalloc((void**)&d->d_wgt4, wgt_bytes ? wgt_bytes : 16), "bone weights")) ||
        (rc = hip(hipMalloc((void**)&d->d_poses, pose_bytes), "key poses")) ||
        (rc = hip(hipMemcpy(d->d_rest, rest3, rest_bytes, hipMemcpyHostToDevice), "rest shape upload")) ||
        (rc = hip(hipMemcpy(d->d_idx4, idx4, idx_bytes, hipMemcpyHostToDevice), "bone index upload")) ||
        (rc = hip(hipMemcpy(d->d_wgt4, wgt4, wgt_bytes, hipMemcpyHostToDevice), "bone weight upload")) ||
        (rc = hip(hipMemcpy(d->d_poses, poses12, pose_bytes, hipMemcpyHostToDevice), "key pose upload")))
        return bail(rc);
    d->scene->info.device_bytes += rest_bytes + idx_bytes + wgt_bytes + pose_bytes;
    *out = d;
    return LRC_OK;
}

}  // extern "C"
