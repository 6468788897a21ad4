// lrc_lab.h -- the laboratory build of lidarcast.hip (-DLRC_VARIANTS; tests/test_parity_gpu.py::
// test_kernel_variants_are_bit_identical, tools/): the measured alternatives of DESIGN.md section 4.1 that are kernels of their
// own -- private refill, the packet kernel (lrc_sector.h) -- and the dispatch that selects them, and the alternative
// instantiations of trace_kernel, by environment variables.  Every one returns the product kernel's bytes.  Included by
// lidarcast.hip alone, behind its device code and in front of launch_trace; the product build never sees it.  (The variants
// INSIDE trace_kernel's traversal -- four-wide nodes, speculative order, the force-redo hook -- stay there, under the same macro.)
#pragma once

static int ensure_prim_plane(lrc_scene* s, hipStream_t st);      // lidarcast.hip, behind this header

namespace {

// ---- measured alternative: K rays per lane with private refill (LRC_REFILL=K) -------------
// One wave owns K consecutive 64-ray tiles of a pose-batched scan; lane l traces rays l, 64+l, 128+l, ... one after the
// other, starting its next ray the moment the current one is done instead of idling until the slowest lane of the wave
// has finished ("private refill").  The closest hit (t, slot) of each ray is parked in LDS and the whole write-back
// runs afterwards, coherently, K passes of 64 lanes.  The next ray's direction is fetched while the current one is
// traced.  Same arithmetic, same result bytes as trace_kernel (tests/test_parity_gpu.py::
// test_kernel_variants_are_bit_identical); what changes is the balance of work inside a wave (tools/trav_stats.py:
// 0.68 -> 0.77 / 0.84 for K = 2 / 4) at the price of (a) refilled lanes restarting at the root while their
// neighbours are deep in the tree, which takes the wave off the scalar-fetch path, (b) K x 512 B more LDS per wave and
// 6 more VGPRs, i.e. fewer resident waves.
// W = resident waves per SIMD the register allocator must leave room for (its natural footprint is 78 / 93 VGPRs for
// K = 2 / 4, i.e. 6 / 5 waves; 7 waves cost a few spilled registers)
template <int K, int W>
__global__ __launch_bounds__(kTBlock, W) void trace_refill_kernel(const TraceParams p, uint32_t depth) {
    extern __shared__ int s_mem[];                 // [depth][64] stacks | [K][64] {t bits, slot}
    int* s_stack = s_mem;
    uint2* s_res = (uint2*)(s_mem + (size_t)depth * 64);
    const uint32_t tid = threadIdx.x;
    // the host launches this kernel only when rays_per_pose % (64 K) == 0: a wave's K tiles lie in ONE pose, so the pose
    // and everything derived from it is wave-uniform (scalar loads, SGPR operands)
    const uint64_t N = p.rays_per_pose;
    const uint64_t tile0 = (uint64_t)xcd_tile(blockIdx.x, gridDim.x) * (64u * K);
    if (tile0 >= p.total) return;
    const uint64_t pose = tile0 / N;
    const uint32_t i0 = (uint32_t)(tile0 - pose * N);
    const double* M = p.poses16 + pose * 16;
    const uint64_t base = tile0 + tid;

    V3 o, d;
    RaySlab sl;
    float tbest;
    uint32_t best_slot, best_prim;
    int sp = 0, ref = ~0;
    int k = 0;
    double nd0 = 0.0, nd1 = 0.0, nd2 = 0.0;        // next ray's sensor-frame direction, in flight

    auto fetch_next = [&](int kk) {
        if (kk < K) {
            const double* dv = p.dirs3 + (size_t)(i0 + (uint32_t)kk * 64u + tid) * 3;
            nd0 = dv[0]; nd1 = dv[1]; nd2 = dv[2];
        }
    };
    // ray kk from the prefetched direction; false when the lane has no ray kk
    auto begin = [&](int kk) -> bool {
        if (kk >= K) return false;
        d.x = (float)dgemm_row(nd0, nd1, nd2, M[0], M[1], M[2]);
        d.y = (float)dgemm_row(nd0, nd1, nd2, M[4], M[5], M[6]);
        d.z = (float)dgemm_row(nd0, nd1, nd2, M[8], M[9], M[10]);
        o.x = (float)M[3]; o.y = (float)M[7]; o.z = (float)M[11];
        sl = make_slab(o, d);
        tbest = __builtin_inff();
        best_slot = 0xFFFFFFFFu; best_prim = 0xFFFFFFFFu;
        sp = 0;
        ref = (p.num_nodes && finite_ray(o, d)) ? 0 : ~0;
        return true;
    };
    fetch_next(0);
    begin(0);
    fetch_next(1);

    auto step = [&](const F4 q0, const F4 q1, const F4 q2, const F4 q3) {
        float n0, f0, n1, f1;
        slab_interval(sl, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, n0, f0);
        slab_interval(sl, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, n1, f1);
        const bool h0 = (n0 <= f0) & (n0 <= tbest);
        const bool h1 = (n1 <= f1) & (n1 <= tbest);
        const int r0 = __float_as_int(q3.x), r1 = __float_as_int(q3.y);
        if (h0 & h1) {
            const bool first0 = n0 <= n1;
            s_stack[sp * 64 + tid] = first0 ? r1 : r0;
            ++sp;
            ref = first0 ? r0 : r1;
        } else if (h0) {
            ref = r0;
        } else if (h1) {
            ref = r1;
        } else if (sp == 0) {
            ref = ~0;
        } else {
            --sp;
            ref = s_stack[sp * 64 + tid];
        }
    };
    auto leaf = [&](const int lref) {
        const uint32_t enc = (uint32_t)(~lref);
        const uint32_t first = enc >> 3, cnt = enc & 7u;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t slot = first + j;
            const float4* tr = p.tris + (size_t)slot * 3;
            const float4 a = tr[0], b = tr[1], c = tr[2];
            const V3 v0{a.x, a.y, a.z}, e1{a.w, b.x, b.y}, e2{b.z, b.w, c.x}, ng{c.y, c.z, c.w};
            float t;
            if (tri_hit(o, d, sl, v0, e1, e2, ng, p.slot_box + (size_t)slot * 6, t)) {
                if (t < tbest) {
                    tbest = t; best_slot = slot; best_prim = 0xFFFFFFFFu;
                } else if (t == tbest) {
                    if (best_prim == 0xFFFFFFFFu) best_prim = p.slot_prim[best_slot];
                    const uint32_t pr = p.slot_prim[slot];
                    if (pr < best_prim) { best_slot = slot; best_prim = pr; }
                }
            }
        }
    };

    while (true) {
        while (ref >= 0) {
            const int uref = __builtin_amdgcn_readfirstlane(ref);
            if (__builtin_amdgcn_ballot_w64(ref != uref) == 0ull) {
                const float4* n = p.nodes + (size_t)uref * 4;
                step(ld_uniform(n), ld_uniform(n + 1), ld_uniform(n + 2), ld_uniform(n + 3));
            } else {
                const F4* n = (const F4*)(p.nodes + (size_t)ref * 4);
                step(n[0], n[1], n[2], n[3]);
            }
        }
        leaf(ref);
        if (sp != 0) {
            --sp;
            ref = s_stack[sp * 64 + tid];
            continue;
        }
        // this lane's ray is done: park its hit, start the next one
        s_res[k * 64 + tid] = make_uint2(__float_as_uint(tbest), best_slot);
        ++k;
        if (!begin(k)) break;
        fetch_next(k + 1);
    }

    // ---- coherent write-back, one pass per tile ----
#pragma unroll 1
    for (int kk = 0; kk < K; ++kk) {
        const uint64_t gid = base + (uint64_t)kk * 64u;
        double cx, cy, cz;
        gen_ray(p.poses16, p.dirs3, pose, i0 + (uint32_t)kk * 64u + tid, o, d, cx, cy, cz);
        const uint2 r = s_res[kk * 64 + tid];
        write_back<true>(p, gid, tid, o, d, cx, cy, cz, __uint_as_float(r.x), r.y);
    }
}

#include "lrc_sector.h"

// Bounding sphere of every triangle's axis-aligned box (centre and half diagonal, rounded up): what sector_kernel
// tests against a packet of rays before it runs the exact ray/triangle test.  Built on first use of the packet kernel.
__global__ __launch_bounds__(kBlock) void slot_sphere_kernel(const float* __restrict__ slot_box, uint32_t num_slots,
                                                             float4* __restrict__ sphere) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= num_slots) return;
    const float* bx = slot_box + (size_t)k * 6;
    float ctr[3];
    double hd2 = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {       // distance from the ROUNDED centre to the farthest corner
        const double lo = (double)bx[q], hi = (double)bx[3 + q];
        ctr[q] = (float)(0.5 * (lo + hi));
        const double cc = (double)ctr[q];
        const double e = fmax(hi - cc, cc - lo);
        hd2 += e * e;
    }
    const float r = (float)__builtin_sqrt(hd2);
    sphere[k] = make_float4(ctr[0], ctr[1], ctr[2], __uint_as_float(__float_as_uint(r) + 1u));    // nextafter(r, +inf), r >= 0
}

}  // namespace

// The laboratory's part of launch_trace: the variant the environment selects is launched in the place of the product kernel.
// Returns 1 when no variant is selected (the caller goes on with the product dispatch).
static int launch_trace_lab(lrc_scene* s, TraceParams& p, int gen, hipStream_t st, bool stats, uint64_t nblk, size_t lds,
                            uint32_t depth) {
    {   // A/B knob (tools/chunk_sweep*.sh): LRC_TILE_CHUNK = n (power of two) tiles per chunk, -1 = contiguous ranges
        static const int tc = env_int("LRC_TILE_CHUNK", 0);
        if (tc < 0) p.tile_chunk_log2 = 0;
        if (tc > 0 && (tc & (tc - 1)) == 0) { uint32_t k = 0; while ((1 << k) < tc) ++k; p.tile_chunk_log2 = k + 1; }
    }
    static const int force_redo = env_int("LRC_DEBUG_FORCE_REDO", 0);
    static const int leafw = env_int("LRC_LEAFW", kLeafW) == 1 ? 1 : 2, uni = env_int("LRC_UNIFORM", 1), spec = env_int("LRC_SPEC", 0);
    static const int sector = env_int("LRC_SECTOR", 1), refill = env_int("LRC_REFILL", 0);
    p.force_redo = (uint32_t)force_redo;
    // a pipelined launch (lrc_pipe_*) carries leading workgroups that scatter or assemble an earlier scan: only the product
    // dispatch sizes its grid for them (nblk + p.pre.blocks); the variants below ignore p.pre
    if (p.pre.blocks != 0u) return 1;
    const bool qn = s->d_nodes_q != nullptr, wide = s->d_nodes_q4 != nullptr;
#define LRC_LAB(G, W, U, S, Q) \
    hipLaunchKernelGGL((trace_kernel<G, W, U, S, false, Q>), dim3((uint32_t)nblk), dim3(kTBlock), lds, st, p)
#define LRC_LAB_PICK(G)                                                                              \
    do {                                                                                             \
        if (spec) { if (leafw == 2) LRC_LAB(G, 2, true, true, 0); else LRC_LAB(G, 1, true, true, 0); } \
        else if (!uni) { if (leafw == 2) LRC_LAB(G, 2, false, false, 0); else LRC_LAB(G, 1, false, false, 0); } \
        else { if (qn) LRC_LAB(G, 1, true, false, 1); else LRC_LAB(G, 1, true, false, 0); }     /* leafw == 1 */ \
    } while (0)
    if (gen == kGenGrid && sector && !stats) {
        const lrc_grid& g = *s->cur_grid;
        SectorParams q{};
        { int rc = ensure_prim_plane(s, st); if (rc) return rc; }      // the packet kernel keys rays by triangle row
        p.prim_plane = s->d_prim_plane;
        q.tp = p;
        if (!s->d_slot_sphere && s->info.num_slots) {
            LRC_HIP(hipMalloc((void**)&s->d_slot_sphere, s->info.num_slots * 16));
            s->info.device_bytes += s->info.num_slots * 16;
            hipLaunchKernelGGL(slot_sphere_kernel, dim3((uint32_t)blocks_of(s->info.num_slots, kBlock)), dim3(kBlock),
                               0, st, (const float*)s->d_slot_box, (uint32_t)s->info.num_slots, s->d_slot_sphere);
        }
        q.slot_sphere = s->d_slot_sphere;
        q.H = g.lines; q.W = g.width;
        static const int nl_env = env_int("LRC_SECTOR_LINES", 0);
        uint32_t nl = nl_env > 0 ? (uint32_t)nl_env : 8u;
        if (nl > 8u) nl = 8u;
        if (nl > g.lines) nl = g.lines;
        q.nl = nl;
        q.groups = (g.lines + nl - 1) / nl;
        q.az0 = (float)g.az0; q.az_step = (float)g.az_step;
        q.levels = s->info.max_depth + 1u;
        q.stack_cap = 128u * q.levels;
        const uint64_t P = p.total / p.rays_per_pose;
        q.num_packets = P * q.groups * (g.width / 64u);
        if (q.num_packets > 0x7FFFFFFFull) return fail(LRC_ERR_INVALID_ARG, "too many rays for one launch");
        const size_t R = (size_t)nl * 64;
        const size_t lds_s = R * 8 + R * 12 + (size_t)q.levels * 4 + (size_t)q.stack_cap * 4 + kLeafQ * 4 + kPairQ * 8;
        static const int sdiag = env_int("LRC_SECTOR_DIAG", 0);
        if (sdiag) {      // work totals of this launch, printed to stderr (tools only)
            unsigned long long* d = nullptr;
            LRC_HIP(hipMalloc((void**)&d, kSectorDiagWords * 8));
            LRC_HIP(hipMemsetAsync(d, 0, kSectorDiagWords * 8, st));
            q.diag = d;
            hipLaunchKernelGGL(sector_kernel<true>, dim3((uint32_t)q.num_packets), dim3(64), lds_s, st, q);
            unsigned long long h[kSectorDiagWords];
            LRC_HIP(hipStreamSynchronize(st));
            LRC_HIP(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
            (void)hipFree(d);
            std::fprintf(stderr, "[sector diag] packets %llu lines/packet %u: node rounds %llu, nodes %llu, leaves %llu, "
                                 "triangles %llu, pairs %llu, pair rounds %llu, candidate rays %llu, accepted %llu\n",
                         (unsigned long long)q.num_packets, nl, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
        } else {
            hipLaunchKernelGGL(sector_kernel<false>, dim3((uint32_t)q.num_packets), dim3(64), lds_s, st, q);
        }
        return LRC_OK;
    }
    if (gen == kGenGrid) gen = kGenPoses;
    if (refill > 1 && gen == kGenPoses && !stats && p.rays_per_pose % (64u * (refill >= 4 ? 4 : 2)) == 0) {
        const int K = refill >= 4 ? 4 : 2;        // K rays per lane with private refill
        const uint64_t nb = (p.total + 64ull * K - 1) / (64ull * K);
        const size_t ldsK = ((size_t)depth * 64 + (size_t)K * 64 * 2) * sizeof(int);
        static const int rw = env_int("LRC_REFILL_W", 0);
        // this kernel takes no ray table: the launch carries none, so that the consumers of a pipeline's lean record set
        // (LeanIn), who decide a tile's form by the table the launch carried, find the rows its write_back stores
        p.ray_tab = nullptr;
#define LRC_RF(KK, WW) hipLaunchKernelGGL((trace_refill_kernel<KK, WW>), dim3((uint32_t)nb), dim3(kTBlock), ldsK, st, p, depth)
        if (K == 4) { if (rw >= 7) LRC_RF(4, 7); else LRC_RF(4, 5); }
        else { if (rw >= 7) LRC_RF(2, 7); else LRC_RF(2, 6); }
#undef LRC_RF
        return LRC_OK;
    }
    if (stats) {
        if (gen == kGenPoses && qn && wide) { hipLaunchKernelGGL((trace_kernel<kGenPoses, kLeafW, true, false, true, 2>), dim3((uint32_t)nblk), dim3(kTBlock), lds, st, p); return LRC_OK; }
        return 1;
    }
    const bool plain = leafw == kLeafW && uni && !spec && !(qn && wide);
    if (plain || !gen_has_lab_variant(gen)) return 1;
    const bool wide_only = qn && wide && leafw == kLeafW && uni && !spec;
    if (gen == kGenPoses) { if (wide_only) LRC_LAB(kGenPoses, kLeafW, true, false, 2); else LRC_LAB_PICK(kGenPoses); }
    else { if (wide_only) LRC_LAB(kGenRays, kLeafW, true, false, 2); else LRC_LAB_PICK(kGenRays); }
#undef LRC_LAB_PICK
#undef LRC_LAB
    return LRC_OK;
}
