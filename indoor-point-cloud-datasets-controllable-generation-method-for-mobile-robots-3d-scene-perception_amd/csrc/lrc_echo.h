// lrc_echo.h -- beam footprint and multi-echo returns of lrc_scan_echoes_* (include/lidarcast.h "beam footprint and
// multi-echo returns"): what the trace kernel needs of an lrc_beam (kGenEchoes), and the reduction of
// one beam's K closest-hit distances to at most E echoes, written once for the host (reduce_beam) and once across the lanes of a
// beam's group (reduce_lanes: the tail of trace_kernel<kGenEchoes>, lidarcast.hip).  lrc_echo_reduce calls the former, and the
// tests compare the two through the explicit-ray path.
//
//   order     the sub-rays that hit, by (t_k, k) ascending: s_0 <= s_1 <= ...
//   clusters  a new cluster starts at m = 0 and wherever (s_m - s_(m-1)) > separation: one float32 subtraction, one float32
//             compare.  A surface seen at a grazing angle chains into one cluster however long the chain is.
//   cluster   weight n_c = members; representative = the member with the smallest k; range = the representative's t
//   echoes    clusters with n_c < min_count are discarded; the first E of the rest, in ascending order, are echoes 0..E-1
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "lrc_device.h"
#endif

namespace lrcecho {

constexpr uint32_t kMaxSubrays = 16, kMaxEchoes = 4;

// what the trace kernel needs of an lrc_beam (24 bytes)
struct Params {
    const double* offsets2;      // device: (K, 2) float64 (du_k, dv_k), radians
    uint8_t* weight;             // device, nullable: n_c per echo record, 0 for an empty slot
    float separation;            // metres
    uint8_t subrays;             // K
    uint8_t group_log2;          // lanes per beam G = 1 << group_log2
    uint8_t max_echoes;          // E
    uint8_t min_count;
};

// lanes per beam: the power of two that holds the K sub-rays and the E lanes that write the echoes (1, 2, 4, 8 or 16)
inline uint32_t group_log2_of(uint32_t K, uint32_t E) {
    const uint32_t m = K > E ? K : E;
    uint32_t g = 0;
    while ((1u << g) < m) ++g;
    return g;
}

// One beam: t[K] float32 closest-hit distances, +inf for a sub-ray without a hit (anything that is not < +inf takes no part).
// rep[E] receives the representative sub-ray of echo e (-1: empty slot), weight[E] its member count (0: empty slot).
inline void reduce_beam(const float* t, uint32_t K, uint32_t E, uint32_t min_count, float separation, int32_t* rep,
                        uint8_t* weight) {
    uint32_t order[kMaxSubrays];
    uint32_t n = 0;
    for (uint32_t k = 0; k < K; ++k) {
        if (!(t[k] < __builtin_inff())) continue;
        uint32_t m = n++;       // insertion by (t, k): k rises, so an equal t stays in front
        while (m > 0 && t[order[m - 1]] > t[k]) { order[m] = order[m - 1]; --m; }
        order[m] = k;
    }
    for (uint32_t e = 0; e < E; ++e) { rep[e] = -1; weight[e] = 0; }
    uint32_t e = 0, m = 0;
    while (m < n && e < E) {
        uint32_t count = 1, first = order[m];
        uint32_t j = m + 1;
        for (; j < n; ++j) {
            const float gap = t[order[j]] - t[order[j - 1]];
            if (gap > separation) break;
            ++count;
            if (order[j] < first) first = order[j];
        }
        if (count >= min_count) { rep[e] = (int32_t)first; weight[e] = (uint8_t)count; ++e; }
        m = j;
    }
}

#if defined(__HIPCC__)
// The same reduction across the G lanes of a beam's group: the tail of trace_kernel<kGenEchoes>, behind the traversal.  Lane
// `tid` of the wave is lane `lane` of the launch (beam * G + k) and holds sub-ray k's closest hit (tbest, slot, label; slot =
// 0xFFFFFFFF: none -- lanes k >= K cast nothing).  EVERY lane of the wave must be here: the kernel's only exit in front of it
// takes whole groups.  Lane e < E of a group then holds echo e and hands it to record(beam, rec, t, slot, label) -- the kernel
// forms the beam's AXIS ray again there and writes record rec = beam * E + e through its fused write-back -- and the weight
// goes to q.weight[rec]; an empty slot is t = +inf, slot = 0xFFFFFFFF, weight 0.  The other lanes write nothing.
template <class Record>
__device__ __forceinline__ void reduce_lanes(const Params& q, uint32_t tid, uint64_t lane, float tbest, uint32_t best_slot,
                                             uint32_t best_label, Record record) {
    const uint32_t glog = q.group_log2, G = 1u << glog, k = tid & (G - 1u), base = tid - k;
    const uint32_t gbits = (1u << G) - 1u;                // G <= 16
    const float inf = __builtin_inff();
    const bool hit = best_slot != 0xFFFFFFFFu;
    const float tk = hit ? tbest : inf;
    // who is in front of this sub-ray in the order by (t, k), and the range of the one directly in front
    uint32_t less = 0u;
    float pred = -inf;
    for (uint32_t j = 0; j < G; ++j) {
        const float tj = __shfl(tk, (int)(base + j), 64);
        const bool front = (tj < inf) & ((tj < tk) | ((tj == tk) & (j < k)));
        less |= front ? (1u << j) : 0u;
        pred = front ? lrcdev::max2(pred, tj) : pred;
    }
    // a cluster starts at the first hit and wherever the gap to the one in front exceeds the separation
    const bool start = hit & ((less == 0u) | ((tk - pred) > q.separation));
    const uint32_t smask = (uint32_t)(__ballot(start) >> base) & gbits;
    const uint32_t cid = hit ? (uint32_t)__popc(smask & (less | (1u << k))) : 0u;      // 1, 2, ... in ascending order; 0: no hit
    uint32_t same = 0u;                                                                 // the members of this lane's cluster
    for (uint32_t j = 0; j < G; ++j) {
        const uint32_t cj = (uint32_t)__shfl((int)cid, (int)(base + j), 64);
        same |= ((cj == cid) & (cj != 0u)) ? (1u << j) : 0u;
    }
    const uint32_t count = (uint32_t)__popc(same);
    // the representative (smallest k) of a cluster that is large enough speaks for it; clusters lie in the order one behind
    // the other, so the echo's number is the number of such representatives in front of this one
    const bool valid = hit & (same != 0u) & ((same & ((1u << k) - 1u)) == 0u) & (count >= (uint32_t)q.min_count);
    const uint32_t vmask = (uint32_t)(__ballot(valid) >> base) & gbits;
    const uint32_t eidx = (uint32_t)__popc(vmask & less);
    uint32_t src = 0xFFFFFFFFu;                           // lane e < E: the lane of echo e's representative
    for (uint32_t e = 0; e < (uint32_t)q.max_echoes; ++e) {
        const uint32_t m = (uint32_t)(__ballot(valid & (eidx == e)) >> base) & gbits;
        if (k == e && m != 0u) src = base + (uint32_t)__builtin_ctz(m);
    }
    const int from = (int)(src != 0xFFFFFFFFu ? src : tid);
    float t_e = __shfl(tk, from, 64);
    uint32_t slot_e = (uint32_t)__shfl((int)best_slot, from, 64);
    const uint32_t label_e = (uint32_t)__shfl((int)best_label, from, 64);
    uint32_t n_e = (uint32_t)__shfl((int)count, from, 64);
    if (k >= (uint32_t)q.max_echoes) return;              // the other lanes write nothing
    if (src == 0xFFFFFFFFu) { t_e = inf; slot_e = 0xFFFFFFFFu; n_e = 0u; }
    const uint64_t beam = lane >> glog;
    const uint64_t rec = beam * (uint32_t)q.max_echoes + k;
    record(beam, rec, t_e, slot_e, label_e);
    if (q.weight) q.weight[rec] = (uint8_t)n_e;
}
#endif

}  // namespace lrcecho
