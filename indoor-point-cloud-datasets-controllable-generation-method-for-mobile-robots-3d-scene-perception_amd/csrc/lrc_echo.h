// lrc_echo.h -- beam footprint and multi-echo returns of lrc_scan_echoes_* (include/lidarcast.h "beam footprint and
// multi-echo returns"): what the trace kernel needs of an lrc_beam (GEN = 6), and the reduction of one
// beam's K closest-hit distances to at most E echoes, written once for the host.  The kernel does the same reduction across
// the lanes of a beam's group (lidarcast.hip, trace_kernel GEN = 6); lrc_echo_reduce calls the function below, and the
// tests compare the two through the explicit-ray path.
//
//   order     the sub-rays that hit, by (t_k, k) ascending: s_0 <= s_1 <= ...
//   clusters  a new cluster starts at m = 0 and wherever (s_m - s_(m-1)) > separation: one float32 subtraction, one float32
//             compare.  A surface seen at a grazing angle chains into one cluster however long the chain is.
//   cluster   weight n_c = members; representative = the member with the smallest k; range = the representative's t
//   echoes    clusters with n_c < min_count are discarded; the first E of the rest, in ascending order, are echoes 0..E-1
#pragma once
#include <stdint.h>

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

}  // namespace lrcecho
