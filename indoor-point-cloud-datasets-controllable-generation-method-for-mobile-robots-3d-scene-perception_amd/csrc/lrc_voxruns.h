// lrc_voxruns.h -- key runs of the occupancy grids: how returns are appended as 64-bit keys and voted on, for the static grid
// (lrc_voxgrid.hip) and the frame slots (lrc_voxseq.hip, section 5u).
//
//   Keys      a returned ray appends one key per column, the voxel's index in the high bits: (index << shift) | payload.  The
//             columns hold key_cap slots; [0, reserved) are valid or all ones (unused slots, which sort last).  Growth doubles
//             the columns, up to kMaxKeys slots: no return is ever dropped.
//   Runs      rocprim radix sort of a column, run-length encoding of equal keys, a head flag on the first run of every
//             index < G and an exclusive scan of the flags: the head's place in the sparse list.
//   Vote      label keys (index << 32) | (sem << 16) | ins: returns[v] = the runs' counts summed; sem[v] = most frequent sem
//             among v's returns (ties to the smallest), ins[v] = most frequent ins among the returns with that sem (ties to
//             the smallest).
// Everything here lives in an anonymous namespace, as in lrc_knn64.h: each translation unit gets its own copy of the kernel
// and of the host code that launches it.
#ifndef LRC_VOXRUNS_H
#define LRC_VOXRUNS_H

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <initializer_list>

#include "lrc_internal.h"

namespace {

constexpr uint64_t kMaxKeys = 0x7FFFFFFFull;        // reserved key slots between resets
constexpr unsigned long long kNoSlot = ~0ull;

// ---- appending -----------------------------------------------------------------------------------------------------
// Slot of this lane's key(s), one atomic per wave on *appended; every lane of the wave calls it.  kNoSlot for a lane
// without a return, and past the reserved slots (never expected: *overflow is set).
__device__ inline unsigned long long wave_append(bool ret, unsigned long long* __restrict__ appended,
                                                 unsigned long long* __restrict__ overflow, uint64_t key_cap) {
    const unsigned long long m = __ballot(ret);
    if (!m) return kNoSlot;                                    // wave-uniform
    const uint32_t lane = __lane_id(), leader = (uint32_t)__ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(appended, (unsigned long long)__popcll(m));
    base = __shfl(base, (int)leader);
    if (!ret) return kNoSlot;
    const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < key_cap) return pos;
    atomicOr(overflow, 1ull);
    return kNoSlot;
}

// Room for `need` slots in the key column *col0 and, unless col1 is NULL, in *col1; the first `reserved` slots are kept.  On a
// failure the new buffers are freed and the columns stay as they were.  The old buffers are freed only on success, after the
// stream has drained (the copies, and enqueued work that may still read them); an error of that hipFree is not reported:
// the columns already are the new buffers.
inline int grow_key_columns(unsigned long long** col0, unsigned long long** col1, uint64_t* key_cap, uint64_t reserved,
                            uint64_t need, hipStream_t st) {
    if (need <= *key_cap) return LRC_OK;
    uint64_t cap = *key_cap * 2;
    if (cap < need) cap = need;
    if (cap > kMaxKeys) cap = kMaxKeys;
    unsigned long long** const col[2] = {col0, col1};
    unsigned long long* nk[2] = {nullptr, nullptr};
    const int n = col1 ? 2 : 1;
    hipError_t e = hipSuccess;
    for (int c = 0; c < n && e == hipSuccess; ++c) e = hipMalloc((void**)&nk[c], cap * 8);
    for (int c = 0; c < n && e == hipSuccess && reserved; ++c)
        e = hipMemcpyAsync(nk[c], *col[c], reserved * 8, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        for (unsigned long long* p : nk)
            if (p) (void)hipFree(p);
        LRC_HIP(e);
    }
    for (int c = 0; c < n; ++c) {
        if (*col[c]) (void)hipFree(*col[c]);
        *col[c] = nk[c];
    }
    *key_cap = cap;
    return LRC_OK;
}

// ---- runs ----------------------------------------------------------------------------------------------------------
inline uint32_t index_bits(uint64_t G) {             // G < 2^b: every valid key's index field is below all ones
    uint32_t b = 0;
    while (b < 32 && (1ull << b) <= G) ++b;
    return b;
}

// head of an index' runs in the sorted sequence of unique keys; the index is key >> shift
__global__ __launch_bounds__(kBlock) void seq_head_kernel(const unsigned long long* __restrict__ ukeys,
                                                          const uint32_t* __restrict__ nruns, uint64_t R, uint32_t shift,
                                                          uint64_t G, uint32_t* __restrict__ flag) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j > R) return;
    uint32_t f = 0;
    if (j < *nruns) {
        const unsigned long long g = ukeys[j] >> shift;
        f = g < G && (j == 0 || (ukeys[j - 1] >> shift) != g);
    }
    flag[j] = f;
}

struct KeyColumn {
    const unsigned long long* keys;
    uint32_t shift;                                  // the index field starts at this bit
};

// The finalize scratch of one grid or sequence, sized for fin_cap keys; G (the number of valid indices) is set by the owner.
struct KeyRuns {
    uint64_t G = 0;
    uint64_t fin_cap = 0;
    unsigned long long* d_sorted = nullptr;
    unsigned long long* d_ukeys = nullptr;
    uint32_t* d_counts = nullptr;
    uint32_t* d_flag = nullptr;                      // fin_cap + 1
    uint32_t* d_pos = nullptr;                       // fin_cap + 1
    uint32_t* d_nruns = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;

    void release() {
        void* ps[] = {d_sorted, d_ukeys, d_counts, d_flag, d_pos, d_nruns, d_tmp};
        for (void* p : ps)
            if (p) (void)hipFree(p);
        d_sorted = d_ukeys = nullptr;
        d_counts = d_flag = d_pos = d_nruns = nullptr;
        d_tmp = nullptr;
        fin_cap = 0;
        tmp_bytes = 0;
    }

    // scratch for R keys of every column; the temporary storage is the largest any call of runs_of asks for
    int ensure(uint64_t R, std::initializer_list<KeyColumn> cols, hipStream_t st) {
        if (R <= fin_cap) return LRC_OK;
        LRC_HIP(hipStreamSynchronize(st));              // the old scratch may still be read by enqueued work
        release();
        const uint64_t cap = R;
        LRC_HIP(hipMalloc((void**)&d_sorted, cap * 8));
        LRC_HIP(hipMalloc((void**)&d_ukeys, cap * 8));
        LRC_HIP(hipMalloc((void**)&d_counts, cap * 4));
        LRC_HIP(hipMalloc((void**)&d_flag, (cap + 1) * 4));
        LRC_HIP(hipMalloc((void**)&d_pos, (cap + 1) * 4));
        LRC_HIP(hipMalloc((void**)&d_nruns, 4));
        size_t most = 0, b = 0;
        for (const KeyColumn& c : cols) {
            LRC_HIP(rocprim::radix_sort_keys(nullptr, b, c.keys, d_sorted, (size_t)cap, 0, c.shift + index_bits(G), st));
            if (b > most) most = b;
        }
        LRC_HIP(rocprim::run_length_encode(nullptr, b, (const unsigned long long*)d_sorted, (unsigned int)cap, d_ukeys,
                                         d_counts, d_nruns, st));
        if (b > most) most = b;
        LRC_HIP(rocprim::exclusive_scan(nullptr, b, (const uint32_t*)d_flag, d_pos, 0u, (size_t)(cap + 1),
                                      rocprim::plus<uint32_t>(), st));
        if (b > most) most = b;
        tmp_bytes = most;
        LRC_HIP(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 1));
        fin_cap = cap;
        return LRC_OK;
    }

    // sort one key column, encode its runs, flag the heads and scan them into d_pos
    int runs_of(KeyColumn c, uint64_t R, hipStream_t st) {
        size_t tb = tmp_bytes;
        LRC_HIP(rocprim::radix_sort_keys(d_tmp, tb, c.keys, d_sorted, (size_t)R, 0, c.shift + index_bits(G), st));
        tb = tmp_bytes;
        LRC_HIP(rocprim::run_length_encode(d_tmp, tb, (const unsigned long long*)d_sorted, (unsigned int)R, d_ukeys,
                                         d_counts, d_nruns, st));
        hipLaunchKernelGGL(seq_head_kernel, dim3((uint32_t)blocks_of(R + 1, kBlock)), dim3(kBlock), 0, st,
                           (const unsigned long long*)d_ukeys, (const uint32_t*)d_nruns, R, c.shift, G, d_flag);
        LRC_HIP(hipGetLastError());
        tb = tmp_bytes;
        LRC_HIP(rocprim::exclusive_scan(d_tmp, tb, (const uint32_t*)d_flag, d_pos, 0u, (size_t)(R + 1),
                                      rocprim::plus<uint32_t>(), st));
        return LRC_OK;
    }
};

// ---- vote ----------------------------------------------------------------------------------------------------------
struct LabelVote {
    uint32_t total, sem, ins;
};

// the vote of the head j of a label column over its runs [j, ...) among nr: the returns, the sem, then the ins within it
__device__ inline LabelVote label_vote(const unsigned long long* __restrict__ ukeys, const uint32_t* __restrict__ counts,
                                       uint64_t nr, uint64_t j) {
    const uint32_t idx = (uint32_t)(ukeys[j] >> 32);
    uint32_t total = 0, best_cnt = 0, best_sem = 0, best_ins = 0;
    uint64_t k = j;
    while (k < nr && (uint32_t)(ukeys[k] >> 32) == idx) {
        const unsigned long long top = ukeys[k] >> 16;           // (idx, sem)
        uint32_t sem_cnt = 0, ins_cnt = 0, ins = 0;
        while (k < nr && (ukeys[k] >> 16) == top) {
            const uint32_t c = counts[k];
            sem_cnt += c;
            if (c > ins_cnt) { ins_cnt = c; ins = (uint32_t)(ukeys[k] & 0xFFFFull); }   // ascending ins: ties keep the smallest
            ++k;
        }
        total += sem_cnt;
        if (sem_cnt > best_cnt) { best_cnt = sem_cnt; best_sem = (uint32_t)(top & 0xFFFFull); best_ins = ins; }
    }
    return LabelVote{total, best_sem, best_ins};
}

}  // namespace

#endif  // LRC_VOXRUNS_H
