// lrc_voxseq.h -- layout of an occupancy sequence (lrc_voxseq.hip; include/lidarcast.h "dynamic occupancy").
//
// F frame slots of one grid geometry share one bitset and one key space.  A slot takes W = ceil(V / 32) words, so its
// free bits start on a word boundary; the GLOBAL index of voxel idx of slot f is gidx = f * 32 * W + idx, which is also its
// bit in the bitset.  Create refuses F * 32 * W > 2^31 - 1, so gidx fits 31 bits and the two keys of a return are
//   label key  (gidx << 32) | (sem << 16) | ins       the sem / ins vote, as lrc_voxgrid's key with gidx for idx
//   mover key  (gidx <<  8) | mover                   the second, independent vote
// Both sort ascending by (slot, idx) first.  Unused reserved key slots hold all ones in both columns and sort last.
#ifndef LRC_VOXSEQ_H
#define LRC_VOXSEQ_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lrcseq {

constexpr uint64_t kMaxBits = 0x7FFFFFFFull;        // F * 32 * W

// accumulator words (uint64): keys appended, key slots overflowed (never expected), rays of poses without a slot
enum { kAccKeys = 0, kAccOverflow = 1, kAccSkipped = 2, kAccWords = 4 };

__host__ __device__ inline unsigned long long label_key(uint32_t gidx, uint32_t sem, uint32_t ins) {
    return ((unsigned long long)gidx << 32) | ((unsigned long long)(sem & 0xFFFFu) << 16) | (unsigned long long)(ins & 0xFFFFu);
}
__host__ __device__ inline unsigned long long mover_key(uint32_t gidx, uint32_t mover) {
    return ((unsigned long long)gidx << 8) | (unsigned long long)(mover & 0xFFu);
}

}  // namespace lrcseq

#endif  // LRC_VOXSEQ_H
