// lrc_voxseq.hip -- dynamic occupancy: per-frame grids under movers, carved from explicit segments (gfx950).
//
// Definition: include/lidarcast.h "dynamic occupancy", DESIGN.md section 5u, tests/voxseq_restate.py.  The grid, the walk and
// its limits are lrc_voxwalk.h's, the keys, their runs and the sem / ins vote lrc_voxruns.h's, as for the static grid
// (lrc_voxgrid.hip); new are the frame slots (lrc_voxseq.h), the explicit segments (origin, end point and labels come from the
// scan's records instead of regenerated rays), STATIC_ONLY and the mover vote.
//
// Kernels
//   seq_walk   one thread per ray: walk_segment into a FreeSink on the ray's slot only -- a slot sees only its own frame's
//              rays, so the words around the sensor's voxel are contended by one frame's waves at once and set after the
//              first of them.  Returns: the label key and the mover key of a returned ray go to the same position of two key
//              columns, one atomic per wave for the slots.
//   finalize   the runs of each key column (KeyRuns) -- both columns hold the same (slot, voxel) set, so both give the same
//              places in the sparse list.  One thread per head votes: sem then ins on the label runs, the mover id on the
//              mover runs.  Frame offsets from the heads, per-slot counts by one block per slot (no atomics).  Integer work
//              only after the walk.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "lrc_internal.h"
#include "lrc_voxwalk.h"
#include "lrc_voxruns.h"
#include "lrc_voxseq.h"

namespace {

using namespace lrcwalk;
using namespace lrcseq;

struct WalkArgs {
    const float* origins3;
    const float* t;
    const float* point3;
    const uint16_t* sem;
    const uint16_t* ins;
    const uint8_t* mover;                 // nullable: all zero
    const uint32_t* frame_of_pose;        // nullable: first_frame + p
    uint64_t first_frame, N, total, key_cap;
    uint32_t per_ray, flags, F, W;
    Grid g;
    uint32_t* bits;                       // F * W words
    unsigned long long* lkeys;
    unsigned long long* mkeys;
    unsigned long long* acc;              // kAccWords
    unsigned long long* rejected;         // F
};

struct HostSink {
    uint32_t* bits;
    void add(uint32_t idx) { bits[idx >> 5] |= 1u << (idx & 31u); }
    void flush() {}
};

__global__ __launch_bounds__(kBlock) void seq_walk_kernel(WalkArgs a) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool ret = false, rejected = false, skipped = false;
    uint32_t f = 0, gidx = 0, label = 0, mv = 0;
    if (gid < a.total) {
        const float t = a.t[gid];
        if (finite_f(t)) {
            const uint64_t p = gid / a.N;
            const uint64_t fs = a.frame_of_pose ? (uint64_t)a.frame_of_pose[p] : a.first_frame + p;
            if (fs >= a.F) {
                skipped = true;                               // no access is made with this slot
            } else {
                f = (uint32_t)fs;
                const float* __restrict__ o = a.origins3 + 3 * (a.per_ray ? gid : p);
                const float* __restrict__ e = a.point3 + 3 * gid;
                mv = a.mover ? (uint32_t)a.mover[gid] : 0u;
                FreeSink sink{a.bits + (uint64_t)f * a.W};
                uint32_t end = 0;
                int32_t b3[3];
                const int rc = walk_segment(a.g, o[0], o[1], o[2], e[0], e[1], e[2], sink, end, b3);
                    rejected = rc == kWalkRejected;
                if (rc == kWalkEnd && !((a.flags & LRC_VOXSEQ_STATIC_ONLY) && mv != 0u)) {
                    ret = true;
                    gidx = f * 32u * a.W + end;
                    label = (uint32_t)a.sem[gid] | ((uint32_t)a.ins[gid] << 16);
                }
            }
        }
    }
    const uint32_t lane = __lane_id();
    const unsigned long long sm = __ballot(skipped);
    if (sm && lane == (uint32_t)__ffsll((long long)sm) - 1) atomicAdd(&a.acc[kAccSkipped], (unsigned long long)__popcll(sm));
    const unsigned long long rm = __ballot(rejected);
    if (rm) {                                                  // wave-uniform; a wave's rays mostly share one slot
        const uint32_t leader = (uint32_t)__ffsll((long long)rm) - 1;
        const uint32_t fl = (uint32_t)__shfl((int)f, (int)leader);
        const unsigned long long same = __ballot(rejected && f == fl);
        if (lane == leader) atomicAdd(&a.rejected[fl], (unsigned long long)__popcll(same));
        else if (rejected && f != fl) atomicAdd(&a.rejected[f], 1ull);
    }
    const unsigned long long pos = wave_append(ret, &a.acc[kAccKeys], &a.acc[kAccOverflow], a.key_cap);
    if (pos != kNoSlot) {
        a.lkeys[pos] = label_key(gidx, label & 0xFFFFu, label >> 16);
        a.mkeys[pos] = mover_key(gidx, mv);
    }
}

// ---- finalize ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void seq_dense_kernel(const uint32_t* __restrict__ bits, uint32_t V, uint32_t W,
                                                           uint64_t FV, uint8_t* __restrict__ state) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= FV) return;
    const uint64_t f = i / V;
    const uint32_t v = (uint32_t)(i - f * V);
    state[i] = (uint8_t)((bits[f * W + (v >> 5)] >> (v & 31u)) & 1u);
}

// one thread per head of the label runs: count its returns and vote sem, then ins within the winning sem; the first head of a
// slot (and of the empty slots before it) writes the slot's offset
__global__ __launch_bounds__(kBlock) void seq_label_vote_kernel(
    const unsigned long long* __restrict__ ukeys, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ nruns,
    const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint64_t R, uint32_t min_returns, uint32_t V,
    uint32_t W, uint32_t* __restrict__ o_idx, uint16_t* __restrict__ o_sem, uint16_t* __restrict__ o_ins,
    uint32_t* __restrict__ o_ret, uint64_t* __restrict__ offsets, uint8_t* __restrict__ state) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= R || !flag[j]) return;
    const LabelVote v = label_vote(ukeys, counts, *nruns, j);
    const uint32_t gidx = (uint32_t)(ukeys[j] >> 32), bps = 32u * W;
    const uint32_t f = gidx / bps, idx = gidx - f * bps, o = pos[j];
    o_idx[o] = idx;
    o_sem[o] = (uint16_t)v.sem;
    o_ins[o] = (uint16_t)v.ins;
    o_ret[o] = v.total;
    if (state && v.total >= min_returns) state[(uint64_t)f * V + idx] = 2;
    const uint32_t first = j == 0 ? 0u : (uint32_t)(ukeys[j - 1] >> 32) / bps + 1u;       // j - 1: the voxel before
    for (uint32_t s = first; s <= f; ++s) offsets[s] = o;
}

// offsets of the slots after the last one with a return (F included): the length of the sparse list
__global__ __launch_bounds__(kBlock) void seq_tail_kernel(const unsigned long long* __restrict__ ukeys,
                                                          const uint32_t* __restrict__ nruns, const uint32_t* __restrict__ pos,
                                                          uint64_t R, uint64_t G, uint32_t W, uint32_t F,
                                                          uint64_t* __restrict__ offsets) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s > F) return;
    int64_t last = (int64_t)*nruns - 1;
    if (last >= 0 && (ukeys[last] >> 32) >= G) --last;           // the all-ones run of the unused slots
    const int64_t fl = last >= 0 ? (int64_t)((uint32_t)(ukeys[last] >> 32) / (32u * W)) : -1;
    if ((int64_t)s > fl) offsets[s] = pos[R];
}

// one thread per head of the mover runs: the most frequent mover id (ascending ids: ties keep the smallest) and the returns
// with id != 0
__global__ __launch_bounds__(kBlock) void seq_mover_vote_kernel(const unsigned long long* __restrict__ ukeys,
                                                                const uint32_t* __restrict__ counts,
                                                                const uint32_t* __restrict__ nruns,
                                                                const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                                uint64_t R, uint8_t* __restrict__ o_mover,
                                                                uint32_t* __restrict__ o_mret) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= R || !flag[j]) return;
    const uint64_t nr = *nruns;
    const unsigned long long g = ukeys[j] >> 8;
    uint32_t total = 0, zero = 0, best_cnt = 0, best = 0;
    for (uint64_t k = j; k < nr && (ukeys[k] >> 8) == g; ++k) {
        const uint32_t c = counts[k], id = (uint32_t)(ukeys[k] & 0xFFull);
        total += c;
        if (id == 0) zero = c;
        if (c > best_cnt) { best_cnt = c; best = id; }
    }
    const uint32_t o = pos[j];
    o_mover[o] = (uint8_t)best;
    o_mret[o] = total - zero;
}

// counts of one slot, one block per slot: [0] sparse entries, [1] free, [2] occupied, [3] unknown, [4] rejected rays,
// [5] returns recorded -- from the slot's part of the sparse list and its words of the bitset
__global__ __launch_bounds__(kBlock) void seq_counts_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ o_idx,
                                                            const uint32_t* __restrict__ o_ret, const uint32_t* __restrict__ bits,
                                                            const unsigned long long* __restrict__ rejected, uint32_t min_returns,
                                                            uint32_t V, uint32_t W, uint64_t* __restrict__ out) {
    __shared__ unsigned long long s_part[kBlock / 64][4];
    const uint32_t f = blockIdx.x;
    const uint32_t* __restrict__ wb = bits + (uint64_t)f * W;
    const uint64_t lo = offsets[f], hi = offsets[f + 1];
    unsigned long long occ = 0, overlap = 0, rets = 0, pop = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
        const uint32_t r = o_ret[i];
        rets += r;
        if (r >= min_returns) {
            const uint32_t idx = o_idx[i];
            ++occ;
            overlap += (wb[idx >> 5] >> (idx & 31u)) & 1u;
        }
    }
    for (uint32_t w = threadIdx.x; w < W; w += kBlock) pop += (unsigned long long)__popc(wb[w]);    // bits >= V are never set
    for (int o = 32; o > 0; o >>= 1) {
        occ += __shfl_down(occ, o);
        overlap += __shfl_down(overlap, o);
        rets += __shfl_down(rets, o);
        pop += __shfl_down(pop, o);
    }
    if (__lane_id() == 0) {
        s_part[threadIdx.x / 64][0] = occ;
        s_part[threadIdx.x / 64][1] = overlap;
        s_part[threadIdx.x / 64][2] = rets;
        s_part[threadIdx.x / 64][3] = pop;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[4] = {0, 0, 0, 0};
        for (int i = 0; i < kBlock / 64; ++i)
            for (int c = 0; c < 4; ++c) t[c] += s_part[i][c];
        const uint64_t fr = t[3] - t[1];
        uint64_t* o6 = out + (uint64_t)f * 6;
        o6[0] = hi - lo;
        o6[1] = fr;
        o6[2] = t[0];
        o6[3] = (uint64_t)V - fr - t[0];
        o6[4] = rejected[f];
        o6[5] = t[2];
    }
}

}  // namespace

struct lrc_voxseq {
    int device = 0;
    Grid g{};
    uint64_t V = 0, W = 0, F = 0;
    uint32_t* d_bits = nullptr;                 // F * W words
    unsigned long long* d_lkeys = nullptr;      // key_cap slots each; [0, reserved) valid or all-ones
    unsigned long long* d_mkeys = nullptr;
    uint64_t key_cap = 0, reserved = 0;
    unsigned long long* d_acc = nullptr;        // kAccWords + F rejected counters
    KeyRuns runs;                               // finalize scratch; runs.G = F * 32 * W global indices
};

namespace {

void release(lrc_voxseq* v) {
    v->runs.release();
    void* ps[] = {v->d_bits, v->d_lkeys, v->d_mkeys, v->d_acc};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    v->d_bits = nullptr;
    v->d_lkeys = v->d_mkeys = nullptr;
    v->d_acc = nullptr;
}

uint64_t sparse_bound(const lrc_voxseq* v) {
    const uint64_t FV = v->F * v->V;
    return v->reserved < FV ? v->reserved : FV;
}

}  // namespace

extern "C" {

int lrc_voxseq_destroy(lrc_voxseq* seq) {
    if (!seq) return LRC_OK;
    (void)hipSetDevice(seq->device);
    release(seq);
    delete seq;
    return LRC_OK;
}

int lrc_voxseq_create(lrc_ctx* ctx, const double* origin3, double voxel_size, const int64_t* dims3, uint64_t num_frames,
                      lrc_voxseq** out_seq) {
    if (!out_seq) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_create: out_seq is NULL");
    *out_seq = nullptr;
    if (!ctx || !origin3 || !dims3) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_create: NULL argument");
    for (int a = 0; a < 3; ++a)
        if (!__builtin_isfinite(origin3[a]))
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_create: origin must be finite");
    if (!__builtin_isfinite(voxel_size) || !(voxel_size > 0.0))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_create: voxel_size must be finite and > 0");
    uint64_t V = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims3[a] < 1 || dims3[a] > 0x7FFFFFFFll)
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_create: every dim must be >= 1");
        V *= (uint64_t)dims3[a];
        if (V > 0x7FFFFFFFull)
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_create: nx*ny*nz must not exceed 2^31 - 1");
    }
    if (num_frames < 1) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_create: num_frames must be >= 1");
    const uint64_t W = (V + 31) / 32;
    if (num_frames > kMaxBits / (32 * W))                // F * 32 * W <= 2^31 - 1, without overflow
        return lrc_internal_fail(LRC_ERR_INVALID_ARG,
                                 "lrc_voxseq_create: num_frames * 32 * ceil(nx*ny*nz / 32) must not exceed 2^31 - 1");
    lrc_voxseq* v = new (std::nothrow) lrc_voxseq();
    if (!v) return lrc_internal_fail(LRC_ERR_OOM, "lrc_voxseq_create: out of host memory");
    v->device = ctx->device;
    v->g.gx = origin3[0];
    v->g.gy = origin3[1];
    v->g.gz = origin3[2];
    v->g.s = voxel_size;
    v->g.nx = (int32_t)dims3[0];
    v->g.ny = (int32_t)dims3[1];
    v->g.nz = (int32_t)dims3[2];
    v->g.V = (uint32_t)V;
    v->V = V;
    v->W = W;
    v->F = num_frames;
    v->runs.G = num_frames * 32 * W;                    // global indices
    auto run = [&]() -> int {
        LRC_HIP(hipSetDevice(v->device));
        LRC_HIP(hipMalloc((void**)&v->d_bits, v->F * v->W * 4));
        LRC_HIP(hipMalloc((void**)&v->d_acc, (kAccWords + v->F) * 8));
        LRC_HIP(hipMemset(v->d_bits, 0, v->F * v->W * 4));
        LRC_HIP(hipMemset(v->d_acc, 0, (kAccWords + v->F) * 8));
        return LRC_OK;
    };
    const int rc = run();
    if (rc != LRC_OK) {
        lrc_voxseq_destroy(v);
        return rc;
    }
    *out_seq = v;
    return LRC_OK;
}

int lrc_voxseq_get_info(const lrc_voxseq* seq, lrc_voxseq_info* out) {
    if (!seq || !out) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_get_info: NULL argument");
    out->origin[0] = seq->g.gx;
    out->origin[1] = seq->g.gy;
    out->origin[2] = seq->g.gz;
    out->voxel_size = seq->g.s;
    out->dims[0] = seq->g.nx;
    out->dims[1] = seq->g.ny;
    out->dims[2] = seq->g.nz;
    out->num_voxels = seq->V;
    out->words_per_frame = seq->W;
    out->num_frames = seq->F;
    out->reserved_keys = seq->reserved;
    out->sparse_bound = sparse_bound(seq);
    return LRC_OK;
}

int lrc_voxseq_reset(lrc_voxseq* seq, void* stream) {
    if (!seq) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_reset: NULL argument");
    const hipStream_t st = (hipStream_t)stream;
    LRC_HIP(hipSetDevice(seq->device));
    LRC_HIP(hipMemsetAsync(seq->d_bits, 0, seq->F * seq->W * 4, st));
    LRC_HIP(hipMemsetAsync(seq->d_acc, 0, (kAccWords + seq->F) * 8, st));
    seq->reserved = 0;
    return LRC_OK;
}

int lrc_voxseq_accumulate_dev(lrc_voxseq* seq, const float* d_origins3, int origin_per_ray, uint64_t num_poses,
                              uint64_t rays_per_pose, const uint32_t* d_frame_of_pose, uint64_t first_frame,
                              const lrc_hits* d_records, const uint8_t* d_mover, uint32_t flags, void* stream) {
    if (!seq) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_accumulate_dev: NULL argument");
    if (flags & ~(uint32_t)LRC_VOXSEQ_STATIC_ONLY)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_accumulate_dev: unknown flag");
    if (origin_per_ray != 0 && origin_per_ray != 1)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_accumulate_dev: origin_per_ray must be 0 or 1");
    if (!d_frame_of_pose && (first_frame > seq->F || num_poses > seq->F - first_frame))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_accumulate_dev: first_frame + num_poses exceeds num_frames");
    if (num_poses == 0 || rays_per_pose == 0) return LRC_OK;
    if (!d_origins3 || !d_records)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_accumulate_dev: NULL argument");
    if (!d_records->t || !d_records->point3 || !d_records->sem || !d_records->ins)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_accumulate_dev: the records need t, point3, sem and ins");
    if (num_poses > kMaxKeys || rays_per_pose > kMaxKeys || num_poses * rays_per_pose > kMaxKeys - seq->reserved)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_accumulate_dev: more than 2^31 - 1 rays between resets");
    const uint64_t total = num_poses * rays_per_pose;
    const hipStream_t st = (hipStream_t)stream;
    LRC_HIP(hipSetDevice(seq->device));
    const uint64_t need = seq->reserved + total;
    // both columns grow together: no return is ever dropped
    const int rc = grow_key_columns(&seq->d_lkeys, &seq->d_mkeys, &seq->key_cap, seq->reserved, need, st);
    if (rc != LRC_OK) return rc;
    LRC_HIP(hipMemsetAsync(seq->d_lkeys + seq->reserved, 0xFF, total * 8, st));   // unfilled slots sort last
    LRC_HIP(hipMemsetAsync(seq->d_mkeys + seq->reserved, 0xFF, total * 8, st));
    seq->reserved = need;
    WalkArgs a{};
    a.origins3 = d_origins3;
    a.t = d_records->t;
    a.point3 = d_records->point3;
    a.sem = d_records->sem;
    a.ins = d_records->ins;
    a.mover = d_mover;
    a.frame_of_pose = d_frame_of_pose;
    a.first_frame = first_frame;
    a.N = rays_per_pose;
    a.total = total;
    a.key_cap = seq->reserved;
    a.per_ray = (uint32_t)origin_per_ray;
    a.flags = flags;
    a.F = (uint32_t)seq->F;
    a.W = (uint32_t)seq->W;
    a.g = seq->g;
    a.bits = seq->d_bits;
    a.lkeys = seq->d_lkeys;
    a.mkeys = seq->d_mkeys;
    a.acc = seq->d_acc;
    a.rejected = seq->d_acc + kAccWords;
    hipLaunchKernelGGL(seq_walk_kernel, dim3((uint32_t)blocks_of(total, kBlock)), dim3(kBlock), 0, st, a);
    LRC_HIP(hipGetLastError());
    return LRC_OK;
}

int lrc_voxseq_finalize_dev(lrc_voxseq* seq, uint32_t min_returns, const lrc_voxseq_out* d_out, uint64_t capacity,
                            void* stream) {
    if (!seq || !d_out || !d_out->frame_offsets || !d_out->counts || !d_out->skipped)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_finalize_dev: NULL argument");
    if (min_returns < 1) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_finalize_dev: min_returns must be >= 1");
    const uint64_t R = seq->reserved, bound = sparse_bound(seq);
    if (bound && (!d_out->idx || !d_out->sem || !d_out->ins || !d_out->returns || !d_out->mover || !d_out->mover_returns))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_finalize_dev: NULL sparse output");
    if (capacity < bound)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_finalize_dev: capacity below sparse_bound");
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t V = seq->g.V, W = (uint32_t)seq->W, F = (uint32_t)seq->F;
    LRC_HIP(hipSetDevice(seq->device));
    if (d_out->state)
        hipLaunchKernelGGL(seq_dense_kernel, dim3((uint32_t)blocks_of(seq->F * seq->V, kBlock)), dim3(kBlock), 0, st,
                           (const uint32_t*)seq->d_bits, V, W, seq->F * seq->V, d_out->state);
    if (R) {
        KeyRuns& r = seq->runs;
        const KeyColumn lcol{seq->d_lkeys, 32}, mcol{seq->d_mkeys, 8};
        int rc = r.ensure(R, {lcol, mcol}, st);
        if (rc == LRC_OK) rc = r.runs_of(lcol, R, st);
        if (rc != LRC_OK) return rc;
        hipLaunchKernelGGL(seq_label_vote_kernel, dim3((uint32_t)blocks_of(R, kBlock)), dim3(kBlock), 0, st,
                           (const unsigned long long*)r.d_ukeys, (const uint32_t*)r.d_counts,
                           (const uint32_t*)r.d_nruns, (const uint32_t*)r.d_flag, (const uint32_t*)r.d_pos, R,
                           min_returns, V, W, d_out->idx, d_out->sem, d_out->ins, d_out->returns, d_out->frame_offsets,
                           d_out->state);
        hipLaunchKernelGGL(seq_tail_kernel, dim3((uint32_t)blocks_of(seq->F + 1, kBlock)), dim3(kBlock), 0, st,
                           (const unsigned long long*)r.d_ukeys, (const uint32_t*)r.d_nruns, (const uint32_t*)r.d_pos,
                           R, r.G, W, F, d_out->frame_offsets);
        LRC_HIP(hipGetLastError());
        rc = r.runs_of(mcol, R, st);
        if (rc != LRC_OK) return rc;
        hipLaunchKernelGGL(seq_mover_vote_kernel, dim3((uint32_t)blocks_of(R, kBlock)), dim3(kBlock), 0, st,
                           (const unsigned long long*)r.d_ukeys, (const uint32_t*)r.d_counts,
                           (const uint32_t*)r.d_nruns, (const uint32_t*)r.d_flag, (const uint32_t*)r.d_pos, R,
                           d_out->mover, d_out->mover_returns);
    } else {
        LRC_HIP(hipMemsetAsync(d_out->frame_offsets, 0, (seq->F + 1) * 8, st));
    }
    hipLaunchKernelGGL(seq_counts_kernel, dim3(F), dim3(kBlock), 0, st, (const uint64_t*)d_out->frame_offsets,
                       (const uint32_t*)d_out->idx, (const uint32_t*)d_out->returns, (const uint32_t*)seq->d_bits,
                       (const unsigned long long*)(seq->d_acc + kAccWords), min_returns, V, W, d_out->counts);
    LRC_HIP(hipGetLastError());
    LRC_HIP(hipMemcpyAsync(d_out->skipped, seq->d_acc + kAccSkipped, 8, hipMemcpyDeviceToDevice, st));
    return LRC_OK;
}

int lrc_voxseq_finalize(lrc_voxseq* seq, uint32_t min_returns, const lrc_voxseq_out* out, uint64_t capacity) {
    if (!seq || !out || !out->frame_offsets || !out->counts || !out->skipped)
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_finalize: NULL argument");
    const uint64_t bound = sparse_bound(seq);
    if (bound && (!out->idx || !out->sem || !out->ins || !out->returns || !out->mover || !out->mover_returns))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_finalize: NULL sparse output");
    if (capacity < bound) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_finalize: capacity below sparse_bound");
    LRC_HIP(hipSetDevice(seq->device));
    LRC_HIP(hipDeviceSynchronize());                      // work the caller enqueued on other streams
    const uint64_t n = bound ? bound : 1, F = seq->F, FV = seq->F * seq->V;
    struct Bufs {
        std::vector<void*> p;
        ~Bufs() {
            for (void* q : p) (void)hipFree(q);
        }
    } bufs;
    auto dev = [&](size_t bytes, void** q) -> int {
        LRC_HIP(hipMalloc(q, bytes ? bytes : 1));
        bufs.p.push_back(*q);
        return LRC_OK;
    };
    lrc_voxseq_out d{};
    int rc;
    if ((rc = dev(n * 4, (void**)&d.idx)) != LRC_OK || (rc = dev(n * 2, (void**)&d.sem)) != LRC_OK ||
        (rc = dev(n * 2, (void**)&d.ins)) != LRC_OK || (rc = dev(n * 4, (void**)&d.returns)) != LRC_OK ||
        (rc = dev(n, (void**)&d.mover)) != LRC_OK || (rc = dev(n * 4, (void**)&d.mover_returns)) != LRC_OK ||
        (rc = dev((F + 1) * 8, (void**)&d.frame_offsets)) != LRC_OK || (rc = dev(F * 48, (void**)&d.counts)) != LRC_OK ||
        (rc = dev(8, (void**)&d.skipped)) != LRC_OK)
        return rc;
    if (out->state && (rc = dev(FV, (void**)&d.state)) != LRC_OK) return rc;
    rc = lrc_voxseq_finalize_dev(seq, min_returns, &d, n, nullptr);
    if (rc != LRC_OK) return rc;
    LRC_HIP(hipMemcpy(out->frame_offsets, d.frame_offsets, (F + 1) * 8, hipMemcpyDeviceToHost));     // synchronises
    const uint64_t k = out->frame_offsets[F];
    if (k) {
        LRC_HIP(hipMemcpy(out->idx, d.idx, k * 4, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out->sem, d.sem, k * 2, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out->ins, d.ins, k * 2, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out->returns, d.returns, k * 4, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out->mover, d.mover, k, hipMemcpyDeviceToHost));
        LRC_HIP(hipMemcpy(out->mover_returns, d.mover_returns, k * 4, hipMemcpyDeviceToHost));
    }
    LRC_HIP(hipMemcpy(out->counts, d.counts, F * 48, hipMemcpyDeviceToHost));
    LRC_HIP(hipMemcpy(out->skipped, d.skipped, 8, hipMemcpyDeviceToHost));
    if (out->state) LRC_HIP(hipMemcpy(out->state, d.state, FV, hipMemcpyDeviceToHost));
    return LRC_OK;
}

int lrc_voxseq_export_bits(lrc_voxseq* seq, uint32_t* out_bits) {
    if (!seq || !out_bits) return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_export_bits: NULL argument");
    LRC_HIP(hipSetDevice(seq->device));
    LRC_HIP(hipDeviceSynchronize());
    LRC_HIP(hipMemcpy(out_bits, seq->d_bits, seq->F * seq->W * 4, hipMemcpyDeviceToHost));
    return LRC_OK;
}

// Host step, no GPU: the walk of n segments, compiled from the functions the kernel calls.
int lrc_voxseq_walk(const double* origin3, double voxel_size, const int64_t* dims3, const float* o3, const float* e3,
                    uint64_t n, uint32_t* io_free_bits, int64_t* out_end3, uint8_t* out_rejected) {
    if (!origin3 || !dims3 || !io_free_bits || (n && (!o3 || !e3 || !out_end3 || !out_rejected)))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_walk: NULL argument");
    if (!(__builtin_isfinite(origin3[0]) && __builtin_isfinite(origin3[1]) && __builtin_isfinite(origin3[2])))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_walk: origin must be finite");
    if (!__builtin_isfinite(voxel_size) || !(voxel_size > 0.0))
        return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_walk: voxel_size must be finite and > 0");
    uint64_t V = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims3[a] < 1 || dims3[a] > 0x7FFFFFFFll)
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_walk: every dim must be >= 1");
        V *= (uint64_t)dims3[a];
        if (V > 0x7FFFFFFFull)
            return lrc_internal_fail(LRC_ERR_INVALID_ARG, "lrc_voxseq_walk: nx*ny*nz must not exceed 2^31 - 1");
    }
    Grid g{origin3[0], origin3[1], origin3[2], voxel_size, (int32_t)dims3[0], (int32_t)dims3[1], (int32_t)dims3[2], (uint32_t)V};
    HostSink sink{io_free_bits};
    for (uint64_t r = 0; r < n; ++r) {
        int32_t b3[3] = {0, 0, 0};
        uint32_t end = 0;
        const float* o = o3 + 3 * r;
        const float* e = e3 + 3 * r;
        const int rc = walk_segment(g, o[0], o[1], o[2], e[0], e[1], e[2], sink, end, b3);
        out_rejected[r] = rc == kWalkRejected;
        for (int a = 0; a < 3; ++a) out_end3[3 * r + a] = b3[a];
    }
    return LRC_OK;
}

}  // extern "C"
