// svoxt_raylists.h -- the storage of the per-ray operators with a sigma-only gradient (the kernels of svoxt_raysweep.h):
// the recorded sample lists a forward leaves for its backward, and the tile's LDS hash table that turns the backward's
// per-sample values into one global atomic per distinct feature row.
//
//   lists   three planes of [tile][k][lane] words (feature row, delta_t, z) -- a wavefront's k-th records are one 256-byte
//           line per plane -- up to S a ray, and one {count | kDmOver, t to resume the march from} per ray.
//   table   kDmTable slots keyed by feature row (integer atomicCAS on the key, LDS float add on the value), flushed as one
//           global atomicAdd per distinct row after every kDmRounds samples a lane: one 4-byte float atomic per sample with
//           one lane per row is the slowest atomic shape of this target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_launch.h"
#include "svoxt_wave.h"

namespace svoxt {

constexpr int kDmGroup = 4;          // records a lane fetches together
constexpr int kDmTable = 1024;       // rows of the tile's hash table (8 KiB of LDS a wavefront)
constexpr int kDmRounds = 12;        // samples a lane between two flushes: 64 x 12 = 768 entries at most in 1024 slots
constexpr int kDmMaxSamples = 4096;
constexpr uint32_t kDmOver = 0x80000000u;
static_assert(kDmRounds % kDmGroup == 0 && 64 * kDmRounds < kDmTable, "a pass must fit the table with room to probe");
static_assert(kBlock == 64, "one wavefront per tile");

struct DmLists {
    uint2* __restrict__ aux;         // [Qpad] {records | kDmOver if the ray has more, t of the first unrecorded sample}
    uint32_t* __restrict__ row;      // [tiles][S][64]
    float* __restrict__ dt;
    float* __restrict__ z;
    int S;                           // 0: no lists
};

__device__ __forceinline__ int64_t dm_index(int64_t tile, int S, int k, int lane) {
    return ((tile * S + k) << 6) + lane;
}

// the table of one wavefront, keys[kDmTable], vals[kDmTable] in LDS: svoxt_wave.h's value table with the barriers of its phases
__device__ __forceinline__ void dm_table_clear(int32_t* keys, float* vals, int lane) {
    row_values_clear<kDmTable, 64>(keys, vals, lane);
    __syncthreads();
}
__device__ __forceinline__ void dm_table_put(int32_t* keys, float* vals, int32_t idx, float v) { row_values_add<kDmTable>(keys, vals, idx, v); }
// adds every row's sum to column `col` of grad [M, gstride] and leaves the table empty
__device__ __forceinline__ void dm_table_flush(int32_t* keys, float* vals, int lane, float* __restrict__ grad, int gstride, int col) {
    __syncthreads();
    row_values_flush<kDmTable, 64>(keys, vals, lane, grad, gstride, col);
    __syncthreads();
}

// the kernels' view of a workspace of `bytes` for Q rays: as many records a ray as fit (a multiple of kDmGroup), 0: none
static inline DmLists dm_lists(void* workspace, int64_t bytes, int64_t Q) {
    DmLists L = {};
    if (workspace == nullptr || bytes <= 0 || Q <= 0) return L;
    const int64_t qpad = rec_rays(Q);
    int64_t S = (bytes / qpad - 8) / 12 / kDmGroup * kDmGroup;
    if (S < kDmGroup) return L;
    if (S > kDmMaxSamples) S = kDmMaxSamples;
    char* p = reinterpret_cast<char*>(workspace);
    L.aux = reinterpret_cast<uint2*>(p);
    L.row = reinterpret_cast<uint32_t*>(p + qpad * 8);
    L.dt = reinterpret_cast<float*>(p + qpad * 8 + qpad * S * 4);
    L.z = reinterpret_cast<float*>(p + qpad * 8 + qpad * S * 8);
    L.S = (int)S;
    return L;
}

// the workspace that holds max_samples records a ray (rounded up to kDmGroup): 8 bytes + 12 a sample for every ray of the
// batch rounded up to 64; -1: negative argument
static inline int64_t dm_workspace_bytes(int64_t Q, int64_t max_samples) {
    if (Q < 0 || max_samples < 0) return -1;
    if (Q == 0 || max_samples == 0) return 0;
    int64_t S = (max_samples + kDmGroup - 1) / kDmGroup * kDmGroup;
    if (S > kDmMaxSamples) S = kDmMaxSamples;
    return rec_rays(Q) * (8 + 12 * S);
}

}  // namespace svoxt
