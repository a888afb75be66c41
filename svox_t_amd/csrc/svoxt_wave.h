// svoxt_wave.h -- the wavefront and LDS plumbing under the kernels, each idiom once: cross-lane reductions (two
// families), the inclusive scan over the 64 lanes, the ballot rank, and the LDS hash table keyed by feature row
// (DESIGN.md 4.24).  Only __device__ __forceinline__ functions over the HIP runtime; no kernel and no barrier: the
// barriers stay at the call sites, where the kernels' phases are written down.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svoxt {

// ---- reductions, result in EVERY lane: the xor butterfly, 32 down to LO (LO = 1: the wavefront; LO = K, a power of
// two: over the lanes that agree in their low log2(K) bits -- lane = column layouts).  A float sum by this family adds
// (((v + v^32) + ^16) + ...): a site keeps the family it was written with.
template <int LO = 1, typename V, typename Op>
__device__ __forceinline__ V wave_all(V v, Op op) {
#pragma unroll
    for (int off = 32; off >= LO; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}
template <int LO = 1, typename V> __device__ __forceinline__ V wave_all_max(V v) { return wave_all<LO>(v, [](V a, V b) { return max(a, b); }); }
template <typename V> __device__ __forceinline__ V wave_all_min(V v) { return wave_all(v, [](V a, V b) { return min(a, b); }); }
template <typename V> __device__ __forceinline__ V wave_all_sum(V v) { return wave_all(v, [](V a, V b) { return a + b; }); }
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) { return wave_all(v, [](uint32_t a, uint32_t b) { return a ^ b; }); }
// The maximum of a per-lane count (a list's length) as a SCALAR.  The butterfly's result is wavefront-uniform by
// construction, but the compiler does not know that; readfirstlane says so, because everything that decides how many
// workgroup barriers a wavefront executes -- trip counts, early returns -- must be scalar control flow.
template <int LO = 1>
__device__ __forceinline__ int wave_uniform_max(int v) { return __builtin_amdgcn_readfirstlane(wave_all_max<LO>(v)); }
// the sum over groups of G neighbouring lanes (a power of two), in each of them, the offsets going UP (1, 2, ..): the
// other association of a float sum, for the sites written with it
template <int G, typename V>
__device__ __forceinline__ V wave_group_sum(V v) {
#pragma unroll
    for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The tail of a count kernel (svoxt_listemit.h), called by every lane of the wavefront: its lanes' counts summed, and
// one atomic from lane 0 onto the 64-bit total where the sum is not zero (integers: the same total in every run).
template <typename V>
__device__ __forceinline__ void wave_add_to_total(V n, unsigned long long* __restrict__ total) {
    const V sum = wave_all_sum(n);
    if ((threadIdx.x & 63) == 0 && sum != (V)0) atomicAdd(total, (unsigned long long)sum);
}

// ---- reductions, result in LANE 0 only (__shfl_down, 32 down to 1; the other lanes end with partial results)
template <typename V, typename Op>
__device__ __forceinline__ V wave_to0(V v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, 64));
    return v;
}
template <typename V> __device__ __forceinline__ V wave_sum(V v) { return wave_to0(v, [](V a, V b) { return a + b; }); }
template <typename V> __device__ __forceinline__ V wave_max(V v) { return wave_to0(v, [](V a, V b) { return max(a, b); }); }

// ---- Hillis-Steele inclusive scan over the 64 lanes; lane 63 ends with the total
template <typename V>
__device__ __forceinline__ V wave_inclusive_scan(V v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const V u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    return v;
}

// ---- a lane's rank among the lanes of a ballot: the set lanes below it
__device__ __forceinline__ int lane_rank(unsigned long long mask, int lane) { return (int)__popcll(mask & ((1ull << lane) - 1ull)); }

// ---- the row table: T (a power of two) LDS slots keyed by feature row, -1 = free.  Plain pointers, no struct of them
// (svoxt_tile_reduce.inc says what that cost).
// The slot of row idx, claimed if it had none: multiplicative hash, atomicCAS on the key, linear probe.  The table may
// run full as long as every key searched for is then present.
template <int T>
__device__ __forceinline__ uint32_t row_table_claim(int32_t* keys, int32_t idx) {
    static_assert(T > 1 && (T & (T - 1)) == 0, "a power of two");
    uint32_t h = ((uint32_t)idx * 0x9E3779B1u) >> (32 - __builtin_ctz(T));
    while (true) {
        const int32_t old = atomicCAS(keys + h, -1, idx);
        if (old == -1 || old == idx) return h;
        h = (h + 1u) & (uint32_t)(T - 1);
    }
}
// Exclusive scan, in place, of the table's T counters by one wavefront (T / 64 consecutive entries a lane): cnt[h]
// becomes where slot h's first record goes.  Returns the inclusive sum: in lane 63 the total.
template <int T>
__device__ __forceinline__ int row_table_counts_scan(int32_t* cnt, int lane) {
    constexpr int PER = T / 64;
    int mine[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { mine[j] = cnt[lane * PER + j]; sum += mine[j]; }
    const int incl = wave_inclusive_scan(sum, lane);
    int run = incl - sum;
#pragma unroll
    for (int j = 0; j < PER; ++j) { cnt[lane * PER + j] = run; run += mine[j]; }
    return incl;
}
// The table with one float per row, shared by the NT threads of a workgroup (tid = threadIdx.x): LDS float add on the
// slot's value; flush sends one global atomic per occupied slot to column col of grad [M, gstride] and leaves the table
// empty.  The caller puts a workgroup barrier between clear / add / flush.
template <int T, int NT>
__device__ __forceinline__ void row_values_clear(int32_t* keys, float* vals, int tid) {
    for (int i = tid; i < T; i += NT) { keys[i] = -1; vals[i] = 0.f; }
}
template <int T>
__device__ __forceinline__ void row_values_add(int32_t* keys, float* vals, int32_t idx, float v) { atomicAdd(vals + row_table_claim<T>(keys, idx), v); }
template <int T, int NT>
__device__ __forceinline__ void row_values_flush(int32_t* keys, float* vals, int tid, float* __restrict__ grad, int gstride, int col) {
    for (int i = tid; i < T; i += NT) {
        const int32_t key = keys[i];
        if (key >= 0) {
            atomicAdd(grad + (int64_t)key * gstride + col, vals[i]);
            keys[i] = -1;
            vals[i] = 0.f;
        }
    }
}

}  // namespace svoxt
