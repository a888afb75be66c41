// svoxt_sort.h -- one pass of the stable LSD radix sort of (uint32 key, uint32 value) pairs that svoxt_p2v.hip (voxelize)
// and svoxt_quant.hip (quantize_median_cut) share: per-workgroup digit histogram, exclusive scan of the counters
// (svoxt_order.hip's two kernels), a scatter that ranks equal digits within a wavefront with ballots.  Pairs with
// equal digits keep their order.
#pragma once

#include <hip/hip_runtime.h>

#include "svoxt_host.h"
#include "svoxt_wave.h"

namespace svoxt {

constexpr int kSortSteps = 16, kSortSpan = 64 * kSortSteps;     // keys per sort workgroup (one wavefront)

// per-workgroup digit histogram: counts[d * nblocks + block]
static __global__ void __launch_bounds__(64)
sort_hist_kernel(const uint32_t* __restrict__ keys, uint32_t P, int shift, uint32_t radix, uint32_t nblocks,
                 uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[256];
    for (uint32_t d = threadIdx.x; d < radix; d += 64) h[d] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortSpan;
    for (int s = 0; s < kSortSteps; ++s) {
        const uint32_t idx = base + s * 64 + threadIdx.x;
        if (idx < P) atomicAdd(&h[(keys[idx] >> shift) & (radix - 1)], 1u);
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < radix; d += 64) counts[(size_t)d * nblocks + blockIdx.x] = h[d];
}

// stable scatter: the workgroup's keys in order, 64 at a time; a lane's rank among the lanes with its digit comes
// from one ballot per digit bit, the running offset of each digit lives in LDS.  vals_in NULL = the identity.
static __global__ void __launch_bounds__(64)
sort_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t P, int shift, int bits,
                    uint32_t nblocks, const uint32_t* __restrict__ starts, uint32_t* __restrict__ keys_out,
                    uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t run[256];
    const uint32_t radix = 1u << bits, lane = threadIdx.x;
    for (uint32_t d = lane; d < radix; d += 64) run[d] = starts[(size_t)d * nblocks + blockIdx.x];
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortSpan;
    for (int s = 0; s < kSortSteps; ++s) {
        const uint32_t idx = base + s * 64 + lane;
        const bool valid = idx < P;
        const uint32_t key = valid ? keys_in[idx] : 0u;
        const uint32_t dig = (key >> shift) & (radix - 1);
        unsigned long long m = __ballot(valid);
        for (int b = 0; b < bits; ++b) {
            const bool bit = (dig >> b) & 1u;
            const unsigned long long on = __ballot(bit);
            m &= bit ? on : ~on;
        }
        const uint32_t rank = (uint32_t)lane_rank(m, lane);
        const uint32_t at = valid ? run[dig] : 0u;
        __syncthreads();                                     // every lane has read its digit's offset
        if (valid) {
            keys_out[at + rank] = key;
            vals_out[at + rank] = vals_in != nullptr ? vals_in[idx] : idx;
            if (rank == (uint32_t)__popcll(m) - 1u) run[dig] = at + rank + 1u;   // the digit's last lane moves it on
        }
        __syncthreads();
    }
}

inline uint32_t sort_blocks(uint64_t P) { return (uint32_t)((P + kSortSpan - 1) / kSortSpan); }

// One pass over `bits` (<= 8) bits of the keys from `shift` up.  counts / starts hold 256 * sort_blocks(P) words each,
// chunks exclusive_scan_chunks of that many.
static int sort_pass(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t P, int shift, int bits, uint32_t* counts,
                     uint32_t* starts, uint32_t* chunks, uint32_t* keys_out, uint32_t* vals_out, hipStream_t st, const char* fn) {
    const uint32_t radix = 1u << bits, nblocks = sort_blocks(P);
    int rc;
    hipLaunchKernelGGL(sort_hist_kernel, dim3(nblocks), dim3(64), 0, st, keys_in, P, shift, radix, nblocks, counts);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(counts, (size_t)radix * nblocks, chunks, starts, st, fn))) return rc;
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(nblocks), dim3(64), 0, st, keys_in, vals_in, P, shift, bits, nblocks, starts,
                       keys_out, vals_out);
    return check_launch(fn);
}

}  // namespace svoxt
