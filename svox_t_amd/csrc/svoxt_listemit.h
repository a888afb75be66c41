// svoxt_listemit.h -- what the producers of sample lists share: ray_samples (svoxt_samples.hip), select
// (svoxt_scan.hip), split and merge (svoxt_cut.hip) all run count -> scan -> one host read -> emit.  Here: the workspace
// of the count, the two kernels that widen the scan into the int64 offsets of the new lists, the empty answer, and the
// checks of an emit's arrays.  The count and emit kernels themselves stay with their units.  Not part of the public C ABI.
//
// Two shapes of count:
//   per ray     n = Q counters, counts[q] = the samples ray q will have: offsets'[q] = starts[q], offsets'[Q] = the total
//   per sample  n = T + 1 counters, counts[k] = what input sample k turns into, entry T = 0: pos = the scan,
//               offsets'[q] = pos[offsets[q] clamped to [0, T]]; the emit reads pos again
// A count that can pass 2^32 (ray_samples, split, merge) also adds up a 64-bit total, a wavefront at a time
// (wave_add_to_total, svoxt_wave.h); the scan's uint32 entries wrap there, and the caller refuses from 2^31 on.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_workspace.h"

namespace svoxt {

// workspace of a count: [total u64]? [counts u32[n]] [starts u32[n]] [chunk sums of n]; the total is the cleared prefix
struct ListSpace {
    unsigned long long* total;               // NULL without one
    uint32_t *counts, *starts, *chunks;
    size_t clear_bytes, bytes;
};
inline ListSpace list_carve(void* workspace, size_t n, bool with_total) {
    ListSpace sp;
    Carver w(workspace);
    sp.total = with_total ? w.take<unsigned long long>(1) : nullptr;
    sp.clear_bytes = w.bytes();
    sp.counts = w.take<uint32_t>(n);
    sp.starts = w.take<uint32_t>(n);
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks(n));
    sp.bytes = w.bytes();
    return sp;
}
// the answer of a *_workspace_bytes query over `extent` rays or samples and extent + extra counters
inline int64_t list_space_bytes(int64_t extent, size_t extra, bool with_total) {
    if (!in31(extent)) return -1;
    if (extent == 0) return 0;
    return (int64_t)list_carve(nullptr, (size_t)extent + extra, with_total).bytes;
}
// The workspace argument of a count or an emit: 8-byte aligned, not NULL, of the size `query` names; carved into *sp.
inline int list_space_check(const char* fn, const void* workspace, int64_t bytes, size_t n, bool with_total, const char* query,
                            ListSpace* sp) {
    if (misaligned(workspace, 8)) return fail(SVOXT_ERR_INVALID, "%s: workspace is not 8-byte aligned", fn);
    *sp = list_carve(const_cast<void*>(workspace), n, with_total);
    return workspace_check(fn, workspace, bytes, (int64_t)sp->bytes, query);
}

// per ray: offsets[q] = starts[q], offsets[Q] = the 64-bit sum, which TOTAL also writes to total[0]
template <bool TOTAL>
__global__ void __launch_bounds__(kLaunchBlock)
list_ray_offsets_kernel(const uint32_t* __restrict__ starts, const unsigned long long* __restrict__ sum, int64_t Q,
                        int64_t* __restrict__ offsets, int64_t* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (i < Q) offsets[i] = (int64_t)starts[i];
    else if (i == Q) {
        offsets[Q] = (int64_t)sum[0];
        if constexpr (TOTAL) total[0] = (int64_t)sum[0];
    }
}

// per sample: offsets_out[q] = pos[clamped offsets[q]]; total[0] = the 64-bit sum (SUM64: pos wraps at 2^32, the caller
// refuses from 2^31) or pos[T] (a count that cannot pass T)
template <bool SUM64>
__global__ void __launch_bounds__(kLaunchBlock)
list_pos_offsets_kernel(const uint32_t* __restrict__ pos, const unsigned long long* __restrict__ sum, const int64_t* __restrict__ offsets,
                        int64_t Q, int64_t T, int64_t* __restrict__ offsets_out, int64_t* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (i <= Q) offsets_out[i] = (int64_t)pos[min(max(offsets[i], (int64_t)0), T)];
    if (i == 0) total[0] = SUM64 ? (int64_t)sum[0] : (int64_t)pos[T];
}

// What follows a count kernel on `st`: its launch check, the scan of the n counters, and the offsets kernel.  Templates,
// so that a unit holds the instances it launches and no other: TOTAL with a `total` to write, SUM64 over a ListSpace
// carved with a total.
template <bool TOTAL>
int list_ray_offsets(const char* fn, const ListSpace& sp, int64_t Q, int64_t* offsets, int64_t* total, hipStream_t st) {
    int rc;
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.counts, (size_t)Q, sp.chunks, sp.starts, st, fn))) return rc;
    hipLaunchKernelGGL(list_ray_offsets_kernel<TOTAL>, dim3(launch_blocks(Q + 1)), dim3(kLaunchBlock), 0, st, sp.starts, sp.total, Q, offsets,
                       total);
    return check_launch(fn);
}
template <bool SUM64>
int list_pos_offsets(const char* fn, const ListSpace& sp, const int64_t* offsets, int64_t Q, int64_t T, int64_t* offsets_out, int64_t* total,
                     hipStream_t st) {
    int rc;
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.counts, (size_t)T + 1, sp.chunks, sp.starts, st, fn))) return rc;
    hipLaunchKernelGGL(list_pos_offsets_kernel<SUM64>, dim3(launch_blocks(Q + 1)), dim3(kLaunchBlock), 0, st, sp.starts, sp.total, offsets, Q, T,
                       offsets_out, total);
    return check_launch(fn);
}

// the answer of a count with nothing to do: Q empty segments, no sample; nothing else is read
inline int clear_counts(const char* fn, int64_t* offsets_out, int64_t Q, int64_t* total, hipStream_t st) {
    int rc;
    if ((rc = memset_async(offsets_out, (size_t)(Q + 1) * sizeof(int64_t), st, fn))) return rc;
    return memset_async(total, sizeof(int64_t), st, fn);
}
// what a count checks of the caller's offsets_out [Q + 1] and total [1]
inline int counts_out_check(const char* fn, const int64_t* offsets_out, const int64_t* total) {
    if (offsets_out == nullptr || total == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets_out / total is NULL", fn);
    if (misaligned(offsets_out, 8) || misaligned(total, 8)) return fail(SVOXT_ERR_INVALID, "%s: offsets_out / total is not 8-byte aligned", fn);
    return SVOXT_OK;
}

// the arrays of an emit that copies samples: the old lists, the new ones, and the index of every new sample's source
inline int emit_arrays_check(const char* fn, const int32_t* ray, const int32_t* row, const float* depth, const float* length,
                             const int32_t* ray_out, const int32_t* row_out, const float* depth_out, const float* length_out,
                             const int64_t* index) {
    if (ray == nullptr || row == nullptr || depth == nullptr || length == nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: ray / row / depth / length is NULL", fn);
    if (ray_out == nullptr || row_out == nullptr || depth_out == nullptr || length_out == nullptr || index == nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: an output is NULL", fn);
    if (misaligned(ray, 4) || misaligned(row, 4) || misaligned(depth, 4) || misaligned(length, 4) || misaligned(ray_out, 4) ||
        misaligned(row_out, 4) || misaligned(depth_out, 4) || misaligned(length_out, 4) || misaligned(index, 8))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (index: 8 bytes, the other arrays: 4)", fn);
    return SVOXT_OK;
}

}  // namespace svoxt
