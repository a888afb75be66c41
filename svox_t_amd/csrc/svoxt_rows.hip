// svoxt_rows.hip -- the row side of the per-sample interface (not in the reference): from samples to
// feature rows and back, without a float atomic anywhere.
//
//   row plan       the inverse of a sample list's `row` array: for every feature row the samples that name it, in
//                  ascending sample index.  key = row where 0 <= row < M, M for anything else -> stable LSD radix sort
//                  over the bits of M (svoxt_sort.h; the last pass writes perm) -> row_ptr[r] by a binary search per
//                  row (4.16's) -> per row n = row_ptr[r + 1] - row_ptr[r]: the longest segment (an integer atomicMax),
//                  flag = n > SVOXT_ROW_CHUNK and ceil(n / SVOXT_ROW_CHUNK) chunks, two exclusive scans -> the info
//                  record (n_outside, longest, long rows, their chunks) for the one host read.  svoxt_row_plan_long
//                  then lists the long rows (flag / scan / emit), each one's first chunk, and per chunk its long row.
//   gather_rows    out[k, j] = table[row[k], cols[j]]: a lane per (sample, column), or per (sample, four columns) with
//                  16-byte loads and stores where all K columns are taken, K is a multiple of 4 and both arrays are
//                  16-byte aligned.  A row outside [0, M) gives zeros, the table is not read.
//   reduce_rows    gather only.  rows_short_kernel: a lane per (row, column) walks the row's samples in ascending index
//                  (tv_rows_kernel's shape) for rows of at most SVOXT_ROW_CHUNK samples, and writes `empty` for rows
//                  without one.  Long rows: rows_chunk_kernel, a lane per (chunk, column), leaves the chunk's partial in
//                  the workspace; rows_join_kernel, a lane per (long row, column), joins them in chunk order.  The
//                  order is part of the definition (include/svoxt.h; tests compare bits).  The three kernels live in
//                  svoxt_rowwalk.h, over any source of per-sample values; here the source is the [T, C] table.
// C ABI: svoxt_row_plan_* / svoxt_gather_rows / svoxt_reduce_rows* (include/svoxt.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_rowwalk.h"
#include "svoxt_sort.h"
#include "svoxt_wave.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

// workspace of the plan: [longest u32] (cleared) [keys u32[T]] x 2 [vals u32[T]] x 2 [counts] [starts] [chunk sums]
// [flag u32[M + 1]] [rank] [nchunks] [cstart] [chunk sums]; svoxt_row_plan_long reads flag / rank / cstart
struct RowPlanSpace {
    uint32_t *longest, *keys[2], *vals[2], *counts, *starts, *chunks, *flag, *rank, *nchunks, *cstart, *mchunks;
    size_t clear_bytes, bytes;
};
static RowPlanSpace row_plan_carve(void* workspace, int64_t T, int64_t M) {
    RowPlanSpace sp;
    Carver w(workspace);
    const size_t cc = (size_t)256 * sort_blocks((uint64_t)T);
    sp.longest = w.take<uint32_t>(1);
    sp.clear_bytes = w.bytes();
    for (int i = 0; i < 2; ++i) sp.keys[i] = w.take<uint32_t>((size_t)T);
    for (int i = 0; i < 2; ++i) sp.vals[i] = w.take<uint32_t>((size_t)T);
    sp.counts = w.take<uint32_t>(cc);
    sp.starts = w.take<uint32_t>(cc);
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks(cc));
    sp.flag = w.take<uint32_t>((size_t)M + 1);
    sp.rank = w.take<uint32_t>((size_t)M + 1);
    sp.nchunks = w.take<uint32_t>((size_t)M + 1);
    sp.cstart = w.take<uint32_t>((size_t)M + 1);
    sp.mchunks = w.take<uint32_t>(exclusive_scan_chunks((size_t)M + 1));
    sp.bytes = w.bytes();
    return sp;
}

// (svoxt_rowwalk.h) INVARIANT the deterministic render backward (svoxt_rowgrad.hip) relies on: vals[0] is read and written by
// the sort passes of svoxt_row_plan_build alone -- the last pass writes perm, row_ptr_kernel reads keys -- and
// svoxt_row_plan_long reads flag / rank / cstart only.  From the build's last kernel on these T words are free, until the
// next build over the same workspace.  Whoever changes the sort's buffers or what svoxt_row_plan_long reads keeps this true
// or gives svoxt_rowgrad.hip a piece of its own.
uint32_t* row_plan_sort_scratch(void* workspace, int64_t T, int64_t M) { return row_plan_carve(workspace, T, M).vals[0]; }

// --------------------------------------------------------------------------------------------------------------- plan
__global__ void __launch_bounds__(kLaunchBlock)
row_key_kernel(const int32_t* __restrict__ row, int64_t T, int64_t M, uint32_t* __restrict__ keys) {
    const int64_t k = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (k >= T) return;
    const int64_t r = row[k];
    keys[k] = (uint32_t)(r >= 0 && r < M ? r : M);
}

// row_ptr[r] = the first sorted position whose key is >= r  (r in [0, M])
__global__ void __launch_bounds__(kLaunchBlock)
row_ptr_kernel(const uint32_t* __restrict__ keys, int64_t T, int64_t M, int32_t* __restrict__ row_ptr) {
    const int64_t r = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (r > M) return;
    int64_t lo = 0, hi = T;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < r) lo = mid + 1; else hi = mid;
    }
    row_ptr[r] = (int32_t)lo;
}

// per row (and the slot M behind them, which the scans need): long or not, its chunks, the longest segment
__global__ void __launch_bounds__(kLaunchBlock)
row_mark_kernel(const int32_t* __restrict__ row_ptr, int64_t M, uint32_t* __restrict__ flag, uint32_t* __restrict__ nchunks,
                uint32_t* __restrict__ longest) {
    const int64_t r = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    uint32_t n = 0;
    if (r < M) n = (uint32_t)(row_ptr[r + 1] - row_ptr[r]);
    if (r <= M) {
        const bool is_long = n > (uint32_t)kRowChunk;
        flag[r] = is_long ? 1u : 0u;
        nchunks[r] = is_long ? (n + (uint32_t)kRowChunk - 1u) / (uint32_t)kRowChunk : 0u;
    }
    const uint32_t m = wave_all_max(n);                          // (integers: the same in every run)
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(longest, m);
}

__global__ void __launch_bounds__(64)
row_info_kernel(const int32_t* __restrict__ row_ptr, int64_t T, int64_t M, const uint32_t* __restrict__ longest,
                const uint32_t* __restrict__ rank, const uint32_t* __restrict__ cstart, int64_t* __restrict__ info) {
    if (threadIdx.x != 0) return;
    info[0] = T - (int64_t)row_ptr[M];
    info[1] = (int64_t)longest[0];
    info[2] = (int64_t)rank[M];
    info[3] = (int64_t)cstart[M];
}

// long_chunk_ptr[rank[r]] = cstart[r] for the long rows r, long_chunk_ptr[n_long] = n_chunks
__global__ void __launch_bounds__(kLaunchBlock)
row_long_ptr_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ cstart, int64_t M,
                    int64_t n_long, int64_t n_chunks, int32_t* __restrict__ long_chunk_ptr) {
    const int64_t r = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (r < M && flag[r] != 0u && (int64_t)rank[r] < n_long) long_chunk_ptr[rank[r]] = (int32_t)cstart[r];
    if (r == M) long_chunk_ptr[n_long] = (int32_t)n_chunks;
}

// chunk_long[c] = the last long row whose first chunk is <= c
__global__ void __launch_bounds__(kLaunchBlock)
row_chunk_long_kernel(const int32_t* __restrict__ long_chunk_ptr, int64_t n_long, int64_t n_chunks, int32_t* __restrict__ chunk_long) {
    const int64_t c = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (c >= n_chunks) return;
    int64_t lo = 0, hi = n_long;                                 // first i with long_chunk_ptr[i] > c
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)long_chunk_ptr[mid] <= c) lo = mid + 1; else hi = mid;
    }
    chunk_long[c] = (int32_t)(lo > 0 ? lo - 1 : 0);
}

// ------------------------------------------------------------------------------------------------------------- gather
// lane t = k * Kc + j
__global__ void __launch_bounds__(kLaunchBlock)
gather_rows_kernel(const float* __restrict__ table, int64_t M, int K, const int32_t* __restrict__ row, int64_t T,
                   const int32_t* __restrict__ cols, int Kc, float* __restrict__ out) {
    const int64_t t = launch_lane();
    const int64_t k = t / Kc;
    if (k >= T) return;
    const int j = (int)(t - k * Kc);
    const int c = cols != nullptr ? cols[j] : j;
    const int64_t r = row[k];
    out[t] = (r >= 0 && r < M && c >= 0 && c < K) ? table[r * K + c] : 0.f;
}

// lane t = k * K4 + j: columns 4 j .. 4 j + 3 of sample k (all K = 4 K4 columns, both arrays 16-byte aligned)
__global__ void __launch_bounds__(kLaunchBlock)
gather_rows4_kernel(const float4* __restrict__ table, int64_t M, int K4, const int32_t* __restrict__ row, int64_t T,
                    float4* __restrict__ out) {
    const int64_t t = launch_lane();
    const int64_t k = t / K4;
    if (k >= T) return;
    const int j = (int)(t - k * K4);
    const int64_t r = row[k];
    out[t] = (r >= 0 && r < M) ? table[r * K4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------------------------- checks
static int rows_extents_check(int64_t T, int64_t M, const char* fn) {
    const int rc = extent31_check(fn, T, "T");
    return rc ? rc : extent31_check(fn, M, "M");
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_row_plan_workspace_bytes(int64_t T, int64_t M) {
    if (!in31(T) || !in31(M)) return -1;
    if (T == 0) return 0;
    return (int64_t)row_plan_carve(nullptr, T, M).bytes;
}

int svoxt_row_plan_build(const int32_t* row, int64_t T, int64_t M, int32_t* row_ptr, int32_t* perm, int64_t* info, void* workspace,
                         int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_row_plan_build";
    int rc;
    if ((rc = rows_extents_check(T, M, fn))) return rc;
    if (row_ptr == nullptr) return fail(SVOXT_ERR_INVALID, "%s: row_ptr is NULL", fn);
    if (info == nullptr) return fail(SVOXT_ERR_INVALID, "%s: info is NULL", fn);
    if (T > 0 && (row == nullptr || perm == nullptr)) return fail(SVOXT_ERR_INVALID, "%s: row / perm is NULL", fn);
    if (misaligned(row, 4) || misaligned(row_ptr, 4) || misaligned(perm, 4)) return fail(SVOXT_ERR_INVALID, "%s: row / row_ptr / perm is not 4-byte aligned", fn);
    if (misaligned(info, 8)) return fail(SVOXT_ERR_INVALID, "%s: info is not 8-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) {                                                // no sample: every segment empty, nothing long
        if ((rc = memset_async(row_ptr, sizeof(int32_t) * ((size_t)M + 1), st, fn))) return rc;
        return memset_async(info, sizeof(int64_t) * 4, st, fn);
    }
    if (misaligned(workspace, 4)) return fail(SVOXT_ERR_INVALID, "%s: workspace is not 4-byte aligned", fn);
    if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_row_plan_workspace_bytes(T, M), "svoxt_row_plan_workspace_bytes(T, M)")))
        return rc;
    const RowPlanSpace sp = row_plan_carve(workspace, T, M);
    if ((rc = memset_async(workspace, sp.clear_bytes, st, fn))) return rc;
    hipLaunchKernelGGL(row_key_kernel, dim3(launch_blocks(T)), dim3(kLaunchBlock), 0, st, row, T, M, sp.keys[0]);
    if ((rc = check_launch(fn))) return rc;
    // the keys are in [0, M]: sort over the bits of M, in passes of at most 8 bits, all of (nearly) the same width
    int bits = 1;
    while (((uint64_t)M >> bits) != 0) ++bits;
    const int passes = (bits + 7) / 8, per = (bits + passes - 1) / passes;
    int cur = 0;
    for (int p = 0, shift = 0; p < passes; ++p, shift += per) {
        const int b = bits - shift < per ? bits - shift : per;
        uint32_t* vals_out = p == passes - 1 ? reinterpret_cast<uint32_t*>(perm) : sp.vals[cur ^ 1];
        if ((rc = sort_pass(sp.keys[cur], p == 0 ? nullptr : sp.vals[cur], (uint32_t)T, shift, b, sp.counts, sp.starts, sp.chunks,
                            sp.keys[cur ^ 1], vals_out, st, fn)))
            return rc;
        cur ^= 1;
    }
    hipLaunchKernelGGL(row_ptr_kernel, dim3(launch_blocks(M + 1)), dim3(kLaunchBlock), 0, st, sp.keys[cur], T, M, row_ptr);
    hipLaunchKernelGGL(row_mark_kernel, dim3(launch_blocks(M + 1)), dim3(kLaunchBlock), 0, st, row_ptr, M, sp.flag, sp.nchunks, sp.longest);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.flag, (size_t)M + 1, sp.mchunks, sp.rank, st, fn)) ||
        (rc = exclusive_scan(sp.nchunks, (size_t)M + 1, sp.mchunks, sp.cstart, st, fn)))
        return rc;
    hipLaunchKernelGGL(row_info_kernel, dim3(1), dim3(64), 0, st, row_ptr, T, M, sp.longest, sp.rank, sp.cstart, info);
    return check_launch(fn);
}

int svoxt_row_plan_long(const int32_t* row_ptr, int64_t T, int64_t M, int64_t n_long, int64_t n_chunks, const void* workspace,
                        int64_t workspace_bytes, int32_t* long_rows, int32_t* long_chunk_ptr, int32_t* chunk_long, void* stream) {
    const char* fn = "svoxt_row_plan_long";
    int rc;
    const RowPlanRef plan{row_ptr, nullptr, long_rows, long_chunk_ptr, chunk_long, T, M, n_long, n_chunks};   // (the arrays to write)
    if ((rc = rows_extents_check(T, M, fn)) || (rc = row_plan_check(fn, plan))) return rc;
    if (long_chunk_ptr == nullptr) return fail(SVOXT_ERR_INVALID, "%s: long_chunk_ptr is NULL", fn);
    if (n_long > 0 && (row_ptr == nullptr || long_rows == nullptr || chunk_long == nullptr))
        return fail(SVOXT_ERR_INVALID, "%s: row_ptr / long_rows / chunk_long is NULL", fn);
    if (row_plan_misaligned(plan))
        return fail(SVOXT_ERR_INVALID, "%s: row_ptr / long_rows / long_chunk_ptr / chunk_long is not 4-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) return memset_async(long_chunk_ptr, sizeof(int32_t), st, fn);
    if (misaligned(workspace, 4)) return fail(SVOXT_ERR_INVALID, "%s: workspace is not 4-byte aligned", fn);
    if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_row_plan_workspace_bytes(T, M), "svoxt_row_plan_workspace_bytes(T, M)")))
        return rc;
    const RowPlanSpace sp = row_plan_carve(const_cast<void*>(workspace), T, M);
    hipLaunchKernelGGL(scatter_ranked_kernel<int32_t>, dim3(launch_blocks(M)), dim3(kLaunchBlock), 0, st, sp.flag, sp.rank, M, n_long, long_rows);
    hipLaunchKernelGGL(row_long_ptr_kernel, dim3(launch_blocks(M + 1)), dim3(kLaunchBlock), 0, st, sp.flag, sp.rank, sp.cstart, M, n_long,
                       n_chunks, long_chunk_ptr);
    hipLaunchKernelGGL(row_chunk_long_kernel, dim3(launch_blocks(n_chunks)), dim3(kLaunchBlock), 0, st, long_chunk_ptr, n_long, n_chunks,
                       chunk_long);
    return check_launch(fn);
}

int svoxt_gather_rows(const float* table, int64_t M, int32_t K, const int32_t* row, int64_t T, const int32_t* cols, int32_t n_cols,
                      float* out, void* stream) {
    const char* fn = "svoxt_gather_rows";
    int rc;
    if ((rc = rows_extents_check(T, M, fn))) return rc;
    if (K < 1) return fail(SVOXT_ERR_INVALID, "%s: K must be >= 1", fn);
    if ((rc = cols_check(fn, cols, n_cols, K))) return rc;
    const int Kc = cols != nullptr ? n_cols : K;
    if (!elems_fit((double)T, Kc) || !elems_fit((double)M, K))
        return fail(SVOXT_ERR_INVALID, "%s: T * columns and M * K must be below 2^38", fn);
    if (T == 0) return SVOXT_OK;
    if (row == nullptr || out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: row / out is NULL", fn);
    if (M > 0 && table == nullptr) return fail(SVOXT_ERR_INVALID, "%s: table is NULL", fn);
    if (misaligned(table, 4) || misaligned(row, 4) || misaligned(cols, 4) || misaligned(out, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    hipStream_t st = (hipStream_t)stream;
    if (cols == nullptr && K % 4 == 0 && !misaligned(table, 16) && !misaligned(out, 16)) {
        const int K4 = K / 4;
        hipLaunchKernelGGL(gather_rows4_kernel, launch_grid(T * K4), dim3(kLaunchBlock), 0, st, reinterpret_cast<const float4*>(table),
                           M, K4, row, T, reinterpret_cast<float4*>(out));
    } else {
        hipLaunchKernelGGL(gather_rows_kernel, launch_grid(T * Kc), dim3(kLaunchBlock), 0, st, table, M, (int)K, row, T, cols, Kc, out);
    }
    return check_launch(fn);
}

int64_t svoxt_reduce_rows_workspace_bytes(int64_t n_chunks, int32_t C) {
    if (!in31(n_chunks) || C < 1 || !elems_fit((double)n_chunks, C)) return -1;
    if (n_chunks == 0) return 0;
    return (int64_t)align256(sizeof(float) * (size_t)n_chunks * (size_t)C);
}

int svoxt_reduce_rows(const float* values, int64_t T, int32_t C, const int32_t* row_ptr, const int32_t* perm, int64_t M,
                      const int32_t* long_rows, const int32_t* long_chunk_ptr, const int32_t* chunk_long, int64_t n_long, int64_t n_chunks,
                      const int32_t* cols, int32_t n_cols, int32_t K, int32_t op, float empty, float* out, void* workspace,
                      int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_reduce_rows";
    int rc;
    const RowPlanRef plan{row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, T, M, n_long, n_chunks};
    if ((rc = rows_extents_check(T, M, fn))) return rc;
    if (C < 1 || K < 1) return fail(SVOXT_ERR_INVALID, "%s: C and K must be >= 1", fn);
    if ((rc = cols_check(fn, cols, n_cols, K))) return rc;
    if (C != (cols != nullptr ? n_cols : K))
        return fail(SVOXT_ERR_INVALID, "%s: values must have one column per selected column (C = n_cols, or C = K without cols)", fn);
    if (op != ROWS_SUM && op != ROWS_MEAN && op != ROWS_MAX && op != ROWS_MIN)
        return fail(SVOXT_ERR_INVALID, "%s: op must be one of SVOXT_ROWS_SUM / MEAN / MAX / MIN", fn);
    if (!elems_fit((double)T, C) || !elems_fit((double)M, K))
        return fail(SVOXT_ERR_INVALID, "%s: T * C and M * K must be below 2^38", fn);
    if ((rc = row_plan_check(fn, plan))) return rc;
    if (M == 0) return SVOXT_OK;
    if (out == nullptr || row_ptr == nullptr) return fail(SVOXT_ERR_INVALID, "%s: out / row_ptr is NULL", fn);
    if (T > 0 && (values == nullptr || perm == nullptr)) return fail(SVOXT_ERR_INVALID, "%s: values / perm is NULL", fn);
    if ((rc = row_plan_long_check(fn, plan))) return rc;
    if (misaligned(values, 4) || row_plan_misaligned(plan) || misaligned(cols, 4) || misaligned(out, 4) || misaligned(workspace, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    if (n_long > 0 &&
        (rc = workspace_check(fn, workspace, workspace_bytes, svoxt_reduce_rows_workspace_bytes(n_chunks, C), "svoxt_reduce_rows_workspace_bytes(n_chunks, C)")))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (cols != nullptr && (rc = memset_async(out, sizeof(float) * (size_t)M * (size_t)K, st, fn))) return rc;   // every element written
    float* partials = static_cast<float*>(workspace);
    const bool ok = with_int(IntSet<ROWS_SUM, ROWS_MEAN, ROWS_MAX, ROWS_MIN>{}, op, [&](auto OP) {
        // the partials of a mean are the sum's; the division is the join's (and the short rows')
        constexpr int PART = OP.value == ROWS_MEAN ? (int)ROWS_SUM : OP.value;
        rows_launch<OP.value, PART>(TableValues{values, T, (int)C}, (int)C, plan, cols, (int)K, empty, out, partials, st);
        return true;
    });
    if (!ok) return fail(SVOXT_ERR_INVALID, "%s: op must be one of SVOXT_ROWS_SUM / MEAN / MAX / MIN", fn);
    return check_launch(fn);
}

}  // extern "C"
