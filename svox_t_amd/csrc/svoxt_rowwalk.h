// svoxt_rowwalk.h -- the row reduction of DESIGN.md 4.21 over any source of per-sample values: reduce_rows reads them from
// a [T, C] table (svoxt_rows.hip), the deterministic render backward forms them on the fly (svoxt_rowgrad.hip).  Not part
// of the public C ABI.
//
// A source V hands out one column at a time: `auto col = src.col(j)` once per lane, then `col.at(k)` = the value of
// sample k at column j (0.f for a k outside [0, T): a plan's perm is in range, never the zero).  The three kernels are
// the order rule of include/svoxt.h (svoxt_reduce_rows), which is part of the definition:
//   rows_short_kernel   a lane per (row, column) walks the row's samples in ascending index, for rows of at most
//                       SVOXT_ROW_CHUNK samples, and writes `empty` for rows without one;
//   rows_chunk_kernel   a lane per (chunk, column) of the long rows leaves the chunk's partial in the workspace;
//   rows_join_kernel    a lane per (long row, column) joins the partials in chunk order.
// On the host: RowPlanRef, a caller's plan as one value, the checks every entry point over a plan makes
// of it (row_plan_check, row_plan_long_check, row_plan_misaligned, cols_check), and rows_launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

constexpr int kRowChunk = SVOXT_ROW_CHUNK;
enum { ROWS_SUM = SVOXT_ROWS_SUM, ROWS_MEAN = SVOXT_ROWS_MEAN, ROWS_MAX = SVOXT_ROWS_MAX, ROWS_MIN = SVOXT_ROWS_MIN };

// T words inside the workspace of svoxt_row_plan_build(.., T, M, ..) that are free from the build's last kernel on: a later
// kernel on the same stream may keep a value per sample there (svoxt_row_plan_long does not read them).  svoxt_rows.hip.
uint32_t* row_plan_sort_scratch(void* workspace, int64_t T, int64_t M);

// values float32 [T, C] in memory
struct TableValues {
    const float* __restrict__ values;
    int64_t T;
    int C;
    struct Col {
        const float* __restrict__ p;
        int64_t T;
        int C;
        __device__ __forceinline__ float at(int64_t k) const { return (k >= 0 && k < T) ? p[k * C] : 0.f; }
    };
    __device__ __forceinline__ Col col(int j) const { return Col{values + j, T, C}; }
};

// One step of a row's walk.  SUM / MEAN: acc + v.  MAX / MIN: the larger / smaller, NaN as soon as either is.
template <int OP>
__device__ __forceinline__ float rows_step(float acc, float v) {
    if constexpr (OP == ROWS_SUM || OP == ROWS_MEAN) return acc + v;
    else if constexpr (OP == ROWS_MAX) return (v > acc || v != v) ? v : acc;
    else return (v < acc || v != v) ? v : acc;
}

// the samples perm[b0 .. b1) of one chunk (or one short row) at one column; b1 > b0
template <int OP, class Col>
__device__ __forceinline__ float rows_walk(const Col& col, const int32_t* __restrict__ perm, int32_t b0, int32_t b1) {
    float acc = 0.f;
    int32_t p = b0;
    if constexpr (OP == ROWS_MAX || OP == ROWS_MIN) acc = col.at(perm[p++]);
#pragma unroll 4
    for (; p < b1; ++p) acc = rows_step<OP>(acc, col.at(perm[p]));
    return acc;
}

// out[r, c] for the rows of at most kRowChunk samples; lane t = r * C + j, c = cols[j] or j, out has K floats a row
template <int OP, class V>
__global__ void __launch_bounds__(kLaunchBlock)
rows_short_kernel(V src, int64_t T, int C, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ perm, int64_t M,
                  const int32_t* __restrict__ cols, int K, float empty, float* __restrict__ out) {
    const int64_t t = launch_lane();
    const int64_t r = t / C;
    if (r >= M) return;
    const int j = (int)(t - r * C);
    const int c = cols != nullptr ? cols[j] : j;
    if (c < 0 || c >= K) return;
    int32_t b0 = row_ptr[r], b1 = row_ptr[r + 1];
    b0 = b0 < 0 ? 0 : b0;
    b1 = (int64_t)b1 > T ? (int32_t)T : b1;
    const int32_t n = b1 - b0;
    if (n > kRowChunk) return;                                   // the long rows' kernels write it
    float v = empty;
    if (n > 0) {
        v = rows_walk<OP>(src.col(j), perm, b0, b1);
        if constexpr (OP == ROWS_MEAN) v = v / (float)n;
    }
    out[r * K + c] = v;
}

// partials[ch, j] for chunk ch of the long rows; lane t = ch * C + j
template <int OP, class V>
__global__ void __launch_bounds__(kLaunchBlock)
rows_chunk_kernel(V src, int64_t T, int C, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ perm, int64_t M,
                  const int32_t* __restrict__ long_rows, const int32_t* __restrict__ long_chunk_ptr,
                  const int32_t* __restrict__ chunk_long, int64_t n_long, int64_t n_chunks, float* __restrict__ partials) {
    const int64_t t = launch_lane();
    const int64_t ch = t / C;
    if (ch >= n_chunks) return;
    const int j = (int)(t - ch * C);
    float v = 0.f;
    const int64_t li = chunk_long[ch];
    if (li >= 0 && li < n_long) {
        const int64_t r = long_rows[li];
        const int64_t jc = ch - (int64_t)long_chunk_ptr[li];
        if (r >= 0 && r < M && jc >= 0) {
            int64_t b1 = row_ptr[r + 1];
            b1 = b1 > T ? T : b1;
            const int64_t c0 = (int64_t)row_ptr[r] + jc * kRowChunk;
            const int64_t c1 = c0 + kRowChunk < b1 ? c0 + kRowChunk : b1;
            if (c0 >= 0 && c1 > c0) v = rows_walk<OP>(src.col(j), perm, (int32_t)c0, (int32_t)c1);
        }
    }
    partials[t] = v;
}

// out[r, c] = (p_0 + p_1) + p_2 ... over the long row's chunks, in chunk order; lane t = li * C + j
template <int OP>
__global__ void __launch_bounds__(kLaunchBlock)
rows_join_kernel(const float* __restrict__ partials, int C, const int32_t* __restrict__ row_ptr, int64_t M,
                 const int32_t* __restrict__ long_rows, const int32_t* __restrict__ long_chunk_ptr, int64_t n_long, int64_t n_chunks,
                 const int32_t* __restrict__ cols, int K, float* __restrict__ out) {
    const int64_t t = launch_lane();
    const int64_t li = t / C;
    if (li >= n_long) return;
    const int j = (int)(t - li * C);
    const int c = cols != nullptr ? cols[j] : j;
    const int64_t r = long_rows[li];
    if (c < 0 || c >= K || r < 0 || r >= M) return;
    int64_t q0 = long_chunk_ptr[li], q1 = long_chunk_ptr[li + 1];
    q0 = q0 < 0 ? 0 : q0;
    q1 = q1 > n_chunks ? n_chunks : q1;
    if (q1 <= q0) return;
    float acc = partials[q0 * C + j];
#pragma unroll 4
    for (int64_t q = q0 + 1; q < q1; ++q) acc = rows_step<OP>(acc, partials[q * C + j]);
    if constexpr (OP == ROWS_MEAN) acc = acc / (float)(row_ptr[r + 1] - row_ptr[r]);
    out[r * K + c] = acc;
}

// A caller's row plan as one host-side value: what svoxt_row_plan_build / _long wrote for T samples (or entries) and M
// rows.  The entry points build it from their arguments; the kernels take its pointers one by one (rows_launch), as
// __restrict__ parameters.
struct RowPlanRef {
    const int32_t *row_ptr, *perm, *long_rows, *long_chunk_ptr, *chunk_long;
    int64_t T, M, n_long, n_chunks;
};
// The counts of the long rows against T and M; `t_name` is what the caller's text calls T ("8 Q" for a stencil's entries).
inline int row_plan_check(const char* fn, const RowPlanRef& p, const char* t_name = "T") {
    if (p.n_long < 0 || p.n_long > p.M || p.n_long > p.T / (kRowChunk + 1))
        return fail(SVOXT_ERR_INVALID, "%s: n_long must be in [0, min(M, %s / (SVOXT_ROW_CHUNK + 1))]", fn, t_name);
    if (p.n_chunks < 2 * p.n_long || p.n_chunks > p.T / kRowChunk + p.n_long)
        return fail(SVOXT_ERR_INVALID, "%s: n_chunks must be in [2 n_long, %s / SVOXT_ROW_CHUNK + n_long]", fn, t_name);
    return SVOXT_OK;
}
// the long rows' arrays of a plan that is read: there where there are long rows
inline int row_plan_long_check(const char* fn, const RowPlanRef& p) {
    if (p.n_long > 0 && (p.long_rows == nullptr || p.long_chunk_ptr == nullptr || p.chunk_long == nullptr))
        return fail(SVOXT_ERR_INVALID, "%s: long_rows / long_chunk_ptr / chunk_long is NULL", fn);
    return SVOXT_OK;
}
inline bool row_plan_misaligned(const RowPlanRef& p) {
    return misaligned(p.row_ptr, 4) || misaligned(p.perm, 4) || misaligned(p.long_rows, 4) || misaligned(p.long_chunk_ptr, 4) ||
           misaligned(p.chunk_long, 4);
}
// a column selection over a table of K columns: none (NULL / 0), or n_cols of them
inline int cols_check(const char* fn, const int32_t* cols, int32_t n_cols, int32_t K) {
    if ((cols == nullptr) != (n_cols == 0) || n_cols < 0 || n_cols > K)
        return fail(SVOXT_ERR_INVALID, "%s: cols / n_cols must be NULL / 0 (all columns) or n_cols in [1, K] distinct columns", fn);
    return SVOXT_OK;
}

// The three launches over a plan on `st`: the short rows, and with long rows their chunks and the join.  PART is the
// op of the chunk partials (a mean's are the sum's; the division is the join's and the short rows').
template <int OP, int PART, class V>
inline void rows_launch(const V& src, int C, const RowPlanRef& p, const int32_t* cols, int K, float empty, float* out, float* partials,
                        hipStream_t st) {
    hipLaunchKernelGGL((rows_short_kernel<OP, V>), launch_grid(p.M * C), dim3(kLaunchBlock), 0, st, src, p.T, C, p.row_ptr, p.perm, p.M,
                       cols, K, empty, out);
    if (p.n_long > 0) {
        hipLaunchKernelGGL((rows_chunk_kernel<PART, V>), launch_grid(p.n_chunks * C), dim3(kLaunchBlock), 0, st, src, p.T, C, p.row_ptr,
                           p.perm, p.M, p.long_rows, p.long_chunk_ptr, p.chunk_long, p.n_long, p.n_chunks, partials);
        hipLaunchKernelGGL((rows_join_kernel<OP>), launch_grid(p.n_long * C), dim3(kLaunchBlock), 0, st, partials, C, p.row_ptr, p.M,
                           p.long_rows, p.long_chunk_ptr, p.n_long, p.n_chunks, cols, K, out);
    }
}

}  // namespace svoxt
