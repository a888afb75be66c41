// svoxt_scan.hip -- running values along a ray, a crossing of the running weight, and a subset of the lists (DESIGN.md
// 4.25; not in the reference).  The per-sample family's conventions (svoxt_samples.hip): ray q's segment is
// max(offsets[q], 0) .. min(offsets[q + 1], T), float32, sequential in list order, no contraction, no float atomic.
//
//   ray_scan       a lane per (ray, channel), t = q * C + c, walks the segment in list order (or from the last sample to
//                  the first: reverse) from acc = 0 / 1 / -inf / +inf:
//                      new = acc + v | acc * v | (v > acc) ? v : acc | (v < acc) ? v : acc;   out = new (exclusive: acc)
//                  Backward, one entry per sample, no atomics, no workspace:
//                      sum       the scan of grad_out in the other direction (the forward kernel)
//                      prod      zero-safe, no division; positions 0 .. n-1 along the scan direction:
//                                sweep 1, against it, into grad_values:  S_j = g_j + v_{j+1} S_{j+1},  S_{n-1} = g_{n-1}
//                                                     (exclusive:         S_j = g_{j+1} + v_{j+1} S_{j+1},  S_{n-1} = 0)
//                                sweep 2, along it, P = 1:  grad_j = P * S_j;  P *= v_j
//                      max / min one sweep along the direction with the running argument: the g of every position is
//                                added, in scan order from 0, to the sample that supplied the value written there
//                                (inclusive: the argument moves before the add; exclusive: after it, and a position
//                                that wrote the identity sends its g nowhere)
//   ray_quantile   a lane per (ray, quantile): c += w over the samples with w > 0; the first of them with c >= target,
//                  and where inside it the target lies
//   select         flag -> scan -> emit (svoxt_listemit.h, the per-sample shape without a 64-bit total): pos = exclusive scan of keep over T + 1 entries;
//                  offsets'[q] = pos[clamped offsets[q]], T' = pos[T]; a lane per sample copies the kept samples to pos[k]
// C ABI: svoxt_ray_scan_* / svoxt_ray_quantile / svoxt_samples_select_* (include/svoxt.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_listemit.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

template <int OP>
__device__ __forceinline__ float scan_identity() {
    if constexpr (OP == SVOXT_SCAN_SUM) return 0.f;
    else if constexpr (OP == SVOXT_SCAN_PROD) return 1.f;
    else if constexpr (OP == SVOXT_SCAN_MAX) return -__builtin_huge_valf();
    else return __builtin_huge_valf();
}
// (max / min: a NaN is never taken, the first occurrence wins a tie)
template <int OP>
__device__ __forceinline__ float scan_step(float acc, float v) {
    if constexpr (OP == SVOXT_SCAN_SUM) return acc + v;
    else if constexpr (OP == SVOXT_SCAN_PROD) return acc * v;
    else if constexpr (OP == SVOXT_SCAN_MAX) return v > acc ? v : acc;
    else return v < acc ? v : acc;
}

// The walk of lane t = q * C + c: n samples, the first at element `at` of a [T, C] array, `step` elements apart
// (negative for a reverse scan); n <= 0 for an empty or malformed segment.
struct ScanWalk {
    int64_t n, at, step;
};
__device__ __forceinline__ bool scan_walk(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, int C, bool reverse, ScanWalk& w) {
    const int64_t t = launch_lane();
    const int64_t q = t / C;
    if (q >= Q) return false;
    const int64_t c = t - q * C;
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    w.n = e - b;
    w.at = (reverse ? e - 1 : b) * C + c;
    w.step = reverse ? -(int64_t)C : (int64_t)C;
    return true;
}

template <int OP>
__global__ void __launch_bounds__(kLaunchBlock)
ray_scan_fwd_kernel(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ values, int C,
                    bool exclusive, bool reverse, float* __restrict__ out) {
    ScanWalk w;
    if (!scan_walk(offsets, Q, T, C, reverse, w)) return;
    float acc = scan_identity<OP>();
    int64_t i = w.at;
    for (int64_t j = 0; j < w.n; ++j, i += w.step) {
        const float nw = scan_step<OP>(acc, values[i]);
        out[i] = exclusive ? acc : nw;
        acc = nw;
    }
}

__global__ void __launch_bounds__(kLaunchBlock)
ray_scan_prod_bwd_kernel(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ values, int C,
                         bool exclusive, bool reverse, const float* __restrict__ grad_out, float* __restrict__ grad_values) {
    ScanWalk w;
    if (!scan_walk(offsets, Q, T, C, reverse, w) || w.n <= 0) return;
    // sweep 1, against the direction: S into grad_values
    int64_t i = w.at + (w.n - 1) * w.step;
    float S = 0.f, v_next = 0.f, g_next = 0.f;
    for (int64_t j = w.n - 1; j >= 0; --j, i -= w.step) {
        const float g = grad_out[i], v = values[i];
        if (j == w.n - 1) S = exclusive ? 0.f : g;
        else S = (exclusive ? g_next : g) + v_next * S;
        grad_values[i] = S;
        v_next = v;
        g_next = g;
    }
    // sweep 2, along it
    float P = 1.f;
    i = w.at;
    for (int64_t j = 0; j < w.n; ++j, i += w.step) {
        grad_values[i] = P * grad_values[i];
        P *= values[i];
    }
}

template <int OP>
__global__ void __launch_bounds__(kLaunchBlock)
ray_scan_arg_bwd_kernel(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ values, int C,
                        bool exclusive, bool reverse, const float* __restrict__ grad_out, float* __restrict__ grad_values) {
    ScanWalk w;
    if (!scan_walk(offsets, Q, T, C, reverse, w)) return;
    float acc = scan_identity<OP>(), sum = 0.f;
    int64_t arg = -1;                                            // the element that supplied acc; its gradient so far is `sum`
    int64_t i = w.at;
    for (int64_t j = 0; j < w.n; ++j, i += w.step) {
        const float v = values[i], g = grad_out[i];
        if (exclusive && arg >= 0) sum += g;
        if (OP == SVOXT_SCAN_MAX ? v > acc : v < acc) {            // (taken, as scan_step takes it)
            if (arg >= 0) grad_values[arg] = sum;
            arg = i;
            sum = 0.f;
            acc = v;
        } else {
            grad_values[i] = 0.f;
        }
        if (!exclusive && arg >= 0) sum += g;
    }
    if (arg >= 0) grad_values[arg] = sum;
}

// lane t = q * nq + i
__global__ void __launch_bounds__(kLaunchBlock)
ray_quantile_kernel(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ w,
                    const float* __restrict__ qs, int nq, bool normalize, int64_t* __restrict__ index, float* __restrict__ frac) {
    const int64_t t = launch_lane();
    const int64_t q = t / nq;
    if (q >= Q) return;
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    float target = qs[t - q * nq];
    if (normalize) {
        float total = 0.f;
        for (int64_t k = b; k < e; ++k) {
            const float wk = w[k];
            if (wk > 0.f) total = total + wk;
        }
        target = target * total;
    }
    float c = 0.f, f = 0.f;
    int64_t at = -1;
    for (int64_t k = b; k < e; ++k) {
        const float wk = w[k];
        if (wk > 0.f) {
            const float before = c;
            c = c + wk;
            if (c >= target) {
                at = k;
                f = (target - before) / wk;
                f = !(f > 0.f) ? 0.f : (f > 1.f ? 1.f : f);
                break;
            }
        }
    }
    index[t] = at;
    frac[t] = f;
}

// ------------------------------------------------------------------------------------------------------------- select
// workspace of svoxt_samples_select_count, read again by _emit: the per-sample ListSpace (svoxt_listemit.h) without a
// total (T' <= T), counts = flag, starts = pos

__global__ void __launch_bounds__(kLaunchBlock)
select_flag_kernel(const uint8_t* __restrict__ keep, int64_t T, uint32_t* __restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (k <= T) flag[k] = (k < T && keep[k] != 0) ? 1u : 0u;
}

__global__ void __launch_bounds__(kLaunchBlock)
select_emit_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ pos, int64_t T, int64_t T_out,
                   const int32_t* __restrict__ ray, const int32_t* __restrict__ row, const float* __restrict__ depth,
                   const float* __restrict__ length, int32_t* __restrict__ ray_out, int32_t* __restrict__ row_out,
                   float* __restrict__ depth_out, float* __restrict__ length_out, int64_t* __restrict__ index) {
    const int64_t k = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (k >= T || keep[k] == 0) return;
    const int64_t at = (int64_t)pos[k];
    if (at >= T_out) return;                                     // (the caller's T' is the scan's: never taken)
    ray_out[at] = ray[k];
    row_out[at] = row[k];
    depth_out[at] = depth[k];
    length_out[at] = length[k];
    index[at] = k;
}

// ------------------------------------------------------------------------------------------------------------- checks
static int scan_check(int64_t Q, int64_t T, int32_t C, int32_t op, int32_t flags, const char* fn) {
    int rc;
    if ((rc = extent31_check(fn, Q, "Q")) || (rc = extent31_check(fn, T, "T"))) return rc;
    if (C < 1 || !elems_fit((double)Q, C) || !elems_fit((double)T, C))
        return fail(SVOXT_ERR_INVALID, "%s: C must be >= 1 with Q * C and T * C below 2^38", fn);
    if (op < SVOXT_SCAN_SUM || op > SVOXT_SCAN_MIN) return fail(SVOXT_ERR_INVALID, "%s: op must be SVOXT_SCAN_SUM / PROD / MAX / MIN (0 .. 3)", fn);
    if ((flags & ~(SVOXT_SCAN_EXCLUSIVE | SVOXT_SCAN_REVERSE)) != 0)
        return fail(SVOXT_ERR_INVALID, "%s: flags must be a combination of SVOXT_SCAN_EXCLUSIVE and SVOXT_SCAN_REVERSE", fn);
    return SVOXT_OK;
}

template <int OP>
static void launch_scan_fwd(const int64_t* offsets, int64_t Q, int64_t T, const float* values, int C, bool exclusive, bool reverse,
                            float* out, hipStream_t st) {
    hipLaunchKernelGGL(ray_scan_fwd_kernel<OP>, launch_grid(Q * C), dim3(kLaunchBlock), 0, st, offsets, Q, T, values, C,
                       exclusive, reverse, out);
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int svoxt_ray_scan_fwd(const int64_t* offsets, int64_t Q, int64_t T, const float* values, int32_t C, int32_t op, int32_t flags,
                       float* out, void* stream) {
    const char* fn = "svoxt_ray_scan_fwd";
    int rc;
    if ((rc = scan_check(Q, T, C, op, flags, fn))) return rc;
    if (Q == 0 || T == 0) return SVOXT_OK;
    if (offsets == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets is NULL", fn);
    if (values == nullptr || out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: values / out is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(values, 4) || misaligned(out, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the float arrays: 4)", fn);
    if (overlap(values, out, 4.0 * (double)T * C)) return fail(SVOXT_ERR_INVALID, "%s: out overlaps values", fn);
    const bool ex = (flags & SVOXT_SCAN_EXCLUSIVE) != 0, rev = (flags & SVOXT_SCAN_REVERSE) != 0;
    hipStream_t st = (hipStream_t)stream;
    with_int(IntSet<SVOXT_SCAN_SUM, SVOXT_SCAN_PROD, SVOXT_SCAN_MAX, SVOXT_SCAN_MIN>{}, op, [&](auto OP) {
        launch_scan_fwd<OP.value>(offsets, Q, T, values, (int)C, ex, rev, out, st);
        return true;
    });
    return check_launch(fn);
}

int svoxt_ray_scan_bwd(const int64_t* offsets, int64_t Q, int64_t T, const float* values, int32_t C, int32_t op, int32_t flags,
                       const float* grad_out, float* grad_values, void* stream) {
    const char* fn = "svoxt_ray_scan_bwd";
    int rc;
    if ((rc = scan_check(Q, T, C, op, flags, fn))) return rc;
    if (T == 0) return SVOXT_OK;
    if (grad_out == nullptr || grad_values == nullptr) return fail(SVOXT_ERR_INVALID, "%s: grad_out / grad_values is NULL", fn);
    if (op != SVOXT_SCAN_SUM && values == nullptr) return fail(SVOXT_ERR_INVALID, "%s: values is NULL (only the sum does without them)", fn);
    if (Q > 0 && offsets == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(values, 4) || misaligned(grad_out, 4) || misaligned(grad_values, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the float arrays: 4)", fn);
    const double bytes = 4.0 * (double)T * C;
    if (overlap(grad_out, grad_values, bytes) || overlap(values, grad_values, bytes))
        return fail(SVOXT_ERR_INVALID, "%s: grad_values overlaps grad_out / values", fn);
    const bool ex = (flags & SVOXT_SCAN_EXCLUSIVE) != 0, rev = (flags & SVOXT_SCAN_REVERSE) != 0;
    hipStream_t st = (hipStream_t)stream;
    // one entry per sample: samples outside every segment get 0
    if ((rc = memset_async(grad_values, (size_t)T * (size_t)C * sizeof(float), st, fn))) return rc;
    if (Q == 0) return SVOXT_OK;
    const dim3 grid = launch_grid(Q * C), block(kLaunchBlock);
    if (op == SVOXT_SCAN_SUM) launch_scan_fwd<SVOXT_SCAN_SUM>(offsets, Q, T, grad_out, (int)C, ex, !rev, grad_values, st);
    else if (op == SVOXT_SCAN_PROD)
        hipLaunchKernelGGL(ray_scan_prod_bwd_kernel, grid, block, 0, st, offsets, Q, T, values, (int)C, ex, rev, grad_out, grad_values);
    else if (op == SVOXT_SCAN_MAX)
        hipLaunchKernelGGL(ray_scan_arg_bwd_kernel<SVOXT_SCAN_MAX>, grid, block, 0, st, offsets, Q, T, values, (int)C, ex, rev, grad_out, grad_values);
    else
        hipLaunchKernelGGL(ray_scan_arg_bwd_kernel<SVOXT_SCAN_MIN>, grid, block, 0, st, offsets, Q, T, values, (int)C, ex, rev, grad_out, grad_values);
    return check_launch(fn);
}

int svoxt_ray_quantile(const int64_t* offsets, int64_t Q, int64_t T, const float* w, const float* q, int32_t nq, int32_t normalize,
                       int64_t* index, float* frac, void* stream) {
    const char* fn = "svoxt_ray_quantile";
    int rc;
    if ((rc = extent31_check(fn, Q, "Q")) || (rc = extent31_check(fn, T, "T"))) return rc;
    if (nq < 1 || !elems_fit((double)Q, nq)) return fail(SVOXT_ERR_INVALID, "%s: nq must be >= 1 with Q * nq below 2^38", fn);
    if (Q == 0) return SVOXT_OK;
    if (offsets == nullptr || q == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets / q is NULL", fn);
    if (index == nullptr || frac == nullptr) return fail(SVOXT_ERR_INVALID, "%s: index / frac is NULL", fn);
    if (T > 0 && w == nullptr) return fail(SVOXT_ERR_INVALID, "%s: w is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(index, 8) || misaligned(w, 4) || misaligned(q, 4) || misaligned(frac, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets, index: 8 bytes, the float arrays: 4)", fn);
    hipLaunchKernelGGL(ray_quantile_kernel, launch_grid(Q * nq), dim3(kLaunchBlock), 0, (hipStream_t)stream, offsets, Q, T, w, q,
                       (int)nq, normalize != 0, index, frac);
    return check_launch(fn);
}

int64_t svoxt_samples_select_workspace_bytes(int64_t T) {
    return list_space_bytes(T, 1, false);
}

int svoxt_samples_select_count(const uint8_t* keep, const int64_t* offsets, int64_t Q, int64_t T, int64_t* offsets_out, int64_t* total,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_samples_select_count";
    int rc;
    if ((rc = extent31_check(fn, Q, "Q")) || (rc = extent31_check(fn, T, "T")) || (rc = counts_out_check(fn, offsets_out, total))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) return clear_counts(fn, offsets_out, Q, total, st);          // nothing to keep: empty lists
    if (keep == nullptr || offsets == nullptr) return fail(SVOXT_ERR_INVALID, "%s: keep / offsets is NULL", fn);
    if (misaligned(offsets, 8)) return fail(SVOXT_ERR_INVALID, "%s: offsets is not 8-byte aligned", fn);
    if (overlap(offsets, offsets_out, 8.0 * (double)(Q + 1))) return fail(SVOXT_ERR_INVALID, "%s: offsets_out overlaps offsets", fn);
    ListSpace sp;
    if ((rc = list_space_check(fn, workspace, workspace_bytes, (size_t)T + 1, false, "svoxt_samples_select_workspace_bytes(T)", &sp))) return rc;
    hipLaunchKernelGGL(select_flag_kernel, dim3(launch_blocks(T + 1)), dim3(kLaunchBlock), 0, st, keep, T, sp.counts);
    return list_pos_offsets<false>(fn, sp, offsets, Q, T, offsets_out, total, st);    // (T' = pos[T])
}

int svoxt_samples_select_emit(const uint8_t* keep, int64_t T, const void* workspace, int64_t workspace_bytes, const int32_t* ray,
                              const int32_t* row, const float* depth, const float* length, int64_t T_out, int32_t* ray_out,
                              int32_t* row_out, float* depth_out, float* length_out, int64_t* index, void* stream) {
    const char* fn = "svoxt_samples_select_emit";
    int rc;
    if ((rc = extent31_check(fn, T, "T"))) return rc;
    if (T_out < 0 || T_out > T) return fail(SVOXT_ERR_INVALID, "%s: T_out must be in [0, T]", fn);
    if (T_out == 0) return SVOXT_OK;
    if (keep == nullptr) return fail(SVOXT_ERR_INVALID, "%s: keep is NULL", fn);
    ListSpace sp;
    if ((rc = emit_arrays_check(fn, ray, row, depth, length, ray_out, row_out, depth_out, length_out, index)) ||
        (rc = list_space_check(fn, workspace, workspace_bytes, (size_t)T + 1, false, "svoxt_samples_select_workspace_bytes(T)", &sp)))
        return rc;
    hipLaunchKernelGGL(select_emit_kernel, dim3(launch_blocks(T)), dim3(kLaunchBlock), 0, (hipStream_t)stream, keep, sp.starts, T, T_out, ray,
                       row, depth, length, ray_out, row_out, depth_out, length_out, index);
    return check_launch(fn);
}

}  // extern "C"
