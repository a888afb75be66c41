// svoxt_viewrot.hip -- shade_samples with per-row rotations of the view direction (the reference serves
// transformation_matrices in its render kernels only and has no gradient in them): the colour of every sample of a
// RaySamples list from its feature row and the basis of u = rotations[row] * viewdirs[ray], and the three gradients --
// in the feature table, in the rotations and in the view directions.  No [T, basis_dim] and no [T, K] array, no float
// atomic anywhere; every result has the same bits in every run.
//
// The shading core is svoxt_shade.h's, over the basis source RotBasis<BD> (SH: BD at compile time, in registers; SG / ASG:
// one lobe at a time); this file holds what only the rotated call has, and the entry points.
//   forward      shade_fwd_kernel<RotBasis<BD>>  the plain call's kernel; the lane rotates its ray's direction by its row's
//                                              matrix and forms the basis
//   features     the row kernels of svoxt_rowwalk.h over ShadeValues<RotBasis<BD>>: a lane per (row, column) holds the row's
//                matrix (loaded once, at its first sample) and forms (g_values[k, c] * d[k, c]) * B_i(k) on the fly
//   gu           shade_rot_dir_kernel<BD, CS>  a lane per sample: gB_i = sum_c t[k, c] * features[row, c * bd + i], then
//                                              view_basis_grad (svoxt_shade.h) at u(k) into gu[k, 0:3], 12 bytes a sample
//   rotations    the row kernels over RotGradValues: a lane per (row, a, b) sums gu[k, a] * viewdirs[ray[k], b]
//   viewdirs     shade_rot_vdirs_kernel        a lane per ray over its segment in list order: acc[b] += m[a, b] * gu[k, a]
// C ABI: svoxt_shade_rot_* (include/svoxt.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_device.h"
#include "svoxt_host.h"
#include "svoxt_rowwalk.h"
#include "svoxt_shade.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

// ------------------------------------------------------------------------------------------------------------- values
// gu[k, a] * viewdirs[ray[k], b] at column j = a * d + b of the row's matrix; the columns outside the 3 x 3 block are ZERO
struct RotGradValues {
    const int32_t* __restrict__ ray;
    const float* __restrict__ gu;
    const float* __restrict__ vdirs;
    int64_t T, Q;
    int d;
    struct Col {
        const int32_t* __restrict__ ray;
        const float* __restrict__ g;       // gu + a
        const float* __restrict__ v;       // viewdirs + b
        int64_t T, Q;
        bool zero;
        __device__ __forceinline__ float at(int64_t k) const {
            if (zero || k < 0 || k >= T) return 0.f;
            const int64_t q = ray[k];
            if (q < 0 || q >= Q) return 0.f;
            return g[3 * k] * v[3 * q];
        }
    };
    __device__ __forceinline__ Col col(int j) const {
        const int a = j / d, b = j - a * d;
        const bool zero = a >= 3 || b >= 3;
        return Col{ray, gu + (zero ? 0 : a), vdirs + (zero ? 0 : b), T, Q, zero};
    }
};

// ------------------------------------------------------------------------------------------------------------------ gu
// lane k: gu[k, 0:3] = view_basis_grad at u(k) with grad_basis = gB(k), gB_i = sum over c ascending from 0.f of t[k, c] *
// features[row[k], c * bd + i] inside [min_comp, max_comp] and 0.f outside; t[k, c] = grad_values[k, c] * d[k, c].  SG reads
// B_i(k) recomputed by the forward's sequence.  CS: C at compile time, t in registers (0: the run-time loop forms t[k, c]
// where it is used).  Zeros for a sample whose row or ray is outside its range and for a NULL grad_values.
template <int BD, int CS>
__global__ void __launch_bounds__(kLaunchBlock)
shade_rot_dir_kernel(const float* __restrict__ features, int K, int C_rt, int bd_rt, int min_comp, int max_comp, bool activate, RotDev R,
                     int64_t T, const int32_t* __restrict__ row, const int32_t* __restrict__ ray, const float* __restrict__ values,
                     const float* __restrict__ gv, float* __restrict__ gu) {
    const int C = CS > 0 ? CS : C_rt;
    const int bd = BD > 0 ? BD : bd_rt;
    const int64_t k = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (k >= T) return;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    const int64_t idx = row[k], q = ray[k];
    if (gv != nullptr && idx >= 0 && idx < R.M && q >= 0 && q < R.Q) {
        const TreeDev tr = lobes_only(R.extra, R.extra_rows, R.extra_cols);
        Mat3 m;
        m.load(R.rot, idx, R.d);
        float u0, u1, u2;
        m.apply(R.vdirs + 3 * q, u0, u1, u2);
        const float* __restrict__ frow = features + idx * K;
        const float* __restrict__ g = gv + k * C;
        const float* __restrict__ v = values + k * C;
        auto bracket = [&](int c) { return shade_bracket(g[c], v + c, activate); };
        [[maybe_unused]] float ts[CS > 0 ? CS : 1];
        if constexpr (CS > 0) {
#pragma unroll
            for (int c = 0; c < CS; ++c) ts[c] = bracket(c);
        }
        auto gb = [&](int i) {
            float s = 0.f;
            if (i >= min_comp && i <= max_comp) {
                if constexpr (CS > 0) {
#pragma unroll
                    for (int c = 0; c < CS; ++c) s += ts[c] * frow[c * bd + i];
                } else {
                    for (int c = 0; c < C; ++c) s += bracket(c) * frow[c * bd + i];
                }
            }
            return s;
        };
        auto b = [&](int i) { return lobe_value(R.format, tr, u0, u1, u2, i, bd); };
        view_basis_grad(tr, R.format, bd, u0, u1, u2, gb, b, gx, gy, gz);
    }
    float* __restrict__ o = gu + 3 * k;
    o[0] = gx; o[1] = gy; o[2] = gz;
}

// ------------------------------------------------------------------------------------------------------------ viewdirs
// lane q: grad_vdirs[q, b] = the sum over ray q's segment in list order, and per sample over a = 0, 1, 2, of m[a, b] *
// gu[k, a], m the matrix of the sample's row; three accumulators from 0.f.  A lane owns its ray: no ray's sum is shared
// between lanes or workgroups.  Samples of another ray or of a row outside [0, M) are passed over.
__global__ void __launch_bounds__(kLaunchBlock)
shade_rot_vdirs_kernel(const float* __restrict__ rot, int d, int64_t M, int64_t Q, int64_t T, const int64_t* __restrict__ offsets,
                       const int32_t* __restrict__ row, const int32_t* __restrict__ ray, const float* __restrict__ gu,
                       float* __restrict__ grad_vdirs) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (q >= Q) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    for (int64_t k = b; k < e; ++k) {
        const int64_t idx = row[k];
        if (ray[k] != q || idx < 0 || idx >= M) continue;
        const float* __restrict__ m = rot + idx * (d * d);
        const float* __restrict__ g = gu + 3 * k;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float ga = g[a];
            a0 += m[a * d] * ga;
            a1 += m[a * d + 1] * ga;
            a2 += m[a * d + 2] * ga;
        }
    }
    float* __restrict__ o = grad_vdirs + 3 * q;
    o[0] = a0; o[1] = a1; o[2] = a2;
}

// ------------------------------------------------------------------------------------------------------------- checks
inline bool ranges_overlap(const void* a, double a_bytes, const void* b, double b_bytes) {
    if (a == nullptr || b == nullptr) return false;
    const double x = (double)(uintptr_t)a, y = (double)(uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// `out` of out_bytes against the inputs of a rotated call
static bool rot_out_overlaps(const void* out, double out_bytes, const float* features, int64_t M, int32_t K, const RotArgs& a, int64_t Q,
                             const int32_t* row, const int32_t* ray, int64_t T) {
    const double dd = (double)a.rot_dim * a.rot_dim;
    return ranges_overlap(out, out_bytes, features, 4.0 * (double)M * K) || ranges_overlap(out, out_bytes, a.rotations, 4.0 * (double)M * dd) ||
           ranges_overlap(out, out_bytes, a.viewdirs, 12.0 * (double)Q) || ranges_overlap(out, out_bytes, row, 4.0 * (double)T) ||
           ranges_overlap(out, out_bytes, ray, 4.0 * (double)T) ||
           ranges_overlap(out, out_bytes, a.extra, 4.0 * (double)a.extra_rows * (double)a.extra_cols);
}

// f(Int<BD>{}) for the basis of `opt`: the SH sizes at compile time, 0 for the lobes of SG / ASG
template <class F>
static void with_basis(const svoxt_options* opt, F&& f) {
    if (opt->format != SVOXT_FORMAT_SH) f(Int<0>{});
    else with_int(SpecialBases{}, (int)opt->basis_dim, [&](auto bd) { f(bd); return true; });
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int svoxt_shade_rot_fwd(const float* features, int64_t M, int32_t K, const svoxt_options* opt, const float* extra, int32_t extra_rows,
                        int32_t extra_cols, const float* rotations, int32_t rot_dim, const float* viewdirs, int64_t Q,
                        const int32_t* row, const int32_t* ray, int64_t T, int32_t activate, float* values, float* sigma, void* stream) {
    const char* fn = "svoxt_shade_rot_fwd";
    int rc, C, bd;
    const RotArgs a{extra, rotations, viewdirs, extra_rows, extra_cols, rot_dim};
    if ((rc = shade_fwd_check(fn, opt, &a, features, M, K, row, ray, T, nullptr, Q, values, sigma, &C, &bd)) || T == 0) return rc;
    const double vb = 4.0 * (double)T * C, sb = 4.0 * (double)T;
    if (rot_out_overlaps(values, vb, features, M, K, a, Q, row, ray, T) || rot_out_overlaps(sigma, sb, features, M, K, a, Q, row, ray, T) ||
        ranges_overlap(values, vb, sigma, sb))
        return fail(SVOXT_ERR_INVALID, "%s: values / sigma overlaps an input or the other output", fn);
    const RotDev R = rot_dev(opt, a, M, Q);
    with_basis(opt, [&](auto BD) {
        using S = RotBasis<decltype(BD)::value>;
        hipLaunchKernelGGL(shade_fwd_kernel<S>, launch_grid(T * (C + 1)), dim3(kLaunchBlock), 0, (hipStream_t)stream, features, M, (int)K, C,
                           (int)opt->min_comp, (int)opt->max_comp, activate != 0, S{R, row, bd}, T, row, ray, values, sigma);
    });
    return check_launch(fn);
}

int svoxt_shade_rot_bwd(const svoxt_options* opt, int64_t M, int32_t K, const float* extra, int32_t extra_rows, int32_t extra_cols,
                        const float* rotations, int32_t rot_dim, const float* viewdirs, int64_t Q, const int32_t* row, const int32_t* ray,
                        int64_t T, int32_t activate, const float* values, const float* grad_values, const float* grad_sigma,
                        const int32_t* row_ptr, const int32_t* perm, const int32_t* long_rows, const int32_t* long_chunk_ptr,
                        const int32_t* chunk_long, int64_t n_long, int64_t n_chunks, float* grad, void* workspace, int64_t workspace_bytes,
                        void* stream) {
    const char* fn = "svoxt_shade_rot_bwd";
    int rc, C, bd;
    const RotArgs a{extra, rotations, viewdirs, extra_rows, extra_cols, rot_dim};
    const RowPlanRef plan{row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, T, M, n_long, n_chunks};
    float* partials;
    if ((rc = shade_bwd_check(fn, opt, &a, plan, K, row, ray, nullptr, Q, activate, values, &grad_values, grad_sigma, grad, workspace, &C,
                              &bd)) || M == 0)
        return rc;
    const double gb = 4.0 * (double)M * K, tc = 4.0 * (double)T * C;
    if (rot_out_overlaps(grad, gb, nullptr, M, K, a, Q, row, ray, T) || ranges_overlap(grad, gb, values, tc) ||
        ranges_overlap(grad, gb, grad_values, tc) || ranges_overlap(grad, gb, grad_sigma, 4.0 * (double)T))
        return fail(SVOXT_ERR_INVALID, "%s: grad overlaps an input", fn);
    if ((rc = shade_partials(fn, plan, K, workspace, workspace_bytes, "svoxt_shade_samples_bwd_workspace_bytes(n_chunks, K)", &partials)))
        return rc;
    const RotDev R = rot_dev(opt, a, M, Q);
    // a lane per (row, column) over all K columns: every element of grad is written
    with_basis(opt, [&](auto BD) {
        using S = RotBasis<decltype(BD)::value>;
        const ShadeValues<S> src{ray, values, grad_values, grad_sigma, S{R, row, bd}, T, (int)K, C, (int)opt->min_comp, (int)opt->max_comp,
                                 activate != 0};
        rows_launch<ROWS_SUM, ROWS_SUM>(src, (int)K, plan, nullptr, (int)K, 0.f, grad, partials, (hipStream_t)stream);
    });
    return check_launch(fn);
}

int svoxt_shade_rot_bwd_dir(const float* features, int64_t M, int32_t K, const svoxt_options* opt, const float* extra, int32_t extra_rows,
                            int32_t extra_cols, const float* rotations, int32_t rot_dim, const float* viewdirs, int64_t Q,
                            const int32_t* row, const int32_t* ray, int64_t T, int32_t activate, const float* values,
                            const float* grad_values, float* gu, void* stream) {
    const char* fn = "svoxt_shade_rot_bwd_dir";
    int rc, C, bd;
    const RotArgs a{extra, rotations, viewdirs, extra_rows, extra_cols, rot_dim};
    if ((rc = shade_dims(opt, M, K, T, Q, &C, &bd, fn)) || (rc = rot_check(fn, opt, a, M, Q))) return rc;
    if (T == 0) return SVOXT_OK;
    if (gu == nullptr || row == nullptr || ray == nullptr) return fail(SVOXT_ERR_INVALID, "%s: gu / row / ray is NULL", fn);
    if (C == 0) grad_values = nullptr;                           // (zeros: nothing is read)
    if (grad_values != nullptr && ((activate != 0 && values == nullptr) || (M > 0 && features == nullptr)))
        return fail(SVOXT_ERR_INVALID, "%s: values / features is NULL", fn);
    if (misaligned(features, 4) || misaligned(row, 4) || misaligned(ray, 4) || misaligned(values, 4) || misaligned(grad_values, 4) ||
        misaligned(gu, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    const double ub = 12.0 * (double)T, tc = 4.0 * (double)T * C;
    if (rot_out_overlaps(gu, ub, features, M, K, a, Q, row, ray, T) || ranges_overlap(gu, ub, values, tc) || ranges_overlap(gu, ub, grad_values, tc))
        return fail(SVOXT_ERR_INVALID, "%s: gu overlaps an input", fn);
    const RotDev R = rot_dev(opt, a, M, Q);
    with_basis(opt, [&](auto BD) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(launch_blocks(T)), dim3(kLaunchBlock), 0, (hipStream_t)stream, features, (int)K, C, bd,
                               (int)opt->min_comp, (int)opt->max_comp, activate != 0, R, T, row, ray, values, grad_values, gu);
        };
        if (C == 3) launch(shade_rot_dir_kernel<decltype(BD)::value, 3>);
        else launch(shade_rot_dir_kernel<decltype(BD)::value, 0>);
    });
    return check_launch(fn);
}

int svoxt_shade_rot_bwd_rotations(const float* gu, const float* viewdirs, int64_t Q, const int32_t* ray, int64_t T, int64_t M,
                                  int32_t rot_dim, const int32_t* row_ptr, const int32_t* perm, const int32_t* long_rows,
                                  const int32_t* long_chunk_ptr, const int32_t* chunk_long, int64_t n_long, int64_t n_chunks,
                                  float* grad_rotations, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_shade_rot_bwd_rotations";
    int rc;
    const RowPlanRef plan{row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, T, M, n_long, n_chunks};
    if ((rc = extent31_check(fn, T, "T")) || (rc = extent31_check(fn, M, "M")) || (rc = extent31_check(fn, Q, "Q"))) return rc;
    if (rot_dim != 3 && rot_dim != 4) return fail(SVOXT_ERR_INVALID, "%s: rot_dim must be 3 or 4", fn);
    if ((rc = row_plan_check(fn, plan))) return rc;
    if (M == 0) return SVOXT_OK;
    if (grad_rotations == nullptr || row_ptr == nullptr) return fail(SVOXT_ERR_INVALID, "%s: grad_rotations / row_ptr is NULL", fn);
    if (T > 0 && (perm == nullptr || gu == nullptr || ray == nullptr || (Q > 0 && viewdirs == nullptr)))
        return fail(SVOXT_ERR_INVALID, "%s: perm / gu / ray / viewdirs is NULL", fn);
    if ((rc = row_plan_long_check(fn, plan))) return rc;
    if (misaligned(gu, 4) || misaligned(viewdirs, 4) || misaligned(ray, 4) || row_plan_misaligned(plan) || misaligned(grad_rotations, 4) ||
        misaligned(workspace, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    const int dd = rot_dim * rot_dim;
    const double gb = 4.0 * (double)M * dd;
    if (ranges_overlap(grad_rotations, gb, gu, 12.0 * (double)T) || ranges_overlap(grad_rotations, gb, viewdirs, 12.0 * (double)Q) ||
        ranges_overlap(grad_rotations, gb, ray, 4.0 * (double)T))
        return fail(SVOXT_ERR_INVALID, "%s: grad_rotations overlaps an input", fn);
    float* partials;
    if ((rc = shade_partials(fn, plan, dd, workspace, workspace_bytes, "svoxt_shade_samples_bwd_workspace_bytes(n_chunks, rot_dim * rot_dim)",
                             &partials)))
        return rc;
    const RotGradValues src{ray, gu, viewdirs, T, Q, (int)rot_dim};
    // a lane per (row, a, b) over all rot_dim^2 columns: every element of grad_rotations is written
    rows_launch<ROWS_SUM, ROWS_SUM>(src, dd, plan, nullptr, dd, 0.f, grad_rotations, partials, (hipStream_t)stream);
    return check_launch(fn);
}

int svoxt_shade_rot_bwd_viewdirs(const float* gu, const float* rotations, int32_t rot_dim, int64_t M, const int64_t* offsets,
                                 const int32_t* row, const int32_t* ray, int64_t T, int64_t Q, float* grad_vdirs, void* stream) {
    const char* fn = "svoxt_shade_rot_bwd_viewdirs";
    int rc;
    if ((rc = extent31_check(fn, T, "T")) || (rc = extent31_check(fn, M, "M")) || (rc = extent31_check(fn, Q, "Q"))) return rc;
    if (rot_dim != 3 && rot_dim != 4) return fail(SVOXT_ERR_INVALID, "%s: rot_dim must be 3 or 4", fn);
    if (Q == 0) return SVOXT_OK;
    if (offsets == nullptr || grad_vdirs == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets / grad_vdirs is NULL", fn);
    if (T > 0 && (gu == nullptr || row == nullptr || ray == nullptr || (M > 0 && rotations == nullptr)))
        return fail(SVOXT_ERR_INVALID, "%s: gu / row / ray / rotations is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(gu, 4) || misaligned(rotations, 4) || misaligned(row, 4) || misaligned(ray, 4) ||
        misaligned(grad_vdirs, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the others: 4)", fn);
    const double ob = 12.0 * (double)Q;
    if (ranges_overlap(grad_vdirs, ob, gu, 12.0 * (double)T) || ranges_overlap(grad_vdirs, ob, rotations, 4.0 * (double)M * rot_dim * rot_dim) ||
        ranges_overlap(grad_vdirs, ob, offsets, 8.0 * (double)(Q + 1)) || ranges_overlap(grad_vdirs, ob, row, 4.0 * (double)T) ||
        ranges_overlap(grad_vdirs, ob, ray, 4.0 * (double)T))
        return fail(SVOXT_ERR_INVALID, "%s: grad_vdirs overlaps an input", fn);
    hipLaunchKernelGGL(shade_rot_vdirs_kernel, dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, rotations, (int)rot_dim, M, Q,
                       T, offsets, row, ray, gu, grad_vdirs);
    return check_launch(fn);
}

}  // extern "C"
