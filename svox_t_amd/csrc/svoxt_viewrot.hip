// svoxt_viewrot.hip -- shade_samples with per-row rotations of the view direction (the reference serves
// transformation_matrices in its render kernels only and has no gradient in them): the colour of every sample of a
// RaySamples list from its feature row and the basis of u = rotations[row] * viewdirs[ray], and the three gradients --
// in the feature table, in the rotations and in the view directions.  No [T, basis_dim] and no [T, K] array, no float
// atomic anywhere; every result has the same bits in every run.
//
//   forward      shade_rot_fwd_kernel<BD>      a lane per (sample, channel) and one per sample behind them for sigma, as
//                                              shade_fwd_kernel; the lane rotates its ray's direction by its row's matrix
//                                              and forms the basis (SH: BD at compile time, in registers; SG / ASG: one
//                                              lobe at a time)
//   features     the row kernels of svoxt_rowwalk.h over ShadeRotValues<BD>: a lane per (row, column) holds the row's matrix
//                (loaded once, at its first sample) and forms (g_values[k, c] * d[k, c]) * B_i(k) on the fly
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

// the lobes of SG / ASG as the basis functions take them: a TreeDev of which nothing else is read
__host__ __device__ __forceinline__ TreeDev lobes_only(const float* extra, int extra_rows, int extra_cols) {
    TreeDev tr{};
    tr.extra = extra;
    tr.extra_rows = extra_rows;
    tr.extra_cols = extra_cols;
    return tr;
}

// the rotated call's view side: rotations float32 [M, d, d] (the upper-left 3 x 3 is read), viewdirs float32 [Q, 3]
struct RotDev {
    const float* __restrict__ rot;
    const float* __restrict__ vdirs;
    const float* __restrict__ extra;
    int64_t M, Q;
    int d, extra_rows, extra_cols, format;
};

// the upper-left 3 x 3 of row idx's matrix, in registers
struct Mat3 {
    float m00, m01, m02, m10, m11, m12, m20, m21, m22;
    __device__ __forceinline__ void load(const float* __restrict__ rot, int64_t idx, int d) {
        const float* __restrict__ m = rot + idx * (d * d);
        m00 = m[0]; m01 = m[1]; m02 = m[2];
        m10 = m[d]; m11 = m[d + 1]; m12 = m[d + 2];
        m20 = m[2 * d]; m21 = m[2 * d + 1]; m22 = m[2 * d + 2];
    }
    // u = m * v, rotated_dir's sequence
    __device__ __forceinline__ void apply(const float* __restrict__ v, float& u0, float& u1, float& u2) const {
        const float v0 = v[0], v1 = v[1], v2 = v[2];
        u0 = m00 * v0 + m01 * v1 + m02 * v2;
        u1 = m10 * v0 + m11 * v1 + m12 * v2;
        u2 = m20 * v0 + m21 * v1 + m22 * v2;
    }
};

// component i of the SH basis of BD values at (x, y, z): precalc_basis<BD> into registers, selected without an index
template <int BD>
__device__ __forceinline__ float sh_component(const TreeDev& tr, float x, float y, float z, int i) {
    float B[BD];
    precalc_basis<BD>(FMT_SH, BD, tr, x, y, z, B);
    float b = 0.f;
#pragma unroll
    for (int I = 0; I < BD; ++I)
        if (i == I) b = B[I];
    return b;
}

// ------------------------------------------------------------------------------------------------------------ forward
// lane t = k * (C + 1) + c.  c < C: values[k, c]; c == C: sigma[k].  BD: the SH basis' size (0: SG / ASG, bd lobes)
template <int BD>
__global__ void __launch_bounds__(kLaunchBlock)
shade_rot_fwd_kernel(const float* __restrict__ features, int K, int C, int bd_rt, int min_comp, int max_comp, bool activate, RotDev R,
                     int64_t T, const int32_t* __restrict__ row, const int32_t* __restrict__ ray, float* __restrict__ values,
                     float* __restrict__ sigma) {
    const int bd = BD > 0 ? BD : bd_rt;
    const int64_t t = launch_lane();
    const int64_t k = t / (C + 1);
    if (k >= T) return;
    const int c = (int)(t - k * (C + 1));
    const int64_t idx = row[k];
    const bool inside = idx >= 0 && idx < R.M;
    const float* __restrict__ frow = features + (inside ? idx : 0) * K;
    if (c == C) {
        sigma[k] = inside ? frow[K - 1] : 0.f;
        return;
    }
    float v = 0.f;
    const int64_t q = ray[k];
    if (inside && q >= 0 && q < R.Q) {                           // (a ray outside [0, Q): zeros, as a row outside [0, M))
        const TreeDev tr = lobes_only(R.extra, R.extra_rows, R.extra_cols);
        Mat3 m;
        m.load(R.rot, idx, R.d);
        float u0, u1, u2;
        m.apply(R.vdirs + 3 * q, u0, u1, u2);
        const float* __restrict__ f = frow + c * bd;
        float tmp = 0.f;
        if constexpr (BD > 0) {
            float B[BD];
            precalc_basis<BD>(FMT_SH, BD, tr, u0, u1, u2, B);
#pragma unroll
            for (int i = 0; i < BD; ++i)
                if (i >= min_comp && i <= max_comp) tmp += B[i] * f[i];
        } else {
            for (int i = min_comp; i <= max_comp; ++i) tmp += lobe_value(R.format, tr, u0, u1, u2, i, bd) * f[i];
        }
        v = shade_value(tmp, activate);
    }
    values[k * C + c] = v;
}

// ------------------------------------------------------------------------------------------------------------- values
// The contribution of sample k to column j of its row, for the row kernels of svoxt_rowwalk.h, beside ShadeValues: the
// basis value is recomputed from the row's matrix and the ray's direction by the forward's sequence.  All samples a lane
// walks name one row: the lane loads that row's matrix at its first sample and keeps it.  A NULL upstream gradient is
// zeros: its columns are ZERO columns, nothing is read.
template <int BD>
struct ShadeRotValues {
    const int32_t* __restrict__ row;
    const int32_t* __restrict__ ray;
    const float* __restrict__ values;
    const float* __restrict__ gv;
    const float* __restrict__ gs;
    RotDev R;
    int64_t T;
    int K, C, bd, min_comp, max_comp;
    bool activate;
    enum { ZERO, SIGMA, BASIS, BASIS_LINEAR };
    struct Col {
        const int32_t* __restrict__ row;
        const int32_t* __restrict__ ray;
        const float* __restrict__ v;       // BASIS: values + c
        const float* __restrict__ g;       // SIGMA: g_sigma;  the colour modes: g_values + c
        RotDev R;
        int64_t T;
        int mode, C, bd, i;
        mutable Mat3 m;
        mutable bool have;
        __device__ __forceinline__ float at(int64_t k) const {
            if (mode == ZERO || k < 0 || k >= T) return 0.f;
            if (mode == SIGMA) return g[k];
            const float gc = g[k * C];
            const int64_t q = ray[k];
            if (q < 0 || q >= R.Q) return 0.f;                   // (the forward gave this sample zeros)
            if (!have) {
                const int64_t idx = row[k];
                if (idx < 0 || idx >= R.M) return 0.f;           // (a plan names no such sample)
                m.load(R.rot, idx, R.d);
                have = true;
            }
            float u0, u1, u2;
            m.apply(R.vdirs + 3 * q, u0, u1, u2);
            const TreeDev tr = lobes_only(R.extra, R.extra_rows, R.extra_cols);
            float b;
            if constexpr (BD > 0) b = sh_component<BD>(tr, u0, u1, u2, i);
            else b = lobe_value(R.format, tr, u0, u1, u2, i, bd);
            if (mode == BASIS_LINEAR) return gc * b;
            const float sig = v[k * C];
            const float d = (float)((double)sig * (1.0 - (double)sig));
            return (gc * d) * b;
        }
    };
    __device__ __forceinline__ Col col(int j) const {
        Col o{row, ray, values, gs, R, T, ZERO, C, bd, 0, Mat3{}, false};
        if (j == K - 1) {
            if (gs != nullptr) o.mode = SIGMA;
        } else if (gv != nullptr && j < C * bd) {
            const int c = j / bd, i = j - c * bd;
            if (i >= min_comp && i <= max_comp) {
                o.mode = activate ? BASIS : BASIS_LINEAR;
                o.v = values + c; o.g = gv + c; o.i = i;
            }
        }
        return o;
    }
};

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
        auto bracket = [&](int c) {
            float t = g[c];
            if (activate) {
                const float sig = v[c];
                t = t * (float)((double)sig * (1.0 - (double)sig));
            }
            return t;
        };
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

// what the rotated call is given, as the entry points check it: a format with a basis, its lobes, the matrices, the directions
struct RotArgs {
    const float *extra, *rotations, *viewdirs;
    int32_t extra_rows, extra_cols, rot_dim;
};
static int rot_check(const char* fn, const svoxt_options* opt, const RotArgs& a, int64_t M, int64_t Q) {
    if (opt->format == SVOXT_FORMAT_RGBA)
        return fail(SVOXT_ERR_INVALID, "%s: RGBA has no basis to rotate (svoxt_shade_samples_* serve it)", fn);
    if (opt->format == SVOXT_FORMAT_SH && !special_basis(opt->basis_dim))
        return fail(SVOXT_ERR_INVALID, "%s: SH basis_dim must be 1, 4, 9, 16 or 25", fn);
    if (opt->format == SVOXT_FORMAT_SG || opt->format == SVOXT_FORMAT_ASG) {
        const int need = opt->format == SVOXT_FORMAT_SG ? 4 : 11;
        if (a.extra == nullptr || a.extra_rows < opt->basis_dim || a.extra_cols < need)
            return fail(SVOXT_ERR_INVALID, "%s: SG/ASG formats need extra [basis_dim, >=4/11]", fn);
    }
    if (a.rot_dim != 3 && a.rot_dim != 4) return fail(SVOXT_ERR_INVALID, "%s: rot_dim must be 3 or 4", fn);
    if ((M > 0 && a.rotations == nullptr) || (Q > 0 && a.viewdirs == nullptr))
        return fail(SVOXT_ERR_INVALID, "%s: rotations / viewdirs is NULL", fn);
    if (misaligned(a.extra, 4) || misaligned(a.rotations, 4) || misaligned(a.viewdirs, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    return SVOXT_OK;
}
static RotDev rot_dev(const svoxt_options* opt, const RotArgs& a, int64_t M, int64_t Q) {
    return RotDev{a.rotations, a.viewdirs, a.extra, M, Q, (int)a.rot_dim, (int)a.extra_rows, (int)a.extra_cols, (int)opt->format};
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
    if ((rc = shade_dims(opt, M, K, T, Q, &C, &bd, fn)) || (rc = rot_check(fn, opt, a, M, Q))) return rc;
    if (T == 0) return SVOXT_OK;
    if (row == nullptr || sigma == nullptr || (C > 0 && (values == nullptr || ray == nullptr)))
        return fail(SVOXT_ERR_INVALID, "%s: row / ray / values / sigma is NULL", fn);
    if (M > 0 && features == nullptr) return fail(SVOXT_ERR_INVALID, "%s: features is NULL", fn);
    if (misaligned(features, 4) || misaligned(row, 4) || misaligned(ray, 4) || misaligned(values, 4) || misaligned(sigma, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    const double vb = 4.0 * (double)T * C, sb = 4.0 * (double)T;
    if (rot_out_overlaps(values, vb, features, M, K, a, Q, row, ray, T) || rot_out_overlaps(sigma, sb, features, M, K, a, Q, row, ray, T) ||
        ranges_overlap(values, vb, sigma, sb))
        return fail(SVOXT_ERR_INVALID, "%s: values / sigma overlaps an input or the other output", fn);
    const RotDev R = rot_dev(opt, a, M, Q);
    with_basis(opt, [&](auto BD) {
        hipLaunchKernelGGL((shade_rot_fwd_kernel<decltype(BD)::value>), launch_grid(T * (C + 1)), dim3(kLaunchBlock), 0, (hipStream_t)stream,
                           features, (int)K, C, bd, (int)opt->min_comp, (int)opt->max_comp, activate != 0, R, T, row, ray, values, sigma);
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
    if ((rc = shade_dims(opt, M, K, T, Q, &C, &bd, fn)) || (rc = rot_check(fn, opt, a, M, Q)) || (rc = row_plan_check(fn, plan))) return rc;
    if (M == 0) return SVOXT_OK;
    if (grad == nullptr || row_ptr == nullptr) return fail(SVOXT_ERR_INVALID, "%s: grad / row_ptr is NULL", fn);
    if (C == 0) grad_values = nullptr;                           // (no colour column: nothing of it is read)
    if (T > 0 && (perm == nullptr || (grad_values != nullptr && (row == nullptr || ray == nullptr || (activate != 0 && values == nullptr)))))
        return fail(SVOXT_ERR_INVALID, "%s: perm / row / ray / values is NULL", fn);
    if ((rc = row_plan_long_check(fn, plan))) return rc;
    if (misaligned(row, 4) || misaligned(ray, 4) || misaligned(values, 4) || misaligned(grad_values, 4) || misaligned(grad_sigma, 4) ||
        row_plan_misaligned(plan) || misaligned(grad, 4) || misaligned(workspace, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    const double gb = 4.0 * (double)M * K, tc = 4.0 * (double)T * C;
    if (rot_out_overlaps(grad, gb, nullptr, M, K, a, Q, row, ray, T) || ranges_overlap(grad, gb, values, tc) ||
        ranges_overlap(grad, gb, grad_values, tc) || ranges_overlap(grad, gb, grad_sigma, 4.0 * (double)T))
        return fail(SVOXT_ERR_INVALID, "%s: grad overlaps an input", fn);
    if (n_long > 0 && (rc = workspace_check(fn, workspace, workspace_bytes, svoxt_shade_samples_bwd_workspace_bytes(n_chunks, K),
                                            "svoxt_shade_samples_bwd_workspace_bytes(n_chunks, K)")))
        return rc;
    Carver w(workspace);
    float* partials = w.take<float>((size_t)n_chunks * (size_t)K);
    const RotDev R = rot_dev(opt, a, M, Q);
    // a lane per (row, column) over all K columns: every element of grad is written
    with_basis(opt, [&](auto BD) {
        const ShadeRotValues<decltype(BD)::value> src{row, ray, values, grad_values, grad_sigma, R, T, (int)K, C, bd, (int)opt->min_comp,
                                                      (int)opt->max_comp, activate != 0};
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
    if (n_long > 0 && (rc = workspace_check(fn, workspace, workspace_bytes, svoxt_shade_samples_bwd_workspace_bytes(n_chunks, dd),
                                            "svoxt_shade_samples_bwd_workspace_bytes(n_chunks, rot_dim * rot_dim)")))
        return rc;
    Carver w(workspace);
    float* partials = w.take<float>((size_t)n_chunks * (size_t)dd);
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
