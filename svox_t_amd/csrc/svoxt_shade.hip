// svoxt_shade.hip -- shade_samples (not in the reference): the colour of every sample of a RaySamples
// list from its feature row and its ray's basis values, and the gradient with respect to the feature table summed per
// table entry over the row plan in svoxt_reduce_rows' order -- no [T, K] array and no float atomic anywhere.
//
//   view_basis   view_basis_kernel        a lane per ray, no march: precalc_basis<0> of load_vdir into basis[q, :]
// The shading core is svoxt_shade.h's, shared with svoxt_viewrot.hip; here it runs over the basis source TableBasis, the
// per-ray table basis[ray[k], i] (bd at run time, 0 for RGBA).
//   forward      shade_fwd_kernel<TableBasis>  a lane per (sample, channel) and one per sample behind them for sigma
//                shade_fwd_rgba4_kernel   RGBA rows of K = 4 K4 floats in a 16-byte aligned table: a lane per (sample,
//                                         four columns), one 16-byte load each (gather_rows4_kernel's cut)
//   backward     the row kernels of svoxt_rowwalk.h, a lane per (row, column) over all K columns, the value of sample k
//                at column j formed on the fly (ShadeValues<TableBasis>): a colour column (g_values[k, c] * d[k, c]) *
//                basis[ray[k], i], the sigma column g_sigma[k], every other column 0.f.  sig is the forward's own output.
//   view gradient
//                view_basis_bwd_kernel    a lane per ray: the analytic derivative of precalc_basis' expression, summed over
//                                         the components in ascending order into grad_viewdirs[q, 0:3] (view_basis_grad,
//                                         svoxt_shade.h: svoxt_viewrot.hip calls the same body per sample)
//                shade_bwd_basis_kernel   basis_dim lanes a ray over its segment in list order: grad_basis[q, i], the sum of
//                                         (g_values[k, c] * d[k, c]) * features[row[k], c * bd + i]; whole rays a workgroup
// Per sample 4 * (C + 1) bytes out of the forward; the backward keeps values, basis and ray (and the table's pointer where
// the basis requires grad).  C ABI: svoxt_view_basis, svoxt_view_basis_bwd, svoxt_shade_samples_* (include/svoxt.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_device.h"
#include "svoxt_host.h"
#include "svoxt_rowwalk.h"
#include "svoxt_shade.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

// --------------------------------------------------------------------------------------------------------- view_basis
// lane q: the basis values the render kernels form for ray q (every component, whatever the component range)
__global__ void __launch_bounds__(kLaunchBlock)
view_basis_kernel(TreeDev tr, RaysDev rays, int format, int bd, float* __restrict__ basis) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (q >= rays.Q) return;
    float vd[3];
    load_vdir(rays, q, vd);
    precalc_basis<0>(format, bd, tr, vd[0], vd[1], vd[2], basis + q * bd);
}

// lane q: grad_vdirs[q, :] = view_basis_grad (svoxt_shade.h) at the ray's direction as given, grad_basis[q, i] read at
// compile-time indices guarded by bd, the lobes of SG / ASG one at a time from memory, SG's basis value the forward's own
// output: no private array, nothing in scratch.
__global__ void __launch_bounds__(kLaunchBlock)
view_basis_bwd_kernel(TreeDev tr, RaysDev rays, int format, int bd, const float* __restrict__ basis,
                      const float* __restrict__ grad_basis, float* __restrict__ grad_vdirs) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (q >= rays.Q) return;
    float vd[3];
    load_vdir(rays, q, vd);
    const float* __restrict__ gb = grad_basis + q * bd;
    float gx, gy, gz;
    view_basis_grad(tr, format, bd, vd[0], vd[1], vd[2], [gb](int i) { return gb[i]; }, [basis, q, bd](int i) { return basis[q * bd + i]; },
                    gx, gy, gz);
    float* __restrict__ o = grad_vdirs + 3 * q;
    o[0] = gx; o[1] = gy; o[2] = gz;
}

// ------------------------------------------------------------------------------------------------------------ forward
// lane t = k * K4 + j: columns 4 j .. 4 j + 3 of sample k's RGBA row (K = 4 K4, C = K - 1, the table 16-byte aligned);
// the last column of the last lane is sigma
__global__ void __launch_bounds__(kLaunchBlock)
shade_fwd_rgba4_kernel(const float4* __restrict__ features, int64_t M, int K4, bool activate, int64_t T,
                       const int32_t* __restrict__ row, float* __restrict__ values, float* __restrict__ sigma) {
    const int64_t t = launch_lane();
    const int64_t k = t / K4;
    if (k >= T) return;
    const int j = (int)(t - k * K4);
    const int64_t idx = row[k];
    const bool inside = idx >= 0 && idx < M;
    const int C = 4 * K4 - 1;
    const float4 x = inside ? features[idx * K4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
    float* __restrict__ o = values + k * C + 4 * j;
    o[0] = inside ? shade_value(x.x, activate) : 0.f;
    o[1] = inside ? shade_value(x.y, activate) : 0.f;
    o[2] = inside ? shade_value(x.z, activate) : 0.f;
    if (j == K4 - 1) sigma[k] = x.w;
    else o[3] = inside ? shade_value(x.w, activate) : 0.f;
}

// ----------------------------------------------------------------------------------------------------- backward, basis
// grad_basis[q, i] = the sum over ray q's segment in list order, and per sample over c ascending, of
// (grad_values[k, c] * d[k, c]) * features[row[k], c * bd + i] -- the table backward's factor (shade_bracket) times the coefficient the
// forward multiplied basis[q, i] by.  bd lanes a ray walk the segment together: lane i reads frow[c * bd + i], so a
// ray's lanes read neighbouring floats of one row and the same grad_values / values words.  A block holds
// kLaunchBlock / bd whole rays (its last kLaunchBlock % bd lanes idle): no ray's lanes straddle two blocks.  One
// accumulator a lane; CS: C at compile time (0: the run-time loop).
template <int CS>
__global__ void __launch_bounds__(kLaunchBlock)
shade_bwd_basis_kernel(const float* __restrict__ features, int64_t M, int K, int C_rt, int bd, int min_comp, int max_comp,
                       bool activate, int64_t Q, int64_t T, const int64_t* __restrict__ offsets, const int32_t* __restrict__ row,
                       const int32_t* __restrict__ ray, const float* __restrict__ values, const float* __restrict__ gv,
                       float* __restrict__ grad_basis) {
    const int C = CS > 0 ? CS : C_rt;
    const int rays_per_block = kLaunchBlock / bd;
    const int r = (int)threadIdx.x / bd, i = (int)threadIdx.x - r * bd;
    const int64_t q = (int64_t)blockIdx.x * rays_per_block + r;
    if (r >= rays_per_block || q >= Q) return;
    float acc = 0.f;
    if (gv != nullptr && i >= min_comp && i <= max_comp) {
        const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
        for (int64_t k = b; k < e; ++k) {
            const int64_t idx = row[k];
            if (ray[k] != q || idx < 0 || idx >= M) continue;
            const float* __restrict__ f = features + idx * K + i;
            const float* __restrict__ g = gv + k * C;
            const float* __restrict__ v = values + k * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc += shade_bracket(g[c], v + c, activate) * f[c * bd];
        }
    }
    grad_basis[q * bd + i] = acc;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int svoxt_view_basis(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, float* basis, void* stream) {
    const char* fn = "svoxt_view_basis";
    int rc;
    if ((rc = check_tree(tree, fn)) || (rc = check_rays(rays, fn)) || (rc = check_opts(opt, tree, fn, true))) return rc;
    if (tree->xform != nullptr) return fail(SVOXT_ERR_INVALID, "%s: transformation_matrices (tree.xform) are not served by shade_samples", fn);
    if (rays->Q > 0x7fffffffLL) return fail(SVOXT_ERR_INVALID, "%s: too many rays (ray indices are int32)", fn);
    if (opt->format == SVOXT_FORMAT_RGBA || rays->Q == 0) return SVOXT_OK;     // [Q, 0]: nothing to write
    if (basis == nullptr || misaligned(basis, 4)) return fail(SVOXT_ERR_INVALID, "%s: basis is NULL or not 4-byte aligned", fn);
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree);
    hipLaunchKernelGGL(view_basis_kernel, dim3(launch_blocks(rays->Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, tr, rd, (int)opt->format,
                       (int)opt->basis_dim, basis);
    return check_launch(fn);
}

int svoxt_view_basis_bwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* basis,
                         const float* grad_basis, float* grad_vdirs, void* stream) {
    const char* fn = "svoxt_view_basis_bwd";
    int rc;
    if ((rc = check_tree(tree, fn)) || (rc = check_rays(rays, fn)) || (rc = check_opts(opt, tree, fn, true))) return rc;
    if (rays->c2w != nullptr) return fail(SVOXT_ERR_INVALID, "%s: camera mode has no viewdirs tensor to receive a gradient (rays.c2w must be NULL)", fn);
    if (tree->xform != nullptr) return fail(SVOXT_ERR_INVALID, "%s: transformation_matrices (tree.xform) are not served by shade_samples", fn);
    if (rays->Q > 0x7fffffffLL) return fail(SVOXT_ERR_INVALID, "%s: too many rays (ray indices are int32)", fn);
    if (opt->format == SVOXT_FORMAT_RGBA || rays->Q == 0) return SVOXT_OK;     // [Q, 0]: no basis, no gradient
    if (grad_basis == nullptr || grad_vdirs == nullptr || (opt->format == SVOXT_FORMAT_SG && basis == nullptr))
        return fail(SVOXT_ERR_INVALID, "%s: grad_basis / grad_vdirs / basis (SG) is NULL", fn);
    if (misaligned(basis, 4) || misaligned(grad_basis, 4) || misaligned(grad_vdirs, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree);
    hipLaunchKernelGGL(view_basis_bwd_kernel, dim3(launch_blocks(rays->Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, tr, rd,
                       (int)opt->format, (int)opt->basis_dim, basis, grad_basis, grad_vdirs);
    return check_launch(fn);
}

int svoxt_shade_samples_bwd_basis(const float* features, int64_t M, int32_t K, const svoxt_options* opt, const int64_t* offsets,
                                  const int32_t* row, const int32_t* ray, int64_t T, int64_t Q, int32_t activate,
                                  const float* values, const float* grad_values, float* grad_basis, void* stream) {
    const char* fn = "svoxt_shade_samples_bwd_basis";
    int rc, C, bd;
    if ((rc = shade_dims(opt, M, K, T, Q, &C, &bd, fn))) return rc;
    if (bd == 0 || Q == 0) return SVOXT_OK;                      // RGBA: no basis, no gradient
    if (offsets == nullptr || grad_basis == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets / grad_basis is NULL", fn);
    if (C == 0 || T == 0) grad_values = nullptr;                 // (zeros: nothing is read)
    if (grad_values != nullptr &&
        (row == nullptr || ray == nullptr || (activate != 0 && values == nullptr) || (M > 0 && features == nullptr)))
        return fail(SVOXT_ERR_INVALID, "%s: row / ray / values / features is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(features, 4) || misaligned(row, 4) || misaligned(ray, 4) || misaligned(values, 4) ||
        misaligned(grad_values, 4) || misaligned(grad_basis, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the others: 4)", fn);
    const int rays_per_block = kLaunchBlock / bd;
    const dim3 grid((unsigned)((Q + rays_per_block - 1) / rays_per_block));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kLaunchBlock), 0, (hipStream_t)stream, features, M, (int)K, C, bd, (int)opt->min_comp,
                           (int)opt->max_comp, activate != 0, Q, T, offsets, row, ray, values, grad_values, grad_basis);
    };
    if (C == 3) launch(shade_bwd_basis_kernel<3>);
    else launch(shade_bwd_basis_kernel<0>);
    return check_launch(fn);
}

int svoxt_shade_samples_fwd(const float* features, int64_t M, int32_t K, const svoxt_options* opt, const int32_t* row,
                            const int32_t* ray, int64_t T, const float* basis, int64_t Q, int32_t activate, float* values,
                            float* sigma, void* stream) {
    const char* fn = "svoxt_shade_samples_fwd";
    int rc, C, bd;
    if ((rc = shade_fwd_check(fn, opt, nullptr, features, M, K, row, ray, T, basis, Q, values, sigma, &C, &bd)) || T == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (bd == 0 && K % 4 == 0 && !misaligned(features, 16)) {
        const int K4 = K / 4;
        hipLaunchKernelGGL(shade_fwd_rgba4_kernel, launch_grid(T * K4), dim3(kLaunchBlock), 0, st,
                           reinterpret_cast<const float4*>(features), M, K4, activate != 0, T, row, values, sigma);
    } else {
        hipLaunchKernelGGL(shade_fwd_kernel<TableBasis>, launch_grid(T * (C + 1)), dim3(kLaunchBlock), 0, st, features, M, (int)K, C,
                           (int)opt->min_comp, (int)opt->max_comp, activate != 0, TableBasis{basis, Q, bd}, T, row, ray, values, sigma);
    }
    return check_launch(fn);
}

int64_t svoxt_shade_samples_bwd_workspace_bytes(int64_t n_chunks, int32_t K) {
    if (!in31(n_chunks) || K < 1 || !elems_fit((double)n_chunks, K)) return -1;
    if (n_chunks == 0) return 0;
    Carver w(nullptr);
    w.take<float>((size_t)n_chunks * (size_t)K);
    return (int64_t)w.bytes();
}

int svoxt_shade_samples_bwd(const svoxt_options* opt, int64_t M, int32_t K, const int32_t* ray, int64_t T, const float* basis,
                            int64_t Q, int32_t activate, const float* values, const float* grad_values,
                            const float* grad_sigma, const int32_t* row_ptr, const int32_t* perm, const int32_t* long_rows,
                            const int32_t* long_chunk_ptr, const int32_t* chunk_long, int64_t n_long, int64_t n_chunks,
                            float* grad, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_shade_samples_bwd";
    int rc, C, bd;
    const RowPlanRef plan{row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, T, M, n_long, n_chunks};
    float* partials;
    if ((rc = shade_bwd_check(fn, opt, nullptr, plan, K, nullptr, ray, basis, Q, activate, values, &grad_values, grad_sigma, grad, workspace,
                              &C, &bd)) || M == 0)
        return rc;
    if ((rc = shade_partials(fn, plan, K, workspace, workspace_bytes, "svoxt_shade_samples_bwd_workspace_bytes(n_chunks, K)", &partials)))
        return rc;
    const ShadeValues<TableBasis> src{ray, values, grad_values, grad_sigma, TableBasis{basis, Q, bd}, T, (int)K, C, (int)opt->min_comp,
                                      (int)opt->max_comp, activate != 0};
    // a lane per (row, column) over all K columns: every element of grad is written
    rows_launch<ROWS_SUM, ROWS_SUM>(src, (int)K, plan, nullptr, (int)K, 0.f, grad, partials, (hipStream_t)stream);
    return check_launch(fn);
}

}  // extern "C"
