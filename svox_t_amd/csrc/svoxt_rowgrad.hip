// svoxt_rowgrad.hip -- the deterministic render backward (not in the reference): the gradient of
// volume_render / opacity_render with respect to the feature table, every sample's contribution formed with the
// arithmetic of render_bwd_generic_kernel (the reference's trace_ray_backward, rt_kernel.cu:331-496), operation for
// operation, and summed per table entry over the row plan in svoxt_reduce_rows' order -- no float atomic anywhere.
//
//   count     svoxt_ray_samples_count with min_sigma = 0: the crossings with sigma > 0.f, as CSR offsets in ray-index order
//   emit      rowgrad_record_kernel   a lane per ray on the shared march: row, ray and delta_t at offsets[q] + k, the
//                                     ray's basis values and delta_scale once
//   plan      svoxt_row_plan_build over the emitted rows (its one host read: the info record)
//   sweep     rowgrad_shade_kernel    a lane per (sample, channel): e = pexpf(-sum_i basis[i] * row[off + i]) (RGBA:
//                                     pexpf(-row[j])); the lane behind a sample's channels: att = pexpf(-delta_t * sigma *
//                                     delta_scale).  The row reads of a sample's lanes fall into the same cache lines.
//             rowgrad_totals_kernel   a lane per sample over its channels in order: total_color as pass 1 sums it (float)
//                                     and as pass 2 does (through double), and gsig (RGBA: sig) in the place of e.  The
//                                     two totals go where `row` was (the plan is built, the rows are shaded) and into a
//                                     sort buffer of the plan's workspace that its build has left free.
//             rowgrad_sweep_kernel    a lane per ray over its list, the generic kernel's two passes over four floats a
//                                     sample: pass 1 forms accum and the ray's final light, pass 2 leaves per sample the
//                                     weight and the sigma contribution in the places of delta_t and att
//   reduce    svoxt_row_plan_long and the row kernels of svoxt_rowwalk.h, a lane per (row, column), the value of sample k
//             at column j formed on the fly (GradValues): a colour column weight[k] * basis[ray[k], i] * gsig[k, c] *
//             g[ray[k], c] (RGBA: weight[k] * sig * (1.f - sig) * g[ray[k], j]), the sigma column the stored contribution,
//             every other column 0.f.  No [T, K] array exists at any point.
// Per sample 4 * (C + 4) bytes (row, ray, weight, sigma contribution, C channel values) and the plan's perm; per ray
// basis_dim + 1 floats.  C ABI: svoxt_render_grad_rows_* (include/svoxt.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_device.h"
#include "svoxt_host.h"
#include "svoxt_rowwalk.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

// workspace: per ray [basis f32[Q * bd]] [dscale f32[Q]]; per sample [row] [ray] [wgt] [sigc] [chan f32[T * C]]; the plan
// [perm] [row_ptr i32[M + 1]] [long_rows] [long_chunk_ptr] [chunk_long] [partials f32[chunks * K]] and svoxt_row_plan_build's
// own workspace.  The long rows' pieces are sized by their bounds (T / 257 long rows, T / 256 + T / 257 chunks).
struct RowGradSpace {
    float *basis, *dscale;
    int32_t *row, *ray;
    float *wgt, *sigc, *chan;
    int32_t *perm, *row_ptr, *long_rows, *long_chunk_ptr, *chunk_long;
    float* partials;
    void* plan;
    int64_t plan_bytes, n_long_max, n_chunks_max;
    size_t bytes;
};
static RowGradSpace rowgrad_carve(void* workspace, int64_t Q, int64_t T, int64_t M, int K, int C, int bd) {
    RowGradSpace sp;
    Carver w(workspace);
    sp.n_long_max = T / (kRowChunk + 1);
    sp.n_chunks_max = T / kRowChunk + sp.n_long_max;
    sp.basis = w.take<float>((size_t)Q * (size_t)bd);
    sp.dscale = w.take<float>((size_t)Q);
    sp.row = w.take<int32_t>((size_t)T);
    sp.ray = w.take<int32_t>((size_t)T);
    sp.wgt = w.take<float>((size_t)T);
    sp.sigc = w.take<float>((size_t)T);
    sp.chan = w.take<float>((size_t)T * (size_t)C);
    sp.perm = w.take<int32_t>((size_t)T);
    sp.row_ptr = w.take<int32_t>((size_t)M + 1);
    sp.long_rows = w.take<int32_t>((size_t)sp.n_long_max);
    sp.long_chunk_ptr = w.take<int32_t>((size_t)sp.n_long_max + 1);
    sp.chunk_long = w.take<int32_t>((size_t)sp.n_chunks_max);
    sp.partials = w.take<float>((size_t)sp.n_chunks_max * (size_t)K);
    sp.plan_bytes = svoxt_row_plan_workspace_bytes(T, M);
    sp.plan = w.take<char>((size_t)sp.plan_bytes);
    sp.bytes = w.bytes();
    return sp;
}

// ------------------------------------------------------------------------------------------------------------- record
// The samples of walk_samples (svoxt_device.h) with min_sigma = 0, in march order: the walk svoxt_ray_samples_count
// counted them with, so the two cannot disagree.
template <bool N2>
__global__ void __launch_bounds__(kBlock)
rowgrad_record_kernel(TreeDev tr, RaysDev rays, Opts opt, int bd, const int64_t* __restrict__ offsets, int64_t T,
                      int32_t* __restrict__ row, int32_t* __restrict__ ray, float* __restrict__ dt, float* __restrict__ basis,
                      float* __restrict__ dscale) {
    const int64_t q = ray_of_thread(rays, (int64_t)blockIdx.x * kBlock + threadIdx.x);
    if (q >= rays.Q) return;
    Ray r;
    if (!setup_ray(tr, rays, opt, q, r)) return;                 // (no sample: nothing reads this ray's basis or scale)
    int64_t at = offsets[q];
    const int64_t end = min(offsets[q + 1], T);
    if (at < 0 || at >= end) return;
    dscale[q] = r.delta_scale;
    if (bd > 0) {
        float vd[3];
        load_vdir(rays, q, vd);
        precalc_basis<0>(opt.format, bd, tr, vd[0], vd[1], vd[2], basis + q * bd);
    }
    walk_samples<N2>(tr, r, opt.step_size, r.tmin, 0.f, [&](const Sample& s, float, float) {
        if (at < end) {
            row[at] = s.idx;
            ray[at] = (int32_t)q;
            dt[at] = s.delta_t;
            ++at;
        }
        return true;
    });
}

// -------------------------------------------------------------------------------------------------------------- shade
// lane t = k * (C + 1) + c.  c < C: chan[k, c] = e of channel c; c == C: att[k]
__global__ void __launch_bounds__(kLaunchBlock)
rowgrad_shade_kernel(const float* __restrict__ features, int64_t M, int K, Opts opt, int C, int bd, int64_t Q, int64_t T,
                     const int32_t* __restrict__ row, const int32_t* __restrict__ ray, const float* __restrict__ dt,
                     const float* __restrict__ basis, const float* __restrict__ dscale, float* __restrict__ att,
                     float* __restrict__ chan) {
    const int64_t t = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    const int64_t k = t / (C + 1);
    if (k >= T) return;
    const int c = (int)(t - k * (C + 1));
    const int64_t idx = row[k], q = ray[k];
    if (idx < 0 || idx >= M || q < 0 || q >= Q) return;          // (the record kernel wrote both in range)
    const float* __restrict__ frow = features + idx * K;
    if (c == C) {
        att[k] = pexpf(-dt[k] * frow[K - 1] * dscale[q]);
        return;
    }
    float x;
    if (opt.format != FMT_RGBA) {
        const float* __restrict__ b = basis + q * bd;
        const int off = c * bd;
        float tmp = 0.f;
        for (int i = opt.min_comp; i <= opt.max_comp; ++i) tmp += b[i] * frow[off + i];
        x = tmp;
    } else {
        x = frow[c];
    }
    chan[k * C + c] = pexpf(-x);
}

// ------------------------------------------------------------------------------------------------------------- totals
// A lane per sample over its channels in ascending order; in: chan = e.  out: chan = gsig (RGBA: sig), tc1 / tc2 = the
// sample's total_color as the reference's pass 1 / pass 2 forms it.
__global__ void __launch_bounds__(kLaunchBlock)
rowgrad_totals_kernel(Opts opt, int C, int64_t Q, int64_t T, const int32_t* __restrict__ ray, const float* __restrict__ grad_out,
                      float* __restrict__ chan, float* __restrict__ tc1, float* __restrict__ tc2) {
    const int64_t k = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (k >= T) return;
    const int64_t q = ray[k];
    if (q < 0 || q >= Q) return;                                 // (the record kernel's own index: never)
    const float* __restrict__ g = grad_out + q * (C + 1);
    float* __restrict__ ch = chan + k * C;
    const bool rgba = opt.format == FMT_RGBA;
    float t1 = 0.f, t2 = 0.f;
    for (int c = 0; c < C; ++c) {
        const double d = 1.0 / (1.0 + (double)ch[c]);
        const float sig = (float)d;
        t1 += sig * g[c];
        t2 = (float)((double)t2 + d * (double)g[c]);
        ch[c] = rgba ? sig : (float)((double)sig * (1.0 - (double)sig));
    }
    tc1[k] = t1;
    tc2[k] = t2;
}

// -------------------------------------------------------------------------------------------------------------- sweep
// A lane per ray over its list; in: wgt = delta_t, sigc = att.  out: wgt = weight, sigc = the sigma contribution.
__global__ void __launch_bounds__(kBlock)
rowgrad_sweep_kernel(Opts opt, int C, const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ grad_out,
                     const float* __restrict__ dscale, const float* __restrict__ tc1, const float* __restrict__ tc2,
                     float* __restrict__ wgt, float* __restrict__ sigc) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= Q) return;
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    if (b >= e) return;
    const float* __restrict__ g = grad_out + q * (C + 1);
    const float delta_scale = dscale[q];
    float accum = 0.f;
    float light_ray;
    {   // pass 1
        float light = 1.f;
        for (int64_t k = b; k < e; ++k) {
            const float att = sigc[k];
            const float weight = light * (1.f - att);
            const float total_color = tc1[k];
            light *= att;
            accum += weight * total_color;
        }
        float total_grad = 0.f;
        for (int j = 0; j < C; ++j) total_grad += g[j];
        accum += light * opt.background_brightness * total_grad;
        light_ray = light;
    }
    {   // pass 2
        float light = 1.f;
        for (int64_t k = b; k < e; ++k) {
            const float total_color = tc2[k];
            const float att = sigc[k];
            const float delta_t = wgt[k];
            const float weight = light * (1.f - att);
            light *= att;
            accum -= weight * total_color;
            const float toadd = delta_t * delta_scale * (total_color * light - accum)
                              + delta_t * delta_scale * g[C] * light_ray;
            wgt[k] = weight;
            sigc[k] = toadd;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- values
// The contribution of sample k to column j of its row, for the row kernels of svoxt_rowwalk.h.
struct GradValues {
    const int32_t* __restrict__ ray;
    const float* __restrict__ wgt;
    const float* __restrict__ sigc;
    const float* __restrict__ chan;
    const float* __restrict__ basis;
    const float* __restrict__ g;
    int64_t T, Q;
    int K, C, bd, min_comp, max_comp;
    bool rgba;
    enum { ZERO, SIGMA, BASIS, RGBA };
    struct Col {
        const int32_t* __restrict__ ray;
        const float* __restrict__ wgt;
        const float* __restrict__ v;       // SIGMA: sigc;  BASIS / RGBA: chan + c
        const float* __restrict__ b;       // BASIS: basis + i
        const float* __restrict__ g;       // grad_out + c
        int64_t T, Q;
        int mode, C, bd;
        __device__ __forceinline__ float at(int64_t k) const {
            if (mode == ZERO || k < 0 || k >= T) return 0.f;
            if (mode == SIGMA) return v[k];
            const int64_t q = ray[k];
            if (q < 0 || q >= Q) return 0.f;                     // (the record kernel's own index: never)
            const float gc = g[q * (C + 1)];
            if (mode == BASIS) return wgt[k] * b[q * bd] * v[k * C] * gc;
            const float sig = v[k * C];
            return wgt[k] * sig * (1.f - sig) * gc;
        }
    };
    __device__ __forceinline__ Col col(int j) const {
        Col o{ray, wgt, sigc, basis, g, T, Q, ZERO, C, bd};
        if (j == K - 1) {
            o.mode = SIGMA;
        } else if (rgba) {
            if (j < C) { o.mode = RGBA; o.v = chan + j; o.g = g + j; }
        } else if (C > 0 && j < C * bd) {
            const int c = j / bd, i = j - c * bd;
            if (i >= min_comp && i <= max_comp) { o.mode = BASIS; o.v = chan + c; o.b = basis + i; o.g = g + c; }
        }
        return o;
    }
};

// ------------------------------------------------------------------------------------------------------------- checks
// the basis values a ray keeps: none for RGBA rows and for the opacity backward
static int basis_floats(const svoxt_options* opt, int C) { return (opt->format != SVOXT_FORMAT_RGBA && C > 0) ? opt->basis_dim : 0; }

// What the steps share: the specs, grad_out [Q, C + 1], T samples in a workspace of the query's size.
static int rowgrad_check(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int64_t* offsets, int64_t T,
                         const float* grad_out, int32_t grad_cols, const void* workspace, int64_t workspace_bytes, bool need_ws,
                         const char* fn) {
    int rc;
    if ((rc = check_tree(tree, fn)) || (rc = check_rays(rays, fn)) || (rc = check_opts(opt, tree, fn, grad_cols > 1))) return rc;
    if (tree->xform != nullptr) return fail(SVOXT_ERR_INVALID, "%s: transformation_matrices (tree.xform) are not served by the deterministic backward", fn);
    if (rays->Q > 0x7fffffffLL) return fail(SVOXT_ERR_INVALID, "%s: too many rays (ray indices are int32)", fn);
    if (tree->M > 0x7fffffffLL) return fail(SVOXT_ERR_INVALID, "%s: M must be below 2^31", fn);
    if ((rc = extent31_check(fn, T, "T"))) return rc;
    const int C = grad_cols - 1;
    if (C < 0) return fail(SVOXT_ERR_INVALID, "%s: grad_cols must be >= 1", fn);
    if (C > 0 && svoxt_out_data_dim(opt, tree->K) != grad_cols)
        return fail(SVOXT_ERR_INVALID, "%s: grad_out columns do not match get_out_data_dim (C + 1)", fn);
    if (!elems_fit((double)T, C + 1) || !elems_fit((double)tree->M, tree->K))
        return fail(SVOXT_ERR_INVALID, "%s: T * (C + 1) and M * K must be below 2^38", fn);
    if (rays->Q > 0 && (offsets == nullptr || grad_out == nullptr)) return fail(SVOXT_ERR_INVALID, "%s: offsets / grad_out is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(grad_out, 4)) return fail(SVOXT_ERR_INVALID, "%s: offsets (8 bytes) / grad_out (4 bytes) is misaligned", fn);
    if (need_ws) {
        if (misaligned(workspace, 8)) return fail(SVOXT_ERR_INVALID, "%s: workspace is not 8-byte aligned", fn);
        const int64_t need = svoxt_render_grad_rows_workspace_bytes(rays->Q, T, tree->M, tree->K, C, basis_floats(opt, C));
        if ((rc = workspace_check(fn, workspace, workspace_bytes, need, "svoxt_render_grad_rows_workspace_bytes(Q, T, M, K, C, basis_dim)")))
            return rc;
    }
    return SVOXT_OK;
}

// ================================================================================= the Gauss-Newton diagonal (4.34)
// svoxt_render_hess_rows_*: next to the gradient, hess[m, j] = the sum over the samples k naming row m and the outputs c of
// curv[ray(k), c] * J(k, c, j)^2 (include/svoxt.h has the sequence).  Count, emit and plan are the gradient's over the
// larger workspace; the sweep runs the gradient's kernels with three of its own in between:
//   rowhess_sig_kernel     a lane per (sample, channel), between the shade and the totals (chan = e): sig = (float)(1.0 /
//                          (1.0 + (double)e)) into the transient [T, C]
//   rowhess_sweep_kernel   a lane per (ray, output): a channel's lane walks the ray's list twice (accum_c, then the sigma
//                          Jacobian of that channel alone) and leaves (jac * jac) * curv in the place of sig; the alpha
//                          lane leaves its term in hsig.  The C + 1 lanes of a ray read a sample's C values side by side.
//   rowhess_sigma_kernel   a lane per sample: hsig = the channels' terms in ascending order from 0.f, then the alpha's
// before the gradient's sweep overwrites delta_t and att.  The reduce sums HessValues over the gradient's plan: a colour
// column squares GradValues' prefix weight * basis * gsig on the fly, the sigma column reads hsig.
// Workspace: the gradient's, then [hsig f32[T]] (persistent: one float a sample) and [sig f32[T * C]] (transient).
struct RowHessSpace {
    RowGradSpace g;
    float *hsig, *sig;
    size_t bytes;
};
static RowHessSpace rowhess_carve(void* workspace, int64_t Q, int64_t T, int64_t M, int K, int C, int bd) {
    RowHessSpace sp;
    sp.g = rowgrad_carve(workspace, Q, T, M, K, C, bd);
    Carver w(workspace != nullptr ? static_cast<char*>(workspace) + sp.g.bytes : nullptr);
    sp.hsig = w.take<float>((size_t)T);
    sp.sig = w.take<float>((size_t)T * (size_t)C);
    sp.bytes = sp.g.bytes + w.bytes();
    return sp;
}

// lane t = k * C + c; in: chan = e
__global__ void __launch_bounds__(kLaunchBlock)
rowhess_sig_kernel(int64_t n, const float* __restrict__ chan, float* __restrict__ sig) {
    const int64_t t = launch_lane();
    if (t >= n) return;
    sig[t] = (float)(1.0 / (1.0 + (double)chan[t]));
}

// lane t = q * (C + 1) + c over the ray's list; in: dt = delta_t, att, sig [T, C].  out: sig[k, c] = channel c's term of
// the sigma entry of sample k (c < C), hsig[k] = the alpha's (c == C).
__global__ void __launch_bounds__(kLaunchBlock)
rowhess_sweep_kernel(Opts opt, int C, const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ curv,
                     const float* __restrict__ dscale, const float* __restrict__ dt, const float* __restrict__ att,
                     float* __restrict__ sig, float* __restrict__ hsig) {
    const int64_t t = launch_lane();
    const int64_t q = t / (C + 1);
    if (q >= Q) return;
    const int c = (int)(t - q * (C + 1));
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    if (b >= e) return;
    const float delta_scale = dscale[q];
    const float cv = curv[q * (C + 1) + c];
    if (c == C) {                                                // the alpha channel: out[q, C] = 1 - light_ray
        float light_ray = 1.f;
        for (int64_t k = b; k < e; ++k) light_ray *= att[k];
        for (int64_t k = b; k < e; ++k) {
            const float jac = (dt[k] * delta_scale) * light_ray;
            hsig[k] = (jac * jac) * cv;
        }
        return;
    }
    float accum = 0.f;
    {   // pass 1
        float light = 1.f;
        for (int64_t k = b; k < e; ++k) {
            const float a = att[k];
            const float weight = light * (1.f - a);
            light *= a;
            accum += weight * sig[k * C + c];
        }
        accum += light * opt.background_brightness;
    }
    {   // pass 2
        float light = 1.f;
        for (int64_t k = b; k < e; ++k) {
            const float a = att[k];
            const float s = sig[k * C + c];
            const float weight = light * (1.f - a);
            light *= a;
            accum -= weight * s;
            const float jac = (dt[k] * delta_scale) * (s * light - accum);
            sig[k * C + c] = (jac * jac) * cv;
        }
    }
}

// a lane per sample; in: hc [T, C] = the channels' terms, hsig = the alpha's.  out: hsig = the sample's sigma entry
__global__ void __launch_bounds__(kLaunchBlock)
rowhess_sigma_kernel(int C, int64_t T, const float* __restrict__ hc, float* __restrict__ hsig) {
    const int64_t k = launch_lane();
    if (k >= T) return;
    float h = 0.f;
    for (int c = 0; c < C; ++c) h += hc[k * C + c];
    h += hsig[k];
    hsig[k] = h;
}

// The entry of sample k at column j of hess: GradValues' columns with sigc = hsig and g = curv.
struct HessValues {
    GradValues v;
    struct Col {
        GradValues::Col c;
        __device__ __forceinline__ float at(int64_t k) const {
            if (c.mode == GradValues::ZERO || k < 0 || k >= c.T) return 0.f;
            if (c.mode == GradValues::SIGMA) return c.v[k];
            const int64_t q = c.ray[k];
            if (q < 0 || q >= c.Q) return 0.f;                   // (the record kernel's own index: never)
            float jac;
            if (c.mode == GradValues::BASIS) {
                jac = c.wgt[k] * c.b[q * c.bd] * c.v[k * c.C];
            } else {
                const float sig = c.v[k * c.C];
                jac = c.wgt[k] * sig * (1.f - sig);
            }
            return (jac * jac) * c.g[q * (c.C + 1)];
        }
    };
    __device__ __forceinline__ Col col(int j) const { return Col{v.col(j)}; }
};

// rowgrad_check's, the curvature beside grad_out, the workspace by the Hessian's query
static int rowhess_check(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int64_t* offsets, int64_t T,
                         const float* grad_out, const float* curv, int32_t grad_cols, const void* workspace, int64_t workspace_bytes,
                         const char* fn) {
    int rc;
    if ((rc = rowgrad_check(tree, rays, opt, offsets, T, grad_out, grad_cols, workspace, workspace_bytes, false, fn))) return rc;
    if (rays->Q > 0 && curv == nullptr) return fail(SVOXT_ERR_INVALID, "%s: curv is NULL", fn);
    if (misaligned(curv, 4)) return fail(SVOXT_ERR_INVALID, "%s: curv (4 bytes) is misaligned", fn);
    if (T > 0) {
        if (misaligned(workspace, 8)) return fail(SVOXT_ERR_INVALID, "%s: workspace is not 8-byte aligned", fn);
        const int C = grad_cols - 1;
        const int64_t need = svoxt_render_hess_rows_workspace_bytes(rays->Q, T, tree->M, tree->K, C, basis_floats(opt, C));
        if ((rc = workspace_check(fn, workspace, workspace_bytes, need, "svoxt_render_hess_rows_workspace_bytes(Q, T, M, K, C, basis_dim)")))
            return rc;
    }
    return SVOXT_OK;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_render_grad_rows_workspace_bytes(int64_t Q, int64_t T, int64_t M, int32_t K, int32_t C, int32_t basis_dim) {
    if (!in31(Q) || !in31(T) || !in31(M)) return -1;
    if (K < 1 || C < 0 || C >= K || basis_dim < 0 || basis_dim > 25) return -1;
    if (!elems_fit((double)T, C + 1) || !elems_fit((double)M, K)) return -1;
    if (T == 0) return 0;
    return (int64_t)rowgrad_carve(nullptr, Q, T, M, K, C, basis_dim).bytes;
}

int svoxt_render_grad_rows_count(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, int64_t* offsets,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_render_grad_rows_count";
    if (tree != nullptr && tree->xform != nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: transformation_matrices (tree.xform) are not served by the deterministic backward", fn);
    const float zero = 0.f;                                      // sigma > 0.f: the backward's sample set, whatever the thresholds say
    return svoxt_ray_samples_count(tree, rays, opt, &zero, offsets, workspace, workspace_bytes, stream);
}

int svoxt_render_grad_rows_emit(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int64_t* offsets,
                                int64_t T, const float* grad_out, int32_t grad_cols, void* workspace, int64_t workspace_bytes,
                                void* stream) {
    const char* fn = "svoxt_render_grad_rows_emit";
    int rc;
    if ((rc = rowgrad_check(tree, rays, opt, offsets, T, grad_out, grad_cols, workspace, workspace_bytes, T > 0, fn))) return rc;
    const int64_t Q = rays->Q;
    if (Q == 0 || T == 0) return SVOXT_OK;
    const int C = grad_cols - 1, bd = basis_floats(opt, C);
    const RowGradSpace sp = rowgrad_carve(workspace, Q, T, tree->M, tree->K, C, bd);
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree);
    const Opts od = to_dev(opt);
    hipStream_t st = (hipStream_t)stream;
    with_bool(tree->N == 2, [&](auto N2) {
        hipLaunchKernelGGL((rowgrad_record_kernel<N2.value>), dim3(nblocks(Q)), dim3(kBlock), 0, st, tr, rd, od, bd, offsets, T, sp.row, sp.ray,
                           sp.wgt, sp.basis, sp.dscale);
        return true;
    });
    return check_launch(fn);
}

int svoxt_render_grad_rows_plan(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int64_t* offsets,
                                int64_t T, const float* grad_out, int32_t grad_cols, int64_t* info, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_render_grad_rows_plan";
    int rc;
    if ((rc = rowgrad_check(tree, rays, opt, offsets, T, grad_out, grad_cols, workspace, workspace_bytes, T > 0, fn))) return rc;
    if (info == nullptr || misaligned(info, 8)) return fail(SVOXT_ERR_INVALID, "%s: info is NULL or not 8-byte aligned", fn);
    if (T == 0) return memset_async(info, sizeof(int64_t) * 4, (hipStream_t)stream, fn);
    const int C = grad_cols - 1;
    const RowGradSpace sp = rowgrad_carve(workspace, rays->Q, T, tree->M, tree->K, C, basis_floats(opt, C));
    return svoxt_row_plan_build(sp.row, T, tree->M, sp.row_ptr, sp.perm, info, sp.plan, sp.plan_bytes, stream);
}

int svoxt_render_grad_rows_sweep(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int64_t* offsets,
                                 int64_t T, const float* grad_out, int32_t grad_cols, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
    const char* fn = "svoxt_render_grad_rows_sweep";
    int rc;
    if ((rc = rowgrad_check(tree, rays, opt, offsets, T, grad_out, grad_cols, workspace, workspace_bytes, T > 0, fn))) return rc;
    const int64_t Q = rays->Q;
    if (Q == 0 || T == 0) return SVOXT_OK;
    const int C = grad_cols - 1, bd = basis_floats(opt, C);
    const RowGradSpace sp = rowgrad_carve(workspace, Q, T, tree->M, tree->K, C, bd);
    const TreeDev tr = to_dev(tree);
    const Opts od = to_dev(opt);
    hipStream_t st = (hipStream_t)stream;
    // the plan is built and the shade kernel is the last reader of `row`: the two totals of a sample go there and into the
    // plan's free sort buffer
    float* tc1 = reinterpret_cast<float*>(sp.row);
    float* tc2 = reinterpret_cast<float*>(row_plan_sort_scratch(sp.plan, T, tree->M));
    hipLaunchKernelGGL(rowgrad_shade_kernel, dim3(launch_blocks(T * (C + 1))), dim3(kLaunchBlock), 0, st, tr.features, tr.M, tr.K, od, C, bd, Q, T,
                       sp.row, sp.ray, sp.wgt, sp.basis, sp.dscale, sp.sigc, sp.chan);
    hipLaunchKernelGGL(rowgrad_totals_kernel, dim3(launch_blocks(T)), dim3(kLaunchBlock), 0, st, od, C, Q, T, sp.ray, grad_out, sp.chan, tc1, tc2);
    hipLaunchKernelGGL(rowgrad_sweep_kernel, dim3(nblocks(Q)), dim3(kBlock), 0, st, od, C, offsets, Q, T, grad_out, sp.dscale, tc1, tc2, sp.wgt,
                       sp.sigc);
    return check_launch(fn);
}

int svoxt_render_grad_rows_reduce(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int64_t* offsets,
                                  int64_t T, const float* grad_out, int32_t grad_cols, int64_t n_long, int64_t n_chunks,
                                  float* grad, int32_t grad_stride, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_render_grad_rows_reduce";
    int rc;
    if ((rc = rowgrad_check(tree, rays, opt, offsets, T, grad_out, grad_cols, workspace, workspace_bytes, T > 0, fn))) return rc;
    const int64_t M = tree->M;
    const int K = tree->K;
    const int gs = grad_stride > 0 ? grad_stride : K;
    if (gs < K) return fail(SVOXT_ERR_INVALID, "%s: grad_stride smaller than data_dim", fn);
    if (!elems_fit((double)M, gs)) return fail(SVOXT_ERR_INVALID, "%s: M * grad_stride must be below 2^38", fn);
    if ((rc = row_plan_check(fn, RowPlanRef{nullptr, nullptr, nullptr, nullptr, nullptr, T, M, n_long, n_chunks}))) return rc;   // (its counts)
    if (M == 0) return SVOXT_OK;
    if (grad == nullptr || misaligned(grad, 4)) return fail(SVOXT_ERR_INVALID, "%s: grad is NULL or not 4-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) {                                                // no sample: zeros in the K columns of every row, the padding untouched
        const hipError_t e = hipMemset2DAsync(grad, sizeof(float) * (size_t)gs, 0, sizeof(float) * (size_t)K, (size_t)M, st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemset2DAsync: %s", fn, hipGetErrorString(e));
        return SVOXT_OK;
    }
    const int C = grad_cols - 1, bd = basis_floats(opt, C);
    const RowGradSpace sp = rowgrad_carve(workspace, rays->Q, T, M, K, C, bd);
    if ((rc = svoxt_row_plan_long(sp.row_ptr, T, M, n_long, n_chunks, sp.plan, sp.plan_bytes, sp.long_rows, sp.long_chunk_ptr, sp.chunk_long,
                                  stream)))
        return rc;
    const GradValues src{sp.ray, sp.wgt, sp.sigc, sp.chan, sp.basis, grad_out, T, rays->Q, K, C, bd, opt->min_comp, opt->max_comp,
                         opt->format == SVOXT_FORMAT_RGBA};
    // a lane per (row, column) over all K columns; the row stride stands where reduce_rows has its table's width
    const RowPlanRef plan{sp.row_ptr, sp.perm, sp.long_rows, sp.long_chunk_ptr, sp.chunk_long, T, M, n_long, n_chunks};
    rows_launch<ROWS_SUM, ROWS_SUM>(src, K, plan, nullptr, gs, 0.f, grad, sp.partials, st);
    return check_launch(fn);
}

int64_t svoxt_render_hess_rows_workspace_bytes(int64_t Q, int64_t T, int64_t M, int32_t K, int32_t C, int32_t basis_dim) {
    if (!in31(Q) || !in31(T) || !in31(M)) return -1;
    if (K < 1 || C < 0 || C >= K || basis_dim < 0 || basis_dim > 25) return -1;
    if (!elems_fit((double)T, C + 1) || !elems_fit((double)M, K)) return -1;
    if (T == 0) return 0;
    return (int64_t)rowhess_carve(nullptr, Q, T, M, K, C, basis_dim).bytes;
}

int svoxt_render_hess_rows_sweep(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int64_t* offsets,
                                 int64_t T, const float* grad_out, const float* curv, int32_t grad_cols, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_render_hess_rows_sweep";
    int rc;
    if ((rc = rowhess_check(tree, rays, opt, offsets, T, grad_out, curv, grad_cols, workspace, workspace_bytes, fn))) return rc;
    const int64_t Q = rays->Q;
    if (Q == 0 || T == 0) return SVOXT_OK;
    const int C = grad_cols - 1, bd = basis_floats(opt, C);
    const RowHessSpace hs = rowhess_carve(workspace, Q, T, tree->M, tree->K, C, bd);
    const RowGradSpace& sp = hs.g;
    const TreeDev tr = to_dev(tree);
    const Opts od = to_dev(opt);
    hipStream_t st = (hipStream_t)stream;
    float* tc1 = reinterpret_cast<float*>(sp.row);
    float* tc2 = reinterpret_cast<float*>(row_plan_sort_scratch(sp.plan, T, tree->M));
    // the launches of svoxt_render_grad_rows_sweep, argument for argument, with the Hessian's three between the shade (which
    // leaves e, delta_t and att) and the totals / sweep (which overwrite them)
    hipLaunchKernelGGL(rowgrad_shade_kernel, dim3(launch_blocks(T * (C + 1))), dim3(kLaunchBlock), 0, st, tr.features, tr.M, tr.K, od, C, bd, Q, T,
                       sp.row, sp.ray, sp.wgt, sp.basis, sp.dscale, sp.sigc, sp.chan);
    if (C > 0)
        hipLaunchKernelGGL(rowhess_sig_kernel, launch_grid(T * C), dim3(kLaunchBlock), 0, st, T * C, sp.chan, hs.sig);
    hipLaunchKernelGGL(rowhess_sweep_kernel, launch_grid(Q * (C + 1)), dim3(kLaunchBlock), 0, st, od, C, offsets, Q, T, curv, sp.dscale, sp.wgt,
                       sp.sigc, hs.sig, hs.hsig);
    hipLaunchKernelGGL(rowhess_sigma_kernel, launch_grid(T), dim3(kLaunchBlock), 0, st, C, T, hs.sig, hs.hsig);
    hipLaunchKernelGGL(rowgrad_totals_kernel, dim3(launch_blocks(T)), dim3(kLaunchBlock), 0, st, od, C, Q, T, sp.ray, grad_out, sp.chan, tc1, tc2);
    hipLaunchKernelGGL(rowgrad_sweep_kernel, dim3(nblocks(Q)), dim3(kBlock), 0, st, od, C, offsets, Q, T, grad_out, sp.dscale, tc1, tc2, sp.wgt,
                       sp.sigc);
    return check_launch(fn);
}

int svoxt_render_hess_rows_reduce(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int64_t* offsets,
                                  int64_t T, const float* grad_out, const float* curv, int32_t grad_cols, int64_t n_long,
                                  int64_t n_chunks, float* grad, int32_t grad_stride, float* hess, int32_t hess_stride, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_render_hess_rows_reduce";
    int rc;
    if ((rc = rowhess_check(tree, rays, opt, offsets, T, grad_out, curv, grad_cols, workspace, workspace_bytes, fn))) return rc;
    const int64_t M = tree->M;
    const int K = tree->K;
    const int hstride = hess_stride > 0 ? hess_stride : K;
    if (hstride < K) return fail(SVOXT_ERR_INVALID, "%s: hess_stride smaller than data_dim", fn);
    if (!elems_fit((double)M, hstride)) return fail(SVOXT_ERR_INVALID, "%s: M * hess_stride must be below 2^38", fn);
    if (M > 0 && (hess == nullptr || misaligned(hess, 4))) return fail(SVOXT_ERR_INVALID, "%s: hess is NULL or not 4-byte aligned", fn);
    if (M > 0 && hess == grad) return fail(SVOXT_ERR_INVALID, "%s: grad and hess must be distinct", fn);
    // the gradient, by its own entry point: its checks of the counts, of grad and its stride, svoxt_row_plan_long, its sums
    if ((rc = svoxt_render_grad_rows_reduce(tree, rays, opt, offsets, T, grad_out, grad_cols, n_long, n_chunks, grad, grad_stride, workspace,
                                            workspace_bytes, stream)))
        return rc;
    if (M == 0) return SVOXT_OK;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) {
        const hipError_t e = hipMemset2DAsync(hess, sizeof(float) * (size_t)hstride, 0, sizeof(float) * (size_t)K, (size_t)M, st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemset2DAsync: %s", fn, hipGetErrorString(e));
        return SVOXT_OK;
    }
    const int C = grad_cols - 1, bd = basis_floats(opt, C);
    const RowHessSpace hs = rowhess_carve(workspace, rays->Q, T, M, K, C, bd);
    const RowGradSpace& sp = hs.g;
    const HessValues src{GradValues{sp.ray, sp.wgt, hs.hsig, sp.chan, sp.basis, curv, T, rays->Q, K, C, bd, opt->min_comp, opt->max_comp,
                                    opt->format == SVOXT_FORMAT_RGBA}};
    const RowPlanRef plan{sp.row_ptr, sp.perm, sp.long_rows, sp.long_chunk_ptr, sp.chunk_long, T, M, n_long, n_chunks};
    rows_launch<ROWS_SUM, ROWS_SUM>(src, K, plan, nullptr, hstride, 0.f, hess, sp.partials, st);
    return check_launch(fn);
}

}  // extern "C"
