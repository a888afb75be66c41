// svoxt_samples.hip -- the per-sample interface (not in the reference): a ray batch's leaf crossings as
// CSR lists, and the two primitives that turn per-sample values back into per-ray values.
//
//   ray_samples      count -> scan -> emit.  Both kernels take the shared walk (setup_ray, then walk_samples / walk_crossings
//                    of svoxt_device.h), one lane per ray by ray_of_thread, through one adapter (ray_samples below).  The count
//                    kernel writes counts[q] at the ray's own index and adds each wavefront's count to one 64-bit total;
//                    the per-ray tail of svoxt_listemit.h scans the counts into starts and widens them to int64
//                    offsets[Q + 1] with the 64-bit total at offsets[Q].  The emit kernel marches again and writes (row, ray, depth, length) at
//                    offsets[q] + k, never at or behind offsets[q + 1]: the lists are in ray-index order whatever the lane
//                    assignment was.  No float sum anywhere: bit-identical from run to run.
//                        depth = delta_scale * t         (the `entry` z of the depth moments, this operand order)
//                        length = delta_t * delta_scale  (the d of the sweeps)
//   sample_weights   one lane per ray walks its segment in list order, float32, no contraction:
//                        sigma > 0:  att = pexpf(-(length * sigma));  w = T * (1 - att);  T *= att      else: w = 0
//                    alpha = 1 - T_end.  Backward, two forward-running sweeps over the same products ("subtract down from
//                    the total", as raysweep_bwd_kernel): sweep 1 forms total = sum_j gw_j w_j and T_end; sweep 2 per
//                    sample: total -= gw * w;  grad_sigma = length * ((gw * T_after - total) + ga * T_end); 0 where
//                    sigma <= 0.  One entry per sample, no atomics.  svoxt_sample_weights_bwd_length is the same pass with
//                    a second output, grad_length = sigma * that bracket (the <true> instance of the kernel).
//   accumulate       a lane per (ray, channel): acc += w * v in list order.  Backward: a lane per sample, one pass over
//                    values: grad_w = sum_c g[ray, c] * v[c] in ascending c, grad_values[c] = w * g[ray, c].
//   faces             svoxt_ray_samples_emit_faces is the emit with a fifth array: per sample the axis of
//                    the plane the ray entered its leaf through and of the one it leaves through, entry | exit << 2
//                    (exit_axis / cube_entry_axis below).  An adapter and an emit instance of their own; the count is the
//                    shared one and the plain emit's kernels are untouched.
//   sample_geometry  backward only (the forward is the two list arrays): a lane per ray walks its segment in list order
//                    and sums the two planes' terms into six accumulators -- grad_origins / grad_dirs [Q, 3], every
//                    ray written, no atomics (sample_geometry_bwd_kernel).
// C ABI: svoxt_ray_samples_* / svoxt_sample_weights_* / svoxt_sample_accumulate_* / svoxt_sample_geometry_bwd (include/svoxt.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_device.h"
#include "svoxt_host.h"
#include "svoxt_listemit.h"
#include "svoxt_wave.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

// The samples of ray q in march order: f(row, depth, length) per sample of the shared walk (svoxt_device.h); without
// FILTER per crossing whose data word names a feature row -- the crossing layer: sigma is not read.
template <bool N2, bool FILTER, class F>
__device__ __forceinline__ void ray_samples(const TreeDev& tr, const RaysDev& rays, const Opts& opt, float min_sigma, int64_t q, F&& f) {
    Ray r;
    if (!setup_ray(tr, rays, opt, q, r)) return;
    auto emit = [&](const Sample& s, float t) { f(s.idx, r.delta_scale * t, s.delta_t * r.delta_scale); return true; };
    if constexpr (FILTER) walk_samples<N2>(tr, r, opt.step_size, r.tmin, min_sigma, [&](const Sample& s, float t, float) { return emit(s, t); });
    else walk_crossings<N2>(tr, r, opt.step_size, r.tmin, [&](const Sample& s, float t) { return !s.valid || emit(s, t); });
}

template <bool N2, bool FILTER>
__global__ void __launch_bounds__(kBlock)
samples_count_kernel(TreeDev tr, RaysDev rays, Opts opt, float min_sigma, uint32_t* __restrict__ counts,
                     unsigned long long* __restrict__ total) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = ray_of_thread(rays, tid);
    uint32_t n = 0;
    if (q < rays.Q) {
        ray_samples<N2, FILTER>(tr, rays, opt, min_sigma, q, [&](int32_t, float, float) { ++n; });
        counts[q] = n;
    }
    wave_add_to_total(n, total);                                 // (a wavefront's 64 counts: far below 2^32)
}

template <bool N2, bool FILTER>
__global__ void __launch_bounds__(kBlock)
samples_emit_kernel(TreeDev tr, RaysDev rays, Opts opt, float min_sigma, const int64_t* __restrict__ offsets,
                    int32_t* __restrict__ row, int32_t* __restrict__ ray, float* __restrict__ depth, float* __restrict__ length) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = ray_of_thread(rays, tid);
    if (q >= rays.Q) return;
    int64_t at = offsets[q];
    const int64_t end = offsets[q + 1];
    if (at < 0) return;
    ray_samples<N2, FILTER>(tr, rays, opt, min_sigma, q, [&](int32_t idx, float z, float d) {
        if (at < end) {                                          // (the count's march found as many: never past the ray's own segment)
            row[at] = idx;
            ray[at] = (int32_t)q;
            depth[at] = z;
            length[at] = d;
            ++at;
        }
    });
}

// ------------------------------------------------------------------------------------------------------------- faces
// The axis of the plane a ray leaves a leaf through: m_a = fmaxf(-l_a * i_a, -l_a * i_a + i_a) on the leaf-local point,
// the three values whose minimum leaf_delta_t takes, recomputed here in its operations; the first axis in x, y, z that
// holds the minimum, by a strict-less update.
__device__ __forceinline__ uint32_t exit_axis(const Leaf& lf, const Ray& r) {
    float t1, t2;
    t1 = -lf.lx * r.ix; t2 = t1 + r.ix; const float mx = fmaxf(t1, t2);
    t1 = -lf.ly * r.iy; t2 = t1 + r.iy; const float my = fmaxf(t1, t2);
    t1 = -lf.lz * r.iz; t2 = t1 + r.iz; const float mz = fmaxf(t1, t2);
    uint32_t a = 0;
    float best = mx;
    if (my < best) { best = my; a = 1; }
    if (mz < best) a = 2;
    return a;
}

// The axis of the cube's plane a ray enters through: n_a = fminf(t1, t2) of dda_unit's slab test; with r.tmin > 0 the
// first axis in x, y, z whose n_a is r.tmin, else 3 -- no plane: the origin lies inside or on the cube.
__device__ __forceinline__ uint32_t cube_entry_axis(const Ray& r) {
    if (!(r.tmin > 0.f)) return 3;
    float t1, t2;
    t1 = -r.ox * r.ix; t2 = t1 + r.ix; const float nx = fminf(t1, t2);
    t1 = -r.oy * r.iy; t2 = t1 + r.iy; const float ny = fminf(t1, t2);
    t1 = -r.oz * r.iz; t2 = t1 + r.iz; const float nz = fminf(t1, t2);
    return nx == r.tmin ? 0u : ny == r.tmin ? 1u : nz == r.tmin ? 2u : 3u;
}

// ray_samples with the face byte: f(row, depth, length, entry | exit << 2).  Every crossing comes through here -- the
// entry axis of a sample is the exit axis of the crossing marched before it, emitted or not --, so the FILTER variant
// is walk_crossings with is_sample inside, not walk_samples.
template <bool N2, bool FILTER, class F>
__device__ __forceinline__ void ray_samples_faces(const TreeDev& tr, const RaysDev& rays, const Opts& opt, float min_sigma, int64_t q, F&& f) {
    Ray r;
    if (!setup_ray(tr, rays, opt, q, r)) return;
    uint32_t entry = cube_entry_axis(r);
    walk_crossings<N2>(tr, r, opt.step_size, r.tmin, [&](const Sample& s, float t) {
        const uint32_t exit = exit_axis(s.leaf, r);
        bool is;
        if constexpr (FILTER) {
            float sigma;
            is = is_sample(tr, s, min_sigma, sigma);
        } else {
            is = s.valid;
        }
        if (is) f(s.idx, r.delta_scale * t, s.delta_t * r.delta_scale, (uint8_t)(entry | exit << 2));
        entry = exit;
        return true;
    });
}

template <bool N2, bool FILTER>
__global__ void __launch_bounds__(kBlock)
samples_emit_faces_kernel(TreeDev tr, RaysDev rays, Opts opt, float min_sigma, const int64_t* __restrict__ offsets,
                          int32_t* __restrict__ row, int32_t* __restrict__ ray, float* __restrict__ depth, float* __restrict__ length,
                          uint8_t* __restrict__ face) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = ray_of_thread(rays, tid);
    if (q >= rays.Q) return;
    int64_t at = offsets[q];
    const int64_t end = offsets[q + 1];
    if (at < 0) return;
    ray_samples_faces<N2, FILTER>(tr, rays, opt, min_sigma, q, [&](int32_t idx, float z, float d, uint8_t fc) {
        if (at < end) {                                          // (as samples_emit_kernel: never past the ray's own segment)
            row[at] = idx;
            ray[at] = (int32_t)q;
            depth[at] = z;
            length[at] = d;
            face[at] = fc;
            ++at;
        }
    });
}

// ---------------------------------------------------------------------------------------------------- sample_geometry
// The gradient of the two planes of every crossing (include/svoxt.h states the sequence): z = (P_a - o_a) / d_a in the
// parameter along dirs as given, so dz/do_a = -1 / d_a and dz/dd_a = -z / d_a.  The accumulators are addressed by a
// run-time axis: written with selects, never as an indexed private array (which would live in scratch memory).
__global__ void __launch_bounds__(kLaunchBlock)
sample_geometry_bwd_kernel(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const uint8_t* __restrict__ face,
                           const float* __restrict__ depth, const float* __restrict__ length, const float* __restrict__ dirs,
                           const float* __restrict__ grad_depth, const float* __restrict__ grad_length,
                           float* __restrict__ grad_origins, float* __restrict__ grad_dirs) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (q >= Q) return;
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    const float d0 = dirs[3 * q], d1 = dirs[3 * q + 1], d2 = dirs[3 * q + 2];
    float go0 = 0.f, go1 = 0.f, go2 = 0.f, gd0 = 0.f, gd1 = 0.f, gd2 = 0.f;
    for (int64_t k = b; k < e; ++k) {
        const uint32_t fc = face[k];
        const float z = depth[k], len = length[k];
        const float gD = grad_depth != nullptr ? grad_depth[k] : 0.f;
        const float gL = grad_length != nullptr ? grad_length[k] : 0.f;
        const float gz_in = gD - gL, gz_out = gL;
        const uint32_t a = fc & 3u, x = (fc >> 2) & 3u;
        const float da = a == 0 ? d0 : a == 1 ? d1 : d2;
        if (a < 3 && da != 0.f) {
            const float u = gz_in / da;
            const float uz = u * z;
            go0 = a == 0 ? go0 - u : go0;   go1 = a == 1 ? go1 - u : go1;   go2 = a == 2 ? go2 - u : go2;
            gd0 = a == 0 ? gd0 - uz : gd0;  gd1 = a == 1 ? gd1 - uz : gd1;  gd2 = a == 2 ? gd2 - uz : gd2;
        }
        const float dx = x == 0 ? d0 : x == 1 ? d1 : d2;
        if (x < 3 && dx != 0.f) {                                // (the march writes no exit axis 3)
            const float v = gz_out / dx;
            const float vz = v * (z + len);
            go0 = x == 0 ? go0 - v : go0;   go1 = x == 1 ? go1 - v : go1;   go2 = x == 2 ? go2 - v : go2;
            gd0 = x == 0 ? gd0 - vz : gd0;  gd1 = x == 1 ? gd1 - vz : gd1;  gd2 = x == 2 ? gd2 - vz : gd2;
        }
    }
    grad_origins[3 * q] = go0; grad_origins[3 * q + 1] = go1; grad_origins[3 * q + 2] = go2;
    grad_dirs[3 * q] = gd0; grad_dirs[3 * q + 1] = gd1; grad_dirs[3 * q + 2] = gd2;
}

// ----------------------------------------------------------------------------------------------------- sample_weights
__global__ void __launch_bounds__(kLaunchBlock)
sample_weights_fwd_kernel(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ length,
                          const float* __restrict__ sigma, float* __restrict__ w, float* __restrict__ alpha) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (q >= Q) return;
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    float light = 1.f;
    for (int64_t k = b; k < e; ++k) {
        const float sg = sigma[k];
        float wk = 0.f;
        if (sg > 0.f) {
            const float att = pexpf(-(length[k] * sg));
            wk = light * (1.f - att);
            light *= att;
        }
        w[k] = wk;
    }
    alpha[q] = 1.f - light;
}

// LEN: also grad_length[k] = sigma * the bracket grad_sigma multiplies by length, from the same pass
template <bool LEN>
__global__ void __launch_bounds__(kLaunchBlock)
sample_weights_bwd_kernel(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ length,
                          const float* __restrict__ sigma, const float* __restrict__ grad_w, const float* __restrict__ grad_alpha,
                          float* __restrict__ grad_sigma, float* __restrict__ grad_length) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (q >= Q) return;
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    // sweep 1: the ray's total and final transmittance
    float light = 1.f, total = 0.f;
    for (int64_t k = b; k < e; ++k) {
        const float sg = sigma[k];
        if (sg > 0.f) {
            const float att = pexpf(-(length[k] * sg));
            const float wk = light * (1.f - att);
            light *= att;
            if (grad_w != nullptr) total += grad_w[k] * wk;
        }
    }
    const float tail = (grad_alpha != nullptr ? grad_alpha[q] : 0.f) * light;
    // sweep 2: subtract down
    light = 1.f;
    for (int64_t k = b; k < e; ++k) {
        const float sg = sigma[k];
        float gs = 0.f, gl = 0.f;
        if (sg > 0.f) {
            const float d = length[k];
            const float att = pexpf(-(d * sg));
            const float wk = light * (1.f - att);
            light *= att;
            const float gw = grad_w != nullptr ? grad_w[k] : 0.f;
            total -= gw * wk;
            const float br = (gw * light - total) + tail;
            gs = d * br;
            if constexpr (LEN) gl = sg * br;
        }
        grad_sigma[k] = gs;
        if constexpr (LEN) grad_length[k] = gl;
    }
}

// --------------------------------------------------------------------------------------------------------- accumulate
// lane t = q * C + c
__global__ void __launch_bounds__(kLaunchBlock)
sample_accumulate_fwd_kernel(const int64_t* __restrict__ offsets, int64_t Q, int64_t T, const float* __restrict__ w,
                             const float* __restrict__ values, int C, float* __restrict__ out) {
    const int64_t t = launch_lane();
    const int64_t q = t / C;
    if (q >= Q) return;
    const int c = (int)(t - q * C);
    const int64_t b = max(offsets[q], (int64_t)0), e = min(offsets[q + 1], T);
    float acc = 0.f;
    if (values != nullptr) {
        for (int64_t k = b; k < e; ++k) acc += w[k] * values[k * C + c];
    } else {
        for (int64_t k = b; k < e; ++k) acc += w[k];
    }
    out[t] = acc;
}

// a lane per sample
__global__ void __launch_bounds__(kLaunchBlock)
sample_accumulate_bwd_kernel(const int32_t* __restrict__ ray, int64_t Q, int64_t T, const float* __restrict__ w,
                             const float* __restrict__ values, int C, const float* __restrict__ grad_out,
                             float* __restrict__ grad_w, float* __restrict__ grad_values) {
    const int64_t k = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (k >= T) return;
    const int64_t q = ray[k];
    const bool in = q >= 0 && q < Q;
    const float* __restrict__ g = grad_out + (in ? q : 0) * C;
    const float wk = grad_values != nullptr ? w[k] : 0.f;
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
        const float gc = in ? g[c] : 0.f;
        if (values != nullptr) s += gc * values[k * C + c];
        else s += gc;
        if (grad_values != nullptr) grad_values[k * C + c] = wk * gc;
    }
    if (grad_w != nullptr) grad_w[k] = s;
}

// ------------------------------------------------------------------------------------------------------------- checks
static int ray_samples_check(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* min_sigma,
                             const int64_t* offsets, const char* fn) {
    int rc;
    if ((rc = check_tree(tree, fn)) || (rc = check_rays(rays, fn)) || (rc = check_opts(opt, tree, fn, false))) return rc;
    if (rays->Q > 0x7fffffffLL) return fail(SVOXT_ERR_INVALID, "%s: too many rays (ray indices are int32)", fn);
    if (min_sigma != nullptr && *min_sigma != *min_sigma) return fail(SVOXT_ERR_INVALID, "%s: min_sigma is NaN", fn);
    if (rays->Q > 0 && offsets == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets is NULL", fn);
    if (misaligned(offsets, 8)) return fail(SVOXT_ERR_INVALID, "%s: offsets is not 8-byte aligned", fn);
    return SVOXT_OK;
}

// the CSR arguments of the four per-sample entry points: Q rays, T samples, both below 2^31
static int csr_check(int64_t Q, int64_t T, const char* fn) {
    const int rc = extent31_check(fn, Q, "Q");
    return rc ? rc : extent31_check(fn, T, "T");
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_ray_samples_workspace_bytes(int64_t Q) {
    return list_space_bytes(Q, 0, true);
}

int svoxt_ray_samples_count(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* min_sigma,
                            int64_t* offsets, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_ray_samples_count";
    int rc;
    if ((rc = ray_samples_check(tree, rays, opt, min_sigma, offsets, fn))) return rc;
    const int64_t Q = rays->Q;
    if (Q == 0) return SVOXT_OK;
    ListSpace sp;
    if ((rc = list_space_check(fn, workspace, workspace_bytes, (size_t)Q, true, "svoxt_ray_samples_workspace_bytes(Q)", &sp))) return rc;
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree);
    const Opts od = to_dev(opt);
    const float ms = min_sigma != nullptr ? *min_sigma : 0.f;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = memset_async(workspace, sp.clear_bytes, st, fn))) return rc;
    with_bool(tree->N == 2, [&](auto N2) {
        return with_bool(min_sigma != nullptr, [&](auto FILTER) {
            hipLaunchKernelGGL((samples_count_kernel<N2.value, FILTER.value>), dim3(nblocks(Q)), dim3(kBlock), 0, st, tr, rd, od, ms,
                               sp.counts, sp.total);
            return true;
        });
    });
    return list_ray_offsets<false>(fn, sp, Q, offsets, nullptr, st);     // (the caller reads the total at offsets[Q])
}

int svoxt_ray_samples_emit(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* min_sigma,
                           const int64_t* offsets, int32_t* row, int32_t* ray, float* depth, float* length, void* stream) {
    const char* fn = "svoxt_ray_samples_emit";
    int rc;
    if ((rc = ray_samples_check(tree, rays, opt, min_sigma, offsets, fn))) return rc;
    const int64_t Q = rays->Q;
    if (Q == 0) return SVOXT_OK;
    if (row == nullptr || ray == nullptr || depth == nullptr || length == nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: row / ray / depth / length is NULL", fn);
    if (misaligned(row, 4) || misaligned(ray, 4) || misaligned(depth, 4) || misaligned(length, 4))
        return fail(SVOXT_ERR_INVALID, "%s: row / ray / depth / length is not 4-byte aligned", fn);
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree);
    const Opts od = to_dev(opt);
    const float ms = min_sigma != nullptr ? *min_sigma : 0.f;
    hipStream_t st = (hipStream_t)stream;
    with_bool(tree->N == 2, [&](auto N2) {
        return with_bool(min_sigma != nullptr, [&](auto FILTER) {
            hipLaunchKernelGGL((samples_emit_kernel<N2.value, FILTER.value>), dim3(nblocks(Q)), dim3(kBlock), 0, st, tr, rd, od, ms,
                               offsets, row, ray, depth, length);
            return true;
        });
    });
    return check_launch(fn);
}

int svoxt_ray_samples_emit_faces(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* min_sigma,
                                 const int64_t* offsets, int32_t* row, int32_t* ray, float* depth, float* length, uint8_t* face,
                                 void* stream) {
    const char* fn = "svoxt_ray_samples_emit_faces";
    int rc;
    if ((rc = ray_samples_check(tree, rays, opt, min_sigma, offsets, fn))) return rc;
    const int64_t Q = rays->Q;
    if (Q == 0) return SVOXT_OK;
    if (row == nullptr || ray == nullptr || depth == nullptr || length == nullptr || face == nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: row / ray / depth / length / face is NULL", fn);
    if (misaligned(row, 4) || misaligned(ray, 4) || misaligned(depth, 4) || misaligned(length, 4))
        return fail(SVOXT_ERR_INVALID, "%s: row / ray / depth / length is not 4-byte aligned", fn);
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree);
    const Opts od = to_dev(opt);
    const float ms = min_sigma != nullptr ? *min_sigma : 0.f;
    hipStream_t st = (hipStream_t)stream;
    with_bool(tree->N == 2, [&](auto N2) {
        return with_bool(min_sigma != nullptr, [&](auto FILTER) {
            hipLaunchKernelGGL((samples_emit_faces_kernel<N2.value, FILTER.value>), dim3(nblocks(Q)), dim3(kBlock), 0, st, tr, rd, od, ms,
                               offsets, row, ray, depth, length, face);
            return true;
        });
    });
    return check_launch(fn);
}

int svoxt_sample_weights_fwd(const int64_t* offsets, int64_t Q, int64_t T, const float* length, const float* sigma, float* w,
                             float* alpha, void* stream) {
    const char* fn = "svoxt_sample_weights_fwd";
    int rc;
    if ((rc = csr_check(Q, T, fn))) return rc;
    if (Q == 0) return SVOXT_OK;
    if (offsets == nullptr || alpha == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets / alpha is NULL", fn);
    if (T > 0 && (length == nullptr || sigma == nullptr || w == nullptr)) return fail(SVOXT_ERR_INVALID, "%s: length / sigma / w is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(length, 4) || misaligned(sigma, 4) || misaligned(w, 4) || misaligned(alpha, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the float arrays: 4)", fn);
    hipLaunchKernelGGL(sample_weights_fwd_kernel, dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, offsets, Q, T,
                       length, sigma, w, alpha);
    return check_launch(fn);
}

int svoxt_sample_weights_bwd(const int64_t* offsets, int64_t Q, int64_t T, const float* length, const float* sigma,
                             const float* grad_w, const float* grad_alpha, float* grad_sigma, void* stream) {
    const char* fn = "svoxt_sample_weights_bwd";
    int rc;
    if ((rc = csr_check(Q, T, fn))) return rc;
    if (Q == 0 || T == 0) return SVOXT_OK;
    if (offsets == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets is NULL", fn);
    if (length == nullptr || sigma == nullptr || grad_sigma == nullptr) return fail(SVOXT_ERR_INVALID, "%s: length / sigma / grad_sigma is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(length, 4) || misaligned(sigma, 4) || misaligned(grad_w, 4) || misaligned(grad_alpha, 4) ||
        misaligned(grad_sigma, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the float arrays: 4)", fn);
    hipLaunchKernelGGL(sample_weights_bwd_kernel<false>, dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, offsets, Q, T,
                       length, sigma, grad_w, grad_alpha, grad_sigma, (float*)nullptr);
    return check_launch(fn);
}

int svoxt_sample_weights_bwd_length(const int64_t* offsets, int64_t Q, int64_t T, const float* length, const float* sigma,
                                    const float* grad_w, const float* grad_alpha, float* grad_sigma, float* grad_length, void* stream) {
    const char* fn = "svoxt_sample_weights_bwd_length";
    int rc;
    if ((rc = csr_check(Q, T, fn))) return rc;
    if (Q == 0 || T == 0) return SVOXT_OK;
    if (offsets == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets is NULL", fn);
    if (length == nullptr || sigma == nullptr || grad_sigma == nullptr || grad_length == nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: length / sigma / grad_sigma / grad_length is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(length, 4) || misaligned(sigma, 4) || misaligned(grad_w, 4) || misaligned(grad_alpha, 4) ||
        misaligned(grad_sigma, 4) || misaligned(grad_length, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the float arrays: 4)", fn);
    hipLaunchKernelGGL(sample_weights_bwd_kernel<true>, dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, offsets, Q, T,
                       length, sigma, grad_w, grad_alpha, grad_sigma, grad_length);
    return check_launch(fn);
}

int svoxt_sample_geometry_bwd(const int64_t* offsets, int64_t Q, int64_t T, const uint8_t* face, const float* depth, const float* length,
                              const float* dirs, const float* grad_depth, const float* grad_length, float* grad_origins,
                              float* grad_dirs, void* stream) {
    const char* fn = "svoxt_sample_geometry_bwd";
    int rc;
    if ((rc = csr_check(Q, T, fn))) return rc;
    if (Q == 0) return SVOXT_OK;
    if (offsets == nullptr || dirs == nullptr || grad_origins == nullptr || grad_dirs == nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: offsets / dirs / grad_origins / grad_dirs is NULL", fn);
    if (T > 0 && (face == nullptr || depth == nullptr || length == nullptr)) return fail(SVOXT_ERR_INVALID, "%s: face / depth / length is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(depth, 4) || misaligned(length, 4) || misaligned(dirs, 4) || misaligned(grad_depth, 4) ||
        misaligned(grad_length, 4) || misaligned(grad_origins, 4) || misaligned(grad_dirs, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the float arrays: 4)", fn);
    hipLaunchKernelGGL(sample_geometry_bwd_kernel, dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, offsets, Q, T, face,
                       depth, length, dirs, grad_depth, grad_length, grad_origins, grad_dirs);
    return check_launch(fn);
}

int svoxt_sample_accumulate_fwd(const int64_t* offsets, int64_t Q, int64_t T, const float* w, const float* values, int32_t C,
                                float* out, void* stream) {
    const char* fn = "svoxt_sample_accumulate_fwd";
    int rc;
    if ((rc = csr_check(Q, T, fn))) return rc;
    if (C < 1 || !elems_fit((double)Q, C) || !elems_fit((double)T, C))
        return fail(SVOXT_ERR_INVALID, "%s: C must be >= 1 with Q * C and T * C below 2^38", fn);
    if (values == nullptr && C != 1 && T > 0) return fail(SVOXT_ERR_INVALID, "%s: values is NULL: C must be 1 (the plain sum of w)", fn);
    if (Q == 0) return SVOXT_OK;
    if (offsets == nullptr || out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets / out is NULL", fn);
    if (T > 0 && w == nullptr) return fail(SVOXT_ERR_INVALID, "%s: w is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(w, 4) || misaligned(values, 4) || misaligned(out, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets: 8 bytes, the float arrays: 4)", fn);
    hipLaunchKernelGGL(sample_accumulate_fwd_kernel, launch_grid(Q * C), dim3(kLaunchBlock), 0, (hipStream_t)stream, offsets, Q, T,
                       w, values, (int)C, out);
    return check_launch(fn);
}

int svoxt_sample_accumulate_bwd(const int32_t* ray, int64_t Q, int64_t T, const float* w, const float* values, int32_t C,
                                const float* grad_out, float* grad_w, float* grad_values, void* stream) {
    const char* fn = "svoxt_sample_accumulate_bwd";
    int rc;
    if ((rc = csr_check(Q, T, fn))) return rc;
    if (C < 1 || !elems_fit((double)Q, C) || !elems_fit((double)T, C))
        return fail(SVOXT_ERR_INVALID, "%s: C must be >= 1 with Q * C and T * C below 2^38", fn);
    if (values == nullptr && T > 0 && (C != 1 || grad_values != nullptr))
        return fail(SVOXT_ERR_INVALID, "%s: values is NULL: C must be 1 and grad_values NULL", fn);
    if (Q == 0 || T == 0 || (grad_w == nullptr && grad_values == nullptr)) return SVOXT_OK;
    if (ray == nullptr || grad_out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: ray / grad_out is NULL", fn);
    if (grad_values != nullptr && w == nullptr) return fail(SVOXT_ERR_INVALID, "%s: w is NULL", fn);
    if (misaligned(ray, 4) || misaligned(w, 4) || misaligned(values, 4) || misaligned(grad_out, 4) || misaligned(grad_w, 4) ||
        misaligned(grad_values, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    hipLaunchKernelGGL(sample_accumulate_bwd_kernel, dim3(launch_blocks(T)), dim3(kLaunchBlock), 0, (hipStream_t)stream, ray, Q, T, w,
                       values, (int)C, grad_out, grad_w, grad_values);
    return check_launch(fn);
}

}  // extern "C"
