// svoxt_distort.hip -- render_distortion: the distortion loss of mip-NeRF 360 per ray over the exact leaf crossings, and
// its gradient with respect to the sigma column of the feature table.
//
//     L = sum_i sum_j w_i w_j |s_i - s_j| + (1/3) sum_i w_i^2 d_i        w_k = T_k (1 - att_k)
//     s_k = delta_scale (t + 0.5 delta_t)  (the middle of the crossing)  d_k = delta_t delta_scale  (its length)
//
// Leaves are piecewise constant, so the interval form is exact here, not a quadrature.  The march is the shared one
// (svoxt_device.h), walked exactly as depthmom_fwd_kernel walks it; the record planes and the tile's LDS hash table are
// those of svoxt_raylists.h.  Not in the reference.
//
// The pair term in O(n): with A_k = sum_{j<k} w_j and D_k = sum_{j<k} w_j (s_k - s_j),
//     D_k = D_{k-1} + A_k (s_k - s_{k-1})        (every addend >= 0: no cancellation)
//     sum_i sum_j w_i w_j |s_i - s_j| = 2 sum_k w_k D_k
//
//   distort_fwd_kernel<N2, REC>   one lane per ray (ray_of_thread), accumulators in registers, one 8-byte row
//                                 (L, alpha) stored per ray.  REC: a backward will follow -- every sample with sigma > 0
//                                 is also written as (feature row, delta_t, s) into the caller's workspace, up to S a ray.
//   distort_bwd_kernel<N2>        one wavefront per tile of 64 rays, two forward-running sweeps.  With
//                                     E_k = sum_{j>k} w_j (s_j - s_k)        u_k = dL/dw_k = 2 (D_k + E_k) + (2/3) w_k d_k
//                                 the sigma of sample k receives
//                                     d_k gd (u_k T_{k+1} - sum_{i>k} w_i u_i) + d_k ga T_end.
//                                 Sweep 1 forms A_tot, E_0, T_end and L.  L is homogeneous of degree 2 in w, so
//                                 sum_all w_i u_i = 2 L: sweep 2 subtracts the suffix sum down from 2 L sample by sample,
//                                 carrying D as the forward does and E_k = E_{k-1} - (A_tot - A_k)(s_k - s_{k-1}).
//                                 Both sweeps read the recorded lists, kDmGroup records a lane at a time, and march what
//                                 was not recorded; the state (T, A, D, E, s_{k-1}, the suffix sum) is the lane's and
//                                 crosses the seam unchanged.  The values are summed by feature row in the tile's LDS
//                                 table and flushed as one global atomic per distinct row and pass; the marched part
//                                 goes through the same table in lock step.  No path adds to global memory per sample
//                                 and lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_device.h"
#include "svoxt_host.h"
#include "svoxt_launch.h"
#include "svoxt_raylists.h"

#pragma clang fp contract(off)

namespace svoxt {

template <bool N2, bool REC>
__global__ void __launch_bounds__(kBlock)
distort_fwd_kernel(TreeDev tr, RaysDev rays, Opts opt, float* __restrict__ out, DmLists L) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = ray_of_thread(rays, tid);
    if (q >= rays.Q) {
        if constexpr (REC) L.aux[tid] = make_uint2(0u, 0u);
        return;
    }
    float Lb = 0.f, Lu = 0.f, A = 0.f, D = 0.f, sp = 0.f, light = 1.f;
    int nrec = 0;
    bool over = false;
    float t_resume = 0.f;
    Ray r;
    if (setup_ray(tr, rays, opt, q, r)) {
        const int K = tr.K;
        const int S = L.S;
        float t = r.tmin;
        bool stopped = false;
        while (t < r.tmax) {
            Sample s;
            march_step<N2>(tr, r, opt.step_size, t, s);
            if (s.valid) {
                const float sigma = tr.features[(int64_t)s.idx * K + (K - 1)];
                // (REC: every sigma > 0 is recorded, and composited only by the forward's own rules)
                if (sigma > (REC ? 0.f : opt.sigma_thresh)) {
                    const float z = r.delta_scale * (t + 0.5f * s.delta_t);
                    if constexpr (REC) {
                        if (nrec < S) {
                            const int64_t i = dm_index(tid >> 6, S, nrec, (int)threadIdx.x);
                            L.row[i] = (uint32_t)s.idx;
                            L.dt[i] = s.delta_t;
                            L.z[i] = z;
                            ++nrec;
                        } else if (!over) {
                            over = true;
                            t_resume = t;
                        }
                    }
                    if (!REC || (sigma > opt.sigma_thresh && !stopped)) {
                        const float att = pexpf(-s.delta_t * r.delta_scale * sigma);
                        const float w = light * (1.f - att);
                        D += A * (z - sp);                       // (the first sample: A == 0, nothing is added)
                        sp = z;
                        Lb += w * D;
                        Lu += (w * w) * (s.delta_t * r.delta_scale);
                        A += w;
                        light *= att;
                        if (light <= opt.stop_thresh) {          // the moments' rescale, once per factor of w
                            const float scale = (float)(1.0 / (1.0 - (double)light));
                            Lb *= scale;
                            Lb *= scale;
                            Lu *= scale;
                            Lu *= scale;
                            if constexpr (!REC) break;
                            stopped = true;
                        }
                    }
                    if (REC && over && stopped) break;           // nothing left to record or to composite
                }
            }
            t = march_advance(t, s.delta_t);
        }
    }
    out[q * 2 + 0] = 2.f * Lb + Lu * (1.f / 3.f);
    out[q * 2 + 1] = 1.f - light;
    if constexpr (REC) L.aux[tid] = make_uint2((uint32_t)nrec | (over ? kDmOver : 0u), __float_as_uint(t_resume));
}

// a lane's state along its ray in the backward's sweeps
struct DsSweep {
    float light, A, D, sp;
    // sweep 1
    float Lb, Lu, E0, s0;
    bool seen;
    // sweep 2
    float E, Atot, rem;
};

__device__ __forceinline__ void ds_sweep1(DsSweep& c, float att, float z, float d) {
    const float w = c.light * (1.f - att);
    if (!c.seen) {
        c.s0 = z;
        c.seen = true;
    }
    c.D += c.A * (z - c.sp);
    c.sp = z;
    c.Lb += w * c.D;
    c.Lu += (w * w) * d;
    c.E0 += w * (z - c.s0);
    c.A += w;
    c.light *= att;
}

// d L / d w_k and the suffix sum behind k; returns d_k (u_k T_{k+1} - sum_{i>k} w_i u_i)
__device__ __forceinline__ float ds_sweep2(DsSweep& c, float att, float z, float d) {
    const float w = c.light * (1.f - att);
    const float ds = z - c.sp;                                   // (the first sample: sp == s_0, ds == 0)
    c.sp = z;
    c.D += c.A * ds;
    c.E -= (c.Atot - c.A) * ds;
    const float u = 2.f * (c.D + c.E) + (2.f / 3.f) * (w * d);
    c.A += w;
    c.light *= att;
    c.rem -= w * u;
    return d * (u * c.light - c.rem);
}

template <bool N2>
__global__ void __launch_bounds__(64)
distort_bwd_kernel(TreeDev tr, RaysDev rays, Opts opt, const float* __restrict__ grad_out,
                   float* __restrict__ grad, int gstride, DmLists L) {
    __shared__ int32_t keys[kDmTable];
    __shared__ float vals[kDmTable];
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t tid = tile * 64 + lane;
    const int64_t q = ray_of_thread(rays, tid);
    const int K = tr.K, S = L.S;
    Ray r;
    bool live = q < rays.Q;
    if (live) live = setup_ray(tr, rays, opt, q, r);
    int nrec = 0;
    bool over = false;
    float t_tail = 0.f, gd = 0.f, ga = 0.f;
    if (live) {
        if (S > 0) {
            const uint2 a = L.aux[tid];
            nrec = min((int)(a.x & ~kDmOver), S);
            over = (a.x & kDmOver) != 0u;
            t_tail = __uint_as_float(a.y);
        } else {
            over = true;
            t_tail = r.tmin;
        }
        gd = grad_out[q * 2 + 0];
        ga = grad_out[q * 2 + 1];
    }
    int maxn = nrec;
    for (int off = 32; off > 0; off >>= 1) maxn = max(maxn, __shfl_xor(maxn, off, 64));
    maxn = __builtin_amdgcn_readfirstlane(maxn);
    if (maxn == 0 && !__any(over)) return;
    dm_table_clear(keys, vals, lane);

    // kDmGroup records of a lane: rows, steps and midpoints, the rows' sigma, the exponentials (slots past the count hold
    // stale bits: row 0 is gathered for them and nothing is used)
    auto fetch = [&](int kb, float (&dt)[kDmGroup], float (&z)[kDmGroup], float (&att)[kDmGroup], int32_t (&row)[kDmGroup]) {
        float sig[kDmGroup];
#pragma unroll
        for (int j = 0; j < kDmGroup; ++j) {
            const bool have = kb + j < nrec;
            const int64_t i = dm_index(tile, S, have ? kb + j : 0, lane);
            row[j] = have ? (int32_t)L.row[i] : 0;
            dt[j] = have ? L.dt[i] : 0.f;
            z[j] = have ? L.z[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kDmGroup; ++j) sig[j] = tr.features[(int64_t)row[j] * K + (K - 1)];
#pragma unroll
        for (int j = 0; j < kDmGroup; ++j) att[j] = pexpf(-dt[j] * sig[j] * r.delta_scale);
    };

    // sweep 1: A_tot, E_0, T_end and L, with the backward's association of the exponent
    DsSweep c = {};
    c.light = 1.f;
    for (int kb = 0; kb < nrec; kb += kDmGroup) {
        float dt[kDmGroup], z[kDmGroup], att[kDmGroup];
        int32_t row[kDmGroup];
        fetch(kb, dt, z, att, row);
#pragma unroll
        for (int j = 0; j < kDmGroup; ++j)
            if (kb + j < nrec) ds_sweep1(c, att[j], z[j], dt[j] * r.delta_scale);
    }
    if (over) {
        float t = t_tail;
        while (t < r.tmax) {
            Sample s;
            march_step<N2>(tr, r, opt.step_size, t, s);
            if (s.valid) {
                const float sigma = tr.features[(int64_t)s.idx * K + (K - 1)];
                if (sigma > 0.f)
                    ds_sweep1(c, pexpf(-s.delta_t * sigma * r.delta_scale), r.delta_scale * (t + 0.5f * s.delta_t),
                              s.delta_t * r.delta_scale);
            }
            t = march_advance(t, s.delta_t);
        }
    }
    const float light_ray = c.light;
    c.Atot = c.A;
    c.E = c.E0;
    c.rem = 2.f * (2.f * c.Lb + c.Lu * (1.f / 3.f));
    c.light = 1.f;
    c.A = 0.f;
    c.D = 0.f;
    c.sp = c.s0;

    // sweep 2
    for (int k0 = 0; k0 < maxn; k0 += kDmRounds) {
#pragma unroll 1
        for (int kb = k0; kb < min(k0 + kDmRounds, maxn); kb += kDmGroup) {
            if (kb >= nrec) continue;
            float dt[kDmGroup], z[kDmGroup], att[kDmGroup];
            int32_t row[kDmGroup];
            fetch(kb, dt, z, att, row);
#pragma unroll
            for (int j = 0; j < kDmGroup; ++j) {
                if (kb + j < nrec) {
                    const float d = dt[j] * r.delta_scale;
                    const float v = ds_sweep2(c, att[j], z[j], d);
                    dm_table_put(keys, vals, row[j], gd * v + d * ga * light_ray);
                }
            }
        }
        dm_table_flush(keys, vals, lane, grad, gstride, K - 1);
    }
    // what was not recorded, in lock step: a round takes every such lane to its next sample with sigma > 0
    bool more = over;
    float t = t_tail;
    int round = 0;
    while (__any(more)) {
        if (more) {
            bool found = false;
            while (!found && t < r.tmax) {
                Sample s;
                march_step<N2>(tr, r, opt.step_size, t, s);
                if (s.valid) {
                    const float sigma = tr.features[(int64_t)s.idx * K + (K - 1)];
                    if (sigma > 0.f) {
                        const float d = s.delta_t * r.delta_scale;
                        const float v = ds_sweep2(c, pexpf(-s.delta_t * sigma * r.delta_scale),
                                                  r.delta_scale * (t + 0.5f * s.delta_t), d);
                        dm_table_put(keys, vals, s.idx, gd * v + d * ga * light_ray);
                        found = true;
                    }
                }
                t = march_advance(t, s.delta_t);
            }
            more = found;
        }
        if (++round == kDmRounds) {
            dm_table_flush(keys, vals, lane, grad, gstride, K - 1);
            round = 0;
        }
    }
    if (round != 0) dm_table_flush(keys, vals, lane, grad, gstride, K - 1);
}

static int ds_check(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                    const void* workspace, int64_t workspace_bytes, const char* fn) {
    int rc;
    if ((rc = check_tree(tree, fn)) || (rc = check_rays(rays, fn)) || (rc = check_opts(opt, tree, fn, false))) return rc;
    if (workspace_bytes < 0 || (workspace_bytes > 0 && workspace == nullptr) || ((uintptr_t)workspace & 7u) != 0)
        return fail(SVOXT_ERR_INVALID, "%s: workspace is NULL with a size, not 8-byte aligned, or its size negative", fn);
    if (rays->Q > 0x7fffffffLL * 64) return fail(SVOXT_ERR_INVALID, "%s: too many rays", fn);
    return SVOXT_OK;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_distortion_workspace_bytes(int64_t Q, int64_t max_samples) { return dm_workspace_bytes(Q, max_samples); }

int svoxt_distortion_fwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                         float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_distortion_fwd";
    int rc;
    if ((rc = ds_check(tree, rays, opt, workspace, workspace_bytes, fn))) return rc;
    if (rays->Q == 0) return SVOXT_OK;
    if (out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: out is NULL", fn);
    const DmLists L = dm_lists(workspace, workspace_bytes, rays->Q);
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree);
    const Opts od = to_dev(opt);
    const unsigned nb = nblocks(rays->Q);
    hipStream_t st = (hipStream_t)stream;
    with_bool(tree->N == 2, [&](auto N2) {
        return with_bool(L.S > 0, [&](auto REC) {
            hipLaunchKernelGGL((distort_fwd_kernel<N2.value, REC.value>), dim3(nb), dim3(kBlock), 0, st, tr, rd, od, out, L);
            return true;
        });
    });
    return check_launch(fn);
}

int svoxt_distortion_bwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                         const float* grad_out, float* grad, int32_t gstride,
                         void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_distortion_bwd";
    int rc;
    if ((rc = ds_check(tree, rays, opt, workspace, workspace_bytes, fn))) return rc;
    if (grad == nullptr && tree->M > 0) return fail(SVOXT_ERR_INVALID, "%s: grad is NULL", fn);
    if (rays->Q > 0 && grad_out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: grad_out is NULL", fn);
    const int gs = gstride > 0 ? gstride : tree->K;
    if (gs < tree->K) return fail(SVOXT_ERR_INVALID, "%s: gstride smaller than data_dim", fn);
    if (rays->Q == 0 || tree->M == 0) return SVOXT_OK;
    const DmLists L = dm_lists(workspace, workspace_bytes, rays->Q);
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree);
    const Opts od = to_dev(opt);
    const unsigned nb = nblocks(rays->Q);
    hipStream_t st = (hipStream_t)stream;
    with_bool(tree->N == 2, [&](auto N2) {
        hipLaunchKernelGGL((distort_bwd_kernel<N2.value>), dim3(nb), dim3(64), 0, st, tr, rd, od, grad_out, grad, gs, L);
        return true;
    });
    return check_launch(fn);
}

}  // extern "C"
