// svoxt_raysweep.h -- the loop of the per-ray operators with a sigma-only gradient (svoxt_depthmom.hip, svoxt_distort.hip;
// DESIGN.md 4.17): one forward that composites a payload along each ray, one backward of two forward-running sweeps.
// The march is the shared walk of svoxt_device.h (setup_ray, then walk_samples; the lock-step tail of sweep 2 takes
// next_crossing / is_sample itself), so the forward, the tails that resume from its t_resume and every other per-ray
// operator see the same samples; lists and table are those of svoxt_raylists.h.  An operator is a payload P:
//
//   P::kOut                      floats per ray of the output row (and of grad_out); the last one is alpha = 1 - T_end
//   P::z(r, t, delta_t)          the distance of a sample: recorded, composited, handed to the sweeps
//   P::Fwd                       the forward's accumulators (zero-initialised): add(w, z, d) per composited sample,
//                                rescale(scale) at the stop threshold, store(out_row, T) at the end
//   P::Bwd                       a lane's state in the backward (zero-initialised): init(grad_out_row) for a live ray;
//                                sweep1(w, T_after, z, d) per sample; turn() between the sweeps; sweep2(w, T_after, z, d)
//                                per sample, which returns what the sample's row receives without the alpha term
//
// with w = T (1 - att) and d = delta_t delta_scale.  A payload holds no loop, no record access, no march and no table call.
//
//   raysweep_fwd_kernel<P, N2, REC>   one lane per ray (ray_of_thread: 8 x 8 tiles of a declared image, the order of a
//                                     sorted batch), accumulators in registers, one row stored per ray.  REC: a backward
//                                     will follow -- every sample with sigma > 0 (the backward's set, rt_kernel.cu:382) is
//                                     also written as (feature row, delta_t, z) into the caller's workspace, up to S a
//                                     ray; where a longer ray's records end is kept as the t to resume the march from.
//   raysweep_bwd_kernel<P, N2>        one wavefront per tile of 64 rays.  Both sweeps use the backward's association of
//                                     the exponent (:397), read the recorded lists (kDmGroup records a lane at a time:
//                                     their sigma gathers and exponentials are independent, only the products run in list
//                                     order) and march what was not recorded -- the tail of an over-long ray, or all of
//                                     it when there is no workspace; a lane's state crosses that seam unchanged.  Sweep 2
//                                     adds d ga T_end to the payload's value and sums by feature row in the tile's LDS
//                                     table, flushed after every kDmRounds samples a lane.  The marched part goes through
//                                     the same table, in lock step: every round each lane marches to its next sample with
//                                     sigma > 0.  No path adds to global memory per sample and lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_device.h"
#include "svoxt_host.h"
#include "svoxt_launch.h"
#include "svoxt_raylists.h"

#pragma clang fp contract(off)

namespace svoxt {

template <class P, bool N2, bool REC>
__global__ void __launch_bounds__(kBlock)
raysweep_fwd_kernel(TreeDev tr, RaysDev rays, Opts opt, float* __restrict__ out, DmLists L) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = ray_of_thread(rays, tid);
    if (q >= rays.Q) {
        if constexpr (REC) L.aux[tid] = make_uint2(0u, 0u);
        return;
    }
    typename P::Fwd acc = {};
    float light = 1.f;
    int nrec = 0;
    bool over = false;
    float t_resume = 0.f;
    Ray r;
    if (setup_ray(tr, rays, opt, q, r)) {
        const int S = L.S;
        bool stopped = false;
        // (REC: every sigma > 0 is recorded, and composited only by the forward's own rules)
        walk_samples<N2>(tr, r, opt.step_size, r.tmin, REC ? 0.f : opt.sigma_thresh, [&](const Sample& s, float t, float sigma) {
            const float z = P::z(r, t, s.delta_t);
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
                acc.add(w, z, s.delta_t * r.delta_scale);
                light *= att;
                if (light <= opt.stop_thresh) {                  // as the colour forward scales its channels (rt_kernel.cu:313-319)
                    acc.rescale((float)(1.0 / (1.0 - (double)light)));
                    if constexpr (!REC) return false;
                    stopped = true;
                }
            }
            return !(REC && over && stopped);                    // false: nothing left to record or to composite
        });
    }
    acc.store(out + q * P::kOut, light);
    if constexpr (REC) L.aux[tid] = make_uint2((uint32_t)nrec | (over ? kDmOver : 0u), __float_as_uint(t_resume));
}

template <class P, bool N2>
__global__ void __launch_bounds__(64)
raysweep_bwd_kernel(TreeDev tr, RaysDev rays, Opts opt, const float* __restrict__ grad_out,
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
    float t_tail = 0.f, ga = 0.f;
    typename P::Bwd c = {};
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
        c.init(grad_out + q * P::kOut);
        ga = grad_out[q * P::kOut + (P::kOut - 1)];
    }
    const int maxn = wave_uniform_max(nrec);
    if (maxn == 0 && !__any(over)) return;
    dm_table_clear(keys, vals, lane);

    // kDmGroup records of a lane: rows, steps and distances, the rows' sigma, the exponentials (slots past the count hold
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

    // sweep 1: the ray's totals and final transmittance (rt_kernel.cu:397-428, no background)
    float light = 1.f;
    for (int kb = 0; kb < nrec; kb += kDmGroup) {
        float dt[kDmGroup], z[kDmGroup], att[kDmGroup];
        int32_t row[kDmGroup];
        fetch(kb, dt, z, att, row);
#pragma unroll
        for (int j = 0; j < kDmGroup; ++j) {
            if (kb + j < nrec) {
                const float w = light * (1.f - att[j]);
                light *= att[j];
                c.sweep1(w, light, z[j], dt[j] * r.delta_scale);
            }
        }
    }
    if (over) {
        walk_samples<N2>(tr, r, opt.step_size, t_tail, 0.f, [&](const Sample& s, float t, float sigma) {
            const float att = pexpf(-s.delta_t * sigma * r.delta_scale);
            const float w = light * (1.f - att);
            light *= att;
            c.sweep1(w, light, P::z(r, t, s.delta_t), s.delta_t * r.delta_scale);
            return true;
        });
    }
    const float light_ray = light;
    c.turn();

    // sweep 2 (:461-490)
    light = 1.f;
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
                    const float w = light * (1.f - att[j]);
                    light *= att[j];
                    dm_table_put(keys, vals, row[j], c.sweep2(w, light, z[j], d) + d * ga * light_ray);
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
                const float t_at = t;
                Sample s;
                float sigma;
                next_crossing<N2>(tr, r, opt.step_size, t, s);
                if (is_sample(tr, s, 0.f, sigma)) {
                    const float d = s.delta_t * r.delta_scale;
                    const float att = pexpf(-s.delta_t * sigma * r.delta_scale);
                    const float w = light * (1.f - att);
                    light *= att;
                    dm_table_put(keys, vals, s.idx, c.sweep2(w, light, P::z(r, t_at, s.delta_t), d) + d * ga * light_ray);
                    found = true;
                }
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

// the arguments every entry point shares; at: the operator's SVOXT_DEPTH_AT_* argument, NULL where it has none
static int raysweep_check(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int32_t* at,
                          const void* workspace, int64_t workspace_bytes, const char* fn) {
    int rc;
    if ((rc = check_tree(tree, fn)) || (rc = check_rays(rays, fn)) || (rc = check_opts(opt, tree, fn, false))) return rc;
    if (at != nullptr && *at != SVOXT_DEPTH_AT_ENTRY && *at != SVOXT_DEPTH_AT_MID)
        return fail(SVOXT_ERR_INVALID, "%s: at must be SVOXT_DEPTH_AT_ENTRY (0) or SVOXT_DEPTH_AT_MID (1)", fn);
    if (workspace_bytes < 0 || (workspace_bytes > 0 && workspace == nullptr) || ((uintptr_t)workspace & 7u) != 0)
        return fail(SVOXT_ERR_INVALID, "%s: workspace is NULL with a size, not 8-byte aligned, or its size negative", fn);
    if (rays->Q > 0x7fffffffLL * 64) return fail(SVOXT_ERR_INVALID, "%s: too many rays", fn);
    return SVOXT_OK;
}

template <class P>
static int raysweep_fwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int32_t* at,
                        float* out, void* workspace, int64_t workspace_bytes, void* stream, const char* fn) {
    int rc;
    if ((rc = raysweep_check(tree, rays, opt, at, workspace, workspace_bytes, fn))) return rc;
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
            hipLaunchKernelGGL((raysweep_fwd_kernel<P, N2.value, REC.value>), dim3(nb), dim3(kBlock), 0, st, tr, rd, od, out, L);
            return true;
        });
    });
    return check_launch(fn);
}

template <class P>
static int raysweep_bwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const int32_t* at,
                        const float* grad_out, float* grad, int32_t gstride, void* workspace, int64_t workspace_bytes,
                        void* stream, const char* fn) {
    int rc;
    if ((rc = raysweep_check(tree, rays, opt, at, workspace, workspace_bytes, fn))) return rc;
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
        hipLaunchKernelGGL((raysweep_bwd_kernel<P, N2.value>), dim3(nb), dim3(64), 0, st, tr, rd, od, grad_out, grad, gs, L);
        return true;
    });
    return check_launch(fn);
}

}  // namespace svoxt
