// svoxt_depthmom.hip -- render_depth_moments: the first two moments of the compositing weights over distance and the
// accumulated alpha, per ray, and their gradient with respect to the sigma column of the feature table.
//
//     m1 = sum_k w_k z_k     m2 = sum_k w_k z_k^2     alpha = 1 - T_end     w_k = T_k (1 - att_k)
//
// Not in the reference.  The loop is svoxt_raysweep.h's; this file is its payload.  Forward: one 12-byte row per ray; at
// the stop threshold m1 and m2 are rescaled once each.  Backward: with c_k = g1 z_k + g2 z_k^2, sweep 1 forms the ray's
// full sum sum_k w_k c_k, sweep 2 subtracts it down sample by sample (rt_kernel.cu:480) and hands the table (:486-490
// with total_color = c_k; the skeleton adds delta_t ds ga T_end)
//     delta_t ds (c_k T_{k+1} - sum_{i>k} w_i c_i).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_raysweep.h"

#pragma clang fp contract(off)

namespace svoxt {

template <bool MID>
struct DepthMoments {
    static constexpr int kOut = 3;

    static __device__ __forceinline__ float z(const Ray& r, float t, float delta_t) {
        if constexpr (MID) return r.delta_scale * (t + 0.5f * delta_t);
        else return r.delta_scale * t;
    }

    struct Fwd {
        float m1, m2;
        __device__ __forceinline__ void add(float w, float z, float) {
            m1 += w * z;
            m2 += w * (z * z);
        }
        __device__ __forceinline__ void rescale(float scale) {
            m1 *= scale;
            m2 *= scale;
        }
        __device__ __forceinline__ void store(float* __restrict__ row, float light) const {
            row[0] = m1;
            row[1] = m2;
            row[2] = 1.f - light;
        }
    };

    struct Bwd {
        float g1, g2, accum;
        __device__ __forceinline__ void init(const float* __restrict__ g) {
            g1 = g[0];
            g2 = g[1];
        }
        __device__ __forceinline__ void sweep1(float w, float, float z, float) { accum += w * (g1 * z + g2 * (z * z)); }
        __device__ __forceinline__ void turn() {}
        __device__ __forceinline__ float sweep2(float w, float light, float z, float d) {
            const float c = g1 * z + g2 * (z * z);
            accum -= w * c;
            return d * (c * light - accum);
        }
    };
};

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_depth_moments_workspace_bytes(int64_t Q, int64_t max_samples) {
    return dm_workspace_bytes(Q, max_samples);
}

int svoxt_depth_moments_fwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, int32_t at,
                            float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    // (&at: this operator has the argument; raysweep_check refuses an invalid one, which is dispatched as ENTRY until then)
    return with_bool(at == SVOXT_DEPTH_AT_MID, [&](auto MID) {
        return raysweep_fwd<DepthMoments<MID.value>>(tree, rays, opt, &at, out, workspace, workspace_bytes, stream,
                                                     "svoxt_depth_moments_fwd");
    });
}

int svoxt_depth_moments_bwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, int32_t at,
                            const float* grad_out, float* grad, int32_t gstride,
                            void* workspace, int64_t workspace_bytes, void* stream) {
    return with_bool(at == SVOXT_DEPTH_AT_MID, [&](auto MID) {
        return raysweep_bwd<DepthMoments<MID.value>>(tree, rays, opt, &at, grad_out, grad, gstride, workspace, workspace_bytes,
                                                     stream, "svoxt_depth_moments_bwd");
    });
}

}  // extern "C"
