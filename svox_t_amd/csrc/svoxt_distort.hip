// svoxt_distort.hip -- render_distortion: the distortion loss of mip-NeRF 360 per ray over the exact leaf crossings, and
// its gradient with respect to the sigma column of the feature table.
//
//     L = sum_i sum_j w_i w_j |s_i - s_j| + (1/3) sum_i w_i^2 d_i        w_k = T_k (1 - att_k)
//     s_k = delta_scale (t + 0.5 delta_t)  (the middle of the crossing)  d_k = delta_t delta_scale  (its length)
//
// Leaves are piecewise constant, so the interval form is exact here, not a quadrature.  Not in the reference.  The loop is
// svoxt_raysweep.h's; this file is its payload.
//
// The pair term in O(n): with A_k = sum_{j<k} w_j and D_k = sum_{j<k} w_j (s_k - s_j),
//     D_k = D_{k-1} + A_k (s_k - s_{k-1})        (every addend >= 0: no cancellation)
//     sum_i sum_j w_i w_j |s_i - s_j| = 2 sum_k w_k D_k
// Forward: one 8-byte row (L, alpha) per ray; at the stop threshold the moments' rescale, once per factor of w.
//
// Backward: with
//     E_k = sum_{j>k} w_j (s_j - s_k)        u_k = dL/dw_k = 2 (D_k + E_k) + (2/3) w_k d_k
// the sigma of sample k receives (the skeleton adds d_k ga T_end)
//     d_k gd (u_k T_{k+1} - sum_{i>k} w_i u_i).
// Sweep 1 forms A_tot, E_0 and L.  L is homogeneous of degree 2 in w, so sum_all w_i u_i = 2 L: sweep 2 subtracts the
// suffix sum down from 2 L sample by sample, carrying D as the forward does and E_k = E_{k-1} - (A_tot - A_k)(s_k - s_{k-1}).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_raysweep.h"

#pragma clang fp contract(off)

namespace svoxt {

struct Distortion {
    static constexpr int kOut = 2;

    static __device__ __forceinline__ float z(const Ray& r, float t, float delta_t) {
        return r.delta_scale * (t + 0.5f * delta_t);
    }

    struct Fwd {
        float Lb, Lu, A, D, sp;
        __device__ __forceinline__ void add(float w, float z, float d) {
            D += A * (z - sp);                                   // (the first sample: A == 0, nothing is added)
            sp = z;
            Lb += w * D;
            Lu += (w * w) * d;
            A += w;
        }
        __device__ __forceinline__ void rescale(float scale) {
            Lb *= scale;
            Lb *= scale;
            Lu *= scale;
            Lu *= scale;
        }
        __device__ __forceinline__ void store(float* __restrict__ row, float light) const {
            row[0] = 2.f * Lb + Lu * (1.f / 3.f);
            row[1] = 1.f - light;
        }
    };

    struct Bwd {
        float gd, A, D, sp;
        // sweep 1
        float Lb, Lu, E0, s0;
        bool seen;
        // sweep 2
        float E, Atot, rem;

        __device__ __forceinline__ void init(const float* __restrict__ g) { gd = g[0]; }
        __device__ __forceinline__ void sweep1(float w, float, float z, float d) {
            if (!seen) {
                s0 = z;
                seen = true;
            }
            D += A * (z - sp);
            sp = z;
            Lb += w * D;
            Lu += (w * w) * d;
            E0 += w * (z - s0);
            A += w;
        }
        __device__ __forceinline__ void turn() {
            Atot = A;
            E = E0;
            rem = 2.f * (2.f * Lb + Lu * (1.f / 3.f));
            A = 0.f;
            D = 0.f;
            sp = s0;
        }
        // d L / d w_k and the suffix sum behind k
        __device__ __forceinline__ float sweep2(float w, float light, float z, float d) {
            const float ds = z - sp;                             // (the first sample: sp == s_0, ds == 0)
            sp = z;
            D += A * ds;
            E -= (Atot - A) * ds;
            const float u = 2.f * (D + E) + (2.f / 3.f) * (w * d);
            A += w;
            rem -= w * u;
            return gd * (d * (u * light - rem));
        }
    };
};

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_distortion_workspace_bytes(int64_t Q, int64_t max_samples) { return dm_workspace_bytes(Q, max_samples); }

int svoxt_distortion_fwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                         float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    return raysweep_fwd<Distortion>(tree, rays, opt, nullptr, out, workspace, workspace_bytes, stream, "svoxt_distortion_fwd");
}

int svoxt_distortion_bwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                         const float* grad_out, float* grad, int32_t gstride,
                         void* workspace, int64_t workspace_bytes, void* stream) {
    return raysweep_bwd<Distortion>(tree, rays, opt, nullptr, grad_out, grad, gstride, workspace, workspace_bytes, stream,
                                    "svoxt_distortion_bwd");
}

}  // extern "C"
