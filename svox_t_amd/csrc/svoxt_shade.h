// svoxt_shade.h -- what svoxt_shade.hip (shade_samples, view_basis) and svoxt_viewrot.hip
// (shade_samples with per-row rotations) share: a channel's value, the analytic derivative of the basis in
// the direction it is evaluated at, and the check of a table's extents.  Not part of the public C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_device.h"
#include "svoxt_host.h"

#pragma clang fp contract(off)

namespace svoxt {

// one channel's value from tmp: the backward's pass-1 sig, or tmp itself
__device__ __forceinline__ float shade_value(float tmp, bool activate) {
    return activate ? (float)(1.0 / (1.0 + (double)pexpf(-tmp))) : tmp;
}

// (gx, gy, gz) = sum over i ascending of gb(i) * d out_i / d (x, y, z), the analytic derivative of the expression
// precalc_basis evaluates at (x, y, z), in the three components as given (include/svoxt.h, svoxt_view_basis_bwd, states
// the sequence).  A partial that is identically zero is not added.  gb(i): the upstream gradient of component i, asked
// for at compile-time indices guarded by bd (the lobes of SG / ASG one at a time); b(i): the forward's value of lobe i,
// asked for by SG alone.  No private array, nothing in scratch.
#define SVOXT_VB_ADD(gi, dx, dy, dz) do { const float g = (gi); gx += g * (dx); gy += g * (dy); gz += g * (dz); } while (0)
template <class G, class B>
__device__ __forceinline__ void view_basis_grad(const TreeDev& tr, int format, int bd, float x, float y, float z, const G& gb, const B& b,
                                                float& gx, float& gy, float& gz) {
    gx = 0.f; gy = 0.f; gz = 0.f;
    if (format == FMT_SH) {
        const float xx = x * x, yy = y * y, zz = z * z;
        const float xy = x * y, yz = y * z, xz = x * z;
        if (bd == 25 || bd == 16 || bd == 9 || bd == 4) {
            gy += gb(1) * -kC1;
            gz += gb(2) * kC1;
            gx += gb(3) * -kC1;
        }
        if (bd == 25 || bd == 16 || bd == 9) {
            { const float g = gb(4); gx += g * (kC2[0] * y); gy += g * (kC2[0] * x); }
            { const float g = gb(5); gy += g * (kC2[1] * z); gz += g * (kC2[1] * y); }
            SVOXT_VB_ADD(gb(6), kC2[2] * (-2.f * x), kC2[2] * (-2.f * y), kC2[2] * (4.f * z));
            { const float g = gb(7); gx += g * (kC2[3] * z); gz += g * (kC2[3] * x); }
            { const float g = gb(8); gx += g * (kC2[4] * (2.f * x)); gy += g * (kC2[4] * (-2.f * y)); }
        }
        if (bd == 25 || bd == 16) {
            const float a = 3.f * xx - 3.f * yy;
            { const float g = gb(9); gx += g * (kC3[0] * (6.f * xy)); gy += g * (kC3[0] * a); }
            SVOXT_VB_ADD(gb(10), kC3[1] * yz, kC3[1] * xz, kC3[1] * xy);
            SVOXT_VB_ADD(gb(11), kC3[2] * (-2.f * xy), kC3[2] * (4.f * zz - xx - 3.f * yy), kC3[2] * (8.f * yz));
            SVOXT_VB_ADD(gb(12), kC3[3] * (-6.f * xz), kC3[3] * (-6.f * yz), kC3[3] * (6.f * zz - 3.f * xx - 3.f * yy));
            SVOXT_VB_ADD(gb(13), kC3[4] * (4.f * zz - 3.f * xx - yy), kC3[4] * (-2.f * xy), kC3[4] * (8.f * xz));
            SVOXT_VB_ADD(gb(14), kC3[5] * (2.f * xz), kC3[5] * (-2.f * yz), kC3[5] * (xx - yy));
            { const float g = gb(15); gx += g * (kC3[6] * a); gy += g * (kC3[6] * (-6.f * xy)); }
        }
        if (bd == 25) {
            const float a = 3.f * xx - 3.f * yy;                 // (as above)
            const float p = 3.f * xx - yy, m = xx - 3.f * yy;
            const float s1 = 7.f * zz - 1.f, s3 = 7.f * zz - 3.f, t3 = 21.f * zz - 3.f;
            { const float g = gb(16); gx += g * (kC4[0] * (y * p)); gy += g * (kC4[0] * (x * m)); }
            SVOXT_VB_ADD(gb(17), kC4[1] * ((6.f * xy) * z), kC4[1] * (z * a), kC4[1] * (y * p));
            SVOXT_VB_ADD(gb(18), kC4[2] * (y * s1), kC4[2] * (x * s1), kC4[2] * ((14.f * xy) * z));
            { const float g = gb(19); gy += g * (kC4[3] * (z * s3)); gz += g * (kC4[3] * (y * t3)); }
            gz += gb(20) * (kC4[4] * (z * (140.f * zz - 60.f)));
            { const float g = gb(21); gx += g * (kC4[5] * (z * s3)); gz += g * (kC4[5] * (x * t3)); }
            SVOXT_VB_ADD(gb(22), kC4[6] * ((2.f * x) * s1), kC4[6] * ((-2.f * y) * s1), kC4[6] * ((xx - yy) * (14.f * z)));
            SVOXT_VB_ADD(gb(23), kC4[7] * (z * a), kC4[7] * ((-6.f * xy) * z), kC4[7] * (x * m));
            { const float g = gb(24); gx += g * (kC4[8] * (x * (4.f * xx - 12.f * yy))); gy += g * (kC4[8] * (y * (4.f * yy - 12.f * xx))); }
        }
    } else if (format == FMT_SG) {
        for (int i = 0; i < bd; ++i) {
            const float* lobe = tr.extra + (int64_t)i * tr.extra_cols;
            const float s = b(i) * lobe[0];                      // (the forward's own value: no exponential here)
            SVOXT_VB_ADD(gb(i), s * lobe[1], s * lobe[2], s * lobe[3]);
        }
    } else if (format == FMT_ASG) {
        const float dir[3] = {x, y, z};
        for (int i = 0; i < bd; ++i) {
            const float* lobe = tr.extra + (int64_t)i * tr.extra_cols;
            const float S = dot3(dir, lobe + 8);
            const float dot_x = dot3(dir, lobe + 2);
            const float dot_y = dot3(dir, lobe + 5);
            const float E = pexpf(-lobe[0] * dot_x * dot_x - lobe[1] * dot_y * dot_y);     // (the forward's sequence)
            const float SE = S * E;
            const float cx = (-2.f * lobe[0]) * dot_x, cy = (-2.f * lobe[1]) * dot_y;
            const float n = (float)bd;
            SVOXT_VB_ADD(gb(i), (lobe[8] * E + SE * (cx * lobe[2] + cy * lobe[5])) / n,
                         (lobe[9] * E + SE * (cx * lobe[3] + cy * lobe[6])) / n,
                         (lobe[10] * E + SE * (cx * lobe[4] + cy * lobe[7])) / n);
        }
    }
}
#undef SVOXT_VB_ADD

// C and the basis values a ray has (0 for RGBA) for a table of K columns; what every direction of shade_samples checks first
inline int shade_dims(const svoxt_options* opt, int64_t M, int32_t K, int64_t T, int64_t Q, int* C, int* bd, const char* fn) {
    if (opt == nullptr) return fail(SVOXT_ERR_INVALID, "%s: options is NULL", fn);
    if (opt->format < SVOXT_FORMAT_RGBA || opt->format > SVOXT_FORMAT_ASG) return fail(SVOXT_ERR_INVALID, "%s: unknown data format", fn);
    if (K < 1) return fail(SVOXT_ERR_INVALID, "%s: K must be >= 1", fn);
    int rc;
    if ((rc = extent31_check(fn, T, "T")) || (rc = extent31_check(fn, M, "M")) || (rc = extent31_check(fn, Q, "Q"))) return rc;
    if (opt->format == SVOXT_FORMAT_RGBA) {
        *bd = 0;
        *C = K - 1;
    } else {
        if (opt->basis_dim < 1 || opt->basis_dim > 25) return fail(SVOXT_ERR_INVALID, "%s: basis_dim must be in [1, 25]", fn);
        if (opt->min_comp < 0 || opt->max_comp >= opt->basis_dim)
            return fail(SVOXT_ERR_INVALID, "%s: min_comp / max_comp outside [0, basis_dim)", fn);
        *bd = opt->basis_dim;
        *C = (K - 1) / opt->basis_dim;
    }
    if (!elems_fit((double)T, *C + 1) || !elems_fit((double)M, K))
        return fail(SVOXT_ERR_INVALID, "%s: T * (C + 1) and M * K must be below 2^38", fn);
    return SVOXT_OK;
}

}  // namespace svoxt
