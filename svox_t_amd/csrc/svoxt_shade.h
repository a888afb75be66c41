// svoxt_shade.h -- the one statement of shade_samples that svoxt_shade.hip (the plain form and view_basis; DESIGN.md 4.23,
// 4.30) and svoxt_viewrot.hip (per-row rotations) share.  Not part of the public C ABI.
//   device   shade_value, shade_bracket          a channel's value from tmp; the backward's factor t[k, c]
//            view_basis_grad                     the analytic derivative of the basis in the direction it is evaluated at
//            lobes_only, RotDev, Mat3, sh_component
//            TableBasis, RotBasis<BD>            the basis sources: where a sample's basis values come from
//            shade_fwd_kernel<S>                 the forward over a source
//            ShadeValues<S>                      the table backward's value source for the row kernels of svoxt_rowwalk.h
//   host     shade_dims, RotArgs, rot_check, rot_dev
//            shade_fwd_check, shade_bwd_check, shade_partials      the check ladders of the forward and the table backward
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_device.h"
#include "svoxt_host.h"
#include "svoxt_rowwalk.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

// one channel's value from tmp: the backward's pass-1 sig, or tmp itself
__device__ __forceinline__ float shade_value(float tmp, bool activate) {
    return activate ? (float)(1.0 / (1.0 + (double)pexpf(-tmp))) : tmp;
}

// t[k, c] = g * d[k, c], the factor every gradient of shade_samples multiplies by: d = sig * (1 - sig) of the forward's own
// output values[k, c] at `v`, the product in float64 rounded to float32 once; activate == false: g itself, v is not read
__device__ __forceinline__ float shade_bracket(float g, const float* __restrict__ v, bool activate) {
    if (!activate) return g;
    const float sig = *v;
    return g * (float)((double)sig * (1.0 - (double)sig));
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

// ------------------------------------------------------------------------------------------------------ basis sources
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

// A basis source S says where the basis values of a sample (row idx, ray q inside [0, rays())) come from.  It offers
//   kRgba, bd(), rays()                   whether bd() == 0 (RGBA: no basis) can occur; the values a ray has; Q
//   dot(idx, q, f, lo, hi)                the forward's tmp of one channel: from 0.f, i ascending over [lo, hi], B_i * f[i]
//   lane(i), component(lane, k, q, b)     the row kernels' one component i: b = B_i of sample k, false where the sample has
//                                         none; `lane` is the state a lane keeps over the samples of its row
// and is passed by value, as its lane state is.
// basis[q, i] of a per-ray table float32 [Q, bd]; bd at run time, 0 for RGBA
struct TableBasis {
    const float* __restrict__ basis;
    int64_t Q;
    int bd_rt;
    static constexpr bool kRgba = true;
    struct Lane {
        const float* __restrict__ b;       // basis + i
    };
    __device__ __forceinline__ int bd() const { return bd_rt; }
    __device__ __forceinline__ int64_t rays() const { return Q; }
    __device__ __forceinline__ float dot(int64_t, int64_t q, const float* __restrict__ f, int lo, int hi) const {
        const float* __restrict__ b = basis + q * bd_rt;
        float tmp = 0.f;
        for (int i = lo; i <= hi; ++i) tmp += b[i] * f[i];
        return tmp;
    }
    __device__ __forceinline__ Lane lane(int i) const { return Lane{basis + i}; }
    __device__ __forceinline__ bool component(Lane& l, int64_t, int64_t q, float& b) const {
        b = l.b[q * bd_rt];
        return true;
    }
};

// the basis at u = rotations[row[k]] * viewdirs[ray[k]], recomputed by the render kernels' sequence.  BD: the SH basis'
// size at compile time, evaluated once into registers (0: SG / ASG, bd_rt lobes, one at a time)
template <int BD>
struct RotBasis {
    RotDev R;
    const int32_t* __restrict__ row;
    int bd_rt;
    static constexpr bool kRgba = false;
    struct Lane {
        int i;
        Mat3 m;                            // the row's matrix, loaded once at the lane's first sample
        bool have;
    };
    __device__ __forceinline__ int bd() const { return BD > 0 ? BD : bd_rt; }
    __device__ __forceinline__ int64_t rays() const { return R.Q; }
    __device__ __forceinline__ TreeDev lobes() const { return lobes_only(R.extra, R.extra_rows, R.extra_cols); }
    __device__ __forceinline__ float dot(int64_t idx, int64_t q, const float* __restrict__ f, int lo, int hi) const {
        const TreeDev tr = lobes();
        Mat3 m;
        m.load(R.rot, idx, R.d);
        float u0, u1, u2;
        m.apply(R.vdirs + 3 * q, u0, u1, u2);
        float tmp = 0.f;
        if constexpr (BD > 0) {
            float B[BD];
            precalc_basis<BD>(FMT_SH, BD, tr, u0, u1, u2, B);
#pragma unroll
            for (int i = 0; i < BD; ++i)
                if (i >= lo && i <= hi) tmp += B[i] * f[i];
        } else {
            for (int i = lo; i <= hi; ++i) tmp += lobe_value(R.format, tr, u0, u1, u2, i, bd_rt) * f[i];
        }
        return tmp;
    }
    __device__ __forceinline__ Lane lane(int i) const { return Lane{i, Mat3{}, false}; }
    __device__ __forceinline__ bool component(Lane& l, int64_t k, int64_t q, float& b) const {
        if (!l.have) {
            const int64_t idx = row[k];
            if (idx < 0 || idx >= R.M) return false;             // (a plan names no such sample)
            l.m.load(R.rot, idx, R.d);
            l.have = true;
        }
        float u0, u1, u2;
        l.m.apply(R.vdirs + 3 * q, u0, u1, u2);
        if constexpr (BD > 0) b = sh_component<BD>(lobes(), u0, u1, u2, l.i);
        else b = lobe_value(R.format, lobes(), u0, u1, u2, l.i, bd_rt);
        return true;
    }
};

// ------------------------------------------------------------------------------------------------------------ forward
// lane t = k * (C + 1) + c.  c < C: values[k, c]; c == C: sigma[k] (rowgrad_shade_kernel's cut: a sample's lanes read the
// same feature row).  A row outside [0, M) or a ray outside [0, Q): zeros.
template <class S>
__global__ void __launch_bounds__(kLaunchBlock)
shade_fwd_kernel(const float* __restrict__ features, int64_t M, int K, int C, int min_comp, int max_comp, bool activate, S src, int64_t T,
                 const int32_t* __restrict__ row, const int32_t* __restrict__ ray, float* __restrict__ values, float* __restrict__ sigma) {
    const int64_t t = launch_lane();
    const int64_t k = t / (C + 1);
    if (k >= T) return;
    const int c = (int)(t - k * (C + 1));
    const int64_t idx = row[k];
    const bool inside = idx >= 0 && idx < M;
    const float* __restrict__ frow = features + (inside ? idx : 0) * K;
    if (c == C) {
        sigma[k] = inside ? frow[K - 1] : 0.f;
        return;
    }
    float v = 0.f;
    if (inside) {
        if (!S::kRgba || src.bd() > 0) {
            const int64_t q = ray[k];
            if (q >= 0 && q < src.rays()) v = shade_value(src.dot(idx, q, frow + c * src.bd(), min_comp, max_comp), activate);
        } else {
            v = shade_value(frow[c], activate);
        }
    }
    values[k * C + c] = v;
}

// ------------------------------------------------------------------------------------------------------------- values
// The contribution of sample k to column j of its row, for the row kernels of svoxt_rowwalk.h: a colour column
// (g_values[k, c] * d[k, c]) * B_i(k) with B_i from the source S, the sigma column g_sigma[k], every other column 0.f.  sig
// is the forward's own output.  A NULL upstream gradient is zeros: its columns are ZERO columns, nothing is read.  The
// RGBA modes keep their own factor, the float32 product sig * (1.f - sig).
template <class S>
struct ShadeValues {
    const int32_t* __restrict__ ray;
    const float* __restrict__ values;
    const float* __restrict__ gv;
    const float* __restrict__ gs;
    S src;
    int64_t T;
    int K, C, min_comp, max_comp;
    bool activate;
    enum { ZERO, SIGMA, BASIS, BASIS_LINEAR, RGBA, RGBA_LINEAR };
    struct Col {
        const int32_t* __restrict__ ray;
        const float* __restrict__ v;       // BASIS / RGBA: values + c
        const float* __restrict__ g;       // SIGMA: g_sigma;  the colour modes: g_values + c
        S src;
        int64_t T;
        int mode, C;
        mutable typename S::Lane lane;
        __device__ __forceinline__ float at(int64_t k) const {
            if (mode == ZERO || k < 0 || k >= T) return 0.f;
            if (mode == SIGMA) return g[k];
            const float gc = g[k * C];
            if constexpr (S::kRgba) {
                if (mode == RGBA_LINEAR) return gc;
                if (mode == RGBA) {
                    const float sig = v[k * C];
                    return gc * (sig * (1.f - sig));
                }
            }
            const int64_t q = ray[k];
            if (q < 0 || q >= src.rays()) return 0.f;            // (the forward gave this sample zeros)
            float b;
            if (!src.component(lane, k, q, b)) return 0.f;
            return shade_bracket(gc, v + k * C, mode == BASIS) * b;
        }
    };
    __device__ __forceinline__ Col col(int j) const {
        Col o{ray, values, gs, src, T, ZERO, C, src.lane(0)};
        const int bd = src.bd();
        if (j == K - 1) {
            if (gs != nullptr) o.mode = SIGMA;
        } else if (gv == nullptr) {
            // (zeros upstream: every colour column is 0.f)
        } else if (S::kRgba && bd == 0) {
            if (j < C) { o.mode = activate ? RGBA : RGBA_LINEAR; o.v = values + j; o.g = gv + j; }
        } else if (j < C * bd) {
            const int c = j / bd, i = j - c * bd;
            if (i >= min_comp && i <= max_comp) {
                o.mode = activate ? BASIS : BASIS_LINEAR;
                o.v = values + c; o.g = gv + c; o.lane = src.lane(i);
            }
        }
        return o;
    }
};

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

// what the rotated call is given, as the entry points check it: a format with a basis, its lobes, the matrices, the directions
struct RotArgs {
    const float *extra, *rotations, *viewdirs;
    int32_t extra_rows, extra_cols, rot_dim;
};
inline int rot_check(const char* fn, const svoxt_options* opt, const RotArgs& a, int64_t M, int64_t Q) {
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
inline RotDev rot_dev(const svoxt_options* opt, const RotArgs& a, int64_t M, int64_t Q) {
    return RotDev{a.rotations, a.viewdirs, a.extra, M, Q, (int)a.rot_dim, (int)a.extra_rows, (int)a.extra_cols, (int)opt->format};
}

// The forward's checks up to the launch: dims, the view side of a rotated call (`rot`; NULL: the plain call, whose view
// side is `basis`), then for T > 0 the NULLs and the alignment.  The rotated call reads ray wherever there is a colour.
inline int shade_fwd_check(const char* fn, const svoxt_options* opt, const RotArgs* rot, const float* features, int64_t M, int32_t K,
                           const int32_t* row, const int32_t* ray, int64_t T, const float* basis, int64_t Q, const float* values,
                           const float* sigma, int* C, int* bd) {
    int rc;
    if ((rc = shade_dims(opt, M, K, T, Q, C, bd, fn)) || (rot != nullptr && (rc = rot_check(fn, opt, *rot, M, Q)))) return rc;
    if (T == 0) return SVOXT_OK;
    const bool colour = *C > 0;
    if (row == nullptr || sigma == nullptr || (colour && (values == nullptr || (rot != nullptr && ray == nullptr))))
        return fail(SVOXT_ERR_INVALID, rot != nullptr ? "%s: row / ray / values / sigma is NULL" : "%s: row / values / sigma is NULL", fn);
    if (M > 0 && features == nullptr) return fail(SVOXT_ERR_INVALID, "%s: features is NULL", fn);
    if (rot == nullptr && *bd > 0 && colour && (ray == nullptr || (Q > 0 && basis == nullptr)))
        return fail(SVOXT_ERR_INVALID, "%s: ray / basis is NULL", fn);
    if (misaligned(features, 4) || misaligned(row, 4) || misaligned(ray, 4) || misaligned(basis, 4) || misaligned(values, 4) ||
        misaligned(sigma, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    return SVOXT_OK;
}

// The table backward's checks up to the alignment: dims, the view side of a rotated call (`rot` and `row`; NULL: the plain
// call, whose view side is `basis`), the plan's counts, then for M > 0 the NULLs, the plan's long rows and the alignment.
// *grad_values becomes NULL where no colour column exists (nothing of it is read).
inline int shade_bwd_check(const char* fn, const svoxt_options* opt, const RotArgs* rot, const RowPlanRef& plan, int32_t K, const int32_t* row,
                           const int32_t* ray, const float* basis, int64_t Q, int32_t activate, const float* values,
                           const float** grad_values, const float* grad_sigma, const float* grad, const void* workspace, int* C, int* bd) {
    int rc;
    if ((rc = shade_dims(opt, plan.M, K, plan.T, Q, C, bd, fn)) || (rot != nullptr && (rc = rot_check(fn, opt, *rot, plan.M, Q))) ||
        (rc = row_plan_check(fn, plan)))
        return rc;
    if (plan.M == 0) return SVOXT_OK;
    if (grad == nullptr || plan.row_ptr == nullptr) return fail(SVOXT_ERR_INVALID, "%s: grad / row_ptr is NULL", fn);
    if (*C == 0) *grad_values = nullptr;
    const bool reads_values = *grad_values != nullptr && activate != 0;
    const bool reads_basis = *grad_values != nullptr && *bd > 0;
    const bool view_null = ray == nullptr || (rot != nullptr ? row == nullptr : Q > 0 && basis == nullptr);
    if (plan.T > 0 && (plan.perm == nullptr || (reads_values && values == nullptr) || (reads_basis && view_null)))
        return fail(SVOXT_ERR_INVALID, rot != nullptr ? "%s: perm / row / ray / values is NULL" : "%s: perm / values / ray / basis is NULL", fn);
    if ((rc = row_plan_long_check(fn, plan))) return rc;
    if (misaligned(row, 4) || misaligned(ray, 4) || misaligned(basis, 4) || misaligned(values, 4) || misaligned(*grad_values, 4) ||
        misaligned(grad_sigma, 4) || row_plan_misaligned(plan) || misaligned(grad, 4) || misaligned(workspace, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    return SVOXT_OK;
}

// the long rows' partials float32 [n_chunks, cols] of a row reduction, carved from a workspace that is checked where there
// are long rows; `query`: the workspace query as the refusal names it
inline int shade_partials(const char* fn, const RowPlanRef& plan, int cols, void* workspace, int64_t workspace_bytes, const char* query,
                          float** partials) {
    int rc;
    if (plan.n_long > 0 &&
        (rc = workspace_check(fn, workspace, workspace_bytes, svoxt_shade_samples_bwd_workspace_bytes(plan.n_chunks, cols), query)))
        return rc;
    Carver w(workspace);
    *partials = w.take<float>((size_t)plan.n_chunks * (size_t)cols);
    return SVOXT_OK;
}

}  // namespace svoxt
