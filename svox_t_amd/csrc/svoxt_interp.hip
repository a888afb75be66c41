// svoxt_interp.hip -- N3Tree.interp: a trilinear lookup over the leaves around a point, with the gradients with respect
// to the feature table and to the point (the reference has no such operator).  Gather only, a fixed
// float32 order, no float atomic: every result is bit-identical from run to run and to a restatement of
// include/svoxt.h's definition ("interp").
//
//   stencil     a lane per point: query_leaf (svoxt_device.h: the transform, clamp and descent of svoxt_query_fwd, with
//               the descent's digits kept as the leaf's integer cell coordinate c), per axis the side s and the fraction f
//               of the point against the leaf's centre, then for each of the eight corners c + b * s ONE integer descent
//               from the root by the digits of that cell (svoxt_leaf_neighbors' rule), continued through the cell's
//               centre where finer leaves cover it: the leaf the nearest-leaf query reports at the centre of the cell.
//               rows int32 [Q, 8], weights float32 [Q, 8].
//   rows_fwd    out[q, jc] = sum over the eight corners, in ascending corner, of w * table[row, col]: the lanes of a point
//               move its rows together, a contiguous segment of a row per instruction (query_rows' shape), 16 bytes a lane
//               where all K = 4 n columns are taken and table and out are 16-byte aligned.
//   rows_bwd    the gradient with respect to the table: svoxt_reduce_rows' kernels (svoxt_rowwalk.h) over the row plan of
//               `rows` viewed as [8 Q], the value of entry e at column j formed on the fly: weights[e] * g[e >> 3, j].
//               No [8 Q, C] array exists at any point.
//   points_bwd  eight lanes per point: lane j dots the upstream gradient into corner j's row (sequentially in ascending
//               column, four columns a load where K and the alignment allow), the eight dot products meet by cross-lane
//               reads, lanes 0 .. 2 form the derivative along x, y, z.
// C ABI: svoxt_interp_* (include/svoxt.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_rowwalk.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

enum { FILL_SELF = SVOXT_INTERP_FILL_SELF, FILL_ZERO = SVOXT_INTERP_FILL_ZERO };
constexpr int kInterpDeeper = 64;        // levels a corner's descent follows below the query leaf's level before it gives up (no row)

typedef float float4i __attribute__((ext_vector_type(4)));
typedef int int4i __attribute__((ext_vector_type(4)));

// What the stencil of a point is made of: steps 1 and 2 of the definition.
struct InterpPoint {
    int32_t own;                         // the query leaf's feature row, -1 for an empty leaf
    float fx, fy, fz, gx, gy, gz;        // f = |l - 0.5|, g = 1 - f
    int32_t sx, sy, sz;                  // -1 where l < 0.5, else +1
    float cube_sz;                       // N^(d + 1)
    uint32_t cx, cy, cz, side;           // the leaf's cell, cells per axis at its level
    bool cell_ok;
    int d;                               // the leaf's depth
    bool kx, ky, kz;                     // the clamp changed this coordinate
};

template <bool N2>
__device__ __forceinline__ InterpPoint interp_point(const TreeDev& tr, const float* __restrict__ points, int64_t q) {
    InterpPoint ip;
    LeafCell lf;
    float tx, ty, tz;
    query_leaf<N2>(tr, points, q, lf, tx, ty, tz);
    const int32_t idx = tr.data[lf.slot];
    ip.own = (idx >= 0 && (int64_t)idx < tr.M) ? idx : -1;
    const float ux = lf.lx - 0.5f, uy = lf.ly - 0.5f, uz = lf.lz - 0.5f;
    ip.sx = ux < 0.f ? -1 : 1; ip.sy = uy < 0.f ? -1 : 1; ip.sz = uz < 0.f ? -1 : 1;
    ip.fx = fabsf(ux); ip.fy = fabsf(uy); ip.fz = fabsf(uz);
    ip.gx = 1.0f - ip.fx; ip.gy = 1.0f - ip.fy; ip.gz = 1.0f - ip.fz;
    ip.cube_sz = lf.cube_sz;
    ip.cx = lf.cx; ip.cy = lf.cy; ip.cz = lf.cz; ip.side = lf.side; ip.cell_ok = lf.cell_ok;
    ip.d = lf.levels - 1;
    ip.kx = fmaxf(0.f, fminf(kClampHi, tx)) != tx;
    ip.ky = fmaxf(0.f, fminf(kClampHi, ty)) != ty;
    ip.kz = fmaxf(0.f, fminf(kClampHi, tz)) != tz;
    return ip;
}

// Step 4: the feature row of cell (tx, ty, tz) of level d (side = N^(d + 1) cells per axis, all three inside), or -1.
// One descent from the root by the cell's digits; a cell that is still a node after level d is followed through its
// centre: digit N / 2 once and then 0 for an even N, (N - 1) / 2 at every level for an odd one.
template <bool N2>
__device__ __forceinline__ int32_t interp_cell_row(const TreeDev& tr, int32_t n, int d, uint32_t side, uint32_t tx, uint32_t ty, uint32_t tz) {
    const uint32_t N = (uint32_t)tr.N, n3 = N * N * N;
    int32_t node = 0;
    uint32_t pw = N2 ? 0u : side / N;                            // N^(d - l) at level l (generic N)
    uint32_t slot = 0;
    bool leaf = false;
#pragma unroll 1
    for (int l = 0; l <= d; ++l) {
        uint32_t u, v, w;
        if constexpr (N2) {
            const int sh = d - l;
            u = (tx >> sh) & 1u; v = (ty >> sh) & 1u; w = (tz >> sh) & 1u;
        } else {
            u = (tx / pw) % N; v = (ty / pw) % N; w = (tz / pw) % N;
            pw /= N;
        }
        slot = (uint32_t)node * n3 + (u * N + v) * N + w;
        const int32_t ch = tr.child[slot];
        if (ch == 0) { leaf = true; break; }
        node += ch;
        if (node <= 0 || node >= n) return -1;                   // a malformed table
    }
    if (!leaf) {
        uint32_t dg = N / 2u;
#pragma unroll 1
        for (int l = 0; l < kInterpDeeper; ++l) {
            slot = (uint32_t)node * n3 + (dg * N + dg) * N + dg;
            const int32_t ch = tr.child[slot];
            if (ch == 0) { leaf = true; break; }
            node += ch;
            if (node <= 0 || node >= n) return -1;
            if ((N & 1u) == 0u) dg = 0u;
        }
        if (!leaf) return -1;
    }
    const int32_t idx = tr.data[slot];
    return (idx >= 0 && (int64_t)idx < tr.M) ? idx : -1;
}

// ------------------------------------------------------------------------------------------------------------ stencil
// VEC: rows and weights are 16-byte aligned, a point's eight entries leave as two 16-byte stores each.
template <bool N2, bool VEC>
__global__ void __launch_bounds__(kLaunchBlock)
interp_stencil_kernel(TreeDev tr, int32_t n, const float* __restrict__ points, int64_t Q, int fill, int32_t* __restrict__ rows,
                      float* __restrict__ weights) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (q >= Q) return;
    const InterpPoint ip = interp_point<N2>(tr, points, q);
    int32_t r[8];
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int bx = j >> 2, by = (j >> 1) & 1, bz = j & 1;
        w[j] = ((bx ? ip.fx : ip.gx) * (by ? ip.fy : ip.gy)) * (bz ? ip.fz : ip.gz);
        int32_t row = -1;
        if (ip.own >= 0) {
            row = (j == 0 || fill == FILL_SELF) ? ip.own : -1;
            if (j != 0 && ip.cell_ok) {
                const int64_t tx = (int64_t)ip.cx + bx * ip.sx, ty = (int64_t)ip.cy + by * ip.sy, tz = (int64_t)ip.cz + bz * ip.sz;
                const int64_t side = (int64_t)ip.side;
                if (tx >= 0 && tx < side && ty >= 0 && ty < side && tz >= 0 && tz < side) {
                    const int32_t rr = interp_cell_row<N2>(tr, n, ip.d, ip.side, (uint32_t)tx, (uint32_t)ty, (uint32_t)tz);
                    if (rr >= 0) row = rr;
                }
            }
        }
        r[j] = row;
    }
    if constexpr (VEC) {
        int4i* ro = reinterpret_cast<int4i*>(rows + 8 * q);
        float4i* wo = reinterpret_cast<float4i*>(weights + 8 * q);
        ro[0] = int4i{r[0], r[1], r[2], r[3]}; ro[1] = int4i{r[4], r[5], r[6], r[7]};
        wo[0] = float4i{w[0], w[1], w[2], w[3]}; wo[1] = float4i{w[4], w[5], w[6], w[7]};
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { rows[8 * q + j] = r[j]; weights[8 * q + j] = w[j]; }
    }
}

// ----------------------------------------------------------------------------------------------------------- rows_fwd
// Thread t: point t >> lg, lane s = t & (2^lg - 1) of the point's 2^lg lanes; a lane owns the units s, s + 2^lg, ... of
// the point's output row.  V = float4i: a unit is four columns (all K = 4 KU columns, 16-byte aligned table and out);
// V = float: a unit is the selected column cols[u] (or u).
template <typename V>
__global__ void __launch_bounds__(kLaunchBlock)
interp_rows_fwd_kernel(const V* __restrict__ table, int64_t M, int KU, const int32_t* __restrict__ rows, const float* __restrict__ weights,
                       int64_t Q, const int32_t* __restrict__ cols, int CU, int lg, V* __restrict__ out) {
    const int64_t t = launch_lane();
    const int64_t q = t >> lg;
    if (q >= Q) return;
    const int s = (int)(t & ((1 << lg) - 1));
    int32_t r[8];
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int32_t rr = rows[8 * q + j];
        r[j] = (rr >= 0 && (int64_t)rr < M) ? rr : -1;
        w[j] = weights[8 * q + j];
    }
    for (int u = s; u < CU; u += 1 << lg) {
        const int c = cols != nullptr ? cols[u] : u;
        V acc = V(0.f);
        if (c >= 0 && c < KU) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (r[j] >= 0) {
                    const V v = table[(int64_t)r[j] * KU + c];
                    const V p = v * w[j];
                    acc = acc + p;
                }
            }
        }
        out[q * CU + u] = acc;
    }
}

// ----------------------------------------------------------------------------------------------------------- rows_bwd
// The value of entry e = 8 q + j at column jc for the row kernels of svoxt_rowwalk.h: weights[e] * g[q, jc].
struct InterpValues {
    const float* __restrict__ weights;
    const float* __restrict__ g;
    int64_t E;
    int C;
    struct Col {
        const float* __restrict__ w;
        const float* __restrict__ g;     // g + jc
        int64_t E;
        int C;
        __device__ __forceinline__ float at(int64_t e) const { return (e >= 0 && e < E) ? w[e] * g[(e >> 3) * C] : 0.f; }
    };
    __device__ __forceinline__ Col col(int j) const { return Col{weights, g + j, E, C}; }
};

// --------------------------------------------------------------------------------------------------------- points_bwd
// Thread t: point t >> 3, corner j = t & 7.  No lane leaves before the cross-lane reads.  VEC: all K = 4 n columns, table
// and g 16-byte aligned -- a lane reads its row and the point's gradient four columns a load, and adds the four
// products in column order: D_j's sequence is the same.
template <bool N2, bool VEC>
__global__ void __launch_bounds__(kLaunchBlock)
interp_points_bwd_kernel(TreeDev tr, const float* __restrict__ points, int64_t Q, const int32_t* __restrict__ rows,
                         const float* __restrict__ table, int64_t M, int K, const int32_t* __restrict__ cols, int C,
                         const float* __restrict__ g, float* __restrict__ grad_points) {
    const int64_t t = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    const int64_t q = t >> 3;
    const int j = (int)(t & 7);
    const bool live = q < Q;
    float D = 0.f;
    InterpPoint ip = {};
    if (live) {
        const int32_t r = rows[8 * q + j];
        if (r >= 0 && (int64_t)r < M) {
            const float* __restrict__ row = table + (int64_t)r * K;
            const float* __restrict__ gq = g + q * C;
            if constexpr (VEC) {
                const float4i* __restrict__ row4 = reinterpret_cast<const float4i*>(row);
                const float4i* __restrict__ g4 = reinterpret_cast<const float4i*>(gq);
                for (int u = 0; u < (K >> 2); ++u) {
                    const float4i p = g4[u] * row4[u];
                    D = D + p.x; D = D + p.y; D = D + p.z; D = D + p.w;
                }
            } else {
                for (int jc = 0; jc < C; ++jc) {
                    const int c = cols != nullptr ? cols[jc] : jc;
                    if (c >= 0 && c < K) {
                        const float p = gq[jc] * row[c];
                        D = D + p;
                    }
                }
            }
        }
        ip = interp_point<N2>(tr, points, q);
    }
    // the lane's axis a = j (lanes 3 .. 7 of a point compute along and write nothing)
    const int lane0 = (int)(threadIdx.x & 63) & ~7;
    float S = 0.f;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const float Dj = __shfl(D, lane0 + jj, 64);
        const int bx = jj >> 2, by = (jj >> 1) & 1, bz = jj & 1;
        const float mx = bx ? ip.fx : ip.gx, my = by ? ip.fy : ip.gy, mz = bz ? ip.fz : ip.gz;
        float m;
        int b;
        if (j == 0) { m = my * mz; b = bx; }
        else if (j == 1) { m = mx * mz; b = by; }
        else { m = mx * my; b = bz; }
        const float sm = b ? m : -m;
        const float p = sm * Dj;
        S = S + p;
    }
    if (live && j < 3) {
        const float sa = (float)(j == 0 ? ip.sx : (j == 1 ? ip.sy : ip.sz));
        const bool clamped = j == 0 ? ip.kx : (j == 1 ? ip.ky : ip.kz);
        const float v = ((S * sa) * ip.cube_sz) * tr.scaling[j];
        grad_points[3 * q + j] = clamped ? 0.f : v;
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
constexpr int64_t kInterpMaxQ = 0x0fffffffLL;                     // 8 Q < 2^31: the entries e = 8 q + j are int32 in the plan

static int interp_extents_check(int64_t Q, int64_t M, const char* fn) {
    if (Q < 0 || Q > kInterpMaxQ) return fail(SVOXT_ERR_INVALID, "%s: Q must be in [0, 2^28) (8 Q < 2^31)", fn);
    return extent31_check(fn, M, "M");
}

static int interp_cols_check(const int32_t* cols, int32_t n_cols, int32_t K, const char* fn) {
    if (K < 1) return fail(SVOXT_ERR_INVALID, "%s: K must be >= 1", fn);
    return cols_check(fn, cols, n_cols, K);
}
// Q points by C columns, M rows by K
static bool interp_elems_fit(int64_t Q, int C, int64_t M, int K) { return elems_fit((double)Q, C) && elems_fit((double)M, K); }

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int svoxt_interp_stencil(const svoxt_tree* tree, const float* points, int64_t Q, int32_t fill, int32_t* rows, float* weights,
                         void* stream) {
    const char* fn = "svoxt_interp_stencil";
    int rc;
    if ((rc = check_tree(tree, fn))) return rc;
    if (tree->N > 16) return fail(SVOXT_ERR_INVALID, "%s: branching factor N must be in [2, 16]", fn);
    if ((rc = interp_extents_check(Q, tree->M, fn))) return rc;
    if (fill != FILL_SELF && fill != FILL_ZERO) return fail(SVOXT_ERR_INVALID, "%s: fill must be SVOXT_INTERP_FILL_SELF or SVOXT_INTERP_FILL_ZERO", fn);
    if (Q == 0) return SVOXT_OK;
    if (points == nullptr || rows == nullptr || weights == nullptr) return fail(SVOXT_ERR_INVALID, "%s: points / rows / weights is NULL", fn);
    if (misaligned(points, 4) || misaligned(rows, 4) || misaligned(weights, 4)) return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    const TreeDev tr = to_dev(tree);
    const int32_t n = (int32_t)tree->n_internal;
    with_bool(tree->N == 2, [&](auto N2) {
        return with_bool(!misaligned(rows, 16) && !misaligned(weights, 16), [&](auto VEC) {
            hipLaunchKernelGGL((interp_stencil_kernel<N2.value, VEC.value>), dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, tr,
                               n, points, Q, (int)fill, rows, weights);
            return true;
        });
    });
    return check_launch(fn);
}

int svoxt_interp_rows_fwd(const float* table, int64_t M, int32_t K, const int32_t* rows, const float* weights, int64_t Q,
                          const int32_t* cols, int32_t n_cols, float* out, void* stream) {
    const char* fn = "svoxt_interp_rows_fwd";
    int rc;
    if ((rc = interp_extents_check(Q, M, fn)) || (rc = interp_cols_check(cols, n_cols, K, fn))) return rc;
    const int C = cols != nullptr ? n_cols : K;
    if (!interp_elems_fit(Q, C, M, K))
        return fail(SVOXT_ERR_INVALID, "%s: Q * columns and M * K must be below 2^38", fn);
    if (Q == 0) return SVOXT_OK;
    if (rows == nullptr || weights == nullptr || out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: rows / weights / out is NULL", fn);
    if (M > 0 && table == nullptr) return fail(SVOXT_ERR_INVALID, "%s: table is NULL", fn);
    if (misaligned(table, 4) || misaligned(rows, 4) || misaligned(weights, 4) || misaligned(cols, 4) || misaligned(out, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = cols == nullptr && K % 4 == 0 && !misaligned(table, 16) && !misaligned(out, 16);
    const int units = vec ? K / 4 : C;
    int lg = 0;                                                  // lanes per point: the power of two from the units up, 64 at most
    while ((1 << lg) < units && lg < 6) ++lg;
    const dim3 blocks = launch_grid(Q << lg);
    if (vec)
        hipLaunchKernelGGL(interp_rows_fwd_kernel<float4i>, blocks, dim3(kLaunchBlock), 0, st, reinterpret_cast<const float4i*>(table), M,
                           units, rows, weights, Q, (const int32_t*)nullptr, units, lg, reinterpret_cast<float4i*>(out));
    else
        hipLaunchKernelGGL(interp_rows_fwd_kernel<float>, blocks, dim3(kLaunchBlock), 0, st, table, M, (int)K, rows, weights, Q, cols, C,
                           lg, out);
    return check_launch(fn);
}

int64_t svoxt_interp_rows_bwd_workspace_bytes(int64_t n_chunks, int32_t C) {
    if (!in31(n_chunks) || C < 1 || !elems_fit((double)n_chunks, C)) return -1;
    if (n_chunks == 0) return 0;
    return (int64_t)align256(sizeof(float) * (size_t)n_chunks * (size_t)C);
}

int svoxt_interp_rows_bwd(const float* grad_out, const float* weights, int64_t Q, int32_t C, const int32_t* row_ptr,
                          const int32_t* perm, int64_t M, const int32_t* long_rows, const int32_t* long_chunk_ptr,
                          const int32_t* chunk_long, int64_t n_long, int64_t n_chunks, const int32_t* cols, int32_t n_cols,
                          int32_t K, float* grad, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_interp_rows_bwd";
    int rc;
    if ((rc = interp_extents_check(Q, M, fn)) || (rc = interp_cols_check(cols, n_cols, K, fn))) return rc;
    if (C != (cols != nullptr ? n_cols : K))
        return fail(SVOXT_ERR_INVALID, "%s: grad_out must have one column per selected column (C = n_cols, or C = K without cols)", fn);
    if (!interp_elems_fit(Q, C, M, K))
        return fail(SVOXT_ERR_INVALID, "%s: Q * C and M * K must be below 2^38", fn);
    const int64_t T = 8 * Q;
    const RowPlanRef plan{row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, T, M, n_long, n_chunks};
    if ((rc = row_plan_check(fn, plan, "8 Q"))) return rc;
    if (M == 0) return SVOXT_OK;
    if (grad == nullptr || row_ptr == nullptr) return fail(SVOXT_ERR_INVALID, "%s: grad / row_ptr is NULL", fn);
    if (Q > 0 && (grad_out == nullptr || weights == nullptr || perm == nullptr)) return fail(SVOXT_ERR_INVALID, "%s: grad_out / weights / perm is NULL", fn);
    if ((rc = row_plan_long_check(fn, plan))) return rc;
    if (misaligned(grad_out, 4) || misaligned(weights, 4) || row_plan_misaligned(plan) || misaligned(cols, 4) || misaligned(grad, 4) ||
        misaligned(workspace, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    if (n_long > 0 && (rc = workspace_check(fn, workspace, workspace_bytes, svoxt_interp_rows_bwd_workspace_bytes(n_chunks, C),
                                            "svoxt_interp_rows_bwd_workspace_bytes(n_chunks, C)")))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (cols != nullptr && (rc = memset_async(grad, sizeof(float) * (size_t)M * (size_t)K, st, fn))) return rc;     // every element written
    const InterpValues src{weights, grad_out, T, (int)C};
    rows_launch<ROWS_SUM, ROWS_SUM>(src, (int)C, plan, cols, (int)K, 0.f, grad, static_cast<float*>(workspace), st);
    return check_launch(fn);
}

int svoxt_interp_points_bwd(const svoxt_tree* tree, const float* points, int64_t Q, const int32_t* rows, const float* table,
                            int64_t M, int32_t K, const int32_t* cols, int32_t n_cols, const float* grad_out, float* grad_points,
                            void* stream) {
    const char* fn = "svoxt_interp_points_bwd";
    int rc;
    if ((rc = check_tree(tree, fn))) return rc;
    if (tree->N > 16) return fail(SVOXT_ERR_INVALID, "%s: branching factor N must be in [2, 16]", fn);
    if ((rc = interp_extents_check(Q, M, fn)) || (rc = interp_cols_check(cols, n_cols, K, fn))) return rc;
    const int C = cols != nullptr ? n_cols : K;
    if (!interp_elems_fit(Q, C, M, K))
        return fail(SVOXT_ERR_INVALID, "%s: Q * columns and M * K must be below 2^38", fn);
    if (Q == 0) return SVOXT_OK;
    if (points == nullptr || rows == nullptr || grad_out == nullptr || grad_points == nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: points / rows / grad_out / grad_points is NULL", fn);
    if (M > 0 && table == nullptr) return fail(SVOXT_ERR_INVALID, "%s: table is NULL", fn);
    if (misaligned(points, 4) || misaligned(rows, 4) || misaligned(table, 4) || misaligned(cols, 4) || misaligned(grad_out, 4) ||
        misaligned(grad_points, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (4 bytes)", fn);
    const TreeDev tr = to_dev(tree);
    const bool vec = cols == nullptr && K % 4 == 0 && !misaligned(table, 16) && !misaligned(grad_out, 16);
    with_bool(tree->N == 2, [&](auto N2) {
        return with_bool(vec, [&](auto VEC) {
            hipLaunchKernelGGL((interp_points_bwd_kernel<N2.value, VEC.value>), dim3(launch_blocks(8 * Q)), dim3(kLaunchBlock), 0,
                               (hipStream_t)stream, tr, points, Q, rows, table, M, (int)K, cols, C, grad_out, grad_points);
            return true;
        });
    });
    return check_launch(fn);
}

}  // extern "C"
