// svoxt_assign.hip -- write and locate leaves by position: N3Tree.set (a deterministic scatter of point values into the
// feature rows of the points' leaves), the lower corners of leaf slots, and N3Tree.snap (descend, then corner).
// C ABI: svoxt_assign_* / svoxt_leaf_corners / svoxt_snap_points (include/svoxt.h).
//
// The reference has set as assign_vertical (svox_kernel.cu:96-108, 326-343: "if multiple indices point to same leaf
// node, only one of them will be taken", and a write through a null pointer: SURVEY A14) and the corners as a loop of
// masked tensor ops with a host read per level (svox.py:808-826).  Here:
//
// locate     a lane per point: query_locate (svoxt_device.h: the transform, clamp and descent of svoxt_query_fwd), the
//            point's feature ROW or none (a data word that is no row of the table: an empty leaf).  Points are grouped
//            by row, not by slot: slots that share a row (refine, merge, quantize) form one group.
// "last"     winner[row] = max point index, an integer atomicMax: exact, independent of the order of arrival.  Then a
//            copy kernel, lanes across the columns of a point's row (16 bytes a lane where K % 4 == 0): only the
//            winner of a row writes it.  No sort.
// others     stable LSD radix sort (svoxt_sort.h) of (row, point index) over the bits the number M needs -- points
//            without a row carry the key M and end up behind all groups -- so a group's points lie together in
//            ASCENDING POINT INDEX.  Heads of groups flag themselves (key differs from the one before), an exclusive
//            scan ranks them, an emit kernel lists them: heads[u] = sorted position of group u, u ascending in the row.
//            The reduce kernel gives a group to K / 4 (or K) lanes, each walking the group's points in that order with
//            its own columns: acc = first row, then acc = acc + x / x > acc ? x : acc / x < acc ? x : acc, sequential
//            float32, no fused multiply-add; mean divides the sum once by float(count).  The order is part of the
//            contract (tests compare bits).  A group is walked by ONE set of lanes: a single group of L points costs L
//            dependent iterations of one row load each, whatever the size of the rest (DESIGN.md 4.13 has the
//            measurement) -- the price of a fixed order; a tree-shaped sum would be another number.
// counts     row_count[row] += 1 per located point, integer atomics (optional output).
// corners    a lane per leaf slot walks parent_depth[:, 0] up to the root: corner = (corner + xyz) / N per level, the
//            operations and the order of N3Tree._calc_corners' torch walk, IEEE divide: the same bits.
// Every output is a function of the inputs: two runs give the same bytes.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_sort.h"
#include "svoxt_workspace.h"

namespace svoxt {

constexpr int kAssignBlock = kLaunchBlock;
static_assert(kAssignBlock == kLaunchBlock, "assign_copy_kernel and assign_reduce_kernel index by launch_lane()");
constexpr int kMaxWalk = 128;            // levels a corner walk follows before it gives up (NaN): a malformed table
enum { AS_LAST = SVOXT_ASSIGN_LAST, AS_SUM = SVOXT_ASSIGN_SUM, AS_MEAN = SVOXT_ASSIGN_MEAN, AS_MAX = SVOXT_ASSIGN_MAX,
       AS_MIN = SVOXT_ASSIGN_MIN };

typedef float float4a __attribute__((ext_vector_type(4)));

// workspace of "last": [row i32[Q]] [winner i32[M]]
// of the others:       [keys u32[Q + 1]] x 2 [vals u32[Q + 1]] x 2 [counts] [starts] [chunk sums] [heads u32[Q]]; after
//                      the sort the pair of buffers it did not end in serves as the head flags and their ranks
struct AssignSpace {
    int32_t *row, *winner;
    uint32_t *keys[2], *vals[2], *counts, *starts, *chunks, *heads;
    size_t bytes;
};

static AssignSpace assign_carve(void* workspace, int64_t Q, int64_t M, int32_t reduce) {
    AssignSpace sp = {};
    Carver w(workspace);
    if (reduce == AS_LAST) {
        sp.row = w.take<int32_t>((size_t)Q);
        sp.winner = w.take<int32_t>((size_t)M);
    } else {
        const size_t cc = (size_t)256 * sort_blocks((uint64_t)Q);
        for (int i = 0; i < 2; ++i) sp.keys[i] = w.take<uint32_t>((size_t)Q + 1);
        for (int i = 0; i < 2; ++i) sp.vals[i] = w.take<uint32_t>((size_t)Q + 1);
        sp.counts = w.take<uint32_t>(cc);
        sp.starts = w.take<uint32_t>(cc);
        sp.chunks = w.take<uint32_t>(exclusive_scan_chunks(cc > (size_t)Q + 1 ? cc : (size_t)Q + 1));
        sp.heads = w.take<uint32_t>((size_t)Q + 1);            // (Q words are used: the piece is as long as the keys')
    }
    sp.bytes = w.bytes() + 256;
    return sp;
}

// ------------------------------------------------------------------------------------------------------------ locate
// SORT: keys[q] = the point's row, or M without one.  Else: row[q] = the row or -1, winner[row] = max(winner[row], q).
template <bool N2, bool SORT>
__global__ void __launch_bounds__(kAssignBlock)
assign_locate_kernel(TreeDev tr, const float* __restrict__ points, int64_t Q, int32_t* __restrict__ row, int32_t* __restrict__ winner,
                     uint32_t* __restrict__ keys, int32_t* __restrict__ row_count) {
    const int64_t q = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (q >= Q) return;
    uint32_t slot;
    const int32_t r = query_locate<N2>(tr, points, q, slot);       // in [0, M), or -1
    if constexpr (SORT) {
        keys[q] = r >= 0 ? (uint32_t)r : (uint32_t)tr.M;
    } else {
        row[q] = r;
        if (r >= 0) atomicMax(winner + r, (int32_t)q);
    }
    if (r >= 0 && row_count != nullptr) atomicAdd(row_count + r, 1);
}

// "last": the lanes of point q copy its values into its row if q is the row's winner.  V: float4a (lpr = K / 4) or float.
template <typename V>
__global__ void __launch_bounds__(kAssignBlock)
assign_copy_kernel(const int32_t* __restrict__ row, const int32_t* __restrict__ winner, int64_t Q, int lpr,
                   const V* __restrict__ values, V* __restrict__ table) {
    const int64_t t = launch_lane();
    const int64_t q = t / lpr;
    const int j = (int)(t - q * lpr);
    if (q >= Q) return;
    const int32_t r = row[q];
    if (r < 0 || (int64_t)winner[r] != q) return;
    table[(int64_t)r * lpr + j] = values[q * lpr + j];
}

// ------------------------------------------------------------------------------------------------- heads of the groups
// flag[i] = 1 where sorted position i starts a group with a row (i in [0, Q]; flag[Q] = 0: the scan reads Q + 1 words)
__global__ void __launch_bounds__(kAssignBlock)
assign_flag_kernel(const uint32_t* __restrict__ keys, int64_t Q, uint32_t M, uint32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (i > Q) return;
    bool head = false;
    if (i < Q) {
        const uint32_t k = keys[i];
        head = k < M && (i == 0 || keys[i - 1] != k);
    }
    flag[i] = head ? 1u : 0u;
}

// ------------------------------------------------------------------------------------------------------------ reduce
template <typename V>
__device__ __forceinline__ V assign_pick(V x, V acc, bool is_max);
template <>
__device__ __forceinline__ float assign_pick<float>(float x, float acc, bool is_max) {
    return (is_max ? x > acc : x < acc) ? x : acc;                 // strict: the first point that attains the extremum stays
}
template <>
__device__ __forceinline__ float4a assign_pick<float4a>(float4a x, float4a acc, bool is_max) {
    float4a r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = assign_pick<float>(x[e], acc[e], is_max);
    return r;
}

// Group g (< U = rank[Q]) belongs to lpr consecutive lanes; lane j owns element j of the row (V: 4 columns or 1) and walks
// the group's points in sorted order = ascending point index.
template <typename V>
__global__ void __launch_bounds__(kAssignBlock)
assign_reduce_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ heads,
                     const uint32_t* __restrict__ rank, int64_t Q, uint32_t M, int lpr, int op, const V* __restrict__ values,
                     V* __restrict__ table) {
    const int64_t t = launch_lane();
    const int64_t g = t / lpr;
    const int j = (int)(t - g * lpr);
    if (g >= (int64_t)rank[Q]) return;
    int64_t i = heads[g];
    if (i >= Q) return;                                            // (never: heads hold sorted positions)
    const uint32_t key = keys[i];
    if (key >= M) return;                                          // (never: only groups with a row are flagged)
    const uint32_t p0 = vals[i];
    V acc = values[(int64_t)p0 * lpr + j];
    int count = 1;
    for (++i; i < Q && keys[i] == key; ++i) {
        const V x = values[(int64_t)vals[i] * lpr + j];
        if (op == AS_SUM || op == AS_MEAN) acc = acc + x;
        else acc = assign_pick<V>(x, acc, op == AS_MAX);
        ++count;
    }
    if (op == AS_MEAN) acc = acc / (float)count;
    table[(int64_t)key * lpr + j] = acc;
}

// ----------------------------------------------------------------------------------------------------------- corners
// Lower corner in [0, 1]^3 of slot (node, x, y, z): N3Tree._calc_corners' walk.  NaN for a slot or a table out of range.
__device__ __forceinline__ void corner_walk(const int32_t* __restrict__ parent_depth, int64_t n, int32_t N, int64_t node, int32_t x,
                                            int32_t y, int32_t z, float c[3]) {
    const float Nf = (float)N, bad = __int_as_float(0x7fc00000);
    const int32_t n3 = N * N * N;
    c[0] = c[1] = c[2] = 0.f;
    if (node < 0 || node >= n || x < 0 || x >= N || y < 0 || y >= N || z < 0 || z >= N) { c[0] = c[1] = c[2] = bad; return; }
#pragma unroll 1
    for (int lvl = 0; lvl < kMaxWalk; ++lvl) {
        c[0] = (c[0] + (float)x) / Nf;
        c[1] = (c[1] + (float)y) / Nf;
        c[2] = (c[2] + (float)z) / Nf;
        if (node == 0) return;
        const int32_t packed = parent_depth[2 * node];
        const int32_t up = packed / n3;
        if (packed < 0 || up >= n) break;
        int32_t rem = packed - up * n3;
        z = rem % N; rem /= N;
        y = rem % N;
        x = rem / N;
        node = up;
    }
    c[0] = c[1] = c[2] = bad;
}

__global__ void __launch_bounds__(kAssignBlock)
leaf_corners_kernel(const int32_t* __restrict__ parent_depth, int64_t n, int32_t N, const int64_t* __restrict__ leaf_node, int64_t Q,
                    float* __restrict__ corners) {
    const int64_t q = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (q >= Q) return;
    const int64_t* l = leaf_node + 4 * q;
    const int64_t node = l[0], x = l[1], y = l[2], z = l[3];
    const bool ok = x >= 0 && x < N && y >= 0 && y < N && z >= 0 && z < N;
    float c[3];
    corner_walk(parent_depth, n, N, ok ? node : -1, (int32_t)(ok ? x : 0), (int32_t)(ok ? y : 0), (int32_t)(ok ? z : 0), c);
    corners[3 * q] = c[0]; corners[3 * q + 1] = c[1]; corners[3 * q + 2] = c[2];
}

// descend, then corner, then back through the transform the points came in by: (corner - offset) / scaling
template <bool N2>
__global__ void __launch_bounds__(kAssignBlock)
snap_kernel(TreeDev tr, const int32_t* __restrict__ parent_depth, int64_t n, const float* __restrict__ points, int64_t Q,
            float* __restrict__ corners) {
    const int64_t q = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (q >= Q) return;
    uint32_t slot;
    query_locate<N2>(tr, points, q, slot);
    const uint32_t N = (uint32_t)tr.N;
    const int32_t z = (int32_t)(slot % N), y = (int32_t)((slot / N) % N), x = (int32_t)((slot / (N * N)) % N);
    float c[3];
    corner_walk(parent_depth, n, tr.N, (int64_t)(slot / (N * N * N)), x, y, z, c);
#pragma unroll
    for (int a = 0; a < 3; ++a) corners[3 * q + a] = (c[a] - tr.offset[a]) / tr.scaling[a];
}

static bool aligned16(const void* a, const void* b) { return (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0; }

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_assign_workspace_bytes(int64_t Q, int64_t M, int32_t reduce) {
    if (Q < 0 || Q >= 0x7fffffff || M < 0 || M >= 0x7fffffff || reduce < AS_LAST || reduce > AS_MIN) return -1;
    return (int64_t)assign_carve(nullptr, Q, M, reduce).bytes;
}

int svoxt_assign_leaves(const svoxt_tree* tree, const float* points, int64_t Q, const float* values, int32_t reduce, float* table,
                        int32_t* row_count, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_assign_leaves";
    int rc;
    if ((rc = check_tree(tree, fn))) return rc;
    if (reduce < AS_LAST || reduce > AS_MIN)
        return set_error(SVOXT_ERR_INVALID, "%s: reduce must be one of SVOXT_ASSIGN_LAST / SUM / MEAN / MAX / MIN", fn);
    if (Q < 0 || Q >= 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the number of points must be in [0, 2^31 - 1)", fn);
    if (tree->M >= 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the number of feature rows must be below 2^31 - 1", fn);
    if ((double)Q * tree->K >= 274877906944.0) return set_error(SVOXT_ERR_INVALID, "%s: Q * K must be below 2^38", fn);
    const int64_t M = tree->M;
    const int K = tree->K;
    if (M > 0 && table == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: table is NULL", fn);
    if (Q > 0 && (points == nullptr || values == nullptr)) return set_error(SVOXT_ERR_INVALID, "%s: points / values is NULL", fn);
    if (Q > 0 && M > 0) {
        if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_assign_workspace_bytes(Q, M, reduce),
                                  "svoxt_assign_workspace_bytes(Q, M, reduce)")))
            return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (row_count != nullptr && M > 0) {
        e = hipMemsetAsync(row_count, 0, sizeof(int32_t) * (size_t)M, st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    }
    if (Q == 0 || M == 0) return SVOXT_OK;
    const AssignSpace sp = assign_carve(workspace, Q, M, reduce);
    const TreeDev tr = to_dev(tree);
    const bool n2 = tree->N == 2, vec = K % 4 == 0 && aligned16(values, table);
    const int lpr = vec ? K / 4 : K;
    if (reduce == AS_LAST) {
        e = hipMemsetAsync(sp.winner, 0xff, sizeof(int32_t) * (size_t)M, st);        // -1: below every point index
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
        hipLaunchKernelGGL((n2 ? assign_locate_kernel<true, false> : assign_locate_kernel<false, false>), dim3(launch_blocks(Q)),
                           dim3(kAssignBlock), 0, st, tr, points, Q, sp.row, sp.winner, (uint32_t*)nullptr, row_count);
        if ((rc = check_launch(fn))) return rc;
        const dim3 grid = launch_grid(Q * lpr);
        if (vec)
            hipLaunchKernelGGL(assign_copy_kernel<float4a>, grid, dim3(kAssignBlock), 0, st, sp.row, sp.winner, Q, lpr,
                               reinterpret_cast<const float4a*>(values), reinterpret_cast<float4a*>(table));
        else
            hipLaunchKernelGGL(assign_copy_kernel<float>, grid, dim3(kAssignBlock), 0, st, sp.row, sp.winner, Q, lpr, values, table);
        return check_launch(fn);
    }
    hipLaunchKernelGGL((n2 ? assign_locate_kernel<true, true> : assign_locate_kernel<false, true>), dim3(launch_blocks(Q)),
                       dim3(kAssignBlock), 0, st, tr, points, Q, (int32_t*)nullptr, (int32_t*)nullptr, sp.keys[0], row_count);
    if ((rc = check_launch(fn))) return rc;
    // the keys are in [0, M]: sort over the bits of M, in passes of at most 8 bits, all of (nearly) the same width
    int bits = 0;
    while (((uint64_t)M >> bits) != 0) ++bits;
    const int passes = (bits + 7) / 8, per = (bits + passes - 1) / passes;
    int cur = 0;
    for (int p = 0, shift = 0; p < passes; ++p, shift += per) {
        const int b = bits - shift < per ? bits - shift : per;
        if ((rc = sort_pass(sp.keys[cur], p == 0 ? nullptr : sp.vals[cur], (uint32_t)Q, shift, b, sp.counts, sp.starts, sp.chunks,
                            sp.keys[cur ^ 1], sp.vals[cur ^ 1], st, fn)))
            return rc;
        cur ^= 1;
    }
    uint32_t *flag = sp.keys[cur ^ 1], *rank = sp.vals[cur ^ 1];
    hipLaunchKernelGGL(assign_flag_kernel, dim3(launch_blocks(Q + 1)), dim3(kAssignBlock), 0, st, sp.keys[cur], Q, (uint32_t)M, flag);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(flag, (size_t)Q + 1, sp.chunks, rank, st, fn))) return rc;
    hipLaunchKernelGGL(scatter_ranked_kernel<uint32_t>, dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, st, flag, rank, Q, Q, sp.heads);
    if ((rc = check_launch(fn))) return rc;
    const int64_t groups = Q < M ? Q : M;                          // an upper bound: the kernel reads the number itself
    const dim3 grid = launch_grid(groups * lpr);
    if (vec)
        hipLaunchKernelGGL(assign_reduce_kernel<float4a>, grid, dim3(kAssignBlock), 0, st, sp.keys[cur], sp.vals[cur], sp.heads, rank, Q,
                           (uint32_t)M, lpr, (int)reduce, reinterpret_cast<const float4a*>(values), reinterpret_cast<float4a*>(table));
    else
        hipLaunchKernelGGL(assign_reduce_kernel<float>, grid, dim3(kAssignBlock), 0, st, sp.keys[cur], sp.vals[cur], sp.heads, rank, Q,
                           (uint32_t)M, lpr, (int)reduce, values, table);
    return check_launch(fn);
}

int svoxt_leaf_corners(const int32_t* parent_depth, int64_t n_internal, int32_t N, const int64_t* leaf_node, int64_t Q,
                       float* corners, void* stream) {
    const char* fn = "svoxt_leaf_corners";
    int rc;
    if ((rc = tree_extents_check(fn, n_internal, N, 0))) return rc;
    if (Q < 0 || Q >= (int64_t)kAssignBlock * 2147483647LL) return set_error(SVOXT_ERR_INVALID, "%s: bad leaf count", fn);
    if (Q == 0) return SVOXT_OK;
    if (parent_depth == nullptr || leaf_node == nullptr || corners == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: parent_depth / leaf_node / corners is NULL", fn);
    hipLaunchKernelGGL(leaf_corners_kernel, dim3(launch_blocks(Q)), dim3(kAssignBlock), 0, (hipStream_t)stream, parent_depth, n_internal, N,
                       leaf_node, Q, corners);
    return check_launch(fn);
}

int svoxt_snap_points(const svoxt_tree* tree, const int32_t* parent_depth, const float* points, int64_t Q, float* corners,
                      void* stream) {
    const char* fn = "svoxt_snap_points";
    int rc;
    if ((rc = check_tree(tree, fn))) return rc;
    if (tree->N > 16) return set_error(SVOXT_ERR_INVALID, "%s: branching factor N must be in [2, 16]", fn);
    if (Q < 0 || Q >= (int64_t)kAssignBlock * 2147483647LL) return set_error(SVOXT_ERR_INVALID, "%s: bad point count", fn);
    if (Q == 0) return SVOXT_OK;
    if (parent_depth == nullptr || points == nullptr || corners == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: parent_depth / points / corners is NULL", fn);
    hipLaunchKernelGGL(tree->N == 2 ? snap_kernel<true> : snap_kernel<false>, dim3(launch_blocks(Q)), dim3(kAssignBlock), 0,
                       (hipStream_t)stream, to_dev(tree), parent_depth, tree->n_internal, points, Q, corners);
    return check_launch(fn);
}

}  // extern "C"
