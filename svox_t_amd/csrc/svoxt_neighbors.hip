// svoxt_neighbors.hip -- which leaves touch which, and the smoothness loss built on it: N3Tree.leaf_neighbors (the
// face neighbour of every leaf across each of its six faces), the cached edge plan (every pair of face-adjacent leaves
// once, grouped by feature row) and N3Tree.tv / tv_add_grad (a total-variation loss over those pairs and its gradient
// as ONE gather-only kernel over feature rows).  The reference has none of this.
// C ABI: svoxt_neighbors_* / svoxt_leaf_neighbors / svoxt_tv_* (include/svoxt.h).
//
// neighbours  integer work only.  flag = (child == 0) per slot, exclusive scan: a leaf slot's LEAF INDEX (its place in
//             _all_leaves() order).  Then a thread per leaf slot: walk parent_depth[:, 0] to the root collecting the
//             base-N digits of its cell coordinate c in [0, N^(d + 1))^3, and for each face (-x +x -y +y -z +z) descend
//             from the root along the digits of c +- e_a, never below the leaf's own level d: the first leaf met is the
//             neighbour (same size or coarser); -1 outside the cube; -2 where the cell is still a node after level d.
// plan        mark (a slot (i, k) of the table is an EDGE: neighbour j >= 0, coarser or -- at equal depth -- on a +
//             face, both leaves name a row, the rows differ) -> scan -> the host reads E -> fill (two incidences per
//             edge, keyed by the owning row, in ascending incidence id) -> stable radix sort by row (svoxt_sort.h) ->
//             emit other[] / meta[] in sorted order and row_ptr[] by a binary search per row.  A CSR over feature rows.
// tv          tv_rows_kernel, a lane per (row, selected column): reads f[r, c] once, walks the row's incidences in
//             ascending id with one gathered f[other, c] each, accumulates the gradient entry and -- over the + (even)
//             incidences only, so every edge counts once -- the loss, sequentially in float32, no fused multiply-add.
//             No atomics anywhere: the per-lane loss sums meet in a fixed-shape tree per workgroup of 256 lanes
//             (v[i] += v[i + s], s = 128 .. 1), the workgroups' sums in tv_loss_kernel: lane i adds the partial sums
//             i, i + 256, ... in that order, then the same tree.  The order is part of the definition (tests compare
//             bits).  A row is walked by ONE lane per column: a row shared by L leaves costs on the order of L
//             dependent steps, whatever the rest of the table looks like.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_sort.h"
#include "svoxt_workspace.h"

namespace svoxt {

constexpr int kNbBlock = kLaunchBlock;       // (the per-slot passes stride over the slots: stride_blocks)
constexpr int kTvBlock = 256;                // the loss tree's shape: part of the definition
enum { TV_LOSS = SVOXT_TV_LOSS, TV_LOSS_GRAD = SVOXT_TV_LOSS_GRAD, TV_ACCUMULATE = SVOXT_TV_ACCUMULATE };

// workspace of leaf_neighbors: [flag u32[slots + 1]] [rank u32[slots + 1]] [chunk sums]
struct NbSpace {
    uint32_t *flag, *rank, *chunks;
    size_t bytes;
};
static NbSpace nb_carve(void* workspace, int64_t slots) {
    NbSpace sp;
    Carver w(workspace);
    sp.flag = w.take<uint32_t>((size_t)slots + 1);
    sp.rank = w.take<uint32_t>((size_t)slots + 1);
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks((size_t)slots + 1));
    sp.bytes = w.bytes();
    return sp;
}

// the marks of the plan (svoxt_tv_plan_count writes, svoxt_tv_plan_emit reads): [flag u32[6 L + 1]] [rank] [chunk sums]
static NbSpace marks_carve(void* workspace, int64_t L) { return nb_carve(workspace, 6 * L); }

// the sort space of svoxt_tv_plan_emit: [keys u32[2 E]] x 2 [vals u32[2 E]] x 2 [counts] [starts] [chunk sums] [list u32[E]]
struct PlanSpace {
    uint32_t *keys[2], *vals[2], *counts, *starts, *chunks, *list;
    size_t bytes;
};
static PlanSpace plan_carve(void* workspace, int64_t E) {
    PlanSpace sp;
    Carver w(workspace);
    const size_t cc = (size_t)256 * sort_blocks(2 * (uint64_t)E);
    for (int i = 0; i < 2; ++i) sp.keys[i] = w.take<uint32_t>(2 * (size_t)E);
    for (int i = 0; i < 2; ++i) sp.vals[i] = w.take<uint32_t>(2 * (size_t)E);
    sp.counts = w.take<uint32_t>(cc);
    sp.starts = w.take<uint32_t>(cc);
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks(cc));
    sp.list = w.take<uint32_t>((size_t)E);
    sp.bytes = w.bytes() + 256;
    return sp;
}

// --------------------------------------------------------------------------------------------------------- neighbours
__global__ void __launch_bounds__(kNbBlock)
leaf_flag_kernel(const int32_t* __restrict__ child, int32_t slots, uint32_t* __restrict__ flag) {
    for (int64_t s = (int64_t)blockIdx.x * kNbBlock + threadIdx.x; s <= slots; s += (int64_t)gridDim.x * kNbBlock)
        flag[s] = (s < slots && child[s] == 0) ? 1u : 0u;                    // (s == slots: the scan's extra element)
}

// The leaf met by descending from the root along the digits of cell (tx, ty, tz) of level d (pw = N^d): its leaf index,
// -2 where the cell is a node, -1 for tables that lead out of range.
__device__ __forceinline__ int32_t descend_to(const int32_t* __restrict__ child, const uint32_t* __restrict__ rank, int32_t n, int32_t N,
                                              int32_t n3, int32_t d, int32_t pw, int32_t tx, int32_t ty, int32_t tz) {
    int32_t node = 0, q = pw;
#pragma unroll 1
    for (int32_t l = 0; l <= d; ++l) {
        const int32_t slot = (((tx / q) % N) * N + (ty / q) % N) * N + (tz / q) % N;
        const int32_t s = node * n3 + slot;
        const int32_t ch = child[s];
        if (ch == 0) return (int32_t)rank[s];
        node += ch;
        if (node <= 0 || node >= n) return -1;
        q /= N;
    }
    return -2;
}

__global__ void __launch_bounds__(kNbBlock)
leaf_neighbors_kernel(const int32_t* __restrict__ child, const int32_t* __restrict__ parent_depth, int32_t n, int32_t N, int32_t n3,
                      int32_t slots, int32_t max_depth, const uint32_t* __restrict__ rank, int64_t L, int32_t* __restrict__ neighbors) {
    for (int64_t s64 = (int64_t)blockIdx.x * kNbBlock + threadIdx.x; s64 < slots; s64 += (int64_t)gridDim.x * kNbBlock) {
        const int32_t s = (int32_t)s64;
        if (child[s] != 0) continue;
        const int64_t i = (int64_t)rank[s];
        if (i >= L) continue;                                                // (never: L is the number of leaf slots)
        int32_t node = s / n3, slot = s - node * n3;
        const int32_t d = parent_depth[2 * (int64_t)node + 1];
        bool ok = d >= 0 && d <= max_depth;                                  // N^(d + 1) < 2^31 for these
        int32_t cx = 0, cy = 0, cz = 0, pw = 1;                              // pw: N^level, N^d behind the walk
        if (ok) {
#pragma unroll 1
            for (int32_t lvl = 0;; ++lvl) {
                cx += (slot / (N * N)) * pw;
                cy += ((slot / N) % N) * pw;
                cz += (slot % N) * pw;
                if (lvl == d) { ok = node == 0; break; }
                if (node <= 0) { ok = false; break; }                        // the root above level d: a malformed table
                const int32_t packed = parent_depth[2 * (int64_t)node];
                const int32_t up = packed / n3;
                if (packed < 0 || up >= n) { ok = false; break; }
                slot = packed - up * n3;
                node = up;
                pw *= N;
            }
        }
        const int32_t side = pw * N;                                         // cells per axis at the leaf's level
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int32_t step = (k & 1) ? 1 : -1;
            const int32_t tx = cx + (k >> 1 == 0 ? step : 0), ty = cy + (k >> 1 == 1 ? step : 0), tz = cz + (k >> 1 == 2 ? step : 0);
            const int32_t moved = k >> 1 == 0 ? tx : (k >> 1 == 1 ? ty : tz);
            int32_t res = -1;
            if (ok && moved >= 0 && moved < side) res = descend_to(child, rank, n, N, n3, d, pw, tx, ty, tz);
            neighbors[6 * i + k] = res;
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- plan
__device__ __forceinline__ bool tv_is_edge(const int32_t* __restrict__ neighbors, const int32_t* __restrict__ depths,
                                           const int64_t* __restrict__ rows, int64_t L, int64_t M, int64_t e) {
    const int64_t i = e / 6;
    const int k = (int)(e - 6 * i);
    const int64_t j = neighbors[e];
    if (j < 0 || j >= L) return false;
    const int32_t di = depths[i], dj = depths[j];
    if (!(dj < di || (dj == di && (k & 1)))) return false;                   // from the finer side; at equal sizes from the lower
    const int64_t ri = rows[i], rj = rows[j];
    return ri >= 0 && ri < M && rj >= 0 && rj < M && ri != rj;
}

__global__ void __launch_bounds__(kNbBlock)
tv_mark_kernel(const int32_t* __restrict__ neighbors, const int32_t* __restrict__ depths, const int64_t* __restrict__ rows, int64_t L,
               int64_t M, uint32_t* __restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * kNbBlock + threadIdx.x; e <= 6 * L; e += (int64_t)gridDim.x * kNbBlock)
        flag[e] = (e < 6 * L && tv_is_edge(neighbors, depths, rows, L, M, e)) ? 1u : 0u;
}

// edge number r (slot e) -> incidences 2 r (row_i's) and 2 r + 1 (row_j's): their keys, and the slot for the emit
__global__ void __launch_bounds__(kNbBlock)
tv_fill_kernel(const int32_t* __restrict__ neighbors, const int64_t* __restrict__ rows, int64_t L, const uint32_t* __restrict__ flag,
               const uint32_t* __restrict__ rank, int64_t E, uint32_t* __restrict__ keys, uint32_t* __restrict__ list) {
    for (int64_t e = (int64_t)blockIdx.x * kNbBlock + threadIdx.x; e < 6 * L; e += (int64_t)gridDim.x * kNbBlock) {
        if (flag[e] == 0u) continue;
        const int64_t r = (int64_t)rank[e];
        const int64_t j = neighbors[e];
        if (r >= E || j < 0 || j >= L) continue;                             // (the caller's E is the scan's: never taken)
        list[r] = (uint32_t)e;
        keys[2 * r] = (uint32_t)rows[e / 6];
        keys[2 * r + 1] = (uint32_t)rows[j];
    }
}

// sorted position p holds incidence vals[p] = 2 r + side of edge list[r]: the other row, and (depth of leaf i) << 1 | side
__global__ void __launch_bounds__(kNbBlock)
tv_emit_kernel(const int32_t* __restrict__ neighbors, const int32_t* __restrict__ depths, const int64_t* __restrict__ rows, int64_t L,
               int64_t M, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ list, int64_t E, int32_t* __restrict__ other,
               uint8_t* __restrict__ meta) {
    const int64_t p = (int64_t)blockIdx.x * kNbBlock + threadIdx.x;
    if (p >= 2 * E) return;
    const uint32_t q = vals[p];
    int32_t o = 0;
    uint8_t m = (uint8_t)(q & 1u);
    if ((int64_t)q < 2 * E) {
        const int64_t e = (int64_t)list[q >> 1];
        if (e < 6 * L) {
            const int64_t i = e / 6, j = neighbors[e];
            if (j >= 0 && j < L) {
                const int64_t row = (q & 1u) ? rows[i] : rows[j];
                if (row >= 0 && row < M) o = (int32_t)row;
                m = (uint8_t)(((depths[i] & 63) << 1) | (int32_t)(q & 1u));
            }
        }
    }
    other[p] = o;
    meta[p] = m;
}

// row_ptr[r] = the first sorted position whose key is >= r  (r in [0, M])
__global__ void __launch_bounds__(kNbBlock)
tv_row_ptr_kernel(const uint32_t* __restrict__ keys, int64_t E2, int64_t M, int32_t* __restrict__ row_ptr) {
    const int64_t r = (int64_t)blockIdx.x * kNbBlock + threadIdx.x;
    if (r > M) return;
    int64_t lo = 0, hi = E2;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < r) lo = mid + 1; else hi = mid;
    }
    row_ptr[r] = (int32_t)lo;
}

// ----------------------------------------------------------------------------------------------------------------- tv
// Lane t = r * Kc + j: row r, column c = cols[j] (or j).  P: the norm; MODE: TV_LOSS / TV_LOSS_GRAD / TV_ACCUMULATE.
template <int P, int MODE>
__global__ void __launch_bounds__(kTvBlock)
tv_rows_kernel(const float* __restrict__ f, int64_t M, int K, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ other,
               const uint8_t* __restrict__ meta, const int32_t* __restrict__ cols, int Kc, const float* __restrict__ wtab, float divisor,
               float scale, float* __restrict__ partials, float* G) {
    const int64_t blk = launch_block();
    if (blk * kTvBlock >= M * Kc) return;                        // (a workgroup the grid's fold added: it has no partial)
    const int64_t t = blk * kTvBlock + threadIdx.x;
    const int64_t r = t / Kc;
    float l = 0.f;
    if (r < M) {
        const int j = (int)(t - r * Kc);
        const int c = cols != nullptr ? cols[j] : j;
        const int32_t b0 = row_ptr[r], b1 = row_ptr[r + 1];
        float g = 0.f;
        if (b1 > b0 && c >= 0 && c < K) {
            const float a = f[r * K + c];
#pragma unroll 1
            for (int32_t p = b0; p < b1; ++p) {
                const int32_t o = other[p];
                const uint32_t m = meta[p];
                const float b = f[(int64_t)o * K + c];
                const float w = wtab != nullptr ? wtab[(m >> 1) & 31u] : 1.f;
                const float diff = a - b;
                if constexpr (P == 2) {
                    const float wd = w * diff;
                    g = g + (wd + wd);
                    if (MODE != TV_ACCUMULATE && (m & 1u) == 0u) l = l + wd * diff;
                } else {
                    const float sg = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                    g = g + sg * w;
                    if (MODE != TV_ACCUMULATE && (m & 1u) == 0u) l = l + w * fabsf(diff);
                }
            }
            if constexpr (MODE == TV_ACCUMULATE) {
                const float sg = scale * g;
                G[r * K + c] = G[r * K + c] + sg;
            }
        }
        if constexpr (MODE == TV_LOSS_GRAD) {
            if (c >= 0 && c < K) G[r * K + c] = divisor != 0.f ? g / divisor : g;
        }
    }
    if constexpr (MODE != TV_ACCUMULATE) {
        __shared__ float red[kTvBlock];
        red[threadIdx.x] = l;
        __syncthreads();
#pragma unroll
        for (int s = kTvBlock / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) partials[blk] = red[0];
    }
}

// loss = tree(lane i: partials[i] + partials[i + 256] + ...) [/ divisor]
__global__ void __launch_bounds__(kTvBlock)
tv_loss_kernel(const float* __restrict__ partials, int64_t B, float divisor, float* __restrict__ loss) {
    __shared__ float red[kTvBlock];
    float acc = 0.f;
    for (int64_t q = threadIdx.x; q < B; q += kTvBlock) acc = acc + partials[q];
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = kTvBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = divisor != 0.f ? red[0] / divisor : red[0];
}

template <int P, int MODE>
static void tv_launch(dim3 blocks, hipStream_t st, const float* f, int64_t M, int K, const int32_t* row_ptr, const int32_t* other,
                      const uint8_t* meta, const int32_t* cols, int Kc, const float* wtab, float divisor, float scale, float* partials,
                      float* G) {
    hipLaunchKernelGGL((tv_rows_kernel<P, MODE>), blocks, dim3(kTvBlock), 0, st, f, M, K, row_ptr, other, meta, cols, Kc, wtab,
                       divisor, scale, partials, G);
}

static int plan_check(const char* fn, const int32_t* neighbors, const int32_t* depths, const int64_t* rows, int64_t L, int64_t M) {
    if (L < 0 || 12 * (double)L >= 2147483648.0) return set_error(SVOXT_ERR_INVALID, "%s: the number of leaves must be >= 0 with 12 * L < 2^31", fn);
    if (M < 0 || M > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the number of feature rows must be in [0, 2^31)", fn);
    if (L > 0 && (neighbors == nullptr || depths == nullptr || rows == nullptr))
        return set_error(SVOXT_ERR_INVALID, "%s: neighbors / depths / rows is NULL", fn);
    return SVOXT_OK;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_neighbors_workspace_bytes(int64_t n_internal, int32_t N) {
    if (N < 2 || N > 16 || n_internal < 1 || (double)n_internal * N * N * N >= 2147483648.0) return -1;
    return (int64_t)nb_carve(nullptr, n_internal * N * N * N).bytes;
}

int svoxt_leaf_neighbors(const int32_t* child, const int32_t* parent_depth, int64_t n_internal, int32_t N, int32_t max_depth, int64_t L,
                         int32_t* neighbors, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_leaf_neighbors";
    int rc;
    if ((rc = tree_extents_check(fn, n_internal, N, 0))) return rc;
    double side = N;
    for (int32_t l = 0; l < max_depth && side < 4294967296.0; ++l) side *= N;
    if (max_depth < 0 || side >= 2147483648.0)
        return set_error(SVOXT_ERR_INVALID, "%s: max_depth must be >= 0 with N^(max_depth + 1) < 2^31 (cell coordinates are int32)", fn);
    const int64_t slots = n_internal * N * N * N;
    if (L < 0 || L > slots || 12 * (double)L >= 2147483648.0)
        return set_error(SVOXT_ERR_INVALID, "%s: the number of leaves must be in [0, n_internal * N^3] with 12 * L < 2^31", fn);
    if (child == nullptr || parent_depth == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: child / parent_depth is NULL", fn);
    if (L > 0 && neighbors == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: neighbors is NULL", fn);
    if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_neighbors_workspace_bytes(n_internal, N),
                              "svoxt_neighbors_workspace_bytes(n_internal, N)")))
        return rc;
    if (L == 0) return SVOXT_OK;
    hipStream_t st = (hipStream_t)stream;
    const NbSpace sp = nb_carve(workspace, slots);
    hipLaunchKernelGGL(leaf_flag_kernel, dim3(stride_blocks(slots + 1)), dim3(kNbBlock), 0, st, child, (int32_t)slots, sp.flag);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.flag, (size_t)slots + 1, sp.chunks, sp.rank, st, fn))) return rc;
    hipLaunchKernelGGL(leaf_neighbors_kernel, dim3(stride_blocks(slots)), dim3(kNbBlock), 0, st, child, parent_depth,
                       (int32_t)n_internal, N, N * N * N, (int32_t)slots, max_depth, sp.rank, L, neighbors);
    return check_launch(fn);
}

int64_t svoxt_tv_plan_workspace_bytes(int64_t L, int64_t E) {
    if (L < 0 || 12 * (double)L >= 2147483648.0 || E > 6 * L) return -1;
    return (int64_t)(E < 0 ? marks_carve(nullptr, L).bytes : plan_carve(nullptr, E).bytes);
}

int svoxt_tv_plan_count(const int32_t* neighbors, const int32_t* depths, const int64_t* rows, int64_t L, int64_t M, void* marks,
                        int64_t marks_bytes, int64_t* count, void* stream) {
    const char* fn = "svoxt_tv_plan_count";
    int rc;
    if ((rc = plan_check(fn, neighbors, depths, rows, L, M))) return rc;
    if (marks == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: marks is NULL", fn);
    if (marks_bytes < svoxt_tv_plan_workspace_bytes(L, -1))
        return set_error(SVOXT_ERR_INVALID, "%s: marks smaller than svoxt_tv_plan_workspace_bytes(L, -1)", fn);
    if (count == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: count is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    const NbSpace sp = marks_carve(marks, L);
    hipLaunchKernelGGL(tv_mark_kernel, dim3(stride_blocks(6 * L + 1)), dim3(kNbBlock), 0, st, neighbors, depths, rows, L, M, sp.flag);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.flag, (size_t)(6 * L) + 1, sp.chunks, sp.rank, st, fn))) return rc;
    hipLaunchKernelGGL(rank_totals_kernel<1>, dim3(1), dim3(64), 0, st, RankTotals<1>{{sp.rank}, {6 * L}}, count);
    return check_launch(fn);
}

int svoxt_tv_plan_emit(const int32_t* neighbors, const int32_t* depths, const int64_t* rows, int64_t L, int64_t M, int64_t E,
                       const void* marks, int64_t marks_bytes, void* workspace, int64_t workspace_bytes, int32_t* row_ptr, int32_t* other,
                       uint8_t* meta, void* stream) {
    const char* fn = "svoxt_tv_plan_emit";
    int rc;
    if ((rc = plan_check(fn, neighbors, depths, rows, L, M))) return rc;
    if (E < 0 || E > 6 * L) return set_error(SVOXT_ERR_INVALID, "%s: E must be in [0, 6 L]", fn);
    if (E > 0 && M < 2) return set_error(SVOXT_ERR_INVALID, "%s: an edge joins two different rows: E > 0 needs M >= 2", fn);
    if (marks == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: marks is NULL", fn);
    if (marks_bytes < svoxt_tv_plan_workspace_bytes(L, -1))
        return set_error(SVOXT_ERR_INVALID, "%s: marks smaller than svoxt_tv_plan_workspace_bytes(L, -1)", fn);
    if (row_ptr == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: row_ptr is NULL", fn);
    if (E > 0) {
        if (other == nullptr || meta == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: other / meta is NULL", fn);
        if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_tv_plan_workspace_bytes(L, E), "svoxt_tv_plan_workspace_bytes(L, E)")))
            return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    if (E == 0) {
        const hipError_t e = hipMemsetAsync(row_ptr, 0, sizeof(int32_t) * ((size_t)M + 1), st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
        return SVOXT_OK;
    }
    const NbSpace mk = marks_carve(const_cast<void*>(marks), L);
    const PlanSpace sp = plan_carve(workspace, E);
    hipLaunchKernelGGL(tv_fill_kernel, dim3(stride_blocks(6 * L)), dim3(kNbBlock), 0, st, neighbors, rows, L, mk.flag, mk.rank, E,
                       sp.keys[0], sp.list);
    if ((rc = check_launch(fn))) return rc;
    // the keys are rows in [0, M): sort over the bits of M - 1, in passes of at most 8 bits, all of (nearly) the same width
    int bits = 1;
    while (((uint64_t)(M - 1) >> bits) != 0) ++bits;
    const int passes = (bits + 7) / 8, per = (bits + passes - 1) / passes;
    int cur = 0;
    for (int p = 0, shift = 0; p < passes; ++p, shift += per) {
        const int b = bits - shift < per ? bits - shift : per;
        if ((rc = sort_pass(sp.keys[cur], p == 0 ? nullptr : sp.vals[cur], (uint32_t)(2 * E), shift, b, sp.counts, sp.starts, sp.chunks,
                            sp.keys[cur ^ 1], sp.vals[cur ^ 1], st, fn)))
            return rc;
        cur ^= 1;
    }
    hipLaunchKernelGGL(tv_emit_kernel, dim3(launch_blocks(2 * E)), dim3(kNbBlock), 0, st, neighbors, depths, rows, L, M, sp.vals[cur], sp.list,
                       E, other, meta);
    hipLaunchKernelGGL(tv_row_ptr_kernel, dim3(launch_blocks(M + 1)), dim3(kNbBlock), 0, st, sp.keys[cur], 2 * E, M, row_ptr);
    return check_launch(fn);
}

int64_t svoxt_tv_workspace_bytes(int64_t M, int32_t n_cols) {
    if (M < 0 || M > 0x7fffffff || n_cols < 1 || (double)M * n_cols >= 274877906944.0) return -1;
    return (int64_t)align256(sizeof(float) * (size_t)((M * n_cols + kTvBlock - 1) / kTvBlock)) + 256;
}

int svoxt_tv_rows(const float* features, int64_t M, int32_t K, const int32_t* row_ptr, const int32_t* other, const uint8_t* meta,
                  int64_t E, const int32_t* cols, int32_t n_cols, int32_t p, const float* depth_weights, float divisor, float scale,
                  int32_t mode, float* loss, float* table, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_tv_rows";
    if (p != 1 && p != 2) return set_error(SVOXT_ERR_INVALID, "%s: p must be 1 or 2", fn);
    if (mode != TV_LOSS && mode != TV_LOSS_GRAD && mode != TV_ACCUMULATE)
        return set_error(SVOXT_ERR_INVALID, "%s: mode must be one of SVOXT_TV_LOSS / LOSS_GRAD / ACCUMULATE", fn);
    if (M < 0 || M > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the number of feature rows must be in [0, 2^31)", fn);
    if (K < 1) return set_error(SVOXT_ERR_INVALID, "%s: K must be >= 1", fn);
    if (E < 0 || 2 * (double)E >= 2147483648.0) return set_error(SVOXT_ERR_INVALID, "%s: E must be >= 0 with 2 E < 2^31", fn);
    if ((cols == nullptr) != (n_cols == 0) || n_cols < 0 || n_cols > K)
        return set_error(SVOXT_ERR_INVALID, "%s: cols / n_cols must be NULL / 0 (all columns) or n_cols in [1, K] distinct columns", fn);
    const int Kc = cols != nullptr ? n_cols : K;
    if ((double)M * Kc >= 274877906944.0) return set_error(SVOXT_ERR_INVALID, "%s: M * columns must be below 2^38", fn);
    if (!(divisor >= 0.f) || divisor > 3.0e38f) return set_error(SVOXT_ERR_INVALID, "%s: divisor must be finite and >= 0 (0: none)", fn);
    if (scale != scale) return set_error(SVOXT_ERR_INVALID, "%s: scale is NaN", fn);
    const bool wants_loss = mode != TV_ACCUMULATE, wants_table = mode != TV_LOSS;
    if (wants_loss && loss == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: loss is NULL", fn);
    if (wants_table && M > 0 && table == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: table is NULL", fn);
    if (M > 0 && E > 0) {
        if (features == nullptr || row_ptr == nullptr || other == nullptr || meta == nullptr)
            return set_error(SVOXT_ERR_INVALID, "%s: features / row_ptr / other / meta is NULL", fn);
        if (wants_loss) {
            int rc;
            if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_tv_workspace_bytes(M, Kc), "svoxt_tv_workspace_bytes(M, columns)")))
                return rc;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    const bool empty = M == 0 || E == 0;
    if (mode == TV_LOSS_GRAD && M > 0 && (empty || cols != nullptr)) {      // with all columns the kernel writes every element
        e = hipMemsetAsync(table, 0, sizeof(float) * (size_t)M * (size_t)K, st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    }
    if (empty) {
        if (wants_loss) {
            e = hipMemsetAsync(loss, 0, sizeof(float), st);
            if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
        }
        return SVOXT_OK;
    }
    const int64_t B = (M * Kc + kTvBlock - 1) / kTvBlock;
    float* partials = static_cast<float*>(workspace);
    const dim3 blocks = launch_grid(M * Kc, kTvBlock);           // B workgroups (and what the fold adds: they leave at once)
#define SVOXT_TV_GO(P, MODE) tv_launch<P, MODE>(blocks, st, features, M, K, row_ptr, other, meta, cols, Kc, depth_weights, divisor, scale, partials, table)
    if (p == 2) {
        if (mode == TV_LOSS) SVOXT_TV_GO(2, TV_LOSS); else if (mode == TV_LOSS_GRAD) SVOXT_TV_GO(2, TV_LOSS_GRAD); else SVOXT_TV_GO(2, TV_ACCUMULATE);
    } else {
        if (mode == TV_LOSS) SVOXT_TV_GO(1, TV_LOSS); else if (mode == TV_LOSS_GRAD) SVOXT_TV_GO(1, TV_LOSS_GRAD); else SVOXT_TV_GO(1, TV_ACCUMULATE);
    }
#undef SVOXT_TV_GO
    int rc;
    if ((rc = check_launch(fn)) || !wants_loss) return rc;
    hipLaunchKernelGGL(tv_loss_kernel, dim3(1), dim3(kTvBlock), 0, st, partials, B, divisor, loss);
    return check_launch(fn);
}

}  // extern "C"
