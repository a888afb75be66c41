// svoxt_workspace.h -- what the tree operators (prune, merge / frontier, subdivide / unshare, leaf_neighbors / tv_plan,
// assign, quantize, voxelize) share on the host side and in their flag / scan / emit passes: the workspace carver, the
// launch sizes, the extents and workspace checks, and the small kernels every such pipeline ends in.  Not part of the
// public C ABI.
//
// Workspace layout rules (the *_workspace_bytes queries promise sizes; callers allocate by them):
//   - a workspace is a sequence of pieces, each starting on a 256-byte line and padded to a multiple of 256 bytes;
//   - a unit's XSpace struct names its pieces, its carve function takes them in layout order: the order IS the layout;
//   - the carve function runs twice per call: over NULL to size the workspace (no pointer is formed), over the caller's
//     pointer to hand out the pieces;
//   - what an entry point clears with one hipMemsetAsync is a PREFIX of the workspace: the flags come first and the
//     carve function records Carver::bytes() behind them as clear_bytes.
// Per-slot passes over a tree run at most kStrideBlocksMax workgroups and stride beyond that; what is sized by the
// number of workgroups of such a pass (prune's per-workgroup drop counts) is sized by this one constant.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"

namespace svoxt {

constexpr int kLaunchBlock = 256;            // threads per workgroup of every kernel launched through the helpers below
constexpr int kStrideBlocksMax = 2048;       // workgroups of a striding pass, at most

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned launch_blocks(int64_t n) { return (unsigned)((n + kLaunchBlock - 1) / kLaunchBlock); }
// A launch of a lane per ELEMENT of an array that may hold 2^32 elements or more (the "below 2^38" entry points).  HIP
// launches fewer than 2^32 work-items along a grid dimension, so from kGridFoldBlocks workgroups on the workgroups fold
// over grid.y; the kernel's lane index is launch_lane(), its workgroup's launch_block().  Below that the grid is the
// one-dimensional grid of launch_blocks(n) and blockIdx.y is 0.  The fold may add up to kGridFoldBlocks - 1 workgroups
// behind the last element: every such kernel leaves on its extent check, as its last workgroup's tail lanes do.
constexpr int64_t kGridFoldBlocks = (int64_t)1 << 22;            // 2^30 lanes along x
inline dim3 launch_grid(int64_t n, int block = kLaunchBlock) {
    const int64_t b = (n + block - 1) / block;
    if (b <= kGridFoldBlocks) return dim3((unsigned)b);
    return dim3((unsigned)kGridFoldBlocks, (unsigned)((b + kGridFoldBlocks - 1) / kGridFoldBlocks));
}
__device__ __forceinline__ int64_t launch_block() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }
// (launch_lane() is for kernels of kLaunchBlock threads a workgroup; one launched with another `block` forms its lane from
// launch_block() itself, as tv_rows_kernel does)
__device__ __forceinline__ int64_t launch_lane() { return launch_block() * kLaunchBlock + threadIdx.x; }

inline unsigned stride_blocks(int64_t n) {
    const unsigned need = launch_blocks(n);
    return need < (unsigned)kStrideBlocksMax ? need : (unsigned)kStrideBlocksMax;
}

// A bump allocator over a workspace that may be NULL (then it only measures).
class Carver {
public:
    explicit Carver(void* workspace) : base_(static_cast<char*>(workspace)), at_(0) {}
    template <typename T>
    T* take(size_t count) {
        T* p = base_ != nullptr ? reinterpret_cast<T*>(base_ + at_) : nullptr;
        at_ += align256(sizeof(T) * count);
        return p;
    }
    size_t bytes() const { return at_; }

private:
    char* base_;
    size_t at_;
};

// The extents every tree operator takes: N in [2, 16], n * N^3 < 2^31 slots, M in [0, 2^31) feature rows.
inline int tree_extents_check(const char* fn, int64_t n, int32_t N, int64_t M) {
    if (N < 2 || N > 16) return set_error(SVOXT_ERR_INVALID, "%s: branching factor N must be in [2, 16]", fn);
    if (n < 1 || (double)n * N * N * N >= 2147483648.0)
        return set_error(SVOXT_ERR_INVALID, "%s: n_internal must be >= 1 with n_internal * N^3 < 2^31", fn);
    if (M < 0 || M > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the number of feature rows must be in [0, 2^31)", fn);
    return SVOXT_OK;
}

// `need` is the answer of the query named `query`, e.g. "svoxt_prune_workspace_bytes(n_internal, M)".
inline int workspace_check(const char* fn, const void* workspace, int64_t bytes, int64_t need, const char* query) {
    if (workspace == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: workspace is NULL", fn);
    if (bytes < need) return set_error(SVOXT_ERR_INVALID, "%s: workspace smaller than %s", fn, query);
    return SVOXT_OK;
}

// The caller's decision about a slot: a mask, or weights against a threshold, or neither (every slot).
struct SlotDecision {
    const uint8_t* mask;
    const float* weights;
    float threshold;
    __device__ __forceinline__ bool operator()(int32_t s) const {
        if (mask != nullptr) return mask[s] != 0;
        if (weights != nullptr) return weights[s] >= threshold;                  // (a NaN weight: no)
        return true;
    }
};

// The parent_depth row of node `node` at its new place `id`, for emits that renumber nodes by node_rank: the packed
// parent slot follows the parent's new id (the root's row, and a parent out of range, are carried), the depth is kept.
__device__ __forceinline__ void emit_renumbered_parent_depth(const int32_t* __restrict__ parent_depth, int32_t node, int32_t n, int32_t n3,
                                                             const uint32_t* __restrict__ node_rank, int32_t id,
                                                             int32_t* __restrict__ pd_out) {
    const int32_t packed = parent_depth[2 * (int64_t)node];
    int32_t p = packed;                                          // the root's row is carried
    if (node != 0) {
        const int32_t up = packed / n3;
        p = (up >= 0 && up < n) ? (int32_t)node_rank[up] * n3 + (packed - up * n3) : packed;
    }
    pd_out[2 * (int64_t)id] = p;
    pd_out[2 * (int64_t)id + 1] = parent_depth[2 * (int64_t)node + 1];
}

// out[rank[i]] = i for the flagged i in [0, n) whose rank is below `limit` (the caller's count is the scan's: the
// second test is never taken): the flagged ids in ascending order.
template <typename Out>
__global__ void __launch_bounds__(kLaunchBlock)
scatter_ranked_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, int64_t n, int64_t limit,
                      Out* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (i < n && flag[i] != 0u && (int64_t)rank[i] < limit) out[rank[i]] = (Out)i;
}

// counts[r] = rank[r][last[r]], the total an exclusive scan leaves one element past the end, for r < R; a NULL rank
// array stands for a scan that was not run: its total is last[r] itself (nothing was dropped).
template <int R>
struct RankTotals {
    const uint32_t* rank[R];
    int64_t last[R];
};
template <int R>
__global__ void __launch_bounds__(64)
rank_totals_kernel(RankTotals<R> t, int64_t* __restrict__ counts) {
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int r = 0; r < R; ++r) counts[r] = t.rank[r] != nullptr ? (int64_t)t.rank[r][t.last[r]] : t.last[r];
}

}  // namespace svoxt
