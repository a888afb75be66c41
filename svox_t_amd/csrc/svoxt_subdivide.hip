// svoxt_subdivide.hip -- N3Tree.subdivide and N3Tree.unshare: grow a tree on the device.  subdivide splits the selected
// leaves into new nodes behind `filled` (the topology the reference's refine(sel) writes, svox_t/svox.py:520-546) and,
// with own_rows, gives every new leaf but the first a feature row of its own; unshare gives every leaf slot that names
// a row another, earlier slot names a row of its own.  Both hand back row_map, the old row of every new row.
// C ABI: svoxt_subdivide_* / svoxt_unshare_* (include/svoxt.h).
//
// Pipelines, one stream, integer work only, one host read between count and emit (the counts that size the outputs):
//   subdivide
//     mark   a thread per slot (at most 2048 workgroups striding over the slots) writes two flags: the slot splits (a
//            leaf, selected, its node shallower than the depth limit, not empty unless split_empty), and it brings rows
//            (it splits, names a row and own_rows is set)
//     scan   exclusive scans of both flags, one element past the end: the new node of a splitting slot is filled + its
//            rank, its rows start at M + rows rank * (N^3 - 1), and the last elements are the two counts
//     list   a thread per slot: a splitting slot writes itself (bit 31: it brings rows) at list[rank]
//     emit   a thread per NEW slot (nodes_added * N^3): child 0, the data word (the parent's; with own_rows the
//            parent's at slot 0, a new row behind it, the empty index below an empty leaf) and the row_map entry of a
//            new row; the first slot's thread writes the new node's parent_depth row and the parent's child word
//   unshare
//     owner  a thread per slot: atomicMin(owner[row], slot) over the leaf slots that name a row -- an integer minimum,
//            the same whatever the order of the threads
//     mark   a thread per slot: the flag is set where a leaf names a row whose owner is another slot
//     scan   exclusive scan of the flag: a flagged slot's new row is M + rank
//     emit   a thread per slot: a flagged slot writes its new data word and row_map[M + rank] = its old row
//   and for both: row_map[0 .. M) = 0 .. M - 1; the feature table is then svoxt_prune_gather_rows through row_map.
// Every output word is a function of the input alone: two runs give the same bytes.
//
// In place.  Both emits write into the tables they read, and no pass reads a word that another thread of the same
// pass writes:
//   - subdivide's emit reads data[s] and parent_depth[node, 1] of OLD slots / nodes only (s < filled * N^3, node <
//     filled) and writes data, child and parent_depth rows of NEW nodes only (>= filled), except child[s] of a
//     splitting slot -- written by the one thread of the new node's slot 0, and read by no thread of the emit: what
//     splits was decided by the mark pass and reaches the emit through the workspace (list, ranks), never through
//     child.  The caller's selection is not read by the emit either, so the tables may be regrown between the two
//     entry points.
//   - unshare's emit reads data[s] and writes data[s] in the same thread; who owns a row is not looked up again (the
//     mark pass stored the answer in the flag), so no thread reads another slot's data word while it changes.
//   - within the count entry points every pass writes workspace words only, and each pass reads what an EARLIER pass
//     (an earlier kernel on the stream) wrote; the owner pass's atomicMin is the one place where threads meet on a word,
//     and nothing reads `owner` before the next kernel.
// HBM traffic, per slot of the tree: 4 B child + 4 B data + 1 or 4 B decision read and 8 B of flags written (mark),
// 16 B read and written twice over by the two scans, 12 B read by the list pass; per NEW node 4 B of list and
// 2 * 4 N^3 + 12 B of tables written, 8 B of row_map per new row; then the feature table read and written once by the
// gather, which is most of the bytes (DESIGN.md 4.15 has the figures).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_workspace.h"

namespace svoxt {

constexpr int kSubBlock = kLaunchBlock;      // (the per-slot passes stride over the slots: stride_blocks)
constexpr uint32_t kSubBringsBit = 0x80000000u;

struct SubIn {
    const int32_t* child;
    const int32_t* data;
    const int32_t* parent_depth;
    SlotDecision selected;                   // at most one of mask / weights; neither: every leaf is selected
    int32_t depth_limit;                     // a slot splits iff its node's depth is below this
    int32_t n;                               // internal nodes
    int32_t n3;                              // slots per node
    uint32_t M;                              // feature rows: unsigned data >= M is an empty leaf
    int32_t slots;                           // n * n3 < 2^31
};

// workspace of subdivide: [split_flag u32[slots + 1]] [rows_flag] [split_rank] [rows_rank] [list u32[slots]] [chunk sums]
struct SubSpace {
    uint32_t *split_flag, *rows_flag, *split_rank, *rows_rank, *list, *chunks;
    size_t bytes;
};
// workspace of unshare: [flag u32[slots + 1]] [rank u32[slots + 1]] [owner u32[M]] [chunk sums]
struct UnshareSpace {
    uint32_t *flag, *rank, *owner, *chunks;
    size_t owner_bytes, bytes;
};

static SubSpace sub_carve(void* workspace, int64_t slots) {
    SubSpace sp;
    Carver w(workspace);
    sp.split_flag = w.take<uint32_t>((size_t)slots + 1);
    sp.rows_flag = w.take<uint32_t>((size_t)slots + 1);
    sp.split_rank = w.take<uint32_t>((size_t)slots + 1);
    sp.rows_rank = w.take<uint32_t>((size_t)slots + 1);
    sp.list = w.take<uint32_t>((size_t)slots + 1);             // (slots words are used: the piece is as long as the flags')
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks((size_t)slots + 1));
    sp.bytes = w.bytes();
    return sp;
}

static UnshareSpace unshare_carve(void* workspace, int64_t slots, int64_t M) {
    UnshareSpace sp;
    Carver w(workspace);
    sp.flag = w.take<uint32_t>((size_t)slots + 1);
    sp.rank = w.take<uint32_t>((size_t)slots + 1);
    sp.owner = w.take<uint32_t>((size_t)M);
    sp.owner_bytes = sizeof(uint32_t) * (size_t)M;
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks((size_t)slots + 1));
    sp.bytes = w.bytes();
    return sp;
}

__global__ void __launch_bounds__(kSubBlock)
subdivide_mark_kernel(SubIn in, bool split_empty, bool own_rows, uint32_t* __restrict__ split_flag, uint32_t* __restrict__ rows_flag) {
    for (int64_t s64 = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; s64 <= in.slots; s64 += (int64_t)gridDim.x * kSubBlock) {
        const int32_t s = (int32_t)s64;
        uint32_t split = 0u, rows = 0u;
        if (s < in.slots && in.child[s] == 0 && in.selected(s)) {                  // (s == slots: the scans' extra element)
            const int32_t node = s / in.n3;
            const bool full = (uint32_t)in.data[s] < in.M;
            if (in.parent_depth[2 * (int64_t)node + 1] < in.depth_limit && (full || split_empty)) {
                split = 1u;
                rows = (full && own_rows) ? 1u : 0u;
            }
        }
        split_flag[s] = split;
        rows_flag[s] = rows;
    }
}

// counts[0] = nodes added, counts[1] = feature rows added
__global__ void __launch_bounds__(64)
subdivide_counts_kernel(const uint32_t* __restrict__ split_rank, const uint32_t* __restrict__ rows_rank, int32_t slots, int32_t n3,
                        int64_t* __restrict__ counts) {
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)split_rank[slots];
        counts[1] = (int64_t)rows_rank[slots] * (n3 - 1);
    }
}

__global__ void __launch_bounds__(kSubBlock)
subdivide_list_kernel(const uint32_t* __restrict__ split_flag, const uint32_t* __restrict__ rows_flag,
                      const uint32_t* __restrict__ split_rank, int32_t slots, uint32_t* __restrict__ list) {
    for (int64_t s = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; s < slots; s += (int64_t)gridDim.x * kSubBlock)
        if (split_flag[s] != 0u) list[split_rank[s]] = (uint32_t)s | (rows_flag[s] != 0u ? kSubBringsBit : 0u);   // rank < slots
}

__global__ void __launch_bounds__(kSubBlock)
subdivide_emit_kernel(int32_t n, int32_t n3, uint32_t M, int32_t slots, bool own_rows, const uint32_t* __restrict__ list,
                      const uint32_t* __restrict__ split_rank, const uint32_t* __restrict__ rows_rank, int64_t nodes_added,
                      int64_t new_M, int32_t empty_index, int32_t* child, int32_t* data, int32_t* parent_depth,
                      int64_t* __restrict__ row_map) {
    const int64_t t = (int64_t)blockIdx.x * kSubBlock + threadIdx.x;
    const int64_t i = t / n3;
    const int32_t j = (int32_t)(t - i * n3);
    if (i >= nodes_added || i >= (int64_t)split_rank[slots]) return;     // (the caller's count is the scan's: the second test is never taken)
    const uint32_t e = list[i];
    const int32_t s = (int32_t)(e & ~kSubBringsBit);
    if (s >= slots) return;                                              // (never taken)
    const int32_t node = s / n3;
    const int64_t id = (int64_t)n + i, at = id * n3 + j;
    int32_t d = data[s];                                                 // an old slot: no thread writes it
    if (own_rows) {
        if ((e & kSubBringsBit) == 0u) {
            d = empty_index;                                             // below an empty leaf: empty leaves, no rows
        } else if (j > 0) {
            const int64_t row = (int64_t)M + (int64_t)rows_rank[s] * (n3 - 1) + (j - 1);
            if (row >= new_M) return;                                    // (never taken)
            row_map[row] = (int64_t)(uint32_t)d;
            d = (int32_t)row;
        }
    }
    child[at] = 0;
    data[at] = d;
    if (j == 0) {
        parent_depth[2 * id] = s;
        parent_depth[2 * id + 1] = parent_depth[2 * (int64_t)node + 1] + 1;      // an old node's row: no thread writes it
        child[s] = (int32_t)(id - node);
    }
}

__global__ void __launch_bounds__(kSubBlock)
row_map_head_kernel(int64_t M, int64_t* __restrict__ row_map) {
    const int64_t r = (int64_t)blockIdx.x * kSubBlock + threadIdx.x;
    if (r < M) row_map[r] = r;
}

__global__ void __launch_bounds__(kSubBlock)
unshare_owner_kernel(const int32_t* __restrict__ child, const int32_t* __restrict__ data, int32_t slots, uint32_t M,
                     uint32_t* __restrict__ owner) {
    for (int64_t s = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; s < slots; s += (int64_t)gridDim.x * kSubBlock) {
        if (child[s] != 0) continue;
        const uint32_t d = (uint32_t)data[s];
        if (d < M) atomicMin(owner + d, (uint32_t)s);
    }
}

__global__ void __launch_bounds__(kSubBlock)
unshare_mark_kernel(const int32_t* __restrict__ child, const int32_t* __restrict__ data, int32_t slots, uint32_t M,
                    const uint32_t* __restrict__ owner, uint32_t* __restrict__ flag) {
    for (int64_t s = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; s <= slots; s += (int64_t)gridDim.x * kSubBlock) {
        uint32_t f = 0u;
        if (s < slots && child[s] == 0) {
            const uint32_t d = (uint32_t)data[s];
            if (d < M && owner[d] != (uint32_t)s) f = 1u;
        }
        flag[s] = f;
    }
}

__global__ void __launch_bounds__(kSubBlock)
unshare_emit_kernel(int32_t slots, uint32_t M, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                    int64_t rows_added, int32_t* data, int64_t* __restrict__ row_map) {
    const int64_t s = (int64_t)blockIdx.x * kSubBlock + threadIdx.x;
    if (s >= slots || flag[s] == 0u) return;
    const int64_t r = (int64_t)rank[s];
    if (r >= rows_added) return;                                         // (the caller's count is the scan's: never taken)
    row_map[(int64_t)M + r] = (int64_t)(uint32_t)data[s];
    data[s] = (int32_t)((int64_t)M + r);
}

// The extents every entry point shares.  Nothing here touches HIP.
static int sub_check_extents(const char* fn, int64_t n, int32_t N, int64_t M, const void* workspace, int64_t workspace_bytes) {
    int rc;
    if ((rc = tree_extents_check(fn, n, N, M))) return rc;
    return workspace_check(fn, workspace, workspace_bytes, svoxt_subdivide_workspace_bytes(n, N, M),
                           "svoxt_subdivide_workspace_bytes(n_internal, N, M)");
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_subdivide_workspace_bytes(int64_t n_internal, int32_t N, int64_t M) {
    if (N < 2 || N > 16 || n_internal < 1 || (double)n_internal * N * N * N >= 2147483648.0 || M < 0 || M > 0x7fffffff) return -1;
    const int64_t slots = n_internal * N * N * N;
    const size_t a = sub_carve(nullptr, slots).bytes, b = unshare_carve(nullptr, slots, M).bytes;
    return (int64_t)(a > b ? a : b);
}

int svoxt_subdivide_count(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal, int32_t N,
                          int64_t M, const uint8_t* sel, const float* weights, float threshold, int32_t depth_limit,
                          int32_t split_empty, int32_t own_rows, void* workspace, int64_t workspace_bytes, int64_t* counts,
                          void* stream) {
    const char* fn = "svoxt_subdivide_count";
    int rc;
    if ((rc = sub_check_extents(fn, n_internal, N, M, workspace, workspace_bytes))) return rc;
    if (child == nullptr || data == nullptr || parent_depth == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: child / data / parent_depth is NULL", fn);
    if (sel != nullptr && weights != nullptr) return set_error(SVOXT_ERR_INVALID, "%s: at most one of sel / weights may be given", fn);
    if (weights != nullptr && threshold != threshold) return set_error(SVOXT_ERR_INVALID, "%s: threshold is NaN", fn);
    if (counts == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: counts is NULL", fn);
    SubIn in;
    in.child = child; in.data = data; in.parent_depth = parent_depth; in.selected = SlotDecision{sel, weights, threshold};
    in.depth_limit = depth_limit; in.n = (int32_t)n_internal; in.n3 = N * N * N; in.M = (uint32_t)M;
    in.slots = (int32_t)(n_internal * in.n3);
    hipStream_t st = (hipStream_t)stream;
    const SubSpace sp = sub_carve(workspace, in.slots);
    hipLaunchKernelGGL(subdivide_mark_kernel, dim3(stride_blocks((int64_t)in.slots + 1)), dim3(kSubBlock), 0, st, in,
                       split_empty != 0, own_rows != 0, sp.split_flag, sp.rows_flag);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.split_flag, (size_t)in.slots + 1, sp.chunks, sp.split_rank, st, fn)) ||
        (rc = exclusive_scan(sp.rows_flag, (size_t)in.slots + 1, sp.chunks, sp.rows_rank, st, fn)))
        return rc;
    hipLaunchKernelGGL(subdivide_list_kernel, dim3(stride_blocks(in.slots)), dim3(kSubBlock), 0, st, sp.split_flag, sp.rows_flag,
                       sp.split_rank, in.slots, sp.list);
    hipLaunchKernelGGL(subdivide_counts_kernel, dim3(1), dim3(64), 0, st, sp.split_rank, sp.rows_rank, in.slots, in.n3, counts);
    return check_launch(fn);
}

int svoxt_subdivide_emit(int32_t* child, int32_t* data, int32_t* parent_depth, int64_t n_internal, int32_t N, int64_t M,
                         int64_t capacity, int32_t own_rows, const void* workspace, int64_t workspace_bytes, int64_t nodes_added,
                         int64_t rows_added, int32_t empty_index, int64_t* row_map, void* stream) {
    const char* fn = "svoxt_subdivide_emit";
    int rc;
    if ((rc = sub_check_extents(fn, n_internal, N, M, workspace, workspace_bytes))) return rc;
    const int64_t n3 = (int64_t)N * N * N, slots = n_internal * n3;
    if (nodes_added < 0 || nodes_added > slots) return set_error(SVOXT_ERR_INVALID, "%s: nodes_added must be in [0, n_internal * N^3]", fn);
    if (capacity < n_internal + nodes_added)
        return set_error(SVOXT_ERR_INVALID, "%s: bad extents (n_internal + nodes_added must fit the capacity)", fn);
    if ((double)capacity * (double)n3 >= 2147483648.0)
        return set_error(SVOXT_ERR_INVALID, "%s: tree too large for 32-bit slot indices (capacity * N^3 must be < 2^31)", fn);
    if (rows_added < 0 || rows_added % (n3 - 1) != 0 || rows_added / (n3 - 1) > nodes_added || (own_rows == 0 && rows_added != 0))
        return set_error(SVOXT_ERR_INVALID, "%s: rows_added must be a multiple of N^3 - 1, at most nodes_added of them (0 without own_rows)", fn);
    if ((int64_t)(uint32_t)empty_index <= M + rows_added)
        return set_error(SVOXT_ERR_INVALID, "%s: M + rows_added must stay below empty_index as an unsigned number", fn);
    if (child == nullptr || data == nullptr || parent_depth == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: child / data / parent_depth is NULL", fn);
    if (own_rows != 0 && M + rows_added > 0 && row_map == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: row_map is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    const SubSpace sp = sub_carve(const_cast<void*>(workspace), slots);
    if (own_rows != 0 && M > 0) hipLaunchKernelGGL(row_map_head_kernel, dim3(launch_blocks(M)), dim3(kSubBlock), 0, st, M, row_map);
    if (nodes_added > 0)
        hipLaunchKernelGGL(subdivide_emit_kernel, dim3(launch_blocks(nodes_added * n3)), dim3(kSubBlock), 0, st, (int32_t)n_internal,
                           (int32_t)n3, (uint32_t)M, (int32_t)slots, own_rows != 0, sp.list, sp.split_rank, sp.rows_rank, nodes_added,
                           M + rows_added, empty_index, child, data, parent_depth, row_map);
    return check_launch(fn);
}

int svoxt_unshare_count(const int32_t* child, const int32_t* data, int64_t n_internal, int32_t N, int64_t M, void* workspace,
                        int64_t workspace_bytes, int64_t* counts, void* stream) {
    const char* fn = "svoxt_unshare_count";
    int rc;
    if ((rc = sub_check_extents(fn, n_internal, N, M, workspace, workspace_bytes))) return rc;
    if (child == nullptr || data == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: child / data is NULL", fn);
    if (counts == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: counts is NULL", fn);
    const int32_t slots = (int32_t)(n_internal * N * N * N);
    hipStream_t st = (hipStream_t)stream;
    const UnshareSpace sp = unshare_carve(workspace, slots, M);
    if (M > 0) {
        const hipError_t e = hipMemsetAsync(sp.owner, 0xff, sp.owner_bytes, st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
        hipLaunchKernelGGL(unshare_owner_kernel, dim3(stride_blocks(slots)), dim3(kSubBlock), 0, st, child, data, slots, (uint32_t)M,
                           sp.owner);
    }
    hipLaunchKernelGGL(unshare_mark_kernel, dim3(stride_blocks((int64_t)slots + 1)), dim3(kSubBlock), 0, st, child, data, slots,
                       (uint32_t)M, sp.owner, sp.flag);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.flag, (size_t)slots + 1, sp.chunks, sp.rank, st, fn))) return rc;
    hipLaunchKernelGGL(rank_totals_kernel<1>, dim3(1), dim3(64), 0, st, RankTotals<1>{{sp.rank}, {(int64_t)slots}}, counts);
    return check_launch(fn);
}

int svoxt_unshare_emit(int32_t* data, int64_t n_internal, int32_t N, int64_t M, const void* workspace, int64_t workspace_bytes,
                       int64_t rows_added, int32_t empty_index, int64_t* row_map, void* stream) {
    const char* fn = "svoxt_unshare_emit";
    int rc;
    if ((rc = sub_check_extents(fn, n_internal, N, M, workspace, workspace_bytes))) return rc;
    const int64_t slots = n_internal * N * N * N;
    if (rows_added < 0 || rows_added > slots) return set_error(SVOXT_ERR_INVALID, "%s: rows_added must be in [0, n_internal * N^3]", fn);
    if ((int64_t)(uint32_t)empty_index <= M + rows_added)
        return set_error(SVOXT_ERR_INVALID, "%s: M + rows_added must stay below empty_index as an unsigned number", fn);
    if (data == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: data is NULL", fn);
    if (M + rows_added > 0 && row_map == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: row_map is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    const UnshareSpace sp = unshare_carve(const_cast<void*>(workspace), slots, M);
    if (M > 0) hipLaunchKernelGGL(row_map_head_kernel, dim3(launch_blocks(M)), dim3(kSubBlock), 0, st, M, row_map);
    if (rows_added > 0)
        hipLaunchKernelGGL(unshare_emit_kernel, dim3(launch_blocks(slots)), dim3(kSubBlock), 0, st, (int32_t)slots, (uint32_t)M, sp.flag,
                           sp.rank, rows_added, data, row_map);
    return check_launch(fn);
}

}  // extern "C"
