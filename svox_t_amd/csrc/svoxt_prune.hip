// svoxt_prune.hip -- N3Tree.prune: drop leaves, collapse the nodes nothing is left below, renumber the nodes that
// remain and the feature rows that are still used.  C ABI: svoxt_prune_* (include/svoxt.h).
//
// The reference has the two halves of this as tensor ops, both stale in this fork: merge() (svox_t/svox.py:352-389)
// reads `data` as float values, shrink_to_fit() (:600-642) defragments nodes and never touches the feature table
// `data` indexes.  What it fixes is the layout of the tables: child words are offsets new_id(child) - new_id(node)
// (:589), parent_depth[:, 0] is the packed parent slot, unused rows look like those of a fresh tree.
//
// A slot "survives" when it is a leaf (child == 0), kept by the caller's decision and not empty (unsigned data < M).
// Pipeline, one stream, integer work only, the only host read between the two entry points (the two counts that size
// the outputs, and the number of leaves dropped):
//   mark     a thread per slot (at most 2048 workgroups striding over the slots).  A surviving slot flags its feature row and its node, then walks parent_depth[:, 0]
//            upwards flagging nodes until it meets one that is flagged already: whoever flagged that one goes on from
//            there (or has), so every ancestor of a surviving leaf ends up flagged.  All writers store the same 1: plain
//            stores, no atomics, and nothing depends on who came first; the leaves dropped are counted per workgroup.  Without collapsing every node is flagged.
//   scan     exclusive scans of the node flags and the row flags (svoxt_order.hip's two kernels): new ids, and -- one
//            element past the end -- the two counts
//   emit     a thread per slot of a flagged node writes its child / data word at the node's new place (a child whose
//            node is gone becomes an empty leaf; inner slots get the empty index instead of their stale word); the
//            first slot's thread writes the parent_depth row; a thread per flagged feature row writes row_map
//            (scatter_ranked_kernel, svoxt_workspace.h)
//   gather   new feature table = old rows in row_map's order, 16 bytes a thread (svoxt_prune_gather_rows)
// Every output word is a function of the input alone: two runs give the same bytes.
// HBM traffic: child, data and the decision read twice (mark, emit), parent_depth's first column chased by the walks
// (a few steps per node: most stop at the first flagged ancestor), 8 bytes per node and per feature row of flags and
// ranks, the new tables written once -- and then the kept rows, read and written once: most of the BYTES (597 of 710 MiB on
// the depth-9 / K = 32 tree), and 0.11 of its 0.40 ms (profiles/prune_timing.txt).
// The gather is a kernel of its own because it measured 2.1x faster than svoxt_permute_rows (a float a thread, int32
// index) on 128-byte rows: 0.116 against 0.243 ms for 2.37 M rows.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_wave.h"
#include "svoxt_workspace.h"

namespace svoxt {

constexpr int kPruneBlock = kLaunchBlock;
constexpr int kMarkBlocksMax = kStrideBlocksMax;   // the mark pass strides over the slots: a count of dropped leaves per workgroup, no atomics

struct PruneIn {
    const int32_t* child;
    const int32_t* data;
    const int32_t* parent_depth;
    SlotDecision kept;                   // one of mask / weights (prune_check refuses neither)
    int32_t n;                           // internal nodes
    int32_t n3;                          // slots per node
    uint32_t M;                          // feature rows: unsigned data >= M is an empty leaf
    int32_t slots;                       // n * n3 < 2^31
};

// workspace: [dropped u32[kMarkBlocksMax]: per workgroup of the mark pass] [node_flag u32[n + 1]] [row_flag u32[M + 1]] [node_rank u32[n + 1]] [row_rank u32[M + 1]]
// [chunk sums]; the flags (and the counter) are what svoxt_prune_count clears
struct PruneSpace {
    uint32_t* dropped;
    uint32_t *node_flag, *row_flag, *node_rank, *row_rank, *chunks;
    size_t clear_bytes, bytes;
};

static PruneSpace prune_carve(void* workspace, int64_t n, int64_t M) {
    PruneSpace sp;
    Carver w(workspace);
    sp.dropped = w.take<uint32_t>(kMarkBlocksMax);
    sp.node_flag = w.take<uint32_t>((size_t)n + 1);
    sp.row_flag = w.take<uint32_t>((size_t)M + 1);
    sp.clear_bytes = w.bytes();
    sp.node_rank = w.take<uint32_t>((size_t)n + 1);
    sp.row_rank = w.take<uint32_t>((size_t)M + 1);
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks((size_t)(n > M ? n : M) + 1));
    sp.bytes = w.bytes();
    return sp;
}

__global__ void __launch_bounds__(kPruneBlock)
prune_mark_kernel(PruneIn in, bool collapse, bool rows, uint32_t* __restrict__ node_flag, uint32_t* __restrict__ row_flag,
                  uint32_t* __restrict__ dropped) {
    __shared__ uint32_t wave_drops[kPruneBlock / 64];
    uint32_t drops = 0;
    for (int64_t s64 = (int64_t)blockIdx.x * kPruneBlock + threadIdx.x; s64 < in.slots; s64 += (int64_t)gridDim.x * kPruneBlock) {
        const int32_t s = (int32_t)s64;
        int32_t node = s / in.n3;
        if (s == 0 || (!collapse && s == node * in.n3)) node_flag[node] = 1u;          // the root always; without collapsing every node
        if (in.child[s] != 0) continue;
        const uint32_t d = (uint32_t)in.data[s];
        if (d >= in.M) continue;
        if (!in.kept(s)) { ++drops; continue; }
        if (rows) row_flag[d] = 1u;
        if (!collapse) continue;
        // at most one step per level: a flagged node ends the walk, and every step flags one
        while (__atomic_load_n(node_flag + node, __ATOMIC_RELAXED) == 0u) {
            __atomic_store_n(node_flag + node, 1u, __ATOMIC_RELAXED);
            if (node == 0) break;
            const int32_t up = in.parent_depth[2 * (int64_t)node] / in.n3;
            if (up < 0 || up >= in.n) break;                                            // (a malformed table: no walk out of it)
            node = up;
        }
    }
    // leaves dropped by this workgroup: one plain store (a same-address atomic per wavefront was 0.9 of the pass's 1.0 ms)
    drops = wave_all_sum(drops);
    if ((threadIdx.x & 63) == 0) wave_drops[threadIdx.x >> 6] = drops;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kPruneBlock / 64; ++w) t += wave_drops[w];
        dropped[blockIdx.x] = t;
    }
}

// counts[0] = nodes that remain, counts[1] = feature rows that remain, counts[2] = leaves dropped
__global__ void __launch_bounds__(64)
prune_counts_kernel(const uint32_t* __restrict__ node_rank, int32_t n, const uint32_t* __restrict__ row_rank, uint32_t M, bool rows,
                    const uint32_t* __restrict__ dropped, int mark_blocks, int64_t* __restrict__ counts) {
    unsigned long long t = 0;
    for (int b = threadIdx.x; b < mark_blocks; b += 64) t += dropped[b];
    t = wave_all_sum(t);
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)node_rank[n];
        counts[1] = rows ? (int64_t)row_rank[M] : (int64_t)M;
        counts[2] = (int64_t)t;
    }
}

__global__ void __launch_bounds__(kPruneBlock)
prune_emit_kernel(PruneIn in, bool rows, const uint32_t* __restrict__ node_flag, const uint32_t* __restrict__ node_rank,
                  const uint32_t* __restrict__ row_rank, int32_t new_n, int32_t empty_index, int32_t* __restrict__ child_out,
                  int32_t* __restrict__ data_out, int32_t* __restrict__ pd_out) {
    const int32_t s = (int32_t)(blockIdx.x * kPruneBlock + threadIdx.x);
    if (s >= in.slots) return;
    const int32_t node = s / in.n3, k = s - node * in.n3;
    if (node_flag[node] == 0u) return;
    const int32_t id = (int32_t)node_rank[node];
    if (id >= new_n) return;                                     // (the caller's count is the scan's: never taken)
    int32_t c = in.child[s], d = empty_index;
    if (c != 0) {
        const int64_t kid = (int64_t)node + c;
        c = (kid >= 0 && kid < in.n && node_flag[kid] != 0u) ? (int32_t)node_rank[kid] - id : 0;
    } else {
        const int32_t old = in.data[s];
        if ((uint32_t)old >= in.M) d = old;                      // an empty leaf keeps its word
        else if (in.kept(s)) d = rows ? (int32_t)row_rank[(uint32_t)old] : old;
    }
    const int64_t at = (int64_t)id * in.n3 + k;
    child_out[at] = c;
    data_out[at] = d;
    if (k == 0) emit_renumbered_parent_depth(in.parent_depth, node, in.n, in.n3, node_rank, id, pd_out);
}

// dst[i, :] = src[row_map[i], :], a thread per V floats of a row (V = 4: 16-byte loads and stores; a 128-byte row is 8 lanes)
template <int V>
__global__ void __launch_bounds__(kPruneBlock)
prune_gather_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ row_map, float* __restrict__ dst, int64_t n,
                         int per_row, int64_t src_rows) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const int64_t i = (int64_t)blockIdx.x * kPruneBlock + threadIdx.x;
    if (i >= n * per_row) return;
    const int64_t row = i / per_row;
    const int c = (int)(i - row * per_row);
    const int64_t from = row_map[row];
    if (from < 0 || from >= src_rows) return;                    // (not a row of src: nothing is read)
    reinterpret_cast<vec*>(dst)[i] = reinterpret_cast<const vec*>(src)[from * per_row + c];
}

// Argument checks of the two entry points.  Nothing here touches HIP.
static int prune_check(const char* fn, const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n, int32_t N,
                       int64_t M, const uint8_t* keep, const float* weights, float threshold, const void* workspace,
                       int64_t workspace_bytes, PruneIn& in) {
    int rc;
    if ((rc = tree_extents_check(fn, n, N, M))) return rc;
    if (child == nullptr || data == nullptr || parent_depth == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: child / data / parent_depth is NULL", fn);
    if ((keep == nullptr) == (weights == nullptr)) return set_error(SVOXT_ERR_INVALID, "%s: exactly one of keep / weights must be given", fn);
    if (weights != nullptr && threshold != threshold) return set_error(SVOXT_ERR_INVALID, "%s: threshold is NaN", fn);
    if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_prune_workspace_bytes(n, M),
                              "svoxt_prune_workspace_bytes(n_internal, M)")))
        return rc;
    in.child = child; in.data = data; in.parent_depth = parent_depth;
    in.kept = SlotDecision{keep, weights, threshold};
    in.n = (int32_t)n; in.n3 = N * N * N; in.M = (uint32_t)M; in.slots = (int32_t)(n * in.n3);
    return SVOXT_OK;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_prune_workspace_bytes(int64_t n_internal, int64_t M) {
    if (n_internal < 1 || n_internal > 0x7fffffff || M < 0 || M > 0x7fffffff) return -1;
    return (int64_t)prune_carve(nullptr, n_internal, M).bytes;
}

int svoxt_prune_count(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal, int32_t N,
                      int64_t M, const uint8_t* keep, const float* weights, float threshold, int32_t collapse,
                      int32_t compact_features, void* workspace, int64_t workspace_bytes, int64_t* counts, void* stream) {
    const char* fn = "svoxt_prune_count";
    PruneIn in;
    int rc;
    if ((rc = prune_check(fn, child, data, parent_depth, n_internal, N, M, keep, weights, threshold, workspace, workspace_bytes, in)))
        return rc;
    if (counts == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: counts is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    const PruneSpace sp = prune_carve(workspace, n_internal, M);
    const bool rows = compact_features != 0;
    const hipError_t e = hipMemsetAsync(workspace, 0, sp.clear_bytes, st);
    if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    const unsigned mark_blocks = stride_blocks(in.slots);
    hipLaunchKernelGGL(prune_mark_kernel, dim3(mark_blocks), dim3(kPruneBlock), 0, st, in, collapse != 0, rows,
                       sp.node_flag, sp.row_flag, sp.dropped);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.node_flag, (size_t)n_internal + 1, sp.chunks, sp.node_rank, st, fn))) return rc;
    if (rows && (rc = exclusive_scan(sp.row_flag, (size_t)M + 1, sp.chunks, sp.row_rank, st, fn))) return rc;
    hipLaunchKernelGGL(prune_counts_kernel, dim3(1), dim3(64), 0, st, sp.node_rank, in.n, sp.row_rank, in.M, rows, sp.dropped,
                       (int)mark_blocks, counts);
    return check_launch(fn);
}

int svoxt_prune_emit(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal, int32_t N,
                     int64_t M, const uint8_t* keep, const float* weights, float threshold, int32_t compact_features,
                     const void* workspace, int64_t workspace_bytes, int64_t new_n_internal, int64_t new_M, int32_t empty_index,
                     int32_t* child_out, int32_t* data_out, int32_t* parent_depth_out, int64_t* row_map, void* stream) {
    const char* fn = "svoxt_prune_emit";
    PruneIn in;
    int rc;
    if ((rc = prune_check(fn, child, data, parent_depth, n_internal, N, M, keep, weights, threshold, workspace, workspace_bytes, in)))
        return rc;
    const bool rows = compact_features != 0;
    if (new_n_internal < 1 || new_n_internal > n_internal)
        return set_error(SVOXT_ERR_INVALID, "%s: new_n_internal must be in [1, n_internal]", fn);
    if (new_M < 0 || new_M > M || (!rows && new_M != M))
        return set_error(SVOXT_ERR_INVALID, "%s: new_M must be in [0, M] (M itself without compact_features)", fn);
    if ((int64_t)(uint32_t)empty_index < M) return set_error(SVOXT_ERR_INVALID, "%s: empty_index must be >= M as an unsigned number", fn);
    if (child_out == nullptr || data_out == nullptr || parent_depth_out == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: child_out / data_out / parent_depth_out is NULL", fn);
    if (rows && new_M > 0 && row_map == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: row_map is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    const PruneSpace sp = prune_carve(const_cast<void*>(workspace), n_internal, M);
    hipLaunchKernelGGL(prune_emit_kernel, dim3(launch_blocks(in.slots)), dim3(kPruneBlock), 0, st, in, rows, sp.node_flag, sp.node_rank,
                       sp.row_rank, (int32_t)new_n_internal, empty_index, child_out, data_out, parent_depth_out);
    if (rows && new_M > 0)
        hipLaunchKernelGGL(scatter_ranked_kernel<int64_t>, dim3(launch_blocks(M)), dim3(kLaunchBlock), 0, st, sp.row_flag, sp.row_rank, M,
                           new_M, row_map);
    return check_launch(fn);
}

int svoxt_prune_gather_rows(const float* src, int64_t src_rows, const int64_t* row_map, float* dst, int64_t n, int32_t cols,
                            void* stream) {
    const char* fn = "svoxt_prune_gather_rows";
    if (n < 0 || src_rows < 0 || cols < 1) return set_error(SVOXT_ERR_INVALID, "%s: bad extents", fn);
    if (n == 0) return SVOXT_OK;
    if (src == nullptr || row_map == nullptr || dst == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: NULL argument", fn);
    hipStream_t st = (hipStream_t)stream;
    const bool wide = cols % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
    const int per_row = wide ? cols / 4 : cols;
    if ((double)n * per_row >= 2147483648.0 * kPruneBlock) return set_error(SVOXT_ERR_INVALID, "%s: too many rows for one launch (2^39 threads)", fn);
    const unsigned nb = launch_blocks(n * per_row);
    if (wide) hipLaunchKernelGGL(prune_gather_rows_kernel<4>, dim3(nb), dim3(kPruneBlock), 0, st, src, row_map, dst, n, per_row, src_rows);
    else hipLaunchKernelGGL(prune_gather_rows_kernel<1>, dim3(nb), dim3(kPruneBlock), 0, st, src, row_map, dst, n, per_row, src_rows);
    return check_launch(fn);
}

}  // extern "C"
