// svoxt_merge.hip -- the frontier of a tree (the nodes whose slots are all leaves), reductions over the feature rows of
// a frontier node's children, and N3Tree.merge: a frontier node is removed and its parent slot becomes one leaf.
// C ABI: svoxt_frontier_* / svoxt_merge_* (include/svoxt.h).
//
// The reference has these as tensor ops (merge, reduce_frontier, max_frontier, diam_frontier, _frontier:
// svox_t/svox.py:352-483), stale in this fork: they read the int32 `data` words as values.  Here `data` names rows of
// the feature table, and a child is EMPTY when its word, read as unsigned, is >= M.
//
// frontier   flag a thread per node (all N^3 child words 0, and not the root), exclusive scan (svoxt_order.hip), the
//            host reads F, a thread per node writes its id at its rank: ascending ids.
// reduce     out[f, j] = op over the children c = 0 .. N^3 - 1 of node f of features[data[f, c], cols[j]], in slot
//            order, sequential float32 -- the order is part of the contract (tests compare bits).  That rules out a
//            butterfly across the lanes that hold the 8 children: ((x0 + x1) + (x2 + x3)) + ... is another sum.  So the
//            fast kernel (N = 2, every column, K a multiple of 4, K <= 32) gives a node to 8 lanes instead of a child:
//            lane p of the 8 owns columns 4p .. 4p + 3, issues the 8 children's 16-byte loads back to back (8 rows in
//            flight per lane; the 8 lanes of a node read one 128-byte row together) and adds them in slot order in
//            registers; a wavefront takes 8 nodes a pass and writes 1 KiB of contiguous output.  No cross-lane move
//            is left in reduce; diam needs them: every lane has its 4 columns' share of the 28 squared distances,
//            summed over the node's 8 lanes by three xor steps each.
//            Other N, other K and column subsets take a generic kernel: a thread per (node, column).
// backward   of reduce wrt the feature table: sum / mean scatter the upstream row (divided by the count for mean) to
//            every non-empty child's row, max / min give it to the first slot that attains the extremum; float
//            atomics, as svoxt_query_bwd (rows named by several leaves; where every row is named once there is one
//            add per element into a zeroed table: the same bits every run).
// merge      mark      a thread per node: merged = selected, not the root, all slots leaves.  A node that stays flags
//                      itself and the feature rows its leaves name; a merged node decides its parent slot's new word:
//                      all words equal -> that word (its row is flagged), all children empty -> the first child's
//                      word; otherwise a NEW row: the node flags itself in new_flag
//            scan      node flags, row flags, new-row flags: three exclusive scans; counts = their totals
//            emit      as prune's: a thread per slot of a staying node; a child that was merged becomes a leaf whose
//                      word is the decided one (renumbered) or carried + rank of its new row
//            new rows  the reduce kernel over the merged nodes that got a new row, written behind the carried rows
// Every output word of merge is a function of the input alone.  The emit kernel is a sibling of prune_emit_kernel, not
// shared with it: the two differ in every branch but the parent_depth row (a slot decision there, a node decision and
// a third rank here), and prune's is measured as it stands (profiles/prune_timing.txt); what they share -- the scan,
// the row gather, the parent_depth row, the ranked scatter and the totals behind the scans, the workspace carver and
// the extents / workspace checks -- is used, not copied (exclusive_scan, svoxt_prune_gather_rows, svoxt_workspace.h).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_wave.h"
#include "svoxt_workspace.h"

namespace svoxt {

constexpr int kMergeBlock = kLaunchBlock;
enum { OP_MEAN = SVOXT_REDUCE_MEAN, OP_SUM = SVOXT_REDUCE_SUM, OP_MAX = SVOXT_REDUCE_MAX, OP_MIN = SVOXT_REDUCE_MIN };

typedef float float4v __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------- frontier
// workspace: [flag u32[n + 1]] [rank u32[n + 1]] [chunk sums]
struct FrontierSpace {
    uint32_t *flag, *rank, *chunks;
    size_t bytes;
};

static FrontierSpace frontier_carve(void* workspace, int64_t n) {
    FrontierSpace sp;
    Carver w(workspace);
    sp.flag = w.take<uint32_t>((size_t)n + 1);
    sp.rank = w.take<uint32_t>((size_t)n + 1);
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks((size_t)n + 1));
    sp.bytes = w.bytes();
    return sp;
}

__device__ __forceinline__ bool all_leaves(const int32_t* __restrict__ child, int32_t node, int32_t n3) {
    const int32_t* c = child + (int64_t)node * n3;
    int32_t any = 0;
    for (int k = 0; k < n3; ++k) any |= c[k];
    return any == 0;
}

__global__ void __launch_bounds__(kMergeBlock)
frontier_flag_kernel(const int32_t* __restrict__ child, int32_t n, int32_t n3, uint32_t* __restrict__ flag) {
    const int32_t i = (int32_t)(blockIdx.x * kMergeBlock + threadIdx.x);
    if (i > n) return;
    flag[i] = (i > 0 && i < n && all_leaves(child, i, n3)) ? 1u : 0u;        // (flag[n] = 0: the scan reads n + 1 words)
}

// ------------------------------------------------------------------------------------------------------------ reduce
struct ReduceIn {
    const float* features;
    const int32_t* data;
    const int64_t* nodes;                // [F] node ids
    const int32_t* cols;                 // [Kc] columns of features, or NULL: all K
    int64_t F;
    int32_t n;                           // internal nodes: node ids outside [0, n) read nothing and give a zero row
    int32_t n3;
    uint32_t M;
    int32_t K, Kc;
    int32_t op;
    bool skip;                           // empty children are left out (else: they count as zero rows)
};

// The extremum in slot order: the first slot that attains it wins (a strict comparison; NaN never wins).
__device__ __forceinline__ bool reduce_better(int op, float x, float best) { return op == OP_MAX ? x > best : x < best; }

// One (node, column): the value, and for the backward the slot that gave the extremum (-1: none) and the count.
__device__ __forceinline__ float reduce_column(const ReduceIn& in, const int32_t* __restrict__ words, int col, int& arg, int& count) {
    float acc = 0.f;
    arg = -1;
    count = 0;
    bool first = true;
    for (int c = 0; c < in.n3; ++c) {
        const uint32_t w = (uint32_t)words[c];
        const bool has = w < in.M;
        if (!has && in.skip) continue;
        const float x = has ? in.features[(int64_t)w * in.K + col] : 0.f;
        ++count;
        if (in.op <= OP_SUM) acc = first ? x : acc + x;
        else if (first || reduce_better(in.op, x, acc)) { acc = x; arg = c; }
        first = false;
    }
    if (in.op == OP_MEAN && count > 0) acc = acc / (float)count;
    return acc;
}

__global__ void __launch_bounds__(kMergeBlock)
reduce_generic_kernel(ReduceIn in, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (i >= in.F * in.Kc) return;
    const int64_t f = i / in.Kc;
    const int j = (int)(i - f * in.Kc);
    const int64_t node = in.nodes[f];
    if (node < 0 || node >= in.n) { out[i] = 0.f; return; }
    int arg, count;
    out[i] = reduce_column(in, in.data + node * in.n3, in.cols != nullptr ? in.cols[j] : j, arg, count);
}

// N = 2, all columns, K = 4 * Q4 <= 32: 8 lanes a node, lane p columns 4p .. 4p + 3 (p >= Q4 idles), 8 loads in flight.
struct Rows8 {
    float4v x[8];
    uint32_t has;                        // bit c: child c names a row
};

__device__ __forceinline__ Rows8 load_rows8(const ReduceIn& in, int64_t node, int p, bool live) {
    Rows8 r;
    r.has = 0;
    int32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        const int4* wp = reinterpret_cast<const int4*>(in.data + node * 8);       // 32-byte aligned: a node's 8 words
        const int4 a = wp[0], b = wp[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool has = live && (uint32_t)w[c] < in.M;
        r.x[c] = has ? reinterpret_cast<const float4v*>(in.features + (int64_t)(uint32_t)w[c] * in.K)[p] : (float4v)(0.f);
        r.has |= (has ? 1u : 0u) << c;
    }
    return r;
}

__global__ void __launch_bounds__(kMergeBlock)
reduce_rows8_kernel(ReduceIn in, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    const int64_t f = t >> 3;
    const int p = (int)(t & 7), q4 = in.K >> 2;
    if (f >= in.F || p >= q4) return;
    const int64_t node = in.nodes[f];
    const Rows8 r = load_rows8(in, node, p, node >= 0 && node < in.n);
    float4v acc = (float4v)(0.f);
    int count = 0;
    bool first = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (in.skip && !((r.has >> c) & 1u)) continue;
        ++count;
        if (in.op <= OP_SUM) acc = first ? r.x[c] : acc + r.x[c];
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (first || reduce_better(in.op, r.x[c][e], acc[e])) acc[e] = r.x[c][e];
        }
        first = false;
    }
    if (in.op == OP_MEAN && count > 0) acc = acc / (float)count;
    reinterpret_cast<float4v*>(out + f * in.K)[p] = acc;
}

// Backward of reduce: grad [M, K] += ..., zeroed by the caller of the kernel (the entry point).
__global__ void __launch_bounds__(kMergeBlock)
reduce_bwd_kernel(ReduceIn in, const float* __restrict__ grad_out, float* __restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (i >= in.F * in.Kc) return;
    const int64_t f = i / in.Kc;
    const int j = (int)(i - f * in.Kc);
    const int64_t node = in.nodes[f];
    if (node < 0 || node >= in.n) return;
    const int32_t* words = in.data + node * in.n3;
    const int col = in.cols != nullptr ? in.cols[j] : j;
    int arg, count;
    reduce_column(in, words, col, arg, count);
    float g = grad_out[i];
    if (in.op <= OP_SUM) {
        if (in.op == OP_MEAN && count > 0) g = g / (float)count;
        for (int c = 0; c < in.n3; ++c) {
            const uint32_t w = (uint32_t)words[c];
            if (w < in.M) atomicAdd(grad + (int64_t)w * in.K + col, g);
        }
    } else if (arg >= 0) {
        const uint32_t w = (uint32_t)words[arg];
        if (w < in.M) atomicAdd(grad + (int64_t)w * in.K + col, g);         // (an empty child's zero won: nobody's gradient)
    }
}

// -------------------------------------------------------------------------------------------------------------- diam
// out[f] = max over pairs of children (a < b; under skip: both non-empty) of sqrt(sum_j ((x_a[j] - x_b[j]) * scale)^2)
__global__ void __launch_bounds__(kMergeBlock)
diam_generic_kernel(ReduceIn in, float scale, float* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (f >= in.F) return;
    const int64_t node = in.nodes[f];
    float best = 0.f;
    if (node >= 0 && node < in.n) {
        const int32_t* words = in.data + node * in.n3;
        for (int a = 0; a < in.n3; ++a) {
            const uint32_t wa = (uint32_t)words[a];
            if (wa >= in.M && in.skip) continue;
            for (int b = a + 1; b < in.n3; ++b) {
                const uint32_t wb = (uint32_t)words[b];
                if (wb >= in.M && in.skip) continue;
                if (wa == wb || (wa >= in.M && wb >= in.M)) continue;             // distance 0
                float s = 0.f;
                for (int j = 0; j < in.Kc; ++j) {
                    const int col = in.cols != nullptr ? in.cols[j] : j;
                    const float xa = wa < in.M ? in.features[(int64_t)wa * in.K + col] : 0.f;
                    const float xb = wb < in.M ? in.features[(int64_t)wb * in.K + col] : 0.f;
                    const float d = (xa - xb) * scale;
                    s += d * d;
                }
                best = s > best ? s : best;
            }
        }
    }
    out[f] = sqrtf(best);
}

__global__ void __launch_bounds__(kMergeBlock)
diam_rows8_kernel(ReduceIn in, float scale, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    const int64_t f = t >> 3;                                  // (F is padded to whole wavefronts by the idle lanes: the
    const int p = (int)(t & 7), q4 = in.K >> 2;                //  shuffles below need all 8 lanes of a node present)
    const bool live_node = f < in.F;
    const int64_t node = live_node ? in.nodes[f] : -1;
    const Rows8 r = load_rows8(in, node, p, p < q4 && node >= 0 && node < in.n);
    // a node's `has` bits: the same on its live lanes; lanes p >= q4 hold zeros and no bits
    const uint32_t has = (uint32_t)__shfl((int)r.has, (int)(threadIdx.x & 63 & ~7), 64);
    float best = 0.f;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
#pragma unroll
        for (int b = a + 1; b < 8; ++b) {
            const float4v d = (r.x[a] - r.x[b]) * scale;
            float s = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
            s = wave_group_sum<8>(s);
            const bool counts = !in.skip || (((has >> a) & (has >> b)) & 1u);
            best = (counts && s > best) ? s : best;
        }
    }
    if (live_node && p == 0) out[f] = sqrtf(best);
}

// ------------------------------------------------------------------------------------------------------------- merge
struct MergeIn {
    const int32_t* child;
    const int32_t* data;
    const int32_t* parent_depth;
    const uint8_t* sel;                  // per node: non-zero = merge it if it is a frontier node
    int32_t n, n3;
    uint32_t M;
    int32_t slots;
    bool rows;
};

// workspace: [node_flag u32[n + 1]] [new_flag u32[n + 1]] [row_flag u32[M + 1]] | [word i32[n]] [node_rank] [new_rank]
// [row_rank] [chunk sums]; the flags are what svoxt_merge_count clears
struct MergeSpace {
    uint32_t *node_flag, *new_flag, *row_flag, *node_rank, *new_rank, *row_rank, *chunks;
    int32_t* word;
    size_t clear_bytes, bytes;
};

static MergeSpace merge_carve(void* workspace, int64_t n, int64_t M) {
    MergeSpace sp;
    Carver w(workspace);
    sp.node_flag = w.take<uint32_t>((size_t)n + 1);
    sp.new_flag = w.take<uint32_t>((size_t)n + 1);
    sp.row_flag = w.take<uint32_t>((size_t)M + 1);
    sp.clear_bytes = w.bytes();
    sp.word = w.take<int32_t>((size_t)n + 1);                  // (n words are used: the piece is as long as the flags')
    sp.node_rank = w.take<uint32_t>((size_t)n + 1);
    sp.new_rank = w.take<uint32_t>((size_t)n + 1);
    sp.row_rank = w.take<uint32_t>((size_t)M + 1);
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks((size_t)(n > M ? n : M) + 1));
    sp.bytes = w.bytes();
    return sp;
}

__global__ void __launch_bounds__(kMergeBlock)
merge_mark_kernel(MergeIn in, uint32_t* __restrict__ node_flag, uint32_t* __restrict__ new_flag, uint32_t* __restrict__ row_flag,
                  int32_t* __restrict__ word) {
    const int32_t i = (int32_t)(blockIdx.x * kMergeBlock + threadIdx.x);
    if (i >= in.n) return;
    const int32_t* d = in.data + (int64_t)i * in.n3;
    const int32_t* ch = in.child + (int64_t)i * in.n3;
    const bool merged = i > 0 && in.sel[i] != 0 && all_leaves(in.child, i, in.n3);
    if (!merged) {
        node_flag[i] = 1u;
        if (in.rows)
            for (int k = 0; k < in.n3; ++k) if (ch[k] == 0 && (uint32_t)d[k] < in.M) row_flag[(uint32_t)d[k]] = 1u;   // (all writers store 1)
        return;
    }
    const int32_t w0 = d[0];
    bool equal = true, none = true;
    for (int k = 0; k < in.n3; ++k) {
        equal = equal && d[k] == w0;
        none = none && (uint32_t)d[k] >= in.M;
    }
    if (equal || none) {                                       // the parent slot takes the word: no new row
        word[i] = w0;
        if (in.rows && (uint32_t)w0 < in.M) row_flag[(uint32_t)w0] = 1u;
    } else {
        new_flag[i] = 1u;
    }
}

__global__ void __launch_bounds__(kMergeBlock)
merge_emit_kernel(MergeIn in, MergeSpace sp, int32_t new_n, int64_t carried, int32_t empty_index, int32_t* __restrict__ child_out,
                  int32_t* __restrict__ data_out, int32_t* __restrict__ pd_out) {
    const int32_t s = (int32_t)(blockIdx.x * kMergeBlock + threadIdx.x);
    if (s >= in.slots) return;
    const int32_t node = s / in.n3, k = s - node * in.n3;
    if (sp.node_flag[node] == 0u) return;
    const int32_t id = (int32_t)sp.node_rank[node];
    if (id >= new_n) return;                                     // (the caller's count is the scan's: never taken)
    int32_t c = in.child[s], d = empty_index;
    bool leaf_word = false;
    if (c != 0) {
        const int64_t kid = (int64_t)node + c;
        if (kid < 0 || kid >= in.n) c = 0;                       // (a malformed table: an empty leaf)
        else if (sp.node_flag[kid] != 0u) c = (int32_t)sp.node_rank[kid] - id;
        else {                                                   // the child was merged: this slot is its leaf
            c = 0;
            if (sp.new_flag[kid] != 0u) d = (int32_t)(carried + (int64_t)sp.new_rank[kid]);
            else { d = sp.word[kid]; leaf_word = true; }
        }
    } else {
        d = in.data[s];
        leaf_word = true;
    }
    if (leaf_word && in.rows && (uint32_t)d < in.M) d = (int32_t)sp.row_rank[(uint32_t)d];
    const int64_t at = (int64_t)id * in.n3 + k;
    child_out[at] = c;
    data_out[at] = d;
    if (k == 0) emit_renumbered_parent_depth(in.parent_depth, node, in.n, in.n3, sp.node_rank, id, pd_out);
}

// row_map[rank] = old row, new_nodes[rank] = merged node that gets a new row
__global__ void __launch_bounds__(kMergeBlock)
merge_lists_kernel(MergeSpace sp, int32_t n, uint32_t M, bool rows, int64_t carried, int64_t added, int64_t* __restrict__ row_map,
                   int64_t* __restrict__ new_nodes) {
    const uint32_t i = blockIdx.x * kMergeBlock + threadIdx.x;
    if (rows && i < M && sp.row_flag[i] != 0u && (int64_t)sp.row_rank[i] < carried) row_map[sp.row_rank[i]] = (int64_t)i;
    if (i < (uint32_t)n && sp.new_flag[i] != 0u && (int64_t)sp.new_rank[i] < added) new_nodes[sp.new_rank[i]] = (int64_t)i;
}

// ------------------------------------------------------------------------------------------------- argument checks
static int reduce_check(const char* fn, const float* features, int64_t M, int32_t K, const int32_t* data, int64_t n, int32_t N,
                        const int64_t* nodes, int64_t F, const int32_t* cols, int32_t n_cols, int32_t op, int32_t empty_mode,
                        ReduceIn& in) {
    int rc;
    if ((rc = tree_extents_check(fn, n, N, M))) return rc;
    if (K < 1) return set_error(SVOXT_ERR_INVALID, "%s: K must be >= 1", fn);
    if (F < 0 || n_cols < 0) return set_error(SVOXT_ERR_INVALID, "%s: F and n_cols must be >= 0", fn);
    if (op < OP_MEAN || op > OP_MIN) return set_error(SVOXT_ERR_INVALID, "%s: op must be one of SVOXT_REDUCE_MEAN / SUM / MAX / MIN", fn);
    if (empty_mode != SVOXT_EMPTY_ZERO && empty_mode != SVOXT_EMPTY_SKIP)
        return set_error(SVOXT_ERR_INVALID, "%s: empty_mode must be SVOXT_EMPTY_ZERO or SVOXT_EMPTY_SKIP", fn);
    if ((n_cols > 0) != (cols != nullptr)) return set_error(SVOXT_ERR_INVALID, "%s: cols and n_cols go together", fn);
    const int32_t Kc = cols != nullptr ? n_cols : K;
    if ((double)F * Kc >= 2147483648.0 * 32) return set_error(SVOXT_ERR_INVALID, "%s: F * columns must be below 2^36", fn);
    if (F > 0 && (data == nullptr || nodes == nullptr || (M > 0 && features == nullptr)))
        return set_error(SVOXT_ERR_INVALID, "%s: features / data / nodes is NULL", fn);
    in.features = features; in.data = data; in.nodes = nodes; in.cols = cols;
    in.F = F; in.n = (int32_t)n; in.n3 = N * N * N; in.M = (uint32_t)M; in.K = K; in.Kc = Kc; in.op = op;
    in.skip = empty_mode == SVOXT_EMPTY_SKIP;
    return SVOXT_OK;
}

// the 8-lanes-a-node kernels: an octree, every column, rows of whole 16-byte pieces that start on 16-byte lines
static bool rows8(const ReduceIn& in, const float* out, bool out_rows) {
    return in.n3 == 8 && in.cols == nullptr && in.K % 4 == 0 && in.K <= 32 && (uintptr_t)in.features % 16 == 0 &&
           (uintptr_t)in.data % 16 == 0 && (!out_rows || (uintptr_t)out % 16 == 0);
}

static int merge_check(const char* fn, const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n, int32_t N,
                       int64_t M, const uint8_t* sel, int32_t compact_features, const void* workspace,
                       int64_t workspace_bytes, MergeIn& in) {
    int rc;
    if ((rc = tree_extents_check(fn, n, N, M))) return rc;
    if (child == nullptr || data == nullptr || parent_depth == nullptr || sel == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: child / data / parent_depth / selected is NULL", fn);
    if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_merge_workspace_bytes(n, M),
                              "svoxt_merge_workspace_bytes(n_internal, M)")))
        return rc;
    in.child = child; in.data = data; in.parent_depth = parent_depth; in.sel = sel;
    in.n = (int32_t)n; in.n3 = N * N * N; in.M = (uint32_t)M; in.slots = (int32_t)(n * in.n3);
    in.rows = compact_features != 0;
    return SVOXT_OK;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_frontier_workspace_bytes(int64_t n_internal) {
    if (n_internal < 1 || n_internal > 0x7fffffff) return -1;
    return (int64_t)frontier_carve(nullptr, n_internal).bytes;
}

int svoxt_frontier_count(const int32_t* child, int64_t n_internal, int32_t N, void* workspace, int64_t workspace_bytes,
                         int64_t* count, void* stream) {
    const char* fn = "svoxt_frontier_count";
    int rc;
    if ((rc = tree_extents_check(fn, n_internal, N, 0))) return rc;
    if (child == nullptr || count == nullptr || workspace == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: child / count / workspace is NULL", fn);
    if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_frontier_workspace_bytes(n_internal),
                              "svoxt_frontier_workspace_bytes(n_internal)")))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const FrontierSpace sp = frontier_carve(workspace, n_internal);
    hipLaunchKernelGGL(frontier_flag_kernel, dim3(launch_blocks(n_internal + 1)), dim3(kMergeBlock), 0, st, child, (int32_t)n_internal,
                       N * N * N, sp.flag);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.flag, (size_t)n_internal + 1, sp.chunks, sp.rank, st, fn))) return rc;
    hipLaunchKernelGGL(rank_totals_kernel<1>, dim3(1), dim3(64), 0, st, RankTotals<1>{{sp.rank}, {n_internal}}, count);
    return check_launch(fn);
}

int svoxt_frontier_emit(const void* workspace, int64_t workspace_bytes, int64_t n_internal, int64_t F, int64_t* frontier, void* stream) {
    const char* fn = "svoxt_frontier_emit";
    if (n_internal < 1 || n_internal > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: n_internal must be in [1, 2^31)", fn);
    if (F < 0 || F > n_internal - 1) return set_error(SVOXT_ERR_INVALID, "%s: F must be in [0, n_internal)", fn);
    int rc;
    if ((rc = workspace_check(fn, workspace, workspace_bytes, svoxt_frontier_workspace_bytes(n_internal),
                              "svoxt_frontier_workspace_bytes(n_internal)")))
        return rc;
    if (F == 0) return SVOXT_OK;
    if (frontier == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: frontier is NULL", fn);
    const FrontierSpace sp = frontier_carve(const_cast<void*>(workspace), n_internal);
    hipLaunchKernelGGL(scatter_ranked_kernel<int64_t>, dim3(launch_blocks(n_internal)), dim3(kLaunchBlock), 0, (hipStream_t)stream, sp.flag,
                       sp.rank, n_internal, F, frontier);
    return check_launch(fn);
}

int svoxt_frontier_reduce(const float* features, int64_t M, int32_t K, const int32_t* data, int64_t n_internal, int32_t N,
                          const int64_t* nodes, int64_t F, const int32_t* cols, int32_t n_cols, int32_t op, int32_t empty_mode,
                          float* out, void* stream) {
    const char* fn = "svoxt_frontier_reduce";
    ReduceIn in;
    int rc;
    if ((rc = reduce_check(fn, features, M, K, data, n_internal, N, nodes, F, cols, n_cols, op, empty_mode, in))) return rc;
    if (F == 0) return SVOXT_OK;
    if (out == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: out is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    if (rows8(in, out, true)) hipLaunchKernelGGL(reduce_rows8_kernel, dim3(launch_blocks(F * 8)), dim3(kMergeBlock), 0, st, in, out);
    else hipLaunchKernelGGL(reduce_generic_kernel, dim3(launch_blocks(F * in.Kc)), dim3(kMergeBlock), 0, st, in, out);
    return check_launch(fn);
}

int svoxt_frontier_reduce_bwd(const float* features, int64_t M, int32_t K, const int32_t* data, int64_t n_internal, int32_t N,
                              const int64_t* nodes, int64_t F, const int32_t* cols, int32_t n_cols, int32_t op, int32_t empty_mode,
                              const float* grad_out, float* grad_features, void* stream) {
    const char* fn = "svoxt_frontier_reduce_bwd";
    ReduceIn in;
    int rc;
    if ((rc = reduce_check(fn, features, M, K, data, n_internal, N, nodes, F, cols, n_cols, op, empty_mode, in))) return rc;
    if (M > 0 && grad_features == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: grad_features is NULL", fn);
    if (F > 0 && grad_out == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: grad_out is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    if (M > 0) {
        const hipError_t e = hipMemsetAsync(grad_features, 0, sizeof(float) * (size_t)M * K, st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    }
    if (F == 0 || M == 0) return SVOXT_OK;
    hipLaunchKernelGGL(reduce_bwd_kernel, dim3(launch_blocks(F * in.Kc)), dim3(kMergeBlock), 0, st, in, grad_out, grad_features);
    return check_launch(fn);
}

int svoxt_frontier_diam(const float* features, int64_t M, int32_t K, const int32_t* data, int64_t n_internal, int32_t N,
                        const int64_t* nodes, int64_t F, const int32_t* cols, int32_t n_cols, int32_t empty_mode, float scale,
                        float* out, void* stream) {
    const char* fn = "svoxt_frontier_diam";
    ReduceIn in;
    int rc;
    if ((rc = reduce_check(fn, features, M, K, data, n_internal, N, nodes, F, cols, n_cols, OP_MAX, empty_mode, in))) return rc;
    if (scale != scale) return set_error(SVOXT_ERR_INVALID, "%s: scale is NaN", fn);
    if (F == 0) return SVOXT_OK;
    if (out == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: out is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    if (rows8(in, out, false)) hipLaunchKernelGGL(diam_rows8_kernel, dim3(launch_blocks(F * 8)), dim3(kMergeBlock), 0, st, in, scale, out);
    else hipLaunchKernelGGL(diam_generic_kernel, dim3(launch_blocks(F)), dim3(kMergeBlock), 0, st, in, scale, out);
    return check_launch(fn);
}

int64_t svoxt_merge_workspace_bytes(int64_t n_internal, int64_t M) {
    if (n_internal < 1 || n_internal > 0x7fffffff || M < 0 || M > 0x7fffffff) return -1;
    return (int64_t)merge_carve(nullptr, n_internal, M).bytes;
}

int svoxt_merge_count(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal, int32_t N,
                      int64_t M, const uint8_t* selected, int32_t compact_features, void* workspace,
                      int64_t workspace_bytes, int64_t* counts, void* stream) {
    const char* fn = "svoxt_merge_count";
    MergeIn in;
    int rc;
    if ((rc = merge_check(fn, child, data, parent_depth, n_internal, N, M, selected, compact_features, workspace,
                          workspace_bytes, in)))
        return rc;
    if (counts == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: counts is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    const MergeSpace sp = merge_carve(workspace, n_internal, M);
    const hipError_t e = hipMemsetAsync(workspace, 0, sp.clear_bytes, st);
    if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(merge_mark_kernel, dim3(launch_blocks(n_internal)), dim3(kMergeBlock), 0, st, in, sp.node_flag, sp.new_flag,
                       sp.row_flag, sp.word);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(sp.node_flag, (size_t)n_internal + 1, sp.chunks, sp.node_rank, st, fn)) ||
        (rc = exclusive_scan(sp.new_flag, (size_t)n_internal + 1, sp.chunks, sp.new_rank, st, fn)))
        return rc;
    if (in.rows && (rc = exclusive_scan(sp.row_flag, (size_t)M + 1, sp.chunks, sp.row_rank, st, fn))) return rc;
    // counts[0] = nodes that remain, counts[1] = old feature rows carried (all M where rows are not compacted), counts[2] = new rows
    const RankTotals<3> totals = {{sp.node_rank, in.rows ? sp.row_rank : nullptr, sp.new_rank}, {n_internal, M, n_internal}};
    hipLaunchKernelGGL(rank_totals_kernel<3>, dim3(1), dim3(64), 0, st, totals, counts);
    return check_launch(fn);
}

int svoxt_merge_emit(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal, int32_t N,
                     int64_t M, const uint8_t* selected, int32_t compact_features, const void* workspace,
                     int64_t workspace_bytes, int64_t new_n_internal, int64_t carried, int64_t rows_added, int32_t empty_index,
                     int32_t* child_out, int32_t* data_out, int32_t* parent_depth_out, int64_t* row_map, int64_t* new_row_nodes,
                     void* stream) {
    const char* fn = "svoxt_merge_emit";
    MergeIn in;
    int rc;
    if ((rc = merge_check(fn, child, data, parent_depth, n_internal, N, M, selected, compact_features, workspace,
                          workspace_bytes, in)))
        return rc;
    if (new_n_internal < 1 || new_n_internal > n_internal)
        return set_error(SVOXT_ERR_INVALID, "%s: new_n_internal must be in [1, n_internal]", fn);
    if (carried < 0 || carried > M || (!in.rows && carried != M))
        return set_error(SVOXT_ERR_INVALID, "%s: carried must be in [0, M] (M itself without compact_features)", fn);
    if (rows_added < 0 || rows_added > n_internal - new_n_internal)
        return set_error(SVOXT_ERR_INVALID, "%s: rows_added must be in [0, n_internal - new_n_internal]", fn);
    if (carried + rows_added > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: carried + rows_added must be below 2^31", fn);
    if ((int64_t)(uint32_t)empty_index < carried + rows_added || (int64_t)(uint32_t)empty_index < M)
        return set_error(SVOXT_ERR_INVALID, "%s: empty_index must be >= M and >= the new number of rows as an unsigned number", fn);
    if (child_out == nullptr || data_out == nullptr || parent_depth_out == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: child_out / data_out / parent_depth_out is NULL", fn);
    if (in.rows && carried > 0 && row_map == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: row_map is NULL", fn);
    if (rows_added > 0 && new_row_nodes == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: new_row_nodes is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    const MergeSpace sp = merge_carve(const_cast<void*>(workspace), n_internal, M);
    hipLaunchKernelGGL(merge_emit_kernel, dim3(launch_blocks(in.slots)), dim3(kMergeBlock), 0, st, in, sp, (int32_t)new_n_internal, carried,
                       empty_index, child_out, data_out, parent_depth_out);
    if ((in.rows && carried > 0) || rows_added > 0)
        hipLaunchKernelGGL(merge_lists_kernel, dim3(launch_blocks((M > n_internal ? M : n_internal))), dim3(kMergeBlock), 0, st, sp, in.n,
                           in.M, in.rows && carried > 0, carried, rows_added, row_map, new_row_nodes);
    return check_launch(fn);
}

}  // extern "C"
