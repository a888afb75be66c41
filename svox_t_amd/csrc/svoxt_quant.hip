// svoxt_quant.hip -- quantize_median_cut: median-cut palette quantisation of a feature table (the reference's
// svox_t/csrc/quantizer.cpp:48-157, a single-threaded CPU recursion), and the remap of a tree's data words through the
// colour-id map.
//
// The recursion is run level by level: all segments of a level at once, `order` levels, nothing read back.  State:
// `perm` (position -> row; the rows of a segment are consecutive positions), seg_start (segment -> first position,
// closed by M), pos_seg (position -> segment), row_seg (row -> segment; the caller's color_id_map holds it).  A level:
//   1. extremes: per (segment, column) min and max, integer atomicMin / atomicMax on order-preserving uint32 encodings
//      of the floats (-0.0 counted as +0.0); the rows are walked in position order, so a wavefront spans few segments,
//      and each run of equal segment within it is reduced with shuffles first: one pair of atomics per run and column.
//   2. choose: a thread per segment takes the first column with the largest float32 (max - min); a segment of <= 1
//      rows is closed: it has no column, splits no further and keeps its place.
//   3. sort: key[row] = the encoding of the row's value in its segment's column; a stable LSD radix sort from the
//      identity row order, four 8-bit passes over the key, then the passes the segment id needs (level bits): the
//      order (segment, value, row) without a wider key.  The passes are svoxt_sort.h's, shared with voxelize.
//   4. cut: unweighted l + (r - l) / 2.  Weighted: a float64 segmented inclusive scan of the weights in sorted order
//      (256 positions a workgroup, the workgroups' tails scanned by one workgroup), then the first position whose
//      prefix is > 0.5 x the segment's total (integer atomicMin, one per rising edge), r where none is.
//   5. split: an open segment gives two children (an empty one included), a closed one carries over; an exclusive scan
//      of 2 / 1 gives the slots; pos_seg and row_seg are rewritten.
// After the last level the segment number is the colour index (the reference's depth-first emission order is the
// left-to-right order of the closed segments), and a colour is the segment's (weighted) mean: float64 sums of fixed
// shape (a lane or thread strides the segment, then a shuffle tree), rounded once to float32.
// No float atomics anywhere: the result is a function of the inputs, bit-identical from run to run.

#include <hip/hip_runtime.h>

#include "svoxt_host.h"
#include "svoxt_sort.h"
#include "svoxt_wave.h"
#include "svoxt_workspace.h"

namespace svoxt {

constexpr int kQBlock = 256;
constexpr uint32_t kQClosed = 0xffffffffu;             // seg_col of a segment that splits no further

// float -> uint32 with the floats' order (the sign of zero dropped: x + 0 is +0 for both zeros) and back
__device__ __forceinline__ uint32_t q_encode(float x) {
    const uint32_t u = __float_as_uint(x + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float q_decode(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

__global__ void q_init_kernel(uint32_t* __restrict__ seg_start, uint32_t* __restrict__ n_seg, uint32_t n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { seg_start[0] = 0; seg_start[1] = n; *n_seg = 1; }
}

__global__ void __launch_bounds__(kQBlock)
q_ext_init_kernel(uint2* __restrict__ ext, size_t count) {
    const size_t i = (size_t)blockIdx.x * kQBlock + threadIdx.x;
    if (i < count) ext[i] = make_uint2(0xffffffffu, 0u);
}

// 1. perm NULL = the identity
__global__ void __launch_bounds__(kQBlock)
q_extremes_kernel(const float* __restrict__ data, int K, uint32_t n, const uint32_t* __restrict__ perm,
                  const uint32_t* __restrict__ pos_seg, uint32_t* __restrict__ ext) {
    const uint32_t pos = blockIdx.x * kQBlock + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = pos < n;
    const size_t row = valid ? (perm != nullptr ? perm[pos] : pos) : 0;
    const uint32_t seg = valid ? pos_seg[pos] : 0xffffffffu;
    const bool head = lane == 0 || (uint32_t)__shfl_up((int)seg, 1, 64) != seg;
    uint32_t same = 0;                                       // bit k: lane + 2^k is in this lane's run
    for (int k = 0; k < 6; ++k) {
        const uint32_t other = (uint32_t)__shfl_down((int)seg, 1u << k, 64);
        if (lane + (1u << k) < 64 && other == seg) same |= 1u << k;
    }
    for (int c = 0; c < K; ++c) {
        const uint32_t v = valid ? q_encode(data[row * K + c]) : 0u;
        uint32_t mn = v, mx = v;
        for (int k = 0; k < 6; ++k) {
            const uint32_t omn = (uint32_t)__shfl_down((int)mn, 1u << k, 64), omx = (uint32_t)__shfl_down((int)mx, 1u << k, 64);
            if (same >> k & 1u) { mn = min(mn, omn); mx = max(mx, omx); }
        }
        if (valid && head) {
            atomicMin(&ext[((size_t)seg * K + c) * 2], mn);
            atomicMax(&ext[((size_t)seg * K + c) * 2 + 1], mx);
        }
    }
}

// 2. one thread per segment slot of this level (bound + 1 of them: counts past the last segment are 0 for the scan)
__global__ void __launch_bounds__(kQBlock)
q_choose_kernel(const uint32_t* __restrict__ ext, int K, const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ n_seg,
                uint32_t bound, uint32_t* __restrict__ seg_col, uint32_t* __restrict__ counts, uint32_t* __restrict__ cut) {
    const uint32_t s = blockIdx.x * kQBlock + threadIdx.x;
    if (s > bound) return;
    if (s >= *n_seg) { counts[s] = 0; return; }
    const uint32_t l = seg_start[s], r = seg_start[s + 1];
    const bool open = r - l > 1;
    uint32_t col = kQClosed;
    if (open) {
        float best = -1.f;
        col = 0;
        for (int c = 0; c < K; ++c) {
            const float range = q_decode(ext[((size_t)s * K + c) * 2 + 1]) - q_decode(ext[((size_t)s * K + c) * 2]);
            if (range > best) { best = range; col = (uint32_t)c; }
        }
    }
    seg_col[s] = col;
    counts[s] = open ? 2u : 1u;
    cut[s] = r;
}

// 3. the sort key of every row, in row order
__global__ void __launch_bounds__(kQBlock)
q_key_kernel(const float* __restrict__ data, int K, uint32_t n, const uint32_t* __restrict__ row_seg,
             const uint32_t* __restrict__ seg_col, uint32_t* __restrict__ keys) {
    const uint32_t row = blockIdx.x * kQBlock + threadIdx.x;
    if (row >= n) return;
    const uint32_t col = seg_col[row_seg[row]];
    keys[row] = col == kQClosed ? 0u : q_encode(data[(size_t)row * K + col]);
}

// keys[i] = the segment of the row at i of the order the value passes left
__global__ void __launch_bounds__(kQBlock)
q_seg_key_kernel(const uint32_t* __restrict__ row_seg, const uint32_t* __restrict__ rows, uint32_t n, uint32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * kQBlock + threadIdx.x;
    if (i < n) keys[i] = row_seg[rows[i]];
}

// 4. Segmented inclusive scan over the 256 threads of a workgroup: (f, v) = (a segment starts in the span behind v, the
// sum since that start or since the span's beginning).  earlier (+) later = (f1 | f2, f2 ? v2 : v1 + v2).
__device__ __forceinline__ void q_block_segscan(bool& f, double& v, double* sv, uint32_t* sf) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const int f2 = __shfl_up((int)f, off, 64);
        const double v2 = __shfl_up(v, off, 64);
        if (lane >= off) {
            if (!f) v = v2 + v;
            f = f || f2 != 0;
        }
    }
    if (lane == 63) { sv[wave] = v; sf[wave] = f ? 1u : 0u; }
    __syncthreads();
    bool cf = false;
    double cv = 0.0;
    for (uint32_t j = 0; j < wave; ++j) {
        if (sf[j]) { cv = sv[j]; cf = true; } else cv = cv + sv[j];
    }
    if (!f) v = cv + v;
    f = f || cf;
    __syncthreads();
}

__global__ void __launch_bounds__(kQBlock)
q_wscan_local_kernel(const float* __restrict__ weights, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pos_seg,
                     const uint32_t* __restrict__ seg_start, uint32_t n, double* __restrict__ local, double* __restrict__ agg_v,
                     uint32_t* __restrict__ agg_f) {
    __shared__ double sv[4];
    __shared__ uint32_t sf[4];
    const uint32_t pos = blockIdx.x * kQBlock + threadIdx.x;
    const bool valid = pos < n;
    double v = valid ? (double)weights[perm[pos]] : 0.0;
    bool f = valid ? seg_start[pos_seg[pos]] == pos : true;
    q_block_segscan(f, v, sv, sf);
    if (valid) local[pos] = v;
    if (threadIdx.x == kQBlock - 1) { agg_v[blockIdx.x] = v; agg_f[blockIdx.x] = f ? 1u : 0u; }
}

// the workgroups' tails, scanned in place by one workgroup, 256 at a time with a carry
__global__ void __launch_bounds__(kQBlock)
q_wscan_chunks_kernel(double* __restrict__ agg_v, uint32_t* __restrict__ agg_f, uint32_t n_chunks) {
    __shared__ double sv[4];
    __shared__ uint32_t sf[4];
    __shared__ double last_v;
    __shared__ uint32_t last_f;
    bool cf = false;
    double cv = 0.0;
    for (uint32_t base = 0; base < n_chunks; base += kQBlock) {
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < n_chunks;
        bool f = valid ? agg_f[i] != 0 : false;
        double v = valid ? agg_v[i] : 0.0;
        q_block_segscan(f, v, sv, sf);
        if (!f) v = cv + v;
        f = f || cf;
        if (valid) { agg_v[i] = v; agg_f[i] = f ? 1u : 0u; }
        if (threadIdx.x == kQBlock - 1) { last_v = v; last_f = f ? 1u : 0u; }
        __syncthreads();
        cv = last_v;
        cf = last_f != 0;
        __syncthreads();
    }
}

// the inclusive prefix at pos of a segment that starts at l
__device__ __forceinline__ double q_prefix(const double* __restrict__ local, const double* __restrict__ agg_v, uint32_t pos, uint32_t l) {
    const uint32_t chunk = pos / kQBlock;
    const double v = local[pos];
    return chunk > 0 && l < chunk * kQBlock ? agg_v[chunk - 1] + v : v;
}

__global__ void __launch_bounds__(kQBlock)
q_wcut_kernel(const double* __restrict__ local, const double* __restrict__ agg_v, const uint32_t* __restrict__ pos_seg,
              const uint32_t* __restrict__ seg_start, uint32_t n, uint32_t* __restrict__ cut) {
    const uint32_t pos = blockIdx.x * kQBlock + threadIdx.x;
    if (pos >= n) return;
    const uint32_t s = pos_seg[pos], l = seg_start[s], r = seg_start[s + 1];
    if (r - l <= 1) return;
    const double half = 0.5 * q_prefix(local, agg_v, r - 1, l);
    if (!(q_prefix(local, agg_v, pos, l) > half)) return;
    if (pos > l && q_prefix(local, agg_v, pos - 1, l) > half) return;       // not the first of its run
    atomicMin(&cut[s], pos);
}

// 5. the next level's segment table
__global__ void __launch_bounds__(kQBlock)
q_split_kernel(const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ n_seg, const uint32_t* __restrict__ slots,
               const uint32_t* __restrict__ cut, int weighted, uint32_t n, uint32_t* __restrict__ new_start,
               uint32_t* __restrict__ new_n_seg) {
    const uint32_t s = blockIdx.x * kQBlock + threadIdx.x, ns = *n_seg;
    if (s >= ns) return;
    const uint32_t l = seg_start[s], r = seg_start[s + 1], slot = slots[s];
    const bool open = r - l > 1;
    new_start[slot] = l;
    if (open) new_start[slot + 1] = weighted ? cut[s] : l + (r - l) / 2;
    if (s == ns - 1) {
        const uint32_t total = slot + (open ? 2u : 1u);
        new_start[total] = n;
        *new_n_seg = total;
    }
}

__global__ void __launch_bounds__(kQBlock)
q_rewrite_kernel(const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ new_start,
                 const uint32_t* __restrict__ perm, uint32_t n, uint32_t* __restrict__ pos_seg, uint32_t* __restrict__ row_seg) {
    const uint32_t pos = blockIdx.x * kQBlock + threadIdx.x;
    if (pos >= n) return;
    const uint32_t s = pos_seg[pos], slot = slots[s];
    const bool open = seg_start[s + 1] - seg_start[s] > 1;
    const uint32_t to = slot + (open && pos >= new_start[slot + 1] ? 1u : 0u);
    pos_seg[pos] = to;
    row_seg[perm[pos]] = to;
}

// Colours: T threads (a wavefront, or the workgroup) per (segment, column); thread j adds the rows at l + j, l + j + T,
// ... in float64, a shuffle tree adds the threads, wavefront 0 the wavefronts' sums in order.  An empty segment's row is
// left as it was (zero).  weights NULL = unweighted; a weight sum of zero falls back to the plain mean.
template <int T>
__global__ void __launch_bounds__(kQBlock)
q_color_kernel(const float* __restrict__ data, int K, const float* __restrict__ weights, const uint32_t* __restrict__ perm,
               const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ n_seg, float* __restrict__ colors) {
    __shared__ double part[3][kQBlock / 64];
    const uint32_t s = blockIdx.x;
    if (s >= *n_seg) return;
    const uint32_t l = seg_start[s], r = seg_start[s + 1];
    if (r == l) return;
    constexpr int kCols = kQBlock / T;                       // columns a workgroup works on at once
    const uint32_t sub = threadIdx.x % T, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c0 = (int)blockIdx.y * kCols; c0 < K; c0 += (int)gridDim.y * kCols) {
        const int c = c0 + (int)(threadIdx.x / T);
        double sx = 0.0, swx = 0.0, sw = 0.0;
        if (c < K)
            for (uint32_t pos = l + sub; pos < r; pos += T) {
                const size_t row = perm != nullptr ? perm[pos] : pos;
                const double x = (double)data[row * K + c];
                sx = sx + x;
                if (weights != nullptr) {
                    const double w = (double)weights[row];
                    swx = swx + w * x;
                    sw = sw + w;
                }
            }
        sx = wave_sum(sx); swx = wave_sum(swx); sw = wave_sum(sw);   // (each sum its own chain: the same bits as one loop over the three)
        if constexpr (T > 64) {
            if (lane == 0) { part[0][wave] = sx; part[1][wave] = swx; part[2][wave] = sw; }
            __syncthreads();
            if (threadIdx.x == 0)
                for (int j = 1; j < kQBlock / 64; ++j) { sx = sx + part[0][j]; swx = swx + part[1][j]; sw = sw + part[2][j]; }
            __syncthreads();
        }
        if (sub == 0 && c < K)
            colors[(size_t)s * K + c] = (float)(weights != nullptr && sw != 0.0 ? swx / sw : sx / (double)(r - l));
    }
}

__global__ void __launch_bounds__(kQBlock)
q_remap_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t n, const int32_t* __restrict__ map, uint32_t M) {
    const int64_t i = (int64_t)blockIdx.x * kQBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t w = in[i];
    out[i] = (uint32_t)w < M ? map[(uint32_t)w] : w;
}

struct QuantSpace {
    uint32_t n_chunks;                       // workgroups of the weight scan
    uint32_t *keys[2], *vals[2], *pos_seg, *seg_start[2], *n_seg, *seg_col, *counts, *slots, *cut, *ext, *sort_counts, *sort_starts,
             *chunks, *agg_f;
    double *local, *agg_v;                   // (the three pieces of the weight scan: empty unless weighted)
    size_t bytes;
};

static int q_check(int64_t M, int32_t K, int32_t order, const char* fn) {
    if (order < 0 || order > 16) return set_error(SVOXT_ERR_INVALID, "%s: order must be in [0, 16]", fn);
    if (K < 1) return set_error(SVOXT_ERR_INVALID, "%s: data needs at least one column", fn);
    if (M > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the number of rows must be below 2^31", fn);
    if (M < ((int64_t)1 << order)) return set_error(SVOXT_ERR_INVALID, "%s: 2^order colours need at least 2^order rows", fn);
    return SVOXT_OK;
}

static QuantSpace q_carve(void* workspace, int64_t M, int32_t K, int32_t order, bool weighted) {
    QuantSpace sp;
    Carver w(workspace);
    const size_t n = (size_t)M, S = (size_t)1 << order;
    const size_t sortw = (size_t)256 * sort_blocks((uint64_t)M);
    sp.n_chunks = (uint32_t)((n + kQBlock - 1) / kQBlock);
    for (int b = 0; b < 2; ++b) { sp.keys[b] = w.take<uint32_t>(n); sp.vals[b] = w.take<uint32_t>(n); }
    sp.pos_seg = w.take<uint32_t>(n);
    for (int b = 0; b < 2; ++b) sp.seg_start[b] = w.take<uint32_t>(S + 1);
    sp.n_seg = w.take<uint32_t>(2);
    sp.seg_col = w.take<uint32_t>(S);
    sp.counts = w.take<uint32_t>(S + 1);
    sp.slots = w.take<uint32_t>(S + 1);
    sp.cut = w.take<uint32_t>(S);
    sp.ext = w.take<uint32_t>(2 * S * (size_t)K);
    sp.sort_counts = w.take<uint32_t>(sortw);
    sp.sort_starts = w.take<uint32_t>(sortw);
    sp.chunks = w.take<uint32_t>(exclusive_scan_chunks(sortw > S + 1 ? sortw : S + 1));
    sp.local = w.take<double>(weighted ? n : 0);
    sp.agg_v = w.take<double>(weighted ? sp.n_chunks : 0);
    sp.agg_f = w.take<uint32_t>(weighted ? sp.n_chunks : 0);
    sp.bytes = w.bytes();
    return sp;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_quantize_workspace_bytes(int64_t M, int32_t K, int32_t order, int32_t weighted) {
    if (q_check(M, K, order, "svoxt_quantize_workspace_bytes") != SVOXT_OK) return -1;
    return (int64_t)q_carve(nullptr, M, K, order, weighted != 0).bytes;
}

int svoxt_quantize_median_cut(const float* data, int64_t M, int32_t K, const float* weights, int32_t order, float* colors,
                              int32_t* color_id_map, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_quantize_median_cut";
    int rc;
    if ((rc = q_check(M, K, order, fn))) return rc;
    if (data == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: data is NULL", fn);
    if (colors == nullptr || color_id_map == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: colors / color_id_map is NULL", fn);
    if (workspace == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: workspace is NULL", fn);
    const bool weighted = weights != nullptr;
    const QuantSpace sp = q_carve(workspace, M, K, order, weighted);
    if (workspace_bytes < (int64_t)sp.bytes) return set_error(SVOXT_ERR_INVALID, "%s: workspace too small", fn);
    hipStream_t st = (hipStream_t)stream;
    uint32_t* row_seg = reinterpret_cast<uint32_t*>(color_id_map);
    const uint32_t n = (uint32_t)M, S = 1u << order;
    const unsigned nb = (n + kQBlock - 1) / kQBlock;
    auto blocks = [](size_t items) { return dim3((unsigned)((items + kQBlock - 1) / kQBlock)); };

    hipError_t e = hipMemsetAsync(colors, 0, sizeof(float) * (size_t)S * K, st);
    if (e == hipSuccess) e = hipMemsetAsync(row_seg, 0, sizeof(uint32_t) * (size_t)n, st);
    if (e == hipSuccess) e = hipMemsetAsync(sp.pos_seg, 0, sizeof(uint32_t) * (size_t)n, st);
    if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(q_init_kernel, dim3(1), dim3(64), 0, st, sp.seg_start[0], sp.n_seg, n);
    if ((rc = check_launch(fn))) return rc;

    const uint32_t* perm = nullptr;          // the identity before the first sort
    int cur = 0, tab = 0;                    // the sort's current buffers; the current segment table
    for (int level = 0; level < order; ++level) {
        const uint32_t bound = 1u << level;  // segments at this level, at most
        hipLaunchKernelGGL(q_ext_init_kernel, blocks((size_t)bound * K), dim3(kQBlock), 0, st, reinterpret_cast<uint2*>(sp.ext), (size_t)bound * K);
        hipLaunchKernelGGL(q_extremes_kernel, dim3(nb), dim3(kQBlock), 0, st, data, (int)K, n, perm, sp.pos_seg, sp.ext);
        hipLaunchKernelGGL(q_choose_kernel, blocks((size_t)bound + 1), dim3(kQBlock), 0, st, sp.ext, (int)K, sp.seg_start[tab], sp.n_seg + tab, bound, sp.seg_col,
                           sp.counts, sp.cut);
        hipLaunchKernelGGL(q_key_kernel, dim3(nb), dim3(kQBlock), 0, st, data, (int)K, n, row_seg, sp.seg_col, sp.keys[cur]);
        if ((rc = check_launch(fn))) return rc;
        for (int shift = 0; shift < 32; shift += 8) {
            if ((rc = sort_pass(sp.keys[cur], shift == 0 ? nullptr : sp.vals[cur], n, shift, 8, sp.sort_counts, sp.sort_starts, sp.chunks, sp.keys[cur ^ 1],
                                sp.vals[cur ^ 1], st, fn))) return rc;
            cur ^= 1;
        }
        if (level > 0) {
            hipLaunchKernelGGL(q_seg_key_kernel, dim3(nb), dim3(kQBlock), 0, st, row_seg, sp.vals[cur], n, sp.keys[cur]);
            if ((rc = check_launch(fn))) return rc;
            for (int shift = 0; shift < level; shift += 8) {
                if ((rc = sort_pass(sp.keys[cur], sp.vals[cur], n, shift, level - shift < 8 ? level - shift : 8, sp.sort_counts, sp.sort_starts, sp.chunks,
                                    sp.keys[cur ^ 1], sp.vals[cur ^ 1], st, fn))) return rc;
                cur ^= 1;
            }
        }
        perm = sp.vals[cur];
        if (weighted) {
            hipLaunchKernelGGL(q_wscan_local_kernel, dim3(sp.n_chunks), dim3(kQBlock), 0, st, weights, perm, sp.pos_seg, sp.seg_start[tab], n, sp.local,
                               sp.agg_v, sp.agg_f);
            hipLaunchKernelGGL(q_wscan_chunks_kernel, dim3(1), dim3(kQBlock), 0, st, sp.agg_v, sp.agg_f, sp.n_chunks);
            hipLaunchKernelGGL(q_wcut_kernel, dim3(nb), dim3(kQBlock), 0, st, sp.local, sp.agg_v, sp.pos_seg, sp.seg_start[tab], n, sp.cut);
            if ((rc = check_launch(fn))) return rc;
        }
        if ((rc = exclusive_scan(sp.counts, (size_t)bound + 1, sp.chunks, sp.slots, st, fn))) return rc;
        hipLaunchKernelGGL(q_split_kernel, blocks(bound), dim3(kQBlock), 0, st, sp.seg_start[tab], sp.n_seg + tab, sp.slots, sp.cut, weighted ? 1 : 0, n,
                           sp.seg_start[tab ^ 1], sp.n_seg + (tab ^ 1));
        hipLaunchKernelGGL(q_rewrite_kernel, dim3(nb), dim3(kQBlock), 0, st, sp.seg_start[tab], sp.slots, sp.seg_start[tab ^ 1], perm, n, sp.pos_seg, row_seg);
        if ((rc = check_launch(fn))) return rc;
        tab ^= 1;
    }
    // big segments (few of them) get a workgroup per column, small ones a wavefront per column
    if ((n >> order) >= 2048) {
        hipLaunchKernelGGL(q_color_kernel<kQBlock>, dim3(S, (unsigned)(K < 1024 ? K : 1024)), dim3(kQBlock), 0, st, data, (int)K, weights, perm,
                           sp.seg_start[tab], sp.n_seg + tab, colors);
    } else {
        const int groups = (K + 3) / 4;
        hipLaunchKernelGGL(q_color_kernel<64>, dim3(S, (unsigned)(groups < 1024 ? groups : 1024)), dim3(kQBlock), 0, st, data, (int)K, weights,
                           perm, sp.seg_start[tab], sp.n_seg + tab, colors);
    }
    return check_launch(fn);
}

int svoxt_remap_index(const int32_t* data_in, int32_t* data_out, int64_t n, const int32_t* map, int64_t M, void* stream) {
    const char* fn = "svoxt_remap_index";
    if (n < 0 || n > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the number of words must be in [0, 2^31)", fn);
    if (M < 0 || M > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the map's length must be in [0, 2^31)", fn);
    if (n == 0) return SVOXT_OK;
    if (data_in == nullptr || data_out == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: data is NULL", fn);
    if (M > 0 && map == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: map is NULL", fn);
    hipLaunchKernelGGL(q_remap_kernel, dim3((unsigned)((n + kQBlock - 1) / kQBlock)), dim3(kQBlock), 0, (hipStream_t)stream, data_in, data_out, n,
                       map, (uint32_t)M);
    return check_launch(fn);
}

}  // extern "C"
