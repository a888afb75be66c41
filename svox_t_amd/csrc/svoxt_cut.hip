// svoxt_cut.hip -- new lists out of old ones by cutting crossings at breakpoints (not in the reference).
// The per-sample family's conventions (svoxt_samples.hip): ray q's segment is max(offsets[q], 0) .. min(offsets[q + 1], T),
// float32, every operation rounded by itself, no contraction, no float atomic, no LDS: the same bits in every run.
//
//   split    count -> scan -> emit (svoxt_listemit.h, the per-sample shape).  A lane per sample forms its number of pieces
//                m = 1                                    where length > 0 is false, or mf >= 1 is false
//                m = (int)min(mf, (float)max_pieces)      otherwise;  mf = ceilf(length / max_length) or (float)pieces[k]
//            and each wavefront adds its lanes' counts to one 64-bit total; pos = exclusive scan of m over T + 1 entries,
//            offsets'[q] = pos[clamped offsets[q]].  The emit takes a lane per OUTPUT piece j: a binary search in pos finds
//            its source k (pos[k] <= j < pos[k + 1]) -- once per wavefront over all of pos for its first piece, then per
//            lane over the 64 entries behind that --, p = j - pos[k]:
//                m == 1:  depth and length copied bit for bit
//                else:    step = length / (float)m;  depth' = depth + (float)p * step;  length' = step
//   merge    count -> scan -> emit (the per-ray shape), a lane per ray.  Both kernels compile the same walk (merge_walk below) over the ray's two
//            segments, once to count the pieces and once to write them at offsets'[q] ..; the count kernel adds each
//            wavefront's pieces to one 64-bit total.
// C ABI: svoxt_samples_split_* / svoxt_samples_merge_* (include/svoxt.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"
#include "svoxt_listemit.h"
#include "svoxt_wave.h"
#include "svoxt_workspace.h"

#pragma clang fp contract(off)

namespace svoxt {

// -------------------------------------------------------------------------------------------------------------- split
// workspace of svoxt_samples_split_count, read again by _emit: the per-sample ListSpace (svoxt_listemit.h) with a total,
// counts = m, starts = pos

// The entries k <= T, strided over at most kSplitCountBlocks workgroups; entry T is the scan's end and holds 0.  A lane adds
// its counts up and a wavefront sends one atomic: with a lane per sample and an atomic per 64 of them, the 92 000
// wavefronts of the headline lists queued on the one address for 0.87 ms.
constexpr int kSplitCountBlocks = 1024;
__global__ void __launch_bounds__(kLaunchBlock)
split_count_kernel(const float* __restrict__ length, const int32_t* __restrict__ pieces, float max_length, float max_pieces, int64_t T,
                   uint32_t* __restrict__ m_out, unsigned long long* __restrict__ total) {
    const int64_t stride = (int64_t)gridDim.x * kLaunchBlock;
    unsigned long long sum = 0ull;
    for (int64_t k = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x; k <= T; k += stride) {
        uint32_t m = 0u;
        if (k < T) {
            const float len = length[k];
            const float mf = pieces != nullptr ? (float)pieces[k] : ceilf(len / max_length);
            m = (len > 0.f && mf >= 1.f) ? (uint32_t)(int32_t)fminf(mf, max_pieces) : 1u;
        }
        m_out[k] = m;
        sum += m;
    }
    wave_add_to_total(sum, total);
}

// a lane per output piece
__global__ void __launch_bounds__(kLaunchBlock)
split_emit_kernel(const uint32_t* __restrict__ pos, int64_t T, int64_t T_out, const int32_t* __restrict__ ray,
                  const int32_t* __restrict__ row, const float* __restrict__ depth, const float* __restrict__ length,
                  int32_t* __restrict__ ray_out, int32_t* __restrict__ row_out, float* __restrict__ depth_out,
                  float* __restrict__ length_out, int64_t* __restrict__ index) {
    // The search in two stages.  A wavefront's 64 pieces are neighbours, and m >= 1, so their sources lie within 64
    // samples of the source of its first piece j0: that one is found once per wavefront with wavefront-uniform control
    // flow and addresses (readfirstlane says so to the compiler: the 20-odd dependent loads become scalar loads), and
    // each lane then searches the at most 64 entries behind it, which share a few cache lines.
    const int64_t n_out = min(T_out, (int64_t)pos[T]);           // (the caller's T' is the scan's)
    const int64_t j0 = (int64_t)blockIdx.x * kLaunchBlock + 64 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j0 >= n_out) return;
    int64_t k0 = 0, end0 = T;                                    // pos[k0] <= j0 < pos[end0]
    while (end0 - k0 > 1) {
        const int64_t mid = k0 + ((end0 - k0) >> 1);
        if ((int64_t)pos[mid] <= j0) k0 = mid;
        else end0 = mid;
    }
    const int64_t j = j0 + (threadIdx.x & 63);
    if (j >= n_out) return;
    int64_t lo = k0, hi = min(T, k0 + (j - j0) + 1);              // pos[lo] <= j < pos[hi]: pos[k0 + 1] > j0, and every m >= 1
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)pos[mid] <= j) lo = mid;
        else hi = mid;
    }
    const uint32_t first = pos[lo], m = pos[lo + 1] - first;
    float z = depth[lo], d = length[lo];
    if (m != 1u) {
        const float step = d / (float)m;
        z = z + (float)(uint32_t)(j - (int64_t)first) * step;
        d = step;
    }
    ray_out[j] = ray[lo];
    row_out[j] = row[lo];
    depth_out[j] = z;
    length_out[j] = d;
    index[j] = lo;
}

// -------------------------------------------------------------------------------------------------------------- merge
// workspace of svoxt_samples_merge_count: the per-ray ListSpace (svoxt_listemit.h) with a total

// One list of a ray under the walk: the current sample [s, e) with its length as stored, and the cursor c inside it.
struct CutList {
    const float* __restrict__ depth;
    const float* __restrict__ length;
    int64_t k, end;
    float s, e, len, c;
    __device__ __forceinline__ bool live() const { return k < end; }
    __device__ __forceinline__ void load() {
        if (k < end) {
            s = depth[k];
            len = length[k];
            e = s + len;
            c = s;
        }
    }
    __device__ __forceinline__ void next() { ++k; load(); }
    // what is left of the current sample, from the cursor to its end
    __device__ __forceinline__ float rest() const { return c == s ? len : e - c; }
};

struct CutLists {
    const int64_t *offsets_a, *offsets_b;
    const float *depth_a, *length_a, *depth_b, *length_b;
    int64_t T_a, T_b;
};

// The union of ray q's two lists, piece by piece: f(depth, length, index_a, index_b), an index -1 where that list does
// not cover the piece.  The definition is in include/svoxt.h, step by step; tests/cut_restate.py restates it.
template <class F>
__device__ __forceinline__ void merge_walk(const CutLists& L, int64_t q, F&& f) {
    CutList a{L.depth_a, L.length_a, max(L.offsets_a[q], (int64_t)0), min(L.offsets_a[q + 1], L.T_a), 0.f, 0.f, 0.f, 0.f};
    CutList b{L.depth_b, L.length_b, max(L.offsets_b[q], (int64_t)0), min(L.offsets_b[q + 1], L.T_b), 0.f, 0.f, 0.f, 0.f};
    a.load();
    b.load();
    while (a.live() || b.live()) {
        if (a.live() && !(a.e > a.s)) {                          // 1. a degenerate sample: whole and alone, A's first
            f(a.s, a.len, a.k, (int64_t)-1);
            a.next();
        } else if (b.live() && !(b.e > b.s)) {
            f(b.s, b.len, (int64_t)-1, b.k);
            b.next();
        } else if (a.live() && (!b.live() || a.e <= b.c)) {      // 2. A lies wholly in front
            f(a.c, a.rest(), a.k, (int64_t)-1);
            a.next();
        } else if (!a.live() || b.e <= a.c) {                    // 3. B lies wholly in front
            f(b.c, b.rest(), (int64_t)-1, b.k);
            b.next();
        } else if (a.c < b.c) {                                  // 4. A starts first
            f(a.c, b.c - a.c, a.k, (int64_t)-1);
            a.c = b.c;
        } else if (b.c < a.c) {                                  // 5. B starts first
            f(b.c, a.c - b.c, (int64_t)-1, b.k);
            b.c = a.c;
        } else {                                                 // 6. both cover from here
            const float hi = b.e < a.e ? b.e : a.e;
            const float d = (a.c == a.s && hi == a.e) ? a.len : ((b.c == b.s && hi == b.e) ? b.len : hi - a.c);
            f(a.c, d, a.k, b.k);
            const bool a_done = a.e <= hi, b_done = b.e <= hi;
            a.c = hi;
            b.c = hi;
            if (a_done) a.next();
            if (b_done) b.next();
        }
    }
}

__global__ void __launch_bounds__(kLaunchBlock)
merge_count_kernel(CutLists L, int64_t Q, uint32_t* __restrict__ counts, unsigned long long* __restrict__ total) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    unsigned long long n = 0ull;                                 // (at most 2 (n_a + n_b): below 2^33)
    if (q < Q) {
        merge_walk(L, q, [&](float, float, int64_t, int64_t) { ++n; });
        counts[q] = (uint32_t)n;
    }
    wave_add_to_total(n, total);
}

__global__ void __launch_bounds__(kLaunchBlock)
merge_emit_kernel(CutLists L, int64_t Q, const int64_t* __restrict__ offsets_out, int64_t T_out, int32_t* __restrict__ ray_out,
                  int32_t* __restrict__ row_out, float* __restrict__ depth_out, float* __restrict__ length_out,
                  int64_t* __restrict__ index_a, int64_t* __restrict__ index_b) {
    const int64_t q = (int64_t)blockIdx.x * kLaunchBlock + threadIdx.x;
    if (q >= Q) return;
    int64_t at = offsets_out[q];
    const int64_t end = min(offsets_out[q + 1], T_out);
    if (at < 0) return;
    merge_walk(L, q, [&](float z, float d, int64_t ia, int64_t ib) {
        if (at < end) {                                          // (the count's walk found as many: never past the ray's own segment)
            ray_out[at] = (int32_t)q;
            row_out[at] = -1;
            depth_out[at] = z;
            length_out[at] = d;
            index_a[at] = ia;
            index_b[at] = ib;
            ++at;
        }
    });
}

// ------------------------------------------------------------------------------------------------------------- checks
// one side of a merge: its arrays may be NULL only where it has no sample
static int merge_side_check(const int64_t* offsets, const float* depth, const float* length, int64_t T, const char* fn) {
    if (offsets == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets_a / offsets_b is NULL", fn);
    if (T > 0 && (depth == nullptr || length == nullptr)) return fail(SVOXT_ERR_INVALID, "%s: depth / length of a list with samples is NULL", fn);
    if (misaligned(offsets, 8) || misaligned(depth, 4) || misaligned(length, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets, index: 8 bytes, the other arrays: 4)", fn);
    return SVOXT_OK;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_samples_split_workspace_bytes(int64_t T) {
    return list_space_bytes(T, 1, true);
}

int svoxt_samples_split_count(const float* length, const int32_t* pieces, float max_length, int32_t max_pieces, const int64_t* offsets,
                              int64_t Q, int64_t T, int64_t* offsets_out, int64_t* total, void* workspace, int64_t workspace_bytes,
                              void* stream) {
    const char* fn = "svoxt_samples_split_count";
    int rc;
    if ((rc = extent31_check(fn, Q, "Q")) || (rc = extent31_check(fn, T, "T"))) return rc;
    if (max_pieces < 1 || max_pieces > (1 << 30)) return fail(SVOXT_ERR_INVALID, "%s: max_pieces must be in [1, 2^30]", fn);
    if ((rc = counts_out_check(fn, offsets_out, total))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) return clear_counts(fn, offsets_out, Q, total, st);          // nothing to cut: empty lists, nothing else is read
    if (pieces == nullptr && max_length == 0.f) return fail(SVOXT_ERR_INVALID, "%s: neither max_length nor pieces is given", fn);
    if (pieces != nullptr && max_length != 0.f) return fail(SVOXT_ERR_INVALID, "%s: both max_length and pieces are given (max_length must be 0 with pieces)", fn);
    if (pieces == nullptr && !(max_length > 0.f)) return fail(SVOXT_ERR_INVALID, "%s: max_length must be > 0", fn);
    if (length == nullptr || offsets == nullptr) return fail(SVOXT_ERR_INVALID, "%s: length / offsets is NULL", fn);
    if (misaligned(offsets, 8)) return fail(SVOXT_ERR_INVALID, "%s: offsets is not 8-byte aligned", fn);
    if (misaligned(length, 4) || misaligned(pieces, 4)) return fail(SVOXT_ERR_INVALID, "%s: length / pieces is not 4-byte aligned", fn);
    if (overlap(offsets, offsets_out, 8.0 * (double)(Q + 1))) return fail(SVOXT_ERR_INVALID, "%s: offsets_out overlaps offsets", fn);
    ListSpace sp;
    if ((rc = list_space_check(fn, workspace, workspace_bytes, (size_t)T + 1, true, "svoxt_samples_split_workspace_bytes(T)", &sp)) ||
        (rc = memset_async(workspace, sp.clear_bytes, st, fn)))
        return rc;
    hipLaunchKernelGGL(split_count_kernel, dim3(min(launch_blocks(T + 1), (unsigned)kSplitCountBlocks)), dim3(kLaunchBlock), 0, st, length, pieces, max_length,
                       (float)max_pieces, T, sp.counts, sp.total);
    return list_pos_offsets<true>(fn, sp, offsets, Q, T, offsets_out, total, st);
}

int svoxt_samples_split_emit(int64_t T, const void* workspace, int64_t workspace_bytes, const int32_t* ray, const int32_t* row,
                             const float* depth, const float* length, int64_t T_out, int32_t* ray_out, int32_t* row_out,
                             float* depth_out, float* length_out, int64_t* index, void* stream) {
    const char* fn = "svoxt_samples_split_emit";
    int rc;
    if ((rc = extent31_check(fn, T, "T"))) return rc;
    if (!in31(T_out) || (T_out > 0 && T == 0)) return fail(SVOXT_ERR_INVALID, "%s: T_out must be in [0, 2^31), 0 for T = 0", fn);
    if (T_out == 0) return SVOXT_OK;
    ListSpace sp;
    if ((rc = emit_arrays_check(fn, ray, row, depth, length, ray_out, row_out, depth_out, length_out, index)) ||
        (rc = list_space_check(fn, workspace, workspace_bytes, (size_t)T + 1, true, "svoxt_samples_split_workspace_bytes(T)", &sp)))
        return rc;
    hipLaunchKernelGGL(split_emit_kernel, dim3(launch_blocks(T_out)), dim3(kLaunchBlock), 0, (hipStream_t)stream, sp.starts, T, T_out, ray,
                       row, depth, length, ray_out, row_out, depth_out, length_out, index);
    return check_launch(fn);
}

int64_t svoxt_samples_merge_workspace_bytes(int64_t Q) {
    return list_space_bytes(Q, 0, true);
}

int svoxt_samples_merge_count(const int64_t* offsets_a, const float* depth_a, const float* length_a, int64_t T_a, const int64_t* offsets_b,
                              const float* depth_b, const float* length_b, int64_t T_b, int64_t Q, int64_t* offsets_out, int64_t* total,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_samples_merge_count";
    int rc;
    if ((rc = extent31_check(fn, Q, "Q")) || (rc = extent31_check(fn, T_a, "T_a")) || (rc = extent31_check(fn, T_b, "T_b")) ||
        (rc = counts_out_check(fn, offsets_out, total)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (Q == 0 || (T_a == 0 && T_b == 0)) return clear_counts(fn, offsets_out, Q, total, st);        // nothing to merge: empty lists
    if ((rc = merge_side_check(offsets_a, depth_a, length_a, T_a, fn)) || (rc = merge_side_check(offsets_b, depth_b, length_b, T_b, fn))) return rc;
    if (overlap(offsets_a, offsets_out, 8.0 * (double)(Q + 1)) || overlap(offsets_b, offsets_out, 8.0 * (double)(Q + 1)))
        return fail(SVOXT_ERR_INVALID, "%s: offsets_out overlaps offsets_a / offsets_b", fn);
    ListSpace sp;
    if ((rc = list_space_check(fn, workspace, workspace_bytes, (size_t)Q, true, "svoxt_samples_merge_workspace_bytes(Q)", &sp)) ||
        (rc = memset_async(workspace, sp.clear_bytes, st, fn)))
        return rc;
    const CutLists L{offsets_a, offsets_b, depth_a, length_a, depth_b, length_b, T_a, T_b};
    hipLaunchKernelGGL(merge_count_kernel, dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, st, L, Q, sp.counts, sp.total);
    return list_ray_offsets<true>(fn, sp, Q, offsets_out, total, st);
}

int svoxt_samples_merge_emit(const int64_t* offsets_a, const float* depth_a, const float* length_a, int64_t T_a, const int64_t* offsets_b,
                             const float* depth_b, const float* length_b, int64_t T_b, int64_t Q, const int64_t* offsets_out, int64_t T_out,
                             int32_t* ray_out, int32_t* row_out, float* depth_out, float* length_out, int64_t* index_a, int64_t* index_b,
                             void* stream) {
    const char* fn = "svoxt_samples_merge_emit";
    int rc;
    if ((rc = extent31_check(fn, Q, "Q")) || (rc = extent31_check(fn, T_a, "T_a")) || (rc = extent31_check(fn, T_b, "T_b")) ||
        (rc = extent31_check(fn, T_out, "T_out")))
        return rc;
    if (T_out == 0 || Q == 0) return SVOXT_OK;
    if ((rc = merge_side_check(offsets_a, depth_a, length_a, T_a, fn)) || (rc = merge_side_check(offsets_b, depth_b, length_b, T_b, fn))) return rc;
    if (offsets_out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: offsets_out is NULL", fn);
    if (ray_out == nullptr || row_out == nullptr || depth_out == nullptr || length_out == nullptr || index_a == nullptr || index_b == nullptr)
        return fail(SVOXT_ERR_INVALID, "%s: an output is NULL", fn);
    if (misaligned(offsets_out, 8) || misaligned(index_a, 8) || misaligned(index_b, 8) || misaligned(ray_out, 4) || misaligned(row_out, 4) ||
        misaligned(depth_out, 4) || misaligned(length_out, 4))
        return fail(SVOXT_ERR_INVALID, "%s: a misaligned argument (offsets, index: 8 bytes, the other arrays: 4)", fn);
    const CutLists L{offsets_a, offsets_b, depth_a, length_a, depth_b, length_b, T_a, T_b};
    hipLaunchKernelGGL(merge_emit_kernel, dim3(launch_blocks(Q)), dim3(kLaunchBlock), 0, (hipStream_t)stream, L, Q, offsets_out, T_out,
                       ray_out, row_out, depth_out, length_out, index_a, index_b);
    return check_launch(fn);
}

}  // extern "C"
