// svoxt_host.h -- host-side helpers shared by the translation units of
// libsvoxt_hip.so (not part of the public C ABI): compile-time dispatch, the error text, the checks of the C structs,
// the argument predicates of the per-sample units, the exclusive scan.
#pragma once

#include <type_traits>

#include "../../include/svoxt.h"
#include "svoxt_device.h"

namespace svoxt {

// A set of compile-time ints: the payload sizes below, and the instances a launch dispatches over.
template <int... Vs>
struct IntSet {
    static constexpr bool has(int v) { return ((v == Vs) || ...); }
};

// Compile-time dispatch of the launches.  with_int(IntSet<Vs...>{}, v, f) calls f(std::integral_constant<int, V>{}) for
// the V among Vs equal to v and returns its result, or false where none is: the instances are exactly f's for Vs.
// with_bool(b, f) calls f(std::true_type{}) or f(std::false_type{}) and returns its result.
template <int... Vs, class F>
bool with_int(IntSet<Vs...>, int v, F&& f) {
    bool r = false;
    (void)((v == Vs && (r = f(std::integral_constant<int, Vs>{}), true)) || ...);
    return r;
}
template <class F>
auto with_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}
template <int V>
using Int = std::integral_constant<int, V>;     // a compile-time int argument of a dispatch lambda, e.g. Int<FMT_SH>{}

// The payload sizes with specialised kernels: SH bases of degree 0 .. 4 (and as many SG / ASG lobes), RGBA-style rows of
// 8 / 16 / 32 floats (channels on lanes, the exponentials table), and the SH bases whose view-rotation forms run as one
// launch (fwd_roles_kernel<..., XF>, grad_fused_kernel<..., XF>).
using SpecialBases = IntSet<1, 4, 9, 16, 25>;
using ChanRows = IntSet<8, 16, 32>;
using XfRolesBases = IntSet<1, 4, 9>;
inline bool special_basis(int basis_dim) { return SpecialBases::has(basis_dim); }
inline bool chan_rows(int K) { return ChanRows::has(K); }
inline bool xf_roles_basis(int basis_dim) { return XfRolesBases::has(basis_dim); }

// Records the text svoxt_last_error() returns on this thread and hands back `code`.
int set_error(int code, const char* fmt, const char* a = "", const char* b = "");

inline int fail(int code, const char* fmt, const char* a = "", const char* b = "") { return set_error(code, fmt, a, b); }

// hipGetLastError() -> SVOXT_OK / SVOXT_ERR_HIP (+ error text)
int check_launch(const char* what);

// The argument predicates of the per-sample units, each once.  A NULL pointer is aligned and overlaps
// nothing: whether it may be NULL is the entry point's own check.
inline unsigned nblocks(int64_t Q) { return (unsigned)((Q + kBlock - 1) / kBlock); }
inline bool misaligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1u)) != 0; }
inline bool overlap(const void* a, const void* b, double bytes) {
    if (a == nullptr || b == nullptr) return false;
    const double x = (double)(uintptr_t)a, y = (double)(uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}
// an extent that int32 indices reach: a number of rays, samples, rows or chunks
inline bool in31(int64_t v) { return v >= 0 && v <= 0x7fffffffLL; }
inline int extent31_check(const char* fn, int64_t v, const char* name) {
    return in31(v) ? SVOXT_OK : fail(SVOXT_ERR_INVALID, "%s: %s must be in [0, 2^31)", fn, name);
}
// the elements of an [a, b] array that a launch of a lane per element covers: below 2^38
constexpr double kMaxElems = 274877906944.0;
inline bool elems_fit(double a, double b) { return a * b < kMaxElems; }
// zeros into `bytes` bytes at p on `st`
inline int memset_async(void* p, size_t bytes, hipStream_t st, const char* fn) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    return SVOXT_OK;
}

// Argument validation shared by every entry point (the TORCH_CHECKs of
// data_spec.hpp:57-64, 85-110 for raw pointers); `fn` names the caller in the error text.
int check_tree(const svoxt_tree* t, const char* fn);
// ... and of the entry points whose kernels read tree.features (and tree.exp_table) as 16-byte vectors when K % 4 == 0
// (load_row, the channel-row kernels, exp_table_kernel: the colour render forward and backwards, svoxt_step_*,
// svoxt_exp_table_build): such a table must start on a 16-byte boundary.  Called next to check_tree, before any launch.
int check_features_vec(const svoxt_tree* t, const char* fn);
int check_rays(const svoxt_rays* r, const char* fn);
int check_opts(const svoxt_options* o, const svoxt_tree* t, const char* fn, bool needs_basis);

// C structs -> what the kernels take by value
TreeDev to_dev(const svoxt_tree* t);
// t (may be NULL) decides the walk order of an image's tiles -- unless the lists (may be NULL) name the walk they were recorded with
RaysDev to_dev(const svoxt_rays* r, const svoxt_tree* t, const svoxt_sample_lists* l = nullptr);
Opts to_dev(const svoxt_options* o);

// Exclusive scan of n uint32 counters into starts (not in place), two launches on `st` (svoxt_order.hip);
// chunk_sums holds exclusive_scan_chunks(n) words.  Returns SVOXT_OK / SVOXT_ERR_HIP.
size_t exclusive_scan_chunks(size_t n);
int exclusive_scan(const uint32_t* counts, size_t n, uint32_t* chunk_sums, uint32_t* starts, hipStream_t st, const char* fn);

}  // namespace svoxt
