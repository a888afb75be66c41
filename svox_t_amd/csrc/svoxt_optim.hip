// svoxt_optim.hip -- the update of a feature table: SGD (with or without momentum), RMSprop and Adam as ONE streaming
// kernel over the rows of the table, which can skip the rows a backward did not touch.
// C ABI: svoxt_optim_step / svoxt_optim_state_count (include/svoxt.h has the arithmetic, operation by operation).
//
// The reference has no optimizer: its users hand the dense [M, K] table to torch.optim, which reads and writes every
// element of the parameter and of every state table although one view's backward touches only the rows its rays cross.
//
// rows       a row of E elements (V: 4 columns where K % 4 == 0 and every table is 16-byte aligned, else 1) belongs to a
//            group of G consecutive lanes, G the power of two >= E, at most 64: K = 28 is 7 x 16 bytes on 8 lanes, 8 rows
//            a wavefront.  A row wider than 64 elements is walked by its 64 lanes in steps of 64.
// touched    a row is touched iff some element of its gradient compares != 0 (+-0 no, NaN yes).  Every lane ORs its
//            elements, one ballot gives the wavefront's lanes, a group reads its own bits of it.
// lazy       an untouched row ends there: p and the state tables are neither read nor written, the gradient was read
//            once.  Dense (lazy == 0) updates every row: the moments decay where g == 0, as torch.optim's do.
// arithmetic float32, every operation a separate correctly rounded + - * / sqrt (-ffp-contract=off; sqrtf and / are the
//            correctly rounded forms, svoxt_device.h), in the order of the header: a numpy restatement gives the same bits.
//            An element depends on nothing but its own p, g, m, v: the result is a function of the inputs.
// One launch on the caller's stream; no workspace, no allocation, no host read.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_host.h"

namespace svoxt {

constexpr int kOptimBlock = 256;
enum { OPT_SGD = SVOXT_OPTIM_SGD, OPT_MOMENTUM = SVOXT_OPTIM_SGD_MOMENTUM, OPT_RMSPROP = SVOXT_OPTIM_RMSPROP,
       OPT_ADAM = SVOXT_OPTIM_ADAM };

typedef float float4o __attribute__((ext_vector_type(4)));

template <typename V> struct OptimWidth;
template <> struct OptimWidth<float> { static constexpr int n = 1; };
template <> struct OptimWidth<float4o> { static constexpr int n = 4; };

__device__ __forceinline__ float optim_get(const float4o& v, int e) { return v[e]; }
__device__ __forceinline__ float optim_get(const float& v, int) { return v; }
__device__ __forceinline__ void optim_put(float4o& v, int e, float x) { v[e] = x; }
__device__ __forceinline__ void optim_put(float& v, int, float x) { v = x; }

// One element.  p: the parameter, g: its gradient, a / b: the first / second state table's element.
template <int KIND>
__device__ __forceinline__ void optim_element(float& p, float g, float& a, float& b, const svoxt_optim_hyper& h) {
    if constexpr (KIND == OPT_SGD) {
        p = p + h.neg_step * g;
    } else if constexpr (KIND == OPT_MOMENTUM) {
        a = h.momentum * a + g;
        p = p + h.neg_step * a;
    } else if constexpr (KIND == OPT_RMSPROP) {
        a = h.beta2 * a + h.one_minus_beta2 * (g * g);
        p = p + h.neg_step * (g / (sqrtf(a) + h.eps));
    } else {
        a = a + (g - a) * h.one_minus_beta1;
        b = h.beta2 * b + h.one_minus_beta2 * (g * g);
        const float d = sqrtf(b) / h.bias2_sqrt + h.eps;
        p = p + h.neg_step * (a / d);
    }
}

// lane t: row t >> log2G, element (t & (G - 1)) + 64 i of it.  E: elements of V a row.
template <int KIND, typename V>
__global__ void __launch_bounds__(kOptimBlock)
optim_step_kernel(V* __restrict__ param, const V* __restrict__ grad, V* __restrict__ state1, V* __restrict__ state2, int64_t M, int E,
                  int log2G, svoxt_optim_hyper h, int lazy) {
    constexpr int W = OptimWidth<V>::n;
    constexpr int NS = KIND == OPT_SGD ? 0 : KIND == OPT_ADAM ? 2 : 1;
    const int64_t t = (int64_t)blockIdx.x * kOptimBlock + threadIdx.x;
    const int G = 1 << log2G;
    const int64_t row = t >> log2G;
    const int j = (int)(t & (G - 1));
    const bool in_table = row < M;
    const int64_t base = row * E;
    const bool single = E <= G;                    // the row fits its group: the gradient stays in a register
    V g0 = V(0.f);
    if (lazy != 0) {
        bool nz = false;
        if (in_table) {
            if (single) {
                if (j < E) g0 = grad[base + j];
#pragma unroll
                for (int e = 0; e < W; ++e) nz |= optim_get(g0, e) != 0.f;
            } else {
                for (int i = j; i < E; i += G) {
                    const V x = grad[base + i];
#pragma unroll
                    for (int e = 0; e < W; ++e) nz |= optim_get(x, e) != 0.f;
                }
            }
        }
        const uint64_t any = __ballot(nz);         // (lanes that left or hold no element vote 0)
        const int lane = threadIdx.x & 63;
        const uint64_t mine = (G == 64 ? ~(uint64_t)0 : (((uint64_t)1 << G) - 1)) << (lane & ~(G - 1));
        if ((any & mine) == 0) return;             // untouched: p and the state keep their bits, unread
    } else if (in_table && single && j < E) {
        g0 = grad[base + j];
    }
    if (!in_table) return;
    for (int i = j; i < E; i += G) {
        const int64_t at = base + i;
        const V g = single ? g0 : grad[at];
        V p = param[at];
        V a = V(0.f), b = V(0.f);
        if constexpr (NS >= 1) a = state1[at];
        if constexpr (NS >= 2) b = state2[at];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            float pe = optim_get(p, e), ae = optim_get(a, e), be = optim_get(b, e);
            optim_element<KIND>(pe, optim_get(g, e), ae, be, h);
            optim_put(p, e, pe); optim_put(a, e, ae); optim_put(b, e, be);
        }
        param[at] = p;
        if constexpr (NS >= 1) state1[at] = a;
        if constexpr (NS >= 2) state2[at] = b;
    }
}

// lanes a row: the power of two >= E, at most 64
static int optim_log2_group(int E) {
    int log2G = 0;
    while (log2G < 6 && (1 << log2G) < E) ++log2G;
    return log2G;
}

template <int KIND, typename V>
static void optim_launch(float* param, const float* grad, float* state1, float* state2, int64_t M, int E, const svoxt_optim_hyper& h,
                         int lazy, hipStream_t st) {
    const int log2G = optim_log2_group(E);
    const int64_t lanes = M << log2G;
    hipLaunchKernelGGL((optim_step_kernel<KIND, V>), dim3((unsigned)((lanes + kOptimBlock - 1) / kOptimBlock)), dim3(kOptimBlock), 0, st,
                       reinterpret_cast<V*>(param), reinterpret_cast<const V*>(grad), reinterpret_cast<V*>(state1),
                       reinterpret_cast<V*>(state2), M, E, log2G, h, lazy);
}

// The damped Newton step on a diagonal curvature (svoxt_gauss_newton_step): lane t is element t & (G - 1) + 64 i of row
// t >> log2G, the touched test and the lazy exit as in optim_step_kernel.  d = h + damping; where d > 0.f
// p = p - lr * (g / d), else the element is not written.
__global__ void __launch_bounds__(kOptimBlock)
gauss_newton_step_kernel(float* __restrict__ param, const float* __restrict__ grad, const float* __restrict__ hess, int64_t M, int K,
                         int log2G, float lr, float damping, int lazy) {
    const int64_t t = (int64_t)blockIdx.x * kOptimBlock + threadIdx.x;
    const int G = 1 << log2G;
    const int64_t row = t >> log2G;
    const int j = (int)(t & (G - 1));
    const bool in_table = row < M;
    const int64_t base = row * K;
    if (lazy != 0) {
        bool nz = false;
        if (in_table)
            for (int i = j; i < K; i += G) nz |= grad[base + i] != 0.f;
        const uint64_t any = __ballot(nz);         // (lanes that left or hold no element vote 0)
        const int lane = threadIdx.x & 63;
        const uint64_t mine = (G == 64 ? ~(uint64_t)0 : (((uint64_t)1 << G) - 1)) << (lane & ~(G - 1));
        if ((any & mine) == 0) return;             // untouched: p keeps its bits, hess is not read
    }
    if (!in_table) return;
    for (int i = j; i < K; i += G) {
        const int64_t at = base + i;
        const float d = hess[at] + damping;
        if (d > 0.f) param[at] = param[at] - lr * (grad[at] / d);
    }
}

static int optim_states(int32_t kind) {
    switch (kind) {
        case OPT_SGD: return 0;
        case OPT_MOMENTUM: case OPT_RMSPROP: return 1;
        case OPT_ADAM: return 2;
        default: return -1;
    }
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int svoxt_optim_state_count(int32_t kind) { return optim_states(kind); }

int svoxt_optim_step(int32_t kind, float* param, const float* grad, float* state1, float* state2, int64_t M, int32_t K,
                     svoxt_optim_hyper hyper, int32_t lazy, void* stream) {
    const char* fn = "svoxt_optim_step";
    const int ns = optim_states(kind);
    if (ns < 0) return set_error(SVOXT_ERR_INVALID, "%s: kind must be one of SVOXT_OPTIM_SGD / SGD_MOMENTUM / RMSPROP / ADAM", fn);
    if (M < 1 || K < 1) return set_error(SVOXT_ERR_INVALID, "%s: M and K must be >= 1", fn);
    if ((double)M * (double)K >= 137438953472.0) return set_error(SVOXT_ERR_INVALID, "%s: M * K must be below 2^37", fn);
    if (param == nullptr || grad == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: param / grad is NULL", fn);
    if (ns >= 1 && state1 == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: state1 is NULL (this kind keeps a state table)", fn);
    if (ns >= 2 && state2 == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: state2 is NULL (this kind keeps two state tables)", fn);
    if (lazy != 0 && lazy != 1) return set_error(SVOXT_ERR_INVALID, "%s: lazy must be 0 or 1", fn);
    const void* tabs[4] = {param, grad, ns >= 1 ? state1 : nullptr, ns >= 2 ? state2 : nullptr};
    bool vec = K % 4 == 0;
    for (int i = 0; i < 4; ++i) {
        if (tabs[i] == nullptr) continue;
        if ((uintptr_t)tabs[i] % 4 != 0) return set_error(SVOXT_ERR_INVALID, "%s: a table is not 4-byte aligned", fn);
        vec = vec && (uintptr_t)tabs[i] % 16 == 0;
        for (int k = 0; k < i; ++k)
            if (tabs[k] == tabs[i]) return set_error(SVOXT_ERR_INVALID, "%s: param, grad and the state tables must be distinct", fn);
    }
    // one lane per (row, slot of its group): a launch holds fewer than 2^32 of them
    if ((double)M * (double)(1 << optim_log2_group(vec ? K / 4 : K)) >= 4294967296.0 - kOptimBlock)
        return set_error(SVOXT_ERR_INVALID, "%s: M * (lanes a row) must be below 2^32 - 256; lanes a row = the power of two >= K / 4 "
                         "(K where K % 4 != 0 or a table is not 16-byte aligned), at most 64", fn);
    hipStream_t st = (hipStream_t)stream;
    const int k = (int)kind;
    const bool known = with_int(IntSet<OPT_SGD, OPT_MOMENTUM, OPT_RMSPROP, OPT_ADAM>{}, k, [&](auto kc) {
        constexpr int KIND = decltype(kc)::value;
        if (vec) optim_launch<KIND, float4o>(param, grad, state1, state2, M, K / 4, hyper, lazy, st);
        else optim_launch<KIND, float>(param, grad, state1, state2, M, K, hyper, lazy, st);
        return true;
    });
    if (!known) return set_error(SVOXT_ERR_INVALID, "%s: kind has no kernel", fn);
    return check_launch(fn);
}

int svoxt_gauss_newton_step(float* param, const float* grad, const float* hess, int64_t M, int32_t K, float lr, float damping,
                            int32_t lazy, void* stream) {
    const char* fn = "svoxt_gauss_newton_step";
    if (M < 1 || K < 1) return set_error(SVOXT_ERR_INVALID, "%s: M and K must be >= 1", fn);
    if ((double)M * (double)K >= 137438953472.0) return set_error(SVOXT_ERR_INVALID, "%s: M * K must be below 2^37", fn);
    if (param == nullptr || grad == nullptr || hess == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: param / grad / hess is NULL", fn);
    if (lazy != 0 && lazy != 1) return set_error(SVOXT_ERR_INVALID, "%s: lazy must be 0 or 1", fn);
    if ((uintptr_t)param % 4 != 0 || (uintptr_t)grad % 4 != 0 || (uintptr_t)hess % 4 != 0)
        return set_error(SVOXT_ERR_INVALID, "%s: a table is not 4-byte aligned", fn);
    if (param == grad || param == hess) return set_error(SVOXT_ERR_INVALID, "%s: param must be distinct from grad and hess", fn);
    const int log2G = optim_log2_group(K);
    if ((double)M * (double)(1 << log2G) >= 4294967296.0 - kOptimBlock)
        return set_error(SVOXT_ERR_INVALID, "%s: M * (lanes a row) must be below 2^32 - 256; lanes a row = the power of two >= K, at most 64", fn);
    const int64_t lanes = M << log2G;
    hipLaunchKernelGGL(gauss_newton_step_kernel, dim3((unsigned)((lanes + kOptimBlock - 1) / kOptimBlock)), dim3(kOptimBlock), 0,
                       (hipStream_t)stream, param, grad, hess, M, (int)K, log2G, lr, damping, (int)lazy);
    return check_launch(fn);
}

}  // extern "C"
