// Stand-in for <cuda_runtime.h>: lets g++ compile the *device* code of the
// reference's .cu files as plain C++ for one host thread (oracle/ref.py,
// oracle/ref_driver.cpp).  TEST INFRASTRUCTURE ONLY.  Only what that device
// code (and the two headers it includes whole) names is defined here; each
// block says where its semantics come from.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include <ATen/core/TensorAccessor.h>

// ---- function and variable qualifiers (CUDA C++ Programming Guide, "Function
// execution space specifiers", "Variable memory space specifiers"): no meaning
// on a host-only build.  __restrict__ and __inline__ are GNU keywords already.
#define __device__
#define __host__
#define __global__
#define __constant__

// ---- built-in index variables (Programming Guide, "Built-in variables"): uint3
// / dim3 with members x, y, z.  The driver runs one thread at a time and sets
// them before each call: blockDim.x = 1, threadIdx.x = 0, blockIdx.x = thread id.
struct svoxt_ref_uint3 { unsigned int x, y, z; };
static svoxt_ref_uint3 blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, threadIdx = {0, 0, 0};

// ---- torch::RestrictPtrTraits: torch's own definition
// (torch/headeronly/core/TensorAccessor.h), which its headers compile only under
// a CUDA or HIP compiler.  namespace torch sees namespace at.
namespace at {
template <typename T>
struct RestrictPtrTraits {
    typedef T* __restrict__ PtrType;
};
}  // namespace at

// ---- min / max (CUDA Math API, and the overload set of
// crt/math_functions.hpp): min(float, float) is fminf, min(double, double) is
// fmin -- a NaN operand loses -- and the mixed overloads min(float, double) /
// min(double, float) convert the float and return double.  So
// `min(scalar_t(1.0) - 1e-6, q[i])` compares in double and rounds on the store.
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }
inline double min(float a, double b) { return fmin((double)a, b); }
inline double min(double a, float b) { return fmin(a, (double)b); }
inline double max(float a, double b) { return fmax((double)a, b); }
inline double max(double a, float b) { return fmax(a, (double)b); }

// ---- bit reinterpretation (CUDA Math API, "Type casting intrinsics")
inline int __float_as_int(float x) { int r; std::memcpy(&r, &x, sizeof r); return r; }
inline float __int_as_float(int x) { float r; std::memcpy(&r, &x, sizeof r); return r; }
inline long long __double_as_longlong(double x) { long long r; std::memcpy(&r, &x, sizeof r); return r; }
inline double __longlong_as_double(long long x) { double r; std::memcpy(&r, &x, sizeof r); return r; }

// ---- atomics (Programming Guide, "Atomic functions"): read old, store
// old + val (or the compared value), return old.  One thread runs at a time, so
// the read-modify-write is a plain one; float atomicAdd rounds once, as the
// hardware's does.
inline float atomicAdd(float* address, float val) { const float old = *address; *address = old + val; return old; }
inline double atomicAdd(double* address, double val) { const double old = *address; *address = old + val; return old; }
inline unsigned int atomicCAS(unsigned int* address, unsigned int compare, unsigned int val) {
    const unsigned int old = *address;
    if (old == compare) *address = val;
    return old;
}
inline unsigned long long atomicCAS(unsigned long long* address, unsigned long long compare, unsigned long long val) {
    const unsigned long long old = *address;
    if (old == compare) *address = val;
    return old;
}

// ---- the two runtime names that the reference's common header uses in a host
// helper it defines (a core count per device generation): needed to parse that
// header, never called.
struct cudaDeviceProp { int multiProcessorCount, major, minor; };
typedef int cudaError_t;
inline cudaError_t cudaGetDeviceProperties(cudaDeviceProp* p, int) { p->multiProcessorCount = p->major = p->minor = 0; return 0; }
