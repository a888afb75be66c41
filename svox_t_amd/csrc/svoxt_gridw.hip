// svoxt_gridw.hip -- grid_weights: march many views (or a ray batch) through a dense [R, R, R] density volume and keep,
// per cell, the largest compositing weight any ray gave it and the number of samples that landed in it (the
// reference's grid_weight_render, svox_t/csrc/rt_kernel.cu:1240-1344, host :1454-1478).
//
// One ray (grid_trace_ray): the preamble of svoxt_device.h (setup_ray: camera ray, NDC warp, world -> unit cube,
// direction normalised, invdir in double, slab test), then a loop of its own -- not the shared walk of svoxt_device.h,
// whose crossing is a tree leaf found by march_step; here it is a cell of the volume: while t < tmax: pos = origin + t dir, clamped to
// [0, 1 - 1e-6], times R, split into cell (u, v, w) and the cell-local point; delta_t = the cell's chord / R +
// step_size (leaf_delta_t: _dda_unit on the local point, whose entry distance is 0); sigma = volume[cell]; if sigma >
// sigma_thresh: att = pexpf(-delta_t delta_scale sigma), w = T (1 - att), T *= att, weight[cell] = max(.., w),
// hits[cell] += 1; t = march_advance(t, delta_t).  No early stop: a sample taken with T == 0 still counts as a hit.
// This unit is built with -ffp-contract=off like the others: the stepping arithmetic is the reference's operation
// sequence and decides which cells a ray visits.
//
// What differs from the reference is outside the per-ray semantics:
//   - the result does not depend on the order rays arrive in.  The maximum is a signed-integer max on the weight's bit
//     pattern (monotone for floats >= 0; a negative weight, possible only with a negative sigma_thresh, is a negative
//     integer and never raises a cell above what it holds); the count is an integer add, made in place in the hits
//     buffer and converted to float once by a finishing kernel (the reference adds 1.0f with a float atomic: the same
//     number up to 2^24 a cell).  Both are native agent-scope atomics (global_atomic_smax / global_atomic_add, no
//     compare-and-swap loop), so the outputs are bit-identical from run to run and to a CPU restatement;
//   - many cameras per launch: workgroup b marches 8 x 8 pixel tile (b % tiles) of view (b / tiles), a wavefront a tile
//     (pixels past the image's edge idle), so that its 64 rays cross neighbouring cells;
//   - every lane sends its own atomics.  Merging the lanes of a wavefront that sample the same cell in the same step
//     (one max and one add of the lane count per distinct cell) was built and measured: it loses on three of the
//     four timed cases (NOTEBOOK.md) and was removed;
//   - the max is skipped where the weight does not exceed what a plain load of the cell (issued with the sigma load)
//     already shows: cell values only grow, so a stale value can only fail to skip.
//   - accumulate: the outputs are updated, not zeroed, so a view set can be streamed through several calls.

#include <math.h>
#include <hip/hip_runtime.h>

#include "svoxt_host.h"

#pragma clang fp contract(off)

namespace svoxt {

constexpr int kGwConvBlock = 256;
constexpr unsigned kGwConvBlocksMax = 1u << 16;

struct GridW {
    int R;                      // cells per axis; R^3 < 2^31
    float Rf;
    uint32_t tiles_x;           // camera mode: 8 x 8 tiles per image row, ...
    uint32_t tiles_per_view;    // ... per view (0: ray-batch mode, workgroup b = rays 64 b .. 64 b + 63)
    int c2w_stride;             // floats from one camera matrix to the next (12 or 16)
};

__global__ void __launch_bounds__(64)
grid_weights_kernel(const float* __restrict__ sigma, GridW g, TreeDev tr, RaysDev rays, Opts opt, int32_t* weight_bits,
                    uint32_t* hits) {
    const int lane = (int)threadIdx.x;
    int64_t q;
    bool live;
    if (g.tiles_per_view != 0) {
        const uint32_t view = blockIdx.x / g.tiles_per_view, tile = blockIdx.x - view * g.tiles_per_view;
        const uint32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
        const int px = (int)(tx * 8) + (lane & 7), py = (int)(ty * 8) + (lane >> 3);
        live = px < rays.width && py < rays.height;
        q = (int64_t)py * rays.width + px;
        rays.c2w += (size_t)view * g.c2w_stride;
    } else {
        q = (int64_t)blockIdx.x * 64 + lane;
        live = q < rays.Q;
    }
    Ray r;
    const bool go = live && setup_ray(tr, rays, opt, q, r);
    const int R = g.R, top = R - 1;
    if (!go) return;
    float T = 1.f, t = r.tmin;
    while (t < r.tmax) {
        float px = r.ox + t * r.dx, py = r.oy + t * r.dy, pz = r.oz + t * r.dz;
        px = fmaxf(0.f, fminf(kClampHi, px));                // clamp_coord (common.cuh:36-42)
        py = fmaxf(0.f, fminf(kClampHi, py));
        pz = fmaxf(0.f, fminf(kClampHi, pz));
        px *= g.Rf; py *= g.Rf; pz *= g.Rf;
        const float fu = floorf(px), fv = floorf(py), fw = floorf(pz);
        px -= fu; py -= fv; pz -= fw;
        // (the clamped point times R stays below R; the min / max only keep a broken input inside the volume)
        const int u = min(max((int)fu, 0), top), v = min(max((int)fv, 0), top), w = min(max((int)fw, 0), top);
        const uint32_t cell = ((uint32_t)u * (uint32_t)R + (uint32_t)v) * (uint32_t)R + (uint32_t)w;
        const float delta_t = leaf_delta_t<false>(px, py, pz, g.Rf, r, opt.step_size);
        const float s = sigma[cell];
        const int32_t cur = __hip_atomic_load(weight_bits + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s > opt.sigma_thresh) {
            const float att = pexpf(-delta_t * r.delta_scale * s);
            const int32_t wb = __float_as_int(T * (1.f - att));
            T *= att;
            if (wb > cur) __hip_atomic_fetch_max(weight_bits + cell, wb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(hits + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        t = march_advance(t, delta_t);
    }
}

// hits between its two forms, in place: the float the caller sees <-> the integer the march counts in
template <bool TO_FLOAT>
__global__ void __launch_bounds__(kGwConvBlock)
grid_hits_convert_kernel(uint32_t* hits, size_t n) {
    const size_t stride = (size_t)gridDim.x * kGwConvBlock;
    for (size_t i = (size_t)blockIdx.x * kGwConvBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t x = hits[i];
        if constexpr (TO_FLOAT) {
            hits[i] = (uint32_t)__float_as_int((float)x);
        } else {
            const float f = __int_as_float((int)x);
            hits[i] = f >= 4294967296.f ? 0xffffffffu : (f > 0.f ? (uint32_t)f : 0u);       // NaN and negatives: 0
        }
    }
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int svoxt_grid_weights(const float* sigma, int32_t R, const svoxt_rays* rays, int32_t n_views, int32_t c2w_stride,
                       const svoxt_options* opt, const float* offset, const float* scaling, int32_t flags, float* weight,
                       float* hits, void* stream) {
    const char* fn = "svoxt_grid_weights";
    if (R < 1 || (double)R * R * R >= 2147483648.0)
        return set_error(SVOXT_ERR_INVALID, "%s: R must be >= 1 with R^3 < 2^31 (32-bit cell indices)", fn);
    if (sigma == nullptr || weight == nullptr || hits == nullptr)
        return set_error(SVOXT_ERR_INVALID, "%s: sigma / weight / hits is NULL", fn);
    if ((void*)weight == (void*)hits || (const void*)sigma == (void*)weight || (const void*)sigma == (void*)hits)
        return set_error(SVOXT_ERR_INVALID, "%s: sigma, weight and hits must be three buffers", fn);
    if (offset == nullptr || scaling == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: offset / scaling is NULL", fn);
    if (opt == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: options is NULL", fn);
    // the march ends because every step adds at least step_size (march_advance ends it where that no longer moves t)
    if (!(opt->step_size > 0.f) || !isfinite(opt->step_size))
        return set_error(SVOXT_ERR_INVALID, "%s: step_size must be finite and > 0", fn);
    if (flags & ~SVOXT_GRIDW_ACCUMULATE) return set_error(SVOXT_ERR_INVALID, "%s: unknown flags", fn);
    if (rays == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: rays is NULL", fn);
    if (rays->Q < 0) return set_error(SVOXT_ERR_INVALID, "%s: negative ray count", fn);
    GridW g;
    g.R = R; g.Rf = (float)R;
    g.tiles_x = 0; g.tiles_per_view = 0; g.c2w_stride = 0;
    int64_t blocks;
    if (rays->c2w != nullptr) {
        if (n_views < 1) return set_error(SVOXT_ERR_INVALID, "%s: camera mode needs n_views >= 1", fn);
        if (c2w_stride != 12 && c2w_stride != 16)
            return set_error(SVOXT_ERR_INVALID, "%s: c2w_stride must be 12 ([V, 3, 4]) or 16 ([V, 4, 4])", fn);
        if (rays->image_width < 1 || rays->image_height < 1 || (int64_t)rays->image_width * rays->image_height != rays->Q)
            return set_error(SVOXT_ERR_INVALID, "%s: camera mode needs Q == image_width * image_height (one view's rays)", fn);
        if (!isfinite(rays->fx) || !isfinite(rays->fy) || rays->fx == 0.f || rays->fy == 0.f)
            return set_error(SVOXT_ERR_INVALID, "%s: camera focal lengths must be finite and non-zero", fn);
        const int64_t tx = ((int64_t)rays->image_width + 7) / 8, ty = ((int64_t)rays->image_height + 7) / 8;
        if (tx * ty > 0x7fffffffLL || tx * ty * n_views > 0x7fffffffLL)
            return set_error(SVOXT_ERR_INVALID, "%s: too many rays for one call (views x 8 x 8 pixel tiles must stay below 2^31)", fn);
        g.tiles_x = (uint32_t)tx; g.tiles_per_view = (uint32_t)(tx * ty); g.c2w_stride = c2w_stride;
        blocks = tx * ty * n_views;
    } else {
        if (n_views != 1) return set_error(SVOXT_ERR_INVALID, "%s: a ray batch is one view: n_views must be 1 (or cameras are missing)", fn);
        if (rays->Q > 0 && (rays->origins == nullptr || rays->dirs == nullptr))
            return set_error(SVOXT_ERR_INVALID, "%s: rays.origins / dirs is NULL", fn);
        blocks = (rays->Q + 63) / 64;
        if (blocks > 0x7fffffffLL) return set_error(SVOXT_ERR_INVALID, "%s: too many rays", fn);
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)R * R * R;
    const unsigned cb = (unsigned)((n + kGwConvBlock - 1) / kGwConvBlock < kGwConvBlocksMax ? (n + kGwConvBlock - 1) / kGwConvBlock
                                                                                           : kGwConvBlocksMax);
    uint32_t* hits_u = reinterpret_cast<uint32_t*>(hits);
    if (flags & SVOXT_GRIDW_ACCUMULATE) {
        hipLaunchKernelGGL(grid_hits_convert_kernel<false>, dim3(cb), dim3(kGwConvBlock), 0, st, hits_u, n);
    } else {
        hipError_t e = hipMemsetAsync(weight, 0, sizeof(float) * n, st);
        if (e == hipSuccess) e = hipMemsetAsync(hits, 0, sizeof(float) * n, st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    }
    if (blocks > 0) {
        TreeDev tr = {};
        tr.offset = offset; tr.scaling = scaling;             // what setup_ray reads of a tree
        RaysDev rd = {};
        rd.origins = rays->origins; rd.dirs = rays->dirs; rd.Q = rays->Q;
        rd.c2w = rays->c2w; rd.fx = rays->fx; rd.fy = rays->fy;
        rd.width = rays->image_width; rd.height = rays->image_height;
        int32_t* wbits = reinterpret_cast<int32_t*>(weight);
        hipLaunchKernelGGL(grid_weights_kernel, dim3((unsigned)blocks), dim3(64), 0, st, sigma, g, tr, rd, to_dev(opt), wbits, hits_u);
    }
    hipLaunchKernelGGL(grid_hits_convert_kernel<true>, dim3(cb), dim3(kGwConvBlock), 0, st, hits_u, n);
    return check_launch(fn);
}

}  // extern "C"
