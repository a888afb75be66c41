// svoxt_bwd.hip -- volume_render_backward (trace_ray_backward, rt_kernel.cu:331-496, 675-694, 1402-1426) and
// opacity_render_backward (:1593-1616) behind the C ABI: which kernel of svoxt_bwd_kernels.h serves a payload / list
// combination.  A translation unit of its own so that the two halves of the library's kernels compile side by side
// (svoxt_kernels.hip keeps the forward, the queries and the utilities).  DESIGN.md 4 (the measurements behind it: NOTEBOOK.md 5).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see build.py).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoxt_launch.h"

#pragma clang fp contract(off)

#include "svoxt_bwd_kernels.h"

using namespace svoxt;

namespace {
int64_t* g_bwd_counters = nullptr;      // svoxt_set_bwd_counters (instrumentation)
int64_t* g_bwd_check = nullptr;         // svoxt_set_bwd_check (instrumentation): the per-tile backwards run their CHECK instances

// specialised kernels with per-leaf view rotations: SH payloads on N = 2 trees
template <bool REPLAY>
bool launch_bwd_xform(const TreeDev& tr, const RaysDev& rays, const Opts& opt, int C,
                      const float* grad_out, float* grad, int gstride, RecLists L, const uint4* aux,
                      const float* fwd_out, hipStream_t st) {
    if (opt.format != FMT_SH || C != 3) return false;
    return with_int(SpecialBases{}, opt.basis_dim, [&](auto BB) {
        hipLaunchKernelGGL((render_bwd_kernel<FMT_SH, 3, BB, true, REPLAY, true>), dim3(nblocks(rays.Q)), dim3(kBlock), 0, st,
                           tr, rays, opt, grad_out, grad, gstride, L, aux, fwd_out);
        return true;
    });
}

bool launch_lobes_bwd_tiles(const TreeDev& tr, const RaysDev& rays, const Opts& opt, const float* grad_out, float* grad,
                            int gstride, RecLists L, const uint4* aux, hipStream_t st, int terms_state) {
    if (L.terms == nullptr || terms_state != 3 || !lobes_payload(opt, tr.K) || g_bwd_counters != nullptr) return false;
    const unsigned nb = nblocks(rays.Q);
    return with_int(SpecialBases{}, opt.basis_dim, [&](auto BB) {
        hipLaunchKernelGGL((render_bwd_kernel<FMT_SH, 3, BB, true, true, false, true, false, true>), dim3(nb), dim3(kBlock), 0, st,
                           tr, rays, opt, grad_out, grad, gstride, L, aux, nullptr, nullptr);
        hipLaunchKernelGGL((grad_fused_kernel<FMT_SH, BB, true, false, 3, true>), dim3(nb), dim3(512), 0, st,
                           tr, rays, opt, grad_out, L, aux, nullptr, grad, gstride);
        return true;
    });
}

// The grad_wide_kernel instance for rows of KK floats (nullptr: none -- a checked run of the fast-math form)
template <int KK>
auto wide_instance(bool check, bool count, bool native, bool etab) -> decltype(&grad_wide_kernel<KK>) {
    if (check) return native ? nullptr : grad_wide_kernel<KK, false, false, true>;
    if (count) return grad_wide_kernel<KK, false, true>;
    if (native) return grad_wide_kernel<KK, true>;
    return etab ? grad_wide_kernel<KK, false, false, false, true> : grad_wide_kernel<KK, false>;
}

// The grad_fused_kernel instance of the one-kernel per-tile backward (nullptr: none).  handover: the forward's
// hand-over in L.terms, terms_state 2 (lane-major) or 3 (position-major); 0: none.
template <int F, int BB>
auto fused_instance(bool check, bool count, bool fwd_out, int handover) -> decltype(&grad_fused_kernel<F, BB, true>) {
    if (check) {
        // the checked instance of the route that would run: the default route (the forward's position-major
        // hand-over) for every payload, the other routes for SH9
        if (handover == 3 && !fwd_out) return grad_fused_kernel<F, BB, true, false, 3, false, true>;
        if constexpr (F == FMT_SH && BB == 9) {
            if (fwd_out) return grad_fused_kernel<F, BB, false, false, 0, false, true>;
            return handover == 2 ? grad_fused_kernel<F, BB, true, false, 2, false, true>
                                 : grad_fused_kernel<F, BB, true, false, 0, false, true>;
        }
        return nullptr;
    }
    if constexpr (BB > 9) {
        // (SH16 / SH25: only over a hand-over, without counters -- see launch_bwd_gather)
        return handover == 2 ? grad_fused_kernel<F, BB, true, false, 2> : grad_fused_kernel<F, BB, true, false, 3>;
    } else {
        if (count) return fwd_out ? grad_fused_kernel<F, BB, false, true> : grad_fused_kernel<F, BB, true, true>;
        if (fwd_out) return grad_fused_kernel<F, BB, false>;
        if (handover == 2) return grad_fused_kernel<F, BB, true, false, 2>;
        if (handover == 3) return grad_fused_kernel<F, BB, true, false, 3>;
        return grad_fused_kernel<F, BB, true>;     // (no hand-over from the forward: both sweeps gather the rows)
    }
}

// The per-tile backward over sample lists on N = 2 trees: the two-kernel form (list walk into coef + grad_merge_kernel)
// for SH 1/4/9 (also with view rotations) and RGBA with 3 channels (K <= 32), or the one-kernel form (grad_fused_kernel,
// grad_wide_kernel) for those, for SH16 / SH25 and for RGBA-style rows of 8 / 16 / 32 floats
bool launch_bwd_gather(const TreeDev& tr, const RaysDev& rays, const Opts& opt, int C,
                       const float* grad_out, float* grad, int gstride, RecLists L, const uint4* aux,
                       const float* fwd_out, float4* coef, bool xf, hipStream_t st, int terms_state = 0,
                       bool native = false) {
    const unsigned nb = nblocks(rays.Q);
    unsigned long long* ctr = reinterpret_cast<unsigned long long*>(g_bwd_counters);
    unsigned long long* chkw = reinterpret_cast<unsigned long long*>(g_bwd_check);
    unsigned long long* words = chkw != nullptr ? chkw : ctr;          // (for the checked / counting instances)
    // The one-kernel per-tile forms launch the tails of overflowed rays first (a tail-only launch of the per-ray kernel);
    // where no per-tile instance serves the call then, it returns false after that launch.
    auto tails = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(kBlock), 0, st, tr, rays, opt, grad_out, grad, gstride, L, aux, fwd_out, nullptr);
    };
    if (C > 3) {
        // RGBA-style rows of 8 / 16 / 32 floats: the exact per-tile form only (one kernel, a float per
        // list slot in L.terms); tails of overflowed rays first, as for the 3-channel fused kernel
        if (opt.format != FMT_RGBA || coef != nullptr || xf || fwd_out != nullptr || L.terms == nullptr || C + 1 != tr.K)
            return false;
        return with_int(ChanRows{}, tr.K, [&](auto KK) {
            tails(render_bwd_kernel<FMT_RGBA, KK - 1, 0, true, true, false, true>);
            const auto k = wide_instance<KK>(chkw != nullptr, ctr != nullptr, native, tr.etab != nullptr);
            if (k == nullptr) return false;
            hipLaunchKernelGGL(k, dim3(nb), dim3(512), 0, st, tr, rays, opt, grad_out, L, aux, grad, gstride, words);
            return true;
        });
    }
    if (C != 3) return false;
    // a caller that hands over a coef buffer asks for the two-kernel form; without one (coef_bytes < 0)
    // the per-tile route runs if it can run as ONE kernel.  (The choice is the caller's alone: the
    // library reads no environment for it.)
    const bool fused = coef == nullptr;
    // the two-kernel form: list walk (coefficients into coef), then merge.  Four wavefronts per tile and tables of
    // 1024 (measured: one wavefront per tile 0.41 ms, two 0.33, four 0.30 before step 15; tables of 512 / 256 cost
    // more passes than they buy)
    auto two_kernels = [&](auto F, auto BB, auto XF) {
        hipLaunchKernelGGL((render_bwd_kernel<F, 3, BB, true, true, XF, true>), dim3(nb), dim3(kBlock), 0, st,
                           tr, rays, opt, grad_out, grad, gstride, L, aux, fwd_out, coef);
        hipLaunchKernelGGL((grad_merge_kernel<F, BB, 1024, XF ? 512 : 1024, 4, XF>), dim3(nb), dim3(256), 0, st,
                           tr, rays, grad_out, L, coef, aux, grad, gstride);
        return true;
    };
    // the one-kernel form: tails, then list walk and merge in one kernel
    auto one_kernel = [&](auto F, auto BB) {
        tails(render_bwd_kernel<F, 3, BB, true, true, false, true>);
        const int handover = L.terms != nullptr && (terms_state == 2 || terms_state == 3) ? terms_state : 0;
        const auto k = fused_instance<F, BB>(chkw != nullptr, ctr != nullptr, fwd_out != nullptr, handover);
        if (k == nullptr) return false;
        hipLaunchKernelGGL(k, dim3(nb), dim3(512), 0, st, tr, rays, opt, grad_out, L, aux, fwd_out, grad, gstride, words);
        return true;
    };
    if (xf) {
        if (opt.format != FMT_SH || (fused && fwd_out != nullptr)) return false;   // (the exact one-kernel form only)
        return with_int(XfRolesBases{}, opt.basis_dim, [&](auto BB) {
            if (!fused) return two_kernels(Int<FMT_SH>{}, BB, std::true_type{});
            // (r04) view rotations as ONE kernel: the rays whose list overflowed whole by the per-ray kernel, every other
            // ray by grad_fused_kernel<..., XF> (no checked / counting instance: svoxt_set_bwd_check and _counters do not
            // see this route); over the forward's hand-over (exponentials of each record's own basis) where it left one
            hipLaunchKernelGGL((render_bwd_kernel<FMT_SH, 3, BB, true, true, true>), dim3(nb), dim3(kBlock), 0, st,
                               tr, rays, opt, grad_out, grad, gstride, L, aux, fwd_out, reinterpret_cast<float4*>(kOnlyOverflowed));
            const auto k = L.terms != nullptr && terms_state == 3 ? grad_fused_kernel<FMT_SH, BB, true, false, 3, false, false, true>
                                                                  : grad_fused_kernel<FMT_SH, BB, true, false, 0, false, false, true>;
            hipLaunchKernelGGL(k, dim3(nb), dim3(512), 0, st, tr, rays, opt, grad_out, L, aux, fwd_out, grad, gstride, nullptr);
            return true;
        });
    }
    if (opt.format == FMT_RGBA)
        return fused ? one_kernel(Int<FMT_RGBA>{}, Int<0>{}) : two_kernels(Int<FMT_RGBA>{}, Int<0>{}, std::false_type{});
    if (opt.format != FMT_SH) return false;
    return with_int(SpecialBases{}, opt.basis_dim, [&](auto BB) {
        if constexpr (BB > 9) {
            // SH16 / SH25 (rows of 49 / 76 floats, r03): the one-kernel per-tile form only, and only over the hand-over a
            // recording forward left (terms_state 2 / 3): the kernel then never holds a feature row
            if (!fused || ctr != nullptr || fwd_out != nullptr || L.terms == nullptr || (terms_state != 2 && terms_state != 3))
                return false;
            return one_kernel(Int<FMT_SH>{}, BB);
        } else {
            return fused ? one_kernel(Int<FMT_SH>{}, BB) : two_kernels(Int<FMT_SH>{}, BB, std::false_type{});
        }
    });
}

template <bool N2, bool REPLAY>
bool launch_bwd_special(const TreeDev& tr, const RaysDev& rays, const Opts& opt, int C,
                        const float* grad_out, float* grad, int gstride, RecLists L, const uint4* aux,
                        const float* fwd_out, hipStream_t st) {
    auto bwd = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nblocks(rays.Q)), dim3(kBlock), 0, st,
                           tr, rays, opt, grad_out, grad, gstride, L, aux, fwd_out, nullptr);
        return true;
    };
    if (opt.format == FMT_RGBA)
        return with_int(RgbaWidths{}, C, [&](auto CC) {
            if constexpr (REPLAY && CC > 3) {
                // lists + a float per slot + the exact form asked for: one sigmoid pass instead of two
                if (L.terms != nullptr && fwd_out == nullptr) return bwd(render_bwd_kernel<FMT_RGBA, CC, 0, N2, true, false, false, true>);
            }
            return bwd(render_bwd_kernel<FMT_RGBA, CC, 0, N2, REPLAY>);
        });
    if (opt.format == FMT_SH)
        return C == 3 && with_int(SpecialBases{}, opt.basis_dim, [&](auto BB) { return bwd(render_bwd_kernel<FMT_SH, 3, BB, N2, REPLAY>); });
    if constexpr (!REPLAY) {
        if (C == 3 && lobes_payload(opt, tr.K))
            return with_int(SpecialBases{}, opt.basis_dim, [&](auto BB) {
                return bwd(render_bwd_kernel<FMT_SH, 3, BB, N2, false, false, false, false, true>);
            });
    }
    return false;
}

}  // namespace

namespace svoxt {

int bwd_common(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
               const float* grad_out, int32_t grad_cols, float* grad_features, int32_t grad_stride,
               void* workspace, int64_t workspace_bytes, const svoxt_sample_lists* lists,
               const float* fwd_out, void* stream, const char* fn) {
    int rc;
    if ((rc = check_tree(tree, fn)) || (rc = check_rays(rays, fn)) ||
        (rc = check_opts(opt, tree, fn, grad_cols > 1)))
        return rc;
    // (the opacity backward, grad_cols == 1, reads sigma alone, float by float)
    if (grad_cols > 1 && (rc = check_features_vec(tree, fn))) return rc;
    if (grad_features == nullptr && tree->M > 0) return fail(SVOXT_ERR_INVALID, "%s: grad_features is NULL", fn);
    if (rays->Q > 0 && grad_out == nullptr) return fail(SVOXT_ERR_INVALID, "%s: grad_out is NULL", fn);
    const int C = grad_cols - 1;
    if (C < 0) return fail(SVOXT_ERR_INVALID, "%s: grad_cols must be >= 1", fn);
    if (C > 0) {
        const int want = svoxt_out_data_dim(opt, tree->K);
        if (want != grad_cols) return fail(SVOXT_ERR_INVALID, "%s: grad_out columns do not match get_out_data_dim", fn);
    }
    const int gs = grad_stride > 0 ? grad_stride : tree->K;
    if (gs < tree->K) return fail(SVOXT_ERR_INVALID, "%s: grad_stride smaller than data_dim", fn);
    hipStream_t st = (hipStream_t)stream;
    // (SVOXT_LISTS_GRAD_ZEROED: the caller's buffer is the scratch svoxt_compact_rows_clear left zeroed)
    if (tree->M > 0 && !(lists != nullptr && (lists->flags & SVOXT_LISTS_GRAD_ZEROED))) {
        const hipError_t e = hipMemsetAsync(grad_features, 0, sizeof(float) * (size_t)tree->M * gs, st);
        if (e != hipSuccess) return fail(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    }
    if (rays->Q == 0 || tree->M == 0) return SVOXT_OK;
    const TreeDev tr = to_dev(tree);
    const RaysDev rd = to_dev(rays, tree, lists);
    const Opts od = to_dev(opt);
    const bool n2 = tree->N == 2;
    bool done = false;
    const bool xf = uses_xform(tree, opt);
    if (xf && lists != nullptr && !(full_comp(opt) && xform_special(tree, opt)))
        return fail(SVOXT_ERR_UNSUPPORTED, "%s: sample lists with transformation_matrices need an SH payload on an N = 2 tree", fn);
    if (C > 0 && full_comp(opt) && xf && xform_special(tree, opt)) {
        const int64_t S = workspace != nullptr ? rec_capacity(workspace_bytes, rays->Q) : 0;
        if (lists != nullptr) {
            const int64_t need = (int64_t)lists->max_samples * rays->Q * 32;
            if (lists->coef != nullptr && tree->K <= 32 && lists->coef_bytes >= need)
                done = launch_bwd_gather(tr, rd, od, C, grad_out, grad_features, gs, lists_dev(lists, rays->Q),
                                         reinterpret_cast<const uint4*>(lists->aux), fwd_out,
                                         reinterpret_cast<float4*>(lists->coef), true, st);
            else if (lists->coef == nullptr && lists->coef_bytes < 0 && tree->K <= 32 && fwd_out == nullptr && C == 3 && n2)
                done = launch_bwd_gather(tr, rd, od, C, grad_out, grad_features, gs, lists_dev(lists, rays->Q),
                                         reinterpret_cast<const uint4*>(lists->aux), fwd_out, nullptr, true, st,
                                         lists->terms_state == 3 ? 3 : 0);     // list walk + merge as one kernel (over the forward's hand-over, if it left one)
            if (!done)
                done = launch_bwd_xform<true>(tr, rd, od, C, grad_out, grad_features, gs, lists_dev(lists, rays->Q),
                                              reinterpret_cast<const uint4*>(lists->aux), fwd_out, st);
        }
        else
            done = launch_bwd_xform<false>(tr, rd, od, C, grad_out, grad_features, gs,
                                           dense_lists(S > 0 ? workspace : nullptr, S, rays->Q), nullptr, nullptr, st);
    } else if (C > 0 && full_comp(opt) && !xf)
    {
        // per-ray sample lists: S entries of 8 bytes per ray, laid out rec[k][q]
        const int64_t S = workspace != nullptr ? rec_capacity(workspace_bytes, rays->Q) : 0;
        const RecLists wl = dense_lists(S > 0 ? workspace : nullptr, S, rays->Q);
        if (lists != nullptr) {
            // hand-over per list slot: 16 bytes for 3-channel payloads; RGBA rows of 8 / 16 / 32 floats: 8 for the
            // per-tile kernel (grad_wide_kernel), 4 for the per-ray one (render_bwd_kernel<ONEPASS>)
            const bool wide = opt->format == SVOXT_FORMAT_RGBA && C > 3;
            const RecLists ll = lists_dev(lists, rays->Q, wide ? 8 : 16);
            const RecLists l1 = wide ? lists_dev(lists, rays->Q, 4) : ll;
            const uint4* laux = reinterpret_cast<const uint4*>(lists->aux);
            // coef_bytes < 0 (and no coef): the per-tile route if it can run fused, which needs no buffer
            if (lobes_payload(od, tree->K)) {
                // SG / ASG: the one-kernel per-tile backward over the forward's hand-over, or nothing
                if (n2 && lists->coef_bytes < 0)
                    done = launch_lobes_bwd_tiles(tr, rd, od, grad_out, grad_features, gs, ll, laux, st, lists->terms_state);
                if (!done) return fail(SVOXT_ERR_UNSUPPORTED, "%s: SG / ASG sample lists serve the per-tile backward only (N = 2, lists.terms filled by the forward: terms_state 3, coef_bytes < 0)", fn);
                return check_launch(fn);
            }
            const bool have_coef = lists->coef != nullptr &&
                                   lists->coef_bytes >= (int64_t)lists->max_samples * rays->Q * 16;
            // (rows wider than 32 floats: SH16 / SH25 over the forward's hand-over, one kernel -- launch_bwd_gather decides)
            if (n2 && (tree->K <= 32 || !have_coef) && (have_coef || lists->coef_bytes < 0))
                // (ll.terms: the exact one-kernel form's hand-over buffer; terms_state 2 = the forward filled it)
                done = launch_bwd_gather(tr, rd, od, C, grad_out, grad_features, gs, ll, laux,
                                         fwd_out, have_coef ? reinterpret_cast<float4*>(lists->coef) : nullptr, false, st,
                                         (lists->terms_state == 2 || lists->terms_state == 3) ? lists->terms_state : 1,
                                         (lists->flags & SVOXT_LISTS_NATIVE_MATH) != 0);
            if (!done)
                done = with_bool(n2, [&](auto N2) {
                    return launch_bwd_special<N2, true>(tr, rd, od, C, grad_out, grad_features, gs, l1, laux, fwd_out, st);
                });
            if (!done) return fail(SVOXT_ERR_UNSUPPORTED, "%s: no specialised kernel for this payload", fn);
        } else {
            done = with_bool(n2, [&](auto N2) {
                return launch_bwd_special<N2, false>(tr, rd, od, C, grad_out, grad_features, gs, wl, nullptr, nullptr, st);
            });
        }
    } else if (lists != nullptr) {
        return fail(SVOXT_ERR_UNSUPPORTED, "%s: sample lists need a specialised payload", fn);
    }
    if (!done) {
        const unsigned nb = nblocks(rays->Q);
        const size_t lds = (size_t)(kBlock / 64) * 64 * (tree->K | 1) * sizeof(float) + kBlock * sizeof(int32_t);
        // shaped atomics through LDS staging (default dynamic-LDS limit: 64 KiB); unstaged for C == 0 (opacity: one value
        // per sample, nothing to shape) or rows too wide to stage
        const bool staged = C > 0 && lds <= 65536;
        const auto k = staged ? (n2 ? render_bwd_generic_staged_kernel<true> : render_bwd_generic_staged_kernel<false>)
                              : (n2 ? render_bwd_generic_kernel<true> : render_bwd_generic_kernel<false>);
        hipLaunchKernelGGL(k, dim3(nb), dim3(kBlock), staged ? lds : 0, st, tr, rd, od, C, grad_out, grad_features, gs);
    }
    return check_launch(fn);
}

}  // namespace svoxt

extern "C" {

int svoxt_set_bwd_counters(int64_t* counters) {
    g_bwd_counters = counters;
    return SVOXT_OK;
}

int svoxt_set_bwd_check(int64_t* words) {
    g_bwd_check = words;
    return SVOXT_OK;
}

}  // extern "C"
