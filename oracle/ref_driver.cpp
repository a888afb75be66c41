// ref_driver.cpp -- runs the reference's own __global__ functions on one host
// thread, one thread id at a time.  TEST INFRASTRUCTURE ONLY.
//
// oracle/ref.py compiles this file with g++ together with two files that it
// derives at build time from the reference's rt_kernel.cu and svox_kernel.cu
// (their text up to the end of the device namespace: the host entry points with
// the <<<...>>> launches are left out) and with the stand-in headers of
// oracle/ref_shim first on the include path.  The derived files live only under
// oracle/_ref/ and are never committed.
//
// Every entry point wraps caller-owned buffers as CPU tensors (torch::from_blob),
// fills TreeSpec / RaysSpec / CameraSpec, packs them exactly as the reference's
// host entry points do (the implicit Packed*Spec constructors), and calls the
// kernel for thread ids 0 .. Q-1 in ascending order.  That is one legal schedule
// of the reference: racing writes and float atomics become deterministic, and a
// sum of atomics is the sequential sum in thread order.  The check() methods are
// not called (they insist on CUDA tensors).  Outputs that the reference
// allocates with torch::zeros are zeroed here; outputs that it allocates with
// torch::empty are left as the caller passed them.
//
// `is_double` selects the reference's float or double instantiation.

#include "rt_kernel.device.inc"
#include "svox_kernel.device.inc"

#include <vector>

namespace {

// all-int64 so that the ctypes mirror in oracle/ref.py has no padding to guess
struct RefTree {
    void* features; int64_t M, K;
    int32_t* data; int32_t* child; int32_t* parent_depth; int64_t n_internal, N;
    void* offset; void* scaling;
    void* extra; int64_t extra_rows, extra_cols;
    void* weight_accum;                                   // [n_internal * N^3] or null
    void* joint_features; int64_t n_joints, F;
    void* skinning_weights; int32_t* joint_index; int64_t B;
    void* xform; int64_t xform_rows, xform_dim;           // transformation_matrices [rows, dim, dim] or null
};

template <typename T> constexpr c10::ScalarType st() { return c10::CppTypeToScalarType<T>::value; }

template <typename T>
torch::Tensor wrap(const void* p, std::vector<int64_t> shape) {
    int64_t n = 1;
    for (int64_t s : shape) n *= s;
    if (p == nullptr || n == 0) return torch::empty(shape, torch::TensorOptions().dtype(st<T>()));
    return torch::from_blob(const_cast<void*>(p), shape, torch::TensorOptions().dtype(st<T>()));
}

// Accessors hold the pointer and copies of the sizes, not the tensor: the buffers are the caller's.
template <typename T, size_t N>
auto acc32(const torch::Tensor& t) { return t.packed_accessor32<T, N, torch::RestrictPtrTraits>(); }
template <typename T, size_t N>
auto acc64(const torch::Tensor& t) { return t.packed_accessor64<T, N, torch::RestrictPtrTraits>(); }

template <typename T>
TreeSpec make_tree(const RefTree& t) {
    TreeSpec s;
    s.features = wrap<T>(t.features, {t.M, t.K});
    s.data = wrap<int32_t>(t.data, {t.n_internal, t.N, t.N, t.N, 1});
    s.child = wrap<int32_t>(t.child, {t.n_internal, t.N, t.N, t.N});
    s.parent_depth = wrap<int32_t>(t.parent_depth, {t.parent_depth ? t.n_internal : 0, 2});
    s.extra_data = wrap<T>(t.extra, {t.extra_rows, t.extra_cols});
    s.offset = wrap<T>(t.offset, {3});
    s.scaling = wrap<T>(t.scaling, {3});
    s._weight_accum = wrap<T>(t.weight_accum, {t.weight_accum ? t.n_internal * t.N * t.N * t.N : 0});
    s.joint_features = wrap<T>(t.joint_features, {t.n_joints, t.F});
    s.skinning_weights = wrap<T>(t.skinning_weights, {t.skinning_weights ? t.M : 0, t.B});
    s.joint_index = wrap<int32_t>(t.joint_index, {t.joint_index ? t.M : 0, t.B});
    s.transformation_matrices = wrap<T>(t.xform, {t.xform ? t.xform_rows : 0, t.xform_dim, t.xform_dim});
    s.n_internal = (int)t.n_internal;
    return s;
}

template <typename T>
RaysSpec make_rays(const void* o, const void* d, const void* v, int64_t Q) {
    RaysSpec r;
    r.origins = wrap<T>(o, {Q, 3});
    r.dirs = wrap<T>(d, {Q, 3});
    r.vdirs = wrap<T>(v, {Q, 3});
    return r;
}

template <typename T>
CameraSpec make_cam(const void* c2w, int64_t rows, float fx, float fy, int w, int h) {
    CameraSpec c;
    c.c2w = wrap<T>(c2w, {rows, 4});
    c.fx = fx; c.fy = fy; c.width = w; c.height = h;
    return c;
}

// thread ids 0 .. n-1 in ascending order, a block of one thread each
template <typename F>
void for_threads(int64_t n, F&& kernel) {
    blockDim.x = 1;
    threadIdx.x = 0;
    for (int64_t i = 0; i < n; ++i) {
        blockIdx.x = (unsigned int)i;
        kernel();
    }
    blockIdx.x = 0;
}

template <typename T> void zero(void* p, int64_t n) { std::memset(p, 0, sizeof(T) * (size_t)n); }

template <typename T>
void volume_render(const RefTree& t, const void* o, const void* d, const void* v, int64_t Q, RenderOptions opt,
                   void* out, int64_t cols) {
    TreeSpec tree = make_tree<T>(t);
    RaysSpec rays = make_rays<T>(o, d, v, Q);
    zero<T>(out, Q * cols);
    auto res = acc32<T, 2>(wrap<T>(out, {Q, cols}));
    PackedTreeSpec<T> pt(tree);
    PackedRaysSpec<T> pr(rays);
    for_threads(Q, [&] { device::render_ray_kernel<T>(pt, pr, opt, res); });
}

template <typename T>
void volume_render_backward(const RefTree& t, const void* o, const void* d, const void* v, int64_t Q, RenderOptions opt,
                            const void* grad_out, int64_t cols, void* grad) {
    TreeSpec tree = make_tree<T>(t);
    RaysSpec rays = make_rays<T>(o, d, v, Q);
    zero<T>(grad, t.M * t.K);
    auto go = acc32<T, 2>(wrap<T>(grad_out, {Q, cols}));
    auto res = acc64<T, 2>(wrap<T>(grad, {t.M, t.K}));
    PackedTreeSpec<T> pt(tree);
    PackedRaysSpec<T> pr(rays);
    for_threads(Q, [&] { device::render_ray_backward_kernel<T>(pt, go, pr, opt, res); });
}

template <typename T>
void volume_render_image(const RefTree& t, const void* c2w, int64_t rows, float fx, float fy, int w, int h, RenderOptions opt,
                         void* out, int64_t cols) {
    TreeSpec tree = make_tree<T>(t);
    CameraSpec cam = make_cam<T>(c2w, rows, fx, fy, w, h);
    zero<T>(out, (int64_t)w * h * cols);
    auto res = acc32<T, 3>(wrap<T>(out, {h, w, cols}));
    PackedTreeSpec<T> pt(tree);
    PackedCameraSpec<T> pc(cam);
    for_threads((int64_t)w * h, [&] { device::render_image_kernel<T>(pt, pc, opt, res); });
}

template <typename T>
void volume_render_image_backward(const RefTree& t, const void* c2w, int64_t rows, float fx, float fy, int w, int h,
                                  RenderOptions opt, const void* grad_out, int64_t cols, void* grad) {
    TreeSpec tree = make_tree<T>(t);
    CameraSpec cam = make_cam<T>(c2w, rows, fx, fy, w, h);
    zero<T>(grad, t.M * t.K);
    auto go = acc32<T, 3>(wrap<T>(grad_out, {h, w, cols}));
    auto res = acc64<T, 2>(wrap<T>(grad, {t.M, t.K}));
    PackedTreeSpec<T> pt(tree);
    PackedCameraSpec<T> pc(cam);
    for_threads((int64_t)w * h, [&] { device::render_image_backward_kernel<T>(pt, go, pc, opt, res); });
}

template <typename T>
void opacity_render(const RefTree& t, const void* o, const void* d, const void* v, int64_t Q, RenderOptions opt, void* out) {
    TreeSpec tree = make_tree<T>(t);
    RaysSpec rays = make_rays<T>(o, d, v, Q);
    zero<T>(out, Q);
    auto res = acc32<T, 2>(wrap<T>(out, {Q, 1}));
    PackedTreeSpec<T> pt(tree);
    PackedRaysSpec<T> pr(rays);
    for_threads(Q, [&] { device::opacity_render_ray_kernel<T>(pt, pr, opt, res); });
}

template <typename T>
void render_depth(const RefTree& t, const void* o, const void* d, const void* v, int64_t Q, RenderOptions opt, void* out) {
    TreeSpec tree = make_tree<T>(t);
    RaysSpec rays = make_rays<T>(o, d, v, Q);
    zero<T>(out, Q);
    auto res = acc32<T, 2>(wrap<T>(out, {Q, 1}));
    PackedTreeSpec<T> pt(tree);
    PackedRaysSpec<T> pr(rays);
    for_threads(Q, [&] { device::depth_render_ray_kernel<T>(pt, pr, opt, res); });
}

template <typename T>
void motion_render(const RefTree& t, const void* o, const void* d, const void* v, int64_t Q, RenderOptions opt,
                   void* out, void* depth, void* hit_point, int64_t* data_idx) {
    TreeSpec tree = make_tree<T>(t);
    RaysSpec rays = make_rays<T>(o, d, v, Q);
    const int64_t J = t.extra_rows;
    zero<T>(out, Q * J); zero<T>(depth, Q); zero<T>(hit_point, Q * 3); zero<int64_t>(data_idx, Q);
    auto a = acc32<T, 2>(wrap<T>(out, {Q, J}));
    auto b = acc32<T, 2>(wrap<T>(depth, {Q, 1}));
    auto c = acc32<T, 2>(wrap<T>(hit_point, {Q, 3}));
    auto e = acc32<int64_t, 2>(wrap<int64_t>(data_idx, {Q, 1}));
    PackedTreeSpec<T> pt(tree);
    PackedRaysSpec<T> pr(rays);
    for_threads(Q, [&] { device::motion_render_ray_kernel<T>(pt, pr, opt, a, b, c, e); });
}

template <typename T>
void motion_feature_render(const RefTree& t, const void* o, const void* d, const void* v, int64_t Q, RenderOptions opt, void* out) {
    TreeSpec tree = make_tree<T>(t);
    RaysSpec rays = make_rays<T>(o, d, v, Q);
    zero<T>(out, Q * t.F);
    auto res = acc32<T, 2>(wrap<T>(out, {Q, t.F}));
    PackedTreeSpec<T> pt(tree);
    PackedRaysSpec<T> pr(rays);
    for_threads(Q, [&] { device::moition_feature_render_ray_kernel<T>(pt, pr, opt, res); });
}

template <typename T>
void grid_weight_render(const void* sigma, int64_t R, const void* c2w, int64_t rows, float fx, float fy, int w, int h,
                        RenderOptions opt, const void* offset, const void* scaling, void* grid_weight, void* grid_hit) {
    CameraSpec cam = make_cam<T>(c2w, rows, fx, fy, w, h);
    auto data = acc32<T, 3>(wrap<T>(sigma, {R, R, R}));
    auto gw = acc32<T, 3>(wrap<T>(grid_weight, {R, R, R}));
    auto gh = acc32<T, 3>(wrap<T>(grid_hit, {R, R, R}));
    PackedCameraSpec<T> pc(cam);
    // not zeroed: the caller passes zeros for one view, or the running result to go on over several
    for_threads((int64_t)w * h, [&] {
        device::grid_weight_render_kernel<T>(data, pc, opt, (const T*)offset, (const T*)scaling, gw, gh);
    });
}

// query_vertical's three kernels.  values / node_ids / data_ids are torch::empty in the reference: rows of points whose
// leaf names no feature row keep what the caller put there.  leaf_node [n_hit, 4] is returned through leaf_node_out
// (capacity rows) and its row count as the result.
template <typename T>
int64_t query_vertical(const RefTree& t, const void* points, int64_t Q, void* values, int64_t* node_ids, int64_t* data_ids,
                       int64_t* leaf_node_out, int64_t capacity) {
    TreeSpec tree = make_tree<T>(t);
    const int64_t slots = t.n_internal * t.N * t.N * t.N;
    torch::Tensor mask = torch::full({slots}, -1, torch::kLong);
    torch::Tensor num_hit = torch::zeros({1}, torch::TensorOptions().dtype(st<T>()));
    auto idx = acc32<T, 2>(wrap<T>(points, {Q, 3}));
    auto val = acc64<T, 2>(wrap<T>(values, {Q, t.K}));
    auto nid = acc32<int64_t, 1>(wrap<int64_t>(node_ids, {Q}));
    auto did = acc32<int64_t, 1>(wrap<int64_t>(data_ids, {Q}));
    auto msk = mask.packed_accessor32<int64_t, 1, torch::RestrictPtrTraits>();
    PackedTreeSpec<T> pt(tree);
    for_threads(Q, [&] { device::query_single_kernel<T>(pt, idx, val, nid, did, msk); });
    auto nh = num_hit.template packed_accessor32<T, 1, torch::RestrictPtrTraits>();
    for_threads(slots, [&] { device::generate_index_kernel<T>(nh, msk); });
    const int64_t n_hit = num_hit.template item<int>();
    torch::Tensor leaf_node = torch::zeros({n_hit, 4}, torch::kLong);
    auto ln = leaf_node.packed_accessor32<int64_t, 2, torch::RestrictPtrTraits>();
    for_threads(slots, [&] { device::unpack_mask_kernel<T>(pt, msk, ln); });
    if (leaf_node_out != nullptr && n_hit <= capacity && n_hit > 0)
        std::memcpy(leaf_node_out, leaf_node.data_ptr<int64_t>(), sizeof(int64_t) * (size_t)n_hit * 4);
    return n_hit;
}

template <typename T>
void query_vertical_backward(const RefTree& t, const void* points, int64_t Q, const void* grad_out, void* grad) {
    TreeSpec tree = make_tree<T>(t);
    zero<T>(grad, t.M * t.K);
    auto idx = acc32<T, 2>(wrap<T>(points, {Q, 3}));
    auto go = acc64<T, 2>(wrap<T>(grad_out, {Q, t.K}));
    auto res = acc32<T, 2>(wrap<T>(grad, {t.M, t.K}));
    PackedTreeSpec<T> pt(tree);
    for_threads(Q, [&] { device::query_single_kernel_backward<T>(pt, idx, go, res); });
}

template <typename T>
void warp_vertices(const void* matrices, int64_t J, int64_t D, const void* points, int64_t Q, const void* sw, const int32_t* ji,
                   int64_t B, void* vertices_out, void* matrix_out) {
    zero<T>(vertices_out, Q * 3); zero<T>(matrix_out, Q * D * D);
    auto m = acc32<T, 3>(wrap<T>(matrices, {J, D, D}));
    auto p = acc32<T, 2>(wrap<T>(points, {Q, 3}));
    auto w = acc32<T, 2>(wrap<T>(sw, {Q, B}));
    auto j = acc32<int32_t, 2>(wrap<int32_t>(ji, {Q, B}));
    auto mo = acc32<T, 3>(wrap<T>(matrix_out, {Q, D, D}));
    auto vo = acc32<T, 2>(wrap<T>(vertices_out, {Q, 3}));
    for_threads(Q, [&] { device::warp_vertices_kernel<T>(m, p, w, j, mo, vo); });
}

template <typename T>
void warp_vertices_backward(const void* matrices, int64_t J, int64_t D, const void* points, int64_t Q, const void* sw,
                            const int32_t* ji, int64_t B, const void* grad_vertices, const void* grad_matrix_out,
                            void* grad_points, void* grad_matrices, void* grad_sw) {
    zero<T>(grad_points, Q * 3); zero<T>(grad_matrices, J * D * D); zero<T>(grad_sw, Q * B);
    auto gv = acc32<T, 2>(wrap<T>(grad_vertices, {Q, 3}));
    auto gm = acc32<T, 3>(wrap<T>(grad_matrix_out, {Q, D, D}));
    auto m = acc32<T, 3>(wrap<T>(matrices, {J, D, D}));
    auto p = acc32<T, 2>(wrap<T>(points, {Q, 3}));
    auto w = acc32<T, 2>(wrap<T>(sw, {Q, B}));
    auto j = acc32<int32_t, 2>(wrap<int32_t>(ji, {Q, B}));
    auto a = acc32<T, 3>(wrap<T>(grad_matrices, {J, D, D}));
    auto b = acc32<T, 2>(wrap<T>(grad_points, {Q, 3}));
    auto c = acc32<T, 2>(wrap<T>(grad_sw, {Q, B}));
    for_threads(Q, [&] { device::warp_vertices_kernel_backward<T>(gv, gm, m, p, w, j, a, b, c); });
}

template <typename T>
void calc_corners(const RefTree& t, const int64_t* indexer, int64_t Q, void* out) {
    TreeSpec tree = make_tree<T>(t);
    zero<T>(out, Q * 3);
    auto ix = acc32<int64_t, 2>(wrap<int64_t>(indexer, {Q, 4}));
    auto res = acc32<T, 2>(wrap<T>(out, {Q, 3}));
    PackedTreeSpec<T> pt(tree);
    for_threads(Q, [&] { device::calc_corner_kernel<T>(pt, ix, res); });
}

}  // namespace

#define BOTH(call) do { if (is_double) { using T = double; call; } else { using T = float; call; } } while (0)

extern "C" {

int svoxt_ref_sizeof_options(void) { return (int)sizeof(RenderOptions); }
int svoxt_ref_sizeof_tree(void) { return (int)sizeof(RefTree); }

void svoxt_ref_volume_render(const RefTree* t, int is_double, const void* o, const void* d, const void* v, int64_t Q,
                             const RenderOptions* opt, void* out, int64_t cols) {
    BOTH(volume_render<T>(*t, o, d, v, Q, *opt, out, cols));
}
void svoxt_ref_volume_render_backward(const RefTree* t, int is_double, const void* o, const void* d, const void* v, int64_t Q,
                                      const RenderOptions* opt, const void* grad_out, int64_t cols, void* grad) {
    BOTH(volume_render_backward<T>(*t, o, d, v, Q, *opt, grad_out, cols, grad));
}
void svoxt_ref_volume_render_image(const RefTree* t, int is_double, const void* c2w, int64_t rows, float fx, float fy, int w, int h,
                                   const RenderOptions* opt, void* out, int64_t cols) {
    BOTH(volume_render_image<T>(*t, c2w, rows, fx, fy, w, h, *opt, out, cols));
}
void svoxt_ref_volume_render_image_backward(const RefTree* t, int is_double, const void* c2w, int64_t rows, float fx, float fy,
                                            int w, int h, const RenderOptions* opt, const void* grad_out, int64_t cols, void* grad) {
    BOTH(volume_render_image_backward<T>(*t, c2w, rows, fx, fy, w, h, *opt, grad_out, cols, grad));
}
void svoxt_ref_opacity_render(const RefTree* t, int is_double, const void* o, const void* d, const void* v, int64_t Q,
                              const RenderOptions* opt, void* out) {
    BOTH(opacity_render<T>(*t, o, d, v, Q, *opt, out));
}
void svoxt_ref_render_depth(const RefTree* t, int is_double, const void* o, const void* d, const void* v, int64_t Q,
                            const RenderOptions* opt, void* out) {
    BOTH(render_depth<T>(*t, o, d, v, Q, *opt, out));
}
void svoxt_ref_motion_render(const RefTree* t, int is_double, const void* o, const void* d, const void* v, int64_t Q,
                             const RenderOptions* opt, void* out, void* depth, void* hit_point, int64_t* data_idx) {
    BOTH(motion_render<T>(*t, o, d, v, Q, *opt, out, depth, hit_point, data_idx));
}
void svoxt_ref_motion_feature_render(const RefTree* t, int is_double, const void* o, const void* d, const void* v, int64_t Q,
                                     const RenderOptions* opt, void* out) {
    BOTH(motion_feature_render<T>(*t, o, d, v, Q, *opt, out));
}
void svoxt_ref_grid_weight_render(int is_double, const void* sigma, int64_t R, const void* c2w, int64_t rows, float fx, float fy,
                                  int w, int h, const RenderOptions* opt, const void* offset, const void* scaling,
                                  void* grid_weight, void* grid_hit) {
    BOTH(grid_weight_render<T>(sigma, R, c2w, rows, fx, fy, w, h, *opt, offset, scaling, grid_weight, grid_hit));
}
int64_t svoxt_ref_query_vertical(const RefTree* t, int is_double, const void* points, int64_t Q, void* values, int64_t* node_ids,
                                 int64_t* data_ids, int64_t* leaf_node_out, int64_t capacity) {
    int64_t n = 0;
    BOTH(n = query_vertical<T>(*t, points, Q, values, node_ids, data_ids, leaf_node_out, capacity));
    return n;
}
void svoxt_ref_query_vertical_backward(const RefTree* t, int is_double, const void* points, int64_t Q, const void* grad_out,
                                       void* grad) {
    BOTH(query_vertical_backward<T>(*t, points, Q, grad_out, grad));
}
void svoxt_ref_warp_vertices(int is_double, const void* matrices, int64_t J, int64_t D, const void* points, int64_t Q,
                             const void* sw, const int32_t* ji, int64_t B, void* vertices_out, void* matrix_out) {
    BOTH(warp_vertices<T>(matrices, J, D, points, Q, sw, ji, B, vertices_out, matrix_out));
}
void svoxt_ref_warp_vertices_backward(int is_double, const void* matrices, int64_t J, int64_t D, const void* points, int64_t Q,
                                      const void* sw, const int32_t* ji, int64_t B, const void* grad_vertices,
                                      const void* grad_matrix_out, void* grad_points, void* grad_matrices, void* grad_sw) {
    BOTH(warp_vertices_backward<T>(matrices, J, D, points, Q, sw, ji, B, grad_vertices, grad_matrix_out, grad_points,
                                   grad_matrices, grad_sw));
}
void svoxt_ref_calc_corners(const RefTree* t, int is_double, const int64_t* indexer, int64_t Q, void* out) {
    BOTH(calc_corners<T>(*t, indexer, Q, out));
}

}  // extern "C"
