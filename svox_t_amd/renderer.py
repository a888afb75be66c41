"""VolumeRenderer: differentiable ray-batch volume rendering of an N3Tree on
MI355X, with the reference's module / autograd.Function surface
(svox_t/renderer.py:39-77, :118-138, :162-205, :207-308, :377-382, :397-439).

    renderer = VolumeRenderer(tree)                       # step_size=1e-3, white background
    out = renderer(features, Rays(origins, dirs, viewdirs))   # [Q, C+1] = colour..., alpha
    out.sum().backward()                                  # d/d features via the HIP backward

Every entry runs the hand-written HIP kernels through `svox_t_amd.csrc`; like
the reference (whose non-CUDA branches are `assert False`) there is no CPU
path: `cuda=False`, or a tree that is not on a GPU, raises.
"""
from __future__ import annotations

from collections import namedtuple
from warnings import warn

import os

import torch
from torch import autograd, nn

from svox_t_amd.helpers import DataFormat, _get_c_extension

NDCConfig = namedtuple("NDCConfig", ["width", "height", "focal"])
Rays = namedtuple("Rays", ["origins", "dirs", "viewdirs"])
SEGrad = namedtuple("SEGrad", ["out", "loss", "grad", "hessdiag"])           # what VolumeRenderer.se_grad returns

_C = _get_c_extension()


def _rays_spec_from_rays(rays, image_shape=None, sort_rays=None):
    """svox_t/renderer.py:44-49, plus two optional hints for the operator layer (svox_t_amd.csrc):
    the batch is a row-major H x W image (walked in 8x8 tiles), and whether to render a batch that
    is not an image in svoxt_ray_order's order (None: decided by its size)."""
    spec = _C.RaysSpec()
    spec.origins = rays.origins
    spec.dirs = rays.dirs
    spec.vdirs = rays.viewdirs
    if image_shape is not None:
        spec.image_height, spec.image_width = int(image_shape[0]), int(image_shape[1])
    spec.sort = None if sort_rays is None else bool(sort_rays)
    return spec


def _will_differentiate(features) -> bool:
    """Can a backward follow this call?  Known here, outside autograd.Function.apply."""
    return bool(torch.is_grad_enabled() and features.requires_grad)


def _make_camera_spec(c2w, width, height, fx, fy):
    """svox_t/renderer.py:51-58."""
    spec = _C.CameraSpec()
    spec.c2w = c2w
    spec.width = width
    spec.height = height
    spec.fx = fx
    spec.fy = fy
    return spec


def pinhole_rays(c2w, width, height, fx, fy, ndc: NDCConfig = None, near=1.0):
    """Row-major [H*W, 3] float32 (origins, dirs, viewdirs) of a pinhole camera.

    cam2world_ray (svox_t/csrc/rt_kernel.cu:1153-1166), with its mixed
    float/double arithmetic: x = (ix - 0.5 W)/fx and y = -(iy - 0.5 H)/fy are
    formed in double and rounded to float, z = sqrtf(x*x + y*y + 1.0).  With an
    NDC config, origins and dirs are then warped as maybe_world2ndc (:1170-1190)
    does; viewdirs keep the un-warped directions.
    """
    dev = c2w.device
    ix = torch.arange(width, device=dev, dtype=torch.float64)
    iy = torch.arange(height, device=dev, dtype=torch.float64)
    x = ((ix - 0.5 * width) / float(torch.tensor(fx, dtype=torch.float32))).float()
    y = (-(iy - 0.5 * height) / float(torch.tensor(fy, dtype=torch.float32))).float()
    X = x[None, :].expand(height, width).reshape(-1)
    Y = y[:, None].expand(height, width).reshape(-1)
    Z = torch.sqrt(((X * X + Y * Y).double() + 1.0).float())
    X, Y, Z = X / Z, Y / Z, -1.0 / Z
    R = c2w[:3, :3]
    dirs = torch.stack([(R[i, 0] * X + R[i, 1] * Y) + R[i, 2] * Z for i in range(3)], dim=-1).contiguous()
    origins = c2w[:3, 3].expand(width * height, 3).contiguous()
    vdirs = dirs
    if ndc is not None and ndc.width >= 0:
        t = -(near + origins[:, 2]) / dirs[:, 2]
        cen = origins + t[:, None] * dirs
        sx, sy = (2 * ndc.focal) / ndc.width, (2 * ndc.focal) / ndc.height
        d0 = -sx * (dirs[:, 0] / dirs[:, 2] - cen[:, 0] / cen[:, 2])
        d1 = -sy * (dirs[:, 1] / dirs[:, 2] - cen[:, 1] / cen[:, 2])
        d2 = -2 * near / cen[:, 2]
        o0 = -sx * (cen[:, 0] / cen[:, 2])
        o1 = -sy * (cen[:, 1] / cen[:, 2])
        o2 = 1 + 2 * near / cen[:, 2]
        nd = torch.stack([d0, d1, d2], -1)
        dirs = (nd / torch.norm(nd, dim=-1, keepdim=True)).contiguous()
        origins = torch.stack([o0, o1, o2], -1).contiguous()
        vdirs = vdirs.clone()
    return origins, dirs, vdirs


class _VolumeRenderFunction(autograd.Function):
    """svox_t/renderer.py:60-77, as it stands there: argument order (data, tree_spec, rays_spec,
    opt), the specs kept on the ctx (not save_for_backward), a gradient for argument 0 only.
    What makes the pair fast -- sample lists recorded by the forward and replayed by the backward,
    coherent ray order -- happens below these two calls (svox_t_amd.csrc, _Plan), so the
    reference's own function gets it too.  (Whether a backward can follow is said by the caller of
    apply() on the spec, `need_grad`: inside an autograd.Function grad mode is off and
    ctx.needs_input_grad ignores torch.no_grad(); without the hint the feature table's
    requires_grad decides.)"""

    @staticmethod
    def forward(ctx, data, tree, rays, opt):
        out = _C.volume_render(tree, rays, opt)
        ctx.tree = tree
        ctx.rays = rays
        ctx.opt = opt
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.needs_input_grad[0]:
            return _C.volume_render_backward(ctx.tree, ctx.rays, ctx.opt, grad_out.contiguous()), None, None, None
        return None, None, None, None


class _VolumeRenderImageFunction(autograd.Function):
    """svox_t/renderer.py:79-94."""

    @staticmethod
    def forward(ctx, data, tree, cam, opt):
        out = _C.volume_render_image(tree, cam, opt)
        ctx.tree = tree
        ctx.cam = cam
        ctx.opt = opt
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.needs_input_grad[0]:
            return _C.volume_render_image_backward(ctx.tree, ctx.cam, ctx.opt, grad_out.contiguous()), \
                None, None, None
        return None, None, None, None


class _MotionFeatureRenderFunction(autograd.Function):
    """svox_t/renderer.py:96-116: differentiable wrt joint_features (argument 0)."""

    @staticmethod
    def forward(ctx, data, tree, rays, opt):
        out = _C.motion_feature_render(tree, rays, opt)
        ctx.tree = tree
        ctx.rays = rays
        ctx.opt = opt
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.needs_input_grad[0]:
            return _C.motion_feature_render_backward(ctx.tree, ctx.rays, ctx.opt, grad_out.contiguous()), \
                None, None, None
        return None, None, None, None


class _OpacityRenderFunction(autograd.Function):
    """svox_t/renderer.py:118-138."""

    @staticmethod
    def forward(ctx, data, tree, rays, opt):
        out = _C.opacity_render(tree, rays, opt)
        ctx.tree = tree
        ctx.rays = rays
        ctx.opt = opt
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.needs_input_grad[0]:
            return _C.opacity_render_backward(ctx.tree, ctx.rays, ctx.opt, grad_out.contiguous()), None, None, None
        return None, None, None, None


class _DeterministicRenderFunction(autograd.Function):
    """Not in the reference: volume_render / opacity_render (`fwd`, run exactly as the default route runs it) whose
    backward is the deterministic one -- contributions summed over the row plan in a fixed order, no float atomics
    (_C.volume_render_backward_rows).  That this route was asked for travels on the ctx."""

    @staticmethod
    def forward(ctx, data, tree, rays, opt, fwd):
        out = fwd(tree, rays, opt)
        ctx.tree = tree
        ctx.rays = rays
        ctx.opt = opt
        ctx.deterministic = True
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad = None
        if ctx.needs_input_grad[0]:
            grad = _C.volume_render_backward_rows(ctx.tree, ctx.rays, ctx.opt, grad_out.contiguous())
        return grad, None, None, None, None


def _refuse_deterministic(what, why):
    raise RuntimeError(f"VolumeRenderer.{what}: deterministic=True is not served: {why} "
                       "(forward and opacity_render take it; see INTEGRATION.md)")


class _RaySweepFunction(autograd.Function):
    """Not in the reference: the per-ray operators that are differentiable wrt the feature table's sigma column --
    depth moments (m1, m2, alpha) and distortion (distortion loss, alpha).  `fwd` / `bwd`: the operator's pair of _C,
    `lead`: what they take behind their common arguments."""

    @staticmethod
    def forward(ctx, data, tree, rays, opt, fwd, bwd, *lead):
        out = fwd(tree, rays, opt, *lead)
        ctx.tree = tree
        ctx.rays = rays
        ctx.opt = opt
        ctx.bwd = bwd
        ctx.lead = lead
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad = None
        if ctx.needs_input_grad[0]:
            grad = ctx.bwd(ctx.tree, ctx.rays, ctx.opt, grad_out.contiguous(), *ctx.lead)
        return (grad,) + (None,) * (5 + len(ctx.lead))


class VolumeRenderer(nn.Module):
    def __init__(self, tree, step_size: float = 1e-3, background_brightness: float = 1.0,
                 ndc: NDCConfig = None, min_comp=0, max_comp=-1):
        """
        :param tree: N3Tree to render
        :param step_size: epsilon added to every leaf-crossing step
        :param background_brightness: 1.0 = white
        :param ndc: NDCConfig or None; only used by image-mode rendering, which
                    is outside this package's scope -- stored and forwarded in
                    RenderOptions for interface parity
        :param min_comp, max_comp: SH/SG component range; -1 = last
        """
        super().__init__()
        self.tree = tree
        self.step_size = step_size
        self.background_brightness = background_brightness
        self.ndc_config = ndc
        self.min_comp = min_comp
        self.max_comp = max_comp
        if isinstance(tree.data_format, DataFormat):
            self.data_format = tree.data_format
        else:
            warn("N3Tree without data_format, inferring from data_dim")
            ddim = tree.data_dim
            self.data_format = DataFormat("") if ddim == 4 else DataFormat(f"SH{(ddim - 1) // 3}")
        if self.max_comp < 0:
            self.max_comp += self.data_format.basis_dim
        self.tree._weight_accum = None

    def _require_gpu(self, cuda, what):
        if not cuda or not self.tree.data.is_cuda:
            raise RuntimeError(f"VolumeRenderer.{what}: only the GPU (HIP) path exists "
                               "(the reference asserts on its non-CUDA branch too)")

    def forward(self, features, rays: Rays, transformation_matrices=None, cuda=True, fast=False,
                image_shape=None, sort_rays=None, deterministic=False):
        """Render a ray batch; differentiable wrt `features`.

        :param features: float32 [M, data_dim] leaf feature table (on the GPU)
        :param rays: Rays(origins [Q,3], dirs [Q,3], viewdirs [Q,3]) in world space
        :param fast: sigma_thresh = stop_thresh = 1e-2 (early termination)
        :param image_shape: optional (H, W) (not in the reference): states that the
               rays are the row-major pixels of an H x W image, which lets the kernels
               walk them in 8x8 tiles; results are unchanged
        :param sort_rays: (not in the reference) render a batch that is not an image in the
               order of its rays' entry points into the tree's cube, so that the 64 rays of
               a wavefront cross the same leaves; every ray's result is unchanged and comes
               back at the ray's own position.  None: from 16 384 rays on (svox_t_amd.csrc
               SORT_RAYS; SVOXT_SORT_RAYS=0/1 overrides)
        :param deterministic: (not in the reference) True: the gradient with respect to `features` is
               bit-identical from run to run and across sort_rays / image_shape / fast / list and pool
               settings: every sample's contribution is summed per table entry in a fixed order over
               the row plan instead of with float atomics (slower).  The output is the
               same bits either way.  Not with transformation_matrices
        :return: [Q, C+1]: C colour/feature channels then accumulated alpha
        """
        self._require_gpu(cuda, "forward")
        rspec = _rays_spec_from_rays(rays, image_shape, sort_rays)
        if deterministic:
            if transformation_matrices is not None:
                _refuse_deterministic("forward", "transformation_matrices are not served by the deterministic backward")
            rspec.need_grad = False          # (its backward marches itself: the forward records nothing for it)
            return _DeterministicRenderFunction.apply(features, self.tree._spec(features), rspec, self._get_options(fast),
                                                      _C.volume_render)
        rspec.need_grad = _will_differentiate(features)
        return _VolumeRenderFunction.apply(
            features,
            self.tree._spec(features, transformation_matrices=transformation_matrices),
            rspec,
            self._get_options(fast))

    def render_persp(self, features, c2w, width=800, height=800, fx=1111.111, fy=None,
                     cuda=True, fast=False, deterministic=False):
        """Render a perspective image; differentiable wrt `features`.

        Same signature and route as the reference (svox_t/renderer.py:310-366:
        _VolumeRenderImageFunction -> volume_render_image with a CameraSpec), whose
        CUDA side cannot run (it allocates and dispatches on the int32 index
        tensor, svox_t/csrc/rt_kernel.cu:1390-1393).  The pinhole rays of
        `cam2world_ray` (:1153-1166) -- and the NDC warp of `maybe_world2ndc`
        (:1170-1190) when the renderer has an `ndc` config -- are generated inside
        the HIP kernels, which walk the image in 8x8 pixel tiles: no ray tensors
        exist in memory.

        :param c2w: (3, 4) or (4, 4) camera-to-world matrix (OpenGL axes: -z forward)
        :return: (height, width, C+1)
        """
        self._require_gpu(cuda, "render_persp")
        if deterministic:
            _refuse_deterministic("render_persp", "camera batches keep the default backward")
        if fy is None:
            fy = fx
        c2w = c2w.to(device=self.tree.data.device, dtype=torch.float32).contiguous()
        cam = _make_camera_spec(c2w, width, height, fx, fy)
        cam.need_grad = _will_differentiate(features)
        return _VolumeRenderImageFunction.apply(features, self.tree._spec(features), cam, self._get_options(fast))

    def motion_render(self, features, rays: Rays, cuda=True, fast=False, image_shape=None, deterministic=False):
        """First sample with sigma > sigma_thresh per ray (svox_t/renderer.py:367-375):
        (distance to each joint position in tree.extra_data [Q, J], depth [Q, 1],
        hit_point [Q, 3], feature row index [Q, 1] int64); zeros where nothing is hit."""
        if deterministic:
            _refuse_deterministic("motion_render", "the motion operators keep the default backward")
        assert self.tree.extra_data is not None, "Need extra data to store skeleton position."
        self._require_gpu(cuda, "motion_render")
        return _C.motion_render(self.tree._spec(features), _rays_spec_from_rays(rays, image_shape),
                                self._get_options(fast))

    def motion_feature_render(self, features, joint_features, skinning_weights, joint_index, rays: Rays,
                              cuda=True, fast=False, image_shape=None, deterministic=False):
        """Composite, per ray, sigmoid(sum_j skinning_weights[row, j] * joint_features[joint_index[row, j]])
        over the samples (svox_t/renderer.py:384-396); [Q, joint_features.shape[1]],
        differentiable wrt `joint_features`."""
        self._require_gpu(cuda, "motion_feature_render")
        if deterministic:
            _refuse_deterministic("motion_feature_render", "the motion operators keep the default backward")
        return _MotionFeatureRenderFunction.apply(
            joint_features, self.tree._spec(features, joint_features, skinning_weights, joint_index),
            _rays_spec_from_rays(rays, image_shape), self._get_options(fast))

    def render_depth(self, features, rays: Rays, cuda=True, fast=False, image_shape=None):
        """[Q, 1] distance to the first sample with sigma > sigma_thresh (0 if none)."""
        self._require_gpu(cuda, "render_depth")
        return _C.render_depth(self.tree._spec(features), _rays_spec_from_rays(rays, image_shape),
                               self._get_options(fast))

    def opacity_render(self, features, rays: Rays, cuda=True, fast=False, image_shape=None, sort_rays=None,
                       deterministic=False):
        """[Q, 1] accumulated alpha only; differentiable wrt `features` (sort_rays, deterministic: see forward)."""
        self._require_gpu(cuda, "opacity_render")
        rspec = _rays_spec_from_rays(rays, image_shape, sort_rays)
        if deterministic:
            rspec.need_grad = False
            return _DeterministicRenderFunction.apply(features, self.tree._spec(features), rspec, self._get_options(fast),
                                                      _C.opacity_render)
        rspec.need_grad = _will_differentiate(features)
        return _OpacityRenderFunction.apply(features, self.tree._spec(features), rspec, self._get_options(fast))

    def render_depth_moments(self, features, rays: Rays, *, at="entry", cuda=True, fast=False, image_shape=None,
                             sort_rays=None):
        """[Q, 3] = (m1, m2, alpha): the first two moments of the compositing weights over distance and the
        accumulated alpha, m1 = sum_k w_k z_k, m2 = sum_k w_k z_k^2, alpha = 1 - T_end with w_k = T_k (1 - att_k);
        differentiable wrt `features` (its sigma column).  Expected depth is m1 / alpha (render_expected_depth), the
        depth variance m2 / alpha - (m1 / alpha)^2.

        :param at: "entry": z_k is the distance at which the ray enters the sample's leaf -- the quantity render_depth
               reports; "mid": the middle of the leaf crossing
        :param fast: sigma_thresh = stop_thresh = 1e-2 in the forward; the gradient is the one at thresholds 0
               (the reference's convention for its backwards)
        :param image_shape, sort_rays: see forward

        A ray that misses the volume gives (0, 0, 0); the background adds nothing (it has no depth).  With an `ndc`
        config z is a distance in the space the march runs in (NDC space), as render_depth's is."""
        self._require_gpu(cuda, "render_depth_moments")
        if at not in ("entry", "mid"):
            raise ValueError(f"at must be 'entry' or 'mid', not {at!r}")
        rspec = _rays_spec_from_rays(rays, image_shape, sort_rays)
        rspec.need_grad = _will_differentiate(features)
        return _RaySweepFunction.apply(features, self.tree._spec(features), rspec, self._get_options(fast),
                                       _C.depth_moments, _C.depth_moments_backward, 0 if at == "entry" else 1)

    def render_expected_depth(self, features, rays: Rays, *, at="entry", cuda=True, fast=False, image_shape=None,
                              sort_rays=None, eps=1e-10):
        """[Q, 1] expected depth m1 / (alpha + eps) of render_depth_moments, in torch ops on top of it: autograd chains
        through (0 where the ray meets nothing)."""
        m = self.render_depth_moments(features, rays, at=at, cuda=cuda, fast=fast, image_shape=image_shape,
                                      sort_rays=sort_rays)
        return m[:, 0:1] / (m[:, 2:3] + eps)

    def render_distortion(self, features, rays: Rays, *, cuda=True, fast=False, image_shape=None, sort_rays=None):
        """[Q, 2] = (L, alpha): the distortion loss of mip-NeRF 360 per ray and the accumulated alpha,

            L = sum_i sum_j w_i w_j |s_i - s_j| + (1/3) sum_i w_i^2 d_i        w_k = T_k (1 - att_k)

        over the ray's leaf crossings: s_k is the distance to the middle of crossing k, d_k its length.  Leaves are
        piecewise constant, so the interval form is exact.  Differentiable wrt `features` (its sigma column).

        :param fast: sigma_thresh = stop_thresh = 1e-2 in the forward; the gradient is the one at thresholds 0
               (the reference's convention for its backwards)
        :param image_shape, sort_rays: see forward

        A ray that misses the volume gives (0, 0); the background adds nothing.  s is not normalised to the ray's
        near / far span: distances are those of render_depth_moments(at="mid")."""
        self._require_gpu(cuda, "render_distortion")
        rspec = _rays_spec_from_rays(rays, image_shape, sort_rays)
        rspec.need_grad = _will_differentiate(features)
        return _RaySweepFunction.apply(features, self.tree._spec(features), rspec, self._get_options(fast),
                                       _C.distortion, _C.distortion_backward)

    def distortion_loss(self, features, rays: Rays, *, reduction="mean", cuda=True, fast=False, image_shape=None,
                        sort_rays=None):
        """The distortion column of render_distortion reduced over the rays, in torch ops on top of it: "mean" and
        "sum" give a scalar, "none" the [Q] per-ray values; autograd chains through."""
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction must be 'mean', 'sum' or 'none', not {reduction!r}")
        per_ray = self.render_distortion(features, rays, cuda=cuda, fast=fast, image_shape=image_shape,
                                         sort_rays=sort_rays)[:, 0]
        if reduction == "mean":
            return per_ray.mean()
        return per_ray.sum() if reduction == "sum" else per_ray

    def grad_hess(self, features, rays: Rays, grad_out, curvature, *, fast=False, cuda=True, image_shape=None, sort_rays=None,
                  transformation_matrices=None):
        """(grad, hessdiag), both float32 [M, data_dim], for a per-pixel separable loss on forward()'s output: `grad_out`
        [Q, C+1] is the loss's first derivative in each output, `curvature` [Q, C+1] its second.

        grad is the gradient forward(deterministic=True) + backward(grad_out) gives, with its bits.  hessdiag is the
        diagonal of the Gauss-Newton Hessian J^T diag(curvature) J, the squares taken PER SAMPLE:

            hessdiag[m, j] = sum over the samples k naming row m and the outputs c of curvature[ray(k), c] * J(k, c, j)^2

        with J(k, c, j) the derivative of out[ray(k), c] in entry j of row m through sample k alone.  That is the exact
        diagonal whenever no ray names a feature row twice; where rows are shared by several leaves (after refine, merge,
        quantize) it is the svox family's approximation: a ray's samples on one row add their squares, not the square
        of their sum.  One march, one row plan and one shade serve both tables; no float atomic, the same bits in every
        run and whatever sort_rays / image_shape / fast say (the sample set is the backward's: sigma > 0, thresholds 0).

        A plain function: no autograd node is made and `features.grad` is not touched.  Not with
        transformation_matrices, camera-mode or NDC rays (forward(deterministic=True)'s scope)."""
        if transformation_matrices is not None:
            _refuse_deterministic("grad_hess", "transformation_matrices are not served by the deterministic backward")
        if self.ndc_config is not None and self.ndc_config.width >= 0:
            _refuse_deterministic("grad_hess", "NDC rays keep the default backward")
        if not all(isinstance(getattr(rays, n, None), torch.Tensor) for n in ("origins", "dirs", "viewdirs")):
            _refuse_deterministic("grad_hess", "camera batches keep the default backward: pass Rays(origins, dirs, viewdirs)")
        if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2:
            raise RuntimeError("grad_hess: features must be a float32 [M, data_dim] tensor")
        for name, t in (("grad_out", grad_out), ("curvature", curvature)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rays.origins.shape[0]:
                raise RuntimeError(f"grad_hess: {name} must be float32 [Q, C+1] with Q = {rays.origins.shape[0]} rays")
        self._require_gpu(cuda, "grad_hess")
        rspec = _rays_spec_from_rays(rays, image_shape, sort_rays)
        rspec.need_grad = False
        with torch.no_grad():
            return _C._extras.volume_render_hess_rows(self.tree._spec(features.detach()), rspec, self._get_options(fast),
                                                      grad_out.contiguous(), curvature.contiguous())

    def se_grad(self, features, rays: Rays, colors, *, weights=None, reduction="mean", fast=False, cuda=True,
                image_shape=None, sort_rays=None, transformation_matrices=None):
        """The svox family's VolumeRenderer.se_grad: render, and return SEGrad(out, loss, grad, hessdiag) for the
        weighted squared error against `colors` -- what a damped Newton step on the leaf table needs
        (svox_t_amd.gauss_newton_step_: p -= lr * grad / (hessdiag + damping)).

        :param colors: float32 [Q, C] target colours, or [Q, C+1] to supervise the alpha column as well
        :param weights: float32 [Q] per-ray weights, or None (ones)
        :param reduction: "mean": the loss is divided by colors.numel(); "sum": it is not
        :return: out [Q, C+1]: forward()'s output with its bits (one default-route forward produces it);
                 loss: sum_q weights[q] * sum_c (out - colors)^2 * scale, scale = 1 / colors.numel() or 1;
                 grad [M, data_dim]: d loss / d features, the deterministic backward's bits for
                 grad_out[q, c] = (out[q, c] - colors[q, c]) * coef[q], coef = (2 * scale) * weights;
                 hessdiag [M, data_dim]: grad_hess's diagonal for curvature[q, c] = coef[q] (see there: exact where no
                 ray names a row twice, per-sample squares where rows are shared).
        Both are zero in the alpha column when `colors` has C columns.  Nothing here makes an autograd node.  Refused
        like forward(deterministic=True): transformation_matrices, camera-mode and NDC rays, cuda=False."""
        if transformation_matrices is not None:
            _refuse_deterministic("se_grad", "transformation_matrices are not served by the deterministic backward")
        if self.ndc_config is not None and self.ndc_config.width >= 0:
            _refuse_deterministic("se_grad", "NDC rays keep the default backward")
        if not all(isinstance(getattr(rays, n, None), torch.Tensor) for n in ("origins", "dirs", "viewdirs")):
            _refuse_deterministic("se_grad", "camera batches keep the default backward: pass Rays(origins, dirs, viewdirs)")
        if reduction not in ("mean", "sum"):
            raise ValueError(f"reduction must be 'mean' or 'sum', not {reduction!r}")
        if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2:
            raise RuntimeError("se_grad: features must be a float32 [M, data_dim] tensor")
        opt = self._get_options(fast)
        cols = _C.get_out_data_dim(opt, features.shape[1])
        Q = rays.origins.shape[0]
        if not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32 or colors.dim() != 2 or colors.shape[0] != Q \
                or colors.shape[1] not in (cols - 1, cols) or colors.device != features.device:
            raise RuntimeError(f"se_grad: colors must be float32 [Q, {cols - 1}] (or [Q, {cols}] with alpha) with Q = {Q} rays, "
                               "on the device of the features")
        if weights is not None and (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32
                                    or tuple(weights.shape) != (Q,) or weights.device != features.device):
            raise RuntimeError(f"se_grad: weights must be float32 [Q] with Q = {Q} rays, on the device of the features, or None")
        self._require_gpu(cuda, "se_grad")
        with torch.no_grad():
            f = features.detach()
            rspec = _rays_spec_from_rays(rays, image_shape, sort_rays)
            rspec.need_grad = False
            spec = self.tree._spec(f)
            out = _C.volume_render(spec, rspec, opt)
            nc = colors.shape[1]
            scale = 1.0 / colors.numel() if (reduction == "mean" and colors.numel() > 0) else 1.0
            w = torch.ones((Q,), dtype=torch.float32, device=f.device) if weights is None else weights
            coef = (2.0 * scale) * w
            resid = out[:, :nc] - colors
            loss = ((resid * resid).sum(dim=1) * w).sum() * scale
            grad_out = torch.zeros_like(out)
            curvature = torch.zeros_like(out)
            grad_out[:, :nc] = resid * coef[:, None]
            curvature[:, :nc] = coef[:, None]
            grad, hess = _C._extras.volume_render_hess_rows(spec, rspec, opt, grad_out, curvature)
        return SEGrad(out, loss, grad, hess)

    def _get_options(self, fast=False):
        """RenderOptions for the operator boundary (svox_t/renderer.py:408-439)."""
        opts = _C.RenderOptions()
        opts.step_size = self.step_size
        opts.background_brightness = self.background_brightness
        opts.format = self.data_format.format
        opts.basis_dim = self.data_format.basis_dim
        opts.min_comp = self.min_comp
        opts.max_comp = self.max_comp
        if self.ndc_config is not None:
            opts.ndc_width = self.ndc_config.width
            opts.ndc_height = self.ndc_config.height
            opts.ndc_focal = self.ndc_config.focal
        else:
            opts.ndc_width = -1
        thresh = 1e-2 if fast else 0.0
        opts.sigma_thresh = getattr(self, "sigma_thresh", thresh)
        opts.stop_thresh = getattr(self, "stop_thresh", thresh)
        return opts
