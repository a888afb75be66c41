"""The per-sample interface: march -> samples -> weights from density -> accumulate along rays.

    samples = renderer.ray_samples(rays, min_sigma=0.0)            # RaySamples: CSR lists of the leaf crossings
    sigma = features[samples.row.long(), -1]                       # any per-sample density, through torch indexing
    w, alpha = sample_weights(samples, sigma)                      # w_k = T_k (1 - exp(-length_k sigma_k)), alpha = 1 - T_end
    out = accumulate(samples, w, values)                           # out[q] = sum_k w_k values_k over ray q's samples
    out, alpha, w = composite(samples, sigma, values)              # the two chained

Every per-sample loss is then a few lines of torch around three HIP operators; a per-leaf statistic is
`torch.zeros(M).index_reduce_(0, samples.row.long(), w, "amax")`.  There is no CPU path.
"""
from __future__ import annotations

import torch
from torch import autograd

from svox_t_amd.helpers import _get_c_extension
from svox_t_amd.renderer import Rays, VolumeRenderer, _rays_spec_from_rays

_C = _get_c_extension()


class RaySamples:
    """The leaf crossings of a ray batch in CSR form, in ray-index order and, within a ray, in march order.

    offsets int64 [Q + 1]   ray q's samples are offsets[q] .. offsets[q + 1] - 1
    ray     int32 [T]       the ray of every sample
    row     int32 [T]       the feature row of the leaf crossed
    depth   float32 [T]     distance at which the ray enters the leaf (the "entry" z of render_depth_moments)
    length  float32 [T]     length of the crossing (+ step_size), in the same units
    """

    def __init__(self, offsets, ray, row, depth, length):
        self.offsets, self.ray, self.row, self.depth, self.length = offsets, ray, row, depth, length
        if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1:
            raise RuntimeError("offsets must be int64 [Q + 1]")
        T = ray.shape[0] if isinstance(ray, torch.Tensor) and ray.dim() == 1 else -1
        for name, x, dt in (("ray", ray, torch.int32), ("row", row, torch.int32), ("depth", depth, torch.float32),
                            ("length", length, torch.float32)):
            if not isinstance(x, torch.Tensor) or x.dtype != dt or tuple(x.shape) != (T,):
                raise RuntimeError(f"{name} must be {str(dt).split('.')[-1]} [T], one entry per sample")

    @property
    def Q(self) -> int:
        return self.offsets.shape[0] - 1

    def __len__(self) -> int:
        return self.ray.shape[0]

    @property
    def counts(self):
        """int64 [Q]: the number of samples of every ray."""
        return self.offsets[1:] - self.offsets[:-1]


def _ray_samples(self, rays: Rays, *, features=None, min_sigma=None, image_shape=None, sort_rays=None) -> RaySamples:
    """The leaf crossings of a ray batch as RaySamples: every crossing of the shared march whose leaf holds a feature
    row, or with `min_sigma` only those whose sigma exceeds it (0.0: the set the backwards walk, sigma > 0).

    :param features: the feature table sigma is read from (default: the tree's own); read only with min_sigma
    :param image_shape, sort_rays: see forward -- they change how the rays are walked, never the lists
    Nothing here is differentiable: the lists are indices and distances of the march.  One host read (the total)."""
    self._require_gpu(True, "ray_samples")
    if features is None:
        features = self.tree.features
    with torch.no_grad():
        spec = self.tree._spec(features.detach())
        rspec = _rays_spec_from_rays(rays, image_shape, sort_rays)
        rspec.need_grad = False
        offsets, row, ray, depth, length, _ = _C.ray_samples(spec, rspec, self._get_options(), min_sigma)
    return RaySamples(offsets, ray, row, depth, length)


VolumeRenderer.ray_samples = _ray_samples


def _require_gpu(what, samples, *tensors):
    if not isinstance(samples, RaySamples):
        raise RuntimeError(f"{what}: samples must be a RaySamples")
    for x in (samples.offsets,) + tensors:
        if x is not None and not x.is_cuda:
            raise RuntimeError(f"{what}: only the GPU (HIP) path exists; the samples and every argument must be on the GPU")


class _SampleWeightsFunction(autograd.Function):
    @staticmethod
    def forward(ctx, sigma, samples):
        sigma = sigma.contiguous()
        w, alpha = _C.sample_weights(samples.offsets, samples.length, sigma)
        ctx.samples = samples
        ctx.save_for_backward(sigma)
        return w, alpha

    @staticmethod
    def backward(ctx, grad_w, grad_alpha):
        if not ctx.needs_input_grad[0]:
            return None, None
        (sigma,) = ctx.saved_tensors
        s = ctx.samples
        gw = None if grad_w is None else grad_w.contiguous()
        ga = None if grad_alpha is None else grad_alpha.contiguous()
        return _C.sample_weights_backward(s.offsets, s.length, sigma, gw, ga), None


class _AccumulateFunction(autograd.Function):
    @staticmethod
    def forward(ctx, w, values, samples):
        w = w.contiguous()
        values = None if values is None else values.contiguous()
        out = _C.sample_accumulate(samples.offsets, w, values)
        ctx.samples = samples
        ctx.has_values = values is not None
        ctx.save_for_backward(*((w,) if values is None else (w, values)))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        w = ctx.saved_tensors[0]
        values = ctx.saved_tensors[1] if ctx.has_values else None
        need_w, need_v = ctx.needs_input_grad[0], ctx.has_values and ctx.needs_input_grad[1]
        if not (need_w or need_v):
            return None, None, None
        s = ctx.samples
        gw, gv = _C.sample_accumulate_backward(s.ray, s.Q, w, values, grad_out.contiguous(), need_w, need_v)
        return gw, gv, None


def sample_weights(samples: RaySamples, sigma):
    """(w float32 [T], alpha float32 [Q]) from a density per sample, differentiable in `sigma`:

        per ray, in list order:  att = exp(-(length * sigma));  w = T * (1 - att);  T *= att;      alpha = 1 - T_end

    A sample with sigma <= 0 gets w = 0, leaves T unchanged and receives no gradient, as the march skips it.  No
    thresholds and no early stop (the convention of the package's backwards).  With sigma = features[samples.row, -1]
    alpha has the bits of opacity_render and of render_depth_moments' third column."""
    if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float32 or sigma.dim() != 1 or \
            not isinstance(samples, RaySamples) or sigma.shape[0] != len(samples):
        raise RuntimeError("sigma must be float32 [T], one entry per sample")
    _require_gpu("sample_weights", samples, sigma)
    return _SampleWeightsFunction.apply(sigma, samples)


def accumulate(samples: RaySamples, w, values=None):
    """out float32 [Q, C]: out[q, c] = sum_k w[k] * values[k, c] over ray q's samples, added in list order; [Q], the plain
    sum of w, without `values`.  Differentiable in `w` and `values`."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 1 or not isinstance(samples, RaySamples) \
            or w.shape[0] != len(samples):
        raise RuntimeError("w must be float32 [T], one entry per sample")
    if values is not None and (not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2
                               or values.shape[0] != len(samples) or values.shape[1] < 1):
        raise RuntimeError("values must be float32 [T, C], one row per sample, C >= 1")
    _require_gpu("accumulate", samples, w, values)
    return _AccumulateFunction.apply(w, values, samples)


def composite(samples: RaySamples, sigma, values=None):
    """(out, alpha, w): accumulate(samples, w, values) with (w, alpha) = sample_weights(samples, sigma)."""
    w, alpha = sample_weights(samples, sigma)
    return accumulate(samples, w, values), alpha, w
