"""grid_weights: the step between `voxelize` and a sparse tree -- march training views through a dense density volume
and keep, per cell, the largest compositing weight any ray gave it and how many samples landed in it (the reference's
grid_weight_render, svox_t/csrc/rt_kernel.cu:1240-1344, which takes one camera per call and zeroes its outputs).

    vol = svox.voxelize(points, feats, corner, size, n, kernel_radius, conv_radius)        # [n, n, n, 1]
    gw = svox.grid_weights(vol, cameras=c2w, fx=f, fy=f, width=W, height=H, radius=r, center=c)
    cells = (gw.weight[..., 0] > thr).nonzero()                                            # cells worth a leaf

The maximum and the count do not depend on the order rays arrive in: the result is bit-identical from run to run
(INTEGRATION.md D).  No autograd, as in the reference: inputs that require a gradient are read detached.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from svox_t_amd import csrc as _C


class GridWeights(NamedTuple):
    weight: torch.Tensor        # float32, shape of sigma: max over rays of T (1 - exp(-delta_t delta_scale sigma))
    hits: torch.Tensor          # float32, shape of sigma: samples taken in the cell with sigma > sigma_thresh


def _vec3(v, name, device):
    if isinstance(v, torch.Tensor):
        if v.numel() not in (1, 3):
            raise RuntimeError(f"{name} must hold 1 or 3 numbers")
        return v.detach().to(device=device, dtype=torch.float32).reshape(-1).expand(3)
    v = [float(v)] * 3 if isinstance(v, (int, float)) else [float(c) for c in v]
    if len(v) != 3:
        raise RuntimeError(f"{name} must hold 1 or 3 numbers")
    return torch.tensor(v, dtype=torch.float32, device=device)


def grid_weights(sigma, *, cameras=None, fx=None, fy=None, width=None, height=None, rays=None, radius=None, center=None,
                 offset=None, scaling=None, step_size=1e-3, sigma_thresh=0.0, ndc=None, out=None) -> GridWeights:
    """Per cell of the dense float32 volume `sigma` ([R, R, R] or the [R, R, R, 1] `voxelize` returns, any R >= 1):
    the largest compositing weight over all rays and the number of samples, as GridWeights(weight, hits).

    Rays, exactly one of:
      cameras   float32 [V, 3, 4] / [V, 4, 4] (or one matrix) with fx, fy (fy defaults to fx), width, height: every pixel
                of V pinhole views, generated in the kernel, one launch for all of them;
      rays      (origins, dirs), float32 [Q, 3] each (a `Rays` works: its viewdirs are not read).
    World -> unit cube, p' = offset + scaling * p, one of: radius (and center, default 0.5) as N3Tree takes them
    (offset = 0.5 (1 - center / radius), scaling = 0.5 / radius); offset and scaling; neither = the unit cube itself.
    ndc: an NDCConfig (cameras only).  out = (weight, hits) from an earlier call: updated in place and returned, so a
    view set too large for one call can be streamed (max and count compose)."""
    if not isinstance(sigma, torch.Tensor):
        raise RuntimeError("sigma must be a tensor")
    sigma = sigma.detach()
    if (cameras is None) == (rays is None):
        raise RuntimeError("exactly one of cameras / rays must be given")
    if (radius is not None or center is not None) and (offset is not None or scaling is not None):
        raise RuntimeError("give radius / center or offset / scaling, not both")
    dev = sigma.device
    if offset is not None or scaling is not None:
        if offset is None or scaling is None:
            raise RuntimeError("offset and scaling go together")
        offset, scaling = _vec3(offset, "offset", dev).contiguous(), _vec3(scaling, "scaling", dev).contiguous()
    else:
        r = _vec3(0.5 if radius is None else radius, "radius", dev)
        c = _vec3(0.5 if center is None else center, "center", dev)
        offset, scaling = (0.5 * (1.0 - c / r)).contiguous(), (0.5 / r).contiguous()
    opt = _C.RenderOptions()
    opt.step_size, opt.sigma_thresh = float(step_size), float(sigma_thresh)
    opt.ndc_width = -1
    if cameras is not None:
        if fx is None or width is None or height is None:
            raise RuntimeError("cameras need fx, width and height")
        if not isinstance(cameras, torch.Tensor):
            raise RuntimeError("cameras must be a tensor")
        spec = _C.CameraSpec()
        spec.c2w = cameras.detach()
        spec.fx, spec.fy = float(fx), float(fx if fy is None else fy)
        spec.width, spec.height = int(width), int(height)
        if ndc is not None:
            opt.ndc_width, opt.ndc_height, opt.ndc_focal = int(ndc.width), int(ndc.height), float(ndc.focal)
    else:
        if ndc is not None:
            raise RuntimeError("ndc goes with cameras: a ray batch is marched as given")
        if not isinstance(rays, (tuple, list)) or len(rays) < 2:
            raise RuntimeError("rays must be (origins, dirs)")
        spec = _C.RaysSpec()
        spec.origins, spec.dirs = rays[0], rays[1]
        if isinstance(spec.origins, torch.Tensor) and isinstance(spec.dirs, torch.Tensor):
            spec.origins, spec.dirs = spec.origins.detach(), spec.dirs.detach()
    weight, hits = _C.grid_weights(sigma, spec, opt, offset, scaling, out=out)
    return GridWeights(weight, hits)
