"""voxelize: the differentiable Gaussian splat of per-point density into a dense [n, n, n, 1] grid
(the reference's svox_t/p2v.py:33-54, kernels svox_t/csrc/p2v_kernel.cu:104-286).

Same signature and the same (point, voxel) pairs as the reference.  Where it differs:
  - the forward is bit-identical from run to run (the reference adds with float atomics);
  - each gradient is computed if and only if its input requires one (the reference computes none unless
    `points` requires one, p2v.py:47);
  - the feature gradient goes to column F-1, the column the forward reads; the other columns are 0 (the
    reference writes column 0, p2v_kernel.cu:203 -- for F = 1 the two agree);
  - float32 only (other dtypes raise RuntimeError), bad arguments raise RuntimeError, and non-finite points
    contribute nothing and get zero gradient (undefined in the reference).
`volume_corner` and `volume_size` (tensors or sequences of 3 numbers) reach the library as host floats: CUDA tensors
are read back, which synchronises.
"""
from __future__ import annotations

import torch
from torch import autograd

from svox_t_amd import csrc as _C


class _VoxelizationFunction(autograd.Function):
    @staticmethod
    def forward(ctx, points, point_features, volume_corner, volume_size, n_voxels, kernel_radius, conv_radius):
        voxels, order = _C.p2v_order(points, point_features, volume_corner, volume_size, n_voxels, kernel_radius,
                                     conv_radius)
        ctx.args = (volume_corner, volume_size, n_voxels, kernel_radius, conv_radius)
        ctx.save_for_backward(points, point_features, order)
        return voxels

    @staticmethod
    def backward(ctx, grad_output):
        need_points, need_features = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_points or need_features):
            return None, None, None, None, None, None, None
        points, point_features, order = ctx.saved_tensors
        points_grad, features_grad = _C.p2v_backward(grad_output, points, point_features, *ctx.args, order=order,
                                                     need_points_grad=need_points,
                                                     need_features_grad=need_features)
        return points_grad, features_grad, None, None, None, None, None


def voxelize(points, point_features, volume_corner, volume_size, n_voxels, kernel_radius, conv_radius):
    """Splat point_features[:, F-1] of the points [P, 3] into a float32 [n_voxels]^3 x 1 volume on the points' device:
    voxel (i, j, k) at volume_corner + (i, j, k) * volume_size / (n_voxels - 1) gets
    sum exp(-r^2 / (2 kernel_radius^2)) * feature over the points within r <= conv_radius of it."""
    if not (torch.is_grad_enabled() and (points.requires_grad or point_features.requires_grad)):
        # no graph to record (torch.no_grad(), or no input needs a gradient): nothing is saved
        return _C.p2v(points, point_features, volume_corner, volume_size, n_voxels, kernel_radius, conv_radius)
    return _VoxelizationFunction.apply(points, point_features, volume_corner, volume_size, n_voxels, kernel_radius,
                                       conv_radius)
