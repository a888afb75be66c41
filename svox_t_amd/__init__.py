"""svox_t_amd -- svox_t's differentiable volume-rendering hot path on AMD
MI355X (gfx950): hand-written HIP kernels behind a C ABI (include/svoxt.h),
with the reference's `N3Tree` / `VolumeRenderer` / autograd surface on top.

    import svox_t_amd as svox_t
    tree = svox_t.N3Tree(...); r = svox_t.VolumeRenderer(tree)
    out = r(features, svox_t.Rays(origins, dirs, viewdirs))

Importing this package loads libsvoxt_hip.so; build it first with
`python svox_t_amd/build.py` (there is no CPU fallback).
"""
from svox_t_amd.helpers import DataFormat, LocalIndex, N3TreeView  # noqa: F401
from svox_t_amd.svox import (InterpStencil, N3Tree, blend_transformation_matrix, get_transformation_matrix,  # noqa: F401
                            interp_rows, warp_vertices)
from svox_t_amd.renderer import NDCConfig, Rays, SEGrad, VolumeRenderer  # noqa: F401
from svox_t_amd.p2v import voxelize  # noqa: F401
from svox_t_amd.gridw import GridWeights, grid_weights  # noqa: F401
from svox_t_amd.quant import quantize_median_cut  # noqa: F401
from svox_t_amd.optim import FeatureAdam, FeatureRMSprop, FeatureSGD, gauss_newton_step_  # noqa: F401
from svox_t_amd.samples import (RaySamples, RowPlan, accumulate, composite, gather_rows, merge_samples,  # noqa: F401
                                quantile_depth, ray_quantile, ray_scan, reduce_rows, sample_geometry, sample_weights, shade_samples,
                                take_samples)

__version__ = "0.1.0"
__all__ = ["N3Tree", "N3TreeView", "VolumeRenderer", "Rays", "NDCConfig",
           "DataFormat", "LocalIndex", "get_transformation_matrix", "warp_vertices",
           "blend_transformation_matrix", "voxelize", "grid_weights", "GridWeights", "quantize_median_cut",
           "FeatureSGD", "FeatureRMSprop", "FeatureAdam", "RaySamples", "sample_weights", "accumulate", "composite",
           "RowPlan", "gather_rows", "reduce_rows", "shade_samples", "ray_scan", "ray_quantile", "quantile_depth",
           "InterpStencil", "interp_rows", "merge_samples", "take_samples", "sample_geometry", "SEGrad",
           "gauss_newton_step_"]
