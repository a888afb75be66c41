"""quantize_median_cut: median-cut palette quantisation of a feature table on the GPU (csrc/svoxt_quant.hip)."""
from __future__ import annotations

from svox_t_amd.helpers import _get_c_extension

_C = _get_c_extension()


def quantize_median_cut(data, order, weights=None):
    """Median-cut quantisation of the rows of `data` (float32 [M, K], on the GPU) into 2^order colours; `weights`
    (float32 [M]) weighs the rows in the cuts and in the means.  Returns (colors float32 [2^order, K], color_id_map
    int32 [M]): colors[color_id_map] is the quantised table.  0 <= order <= 16, 2^order <= M.
    svox_t_amd.csrc.quantize_median_cut has the reference's argument order and the differences from it;
    N3Tree.quantize applies the palette to a tree."""
    return _C.quantize_median_cut(data, weights, order)
