"""The operators of `svox_t.csrc` around the render path: point query (svox_kernel.cu:45-94, 240-324), the roofline
counters, the motion variants (rt_kernel.cu:698-1061), point skinning (svox_kernel.cu:123-211), octree construction
(svox.py:160-161, 488-560), pruning, subdividing, the frontier reductions and merge -- marshalling only, one C-ABI call
each (two for the builder, prune, subdivide, unshare, the frontier and merge)."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from ._abi import _CMotion, _COptimHyper, _CRays, _CTree, _lib
from ._marshal import (CameraSpec, RaysSpec, RenderOptions, TreeSpec, _ACCEL_CACHE, _aligned16, _drop_accel, _call, _check_input, _check_quantize, _numel, _pack_opts, _pack_rays,
                       get_out_data_dim, _on, _pack_tree, _pack_tree_accel, _ptr, _stream)

def _check_indices(indices):
    """check_indices (svox_kernel.cu:36-40)."""
    _check_input(indices, "indices")
    if indices.dim() != 2:
        raise RuntimeError("indices must be 2-D")
    if not indices.is_floating_point():
        raise RuntimeError("indices must be floating point")
    if indices.dtype != torch.float32 or indices.shape[1] != 3:
        raise RuntimeError("indices must be float32 [Q, 3]")


def query_vertical(tree: TreeSpec, indices: torch.Tensor):
    """svox_kernel.cu:274-324.  Returns (values [Q,K], node_ids [Q] int64,
    data_ids [Q] int64, leaf_node [U,4] int64).

    Differences from the reference, all where its result is undefined:
    rows of `values` for empty leaves are zeros (reference: uninitialised,
    :282), `data_ids` is -1 there, and `leaf_node` is sorted by packed leaf id
    (reference: order set by a float atomic counter, :260-269)."""
    ct = _pack_tree(tree)
    _check_indices(indices)
    dev = indices.device
    Q = indices.shape[0]
    N = ct.N
    with _on(dev):
        values = torch.empty((Q, ct.K), dtype=torch.float32, device=dev)
        node_ids = torch.empty((Q,), dtype=torch.int64, device=dev)
        data_ids = torch.empty((Q,), dtype=torch.int64, device=dev)
        mask = torch.zeros((ct.n_internal * N * N * N,), dtype=torch.uint8, device=dev)
        _call("svoxt_query_fwd", ctypes.byref(ct), _ptr(indices), Q, _ptr(values), _ptr(node_ids),
              _ptr(data_ids), _ptr(mask), _stream(dev))
        n_slots = mask.numel()
        cap = min(Q, n_slots)
        leaf_buf = torch.empty((cap, 4), dtype=torch.int64, device=dev)
        count = torch.empty((1,), dtype=torch.int64, device=dev)
        ws = torch.empty((_lib.svoxt_query_leaves_workspace_bytes(n_slots),), dtype=torch.uint8, device=dev)
        _call("svoxt_query_leaves", _ptr(mask), n_slots, N, _ptr(leaf_buf), _ptr(count), _ptr(ws), _stream(dev))
        leaf_node = leaf_buf[:int(count.item())]         # host sync, like the reference's .item() (:312)
    return values, node_ids, data_ids, leaf_node


def query_vertical_backward(tree: TreeSpec, indices: torch.Tensor,
                            grad_output: torch.Tensor) -> torch.Tensor:
    """svox_kernel.cu:380-402."""
    ct = _pack_tree(tree)
    _check_indices(indices)
    _check_input(grad_output, "grad_output")
    if grad_output.dtype != torch.float32 or tuple(grad_output.shape) != (indices.shape[0], ct.K):
        raise RuntimeError("grad_output must be float32 [Q, K]")
    dev = indices.device
    with _on(dev):
        grad = torch.empty((ct.M, ct.K), dtype=torch.float32, device=dev)
        _call("svoxt_query_bwd", ctypes.byref(ct), _ptr(indices), indices.shape[0],
              _ptr(grad_output), _ptr(grad), _stream(dev))
    return grad


def count_forward(tree: TreeSpec, rays: RaysSpec, opt: RenderOptions) -> torch.Tensor:
    """Roofline counters (not in the reference): int64 [5] on the device =
    (rays hitting the cube, leaf crossings, child words read, valid leaves,
    composited samples).  See SURVEY.md 8(d)."""
    ct, cr, co = _pack_tree(tree), _pack_rays(rays), _pack_opts(opt)
    dev = tree.features.device
    with _on(dev):
        counters = torch.zeros((5,), dtype=torch.int64, device=dev)
        _call("svoxt_count_fwd", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co),
              _ptr(counters), _stream(dev))
    return counters


def count_touched(tree: TreeSpec, rays: RaysSpec, opt: RenderOptions):
    """Roofline instrumentation (include/svoxt.h, svoxt_count_touched): what one forward march of
    the batch touches.  Returns a dict of counts: feature rows read by the forward (valid leaves)
    and again by the backward (composited samples), grid cells and (child, data) pairs (or child /
    data words without the grid), and the most leaf crossings of any ray."""
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rays), _pack_opts(opt)
    dev = tree.features.device
    n_slots = ct.n_internal * ct.N ** 3
    with _on(dev):
        rows = torch.zeros((2 * ct.M,), dtype=torch.uint8, device=dev)
        n_cells = (1 << (3 * (ct.accel_log2 & 0xff))) if ct.accel else 0
        tmask = torch.zeros(((n_cells + n_slots) if ct.accel else 2 * n_slots,), dtype=torch.uint8, device=dev)
        longest = torch.zeros((1,), dtype=torch.int64, device=dev)
        _call("svoxt_count_touched", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), _ptr(rows), _ptr(tmask),
              _ptr(longest), _stream(dev))
        first = n_cells if ct.accel else n_slots
        res = {"rows_valid": int(rows[:ct.M].sum(dtype=torch.int64)), "rows_composited": int(rows[ct.M:].sum(dtype=torch.int64)),
               "longest_ray_crossings": int(longest.item()), "accel": bool(ct.accel)}
        a, b = int(tmask[:first].sum(dtype=torch.int64)), int(tmask[first:].sum(dtype=torch.int64))
        res.update({"grid_cells": a, "node_pairs": b} if ct.accel else {"child_words": a, "data_words": b})
    return res


class bwd_counters:
    """`with bwd_counters() as c: ...backward...; c.read()` -> (64-byte atomic requests, (tile, pass, row)
    groups) of the one-kernel per-tile backwards run inside (svoxt_set_bwd_counters)."""

    def __init__(self, device):
        self.buf = torch.zeros((2,), dtype=torch.int64, device=device)

    def __enter__(self):
        _call("svoxt_set_bwd_counters", _ptr(self.buf))
        return self

    def __exit__(self, *exc):
        _call("svoxt_set_bwd_counters", None)

    def read(self):
        return tuple(int(v) for v in self.buf.cpu().tolist())


class bwd_check:
    """`with bwd_check(dev) as c: ...backward...; c.read()` -> ({site: violations}, tiles worked on): the per-tile
    backwards run inside take their CHECKED instances -- every LDS / pool / table index compared with its extent
    (svoxt_set_bwd_check; the sites are listed at grad_fused_kernel / grad_wide_kernel)."""

    def __init__(self, device):
        self.buf = torch.zeros((32,), dtype=torch.int64, device=device)

    def __enter__(self):
        _call("svoxt_set_bwd_check", _ptr(self.buf))
        return self

    def __exit__(self, *exc):
        _call("svoxt_set_bwd_check", None)

    def read(self):
        w = [int(v) for v in self.buf.cpu().tolist()]
        return {site: n for site, n in enumerate(w[2:31]) if n}, w[31]


def motion_render(tree: TreeSpec, rays: RaysSpec, opt: RenderOptions):
    """rt_kernel.cu:1480-1504.  Returns (joint distances [Q, J], depth [Q, 1],
    hit_point [Q, 3], data_idx [Q, 1] int64); J = tree.extra_data.shape[0]."""
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rays), _pack_opts(opt)
    if not _numel(tree.extra_data):
        raise RuntimeError("motion_render needs extra_data [n_joints, >= 3] (the joint positions)")
    dev = tree.features.device
    with _on(dev):
        out = torch.empty((cr.Q, ct.extra_rows), dtype=torch.float32, device=dev)
        depth = torch.empty((cr.Q, 1), dtype=torch.float32, device=dev)
        hit = torch.empty((cr.Q, 3), dtype=torch.float32, device=dev)
        idx = torch.empty((cr.Q, 1), dtype=torch.int64, device=dev)
        _call("svoxt_motion_render", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co),
              _ptr(out), _ptr(depth), _ptr(hit), _ptr(idx), _stream(dev))
    return out, depth, hit, idx


def _pack_motion(tree: TreeSpec, ct: _CTree) -> _CMotion:
    jf, sw, ji = tree.joint_features, tree.skinning_weights, tree.joint_index
    for nm, x in (("joint_features", jf), ("skinning_weights", sw), ("joint_index", ji)):
        if not _numel(x):
            raise RuntimeError(f"motion_feature_render needs {nm}")
        _check_input(x, nm)
    if jf.dtype != torch.float32 or jf.dim() != 2 or sw.dtype != torch.float32 or sw.dim() != 2:
        raise RuntimeError("joint_features / skinning_weights must be float32 and 2-D")
    if ji.dtype != torch.int32 or ji.shape != sw.shape or sw.shape[0] != ct.M:
        raise RuntimeError("joint_index must be int32 with the shape of skinning_weights, [M, n_bind]")
    return _CMotion(jf.data_ptr(), jf.shape[0], jf.shape[1], sw.data_ptr(), ji.data_ptr(), sw.shape[1])


def _motion_workspace(ct: _CTree, cm: _CMotion, dev) -> torch.Tensor:
    nbytes = _lib.svoxt_motion_workspace_bytes(ct.M, cm.feature_dim)
    if nbytes < 0:
        raise RuntimeError("joint feature dim must be in [1, 32] (the reference's tmp_data_dim)")
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def motion_feature_render(tree: TreeSpec, rays: RaysSpec, opt: RenderOptions) -> torch.Tensor:
    """rt_kernel.cu:1525-1543: [Q, joint_features.shape[1]]."""
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rays), _pack_opts(opt)
    cm = _pack_motion(tree, ct)
    dev = tree.features.device
    with _on(dev):
        out = torch.empty((cr.Q, cm.feature_dim), dtype=torch.float32, device=dev)
        ws = _motion_workspace(ct, cm, dev)
        _call("svoxt_motion_feature_render_fwd", ctypes.byref(ct), ctypes.byref(cm), ctypes.byref(cr),
              ctypes.byref(co), _ptr(out), _ptr(ws), ws.numel(), _stream(dev))
    return out


def motion_feature_render_backward(tree: TreeSpec, rays: RaysSpec, opt: RenderOptions,
                                   grad_output: torch.Tensor) -> torch.Tensor:
    """rt_kernel.cu:1546-1572: gradient wrt joint_features, [n_joints, F] (the
    derivative of the forward; the reference's kernel is defective, include/svoxt.h)."""
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rays), _pack_opts(opt)
    cm = _pack_motion(tree, ct)
    _check_input(grad_output, "grad_output")
    if grad_output.dtype != torch.float32 or tuple(grad_output.shape) != (cr.Q, cm.feature_dim):
        raise RuntimeError("grad_output must be float32 [Q, joint feature dim]")
    dev = tree.features.device
    with _on(dev):
        grad = torch.empty((cm.n_joints, cm.feature_dim), dtype=torch.float32, device=dev)
        ws = _motion_workspace(ct, cm, dev)
        _call("svoxt_motion_feature_render_bwd", ctypes.byref(ct), ctypes.byref(cm), ctypes.byref(cr),
              ctypes.byref(co), _ptr(grad_output), _ptr(grad), _ptr(ws), ws.numel(), _stream(dev))
    return grad


def _check_warp(matrices, indices, skinning_weights, joint_index):
    _check_indices(indices)
    for nm, x in (("matrices", matrices), ("skinning_weights", skinning_weights), ("joint_index", joint_index)):
        _check_input(x, nm)
    if matrices.dtype != torch.float32 or matrices.dim() != 3 or tuple(matrices.shape[1:]) != (4, 4):
        raise RuntimeError("matrices must be float32 [n_joints, 4, 4]")
    Q = indices.shape[0]
    if skinning_weights.dtype != torch.float32 or skinning_weights.dim() != 2 or skinning_weights.shape[0] != Q:
        raise RuntimeError("skinning_weights must be float32 [Q, n_bind]")
    if joint_index.dtype != torch.int32 or joint_index.shape != skinning_weights.shape:
        raise RuntimeError("joint_index must be int32 with the shape of skinning_weights")
    return Q, matrices.shape[0], skinning_weights.shape[1]


def warp_vertices(matrices: torch.Tensor, indices: torch.Tensor, skinning_weights: torch.Tensor,
                  joint_index: torch.Tensor):
    """svox_kernel.cu:354-378: linear blend skinning of points.  Returns
    (vertices_out [Q, 3], matrix_out [Q, 4, 4])."""
    Q, J, B = _check_warp(matrices, indices, skinning_weights, joint_index)
    dev = indices.device
    with _on(dev):
        vout = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        mout = torch.empty((Q, 4, 4), dtype=torch.float32, device=dev)
        _call("svoxt_warp_vertices", _ptr(matrices), J, _ptr(indices), Q, _ptr(skinning_weights),
              _ptr(joint_index), B, _ptr(vout), _ptr(mout), _stream(dev))
    return [vout, mout]


def warp_vertices_backward(matrices: torch.Tensor, indices: torch.Tensor, skinning_weights: torch.Tensor,
                           joint_index: torch.Tensor, indices_grad_out: torch.Tensor,
                           matrices_grad_out: torch.Tensor):
    """svox_kernel.cu:404-436.  Returns [grad_indices [Q, 3], grad_matrices [n_joints, 4, 4],
    grad_skinning_weights [Q, n_bind]]."""
    Q, J, B = _check_warp(matrices, indices, skinning_weights, joint_index)
    _check_input(indices_grad_out, "indices_grad_out")
    _check_input(matrices_grad_out, "matrices_grad_out")
    if indices_grad_out.dtype != torch.float32 or tuple(indices_grad_out.shape) != (Q, 3) or \
            matrices_grad_out.dtype != torch.float32 or tuple(matrices_grad_out.shape) != (Q, 4, 4):
        raise RuntimeError("gradients must be float32 [Q, 3] and [Q, 4, 4]")
    dev = indices.device
    with _on(dev):
        gi = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        gm = torch.empty((J, 4, 4), dtype=torch.float32, device=dev)
        gs = torch.empty((Q, B), dtype=torch.float32, device=dev)
        _call("svoxt_warp_vertices_bwd", _ptr(matrices), J, _ptr(indices), Q, _ptr(skinning_weights),
              _ptr(joint_index), B, _ptr(indices_grad_out), _ptr(matrices_grad_out), _ptr(gi), _ptr(gm),
              _ptr(gs), _stream(dev))
    return [gi, gm, gs]


def refine_leaves(child: torch.Tensor, data: torch.Tensor, parent_depth: torch.Tensor, filled: int,
                  leaf_node: torch.Tensor, node_id: torch.Tensor = None) -> None:
    """The table updates of N3Tree.refine for the leaves in `leaf_node` [U, 4] int64
    (svox.py:535-546), in place, as one kernel (not an entry of the reference's
    extension, which does this with tensor ops).  The tables must have room for
    filled + U nodes."""
    for nm, x in (("child", child), ("data", data), ("parent_depth", parent_depth), ("leaf_node", leaf_node)):
        _check_input(x, nm)
    if leaf_node.dtype != torch.int64 or leaf_node.dim() != 2 or leaf_node.shape[1] != 4:
        raise RuntimeError("leaf_node must be int64 [U, 4]")
    if child.dtype != torch.int32 or data.dtype != torch.int32 or parent_depth.dtype != torch.int32:
        raise RuntimeError("child / data / parent_depth must be int32")
    if node_id is not None:
        _check_input(node_id, "node_id")
        if node_id.dtype != torch.int32 or node_id.numel() != leaf_node.shape[0]:
            raise RuntimeError("node_id must be int32 [U]")
    dev = child.device
    with _on(dev):
        _call("svoxt_refine", _ptr(leaf_node), leaf_node.shape[0], child.shape[1], int(filled), child.shape[0],
              _ptr(child), _ptr(data), _ptr(parent_depth), _ptr(node_id), _stream(dev))
    for t in (child, data, parent_depth):
        torch.autograd.graph.increment_version(t)
    _drop_accel(child)


def construct_tree(tree: TreeSpec, indices: torch.Tensor) -> None:
    """svox_kernel.cu:341-352: data[leaf containing point i] = i, in place on
    `tree.data`.  Where several points share a leaf the smallest index is kept
    (the reference keeps whichever thread wrote last)."""
    ct = _pack_tree(tree)
    _check_indices(indices)
    dev = indices.device
    with _on(dev):
        _call("svoxt_construct_tree", ctypes.byref(ct), _ptr(indices), indices.shape[0], _stream(dev))
    # tree.data was written behind torch's back: tell the version counter (the
    # acceleration-grid cache keys on it) and drop any grid built from the old words
    torch.autograd.graph.increment_version(tree.data)
    _drop_accel(tree.child)


def _workspace(dev, nbytes, refusal):
    """The workspace a *_workspace_bytes query asks for; the query's -1 (extents out of range) is refused with `refusal`."""
    if nbytes < 0:
        raise RuntimeError(refusal)
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def _count(dev, nbytes, refusal, n_counts, call):
    """The first half of a count / emit pipeline: the workspace, the counts on the device, `call(workspace pointer,
    nbytes, counts pointer)`, and the one host read that sizes the outputs.  Returns (workspace, [counts as ints])."""
    ws = _workspace(dev, nbytes, refusal)
    counts = torch.empty((n_counts,), dtype=torch.int64, device=dev)
    call(_ptr(ws), nbytes, _ptr(counts))
    return ws, [int(v) for v in counts.tolist()]


def _new_tables(rows, N, used, empty_index, dev):
    """child / data / parent_depth of `rows` rows: the first `used` left for the caller to write, the rows behind them
    initialised like unused rows of an N3Tree."""
    child = torch.empty((rows, N, N, N), dtype=torch.int32, device=dev)
    data = torch.empty((rows, N, N, N, 1), dtype=torch.int32, device=dev)
    parent_depth = torch.empty((rows, 2), dtype=torch.int32, device=dev)
    if rows > used:
        child[used:].zero_()
        data[used:].fill_(int(empty_index))
        parent_depth[used:].zero_()
    return child, data, parent_depth


def slot_decision(child, name, mask, weights, threshold, required):
    """The caller's decision over the slots of child: a bool / uint8 mask (the argument called `name`), or float32 weights
    with a threshold, or -- unless `required` -- neither: every slot.  Returns ({argument name: the tensor given}, the
    threshold for the call); devices are checked with the tables (_check_on_device_of_child)."""
    if required and (mask is None) == (weights is None):
        raise RuntimeError(f"exactly one of {name} / weights must be given")
    if mask is not None and weights is not None:
        raise RuntimeError(f"at most one of {name} / weights may be given")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != tuple(child.shape):
            raise RuntimeError(f"{name} must be a bool or uint8 tensor with the shape of child")
        if threshold is not None:
            raise RuntimeError(f"threshold goes with weights, not with {name}")
        given, thr = {name: mask}, 0.0
    elif weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != tuple(child.shape):
            raise RuntimeError("weights must be a float32 tensor with the shape of child")
        if threshold is None or float(threshold) != float(threshold):
            raise RuntimeError("weights needs a threshold (not NaN)")
        given, thr = {"weights": weights}, float(threshold)
    else:
        if threshold is not None:
            raise RuntimeError("threshold goes with weights")
        given, thr = {}, 0.0
    if any(v.device != child.device for v in given.values()):
        raise RuntimeError(f"{name} / weights must be on the device of child")
    return given, thr


def build_octree(points: torch.Tensor, offset: torch.Tensor, scaling: torch.Tensor, depth: int,
                 empty_index: int, reserve: int = 0):
    """Octree of a point cloud in one pipeline (not an entry of the reference's
    extension; it stands for `depth - 1` rounds of `tree[points].refine()` on a
    fresh N = 2 tree followed by `construct_tree(points)`, include/svoxt.h).

    Returns (child [n + reserve, 2, 2, 2] int32, data [n + reserve, 2, 2, 2, 1] int32,
    parent_depth [n + reserve, 2] int32, n): the first n rows are the tree, the
    `reserve` rows after them are initialised like unused rows of an N3Tree."""
    _check_indices(points)
    for name, x in (("offset", offset), ("scaling", scaling)):
        _check_input(x, name)
        if x.dtype != torch.float32 or x.numel() != 3:
            raise RuntimeError(f"{name} must be float32 [3]")
    dev = points.device
    P = points.shape[0]
    with _on(dev):
        nbytes = _lib.svoxt_build_workspace_bytes(int(depth))
        ws, (n,) = _count(dev, nbytes, "build_octree: depth must be in [1, 10]", 1, lambda w, b, c: _call(
            "svoxt_build_count", _ptr(points), P, _ptr(offset), _ptr(scaling), int(depth), w, b, c, _stream(dev)))
        child, data, parent_depth = _new_tables(n + int(reserve), 2, n, empty_index, dev)
        _call("svoxt_build_emit", _ptr(points), P, _ptr(offset), _ptr(scaling), int(depth),
              _ptr(ws), nbytes, _ptr(child), _ptr(data), _ptr(parent_depth), n, int(empty_index),
              _stream(dev))
    return child, data, parent_depth, n


def prune_tree(child: torch.Tensor, data: torch.Tensor, parent_depth: torch.Tensor, n_internal: int, M: int,
               keep: torch.Tensor = None, weights: torch.Tensor = None, threshold: float = None, collapse: bool = True,
               compact_features: bool = True, reserve: int = 0, empty_index: int = 1410065408, return_dropped: bool = False):
    """The tables of a pruned tree in one pipeline (not an entry of the reference's extension, which has merge and
    shrink_to_fit as tensor ops: svox.py:352-389, 600-642; include/svoxt.h, svoxt_prune_count has the four steps).

    keep: bool / uint8 with the shape of child, or weights: float32 of that shape with `threshold` (kept iff
    weights >= threshold; NaN drops).  Returns (child [n' + reserve, N, N, N], data [n' + reserve, N, N, N, 1],
    parent_depth [n' + reserve, 2], n', row_map): new tensors, the `reserve` rows behind the tree initialised like unused
    rows of an N3Tree; row_map int64 [M'] = the old row of every new feature row (None without compact_features);
    with return_dropped a sixth value, the number of leaves that held a feature row and were not kept.
    One host read (the counts that size the outputs)."""
    _, N, n = _check_tables(child, data, parent_depth, n_internal)
    M, reserve = int(M), int(reserve)
    if M < 0 or reserve < 0:
        raise RuntimeError("M and reserve must be >= 0")
    given, thr = slot_decision(child, "keep", keep, weights, threshold, required=True)
    _check_on_device_of_child(child, data=data, parent_depth=parent_depth, **given)
    dev = child.device
    kp, wp = _ptr(keep), _ptr(weights)
    with _on(dev):
        nbytes = _lib.svoxt_prune_workspace_bytes(n, M)
        ws, (new_n, new_M, dropped) = _count(dev, nbytes, "prune_tree: n_internal and M must be below 2^31", 3, lambda w, b, c: _call(
            "svoxt_prune_count", _ptr(child), _ptr(data), _ptr(parent_depth), n, N, M, kp, wp, thr, int(bool(collapse)),
            int(bool(compact_features)), w, b, c, _stream(dev)))
        child_out, data_out, pd_out = _new_tables(new_n + reserve, N, new_n, empty_index, dev)
        row_map = torch.empty((new_M,), dtype=torch.int64, device=dev) if compact_features else None
        _call("svoxt_prune_emit", _ptr(child), _ptr(data), _ptr(parent_depth), n, N, M, kp, wp, thr, int(bool(compact_features)),
              _ptr(ws), nbytes, new_n, new_M, int(empty_index), _ptr(child_out), _ptr(data_out), _ptr(pd_out), _ptr(row_map),
              _stream(dev))
    res = (child_out, data_out, pd_out, new_n, row_map)
    return res + (dropped,) if return_dropped else res


def gather_rows(src: torch.Tensor, row_map: torch.Tensor) -> torch.Tensor:
    """src[row_map] for a float32 [M, K] table and prune_tree's row_map (svoxt_prune_gather_rows: 16 bytes a thread)."""
    _check_input(src, "src")
    _check_input(row_map, "row_map")
    if src.dtype != torch.float32 or src.dim() != 2 or src.shape[1] < 1:
        raise RuntimeError("src must be float32 [M, K]")
    if row_map.dtype != torch.int64 or row_map.dim() != 1 or row_map.device != src.device:
        raise RuntimeError("row_map must be int64 [M'] on the device of src")
    dev = src.device
    with _on(dev):
        dst = torch.empty((row_map.shape[0], src.shape[1]), dtype=torch.float32, device=dev)
        _call("svoxt_prune_gather_rows", _ptr(src), src.shape[0], _ptr(row_map), _ptr(dst), row_map.shape[0], src.shape[1],
              _stream(dev))
    return dst


def _grown_tables(child, data, parent_depth, rows, empty_index):
    """The three tables with `rows` rows: the old ones copied, the rows behind them initialised like unused rows of an N3Tree."""
    cap, N = child.shape[0], child.shape[1]
    child2, data2, pd2 = _new_tables(rows, N, cap, empty_index, child.device)
    child2[:cap], data2[:cap], pd2[:cap] = child, data.reshape(cap, N, N, N, 1), parent_depth
    return child2, data2, pd2


def subdivide_tree(child: torch.Tensor, data: torch.Tensor, parent_depth: torch.Tensor, n_internal: int, M: int,
                   sel: torch.Tensor = None, weights: torch.Tensor = None, threshold: float = None, depth_limit: int = 0x7fffffff,
                   split_empty: bool = False, own_rows: bool = True, empty_index: int = 1410065408, grow=None,
                   slot_limit: int = 1 << 31):
    """Split the selected leaves of a tree into new nodes behind `n_internal`, in one pipeline (csrc/svoxt_subdivide.hip;
    include/svoxt.h, svoxt_subdivide_count has the rules): the topology N3Tree.refine(sel) writes, with `own_rows` a
    feature row of its own for every new leaf but the first of each node.

    sel: bool / uint8 with the shape of child, or weights: float32 of that shape with `threshold` (selected iff
    weights >= threshold; NaN never splits), or neither: every leaf.  The tables are written IN PLACE where their
    capacity suffices; otherwise `grow(rows_needed)` has to return larger (child, data, parent_depth) holding the old
    rows (None: new tables of exactly the rows needed).  Returns (child, data, parent_depth, nodes_added, rows_added,
    row_map): row_map int64 [M + rows_added] = the old row of every new feature row, None without own_rows.  Refused
    before anything is written: (n_internal + nodes_added) * N^3 >= slot_limit (2^31: slot indices are int32),
    M + rows_added >= empty_index.  One host read (the counts)."""
    cap, N, n = _check_tables(child, data, parent_depth, n_internal)
    M = int(M)
    if M < 0:
        raise RuntimeError("M must be >= 0")
    extra, thr = slot_decision(child, "sel", sel, weights, threshold, required=False)
    _check_on_device_of_child(child, data=data, parent_depth=parent_depth, **extra)
    dev = child.device
    n3 = N ** 3
    limit = max(-0x80000000, min(0x7fffffff, int(depth_limit)))
    with _on(dev):
        nbytes = _lib.svoxt_subdivide_workspace_bytes(n, N, M)
        ws, (added, rows_added) = _count(dev, nbytes, "subdivide_tree: n_internal * N^3 and M must be below 2^31", 2, lambda w, b, c: _call(
            "svoxt_subdivide_count", _ptr(child), _ptr(data), _ptr(parent_depth), n, N, M, _ptr(sel), _ptr(weights), thr, limit,
            int(bool(split_empty)), int(bool(own_rows)), w, b, c, _stream(dev)))
        if (n + added) * n3 >= int(slot_limit):
            raise RuntimeError(f"subdivide_tree: {n} + {added} nodes of {n3} slots do not fit 32-bit slot indices "
                               f"((n_internal + nodes_added) * N^3 must be < {int(slot_limit)})")
        if M + rows_added >= int(empty_index):
            raise RuntimeError(f"subdivide_tree: {M} + {rows_added} feature rows reach the empty index {int(empty_index)}")
        row_map = torch.empty((M + rows_added,), dtype=torch.int64, device=dev) if own_rows else None
        if n + added > cap:
            child, data, parent_depth = grow(n + added) if grow is not None else \
                _grown_tables(child, data, parent_depth, n + added, empty_index)
            _check_tables(child, data, parent_depth, n + added)
            _check_on_device_of_child(child, data=data, parent_depth=parent_depth)
            if child.device != dev:
                raise RuntimeError("grow() must return tables on the device of the old ones")
        _call("svoxt_subdivide_emit", _ptr(child), _ptr(data), _ptr(parent_depth), n, N, M, child.shape[0], int(bool(own_rows)),
              _ptr(ws), nbytes, added, rows_added, int(empty_index), _ptr(row_map), _stream(dev))
    if added > 0:                                     # (nothing splits: row_map = 0 .. M - 1 is all the emit wrote)
        for t in (child, data, parent_depth):
            torch.autograd.graph.increment_version(t)
        _drop_accel(child)
    return child, data, parent_depth, added, rows_added, row_map


def unshare_rows(child: torch.Tensor, data: torch.Tensor, n_internal: int, M: int, empty_index: int = 1410065408):
    """Give every leaf slot that names a feature row an earlier slot names too a row of its own (csrc/svoxt_subdivide.hip;
    include/svoxt.h, svoxt_unshare_count): the slot with the smallest flat index keeps the row, the others get rows M,
    M + 1, ... in slot order.  `data` is rewritten IN PLACE.  Returns (rows_added, row_map int64 [M + rows_added] = the old
    row of every new row).  One host read (the count)."""
    _, N, n = _check_tables(child, data, None, n_internal)
    M = int(M)
    if M < 0:
        raise RuntimeError("M must be >= 0")
    _check_on_device_of_child(child, data=data)
    dev = child.device
    with _on(dev):
        nbytes = _lib.svoxt_subdivide_workspace_bytes(n, N, M)
        ws, (rows_added,) = _count(dev, nbytes, "unshare_rows: n_internal * N^3 and M must be below 2^31", 1, lambda w, b, c: _call(
            "svoxt_unshare_count", _ptr(child), _ptr(data), n, N, M, w, b, c, _stream(dev)))
        if M + rows_added >= int(empty_index):
            raise RuntimeError(f"unshare_rows: {M} + {rows_added} feature rows reach the empty index {int(empty_index)}")
        row_map = torch.empty((M + rows_added,), dtype=torch.int64, device=dev)
        _call("svoxt_unshare_emit", _ptr(data), n, N, M, _ptr(ws), nbytes, rows_added, int(empty_index), _ptr(row_map), _stream(dev))
    if rows_added > 0:
        torch.autograd.graph.increment_version(data)
        _drop_accel(child)
    return rows_added, row_map


REDUCE_OPS = {"mean": 0, "sum": 1, "max": 2, "min": 3}        # SVOXT_REDUCE_* (include/svoxt.h)
EMPTY_MODES = {"zero": 0, "skip": 1}                          # SVOXT_EMPTY_*


def _check_tables(child, data, parent_depth, n_internal):
    """Types and shapes of the tree tables (devices: _check_on_device_of_child).  Returns (cap, N, n)."""
    for nm, x in (("child", child), ("data", data)) + ((("parent_depth", parent_depth),) if parent_depth is not None else ()):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int32:
            raise RuntimeError(f"{nm} must be an int32 tensor")
    if child.dim() != 4 or child.shape[1] < 2 or child.shape[1] > 16 or child.shape[2] != child.shape[1] \
            or child.shape[3] != child.shape[1]:
        raise RuntimeError("child must be int32 [cap, N, N, N] with N in [2, 16]")
    cap, N = child.shape[0], child.shape[1]
    if data.numel() != child.numel() or data.shape[0] != cap:
        raise RuntimeError("data must be int32 [cap, N, N, N, 1] matching child")
    if parent_depth is not None and tuple(parent_depth.shape) != (cap, 2):
        raise RuntimeError("parent_depth must be int32 [cap, 2]")
    n = int(n_internal)
    if n < 1 or n > cap:
        raise RuntimeError("n_internal must be in [1, cap]")
    return cap, N, n


def _check_on_device_of_child(child, **tensors):
    """CHECK_INPUT of the tables (and what goes with them), last: shapes and values are refused before devices."""
    for nm, x in (("child", child),) + tuple(tensors.items()):
        _check_input(x, nm)
        if x.device != child.device:
            raise RuntimeError(f"{nm} must be on the device of child")


def frontier_nodes(child: torch.Tensor, n_internal: int) -> torch.Tensor:
    """int64 [F], ascending: the nodes other than the root whose N^3 slots are all leaves (the reference's _frontier,
    svox.py:471-483, which lists the root too).  Flags, a scan, one host read (F), an emit (csrc/svoxt_merge.hip)."""
    _, N, n = _check_tables(child, child, None, n_internal)
    _check_on_device_of_child(child)
    dev = child.device
    with _on(dev):
        nbytes = _lib.svoxt_frontier_workspace_bytes(n)
        ws, (F,) = _count(dev, nbytes, "frontier_nodes: n_internal must be below 2^31", 1, lambda w, b, c: _call(
            "svoxt_frontier_count", _ptr(child), n, N, w, b, c, _stream(dev)))
        out = torch.empty((F,), dtype=torch.int64, device=dev)
        _call("svoxt_frontier_emit", _ptr(ws), nbytes, n, F, _ptr(out), _stream(dev))
    return out


def _reduce_args(features, data, n_internal, N, nodes, cols, op, empty):
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] < 1:
        raise RuntimeError("features must be float32 [M, K]")
    if not isinstance(data, torch.Tensor) or data.dtype != torch.int32:
        raise RuntimeError("data must be an int32 tensor")
    if not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.int64 or nodes.dim() != 1:
        raise RuntimeError("nodes must be int64 [F]")
    if op not in REDUCE_OPS:
        raise RuntimeError(f"op must be one of {sorted(REDUCE_OPS)}")
    if empty not in EMPTY_MODES:
        raise RuntimeError('empty must be "zero" or "skip"')
    n, N = int(n_internal), int(N)
    if N < 2 or N > 16 or n < 1 or data.numel() < n * N ** 3:
        raise RuntimeError("data must hold n_internal * N^3 words, N in [2, 16]")
    K = features.shape[1]
    if cols is not None:
        if not isinstance(cols, torch.Tensor) or cols.dtype != torch.int32 or cols.dim() != 1:
            raise RuntimeError("cols must be int32 [K']")
        if cols.numel() == 0:
            raise RuntimeError("cols selects no column")
    for nm, x in (("features", features), ("data", data), ("nodes", nodes)) + ((("cols", cols),) if cols is not None else ()):
        _check_input(x, nm)
        if x.device != features.device:
            raise RuntimeError(f"{nm} must be on the device of features")
    return n, N, K, (K if cols is None else cols.shape[0])


def frontier_reduce(features, data, n_internal, N, nodes, cols=None, op="mean", empty="zero", out=None) -> torch.Tensor:
    """[F, K'] float32: row f = op over the N^3 children of node nodes[f] of their (selected) feature rows, in slot
    order (include/svoxt.h, svoxt_frontier_reduce).  cols: int32 [K'] columns in [0, K) or None (all).  out: a
    contiguous float32 [F, K'] tensor to write instead of a new one."""
    n, N, K, Kc = _reduce_args(features, data, n_internal, N, nodes, cols, op, empty)
    if cols is not None and (int(cols.min()) < 0 or int(cols.max()) >= K):
        raise RuntimeError("cols out of range")
    dev = features.device
    F = nodes.shape[0]
    with _on(dev):
        if out is None:
            out = torch.empty((F, Kc), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) != (F, Kc) or not out.is_contiguous() or out.device != dev:
            raise RuntimeError("out must be a contiguous float32 [F, K'] tensor on the device of features")
        _call("svoxt_frontier_reduce", _ptr(features), features.shape[0], K, _ptr(data), n, N, _ptr(nodes), F, _ptr(cols),
              0 if cols is None else Kc, REDUCE_OPS[op], EMPTY_MODES[empty], _ptr(out), _stream(dev))
    return out


def frontier_reduce_backward(features, data, n_internal, N, nodes, cols, op, empty, grad_out) -> torch.Tensor:
    """Gradient of frontier_reduce with respect to features, float32 [M, K] (svoxt_frontier_reduce_bwd)."""
    n, N, K, Kc = _reduce_args(features, data, n_internal, N, nodes, cols, op, empty)
    _check_input(grad_out, "grad_out")
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (nodes.shape[0], Kc) or grad_out.device != features.device:
        raise RuntimeError("grad_out must be float32 [F, K'] on the device of features")
    dev = features.device
    with _on(dev):
        grad = torch.empty_like(features)             # zeroed by the call
        _call("svoxt_frontier_reduce_bwd", _ptr(features), features.shape[0], K, _ptr(data), n, N, _ptr(nodes), nodes.shape[0],
              _ptr(cols), 0 if cols is None else Kc, REDUCE_OPS[op], EMPTY_MODES[empty], _ptr(grad_out), _ptr(grad), _stream(dev))
    return grad


def frontier_diam(features, data, n_internal, N, nodes, cols=None, empty="zero", scale=1.0) -> torch.Tensor:
    """float32 [F]: the largest Euclidean distance between the (selected, scaled) rows of two children of each node
    (svoxt_frontier_diam; the reference's diam_frontier, svox.py:438-468)."""
    n, N, K, Kc = _reduce_args(features, data, n_internal, N, nodes, cols, "max", empty)
    scale = float(scale)
    if scale != scale:
        raise RuntimeError("scale is NaN")
    if cols is not None and (int(cols.min()) < 0 or int(cols.max()) >= K):
        raise RuntimeError("cols out of range")
    dev = features.device
    F = nodes.shape[0]
    if cols is None and N == 2 and K % 4 == 0 and K <= 32:
        # The library's 16-byte route (whole rows of an octree node, taken where features and data are 16-byte aligned)
        # adds a pair's squared differences in another order than its 4-byte route: both inputs are only read, so a
        # tensor that starts elsewhere goes in as an aligned copy -- the same route and the same bits wherever it starts.
        features, data = _aligned16(features), _aligned16(data)
    with _on(dev):
        out = torch.empty((F,), dtype=torch.float32, device=dev)
        _call("svoxt_frontier_diam", _ptr(features), features.shape[0], K, _ptr(data), n, N, _ptr(nodes), F, _ptr(cols),
              0 if cols is None else Kc, EMPTY_MODES[empty], scale, _ptr(out), _stream(dev))
    return out


def merge_tree(child, data, parent_depth, n_internal, features, selected, op="mean", empty="zero", compact_features=True,
               reserve=0, empty_index=1410065408):
    """The tables and the feature table of a tree with the selected frontier nodes merged into leaves (include/svoxt.h,
    svoxt_merge_count; csrc/svoxt_merge.hip).  selected: bool / uint8 [n_internal], per NODE; entries at nodes that are
    not frontier nodes are ignored.  Returns (child [n' + reserve, N, N, N], data [n' + reserve, N, N, N, 1],
    parent_depth [n' + reserve, 2], n', features [carried + rows_added, K], row_map int64 [carried] or None,
    rows_added): new tensors.  One host read (the counts that size the outputs)."""
    _, N, n = _check_tables(child, data, parent_depth, n_internal)
    if op not in ("mean", "max", "min"):
        raise RuntimeError('merge: op must be "mean", "max" or "min"')
    if empty not in EMPTY_MODES:
        raise RuntimeError('empty must be "zero" or "skip"')
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] < 1:
        raise RuntimeError("features must be float32 [M, K]")
    if not isinstance(selected, torch.Tensor) or selected.dtype not in (torch.bool, torch.uint8) or tuple(selected.shape) != (n,):
        raise RuntimeError("selected must be a bool or uint8 tensor [n_internal]")
    reserve = int(reserve)
    if reserve < 0:
        raise RuntimeError("reserve must be >= 0")
    _check_on_device_of_child(child, data=data, parent_depth=parent_depth, features=features, selected=selected)
    dev = child.device
    M, K = features.shape
    compact = int(bool(compact_features))
    with _on(dev):
        nbytes = _lib.svoxt_merge_workspace_bytes(n, M)
        ws, (new_n, carried, added) = _count(dev, nbytes, "merge_tree: n_internal and M must be below 2^31", 3, lambda w, b, c: _call(
            "svoxt_merge_count", _ptr(child), _ptr(data), _ptr(parent_depth), n, N, M, _ptr(selected), compact, w, b, c, _stream(dev)))
        child_out, data_out, pd_out = _new_tables(new_n + reserve, N, new_n, empty_index, dev)
        row_map = torch.empty((carried,), dtype=torch.int64, device=dev) if compact else None
        new_nodes = torch.empty((added,), dtype=torch.int64, device=dev)
        _call("svoxt_merge_emit", _ptr(child), _ptr(data), _ptr(parent_depth), n, N, M, _ptr(selected), compact, _ptr(ws), nbytes,
              new_n, carried, added, int(empty_index), _ptr(child_out), _ptr(data_out), _ptr(pd_out), _ptr(row_map),
              _ptr(new_nodes), _stream(dev))
        table = torch.empty((carried + added, K), dtype=torch.float32, device=dev)
        if compact:
            if carried > 0:
                _call("svoxt_prune_gather_rows", _ptr(features), M, _ptr(row_map), _ptr(table), carried, K, _stream(dev))
        else:
            table[:M].copy_(features)
        if added > 0:                                                   # the reduced rows, behind the carried ones
            frontier_reduce(features, data, n, N, new_nodes, None, op, empty, out=table[carried:])
    return child_out, data_out, pd_out, new_n, table, row_map, added


def _p2v_args(points, point_features, volume_corner, volume_size, n_voxels, kernel_radius, conv_radius):
    """The checks of p2v / p2v_backward (the reference's check_indices, p2v_kernel.cu:241, and more: its kernels
    take anything).  Corner and size come to the library as host floats: reading a CUDA tensor here is a sync."""
    for name, x in (("points", points), ("point_features", point_features)):
        _check_input(x, name)
        if x.dtype != torch.float32 or x.dim() != 2:
            raise RuntimeError(f"{name} must be a 2-D float32 tensor")
    if points.shape[1] != 3:
        raise RuntimeError("points must be [P, 3]")
    if point_features.shape[0] != points.shape[0] or point_features.shape[1] < 1:
        raise RuntimeError("point_features must be [P, F] with the rows of points and F >= 1")
    if point_features.device != points.device:
        raise RuntimeError("points and point_features must be on the same device")
    geo = []
    for name, v in (("volume_corner", volume_corner), ("volume_size", volume_size)):
        if isinstance(v, torch.Tensor):
            if v.is_floating_point() is False or v.numel() != 3:
                raise RuntimeError(f"{name} must hold 3 floating-point numbers")
            v = v.detach().reshape(3).to("cpu", torch.float32).tolist()
        else:
            v = [float(c) for c in v]
            if len(v) != 3:
                raise RuntimeError(f"{name} must hold 3 numbers")
        geo.append((ctypes.c_float * 3)(*v))
    return geo[0], geo[1], int(n_voxels), float(kernel_radius), float(conv_radius)


def p2v_order(points: torch.Tensor, point_features: torch.Tensor, volume_corner, volume_size, n_voxels: int,
              kernel_radius: float, conv_radius: float):
    """p2v and the permutation its sort put the points in (int32 [P]; p2v_backward walks the points in that order)."""
    corner, size, n, kr, cr = _p2v_args(points, point_features, volume_corner, volume_size, n_voxels, kernel_radius,
                                        conv_radius)
    dev = points.device
    P, F = points.shape[0], point_features.shape[1]
    nbytes = _lib.svoxt_p2v_workspace_bytes(P, n, corner, size, cr)
    if nbytes < 0:                                 # the library names what is wrong, before it touches the GPU
        _call("svoxt_p2v_fwd", None, None, P, F, corner, size, n, kr, cr, None, None, None, 0, None)
    with _on(dev):
        voxels = torch.empty((n, n, n, 1), dtype=torch.float32, device=dev)
        order = torch.empty((P,), dtype=torch.int32, device=dev)
        ws = torch.empty((nbytes if P > 0 else 0,), dtype=torch.uint8, device=dev)
        _call("svoxt_p2v_fwd", _ptr(points), _ptr(point_features), P, F, corner, size, n, kr, cr, _ptr(voxels),
              _ptr(order), _ptr(ws), nbytes, _stream(dev))
    return voxels, order


def p2v(points: torch.Tensor, point_features: torch.Tensor, volume_corner, volume_size, n_voxels: int,
        kernel_radius: float, conv_radius: float) -> torch.Tensor:
    """p2v_kernel.cu:240-261: the Gaussian splat of point_features[:, F-1] into a float32 [n, n, n, 1] volume.

    Same (point, voxel) pairs as the reference; unlike it the result is bit-identical from run to run, non-finite
    points contribute nothing, inputs are float32 only and bad arguments raise RuntimeError."""
    return p2v_order(points, point_features, volume_corner, volume_size, n_voxels, kernel_radius, conv_radius)[0]


def p2v_backward(grad_output: torch.Tensor, points: torch.Tensor, point_features: torch.Tensor, volume_corner,
                 volume_size, n_voxels: int, kernel_radius: float, conv_radius: float, order=None,
                 need_points_grad: bool = True, need_features_grad: bool = True):
    """p2v_kernel.cu:263-285.  Returns [points_grad [P, 3], point_features_grad [P, F]] (None for one not asked for).

    The reference writes the feature gradient to column 0 although the forward reads column F-1 (:203 vs :147);
    here column F-1 gets it and the other columns are 0 -- for F = 1 the two agree.  No atomics: each element is
    written once, the sums per point in the reference's order.  `order`: the forward's permutation (speed only)."""
    corner, size, n, kr, cr = _p2v_args(points, point_features, volume_corner, volume_size, n_voxels, kernel_radius,
                                        conv_radius)
    if not isinstance(grad_output, torch.Tensor):
        raise RuntimeError("grad_output must be a tensor")
    grad_output = grad_output.contiguous()         # autograd hands sum().backward() an expanded, stride-0 gradient
    _check_input(grad_output, "grad_output")
    if grad_output.dtype != torch.float32 or tuple(grad_output.shape) != (n, n, n, 1):
        raise RuntimeError(f"grad_output must be float32 [{n}, {n}, {n}, 1]")
    if grad_output.device != points.device:
        raise RuntimeError("grad_output must be on the points' device")
    if order is not None and (order.dtype != torch.int32 or order.shape != (points.shape[0],) or order.device != points.device):
        raise RuntimeError("order must be the forward's int32 [P] permutation")
    dev = points.device
    P, F = points.shape[0], point_features.shape[1]
    with _on(dev):
        pg = torch.empty((P, 3), dtype=torch.float32, device=dev) if need_points_grad else None
        fg = torch.empty((P, F), dtype=torch.float32, device=dev) if need_features_grad else None
        _call("svoxt_p2v_bwd", _ptr(grad_output), _ptr(points), _ptr(point_features), P, F, corner, size, n, kr, cr,
              _ptr(order), _ptr(pg), _ptr(fg), _stream(dev))
    return [pg, fg]


GRIDW_ACCUMULATE = 1          # SVOXT_GRIDW_ACCUMULATE (include/svoxt.h)


def grid_weights(sigma: torch.Tensor, cams_or_rays, opt: RenderOptions, offset: torch.Tensor, scaling: torch.Tensor,
                 out=None):
    """The reference's grid_weight_render (rt_kernel.cu:1240-1344, 1454-1478) over many views: per cell of the dense
    float32 volume sigma [R, R, R] (or [R, R, R, 1]) the largest compositing weight any ray gave it and the number of
    samples taken in it.  Returns (weight, hits), float32 with the shape of sigma.

    cams_or_rays: a CameraSpec whose c2w is [V, 3, 4] / [V, 4, 4] (or one [3, 4] / [4, 4] matrix) -- V cameras
    sharing fx, fy, width, height, all marched by one launch -- or a RaysSpec (origins, dirs [Q, 3]; vdirs is not
    read).  Of opt, step_size, sigma_thresh and ndc_* are read.  out = (weight, hits): updated instead of zeroed
    (max and count compose across calls).
    The checks of shapes and values come before the device checks, and all of them before any GPU work."""
    if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float32:
        raise RuntimeError("sigma must be a float32 tensor")
    if sigma.dim() not in (3, 4) or sigma.shape[0] < 1 or sigma.shape[1] != sigma.shape[0] or sigma.shape[2] != sigma.shape[0] \
            or (sigma.dim() == 4 and sigma.shape[3] != 1):
        raise RuntimeError("sigma must be a cubic volume [R, R, R] or [R, R, R, 1] with R >= 1")
    R = sigma.shape[0]
    if R ** 3 >= 1 << 31:
        raise RuntimeError("sigma is too large: R^3 must be below 2^31")
    step = float(opt.step_size)
    if not (step > 0.0) or step == float("inf"):
        raise RuntimeError("step_size must be finite and > 0")
    for name, x in (("offset", offset), ("scaling", scaling)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.numel() != 3:
            raise RuntimeError(f"{name} must be float32 [3]")
    if isinstance(cams_or_rays, CameraSpec):
        c2w = cams_or_rays.c2w
        if not isinstance(c2w, torch.Tensor) or c2w.dtype != torch.float32 or c2w.dim() not in (2, 3) \
                or tuple(c2w.shape[-2:]) not in ((3, 4), (4, 4)):
            raise RuntimeError("cameras must be float32 [V, 3, 4] or [V, 4, 4]")
        V = c2w.shape[0] if c2w.dim() == 3 else 1
        if V < 1:
            raise RuntimeError("cameras holds no view")
        w, h = int(cams_or_rays.width), int(cams_or_rays.height)
        if w < 1 or h < 1:
            raise RuntimeError("camera width / height must be positive")
        cr = _CRays()
        cr.Q, cr.image_width, cr.image_height = w * h, w, h
        cr.fx, cr.fy = float(cams_or_rays.fx), float(cams_or_rays.fy)
        stride, tensors = 4 * c2w.shape[-2], [("cameras", c2w)]
    elif isinstance(cams_or_rays, RaysSpec):
        o, d = cams_or_rays.origins, cams_or_rays.dirs
        for name, x in (("origins", o), ("dirs", d)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3:
                raise RuntimeError(f"{name} must be float32 [Q, 3]")
        if o.shape[0] != d.shape[0]:
            raise RuntimeError("origins and dirs must have the same number of rays")
        c2w, V, stride = None, 1, 0
        cr = _CRays()
        cr.Q = o.shape[0]
        tensors = [("origins", o), ("dirs", d)]
    else:
        raise RuntimeError("grid_weights needs a CameraSpec or a RaysSpec")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise RuntimeError("out must be (weight, hits)")
        for name, x in zip(("out weight", "out hits"), out):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != tuple(sigma.shape):
                raise RuntimeError(f"{name} must be float32 with the shape of sigma")
        if out[0] is out[1] or out[0].data_ptr() == out[1].data_ptr():
            raise RuntimeError("out weight and out hits must be two tensors")
        tensors += [("out weight", out[0]), ("out hits", out[1])]
    for name, x in [("sigma", sigma), ("offset", offset), ("scaling", scaling)] + tensors:
        _check_input(x, name)
        if x.device != sigma.device:
            raise RuntimeError(f"{name} must be on the device of sigma")
    dev = sigma.device
    if c2w is not None:
        cr.c2w = c2w.data_ptr()
    else:
        cr.origins, cr.dirs = _ptr(o), _ptr(d)
    co = _pack_opts(opt)
    flags = GRIDW_ACCUMULATE if out is not None else 0
    with _on(dev):
        if out is not None:
            weight, hits = out
        else:
            weight = torch.empty(sigma.shape, dtype=torch.float32, device=dev)     # zeroed by the call
            hits = torch.empty(sigma.shape, dtype=torch.float32, device=dev)
        _call("svoxt_grid_weights", sigma.data_ptr(), R, ctypes.byref(cr), V, stride, ctypes.byref(co), offset.data_ptr(),
              scaling.data_ptr(), flags, weight.data_ptr(), hits.data_ptr(), _stream(dev))
    return weight, hits


def quantize_median_cut(data: torch.Tensor, weights, order: int):
    """quantizer.cpp:130-157 on the GPU (csrc/svoxt_quant.hip): median-cut quantisation of the rows of data, float32
    [M, K], into 2^order colours.  weights: float32 [M], or None / an empty tensor for unweighted.  Returns (colors
    float32 [2^order, K], color_id_map int32 [M]); include/svoxt.h has the rule of a cut.  0 <= order <= 16,
    2^order <= M < 2^31.

    Where the reference leaves the result open it is fixed here: ties within a segment are ordered by row index (-0.0
    equal to +0.0), weight prefixes and colour sums run in float64 in a fixed order, so the result is bit-identical
    from run to run.  Three deliberate differences: the row of an empty segment is zero (reference: 0 / 0 = NaN; no
    row maps to it); a non-empty segment whose weights sum to zero takes the plain mean (reference: NaN); NaN in data
    is not checked and the result is then unspecified.  GPU tensors only; bad arguments raise RuntimeError before any
    GPU work."""
    weights, order = _check_quantize(data, weights, order)
    dev = data.device
    M, K = data.shape
    nbytes = _lib.svoxt_quantize_workspace_bytes(M, K, order, int(weights is not None))
    if nbytes < 0:                                 # the library names what is wrong, before it touches the GPU
        _call("svoxt_quantize_median_cut", None, M, K, None, order, None, None, None, 0, None)
    with _on(dev):
        colors = torch.empty((1 << order, K), dtype=torch.float32, device=dev)      # zeroed by the call
        color_id_map = torch.empty((M,), dtype=torch.int32, device=dev)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _call("svoxt_quantize_median_cut", _ptr(data), M, K, _ptr(weights), order, _ptr(colors), _ptr(color_id_map), _ptr(ws),
              nbytes, _stream(dev))
    return colors, color_id_map


def remap_index(data: torch.Tensor, index_map: torch.Tensor) -> torch.Tensor:
    """A new tensor with every word of data (int32, any shape) that names a row -- as an unsigned number below
    len(index_map) -- replaced by index_map[word] (int32 [M]); other words (empty leaves) are copied."""
    for name, x in (("data", data), ("index_map", index_map)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int32:
            raise RuntimeError(f"{name} must be an int32 tensor")
    if index_map.dim() != 1:
        raise RuntimeError("index_map must be 1-D")
    _check_input(data, "data")
    _check_input(index_map, "index_map")
    if index_map.device != data.device:
        raise RuntimeError("index_map must be on the device of data")
    dev = data.device
    with _on(dev):
        out = torch.empty_like(data)
        _call("svoxt_remap_index", _ptr(data), _ptr(out), data.numel(), _ptr(index_map), index_map.shape[0], _stream(dev))
    return out


ASSIGN_MODES = {"last": 0, "sum": 1, "mean": 2, "max": 3, "min": 4}        # SVOXT_ASSIGN_* (include/svoxt.h)


def assign_leaves(tree: TreeSpec, indices: torch.Tensor, values: torch.Tensor, reduce: str = "last", return_counts: bool = False):
    """Scatter values (float32 [Q, K]) into the rows of tree.features, IN PLACE, that the leaves of the points indices
    (float32 [Q, 3]) name -- the leaf of a point is query_vertical's; points in empty leaves are ignored; the points of a
    row are reduced by `reduce` ("last": the highest point index; "sum" / "mean" / "max" / "min": in ascending point
    index, sequential float32; include/svoxt.h, svoxt_assign_leaves).  Rows without a point keep their bits; the result
    is the same bits from run to run.  The table's version counter is bumped.  return_counts: the number of points of
    every row, int32 [M] (else None).  Bad arguments raise RuntimeError before any GPU work."""
    if reduce not in ASSIGN_MODES:
        raise RuntimeError(f"reduce must be one of {sorted(ASSIGN_MODES)}")
    table = tree.features
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] < 1:
        raise RuntimeError("features must be float32 [M, K]")
    if not isinstance(indices, torch.Tensor) or indices.dtype != torch.float32 or indices.dim() != 2 or indices.shape[1] != 3:
        raise RuntimeError("indices must be float32 [Q, 3]")
    Q, (M, K) = indices.shape[0], table.shape
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or tuple(values.shape) != (Q, K):
        raise RuntimeError("values must be float32 [Q, K], K the width of the feature table")
    if values.requires_grad or indices.requires_grad:
        raise RuntimeError("values and indices must not require grad: set() is not differentiable")
    if Q >= 2 ** 31 - 1 or M >= 2 ** 31 - 1:
        raise RuntimeError("the number of points and of feature rows must be below 2^31 - 1")
    _check_indices(indices)
    _check_input(values, "values")
    ct = _pack_tree(tree)
    dev = table.device
    if indices.device != dev or values.device != dev:
        raise RuntimeError("indices and values must be on the device of the feature table")
    mode = ASSIGN_MODES[reduce]
    with _on(dev), torch.no_grad():
        counts = torch.empty((M,), dtype=torch.int32, device=dev) if return_counts else None      # zeroed by the call
        nbytes = _lib.svoxt_assign_workspace_bytes(Q, M, mode)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _call("svoxt_assign_leaves", ctypes.byref(ct), _ptr(indices), Q, _ptr(values), mode, _ptr(table), _ptr(counts), _ptr(ws),
              nbytes, _stream(dev))
        torch.autograd.graph.increment_version(table)           # written behind torch's back: the counter says so
    return counts


def leaf_corners(child: torch.Tensor, parent_depth: torch.Tensor, N: int, leaf_node: torch.Tensor) -> torch.Tensor:
    """float32 [Q, 3]: the lower corner in [0, 1]^3 of the slots leaf_node (int64 [Q, 4]: node, x, y, z) -- one lane per
    slot walks parent_depth[:, 0] to the root with the operations of N3Tree._calc_corners' torch walk, in its order: the
    same bits (svoxt_leaf_corners).  A slot out of range gives NaN."""
    for nm, x in (("child", child), ("parent_depth", parent_depth)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int32:
            raise RuntimeError(f"{nm} must be an int32 tensor")
    N = int(N)
    if child.dim() != 4 or N < 2 or N > 16 or tuple(child.shape[1:]) != (N, N, N) or child.shape[0] < 1:
        raise RuntimeError("child must be int32 [cap, N, N, N] with N in [2, 16]")
    if tuple(parent_depth.shape) != (child.shape[0], 2):
        raise RuntimeError("parent_depth must be int32 [cap, 2]")
    if not isinstance(leaf_node, torch.Tensor) or leaf_node.dtype != torch.int64 or leaf_node.dim() != 2 or leaf_node.shape[1] != 4:
        raise RuntimeError("leaf_node must be int64 [Q, 4]")
    _check_on_device_of_child(child, parent_depth=parent_depth, leaf_node=leaf_node)
    dev = child.device
    Q = leaf_node.shape[0]
    with _on(dev):
        out = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        _call("svoxt_leaf_corners", _ptr(parent_depth), child.shape[0], N, _ptr(leaf_node), Q, _ptr(out), _stream(dev))
    return out


def snap_points(tree: TreeSpec, indices: torch.Tensor) -> torch.Tensor:
    """float32 [Q, 3]: the lower corner of the leaf of every point, in the coordinates the points came in (world, or the
    tree's own where the spec's offset / scaling are 0 / 1): query_vertical's descent, the corner walk, one launch
    (svoxt_snap_points)."""
    _check_indices(indices)
    ct = _pack_tree(tree)
    pd = tree.parent_depth
    if not isinstance(pd, torch.Tensor) or pd.dtype != torch.int32 or pd.dim() != 2 or pd.shape[1] != 2 or pd.shape[0] < ct.n_internal:
        raise RuntimeError("parent_depth must be int32 [>= n_internal, 2]")
    _check_input(pd, "parent_depth")
    dev = indices.device
    if pd.device != dev:
        raise RuntimeError("parent_depth must be on the device of indices")
    Q = indices.shape[0]
    with _on(dev):
        out = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        _call("svoxt_snap_points", ctypes.byref(ct), _ptr(pd), _ptr(indices), Q, _ptr(out), _stream(dev))
    return out


OPTIM_KINDS = {"sgd": 0, "sgd_momentum": 1, "rmsprop": 2, "adam": 3}        # SVOXT_OPTIM_* (include/svoxt.h)
OPTIM_STATES = {"sgd": 0, "sgd_momentum": 1, "rmsprop": 1, "adam": 2}        # svoxt_optim_state_count
_HYPER_FIELDS = tuple(n for n, _ in _COptimHyper._fields_)


def optim_step(kind: str, param: torch.Tensor, grad: torch.Tensor, state1, state2, hyper: dict, lazy: bool = True) -> None:
    """One optimizer step on a feature table, IN PLACE, as one launch on torch's current stream (svoxt_optim_step;
    include/svoxt.h has the arithmetic).  kind: "sgd", "sgd_momentum" (state1 = the momentum buffer), "rmsprop" (state1 =
    the square average) or "adam" (state1, state2 = the two moments); param, grad and the kind's state tables are
    float32 [M, K], contiguous, on one GPU; a table the kind does not keep must be None.  hyper: the float32 scalars of
    svoxt_optim_hyper by name (neg_step, momentum, one_minus_beta1, beta2, one_minus_beta2, bias2_sqrt, eps; the ones
    left out are 0), each computed by the caller in double precision.  lazy: rows whose gradient is all zeros keep
    their bits and are not read.  The version counters of param and of the state tables are bumped (the renderer's
    caches key on them).  Bad arguments raise RuntimeError before any GPU work."""
    if kind not in OPTIM_KINDS:
        raise RuntimeError(f"kind must be one of {sorted(OPTIM_KINDS)}")
    ns = OPTIM_STATES[kind]
    states = (state1, state2)
    for i, x in enumerate(states):
        if (x is not None) != (i < ns):
            raise RuntimeError(f'"{kind}" keeps {ns} state table(s): state{i + 1} must be ' + ("given" if i < ns else "None"))
    tables = [("param", param), ("grad", grad)] + [(f"state{i + 1}", x) for i, x in enumerate(states[:ns])]
    for name, x in tables:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.layout != torch.strided:
            raise RuntimeError(f"{name} must be a dense float32 tensor")
    if param.dim() != 2 or param.shape[0] < 1 or param.shape[1] < 1:
        raise RuntimeError("param must be [M, K] with M, K >= 1")
    for name, x in tables[1:]:
        if tuple(x.shape) != tuple(param.shape):
            raise RuntimeError(f"{name} must have the shape of param, {tuple(param.shape)}")
    for name, x in tables:
        if not x.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
    if not isinstance(hyper, dict) or any(k not in _HYPER_FIELDS for k in hyper):
        raise RuntimeError(f"hyper must be a dict with keys among {_HYPER_FIELDS}")
    ch = _COptimHyper(**{k: float(v) for k, v in hyper.items()})
    for name, x in tables:
        _check_input(x, name)
        if x.device != param.device:
            raise RuntimeError(f"{name} must be on the device of param")
    if len({x.data_ptr() for _, x in tables}) != len(tables):
        raise RuntimeError("param, grad and the state tables must be distinct tensors")
    dev = param.device
    M, K = param.shape
    with _on(dev), torch.no_grad():
        _call("svoxt_optim_step", OPTIM_KINDS[kind], _ptr(param), _ptr(grad), _ptr(state1), _ptr(state2), M, K, ch,
              int(bool(lazy)), _stream(dev))
        for _, x in tables[:1] + tables[2:]:                    # written behind torch's back: the counters say so
            torch.autograd.graph.increment_version(x)


def gauss_newton_step(param: torch.Tensor, grad: torch.Tensor, hess: torch.Tensor, lr: float = 1.0, damping: float = 0.0,
                      lazy: bool = True) -> None:
    """The damped Newton step on a diagonal curvature, IN PLACE, as one launch on torch's current stream
    (svoxt_gauss_newton_step): per element d = hess + damping, and where d > 0 param = param - lr * (grad / d), float32, one
    correctly rounded operation at a time; an element with d <= 0 (or NaN) is not written.  lazy: rows whose grad row is
    all zeros are read no further and not written.  param, grad, hess: float32 [M, K], contiguous, on one GPU, param
    distinct from both.  param's version counter is bumped.  Bad arguments raise RuntimeError before any GPU work."""
    tables = [("param", param), ("grad", grad), ("hess", hess)]
    for name, x in tables:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.layout != torch.strided:
            raise RuntimeError(f"{name} must be a dense float32 tensor")
    if param.dim() != 2 or param.shape[0] < 1 or param.shape[1] < 1:
        raise RuntimeError("param must be [M, K] with M, K >= 1")
    for name, x in tables[1:]:
        if tuple(x.shape) != tuple(param.shape):
            raise RuntimeError(f"{name} must have the shape of param, {tuple(param.shape)}")
    for name, x in tables:
        _check_input(x, name)
        if x.device != param.device:
            raise RuntimeError(f"{name} must be on the device of param")
    for name, v in (("lr", lr), ("damping", damping)):
        if isinstance(v, (torch.Tensor, bool)) or not isinstance(v, (int, float)) or v != v or v < 0:
            raise RuntimeError(f"{name} must be a Python number >= 0")
    if param.data_ptr() in (grad.data_ptr(), hess.data_ptr()):
        raise RuntimeError("param must be distinct from grad and hess")
    dev = param.device
    M, K = param.shape
    with _on(dev), torch.no_grad():
        _call("svoxt_gauss_newton_step", _ptr(param), _ptr(grad), _ptr(hess), M, K, float(lr), float(damping), int(bool(lazy)), _stream(dev))
        torch.autograd.graph.increment_version(param)           # written behind torch's back: the counter says so


def leaf_neighbors(child: torch.Tensor, parent_depth: torch.Tensor, n_internal: int, L: int, max_depth: int) -> torch.Tensor:
    """int32 [L, 6]: for every leaf slot of the nodes below n_internal (in slot order: row i is leaf index i) the leaf
    index of its face neighbour across -x +x -y +y -z +z, -1 outside the cube, -2 where the face is covered by finer
    leaves (svoxt_leaf_neighbors; include/svoxt.h has the rule).  L: the number of those leaf slots; max_depth: the
    deepest node's depth (N^(max_depth + 1) must stay below 2^31).  Integer work, two scans' launches and one kernel."""
    _, N, n = _check_tables(child, child, parent_depth, n_internal)
    L, max_depth = int(L), int(max_depth)
    if L < 0 or 12 * L >= 2 ** 31:
        raise RuntimeError("leaf_neighbors: the number of leaves must be >= 0 with 12 * L < 2^31")
    if max_depth < 0 or N ** (max_depth + 1) >= 2 ** 31:
        raise RuntimeError(f"leaf_neighbors: N^(depth + 1) = {N}^{max_depth + 1} must be below 2^31 (cell coordinates are int32)")
    _check_on_device_of_child(child, parent_depth=parent_depth)
    dev = child.device
    with _on(dev):
        nbytes = _lib.svoxt_neighbors_workspace_bytes(n, N)
        ws = _workspace(dev, nbytes, "leaf_neighbors: n_internal * N^3 must be below 2^31")
        out = torch.empty((L, 6), dtype=torch.int32, device=dev)
        _call("svoxt_leaf_neighbors", _ptr(child), _ptr(parent_depth), n, N, max_depth, L, _ptr(out), _ptr(ws), nbytes, _stream(dev))
    return out


class TVPlan:
    """The edge plan of N3Tree.tv: a CSR over feature rows (include/svoxt.h).  row_ptr int32 [M + 1], other int32 [2 E],
    meta uint8 [2 E], E edges; area_weights float32 [32] on the device: N^(-2 (d + 1)) by depth d."""
    __slots__ = ("row_ptr", "other", "meta", "E", "M", "area_weights")

    def __init__(self, row_ptr, other, meta, E, M, area_weights):
        self.row_ptr, self.other, self.meta, self.E, self.M, self.area_weights = row_ptr, other, meta, E, M, area_weights

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.row_ptr, self.other, self.meta, self.area_weights))


TV_PLAN_BUILDS = 0            # plans built so far (tests count them: N3Tree caches its plan)


def tv_plan(neighbors: torch.Tensor, depths: torch.Tensor, rows: torch.Tensor, M: int, N: int) -> TVPlan:
    """The edge plan for leaf_neighbors' table, the leaves' depths (int32 [L]) and feature rows (int64 [L], -1 = empty)
    and a feature table of M rows: svoxt_tv_plan_count, one host read (E), svoxt_tv_plan_emit."""
    global TV_PLAN_BUILDS
    for nm, x, dt in (("neighbors", neighbors, torch.int32), ("depths", depths, torch.int32), ("rows", rows, torch.int64)):
        if not isinstance(x, torch.Tensor) or x.dtype != dt:
            raise RuntimeError(f"{nm} must be a tensor of {dt}")
    L = depths.shape[0] if depths.dim() == 1 else -1
    if L < 0 or tuple(neighbors.shape) != (L, 6) or tuple(rows.shape) != (L,):
        raise RuntimeError("neighbors must be int32 [L, 6], depths int32 [L], rows int64 [L]")
    M, N = int(M), int(N)
    if M < 0 or M >= 2 ** 31 or N < 2 or N > 16 or 12 * L >= 2 ** 31:
        raise RuntimeError("tv_plan: M must be in [0, 2^31), N in [2, 16], 12 * L below 2^31")
    for nm, x in (("neighbors", neighbors), ("depths", depths), ("rows", rows)):
        _check_input(x, nm)
        if x.device != neighbors.device:
            raise RuntimeError(f"{nm} must be on the device of neighbors")
    dev = neighbors.device
    with _on(dev):
        mbytes = _lib.svoxt_tv_plan_workspace_bytes(L, -1)
        marks, (E,) = _count(dev, mbytes, "tv_plan: 12 * L must be below 2^31", 1, lambda w, b, c: _call(
            "svoxt_tv_plan_count", _ptr(neighbors), _ptr(depths), _ptr(rows), L, M, w, b, c, _stream(dev)))
        row_ptr = torch.empty((M + 1,), dtype=torch.int32, device=dev)
        other = torch.empty((2 * E,), dtype=torch.int32, device=dev)
        meta = torch.empty((2 * E,), dtype=torch.uint8, device=dev)
        nbytes = _lib.svoxt_tv_plan_workspace_bytes(L, E)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _call("svoxt_tv_plan_emit", _ptr(neighbors), _ptr(depths), _ptr(rows), L, M, E, _ptr(marks), mbytes, _ptr(ws), nbytes,
              _ptr(row_ptr), _ptr(other), _ptr(meta), _stream(dev))
        area = torch.tensor([float(N) ** (-2 * (d + 1)) for d in range(32)], dtype=torch.float64).to(torch.float32).to(dev)
    TV_PLAN_BUILDS += 1
    return TVPlan(row_ptr, other, meta, E, M, area)


TV_MODES = {"loss": 0, "loss_grad": 1, "accumulate": 2}       # SVOXT_TV_* (include/svoxt.h)


def tv_rows(features: torch.Tensor, plan: TVPlan, cols=None, p: int = 2, weight: str = "uniform", mean: bool = False,
            mode: str = "loss", out: torch.Tensor = None, scale: float = 0.0):
    """The smoothness loss over a plan's edges as one gather-only kernel (svoxt_tv_rows; include/svoxt.h has the
    arithmetic and the summation order).  features: float32 [M, K], contiguous; cols: int32 [K'] distinct columns or None.
    mode "loss" -> (loss float32 scalar tensor, None); "loss_grad" -> (loss, G float32 [M, K]); "accumulate":
    out[r, c] += scale * G[r, c] in place on `out` (float32 [M, K], contiguous) -> None.  mean: loss and G divided once
    by E * columns.  Bad arguments raise RuntimeError before any GPU work."""
    if p not in (1, 2):
        raise RuntimeError("p must be 1 or 2")
    if weight not in ("uniform", "area"):
        raise RuntimeError('weight must be "uniform" or "area"')
    if mode not in TV_MODES:
        raise RuntimeError(f"mode must be one of {sorted(TV_MODES)}")
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] < 1:
        raise RuntimeError("features must be float32 [M, K]")
    M, K = features.shape
    if not isinstance(plan, TVPlan) or plan.M != M:
        raise RuntimeError("the plan was built for another number of feature rows")
    Kc = K
    if cols is not None:
        if not isinstance(cols, torch.Tensor) or cols.dtype != torch.int32 or cols.dim() != 1 or cols.numel() == 0:
            raise RuntimeError("cols must be int32 [K'], K' >= 1")
        Kc = cols.shape[0]
        if Kc > K:
            raise RuntimeError("cols must be distinct columns")
    tensors = [("features", features), ("row_ptr", plan.row_ptr)] + ([("cols", cols)] if cols is not None else [])
    scale = float(scale)
    if mode == "accumulate":
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (M, K):
            raise RuntimeError("out must be float32 [M, K], the shape of features")
        if scale != scale:
            raise RuntimeError("scale is NaN")
        tensors.append(("out", out))
    for nm, x in tensors:
        _check_input(x, nm)
        if x.device != features.device:
            raise RuntimeError(f"{nm} must be on the device of features")
    if mode == "accumulate" and out.data_ptr() == features.data_ptr() and M > 0:
        raise RuntimeError("out must not be the feature table")
    dev = features.device
    divisor = float(plan.E * Kc) if mean else 0.0
    wants_loss = mode != "accumulate"
    with _on(dev), torch.no_grad():
        loss = torch.empty((), dtype=torch.float32, device=dev) if wants_loss else None
        table = out if mode == "accumulate" else (torch.empty((M, K), dtype=torch.float32, device=dev) if mode == "loss_grad" else None)
        nbytes = _lib.svoxt_tv_workspace_bytes(M, Kc) if wants_loss else 0
        if nbytes < 0:
            raise RuntimeError("tv_rows: M * columns must be below 2^38")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None
        _call("svoxt_tv_rows", _ptr(features), M, K, _ptr(plan.row_ptr), _ptr(plan.other), _ptr(plan.meta), plan.E, _ptr(cols),
              0 if cols is None else Kc, int(p), _ptr(plan.area_weights) if weight == "area" else None, divisor, scale,
              TV_MODES[mode], _ptr(loss), _ptr(table), _ptr(ws), nbytes, _stream(dev))
        if mode == "accumulate":
            torch.autograd.graph.increment_version(out)             # written behind torch's back: the counter says so
            return None
    return loss, table


# ---------------------------------------------------------------------------
# Entry points of svox_t.csrc that are outside this project's hot path
# (SURVEY.md section 2).  They exist so a caller gets a clear error, not an
# AttributeError.
# ---------------------------------------------------------------------------

def _out_of_scope(name, instead=None):
    def fn(*_a, **_k):
        raise NotImplementedError(
            f"svox_t_amd.csrc.{name}: " + (instead or
            "outside the accelerated hot path "
            "(volume_render / opacity / depth / query / construct_tree); see SURVEY.md section 2"))
    fn.__name__ = name
    return fn


# the reference's names stay stubs (their argument lists are the reference's, svox.cpp:80-83); the operators live under new names
assign_vertical = _out_of_scope(
    "assign_vertical", "served under another name: assign_vertical(tree, indices, values) is "
    "assign_leaves(tree, indices, values, reduce='last') -- N3Tree.set(indices, values), which also reduces the points "
    "of a leaf by sum / mean / max / min; see INTEGRATION.md")
calc_corners = _out_of_scope(
    "calc_corners", "served under another name: calc_corners(tree, indexer) is leaf_corners(child, parent_depth, N, "
    "leaf_node); snap_points(tree, indices) descends and takes the corner in one launch -- N3Tree.snap / leaf_boxes; see "
    "INTEGRATION.md")
# the reference's one-camera form of grid_weights; the name is kept a stub
grid_weight_render = _out_of_scope(
    "grid_weight_render", "served under another name: grid_weight_render(data, cam, opt, offset, scaling) is "
    "grid_weights(data, cameras=cam.c2w[None], ...) -- svox_t_amd.grid_weights, or svox_t_amd.csrc.grid_weights(data, cam, "
    "opt, offset, scaling), which returns the reference's (weight, hits); see INTEGRATION.md")


# ---------------------------------------------------------------------------
# Depth moments (svoxt_depthmom.hip; not in the reference)
# ---------------------------------------------------------------------------
DEPTH_AT = {"entry": 0, "mid": 1}
DEPTHMOM_SAMPLES = 128    # samples recorded per ray for the backward (12 bytes each, written only where a ray has them; a longer
                          # ray's tail is marched: at 64 the 1.5 % longer rays of the headline view cost 0.15 ms); 0: never record


def _depth_at(at) -> int:
    if isinstance(at, str):
        if at not in DEPTH_AT:
            raise RuntimeError(f"at must be 'entry' or 'mid' (or 0 / 1), not {at!r}")
        return DEPTH_AT[at]
    if isinstance(at, bool) or not isinstance(at, int) or at not in (0, 1):
        raise RuntimeError(f"at must be 'entry' or 'mid' (or 0 / 1), not {at!r}")
    return at


def _spec_ray_count(rays) -> int:
    if isinstance(rays, CameraSpec):
        return int(rays.width) * int(rays.height)
    if not isinstance(rays.origins, torch.Tensor) or rays.origins.dim() != 2:
        raise RuntimeError("origins must have shape [Q, 3]")
    return rays.origins.shape[0]


def _raysweep_plan_key(csrc, tree, rays, opt, lead):
    f = tree.features
    return lead + (id(f), f._version, f.data_ptr(), csrc._opt_key(opt), csrc._tree_key(tree), csrc._rays_key(rays))


class _RaySweepOp(NamedTuple):
    """A per-ray operator of csrc/svoxt_raysweep.h: what its forward and backward have to agree on."""
    name: str           # the entry points are svoxt_<name>_workspace_bytes / _fwd / _bwd
    cols: int           # floats per ray of the output and of grad_output
    plan_attr: str      # the attribute of the rays spec that keeps the forward's plan
    samples: str        # the module constant with the records kept per ray, read at call time (tests assign it)


def _raysweep_forward(op: _RaySweepOp, tree, rays, opt, lead=()):
    """[Q, op.cols] from svoxt_<op.name>_fwd, whose arguments are the specs, `lead`, the output and the workspace.  Where a
    backward will follow the samples are recorded and the plan (key, feature table, workspace, its size, the rays in the
    order walked or None) is left on the rays spec under op.plan_attr."""
    import svox_t_amd.csrc as csrc
    name, cols, plan_attr, samples = op.name, op.cols, op.plan_attr, globals()[op.samples]
    rr = rays if isinstance(rays, CameraSpec) else csrc._in_coherent_order(tree, rays, opt)[0]
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rr), _pack_opts(opt)
    dev = tree.features.device
    record = csrc._need_grad(tree, rays) and samples > 0 and cr.Q > 0
    with _on(dev):
        out = torch.empty((cr.Q, cols), dtype=torch.float32, device=dev)
        ws, nbytes = None, 0
        if record:
            nbytes = getattr(_lib, f"svoxt_{name}_workspace_bytes")(cr.Q, int(samples))
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _call(f"svoxt_{name}_fwd", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), *lead, _ptr(out), _ptr(ws), nbytes,
              _stream(dev))
    # (the records are only read by the backward: they serve as many backward calls as the graph is kept for)
    setattr(rays, plan_attr, (_raysweep_plan_key(csrc, tree, rays, opt, lead), tree.features, ws, nbytes,
                              None if rr is rays else rr) if record else None)
    return out


def _raysweep_backward(op: _RaySweepOp, tree, rays, opt, grad_output, lead=()):
    """The backward that goes with _raysweep_forward: [M, K] from svoxt_<op.name>_bwd for grad_output [Q, op.cols], over
    the plan the forward left where it still matches, marching otherwise."""
    import svox_t_amd.csrc as csrc
    name, cols, plan_attr = op.name, op.cols, op.plan_attr
    Q = _spec_ray_count(rays)
    if not isinstance(grad_output, torch.Tensor) or grad_output.dtype != torch.float32 or grad_output.dim() != 2 \
            or grad_output.shape[0] != Q or grad_output.shape[1] != cols:
        raise RuntimeError(f"grad_output must be float32 [Q, {cols}] with Q = {Q} rays")
    _check_input(grad_output, "grad_output")
    plan = getattr(rays, plan_attr, None)
    ws, nbytes, rr = None, 0, None
    if plan is not None and plan[1] is tree.features and plan[0] == _raysweep_plan_key(csrc, tree, rays, opt, lead):
        ws, nbytes, rr = plan[2], plan[3], plan[4]
    if rr is None:
        # (the same walk as the forward's where there is a plan; any coherent one otherwise)
        rr = rays if isinstance(rays, CameraSpec) or plan is not None else csrc._in_coherent_order(tree, rays, opt)[0]
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rr), _pack_opts(opt)
    dev = tree.features.device
    with _on(dev):
        grad = torch.zeros_like(tree.features)
        _call(f"svoxt_{name}_bwd", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), *lead, _ptr(grad_output), _ptr(grad), 0,
              _ptr(ws), nbytes, _stream(dev))
    return grad


_DEPTH_MOMENTS = _RaySweepOp("depth_moments", 3, "_svoxt_depth_plan", "DEPTHMOM_SAMPLES")


def depth_moments(tree: TreeSpec, rays, opt: RenderOptions, at=0) -> torch.Tensor:
    """[Q, 3] = (m1, m2, alpha) per ray: the first two moments of the compositing weights over distance and the
    accumulated alpha (include/svoxt.h, svoxt_depth_moments_fwd).  `rays`: a RaysSpec or a CameraSpec.  `at`: "entry" / 0
    (z = delta_scale * t, what render_depth reports) or "mid" / 1 (the middle of the leaf crossing).  A batch that is not
    an image is walked in svoxt_ray_order's order where that pays (RaysSpec.sort), a declared image in 8 x 8 tiles; every
    ray's row stays at its own index.  Where a backward will follow (rays.need_grad, else the feature table's
    requires_grad) the samples are recorded and left on the spec for depth_moments_backward."""
    return _raysweep_forward(_DEPTH_MOMENTS, tree, rays, opt, (_depth_at(at),))


def depth_moments_backward(tree: TreeSpec, rays, opt: RenderOptions, grad_output: torch.Tensor, at=0) -> torch.Tensor:
    """[M, K] gradient of depth_moments with respect to the feature table for grad_output [Q, 3]: the sigma column only
    (every other column is zero), by the reference's convention for its backward -- every sample with sigma > 0, no early
    stop: the true gradient at thresholds 0 (include/svoxt.h, svoxt_depth_moments_bwd).  Reads what the forward of the same
    spec objects recorded if nothing it depends on has changed since; marches otherwise."""
    return _raysweep_backward(_DEPTH_MOMENTS, tree, rays, opt, grad_output, (_depth_at(at),))


# ---------------------------------------------------------------------------
# Distortion loss (svoxt_distort.hip; not in the reference)
# ---------------------------------------------------------------------------
DISTORTION_SAMPLES = 128  # samples recorded per ray for the backward, as DEPTHMOM_SAMPLES; 0: never record
_DISTORTION = _RaySweepOp("distortion", 2, "_svoxt_distortion_plan", "DISTORTION_SAMPLES")


def distortion(tree: TreeSpec, rays, opt: RenderOptions) -> torch.Tensor:
    """[Q, 2] = (L, alpha) per ray: the distortion loss of mip-NeRF 360 over the ray's leaf crossings,
    L = sum_ij w_i w_j |s_i - s_j| + 1/3 sum_i w_i^2 d_i (s: the middle of a crossing, d: its length, both in world
    units), and the accumulated alpha (include/svoxt.h, svoxt_distortion_fwd).  `rays`: a RaysSpec or a CameraSpec; walked
    as depth_moments walks them, every ray's row at its own index.  Where a backward will follow (rays.need_grad, else the
    feature table's requires_grad) the samples are recorded and left on the spec for distortion_backward."""
    return _raysweep_forward(_DISTORTION, tree, rays, opt)


def distortion_backward(tree: TreeSpec, rays, opt: RenderOptions, grad_output: torch.Tensor) -> torch.Tensor:
    """[M, K] gradient of distortion with respect to the feature table for grad_output [Q, 2]: the sigma column only,
    by the reference's convention for its backward -- every sample with sigma > 0, no early stop, no rescale: the true
    gradient at thresholds 0 (include/svoxt.h, svoxt_distortion_bwd).  Reads what the forward of the same spec objects
    recorded if nothing it depends on has changed since; marches otherwise."""
    return _raysweep_backward(_DISTORTION, tree, rays, opt, grad_output)


# ---------------------------------------------------------------------------
# Per-sample interface (svoxt_samples.hip; not in the reference)
# ---------------------------------------------------------------------------
def ray_samples(tree: TreeSpec, rays, opt: RenderOptions, min_sigma=None, faces=False):
    """The leaf crossings of a ray batch as CSR lists (include/svoxt.h, svoxt_ray_samples_count / _emit): returns
    (offsets int64 [Q + 1], row int32 [T], ray int32 [T], depth float32 [T], length float32 [T], T).  `rays`: a RaysSpec
    or a CameraSpec, walked as depth_moments walks them; the lists are in ray-index order.  min_sigma None: every crossing
    with a feature row; a number: only those with features[row, -1] > min_sigma.  One host read (T); T >= 2^31 raises.
    faces=True: svoxt_ray_samples_emit_faces in place of the emit, and a seventh result, face uint8 [T]."""
    import svox_t_amd.csrc as csrc
    ms = None
    if min_sigma is not None:
        ms = float(min_sigma)
        if ms != ms:
            raise RuntimeError("min_sigma is NaN")
        ms = ctypes.byref(ctypes.c_float(ms))
    rr = rays if isinstance(rays, CameraSpec) else csrc._in_coherent_order(tree, rays, opt)[0]
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rr), _pack_opts(opt)
    dev = tree.features.device
    Q = cr.Q
    with _on(dev):
        if Q == 0:
            T, offsets = 0, torch.zeros((1,), dtype=torch.int64, device=dev)
        else:
            offsets = torch.empty((Q + 1,), dtype=torch.int64, device=dev)
            ws = _workspace(dev, _lib.svoxt_ray_samples_workspace_bytes(Q), "ray_samples: the batch must have fewer than 2^31 rays")
            _call("svoxt_ray_samples_count", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), ms, _ptr(offsets), _ptr(ws),
                  ws.numel(), _stream(dev))
            T = int(offsets[Q].item())                  # the one host read
            if T >= 1 << 31:
                raise RuntimeError(f"ray_samples: {T} samples; a batch's lists hold fewer than 2^31 (split the batch)")
        row, ray, depth, length = _new_lists(T, dev)
        face = torch.empty((T,), dtype=torch.uint8, device=dev) if faces else None
        if T > 0 and faces:
            _call("svoxt_ray_samples_emit_faces", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), ms, _ptr(offsets), _ptr(row),
                  _ptr(ray), _ptr(depth), _ptr(length), _ptr(face), _stream(dev))
        elif T > 0:
            _call("svoxt_ray_samples_emit", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), ms, _ptr(offsets), _ptr(row),
                  _ptr(ray), _ptr(depth), _ptr(length), _stream(dev))
    return (offsets, row, ray, depth, length, T, face) if faces else (offsets, row, ray, depth, length, T)


def _new_lists(Tn, dev):
    """The four per-sample arrays of a list of Tn samples: two int32 (ray and row), two float32 (depth and length)."""
    return (torch.empty((Tn,), dtype=torch.int32, device=dev), torch.empty((Tn,), dtype=torch.int32, device=dev),
            torch.empty((Tn,), dtype=torch.float32, device=dev), torch.empty((Tn,), dtype=torch.float32, device=dev))


def _count_and_emit(what, extent, dev, Q, nbytes, count, emit, n_index=1):
    """The pair of calls of a list producer that makes new lists out of old ones (select, split, merge_samples):
    count(offsets_out, total, workspace, workspace_bytes) -- the tail of every svoxt_samples_*_count --, the one host
    read, then emit((workspace, workspace_bytes), offsets_out, T', the pointers of ray', row', depth', length' and of
    n_index index arrays) where T' > 0.  A total of 2^31 or more is refused before anything is allocated or emitted
    (select's T' <= T never gets there).  `extent`: "T" or "Q", what the workspace is sized by.  Returns (offsets', ray', row', depth', length', index.., T')."""
    with _on(dev):
        offsets_out = torch.empty((Q + 1,), dtype=torch.int64, device=dev)
        total = torch.empty((1,), dtype=torch.int64, device=dev)
        ws = _workspace(dev, nbytes, f"{what}: {extent} must be below 2^31")
        count(_ptr(offsets_out), _ptr(total), _ptr(ws), nbytes)
        Tn = int(total.item())                          # the one host read
        if Tn >= 1 << 31:
            raise RuntimeError(f"{what}: the result would hold {Tn} samples; a list holds fewer than 2^31")
        new = _new_lists(Tn, dev) + tuple(torch.empty((Tn,), dtype=torch.int64, device=dev) for _ in range(n_index))
        if Tn > 0:
            emit((_ptr(ws), nbytes), _ptr(offsets_out), Tn, tuple(_ptr(x) for x in new))
    return (offsets_out,) + new + (Tn,)


def _check_csr(offsets, T) -> int:
    """The checks of a CSR pair (offsets int64 [Q + 1], T samples); returns Q."""
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise RuntimeError("offsets must be int64 [Q + 1]")
    _check_input(offsets, "offsets")
    Q = offsets.shape[0] - 1
    if Q >= 1 << 31 or T >= 1 << 31:
        raise RuntimeError("Q and T must be below 2^31")
    return Q


def _check_per_sample(x, name, T, dev, cols=None, dtype=torch.float32):
    shape = (T,) if cols is None else (T, cols)
    if not isinstance(x, torch.Tensor) or x.dtype != dtype or tuple(x.shape) != shape:
        raise RuntimeError(f"{name} must be {str(dtype).split('.')[-1]} {'[T]' if cols is None else '[T, C]'} with T = {T} samples")
    _check_input(x, name)
    if x.device != dev:
        raise RuntimeError(f"{name} must be on the device of offsets")


def sample_weights(offsets, length, sigma):
    """(w float32 [T], alpha float32 [Q]) of svoxt_sample_weights_fwd for offsets int64 [Q + 1], length and sigma [T]."""
    if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float32 or sigma.dim() != 1:
        raise RuntimeError("sigma must be float32 [T]")
    T = sigma.shape[0]
    Q = _check_csr(offsets, T)
    dev = offsets.device
    _check_per_sample(length, "length", T, dev)
    _check_per_sample(sigma, "sigma", T, dev)
    with _on(dev):
        w = torch.empty((T,), dtype=torch.float32, device=dev)
        alpha = torch.empty((Q,), dtype=torch.float32, device=dev)
        _call("svoxt_sample_weights_fwd", _ptr(offsets), Q, T, _ptr(length), _ptr(sigma), _ptr(w), _ptr(alpha), _stream(dev))
    return w, alpha


def sample_weights_backward(offsets, length, sigma, grad_w, grad_alpha):
    """grad_sigma float32 [T] of svoxt_sample_weights_bwd; grad_w [T] / grad_alpha [Q] may be None (zeros)."""
    T = sigma.shape[0]
    Q = _check_csr(offsets, T)
    dev = offsets.device
    _check_per_sample(length, "length", T, dev)
    _check_per_sample(sigma, "sigma", T, dev)
    if grad_w is not None:
        _check_per_sample(grad_w, "grad_w", T, dev)
    if grad_alpha is not None:
        _check_input(grad_alpha, "grad_alpha")
        if grad_alpha.dtype != torch.float32 or tuple(grad_alpha.shape) != (Q,) or grad_alpha.device != dev:
            raise RuntimeError("grad_alpha must be float32 [Q] on the device of offsets")
    with _on(dev):
        gs = torch.empty((T,), dtype=torch.float32, device=dev)
        # (a NULL gradient of an array that has elements: zeros, said by the pointer alone)
        _call("svoxt_sample_weights_bwd", _ptr(offsets), Q, T, _ptr(length), _ptr(sigma), _ptr(grad_w), _ptr(grad_alpha), _ptr(gs),
              _stream(dev))
    return gs


def _check_per_ray(x, name, Q, dev, cols=None):
    shape = (Q,) if cols is None else (Q, cols)
    _check_input(x, name)
    if x.dtype != torch.float32 or tuple(x.shape) != shape or x.device != dev:
        raise RuntimeError(f"{name} must be float32 {'[Q]' if cols is None else f'[Q, {cols}]'} with Q = {Q} rays, on the device of offsets")


def sample_weights_backward_length(offsets, length, sigma, grad_w, grad_alpha):
    """(grad_sigma, grad_length), both float32 [T], of svoxt_sample_weights_bwd_length: one pass, grad_sigma with
    sample_weights_backward's bits; grad_w [T] / grad_alpha [Q] may be None (zeros)."""
    T = sigma.shape[0]
    Q = _check_csr(offsets, T)
    dev = offsets.device
    _check_per_sample(length, "length", T, dev)
    _check_per_sample(sigma, "sigma", T, dev)
    if grad_w is not None:
        _check_per_sample(grad_w, "grad_w", T, dev)
    if grad_alpha is not None:
        _check_per_ray(grad_alpha, "grad_alpha", Q, dev)
    with _on(dev):
        gs = torch.empty((T,), dtype=torch.float32, device=dev)
        gl = torch.empty((T,), dtype=torch.float32, device=dev)
        _call("svoxt_sample_weights_bwd_length", _ptr(offsets), Q, T, _ptr(length), _ptr(sigma), _ptr(grad_w), _ptr(grad_alpha), _ptr(gs),
              _ptr(gl), _stream(dev))
    return gs, gl


def sample_geometry_backward(offsets, face, depth, length, dirs, grad_depth, grad_length):
    """(grad_origins, grad_dirs), both float32 [Q, 3], of svoxt_sample_geometry_bwd for face uint8 [T], depth / length
    float32 [T] and dirs float32 [Q, 3]; grad_depth / grad_length [T] may be None (zeros).  Every ray is written."""
    if not isinstance(face, torch.Tensor) or face.dtype != torch.uint8 or face.dim() != 1:
        raise RuntimeError("face must be uint8 [T]")
    T = face.shape[0]
    Q = _check_csr(offsets, T)
    dev = offsets.device
    _check_per_sample(face, "face", T, dev, dtype=torch.uint8)
    _check_per_sample(depth, "depth", T, dev)
    _check_per_sample(length, "length", T, dev)
    if not isinstance(dirs, torch.Tensor):
        raise RuntimeError("dirs must be float32 [Q, 3]")
    _check_per_ray(dirs, "dirs", Q, dev, 3)
    if grad_depth is not None:
        _check_per_sample(grad_depth, "grad_depth", T, dev)
    if grad_length is not None:
        _check_per_sample(grad_length, "grad_length", T, dev)
    with _on(dev):
        go = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        gd = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        _call("svoxt_sample_geometry_bwd", _ptr(offsets), Q, T, _ptr(face), _ptr(depth), _ptr(length), _ptr(dirs), _ptr(grad_depth),
              _ptr(grad_length), _ptr(go), _ptr(gd), _stream(dev))
    return go, gd


def sample_accumulate(offsets, w, values=None):
    """out float32 [Q, C] (or [Q] without values) of svoxt_sample_accumulate_fwd for w [T] and values [T, C]."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 1:
        raise RuntimeError("w must be float32 [T]")
    T = w.shape[0]
    if values is not None and (not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2
                               or values.shape[0] != T or values.shape[1] < 1):
        raise RuntimeError(f"values must be float32 [T, C] with T = {T} samples and C >= 1")
    Q = _check_csr(offsets, T)
    dev = offsets.device
    _check_per_sample(w, "w", T, dev)
    C = 1 if values is None else values.shape[1]
    if values is not None:
        _check_per_sample(values, "values", T, dev, C)
    with _on(dev):
        out = torch.empty((Q,) if values is None else (Q, C), dtype=torch.float32, device=dev)
        _call("svoxt_sample_accumulate_fwd", _ptr(offsets), Q, T, _ptr(w), _ptr(values), C, _ptr(out), _stream(dev))
    return out


def sample_accumulate_backward(ray, Q, w, values, grad_out, need_w=True, need_values=True):
    """(grad_w [T] or None, grad_values [T, C] or None) of svoxt_sample_accumulate_bwd for grad_out [Q, C] ([Q] without
    values) and ray int32 [T], the ray index of every sample."""
    T = w.shape[0]
    dev = w.device
    _check_per_sample(ray, "ray", T, dev, dtype=torch.int32)
    _check_per_sample(w, "w", T, dev)
    C = 1 if values is None else values.shape[1]
    if values is not None:
        _check_per_sample(values, "values", T, dev, C)
    _check_input(grad_out, "grad_out")
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != ((Q,) if values is None else (Q, C)) or grad_out.device != dev:
        raise RuntimeError("grad_out must be float32 with the shape of the output, on the device of w")
    need_values = bool(need_values and values is not None)
    with _on(dev):
        gw = torch.empty((T,), dtype=torch.float32, device=dev) if need_w else None
        gv = torch.empty((T, C), dtype=torch.float32, device=dev) if need_values else None
        _call("svoxt_sample_accumulate_bwd", _ptr(ray), Q, T, _ptr(w), _ptr(values), C, _ptr(grad_out), _ptr(gw), _ptr(gv), _stream(dev))
    return gw, gv


# ---------------------------------------------------------------------------
# Scans, quantiles and subsets of the lists (svoxt_scan.hip; not in the reference)
# ---------------------------------------------------------------------------
SCAN_OPS = {"sum": 0, "prod": 1, "max": 2, "min": 3}              # SVOXT_SCAN_* (include/svoxt.h)
SCAN_EXCLUSIVE, SCAN_REVERSE = 1, 2


def _scan_args(offsets, values, op, exclusive, reverse):
    if op not in SCAN_OPS:
        raise RuntimeError(f"op must be one of {sorted(SCAN_OPS)}")
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2 or values.shape[1] < 1:
        raise RuntimeError("values must be float32 [T, C], C >= 1")
    T, C = values.shape
    Q = _check_csr(offsets, T)
    _check_per_sample(values, "values", T, offsets.device, C)
    return Q, T, C, SCAN_OPS[op], (SCAN_EXCLUSIVE if exclusive else 0) | (SCAN_REVERSE if reverse else 0)


def ray_scan(offsets, values, op="sum", exclusive=False, reverse=False):
    """out float32 [T, C] of svoxt_ray_scan_fwd for offsets int64 [Q + 1] and values [T, C]; samples outside every
    segment get 0."""
    Q, T, C, opc, flags = _scan_args(offsets, values, op, exclusive, reverse)
    dev = offsets.device
    with _on(dev):
        out = torch.zeros((T, C), dtype=torch.float32, device=dev)
        _call("svoxt_ray_scan_fwd", _ptr(offsets), Q, T, _ptr(values), C, opc, flags, _ptr(out), _stream(dev))
    return out


def ray_scan_backward(offsets, values, op, exclusive, reverse, grad_out):
    """grad_values float32 [T, C] of svoxt_ray_scan_bwd for grad_out [T, C]."""
    Q, T, C, opc, flags = _scan_args(offsets, values, op, exclusive, reverse)
    dev = offsets.device
    _check_per_sample(grad_out, "grad_out", T, dev, C)
    with _on(dev):
        grad = torch.empty((T, C), dtype=torch.float32, device=dev)
        _call("svoxt_ray_scan_bwd", _ptr(offsets), Q, T, None if opc == 0 else _ptr(values), C, opc, flags, _ptr(grad_out), _ptr(grad),
              _stream(dev))
    return grad


def ray_quantile(offsets, w, q, normalize=True):
    """(index int64 [Q, nq], frac float32 [Q, nq]) of svoxt_ray_quantile for w float32 [T] and q float32 [nq] on the
    device (values in [0, 1]: the caller's check)."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 1:
        raise RuntimeError("w must be float32 [T]")
    T = w.shape[0]
    Q = _check_csr(offsets, T)
    dev = offsets.device
    _check_per_sample(w, "w", T, dev)
    if not isinstance(q, torch.Tensor) or q.dtype != torch.float32 or q.dim() != 1 or q.shape[0] < 1:
        raise RuntimeError("q must be float32 [nq], nq >= 1")
    _check_input(q, "q")
    if q.device != dev:
        raise RuntimeError("q must be on the device of offsets")
    nq = q.shape[0]
    with _on(dev):
        index = torch.empty((Q, nq), dtype=torch.int64, device=dev)
        frac = torch.empty((Q, nq), dtype=torch.float32, device=dev)
        _call("svoxt_ray_quantile", _ptr(offsets), Q, T, _ptr(w), _ptr(q), nq, 1 if normalize else 0, _ptr(index), _ptr(frac), _stream(dev))
    return index, frac


def samples_select(keep, offsets, ray, row, depth, length):
    """(offsets' int64 [Q + 1], ray', row', depth', length', index int64 [T'], T') of svoxt_samples_select_count / _emit
    for keep bool [T].  One host read (T')."""
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.dim() != 1:
        raise RuntimeError("keep must be bool [T]")
    T = keep.shape[0]
    Q = _check_csr(offsets, T)
    dev = offsets.device
    _check_per_sample(keep, "keep", T, dev, dtype=torch.bool)
    for name, x, dt in (("ray", ray, torch.int32), ("row", row, torch.int32), ("depth", depth, torch.float32), ("length", length, torch.float32)):
        _check_per_sample(x, name, T, dev, dtype=dt)
    old = (_ptr(ray), _ptr(row), _ptr(depth), _ptr(length))
    return _count_and_emit(
        "select", "T", dev, Q, _lib.svoxt_samples_select_workspace_bytes(T),
        lambda *out: _call("svoxt_samples_select_count", _ptr(keep), _ptr(offsets), Q, T, *out, _stream(dev)),
        lambda ws, _offsets_out, Tn, new: _call("svoxt_samples_select_emit", _ptr(keep), T, *ws, *old, Tn, *new, _stream(dev)))


# ---------------------------------------------------------------------------
# New lists out of old ones (svoxt_cut.hip; not in the reference)
# ---------------------------------------------------------------------------
SPLIT_MAX_PIECES = 1 << 30                                       # the largest max_pieces svoxt_samples_split_count takes


def samples_split(offsets, ray, row, depth, length, max_length=None, pieces=None, max_pieces=4096):
    """(offsets' int64 [Q + 1], ray', row', depth', length', index int64 [T'], T') of svoxt_samples_split_count / _emit:
    exactly one of max_length (a float > 0) and pieces (int32 [T]).  One host read (T')."""
    if (max_length is None) == (pieces is None):
        raise RuntimeError("split: exactly one of max_length and pieces must be given")
    if isinstance(max_pieces, bool) or not isinstance(max_pieces, int) or not 1 <= max_pieces <= SPLIT_MAX_PIECES:
        raise RuntimeError("split: max_pieces must be an int in [1, 2^30]")
    if pieces is None:
        if isinstance(max_length, (bool, torch.Tensor)) or not isinstance(max_length, (int, float)) or not max_length > 0:
            raise RuntimeError("split: max_length must be a float > 0 (inf allowed)")
        max_length = float(max_length)
    if not isinstance(length, torch.Tensor) or length.dim() != 1:
        raise RuntimeError("length must be float32 [T]")
    T = length.shape[0]
    Q = _check_csr(offsets, T)
    dev = offsets.device
    for name, x, dt in (("ray", ray, torch.int32), ("row", row, torch.int32), ("depth", depth, torch.float32), ("length", length, torch.float32)):
        _check_per_sample(x, name, T, dev, dtype=dt)
    if pieces is not None:
        _check_per_sample(pieces, "pieces", T, dev, dtype=torch.int32)
    old = (_ptr(ray), _ptr(row), _ptr(depth), _ptr(length))
    return _count_and_emit(
        "split", "T", dev, Q, _lib.svoxt_samples_split_workspace_bytes(T),
        lambda *out: _call("svoxt_samples_split_count", _ptr(length), None if pieces is None else _ptr(pieces),
                           0.0 if pieces is not None else max_length, max_pieces, _ptr(offsets), Q, T, *out, _stream(dev)),
        lambda ws, _offsets_out, Tn, new: _call("svoxt_samples_split_emit", T, *ws, *old, Tn, *new, _stream(dev)))


def samples_merge(offsets_a, depth_a, length_a, offsets_b, depth_b, length_b):
    """(offsets' int64 [Q + 1], ray', row' (-1), depth', length', index_a int64 [T'], index_b int64 [T'], T') of
    svoxt_samples_merge_count / _emit for two lists of the same Q rays.  One host read (T')."""
    for name, d, ln in (("a", depth_a, length_a), ("b", depth_b, length_b)):
        if not isinstance(d, torch.Tensor) or d.dim() != 1 or not isinstance(ln, torch.Tensor):
            raise RuntimeError(f"depth_{name} and length_{name} must be float32 [T_{name}]")
    Ta, Tb = depth_a.shape[0], depth_b.shape[0]
    Q = _check_csr(offsets_a, Ta)
    if _check_csr(offsets_b, Tb) != Q:
        raise RuntimeError(f"merge_samples: the lists are of {Q} and {offsets_b.shape[0] - 1} rays; they must be lists of the same rays")
    dev = offsets_a.device
    if offsets_b.device != dev:
        raise RuntimeError("merge_samples: the two lists must be on the same device")
    for name, x, T in (("depth_a", depth_a, Ta), ("length_a", length_a, Ta), ("depth_b", depth_b, Tb), ("length_b", length_b, Tb)):
        _check_per_sample(x, name, T, dev)
    lists = (_ptr(offsets_a), _ptr(depth_a), _ptr(length_a), Ta, _ptr(offsets_b), _ptr(depth_b), _ptr(length_b), Tb, Q)
    return _count_and_emit(
        "merge_samples", "Q", dev, Q, _lib.svoxt_samples_merge_workspace_bytes(Q),
        lambda *out: _call("svoxt_samples_merge_count", *lists, *out, _stream(dev)),
        lambda _ws, offsets_out, Tn, new: _call("svoxt_samples_merge_emit", *lists, offsets_out, Tn, *new, _stream(dev)), n_index=2)


# ---------------------------------------------------------------------------
# Samples to feature rows and back (svoxt_rows.hip; not in the reference)
# ---------------------------------------------------------------------------
ROW_CHUNK = 256                                                   # SVOXT_ROW_CHUNK (include/svoxt.h)
ROWS_OPS = {"sum": 0, "mean": 1, "max": 2, "min": 3}              # SVOXT_ROWS_* (include/svoxt.h)
ROW_PLAN_BUILDS = 0           # plans built so far (tests count them: RaySamples caches its plans)


class RowPlanArrays(NamedTuple):
    """What svoxt_row_plan_build / svoxt_row_plan_long write (include/svoxt.h)."""
    row_ptr: torch.Tensor          # int32 [M + 1]
    perm: torch.Tensor             # int32 [T]
    long_rows: torch.Tensor        # int32 [n_long]
    long_chunk_ptr: torch.Tensor   # int32 [n_long + 1]
    chunk_long: torch.Tensor       # int32 [n_chunks]
    T: int
    M: int
    n_outside: int
    longest: int


def _plan_args(plan: RowPlanArrays, with_M: bool = True) -> tuple:
    """A plan as the C ABI takes it: row_ptr, perm, M (svoxt_reduce_rows and svoxt_interp_rows_bwd have it there,
    svoxt_shade_samples_bwd in front: with_M False), long_rows, long_chunk_ptr, chunk_long, n_long, n_chunks."""
    return ((_ptr(plan.row_ptr), _ptr(plan.perm)) + ((plan.M,) if with_M else ()) +
            (_ptr(plan.long_rows), _ptr(plan.long_chunk_ptr), _ptr(plan.chunk_long), plan.long_rows.shape[0], plan.chunk_long.shape[0]))


def _check_rows_extent(M, what) -> int:
    if isinstance(M, bool) or not isinstance(M, int) or M < 0 or M >= 1 << 31:
        raise RuntimeError(f"{what}: M must be an int in [0, 2^31)")
    return M


def row_plan(row: torch.Tensor, M: int) -> RowPlanArrays:
    """The row plan of row int32 [T] for a table of M rows: svoxt_row_plan_build, one host read (the info record),
    svoxt_row_plan_long."""
    global ROW_PLAN_BUILDS
    if not isinstance(row, torch.Tensor) or row.dtype != torch.int32 or row.dim() != 1:
        raise RuntimeError("row must be int32 [T]")
    M = _check_rows_extent(M, "row_plan")
    _check_input(row, "row")
    T, dev = row.shape[0], row.device
    if T >= 1 << 31:
        raise RuntimeError("row_plan: T must be below 2^31")
    with _on(dev):
        nbytes = _lib.svoxt_row_plan_workspace_bytes(T, M)
        ws = _workspace(dev, nbytes, "row_plan: T and M must be below 2^31")
        row_ptr = torch.empty((M + 1,), dtype=torch.int32, device=dev)
        perm = torch.empty((T,), dtype=torch.int32, device=dev)
        info = torch.empty((4,), dtype=torch.int64, device=dev)
        _call("svoxt_row_plan_build", _ptr(row), T, M, _ptr(row_ptr), _ptr(perm), _ptr(info), _ptr(ws), nbytes, _stream(dev))
        n_outside, longest, n_long, n_chunks = (int(v) for v in info.tolist())         # the one host read
        long_rows = torch.empty((n_long,), dtype=torch.int32, device=dev)
        long_chunk_ptr = torch.empty((n_long + 1,), dtype=torch.int32, device=dev)
        chunk_long = torch.empty((n_chunks,), dtype=torch.int32, device=dev)
        _call("svoxt_row_plan_long", _ptr(row_ptr), T, M, n_long, n_chunks, _ptr(ws), nbytes, _ptr(long_rows), _ptr(long_chunk_ptr),
              _ptr(chunk_long), _stream(dev))
    ROW_PLAN_BUILDS += 1
    return RowPlanArrays(row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, T, M, n_outside, longest)


def _check_cols(cols, K, dev):
    """cols: None or int32 [K'] with 1 <= K' <= K on `dev`; returns the number of selected columns."""
    if cols is None:
        return K
    if not isinstance(cols, torch.Tensor) or cols.dtype != torch.int32 or cols.dim() != 1 or cols.numel() == 0 or cols.shape[0] > K:
        raise RuntimeError("cols must be int32 [K'] distinct columns, 1 <= K' <= K")
    _check_input(cols, "cols")
    if cols.device != dev:
        raise RuntimeError("cols must be on the device of the table")
    return cols.shape[0]


def sample_gather_rows(table: torch.Tensor, row: torch.Tensor, cols=None) -> torch.Tensor:
    """out float32 [T, C] of svoxt_gather_rows: out[k, j] = table[row[k], cols[j]], zeros where row[k] is outside [0, M).
    table float32 [M, K] contiguous, row int32 [T], cols int32 [C] or None (all K)."""
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] < 1:
        raise RuntimeError("table must be float32 [M, K], K >= 1")
    if not isinstance(row, torch.Tensor) or row.dtype != torch.int32 or row.dim() != 1:
        raise RuntimeError("row must be int32 [T]")
    _check_input(table, "table")
    _check_input(row, "row")
    dev = table.device
    if row.device != dev:
        raise RuntimeError("row must be on the device of the table")
    (M, K), T = table.shape, row.shape[0]
    C = _check_cols(cols, K, dev)
    with _on(dev):
        out = torch.empty((T, C), dtype=torch.float32, device=dev)
        _call("svoxt_gather_rows", _ptr(table), M, K, _ptr(row), T, _ptr(cols), 0 if cols is None else C, _ptr(out), _stream(dev))
    return out


def sample_reduce_rows(values: torch.Tensor, plan: RowPlanArrays, op: str = "sum", empty: float = 0.0, cols=None, K=None) -> torch.Tensor:
    """out float32 [M, K] of svoxt_reduce_rows for values float32 [T, C] over a plan.  Without cols K = C; with cols
    (int32 [C] distinct columns of a table of K columns) column j lands in out[:, cols[j]], everything else is 0."""
    if op not in ROWS_OPS:
        raise RuntimeError(f"op must be one of {sorted(ROWS_OPS)}")
    if not isinstance(plan, RowPlanArrays):
        raise RuntimeError("plan must be a row plan")
    T, M = plan.T, plan.M
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2 or values.shape[0] != T or values.shape[1] < 1:
        raise RuntimeError(f"values must be float32 [T, C] with T = {T} samples and C >= 1")
    _check_input(values, "values")
    dev = values.device
    if plan.row_ptr.device != dev:
        raise RuntimeError("values must be on the device of the plan")
    C = values.shape[1]
    if cols is None:
        K = C
    elif _check_cols(cols, int(K), dev) != C:
        raise RuntimeError("values must have one column per selected column")
    with _on(dev):
        out = torch.empty((M, K), dtype=torch.float32, device=dev)
        nbytes = _lib.svoxt_reduce_rows_workspace_bytes(plan.chunk_long.shape[0], C)
        ws = _workspace(dev, nbytes, "reduce_rows: chunks * C must be below 2^38")
        _call("svoxt_reduce_rows", _ptr(values), T, C, *_plan_args(plan), _ptr(cols), 0 if cols is None else C, int(K),
              ROWS_OPS[op], float(empty), _ptr(out), _ptr(ws), nbytes, _stream(dev))
    return out


# ---------------------------------------------------------------------------
# The deterministic render backward (svoxt_rowgrad.hip; not in the reference)
# ---------------------------------------------------------------------------
ROWGRAD_LAST = {}             # what the last call allocated and found: Q, T, bytes, per-sample bytes, n_long, n_chunks, longest


def volume_render_backward_rows(tree: TreeSpec, rays: RaysSpec, opt: RenderOptions, grad_output: torch.Tensor, grad=None,
                                timers=None) -> torch.Tensor:
    """[M, K] gradient of volume_render (grad_output [Q, C + 1]) or opacity_render (grad_output [Q, 1]) with respect to
    the feature table, bit-identical from run to run: every sample's contribution has the arithmetic of
    volume_render_backward's generic kernel, and a table entry is their sum in svoxt_reduce_rows' order over the row plan
    of the batch's sample lists (include/svoxt.h, svoxt_render_grad_rows_*).  The bits depend on the tree, the features,
    the rays in index order, the options and grad_output -- not on RaysSpec.sort, an image hint, list capacities or pools.
    Two host reads (the number of samples, the plan's info record); 2^31 samples or more raise before anything is
    allocated for them.  transformation_matrices are not served.  `grad`: a float32 [M, >= K] buffer to write into (its
    first K columns; the rest is not touched) instead of a new tensor.  `timers`: a function called with a step's name
    before each of the five steps (measurement scripts)."""
    import svox_t_amd.csrc as csrc
    if _numel(tree.transformation_matrices):
        raise RuntimeError("volume_render_backward_rows: transformation_matrices are not served by the deterministic backward "
                           "(deterministic=True); use the default backward")
    _check_input(grad_output, "grad_output")
    Q = _spec_ray_count(rays)
    if grad_output.dtype != torch.float32 or grad_output.dim() != 2 or grad_output.shape[0] != Q:
        raise RuntimeError(f"grad_output must be float32 [Q, C + 1] (or [Q, 1]) with Q = {Q} rays")
    cols = grad_output.shape[1]
    M, K = tree.features.shape
    want = get_out_data_dim(opt, K)
    if cols != 1 and cols != want:
        raise RuntimeError(f"grad_output must have {want} columns (get_out_data_dim), or 1 for the opacity backward")
    C = cols - 1
    bd = int(opt.basis_dim) if (int(opt.format) != 0 and C > 0) else 0
    # (any walk gives the same lists: the coherent one marches fastest)
    rr = rays if isinstance(rays, CameraSpec) else csrc._in_coherent_order(tree, rays, opt)[0]
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rr), _pack_opts(opt)
    dev = tree.features.device
    tick = timers if timers is not None else (lambda _name: None)
    with _on(dev):
        stride = 0
        if grad is None:
            grad = torch.empty((M, K), dtype=torch.float32, device=dev)
        else:
            if not isinstance(grad, torch.Tensor) or grad.dtype != torch.float32 or grad.dim() != 2 or grad.shape[0] != M \
                    or grad.shape[1] < K or not grad.is_contiguous() or grad.device != dev:
                raise RuntimeError("grad must be a contiguous float32 [M, >= K] tensor on the device of the features")
            stride = grad.shape[1]
        T = 0
        offsets = None
        tick("count")
        if Q > 0:
            offsets = torch.empty((Q + 1,), dtype=torch.int64, device=dev)
            cws = _workspace(dev, _lib.svoxt_ray_samples_workspace_bytes(Q), "deterministic backward: the batch must have fewer than 2^31 rays")
            _call("svoxt_render_grad_rows_count", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), _ptr(offsets), _ptr(cws),
                  cws.numel(), _stream(dev))
            T = int(offsets[Q].item())                  # host read 1
            if T >= 1 << 31:
                raise RuntimeError(f"deterministic backward: {T} samples; a batch's lists hold fewer than 2^31 (split the batch)")
        nbytes = _lib.svoxt_render_grad_rows_workspace_bytes(Q, T, M, K, C, bd)
        ws = _workspace(dev, nbytes, "deterministic backward: T * (C + 1) and M * K must be below 2^38") if T > 0 else None
        args = (ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), _ptr(offsets), T, _ptr(grad_output), cols)
        n_long = n_chunks = longest = 0
        if T > 0:
            tick("emit")
            _call("svoxt_render_grad_rows_emit", *args, _ptr(ws), nbytes, _stream(dev))
            tick("plan")
            info = torch.empty((4,), dtype=torch.int64, device=dev)
            _call("svoxt_render_grad_rows_plan", *args, _ptr(info), _ptr(ws), nbytes, _stream(dev))
            tick("sweep")
            _call("svoxt_render_grad_rows_sweep", *args, _ptr(ws), nbytes, _stream(dev))      # (queued in front of the read)
            _, longest, n_long, n_chunks = (int(v) for v in info.tolist())        # host read 2
        tick("reduce")
        _call("svoxt_render_grad_rows_reduce", *args, n_long, n_chunks, _ptr(grad), stride, _ptr(ws), nbytes, _stream(dev))
        tick(None)
    ROWGRAD_LAST.update(Q=Q, T=T, bytes=int(nbytes), n_long=n_long, n_chunks=n_chunks, longest=longest)
    return grad


ROWHESS_LAST = {}             # ROWGRAD_LAST's record for the last volume_render_hess_rows


def _rows_out_table(t, name, M, K, dev):
    """(tensor, row stride for the C ABI) of an [M, >= K] output table: a new [M, K] one, or the caller's buffer."""
    if t is None:
        return torch.empty((M, K), dtype=torch.float32, device=dev), 0
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != M or t.shape[1] < K \
            or not t.is_contiguous() or t.device != dev:
        raise RuntimeError(f"{name} must be a contiguous float32 [M, >= K] tensor on the device of the features")
    return t, t.shape[1]


def volume_render_hess_rows(tree: TreeSpec, rays: RaysSpec, opt: RenderOptions, grad_output: torch.Tensor, curvature: torch.Tensor,
                            grad=None, hess=None, timers=None):
    """(grad, hess), both float32 [M, K]: volume_render_backward_rows' gradient for grad_output [Q, C + 1] (or [Q, 1]: the
    opacity render, C = 0) with its bits, and next to it the Gauss-Newton diagonal of a per-pixel separable loss whose
    second derivative in each output is curvature [Q, C + 1]:

        hess[m, j] = sum over the samples k naming row m and the outputs c of curvature[ray(k), c] * J(k, c, j)^2

    with J the derivative of out[ray(k), c] in entry j of row m through sample k alone (include/svoxt.h,
    svoxt_render_hess_rows_*, has the float32 sequence).  The squares are per sample: the exact diagonal whenever no ray
    names a row twice, the svox family's approximation where rows are shared (after refine, merge, quantize).  One
    march, one row plan and one shade serve both tables; no float atomic, the same bits in every run and whatever
    RaysSpec.sort or an image hint say.  Two host reads, as volume_render_backward_rows.  transformation_matrices are not
    served.  `grad`, `hess`: float32 [M, >= K] buffers to write into (their first K columns).  `timers`: a function
    called with a step's name before each of the five steps."""
    import svox_t_amd.csrc as csrc
    if _numel(tree.transformation_matrices):
        raise RuntimeError("volume_render_hess_rows: transformation_matrices are not served by the deterministic backward "
                           "(deterministic=True); use the default backward")
    _check_input(grad_output, "grad_output")
    _check_input(curvature, "curvature")
    Q = _spec_ray_count(rays)
    if grad_output.dtype != torch.float32 or grad_output.dim() != 2 or grad_output.shape[0] != Q:
        raise RuntimeError(f"grad_output must be float32 [Q, C + 1] (or [Q, 1]) with Q = {Q} rays")
    if curvature.dtype != torch.float32 or tuple(curvature.shape) != tuple(grad_output.shape) or curvature.device != grad_output.device:
        raise RuntimeError("curvature must be float32 with the shape and device of grad_output")
    cols = grad_output.shape[1]
    M, K = tree.features.shape
    want = get_out_data_dim(opt, K)
    if cols != 1 and cols != want:
        raise RuntimeError(f"grad_output must have {want} columns (get_out_data_dim), or 1 for the opacity render")
    C = cols - 1
    bd = int(opt.basis_dim) if (int(opt.format) != 0 and C > 0) else 0
    rr = rays if isinstance(rays, CameraSpec) else csrc._in_coherent_order(tree, rays, opt)[0]
    ct, cr, co = _pack_tree_accel(tree), _pack_rays(rr), _pack_opts(opt)
    dev = tree.features.device
    tick = timers if timers is not None else (lambda _name: None)
    with _on(dev):
        grad, gstride = _rows_out_table(grad, "grad", M, K, dev)
        hess, hstride = _rows_out_table(hess, "hess", M, K, dev)
        if grad.data_ptr() == hess.data_ptr() and M > 0:
            raise RuntimeError("grad and hess must be distinct tensors")
        T = 0
        offsets = None
        tick("count")
        if Q > 0:
            offsets = torch.empty((Q + 1,), dtype=torch.int64, device=dev)
            cws = _workspace(dev, _lib.svoxt_ray_samples_workspace_bytes(Q), "se_grad: the batch must have fewer than 2^31 rays")
            _call("svoxt_render_grad_rows_count", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), _ptr(offsets), _ptr(cws),
                  cws.numel(), _stream(dev))
            T = int(offsets[Q].item())                  # host read 1
            if T >= 1 << 31:
                raise RuntimeError(f"se_grad: {T} samples; a batch's lists hold fewer than 2^31 (split the batch)")
        nbytes = _lib.svoxt_render_hess_rows_workspace_bytes(Q, T, M, K, C, bd)
        ws = _workspace(dev, nbytes, "se_grad: T * (C + 1) and M * K must be below 2^38") if T > 0 else None
        lead = (ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), _ptr(offsets), T, _ptr(grad_output))
        n_long = n_chunks = longest = 0
        if T > 0:
            tick("emit")
            _call("svoxt_render_grad_rows_emit", *lead, cols, _ptr(ws), nbytes, _stream(dev))
            tick("plan")
            info = torch.empty((4,), dtype=torch.int64, device=dev)
            _call("svoxt_render_grad_rows_plan", *lead, cols, _ptr(info), _ptr(ws), nbytes, _stream(dev))
            tick("sweep")
            _call("svoxt_render_hess_rows_sweep", *lead, _ptr(curvature), cols, _ptr(ws), nbytes, _stream(dev))   # (queued in front of the read)
            _, longest, n_long, n_chunks = (int(v) for v in info.tolist())        # host read 2
        tick("reduce")
        _call("svoxt_render_hess_rows_reduce", *lead, _ptr(curvature), cols, n_long, n_chunks, _ptr(grad), gstride, _ptr(hess), hstride,
              _ptr(ws), nbytes, _stream(dev))
        tick(None)
    ROWHESS_LAST.update(Q=Q, T=T, bytes=int(nbytes), n_long=n_long, n_chunks=n_chunks, longest=longest)
    return grad, hess


# ---------------------------------------------------------------------------
# shade_samples: per-sample colours from feature rows (svoxt_shade.hip; not in the reference)
# ---------------------------------------------------------------------------
def view_basis(tree: TreeSpec, rays, opt: RenderOptions) -> torch.Tensor:
    """basis float32 [Q, basis_dim] of svoxt_view_basis: every ray's basis values as the render kernels form them; [Q, 0]
    for RGBA.  `rays`: a RaysSpec or a CameraSpec.  transformation_matrices are not served."""
    if _numel(tree.transformation_matrices):
        raise RuntimeError("view_basis: transformation_matrices are not served by shade_samples (the per-leaf rotation of "
                           "the view direction); use forward")
    ct, cr, co = _pack_tree(tree), _pack_rays(rays), _pack_opts(opt)
    dev = tree.features.device
    bd = 0 if int(opt.format) == 0 else int(opt.basis_dim)
    with _on(dev):
        basis = torch.empty((cr.Q, bd), dtype=torch.float32, device=dev)
        _call("svoxt_view_basis", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), _ptr(basis), _stream(dev))
    return basis


def _shade_dims(opt: RenderOptions, K: int):
    """(C, basis_dim or 0 for RGBA) of a table of K columns under `opt`."""
    C = get_out_data_dim(opt, K) - 1
    return C, (0 if int(opt.format) == 0 else int(opt.basis_dim))


def _check_basis(x, name, Q, bd, dev, where, device_refusal=None):
    """x must be float32 [Q, basis_dim] on `dev`; `where` ends the refusal, `device_refusal` is a text of its own for the device."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != (Q, bd) \
            or (device_refusal is None and x.device != dev):
        raise RuntimeError(f"{name} must be float32 [Q, basis_dim] = [{Q}, {bd}] {where}")
    _check_input(x, name)
    if x.device != dev:
        raise RuntimeError(device_refusal)


def _check_grads(values, grad_values, grad_sigma, T, dev, C):
    """The forward's values [T, C] and the upstream gradients grad_values [T, C] / grad_sigma [T], either None for zeros."""
    _check_per_sample(values, "values", T, dev, C)
    if grad_values is not None:
        _check_per_sample(grad_values, "grad_values", T, dev, C)
    if grad_sigma is not None:
        _check_per_sample(grad_sigma, "grad_sigma", T, dev)


def _check_shade(features, row, ray, basis, Q, opt, with_basis=True):
    """The sample side every direction of shade_samples checks: features float32 [M, K], or the (M, K) of a table whose values
    are not read; row / ray int32 [T]; the plain forward's basis; the 2^31 limits.  Returns (M, K, T, C, basis_dim, device)."""
    dev = None
    if not isinstance(features, tuple):
        if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] < 1:
            raise RuntimeError("features must be float32 [M, K], K >= 1")
        _check_input(features, "features")
        dev = features.device
        features = features.shape
    M, K = (int(v) for v in features)
    if not isinstance(row, torch.Tensor) or row.dtype != torch.int32 or row.dim() != 1:
        raise RuntimeError("row must be int32 [T]")
    T, dev = row.shape[0], (row.device if dev is None else dev)
    _check_per_sample(row, "row", T, dev, dtype=torch.int32)
    _check_per_sample(ray, "ray", T, dev, dtype=torch.int32)
    C, bd = _shade_dims(opt, K)
    if bd > 0 and with_basis:
        _check_basis(basis, "basis", Q, bd, dev, "(view_basis of the samples' rays)", "basis must be on the device of the features")
    if M >= 1 << 31 or T >= 1 << 31 or Q >= 1 << 31:
        raise RuntimeError("M, T and Q must be below 2^31")
    return M, K, T, C, bd, dev


def _shade_fwd(entry, features, dims, view, opt, activate):
    """(values, sigma) of the forward `entry`, plain or rotated: `view` is what the entry point takes between the options and
    `activate` (the lists and the view side)."""
    M, K, T, C, _, dev = dims
    co = _pack_opts(opt)
    with _on(dev):
        values = torch.empty((T, C), dtype=torch.float32, device=dev)
        sigma = torch.empty((T,), dtype=torch.float32, device=dev)
        _call(entry, _ptr(features), M, K, ctypes.byref(co), *view, 1 if activate else 0, _ptr(values), _ptr(sigma), _stream(dev))
    return values, sigma


def _shade_bwd(entry, M, K, dev, view, opt, activate, values, grad_values, grad_sigma, plan):
    """grad float32 [M, K] of the table backward `entry`, plain or rotated: `view` as in _shade_fwd."""
    co = _pack_opts(opt)
    with _on(dev):
        grad = torch.empty((M, K), dtype=torch.float32, device=dev)
        nbytes = _lib.svoxt_shade_samples_bwd_workspace_bytes(plan.chunk_long.shape[0], K)
        ws = _workspace(dev, nbytes, "shade_samples: chunks * K must be below 2^38")
        _call(entry, ctypes.byref(co), M, K, *view, 1 if activate else 0, _ptr(values), _ptr(grad_values), _ptr(grad_sigma),
              *_plan_args(plan, with_M=False), _ptr(grad), _ptr(ws), nbytes, _stream(dev))
    return grad


def shade_samples_fwd(features, row, ray, basis, Q: int, opt: RenderOptions, activate: bool = True):
    """(values float32 [T, C], sigma float32 [T]) of svoxt_shade_samples_fwd for features float32 [M, K], row / ray int32 [T]
    and basis float32 [Q, basis_dim] (RGBA: not read, may be None)."""
    dims = _check_shade(features, row, ray, basis, Q, opt)
    view = (_ptr(row), _ptr(ray), dims[2], _ptr(basis) if dims[4] > 0 else None, Q)
    return _shade_fwd("svoxt_shade_samples_fwd", features, dims, view, opt, activate)


def shade_samples_bwd(shape, ray, basis, Q: int, opt: RenderOptions, activate: bool, values, grad_values, grad_sigma,
                      plan: RowPlanArrays) -> torch.Tensor:
    """grad float32 [M, K] of svoxt_shade_samples_bwd for a table of `shape` = (M, K) over the samples' row plan; values is
    the forward's output, grad_values [T, C] / grad_sigma [T] may be None (zeros)."""
    if not isinstance(plan, RowPlanArrays):
        raise RuntimeError("plan must be a row plan")
    M, K = (int(v) for v in shape)
    T = plan.T
    if plan.M != M:
        raise RuntimeError("the plan must be built for the table's M rows")
    C, bd = _shade_dims(opt, K)
    dev = plan.row_ptr.device
    _check_per_sample(ray, "ray", T, dev, dtype=torch.int32)
    _check_grads(values, grad_values, grad_sigma, T, dev, C)
    if bd > 0:
        _check_basis(basis, "basis", Q, bd, dev, "on the device of the plan")
    view = (_ptr(ray), T, _ptr(basis) if bd > 0 else None, Q)
    return _shade_bwd("svoxt_shade_samples_bwd", M, K, dev, view, opt, activate, values, grad_values, grad_sigma, plan)


def view_basis_backward(tree: TreeSpec, rays, opt: RenderOptions, basis, grad_basis) -> torch.Tensor:
    """grad_viewdirs float32 [Q, 3] of svoxt_view_basis_bwd for grad_basis float32 [Q, basis_dim] and `basis`, view_basis'
    own output for these rays (read for SG).  `rays`: a RaysSpec with explicit viewdirs; RGBA: zeros."""
    if _numel(tree.transformation_matrices):
        raise RuntimeError("view_basis: transformation_matrices are not served by shade_samples (the per-leaf rotation of "
                           "the view direction); use forward")
    ct, cr, co = _pack_tree(tree), _pack_rays(rays), _pack_opts(opt)
    dev = tree.features.device
    Q = int(cr.Q)
    bd = 0 if int(opt.format) == 0 else int(opt.basis_dim)
    if bd == 0:
        return torch.zeros((Q, 3), dtype=torch.float32, device=dev)
    _check_basis(basis, "basis", Q, bd, dev, "on the device of the tree")
    _check_basis(grad_basis, "grad_basis", Q, bd, dev, "on the device of the tree")
    with _on(dev):
        gv = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        _call("svoxt_view_basis_bwd", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), _ptr(basis), _ptr(grad_basis), _ptr(gv),
              _stream(dev))
    return gv


def shade_samples_bwd_basis(features, offsets, row, ray, Q: int, opt: RenderOptions, activate: bool, values, grad_values) -> torch.Tensor:
    """grad_basis float32 [Q, basis_dim] of svoxt_shade_samples_bwd_basis for features float32 [M, K] over the lists (offsets
    int64 [Q + 1], row / ray int32 [T]); values is the forward's output, grad_values [T, C] may be None (zeros).  RGBA: an
    empty [Q, 0] tensor, no kernel."""
    M, K, T, C, bd, dev = _check_shade(features, row, ray, None, Q, opt, with_basis=False)
    if _check_csr(offsets, T) != Q:
        raise RuntimeError(f"offsets must be int64 [Q + 1] with Q = {Q}")
    if offsets.device != dev:
        raise RuntimeError("offsets must be on the device of the features")
    _check_grads(values, grad_values, None, T, dev, C)
    co = _pack_opts(opt)
    with _on(dev):
        gb = torch.empty((Q, bd), dtype=torch.float32, device=dev)
        if bd > 0:
            _call("svoxt_shade_samples_bwd_basis", _ptr(features), M, K, ctypes.byref(co), _ptr(offsets), _ptr(row), _ptr(ray), T, Q,
                  1 if activate else 0, _ptr(values), _ptr(grad_values), _ptr(gb), _stream(dev))
    return gb


# ---------------------------------------------------------------------------
# shade_samples with per-row rotations of the view direction (svoxt_viewrot.hip)
# ---------------------------------------------------------------------------
def _is_rotations(x) -> bool:
    """float32 [M, 3, 3] or [M, 4, 4]: one matrix per feature row"""
    return isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 3 and tuple(x.shape[1:]) in ((3, 3), (4, 4))


def _check_rot(features, row, ray, rotations, viewdirs, extra, Q, opt):
    """The checks the rotated call's directions share; `features`: a table or its (M, K), as _check_shade takes it.  Returns
    ((M, K, T, C, basis_dim, device), view), view what the C ABI takes of the view side and the lists: extra, extra_rows,
    extra_cols, rotations, rot_dim, viewdirs, Q, row, ray, T."""
    if int(opt.format) == 0:
        raise RuntimeError("rotations: RGBA has no basis to rotate (shade_samples_fwd serves it)")
    M, K, T, C, bd, dev = dims = _check_shade(features, row, ray, None, Q, opt, with_basis=False)
    if not _is_rotations(rotations) or rotations.shape[0] != M:
        raise RuntimeError(f"rotations must be float32 [M, 3, 3] or [M, 4, 4] with M = {M}, one matrix per feature row")
    if not isinstance(viewdirs, torch.Tensor) or viewdirs.dtype != torch.float32 or tuple(viewdirs.shape) != (Q, 3):
        raise RuntimeError(f"viewdirs must be float32 [Q, 3] with Q = {Q}")
    for name, x in (("rotations", rotations), ("viewdirs", viewdirs)):
        _check_input(x, name)
        if x.device != dev:
            raise RuntimeError(f"{name} must be on the device of the features")
    rows = cols = 0
    if int(opt.format) in (2, 3):
        if not isinstance(extra, torch.Tensor) or extra.dtype != torch.float32 or extra.dim() != 2 or extra.device != dev:
            raise RuntimeError("SG / ASG need the lobes: extra float32 [basis_dim, >= 4 / 11] on the device of the features")
        _check_input(extra, "extra")
        rows, cols = extra.shape
    else:
        extra = None
    return dims, (_ptr(extra), rows, cols, _ptr(rotations), rotations.shape[1], _ptr(viewdirs), Q, _ptr(row), _ptr(ray), T)


def shade_rot_fwd(features, row, ray, rotations, viewdirs, extra, Q: int, opt: RenderOptions, activate: bool = True):
    """(values float32 [T, C], sigma float32 [T]) of svoxt_shade_rot_fwd: shade_samples_fwd with the basis of rotations[row] *
    viewdirs[ray].  rotations float32 [M, 3, 3] or [M, 4, 4], viewdirs float32 [Q, 3], extra: the lobes of SG / ASG."""
    dims, view = _check_rot(features, row, ray, rotations, viewdirs, extra, Q, opt)
    return _shade_fwd("svoxt_shade_rot_fwd", features, dims, view, opt, activate)


def shade_rot_bwd(shape, row, ray, rotations, viewdirs, extra, Q: int, opt: RenderOptions, activate: bool, values, grad_values,
                  grad_sigma, plan: RowPlanArrays) -> torch.Tensor:
    """grad float32 [M, K] of svoxt_shade_rot_bwd for a table of `shape` = (M, K) over the samples' row plan (the table's
    values are not read); values is the forward's output, grad_values [T, C] / grad_sigma [T] may be None (zeros)."""
    if not isinstance(plan, RowPlanArrays):
        raise RuntimeError("plan must be a row plan")
    (M, K, T, C, _, dev), view = _check_rot(tuple(shape), row, ray, rotations, viewdirs, extra, Q, opt)
    if plan.M != M or plan.T != T:
        raise RuntimeError("the plan must be built for the table's M rows and the T samples")
    _check_grads(values, grad_values, grad_sigma, T, dev, C)
    return _shade_bwd("svoxt_shade_rot_bwd", M, K, dev, view, opt, activate, values, grad_values, grad_sigma, plan)


def shade_rot_bwd_dir(features, row, ray, rotations, viewdirs, extra, Q: int, opt: RenderOptions, activate: bool, values,
                      grad_values) -> torch.Tensor:
    """gu float32 [T, 3] of svoxt_shade_rot_bwd_dir: the gradient in every sample's rotated direction, the one scratch the
    gradients in the rotations and in the view directions read; grad_values [T, C] may be None (zeros)."""
    (M, K, T, C, _, dev), view = _check_rot(features, row, ray, rotations, viewdirs, extra, Q, opt)
    _check_grads(values, grad_values, None, T, dev, C)
    co = _pack_opts(opt)
    with _on(dev):
        gu = torch.empty((T, 3), dtype=torch.float32, device=dev)
        _call("svoxt_shade_rot_bwd_dir", _ptr(features), M, K, ctypes.byref(co), *view, 1 if activate else 0, _ptr(values), _ptr(grad_values),
              _ptr(gu), _stream(dev))
    return gu


def shade_rot_bwd_rotations(gu, viewdirs, ray, shape, plan: RowPlanArrays) -> torch.Tensor:
    """grad_rotations float32 of `shape` = (M, d, d) of svoxt_shade_rot_bwd_rotations: grad[m, a, b] = the sum of gu[k, a] *
    viewdirs[ray[k], b] over the row plan; zeros outside the 3 x 3 block of a 4 x 4."""
    if not isinstance(plan, RowPlanArrays):
        raise RuntimeError("plan must be a row plan")
    M, d, d2 = (int(v) for v in shape)
    T = plan.T
    if plan.M != M or d != d2 or d not in (3, 4):
        raise RuntimeError("the plan must be built for the M matrices of [M, 3, 3] or [M, 4, 4]")
    dev = plan.row_ptr.device
    _check_per_sample(gu, "gu", T, dev, 3)
    _check_per_sample(ray, "ray", T, dev, dtype=torch.int32)
    if not isinstance(viewdirs, torch.Tensor) or viewdirs.dtype != torch.float32 or viewdirs.dim() != 2 or viewdirs.shape[1] != 3 \
            or viewdirs.device != dev:
        raise RuntimeError("viewdirs must be float32 [Q, 3] on the device of the plan")
    _check_input(viewdirs, "viewdirs")
    with _on(dev):
        grad = torch.empty((M, d, d), dtype=torch.float32, device=dev)
        nbytes = _lib.svoxt_shade_samples_bwd_workspace_bytes(plan.chunk_long.shape[0], d * d)
        ws = _workspace(dev, nbytes, "shade_samples: chunks must be below 2^31")
        _call("svoxt_shade_rot_bwd_rotations", _ptr(gu), _ptr(viewdirs), viewdirs.shape[0], _ptr(ray), T, M, d,
              *_plan_args(plan, with_M=False), _ptr(grad), _ptr(ws), nbytes, _stream(dev))
    return grad


def shade_rot_bwd_viewdirs(gu, rotations, offsets, row, ray) -> torch.Tensor:
    """grad_viewdirs float32 [Q, 3] of svoxt_shade_rot_bwd_viewdirs: per ray, over its segment in list order,
    acc[b] += rotations[row[k], a, b] * gu[k, a]; zeros for a ray without samples."""
    if not isinstance(row, torch.Tensor) or row.dtype != torch.int32 or row.dim() != 1:
        raise RuntimeError("row must be int32 [T]")
    T = row.shape[0]
    Q = _check_csr(offsets, T)
    dev = offsets.device
    _check_per_sample(row, "row", T, dev, dtype=torch.int32)
    _check_per_sample(ray, "ray", T, dev, dtype=torch.int32)
    _check_per_sample(gu, "gu", T, dev, 3)
    if not _is_rotations(rotations) or rotations.device != dev:
        raise RuntimeError("rotations must be float32 [M, 3, 3] or [M, 4, 4] on the device of offsets")
    _check_input(rotations, "rotations")
    with _on(dev):
        gv = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        _call("svoxt_shade_rot_bwd_viewdirs", _ptr(gu), _ptr(rotations), rotations.shape[1], rotations.shape[0], _ptr(offsets), _ptr(row),
              _ptr(ray), T, Q, _ptr(gv), _stream(dev))
    return gv


# ---------------------------------------------------------------------------
# interp: a trilinear lookup over the leaves around a point (svoxt_interp.hip; not in the reference)
# ---------------------------------------------------------------------------
INTERP_FILLS = {"self": 0, "zero": 1}                             # SVOXT_INTERP_FILL_* (include/svoxt.h)
INTERP_MAX_Q = (1 << 28) - 1                                      # 8 Q < 2^31: the plan's entries are int32


def _check_stencil(rows, weights, dev=None, shapes_only=False):
    """rows int32 [Q, 8] and weights float32 [Q, 8] (shapes_only: that alone), contiguous, on one GPU (`dev` if given);
    returns Q."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 8:
        raise RuntimeError("rows must be int32 [Q, 8]")
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != tuple(rows.shape):
        raise RuntimeError("weights must be float32 [Q, 8], one entry per entry of rows")
    if rows.shape[0] > INTERP_MAX_Q:
        raise RuntimeError("interp: the number of points must be below 2^28 (8 Q < 2^31)")
    if shapes_only:
        return rows.shape[0]
    _check_input(rows, "rows")
    _check_input(weights, "weights")
    if weights.device != rows.device or (dev is not None and rows.device != dev):
        raise RuntimeError("rows and weights must be on one device, the table's")
    return rows.shape[0]


def _check_points(indices):
    """indices float32 [Q, 3]: shape and dtype (checked before any device by the callers)."""
    if not isinstance(indices, torch.Tensor) or indices.dtype != torch.float32 or indices.dim() != 2 or indices.shape[1] != 3:
        raise RuntimeError("indices must be float32 [Q, 3]")


def _check_table(table, name="table"):
    """table float32 [M, K], K >= 1: shape and dtype (checked before any device by the callers); returns (M, K)."""
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] < 1:
        raise RuntimeError(f"{name} must be float32 [M, K], K >= 1")
    return table.shape


def interp_stencil(tree: TreeSpec, indices: torch.Tensor, fill: str = "self"):
    """(rows int32 [Q, 8], weights float32 [Q, 8]) of svoxt_interp_stencil for the points indices float32 [Q, 3]: per
    point the feature rows of the eight cells around it at its leaf's level and their trilinear weights (include/svoxt.h,
    "interp").  tree.features decides M alone: which data words name a row."""
    if fill not in INTERP_FILLS:
        raise RuntimeError(f"fill must be one of {sorted(INTERP_FILLS)}")
    _check_points(indices)
    if indices.shape[0] > INTERP_MAX_Q:
        raise RuntimeError("interp: the number of points must be below 2^28 (8 Q < 2^31)")
    _check_indices(indices)
    ct = _pack_tree(tree)
    dev = indices.device
    if tree.features.device != dev:
        raise RuntimeError("indices must be on the device of the tree")
    Q = indices.shape[0]
    with _on(dev):
        rows = torch.empty((Q, 8), dtype=torch.int32, device=dev)
        weights = torch.empty((Q, 8), dtype=torch.float32, device=dev)
        _call("svoxt_interp_stencil", ctypes.byref(ct), _ptr(indices), Q, INTERP_FILLS[fill], _ptr(rows), _ptr(weights), _stream(dev))
    return rows, weights


def interp_rows_fwd(table: torch.Tensor, rows: torch.Tensor, weights: torch.Tensor, cols=None) -> torch.Tensor:
    """out float32 [Q, C] of svoxt_interp_rows_fwd: out[q, jc] = sum_j weights[q, j] * table[rows[q, j], cols[jc]] in ascending
    j, corners with a row outside [0, M) skipped."""
    M, K = _check_table(table)
    _check_stencil(rows, weights, shapes_only=True)
    _check_input(table, "table")
    dev = table.device
    Q = _check_stencil(rows, weights, dev)
    C = _check_cols(cols, K, dev)
    with _on(dev):
        out = torch.empty((Q, C), dtype=torch.float32, device=dev)
        _call("svoxt_interp_rows_fwd", _ptr(table), M, K, _ptr(rows), _ptr(weights), Q, _ptr(cols), 0 if cols is None else C, _ptr(out),
              _stream(dev))
    return out


def interp_rows_bwd(grad_out: torch.Tensor, weights: torch.Tensor, plan: RowPlanArrays, cols=None, K=None) -> torch.Tensor:
    """grad float32 [M, K] of svoxt_interp_rows_bwd for grad_out float32 [Q, C] over the row plan of the stencil's rows
    viewed as [8 Q]: every element written, reduce_rows' order, no [8 Q, C] tensor."""
    if not isinstance(plan, RowPlanArrays):
        raise RuntimeError("plan must be a row plan")
    M = plan.M
    dev = plan.row_ptr.device
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.dim() != 2 or weights.shape[1] != 8 \
            or 8 * weights.shape[0] != plan.T:
        raise RuntimeError("weights must be float32 [Q, 8] with 8 Q the entries of the plan")
    Q = weights.shape[0]
    if not isinstance(grad_out, torch.Tensor) or grad_out.dtype != torch.float32 or grad_out.dim() != 2 or grad_out.shape[0] != Q \
            or grad_out.shape[1] < 1:
        raise RuntimeError(f"grad_out must be float32 [Q, C] with Q = {Q} points and C >= 1")
    _check_input(weights, "weights")
    _check_input(grad_out, "grad_out")
    if weights.device != dev or grad_out.device != dev:
        raise RuntimeError("grad_out and weights must be on the device of the plan")
    C = grad_out.shape[1]
    if cols is None:
        K = C
    elif _check_cols(cols, int(K), dev) != C:
        raise RuntimeError("grad_out must have one column per selected column")
    with _on(dev):
        grad = torch.empty((M, int(K)), dtype=torch.float32, device=dev)
        nbytes = _lib.svoxt_interp_rows_bwd_workspace_bytes(plan.chunk_long.shape[0], C)
        ws = _workspace(dev, nbytes, "interp: chunks * C must be below 2^38")
        _call("svoxt_interp_rows_bwd", _ptr(grad_out), _ptr(weights), Q, C, *_plan_args(plan), _ptr(cols), 0 if cols is None else C, int(K),
              _ptr(grad), _ptr(ws), nbytes, _stream(dev))
    return grad


def interp_points_bwd(tree: TreeSpec, indices: torch.Tensor, rows: torch.Tensor, table: torch.Tensor, grad_out: torch.Tensor,
                      cols=None) -> torch.Tensor:
    """grad_points float32 [Q, 3] of svoxt_interp_points_bwd: the derivative of interp_rows_fwd's value with respect to the
    points the stencil `rows` was built for (the tree spec's coordinates), for the upstream gradient grad_out [Q, C]."""
    _check_points(indices)
    M, K = _check_table(table)
    Q = indices.shape[0]
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or tuple(rows.shape) != (Q, 8):
        raise RuntimeError("rows must be int32 [Q, 8], the stencil of indices")
    C = K if cols is None else (cols.shape[0] if isinstance(cols, torch.Tensor) and cols.dim() == 1 else -1)
    if not isinstance(grad_out, torch.Tensor) or grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (Q, C):
        raise RuntimeError("grad_out must be float32 [Q, C], one column per selected column")
    _check_indices(indices)
    ct = _pack_tree(tree)
    _check_input(table, "table")
    dev = table.device
    _check_input(rows, "rows")
    _check_cols(cols, K, dev)
    _check_input(grad_out, "grad_out")
    if Q > INTERP_MAX_Q:
        raise RuntimeError("interp: the number of points must be below 2^28 (8 Q < 2^31)")
    if indices.device != dev or rows.device != dev or grad_out.device != dev or tree.features.device != dev:
        raise RuntimeError("indices, rows, grad_out and the tree must be on the device of the table")
    with _on(dev):
        grad = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        _call("svoxt_interp_points_bwd", ctypes.byref(ct), _ptr(indices), Q, _ptr(rows), _ptr(table), M, K, _ptr(cols),
              0 if cols is None else C, _ptr(grad_out), _ptr(grad), _stream(dev))
    return grad
