"""N3Tree: host-side owner of the sparse N^3-tree the HIP kernels traverse.

Mirrors the part of the reference's `svox_t.N3Tree` (svox_t/svox.py:78-158,
:216-285, :488-560, :829-925) that the volume-render hot path touches: the
buffers and their layout, `refine`, the point query with its autograd bridge,
and `_spec`, which packs the tensors for the operator boundary.

Layout (identical to the reference so trees interchange):
    features      float32 [M, data_dim]          nn.Parameter, the leaf feature table
    data          int32   [cap, N, N, N, 1]      per leaf slot: row of `features`; >= M means empty
    child         int32   [cap, N, N, N]         per slot: offset to the child node, 0 = leaf
    parent_depth  int32   [cap, 2]               packed parent slot, depth
    invradius, offset float32 [3]                world -> [0,1]^3 : p' = offset + invradius * p
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import autograd, nn

from svox_t_amd.helpers import DataFormat, LocalIndex, N3TreeView, _get_c_extension

_C = _get_c_extension()
_X = _C._extras            # (interp's wrappers are reached here, not as csrc.* names)

# int(1e10) as int32: the fill value of `data` in the reference (svox.py:124).
EMPTY_INDEX = 1410065408


class PruneResult(NamedTuple):
    """What N3Tree.prune did."""
    n_internal: int
    nodes_removed: int
    leaves_dropped: int            # leaves that held a feature row and were not kept
    row_map: Optional[torch.Tensor]


class QuantizeResult(NamedTuple):
    """What N3Tree.quantize did: the palette (the values of the new `features`) and the palette row of every old row."""
    colors: torch.Tensor
    color_id_map: torch.Tensor


class MergeResult(NamedTuple):
    """What N3Tree.merge did."""
    n_internal: int
    nodes_merged: int
    row_map: Optional[torch.Tensor]   # old row of every carried feature row (None without compact_features)
    rows_added: int                   # new feature rows, behind the carried ones


class SubdivideResult(NamedTuple):
    """What N3Tree.subdivide did."""
    n_internal: int
    nodes_added: int
    rows_added: int                   # new feature rows, behind the old ones
    row_map: Optional[torch.Tensor]   # old row of every new feature row (None without own_rows)


class UnshareResult(NamedTuple):
    """What N3Tree.unshare did."""
    rows_added: int
    row_map: torch.Tensor             # old row of every new feature row


class LeafBoxes(NamedTuple):
    """What N3Tree.leaf_boxes returns: every leaf slot in `_all_leaves()` order, on the tree's device."""
    leaf_node: torch.Tensor           # int64 [L, 4]: node, x, y, z
    corners: torch.Tensor             # float32 [L, 3]: lower corner
    lengths: torch.Tensor             # float32 [L, 3]: side lengths
    depths: torch.Tensor              # int32 [L]
    rows: torch.Tensor                # int64 [L]: the feature row the leaf names, -1 for an empty leaf


class LeafNeighbors(NamedTuple):
    """What N3Tree.leaf_neighbors returns: every leaf slot in `_all_leaves()` order, on the tree's device."""
    leaf_node: torch.Tensor           # int64 [L, 4]: node, x, y, z
    depths: torch.Tensor              # int32 [L]
    rows: torch.Tensor                # int64 [L]: the feature row the leaf names, -1 for an empty leaf
    neighbors: torch.Tensor           # int32 [L, 6]: leaf index across -x +x -y +y -z +z; -1 outside, -2 finer leaves


_ASSIGN_REDUCE = ("last", "sum", "mean", "max", "min")

_REDUCE_CALLABLES = {torch.mean: "mean", torch.sum: "sum", torch.max: "max", torch.min: "min"}


class _FrontierReduceFunction(autograd.Function):
    """reduce_frontier(grad=True): gradient flows to argument 0 (the feature table) only."""

    @staticmethod
    def forward(ctx, features, data, n, N, nodes, cols, op, empty):
        ctx.args = (data, n, N, nodes, cols, op, empty)
        ctx.save_for_backward(features)
        return _C.frontier_reduce(features.detach().contiguous(), data, n, N, nodes, cols, op, empty)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        data, n, N, nodes, cols, op, empty = ctx.args
        return (_C.frontier_reduce_backward(ctx.saved_tensors[0].detach().contiguous(), data, n, N, nodes, cols, op, empty,
                                            grad_out.contiguous()),) + (None,) * 7


class _TVFunction(autograd.Function):
    """N3Tree.tv: gradient flows to argument 0 (the feature table) only.  The forward's one kernel writes the loss and,
    where the table requires a gradient, G = d loss / d features; the backward is grad_out * G."""

    @staticmethod
    def forward(ctx, features, plan, cols, p, weight, mean):
        want = ctx.needs_input_grad[0]
        loss, G = _C.tv_rows(features.detach().contiguous(), plan, cols, p, weight, mean, "loss_grad" if want else "loss")
        ctx.G = G
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0] or ctx.G is None:
            return (None,) * 6
        return (grad_out * ctx.G,) + (None,) * 5


class _QueryVerticalFunction(autograd.Function):
    """svox_t/svox.py:38-56: gradient flows to argument 0 (the feature table) only."""

    @staticmethod
    def forward(ctx, data, tree_spec, indices):
        out, node_ids, data_ids, leaf_node = _C.query_vertical(tree_spec, indices)
        ctx.mark_non_differentiable(node_ids, data_ids, leaf_node)
        ctx.tree_spec = tree_spec
        ctx.save_for_backward(indices)
        return out, node_ids, data_ids, leaf_node

    @staticmethod
    def backward(ctx, grad_out, *_unused):
        if ctx.needs_input_grad[0]:
            return _C.query_vertical_backward(ctx.tree_spec, ctx.saved_tensors[0],
                                              grad_out.contiguous()), None, None
        return None, None, None


_INTERP_FILL = ("self", "zero")


class InterpStencil:
    """What N3Tree.interp_stencil returns: the eight feature rows and trilinear weights of every point (include/svoxt.h,
    "interp").

    rows     int32 [Q, 8]     corner j = 4 b_x + 2 b_y + b_z; corner 0 is the point's own leaf; -1: no row
    weights  float32 [Q, 8]   >= 0, summing to 1 within a few float32 roundings
    Neither is meant to be edited: a row plan built before an edit of `rows` describes the old rows."""

    def __init__(self, rows, weights):
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 8:
            raise RuntimeError("rows must be int32 [Q, 8]")
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != tuple(rows.shape):
            raise RuntimeError("weights must be float32 [Q, 8], one entry per entry of rows")
        self.rows, self.weights = rows, weights

    def __len__(self) -> int:
        return self.rows.shape[0]

    def __iter__(self):
        return iter((self.rows, self.weights))

    def row_plan(self, M: int):
        """The RowPlan (svox_t_amd.samples) of `rows` viewed as int32 [8 Q] for a table of M rows: for every row the
        entries e = 8 q + j that name it, in ascending e.  Built on the GPU with one host read, cached per M."""
        from svox_t_amd.samples import RowPlan
        M = _C._extras._check_rows_extent(M, "row_plan")
        if not self.rows.is_cuda:
            raise RuntimeError("row_plan: only the GPU (HIP) path exists; the stencil must be on the GPU")
        plans = self.__dict__.setdefault("_row_plans", {})
        if M not in plans:
            arrays = _C.row_plan(self.rows.contiguous().reshape(-1), M)
            plans[M] = _C._Produced("stencil_plan", RowPlan(arrays), arrays, self.rows.device)
        return plans[M].ready_on(_C._raw_stream(self.rows.device))   # (built on another stream: that stream waits for it)


class _InterpRowsFunction(autograd.Function):
    """interp_rows: gradient flows to argument 0 (the table) only."""

    @staticmethod
    def forward(ctx, table, stencil, cols):
        ctx.stencil, ctx.cols, ctx.shape = stencil, cols, tuple(table.shape)
        return _X.interp_rows_fwd(table.detach().contiguous(), stencil.rows, stencil.weights, cols)

    @staticmethod
    @autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        M, K = ctx.shape
        plan = ctx.stencil.row_plan(M)                           # built on the first backward: one host read
        return _X.interp_rows_bwd(grad_out.contiguous(), ctx.stencil.weights, plan.arrays, ctx.cols, K), None, None


class _InterpFunction(autograd.Function):
    """N3Tree.interp with points that require a gradient: gradients flow to the table (argument 0) and the points (1)."""

    @staticmethod
    def forward(ctx, table, points, tree_spec, stencil, cols):
        ctx.stencil, ctx.cols, ctx.shape, ctx.tree_spec = stencil, cols, tuple(table.shape), tree_spec
        table = table.detach().contiguous()
        ctx.save_for_backward(table, points)
        return _X.interp_rows_fwd(table, stencil.rows, stencil.weights, cols)

    @staticmethod
    @autograd.function.once_differentiable
    def backward(ctx, grad_out):
        table, points = ctx.saved_tensors
        g = grad_out.contiguous()
        M, K = ctx.shape
        gt = gp = None
        if ctx.needs_input_grad[0]:
            gt = _X.interp_rows_bwd(g, ctx.stencil.weights, ctx.stencil.row_plan(M).arrays, ctx.cols, K)
        if ctx.needs_input_grad[1]:
            gp = _X.interp_points_bwd(ctx.tree_spec, points, ctx.stencil.rows, table, g, ctx.cols)
        return gt, gp, None, None, None


def _interp_columns(dim, K, dev, what):
    """`dim` (None, int, slice, list or tensor, N3Tree.tv's convention) -> int32 distinct columns on `dev`, None for all."""
    if dim is None:
        return None
    if isinstance(dim, torch.Tensor):
        dim = dim.cpu()
    try:
        picked = torch.arange(K)[dim].reshape(-1)
    except (IndexError, TypeError) as e:
        raise RuntimeError(f"{what}: dim does not select columns of a table of {K}: {e}") from None
    if picked.numel() == 0:
        raise RuntimeError(f"{what}: dim selects no column")
    if picked.unique().numel() != picked.numel():
        raise RuntimeError(f"{what}: dim selects a column twice")
    return picked.to(device=dev, dtype=torch.int32)


def interp_rows(stencil, table, dim=None):
    """out float32 [Q, C]: out[q, jc] = sum over the stencil's eight corners, in ascending corner, of
    weights[q, j] * table[rows[q, j], cols[jc]]; corners without a row (-1) are skipped.  `dim` selects the columns as
    N3Tree.tv's does (None: all K); the column axis is kept.  The smooth counterpart of gather_rows: one stencil serves
    any number of tables of the same height.

    Differentiable in `table`, once: the gradient is a full [M, K] table, every element written, summed per entry over
    stencil.row_plan(M) in reduce_rows' fixed order -- no [8 Q, C] tensor, no atomics, the same bits in every run.  The
    plan is built on the first backward (one host read) and cached on the stencil.  GPU only."""
    if not isinstance(stencil, InterpStencil):
        raise RuntimeError("interp_rows: stencil must be an InterpStencil (N3Tree.interp_stencil)")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] < 1:
        raise RuntimeError("interp_rows: table must be float32 [M, K], K >= 1")
    if not table.is_cuda or not stencil.rows.is_cuda:
        raise RuntimeError("interp_rows: only the GPU (HIP) path exists; the stencil and the table must be on the GPU")
    cols = _interp_columns(dim, table.shape[1], table.device, "interp_rows")
    return _InterpRowsFunction.apply(table, stencil, cols)


class _WarpVerticalFunction(autograd.Function):
    """svox_t/svox.py:58-76.  As there, gradients flow only when the
    transformation matrices require one; then all three inputs get theirs."""

    @staticmethod
    def forward(ctx, transformation_matrix, coordinates, skinning_weights, joint_index):
        vertices, matrices = _C.warp_vertices(transformation_matrix, coordinates, skinning_weights, joint_index)
        ctx.save_for_backward(transformation_matrix, coordinates, skinning_weights, joint_index)
        return vertices, matrices

    @staticmethod
    def backward(ctx, vertices_grad_out, matrices_grad_out):
        if ctx.needs_input_grad[0]:
            grad_indices, grad_matrices, grad_skinning_weights = _C.warp_vertices_backward(
                *ctx.saved_tensors, vertices_grad_out.contiguous(), matrices_grad_out.contiguous())
            return grad_matrices, grad_indices, grad_skinning_weights, None
        return None, None, None, None


def get_transformation_matrix(src_pose, tgt_pose):
    """svox_t/svox.py:971-972."""
    return torch.matmul(tgt_pose, torch.inverse(src_pose))


def warp_vertices(transformation_matrix, coordinates, skinning_weights, joint_index):
    """Linear blend skinning of points (svox_t/svox.py:974-976): returns
    (warped points [Q, 3], per-point matrices [Q, 4, 4]); differentiable."""
    return _WarpVerticalFunction.apply(transformation_matrix, coordinates, skinning_weights, joint_index)


def blend_transformation_matrix(transformation_matrix, skinning_weights, joint_index):
    """Per-point blended joint matrices [Q, 4, 4] (svox_t/svox.py:978-981) -- what
    VolumeRenderer.forward takes as `transformation_matrices`."""
    coordinates = torch.zeros((skinning_weights.size(0), 3), device=skinning_weights.device)
    _, matrices = _C.warp_vertices(transformation_matrix, coordinates, skinning_weights, joint_index)
    return matrices


class N3Tree(nn.Module):
    def __init__(self, N=2, data_dim=4, depth_limit=10, init_reserve=1, init_refine=0,
                 geom_resize_fact=1.5, radius=0.5, center=(0.5, 0.5, 0.5),
                 data_format="RGBA", extra_data=None, map_location="cpu"):
        super().__init__()
        assert N >= 2 and depth_limit >= 0
        self.N = int(N)
        self.data_dim = int(data_dim)
        for i in range(1, init_refine + 1):
            init_reserve += (N ** i) ** 3
        dev = map_location
        self.features = nn.Parameter(torch.zeros(init_reserve, data_dim, device=dev))
        self.register_buffer("data", torch.full((init_reserve, N, N, N, 1), EMPTY_INDEX,
                                                dtype=torch.int32, device=dev))
        self.register_buffer("child", torch.zeros(init_reserve, N, N, N, dtype=torch.int32, device=dev))
        self.register_buffer("parent_depth", torch.zeros(init_reserve, 2, dtype=torch.int32, device=dev))
        self.register_buffer("_n_internal", torch.tensor(1, device=dev))
        self.register_buffer("_n_free", torch.tensor(0, device=dev))
        if isinstance(radius, (int, float)):
            radius = [radius] * 3
        radius = torch.tensor(radius, dtype=torch.float32, device=dev)
        center = torch.tensor(center, dtype=torch.float32, device=dev)
        self.register_buffer("invradius", 0.5 / radius)
        self.register_buffer("offset", 0.5 * (1.0 - center / radius))
        self.depth_limit = depth_limit
        self.geom_resize_fact = geom_resize_fact
        self.data_format = DataFormat(data_format) if data_format is not None else None
        if extra_data is not None:
            assert isinstance(extra_data, torch.Tensor)
            self.register_buffer("extra_data", extra_data.to(device=dev))
        else:
            self.extra_data = None
        self._ver = 0
        self._last_all_leaves = None
        self._last_frontier = None
        self._last_neighbors = None
        self._last_tv_plan = None
        self._lock_tree_structure = False
        self._weight_accum = None
        self.filled = 1
        self.refine(repeats=init_refine)

    # ------------------------------------------------------------------ build
    @classmethod
    def from_arrays(cls, child, data, parent_depth, features, data_format="RGBA",
                    radius=0.5, center=(0.5, 0.5, 0.5), depth_limit=10, extra_data=None,
                    device="cpu"):
        """Adopt pre-built topology arrays (e.g. svox_t_amd.synth.shell_tree)."""
        child = torch.as_tensor(child, dtype=torch.int32)
        n, N = child.shape[0], child.shape[1]
        features = torch.as_tensor(features, dtype=torch.float32)
        tree = cls(N=N, data_dim=features.shape[1], depth_limit=depth_limit, init_reserve=1,
                   radius=radius, center=center, data_format=data_format, extra_data=extra_data)
        tree.child = child.contiguous()
        tree.data = torch.as_tensor(data, dtype=torch.int32).reshape(n, N, N, N, 1).contiguous()
        tree.parent_depth = torch.as_tensor(parent_depth, dtype=torch.int32).contiguous()
        tree.features = nn.Parameter(features.contiguous())
        tree._n_internal.fill_(n)
        tree.filled = n
        tree._invalidate()
        return tree.to(device)

    def construct_tree(self, indices):
        """data[leaf containing point i] = i (svox.py:160-161 -> construct_tree_kernel,
        svox_kernel.cu:110-121); the smallest index where points share a leaf."""
        _C.construct_tree(self._spec(self.features), indices.to(self.data.device))
        self._invalidate()

    def build_from_points(self, points, depth, reserve=0):
        """Replace the topology with the octree of a point cloud: what

            for _ in range(depth - 1): tree[points].refine()
            tree.construct_tree(points)

        leaves behind on a fresh tree (helpers.py:101-109, svox.py:488-560, 160-161),
        computed by one HIP pipeline (csrc/svoxt_build.hip) with a single host read
        instead of one query + a dozen tensor ops + a sync per level.  N = 2 only;
        `points` are world coordinates, float32 [P, 3], row i of `features` belongs
        to point i.  `reserve` extra rows are kept free for later refine() calls.
        :return: n_internal"""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        if self.N != 2:
            raise RuntimeError("build_from_points: N = 2 only; use refine() / construct_tree() for other N")
        if not self.data.is_cuda:
            raise RuntimeError("build_from_points: only the GPU (HIP) path exists; move the tree to a GPU")
        with torch.no_grad():
            points = points.to(device=self.data.device, dtype=torch.float32).contiguous()
            child, data, parent_depth, n = _C.build_octree(points, self.offset, self.invradius, depth,
                                                           EMPTY_INDEX, reserve)
            self.child, self.data, self.parent_depth = child, data, parent_depth
            self._n_internal.fill_(n)
            self.filled = n
            self._invalidate()
        return n

    # ------------------------------------------------------------------ query
    def forward(self, features, indices, cuda=True, want_node_ids=False, world=True,
                want_data_ids=False, want_leaf_node=False):
        """Nearest-leaf feature lookup at `indices` [Q, 3]; differentiable wrt
        `features` (svox.py:216-285).  The reference's non-CUDA branch is broken
        by the index indirection (svox.py:263-264); here `cuda=False` is refused."""
        assert not indices.requires_grad
        assert indices.dim() == 2
        if not cuda or not self.data.is_cuda:
            raise RuntimeError("N3Tree.forward: only the GPU (HIP) path exists; "
                               "move the tree to a GPU and call with cuda=True")
        result, node_ids, data_ids, leaf_node = _QueryVerticalFunction.apply(
            features, self._spec(features, world=world), indices)
        if not (want_node_ids or want_data_ids or want_leaf_node):
            return result
        ret = [result]
        if want_node_ids:
            ret.append(node_ids)
        if want_data_ids:
            ret.append(data_ids)
        if want_leaf_node:
            ret.append(leaf_node)
        return ret

    def __getitem__(self, key):
        return N3TreeView(self, key)

    def __setitem__(self, key, values):
        """tree[points] = values: set(points, values, reduce="last") for point keys [Q, 3] (world coordinates) and
        LocalIndex(points) (the tree's own); values float32 [Q, K] or anything that broadcasts to it."""
        local = isinstance(key, LocalIndex)
        if local:
            key = key.val
        if not (torch.is_tensor(key) and key.dim() == 2 and key.shape[1] == 3):
            raise NotImplementedError("N3Tree[key] = values: only point keys of shape [Q, 3] (and LocalIndex) are supported")
        dev = self.data.device
        pts = key.to(device=dev, dtype=torch.float32).contiguous()
        values = torch.as_tensor(values, dtype=torch.float32, device=dev).detach()
        values = values.expand(pts.shape[0], self.features.shape[1]).contiguous()
        self.set(pts, values, world=not local)

    def set(self, indices, values, cuda=True, *, world=True, reduce="last", features=None, return_rows=False):
        """Write `values` (float32 [Q, K], no grad) into the feature rows of the leaves that contain the points
        `indices` (float32 [Q, 3]; world coordinates, the tree's own with world=False) -- the reference's
        N3Tree.set / assign_vertical (svox.py:287-309), with the case it leaves open ("if multiple indices point to same
        leaf node, only one of them will be taken") defined.  One HIP pipeline (csrc/svoxt_assign.hip).

        The leaf of a point is the one forward() / query_vertical reports for it (same transform, clamp, descent); a
        point in an EMPTY leaf (data word >= M) is ignored.  Points are grouped by feature ROW: after refine, merge or
        quantize several slots name one row, and all their points form one group.  Per group:
          reduce="last"           the row takes the values of the group's highest-index point;
          "sum" / "mean"          float32 sum of the group's rows per column, in ASCENDING POINT INDEX, sequential
                                  (acc = v[q0]; acc += v[q1]; ...); mean divides that sum once by float(count);
          "max" / "min"           elementwise over the group, in the same order (x > acc ? x : acc).  Finite values are
                                  the contract: with a NaN in a group the result is unspecified.
        Rows without a point keep their bits; the result is bit-identical from run to run in every mode.

        The table written is `features` if given (float32 [M, K] on the tree's device), else self.features: in place,
        under no_grad, its version counter moves.  Not differentiable.  The topology is not touched, so set() is
        allowed inside accumulate_weights().  GPU only.
        :return: None; with return_rows=True (rows int64 [U] ascending, counts int64 [U]): the rows written and the
                 number of points each received (one host read, as in forward())"""
        if reduce not in _ASSIGN_REDUCE:
            raise RuntimeError(f"set: reduce must be one of {_ASSIGN_REDUCE}")
        if not cuda or not self.data.is_cuda:
            raise RuntimeError("set: only the GPU (HIP) path exists; move the tree to a GPU and call with cuda=True")
        table = self.features if features is None else features
        with torch.no_grad():
            counts = _C.assign_leaves(self._spec(table, world=world), indices, values, reduce, return_counts=return_rows)
        if not return_rows:
            return None
        rows = counts.nonzero(as_tuple=False).squeeze(1)
        return rows, counts[rows].long()

    def snap(self, indices, world=True):
        """float32 [Q, 3]: the lower corner of the leaf that contains each point of `indices` (float32 [Q, 3]) -- what the
        reference writes as tree[indices].corners -- in one launch (descend, then walk up).  World coordinates in and
        out; the tree's own with world=False.  GPU only."""
        if not self.data.is_cuda:
            raise RuntimeError("snap: only the GPU (HIP) path exists; move the tree to a GPU")
        return _C.snap_points(self._spec(self.features, world=world), indices)

    # ------------------------------------------------------------ trilinear
    def _interp_points(self, what, points, world):
        """The point argument of interp / interp_stencil: float32 [Q, 3] on the tree's GPU, or LocalIndex of one (the
        tree's own coordinates).  Returns (points, world)."""
        if isinstance(points, LocalIndex):
            points, world = points.val, False
        if not self.data.is_cuda:
            raise RuntimeError(f"{what}: only the GPU (HIP) path exists; move the tree to a GPU")
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
            raise RuntimeError(f"{what}: points must be float32 [Q, 3]")
        if not points.is_cuda:
            raise RuntimeError(f"{what}: only the GPU (HIP) path exists; the points must be on the tree's GPU")
        return points, bool(world)

    def interp_stencil(self, points, world=True, fill="self", features=None):
        """InterpStencil(rows int32 [Q, 8], weights float32 [Q, 8]) of the points (float32 [Q, 3]; world coordinates, the
        tree's own with world=False or a LocalIndex): for every point the feature rows of the eight cells around it AT ITS
        LEAF'S LEVEL and their trilinear weights (csrc/svoxt_interp.hip; include/svoxt.h has the definition, operation by
        operation).  The point's position against its leaf's centre picks, per axis, the neighbouring cell on that side
        (c + s_a) and the fraction f_a = |l_a - 0.5|; corner j = 4 b_x + 2 b_y + b_z has weight prod(b_a ? f_a :
        1 - f_a) and the row of the leaf that forward() reports at the centre of its cell -- a coarser leaf, the same
        size, or, where finer leaves cover the cell, the one at its centre.  Corner 0 is the point's own leaf.

        fill="self": a corner without a row (outside the cube, an empty leaf) takes the point's own row -- clamp to
        edge, the silhouette of the piecewise-constant field stays hard.  fill="zero": it takes row -1, which
        interp_rows skips.  A point in an empty leaf gets eight rows of -1 either way.

        The field built from a stencil is continuous inside leaves and across faces between leaves of equal depth; it
        is NOT continuous across a change of level.  `features` (default: the tree's own table) only says how many rows
        there are.  Integer descents and twelve float operations per point; not differentiable.  GPU only."""
        if fill not in _INTERP_FILL:
            raise RuntimeError(f"interp_stencil: fill must be one of {_INTERP_FILL}")
        points, world = self._interp_points("interp_stencil", points, world)
        table = self.features if features is None else features
        with torch.no_grad():
            rows, weights = _X.interp_stencil(self._spec(table.detach(), world=world), points.detach().contiguous(), fill)
        return InterpStencil(rows, weights)

    def interp(self, points, features=None, dim=None, world=True, fill="self"):
        """out float32 [Q, C]: the trilinear lookup of `features` (float32 [M, K]; default: the tree's own) at `points`
        (float32 [Q, 3]; world coordinates, the tree's own with world=False or a LocalIndex) --
        interp_rows(self.interp_stencil(points, world, fill), features, dim), see there for the definition and for
        `fill`.  `dim` selects columns as tv()'s does (the column axis is kept).  At the exact centre of a leaf this is
        forward()'s row, bit for bit.

        Differentiable, once, in `features` (a full [M, K] gradient over the stencil's row plan, reduce_rows' fixed
        order, no atomics) and, where points.requires_grad, in `points`: the exact derivative of the value as defined,
        inside a leaf -- it is 0 along an axis on which the point lies outside the cube, and it does not see the jumps
        across a change of level.  No parity claim: the reference has no such operator.  GPU only."""
        if fill not in _INTERP_FILL:
            raise RuntimeError(f"interp: fill must be one of {_INTERP_FILL}")
        points, world = self._interp_points("interp", points, world)
        table = self.features if features is None else features
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] < 1:
            raise RuntimeError("interp: features must be float32 [M, K], K >= 1")
        if not table.is_cuda:
            raise RuntimeError("interp: only the GPU (HIP) path exists; features must be on the tree's GPU")
        stencil = self.interp_stencil(points, world=world, fill=fill, features=table)
        if not points.requires_grad:
            return interp_rows(stencil, table, dim)
        cols = _interp_columns(dim, table.shape[1], table.device, "interp")
        return _InterpFunction.apply(table, points.contiguous(), self._spec(table.detach(), world=world), stencil, cols)

    def leaf_boxes(self, world=True):
        """LeafBoxes(leaf_node, corners, lengths, depths, rows) of EVERY leaf slot, in `_all_leaves()` order, computed
        and kept on the device (a nonzero, one kernel for the corners, three gathers): what a caller samples from
        before set() -- points inside leaf i are corners[i] + u * lengths[i], u in [0, 1)^3.  corners / lengths
        float32 [L, 3] in world coordinates (N3TreeView.corners / .lengths), in the tree's own with world=False (all
        three lengths then equal N^-(depth + 1)); rows: the data word, -1 for empty leaves.  GPU only."""
        if not self.data.is_cuda:
            raise RuntimeError("leaf_boxes: only the GPU (HIP) path exists; move the tree to a GPU")
        with torch.no_grad():
            n = self.filled
            leaf_node = (self.child[:n] == 0).nonzero(as_tuple=False).contiguous()     # (a transposed view on the GPU)
            corners = _C.leaf_corners(self.child, self.parent_depth, self.N, leaf_node)
            depths = self.parent_depth[leaf_node[:, 0], 1]
            lengths = (float(self.N) ** (-depths.float() - 1.0))[:, None]
            if world:
                corners = (corners - self.offset) / self.invradius
                lengths = lengths / self.invradius
            else:
                lengths = lengths.expand(-1, 3).contiguous()
            words = self.data[:n].reshape(n, self.N, self.N, self.N)[tuple(leaf_node.T)].long()
            rows = torch.where((words >= 0) & (words < self.features.shape[0]), words, torch.full_like(words, -1))
        return LeafBoxes(leaf_node, corners, lengths, depths, rows)

    # ------------------------------------------------------------------ copies
    def partial(self, data_sel=None, device=None, data_format=None):
        """A deep copy of the tree on `device` (default: where it is) that keeps the feature columns
        torch.arange(K)[data_sel] -- partial(-1) is the sigma-only tree, a slice or a list keeps several; None keeps all
        (the reference's partial, svox.py:311-337).  `data_dim` follows.  Topology, invradius / offset, extra_data and the
        bookkeeping are copied; no storage is shared.  data_format: kept with data_sel=None, else the copy is a
        plain-row tree ("RGBA") unless `data_format` names another.  `features` is a new nn.Parameter with the
        source's requires_grad.  Works on CPU trees."""
        dev = self.data.device if device is None else torch.device(device)
        feats = self.features.detach()
        if data_sel is not None:
            sel = data_sel.cpu() if isinstance(data_sel, torch.Tensor) else data_sel
            cols = torch.arange(feats.shape[1])[sel].reshape(-1)
            if cols.numel() == 0:
                raise RuntimeError("data_sel selects no column")
            feats = feats[:, cols.to(feats.device)]
        if data_format is None:
            data_format = "RGBA" if data_sel is not None else (None if self.data_format is None else repr(self.data_format))
        extra = None if self.extra_data is None else self.extra_data.to(device=dev, copy=True)
        t = N3Tree(N=self.N, data_dim=feats.shape[1], depth_limit=self.depth_limit, init_reserve=1,
                   geom_resize_fact=self.geom_resize_fact, data_format=data_format, extra_data=extra, map_location=dev)
        with torch.no_grad():
            t.features = nn.Parameter(feats.to(device=dev, copy=True).contiguous(), requires_grad=self.features.requires_grad)
            for nm in ("data", "child", "parent_depth", "_n_internal", "_n_free", "invradius", "offset"):
                setattr(t, nm, getattr(self, nm).to(device=dev, copy=True))
        t.filled = self.filled
        t._invalidate()
        return t

    def clone(self, device=None):
        """A deep copy of the tree on `device` (default: where it is): partial() with every column (svox.py:339-340)."""
        return self.partial(device=device)

    # ----------------------------------------------------------------- refine
    def refine(self, repeats=1, sel=None, leaf_node=None, node_id=None):
        """Split every selected leaf slot into a new internal node
        (svox.py:488-560).  New nodes are appended in selector order; the child
        word holds the offset from the parent node; the new node's slots inherit
        the parent slot's feature index.  Returns True iff buffers were regrown.

        `sel` = tuple of four index tensors (node, x, y, z); default: all leaves
        shallower than depth_limit.  Unlike the reference, `repeats > 1`
        recomputes the selector each round (the reference reuses a stale
        `leaf_node`, svox.py:521-522).  subdivide() selects on the device and
        gives the new leaves feature rows of their own; unshare() does the
        latter for a tree refined here."""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        resized = False
        with torch.no_grad():
            for rep in range(repeats):
                if sel is None:
                    leaves = self._all_leaves()
                    keep = self.parent_depth[leaves[:, 0].to(self.parent_depth.device), 1].cpu() < self.depth_limit
                    leaf_node = leaves[keep].to(self.data.device)
                    sel = tuple(leaf_node.T)
                elif leaf_node is None:
                    leaf_node = torch.stack(sel, dim=-1).to(self.data.device)
                sel = tuple(s.to(self.data.device).long() for s in sel)
                leaf_node = leaf_node.to(self.data.device)
                n_new = sel[0].shape[0]
                if n_new == 0:
                    return resized
                filled = self.filled
                need = filled + n_new - self.capacity
                if need > 0:
                    self._resize_add_cap(need)
                    resized = True
                if self.data.is_cuda:
                    # one kernel instead of a dozen tensor ops (same tables, bit for bit)
                    nid = None if node_id is None else \
                        torch.as_tensor(node_id, dtype=torch.int32, device=self.data.device).contiguous()
                    _C.refine_leaves(self.child, self.data, self.parent_depth, filled,
                                     leaf_node.long().contiguous(), nid)
                else:
                    new_ids = torch.arange(filled, filled + n_new, device=self.data.device, dtype=torch.int32)
                    self.child[sel] = new_ids - leaf_node[:, 0].to(torch.int32)
                    self.data[filled:filled + n_new] = self.data[sel][:, None, None, None]
                    self.parent_depth[filled:filled + n_new, 0] = \
                        self._pack_index(leaf_node).to(torch.int32) if node_id is None else node_id
                    self.parent_depth[filled:filled + n_new, 1] = self.parent_depth[leaf_node[:, 0].long(), 1] + 1
                self._n_internal += n_new
                self.filled += n_new
                self._invalidate()
                sel = leaf_node = node_id = None
        return resized

    def _resize_add_cap(self, cap_needed):
        """Grow the topology buffers geometrically (svox.py:841-863); `features`
        is owned by the caller in this fork and is not resized."""
        cap_needed = max(cap_needed, int(self.capacity * (self.geom_resize_fact - 1.0)))
        dev = self.data.device
        N = self.N
        self.data = torch.cat((self.data, torch.full((cap_needed, N, N, N, 1), EMPTY_INDEX,
                                                     dtype=torch.int32, device=dev)))
        self.child = torch.cat((self.child, torch.zeros((cap_needed, N, N, N), dtype=torch.int32, device=dev)))
        self.parent_depth = torch.cat((self.parent_depth,
                                       torch.zeros((cap_needed, 2), dtype=torch.int32, device=dev)))

    # ------------------------------------------------------------------ prune
    def prune(self, keep=None, *, weights=None, threshold=None, collapse=True, compact_features=True, reserve=0):
        """Drop leaves, collapse what is left empty, compact the tree (one HIP pipeline, csrc/svoxt_prune.hip; the
        reference has the halves as tensor ops, both stale in this fork: merge, svox.py:352-389, and shrink_to_fit,
        :600-642, which never touches `features`; merging occupied leaves is merge() here).

        The decision is per slot of `child`, entries at slots that are not leaves are ignored: `keep`, bool / uint8
        with the shape of `child`, or `weights` (float32 of that shape: what `accumulate_weights()` gives as
        `accum.value`) with `threshold` -- a slot is kept iff weights >= threshold, so a NaN weight drops it.
          1. every leaf that is not kept becomes empty (data = EMPTY_INDEX);
          2. `collapse`: every node but the root below which no kept, non-empty leaf is left is removed, its parent
             slot becomes an empty leaf;
          3. the nodes that remain keep their order and are renumbered, `reserve` free rows behind them;
          4. `compact_features`: the feature rows no remaining leaf names are removed, the others keep their order.
        Without `collapse` the geometry of every remaining leaf is unchanged, and dropping only leaves that contribute
        nothing (sigma <= 0, or empty) leaves every render bit for bit what it was.  With `collapse` empty space is
        described by fewer, larger leaves: the march takes other steps through it (a step is a leaf crossing plus
        `step_size`), so renders change within step-size effects -- the price of a smaller tree, as with the
        reference's merge.

        Replaces `child`, `data`, `parent_depth` and, with `compact_features`, `self.features` by a NEW
        nn.Parameter(features[row_map]): an optimizer that holds the old parameter has to be rebuilt, its state sliced
        with the result's `row_map` -- FeatureSGD / FeatureRMSprop / FeatureAdam do both as `opt.rebind(old, tree.features,
        result.row_map)` (the reference's warning on shrink_to_fit, svox.py:606-607).  A tree left without a
        feature row (nothing kept) is refused by the renderer and the point query (RuntimeError) until it has rows again.  GPU only.
        subdivide() is the growing counterpart: it takes the same per-slot weights and splits the leaves that matter.
        :return: PruneResult(n_internal, nodes_removed, leaves_dropped, row_map); row_map int64 [M'] = the old row of
                 every new feature row, None without `compact_features`"""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        if not self.data.is_cuda:
            raise RuntimeError("prune: only the GPU (HIP) path exists; move the tree to a GPU")
        with torch.no_grad():
            before = self.filled
            child, data, parent_depth, n, row_map, dropped = _C.prune_tree(
                self.child, self.data, self.parent_depth, before, self.features.shape[0], keep, weights, threshold,
                collapse, compact_features, reserve, EMPTY_INDEX, return_dropped=True)
            _C.invalidate_caches(self.child)         # the old tables' acceleration grid goes now, not with the tensor
            self._install_tables(child, data, parent_depth, n)
            if row_map is not None:
                self._replace_features(row_map=row_map)
            self._invalidate()
        return PruneResult(n, before - n, dropped, row_map)

    # -------------------------------------------------------------- subdivide
    _slot_limit = 1 << 31             # slot indices are int32: (filled + nodes_added) * N^3 has to stay below this

    def subdivide(self, sel=None, *, weights=None, threshold=None, max_depth=None, split_empty=False, own_rows=True):
        """Split leaves into new nodes and give the new leaves feature rows of their own: the growing counterpart of
        prune(), one HIP pipeline with one host read (csrc/svoxt_subdivide.hip).  refine() writes the same topology,
        but selects on the host and leaves the N^3 new leaves of a split leaf on ONE feature row, where they cannot
        diverge and there is no row_map for an optimizer.

        The decision is per slot of `child`, entries at slots that are not leaves are ignored: `sel`, bool / uint8
        with the shape of `child`, or `weights` (float32 of that shape: what `accumulate_weights()` gives as
        `accum.value`) with `threshold` -- a slot is selected iff weights >= threshold, so a NaN weight never splits --
        or neither: every leaf.  A selected leaf splits iff its node's depth is below min(depth_limit, max_depth)
        (refine's test) and it is not empty (`split_empty`: empty leaves split too, into N^3 empty leaves).  The
        splitting slots, in `_all_leaves()` order, become the nodes filled, filled + 1, ... exactly as
        refine(sel=<those leaves>) writes them; the tables are regrown geometrically where the capacity does not
        suffice.
          `own_rows` (default): below the k-th split non-empty leaf (row r) slot 0 keeps r, slot j > 0 gets the new row
             M + k (N^3 - 1) + (j - 1), a copy of r: every point query returns the bits it returned before.
             `self.features` becomes a NEW nn.Parameter(features[row_map]); an optimizer that holds the old one:
             `opt.rebind(old, tree.features, result.row_map)` (FeatureSGD / FeatureRMSprop / FeatureAdam).
          `own_rows=False`: every new leaf takes the parent's data word, as after refine(); `features` is untouched.
             unshare() separates the rows later.
        A result with (filled + nodes_added) N^3 >= 2^31 or M' >= EMPTY_INDEX is refused and the tree left as it was.
        GPU only.
        :return: SubdivideResult(n_internal, nodes_added, rows_added, row_map); row_map int64 [M'] = the old row of
                 every new feature row (arange(M), then each r N^3 - 1 times), None without `own_rows`"""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        _C.slot_decision(self.child, "sel", sel, weights, threshold, required=False)     # a bad decision is refused on a CPU tree too
        if not self.data.is_cuda:
            raise RuntimeError("subdivide: only the GPU (HIP) path exists; move the tree to a GPU")
        limit = self.depth_limit if max_depth is None else min(self.depth_limit, int(max_depth))
        with torch.no_grad():
            before, M = self.filled, self.features.shape[0]
            old_child = self.child

            def grow(rows):
                self._resize_add_cap(rows - self.capacity)
                return self.child, self.data, self.parent_depth

            child, data, parent_depth, added, rows_added, row_map = _C.subdivide_tree(
                self.child, self.data.contiguous(), self.parent_depth, before, M,
                None if sel is None else sel.contiguous(), None if weights is None else weights.contiguous(), threshold,
                limit, split_empty, own_rows, EMPTY_INDEX, grow, self._slot_limit)
            if added == 0:
                return SubdivideResult(before, 0, 0, row_map)
            _C.invalidate_caches(old_child, child, data)   # what was cached of the old words goes now
            self._install_tables(child, data, parent_depth, before + added)
            if rows_added > 0:
                self._replace_features(row_map=row_map)
            self._invalidate()
        return SubdivideResult(self.filled, added, rows_added, row_map)

    def spread_rows(self, per_row, empty=0.0):
        """A per-row statistic (float32 [M'], e.g. reduce_rows(samples, w, M, "max")) as a per-slot map, float32 with
        the shape of `child` -- what prune(weights=) and subdivide(weights=) take: a leaf slot whose data word names a
        row below per_row.shape[0] holds per_row[word], every other slot holds `empty`.  Torch ops, under no_grad."""
        if not isinstance(per_row, torch.Tensor) or per_row.dtype != torch.float32 or per_row.dim() != 1:
            raise RuntimeError("spread_rows: per_row must be float32 [M], one entry per feature row")
        if per_row.device != self.data.device:
            raise RuntimeError("spread_rows: per_row must be on the device of the tree")
        with torch.no_grad():
            n = per_row.shape[0]
            words = self.data[..., 0].long()
            named = (self.child == 0) & (words >= 0) & (words < n)
            out = torch.full(self.child.shape, float(empty), dtype=torch.float32, device=self.data.device)
            if n > 0:
                out[named] = per_row[words[named]]
        return out

    def unshare(self):
        """Give every non-empty leaf a feature row of its own (csrc/svoxt_subdivide.hip): of the leaf slots that name
        one row the slot with the smallest flat index keeps it (an integer atomicMin per row: the same result in every
        run), the others get the rows M, M + 1, ... in slot order, each a copy.  Rows no leaf names stay where they
        are, the topology is untouched, every point query returns the bits it returned before.  For trees after
        refine(), subdivide(own_rows=False), merge() or quantize() whose leaves are to be optimised one by one.

        Replaces `self.features` by a NEW nn.Parameter(features[row_map]) when rows were added (an optimizer:
        `opt.rebind(old, tree.features, result.row_map)`).  GPU only.
        :return: UnshareResult(rows_added, row_map); row_map int64 [M'] = the old row of every new feature row"""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        if not self.data.is_cuda:
            raise RuntimeError("unshare: only the GPU (HIP) path exists; move the tree to a GPU")
        with torch.no_grad():
            if not self.data.is_contiguous():
                self.data = self.data.contiguous()
            rows_added, row_map = _C.unshare_rows(self.child, self.data, self.filled, self.features.shape[0], EMPTY_INDEX)
            if rows_added > 0:
                _C.invalidate_caches(self.child, self.data)
                self._replace_features(row_map=row_map)
                self._invalidate()
        return UnshareResult(rows_added, row_map)

    # --------------------------------------------------------------- quantize
    def quantize(self, order, weights=None):
        """Replace the feature table by a palette of 2^order rows: median-cut quantisation of the rows of
        `self.features` (one HIP pipeline, csrc/svoxt_quant.hip; the reference's quantize_median_cut is a CPU
        recursion, quantizer.cpp:48-157), every `data` word that names a row rewritten to the row's colour.  Empty
        leaves stay empty (EMPTY_INDEX) and the topology (`child`, `parent_depth`) is untouched: the result is an
        ordinary tree, rendered and differentiated with respect to the palette by the kernels there are.

        `weights`: float32 [M], one per feature row, weighing the rows in the cuts and in the means (None: every row
        counts once).  Where each row is named by exactly one leaf -- build_from_points, or prune() with
        compact_features -- the per-row weights of `with tree.accumulate_weights() as accum:` renders are

            w = torch.zeros(M, device=dev); leaf = (tree.child[:n] == 0) & (tree.data[:n, ..., 0] < M)
            w[tree.data[:n, ..., 0][leaf].long()] = accum.value[:n][leaf]

        (after refine(), merge() or subdivide(own_rows=False) leaves share rows: unshare() first, or to fine-tune the
        leaves of a quantized tree one by one afterwards).

        Differences from the reference, as svox_t_amd.csrc.quantize_median_cut: an empty segment's palette row is zero
        (reference: NaN), a segment whose weights sum to zero takes the plain mean (reference: NaN), NaN features are
        not checked.  0 <= order <= 16 and 2^order <= M.

        Replaces `self.features` by a NEW nn.Parameter(colors): an optimizer that holds the old parameter has to be
        rebuilt (its state belongs to rows that no longer exist; FeatureSGD / FeatureRMSprop / FeatureAdam:
        `opt.rebind(old, tree.features)`, fresh state; the reference's warning on shrink_to_fit,
        svox.py:606-607).  GPU only.
        :return: QuantizeResult(colors float32 [2^order, K], color_id_map int32 [M])"""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        if not self.data.is_cuda:
            raise RuntimeError("quantize: only the GPU (HIP) path exists; move the tree to a GPU")
        with torch.no_grad():
            colors, color_id_map = _C.quantize_median_cut(self.features.detach().contiguous(), weights, order)
            data = _C.remap_index(self.data.contiguous(), color_id_map)
            _C.invalidate_caches(self.child, self.data)     # what was cached of the old data words goes now
            self.data = data
            self._replace_features(table=colors)
            self._invalidate()
        return QuantizeResult(colors, color_id_map)

    # --------------------------------------------------------------- frontier
    def _frontier_guard(self, what):
        if not self.data.is_cuda:
            raise RuntimeError(f"{what}: only the GPU (HIP) path exists; move the tree to a GPU")

    def frontier(self):
        """int64 [F], ascending: the nodes whose N^3 slots are all leaves -- what merge() can turn into one leaf.  The
        root is never listed (the reference's _frontier, svox.py:471-483, lists it when all its slots are leaves and
        merge then refuses it).  Cached until the tree changes.  GPU only."""
        self._frontier_guard("frontier")
        if self._last_frontier is None:
            fr = _C.frontier_nodes(self.child, self.filled)
            self._last_frontier = _C._Produced("frontier", fr, (fr,), fr.device)
        return self._last_frontier.ready_on(_C._raw_stream(self.child.device))

    def _columns(self, dim, K):
        """`dim` (None, int, slice, list or tensor: what the reference indexes the last axis with) -> (int32 column
        indices on the tree's device or None for all columns, whether the column axis is dropped)."""
        if dim is None:
            return None, False
        if isinstance(dim, torch.Tensor):
            dim = dim.cpu()
        picked = torch.arange(K)[dim]
        if picked.numel() == 0:
            raise RuntimeError("dim selects no column")
        return picked.reshape(-1).to(device=self.data.device, dtype=torch.int32), picked.dim() == 0

    def _gathered(self, features, cols, empty):
        """[F, N^3, K'] rows of the frontier nodes' children with torch ops (differentiable), the mask of the children
        that name a row; empty children are zero rows."""
        fr = self.frontier()
        M = features.shape[0]
        words = self.data[:self.filled].reshape(self.filled, -1)[fr].long() & 0xFFFFFFFF
        has = words < M
        rows = features[words.clamp(max=max(M - 1, 0))] if M > 0 else features.new_zeros(words.shape + (features.shape[1],))
        if cols is not None:
            rows = rows[..., cols.long()]
        return rows * has[..., None].to(rows.dtype), has

    def reduce_frontier(self, op="mean", dim=None, grad=False, features=None, empty="zero"):
        """Reduce the feature rows of every frontier node's N^3 children (the reference's reduce_frontier,
        svox.py:391-418): [F, K'], rows in `frontier()` order.

        op: "mean" | "sum" | "max" | "min" -- one fused HIP kernel (csrc/svoxt_merge.hip) that reads each row once;
        torch.mean / torch.sum / torch.max / torch.min are taken for these by identity.  Any other callable gets the
        gathered [F, N^3, K'] tensor and dim=1, the reference's contract (a tuple result: its first element); that path
        materialises the tensor and, under empty="skip", hands empty children over as zero rows all the same.
        dim: columns of the feature table (int, slice, list, tensor), None for all; an int drops the column axis.
        features: the table to read, self.features by default.
        empty="zero": a child without a row (data word >= M as an unsigned number) counts as a zero row; "skip": only
        the children with a row are reduced ("mean" divides by their number), a node without one gives zeros.
        Sums run over slots 0 .. N^3 - 1 in order, sequential float32; "max" / "min" take the first slot that attains
        the extremum.  grad=True: differentiable with respect to `features` (sum / mean scatter the upstream row, max
        / min give it to the first attaining slot; float atomics where leaves share a row, else bit-reproducible).
        GPU only."""
        self._frontier_guard("reduce_frontier")
        features = self.features if features is None else features
        if empty not in ("zero", "skip"):
            raise RuntimeError('empty must be "zero" or "skip"')
        if not isinstance(op, str):
            op = _REDUCE_CALLABLES.get(op, op)
        cols, squeeze = self._columns(dim, features.shape[1])
        if callable(op):
            rows, _ = self._gathered(features if grad else features.detach(), cols, empty)
            out = op(rows, dim=1)
            out = out[0] if isinstance(out, tuple) else out
            return out.squeeze(-1) if squeeze and out.dim() == 2 else out
        if op not in ("mean", "sum", "max", "min"):
            raise RuntimeError('op must be "mean", "sum", "max", "min" or a callable')
        args = (self.data, self.filled, self.N, self.frontier(), cols, op, empty)
        if grad:
            out = _FrontierReduceFunction.apply(features, *args)
        else:
            out = _C.frontier_reduce(features.detach().contiguous(), *args)
        return out.squeeze(-1) if squeeze else out

    def max_frontier(self, dim=None, grad=False, features=None, empty="zero"):
        """reduce_frontier("max", ...) (the reference's max_frontier, svox.py:420-436)."""
        return self.reduce_frontier("max", dim=dim, grad=grad, features=features, empty=empty)

    def diam_frontier(self, dim=None, grad=False, scale=1.0, features=None, empty="zero"):
        """float32 [F]: per frontier node the largest Euclidean distance between the (selected) feature rows of two of
        its children, times `scale` (the reference's diam_frontier, svox.py:438-468) -- small where merging the node
        loses little.  empty="zero": an empty child is a zero row; "skip": pairs of children with a row only (0 without
        a pair).  The forward is one fused HIP kernel.  grad=True does NOT use it: the value is then computed from the
        gathered [F, N^3, K'] rows with torch ops and differentiated by torch's own autograd.  GPU only."""
        self._frontier_guard("diam_frontier")
        features = self.features if features is None else features
        if empty not in ("zero", "skip"):
            raise RuntimeError('empty must be "zero" or "skip"')
        cols, _ = self._columns(dim, features.shape[1])
        if not grad:
            return _C.frontier_diam(features.detach().contiguous(), self.data, self.filled, self.N, self.frontier(), cols,
                                    empty, scale)
        rows, has = self._gathered(features, cols, empty)
        delta = (rows[:, :, None, :] - rows[:, None, :, :]) * scale
        d2 = (delta * delta).sum(-1)
        if empty == "skip":
            d2 = d2 * (has[:, :, None] & has[:, None, :]).to(d2.dtype)
        best = d2.reshape(d2.shape[0], -1).max(dim=1)[0]
        return torch.where(best > 0, best.clamp_min(1e-45).sqrt(), torch.zeros_like(best))

    # -------------------------------------------------------------- neighbours
    def _table_key(self, M):
        """What the neighbour table and the edge plan were computed from: the topology (`_ver`), the data words (the
        tensor and its version counter: they are also written by callers that change no topology) and the number of
        feature rows (a data word >= M is an empty leaf)."""
        return (self._ver, int(M), self.data.data_ptr(), self.data._version, self.data.device)

    def leaf_neighbors(self):
        """LeafNeighbors(leaf_node, depths, rows, neighbors) of EVERY leaf slot, in `_all_leaves()` order, on the device
        (one HIP pipeline, csrc/svoxt_neighbors.hip; the reference has no such operator): leaf_node / depths / rows as
        in leaf_boxes(), neighbors int32 [L, 6] -- per face, in the order -x +x -y +y -z +z, the index INTO THIS LIST of
        the leaf across it.  A leaf at depth d has the integer cell coordinate c in [0, N^(d + 1))^3 (its slot the least
        significant base-N digit per axis, its ancestors' slots above it); the neighbour is the leaf that holds the
        cell c +- e_a of the same level: the same size or coarser.  -1: outside the cube.  -2: that cell is an internal
        node, the face is covered by several finer leaves -- each of those names this leaf from its side, so every pair
        of face-adjacent leaves appears in the table at least once.  Integer arithmetic only.

        Two host reads (the number of leaves, as in leaf_boxes(), and the deepest node's depth); refused where
        N^(depth + 1) >= 2^31 or 12 L >= 2^31.  Cached until the topology, the data words or the number of feature
        rows change.  GPU only."""
        if not self.data.is_cuda:
            raise RuntimeError("leaf_neighbors: only the GPU (HIP) path exists; move the tree to a GPU")
        key = self._table_key(self.features.shape[0])
        if self._last_neighbors is None or self._last_neighbors[0] != key:
            with torch.no_grad():
                n, N = self.filled, self.N
                leaf_node = (self.child[:n] == 0).nonzero(as_tuple=False).contiguous()
                depths = self.parent_depth[leaf_node[:, 0], 1].contiguous()
                words = self.data[:n].reshape(n, N, N, N)[tuple(leaf_node.T)].long()
                rows = torch.where((words >= 0) & (words < self.features.shape[0]), words, torch.full_like(words, -1))
                deepest = int(self.parent_depth[:n, 1].max().item())
                neighbors = _C.leaf_neighbors(self.child, self.parent_depth, n, leaf_node.shape[0], deepest)
            nb = LeafNeighbors(leaf_node, depths, rows, neighbors)
            self._last_neighbors = (key, _C._Produced("leaf_neighbors", nb, tuple(nb), neighbors.device))
        return self._last_neighbors[1].ready_on(_C._raw_stream(self.data.device))

    def _tv_plan(self, M):
        """The edge plan of tv() for a feature table of M rows (csrc.TVPlan): every pair of
        face-adjacent leaves that name two different rows, once, grouped by row.  Cached like leaf_neighbors()."""
        key = self._table_key(M)
        if self._last_tv_plan is None or self._last_tv_plan[0] != key:
            nb = self.leaf_neighbors()
            rows = nb.rows
            if M != self.features.shape[0]:                  # a table of another height: which leaves are empty follows it
                with torch.no_grad():
                    n, N = self.filled, self.N
                    words = self.data[:n].reshape(n, N, N, N)[tuple(nb.leaf_node.T)].long()
                    rows = torch.where((words >= 0) & (words < M), words, torch.full_like(words, -1))
            plan = _C.tv_plan(nb.neighbors, nb.depths, rows.contiguous(), M, self.N)
            self._last_tv_plan = (key, _C._Produced("tv_plan", plan, (plan.row_ptr, plan.other, plan.meta, plan.area_weights),
                                                    self.data.device))
        return self._last_tv_plan[1].ready_on(_C._raw_stream(self.data.device))

    def _tv_args(self, what, features, dim, p, weight):
        if not self.data.is_cuda:
            raise RuntimeError(f"{what}: only the GPU (HIP) path exists; move the tree to a GPU")
        features = self.features if features is None else features
        if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] < 1:
            raise RuntimeError(f"{what}: features must be float32 [M, K]")
        if features.device != self.data.device:
            raise RuntimeError(f"{what}: features must be on the device of the tree")
        if p not in (1, 2):
            raise RuntimeError(f"{what}: p must be 1 or 2")
        if weight not in ("uniform", "area"):
            raise RuntimeError(f'{what}: weight must be "uniform" or "area"')
        cols, _ = self._columns(dim, features.shape[1])
        if cols is not None and cols.unique().numel() != cols.numel():
            raise RuntimeError(f"{what}: dim selects a column twice")
        return features, cols

    def tv(self, features=None, dim=None, *, p=2, weight="uniform", reduction="sum"):
        """Total-variation (smoothness) loss over the faces between leaves, a scalar tensor:

            loss = sum over edges of  w_e * sum over the selected columns c of  rho(f[row_i, c] - f[row_j, c])

        An EDGE is a pair of face-adjacent leaves (leaf_neighbors()) that name two different feature rows -- every such
        pair once, found from its finer leaf i (at equal sizes from the lower one); empty leaves and leaves that share
        a row contribute nothing.  p=2: rho(v) = v^2; p=1: rho(v) = |v| (subgradient sign(v), sign(0) = 0).
        weight="uniform": w = 1; "area": w = N^(-2 (depth_i + 1)), the shared face's area in tree units (computed in
        double, rounded once to float32).  reduction="mean": divided once by E * columns (0 where E = 0).  dim: columns
        of the table (int, slice, list, tensor; distinct), None for all -- tv(dim=-1) smooths sigma only.  features:
        the table, self.features by default.

        One gather-only HIP kernel over feature rows (csrc/svoxt_neighbors.hip) on a cached plan: no atomics, float32
        sums in a fixed order (include/svoxt.h), so loss and gradient are bit-identical from run to run.  A row shared
        by many leaves (a palette after quantize()) is walked sequentially: correct, not fast.  Differentiable with
        respect to `features` only; the gradient touches every row that has a neighbour, so a lazy=True optimizer skips
        nothing after it.  GPU only."""
        features, cols = self._tv_args("tv", features, dim, p, weight)
        if reduction not in ("sum", "mean"):
            raise RuntimeError('tv: reduction must be "sum" or "mean"')
        plan = self._tv_plan(features.shape[0])
        return _TVFunction.apply(features, plan, cols, p, weight, reduction == "mean")

    def tv_add_grad(self, out, scale, features=None, dim=None, *, p=2, weight="uniform"):
        """out[r, c] = out[r, c] + scale * G[r, c], G the gradient of tv(features, dim, p=p, weight=weight) (reduction
        "sum"), in place, by the same kernel in accumulate mode: one multiply, one add, each rounded, at the selected
        columns of the rows that have an edge; everything else keeps its bits.  The usual way to apply the regulariser:
        `tree.tv_add_grad(tree.features.grad, 1e-3, dim=-1)` in front of `opt.step()`, without a second [M, K] buffer.
        out: float32 [M, K], contiguous, not the table itself; scale: a Python float.  Under no_grad; `out`'s version
        counter moves.  GPU only.
        :return: None"""
        features, cols = self._tv_args("tv_add_grad", features, dim, p, weight)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != tuple(features.shape):
            raise RuntimeError("tv_add_grad: out must be float32 [M, K], the shape of features")
        plan = self._tv_plan(features.shape[0])
        _C.tv_rows(features.detach().contiguous(), plan, cols, p, weight, False, "accumulate", out=out, scale=float(scale))
        return None

    # ------------------------------------------------------------------ merge
    def merge(self, frontier_sel=None, op="mean", *, empty="zero", compact_features=True, reserve=0):
        """Coarsen the tree by one level: every selected frontier node is removed and its parent slot becomes ONE leaf
        (one HIP pipeline, csrc/svoxt_merge.hip; the reference's merge + shrink_to_fit, svox.py:352-389, 600-642).

        frontier_sel: None (every frontier node), a bool mask [F] or int64 indices into `frontier()` (duplicates are
        fine) -- typically a condition on reduce_frontier() / diam_frontier().  op: "mean", "max" or "min" (or
        torch.mean / torch.max / torch.min).  For each merged node:
          - all N^3 data words equal (one shared row -- what refine() leaves -- or all the same empty word): the parent
            slot takes that word, no row is created; so refine(sel) followed by a merge of exactly the new nodes gives
            back the tables word for word (on a tree whose inner slots hold the empty index, as prune() leaves them);
          - no child with a row: the parent slot takes the first child's (empty) word;
          - otherwise the parent slot names a NEW feature row: `op` over the children as reduce_frontier(op, empty=empty).
        The nodes that remain keep their order and are renumbered, with prune()'s layout (inner slots hold the empty
        index, `reserve` free rows behind the tree).  The feature table becomes the carried old rows in their old order
        -- with `compact_features` those a leaf still names, else all -- then the new rows in ascending id of their
        merged node.  Every output word is a function of the input: two runs give the same bytes.

        Replaces `child`, `data`, `parent_depth` and `self.features`, by a NEW nn.Parameter: an optimizer that holds
        the old parameter has to be rebuilt, its state sliced with `row_map` (new rows start fresh; FeatureSGD /
        FeatureRMSprop / FeatureAdam: `opt.rebind(old, tree.features, row_map)` where no rows were added, without
        `row_map` where some were) -- the reference's
        warning on shrink_to_fit, svox.py:606-607.  The acceleration caches are invalidated.  One call merges one
        level; see simplify().  GPU only.
        :return: MergeResult(n_internal, nodes_merged, row_map, rows_added)"""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        if not isinstance(op, str):
            op = _REDUCE_CALLABLES.get(op, op)
        if op not in ("mean", "max", "min"):
            raise RuntimeError('merge: op must be "mean", "max" or "min"')
        if empty not in ("zero", "skip"):
            raise RuntimeError('empty must be "zero" or "skip"')
        if self.filled <= 1:
            raise RuntimeError("Cannot merge root node")
        self._frontier_guard("merge")
        fr = self.frontier()
        if frontier_sel is not None:
            if not isinstance(frontier_sel, torch.Tensor):
                frontier_sel = torch.as_tensor(frontier_sel)
            if frontier_sel.dtype == torch.bool:
                if tuple(frontier_sel.shape) != tuple(fr.shape):
                    raise RuntimeError(f"merge: the mask must have one entry per frontier node, [{fr.shape[0]}]")
            elif frontier_sel.dtype == torch.int64 and frontier_sel.dim() <= 1:
                frontier_sel = frontier_sel.reshape(-1)
                if frontier_sel.numel() and (int(frontier_sel.min()) < 0 or int(frontier_sel.max()) >= fr.shape[0]):
                    raise RuntimeError("merge: index out of range of frontier()")
            else:
                raise RuntimeError("merge: frontier_sel must be None, a bool mask [F] or int64 indices into frontier()")
            fr = fr[frontier_sel.to(fr.device)]
        selected = torch.zeros(self.filled, dtype=torch.uint8, device=self.data.device)
        selected[fr] = 1
        return self._merge_nodes(selected, op, empty, compact_features, reserve)

    def _merge_nodes(self, selected, op, empty, compact_features, reserve):
        """merge() for a per-NODE uint8 selection (entries at nodes that are not frontier nodes are ignored)."""
        with torch.no_grad():
            before = self.filled
            child, data, parent_depth, n, table, row_map, added = _C.merge_tree(
                self.child, self.data, self.parent_depth, before, self.features.detach().contiguous(), selected, op, empty,
                compact_features, reserve, EMPTY_INDEX)
            _C.invalidate_caches(self.child)         # the old tables' acceleration grid goes now, not with the tensor
            self._install_tables(child, data, parent_depth, n)
            self._replace_features(table=table)
            self._invalidate()
        return MergeResult(n, before - n, row_map, added)

    def simplify(self, tol, dim=None, scale=1.0, op="mean", max_rounds=None):
        """Merge, level by level, every frontier node whose children are within `tol` of each other:
        merge(diam_frontier(dim, scale=scale) <= tol, op) until a round merges nothing (or `max_rounds` rounds).  Plain
        Python over the calls above; a round computes the diameter of every node's slots (the merge ignores the
        selection at nodes that are not frontier nodes), so its only host read is merge's.
        :return: the number of nodes merged"""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        if not isinstance(op, str):
            op = _REDUCE_CALLABLES.get(op, op)
        if op not in ("mean", "max", "min"):
            raise RuntimeError('simplify: op must be "mean", "max" or "min"')
        self._frontier_guard("simplify")
        total, rounds = 0, 0
        while self.filled > 1 and (max_rounds is None or rounds < max_rounds):
            cols, _ = self._columns(dim, self.features.shape[1])
            nodes = torch.arange(self.filled, device=self.data.device)
            diam = _C.frontier_diam(self.features.detach().contiguous(), self.data, self.filled, self.N, nodes, cols, "zero", scale)
            merged = self._merge_nodes((diam <= tol).to(torch.uint8), op, "zero", True, 0).nodes_merged
            rounds += 1
            if merged == 0:
                break
            total += merged
        return total

    def shrink_to_fit(self):
        """Trim the topology buffers to the nodes in use (the reference's name, svox.py:600; its node
        defragmentation is what prune() does).  Returns True iff anything changed."""
        if self._lock_tree_structure:
            raise RuntimeError("Tree locked")
        if self.capacity == self.filled:
            return False
        n = self.filled
        self.child, self.data = self.child[:n].clone(), self.data[:n].clone()
        self.parent_depth = self.parent_depth[:n].clone()
        self._invalidate()
        return True

    # ------------------------------------------------------------- properties
    @property
    def n_internal(self):
        return self.filled

    @property
    def capacity(self):
        return self.parent_depth.shape[0]

    @property
    def n_leaves(self):
        return self._all_leaves().shape[0]

    @property
    def max_depth(self):
        return int(self.parent_depth[:self.filled, 1].max().item())

    def _all_leaves(self):
        """[n_leaves, 4] int64 (node, x, y, z) in lexicographic order, on the CPU
        (svox.py:876-880)."""
        if self._last_all_leaves is None:
            self._last_all_leaves = (self.child[:self.filled] == 0).nonzero(as_tuple=False).cpu()
        return self._last_all_leaves

    def _pack_index(self, txyz):
        N = self.N
        return txyz[:, 0] * (N ** 3) + txyz[:, 1] * (N ** 2) + txyz[:, 2] * N + txyz[:, 3]

    def _unpack_index(self, flat):
        N = self.N
        w = flat % N
        v = (flat // N) % N
        u = (flat // (N * N)) % N
        return torch.stack((flat // (N ** 3), u, v, w), dim=-1)

    def _calc_corners(self, nodes):
        """Lower corner in [0,1]^3 of each leaf slot in `nodes` [Q, 4]
        (svox.py:808-826): on a GPU one kernel (svox_t_amd.csrc.leaf_corners), on the CPU the reference's walk of the
        parent chain with torch ops."""
        nodes = nodes.to(self.parent_depth.device).long()
        if self.parent_depth.is_cuda and nodes.dim() == 2 and nodes.shape[1] == 4:
            # one kernel, a lane per slot: the same operations in the same order, the same bits, no host read per level
            return _C.leaf_corners(self.child, self.parent_depth, self.N, nodes.contiguous())
        corner = torch.zeros(nodes.shape[0], 3, device=nodes.device)
        curr = nodes.clone()
        live = torch.ones(nodes.shape[0], dtype=torch.bool, device=nodes.device)
        while True:
            corner[live] = (corner[live] + curr[:, 1:].float()) / self.N
            up = curr[:, 0] != 0
            if not up.any():
                break
            idx = live.nonzero(as_tuple=False).squeeze(1)[up]
            live = torch.zeros_like(live)
            live[idx] = True
            curr = self._unpack_index(self.parent_depth[curr[up, 0], 0].long())
        return corner

    def world2tree(self, indices):
        return torch.addcmul(self.offset, indices, self.invradius)

    def tree2world(self, indices):
        return (indices - self.offset) / self.invradius

    def _install_tables(self, child, data, parent_depth, n):
        """New tables and their node count; the caller drops what was cached of the old ones (invalidate_caches) before
        and calls _invalidate() after."""
        self.child, self.data, self.parent_depth = child, data, parent_depth
        self._n_internal.fill_(n)
        self.filled = n

    def _replace_features(self, table=None, row_map=None):
        """`self.features` becomes a NEW nn.Parameter -- `table`, or the old rows gathered through `row_map` -- that
        requires a gradient iff the old one did."""
        if table is None:
            table = _C.gather_rows(self.features.detach().contiguous(), row_map)
        self.features = nn.Parameter(table, requires_grad=self.features.requires_grad)

    def _invalidate(self):
        self._ver += 1
        self._last_all_leaves = None
        self._last_frontier = None
        self._last_neighbors = None
        self._last_tv_plan = None

    def accumulate_weights(self):
        """`with tree.accumulate_weights() as accum:` -- per-leaf-slot sum of the
        compositing weights of every render inside the block (svox.py:664-676,
        :948-969).  Accumulated with float atomics (the reference races,
        rt_kernel.cu:310)."""
        return WeightAccumulator(self)

    # ------------------------------------------------------------------- spec
    def _spec(self, features, joint_features=None, skinning_weights=None, joint_index=None,
              transformation_matrices=None, world=True):
        """Pack the tree for the operator boundary (svox.py:899-925)."""
        dev = self.data.device
        spec = _C.TreeSpec()
        spec.features = features
        spec.data = self.data
        spec.child = self.child
        spec.parent_depth = self.parent_depth
        spec.extra_data = self.extra_data if self.extra_data is not None else torch.empty((0, 0), device=dev)
        spec.offset = self.offset if world else torch.zeros(3, device=dev)
        spec.scaling = self.invradius if world else torch.ones(3, device=dev)
        spec.n_internal = self.filled
        spec._weight_accum = self._weight_accum if self._weight_accum is not None \
            else torch.empty(0, device=dev)
        spec.joint_features = joint_features if joint_features is not None else torch.empty((0, 0), device=dev)
        spec.skinning_weights = skinning_weights if skinning_weights is not None else torch.empty((0, 0), device=dev)
        spec.joint_index = joint_index if joint_index is not None \
            else torch.empty((0, 0), device=dev, dtype=torch.int32)
        spec.transformation_matrices = transformation_matrices if transformation_matrices is not None \
            else torch.empty((0, 0, 0), device=dev)
        # (not in the reference) `tree.static_features = True`: the caller's promise that the feature table
        # is not written behind torch's version counter, so what is derived from its content may be cached
        spec.static_features = bool(getattr(self, "static_features", False))
        return spec

    def __repr__(self):
        return (f"svox_t_amd.N3Tree(N={self.N}, data_dim={self.data_dim}, depth_limit={self.depth_limit}, "
                f"capacity:{self.filled}/{self.capacity}, data_format:{self.data_format or 'RGBA'})")


class WeightAccumulator:
    def __init__(self, tree):
        self.tree = tree

    def __enter__(self):
        self.tree._lock_tree_structure = True
        self.tree._weight_accum = torch.zeros(self.tree.child.shape, dtype=torch.float32,
                                              device=self.tree.data.device)
        self.weight_accum = self.tree._weight_accum
        return self

    def __exit__(self, *_exc):
        self.tree._weight_accum = None
        self.tree._lock_tree_structure = False

    @property
    def value(self):
        return self.weight_accum

    def __call__(self):
        """Weights of the leaves, in `_all_leaves()` order."""
        leaves = self.tree._all_leaves().to(self.weight_accum.device)
        return self.weight_accum[tuple(leaves.T)]
