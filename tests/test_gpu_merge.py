"""GPU tests of the frontier reductions and N3Tree.merge (csrc/svoxt_merge.hip) through N3Tree / csrc -> ctypes -> C
ABI: frontier, reductions and tables against the numpy restatement (tests/merge_restate.py) -- bits where the order of
the arithmetic is specified, derived bounds where it is not --, gradients against torch autograd on the gathered
formulation, renders and queries behind a merge against the CPU oracle, simplify, refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
from oracle import oracle as O
from svox_t_amd import synth
from tests import merge_restate as MR
from tests import prune_restate as PR
from tests.util import Case, assert_grads_close

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "merge_*.npz")))
TREES = ["shell_d5_k28", "shell_d8_k32", "n3", "radius", "quantized", "refined", "shell_d5_k6"] + FIXTURES
OPS = ["max", "min", "sum", "mean"]


def make_tree(name, gpu):
    """An N3Tree on the GPU.  Shell trees: frontier nodes with empty and full children, every row named once."""
    if name.startswith("shell_d"):
        depth, K = int(name[7]), int(name.split("_k")[1])
        st = synth.shell_tree(depth)
        return svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, synth.shell_features(st.n_features, K, seed=depth),
                                       data_format="RGBA", device=gpu)
    if name in ("n3", "radius"):
        g = np.load(os.path.join(G, "topology_full_n3_l2.npz" if name == "n3" else "topology_points_a.npz"))
        n = int(g["n_internal"])
        data, M = PR.number_leaves(g["child"], n, np.random.default_rng(5))
        feats = torch.randn(M, 5 if name == "n3" else 28, generator=torch.Generator().manual_seed(3))
        kw = dict(radius=[1.0, 2.0, 4.0], center=[1.0, 0.0, -1.0]) if name == "radius" else {}
        return svox.N3Tree.from_arrays(g["child"][:n], data[:n], g["parent_depth"][:n], feats, data_format="RGBA", device=gpu, **kw)
    if name == "quantized":                             # 64 palette rows shared by thousands of leaves
        tree = make_tree("shell_d5_k28", gpu)
        tree.quantize(6)
        return tree
    if name == "refined":                               # every leaf of a shell tree split once more: 8 slots share a row
        tree = make_tree("shell_d4_k32", gpu)
        tree.refine()
        return tree
    g = np.load(os.path.join(G, name))                  # the reference's own trees, its words read as a one-column table
    M = int((g["child"] == 0).sum())
    return svox.N3Tree.from_arrays(g["child"], g["data"], g["parent_depth"], torch.arange(M, dtype=torch.float32)[:, None],
                                   data_format="RGBA", device=gpu)


def tables(tree):
    n = tree.n_internal
    return (tree.child[:n].cpu().numpy(), tree.data[:n].cpu().numpy(), tree.parent_depth[:n].cpu().numpy(), n,
            tree.features.detach().cpu().numpy())


def gathered(tree, features, cols=None):
    """The torch formulation: ([F, N^3, K'] rows, zero where the child is empty; has [F, N^3])."""
    n, M = tree.n_internal, features.shape[0]
    words = tree.data[:n].reshape(n, -1)[tree.frontier()].long() & 0xFFFFFFFF
    has = words < M
    rows = features[words.clamp(max=M - 1)] * has[..., None]
    return (rows if cols is None else rows[..., cols]), has, words


def torch_reduce(rows, has, op, empty, tensor_count=False):
    """tensor_count: the mean as sum / count with the count a TENSOR.  torch.mean's backward on the GPU multiplies by
    the rounded reciprocal of the count (1 / 27 for N = 3), which is the derivative of sum / 27 only to an ulp; a tensor
    divisor makes torch divide, and g / count is what the derivative of the specified forward (sum / count) is."""
    if empty == "zero" and op == "mean" and tensor_count:
        return rows.sum(1) / torch.full_like(rows[:, 0, :1], rows.shape[1])
    if empty == "zero":
        return {"mean": lambda: rows.mean(1), "sum": lambda: rows.sum(1), "max": lambda: rows.max(1)[0], "min": lambda: rows.min(1)[0]}[op]()
    cnt = has.sum(1, keepdim=True)
    if op in ("sum", "mean"):
        s = rows.sum(1)
        return s if op == "sum" else s / cnt.clamp(min=1)
    fill = float("-inf") if op == "max" else float("inf")
    x = rows.masked_fill(~has[..., None], fill)
    x = x.max(1)[0] if op == "max" else x.min(1)[0]
    return torch.where(cnt > 0, x, torch.zeros_like(x))


@pytest.mark.parametrize("name", TREES)
def test_frontier_and_reductions_equal_the_restatement(gpu, name):
    tree = make_tree(name, gpu)
    child, data, pd, n, feats = tables(tree)
    K = feats.shape[1]
    fr = MR.frontier(child, n)
    got = tree.frontier()
    assert got.dtype == torch.int64 and got.device.type == "cuda" and tree.frontier() is got          # cached
    np.testing.assert_array_equal(got.cpu().numpy(), fr)
    assert len(fr) > 10 and fr[0] != 0
    dims = [None] + ([[K - 1, 0], slice(1, None)] if K > 1 else [[0]])
    if name == "shell_d8_k32":                          # (the restatement of a large tree takes its time)
        dims = [None]
    for empty in ("zero", "skip"):
        for dim in dims:
            cols = None if dim is None else np.arange(K)[dim]
            for op in OPS:
                want = MR.reduce(feats, data, n, fr, op, cols=cols, empty=empty)[0]
                out = tree.reduce_frontier(op, dim=dim, empty=empty)
                assert out.dtype == torch.float32 and tuple(out.shape) == want.shape
                # the order of the arithmetic is specified: the same bits
                assert out.cpu().numpy().tobytes() == want.tobytes(), (op, empty, dim)
            # against torch's own sums of the gathered rows: reordering an N^3-term float32 sum moves an entry by at
            # most N^3 2^-24 sum |x_i| (each of the N^3 - 1 partial sums is rounded once, each is at most sum |x_i|)
            rows, has, _ = gathered(tree, tree.features.detach(), None if cols is None else torch.as_tensor(cols, device=gpu))
            bound = tree.N ** 3 * 2.0 ** -24 * rows.abs().sum(1)
            for op in ("sum", "mean"):
                diff = (tree.reduce_frontier(op, dim=dim, empty=empty) - torch_reduce(rows, has, op, empty)).abs()
                scale = 1.0 if op == "sum" else 1.0 / (has.sum(1, keepdim=True).clamp(min=1) if empty == "skip" else tree.N ** 3)
                assert bool((diff <= bound * scale).all()), (op, empty, dim, float((diff - bound * scale).max()))
            # the diameter: K'-term sums of squares and a square root, against float64: (K' + 4) 2^-23 relative
            want = MR.diam(feats, data, n, fr, cols=cols, empty=empty, scale=1.5)
            out = tree.diam_frontier(dim=dim, empty=empty, scale=1.5)
            assert out.dtype == torch.float32 and tuple(out.shape) == (len(fr),)
            Kc = K if cols is None else len(np.atleast_1d(cols))
            err = np.abs(out.cpu().numpy().astype(np.float64) - want)
            assert (err <= (Kc + 4) * 2.0 ** -23 * want).all(), (empty, dim, float((err / np.maximum(want, 1e-300)).max()))
    if name in FIXTURES:                                # the reference's numbers, exactly
        g = np.load(os.path.join(G, name))
        np.testing.assert_array_equal(got.cpu().numpy(), g["frontier"])
        np.testing.assert_array_equal(tree.max_frontier().cpu().numpy(), g["max_frontier"].astype(np.float32))
        np.testing.assert_array_equal(tree.diam_frontier().cpu().numpy(), g["diam_frontier"])
    # an int `dim` drops the column axis, as the reference's data[..., dim] does; max_frontier is reduce_frontier("max")
    assert torch.equal(tree.reduce_frontier("sum", dim=K - 1), tree.reduce_frontier("sum", dim=[K - 1])[:, 0])
    assert torch.equal(tree.max_frontier(empty="skip"), tree.reduce_frontier(torch.max, empty="skip"))


def test_callables(gpu):
    tree = make_tree("shell_d5_k28", gpu)
    for fn, op in ((torch.mean, "mean"), (torch.sum, "sum"), (torch.max, "max"), (torch.min, "min")):
        assert torch.equal(tree.reduce_frontier(fn), tree.reduce_frontier(op))            # by identity: the same kernels
    rows, has, _ = gathered(tree, tree.features.detach())
    seen = {}

    def spread(x, dim):
        seen["shape"], seen["dim"] = tuple(x.shape), dim
        return x.max(dim=dim)[0] - x.min(dim=dim)[0], "second"

    out = tree.reduce_frontier(spread, dim=slice(0, 3))
    assert seen == {"shape": (rows.shape[0], 8, 3), "dim": 1}
    assert torch.equal(out, rows[..., :3].max(1)[0] - rows[..., :3].min(1)[0])
    assert torch.equal(tree.reduce_frontier(lambda x, dim: torch.median(x, dim=dim))[0:5], rows.median(1)[0][0:5])


@pytest.mark.parametrize("empty", ["zero", "skip"])
@pytest.mark.parametrize("name", ["shell_d5_k28", "n3", "shell_d5_k6"])
def test_gradients_are_exact_where_rows_are_unshared(gpu, name, empty):
    """Random floats: no ties among real rows.  Every row is named by one leaf, so each element of the gradient is one
    term added once to a zeroed table: equal to torch autograd on the gathered formulation, bit for bit."""
    tree = make_tree(name, gpu)
    if name == "n3":                                    # number_leaves shares rows: give every leaf its own
        n = tree.n_internal
        leaf = (tree.child[:n] == 0) & (tree.data[:n, ..., 0] < tree.features.shape[0])
        tree.data[:n, ..., 0][leaf] = torch.arange(int(leaf.sum()), dtype=torch.int32, device=gpu)
        tree.features = torch.nn.Parameter(torch.randn(int(leaf.sum()), 5, device=gpu))
        tree._invalidate()
    K = tree.features.shape[1]
    for dim in (None, [K - 1, 1]):
        cols = None if dim is None else torch.as_tensor(dim, device=gpu)
        for op in OPS:
            out = tree.reduce_frontier(op, dim=dim, grad=True, empty=empty)
            gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(gpu)
            tree.features.grad = None
            out.backward(gout)
            got = tree.features.grad.clone()
            f2 = tree.features.detach().clone().requires_grad_(True)
            rows, has, _ = gathered(tree, f2, cols)
            torch_reduce(rows, has, op, empty, tensor_count=True).backward(gout)
            assert int((got != 0).sum()) > 100
            assert torch.equal(got, f2.grad), (op, dim, float((got - f2.grad).abs().max()))
            assert torch.equal(out.detach(), tree.reduce_frontier(op, dim=dim, empty=empty))


@pytest.mark.parametrize("name", ["quantized", "refined"])
def test_gradients_where_rows_are_shared(gpu, name):
    """Rows named by many leaves: float atomics in no fixed order.  Against the float64 sum of the same terms an entry
    that receives c terms is within c 2^-24 sum |terms|: one rounding of each term (g / count for mean; the others are
    exact) and c - 1 roundings of partial sums, none larger than sum |terms|."""
    tree = make_tree(name, gpu)
    for empty in ("zero", "skip"):
        for op in OPS:
            out = tree.reduce_frontier(op, grad=True, empty=empty)
            gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).to(gpu)
            tree.features.grad = None
            out.backward(gout)
            got = tree.features.grad.double()
            f2 = tree.features.detach().double().requires_grad_(True)               # the reference sum: float64
            rows, has, words = gathered(tree, f2)
            res = torch_reduce(rows, has, op, empty, tensor_count=True)
            want, = torch.autograd.grad(res, f2, gout.double(), retain_graph=True)
            abs_sum, = torch.autograd.grad(res, f2, gout.double().abs(), retain_graph=True)   # the weights are >= 0
            if op in ("sum", "mean"):
                c = torch.bincount(words[has], minlength=f2.shape[0]).double()[:, None]
            else:
                c, = torch.autograd.grad(res, f2, torch.ones_like(res))
            assert op in ("max", "min") or float(c.max()) >= 8
            assert bool(((got - want).abs() <= c * 2.0 ** -24 * abs_sum).all()), (op, empty)
            assert bool((got[abs_sum == 0] == 0).all())


def test_diam_gradient_goes_through_torch(gpu):
    tree = make_tree("shell_d5_k6", gpu)
    for empty in ("zero", "skip"):
        for dim in (None, [0, 5]):
            d = tree.diam_frontier(dim=dim, grad=True, scale=0.7, empty=empty)
            fused = tree.diam_frontier(dim=dim, scale=0.7, empty=empty)
            assert bool(((d.detach() - fused).abs() <= (6 + 4) * 2.0 ** -23 * fused).all())
            gout = torch.rand(d.shape, generator=torch.Generator().manual_seed(4)).to(gpu)
            tree.features.grad = None
            d.backward(gout)
            got = tree.features.grad.double()
            f2 = tree.features.detach().double().requires_grad_(True)
            rows, has, _ = gathered(tree, f2, None if dim is None else torch.as_tensor(dim, device=gpu))
            d2 = (((rows[:, :, None] - rows[:, None]) * 0.7) ** 2).sum(-1)
            if empty == "skip":
                d2 = d2 * (has[:, :, None] & has[:, None])
            best = d2.reshape(d2.shape[0], -1).max(1)[0]
            torch.where(best > 0, best.clamp_min(1e-300).sqrt(), torch.zeros_like(best)).backward(gout.double())
            assert int((got != 0).sum()) > 100
            torch.testing.assert_close(got, f2.grad, rtol=1e-5, atol=1e-6)


def selections(fr, seed):
    rng = np.random.default_rng(seed)
    half = rng.random(len(fr)) < 0.5
    return {"all": None, "half": half, "none": np.zeros(len(fr), bool),
            "indices": np.r_[np.nonzero(half)[0][::3], np.nonzero(half)[0][:4]].astype(np.int64)}          # with duplicates


@pytest.mark.parametrize("name", TREES)
def test_merge_equals_the_restatement(gpu, name):
    tree0 = make_tree(name, gpu)
    child, data, pd, n, feats = tables(tree0)
    fr = MR.frontier(child, n)
    combos = [("half", "mean", "zero", True, 0), ("half", "max", "skip", False, 5), ("all", "min", "zero", True, 3),
              ("indices", "mean", "skip", True, 0), ("none", "max", "zero", True, 0)]
    if name == "shell_d8_k32":
        combos = combos[:2]
    for which, op, empty, compact, reserve in combos:
        sel = selections(fr, len(name))[which]
        nodes = fr if sel is None else fr[sel]
        want = MR.merge(child, data, pd, n, feats, nodes, op=op, empty=empty, compact_features=compact, reserve=reserve)
        results = []
        for _ in range(2):
            tree = tree0                                # the same tables again
            tree.child, tree.data, tree.parent_depth = (torch.from_numpy(a).to(gpu) for a in (child, data, pd))
            tree.features = torch.nn.Parameter(torch.from_numpy(feats).to(gpu))
            tree.filled = n
            tree._n_internal.fill_(n)
            tree._invalidate()
            res = tree.merge(None if sel is None else torch.from_numpy(sel).to(gpu), op, empty=empty, compact_features=compact,
                             reserve=reserve)
            got = (tree.child.cpu().numpy(), tree.data.cpu().numpy(), tree.parent_depth.cpu().numpy(), tree.n_internal,
                   tree.features.detach().cpu().numpy(), None if res.row_map is None else res.row_map.cpu().numpy(), res.rows_added)
            results.append(got)
        for g, w, what in zip(got[:3], want[:3], ("child", "data", "parent_depth")):
            assert g.dtype == w.dtype and g.shape == w.shape, what
            np.testing.assert_array_equal(g, w, err_msg=f"{what} {which} {op}")
        assert (res.n_internal, res.nodes_merged, res.rows_added) == (want[3], n - want[3], want[6])
        assert tree.filled == int(tree._n_internal) == want[3] and tree.capacity == want[3] + reserve
        if compact:
            assert got[5].dtype == np.int64
            np.testing.assert_array_equal(got[5], want[5])
        else:
            assert got[5] is None and want[5] is None and got[4].shape[0] == feats.shape[0] + want[6]
        assert got[4].tobytes() == want[4].tobytes()                 # carried rows and new rows: the same bits
        assert isinstance(tree.features, torch.nn.Parameter) and tree.features.requires_grad
        for a, b in zip(results[0], results[1]):                     # two runs: the same bytes
            assert (a is None and b is None) or np.asarray(a).tobytes() == np.asarray(b).tobytes()
        PR.integrity(got[0], got[1], got[2], got[3], tree.N, got[4].shape[0], collapsed=False)
        if which == "none":
            assert res.nodes_merged == 0 and np.array_equal(got[0], child)
    if name in FIXTURES:                                # ... and the reference's own tables
        g = np.load(os.path.join(G, name))
        tree = make_tree(name, gpu)
        tree.merge(torch.from_numpy(g["mask"]).to(gpu), torch.max)
        np.testing.assert_array_equal(tree.child.cpu().numpy(), g["child_after"])
        np.testing.assert_array_equal(tree.parent_depth.cpu().numpy(), g["parent_depth_after"])
        leaf = (tree.child == 0).reshape(-1)
        vals = tree.features.detach()[tree.data.reshape(-1)[leaf].long(), 0]
        np.testing.assert_array_equal(vals.cpu().numpy(), g["data_after"].reshape(-1)[leaf.cpu().numpy()].astype(np.float32))


def test_refine_then_merge_restores_the_tables(gpu):
    tree = make_tree("shell_d5_k28", gpu)
    child, data, pd, n, feats = tables(tree)
    leaves = tree._all_leaves()
    pick = leaves[torch.randperm(leaves.shape[0], generator=torch.Generator().manual_seed(0))[:500].sort()[0]]
    tree.refine(sel=tuple(pick.T))
    assert tree.n_internal == n + 500
    new = torch.arange(n, n + 500, device=gpu)
    fr = tree.frontier()
    idx = torch.searchsorted(fr, new)
    assert torch.equal(fr[idx], new)                    # the new nodes are frontier nodes
    res = tree.merge(idx)
    assert (res.n_internal, res.nodes_merged, res.rows_added) == (n, 500, 0)
    assert torch.equal(res.row_map, torch.arange(feats.shape[0], device=gpu))
    for got, want in zip(tables(tree), (child, data, pd, n, feats)):
        np.testing.assert_array_equal(got, want)


def test_all_equal_children_render_the_same_bits_as_the_restated_tables(gpu):
    """Children of equal VALUE in distinct rows: the merged leaf's new row is their mean.  The merged tree renders bit
    for bit what from_arrays(the restated tables) renders -- and, with caches warmed on the old tables, what the CPU
    oracle makes of the new ones, forward and backward; queries too."""
    c = Case(depth=6, K=28, data_format="SH9", width=64, height=64)
    tree = c.tree(gpu)
    child, data, pd, n, feats = tables(tree)
    fr = MR.frontier(child, n)
    words = data.reshape(n, 8)[fr].astype(np.int64)
    for f, w in zip(fr[::2], words[::2]):               # every other frontier node: its children share one value
        rows = w[w < feats.shape[0]]
        feats[rows] = feats[rows[0]]
    tree.features = torch.nn.Parameter(torch.from_numpy(feats).to(gpu))
    tree.static_features = True
    r = svox.VolumeRenderer(tree)
    rays = c.rays_gpu(gpu)
    with torch.no_grad():
        first = r(tree.features, rays, image_shape=(64, 64)).cpu().numpy()              # warms the caches
    sel = np.zeros(len(fr), bool)
    sel[::2] = True
    want = MR.merge(child, data, pd, n, feats, fr[sel], op="mean", empty="skip")
    res = tree.merge(torch.from_numpy(sel).to(gpu), "mean", empty="skip")
    assert res.nodes_merged == int(sel.sum()) and res.rows_added > 100
    t2 = svox.N3Tree.from_arrays(want[0], want[1], want[2], want[4], data_format="SH9", device=gpu)
    with torch.no_grad():
        got = r(tree.features, rays, image_shape=(64, 64)).cpu().numpy()
        ref = svox.VolumeRenderer(t2)(t2.features, rays, image_shape=(64, 64)).cpu().numpy()
        depth = r.render_depth(tree.features, rays).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    m = tree.n_internal
    ot = O.Tree(tree.features.detach().cpu().numpy(), tree.data[:m].cpu().numpy(), tree.child[:m].cpu().numpy(),
                offset=tree.offset.cpu().numpy(), scaling=tree.invradius.cpu().numpy())
    np.testing.assert_array_equal(got, O.volume_render(ot, *c.rays_np(), c.oracle_opts()))
    np.testing.assert_array_equal(depth, O.render_depth(ot, *c.rays_np(), c.oracle_opts()))
    assert not np.array_equal(got, first)
    g = synth.grad_output(c.Q, got.shape[1], seed=3)
    out = r(tree.features, rays, image_shape=(64, 64))
    out.backward(g.to(gpu))
    gw, abs_sum = O.volume_render_backward(ot, *c.rays_np(), c.oracle_opts(), g.numpy(), want_abs=True)
    assert tree.features.grad.shape == tree.features.shape
    assert_grads_close(tree.features.grad.cpu().numpy(), gw, abs_sum)
    pts = torch.rand(5000, 3, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        vals = tree(tree.features, pts.to(gpu))
    np.testing.assert_array_equal(vals.cpu().numpy(), O.query(ot, pts.numpy())[0])


def test_simplify_collapses_piecewise_constant_levels(gpu):
    """A full depth-3 tree (1 + 8 + 64 + 512 nodes) whose leaf rows hold the id of their depth-2 ancestor: the depth-3
    nodes merge (equal children), then the depth-2 nodes (equal again), and the depth-1 nodes do not (ids differ by
    >= 1 > tol): D - 2 = 1 is left, 1 + 8 nodes, 576 merged."""
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=3, map_location=gpu)
    n = tree.n_internal
    assert n == 585 and tree.max_depth == 3
    leaf = tree.child[:n] == 0
    node = leaf.nonzero()[:, 0]
    assert bool((tree.parent_depth[node.long(), 1] == 3).all())
    anc = tree.parent_depth[node.long(), 0].long() // 8                       # the depth-2 node above the leaf's node
    tree.data[:n, ..., 0][leaf] = torch.arange(node.shape[0], dtype=torch.int32, device=gpu)
    tree.features = torch.nn.Parameter(anc.float()[:, None] * torch.tensor([1.0, -2.0, 0.5, 3.0], device=gpu))
    tree._invalidate()
    assert tree.simplify(0.25, max_rounds=1) == 512 and tree.n_internal == 73
    assert tree.simplify(0.25) == 64
    assert tree.n_internal == 9 and tree.max_depth == 1 and tree.simplify(0.25) == 0
    vals = tree.features.detach()[tree.data[1:9].reshape(-1).long(), 0]
    assert torch.equal(vals.sort()[0], torch.arange(9, 73, device=gpu).float())
    PR.integrity(tree.child.cpu().numpy(), tree.data.cpu().numpy(), tree.parent_depth.cpu().numpy(), 9, 2, tree.features.shape[0],
                 collapsed=False)


def test_refusals(gpu):
    tree = make_tree("shell_d5_k6", gpu)
    F = tree.frontier().shape[0]
    with pytest.raises(RuntimeError, match="one entry per frontier node"):
        tree.merge(torch.ones(F + 1, dtype=torch.bool, device=gpu))
    with pytest.raises(RuntimeError, match="out of range"):
        tree.merge(torch.tensor([0, F], device=gpu))
    with pytest.raises(RuntimeError, match="frontier_sel must be"):
        tree.merge(torch.ones(F, device=gpu))
    with pytest.raises(RuntimeError, match="op must be"):
        tree.merge(op="sum")
    with pytest.raises(RuntimeError, match="op must be"):
        tree.reduce_frontier("median")
    with pytest.raises(RuntimeError, match="empty must be"):
        tree.diam_frontier(empty="drop")
    with pytest.raises((RuntimeError, IndexError)):
        tree.reduce_frontier("max", dim=6)
    with tree.accumulate_weights():
        with pytest.raises(RuntimeError, match="Tree locked"):
            tree.merge()
    root = svox.N3Tree(N=2, data_dim=4, map_location=gpu)
    assert root.frontier().numel() == 0 and tuple(root.reduce_frontier("max").shape) == (0, 4)
    with pytest.raises(RuntimeError, match="Cannot merge root node"):
        root.merge()
    assert tree.frontier().shape[0] == F                # nothing above changed the tree
