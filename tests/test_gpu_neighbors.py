"""GPU tests of N3Tree.leaf_neighbors / tv / tv_add_grad (csrc/svoxt_neighbors.hip) through N3Tree -> csrc -> ctypes ->
C ABI: the neighbour table against the numpy restatement (tests/neighbors_restate.py) byte for byte and against the
float descent of the point query; loss and gradient against the restatement bit for bit and against float64 torch
autograd within bounds derived from float32 sequential summation; the cases that must come out exact; tv_add_grad; the
plan cache behind every operation that changes the tree; the training loop."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from svox_t_amd.csrc import _extras
from tests import neighbors_restate as R
from tests import subdivide_restate as S
from tests.test_gpu_prune import tables_of

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
E = 1410065408
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "topology_*.npz")))
TREES = ["shell_d5", "built_refined", "deep_next_to_coarse"] + FIXTURES
U = 2.0 ** -24


def deep_next_to_coarse():
    """N = 2.  The root's slot 0 is refined five times along its +x and its +z face (the faces it shares with the
    root's slots 4 and 1, which stay leaves): each of those two coarse leaves meets 16 x 16 depth-5 leaves, so its row has
    more than 64 incidences.  Every leaf has a row of its own."""
    child = np.zeros((1, 2, 2, 2), np.int32)
    data = np.arange(8, dtype=np.int32).reshape(1, 2, 2, 2, 1)
    pd = np.zeros((1, 2), np.int32)
    n, M = 1, 8
    for _ in range(5):
        slots, depths, c = R.cells(child, pd, n, 2)
        inside = (c // (2 ** depths)[:, None] == 0).all(1)
        face = (c[:, 0] == 2 ** depths - 1) | (c[:, 2] == 2 ** depths - 1)
        sel = np.zeros(child.shape, bool)
        sel.reshape(-1)[slots[inside & face]] = True
        child, data, pd, added, rows, _ = S.subdivide(child, data, pd, n, M, sel=sel, own_rows=True)
        n, M = n + added, M + rows
    return child, data, pd, n, M


@functools.lru_cache(maxsize=None)
def tables(name, gpu):
    return deep_next_to_coarse() if name == "deep_next_to_coarse" else tables_of(name, gpu)


@functools.lru_cache(maxsize=None)
def restated(name, gpu):
    """(neighbors, slots, depths, cells, rows) of the restatement, computed once per tree."""
    child, data, pd, n, M = tables(name, gpu)
    N = child.shape[1]
    slots, depths, c = R.cells(child, pd, n, N)
    return R.leaf_neighbors(child, pd, n, N), slots, depths, c, R.leaf_rows(child, data, n, M)


def tree_of(name, gpu, K=4, seed=0, features=None):
    child, data, pd, n, M = tables(name, gpu)
    if features is None:
        features = np.random.default_rng(seed).standard_normal((M, K)).astype(np.float32)
    return svox.N3Tree.from_arrays(child[:n], data[:n], pd[:n], torch.from_numpy(features), device=gpu)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def plan_of(tree):
    """The restatement's plan for the tree as it is now."""
    n, N, M = tree.n_internal, tree.N, tree.features.shape[0]
    child, data, pd = tree.child.cpu().numpy(), tree.data.cpu().numpy(), tree.parent_depth.cpu().numpy()
    _, depths, _ = R.cells(child, pd, n, N)
    return R.plan(R.leaf_neighbors(child, pd, n, N), depths, R.leaf_rows(child, data, n, M), M)


def cols_of(dim, K):
    return None if dim is None else np.arange(K)[dim].reshape(-1)


def hip_tv(tree, dim, p, weight, reduction, upstream=1.0, features=None):
    f = tree.features if features is None else features
    loss = tree.tv(f, dim, p=p, weight=weight, reduction=reduction)
    (g,) = torch.autograd.grad(loss, f, torch.tensor(upstream, device=loss.device))
    return loss.detach().cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("name", TREES)
def test_neighbors_equal_the_restatement_and_the_float_descent(gpu, name):
    want, slots, depths, c, rows = restated(name, gpu)
    tree = tree_of(name, gpu)
    N = tree.N
    if name == "deep_next_to_coarse":
        assert tree.max_depth == 5 and (np.bincount(want[want >= 0]).max() > 64)
    got = tree.leaf_neighbors()
    assert got.neighbors.dtype == torch.int32 and same_bits(got.neighbors.cpu().numpy(), want)
    boxes = tree.leaf_boxes()
    assert torch.equal(got.leaf_node, boxes.leaf_node) and torch.equal(got.depths, boxes.depths) and torch.equal(got.rows, boxes.rows)
    assert got.depths.dtype == torch.int32 and got.rows.dtype == torch.int64 and got.leaf_node.dtype == torch.int64
    np.testing.assert_array_equal(got.rows.cpu().numpy(), rows)
    assert tree.leaf_neighbors() is got                                    # cached
    again = tree_of(name, gpu).leaf_neighbors()
    assert same_bits(again.neighbors.cpu().numpy(), want)                  # two runs: the same bytes
    # the float descent of the point query lands in the same leaf: the centre of the target cell -- exact in float32 for
    # N = 2; for N = 3 rounded by at most 2^-24, against the half cell (>= 1 / 54) that separates it from the next leaf
    i, k = np.nonzero(want >= 0)
    t = c[i].astype(np.float64)
    t[np.arange(len(i)), k // 2] += np.where(k % 2 == 1, 1.0, -1.0)
    centre = ((t + 0.5) / (float(N) ** (depths[i] + 1))[:, None])
    pts = centre.astype(np.float32)
    assert (pts.astype(np.float64) == centre).all() if N == 2 else (np.abs(pts.astype(np.float64) - centre) <= U).all()
    with torch.no_grad():
        _, ids = tree(tree.features, torch.from_numpy(pts).to(gpu), want_node_ids=True, world=False)
    np.testing.assert_array_equal(ids.cpu().numpy(), slots[want[i, k]])


def test_neighbors_of_a_tree_above_the_stride_bound_equal_the_restatement(gpu):
    """synth.shell_tree(8) has 990 728 slots: more than 2048 workgroups of 256, so the flag pass and the neighbour walk
    stride (the trees above stay below the bound).  One case, the table alone."""
    from svox_t_amd import synth
    st = synth.shell_tree(8)
    child, pd, n = st.child, st.parent_depth, st.n_internal
    N = child.shape[1]
    assert n * N ** 3 > 2048 * 256
    want = R.leaf_neighbors(child, pd, n, N)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)      # noqa: E731
    got = _C.leaf_neighbors(dev(child), dev(pd), n, want.shape[0], int(pd[:n, 1].max()))
    assert got.dtype == torch.int32 and same_bits(got.cpu().numpy(), want)


CASES = [("shell_d5", 4, None), ("shell_d5", 28, -1), ("shell_d5", 28, slice(0, 3)), ("built_refined", 28, [5, 2]),
         ("deep_next_to_coarse", 65, None), ("deep_next_to_coarse", 1, None), ("deep_next_to_coarse", 28, [5, 2]),
         ("topology_full_n3_l2.npz", 4, -1), ("topology_points_a.npz", 65, slice(0, 3)), ("topology_points_b.npz", 1, -1),
         ("topology_full_n2_l3.npz", 28, None), ("topology_shell_d3.npz", 4, [3, 0]), ("topology_shell_d4.npz", 4, None),
         ("topology_shell_d5.npz", 1, None)]


@pytest.mark.parametrize("name,K,dim", CASES, ids=[f"{n}-K{K}-{d}" for n, K, d in CASES])
def test_loss_and_gradient_equal_the_restatement_bit_for_bit(gpu, name, K, dim):
    tree = tree_of(name, gpu, K=K, seed=K)
    N, f = tree.N, tree.features.detach().cpu().numpy()
    pl = plan_of(tree)
    assert pl["E"] > 0
    cols = cols_of(dim, K)
    for p in (1, 2):
        for weight in ("uniform", "area"):
            for reduction in ("sum", "mean"):
                want_l, want_g = R.tv(f, pl, cols, p, weight, N, mean=reduction == "mean")
                loss, g = hip_tv(tree, dim, p, weight, reduction)
                what = (p, weight, reduction)
                print(what, float(loss), float(want_l))
                assert loss.dtype == np.float32 and loss.shape == () and same_bits(loss, want_l), what
                assert same_bits(g, want_g), what
    again_l, again_g = hip_tv(tree, dim, 2, "area", "mean")
    assert same_bits(again_l, loss) and same_bits(again_g, g)              # two runs: the same bytes
    half_l, half_g = hip_tv(tree, dim, 2, "area", "mean", upstream=0.5)
    assert same_bits(half_g, np.float32(0.5) * g) and same_bits(half_l, loss)
    with torch.no_grad():                                                  # no gradient wanted: the same loss, no G
        assert same_bits(tree.tv(dim=dim, p=2, weight="area", reduction="mean").cpu().numpy(), loss)
    # the plan of the package is the restatement's, byte for byte
    mine = tree._tv_plan(f.shape[0])
    assert mine.E == pl["E"] and mine.nbytes == 4 * (f.shape[0] + 1) + 10 * pl["E"] + 128
    for nm in ("row_ptr", "other", "meta"):
        assert same_bits(getattr(mine, nm).cpu().numpy(), pl[nm]), nm


@pytest.mark.parametrize("name,K,dim", [("shell_d5", 28, None), ("deep_next_to_coarse", 4, -1), ("topology_full_n3_l2.npz", 65, [5, 2])])
def test_float64_autograd_agrees_within_the_float32_summation_bounds(gpu, name, K, dim):
    """The same loss from `neighbors` with float64 torch ops.  Bounds: a float32 sum of T terms, in any order, is within
    (T - 1) u sum|term| of the exact sum, u = 2^-24, to first order -- the issue's T u sum|term|; a gradient entry is a sequential sum
    of J terms, each with up to three roundings of its own: (J + 3) u sum|term|."""
    tree = tree_of(name, gpu, K=K, seed=3)
    nb = tree.leaf_neighbors()
    M = tree.features.shape[0]
    i, k = (nb.neighbors >= 0).nonzero(as_tuple=True)
    j = nb.neighbors[i, k].long()
    di, dj, ri, rj = nb.depths[i], nb.depths[j], nb.rows[i], nb.rows[j]
    edge = ((dj < di) | ((dj == di) & (k % 2 == 1))) & (ri >= 0) & (rj >= 0) & (ri != rj)
    ri, rj, di = ri[edge], rj[edge], di[edge]
    cols = torch.arange(K, device=gpu) if dim is None else torch.arange(K)[dim].reshape(-1).to(gpu)
    for p in (1, 2):
        for weight in ("uniform", "area"):
            w = torch.ones_like(di, dtype=torch.float64) if weight == "uniform" else (float(tree.N) ** (-2.0 * (di.double() + 1))).float().double()
            f64 = tree.features.detach().double().requires_grad_(True)
            diff = f64[ri][:, cols] - f64[rj][:, cols]
            terms = w[:, None] * (diff * diff if p == 2 else diff.abs())
            want = terms.sum()
            (want_g,) = torch.autograd.grad(want, f64)
            loss, g = hip_tv(tree, dim, p, weight, "sum")
            T = terms.numel()
            err, bound = abs(float(loss) - float(want.detach())), T * U * float(terms.detach().abs().sum())
            print(name, p, weight, "loss err", err, "bound", bound)
            assert err <= bound
            gterm = (w[:, None] * (2 * diff if p == 2 else diff.sign())).abs().detach()
            mass = torch.zeros(M, K, dtype=torch.float64, device=gpu)
            mass[:, cols] = torch.zeros(M, len(cols), dtype=torch.float64, device=gpu).index_add_(0, ri, gterm).index_add_(0, rj, gterm)
            J = torch.bincount(torch.cat((ri, rj)), minlength=M).double()[:, None]
            gerr = (torch.from_numpy(g).to(gpu).double() - want_g).abs()
            gbound = (J + 3) * U * mass
            print(name, p, weight, "worst gradient ratio", float((gerr / gbound.clamp_min(1e-300)).max()))
            assert bool((gerr <= gbound).all())


def test_cases_that_come_out_exact(gpu):
    # a constant table
    tree = tree_of("shell_d5", gpu, features=np.full((tables("shell_d5", gpu)[4], 4), 0.37, np.float32))
    for p in (1, 2):
        loss, g = hip_tv(tree, None, p, "area", "sum")
        assert float(loss) == 0.0 and not g.any()
    # leaves that share a row contribute nothing between themselves: refine() without rows of their own ...
    tree = tree_of("topology_shell_d3.npz", gpu, K=4)
    tree.refine()
    M = tree.features.shape[0]
    pl, f = plan_of(tree), tree.features.detach().cpu().numpy()
    shared = tree.leaf_neighbors()
    j = shared.neighbors.clamp(min=0).long()
    assert int(((shared.neighbors >= 0) & (shared.rows[:, None] >= 0) & (shared.rows[j] == shared.rows[:, None])).sum()) > 0
    loss, g = hip_tv(tree, None, 2, "uniform", "sum")
    want_l, want_g = R.tv(f, pl, None, 2, "uniform", 2)
    assert same_bits(loss, want_l) and same_bits(g, want_g) and float(loss) > 0
    # ... and a palette after quantize(order=2): four rows, very long segments
    tree = tree_of("shell_d5", gpu, K=4)
    tree.quantize(2)
    assert tree.features.shape[0] == 4
    pl, f = plan_of(tree), tree.features.detach().cpu().numpy()
    assert np.diff(pl["row_ptr"]).max() > 256
    for p in (1, 2):
        loss, g = hip_tv(tree, -1, p, "area", "mean")
        want_l, want_g = R.tv(f, pl, [3], p, "area", 2, mean=True)
        assert same_bits(loss, want_l) and same_bits(g, want_g)
    # empty leaves and rows no leaf names: zero gradient rows
    child, data, pd, n, M = tables("topology_points_a.npz", gpu)
    d2 = np.ascontiguousarray(data[:n]).copy()
    flat = d2.reshape(-1)
    named = np.nonzero((child[:n].reshape(-1) == 0) & ((flat.astype(np.int64) & 0xFFFFFFFF) < M))[0]
    dropped = flat[named[::3]].copy()
    flat[named[::3]] = E
    dropped = np.setdiff1d(dropped, flat[named])                           # the rows no leaf names any more
    f = np.random.default_rng(1).standard_normal((M + 5, 4)).astype(np.float32)        # five rows behind: named by no leaf
    tree = svox.N3Tree.from_arrays(child[:n], d2, pd[:n], torch.from_numpy(f), device=gpu)
    loss, g = hip_tv(tree, None, 2, "uniform", "sum")
    want_l, want_g = R.tv(f, plan_of(tree), None, 2, "uniform", child.shape[1])
    assert same_bits(loss, want_l) and same_bits(g, want_g) and float(loss) > 0
    assert not g[dropped].any() and not g[M:].any() and len(dropped) > 0
    # one leaf pair only
    child = np.zeros((1, 2, 2, 2), np.int32)
    data = np.full((1, 8), E, np.int32)
    data[0, 0], data[0, 1] = 0, 1
    pair = svox.N3Tree.from_arrays(child, data, np.zeros((1, 2), np.int32), torch.tensor([[1., 2.], [3., 5.]]), device=gpu)
    loss, g = hip_tv(pair, None, 2, "uniform", "sum")
    assert float(loss) == 13.0 and g.tolist() == [[-4, -6], [4, 6]]
    loss, g = hip_tv(pair, 1, 2, "area", "mean")
    assert float(loss) == 2.25 and g.tolist() == [[0, -1.5], [0, 1.5]]
    # a table without rows; a tree whose leaves are all empty: loss 0, nothing raised
    none = svox.N3Tree.from_arrays(child, data, np.zeros((1, 2), np.int32), torch.zeros(0, 3), device=gpu)
    loss, g = hip_tv(none, None, 2, "uniform", "mean")
    assert float(loss) == 0.0 and g.shape == (0, 3)
    empty = svox.N3Tree.from_arrays(child, np.full((1, 8), E, np.int32), np.zeros((1, 2), np.int32), torch.ones(4, 3), device=gpu)
    for reduction in ("sum", "mean"):
        loss, g = hip_tv(empty, None, 1, "area", reduction)
        assert float(loss) == 0.0 and g.shape == (4, 3) and not g.any()
    out = torch.ones(4, 3, device=gpu)
    assert empty.tv_add_grad(out, 2.0) is None and bool((out == 1).all())
    with pytest.raises(RuntimeError, match="twice"):
        pair.tv(dim=[1, 1])


@pytest.mark.parametrize("name,K,dim", [("deep_next_to_coarse", 28, -1), ("shell_d5", 4, None), ("topology_full_n3_l2.npz", 65, [5, 2]),
                                        ("topology_points_b.npz", 28, slice(0, 3))])
def test_tv_add_grad(gpu, name, K, dim):
    tree = tree_of(name, gpu, K=K, seed=2)
    M, N, f = tree.features.shape[0], tree.N, tree.features.detach().cpu().numpy()
    pl, cols = plan_of(tree), cols_of(dim, K)
    sentinel = (np.arange(M * K, dtype=np.float32).reshape(M, K) % 251) * np.float32(0.125) - 7        # NaN-free, every bit pattern known
    for p, weight, scale in ((2, "uniform", 1e-3), (1, "area", -0.75)):
        _, G = R.tv(f, pl, cols, p, weight, N)
        want = R.add_grad(sentinel, scale, G, pl, cols)
        out = torch.from_numpy(sentinel.copy()).to(gpu)
        ver = out._version
        assert tree.tv_add_grad(out, scale, dim=dim, p=p, weight=weight) is None and out._version > ver
        got = out.cpu().numpy()
        assert same_bits(got, want)
        live = np.diff(pl["row_ptr"]) > 0
        keep = np.ones((M, K), bool)
        keep[np.ix_(np.nonzero(live)[0], np.arange(K) if cols is None else cols)] = False
        assert same_bits(got[keep], sentinel[keep]) and (got != sentinel).any()
    assert not tree.features.requires_grad or tree.features.grad is None
    with pytest.raises(RuntimeError):
        tree.tv_add_grad(tree.features.detach(), 1.0)                      # the table itself
    with pytest.raises(RuntimeError):
        tree.tv_add_grad(torch.zeros(M, K + 1, device=gpu), 1.0)


def fresh_loss(tree, **kw):
    n = tree.n_internal
    other = svox.N3Tree.from_arrays(tree.child[:n].cpu(), tree.data[:n].cpu(), tree.parent_depth[:n].cpu(),
                                    tree.features.detach().cpu(), device=tree.data.device)
    return other.tv(**kw).detach().cpu().numpy(), other


def test_the_plan_is_cached_and_follows_the_tree(gpu):
    tree = tree_of("shell_d5", gpu, K=4, seed=5)
    kw = dict(p=2, weight="area", reduction="mean")
    built = _extras.TV_PLAN_BUILDS
    first = tree.tv(**kw)
    second = tree.tv(dim=-1, p=1)
    tree.tv_add_grad(torch.zeros_like(tree.features), 1.0)
    assert _extras.TV_PLAN_BUILDS == built + 1 and float(first.detach()) > 0 and float(second.detach()) > 0
    sel = torch.zeros(tree.child.shape, dtype=torch.bool, device=gpu)
    sel.reshape(-1)[::5] = True
    steps = [("subdivide", lambda: tree.subdivide(sel[:tree.child.shape[0]])),
             ("merge", lambda: tree.merge(torch.arange(0, tree.frontier().shape[0], 3, device=gpu))),
             ("prune", lambda: tree.prune(torch.rand(tree.child.shape, device=gpu, generator=torch.Generator(gpu).manual_seed(1)) < 0.7)),
             ("refine", lambda: tree.refine()),
             ("unshare", lambda: tree.unshare()),
             ("quantize", lambda: tree.quantize(5))]
    last = first.detach().cpu().numpy()
    for what, step in steps:
        before = _extras.TV_PLAN_BUILDS
        step()
        got = tree.tv(**kw).detach().cpu().numpy()
        want, other = fresh_loss(tree, **kw)
        assert _extras.TV_PLAN_BUILDS == before + 2, what                   # the tree's own plan was rebuilt (and the fresh tree's built)
        assert same_bits(got, want) and float(got) > 0, what
        assert torch.equal(tree.leaf_neighbors().neighbors, other.leaf_neighbors().neighbors), what
        assert not same_bits(got, last), what
        last = got
    # data words written behind the tree's back (no topology change): the data tensor's version counter is in the key
    tree.unshare()
    full = ((tree.child[:tree.n_internal] == 0) & (tree.data[:tree.n_internal, ..., 0] != E)).nonzero()
    tree.data[tuple(full[::2].T)] = E
    got = tree.tv(**kw).detach().cpu().numpy()
    assert same_bits(got, fresh_loss(tree, **kw)[0]) and not same_bits(got, last)
    # another table of another height through `features=`: a plan of its own
    taller = torch.cat((tree.features.detach(), torch.ones(3, tree.features.shape[1], device=gpu)))
    assert same_bits(tree.tv(taller, **kw).cpu().numpy(), got)


def test_render_backward_tv_add_grad_adam_loop(gpu):
    from tests.util import Case
    from svox_t_amd import synth

    def run():
        c = Case(depth=5, K=28, data_format="SH9", width=8, height=8)
        tree = c.tree(gpu)
        r = svox.VolumeRenderer(tree)
        opt = svox.FeatureAdam([tree.features], lr=1e-2)
        rays = c.rays_gpu(gpu)
        target = None
        for _ in range(3):
            opt.zero_grad()
            # one 8 x 8 tile: the per-tile backward sums it in a fixed order and hands every row ONE addend, so the render's
            # gradient is reproducible too (across tiles it is summed with float atomics, in the order of arrival)
            out = r(tree.features, rays, image_shape=(8, 8))
            target = synth.grad_output(c.Q, out.shape[1]).to(gpu) if target is None else target
            ((out - target) ** 2).mean().backward()
            tree.tv_add_grad(tree.features.grad, 1e-3, dim=-1)
            opt.step()
        return c.features.numpy(), tree.features.detach().cpu().numpy(), tree

    start, a, tree = run()
    _, b, _ = run()
    touched = np.diff(tree._tv_plan(a.shape[0]).row_ptr.cpu().numpy()) > 0
    assert touched.sum() > 100 and (a[touched, -1] != start[touched, -1]).all()        # sigma moved wherever a leaf has a neighbour
    assert same_bits(a, b) and np.isfinite(a).all()
