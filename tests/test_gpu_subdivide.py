"""GPU tests of N3Tree.subdivide / N3Tree.unshare (csrc/svoxt_subdivide.hip) through csrc.subdivide_tree / unshare_rows
-> ctypes -> C ABI: tables and row_map against the numpy restatement (tests/subdivide_restate.py) byte for byte, against
the reference's own refine (tests/golden/subdivide_*.npz) and against refine() here; queries, renders, gradients and the
renderer's caches behind the operations; the optimizer's rebind; the accumulate -> prune -> subdivide loop; refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from tests import optim_restate as OR
from tests import subdivide_restate as R
from tests.test_gpu_prune import mask_of, tables_of
from tests.util import Case, assert_grads_close, assert_outputs_close

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
E = R.EMPTY_INDEX
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "topology_*.npz")))
GOLDEN = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "subdivide_*.npz")))
TREES = ["shell_d5", "shell_d6", "built_refined"] + FIXTURES
MASKS = ["half", "few", "all", "none", "one"]


def T(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def hip_subdivide(gpu, child, data, pd, n, M, max_depth=None, **kw):
    for k in ("sel", "weights"):
        if k in kw:
            kw[k] = T(kw[k], gpu)
    if max_depth is not None:
        kw["depth_limit"] = min(kw.get("depth_limit", 10), max_depth)
    kw.setdefault("depth_limit", 10)
    c, d, p, added, rows, row_map = _C.subdivide_tree(T(child, gpu), T(data, gpu), T(pd, gpu), n, M, **kw)
    return c.cpu().numpy(), d.cpu().numpy(), p.cpu().numpy(), added, rows, None if row_map is None else row_map.cpu().numpy()


def assert_same(got, want):
    for g, w, what in zip(got[:3], want[:3], ("child", "data", "parent_depth")):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        np.testing.assert_array_equal(g, w, err_msg=what)
    assert got[3:5] == want[3:5]
    if want[5] is None:
        assert got[5] is None
    else:
        assert got[5].dtype == np.int64
        np.testing.assert_array_equal(got[5], want[5], err_msg="row_map")


def padded(child, data, pd, n, rows):
    """The first n rows of the tables and, behind them, rows like unused rows of an N3Tree: `rows` in all."""
    N = child.shape[1]
    c = np.zeros((rows, N, N, N), np.int32)
    d = np.full((rows, N, N, N, 1), E, np.int32)
    p = np.zeros((rows, 2), np.int32)
    c[:n], d[:n], p[:n] = child[:n], data[:n], pd[:n]
    return c, d, p


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", TREES)
def test_tables_and_row_map_equal_the_restatement(gpu, name, mask):
    child, data, pd, n, M = tables_of(name, gpu)
    N = child.shape[1]
    sel = mask_of(mask, child, data, M, seed=len(name) + n)
    deepest = int(pd[:n, 1].max())
    for own in (True, False):
        for empty in (True, False):
            for max_depth in (None, deepest):                   # the second: the deepest level's leaves stay
                kw = dict(sel=sel, own_rows=own, split_empty=empty, max_depth=max_depth)
                want = R.subdivide(child, data, pd, n, M, **kw)
                got = hip_subdivide(gpu, child, data, pd, n, M, **kw)               # capacity as it comes: regrown where short
                assert_same(got, want)
                R.integrity(got[0], got[1], got[2], n + got[3], N, M + got[4], n_before=n, own_rows=own, row_map=got[5], M_before=M)
    # capacity exactly sufficient (in place) and larger; uint8 selections are read like bool ones; two runs give the same bytes
    want = R.subdivide(child, data, pd, n, M, sel=sel)
    first = None
    for extra in (0, 5):
        c, d, p = padded(child, data, pd, n, n + want[3] + extra)
        s = np.zeros(c.shape, np.uint8)
        s[:n] = sel[:n].astype(np.uint8) * 3
        s[n:] = 1                                               # behind the tree: ignored
        w2 = R.subdivide(c, d, p, n, M, sel=s)
        got = hip_subdivide(gpu, c, d, p, n, M, sel=s)
        assert_same(got, w2)
        assert got[0].shape[0] == n + want[3] + extra
        again = hip_subdivide(gpu, c, d, p, n, M, sel=s)
        for a, b in zip(again[:3] + (again[5],), got[:3] + (got[5],)):
            assert a.tobytes() == b.tobytes()
        first = first or got
        np.testing.assert_array_equal(got[5], first[5])
    if mask == "all":                                           # no selection at all = every leaf
        assert_same(hip_subdivide(gpu, child, data, pd, n, M), R.subdivide(child, data, pd, n, M, sel=sel))
    if mask == "none":
        assert got[3:5] == (0, 0)
        np.testing.assert_array_equal(got[5], np.arange(M))


def test_trees_above_the_stride_bound_equal_the_restatement(gpu):
    """synth.shell_tree(8) has 990 728 slots: more than 2048 workgroups of 256, so the per-slot passes of subdivide (mark,
    list) and of unshare (owner, mark) stride (shell_d6 and the fixtures stay below the bound).  One case each."""
    st = synth.shell_tree(8)
    child, data, pd, n, M = st.child, st.data, st.parent_depth, st.n_internal, st.n_features
    N = child.shape[1]
    assert n * N ** 3 > 2048 * 256
    sel = np.random.default_rng(8).random(child.shape) < 0.1
    want = R.subdivide(child, data, pd, n, M, sel=sel, own_rows=True)
    got = hip_subdivide(gpu, child, data, pd, n, M, sel=sel, own_rows=True)
    assert want[3] > 0 and want[4] > 0
    assert_same(got, want)
    R.integrity(got[0], got[1], got[2], n + got[3], N, M + got[4], n_before=n, own_rows=True, row_map=got[5], M_before=M)
    # unshare: the row words divided by 3, so that up to three leaves name a row
    words = data.astype(np.int64) & 0xFFFFFFFF
    shared = np.where(words < M, words // 3, words).astype(np.uint32).view(np.int32).reshape(data.shape)
    want_data, want_rows, want_map = R.unshare(child, shared, n, M)
    assert want_rows > 0
    d = T(shared, gpu)
    rows_added, row_map = _C.unshare_rows(T(child, gpu), d, n, M)
    assert rows_added == want_rows
    np.testing.assert_array_equal(row_map.cpu().numpy(), want_map)
    np.testing.assert_array_equal(d.cpu().numpy(), want_data)


@pytest.mark.parametrize("name", ["shell_d5", "built_refined", "topology_full_n3_l2.npz"])
def test_weights_and_threshold(gpu, name):
    child, data, pd, n, M = tables_of(name, gpu)
    rng = np.random.default_rng(3)
    w = rng.random(child.shape).astype(np.float32)
    flat = w.reshape(-1)
    full = np.nonzero((child.reshape(-1) == 0) & ((data.reshape(-1).astype(np.int64) & 0xFFFFFFFF) < M))[0]
    full = full[full < n * child.shape[1] ** 3]
    thr = float(np.float32(0.4))
    flat[full[0::7]] = np.nan                        # never splits
    flat[full[1::7]] = np.float32(thr)               # splits: >=
    flat[full[2::7]] = np.nextafter(np.float32(thr), np.float32(0))
    flat[full[3::7]] = np.inf
    for own in (True, False):
        want = R.subdivide(child, data, pd, n, M, weights=w, threshold=thr, own_rows=own)
        got = hip_subdivide(gpu, child, data, pd, n, M, weights=w, threshold=thr, own_rows=own)
        assert_same(got, want)
    split = got[0].reshape(-1)[:child.size] != child.reshape(-1)
    assert split[full[1::7]].all() and split[full[3::7]].all() and not split[full[0::7]].any() and not split[full[2::7]].any()
    assert len(full[0::7]) > 0


@pytest.mark.parametrize("name", GOLDEN)
def test_topology_equals_the_references_refine(gpu, name):
    g = np.load(os.path.join(G, name))
    child, data, pd, mask = g["child"], g["data"], g["parent_depth"], g["mask"]
    n, M = child.shape[0], int((child == 0).sum())
    c, d, p, added, rows, row_map = hip_subdivide(gpu, child, data, pd, n, M, sel=mask, own_rows=False, split_empty=True)
    assert added == g["child_after"].shape[0] - n and rows == 0 and row_map is None
    for got, want, what in ((c, g["child_after"], "child"), (d, g["data_after"], "data"), (p, g["parent_depth_after"], "parent_depth")):
        assert got.dtype == want.dtype and got.shape == want.shape, what
        np.testing.assert_array_equal(got, want, err_msg=what)


def tree_of(name, gpu, K=4, seed=0):
    child, data, pd, n, M = tables_of(name, gpu)
    feats = torch.from_numpy(np.random.default_rng(seed).standard_normal((M, K)).astype(np.float32))
    return svox.N3Tree.from_arrays(child[:n], data[:n], pd[:n], feats, device=gpu), child, data, M


@pytest.mark.parametrize("name", ["shell_d5", "built_refined", "topology_full_n3_l2.npz", "topology_points_a.npz"])
def test_equals_refine_on_a_clone(gpu, name):
    tree, child, data, M = tree_of(name, gpu)
    other = tree.clone()
    n = tree.n_internal
    sel = torch.from_numpy(mask_of("half", child[:n], data[:n], M, seed=5)).to(gpu)
    res = tree.subdivide(sel, own_rows=False, split_empty=True)
    leaves = (sel & (other.child == 0)).nonzero(as_tuple=False)            # slot order
    other.refine(sel=tuple(leaves.T))
    assert res.nodes_added == leaves.shape[0] > 0 and res.rows_added == 0 and res.row_map is None
    assert tree.n_internal == other.n_internal == res.n_internal == int(tree._n_internal) == n + res.nodes_added
    assert tree.capacity == other.capacity
    assert torch.equal(tree.child, other.child) and torch.equal(tree.data, other.data)
    assert torch.equal(tree.parent_depth, other.parent_depth)
    # with room left the next round works in place, on the tables there are
    tree.shrink_to_fit()
    other.shrink_to_fit()
    tree._resize_add_cap(40)
    other._resize_add_cap(40)
    table = tree.child
    few = torch.zeros(tree.child.shape, dtype=torch.bool, device=gpu)
    few.reshape(-1)[(tree.child.reshape(-1)[:tree.n_internal * tree.N ** 3] == 0).nonzero()[:30:3, 0]] = True
    res = tree.subdivide(few, own_rows=False, split_empty=True)
    other.refine(sel=tuple((few & (other.child == 0)).nonzero(as_tuple=False).T))
    assert res.nodes_added == 10 and tree.child is table and tree.capacity == other.capacity
    assert torch.equal(tree.child, other.child) and torch.equal(tree.data, other.data)
    assert torch.equal(tree.parent_depth, other.parent_depth)


def quantized_shell(gpu):
    c = Case(depth=5, K=4, data_format="RGBA", width=8, height=8)
    tree = c.tree(gpu)
    tree.quantize(4)
    return tree


@pytest.mark.parametrize("name", ["built_refined", "quantized_shell_d5"])
def test_unshare_equals_the_restatement_and_is_idempotent(gpu, name):
    tree = quantized_shell(gpu) if name.startswith("quantized") else tree_of(name, gpu)[0]
    n, M = tree.n_internal, tree.features.shape[0]
    child, data = tree.child.cpu().numpy(), tree.data.cpu().numpy()
    feats = tree.features.detach().clone()
    pts = torch.rand(4000, 3, generator=torch.Generator().manual_seed(1)).to(gpu)
    with torch.no_grad():
        before = tree(tree.features, pts)
    want_data, want_rows, want_map = R.unshare(child, data, n, M)
    assert want_rows > 0
    res = tree.unshare()
    assert res.rows_added == want_rows and res.row_map.dtype == torch.int64
    np.testing.assert_array_equal(res.row_map.cpu().numpy(), want_map)
    np.testing.assert_array_equal(tree.data.cpu().numpy(), want_data)
    np.testing.assert_array_equal(tree.child.cpu().numpy(), child)
    assert isinstance(tree.features, torch.nn.Parameter) and tree.features.requires_grad
    assert torch.equal(tree.features.detach(), feats[res.row_map])
    leaf = (tree.child[:n] == 0) & (tree.data[:n, ..., 0] != E)
    named = tree.data[:n, ..., 0][leaf]
    assert named.unique().numel() == named.numel()                         # every non-empty leaf a row of its own
    with torch.no_grad():
        assert torch.equal(tree(tree.features, pts), before)               # the same bits at every point
    # two runs on the same tables give the same bytes (the owner of a row is an integer minimum)
    d1, d2 = T(data, gpu), T(data, gpu)
    r1 = _C.unshare_rows(T(child, gpu), d1, n, M)
    r2 = _C.unshare_rows(T(child, gpu), d2, n, M)
    assert r1[0] == r2[0] == want_rows and torch.equal(d1, d2) and torch.equal(r1[1], r2[1]) and torch.equal(d1, tree.data)
    old = tree.features
    again = tree.unshare()
    assert again.rows_added == 0 and torch.equal(again.row_map, torch.arange(M + want_rows, device=gpu)) and tree.features is old
    np.testing.assert_array_equal(tree.data.cpu().numpy(), want_data)


@pytest.mark.parametrize("name", ["shell_d5", "subdivide_full_n3_l2.npz"])
def test_shared_rows_then_unshare_is_own_rows(gpu, name):
    """On trees whose leaves have rows of their own (the shell tree; the fixture's distinct word per leaf)."""
    if name.startswith("subdivide_"):
        g = np.load(os.path.join(G, name))
        child, data, M = g["child"], g["data"], int((g["child"] == 0).sum())
        feats = torch.from_numpy(np.random.default_rng(1).standard_normal((M, 4)).astype(np.float32))
        a = svox.N3Tree.from_arrays(child, data, g["parent_depth"], feats, device=gpu)
    else:
        a, child, data, M = tree_of(name, gpu)
    b = a.clone()
    n = a.n_internal
    sel = torch.from_numpy(mask_of("half", child[:n], data[:n], M, seed=8)).to(gpu)
    ra = a.subdivide(sel)
    rb = b.subdivide(sel, own_rows=False)
    ru = b.unshare()
    assert ra.rows_added == ru.rows_added > 0 and rb.rows_added == 0 and a.n_internal == b.n_internal
    assert torch.equal(a.child, b.child) and torch.equal(a.parent_depth, b.parent_depth) and a.features.shape == b.features.shape
    n2 = a.n_internal
    leaf = (a.child[:n2] == 0) & (a.data[:n2, ..., 0] != E)
    assert torch.equal(leaf, (b.child[:n2] == 0) & (b.data[:n2, ..., 0] != E))
    rows_a, rows_b = a.data[:n2, ..., 0][leaf].long(), b.data[:n2, ..., 0][leaf].long()
    assert torch.equal(rows_a.sort().values, rows_b.sort().values)         # the same rows are named, once each
    assert torch.equal(a.features.detach()[rows_a], b.features.detach()[rows_b])       # and every leaf holds the same values
    assert torch.equal(ra.row_map[rows_a], ru.row_map[rows_b])


def test_queries_and_the_result_object(gpu):
    c = Case(depth=5, K=4, data_format="RGBA", width=8, height=8)
    tree = c.tree(gpu)
    n, M = tree.n_internal, tree.features.shape[0]
    pts = torch.rand(5000, 3, generator=torch.Generator().manual_seed(2)).to(gpu)
    with torch.no_grad():
        before, rows = tree(tree.features, pts, want_data_ids=True)
    assert int((rows >= 0).sum()) > 100
    feats = tree.features.detach().clone()
    sel = mask_of("half", c.st.child, c.st.data, M, 11)
    want = R.subdivide(c.st.child, c.st.data, c.st.parent_depth, n, M, sel=sel)
    old = tree.features
    res = tree.subdivide(torch.from_numpy(sel).to(gpu))
    assert (res.n_internal, res.nodes_added, res.rows_added) == (n + want[3], want[3], want[4]) and want[3] > 0
    assert tree.n_internal == tree.filled == int(tree._n_internal) == n + want[3] <= tree.capacity
    np.testing.assert_array_equal(res.row_map.cpu().numpy(), want[5])
    np.testing.assert_array_equal(tree.child[:res.n_internal].cpu().numpy(), want[0][:res.n_internal])
    np.testing.assert_array_equal(tree.data[:res.n_internal].cpu().numpy(), want[1][:res.n_internal])
    np.testing.assert_array_equal(tree.parent_depth[:res.n_internal].cpu().numpy(), want[2][:res.n_internal])
    assert tree.features is not old and isinstance(tree.features, torch.nn.Parameter) and tree.features.requires_grad
    assert torch.equal(tree.features.detach(), feats[res.row_map])
    with torch.no_grad():
        after, rows2 = tree(tree.features, pts, want_data_ids=True)
    assert torch.equal(after, before) and torch.equal(rows2 >= 0, rows >= 0)
    assert int((rows2 != rows).sum()) > 100                                # ... from rows of their own
    # nothing selected: nothing changes, row_map is the identity (or None)
    old, ver = tree.features, tree._ver
    none = tree.subdivide(torch.zeros(tree.child.shape, dtype=torch.bool, device=gpu))
    assert none[:3] == (res.n_internal, 0, 0) and torch.equal(none.row_map, torch.arange(tree.features.shape[0], device=gpu))
    assert tree.subdivide(max_depth=0, own_rows=False) == (res.n_internal, 0, 0, None)
    assert tree.features is old and tree._ver == ver
    frozen = c.tree(gpu)
    frozen.features.requires_grad_(False)
    frozen.subdivide()
    assert not frozen.features.requires_grad and frozen.features.shape[0] == M * 8


def _oracle_tree(tree):
    n = tree.n_internal
    return O.Tree(tree.features.detach().cpu().numpy(), tree.data[:n].cpu().numpy(), tree.child[:n].cpu().numpy(),
                  offset=tree.offset.cpu().numpy(), scaling=tree.invradius.cpu().numpy())


def test_render_and_gradient_behind_a_subdivide(gpu):
    """The subdivided shell_d5 SH9 tree at 64 x 64 against the CPU oracle, on a renderer that has rendered the tree
    BEFORE (acceleration grid, sigma mask and plans are cached on the tensors it saw); then the same tree subdivided
    with shared rows: the same pixels bit for bit, and the gradient of a shared row is the sum of its copies'."""
    c = Case(depth=5, K=28, data_format="SH9", width=64, height=64)
    tree = c.tree(gpu)
    shared = tree.clone()
    tree.static_features = True
    r = svox.VolumeRenderer(tree)
    rays = c.rays_gpu(gpu)
    with torch.no_grad():
        first = r(tree.features, rays, image_shape=(64, 64)).cpu().numpy()
        r.render_depth(tree.features, rays)
    M, K = tree.features.shape
    sel = torch.from_numpy(mask_of("half", c.st.child, c.st.data, M, 9)).to(gpu)
    res = tree.subdivide(sel)
    assert res.nodes_added > 100 and res.rows_added == 7 * res.nodes_added
    ot = _oracle_tree(tree)
    out = r(tree.features, rays, image_shape=(64, 64))
    want = O.volume_render(ot, *c.rays_np(), c.oracle_opts())
    assert_outputs_close(out.detach().cpu().numpy(), want)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), want)        # no stale cache: the NEW tables, bit for bit
    assert not np.array_equal(want, first)                                 # (smaller leaves: other steps)
    with torch.no_grad():
        np.testing.assert_array_equal(r.render_depth(tree.features, rays).cpu().numpy(), O.render_depth(ot, *c.rays_np(), c.oracle_opts()))
    g = synth.grad_output(c.Q, out.shape[1])
    out.backward(g.to(gpu))
    grad_own = tree.features.grad
    want_g, abs_sum = O.volume_render_backward(ot, *c.rays_np(), c.oracle_opts(), g.numpy(), want_abs=True)
    assert_grads_close(grad_own.cpu().numpy(), want_g, abs_sum)
    # shared rows
    res2 = shared.subdivide(sel, own_rows=False)
    assert res2.nodes_added == res.nodes_added and shared.features.shape[0] == M
    r2 = svox.VolumeRenderer(shared)
    out2 = r2(shared.features, rays, image_shape=(64, 64))
    assert torch.equal(out2.detach(), out.detach())
    out2.backward(g.to(gpu))
    want_s, abs_s = O.volume_render_backward(_oracle_tree(shared), *c.rays_np(), c.oracle_opts(), g.numpy(), want_abs=True)
    assert_grads_close(shared.features.grad.cpu().numpy(), want_s, abs_s)
    folded = torch.zeros(M, K, device=gpu).index_add_(0, res.row_map, grad_own)
    assert_grads_close(folded.cpu().numpy(), shared.features.grad.cpu().numpy().astype(np.float64), abs_s)
    assert int((grad_own[M:] != 0).any(1).sum()) > 100                     # the copies have gradients of their own


def test_render_behind_an_unshare_meets_no_stale_cache(gpu):
    c = Case(depth=5, K=28, data_format="SH9", width=64, height=64)
    tree = c.tree(gpu)
    tree.refine()                                                          # eight leaves on every row
    r = svox.VolumeRenderer(tree)
    rays = c.rays_gpu(gpu)
    with torch.no_grad():
        first = r(tree.features, rays, image_shape=(64, 64))
    M = tree.features.shape[0]
    res = tree.unshare()
    assert res.rows_added == 7 * M
    with torch.no_grad():
        tree.features[:M] = 0                                              # only the first leaf of every row reads these now
        again = r(tree.features, rays, image_shape=(64, 64))
    np.testing.assert_array_equal(again.cpu().numpy(), O.volume_render(_oracle_tree(tree), *c.rays_np(), c.oracle_opts()))
    assert not torch.equal(again, first)


def test_adam_state_follows_the_rows(gpu):
    from tests.test_gpu_optim import gradients, run_restated, same_bits
    c = Case(depth=5, K=28, data_format="SH9", width=32, height=32)
    tree = c.tree(gpu)
    M, K = tree.features.shape
    opt = svox.FeatureAdam([tree.features], lr=1e-2)
    grads = gradients(M, K, 1, seed=3)
    tree.features.grad = torch.from_numpy(grads[0]).to(gpu)
    opt.step()
    want_p, want_s = run_restated("adam", True, c.features.numpy(), grads)
    old = tree.features
    res = tree.subdivide(torch.from_numpy(mask_of("half", c.st.child, c.st.data, M, 4)).to(gpu))
    assert tree.features is not old and tree.features.shape[0] == M + res.rows_added > M
    row_map = res.row_map.cpu().numpy()
    opt.rebind(old, tree.features, res.row_map)
    assert opt.param_groups[0]["params"][0] is tree.features and old not in opt.state
    st = opt.state[tree.features]
    assert float(st["step"]) == 1.0
    for k in ("exp_avg", "exp_avg_sq"):                                    # the copies start from their sources' state
        assert same_bits(st[k].cpu().numpy(), want_s[k][row_map])
        assert same_bits(st[k][M:].cpu().numpy(), st[k][res.row_map[M:]].cpu().numpy())
    assert same_bits(tree.features.detach().cpu().numpy(), want_p[row_map])
    g2 = gradients(row_map.shape[0], K, 1, seed=5)
    tree.features.grad = torch.from_numpy(g2[0]).to(gpu)
    opt.step()
    p2, s2 = run_restated("adam", True, want_p[row_map], g2, t0=1, state={k: v[row_map] for k, v in want_s.items()})
    assert same_bits(tree.features.detach().cpu().numpy(), p2)
    for k in ("exp_avg", "exp_avg_sq"):
        assert same_bits(opt.state[tree.features][k].cpu().numpy(), s2[k])
    assert OR.STATE_KEYS["adam"]


def test_accumulate_prune_subdivide_render(gpu, monkeypatch):
    c = Case(depth=5, K=28, data_format="SH9", width=64, height=64)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)

    def accumulate():
        with tree.accumulate_weights() as accum:
            with pytest.raises(RuntimeError, match="Tree locked"):
                tree.subdivide(weights=accum.value, threshold=0.0)
            with torch.no_grad():
                for az in (0.0, 120.0, 240.0):
                    o, d, v = synth.pinhole_rays(64, 64, c2w=synth.camera_pose(azimuth_deg=az))
                    r(tree.features, svox.Rays(o.to(gpu), d.to(gpu), v.to(gpu)))
        return accum.value

    w = accumulate()
    n0, M0 = tree.n_internal, tree.features.shape[0]
    pruned = tree.prune(weights=w, threshold=0.01)
    assert 1 < pruned.n_internal < n0 and 0 < tree.features.shape[0] < M0
    w = accumulate()                                                       # of the pruned tree: the shape of its child
    n1, M1 = tree.n_internal, tree.features.shape[0]
    thr = float(w[:n1][(tree.child[:n1] == 0)].float().quantile(0.7))
    expect = int(((tree.child[:n1] == 0) & (tree.data[:n1, ..., 0] != E) & (w[:n1] >= thr)).sum())
    monkeypatch.setattr(tree, "_all_leaves", lambda: pytest.fail("subdivide went through the host's leaf list"))
    res = tree.subdivide(weights=w, threshold=thr)
    monkeypatch.undo()
    assert tree._last_all_leaves is None
    assert res.nodes_added == expect > 0 and res.n_internal == tree.n_internal == n1 + expect
    assert res.rows_added == 7 * expect and tree.features.shape[0] == M1 + res.rows_added == res.row_map.shape[0]
    R.integrity(tree.child.cpu().numpy(), tree.data.cpu().numpy(), tree.parent_depth.cpu().numpy(), tree.n_internal, 2,
                tree.features.shape[0], n_before=n1, own_rows=True, row_map=res.row_map.cpu().numpy(), M_before=M1)
    with torch.no_grad():
        out = r(tree.features, c.rays_gpu(gpu), image_shape=(64, 64))
    assert bool(torch.isfinite(out).all()) and float(out[:, -1].max()) > 0.5


def test_refusals(gpu):
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=2, map_location=gpu)
    tree.construct_tree(torch.rand(64, 3, generator=torch.Generator().manual_seed(0)).to(gpu))
    tree.features = torch.nn.Parameter(torch.randn(64, 4, device=gpu))
    n, cap, M = tree.n_internal, tree.capacity, 64
    tables = [t.clone() for t in (tree.child, tree.data, tree.parent_depth)]
    feats = tree.features
    ok = torch.ones(tree.child.shape, dtype=torch.bool, device=gpu)

    def untouched():
        return tree.n_internal == n and tree.capacity == cap and tree.features is feats and \
            all(torch.equal(a, b) for a, b in zip(tables, (tree.child, tree.data, tree.parent_depth)))

    # a selection on another device, of another shape or type
    for kw in (dict(sel=ok.cpu()), dict(weights=ok.float().cpu(), threshold=0.0), dict(sel=ok[:-1]), dict(sel=ok.float()),
               dict(sel=ok, weights=ok.float(), threshold=0.0), dict(weights=ok.float()), dict(weights=ok.float(), threshold=float("nan"))):
        with pytest.raises(RuntimeError) as e:
            tree.subdivide(**kw)
        assert not isinstance(e.value, NotImplementedError) and untouched(), kw
    # the slot range: a small limit in the place of 2^31 -- every leaf splitting would need more slots than it allows
    leaves = int((tree.child[:n] == 0).sum())
    tree._slot_limit = (n + leaves) * 8
    with pytest.raises(RuntimeError, match="slot indices"):
        tree.subdivide(split_empty=True)
    assert untouched()
    tree._slot_limit = (n + leaves) * 8 + 1
    assert tree.subdivide(split_empty=True, own_rows=False).nodes_added == leaves
    del tree._slot_limit
    assert tree._slot_limit == 1 << 31
    # ... and the C entry's own extents: the tables must hold the new nodes, and their slots fit 32 bits
    args = (tree.child, tree.data, tree.parent_depth, tree.n_internal, M)
    lib, n2 = _C._lib, tree.n_internal
    torch.cuda.synchronize()
    nbytes = lib.svoxt_subdivide_workspace_bytes(n2, 2, M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    counts = torch.empty(2, dtype=torch.int64, device=gpu)
    ptrs = [t.data_ptr() for t in args[:3]]
    assert lib.svoxt_subdivide_count(*ptrs, n2, 2, M, None, None, 0.0, 10, 1, 1, ws.data_ptr(), nbytes, counts.data_ptr(), None) == 0
    torch.cuda.synchronize()
    added, rows = counts.tolist()
    assert added == int((tree.child[:n2] == 0).sum()) > 0 and rows % 7 == 0
    row_map = torch.empty(M + rows, dtype=torch.int64, device=gpu)
    before = [t.clone() for t in args[:3]]
    for cap_rows, text in ((n2 + added - 1, b"capacity"), (1 << 28, b"2^31")):
        assert lib.svoxt_subdivide_emit(*ptrs, n2, 2, M, cap_rows, 1, ws.data_ptr(), nbytes, added, rows, E, row_map.data_ptr(), None) == 1
        assert text in lib.svoxt_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, args[:3]))
    # rows that would reach the empty index
    with pytest.raises(RuntimeError, match="empty index"):
        _C.subdivide_tree(*args, empty_index=M + 5)
    with pytest.raises(RuntimeError, match="empty index"):
        _C.unshare_rows(tree.child, tree.data, tree.n_internal, M, empty_index=M + 5)
    for bad in ((tree.child.long(),) + args[1:], args[:2] + (tree.parent_depth[:, :1].contiguous(),) + args[3:],
                args[:3] + (tree.capacity + 1,) + args[4:], args[:4] + (-1,), (tree.child.cpu(),) + args[1:]):
        with pytest.raises(RuntimeError) as e:
            _C.subdivide_tree(*bad)
        assert not isinstance(e.value, NotImplementedError)
