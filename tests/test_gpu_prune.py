"""GPU tests of N3Tree.prune (csrc/svoxt_prune.hip) through csrc.prune_tree / N3Tree.prune -> ctypes -> C ABI: the
tables and row_map against the numpy restatement (tests/prune_restate.py), byte for byte; renders, queries and the
renderer's caches behind a prune; the accumulate -> prune -> refine loop; refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from tests import prune_restate as R
from tests.util import Case

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "topology_*.npz")))
TREES = ["shell_d5", "shell_d6", "built_refined"] + FIXTURES
MASKS = ["half", "few", "all", "none", "one"]


def tables_of(name, gpu):
    """(child, data, parent_depth) numpy as allocated (capacity rows), n, M."""
    if name.startswith("shell_d"):
        st = synth.shell_tree(int(name[-1]))
        return st.child, st.data, st.parent_depth, st.n_internal, st.n_features
    if name == "built_refined":                      # rows shared by the 8 slots of every refined leaf; capacity > n
        rng = np.random.default_rng(7)
        d = rng.normal(size=(3000, 3))
        pts = (0.5 + 0.3 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        tree = svox.N3Tree(N=2, data_dim=4, map_location=gpu)
        tree.build_from_points(torch.from_numpy(pts).to(gpu), 5)
        tree.refine()
        assert tree.capacity >= tree.n_internal
        return (tree.child.cpu().numpy(), tree.data.cpu().numpy(), tree.parent_depth.cpu().numpy(), tree.n_internal,
                pts.shape[0])
    g = np.load(os.path.join(G, name))
    child, n = g["child"], int(g["n_internal"])
    data, M = R.number_leaves(child, n, np.random.default_rng(n))
    return child, data, g["parent_depth"], n, M


def mask_of(kind, child, data, M, seed):
    rng = np.random.default_rng(seed)
    if kind == "half":
        return rng.random(child.shape) < 0.5
    if kind == "few":
        return rng.random(child.shape) < 0.05
    if kind in ("all", "none"):
        return np.full(child.shape, kind == "all")
    one = np.zeros(child.shape, bool)
    full = np.nonzero((child.reshape(-1) == 0) & ((data.reshape(-1).astype(np.int64) & 0xFFFFFFFF) < M))[0]
    one.reshape(-1)[full[len(full) // 2]] = True
    return one


def hip_prune(gpu, child, data, pd, n, M, **kw):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)      # noqa: E731
    for k in ("keep", "weights"):
        if k in kw:
            kw[k] = t(kw[k])
    c, d, p, n2, row_map, *dropped = _C.prune_tree(t(child), t(data), t(pd), n, M, **kw)
    return (c.cpu().numpy(), d.cpu().numpy(), p.cpu().numpy(), n2, None if row_map is None else row_map.cpu().numpy(), *dropped)


def assert_same(got, want):
    for g, w, what in zip(got[:3], want[:3], ("child", "data", "parent_depth")):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        np.testing.assert_array_equal(g, w, err_msg=what)
    assert got[3] == want[3]
    if want[4] is None:
        assert got[4] is None
    else:
        assert got[4].dtype == np.int64
        np.testing.assert_array_equal(got[4], want[4], err_msg="row_map")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", TREES)
def test_tables_and_row_map_equal_the_restatement(gpu, name, mask):
    child, data, pd, n, M = tables_of(name, gpu)
    N = child.shape[1]
    keep = mask_of(mask, child, data, M, seed=len(name) + n)
    for collapse in (True, False):
        for compact in (True, False):
            for reserve in (0, 7):
                kw = dict(keep=keep, collapse=collapse, compact_features=compact, reserve=reserve)
                want = R.prune(child, data, pd, n, M, **kw)
                got = hip_prune(gpu, child, data, pd, n, M, **kw)
                assert_same(got, want)
                R.integrity(got[0], got[1], got[2], got[3], N, M if got[4] is None else len(got[4]), collapsed=collapse)
    # uint8 decisions are read like bool ones; two runs give the same bytes
    first = hip_prune(gpu, child, data, pd, n, M, keep=keep, reserve=7)
    again = hip_prune(gpu, child, data, pd, n, M, keep=keep.astype(np.uint8) * 3, reserve=7)
    assert_same(again, first)
    for a, b in zip(again[:3], first[:3]):
        assert a.tobytes() == b.tobytes()


def test_a_tree_above_the_stride_bound_equals_the_restatement(gpu):
    """synth.shell_tree(8) has 990 728 slots: more than 2048 workgroups of 256, so the mark pass strides and sums its
    drop counts over all 2048 workgroups (shell_d6 and the fixtures stay below the bound).  One case."""
    st = synth.shell_tree(8)
    child, data, pd, n, M = st.child, st.data, st.parent_depth, st.n_internal, st.n_features
    assert n * child.shape[1] ** 3 > 2048 * 256
    kw = dict(keep=mask_of("half", child, data, M, seed=8), collapse=True, compact_features=True)
    want = R.prune(child, data, pd, n, M, **kw)
    got = hip_prune(gpu, child, data, pd, n, M, return_dropped=True, **kw)
    assert_same(got, want)
    assert got[5] == want[5]
    R.integrity(got[0], got[1], got[2], got[3], child.shape[1], len(got[4]), collapsed=True)


@pytest.mark.parametrize("name", ["shell_d5", "built_refined", "topology_full_n3_l2.npz"])
def test_weights_and_threshold(gpu, name):
    child, data, pd, n, M = tables_of(name, gpu)
    rng = np.random.default_rng(3)
    w = rng.random(child.shape).astype(np.float32)
    flat = w.reshape(-1)
    full = np.nonzero((child.reshape(-1) == 0) & ((data.reshape(-1).astype(np.int64) & 0xFFFFFFFF) < M))[0]
    thr = float(np.float32(0.4))
    flat[full[0::7]] = np.nan                        # dropped
    flat[full[1::7]] = np.float32(thr)               # kept: >=
    flat[full[2::7]] = np.nextafter(np.float32(thr), np.float32(0))
    flat[full[3::7]] = np.inf
    for collapse in (True, False):
        want = R.prune(child, data, pd, n, M, weights=w, threshold=thr, collapse=collapse)
        got = hip_prune(gpu, child, data, pd, n, M, weights=w, threshold=thr, collapse=collapse)
        assert_same(got, want)
    kept_rows = set(want[4].tolist())
    rows = data.reshape(-1)
    assert all(int(rows[s]) in kept_rows for s in full[1::7]) and len(full[0::7]) > 0


def test_leaves_dropped_and_the_result_object(gpu):
    c = Case(depth=5, K=4, data_format="RGBA", width=8, height=8)
    tree = c.tree(gpu)
    keep = mask_of("half", c.st.child, c.st.data, c.st.n_features, 11)
    want = R.prune(c.st.child, c.st.data, c.st.parent_depth, c.st.n_internal, c.st.n_features, keep=keep, reserve=5)
    feats = tree.features.detach().clone()
    res = tree.prune(torch.from_numpy(keep).to(gpu), reserve=5)
    assert (res.n_internal, res.nodes_removed, res.leaves_dropped) == (want[3], c.st.n_internal - want[3], want[5])
    assert tree.n_internal == tree.filled == want[3] == int(tree._n_internal) and tree.capacity == want[3] + 5
    np.testing.assert_array_equal(res.row_map.cpu().numpy(), want[4])
    np.testing.assert_array_equal(tree.child.cpu().numpy(), want[0])
    np.testing.assert_array_equal(tree.data.cpu().numpy(), want[1])
    assert isinstance(tree.features, torch.nn.Parameter) and tree.features.requires_grad
    assert torch.equal(tree.features.detach(), feats[res.row_map])              # the HIP gather = torch indexing
    f6 = torch.randn(c.st.n_features, 6, device=gpu)                                        # rows that are not multiples of 16 bytes
    assert torch.equal(_C.gather_rows(f6, res.row_map[:300]), f6[res.row_map[:300]])
    assert tree.shrink_to_fit() is True and tree.capacity == want[3] and tree.shrink_to_fit() is False


def _views(gpu, n_cams=6, side=8):
    """Cameras of side x side pixels: one 8x8 tile each, so that a feature row's gradient is one per-tile sum added
    once to a zeroed table -- the same bits in every run (with several tiles the order in which their float atomics
    arrive is not fixed, and neither are the last bits: tests/test_gpu_bench_contract.py)."""
    out = []
    for k in range(n_cams):
        o, d, v = synth.pinhole_rays(side, side, c2w=synth.camera_pose(azimuth_deg=20.0 + 57.0 * k, elevation_deg=-30.0 + 15.0 * k))
        out.append(svox.Rays(o.to(gpu), d.to(gpu), v.to(gpu)))
    return out


def test_dropping_leaves_that_contribute_nothing_changes_no_render(gpu):
    """collapse=False, dropping only leaves whose sigma is <= 0 (or that were empty already): no leaf's geometry
    changes and the dropped leaves composite nothing (rt_kernel.cu:279, 382), so pixels, depth and the feature gradient
    -- scattered back through row_map -- are bit for bit the unpruned tree's.  This is what catches a wrong remap."""
    c = Case(depth=6, K=28, data_format="SH9", width=64, height=64)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    M, K = tree.features.shape
    rays = c.rays_gpu(gpu)
    views = _views(gpu)

    def renders():
        with torch.no_grad():
            out = r(tree.features, rays, image_shape=(64, 64)).cpu().numpy()
            depth = r.render_depth(tree.features, rays).cpu().numpy()
        grads = []
        for i, v in enumerate(views):
            tree.features.grad = None
            o = r(tree.features, v, image_shape=(8, 8))
            o.backward(synth.grad_output(64, o.shape[1], seed=i).to(gpu))
            grads.append(tree.features.grad.clone())
        return out, depth, grads

    out0, depth0, grads0 = renders()
    sigma = tree.features.detach()[:, -1]
    idx = tree.data[..., 0].long()
    keep = (tree.child == 0) & (idx < M) & (sigma[idx.clamp(0, M - 1)] > 0)
    res = tree.prune(keep, collapse=False)
    assert res.nodes_removed == 0 and 0 < res.leaves_dropped == int((sigma <= 0).sum()) and tree.features.shape[0] == M - res.leaves_dropped
    out1, depth1, grads1 = renders()
    np.testing.assert_array_equal(out1, out0)
    np.testing.assert_array_equal(depth1, depth0)
    touched = 0
    for g0, g1 in zip(grads0, grads1):
        back = torch.zeros(M, K, device=gpu)
        back[res.row_map] = g1
        assert torch.equal(back, g0)
        touched += int((g0 != 0).any(1).sum())
    assert touched > 300


def test_queries_behind_a_collapsing_prune(gpu):
    c = Case(depth=5, K=4, data_format="RGBA", width=8, height=8)
    tree = c.tree(gpu)
    g = torch.Generator().manual_seed(2)
    pts = torch.rand(20000, 3, generator=g).to(gpu)
    with torch.no_grad():
        before, leaf_ids, rows = tree(tree.features, pts, want_node_ids=True, want_data_ids=True)
    assert int((rows >= 0).sum()) > 200
    keep = torch.from_numpy(mask_of("half", c.st.child, c.st.data, c.st.n_features, 4)).to(gpu)
    kept = keep.reshape(-1)[leaf_ids] & (rows >= 0)
    tree.prune(keep)
    with torch.no_grad():
        after, _, rows2 = tree(tree.features, pts, want_node_ids=True, want_data_ids=True)
    assert int(kept.sum()) > 50 and int((~kept & (rows >= 0)).sum()) > 50
    assert torch.equal(after[kept], before[kept]) and bool((rows2[kept] >= 0).all())
    # a dropped leaf answers like any empty leaf: a row of zeros, row index -1
    assert not after[~kept].any() and bool((rows2[~kept] == -1).all())


def test_render_after_a_collapsing_prune_meets_no_stale_cache(gpu):
    """The renderer object has rendered the tree before (acceleration grid, sigma mask and plans are cached on the
    tensors it saw); behind prune() it must render the NEW tables: bit for bit the CPU oracle's render of them."""
    c = Case(depth=6, K=28, data_format="SH9", width=64, height=64)
    tree = c.tree(gpu)
    tree.static_features = True                       # lets the sigma bitmask be cached too
    r = svox.VolumeRenderer(tree)
    rays = c.rays_gpu(gpu)
    with torch.no_grad():
        first = r(tree.features, rays, image_shape=(64, 64)).cpu().numpy()
        r.render_depth(tree.features, rays)
    keep = torch.from_numpy(mask_of("half", c.st.child, c.st.data, c.st.n_features, 9)).to(gpu)
    res = tree.prune(keep)
    assert res.nodes_removed > 0
    n = tree.n_internal
    ot = O.Tree(tree.features.detach().cpu().numpy(), tree.data[:n].cpu().numpy(), tree.child[:n].cpu().numpy(),
                offset=tree.offset.cpu().numpy(), scaling=tree.invradius.cpu().numpy())
    with torch.no_grad():
        got = r(tree.features, rays, image_shape=(64, 64)).cpu().numpy()
        depth = r.render_depth(tree.features, rays).cpu().numpy()
    np.testing.assert_array_equal(got, O.volume_render(ot, *c.rays_np(), c.oracle_opts()))
    np.testing.assert_array_equal(depth, O.render_depth(ot, *c.rays_np(), c.oracle_opts()))
    assert not np.array_equal(got, first)
    # ... and the gradient has the new table's shape
    out = r(tree.features, rays, image_shape=(64, 64))
    out.sum().backward()
    assert tree.features.grad.shape == tree.features.shape and bool(torch.isfinite(tree.features.grad).all())


def test_accumulate_prune_refine_render(gpu):
    c = Case(depth=5, K=28, data_format="SH9", width=64, height=64)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    with tree.accumulate_weights() as accum:
        with pytest.raises(RuntimeError, match="Tree locked"):
            tree.prune(weights=accum.value, threshold=0.0)
        with torch.no_grad():
            for az in (0.0, 120.0, 240.0):
                o, d, v = synth.pinhole_rays(64, 64, c2w=synth.camera_pose(azimuth_deg=az))
                r(tree.features, svox.Rays(o.to(gpu), d.to(gpu), v.to(gpu)))
    w = accum.value
    assert float(w.max()) > 0
    n0, M0 = tree.n_internal, tree.features.shape[0]
    res = tree.prune(weights=w, threshold=0.01)
    assert 1 < res.n_internal < n0 and 0 < tree.features.shape[0] < M0
    tree.refine()
    n = tree.n_internal
    assert n > res.n_internal
    R.integrity(tree.child.cpu().numpy(), tree.data.cpu().numpy(), tree.parent_depth.cpu().numpy(), n, 2,
                tree.features.shape[0], collapsed=False, pruned=False)
    with torch.no_grad():
        out = r(tree.features, c.rays_gpu(gpu), image_shape=(64, 64))
    assert bool(torch.isfinite(out).all()) and float(out[:, -1].max()) > 0.5


def test_refusals(gpu):
    cpu_tree = svox.N3Tree(N=2, data_dim=4, init_refine=1)
    with pytest.raises(RuntimeError, match="GPU"):
        cpu_tree.prune(torch.ones(cpu_tree.child.shape, dtype=torch.bool))
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=2, map_location=gpu)
    args = (tree.child, tree.data, tree.parent_depth, tree.n_internal, tree.features.shape[0])
    ok = torch.ones(tree.child.shape, dtype=torch.bool, device=gpu)
    bad = [dict(), dict(keep=ok, weights=ok.float(), threshold=0.0), dict(keep=ok.float()), dict(keep=ok[:-1]),
           dict(keep=ok.cpu()), dict(keep=ok.reshape(-1)), dict(weights=ok.float()), dict(weights=ok.double(), threshold=0.0),
           dict(weights=ok.float(), threshold=float("nan")), dict(keep=ok, threshold=0.5), dict(keep=ok, reserve=-1),
           dict(keep=ok.permute(0, 3, 2, 1))]
    for kw in bad:
        with pytest.raises(RuntimeError) as e:
            _C.prune_tree(*args, **kw)
        assert not isinstance(e.value, NotImplementedError), kw
    for a in ((tree.child.long(),) + args[1:], args[:2] + (tree.parent_depth[:, :1].contiguous(),) + args[3:],
              args[:3] + (tree.capacity + 1,) + args[4:], args[:4] + (-1,)):
        with pytest.raises(RuntimeError) as e:
            _C.prune_tree(*a, keep=ok)
        assert not isinstance(e.value, NotImplementedError)
    assert _C.prune_tree(*args, keep=ok)[3] == 1           # a tree without a feature index: the root alone remains


def test_a_tree_left_without_rows_is_refused_cleanly(gpu):
    """Nothing kept: the root alone, a [0, K] feature table.  No render or query kernel is launched on it: the operator
    boundary refuses a table without rows (RuntimeError) until the tree has rows again."""
    c = Case(depth=5, K=28, data_format="SH9", width=8, height=8)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    res = tree.prune(torch.zeros(tree.child.shape, dtype=torch.bool, device=gpu))
    assert (res.n_internal, res.leaves_dropped, tuple(res.row_map.shape)) == (1, c.st.n_features, (0,))
    assert tuple(tree.features.shape) == (0, 28) and tree.capacity == 1
    assert not tree.child.any() and bool((tree.data == svox.svox.EMPTY_INDEX).all())
    rays = c.rays_gpu(gpu)
    for call in (lambda: r(tree.features, rays), lambda: r.render_depth(tree.features, rays),
                 lambda: r.opacity_render(tree.features, rays), lambda: tree(tree.features, rays.origins),
                 lambda: r.render_persp(tree.features, torch.eye(4)[:3], width=8, height=8)):
        with pytest.raises(RuntimeError, match="no rows") as e:
            call()
        assert not isinstance(e.value, NotImplementedError)
    # rows again: the tree renders (all leaves empty: background only)
    with torch.no_grad():
        out = r(torch.zeros(1, 28, device=gpu), rays)
    assert bool((out[:, -1] == 0).all())
