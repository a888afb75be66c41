"""N3Tree.interp on the GPU: the stencil, the value, the table gradient and the point gradient bit for bit against the
numpy restatement (tests/interp_restate.py), the corner rows against the existing nearest-leaf query at the cell centres
(integer equality), placement, and torch.autograd end to end.

Trees: the topologies of tests/golden/topology_points_a (N = 2, level changes), shell_d4 (N = 2) and full_n3_l2 (N = 3),
with the rows in a random permutation, every third leaf empty, world offset and scaling non-trivial.  Points: leaf
centres, points on faces, edges and corners of leaves, 0.0 and 1.0, points outside the cube, and random ones -- 2 000 in
a fixed shuffle, of which a test takes the first Q.  The references are computed once per (tree, coordinates, fill)."""
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from svox_t_amd import synth
from tests import interp_restate as IR
from tests import rows_restate as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
E = synth.EMPTY_SENTINEL
_X = _C._extras
KINDS = {"points_a": "topology_points_a.npz", "shell_d4": "topology_shell_d4.npz", "full_n3": "topology_full_n3_l2.npz"}
RADIUS, CENTER = [1.0, 2.0, 0.25], [0.1, -0.2, 0.3]
SENTINEL = 0x7FC0FFEE
_TREES, _POINTS, _STENCILS = {}, {}, {}


def bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def build(kind, gpu, K):
    """(tree on the GPU with a [M, K] table, restatement trees for world and local coordinates, the table as numpy)."""
    key = (kind, K)
    if key not in _TREES:
        g = np.load(os.path.join(G, KINDS[kind]))
        child, pd = g["child"], g["parent_depth"]
        rng = np.random.default_rng(7)
        leaf = child.reshape(-1) == 0
        L = int(leaf.sum())
        words = rng.permutation(L).astype(np.int32)
        words[2::3] = E
        data = np.full(child.size, E, np.int32)
        data[leaf] = words
        table = rng.standard_normal((L, K)).astype(np.float32)
        table[table == 0] = 1.0
        tree = svox.N3Tree.from_arrays(child, data, pd, table, radius=RADIUS, center=CENTER, device=gpu)
        world = IR.tree_of(child, data, L, tree.offset.cpu().numpy(), tree.invradius.cpu().numpy())
        local = IR.tree_of(child, data, L)
        _TREES[key] = (tree, {True: world, False: local}, table)
    return _TREES[key]


def points_for(kind, gpu, world):
    """float32 [2000, 3] numpy, in a fixed shuffle: the point classes of the module docstring, in the coordinates asked for."""
    key = (kind, world)
    if key not in _POINTS:
        tree, _, _ = build(kind, gpu, 4)
        lb = tree.leaf_boxes(world=False)
        c, ln = lb.corners.cpu().numpy().astype(np.float64), lb.lengths.cpu().numpy().astype(np.float64)
        rng = np.random.default_rng(13)
        L = c.shape[0]

        def on_leaves(n, u):
            i = rng.integers(0, L, n)
            return c[i] + u * ln[i]

        centres = on_leaves(300, 0.5)
        mask = rng.integers(0, 2, (500, 3)).astype(bool)
        mask[mask.sum(axis=1) == 0, 0] = True                      # faces, edges and corners: 1, 2 or 3 axes on a boundary
        u = np.where(mask, rng.integers(0, 2, (500, 3)).astype(np.float64), rng.random((500, 3)))
        borders = on_leaves(500, u)
        inside = on_leaves(900, rng.random((900, 3)))
        outside = rng.random((280, 3)) * 3 - 1
        special = np.array([[0, 0, 0], [1, 1, 1], [0, 1, 0.5], [1, 0, 0.25], [0.5, 0.5, 0.5], [0, 0.3, 1]] + [[0.0, 0.0, 0.0]] * 14)
        special[6:] = rng.integers(0, 2, (14, 3))
        p = np.concatenate([centres, borders, inside, outside, special])
        assert p.shape == (2000, 3)
        p = p[rng.permutation(2000)].astype(np.float32)
        if world:
            off, sc = tree.offset.cpu().numpy(), tree.invradius.cpu().numpy()
            p = ((p - off) / sc).astype(np.float32)
        _POINTS[key] = p
    return _POINTS[key]


def stencil_ref(kind, gpu, world, fill):
    key = (kind, world, fill)
    if key not in _STENCILS:
        _, trees, _ = build(kind, gpu, 4)
        _STENCILS[key] = IR.stencil(trees[world], points_for(kind, gpu, world), fill)
    return _STENCILS[key]


def cut(st, Q):
    return IR.Stencil(*(x[:Q] for x in st))


# 1. the stencil -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("Q", [0, 1, 63, 64, 65, 2000])
def test_stencil(gpu, kind, Q):
    tree, _, _ = build(kind, gpu, 4)
    for world in (True, False):
        pts = torch.from_numpy(points_for(kind, gpu, world)[:Q]).to(gpu)
        for fill in ("self", "zero"):
            want = cut(stencil_ref(kind, gpu, world, fill), Q)
            st = tree.interp_stencil(pts, world=world, fill=fill)
            assert isinstance(st, svox.InterpStencil) and st.rows.dtype == torch.int32 and tuple(st.rows.shape) == (Q, 8)
            np.testing.assert_array_equal(st.rows.cpu().numpy(), want.rows)
            np.testing.assert_array_equal(bits(st.weights), bits(want.weights))
            again = tree.interp_stencil(pts, world=world, fill=fill)
            assert torch.equal(again.rows, st.rows) and torch.equal(again.weights, st.weights)
        if not world:
            li = tree.interp_stencil(svox.LocalIndex(pts))
            assert torch.equal(li.rows, tree.interp_stencil(pts, world=False).rows)
    if Q == 2000:
        want = stencil_ref(kind, gpu, True, "zero")
        own = want.rows[:, 0]
        assert (own < 0).sum() > 100 and (own >= 0).sum() > 1000                       # empty and occupied query leaves
        assert ((want.rows[own >= 0, 1:] < 0).sum() > 100)                             # corners without a row
        assert (want.clamped.any(axis=1).sum() > 100)


# 2. values and gradients ----------------------------------------------------------------------------------------------
DIMS = {"all": None, "one": -1, "slice": slice(0, 3)}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("K", [1, 4, 28, 32])
@pytest.mark.parametrize("dim", list(DIMS))
def test_values_and_gradients(gpu, kind, K, dim):
    tree, trees, table = build(kind, gpu, K)
    fill = "self" if K in (1, 28) else "zero"
    world = K != 4
    M = table.shape[0]
    Q = 2000
    p_np = points_for(kind, gpu, world)
    want_st = stencil_ref(kind, gpu, world, fill)
    cols = None if DIMS[dim] is None else np.arange(K)[DIMS[dim]].reshape(-1)
    C = K if cols is None else cols.shape[0]
    rng = np.random.default_rng(K * 7 + len(dim))
    g_np = rng.standard_normal((Q, C)).astype(np.float32)
    want = IR.value(table, want_st.rows, want_st.weights, cols)
    want_G = IR.table_grad(g_np, want_st.rows, want_st.weights, M, K, cols)
    want_gp = IR.point_grad(trees[world], want_st, table, g_np, cols)

    def run():
        feats = tree.features.detach().clone().requires_grad_(True)
        p = torch.from_numpy(p_np).to(gpu).requires_grad_(True)
        out = tree.interp(p, features=feats, dim=DIMS[dim], world=world, fill=fill)
        assert tuple(out.shape) == (Q, C)
        out.backward(torch.from_numpy(g_np).to(gpu))
        return out.detach(), feats.grad, p.grad

    out, G_, gp = run()
    np.testing.assert_array_equal(bits(out), bits(want))
    np.testing.assert_array_equal(bits(G_), bits(want_G))
    np.testing.assert_array_equal(bits(gp), bits(want_gp))
    assert tuple(G_.shape) == (M, K) and tuple(gp.shape) == (Q, 3)
    out2, G2, gp2 = run()                                                              # the same bits on a second run
    assert torch.equal(out2, out) and torch.equal(G2, G_) and torch.equal(gp2, gp)
    # without a gradient for the points: interp_rows over a stencil, the same bits
    st = tree.interp_stencil(torch.from_numpy(p_np).to(gpu), world=world, fill=fill)
    feats = tree.features.detach().clone().requires_grad_(True)
    o3 = svox.interp_rows(st, feats, DIMS[dim])
    o3.backward(torch.from_numpy(g_np).to(gpu))
    assert torch.equal(o3.detach(), out) and torch.equal(feats.grad, G_)
    assert st.row_plan(M) is st.row_plan(M)                                            # cached per M
    assert np.abs(want_gp).max() > 0 and (want_gp[want_st.clamped] == 0).all()


# 3. anchors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_corner_rows_are_the_query_at_the_cell_centres(gpu, kind):
    """rows[q, j] = data_ids of tree.forward at X_j, the centre of cell t_j built on the host in float64 from
    leaf_boxes(world=False) (exact for N = 2), wherever X_j is inside the cube and that leaf has a row; elsewhere the own
    row ("self") or -1 ("zero").  Integer equality."""
    tree, _, _ = build(kind, gpu, 4)
    N = tree.N
    p_np = points_for(kind, gpu, False)
    if N != 2:                                                     # off the centre planes, where float64 corners decide s like l does
        rng = np.random.default_rng(3)
        lb0 = tree.leaf_boxes(world=False)
        i = rng.integers(0, lb0.corners.shape[0], 2000)
        u = 0.05 + 0.9 * rng.random((2000, 3))
        u = np.where(np.abs(u - 0.5) < 0.02, 0.3, u)
        p_np = (lb0.corners.cpu().numpy().astype(np.float64)[i] + u * lb0.lengths.cpu().numpy().astype(np.float64)[i]).astype(np.float32)
    pts = torch.from_numpy(p_np).to(gpu)
    lb = tree.leaf_boxes(world=False)
    _, slot, own = tree.forward(tree.features, pts, world=False, want_node_ids=True, want_data_ids=True)
    packed = tree._pack_index(lb.leaf_node)
    order = torch.argsort(packed)
    leaf = order[torch.searchsorted(packed[order], slot)]
    assert torch.equal(packed[leaf], slot)
    corner, length = lb.corners[leaf].double(), lb.lengths[leaf].double()
    centre = corner + 0.5 * length
    # the clamped point decides the side (outside the cube too)
    s = torch.where(pts.clamp(0.0, float(np.float32(1.0 - 1e-6))).double() - centre < 0, -1.0, 1.0)
    own = own.cpu().numpy()
    seen = 0
    for fill in ("self", "zero"):
        st = tree.interp_stencil(pts, world=False, fill=fill)
        rows = st.rows.cpu().numpy()
        for j in range(8):
            b = torch.tensor([(j >> 2) & 1, (j >> 1) & 1, j & 1], dtype=torch.float64, device=gpu)
            X = centre + b[None, :] * s * length
            inside = ((X > 0) & (X < 1)).all(dim=1).cpu().numpy()
            _, ids = tree.forward(tree.features, X.float().contiguous(), world=False, want_data_ids=True)
            ids = ids.cpu().numpy()
            has = inside & (ids >= 0)
            want = np.where(has, ids, own if fill == "self" else -1)
            want = np.where(own < 0, -1, want)
            np.testing.assert_array_equal(rows[:, j], want, err_msg=f"{kind} {fill} corner {j}")
            seen += int((has & (own >= 0) & (ids != own)).sum())
    assert seen > 2000
    if kind == "points_a":                                         # corners that fall into finer and into coarser leaves
        depth = lb.depths[leaf].cpu().numpy()
        assert len(set(depth.tolist())) > 1


@pytest.mark.parametrize("kind", ["points_a", "shell_d4"])
def test_exact_leaf_centres_have_the_bits_of_forward(gpu, kind):
    tree, _, _ = build(kind, gpu, 28)
    lb = tree.leaf_boxes(world=False)
    pts = (lb.corners + 0.5 * lb.lengths).contiguous()             # exact for N = 2
    with torch.no_grad():
        want = tree.forward(tree.features, pts, world=False)
        for fill in ("self", "zero"):
            got = tree.interp(pts, world=False, fill=fill)
            assert torch.equal(got, want)
    assert int((lb.rows >= 0).sum()) > 50 and int((lb.rows < 0).sum()) > 10


def test_long_rows(gpu):
    """600 points inside one leaf: its own row has more than two chunks of 256 entries."""
    tree, trees, table = build("shell_d4", gpu, 4)
    M, K = table.shape
    lb = tree.leaf_boxes(world=False)
    i = int((lb.rows >= 0).nonzero()[5])
    rng = np.random.default_rng(21)
    p_np = (lb.corners[i].cpu().numpy()[None, :] + rng.random((600, 3)) * lb.lengths[i].cpu().numpy()[None, :]).astype(np.float32)
    g_np = rng.standard_normal((600, K)).astype(np.float32)
    want_st = IR.stencil(trees[False], p_np, "self")
    assert (want_st.rows[:, 0] == int(lb.rows[i])).all()
    assert np.bincount(want_st.rows.reshape(-1)[want_st.rows.reshape(-1) >= 0], minlength=M).max() > 2 * R.CHUNK
    feats = tree.features.detach().clone().requires_grad_(True)
    st = tree.interp_stencil(torch.from_numpy(p_np).to(gpu), world=False)
    out = svox.interp_rows(st, feats)
    g = torch.from_numpy(g_np).to(gpu)
    out.backward(g)
    np.testing.assert_array_equal(bits(feats.grad), bits(IR.table_grad(g_np, want_st.rows, want_st.weights, M, K)))
    plan = st.row_plan(M)
    assert plan.longest > 2 * R.CHUNK and plan.long_rows.shape[0] >= 1
    # reduce_rows' order by construction: the [8 Q, C] tensor the operator never forms, through reduce_rows over the same plan
    vals = (st.weights.reshape(-1)[:, None] * g.repeat_interleave(8, dim=0)).contiguous()
    assert torch.equal(_C.sample_reduce_rows(vals, plan.arrays, "sum", 0.0), feats.grad)


# 4. placement ---------------------------------------------------------------------------------------------------------
def shifted(t, s):
    """(view, buffer): the values of t, s elements into a buffer whose other words hold SENTINEL; the view is contiguous
    and starts 4 s bytes behind the buffer's 16-byte aligned start (the idiom of tests/test_gpu_placement.py)."""
    n = t.numel()
    buf = torch.empty(s + n + 4, dtype=t.dtype, device=t.device)
    buf.view(torch.int32).fill_(SENTINEL)
    buf[s:s + n].copy_(t.detach().reshape(-1))
    view = buf[s:s + n].view(t.shape)
    assert view.is_contiguous() and buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + s * t.element_size()
    return view, buf


def assert_guards(buf, s, n):
    w = buf.view(torch.int32)
    assert bool((w[:s] == SENTINEL).all()) and bool((w[s + n:] == SENTINEL).all())


@pytest.mark.parametrize("K", [4, 32, 7])
def test_placement(gpu, K):
    """points, table, grad_out and out starting 4, 8 and 12 bytes off a 16-byte boundary: the same bits."""
    import ctypes
    tree, _, table = build("points_a", gpu, K)
    M = table.shape[0]
    Q = 333
    p0 = torch.from_numpy(points_for("points_a", gpu, True)[:Q]).to(gpu)
    g0 = torch.from_numpy(np.random.default_rng(5).standard_normal((Q, K)).astype(np.float32)).to(gpu)
    f0 = tree.features.detach().clone()
    assert p0.data_ptr() % 16 == 0 and g0.data_ptr() % 16 == 0 and f0.data_ptr() % 16 == 0

    def run(p, f, g):
        f = f.requires_grad_(True)
        p = p.requires_grad_(True)
        out = tree.interp(p, features=f)
        out.backward(g)
        return out.detach(), f.grad, p.grad

    base = run(p0.clone(), f0.clone(), g0)
    st = tree.interp_stencil(p0)
    spec = tree._spec(f0)
    for s in (1, 2, 3):
        pv, pbuf = shifted(p0, s)
        fv, fbuf = shifted(f0, s)
        gv, gbuf = shifted(g0, s)
        for got in (run(pv.detach(), f0.clone(), g0), run(p0.clone(), fv.detach(), g0)):
            for a, b in zip(got, base):
                assert torch.equal(a, b)
        # grad_out: the two backwards on a shifted upstream gradient (autograd would hand over its own tensor)
        assert torch.equal(_X.interp_rows_bwd(gv, st.weights, st.row_plan(M).arrays, None, K), base[1])
        assert torch.equal(_X.interp_points_bwd(spec, p0, st.rows, f0, gv, None), base[2])
        assert torch.equal(_X.interp_points_bwd(tree._spec(fv), pv, st.rows, fv, gv, None), base[2])
        # out: the forward writes into a shifted output, nothing around it
        ov, obuf = shifted(torch.zeros(Q, K, device=gpu), s)
        _X._call("svoxt_interp_rows_fwd", ctypes.c_void_p(f0.data_ptr()), M, K, ctypes.c_void_p(st.rows.data_ptr()),
                 ctypes.c_void_p(st.weights.data_ptr()), Q, None, 0, ctypes.c_void_p(ov.data_ptr()), _X._stream(gpu))
        torch.cuda.synchronize()
        assert torch.equal(ov, base[0])
        assert_guards(obuf, s, Q * K)
        for buf, n in ((pbuf, Q * 3), (fbuf, M * K), (gbuf, Q * K)):
            assert_guards(buf, s, n)


# 5. autograd end to end -----------------------------------------------------------------------------------------------
def test_both_gradients_through_autograd(gpu):
    tree, trees, table = build("shell_d4", gpu, 4)
    tree.features.grad = None
    p = torch.from_numpy(points_for("shell_d4", gpu, True)[:500]).to(gpu).requires_grad_(True)
    tree.interp(p).sum().backward()
    assert p.grad is not None and tree.features.grad is not None
    assert tuple(p.grad.shape) == (500, 3) and tuple(tree.features.grad.shape) == tuple(tree.features.shape)
    assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 and float(tree.features.grad.abs().max()) > 0
    st = stencil_ref("shell_d4", gpu, True, "self")
    ones = np.ones((500, 4), np.float32)
    np.testing.assert_array_equal(bits(p.grad), bits(IR.point_grad(trees[True], cut(st, 500), table, ones)))
    np.testing.assert_array_equal(bits(tree.features.grad), bits(IR.table_grad(ones, st.rows[:500], st.weights[:500], *table.shape)))
    tree.features.grad = None
    # points without a gradient: the table's alone
    q = p.detach()
    tree.interp(q, dim=-1).sum().backward()
    assert tree.features.grad is not None and float(tree.features.grad[:, :3].abs().max()) == 0
    tree.features.grad = None


def test_ray_samples_points_feed_interp(gpu):
    from tests.util import Case
    c = Case(depth=5, K=4, data_format="RGBA", width=8, height=8)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    rays = c.rays_gpu(gpu)
    s = r.ray_samples(rays, min_sigma=0.0)
    assert s.Q == 64 and len(s) > 100
    pts = s.points(rays)
    z = (s.depth + 0.5 * s.length)[:, None]
    assert torch.equal(pts, rays.origins[s.ray.long()] + rays.dirs[s.ray.long()] * z) and not pts.requires_grad
    feats = tree.features.detach().clone().requires_grad_(True)
    f = tree.interp(pts, features=feats)
    w, alpha = svox.sample_weights(s, f[:, -1].contiguous())
    out = svox.accumulate(s, w, f[:, :3].contiguous())
    assert tuple(out.shape) == (64, 3)
    (out.sum() + alpha.sum()).backward()
    assert bool(torch.isfinite(feats.grad).all()) and float(feats.grad.abs().max()) > 0
    t = IR.tree_of(c.st.child, c.st.data, c.features.shape[0], tree.offset.cpu().numpy(), tree.invradius.cpu().numpy())
    st = IR.stencil(t, pts.cpu().numpy())
    np.testing.assert_array_equal(bits(f), bits(IR.value(c.features.numpy(), st.rows, st.weights)))
    # the mid-points lie in the leaves the march crossed: corner 0 is the sample's own row
    assert float((torch.from_numpy(st.rows[:, 0]).to(gpu) == s.row).float().mean()) > 0.9


def test_axis_aligned_ray_mid_points_are_leaf_centres(gpu):
    """A full N = 2 tree of 8^3 leaves, rays along +x through the leaf centres, step_size 0: every mid-point is an exact
    leaf centre, so the interpolated rows are gather_rows' bit for bit."""
    child, data, pd, L = IR.uniform_tree(3)
    rng = np.random.default_rng(4)
    table = rng.standard_normal((L, 4)).astype(np.float32)
    table[:, -1] = np.abs(table[:, -1]) + 0.1
    tree = svox.N3Tree.from_arrays(child, data, pd, table, device=gpu)
    r = svox.VolumeRenderer(tree, step_size=0.0)
    yz = (torch.arange(8, dtype=torch.float32) + 0.5) / 8
    o = torch.stack([torch.full((64,), -0.5), yz.repeat_interleave(8), yz.repeat(8)], dim=1).to(gpu)
    d = torch.tensor([[1.0, 0.0, 0.0]]).repeat(64, 1).to(gpu)
    rays = svox.Rays(o, d, d)
    s = r.ray_samples(rays)
    assert len(s) == 512 and bool((s.counts == 8).all())
    pts = s.points(rays)
    lb = tree.leaf_boxes(world=True)
    centres = lb.corners + 0.5 * lb.lengths
    assert torch.equal(pts[torch.argsort(s.row)], centres[torch.argsort(lb.rows)])
    with torch.no_grad():
        assert torch.equal(tree.interp(pts), svox.gather_rows(s, tree.features))
        assert torch.equal(tree.interp(pts, dim=-1), svox.gather_rows(s, tree.features, dim=-1))
