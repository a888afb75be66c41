"""N3Tree.set / snap / leaf_boxes and _C.leaf_corners on the GPU, bit for bit against the numpy restatement
(tests/assign_restate.py: the CPU oracle's point query for the leaf of a point, sequential float32 loops in ascending
point index for the reductions) and against the CPU torch walk of the corners.

Every value test asserts its own coverage: at least 25 % of its points land in non-empty leaves and at least 10 % of the
touched rows receive two or more points (uniform points in the cube would not do on the shell trees: the points are
drawn inside occupied leaves through leaf_boxes)."""
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from svox_t_amd import synth
from tests import assign_restate as AR

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
E = synth.EMPTY_SENTINEL
TOPOLOGIES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "topology_*.npz")))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def load(name):
    return np.load(os.path.join(G, name))


def leaf_data(child, every=3):
    """Data words for a topology: leaf l (in slot order) names row l, every `every`-th leaf is empty; M = leaves."""
    leaf = child.reshape(-1) == 0
    L = int(leaf.sum())
    words = np.arange(L, dtype=np.int32)
    words[every - 1::every] = E
    data = np.full(child.size, E, np.int32)
    data[leaf] = words
    return data.reshape(child.shape + (1,)), L


def build(kind, dev, K=8):
    """(tree on the GPU, description): the trees of the value tests."""
    rng = np.random.default_rng(11)
    radius, center = 0.5, (0.5, 0.5, 0.5)
    if kind == "shell_d5":
        g = load("topology_shell_d5.npz")
        st = synth.shell_tree(5)
        assert np.array_equal(st.child, g["child"])
        child, pd, data, M = g["child"], g["parent_depth"], st.data, st.n_features
    elif kind == "points_a":
        g = load("topology_points_a.npz")
        child, pd = g["child"], g["parent_depth"]          # (the fixture is the topology: its data words are all empty)
        data, M = leaf_data(child, every=2)
    elif kind == "full_n3":
        g = load("topology_full_n3_l2.npz")
        child, pd = g["child"], g["parent_depth"]
        data, M = leaf_data(child)
    elif kind in ("refined", "merged", "radius"):
        st = synth.shell_tree(4)
        child, pd, data, M = st.child, st.parent_depth, st.data, st.n_features
        if kind == "radius":
            radius, center = [1.0, 2.0, 0.25], [0.1, -0.2, 0.3]
    else:
        raise ValueError(kind)
    feats = rng.standard_normal((M, K)).astype(np.float32)
    tree = svox.N3Tree.from_arrays(child, data, pd, feats, radius=radius, center=center, device=dev)
    if kind in ("refined", "merged"):
        # every fourth occupied leaf becomes a node whose 8 slots share the leaf's row
        lb = tree.leaf_boxes()
        sel = lb.leaf_node[lb.rows >= 0][::4]
        tree.refine(1, sel=tuple(sel.T), leaf_node=sel)
        shared = tree.data[tree.filled - 1].reshape(-1)
        assert int((shared == shared[0]).sum()) == 8 and int(shared[0]) < M
    if kind == "merged":
        # slot 0 of every new node is refined once more; merge() then takes these deepest nodes back onto their shared
        # word (their parents keep 8 slots that name one row) and gives the shell's own finest nodes NEW rows
        ids = torch.arange(tree.filled - sel.shape[0], tree.filled, device=dev)
        sel2 = torch.stack([ids, torch.zeros_like(ids), torch.zeros_like(ids), torch.zeros_like(ids)], dim=1)
        tree.refine(1, sel=tuple(sel2.T), leaf_node=sel2)
        res = tree.merge(op="mean")
        assert res.nodes_merged > sel.shape[0] and res.rows_added > 0
        shared = tree.data[tree.filled - 1].reshape(-1)
        assert int((shared == shared[0]).sum()) == 8 and int(shared[0]) < tree.features.shape[0]
    return tree


def tables(tree):
    n = tree.filled
    return tree.child[:n].cpu().numpy(), tree.data[:n].cpu().numpy(), tree.features.shape[0], tree.features.shape[1]


def transform(tree, world):
    if world:
        return tree.offset.cpu().numpy(), tree.invradius.cpu().numpy()
    return (0, 0, 0), (1, 1, 1)


def sample_points(tree, world, per_leaf=3, seed=5):
    """Points for a value test: `per_leaf` inside every occupied leaf and one inside every fourth empty one (through
    leaf_boxes: corner + u * length), points outside the cube (clamped), points exactly on dyadic leaf boundaries;
    shuffled, so that a group's point indices are spread over the batch."""
    gen = torch.Generator().manual_seed(seed)
    lb = tree.leaf_boxes(world=world)
    occ = (lb.rows >= 0).nonzero().squeeze(1).cpu()
    emp = (lb.rows < 0).nonzero().squeeze(1).cpu()[::4]
    idx = torch.cat([occ.repeat(per_leaf), emp]).to(lb.corners.device)
    u = torch.rand((idx.shape[0], 3), generator=gen).to(lb.corners.device)
    inside = lb.corners[idx] + u * lb.lengths[idx]
    n_extra = max(8, idx.shape[0] // 10)
    outside = torch.rand((n_extra, 3), generator=gen) * 3.0 - 1.0              # the tree's own coordinates, in [-1, 2)
    N, depth = tree.N, max(1, tree.max_depth + 1)
    dyadic = torch.randint(0, N ** depth + 1, (n_extra, 3), generator=gen).float() / float(N ** depth)
    extra = torch.cat([outside, dyadic]).to(lb.corners.device)
    if world:
        extra = tree.tree2world(extra)
    pts = torch.cat([inside, extra])
    return pts[torch.randperm(pts.shape[0], generator=gen).to(pts.device)].contiguous()


def coverage(rows):
    uniq, counts, _, _ = AR.groups(rows)
    hit = float((rows >= 0).mean()) if rows.size else 0.0
    multi = float((counts >= 2).mean()) if counts.size else 0.0
    return hit, multi, uniq, counts


def assert_coverage(rows):
    hit, multi, uniq, counts = coverage(rows)
    print(f"points {rows.size}: {hit:.1%} in non-empty leaves, rows touched {uniq.size}, {multi:.1%} of them by two or more points")
    assert hit >= 0.25, hit
    assert multi >= 0.10, multi
    return uniq, counts


KINDS = ["shell_d5", "points_a", "full_n3", "refined", "merged", "radius"]


@pytest.mark.parametrize("world", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_set_every_mode_equals_the_restatement(gpu, kind, world):
    tree = build(kind, gpu)
    child, data, M, K = tables(tree)
    pts = sample_points(tree, world)
    Q = pts.shape[0]
    off, sc = transform(tree, world)
    rows = AR.point_rows(child, data, M, pts.cpu().numpy(), off, sc)
    uniq, counts = assert_coverage(rows)
    if kind in ("refined", "merged"):
        # points of several slots that share a row form one group: some row is reached through two different slots
        node_ids = tree.forward(tree.features.detach(), pts, want_node_ids=True, world=world)[1].cpu().numpy()
        per_row = {}
        for r, s in zip(rows.tolist(), node_ids.tolist()):
            if r >= 0:
                per_row.setdefault(r, set()).add(s)
        assert max(len(v) for v in per_row.values()) >= 2
    rng = np.random.default_rng(3)
    vals = (rng.standard_normal((Q, K)) * 100.0).astype(np.float32)
    table0 = rng.standard_normal((M, K)).astype(np.float32)
    vals_d = torch.from_numpy(vals).to(gpu)
    for mode in AR.MODES:
        table = torch.from_numpy(table0).to(gpu)
        ver = table._version
        assert tree.set(pts, vals_d, world=world, reduce=mode, features=table) is None
        assert table._version > ver
        want = AR.assign(table0, rows, vals, mode)
        got = table.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (kind, world, mode, int((bits(got) != bits(want)).any(1).sum()))
        untouched = np.ones(M, bool)
        untouched[uniq] = False
        assert np.array_equal(bits(got[untouched]), bits(table0[untouched]))
        # twice the same bits; the rows and counts
        again = torch.from_numpy(table0).to(gpu)
        r2, c2 = tree.set(pts, vals_d, world=world, reduce=mode, features=again, return_rows=True)
        assert torch.equal(again, table)
        assert r2.dtype == torch.int64 and c2.dtype == torch.int64
        assert np.array_equal(r2.cpu().numpy(), uniq) and np.array_equal(c2.cpu().numpy(), counts)
        if mode == "last":
            assert np.array_equal(bits(got), bits(AR.assign_last(table0, rows, vals)))
            # the query gives every non-ignored point its group's winner back
            back = tree.forward(table, pts, world=world).cpu().numpy()
            winner = np.full(M, -1, np.int64)
            np.maximum.at(winner, rows[rows >= 0], np.nonzero(rows >= 0)[0])
            assert np.array_equal(bits(back[rows >= 0]), bits(vals[winner[rows[rows >= 0]]]))
            assert not back[rows < 0].any()


def test_setitem_and_default_table(gpu):
    tree = build("shell_d5", gpu, K=4)
    tree.features.requires_grad_(True)
    child, data, M, K = tables(tree)
    table0 = tree.features.detach().cpu().numpy().copy()
    for world in (True, False):
        pts = sample_points(tree, world, seed=9)
        rows = AR.point_rows(child, data, M, pts.cpu().numpy(), *transform(tree, world))
        assert_coverage(rows)
        vals = torch.randn(pts.shape[0], K, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            tree.features.copy_(torch.from_numpy(table0))
        ver = tree.features._version
        if world:
            tree[pts] = vals.to(gpu)
        else:
            tree[svox.LocalIndex(pts)] = vals.to(gpu)
        assert tree.features._version > ver and tree.features.requires_grad
        assert np.array_equal(bits(tree.features.detach().cpu().numpy()), bits(AR.assign_last(table0, rows, vals.numpy())))
    # a scalar broadcasts; inside accumulate_weights() the write is allowed
    with tree.accumulate_weights():
        tree[svox.LocalIndex(pts)] = 2.5
    got = tree.features.detach().cpu().numpy()
    uniq = AR.groups(rows)[0]
    assert (got[uniq] == 2.5).all()
    with pytest.raises(RuntimeError, match="must not require grad"):
        tree.set(pts, torch.zeros(pts.shape[0], K, device=gpu, requires_grad=True))
    with pytest.raises(RuntimeError, match="values must be float32"):
        tree.set(pts, torch.zeros(pts.shape[0], K + 1, device=gpu))


@pytest.mark.parametrize("mode", AR.MODES)
def test_no_point_and_only_empty_leaves_leave_the_table_alone(gpu, mode):
    tree = build("shell_d5", gpu)
    M, K = tree.features.shape
    table0 = torch.randn(M, K, device=gpu)
    table = table0.clone()
    r, c = tree.set(torch.zeros(0, 3, device=gpu), torch.zeros(0, K, device=gpu), reduce=mode, features=table, return_rows=True)
    assert r.numel() == 0 and c.numel() == 0 and torch.equal(table, table0)
    lb = tree.leaf_boxes()
    emp = lb.rows < 0
    pts = (lb.corners[emp] + 0.5 * lb.lengths[emp]).contiguous()
    assert pts.shape[0] > 1000
    child, data, _, _ = tables(tree)
    assert (AR.point_rows(child, data, M, pts.cpu().numpy(), *transform(tree, True)) < 0).all()
    r, c = tree.set(pts, torch.randn(pts.shape[0], K, device=gpu), reduce=mode, features=table, return_rows=True)
    assert r.numel() == 0 and torch.equal(table, table0)


def test_set_at_full_size_depth8(gpu):
    """The depth-8 synth tree (M = 668 912, K = 28), 6 points in every occupied leaf (4.0 M points): "last" in full
    against its exact vectorised restatement; "sum" / "mean" on a seeded subset of 2 000 touched rows against the
    sequential loops, and run to run in full."""
    st = synth.shell_tree(8)
    M, K = st.n_features, 28
    assert M == 668912
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, synth.shell_features(M, K), data_format="SH9", device=gpu)
    lb = tree.leaf_boxes()
    occ = (lb.rows >= 0).nonzero().squeeze(1)
    gen = torch.Generator().manual_seed(21)
    idx = occ.repeat(6)
    idx = idx[torch.randperm(idx.shape[0], generator=gen).to(gpu)]
    pts = (lb.corners[idx] + torch.rand((idx.shape[0], 3), generator=gen).to(gpu) * lb.lengths[idx]).contiguous()
    Q = pts.shape[0]
    assert Q == 6 * M
    rows = AR.point_rows(st.child, st.data, M, pts.cpu().numpy(), *transform(tree, True))
    uniq, counts = assert_coverage(rows)
    vals_d = torch.randn((Q, K), generator=gen).to(gpu) * 10.0
    vals = vals_d.cpu().numpy()
    table0 = synth.shell_features(M, K, seed=4)
    t0 = table0.numpy()
    table = table0.to(gpu)
    r, c = tree.set(pts, vals_d, reduce="last", features=table, return_rows=True)
    assert np.array_equal(r.cpu().numpy(), uniq) and np.array_equal(c.cpu().numpy(), counts)
    assert np.array_equal(bits(table.cpu().numpy()), bits(AR.assign_last(t0, rows, vals)))
    pick = np.random.default_rng(8).choice(uniq, 2000, replace=False)
    untouched = np.ones(M, bool)
    untouched[uniq] = False
    for mode in ("sum", "mean"):
        table = table0.to(gpu)
        tree.set(pts, vals_d, reduce=mode, features=table)
        got = table.cpu().numpy()
        want = AR.assign(t0, rows, vals, mode, only_rows=pick)
        assert np.array_equal(bits(got[pick]), bits(want[pick])), mode
        assert np.array_equal(bits(got[untouched]), bits(t0[untouched]))
        again = table0.to(gpu)
        tree.set(pts, vals_d, reduce=mode, features=again)
        assert torch.equal(again, table)


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_leaf_corners_equal_the_cpu_walk_and_the_fixture(gpu, name):
    g = load(name)
    child, pd = g["child"], g["parent_depth"]
    N = child.shape[1]
    cpu = svox.N3Tree.from_arrays(child, g["data"], pd, np.zeros((1, 1), np.float32))
    leaves = cpu._all_leaves()
    want = cpu._calc_corners(leaves)                                           # the torch walk, on the CPU
    dev = cpu.clone(device=gpu)
    got = _C.leaf_corners(dev.child, dev.parent_depth, N, leaves.to(gpu).contiguous())
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.numpy()))
    assert torch.equal(dev._calc_corners(leaves), got)                         # _calc_corners goes through the kernel there
    if "corners" in g.files:
        assert np.array_equal(leaves.numpy(), g["leaves"])
        np.testing.assert_allclose(got.cpu().numpy(), g["corners"], rtol=0, atol=1e-7)
    # a slot out of range gives NaN instead of reading outside the tables
    bad = torch.tensor([[child.shape[0], 0, 0, 0], [0, N, 0, 0], [-1, 0, 0, 0]], device=gpu)
    assert torch.isnan(_C.leaf_corners(dev.child, dev.parent_depth, N, bad)).all()


@pytest.mark.parametrize("kind", ["shell_d5", "full_n3", "radius", "merged"])
def test_snap_and_leaf_boxes(gpu, kind):
    tree = build(kind, gpu)
    lb = tree.leaf_boxes(world=False)
    leaves = tree._all_leaves()
    assert torch.equal(lb.leaf_node.cpu(), leaves) and lb.leaf_node.is_cuda
    cpu = tree.clone(device="cpu")
    assert np.array_equal(bits(lb.corners.cpu().numpy()), bits(cpu._calc_corners(leaves).numpy()))
    words = tree.data[:tree.filled].reshape(-1)[tree._pack_index(lb.leaf_node)].long()
    M = tree.features.shape[0]
    assert torch.equal(lb.rows, torch.where((words >= 0) & (words < M), words, torch.full_like(words, -1)))
    assert int((lb.rows >= 0).sum()) > 0 and int((lb.rows < 0).sum()) > 0
    # the view of the leaves' centres lists every leaf once, in the same order
    centres = (lb.corners + 0.5 * lb.lengths).contiguous()
    view = tree[svox.LocalIndex(centres)]
    assert torch.equal(view.unique_leaf_node, lb.leaf_node)
    lbw = tree.leaf_boxes()
    assert torch.equal(view.depths, lb.depths) and torch.equal(lbw.depths, lb.depths)
    assert torch.equal(view.lengths, lbw.lengths) and torch.equal(view.lengths_local[:, None].expand(-1, 3), lb.lengths)
    assert torch.equal(view.corners, lbw.corners) and torch.equal(view.corners_local, lb.corners)
    # snap = the corner of the leaf the query reports, in the coordinates the points came in
    for world in (False, True):
        pts = sample_points(tree, world, per_leaf=1, seed=2)
        node_ids = tree.forward(tree.features.detach(), pts, want_node_ids=True, world=world)[1]
        local = _C.leaf_corners(tree.child, tree.parent_depth, tree.N, tree._unpack_index(node_ids).contiguous())
        want = (local - tree.offset) / tree.invradius if world else local
        got = tree.snap(pts, world=world)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
    assert tree.snap(torch.zeros(0, 3, device=gpu)).shape == (0, 3)
