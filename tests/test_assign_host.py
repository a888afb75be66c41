"""N3Tree.set / snap / leaf_boxes / partial / clone without a GPU: the numpy restatement (tests/assign_restate.py) on a
hand-made case, the new exports and their argument checks (which come before any HIP call), the refusals of the Python
surface, and partial / clone on CPU trees."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import assign_restate as AR

E = 1410065408
NEW = ["svoxt_assign_workspace_bytes", "svoxt_assign_leaves", "svoxt_leaf_corners", "svoxt_snap_points"]


def hand_case():
    """A root-only octree: slot 0 -> row 0, slots 1 and 2 -> row 1 (shared), the rest empty; M = 2, K = 2.
    Points (the tree's own coordinates): 0 and 2 in slot 0, 1 in slot 1, 4 in slot 2, 3 in the empty slot 3."""
    child = np.zeros((1, 2, 2, 2), np.int32)
    data = np.full((8,), E, np.int32)
    data[[0, 1, 2]] = [0, 1, 1]
    pts = np.array([[0.1, 0.1, 0.1], [0.1, 0.1, 0.7], [0.2, 0.2, 0.2], [0.1, 0.7, 0.7], [0.1, 0.7, 0.1]], np.float32)
    vals = np.array([[1, 10], [2, 20], [3, -30], [100, 100], [5, 50]], np.float32)
    return child, data.reshape(1, 2, 2, 2, 1), pts, vals


def test_restatement_on_a_hand_made_case():
    child, data, pts, vals = hand_case()
    rows = AR.point_rows(child, data, 2, pts)
    assert rows.tolist() == [0, 1, 0, -1, 1]
    uniq, counts, order, starts = AR.groups(rows)
    assert uniq.tolist() == [0, 1] and counts.tolist() == [2, 2] and order.tolist() == [0, 2, 1, 4] and starts.tolist() == [0, 2, 4]
    table = np.full((2, 2), 7.0, np.float32)
    want = {"last": [[3, -30], [5, 50]], "sum": [[4, -20], [7, 70]], "mean": [[2, -10], [3.5, 35]],
            "max": [[3, 10], [5, 50]], "min": [[1, -30], [2, 20]]}
    for mode in AR.MODES:
        assert AR.assign(table, rows, vals, mode).tolist() == want[mode], mode
    assert AR.assign_last(table, rows, vals).tolist() == want["last"]
    # rows without a point keep their bits; only_rows restricts the rewrite
    assert AR.assign(table, np.array([-1, 1, -1, -1, -1]), vals, "sum").tolist() == [[7, 7], [2, 20]]
    assert AR.assign(table, rows, vals, "sum", only_rows=[1]).tolist() == [[7, 7], [7, 70]]
    assert AR.assign(table, np.full(5, -1), vals, "mean").tolist() == table.tolist()
    # the order of a float32 sum is the ascending point index: (1e8 + 1) - 1e8 = 0, not 1
    v = np.array([[1e8], [1.0], [-1e8]], np.float32)
    assert AR.assign(np.zeros((1, 1), np.float32), np.zeros(3, np.int64), v, "sum").tolist() == [[0.0]]
    assert AR.assign(np.zeros((1, 1), np.float32), np.zeros(3, np.int64), v[[0, 2, 1]], "sum").tolist() == [[1.0]]
    # clamped: a point outside the cube belongs to the leaf at the border
    assert AR.point_rows(child, data, 2, np.array([[-3.0, -1.0, 0.2], [0.3, 0.2, 9.0]], np.float32)).tolist() == [0, 1]
    assert AR.point_rows(child, data, 2, np.zeros((0, 3), np.float32)).shape == (0,)
    # world coordinates: p' = offset + scaling * p
    assert AR.point_rows(child, data, 2, np.array([[0.0, 0.0, 1.0]], np.float32), offset=(0.25, 0.25, 0.25),
                         scaling=(0.5, 0.5, 0.5)).tolist() == [1]


def test_new_symbols_abi_version_and_stubs():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for nm in NEW:
        assert nm in _C.EXPORTS and hasattr(lib, nm), nm
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    for nm in ("assign_leaves", "leaf_corners", "snap_points"):
        assert callable(getattr(_C, nm))
    with pytest.raises(NotImplementedError, match="assign_leaves"):
        _C.assign_vertical()
    with pytest.raises(NotImplementedError, match="leaf_corners"):
        _C.calc_corners()


def _fake_tree(buf, M=10, K=4, N=2, n=4):
    t = _C._CTree()
    p = ctypes.addressof(buf)
    t.features, t.data, t.child, t.offset, t.scaling = p, p, p, p, p
    t.M, t.K, t.N, t.n_internal = M, K, N, n
    return t


def test_c_abi_argument_checks_come_before_any_hip_call():
    lib = _C._lib
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err = lambda: lib.svoxt_last_error()                                       # noqa: E731
    ws = lib.svoxt_assign_workspace_bytes
    assert ws(-1, 5, 0) == -1 and ws(5, -1, 0) == -1 and ws(5, 5, 5) == -1 and ws(5, 5, -1) == -1 and ws(1 << 31, 5, 0) == -1
    assert ws(1000, 500, 0) >= 4 * (1000 + 500)
    assert ws(1000, 500, 1) >= 4 * 5 * 1001 and ws(0, 0, 2) >= 0
    big = 1 << 30
    t = _fake_tree(buf)
    asg = lambda **k: lib.svoxt_assign_leaves(k.get("tree", ctypes.byref(t)), k.get("points", p), k.get("Q", 8), k.get("values", p),   # noqa: E731
                                              k.get("reduce", 0), k.get("table", p), None, k.get("ws", p), k.get("bytes", big), None)
    assert asg(tree=None) == 1 and b"tree is NULL" in err()
    assert asg(reduce=5) == 1 and b"reduce must be" in err()
    assert asg(reduce=-1) == 1
    assert asg(Q=-1) == 1 and b"number of points" in err()
    assert asg(Q=1 << 31) == 1
    assert asg(table=None) == 1 and b"table is NULL" in err()
    assert asg(points=None) == 1 and b"points / values is NULL" in err()
    assert asg(values=None) == 1
    assert asg(ws=None) == 1 and b"workspace is NULL" in err()
    assert asg(bytes=16) == 1 and b"workspace smaller" in err()
    assert asg(bytes=16, reduce=2) == 1 and b"workspace smaller" in err()
    assert asg(tree=ctypes.byref(_fake_tree(buf, K=0))) == 1
    assert asg(tree=ctypes.byref(_fake_tree(buf, N=1))) == 1 and b"branching" in err()
    assert asg(Q=0, points=None, values=None, ws=None, bytes=0) == 0         # no point: nothing to do
    lc = lambda **k: lib.svoxt_leaf_corners(k.get("pd", p), k.get("n", 4), k.get("N", 2), k.get("leaf", p), k.get("Q", 3),   # noqa: E731
                                            k.get("out", p), None)
    assert lc(N=1) == 1 and b"branching" in err()
    assert lc(N=17) == 1
    assert lc(n=0) == 1 and b"n_internal" in err()
    assert lc(n=1 << 29) == 1 and b"2^31" in err()
    assert lc(Q=-1) == 1
    assert lc(pd=None) == 1 and b"NULL" in err()
    assert lc(leaf=None) == 1 and lc(out=None) == 1
    assert lc(Q=0, leaf=None, out=None) == 0
    sn = lambda **k: lib.svoxt_snap_points(k.get("tree", ctypes.byref(t)), k.get("pd", p), k.get("points", p), k.get("Q", 3),   # noqa: E731
                                           k.get("out", p), None)
    assert sn(tree=None) == 1 and b"tree is NULL" in err()
    assert sn(tree=ctypes.byref(_fake_tree(buf, N=17))) == 1 and b"branching" in err()
    assert sn(Q=-1) == 1
    assert sn(pd=None) == 1 and b"NULL" in err()
    assert sn(points=None) == 1 and sn(out=None) == 1
    assert sn(Q=0, points=None, out=None) == 0


def test_python_refusals():
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=1)                         # a CPU tree
    pts = torch.rand(5, 3)
    vals = torch.rand(5, 4)
    for call in (lambda: tree.set(pts, vals), lambda: tree.set(pts, vals, cuda=False), lambda: tree.snap(pts), tree.leaf_boxes,
                 lambda: tree.__setitem__(pts, vals)):
        with pytest.raises(RuntimeError, match="GPU") as e:
            call()
        assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="reduce must be"):
        tree.set(pts, vals, reduce="median")
    with pytest.raises(NotImplementedError):
        tree[torch.zeros(3, dtype=torch.long)] = vals                          # leaf-index keys: not served
    with tree.accumulate_weights():                                            # set() does not touch the topology: not locked out
        with pytest.raises(RuntimeError, match="GPU"):
            tree.set(pts, vals)
    # the operator layer: shapes, dtypes and values are refused before devices
    spec = tree._spec(tree.features.detach())
    with pytest.raises(RuntimeError, match="reduce must be"):
        _C.assign_leaves(spec, pts, vals, "median")
    with pytest.raises(RuntimeError, match=r"indices must be float32 \[Q, 3\]"):
        _C.assign_leaves(spec, pts[:, :2], vals)
    with pytest.raises(RuntimeError, match="indices must be float32"):
        _C.assign_leaves(spec, pts.double(), vals)
    with pytest.raises(RuntimeError, match=r"values must be float32 \[Q, K\]"):
        _C.assign_leaves(spec, pts, vals[:4])
    with pytest.raises(RuntimeError, match="values must be float32"):
        _C.assign_leaves(spec, pts, vals[:, :3])
    with pytest.raises(RuntimeError, match="values must be float32"):
        _C.assign_leaves(spec, pts, vals.double())
    with pytest.raises(RuntimeError, match="must not require grad"):
        _C.assign_leaves(spec, pts, vals.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.assign_leaves(spec, pts, vals)
    leaves = tree._all_leaves()
    with pytest.raises(RuntimeError, match=r"leaf_node must be int64 \[Q, 4\]"):
        _C.leaf_corners(tree.child, tree.parent_depth, 2, leaves[:, :3])
    with pytest.raises(RuntimeError, match="leaf_node must be int64"):
        _C.leaf_corners(tree.child, tree.parent_depth, 2, leaves.int())
    with pytest.raises(RuntimeError, match="child must be int32"):
        _C.leaf_corners(tree.child, tree.parent_depth, 3, leaves)
    with pytest.raises(RuntimeError, match="parent_depth must be int32"):
        _C.leaf_corners(tree.child, tree.parent_depth[:-1], 2, leaves)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.leaf_corners(tree.child, tree.parent_depth, 2, leaves)
    with pytest.raises(RuntimeError, match="indices must be"):
        _C.snap_points(spec, pts[:, :2])
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.snap_points(spec, pts)
    # the CPU walk of _calc_corners is what it was
    c = tree._calc_corners(leaves)
    assert c.shape == (leaves.shape[0], 3) and float(c.min()) == 0.0 and float(c.max()) == 0.75


def _same_tree(a, b, cols=None):
    for nm in ("child", "data", "parent_depth", "invradius", "offset", "_n_internal", "_n_free"):
        x, y = getattr(a, nm), getattr(b, nm)
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr(), nm
    want = a.features.detach() if cols is None else a.features.detach()[:, cols]
    assert torch.equal(b.features.detach(), want) and b.features.data_ptr() != a.features.data_ptr()
    assert isinstance(b.features, torch.nn.Parameter) and b.features.requires_grad == a.features.requires_grad
    assert b.features.is_contiguous() and b.data_dim == b.features.shape[1]
    assert (b.N, b.filled, b.depth_limit, b.geom_resize_fact, b.n_internal) == (a.N, a.filled, a.depth_limit, a.geom_resize_fact, a.n_internal)


def test_partial_and_clone_on_cpu_trees():
    extra = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    tree = svox.N3Tree(N=2, data_dim=28, init_refine=2, depth_limit=7, geom_resize_fact=2.0, radius=[1.0, 2.0, 0.5],
                       center=[0.1, -0.2, 0.3], data_format="SH9", extra_data=extra)
    with torch.no_grad():
        tree.features.copy_(torch.arange(tree.features.numel(), dtype=torch.float32).reshape(tree.features.shape))
    sel = tree._all_leaves()[:3]
    tree.refine(1, sel=tuple(sel.T), leaf_node=sel)
    c = tree.clone()
    _same_tree(tree, c)
    assert repr(c.data_format) == "SH9" and c.data_format is not tree.data_format
    assert torch.equal(c.extra_data, extra) and c.extra_data.data_ptr() != tree.extra_data.data_ptr()
    assert torch.equal(c._all_leaves(), tree._all_leaves())
    # no storage is shared: writing the copy leaves the source alone, and the copy can be refined on its own
    with torch.no_grad():
        c.features.zero_()
    c.child[0, 0, 0, 0] = 77
    assert float(tree.features.detach().abs().sum()) > 0 and int(tree.child[0, 0, 0, 0]) != 77
    c.child[0, 0, 0, 0] = tree.child[0, 0, 0, 0]
    c.refine(1)
    assert c.n_internal > tree.n_internal
    # data_sel: -1 (sigma only), a slice, a list; the copy is a plain-row tree unless told otherwise
    s = tree.partial(-1)
    _same_tree(tree, s, cols=[27])
    assert s.data_dim == 1 and repr(s.data_format) == "RGBA" and s.extra_data is not None
    sl = tree.partial(slice(0, 9))
    _same_tree(tree, sl, cols=list(range(9)))
    li = tree.partial([3, 0, 27])
    _same_tree(tree, li, cols=[3, 0, 27])
    assert repr(tree.partial([0, 1, 2, 27], data_format="SH1").data_format) == "SH1"
    assert repr(tree.partial(torch.tensor([0, 27])).data_format) == "RGBA"
    with pytest.raises(RuntimeError, match="selects no column"):
        tree.partial([])
    # requires_grad is carried over, both ways; a tree without extra_data or data_format
    tree.features.requires_grad_(False)
    assert not tree.clone().features.requires_grad and not tree.partial(-1).features.requires_grad
    plain = svox.N3Tree(N=3, data_dim=4, init_refine=1)
    p2 = plain.clone(device="cpu")
    _same_tree(plain, p2)
    assert p2.extra_data is None and repr(p2.data_format) == "RGBA" and p2.N == 3
