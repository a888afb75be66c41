"""leaf_neighbors / tv without a GPU: the numpy restatement the GPU tests compare with (tests/neighbors_restate.py) on
the topology fixtures (`integrity`: a brute-force search on integer boxes) and on small cases worked out by hand; the C
ABI's argument checks (all made before any HIP call, so they run here) and the Python layer's refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import neighbors_restate as R

G = os.path.join(os.path.dirname(__file__), "golden")
E = 1410065408
INVALID = 1
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "topology_*.npz")))


def test_the_fixtures_cover_both_branching_factors():
    Ns = {np.load(os.path.join(G, f))["child"].shape[1] for f in FIXTURES}
    assert Ns == {2, 3} and len(FIXTURES) == 7


@pytest.mark.parametrize("name", FIXTURES)
def test_integrity_on_the_topology_fixtures(name):
    g = np.load(os.path.join(G, name))
    child, pd, n = g["child"], g["parent_depth"], int(g["n_internal"])
    N = child.shape[1]
    nb = R.leaf_neighbors(child, pd, n, N)
    pairs = R.integrity(nb, child, pd, n, N)
    assert pairs > 0
    # the plan: every incidence under its owner, ids ascending within a row, both halves of every edge present
    slots, depths, _ = R.cells(child, pd, n, N)
    L = len(slots)
    rows = np.arange(L) // 2                          # two leaves a row: some neighbours share one and are no edge
    pl = R.plan(nb, depths, rows, (L + 1) // 2)
    assert 0 < pl["E"] <= pairs and pl["row_ptr"][-1] == 2 * pl["E"] == len(pl["other"])
    owner = np.repeat(np.arange((L + 1) // 2), np.diff(pl["row_ptr"]))
    assert (owner != pl["other"]).all()
    assert ((pl["meta"] & 1) == 0).sum() == pl["E"]


def eight_leaves():
    child = np.zeros((1, 2, 2, 2), np.int32)
    return child, np.zeros((1, 2), np.int32)


def one_split_slot():
    """N = 2: the root's slot 0 -> node 1.  Leaves: the root's slots 1 .. 7 (leaf 0 .. 6), node 1's slots (leaf 7 .. 14)."""
    child = np.zeros((2, 8), np.int32)
    child[0, 0] = 1
    pd = np.array([[0, 0], [0, 1]], np.int32)
    return child.reshape(2, 2, 2, 2), pd


def test_an_eight_leaf_root_by_hand():
    child, pd = eight_leaves()
    nb = R.leaf_neighbors(child, pd, 1, 2)
    want = [[-1, 4, -1, 2, -1, 1], [-1, 5, -1, 3, 0, -1], [-1, 6, 0, -1, -1, 3], [-1, 7, 1, -1, 2, -1],
            [0, -1, -1, 6, -1, 5], [1, -1, -1, 7, 4, -1], [2, -1, 4, -1, -1, 7], [3, -1, 5, -1, 6, -1]]
    np.testing.assert_array_equal(nb, want)
    assert R.integrity(nb, child, pd, 1, 2) == 12


def test_a_root_with_one_split_slot_by_hand():
    child, pd = one_split_slot()
    nb = R.leaf_neighbors(child, pd, 2, 2)
    assert nb.shape == (15, 6)
    np.testing.assert_array_equal(nb[0], [-1, 4, -1, 2, -2, -1])        # the root's (0, 0, 1): finer leaves below it
    np.testing.assert_array_equal(nb[6], [2, -1, 4, -1, 5, -1])         # the root's (1, 1, 1)
    np.testing.assert_array_equal(nb[7], [-1, 11, -1, 9, -1, 8])        # node 1's (0, 0, 0)
    np.testing.assert_array_equal(nb[14], [10, 3, 12, 1, 13, 0])        # node 1's (1, 1, 1): three coarser neighbours
    assert (nb == -2).sum() == 3
    assert R.integrity(nb, child, pd, 2, 2) == 12 + 12 + 9
    depths = np.array([0] * 7 + [1] * 8)
    ed = R.edges(nb, depths, np.arange(15), 15)
    assert (6 * 14 + 5, 14, 0) in ed and not any(i == 0 and j >= 7 for _, i, j in ed)      # from the finer side only


def test_tv_of_one_leaf_pair_by_hand():
    child, pd = eight_leaves()
    data = np.full((1, 8), E, np.int32)
    data[0, 0], data[0, 1] = 0, 1                                       # (0, 0, 0) and (0, 0, 1): one face
    rows = R.leaf_rows(child, data, 1, 2)
    np.testing.assert_array_equal(rows, [0, 1, -1, -1, -1, -1, -1, -1])
    nb = R.leaf_neighbors(child, pd, 1, 2)
    pl = R.plan(nb, np.zeros(8, np.int64), rows, 2)
    assert pl["E"] == 1
    np.testing.assert_array_equal(pl["row_ptr"], [0, 1, 2])
    np.testing.assert_array_equal(pl["other"], [1, 0])
    np.testing.assert_array_equal(pl["meta"], [0, 1])
    f = np.array([[1, 2], [3, 5]], np.float32)
    loss, g = R.tv(f, pl, None, 2, "uniform", 2)
    assert loss == 13 and g.tolist() == [[-4, -6], [4, 6]]
    loss, g = R.tv(f, pl, None, 1, "uniform", 2)
    assert loss == 5 and g.tolist() == [[-1, -1], [1, 1]]
    loss, g = R.tv(f, pl, [1], 2, "area", 2, mean=True)                 # the face of a depth-0 leaf: 1 / 4
    assert loss == 2.25 and g.tolist() == [[0, -1.5], [0, 1.5]]
    out = R.add_grad(np.ones((2, 2), np.float32), 0.5, g, pl, [1])
    assert out.tolist() == [[1, 0.25], [1, 1.75]]
    assert R.tv(f[:1], R.plan(nb, np.zeros(8, np.int64), rows, 1), None, 2, "uniform", 2)[0] == 0     # M = 1: row 1 is no row


NEW = ("svoxt_neighbors_workspace_bytes", "svoxt_leaf_neighbors", "svoxt_tv_plan_workspace_bytes", "svoxt_tv_plan_count",
       "svoxt_tv_plan_emit", "svoxt_tv_workspace_bytes", "svoxt_tv_rows")


def test_symbols_and_the_abi_version():
    lib = _C._lib
    header = open(os.path.join(os.path.dirname(G), "..", "include", "svoxt.h")).read()
    for nm in NEW:
        assert nm in _C.EXPORTS and hasattr(lib, nm) and nm + "(" in header, nm
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22              # entry points were added, nothing changed
    q = lib.svoxt_neighbors_workspace_bytes
    assert q(100, 2) >= 8 * 801 and q(0, 2) == -1 and q(5, 1) == -1 and q(5, 17) == -1 and q(1 << 28, 2) == -1
    q = lib.svoxt_tv_plan_workspace_bytes
    assert q(100, -1) >= 8 * 601 and q(100, 600) >= 36 * 600 and q(100, 601) == -1 and q(-1, 0) == -1 and q(1 << 28, 0) == -1
    q = lib.svoxt_tv_workspace_bytes
    assert q(1000, 28) >= 4 * 110 and q(0, 4) > 0 and q(-1, 4) == -1 and q(5, 0) == -1 and q(1 << 31, 4) == -1 and q(1 << 30, 256) == -1


NB_OK = dict(child=1, pd=1, n=100, N=2, depth=9, L=500, out=1, ws=1, nbytes=1 << 40)
NB_BAD = [("child", None), ("pd", None), ("n", 0), ("n", 1 << 28), ("N", 1), ("N", 17), ("depth", -1), ("depth", 30), ("L", -1),
          ("L", 801), ("out", None), ("ws", None), ("nbytes", 64)]


def _ids(bad):
    return [f"{f}={v}" for f, v in bad]


@pytest.mark.parametrize("field,value", NB_BAD, ids=_ids(NB_BAD))
def test_leaf_neighbors_rejects_before_any_hip_call(field, value):
    a = dict(NB_OK)
    a[field] = value
    rc = _C._lib.svoxt_leaf_neighbors(a["child"], a["pd"], a["n"], a["N"], a["depth"], a["L"], a["out"], a["ws"], a["nbytes"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_leaf_neighbors" in _C._lib.svoxt_last_error()


def test_leaf_neighbors_extents():
    lib = _C._lib
    # N^(depth + 1) has to stay below 2^31: 16^7 does, 16^8 does not; and 12 L
    assert lib.svoxt_leaf_neighbors(1, 1, 100, 16, 7, 5, 1, 1, 1 << 40, None) == INVALID and b"max_depth" in lib.svoxt_last_error()
    assert lib.svoxt_leaf_neighbors(1, 1, 100, 16, 6, 5, 1, None, 1 << 40, None) == INVALID and b"workspace is NULL" in lib.svoxt_last_error()
    n = 1 << 27
    assert lib.svoxt_leaf_neighbors(1, 1, n, 2, 9, (1 << 31) // 12 + 1, 1, 1, 1 << 40, None) == INVALID and b"12 * L" in lib.svoxt_last_error()
    # exactly the queried size passes the workspace check; no leaves: nothing to do, no HIP call
    q = lib.svoxt_neighbors_workspace_bytes(100, 2)
    assert lib.svoxt_leaf_neighbors(1, 1, 100, 2, 9, 0, None, 1, q, None) == 0
    assert lib.svoxt_leaf_neighbors(1, 1, 100, 2, 9, 0, None, 1, q - 1, None) == INVALID and b"workspace smaller" in lib.svoxt_last_error()


PLAN_OK = dict(nb=1, depths=1, rows=1, L=100, M=50, marks=1, mbytes=1 << 40, count=1)
PLAN_BAD = [("nb", None), ("depths", None), ("rows", None), ("L", -1), ("L", (1 << 31) // 12 + 1), ("M", -1), ("M", 1 << 31),
            ("marks", None), ("mbytes", 64)]


@pytest.mark.parametrize("field,value", PLAN_BAD + [("count", None)], ids=_ids(PLAN_BAD + [("count", None)]))
def test_tv_plan_count_rejects_before_any_hip_call(field, value):
    a = dict(PLAN_OK)
    a[field] = value
    rc = _C._lib.svoxt_tv_plan_count(a["nb"], a["depths"], a["rows"], a["L"], a["M"], a["marks"], a["mbytes"], a["count"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_tv_plan_count" in _C._lib.svoxt_last_error()


EMIT_BAD = PLAN_BAD + [("E", -1), ("E", 601), ("M", 1), ("ws", None), ("nbytes", 64), ("row_ptr", None), ("other", None), ("meta", None)]


@pytest.mark.parametrize("field,value", EMIT_BAD, ids=_ids(EMIT_BAD))
def test_tv_plan_emit_rejects_before_any_hip_call(field, value):
    a = dict(PLAN_OK, E=300, ws=1, nbytes=1 << 40, row_ptr=1, other=1, meta=1)
    a[field] = value
    rc = _C._lib.svoxt_tv_plan_emit(a["nb"], a["depths"], a["rows"], a["L"], a["M"], a["E"], a["marks"], a["mbytes"], a["ws"], a["nbytes"],
                                    a["row_ptr"], a["other"], a["meta"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_tv_plan_emit" in _C._lib.svoxt_last_error()


TV_OK = dict(f=1, M=50, K=4, row_ptr=1, other=1, meta=1, E=300, cols=None, n_cols=0, p=2, w=None, div=0.0, scale=0.0, mode=1, loss=1,
             table=1, ws=1, nbytes=1 << 40)
TV_BAD = [("p", 0), ("p", 3), ("mode", -1), ("mode", 3), ("M", -1), ("M", 1 << 31), ("K", 0), ("E", -1), ("E", 1 << 30), ("cols", 1),
          ("n_cols", 2), ("div", -1.0), ("div", float("nan")), ("div", float("inf")), ("scale", float("nan")), ("loss", None),
          ("table", None), ("f", None), ("row_ptr", None), ("other", None), ("meta", None), ("ws", None), ("nbytes", 64)]


def _tv(a):
    return _C._lib.svoxt_tv_rows(a["f"], a["M"], a["K"], a["row_ptr"], a["other"], a["meta"], a["E"], a["cols"], a["n_cols"], a["p"],
                                 a["w"], a["div"], a["scale"], a["mode"], a["loss"], a["table"], a["ws"], a["nbytes"], None)


@pytest.mark.parametrize("field,value", TV_BAD, ids=_ids(TV_BAD))
def test_tv_rows_rejects_before_any_hip_call(field, value):
    a = dict(TV_OK)
    a[field] = value
    assert _tv(a) == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_tv_rows" in _C._lib.svoxt_last_error()


def test_tv_rows_more_checks():
    lib = _C._lib
    assert _tv(dict(TV_OK, cols=1, n_cols=5)) == INVALID and b"n_cols" in lib.svoxt_last_error()       # more columns than K
    assert _tv(dict(TV_OK, M=1 << 30, K=256)) == INVALID and b"2^38" in lib.svoxt_last_error()
    assert _tv(dict(TV_OK, mode=2, table=None)) == INVALID and b"table is NULL" in lib.svoxt_last_error()
    q = lib.svoxt_tv_workspace_bytes(50, 4)
    assert _tv(dict(TV_OK, nbytes=q - 1)) == INVALID and b"workspace smaller" in lib.svoxt_last_error()
    assert _tv(dict(TV_OK, nbytes=q, other=None)) == INVALID and b"other" in lib.svoxt_last_error()    # ... and q passes that check
    assert _tv(dict(TV_OK, p=1, mode=2, loss=None, ws=None, nbytes=0, f=None)) == INVALID and b"features" in lib.svoxt_last_error()


def test_python_layer_refuses_cpu_trees_and_bad_arguments():
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=1)
    for call in (tree.leaf_neighbors, tree.tv, lambda: tree.tv_add_grad(torch.zeros_like(tree.features), 1.0)):
        with pytest.raises(RuntimeError, match="only the GPU \\(HIP\\) path exists"):
            call()
    assert tree._last_neighbors is None and tree._last_tv_plan is None
    with pytest.raises(RuntimeError, match="1 or 2"):
        _C.tv_rows(torch.zeros(2, 2), None, p=3)
    with pytest.raises(RuntimeError, match="weight"):
        _C.tv_rows(torch.zeros(2, 2), None, weight="volume")
    with pytest.raises(RuntimeError, match="another number"):
        _C.tv_rows(torch.zeros(2, 2), _C.TVPlan(None, None, None, 0, 3, None))
    with pytest.raises(RuntimeError, match="2\\^31"):
        _C.leaf_neighbors(torch.zeros(1, 16, 16, 16, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), 1, 4096, 7)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.leaf_neighbors(torch.zeros(1, 2, 2, 2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), 1, 8, 0)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.tv_plan(torch.zeros(8, 6, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64), 2, 2)
