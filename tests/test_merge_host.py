"""Frontier reductions and merge without a GPU: the numpy restatement (tests/merge_restate.py) against hand-worked
trees and against fixtures made by the reference's own Python (tests/golden/merge_*.npz, make_merge_golden.py); the
argument checks of the new C-ABI entry points, which come before any HIP call; the refusals of the Python surface."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import merge_restate as MR
from tests import prune_restate as PR

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "merge_*.npz")))
E = MR.EMPTY_INDEX


def chain_tree():
    """root -> node 1 (root slot 3) -> node 2 (node 1 slot 5); N = 2.  Leaves of node 2 name rows 0 .. 7, the other
    leaves of node 1 rows 8 .. 14, the root's other leaves are empty."""
    child = np.zeros((3, 2, 2, 2), np.int32)
    data = np.full((3, 8), E, np.int32)
    child.reshape(3, 8)[0, 3] = 1
    child.reshape(3, 8)[1, 5] = 1
    data[2] = np.arange(8)
    data[1, [0, 1, 2, 3, 4, 6, 7]] = np.arange(8, 15)
    pd = np.array([[0, 0], [3, 1], [8 + 5, 2]], np.int32)
    feats = np.arange(15 * 2, dtype=np.float32).reshape(15, 2) * np.float32(0.5)
    return child, data.reshape(3, 2, 2, 2, 1), pd, feats


def test_fixtures_exist():
    assert len(FIXTURES) >= 4


def test_chain_tree_by_hand():
    child, data, pd, feats = chain_tree()
    assert MR.frontier(child, 3).tolist() == [2]
    val, arg, count = MR.reduce(feats, data, 3, np.array([2]), "max")
    assert val.tolist() == [[7.0, 7.5]] and arg.tolist() == [[7, 7]] and count.tolist() == [8]
    assert MR.reduce(feats, data, 3, np.array([2]), "mean")[0].tolist() == [[3.5, 4.0]]
    assert MR.reduce(feats, data, 3, np.array([2]), "sum", cols=[1])[0].tolist() == [[32.0]]
    # rows 0 and 7 are the farthest apart: (7, 7) -> 7 sqrt 2
    assert MR.diam(feats, data, 3, np.array([2])).tolist() == [7.0 * np.sqrt(2.0)]
    assert MR.diam(feats, data, 3, np.array([2]), cols=[0], scale=2.0).tolist() == [14.0]
    c, d, p, n, table, row_map, added = MR.merge(child, data, pd, 3, feats, [2], op="mean")
    assert (n, added) == (2, 1) and row_map.tolist() == list(range(8, 15))
    assert c.reshape(2, 8).tolist() == [[0, 0, 0, 1, 0, 0, 0, 0], [0] * 8]
    assert d.reshape(2, 8)[1].tolist() == [0, 1, 2, 3, 4, 7, 5, 6]          # slot 5: the new row, behind the 7 carried ones
    assert d.reshape(2, 8)[0].tolist() == [E] * 8 and p.tolist() == [[0, 0], [3, 1]]
    assert table[7].tolist() == [3.5, 4.0] and np.array_equal(table[:7], feats[8:])
    PR.integrity(c, d, p, n, 2, table.shape[0], collapsed=False)
    # the second level: node 1 is a frontier node now
    c2, d2, p2, n2, table2, _, added2 = MR.merge(c, d, p, n, table, MR.frontier(c, n), op="max")
    assert (n2, added2) == (1, 1) and d2.reshape(8).tolist() == [E, E, E, 0, E, E, E, E] and table2.tolist() == [[14.0, 14.5]]
    # not selected, or not a frontier node: nothing happens
    same = MR.merge(child, data, pd, 3, feats, [1], compact_features=False)
    assert same[3] == 3 and same[6] == 0 and np.array_equal(same[0], child) and np.array_equal(same[1], data)


def test_root_only_all_equal_and_all_empty_by_hand():
    root = np.zeros((1, 2, 2, 2), np.int32)
    assert MR.frontier(root, 1).size == 0                         # the root is never a frontier node
    child, data, pd, feats = chain_tree()
    # all-equal children: the parent slot takes the word, no new row
    eq = data.copy()
    eq[2] = 4
    c, d, p, n, table, row_map, added = MR.merge(child, eq, pd, 3, feats, [2], compact_features=False)
    assert added == 0 and row_map is None and d.reshape(2, 8)[1, 5] == 4 and np.array_equal(table, feats)
    c, d, p, n, table, row_map, added = MR.merge(child, eq, pd, 3, feats, [2])
    assert added == 0 and row_map.tolist() == [4] + list(range(8, 15)) and d.reshape(2, 8)[1].tolist() == [1, 2, 3, 4, 5, 0, 6, 7]
    # an all-empty node: an empty leaf, under both modes; a mixed one: zero rows count under "zero", not under "skip"
    em = data.copy()
    em[2] = E
    em.reshape(3, 8)[2, 1] = -5                                    # another empty word: still "all empty"
    for mode in ("zero", "skip"):
        c, d, p, n, table, row_map, added = MR.merge(child, em, pd, 3, feats, [2], empty=mode)
        assert added == 0 and d.reshape(2, 8)[1, 5] == E and table.shape[0] == 7
    mixed = data.copy()
    mixed.reshape(3, 8)[2, 2:] = E                                 # rows 0 and 1 remain: (0, 0.5) and (1, 1.5)
    assert MR.reduce(feats, mixed, 3, np.array([2]), "mean", empty="zero")[0].tolist() == [[0.125, 0.25]]
    assert MR.reduce(feats, mixed, 3, np.array([2]), "mean", empty="skip")[0].tolist() == [[0.5, 1.0]]
    assert MR.reduce(feats, mixed, 3, np.array([2]), "min", empty="zero")[0].tolist() == [[0.0, 0.0]]
    assert MR.reduce(feats, mixed, 3, np.array([2]), "min", empty="skip")[0].tolist() == [[0.0, 0.5]]
    assert MR.diam(feats, mixed, 3, np.array([2]), empty="skip").tolist() == [np.sqrt(2.0)]
    assert MR.diam(feats, mixed, 3, np.array([2]), empty="zero").tolist() == [np.sqrt(1.0 + 2.25)]
    assert MR.reduce(feats, em, 3, np.array([2]), "max", empty="skip")[0].tolist() == [[0.0, 0.0]]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference_on_its_own_trees(name):
    """The reference reduced and merged the leaf WORDS (data_dim = 1); read as features[w] = w they are this fork's
    rows.  Frontier, max and the tables after merge(mask, torch.max) + shrink_to_fit(): equal word for word; the
    diameter of integers: exact."""
    g = np.load(os.path.join(G, name))
    child, data, pd = g["child"], g["data"], g["parent_depth"]
    n, N = child.shape[0], child.shape[1]
    M = int((child == 0).sum())
    feats = np.arange(M, dtype=np.float32)[:, None]
    # (inner slots hold the word 0 in the fixture: they are not leaves and are never read)
    fr = MR.frontier(child, n)
    np.testing.assert_array_equal(fr, g["frontier"])
    np.testing.assert_array_equal(MR.reduce(feats, data, n, fr, "max")[0], g["max_frontier"].astype(np.float32))
    want_diam = g["diam_frontier"].astype(np.float64)
    assert (want_diam == np.round(want_diam)).all() and want_diam.max() < 2 ** 24
    np.testing.assert_array_equal(MR.diam(feats, data, n, fr), want_diam)
    c, d, p, n2, table, row_map, added = MR.merge(child, data, pd, n, feats, fr[g["mask"]], op="max")
    np.testing.assert_array_equal(c, g["child_after"])
    np.testing.assert_array_equal(p, g["parent_depth_after"])
    assert n2 == g["child_after"].shape[0] and added == int(g["mask"].sum())
    leaf = c.reshape(-1) == 0
    np.testing.assert_array_equal(table[d.reshape(-1)[leaf], 0], g["data_after"].reshape(-1)[leaf].astype(np.float32))
    assert np.array_equal(table[:len(row_map), 0], row_map.astype(np.float32))
    PR.integrity(c, d, p, n2, N, table.shape[0], collapsed=False)


def test_new_symbols_and_abi_version():
    names = ["svoxt_frontier_workspace_bytes", "svoxt_frontier_count", "svoxt_frontier_emit", "svoxt_frontier_reduce",
             "svoxt_frontier_reduce_bwd", "svoxt_frontier_diam", "svoxt_merge_workspace_bytes", "svoxt_merge_count",
             "svoxt_merge_emit"]
    lib = ctypes.CDLL(_C.LIB_PATH)
    for nm in names:
        assert nm in _C.EXPORTS and hasattr(lib, nm), nm
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    for nm in ("assign_vertical", "calc_corners", "grid_weight_render"):
        with pytest.raises(NotImplementedError):
            getattr(_C, nm)()


def test_c_abi_argument_checks_come_before_any_hip_call():
    lib = _C._lib
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err = lambda: lib.svoxt_last_error()                                       # noqa: E731
    assert lib.svoxt_frontier_workspace_bytes(0) == -1 and lib.svoxt_frontier_workspace_bytes(1 << 31) == -1
    assert lib.svoxt_frontier_workspace_bytes(1000) >= 2 * 4 * 1001
    assert lib.svoxt_merge_workspace_bytes(0, 5) == -1 and lib.svoxt_merge_workspace_bytes(5, -1) == -1
    assert lib.svoxt_merge_workspace_bytes(1000, 500) >= 4 * (5 * 1001 + 2 * 501)
    assert lib.svoxt_frontier_count(p, 4, 1, p, 1 << 20, p, None) == 1 and b"branching" in err()
    assert lib.svoxt_frontier_count(p, 0, 2, p, 1 << 20, p, None) == 1 and b"n_internal" in err()
    assert lib.svoxt_frontier_count(None, 4, 2, p, 1 << 20, p, None) == 1 and b"NULL" in err()
    assert lib.svoxt_frontier_count(p, 4, 2, p, 8, p, None) == 1 and b"workspace smaller" in err()
    assert lib.svoxt_frontier_emit(p, 1 << 20, 4, 4, p, None) == 1 and b"F must be" in err()
    assert lib.svoxt_frontier_emit(p, 1 << 20, 1, 1, p, None) == 1
    assert lib.svoxt_frontier_emit(p, 1 << 20, 4, 2, None, None) == 1 and b"frontier is NULL" in err()
    assert lib.svoxt_frontier_emit(p, 1 << 20, 4, 0, None, None) == 0         # nothing to write
    red = lambda *a: lib.svoxt_frontier_reduce(*a)                              # noqa: E731
    assert red(p, 10, 0, p, 4, 2, p, 3, None, 0, 0, 0, p, None) == 1 and b"K must" in err()
    assert red(p, 10, 4, p, 4, 2, p, 3, None, 0, 4, 0, p, None) == 1 and b"op must" in err()
    assert red(p, 10, 4, p, 4, 2, p, 3, None, 0, 0, 2, p, None) == 1 and b"empty_mode" in err()
    assert red(p, 10, 4, p, 4, 2, p, 3, None, 2, 0, 0, p, None) == 1 and b"cols and n_cols" in err()
    assert red(p, 10, 4, p, 4, 2, p, 3, p, 0, 0, 0, p, None) == 1
    assert red(p, 10, 4, None, 4, 2, p, 3, None, 0, 0, 0, p, None) == 1 and b"NULL" in err()
    assert red(p, 10, 4, p, 4, 2, p, 3, None, 0, 0, 0, None, None) == 1 and b"out is NULL" in err()
    assert red(p, 10, 4, p, 4, 2, p, -1, None, 0, 0, 0, p, None) == 1
    assert red(p, 10, 4, p, 4, 2, p, 0, None, 0, 0, 0, None, None) == 0       # no node: nothing to do
    assert lib.svoxt_frontier_reduce_bwd(p, 10, 4, p, 4, 2, p, 3, None, 0, 0, 0, p, None, None) == 1 and b"grad_features" in err()
    assert lib.svoxt_frontier_reduce_bwd(p, 10, 4, p, 4, 2, p, 3, None, 0, 0, 0, None, p, None) == 1 and b"grad_out" in err()
    assert lib.svoxt_frontier_diam(p, 10, 4, p, 4, 2, p, 3, None, 0, 0, float("nan"), p, None) == 1 and b"NaN" in err()
    assert lib.svoxt_frontier_diam(p, 10, 4, p, 4, 17, p, 3, None, 0, 0, 1.0, p, None) == 1 and b"branching" in err()
    assert lib.svoxt_frontier_diam(p, 10, 4, p, 4, 2, p, 3, None, 0, 0, 1.0, None, None) == 1 and b"out is NULL" in err()
    big = 1 << 20
    assert lib.svoxt_merge_count(p, p, p, 4, 2, 10, None, 1, p, big, p, None) == 1 and b"NULL" in err()
    assert lib.svoxt_merge_count(p, p, p, 4, 2, 10, p, 1, None, big, p, None) == 1 and b"workspace is NULL" in err()
    assert lib.svoxt_merge_count(p, p, p, 4, 2, 10, p, 1, p, 16, p, None) == 1 and b"workspace smaller" in err()
    assert lib.svoxt_merge_count(p, p, p, 4, 2, 10, p, 1, p, big, None, None) == 1 and b"counts is NULL" in err()
    assert lib.svoxt_merge_count(p, p, p, 1 << 29, 2, 10, p, 1, p, big, p, None) == 1 and b"2^31" in err()
    emit = lambda **k: lib.svoxt_merge_emit(p, p, p, 4, 2, 10, p, k.get("compact", 1), p, big, k.get("new_n", 3), k.get("carried", 9),   # noqa: E731
                                            k.get("added", 1), k.get("empty", E), p, p, k.get("pd", p), k.get("row_map", p),
                                            k.get("new_nodes", p), None)
    assert emit(new_n=0) == 1 and b"new_n_internal" in err()
    assert emit(new_n=5) == 1
    assert emit(carried=11) == 1 and b"carried" in err()
    assert emit(compact=0, carried=9) == 1 and b"carried" in err()
    assert emit(added=2) == 1 and b"rows_added" in err()
    assert emit(empty=9) == 1 and b"empty_index" in err()
    assert emit(pd=None) == 1 and b"parent_depth_out" in err()
    assert emit(row_map=None) == 1 and b"row_map is NULL" in err()
    assert emit(new_nodes=None) == 1 and b"new_row_nodes is NULL" in err()


def test_python_refusals():
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=1)                         # a CPU tree
    for call in (tree.frontier, tree.reduce_frontier, tree.max_frontier, tree.diam_frontier, tree.merge,
                 lambda: tree.simplify(0.1)):
        with pytest.raises(RuntimeError, match="GPU") as e:
            call()
        assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="op must be"):
        tree.merge(op="sum")                                                   # sum is a reduction, not a merge
    with pytest.raises(RuntimeError, match="op must be"):
        tree.merge(op=torch.median)
    with pytest.raises(RuntimeError, match="empty must be"):
        tree.merge(empty="drop")
    with pytest.raises(RuntimeError, match="op must be"):
        tree.simplify(0.1, op="sum")
    with tree.accumulate_weights():
        for call in (tree.merge, lambda: tree.simplify(0.1)):
            with pytest.raises(RuntimeError, match="Tree locked"):
                call()
    with pytest.raises(RuntimeError, match="Cannot merge root node"):
        svox.N3Tree(N=2, data_dim=4).merge()
    # the operator layer: shapes and values are checked before devices
    n = tree.n_internal
    args = (tree.child, tree.data, tree.parent_depth, n, tree.features.detach())
    ok = torch.ones(n, dtype=torch.bool)
    with pytest.raises(RuntimeError, match=r"selected must be .* \[n_internal\]"):
        _C.merge_tree(*args, ok[:-1])                                          # a mask of the wrong length
    with pytest.raises(RuntimeError, match="selected must be"):
        _C.merge_tree(*args, ok.float())
    with pytest.raises(RuntimeError, match="op must be"):
        _C.merge_tree(*args, ok, op="sum")
    with pytest.raises(RuntimeError, match="reserve"):
        _C.merge_tree(*args, ok, reserve=-1)
    with pytest.raises(RuntimeError, match="n_internal"):
        _C.merge_tree(tree.child, tree.data, tree.parent_depth, n + 1, tree.features.detach(), ok)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.merge_tree(*args, ok)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.frontier_nodes(tree.child, n)
    nodes = torch.arange(1, n)
    with pytest.raises(RuntimeError, match="op must be"):
        _C.frontier_reduce(tree.features.detach(), tree.data, n, 2, nodes, None, "median")
    with pytest.raises(RuntimeError, match="empty must be"):
        _C.frontier_reduce(tree.features.detach(), tree.data, n, 2, nodes, None, "max", "drop")
    with pytest.raises(RuntimeError, match="nodes must be int64"):
        _C.frontier_reduce(tree.features.detach(), tree.data, n, 2, nodes.int())
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.frontier_diam(tree.features.detach(), tree.data, n, 2, nodes)
