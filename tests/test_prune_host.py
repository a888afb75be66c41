"""prune without a GPU: the numpy restatement the GPU tests compare with (tests/prune_restate.py) against small cases
worked out by hand and, on the reference-generated topology fixtures, against `integrity`; the C ABI's argument checks
(all made before any HIP call, so they run here) and the Python layer's refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from svox_t_amd import synth
from tests import prune_restate as R

G = os.path.join(os.path.dirname(__file__), "golden")
E = R.EMPTY_INDEX
INVALID = 1
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "topology_*.npz")))


def chain_tree():
    """N = 2, four nodes: the root's slot 0 -> node 1, whose slot 7 -> node 2, whose slot 3 -> node 3 (leaves of node
    3 at depth 3); the root's slot 5 -> node 4, all of whose leaves have rows.  Rows: 0 .. 7 node 3, 8 .. 15 node 4,
    16 the root's slot 1, 17 node 2's slot 0; inner slots hold a stale 99."""
    child = np.zeros((5, 8), np.int32)
    data = np.full((5, 8), E, np.int32)
    pd = np.zeros((5, 2), np.int32)
    for node, slot, kid in ((0, 0, 1), (1, 7, 2), (2, 3, 3), (0, 5, 4)):
        child[node, slot] = kid - node
        data[node, slot] = 99
        pd[kid] = (node * 8 + slot, pd[node, 1] + 1)
    data[3] = np.arange(8)
    data[4] = np.arange(8, 16)
    data[0, 1] = 16
    data[2, 0] = 17
    return child.reshape(5, 2, 2, 2), data.reshape(5, 2, 2, 2, 1), pd, 5, 18


def test_one_leaf_kept_at_depth_3_keeps_its_chain_of_ancestors():
    child, data, pd, n, M = chain_tree()
    keep = np.zeros((n, 8), bool)
    keep[3, 6] = True                                  # row 6
    c, d, p, n2, row_map, dropped = R.prune(child, data, pd, n, M, keep=keep.reshape(n, 2, 2, 2))
    assert n2 == 4 and dropped == 17
    want_child = np.zeros((4, 8), np.int32)
    want_child[0, 0], want_child[1, 7], want_child[2, 3] = 1, 1, 1          # node 4 is gone: the root's slot 5 is a leaf
    want_data = np.full((4, 8), E, np.int32)
    want_data[3, 6] = 0
    np.testing.assert_array_equal(c.reshape(4, 8), want_child)
    np.testing.assert_array_equal(d.reshape(4, 8), want_data)
    np.testing.assert_array_equal(p, [[0, 0], [0, 1], [15, 2], [19, 3]])
    np.testing.assert_array_equal(row_map, [6])
    R.integrity(c, d, p, n2, 2, 1)


def test_nothing_kept_leaves_the_root_alone():
    child, data, pd, n, M = chain_tree()
    c, d, p, n2, row_map, dropped = R.prune(child, data, pd, n, M, keep=np.zeros((n, 2, 2, 2), bool), reserve=2)
    assert n2 == 1 and dropped == 18 and row_map.shape == (0,) and c.shape[0] == 3
    assert not c.any() and (d == E).all() and not p.any()
    R.integrity(c, d, p, n2, 2, 0)


def test_everything_kept_keeps_the_topology_and_clears_stale_inner_words():
    child, data, pd, n, M = chain_tree()
    data[1, 0, 0, 1] = 5                               # a second leaf on row 5
    for collapse in (True, False):
        c, d, p, n2, row_map, dropped = R.prune(child, data, pd, n, M, keep=np.ones((n, 2, 2, 2), bool), collapse=collapse)
        assert n2 == n and dropped == 0
        np.testing.assert_array_equal(c, child)
        np.testing.assert_array_equal(p, pd)
        np.testing.assert_array_equal(row_map, np.arange(18))
        want = data.copy()
        want[child != 0] = E
        np.testing.assert_array_equal(d, want)
        R.integrity(c, d, p, n2, 2, 18)


def test_without_collapse_and_without_row_compaction_only_the_dropped_words_change():
    child, data, pd, n, M = chain_tree()
    keep = np.ones((n, 8), bool)
    keep[4] = False
    keep[2, 0] = False
    c, d, p, n2, row_map, dropped = R.prune(child, data, pd, n, M, keep=keep.reshape(n, 2, 2, 2), collapse=False,
                                            compact_features=False)
    assert n2 == n and row_map is None and dropped == 9
    np.testing.assert_array_equal(c, child)
    want = data.reshape(n, 8).copy()
    want[child.reshape(n, 8) != 0] = E
    want[4] = E
    want[2, 0] = E
    np.testing.assert_array_equal(d.reshape(n, 8), want)
    # the same with the nodes collapsed and the rows compacted: node 4 goes, rows 8 .. 15 and 17 go
    c, d, p, n2, row_map, _ = R.prune(child, data, pd, n, M, keep=keep.reshape(n, 2, 2, 2))
    assert n2 == 4
    np.testing.assert_array_equal(row_map, list(range(8)) + [16])
    assert d.reshape(4, 8)[0, 1] == 8 and c.reshape(4, 8)[0, 5] == 0


def test_weights_form_drops_nan_and_keeps_a_weight_equal_to_the_threshold():
    child, data, pd, n, M = chain_tree()
    w = np.zeros((n, 8), np.float32)
    w[3, 0], w[3, 1], w[3, 2], w[3, 3] = 0.25, np.nan, 0.2499999, np.inf
    *_, row_map, dropped = R.prune(child, data, pd, n, M, weights=w.reshape(n, 2, 2, 2), threshold=0.25)
    np.testing.assert_array_equal(row_map, [0, 3])
    assert dropped == 16


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_keeps_the_fixtures_whole(name):
    g = np.load(os.path.join(G, name))
    child, pd, n = g["child"], g["parent_depth"], int(g["n_internal"])
    N = child.shape[1]
    rng = np.random.default_rng(len(name) + n)
    data, M = R.number_leaves(child, n, rng)
    R.integrity(child, data, pd, n, N, M, collapsed=False, pruned=False)
    leaves = int((child == 0).sum())
    one = np.zeros(child.shape, bool)
    one.reshape(-1)[np.nonzero((child.reshape(-1) == 0) & (data.reshape(-1) != E))[0][-1]] = True
    masks = {"half": rng.random(child.shape) < 0.5, "few": rng.random(child.shape) < 0.05, "all": np.ones(child.shape, bool),
             "none": np.zeros(child.shape, bool), "one": one}
    for mname, keep in masks.items():
        for collapse in (True, False):
            for compact in (True, False):
                c, d, p, n2, row_map, dropped = R.prune(child, data, pd, n, M, keep=keep, collapse=collapse,
                                                        compact_features=compact, reserve=3)
                M2 = M if row_map is None else len(row_map)
                R.integrity(c, d, p, n2, N, M2, collapsed=collapse)
                assert c.shape[0] == n2 + 3 and not c[n2:].any() and (d[n2:] == E).all() and not p[n2:].any()
                assert (n2 == n) if not collapse else (n2 <= n)
                if mname == "all":
                    assert n2 == n and dropped == 0
                if mname == "none":
                    assert dropped == int(((child == 0) & (data[..., 0] != E)).sum()) and (n2 == 1 or not collapse)
                if mname == "one" and collapse:
                    assert n2 == int(pd[np.nonzero(one)[0][0], 1]) + 1            # the chain of ancestors and nothing else
                if row_map is not None:
                    assert (np.diff(row_map) > 0).all()
                    # a kept leaf reads the row it read before
                    kept_old = np.sort(data.reshape(-1)[(child.reshape(-1) == 0) & (data.reshape(-1) != E) & keep.reshape(-1)])
                    got = np.sort(row_map[d[:n2].reshape(-1)[(c[:n2].reshape(-1) == 0) & (d[:n2].reshape(-1) != E)]])
                    np.testing.assert_array_equal(got, kept_old)
    assert leaves > 0


def test_restatement_on_the_shell_tree():
    st = synth.shell_tree(5)
    rng = np.random.default_rng(5)
    keep = rng.random(st.child.shape) < 0.5
    c, d, p, n2, row_map, dropped = R.prune(st.child, st.data, st.parent_depth, st.n_internal, st.n_features, keep=keep)
    R.integrity(c, d, p, n2, 2, len(row_map))
    assert 1 < n2 < st.n_internal and len(row_map) + dropped == st.n_features


# ---- the C ABI's checks (every call below has one bad argument, so none reaches HIP)

OK = dict(child=1, data=1, pd=1, n=100, N=2, M=500, keep=1, weights=None, thr=0.0, ws=1, nbytes=1 << 40)
BAD = [("child", None), ("data", None), ("pd", None), ("n", 0), ("n", -1), ("n", 1 << 28), ("N", 1), ("N", 17), ("M", -1),
       ("M", 1 << 31), ("keep", None), ("weights", 1), ("ws", None), ("nbytes", 64)]


def _ids(bad):
    return [f"{f}={v}" for f, v in bad]


@pytest.mark.parametrize("field,value", BAD + [("counts", None)], ids=_ids(BAD + [("counts", None)]))
def test_count_rejects_before_any_hip_call(field, value):
    a = dict(OK, counts=1)
    a[field] = value
    rc = _C._lib.svoxt_prune_count(a["child"], a["data"], a["pd"], a["n"], a["N"], a["M"], a["keep"], a["weights"], a["thr"],
                                   1, 1, a["ws"], a["nbytes"], a["counts"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_prune_count" in _C._lib.svoxt_last_error()


EMIT_BAD = BAD + [("new_n", 0), ("new_n", 101), ("new_M", -1), ("new_M", 501), ("empty", 499), ("child_out", None),
                  ("data_out", None), ("pd_out", None), ("row_map", None)]


@pytest.mark.parametrize("field,value", EMIT_BAD, ids=_ids(EMIT_BAD))
def test_emit_rejects_before_any_hip_call(field, value):
    a = dict(OK, new_n=50, new_M=200, empty=E, child_out=1, data_out=1, pd_out=1, row_map=1)
    a[field] = value
    rc = _C._lib.svoxt_prune_emit(a["child"], a["data"], a["pd"], a["n"], a["N"], a["M"], a["keep"], a["weights"], a["thr"], 1,
                                  a["ws"], a["nbytes"], a["new_n"], a["new_M"], a["empty"], a["child_out"], a["data_out"],
                                  a["pd_out"], a["row_map"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_prune_emit" in _C._lib.svoxt_last_error()


def test_more_checks_and_the_workspace_query():
    lib = _C._lib
    # a NaN threshold; without compact_features the row count cannot change
    assert lib.svoxt_prune_count(1, 1, 1, 100, 2, 500, None, 1, float("nan"), 1, 1, 1, 1 << 40, 1, None) == INVALID
    assert b"NaN" in lib.svoxt_last_error()
    assert lib.svoxt_prune_emit(1, 1, 1, 100, 2, 500, 1, None, 0.0, 0, 1, 1 << 40, 50, 200, E, 1, 1, 1, None, None) == INVALID
    q = lib.svoxt_prune_workspace_bytes
    assert q(100, 500) >= 8 * (101 + 501) and q(1, 0) > 0       # a flag and a rank per node and per row
    assert q(0, 5) == -1 and q(5, -1) == -1 and q(1 << 31, 5) == -1
    # exactly the queried size passes the workspace check (and the next check, counts, then stops the call)
    assert lib.svoxt_prune_count(1, 1, 1, 100, 2, 500, 1, None, 0.0, 1, 1, 1, q(100, 500), None, None) == INVALID
    assert b"counts is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_prune_count(1, 1, 1, 100, 2, 500, 1, None, 0.0, 1, 1, 1, q(100, 500) - 1, None, None) == INVALID
    assert b"workspace smaller" in lib.svoxt_last_error()
    g = lib.svoxt_prune_gather_rows
    assert g(None, 0, None, None, 0, 4, None) == 0                      # nothing to move
    assert g(1, 5, 1, None, 3, 4, None) == INVALID and g(1, 5, None, 1, 3, 4, None) == INVALID
    assert g(None, 5, 1, 1, 3, 4, None) == INVALID and g(1, 5, 1, 1, 3, 0, None) == INVALID and g(1, 5, 1, 1, -1, 4, None) == INVALID


def test_python_layer_refuses_cpu_trees_and_bad_arguments():
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=1)
    with pytest.raises(RuntimeError, match="GPU"):
        tree.prune(torch.ones(tree.child.shape, dtype=torch.bool))
    for bad in (dict(keep=torch.ones(tree.child.shape, dtype=torch.bool)), dict(), dict(keep=1, weights=2)):
        with pytest.raises(RuntimeError) as e:
            _C.prune_tree(tree.child, tree.data, tree.parent_depth, tree.n_internal, tree.features.shape[0], **bad)
        assert not isinstance(e.value, NotImplementedError)
    with tree.accumulate_weights():
        with pytest.raises(RuntimeError, match="Tree locked"):
            tree.prune(torch.ones(tree.child.shape, dtype=torch.bool))
        with pytest.raises(RuntimeError, match="Tree locked"):
            tree.shrink_to_fit()


def test_shrink_to_fit_trims_the_tables():
    tree = svox.N3Tree(N=2, data_dim=4, init_reserve=50, init_refine=1)
    n = tree.n_internal
    assert tree.capacity > n
    child = tree.child[:n].clone()
    assert tree.shrink_to_fit() is True
    assert tree.capacity == n == tree.n_internal and tree.data.shape[0] == n and tree.parent_depth.shape[0] == n
    assert torch.equal(tree.child, child)
    assert tree.shrink_to_fit() is False
