"""subdivide / unshare without a GPU: the numpy restatement the GPU tests compare with (tests/subdivide_restate.py)
against the reference-generated fixtures (tests/golden/subdivide_*.npz: the reference's own refine(sel)) and small cases
worked out by hand, `integrity` on its outputs; the C ABI's argument checks (all made before any HIP call, so they run
here) and the Python layer's refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import prune_restate as P
from tests import subdivide_restate as R

G = os.path.join(os.path.dirname(__file__), "golden")
E = R.EMPTY_INDEX
INVALID = 1
GOLDEN = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "subdivide_*.npz")))
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "topology_*.npz")))


def test_there_is_a_fixture_for_every_tree_of_the_merge_fixtures():
    assert [g.replace("subdivide_", "") for g in GOLDEN] == \
        sorted(os.path.basename(p).replace("merge_", "") for p in glob.glob(os.path.join(G, "merge_*.npz")))
    assert len(GOLDEN) == 5


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_equals_the_references_refine(name):
    g = np.load(os.path.join(G, name))
    child, data, pd, mask = g["child"], g["data"], g["parent_depth"], g["mask"]
    n, N = child.shape[0], child.shape[1]
    M = int((child == 0).sum())                        # a distinct word per leaf: 0 .. leaves - 1
    c, d, p, added, rows_added, row_map = R.subdivide(child, data, pd, n, M, sel=mask, own_rows=False, split_empty=True)
    assert added == int((mask & (child == 0)).sum()) > 0 and rows_added == 0 and row_map is None
    for got, want, what in ((c, g["child_after"], "child"), (d, g["data_after"], "data"), (p, g["parent_depth_after"], "parent_depth")):
        assert got.dtype == want.dtype and got.shape == want.shape, what
        np.testing.assert_array_equal(got, want, err_msg=what)
    R.integrity(c, d, p, n + added, N, M, n_before=n)
    # with rows of their own: the same topology, and slot 0 of every new node reads what the reference's reads
    c2, d2, p2, added2, rows2, row_map2 = R.subdivide(child, data, pd, n, M, sel=mask, own_rows=True)
    assert added2 == added and rows2 == added * (N ** 3 - 1)
    np.testing.assert_array_equal(c2, c)
    np.testing.assert_array_equal(p2, p)
    np.testing.assert_array_equal(row_map2[d2[n:].reshape(added, -1)], d[n:].reshape(added, -1))
    R.integrity(c2, d2, p2, n + added, N, M + rows2, n_before=n, own_rows=True, row_map=row_map2, M_before=M)


def small_tree():
    """N = 2, two nodes: the root's slot 3 -> node 1.  Rows: the root's slots 0, 1, 2 name 0, 1, 1 (one shared), slot 4
    is empty; node 1's slots name 2 .. 9 except slot 5, which names row 0 again.  Capacity 3."""
    child = np.zeros((3, 8), np.int32)
    data = np.full((3, 8), E, np.int32)
    pd = np.zeros((3, 2), np.int32)
    child[0, 3] = 1
    data[0, 3] = 77                                    # a stale word at an inner slot
    pd[1] = (3, 1)
    data[0, :3] = (0, 1, 1)
    data[1] = np.arange(2, 10)
    data[1, 5] = 0
    return child.reshape(3, 2, 2, 2), data.reshape(3, 2, 2, 2, 1), pd, 2, 10


def test_a_case_by_hand():
    child, data, pd, n, M = small_tree()
    sel = np.zeros((3, 8), bool)
    sel[0, 1] = sel[0, 3] = sel[0, 4] = sel[1, 7] = True           # a leaf, an inner slot (ignored), an empty leaf, a leaf
    sel[2] = True                                                  # behind the tree: ignored
    c, d, p, added, rows, row_map = R.subdivide(child, data, pd, n, M, sel=sel.reshape(3, 2, 2, 2))
    assert (added, rows) == (2, 14) and c.shape[0] == 4            # regrown to exactly what holds the tree
    c, d = c.reshape(4, 8), d.reshape(4, 8)
    assert c[0, 1] == 2 and c[1, 7] == 2 and c[0, 3] == 1 and c[0, 4] == 0 and not c[2:].any()
    np.testing.assert_array_equal(p, [[0, 0], [3, 1], [1, 1], [15, 2]])
    np.testing.assert_array_equal(d[2], [1] + list(range(10, 17)))
    np.testing.assert_array_equal(d[3], [9] + list(range(17, 24)))
    assert d[0, 1] == 1 and d[1, 7] == 9 and d[0, 3] == 77         # the split slots' own words stay
    np.testing.assert_array_equal(row_map, list(range(10)) + [1] * 7 + [9] * 7)
    R.integrity(c, d, p, 4, 2, 24, n_before=2, own_rows=True, row_map=row_map, M_before=10)
    # empty leaves split on request, into empty leaves and no rows; max_depth holds back node 1's leaves
    c, d, p, added, rows, row_map = R.subdivide(child, data, pd, n, M, sel=sel.reshape(3, 2, 2, 2), split_empty=True, max_depth=1)
    assert (added, rows) == (2, 7)
    assert (d.reshape(-1, 8)[3] == E).all() and list(p[3]) == [4, 1] and list(p[2]) == [1, 1]
    # depth_limit 0: nothing splits, row_map is the identity
    c, d, p, added, rows, row_map = R.subdivide(child, data, pd, n, M, depth_limit=0)
    assert (added, rows) == (0, 0) and c.shape[0] == 3
    np.testing.assert_array_equal(row_map, np.arange(10))
    np.testing.assert_array_equal(c, child)
    np.testing.assert_array_equal(d, data)
    # weights: NaN never splits, a weight equal to the threshold does
    w = np.zeros((3, 8), np.float32)
    w[0, 0], w[0, 1], w[0, 2] = np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(0))
    *_, added, rows, row_map = R.subdivide(child, data, pd, n, M, weights=w.reshape(3, 2, 2, 2), threshold=0.5)
    assert added == 1 and list(row_map[10:]) == [1] * 7


def test_unshare_by_hand():
    child, data, pd, n, M = small_tree()
    d, rows, row_map = R.unshare(child, data, n, M)
    d = d.reshape(3, 8)
    assert rows == 2
    np.testing.assert_array_equal(d[0, :5], [0, 1, 10, 77, E])     # the second leaf on row 1 moves; the inner slot is left alone
    assert d[1, 5] == 11 and (d[2] == E).all()
    np.testing.assert_array_equal(row_map, list(range(10)) + [1, 0])
    d2, rows2, row_map2 = R.unshare(child, d.reshape(data.shape), n, M + rows)
    assert rows2 == 0 and (d2.reshape(3, 8) == d).all()
    np.testing.assert_array_equal(row_map2, np.arange(12))


@pytest.mark.parametrize("name", FIXTURES)
def test_integrity_of_the_restatements_outputs(name):
    g = np.load(os.path.join(G, name))
    child, pd, n = g["child"], g["parent_depth"], int(g["n_internal"])
    N = child.shape[1]
    rng = np.random.default_rng(len(name) + n)
    data, M = P.number_leaves(child, n, rng)
    masks = {"half": rng.random(child.shape) < 0.5, "few": rng.random(child.shape) < 0.05, "all": None,
             "none": np.zeros(child.shape, bool)}
    leaves = (child[:n] == 0)
    full = leaves & (data[:n, ..., 0] != E)
    for mname, sel in masks.items():
        for own in (True, False):
            for empty in (True, False):
                c, d, p, added, rows, row_map = R.subdivide(child, data, pd, n, M, sel=sel, own_rows=own, split_empty=empty)
                chosen = (leaves if empty else full) & (True if sel is None else sel[:n])
                assert added == int(chosen.sum()) and c.shape[0] == max(child.shape[0], n + added)
                assert rows == (int((chosen & full).sum()) * (N ** 3 - 1) if own else 0)
                R.integrity(c, d, p, n + added, N, M + rows, n_before=n, own_rows=own, row_map=row_map, M_before=M)
                if mname == "none":
                    np.testing.assert_array_equal(c, child)
                    np.testing.assert_array_equal(d, data)
                # unshare behind it: every row named once, and every leaf reads the row it read before
                d3, rows3, row_map3 = R.unshare(c, d, n + added, M + rows)
                at = (c[:n + added].reshape(-1) == 0) & (d3[:n + added].reshape(-1) != E)
                named = d3[:n + added].reshape(-1)[at]
                assert np.unique(named).size == named.size and rows3 + M + rows == len(row_map3)
                np.testing.assert_array_equal(row_map3[named], d[:n + added].reshape(-1)[at])


# ---- the C ABI's checks (every call below has one bad argument, so none reaches HIP)

OK = dict(child=1, data=1, pd=1, n=100, N=2, M=500, sel=1, weights=None, thr=0.0, ws=1, nbytes=1 << 40)
BAD = [("n", 0), ("n", -1), ("n", 1 << 28), ("N", 1), ("N", 17), ("M", -1), ("M", 1 << 31), ("ws", None), ("nbytes", 64)]
TABLES = [("child", None), ("data", None), ("pd", None)]


def _ids(bad):
    return [f"{f}={v}" for f, v in bad]


COUNT_BAD = BAD + TABLES + [("weights", 1), ("counts", None)]


@pytest.mark.parametrize("field,value", COUNT_BAD, ids=_ids(COUNT_BAD))
def test_subdivide_count_rejects_before_any_hip_call(field, value):
    a = dict(OK, counts=1)
    a[field] = value
    rc = _C._lib.svoxt_subdivide_count(a["child"], a["data"], a["pd"], a["n"], a["N"], a["M"], a["sel"], a["weights"], a["thr"], 10,
                                       0, 1, a["ws"], a["nbytes"], a["counts"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_subdivide_count" in _C._lib.svoxt_last_error()


EMIT_BAD = BAD + TABLES + [("cap", 149), ("cap", 1 << 28), ("added", -1), ("added", 801), ("rows", -7), ("rows", 6), ("rows", 357),
                           ("empty", 500 + 70), ("row_map", None)]


@pytest.mark.parametrize("field,value", EMIT_BAD, ids=_ids(EMIT_BAD))
def test_subdivide_emit_rejects_before_any_hip_call(field, value):
    a = dict(OK, cap=150, added=50, rows=70, empty=E, row_map=1)
    a[field] = value
    rc = _C._lib.svoxt_subdivide_emit(a["child"], a["data"], a["pd"], a["n"], a["N"], a["M"], a["cap"], 1, a["ws"], a["nbytes"],
                                      a["added"], a["rows"], a["empty"], a["row_map"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_subdivide_emit" in _C._lib.svoxt_last_error()


UNSHARE_BAD = BAD + TABLES[:2] + [("counts", None)]


@pytest.mark.parametrize("field,value", UNSHARE_BAD, ids=_ids(UNSHARE_BAD))
def test_unshare_count_rejects_before_any_hip_call(field, value):
    a = dict(OK, counts=1)
    a[field] = value
    rc = _C._lib.svoxt_unshare_count(a["child"], a["data"], a["n"], a["N"], a["M"], a["ws"], a["nbytes"], a["counts"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_unshare_count" in _C._lib.svoxt_last_error()


UNSHARE_EMIT_BAD = BAD + [("data", None), ("rows", -1), ("rows", 801), ("empty", 520), ("row_map", None)]


@pytest.mark.parametrize("field,value", UNSHARE_EMIT_BAD, ids=_ids(UNSHARE_EMIT_BAD))
def test_unshare_emit_rejects_before_any_hip_call(field, value):
    a = dict(OK, rows=20, empty=E, row_map=1)
    a[field] = value
    rc = _C._lib.svoxt_unshare_emit(a["data"], a["n"], a["N"], a["M"], a["ws"], a["nbytes"], a["rows"], a["empty"], a["row_map"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_unshare_emit" in _C._lib.svoxt_last_error()


def test_more_checks_the_workspace_query_and_the_abi_version():
    lib = _C._lib
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22          # entry points were added, nothing changed
    for nm in ("svoxt_subdivide_workspace_bytes", "svoxt_subdivide_count", "svoxt_subdivide_emit", "svoxt_unshare_count",
               "svoxt_unshare_emit"):
        assert nm in _C.EXPORTS and hasattr(lib, nm), nm
    # both selections at once; a NaN threshold; rows without own_rows
    assert lib.svoxt_subdivide_count(1, 1, 1, 100, 2, 500, 1, 1, 0.0, 10, 0, 1, 1, 1 << 40, 1, None) == INVALID
    assert b"at most one" in lib.svoxt_last_error()
    assert lib.svoxt_subdivide_count(1, 1, 1, 100, 2, 500, None, 1, float("nan"), 10, 0, 1, 1, 1 << 40, 1, None) == INVALID
    assert b"NaN" in lib.svoxt_last_error()
    assert lib.svoxt_subdivide_emit(1, 1, 1, 100, 2, 500, 150, 0, 1, 1 << 40, 50, 70, E, None, None) == INVALID
    assert b"rows_added" in lib.svoxt_last_error()
    # the slot range: 100 + 50 nodes fit a capacity of 150 rows, not one of 149; a capacity of 2^28 rows of 8 slots is 2^31 slots
    assert lib.svoxt_subdivide_emit(1, 1, 1, 100, 2, 500, 149, 1, 1, 1 << 40, 50, 70, E, 1, None) == INVALID
    assert b"capacity" in lib.svoxt_last_error()
    assert lib.svoxt_subdivide_emit(1, 1, 1, 100, 2, 500, 1 << 28, 1, 1, 1 << 40, 50, 70, E, 1, None) == INVALID
    assert b"2^31" in lib.svoxt_last_error()
    q = lib.svoxt_subdivide_workspace_bytes
    assert q(100, 2, 500) >= 4 * 5 * 801 and q(1, 2, 0) > 0 and q(1, 2, 10 ** 6) >= 4 * 10 ** 6      # five words a slot; a word a row
    assert q(0, 2, 5) == -1 and q(5, 2, -1) == -1 and q(1 << 28, 2, 5) == -1 and q(5, 1, 5) == -1 and q(5, 17, 5) == -1
    # exactly the queried size passes the workspace check (and the next check, counts, then stops the call)
    assert lib.svoxt_unshare_count(1, 1, 100, 2, 500, 1, q(100, 2, 500), None, None) == INVALID
    assert b"counts is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_unshare_count(1, 1, 100, 2, 500, 1, q(100, 2, 500) - 1, None, None) == INVALID
    assert b"workspace smaller" in lib.svoxt_last_error()


def test_python_layer_refuses_cpu_trees_and_bad_arguments():
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=1)
    ok = torch.ones(tree.child.shape, dtype=torch.bool)
    child, data, filled = tree.child.clone(), tree.data.clone(), tree.filled
    with pytest.raises(RuntimeError, match="only the GPU \\(HIP\\) path exists"):
        tree.subdivide(ok)
    with pytest.raises(RuntimeError, match="only the GPU \\(HIP\\) path exists"):
        tree.subdivide()
    with pytest.raises(RuntimeError, match="only the GPU \\(HIP\\) path exists"):
        tree.unshare()
    bad = [dict(sel=ok, weights=ok.float(), threshold=0.0), dict(weights=ok.float()), dict(sel=ok[:-1]), dict(sel=ok.reshape(-1)),
           dict(sel=ok.float()), dict(weights=ok.double(), threshold=0.0), dict(weights=ok.float()[..., :1], threshold=0.0),
           dict(sel=ok, threshold=0.5), dict(sel=[1, 2])]
    for kw in bad:
        with pytest.raises(RuntimeError) as e:
            tree.subdivide(**kw)
        assert not isinstance(e.value, NotImplementedError) and "GPU" not in str(e.value), kw
    for kw in (dict(sel=ok, weights=ok.float(), threshold=0.0), dict(weights=ok.float()), dict(sel=ok[:-1])):
        with pytest.raises(RuntimeError) as e:
            _C.subdivide_tree(tree.child, tree.data, tree.parent_depth, tree.n_internal, tree.features.shape[0], **kw)
        assert not isinstance(e.value, NotImplementedError)
    with tree.accumulate_weights() as accum:
        with pytest.raises(RuntimeError, match="Tree locked"):
            tree.subdivide(weights=accum.value, threshold=0.0)
        with pytest.raises(RuntimeError, match="Tree locked"):
            tree.unshare()
    assert torch.equal(tree.child, child) and torch.equal(tree.data, data) and tree.filled == filled
