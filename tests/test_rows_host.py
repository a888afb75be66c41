"""Samples to feature rows and back without a GPU: the C ABI's argument checks, the Python layer's, and the anchors of
the restatement (tests/rows_restate.py)."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import rows_restate as R

NAMES = ("svoxt_row_plan_workspace_bytes", "svoxt_row_plan_build", "svoxt_row_plan_long", "svoxt_gather_rows",
         "svoxt_reduce_rows_workspace_bytes", "svoxt_reduce_rows")
BIG = 1 << 31


def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    assert _C._extras.ROW_CHUNK == 256 and _C._extras.ROWS_OPS == {"sum": 0, "mean": 1, "max": 2, "min": 3}


def test_workspace_queries():
    pw, rw = _C._lib.svoxt_row_plan_workspace_bytes, _C._lib.svoxt_reduce_rows_workspace_bytes
    assert pw(0, 0) == 0 and pw(0, 1000) == 0
    for T, M in ((-1, 4), (BIG, 4), (4, -1), (4, BIG)):
        assert pw(T, M) == -1
    for T, M in ((1, 0), (1, 1), (5000, 37), (100000, 3344), (BIG - 1, 1)):
        b = pw(T, M)
        assert b > 0 and b % 256 == 0 and b >= 4 * 4 * T + 4 * 4 * (M + 1)     # two key and two value arrays, four marks
    assert rw(0, 1) == 0 and rw(0, 28) == 0
    for n, C in ((-1, 1), (BIG, 1), (4, 0), (4, -2), (BIG - 1, 1 << 10)):
        assert rw(n, C) == -1
    for n, C in ((1, 1), (7, 28), (1000, 33)):
        assert rw(n, C) >= 4 * n * C and rw(n, C) % 256 == 0


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    err = lib.svoxt_last_error
    buf = (ctypes.c_float * 96)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd4 = ctypes.c_void_p(p.value + 4)                # 4-byte aligned, not 8
    odd1 = ctypes.c_void_p(p.value + 1)
    build, long_, gather, reduce = lib.svoxt_row_plan_build, lib.svoxt_row_plan_long, lib.svoxt_gather_rows, lib.svoxt_reduce_rows
    wb = lib.svoxt_row_plan_workspace_bytes(600, 8)

    # the extents, first everywhere
    for T, M in ((-1, 4), (BIG, 4)):
        assert build(p, T, M, p, p, p, p, 1 << 40, None) == 1 and b"svoxt_row_plan_build: T must be in [0, 2^31)" in err()
        assert long_(p, T, M, 0, 0, p, 1 << 40, p, p, p, None) == 1 and b"svoxt_row_plan_long: T must be in [0, 2^31)" in err()
        assert gather(p, M, 4, p, T, None, 0, p, None) == 1 and b"svoxt_gather_rows: T must be in [0, 2^31)" in err()
        assert reduce(p, T, 4, p, p, M, p, p, p, 0, 0, None, 0, 4, 0, 0.0, p, p, 1 << 40, None) == 1 and \
            b"svoxt_reduce_rows: T must be in [0, 2^31)" in err()
    for T, M in ((4, -1), (4, BIG)):
        assert build(p, T, M, p, p, p, p, 1 << 40, None) == 1 and b"svoxt_row_plan_build: M must be in [0, 2^31)" in err()
        assert long_(p, T, M, 0, 0, p, 1 << 40, p, p, p, None) == 1 and b"svoxt_row_plan_long: M must be in [0, 2^31)" in err()
        assert gather(p, M, 4, p, T, None, 0, p, None) == 1 and b"svoxt_gather_rows: M must be in [0, 2^31)" in err()
        assert reduce(p, T, 4, p, p, M, p, p, p, 0, 0, None, 0, 4, 0, 0.0, p, p, 1 << 40, None) == 1 and \
            b"svoxt_reduce_rows: M must be in [0, 2^31)" in err()

    # svoxt_row_plan_build: outputs, inputs, alignment, the workspace
    assert build(p, 600, 8, None, p, p, p, wb, None) == 1 and b"svoxt_row_plan_build: row_ptr is NULL" in err()
    assert build(p, 600, 8, p, p, None, p, wb, None) == 1 and b"svoxt_row_plan_build: info is NULL" in err()
    assert build(None, 600, 8, p, p, p, p, wb, None) == 1 and b"svoxt_row_plan_build: row / perm is NULL" in err()
    assert build(p, 600, 8, p, None, p, p, wb, None) == 1 and b"svoxt_row_plan_build: row / perm is NULL" in err()
    for a in ((odd1, p, p), (p, odd1, p), (p, p, odd1)):
        assert build(a[0], 600, 8, a[1], a[2], p, p, wb, None) == 1 and b"svoxt_row_plan_build: row / row_ptr / perm is not 4-byte" in err()
    assert build(p, 600, 8, p, p, odd4, p, wb, None) == 1 and b"svoxt_row_plan_build: info is not 8-byte aligned" in err()
    assert build(p, 600, 8, p, p, p, odd1, wb, None) == 1 and b"svoxt_row_plan_build: workspace is not 4-byte aligned" in err()
    assert build(p, 600, 8, p, p, p, None, wb, None) == 1 and b"svoxt_row_plan_build: workspace is NULL" in err()
    assert build(p, 600, 8, p, p, p, p, wb - 1, None) == 1 and b"svoxt_row_plan_build: workspace smaller" in err()

    # svoxt_row_plan_long: the counts against T and M, the outputs, the workspace
    for n_long, n_chunks in ((-1, 0), (9, 18), (3, 6)):                # negative; above M = 8; above 600 / 257 = 2
        assert long_(p, 600, 8, n_long, n_chunks, p, wb, p, p, p, None) == 1 and b"svoxt_row_plan_long: n_long must be in" in err()
    for n_long, n_chunks in ((2, 3), (2, 5), (0, 3)):                  # below 2 n_long; above 600 / 256 + n_long
        assert long_(p, 600, 8, n_long, n_chunks, p, wb, p, p, p, None) == 1 and b"svoxt_row_plan_long: n_chunks must be in" in err()
    assert long_(p, 600, 8, 2, 4, p, wb, p, None, p, None) == 1 and b"svoxt_row_plan_long: long_chunk_ptr is NULL" in err()
    for a in ((None, p, p), (p, None, p), (p, p, None)):
        assert long_(a[0], 600, 8, 2, 4, p, wb, a[1], p, a[2], None) == 1 and \
            b"svoxt_row_plan_long: row_ptr / long_rows / chunk_long is NULL" in err()
    for a in ((odd1, p, p, p), (p, odd1, p, p), (p, p, odd1, p), (p, p, p, odd1)):
        assert long_(a[0], 600, 8, 2, 4, p, wb, a[1], a[2], a[3], None) == 1 and b"svoxt_row_plan_long: row_ptr / long_rows" in err() \
            and b"not 4-byte aligned" in err()
    assert long_(p, 600, 8, 2, 4, odd1, wb, p, p, p, None) == 1 and b"svoxt_row_plan_long: workspace is not 4-byte aligned" in err()
    assert long_(p, 600, 8, 2, 4, None, wb, p, p, p, None) == 1 and b"svoxt_row_plan_long: workspace is NULL" in err()
    assert long_(p, 600, 8, 2, 4, p, wb - 1, p, p, p, None) == 1 and b"svoxt_row_plan_long: workspace smaller" in err()

    # svoxt_gather_rows
    for K in (0, -3):
        assert gather(p, 8, K, p, 4, None, 0, p, None) == 1 and b"svoxt_gather_rows: K must be >= 1" in err()
    for cols, n in ((None, 2), (p, 0), (p, -1), (p, 5)):
        assert gather(p, 8, 4, p, 4, cols, n, p, None) == 1 and b"svoxt_gather_rows: cols / n_cols must be" in err()
    assert gather(p, 8, 1 << 10, p, BIG - 1, None, 0, p, None) == 1 and b"svoxt_gather_rows: T * columns and M * K must be below 2^38" in err()
    assert gather(p, BIG - 1, 1 << 10, p, 4, p, 1, p, None) == 1 and b"svoxt_gather_rows: T * columns and M * K must be below 2^38" in err()
    assert gather(p, 8, 4, None, 4, None, 0, p, None) == 1 and b"svoxt_gather_rows: row / out is NULL" in err()
    assert gather(p, 8, 4, p, 4, None, 0, None, None) == 1 and b"svoxt_gather_rows: row / out is NULL" in err()
    assert gather(None, 8, 4, p, 4, None, 0, p, None) == 1 and b"svoxt_gather_rows: table is NULL" in err()
    for a in ((odd1, p, p, p), (p, odd1, p, p), (p, p, odd1, p), (p, p, p, odd1)):
        assert gather(a[0], 8, 4, a[1], 4, a[2], 2, a[3], None) == 1 and b"svoxt_gather_rows: a misaligned argument" in err()

    # svoxt_reduce_rows
    red = lambda values=p, T=600, C=4, row_ptr=p, perm=p, M=8, lr=p, lcp=p, cl=p, n_long=0, n_chunks=0, cols=None, n_cols=0, K=4, op=0, \
        empty=0.0, out=p, ws=p, wsb=1 << 20: reduce(values, T, C, row_ptr, perm, M, lr, lcp, cl, n_long, n_chunks, cols, n_cols, K, op,
                                                    empty, out, ws, wsb, None)
    for kw in (dict(C=0), dict(C=-1), dict(K=0)):
        assert red(**kw) == 1 and b"svoxt_reduce_rows: C and K must be >= 1" in err()
    for kw in (dict(cols=None, n_cols=2), dict(cols=p, n_cols=0), dict(cols=p, n_cols=-1), dict(cols=p, n_cols=5)):
        assert red(**kw) == 1 and b"svoxt_reduce_rows: cols / n_cols must be" in err()
    for kw in (dict(C=3), dict(cols=p, n_cols=2, C=4), dict(cols=p, n_cols=2, C=1)):
        assert red(**kw) == 1 and b"svoxt_reduce_rows: values must have one column per selected column" in err()
    for op in (-1, 4, 99):
        assert red(op=op) == 1 and b"svoxt_reduce_rows: op must be one of SVOXT_ROWS_SUM" in err()
    assert red(T=BIG - 1, C=1 << 10, K=1 << 10) == 1 and b"svoxt_reduce_rows: T * C and M * K must be below 2^38" in err()
    assert red(M=BIG - 1, C=1, K=1 << 10, cols=p, n_cols=1) == 1 and b"svoxt_reduce_rows: T * C and M * K must be below 2^38" in err()
    for n_long, n_chunks in ((-1, 0), (9, 18), (3, 6)):
        assert red(n_long=n_long, n_chunks=n_chunks) == 1 and b"svoxt_reduce_rows: n_long must be in" in err()
    for n_long, n_chunks in ((2, 3), (2, 5), (0, 3)):
        assert red(n_long=n_long, n_chunks=n_chunks) == 1 and b"svoxt_reduce_rows: n_chunks must be in" in err()
    assert red(out=None) == 1 and b"svoxt_reduce_rows: out / row_ptr is NULL" in err()
    assert red(row_ptr=None) == 1 and b"svoxt_reduce_rows: out / row_ptr is NULL" in err()
    assert red(values=None) == 1 and b"svoxt_reduce_rows: values / perm is NULL" in err()
    assert red(perm=None) == 1 and b"svoxt_reduce_rows: values / perm is NULL" in err()
    for kw in (dict(lr=None), dict(lcp=None), dict(cl=None)):
        assert red(n_long=2, n_chunks=4, **kw) == 1 and b"svoxt_reduce_rows: long_rows / long_chunk_ptr / chunk_long is NULL" in err()
    for name in ("values", "row_ptr", "perm", "lr", "lcp", "cl", "out", "ws"):
        assert red(n_long=2, n_chunks=4, **{name: odd1}) == 1 and b"svoxt_reduce_rows: a misaligned argument" in err(), name
    assert red(cols=odd1, n_cols=4) == 1 and b"svoxt_reduce_rows: a misaligned argument" in err()
    need = lib.svoxt_reduce_rows_workspace_bytes(4, 4)
    assert red(n_long=2, n_chunks=4, ws=None, wsb=need) == 1 and b"svoxt_reduce_rows: workspace is NULL" in err()
    assert red(n_long=2, n_chunks=4, wsb=need - 1) == 1 and b"svoxt_reduce_rows: workspace smaller" in err()
    for empty in (float("nan"), float("inf"), -1.0):                   # `empty` may be anything: the next check is reached
        assert red(empty=empty, out=None) == 1 and b"out / row_ptr is NULL" in err()

    # the empty no-ops that touch no memory
    assert gather(None, 8, 4, None, 0, None, 0, None, None) == 0
    assert gather(None, 0, 4, None, 0, None, 0, None, None) == 0
    assert reduce(None, 0, 4, None, None, 0, None, None, None, 0, 0, None, 0, 4, 0, 0.0, None, None, 0, None) == 0
    assert reduce(None, 600, 4, None, None, 0, None, None, None, 0, 0, None, 0, 4, 2, -1.0, None, None, 0, None) == 0


def cpu_samples(T=6, Q=3):
    off = torch.tensor([0, 2, 2, T], dtype=torch.int64)[:Q + 1]
    return svox.RaySamples(off, torch.zeros(T, dtype=torch.int32), torch.zeros(T, dtype=torch.int32), torch.zeros(T), torch.ones(T))


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the Python layer's shape and dtype checks come before any launch."""
    is_cuda = True


def fake_gpu_samples(T=6):
    s = cpu_samples(T)
    s.offsets = s.offsets.as_subclass(_OnGpu)
    return s


def test_python_layer_checks_device_shapes_and_dtypes():
    s = cpu_samples()
    table = torch.ones(5, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        svox.gather_rows(s, table)
    with pytest.raises(RuntimeError, match="GPU"):
        svox.reduce_rows(s, torch.ones(6), 5)
    with pytest.raises(RuntimeError, match="GPU"):
        svox.reduce_rows(s, torch.ones(6, 3), 5, "max")
    with pytest.raises(RuntimeError, match="GPU"):
        s.row_plan(5)
    with pytest.raises(RuntimeError, match="samples must be a RaySamples"):
        svox.gather_rows((s.row,), table)
    with pytest.raises(RuntimeError, match="samples must be a RaySamples"):
        svox.reduce_rows(None, torch.ones(6), 5)
    for M in (-1, 1 << 31, 2.5, None, True):
        with pytest.raises(RuntimeError, match=r"M must be an int in \[0, 2\^31\)"):
            s.row_plan(M)

    g = fake_gpu_samples()
    gt = table.as_subclass(_OnGpu)
    for t in (torch.ones(5), torch.ones(5, 4, 1), torch.ones(5, 0), torch.ones(5, 4, dtype=torch.float64), torch.ones(5, 4, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match=r"table must be float32 \[M, K\]"):
            svox.gather_rows(g, t.as_subclass(_OnGpu))
    with pytest.raises(RuntimeError, match=r"table must be float32 \[M, K\]"):
        svox.gather_rows(g, None)
    for dim in (4, -5, [0, 4], torch.tensor([7])):
        with pytest.raises(RuntimeError, match="dim does not select columns"):
            svox.gather_rows(g, gt, dim=dim)
    for dim in ([1, 1], [0, -4], torch.tensor([2, 3, 2])):
        with pytest.raises(RuntimeError, match="dim selects a column twice"):
            svox.gather_rows(g, gt, dim=dim)
    for dim in ([], slice(2, 2)):
        with pytest.raises(RuntimeError, match="dim selects no column"):
            svox.gather_rows(g, gt, dim=dim)
    for v in (torch.ones(5), torch.ones(7, 2), torch.ones(6, 2, 1), torch.ones(6, 0), torch.ones(6, dtype=torch.float64),
              torch.ones(6, 2, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match=r"values must be float32 \[T\] or \[T, C\]"):
            svox.reduce_rows(g, v.as_subclass(_OnGpu), 5)
    with pytest.raises(RuntimeError, match=r"values must be float32 \[T\] or \[T, C\]"):
        svox.reduce_rows(g, None, 5)
    for op in ("amax", "prod", None, 0):
        with pytest.raises(RuntimeError, match="op must be one of"):
            svox.reduce_rows(g, torch.ones(6).as_subclass(_OnGpu), 5, op)
    for M in (-1, 1 << 31, 2.5):
        with pytest.raises(RuntimeError, match=r"M must be an int in \[0, 2\^31\)"):
            svox.reduce_rows(g, torch.ones(6).as_subclass(_OnGpu), M)

    # the marshalling layer: devices and contiguity
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.row_plan(s.row, 5)
    with pytest.raises(RuntimeError, match=r"row must be int32 \[T\]"):
        _C.row_plan(s.row.long(), 5)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.sample_gather_rows(table, s.row)
    with pytest.raises(RuntimeError, match=r"row must be int32 \[T\]"):
        _C.sample_gather_rows(table, s.row.long())
    with pytest.raises(RuntimeError, match=r"table must be float32 \[M, K\]"):
        _C.sample_gather_rows(table.double(), s.row)
    with pytest.raises(RuntimeError, match="plan must be a row plan"):
        _C.sample_reduce_rows(torch.ones(6, 2), None)

    tree = svox.N3Tree(N=2, data_dim=4, init_reserve=4)
    for bad in (torch.ones(3, 1), torch.ones(3, dtype=torch.float64), None):
        with pytest.raises(RuntimeError, match=r"per_row must be float32 \[M\]"):
            tree.spread_rows(bad)


def test_spread_rows_on_a_cpu_tree():
    """Torch ops only: the per-slot map of a fresh tree, whose root's 8 leaves all name row 0."""
    tree = svox.N3Tree(N=2, data_dim=4, init_reserve=4)
    out = tree.spread_rows(torch.tensor([0.75]), empty=-1.0)
    assert out.shape == tree.child.shape and out.dtype == torch.float32
    words = tree.data[..., 0].long()
    named = (tree.child == 0) & (words >= 0) & (words < 1)
    assert torch.equal(out[named], torch.full((int(named.sum()),), 0.75)) and torch.all(out[~named] == -1.0)
    assert torch.all(tree.spread_rows(torch.zeros(0), empty=2.0) == 2.0)


# ------------------------------------------------------------------------------------------ anchors of the restatement
def test_the_chunk_rule_is_two_level():
    """A 300-sample row, v_0 = 2^24 and 1.0 elsewhere: chunk 0 stays at 2^24 (2^24 + 1 rounds back, 255 times), chunk 1
    is 44 exactly, their sum 16 777 260 is a float32.  The plain sequential sum never leaves 2^24."""
    v = np.ones((300, 1), np.float32)
    v[0] = 2.0 ** 24
    row = np.zeros(300, np.int32)
    assert R.reduce(v, row, 1, "sum")[0, 0] == np.float32(16777260.0)
    assert R.sum_sequential(v)[0] == np.float32(16777216.0)
    # up to 256 samples the rule is the plain sequential sum
    rng = np.random.default_rng(1)
    w = rng.standard_normal((256, 3)).astype(np.float32)
    np.testing.assert_array_equal(R.reduce(w, np.zeros(256, np.int32), 1, "sum")[0], R.sum_sequential(w))


def test_plan_of_the_hand_made_rows():
    row, M, sizes = R.hand_made()
    P = R.plan(row, M)
    counts = np.diff(P.row_ptr)
    assert counts[0] == 0 and counts[8] == 0 and all(counts[r] == n for r, n in sizes.items())
    assert P.n_outside == 13 and P.longest == 1500 and P.row_ptr[0] == 0 and P.row_ptr[M] == 5000 - 13
    for r in (2, 7, 20):
        ks = P.perm[P.row_ptr[r]:P.row_ptr[r + 1]]
        assert np.all(np.diff(ks) > 0) and np.all(row[ks] == r)
    assert sorted(P.perm.tolist()) == list(range(5000))


def test_sum_is_within_the_standard_bound_of_float64():
    row, M, _ = R.hand_made()
    rng = np.random.default_rng(4)
    v = (rng.standard_normal((5000, 3)) * np.exp(rng.uniform(-3, 3, (5000, 3)))).astype(np.float32)
    got = R.reduce(v, row, M, "sum").astype(np.float64)
    inside = (row >= 0) & (row < M)
    want, mag = np.zeros((M, 3)), np.zeros((M, 3))
    np.add.at(want, row[inside], v[inside].astype(np.float64))
    np.add.at(mag, row[inside], np.abs(v[inside]).astype(np.float64))
    n = np.bincount(row[inside], minlength=M)[:, None]
    assert np.all(np.abs(got - want) <= R.gamma(n) * mag) and np.abs(got - want).max() > 0


def test_max_min_mean_and_empty():
    row, M, _ = R.hand_made()
    rng = np.random.default_rng(5)
    v = rng.standard_normal((5000, 2)).astype(np.float32)
    inside = (row >= 0) & (row < M)
    has = np.bincount(row[inside], minlength=M) > 0
    for op, at, start in (("max", np.maximum.at, -np.inf), ("min", np.minimum.at, np.inf)):
        want = np.full((M, 2), start, np.float32)
        at(want, row[inside], v[inside])
        got = R.reduce(v, row, M, op, empty=-1.0)
        np.testing.assert_array_equal(got[has], want[has])
        assert np.all(got[~has] == -1.0) and (~has).sum() == 2
    # a NaN makes its row NaN in that column, and no other
    v2 = v.copy()
    k = int(np.nonzero(row == 7)[0][700])
    v2[k, 1] = np.nan
    for op in ("max", "min", "sum", "mean"):
        got = R.reduce(v2, row, M, op)
        assert np.isnan(got[7, 1]) and np.isnan(got).sum() == 1
    # the mean of a row of equal values is that value: n * c is exact for these, and divides back
    c = np.full((5000, 1), 0.375, np.float32)
    got = R.reduce(c, row, M, "mean", empty=9.0)
    assert np.all(got[has] == np.float32(0.375)) and np.all(got[~has] == 9.0)
    # 1-D values give a 1-D result
    assert R.reduce(v[:, 0].copy(), row, M, "sum").shape == (M,)


def test_gather_and_its_gradient_restated():
    row, M, _ = R.hand_made()
    rng = np.random.default_rng(6)
    table = rng.standard_normal((M, 5)).astype(np.float32)
    out = R.gather(table, row, [4, 1])
    inside = (row >= 0) & (row < M)
    np.testing.assert_array_equal(out[inside], table[row[inside]][:, [4, 1]])
    assert not out[~inside].any()
    g = rng.standard_normal((5000, 2)).astype(np.float32)
    G = R.gather_grad(g, row, M, 5, [4, 1])
    assert G.shape == (M, 5) and not G[:, [0, 2, 3]].any() and not G[0].any() and G[7, 4] != 0
    np.testing.assert_array_equal(G[:, [4, 1]], R.reduce(g, row, M, "sum"))
