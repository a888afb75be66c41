"""quantize_median_cut without a GPU: the numpy restatement the GPU tests compare with (tests/quantize_restate.py)
against the outputs of the reference's own quantizer recorded in tests/golden/quantize_*.npz; the new names and the
ABI number; the argument checks of the C ABI (all made before any HIP call, so they run here) and of the Python layer."""
import glob
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import quantize_restate as R

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "quantize_*.npz")))
INVALID = 1


def check_against_fixture(g, colors, ids):
    """The criteria the CPU restatement and the GPU result are both held to: color_id_map exactly the reference's;
    every colour entry of a non-empty segment within the float32 sequential-sum bound of the reference's own
    accumulation, (n + 2) 2^-24 sum|w x| / sum w, computed from the fixture's inputs; the rows the reference leaves
    NaN are exactly the empty segments' and are zero here, as every row past the last segment."""
    data, weights, order = g["data"], g["weights"], int(g["order"])
    report = {}
    _, _, _, starts, perm = R.quantize(data, weights, order, report)
    assert report["unique"]                                    # the condition under which the comparison may be exact
    np.testing.assert_array_equal(ids, g["color_id_map"])
    S = len(starts) - 1
    lens = np.diff(starts)
    bound = R.reference_bound(data, weights, starts, perm)
    ref = g["colors"].astype(np.float64)
    got = np.asarray(colors, np.float64)
    assert got.shape == ref.shape == (1 << order, data.shape[1])
    live = lens > 0
    err = np.abs(got[:S][live] - ref[:S][live])
    print(f"max err / bound = {(err / np.maximum(bound[live], 1e-300)).max():.3f}")
    assert (err <= bound[live]).all()
    assert np.isnan(ref[:S][~live]).all() and not np.isnan(ref[:S][live]).any()
    assert (got[:S][~live] == 0).all() and (got[S:] == 0).all() and (ref[S:] == 0).all()


def test_the_fixture_set():
    assert len(FIXTURES) == 4
    shapes = {n: np.load(os.path.join(G, n))["data"].shape for n in FIXTURES}
    assert all(s[0] <= 1024 for s in shapes.values()) and (1000, 28) in shapes.values()
    g = np.load(os.path.join(G, "quantize_unweighted_full.npz"))
    assert g["data"].shape[0] == 1 << int(g["order"])
    g = np.load(os.path.join(G, "quantize_weighted_dominant.npz"))
    assert np.isnan(g["colors"]).any() and len(np.unique(g["color_id_map"])) < (1 << int(g["order"])) - 2


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference(name):
    g = np.load(os.path.join(G, name))
    colors, ids, *_ = R.quantize(g["data"], g["weights"], int(g["order"]))
    check_against_fixture(g, colors, ids)


def test_restatement_by_hand():
    # one column: the cut is the middle of the sorted rows; ties go by row index; -0.0 sorts with +0.0
    data = np.array([[3.0], [-0.0], [0.0], [1.0], [0.0], [2.0]], np.float32)
    colors, ids, *_ = R.quantize(data, None, 1)
    np.testing.assert_array_equal(ids, [1, 0, 0, 1, 0, 1])
    np.testing.assert_array_equal(colors, [[0.0], [2.0]])
    # weighted: the first prefix above half the total; a row that outweighs the rest and sorts first leaves an empty child
    w = np.array([1, 1, 1, 1, 1, 9], np.float32)
    colors, ids, _, starts, _ = R.quantize(data, w, 2)
    np.testing.assert_array_equal(starts, [0, 2, 4, 4, 6])                     # [-0, 0 | 0, 1 || (empty) | 2, 3]
    np.testing.assert_array_equal(ids, [3, 0, 0, 1, 1, 3])
    np.testing.assert_array_equal(colors, [[0.0], [0.5], [0.0], [np.float32((18 + 3) / 10)]])
    # weights that sum to zero: the cut is at r (no prefix is above 0), the colour is the plain mean
    colors, ids, _, starts, _ = R.quantize(data, np.zeros(6, np.float32), 1)
    np.testing.assert_array_equal(starts, [0, 6, 6])
    np.testing.assert_array_equal(colors, [[1.0], [0.0]])


def test_names_and_abi():
    for name in ("svoxt_quantize_workspace_bytes", "svoxt_quantize_median_cut", "svoxt_remap_index"):
        assert name in _C.EXPORTS and hasattr(_C._lib, name)
    assert _C.ABI_VERSION == 22 and _C._lib.svoxt_abi_version() == 22
    assert callable(svox.quantize_median_cut) and callable(svox.N3Tree.quantize)
    assert "quantize_median_cut" in svox.__all__


OK = dict(data=1, M=5000, K=28, weights=None, order=8, colors=1, ids=1, ws=1, nbytes=1 << 40)
BAD = [("data", None), ("M", 255), ("M", 0), ("M", 1 << 31), ("K", 0), ("order", -1), ("order", 17), ("colors", None),
       ("ids", None), ("ws", None), ("nbytes", 64)]


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v}" for f, v in BAD])
def test_c_abi_rejects_before_any_hip_call(field, value):
    a = dict(OK)
    a[field] = value
    rc = _C._lib.svoxt_quantize_median_cut(a["data"], a["M"], a["K"], a["weights"], a["order"], a["colors"], a["ids"],
                                           a["ws"], a["nbytes"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_quantize_median_cut" in _C._lib.svoxt_last_error()


def test_workspace_query_and_remap_checks():
    q = _C._lib.svoxt_quantize_workspace_bytes
    assert q(5000, 28, 8, 0) >= 5 * 4 * 5000 and q(5000, 28, 8, 1) >= q(5000, 28, 8, 0) + 8 * 5000
    assert q(255, 28, 8, 0) == -1 and q(5000, 0, 8, 0) == -1 and q(1 << 20, 4, 17, 0) == -1 and q(1 << 31, 4, 2, 0) == -1
    lib = _C._lib
    # exactly the queried size passes the workspace check
    assert lib.svoxt_quantize_median_cut(1, 5000, 28, None, 8, 1, 1, 1, q(5000, 28, 8, 0) - 1, None) == INVALID
    assert b"workspace too small" in lib.svoxt_last_error()
    r = lib.svoxt_remap_index
    assert r(None, None, 0, None, 5, None) == 0                          # nothing to do
    assert r(None, 1, 8, 1, 5, None) == INVALID and r(1, None, 8, 1, 5, None) == INVALID
    assert r(1, 1, 8, None, 5, None) == INVALID and r(1, 1, -1, 1, 5, None) == INVALID and r(1, 1, 8, 1, -1, None) == INVALID


def test_python_layer_checks_fire_without_a_gpu():
    data = torch.zeros(300, 4)
    cases = [((data, None, 2), "CUDA"),                                  # a CPU tensor
             ((data.double(), None, 2), "float32"), ((data[:, 0], None, 2), "2-D"), ((data, None, 17), "order"),
             ((data, None, -1), "order"), ((data, None, 2.0), "order"), ((data, None, 9), "at least"),
             ((data, torch.ones(299), 2), "one entry per row"), ((data, torch.ones(300, dtype=torch.float64), 2), "weights"),
             ((data, torch.ones(300, 1), 2), "weights"), ((data[:, :0], None, 2), "column"),
             ((data, torch.ones(300), 2), "CUDA"), ((data.T, None, 2), "CUDA")]
    for args, match in cases:
        with pytest.raises(RuntimeError, match=match) as e:
            _C.quantize_median_cut(*args)
        assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="CUDA"):
        svox.quantize_median_cut(data, 2, weights=torch.empty(0))
    with pytest.raises(RuntimeError, match="int32"):
        _C.remap_index(torch.zeros(4), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDA"):
        _C.remap_index(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=1)
    with pytest.raises(RuntimeError, match="GPU"):
        tree.quantize(2)
    with tree.accumulate_weights():
        with pytest.raises(RuntimeError, match="Tree locked"):
            tree.quantize(2)
    for name in ("assign_vertical", "calc_corners"):                     # still outside the scope
        with pytest.raises(NotImplementedError):
            getattr(_C, name)()
