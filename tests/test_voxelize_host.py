"""voxelize without a GPU: the public name, the C ABI's argument checks (all made before any HIP call, so they run
here) and the Python layer's refusals."""
import ctypes

import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C

INVALID = 1


def f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_voxelize_is_exported():
    assert callable(svox.voxelize)
    assert "voxelize" in svox.__all__
    from svox_t_amd.p2v import voxelize
    assert voxelize is svox.voxelize


FWD_OK = dict(points=1, feats=1, P=10, F=2, corner=f3(0, 0, 0), size=f3(1, 1, 1), n=8, kr=1.0, cr=0.5, voxels=1,
              ws=1, nbytes=1 << 40)
BAD = [("n", 1), ("n", 1025), ("n", -3), ("kr", 0.0), ("kr", -1.0), ("kr", float("nan")), ("cr", -0.1),
       ("cr", float("inf")), ("cr", float("nan")), ("P", -1), ("P", 1 << 31), ("F", 0), ("corner", None),
       ("size", None), ("size", f3(1, 0, 1)), ("size", f3(1, float("inf"), 1)), ("corner", f3(0, float("nan"), 0)),
       ("voxels", None), ("points", None), ("feats", None), ("ws", None), ("nbytes", 16)]


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v if not isinstance(v, ctypes.Array) else list(v)}" for f, v in BAD])
def test_forward_rejects_before_any_hip_call(field, value):
    a = dict(FWD_OK)
    a[field] = value
    rc = _C._lib.svoxt_p2v_fwd(a["points"], a["feats"], a["P"], a["F"], a["corner"], a["size"], a["n"], a["kr"], a["cr"],
                               a["voxels"], None, a["ws"], a["nbytes"], None)
    assert rc == INVALID, _C._lib.svoxt_last_error()
    assert b"svoxt_p2v_fwd" in _C._lib.svoxt_last_error()


BWD_BAD = [b for b in BAD if b[0] not in ("voxels", "ws", "nbytes")] + [("grad", None)]


@pytest.mark.parametrize("field,value", BWD_BAD, ids=[f"{f}={v if not isinstance(v, ctypes.Array) else list(v)}" for f, v in BWD_BAD])
def test_backward_rejects_before_any_hip_call(field, value):
    a = dict(FWD_OK, grad=1)
    a[field] = value
    rc = _C._lib.svoxt_p2v_bwd(a["grad"], a["points"], a["feats"], a["P"], a["F"], a["corner"], a["size"], a["n"],
                               a["kr"], a["cr"], None, 1, 1, None)
    assert rc == INVALID, _C._lib.svoxt_last_error()


def test_workspace_query():
    q = _C._lib.svoxt_p2v_workspace_bytes
    assert q(1000, 64, f3(0, 0, 0), f3(1, 1, 1), 0.05) > 0
    assert q(1000, 1, f3(0, 0, 0), f3(1, 1, 1), 0.05) == -1
    assert q(1000, 64, f3(0, 0, 0), None, 0.05) == -1
    assert q(1000, 64, None, f3(1, 1, 1), 0.05) == -1
    assert q(-1, 64, f3(0, 0, 0), f3(1, 1, 1), 0.05) == -1


@pytest.mark.parametrize("corner,radius_voxels", [(0.0, 3.49), (100.0, 3.49), (1000.0, 3.3), (-1000.0, 6.0)])
def test_forward_accepts_exactly_the_queried_workspace(corner, radius_voxels):
    """The query plans with the forward's arguments: a corner far from the origin widens the apron's rounding bound,
    and the forward must take the size the query gave for it (and refuse a byte less).  voxels = NULL makes the
    forward stop right after the workspace checks, before any HIP call."""
    P, n = 1000, 256
    cr = radius_voxels / (n - 1)
    c, s = f3(corner, corner, corner), f3(1, 1, 1)
    nbytes = _C._lib.svoxt_p2v_workspace_bytes(P, n, c, s, cr)
    assert nbytes > 0
    fwd = _C._lib.svoxt_p2v_fwd
    assert fwd(1, 1, P, 1, c, s, n, 1.0, cr, None, None, 1, nbytes, None) == INVALID
    assert b"voxels is NULL" in _C._lib.svoxt_last_error()          # past the workspace checks
    assert fwd(1, 1, P, 1, c, s, n, 1.0, cr, None, None, 1, nbytes - 1, None) == INVALID
    assert b"workspace too small" in _C._lib.svoxt_last_error()


def test_point_count_limit():
    """P up to 2^31 - 1 is served; only a radius that spans too many tiles for that many points is refused."""
    q, big = _C._lib.svoxt_p2v_workspace_bytes, (1 << 31) - 1
    cr = lambda v: v / 255.0                                       # noqa: E731
    assert q(big, 256, f3(0, 0, 0), f3(1, 1, 1), cr(3.0)) > 0
    assert q(big, 256, f3(0, 0, 0), f3(1, 1, 1), cr(30.0)) == -1
    assert _C._lib.svoxt_p2v_fwd(1, 1, big, 1, f3(0, 0, 0), f3(1, 1, 1), 256, 1.0, cr(30.0), None, None, None, 0, None) == 2
    assert b"too many tiles" in _C._lib.svoxt_last_error()


def test_python_layer_refuses_cpu_and_float64():
    pts, feats = torch.rand(5, 3), torch.rand(5, 1)
    for p, f in ((pts, feats), (pts.double(), feats.double())):
        with pytest.raises(RuntimeError):
            svox.voxelize(p, f, [0, 0, 0], [1, 1, 1], 8, 1.0, 0.5)
        with pytest.raises(RuntimeError):
            _C.p2v(p, f, [0, 0, 0], [1, 1, 1], 8, 1.0, 0.5)
        with pytest.raises(RuntimeError):
            _C.p2v_backward(torch.zeros(8, 8, 8, 1), p, f, [0, 0, 0], [1, 1, 1], 8, 1.0, 0.5)


def test_the_two_operators_are_no_longer_stubs():
    for name in ("p2v", "p2v_backward"):
        fn = getattr(_C, name)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor") as e:       # an argument error
            fn(*([torch.zeros(8, 8, 8, 1)] if name == "p2v_backward" else []), torch.rand(2, 3), torch.rand(2, 1),
               [0, 0, 0], [1, 1, 1], 8, 1.0, 0.5)
        assert not isinstance(e.value, NotImplementedError)          # (which subclasses RuntimeError)
