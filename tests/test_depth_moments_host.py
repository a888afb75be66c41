"""render_depth_moments without a GPU: the C ABI's argument checks, the operator layer's, and the three anchors that tie
the restatement (tests/depth_restate.py) to the C++ oracle."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import depth_restate as R
from tests.util import Case


@pytest.fixture(scope="module")
def case():
    return Case(depth=5, K=4, data_format="RGBA", width=48, height=48)


def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in ("svoxt_depth_moments_workspace_bytes", "svoxt_depth_moments_fwd", "svoxt_depth_moments_bwd"):
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    wb = _C._lib.svoxt_depth_moments_workspace_bytes
    assert wb(0, 8) == 0 and wb(64, 0) == 0 and wb(-1, 8) == -1 and wb(8, -1) == -1
    assert wb(65, 6) == 128 * (8 + 12 * 8)           # rays rounded up to 64, samples to 4: 8 bytes + 12 a sample


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    assert lib.svoxt_depth_moments_fwd(None, None, None, 0, None, None, 0, None) == 1
    assert b"tree is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_depth_moments_bwd(None, None, None, 0, None, None, 0, None, 0, None) == 1
    assert b"tree is NULL" in lib.svoxt_last_error()
    buf = (ctypes.c_float * 96)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    t = _C._CTree(features=p, M=1, K=4, N=2, data=p, child=p, n_internal=1, offset=p, scaling=p)
    o = _C._COptions(format=0, basis_dim=-1)
    assert lib.svoxt_depth_moments_fwd(ctypes.byref(t), None, ctypes.byref(o), 0, None, None, 0, None) == 1
    assert b"NULL" in lib.svoxt_last_error()
    r = _C._CRays(Q=64, origins=p, dirs=p, vdirs=p)
    for at in (2, -1):
        assert lib.svoxt_depth_moments_fwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), at, p, None, 0, None) == 1
        assert b"at must be" in lib.svoxt_last_error()
        assert lib.svoxt_depth_moments_bwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), at, p, p, 0, None, 0, None) == 1
        assert b"at must be" in lib.svoxt_last_error()
    assert lib.svoxt_depth_moments_fwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), 0, None, None, 0, None) == 1
    assert b"out is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_depth_moments_fwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), 0, p, None, 64, None) == 1
    assert b"workspace" in lib.svoxt_last_error()
    assert lib.svoxt_depth_moments_bwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), 0, None, p, 0, None, 0, None) == 1
    assert b"grad_out is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_depth_moments_bwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), 0, p, None, 0, None, 0, None) == 1
    assert b"grad is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_depth_moments_bwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), 0, p, p, 3, None, 0, None) == 1
    assert b"gstride" in lib.svoxt_last_error()
    # an empty batch is a valid no-op
    r0 = _C._CRays(Q=0)
    assert lib.svoxt_depth_moments_fwd(ctypes.byref(t), ctypes.byref(r0), ctypes.byref(o), 1, None, None, 0, None) == 0
    assert lib.svoxt_depth_moments_bwd(ctypes.byref(t), ctypes.byref(r0), ctypes.byref(o), 1, None, p, 0, None, 0, None) == 0


def test_operator_layer_checks_at_and_grad_output_shape():
    tree = svox.N3Tree(N=2, data_dim=4, init_reserve=4)
    r = svox.VolumeRenderer(tree)
    rays = svox.Rays(torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        r.render_depth_moments(tree.features, rays)                # tree not on a GPU
    with pytest.raises(RuntimeError, match="GPU"):
        r.render_depth_moments(tree.features, rays, cuda=False)
    with pytest.raises(RuntimeError, match="GPU"):
        r.render_expected_depth(tree.features, rays, cuda=False)
    spec, rspec, opt = tree._spec(tree.features), svox.renderer._rays_spec_from_rays(rays), r._get_options()
    for bad in ("exit", 2, None, True):
        with pytest.raises(RuntimeError, match="at must be"):
            _C.depth_moments(spec, rspec, opt, at=bad)
        with pytest.raises(RuntimeError, match="at must be"):
            _C.depth_moments_backward(spec, rspec, opt, torch.zeros(4, 3), at=bad)
    for g in (torch.zeros(4, 1), torch.zeros(4, 4), torch.zeros(5, 3), torch.zeros(12), torch.zeros(4, 3, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match=r"grad_output must be float32 \[Q, 3\]"):
            _C.depth_moments_backward(spec, rspec, opt, g)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.depth_moments_backward(spec, rspec, opt, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.depth_moments(spec, rspec, opt)


@pytest.mark.parametrize("fast", [False, True])
def test_restatement_alpha_is_the_oracles_opacity(case, fast):
    """The float32 restatement runs the oracle's product sequence T *= expf(-delta_t * delta_scale * sigma) over the same
    leaves.  The comparison that holds is the exact one: bit for bit."""
    opt = case.oracle_opts(fast=fast)
    got = R.moments(case.oracle_tree(), case.rays_np(), opt, "entry", torch.float32).numpy()
    want = O.opacity_render(case.oracle_tree(), *case.rays_np(), opt)
    np.testing.assert_array_equal(got[:, 2:3], want)
    assert (want > 0).sum() > 100


def test_restatement_opaque_depth_is_the_oracles_render_depth(case):
    """sigma = 1e6 everywhere: att == 0 at the first sample with sigma > 0, so w = 1 there and 0 behind it:
    m1 = z of that sample -- what render_depth reports -- and m2 = m1 * m1, exactly."""
    ot = case.oracle_tree()
    feats = ot.features.copy()
    feats[:, -1] = 1e6
    ot = O.Tree(feats, case.st.data, case.st.child, offset=ot.offset, scaling=ot.scaling)
    opt = case.oracle_opts()
    got = R.moments(ot, case.rays_np(), opt, "entry", torch.float32).numpy()
    want = O.render_depth(ot, *case.rays_np(), opt)
    np.testing.assert_array_equal(got[:, 0:1], want)
    np.testing.assert_array_equal(got[:, 1], got[:, 0] * got[:, 0])
    assert (want > 0).sum() > 100


@pytest.mark.parametrize("at", ["entry", "mid"])
def test_restatement_gradient_against_finite_differences(case, at):
    ot, rays, opt = case.oracle_tree(), case.rays_np(), case.oracle_opts()
    rng = np.random.default_rng(7)
    g = rng.standard_normal((case.Q, 3))
    grad = R.moments_grad(ot, rays, opt, at, g)
    assert np.all(grad[:, :-1] == 0)
    touched = np.nonzero((grad[:, -1] != 0) & (ot.features[:, -1] > 1.0))[0]
    assert touched.size > 100
    gt = torch.from_numpy(g)
    base = torch.from_numpy(ot.features).double()

    def loss(feats):
        return float((R.moments(ot, rays, opt, at, torch.float64, features=feats, early_stop=False) * gt).sum())

    for row in rng.choice(touched, size=20, replace=False):
        h = 1e-4 * float(base[row, -1])
        fp, fm = base.clone(), base.clone()
        fp[row, -1] += h
        fm[row, -1] -= h
        fd = (loss(fp) - loss(fm)) / (2 * h)
        # central differences in float64: truncation ~ h^2 f''' and cancellation ~ 1e-16 |loss| / h, both far below 1e-5
        # of the gradient's own addends
        scale = abs(grad[row, -1]) + 1e-6 * abs(grad[:, -1]).max()
        assert abs(fd - grad[row, -1]) <= 1e-5 * scale + 1e-9, (row, fd, grad[row, -1])


def test_restatement_alpha_gradient_is_the_oracles_opacity_backward(case):
    """grad_output (0, 0, ga): the gradient of alpha alone -- O.volume_render_backward with a one-column grad_output."""
    ot, rays, opt = case.oracle_tree(), case.rays_np(), case.oracle_opts()
    rng = np.random.default_rng(3)
    g = np.zeros((case.Q, 3))
    g[:, 2] = rng.standard_normal(case.Q)
    want, _, tight = O.volume_render_backward(ot, *rays, opt, g[:, 2:3].astype(np.float32), want_abs="both")
    got = R.moments_grad(ot, rays, opt, "entry", g[:, 2:3].astype(np.float32).astype(np.float64) * [[0, 0, 1]])
    from tests.util import assert_grads_close
    assert_grads_close(got, want, tight)
    scale = R.moments_grad_scale(ot, rays, opt, "entry", g.astype(np.float32))
    assert np.all((scale == 0) == (tight == 0))          # the same entries are touched
