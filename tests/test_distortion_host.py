"""render_distortion without a GPU: the C ABI's argument checks, the operator layer's, and the anchors that tie the
restatement (tests/distortion_restate.py) to the C++ oracle and to the loss's pairwise definition."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import distortion_restate as R
from tests.depth_restate import march
from tests.util import Case, assert_grads_close


@pytest.fixture(scope="module")
def case():
    return Case(depth=5, K=4, data_format="RGBA", width=48, height=48)


def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in ("svoxt_distortion_workspace_bytes", "svoxt_distortion_fwd", "svoxt_distortion_bwd"):
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    wb = _C._lib.svoxt_distortion_workspace_bytes
    assert wb(0, 8) == 0 and wb(64, 0) == 0 and wb(-1, 8) == -1 and wb(8, -1) == -1
    assert wb(65, 6) == 128 * (8 + 12 * 8)           # rays rounded up to 64, samples to 4: 8 bytes + 12 a sample
    assert wb(65, 6) == _C._lib.svoxt_depth_moments_workspace_bytes(65, 6)
    assert _C._extras.DISTORTION_SAMPLES == 128


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    assert lib.svoxt_distortion_fwd(None, None, None, None, None, 0, None) == 1
    assert b"tree is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_distortion_bwd(None, None, None, None, None, 0, None, 0, None) == 1
    assert b"tree is NULL" in lib.svoxt_last_error()
    buf = (ctypes.c_float * 96)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd = ctypes.c_void_p(p.value + 4)
    t = _C._CTree(features=p, M=1, K=4, N=2, data=p, child=p, n_internal=1, offset=p, scaling=p)
    o = _C._COptions(format=0, basis_dim=-1)
    r = _C._CRays(Q=64, origins=p, dirs=p, vdirs=p)
    T, Rr, Op = ctypes.byref(t), ctypes.byref(r), ctypes.byref(o)
    for args in ((T, None, Op), (T, Rr, None)):
        assert lib.svoxt_distortion_fwd(*args, p, None, 0, None) == 1
        assert b"NULL" in lib.svoxt_last_error()
        assert lib.svoxt_distortion_bwd(*args, p, p, 0, None, 0, None) == 1
        assert b"NULL" in lib.svoxt_last_error()
    assert lib.svoxt_distortion_fwd(T, Rr, Op, None, None, 0, None) == 1
    assert b"out is NULL" in lib.svoxt_last_error()
    # workspace: NULL with a size, a negative size, not 8-byte aligned
    for ws, nbytes in ((None, 64), (p, -8), (odd, 4096)):
        assert lib.svoxt_distortion_fwd(T, Rr, Op, p, ws, nbytes, None) == 1
        assert b"svoxt_distortion_fwd: workspace" in lib.svoxt_last_error()
        assert lib.svoxt_distortion_bwd(T, Rr, Op, p, p, 0, ws, nbytes, None) == 1
        assert b"svoxt_distortion_bwd: workspace" in lib.svoxt_last_error()
    many = _C._CRays(Q=0x7fffffff * 64 + 1, origins=p, dirs=p, vdirs=p)
    assert lib.svoxt_distortion_fwd(T, ctypes.byref(many), Op, p, None, 0, None) == 1
    assert b"too many rays" in lib.svoxt_last_error()
    assert lib.svoxt_distortion_bwd(T, ctypes.byref(many), Op, p, p, 0, None, 0, None) == 1
    assert b"too many rays" in lib.svoxt_last_error()
    assert lib.svoxt_distortion_bwd(T, Rr, Op, None, p, 0, None, 0, None) == 1
    assert b"grad_out is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_distortion_bwd(T, Rr, Op, p, None, 0, None, 0, None) == 1
    assert b"grad is NULL" in lib.svoxt_last_error()
    assert lib.svoxt_distortion_bwd(T, Rr, Op, p, p, 3, None, 0, None) == 1
    assert b"gstride" in lib.svoxt_last_error()
    # an empty batch is a valid no-op
    r0 = _C._CRays(Q=0)
    assert lib.svoxt_distortion_fwd(T, ctypes.byref(r0), Op, None, None, 0, None) == 0
    assert lib.svoxt_distortion_bwd(T, ctypes.byref(r0), Op, None, p, 0, None, 0, None) == 0


def test_operator_layer_checks_device_and_grad_output_shape():
    tree = svox.N3Tree(N=2, data_dim=4, init_reserve=4)
    r = svox.VolumeRenderer(tree)
    rays = svox.Rays(torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        r.render_distortion(tree.features, rays)                   # tree not on a GPU
    with pytest.raises(RuntimeError, match="GPU"):
        r.render_distortion(tree.features, rays, cuda=False)
    with pytest.raises(RuntimeError, match="GPU"):
        r.distortion_loss(tree.features, rays, cuda=False)
    with pytest.raises(ValueError, match="reduction must be"):
        r.distortion_loss(tree.features, rays, reduction="max")
    spec, rspec, opt = tree._spec(tree.features), svox.renderer._rays_spec_from_rays(rays), r._get_options()
    for g in (torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(5, 2), torch.zeros(8), torch.zeros(4, 2, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match=r"grad_output must be float32 \[Q, 2\]"):
            _C.distortion_backward(spec, rspec, opt, g)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.distortion_backward(spec, rspec, opt, torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.distortion(spec, rspec, opt)


@pytest.mark.parametrize("fast", [False, True])
def test_restatement_alpha_is_the_oracles_opacity(case, fast):
    """The float32 restatement runs the oracle's product sequence T *= expf(-delta_t * delta_scale * sigma) over the same
    leaves.  The comparison that holds is the exact one: bit for bit."""
    opt = case.oracle_opts(fast=fast)
    got = R.distortion(case.oracle_tree(), case.rays_np(), opt, torch.float32).numpy()
    want = O.opacity_render(case.oracle_tree(), *case.rays_np(), opt)
    np.testing.assert_array_equal(got[:, 1:2], want)
    assert (want > 0).sum() > 100 and (got[:, 0] > 0).sum() > 100 and np.all(got[got[:, 1] == 0] == 0)


def test_restatement_alpha_gradient_is_the_oracles_opacity_backward(case):
    """grad_output (0, ga): the gradient of alpha alone -- O.volume_render_backward with a one-column grad_output."""
    ot, rays, opt = case.oracle_tree(), case.rays_np(), case.oracle_opts()
    rng = np.random.default_rng(3)
    g = np.zeros((case.Q, 2), dtype=np.float32)
    g[:, 1] = rng.standard_normal(case.Q)
    want, _, tight = O.volume_render_backward(ot, *rays, opt, g[:, 1:2].copy(), want_abs="both")
    got = R.distortion_grad(ot, rays, opt, g.astype(np.float64))
    assert_grads_close(got, want, tight)
    scale = R.distortion_grad_scale(ot, rays, opt, g)
    assert np.all((scale == 0) == (tight == 0))          # the same entries are touched


def pairwise(w, s, d):
    return float((w[:, None] * w[None, :] * np.abs(s[:, None] - s[None, :])).sum() + (w * w * d).sum() / 3.0)


def test_restatement_recurrence_is_the_pairwise_definition(case):
    """L = sum_ij w_i w_j |s_i - s_j| + 1/3 sum_i w_i^2 d_i, the O(n^2) sum over a ray's samples, in float64: the O(n)
    recurrence reorders exact-arithmetic identities only, so the two agree to float64 rounding."""
    ot, rays, opt = case.oracle_tree(), case.rays_np(), case.oracle_opts()
    got = R.distortion(ot, rays, opt, torch.float64).numpy()[:, 0]
    samples = R.ray_samples(ot, rays, opt)
    want = np.array([pairwise(*smp) for smp in samples])
    assert max(len(smp[0]) for smp in samples) > 8 and (want > 0).sum() > 100
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-18)
    # the float32 sequence stays within the output bound of the float64 one
    from tests.util import assert_outputs_close
    assert_outputs_close(R.distortion(ot, rays, opt, torch.float32).numpy(), R.distortion(ot, rays, opt, torch.float64).numpy())


def test_restatement_gradient_against_finite_differences(case):
    ot, rays, opt = case.oracle_tree(), case.rays_np(), case.oracle_opts()
    rng = np.random.default_rng(7)
    g = rng.standard_normal((case.Q, 2))
    grad = R.distortion_grad(ot, rays, opt, g)
    assert np.all(grad[:, :-1] == 0)
    touched = np.nonzero((grad[:, -1] != 0) & (ot.features[:, -1] > 1.0))[0]
    assert touched.size > 100
    gt = torch.from_numpy(g)
    base = torch.from_numpy(ot.features).double()

    def loss(feats):
        return float((R.distortion(ot, rays, opt, torch.float64, features=feats, early_stop=False) * gt).sum())

    for row in rng.choice(touched, size=10, replace=False):
        h = 1e-4 * float(base[row, -1])
        fp, fm = base.clone(), base.clone()
        fp[row, -1] += h
        fm[row, -1] -= h
        fd = (loss(fp) - loss(fm)) / (2 * h)
        # central differences in float64: truncation ~ h^2 f''' and cancellation ~ 1e-16 |loss| / h, both far below 1e-5
        # of the gradient's own addends
        scale = abs(grad[row, -1]) + 1e-6 * abs(grad[:, -1]).max()
        assert abs(fd - grad[row, -1]) <= 1e-5 * scale + 1e-9, (row, fd, grad[row, -1])


def test_a_constant_shift_of_s_changes_nothing(case):
    """L depends on differences of s only."""
    ot, rays, opt = case.oracle_tree(), case.rays_np(), case.oracle_opts(fast=True)
    a = R.distortion(ot, rays, opt, torch.float64).numpy()
    b = R.distortion(ot, rays, opt, torch.float64, shift=3.25).numpy()
    np.testing.assert_array_equal(a[:, 1], b[:, 1])
    # (s + c) - (s' + c) rounds at the size of s + c: a few 1e-16 relative to the differences of neighbours
    np.testing.assert_allclose(a[:, 0], b[:, 0], rtol=1e-10, atol=1e-18)
    assert (a[:, 0] > 0).sum() > 100


def test_a_ray_with_one_sample_gives_its_self_term(case):
    """One sample: no pair, L = w^2 d / 3 -- exactly, in the float32 sequence ((w * w) * d) * (1 / 3)."""
    ot0 = case.oracle_tree()
    rays, opt = case.rays_np(), case.oracle_opts()
    m = march(ot0, rays, opt)
    # the leaf most rays cross first
    rows = torch.cat([row for _, _, _, row in m.steps[:4]])
    keep = int(torch.mode(rows).values)
    feats = ot0.features.copy()
    sig = feats[keep, -1] if feats[keep, -1] > 0 else np.float32(7.0)
    feats[:, -1] = 0
    feats[keep, -1] = sig
    ot = O.Tree(feats, case.st.data, case.st.child, offset=ot0.offset, scaling=ot0.scaling)
    got = R.distortion(ot, rays, opt, torch.float32).numpy()
    want = np.zeros(case.Q, dtype=np.float32)
    count = np.zeros(case.Q, dtype=np.int64)
    for ids, t, delta_t, row in march(ot, rays, opt).steps:
        hit = row == keep
        a = ids[hit].numpy()
        d = (delta_t[hit] * m.delta_scale[ids[hit]]).numpy()
        w = got[a, 1]                                    # T = 1: w = 1 - att = alpha
        want[a] = ((w * w) * d) * (np.float32(1) / np.float32(3))
        count[a] += 1
    assert count.max() == 1 and (count == 1).sum() >= 4 and np.all(want[count == 1] > 0)
    np.testing.assert_array_equal(got[:, 0], want)
    got64 = R.distortion(ot, rays, opt, torch.float64).numpy()
    one = count == 1
    samples = R.ray_samples(ot, rays, opt)
    for q in np.nonzero(one)[0][:16]:
        w, s, d = samples[q]
        assert w.size == 1 and abs(got64[q, 0] - w[0] * w[0] * d[0] / 3.0) <= 1e-15 * got64[q, 0]
