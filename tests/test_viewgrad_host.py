"""The gradient in the view direction without a GPU: the two restated float32 sequences (tests/viewgrad_restate.py) against
their float64 yardsticks within the derived bounds, the new symbols, and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd.csrc._abi import _COptions, _CRays
from tests import samples_restate as R
from tests import shade_restate as SR
from tests import test_gpu_rowgrad as TR
from tests import test_gpu_shade as TS
from tests import viewgrad_restate as V
from tests.test_rowgrad_host import specs

NAMES = ("svoxt_view_basis_bwd", "svoxt_shade_samples_bwd_basis")
_BUILT = {}


def scene(name):
    if name in TS.EXTRA and name not in TR._BUILT:
        TR._BUILT[name] = TS.EXTRA[name]()
    return TR.scene(name)


def extra_of(s):
    return None if s.lobes is None else s.lobes.numpy()


def view_batch(s):
    """66 view directions: the scene's first 65 and one with a zero component -- no multiple of a wavefront."""
    v = np.concatenate([s.rays[2][:65], np.array([[0.6, 0.0, -0.8]], np.float32)]).astype(np.float32)
    v[3, 2] = 0.0
    return np.ascontiguousarray(v)


def worst(got, want, bound):
    """max |got - want| / bound; where the bound is 0 both must be exactly 0."""
    got, want, bound = (np.asarray(a, dtype=np.float64) for a in (got, want, bound))
    zero = bound == 0
    assert not got[zero].any() and not want[zero].any()
    err = np.abs(got - want)
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def host_lists(name):
    """The scene's lists (min_sigma = 0), the forward's values and an upstream gradient, restated once."""
    if name not in _BUILT:
        s = scene(name)
        L = R.lists(s.ot, s.rays, s.opt, 0.0)
        basis = SR.basis(s.opt, s.rays[2], extra_of(s))
        fwd = {a: SR.forward(s.features.numpy(), L.row, L.ray, s.opt, basis, a)[0] for a in (True, False)}
        gv = np.random.default_rng(7).standard_normal((L.row.shape[0], s.C)).astype(np.float32)
        _BUILT[name] = (s, L, fwd, gv)
    return _BUILT[name]


# the restatements against the yardsticks -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n3_sh4", "sh9", "sh16", "sh25", "sg6", "asg6"])
def test_view_sequence_within_the_bound_of_float64(name):
    s = scene(name)
    v = view_batch(s)
    ex = extra_of(s)
    basis = O.basis(s.opt.format, s.opt.basis_dim, v, ex)
    g = np.random.default_rng(3).standard_normal(basis.shape).astype(np.float32)
    got = V.view_backward32(s.opt, v, ex, basis, g)
    want = V.view_grad64(s.opt, v, ex, g)
    bound = V.view_bound(s.opt, v, ex, g)
    tight = V.view_tight(s.opt, v, ex, g)
    r = worst(got, want, bound)
    print(f"{name}: worst |err| / bound = {r:.3f}; worst bound / tight = {(bound / np.maximum(tight, 1e-300)).max():.2e}")
    assert got.dtype == np.float32 and got.shape == (66, 3) and r <= 1
    assert np.count_nonzero(want) >= 3 * 60 and np.all(bound <= 1e-4 * tight)      # the comparison says something
    # the forward the yardstick differentiates is the forward: O.basis within a few ulp of its scale
    b64 = V.basis64(s.opt, torch.from_numpy(v).double(), ex).numpy()
    assert np.abs(b64 - basis).max() <= 1e-5 * max(1.0, np.abs(b64).max())
    # one component at a time: every column of the table on its own
    for i in range(s.opt.basis_dim):
        gi = np.zeros_like(g)
        gi[:, i] = g[:, i]
        assert worst(V.view_backward32(s.opt, v, ex, basis, gi), V.view_grad64(s.opt, v, ex, gi), V.view_bound(s.opt, v, ex, gi)) <= 1, i


def test_view_sequence_sh1_and_zero_direction():
    opt = O.make_options(format=O.FORMAT_SH, basis_dim=1)
    v = np.zeros((3, 3), np.float32)
    assert not V.view_backward32(opt, v, None, np.ones((3, 1), np.float32), np.ones((3, 1), np.float32)).any()
    opt9 = O.make_options(format=O.FORMAT_SH, basis_dim=9)
    g = np.ones((3, 9), np.float32)
    got = V.view_backward32(opt9, v, None, None, g)
    np.testing.assert_array_equal(got, np.tile(np.float32([-V.C1, -V.C1, V.C1]), (3, 1)))   # the linear components alone


@pytest.mark.parametrize("activate", [True, False])
@pytest.mark.parametrize("name", ["n3_sh4", "sh9", "sh16", "sh25", "sg6", "asg6", "sh4_sub", "sh4_c2"])
def test_basis_sequence_within_the_bound_of_float64(name, activate):
    s, L, fwd, gv = host_lists(name)
    args = (s.features.numpy(), L.offsets, L.row, L.ray, s.opt, fwd[activate], gv, activate)
    got = V.basis_backward32(*args)
    want = V.basis_grad64(*args)
    bound = V.basis_bound(*args)
    r = worst(got, want, bound)
    print(f"{name} activate={activate}: worst |err| / bound = {r:.3f}")
    assert got.dtype == np.float32 and got.shape == (s.Q, s.opt.basis_dim) and r <= 1 and np.count_nonzero(got) > 100
    outside = [i for i in range(s.opt.basis_dim) if not s.opt.min_comp <= i <= s.opt.max_comp]
    assert not got[:, outside].any() and not got[np.diff(L.offsets) == 0].any()
    if name == "sh4_sub":
        assert outside == [0, 3]
    assert not V.basis_backward32(*args[:6], None, activate).any()


def test_basis_sequence_skips_foreign_rays_and_rows_outside():
    s, L, fwd, gv = host_lists("sh9")
    row, ray = L.row.astype(np.int64).copy(), L.ray.copy()
    row[::5], row[1::7] = -1, s.ot.M
    ray[2::11] += 1
    args = (s.features.numpy(), L.offsets, row, ray, s.opt, fwd[True], gv, True)
    got, want = V.basis_backward32(*args), V.basis_grad64(*args)
    assert worst(got, want, V.basis_bound(*args)) <= 1
    keep = (row >= 0) & (row < s.ot.M) & (ray == L.ray)
    masked = gv * keep[:, None]
    np.testing.assert_array_equal(got, V.basis_backward32(s.features.numpy(), L.offsets, np.where(keep, row, 0), L.ray, s.opt, fwd[True], masked, True))


# symbols and checks ----------------------------------------------------------------------------------------------------
def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    header = open(_C.LIB_PATH.rsplit("/svox_t_amd/", 1)[0] + "/include/svoxt.h").read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS and n + "(" in header
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22            # entry points added, nothing changed
    assert callable(_C._extras.view_basis_backward) and callable(_C._extras.shade_samples_bwd_basis)
    assert callable(svox.VolumeRenderer.view_basis) and callable(svox.VolumeRenderer.shade_samples)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    err = lib.svoxt_last_error
    vbb, sbb = (getattr(lib, n) for n in NAMES)
    by = ctypes.byref
    t, r, o, p, _keep = specs()
    t28, _, o9, _, _ = specs(K=28, fmt=1, bd=9)
    odd1 = ctypes.c_void_p(p.value + 1)

    # view_basis_bwd: (tree, rays, opt, basis, grad_basis, grad_vdirs, stream)
    assert vbb(None, by(r), by(o9), p, p, p, None) == 1 and b"tree is NULL" in err()
    assert vbb(by(t28), None, by(o9), p, p, p, None) == 1 and b"rays is NULL" in err()
    assert vbb(by(t28), by(r), None, p, p, p, None) == 1 and b"options is NULL" in err()
    cam = _CRays(Q=64, image_width=8, image_height=8, c2w=p, fx=1.0, fy=1.0)
    assert vbb(by(t28), by(cam), by(o9), p, p, p, None) == 1 and b"camera mode has no viewdirs tensor" in err()
    assert vbb(by(specs(K=28, xform=True)[0]), by(r), by(o9), p, p, p, None) == 1 and b"transformation_matrices (tree.xform) are not served" in err()
    assert vbb(by(t28), by(r), by(_COptions(1e-3, 1.0, 1, 7, -1, -1, 0.0, 0, 6, 0.0, 0.0)), p, p, p, None) == 1 and b"SH basis_dim must be" in err()
    assert vbb(by(t28), by(r), by(o9), p, None, p, None) == 1 and b"grad_basis / grad_vdirs / basis (SG) is NULL" in err()
    assert vbb(by(t28), by(r), by(o9), p, p, None, None) == 1 and b"is NULL" in err()
    for args in ((odd1, p, p), (p, odd1, p), (p, p, odd1)):
        assert vbb(by(t28), by(r), by(o9), *args, None) == 1 and b"a misaligned argument" in err()
    assert vbb(by(t), by(r), by(o), None, None, None, None) == 0      # RGBA: no basis, no gradient, nothing launched
    assert vbb(by(t28), by(specs(Q=0)[1]), by(o9), None, None, None, None) == 0

    # shade_samples_bwd_basis: (features, M, K, opt, offsets, row, ray, T, Q, activate, values, grad_values, grad_basis, stream)
    def b(features=p, M=8, K=28, opt=o9, offsets=p, row=p, ray=p, T=600, Q=16, activate=1, values=p, gv=p, gb=p):
        return sbb(features, M, K, None if opt is None else by(opt), offsets, row, ray, T, Q, activate, values, gv, gb, None), err()

    def refused(res, text):
        assert res[0] == 1 and text in res[1], res

    refused(b(opt=None), b"options is NULL")
    refused(b(K=0), b"K must be >= 1")
    refused(b(T=1 << 31), b"T must be in [0, 2^31)")
    refused(b(M=-1), b"M must be in [0, 2^31)")
    refused(b(Q=-1), b"Q must be in [0, 2^31)")
    refused(b(opt=_COptions(1e-3, 1.0, 1, 26, -1, -1, 0.0, 0, 0, 0.0, 0.0)), b"basis_dim must be in [1, 25]")
    refused(b(opt=_COptions(1e-3, 1.0, 1, 9, -1, -1, 0.0, 0, 9, 0.0, 0.0)), b"min_comp / max_comp outside")
    refused(b(offsets=None), b"offsets / grad_basis is NULL")
    refused(b(gb=None), b"offsets / grad_basis is NULL")
    for name in ("row", "ray", "values", "features"):
        refused(b(**{name: None}), b"row / ray / values / features is NULL")
    for name in ("features", "offsets", "row", "ray", "values", "gv", "gb"):
        refused(b(**{name: odd1}), b"a misaligned argument")
    refused(b(offsets=ctypes.c_void_p(p.value + 4)), b"a misaligned argument")       # offsets are int64
    assert b(Q=0, T=0, offsets=None, row=None, ray=None, values=None, gv=None, gb=None)[0] == 0    # no ray, no sample: a no-op
    assert b(opt=o, K=4, offsets=None, gb=None)[0] == 0               # RGBA: no basis, no gradient, nothing launched
