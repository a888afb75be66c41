"""shade_samples without a GPU: the C ABI's symbols and argument checks, the Python layer's refusals, and the anchor of the
restatement (tests/shade_restate.py) -- its gradient is a float64 autograd formula's."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd.csrc._abi import _COptions
from tests import shade_restate as SR
from tests.test_rowgrad_host import specs
from tests.util import assert_grads_close

NAMES = ("svoxt_view_basis", "svoxt_shade_samples_fwd", "svoxt_shade_samples_bwd_workspace_bytes", "svoxt_shade_samples_bwd")
BIG = 1 << 31


def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    header = open(_C.LIB_PATH.rsplit("/svox_t_amd/", 1)[0] + "/include/svoxt.h").read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS and n + "(" in header
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22            # entry points added, nothing changed
    assert callable(_C.view_basis) and callable(_C.shade_samples_fwd) and callable(_C.shade_samples_bwd)
    assert callable(svox.VolumeRenderer.view_basis) and callable(svox.VolumeRenderer.shade_samples)
    assert callable(svox.shade_samples) and "shade_samples" in svox.__all__


def test_workspace_query():
    q = _C._lib.svoxt_shade_samples_bwd_workspace_bytes
    assert q(0, 28) == 0                                               # no long row: no workspace
    for args in ((-1, 4), (BIG, 4), (5, 0), (5, -1), (BIG - 1, 1 << 10)):
        assert q(*args) == -1, args
    for n_chunks, K in ((1, 1), (2, 4), (1000, 28), (46000, 32)):
        b = q(n_chunks, K)
        assert b % 256 == 0 and 4 * n_chunks * K <= b < 4 * n_chunks * K + 256      # the partials, one carved piece


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    err = lib.svoxt_last_error
    vb, fwd, _q, bwd = (getattr(lib, n) for n in NAMES)
    by = ctypes.byref
    t, r, o, p, _keep = specs()
    t28, _, o9, _, _ = specs(K=28, fmt=1, bd=9)
    odd1 = ctypes.c_void_p(p.value + 1)

    # view_basis
    assert vb(None, by(r), by(o), p, None) == 1 and b"tree is NULL" in err()
    assert vb(by(t), None, by(o), p, None) == 1 and b"rays is NULL" in err()
    assert vb(by(t), by(r), None, p, None) == 1 and b"options is NULL" in err()
    assert vb(by(specs(xform=True)[0]), by(r), by(o), p, None) == 1 and b"transformation_matrices (tree.xform) are not served" in err()
    assert vb(by(t28), by(specs(Q=-1)[1]), by(o9), p, None) == 1 and b"negative ray count" in err()
    assert vb(by(t28), by(r), by(_COptions(1e-3, 1.0, 1, 7, -1, -1, 0.0, 0, 6, 0.0, 0.0)), p, None) == 1 and b"SH basis_dim must be" in err()
    assert vb(by(t28), by(r), by(o9), None, None) == 1 and b"basis is NULL or not 4-byte aligned" in err()
    assert vb(by(t28), by(r), by(o9), odd1, None) == 1 and b"basis is NULL or not 4-byte aligned" in err()
    assert vb(by(t), by(r), by(o), None, None) == 0                    # RGBA: [Q, 0], nothing to write, nothing launched
    assert vb(by(t28), by(specs(Q=0)[1]), by(o9), None, None) == 0

    # the forward: (features, M, K, opt, row, ray, T, basis, Q, activate, values, sigma, stream)
    def f(features=p, M=8, K=28, opt=o9, row=p, ray=p, T=600, basis=p, Q=16, values=p, sigma=p):
        return fwd(features, M, K, None if opt is None else by(opt), row, ray, T, basis, Q, 1, values, sigma, None), err()

    def refused(res, text):
        assert res[0] == 1 and text in res[1], res

    refused(f(opt=None), b"options is NULL")
    refused(f(opt=_COptions(1e-3, 1.0, 4, 9, -1, -1, 0.0, 0, 8, 0.0, 0.0)), b"unknown data format")
    refused(f(K=0), b"K must be >= 1")
    for T in (-1, BIG):
        refused(f(T=T), b"T must be in [0, 2^31)")
    for M in (-1, BIG):
        refused(f(M=M), b"M must be in [0, 2^31)")
    for Q in (-1, BIG):
        refused(f(Q=Q), b"Q must be in [0, 2^31)")
    for bd in (0, 26):
        refused(f(opt=_COptions(1e-3, 1.0, 1, bd, -1, -1, 0.0, 0, 0, 0.0, 0.0)), b"basis_dim must be in [1, 25]")
    refused(f(opt=_COptions(1e-3, 1.0, 1, 9, -1, -1, 0.0, -1, 8, 0.0, 0.0)), b"min_comp / max_comp outside")
    refused(f(opt=_COptions(1e-3, 1.0, 1, 9, -1, -1, 0.0, 0, 9, 0.0, 0.0)), b"min_comp / max_comp outside")
    refused(f(K=1 << 10, opt=o, T=BIG - 1), b"must be below 2^38")
    refused(f(K=1 << 10, M=BIG - 1), b"must be below 2^38")
    assert f(T=0, row=None, values=None, sigma=None)[0] == 0           # no sample: a no-op
    refused(f(row=None), b"row / values / sigma is NULL")
    refused(f(values=None), b"row / values / sigma is NULL")
    refused(f(sigma=None), b"row / values / sigma is NULL")
    refused(f(features=None), b"features is NULL")
    refused(f(ray=None), b"ray / basis is NULL")
    refused(f(basis=None), b"ray / basis is NULL")
    for name in ("features", "row", "ray", "basis", "values", "sigma"):
        refused(f(**{name: odd1}), b"a misaligned argument")

    # the backward: (opt, M, K, ray, T, basis, Q, activate, values, grad_values, grad_sigma, row_ptr, perm, long_rows,
    # long_chunk_ptr, chunk_long, n_long, n_chunks, grad, workspace, workspace_bytes, stream)
    def b(opt=o9, M=8, K=28, ray=p, T=600, basis=p, Q=16, activate=1, values=p, gv=p, gs=p, row_ptr=p, perm=p, long_rows=p,
          long_chunk_ptr=p, chunk_long=p, n_long=0, n_chunks=0, grad=p, ws=p, wsb=1 << 40):
        return bwd(None if opt is None else by(opt), M, K, ray, T, basis, Q, activate, values, gv, gs, row_ptr, perm, long_rows,
                   long_chunk_ptr, chunk_long, n_long, n_chunks, grad, ws, wsb, None), err()

    refused(b(opt=None), b"options is NULL")
    refused(b(K=0), b"K must be >= 1")
    refused(b(T=BIG), b"T must be in [0, 2^31)")
    refused(b(M=-1), b"M must be in [0, 2^31)")
    for n_long, n_chunks in ((-1, 0), (9, 18), (3, 6)):
        refused(b(n_long=n_long, n_chunks=n_chunks), b"n_long must be in")
    for n_long, n_chunks in ((2, 3), (2, 5), (0, 3)):
        refused(b(n_long=n_long, n_chunks=n_chunks), b"n_chunks must be in")
    assert b(M=0, grad=None, row_ptr=None)[0] == 0                     # no row: a no-op
    refused(b(grad=None), b"grad / row_ptr is NULL")
    refused(b(row_ptr=None), b"grad / row_ptr is NULL")
    refused(b(grad=None, T=0), b"grad / row_ptr is NULL")              # T = 0 still writes every element
    refused(b(perm=None), b"perm / values / ray / basis is NULL")
    refused(b(values=None), b"perm / values / ray / basis is NULL")
    refused(b(ray=None), b"perm / values / ray / basis is NULL")
    refused(b(basis=None), b"perm / values / ray / basis is NULL")
    refused(b(n_long=2, n_chunks=4, long_rows=None), b"long_rows / long_chunk_ptr / chunk_long is NULL")
    for name in ("ray", "basis", "values", "gv", "gs", "row_ptr", "perm", "grad", "ws"):
        refused(b(**{name: odd1}), b"a misaligned argument")
    need = lib.svoxt_shade_samples_bwd_workspace_bytes(4, 28)
    refused(b(n_long=2, n_chunks=4, ws=None), b"workspace is NULL")
    refused(b(n_long=2, n_chunks=4, wsb=need - 1), b"workspace smaller than svoxt_shade_samples_bwd_workspace_bytes")


def _samples(T=6, Q=2):
    z = torch.zeros(T)
    return svox.RaySamples(torch.tensor([0, T // 2, T], dtype=torch.int64)[:Q + 1], torch.zeros(T, dtype=torch.int32),
                           torch.zeros(T, dtype=torch.int32), z, z + 1)


def test_python_layer_refuses_what_it_cannot_serve():
    """(the trees are on the CPU: the checks of the arguments come first, then `only the GPU path exists`)"""
    sh = svox.VolumeRenderer(svox.N3Tree(N=2, data_dim=28, init_reserve=4, data_format="SH9"))
    rgba = svox.VolumeRenderer(svox.N3Tree(N=2, data_dim=4, init_reserve=4))
    rays = svox.Rays(torch.zeros(2, 3), torch.ones(2, 3), torch.ones(2, 3))
    sm = _samples()
    f28, f4 = torch.zeros(3, 28), torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match="samples must be a RaySamples"):
        sh.shade_samples(sm.row, f28, rays)
    with pytest.raises(RuntimeError, match=r"features must be float32 \[M, K\]"):
        sh.shade_samples(sm, f28.double(), rays)
    with pytest.raises(RuntimeError, match=r"features must be float32 \[M, K\]"):
        sh.shade_samples(sm, f28[0], rays)
    with pytest.raises(RuntimeError, match="needs `rays` or a `basis`"):
        sh.shade_samples(sm, f28)
    for bad in (torch.zeros(2, 4), torch.zeros(3, 9), torch.zeros(2, 9, dtype=torch.float64), torch.zeros(18)):
        with pytest.raises(RuntimeError, match=r"basis must be float32 \[Q, basis_dim\] = \[2, 9\]"):
            sh.shade_samples(sm, f28, basis=bad)
    with pytest.raises(RuntimeError, match="transformation_matrices are not served"):
        sh.shade_samples(sm, f28, rays, transformation_matrices=torch.eye(3).repeat(3, 1, 1))
    with pytest.raises(RuntimeError, match="transformation_matrices are not served"):
        sh.view_basis(rays, transformation_matrices=torch.eye(3).repeat(3, 1, 1))
    # CPU tensors: only the GPU path exists
    with pytest.raises(RuntimeError, match="only the GPU"):
        sh.shade_samples(sm, f28, rays)
    with pytest.raises(RuntimeError, match="only the GPU"):
        sh.shade_samples(sm, f28, basis=torch.zeros(2, 9))
    with pytest.raises(RuntimeError, match="only the GPU"):
        rgba.shade_samples(sm, f4)
    with pytest.raises(RuntimeError, match="only the GPU"):
        sh.view_basis(rays)
    with pytest.raises(RuntimeError, match="must be the VolumeRenderer"):
        svox.shade_samples(sm, f28, rays)
    # the operator layer's own checks (svox_t_amd.csrc), for callers that go below the renderer
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        _C.shade_samples_fwd(f4, sm.row, sm.ray, None, 2, rgba._get_options(), True)
    with pytest.raises(RuntimeError, match=r"features must be float32 \[M, K\]"):
        _C.shade_samples_fwd(f4.double(), sm.row, sm.ray, None, 2, rgba._get_options(), True)
    with pytest.raises(RuntimeError, match="plan must be a row plan"):
        _C.shade_samples_bwd((3, 4), sm.ray, None, 2, rgba._get_options(), True, torch.zeros(6, 3), None, None, None)


# ------------------------------------------------------------------------------------------- anchor of the restatement
CASES = {
    "sh9": (O.FORMAT_SH, 9, 28, None),
    "sh4_sub_gap": (O.FORMAT_SH, 4, 14, (1, 2)),          # a component sub-range and a column that is no channel's
    "sg6": (O.FORMAT_SG, 6, 19, None),
    "rgba4": (O.FORMAT_RGBA, -1, 4, None),
    "rgba32": (O.FORMAT_RGBA, -1, 32, None),
}


@pytest.mark.parametrize("activate", [True, False])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_restatements_gradient_is_the_autograd_formulas(case, activate):
    """T = 6000 samples of Q = 300 rays on M = 50 rows (ten of them named by nobody): the restatement's float32
    contributions, summed per entry in float64, against the float64 gradient of sum(sigmoid(basis . coefficients) * g_values)
    + sum(sigma * g_sigma), within assert_grads_close's rtol = 1e-5 of the per-entry sum of |contributions|.  The table is
    N(0, 0.5^2) clipped to +-2, so |tmp| stays below 3 (RGBA: the clip; the largest met are 1.67 for RGBA, 1.48 for SH9,
    0.35 for SG6): the backward forms d from the float32 sig, whose rounding alone moves 1 - sig by 2^-24 / (1 - sig)
    relative, 1.2e-6 at tmp = 3 -- the bound would not hold for saturated channels, for the reference's arithmetic no
    more than for this one."""
    fmt, bd, K, comp = CASES[case]
    rng = np.random.default_rng(3)
    M, Q, T = 50, 300, 6000
    kw = {} if comp is None else dict(min_comp=comp[0], max_comp=comp[1])
    opt = O.make_options(format=fmt, basis_dim=bd, **kw)
    feats = np.clip(rng.standard_normal((M, K)) * 0.5, -2, 2).astype(np.float32)
    vd = rng.standard_normal((Q, 3))
    vd = (vd / np.linalg.norm(vd, axis=1, keepdims=True)).astype(np.float32)
    extra = None
    if fmt == O.FORMAT_SG:
        mu = rng.standard_normal((bd, 3))
        extra = np.concatenate([rng.uniform(0.5, 4.5, (bd, 1)), mu / np.linalg.norm(mu, axis=1, keepdims=True)], 1).astype(np.float32)
    basis = SR.basis(opt, vd, extra)
    row = rng.integers(0, M - 10, T).astype(np.int32)
    ray = np.sort(rng.integers(0, Q, T)).astype(np.int32)
    C, b = SR.dims(opt, K)
    gv = rng.standard_normal((T, C)).astype(np.float32)
    gs = rng.standard_normal(T).astype(np.float32)
    values, sigma = SR.forward(feats, row, ray, opt, basis, activate)
    np.testing.assert_array_equal(sigma, feats[row, K - 1])
    con = SR.contributions(feats, row, ray, opt, basis, values, gv, gs, activate)
    got = np.zeros((M, K))
    np.add.at(got, row, con.astype(np.float64))
    absum = np.zeros((M, K))
    np.add.at(absum, row, np.abs(con).astype(np.float64))

    f = torch.tensor(feats, dtype=torch.float64, requires_grad=True)
    rows, rays_ = torch.from_numpy(row.astype(np.int64)), torch.from_numpy(ray.astype(np.int64))
    if b:
        lo, hi = opt.min_comp, opt.max_comp + 1
        coef = f[rows][:, :C * b].reshape(T, C, b)[:, :, lo:hi]
        tmp = (coef * torch.from_numpy(basis.astype(np.float64))[rays_][:, None, lo:hi]).sum(-1)
    else:
        tmp = f[rows][:, :C]
    print(f"{case}: max |tmp| = {float(tmp.detach().abs().max()):.3f}")
    assert float(tmp.detach().abs().max()) < 3.0
    vals = torch.sigmoid(tmp) if activate else tmp
    np.testing.assert_allclose(values, vals.detach().numpy(), rtol=1e-6, atol=1e-6)
    ((vals * torch.from_numpy(gv.astype(np.float64))).sum() + (f[rows, K - 1] * torch.from_numpy(gs.astype(np.float64))).sum()).backward()
    want = f.grad.numpy()
    assert np.count_nonzero(want) > 0.5 * (M - 10) * (C + 1)
    assert_grads_close(got, want, absum)                               # (and exactly 0 where nothing contributes)
    assert not got[M - 10:].any() and not absum[M - 10:].any()
    # the chunked float32 sum of the same contributions is what grad returns
    from tests import rows_restate as R
    np.testing.assert_array_equal(SR.grad(feats, row, ray, opt, basis, values, gv, gs, activate), R.reduce(con, row, M, "sum", 0.0))
