"""shade_samples with per-row rotations without a GPU: the new symbols, every argument check of the C ABI over fake
pointers, the Python layer's refusals, the input builders of tests/test_gpu_viewrot.py with the assertions that the inputs
are what they claim, and the restated float32 sequences (tests/viewrot_restate.py) against the float64 yardstick within
the derived bounds."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from svox_t_amd.csrc._abi import _COptions
from tests import samples_restate as R
from tests import test_gpu_rowgrad as TR
from tests import viewrot_restate as VR
from tests.test_rowgrad_host import specs
from tests.test_viewgrad_host import extra_of, worst
from tests.test_viewgrad_host import scene as _scene

NAMES = ("svoxt_shade_rot_fwd", "svoxt_shade_rot_bwd", "svoxt_shade_rot_bwd_dir", "svoxt_shade_rot_bwd_rotations",
         "svoxt_shade_rot_bwd_viewdirs")
LONG = "vr_long_sh9"
BIG = 1 << 31
_BUILT = {}


# the inputs ------------------------------------------------------------------------------------------------------------
def _long_scene():
    """A depth-2 full tree (64 leaves) whose data names 6 feature rows, under 41 x 41 rays, SH9 rows: more than a thousand
    samples a row, so the row walk's chunk and join kernels run; two more rows in the table that no leaf names; Q = 1681 is
    no multiple of 64."""
    t, feats = TR.full_tree(2, 1, 28, rows=6, seed=5, fmt="SH9")
    feats = torch.cat([feats, synth.shell_features(2, 28, seed=6)])
    feats[:, -1] = feats[:, -1].abs() + 0.2
    s = TR.Scene.__new__(TR.Scene)
    s.fmt, s.K, s.W, s.H, s.Q, s.comp, s.lobes = "SH9", 28, 41, 41, 41 * 41, None, None
    s.cpu_tree, s.features = t, feats
    n = t.n_internal
    s.ot = O.Tree(feats.numpy(), t.data[:n].numpy(), t.child[:n].numpy(), offset=t.offset.numpy(), scaling=t.invradius.numpy())
    s.opt = O.make_options(format=O.FORMAT_SH, basis_dim=9)
    s.rays = tuple(a.numpy() for a in synth.pinhole_rays(41, 41, c2w=synth.camera_pose(), fx=41.0))
    s.C, s.g, s._want = 3, synth.grad_output(41 * 41, 4).numpy(), {}
    return s


def scene(name):
    if name == LONG:
        if LONG not in TR._BUILT:
            TR._BUILT[LONG] = _long_scene()
        return TR._BUILT[LONG]
    return _scene(name)


def rotations(M, d=3, seed=17):
    """float32 [M, d, d]: general matrices -- the identity plus N(0, 0.4^2) in every entry, so scale and shear as blended
    skinning matrices have them -- and matrix 1 all zero.  d = 4: the same 3 x 3 blocks inside matrices whose other entries
    are random numbers that must not be read."""
    rng = np.random.default_rng(seed)
    m = (np.eye(3)[None] + 0.4 * rng.standard_normal((M, 3, 3))).astype(np.float32)
    if M > 1:
        m[1] = 0
    if d == 3:
        return m
    full = rng.standard_normal((M, 4, 4)).astype(np.float32)
    full[:, :3, :3] = m
    return full


def viewdirs(s):
    """The scene's view directions with zero components here and there and no negative zero."""
    v = s.rays[2].astype(np.float32).copy()
    v[3, 2], v[5, 0], v[7] = 0.0, 0.0, (0.0, 0.0, 1.0)
    v = v + np.float32(0)
    assert not np.signbit(v[v == 0]).any()
    return np.ascontiguousarray(v)


def host_lists(name):
    """(scene, lists, rotations, viewdirs, g_values, g_sigma): restated once."""
    if name not in _BUILT:
        s = scene(name)
        L = R.lists(s.ot, s.rays, s.opt, 0.0)
        rng = np.random.default_rng(7)
        T = L.row.shape[0]
        _BUILT[name] = (s, L, rotations(s.ot.M), viewdirs(s), rng.standard_normal((T, s.C)).astype(np.float32),
                        rng.standard_normal(T).astype(np.float32))
    return _BUILT[name]


def test_the_inputs_are_what_they_claim():
    s, L, rot, v, _, _ = host_lists(LONG)
    counts = np.bincount(L.row, minlength=s.ot.M)
    assert s.ot.M == 8 and counts.max() > 256 and (counts > 256).sum() >= 1 and (counts[6:] == 0).all()     # long rows; rows never hit
    assert counts[1] > 0                                               # the all-zero matrix is a row that is hit
    assert s.Q % 64 and (np.diff(L.offsets) == 0).any()                # no multiple of a wavefront; a ray without samples
    assert not rot[1].any() and np.abs(rot[0] - np.eye(3)).max() > 0.05
    sym = rot[0] @ rot[0].T                                            # not orthogonal: scale and shear
    assert np.abs(sym - np.eye(3)).max() > 0.05 and abs(np.linalg.det(rot[0].astype(np.float64)) - 1) > 1e-3
    assert (v == 0).any() and not np.signbit(v[v == 0]).any()
    r4 = rotations(s.ot.M, 4)
    np.testing.assert_array_equal(r4[:, :3, :3], rot)
    assert np.abs(r4[:, 3]).min() > 0
    s9, L9, _, _, _, _ = host_lists("sh9")
    assert s9.Q % 64 == 0 and (np.bincount(L9.row, minlength=s9.ot.M) == 0).any()


# symbols and checks ----------------------------------------------------------------------------------------------------
def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    header = open(_C.LIB_PATH.rsplit("/svox_t_amd/", 1)[0] + "/include/svoxt.h").read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS and n + "(" in header
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22            # entry points added, nothing changed
    X = _C._extras
    for f in (X.shade_rot_fwd, X.shade_rot_bwd, X.shade_rot_bwd_dir, X.shade_rot_bwd_rotations, X.shade_rot_bwd_viewdirs):
        assert callable(f)
    import inspect
    assert "rotations" in inspect.signature(svox.VolumeRenderer.shade_samples).parameters
    assert "rotations" in inspect.signature(svox.shade_samples).parameters


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    err = lib.svoxt_last_error
    fwd, bwd, bdir, brot, bvd = (getattr(lib, n) for n in NAMES)
    by = ctypes.byref
    _, _, o9, p, _keep = specs(K=28, fmt=1, bd=9)
    P = [ctypes.c_void_p(p.value + (i << 32)) for i in range(24)]     # far apart, never dereferenced: nothing overlaps
    odd1 = ctypes.c_void_p(p.value + 1)
    sg = _COptions(1e-3, 1.0, 2, 6, -1, -1, 0.0, 0, 5, 0.0, 0.0)
    asg = _COptions(1e-3, 1.0, 3, 6, -1, -1, 0.0, 0, 5, 0.0, 0.0)
    rgba = _COptions(1e-3, 1.0, 0, 0, -1, -1, 0.0, 0, -1, 0.0, 0.0)

    def refused(res, text):
        assert res[0] == 1 and text in res[1], res

    # the forward: (features, M, K, opt, extra, extra_rows, extra_cols, rotations, rot_dim, viewdirs, Q, row, ray, T, activate,
    # values, sigma, stream)
    def f(features=P[0], M=8, K=28, opt=o9, extra=None, er=0, ec=0, rot=P[1], d=3, vd=P[2], Q=16, row=P[3], ray=P[4], T=600,
          values=P[5], sigma=P[6]):
        return fwd(features, M, K, None if opt is None else by(opt), extra, er, ec, rot, d, vd, Q, row, ray, T, 1, values, sigma, None), err()

    # the gradient in gu: (..the forward's view side.., row, ray, T, activate, values, grad_values, gu, stream)
    def g(features=P[0], M=8, K=28, opt=o9, extra=None, er=0, ec=0, rot=P[1], d=3, vd=P[2], Q=16, row=P[3], ray=P[4], T=600,
          activate=1, values=P[5], gv=P[7], gu=P[8]):
        return bdir(features, M, K, None if opt is None else by(opt), extra, er, ec, rot, d, vd, Q, row, ray, T, activate, values, gv, gu,
                    None), err()

    # the table's gradient: (opt, M, K, extra, er, ec, rotations, rot_dim, viewdirs, Q, row, ray, T, activate, values, gv, gs,
    # row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, n_long, n_chunks, grad, workspace, workspace_bytes, stream)
    def b(opt=o9, M=8, K=28, extra=None, er=0, ec=0, rot=P[1], d=3, vd=P[2], Q=16, row=P[3], ray=P[4], T=600, activate=1, values=P[5],
          gv=P[7], gs=P[9], row_ptr=P[10], perm=P[11], long_rows=P[12], long_chunk_ptr=P[13], chunk_long=P[14], n_long=0, n_chunks=0,
          grad=P[15], ws=P[16], wsb=1 << 40):
        return bwd(None if opt is None else by(opt), M, K, extra, er, ec, rot, d, vd, Q, row, ray, T, activate, values, gv, gs, row_ptr,
                   perm, long_rows, long_chunk_ptr, chunk_long, n_long, n_chunks, grad, ws, wsb, None), err()

    for call in (f, g, b):                                             # what the three share
        refused(call(opt=None), b"options is NULL")
        refused(call(opt=_COptions(1e-3, 1.0, 4, 9, -1, -1, 0.0, 0, 8, 0.0, 0.0)), b"unknown data format")
        refused(call(K=0), b"K must be >= 1")
        for T in (-1, BIG):
            refused(call(T=T), b"T must be in [0, 2^31)")
        for M in (-1, BIG):
            refused(call(M=M), b"M must be in [0, 2^31)")
        for Q in (-1, BIG):
            refused(call(Q=Q), b"Q must be in [0, 2^31)")
        for bd in (0, 26):
            refused(call(opt=_COptions(1e-3, 1.0, 1, bd, -1, -1, 0.0, 0, 0, 0.0, 0.0)), b"basis_dim must be in [1, 25]")
        refused(call(opt=_COptions(1e-3, 1.0, 1, 9, -1, -1, 0.0, -1, 8, 0.0, 0.0)), b"min_comp / max_comp outside")
        refused(call(opt=_COptions(1e-3, 1.0, 1, 9, -1, -1, 0.0, 0, 9, 0.0, 0.0)), b"min_comp / max_comp outside")
        refused(call(K=1 << 10, M=BIG - 1), b"must be below 2^38")
        refused(call(opt=rgba, K=4), b"RGBA has no basis to rotate")
        refused(call(opt=_COptions(1e-3, 1.0, 1, 7, -1, -1, 0.0, 0, 6, 0.0, 0.0)), b"SH basis_dim must be")
        refused(call(opt=sg, K=19), b"SG/ASG formats need extra")
        refused(call(opt=sg, K=19, extra=P[17], er=5, ec=4), b"SG/ASG formats need extra")
        refused(call(opt=sg, K=19, extra=P[17], er=6, ec=3), b"SG/ASG formats need extra")
        refused(call(opt=asg, K=19, extra=P[17], er=6, ec=10), b"SG/ASG formats need extra")
        for d in (2, 5, 0, 9):
            refused(call(d=d), b"rot_dim must be 3 or 4")
        refused(call(rot=None), b"rotations / viewdirs is NULL")
        refused(call(vd=None), b"rotations / viewdirs is NULL")
        for name in ("rot", "vd", "row", "ray", "values"):
            refused(call(**{name: odd1}), b"a misaligned argument")
        refused(call(opt=sg, K=19, extra=odd1, er=6, ec=4), b"a misaligned argument")

    # the forward's own
    assert f(T=0, row=None, ray=None, values=None, sigma=None)[0] == 0        # no sample: a no-op
    for name in ("row", "ray", "values", "sigma"):
        refused(f(**{name: None}), b"row / ray / values / sigma is NULL")
    refused(f(features=None), b"features is NULL")
    for name in ("features", "sigma"):
        refused(f(**{name: odd1}), b"a misaligned argument")
    for other in (P[0], P[1], P[2], P[3], P[4]):                      # an output on top of an input, or of the other output
        refused(f(values=other), b"values / sigma overlaps")
    refused(f(sigma=P[5]), b"values / sigma overlaps")
    refused(f(sigma=ctypes.c_void_p(P[0].value + 64)), b"values / sigma overlaps")
    refused(f(opt=sg, K=19, extra=P[17], er=6, ec=4, values=P[17]), b"values / sigma overlaps")

    # gu's own
    assert g(T=0, row=None, ray=None, values=None, gv=None, gu=None)[0] == 0
    for name in ("gu", "row", "ray"):
        refused(g(**{name: None}), b"gu / row / ray is NULL")
    refused(g(values=None), b"values / features is NULL")
    refused(g(features=None), b"values / features is NULL")
    for name in ("features", "gv", "gu"):
        refused(g(**{name: odd1}), b"a misaligned argument")
    for other in (P[0], P[1], P[2], P[3], P[4], P[5], P[7]):
        refused(g(gu=other), b"gu overlaps an input")

    # the table gradient's own
    for n_long, n_chunks in ((-1, 0), (9, 18), (3, 6)):
        refused(b(n_long=n_long, n_chunks=n_chunks), b"n_long must be in")
    for n_long, n_chunks in ((2, 3), (2, 5), (0, 3)):
        refused(b(n_long=n_long, n_chunks=n_chunks), b"n_chunks must be in")
    assert b(M=0, grad=None, row_ptr=None, rot=None)[0] == 0           # no row: a no-op
    refused(b(grad=None), b"grad / row_ptr is NULL")
    refused(b(row_ptr=None), b"grad / row_ptr is NULL")
    for name in ("perm", "row", "ray", "values"):
        refused(b(**{name: None}), b"perm / row / ray / values is NULL")
    refused(b(n_long=2, n_chunks=4, long_rows=None), b"long_rows / long_chunk_ptr / chunk_long is NULL")
    for name in ("gv", "gs", "row_ptr", "perm", "grad", "ws"):
        refused(b(**{name: odd1}), b"a misaligned argument")
    for other in (P[1], P[2], P[3], P[4], P[5], P[7], P[9]):
        refused(b(grad=other), b"grad overlaps an input")
    need = lib.svoxt_shade_samples_bwd_workspace_bytes(4, 28)
    refused(b(n_long=2, n_chunks=4, ws=None), b"workspace is NULL")
    refused(b(n_long=2, n_chunks=4, wsb=need - 1), b"workspace smaller than svoxt_shade_samples_bwd_workspace_bytes")

    # rotations.grad: (gu, viewdirs, Q, ray, T, M, rot_dim, row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, n_long, n_chunks,
    # grad_rotations, workspace, workspace_bytes, stream)
    def r(gu=P[8], vd=P[2], Q=16, ray=P[4], T=600, M=8, d=3, row_ptr=P[10], perm=P[11], long_rows=P[12], long_chunk_ptr=P[13],
          chunk_long=P[14], n_long=0, n_chunks=0, grad=P[18], ws=P[16], wsb=1 << 40):
        return brot(gu, vd, Q, ray, T, M, d, row_ptr, perm, long_rows, long_chunk_ptr, chunk_long, n_long, n_chunks, grad, ws, wsb, None), err()

    refused(r(T=BIG), b"T must be in [0, 2^31)")
    refused(r(M=-1), b"M must be in [0, 2^31)")
    refused(r(Q=BIG), b"Q must be in [0, 2^31)")
    refused(r(d=5), b"rot_dim must be 3 or 4")
    refused(r(n_long=9, n_chunks=18), b"n_long must be in")
    refused(r(n_long=2, n_chunks=3), b"n_chunks must be in")
    assert r(M=0, grad=None, row_ptr=None)[0] == 0
    refused(r(grad=None), b"grad_rotations / row_ptr is NULL")
    refused(r(row_ptr=None), b"grad_rotations / row_ptr is NULL")
    for name in ("perm", "gu", "ray", "vd"):
        refused(r(**{name: None}), b"perm / gu / ray / viewdirs is NULL")
    refused(r(n_long=2, n_chunks=4, chunk_long=None), b"long_rows / long_chunk_ptr / chunk_long is NULL")
    for name in ("gu", "vd", "ray", "row_ptr", "perm", "grad", "ws"):
        refused(r(**{name: odd1}), b"a misaligned argument")
    for other in (P[8], P[2], P[4]):
        refused(r(grad=other), b"grad_rotations overlaps an input")
    refused(r(n_long=2, n_chunks=4, ws=None), b"workspace is NULL")
    refused(r(n_long=2, n_chunks=4, d=4, wsb=lib.svoxt_shade_samples_bwd_workspace_bytes(4, 16) - 1), b"workspace smaller than")

    # viewdirs.grad: (gu, rotations, rot_dim, M, offsets, row, ray, T, Q, grad_vdirs, stream)
    def v(gu=P[8], rot=P[1], d=3, M=8, offsets=P[19], row=P[3], ray=P[4], T=600, Q=16, grad=P[20]):
        return bvd(gu, rot, d, M, offsets, row, ray, T, Q, grad, None), err()

    refused(v(T=-1), b"T must be in [0, 2^31)")
    refused(v(M=BIG), b"M must be in [0, 2^31)")
    refused(v(Q=-1), b"Q must be in [0, 2^31)")
    refused(v(d=2), b"rot_dim must be 3 or 4")
    assert v(Q=0, offsets=None, grad=None)[0] == 0
    refused(v(offsets=None), b"offsets / grad_vdirs is NULL")
    refused(v(grad=None), b"offsets / grad_vdirs is NULL")
    for name in ("gu", "row", "ray", "rot"):
        refused(v(**{name: None}), b"gu / row / ray / rotations is NULL")
    for name in ("gu", "rot", "row", "ray", "grad", "offsets"):
        refused(v(**{name: odd1}), b"a misaligned argument")
    refused(v(offsets=ctypes.c_void_p(P[19].value + 4)), b"a misaligned argument")   # offsets are int64
    for other in (P[8], P[1], P[19], P[3], P[4]):
        refused(v(grad=other), b"grad_vdirs overlaps an input")


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
    rot = torch.eye(3).repeat(3, 1, 1)
    with pytest.raises(RuntimeError, match="`rotations` and `basis` exclude each other"):
        sh.shade_samples(sm, f28, rays, basis=torch.zeros(2, 9), rotations=rot)
    for bad in (torch.eye(3), rot.double(), torch.zeros(3, 3, 4), torch.zeros(3, 2, 2), torch.zeros(3, 9), [rot]):
        with pytest.raises(RuntimeError, match=r"rotations must be float32 \[M, 3, 3\] or \[M, 4, 4\]"):
            sh.shade_samples(sm, f28, rays, rotations=bad)
    with pytest.raises(RuntimeError, match="rotations holds 4 matrices, the feature table 3 rows"):
        sh.shade_samples(sm, f28, rays, rotations=torch.eye(4).repeat(4, 1, 1))
    with pytest.raises(RuntimeError, match="`rotations` needs `rays`"):
        sh.shade_samples(sm, f28, rotations=rot)
    with pytest.raises(RuntimeError, match="`rotations` needs `rays`"):        # a camera is no Rays: its directions are the kernels'
        sh.shade_samples(sm, f28, object(), rotations=rot)
    for bad in (torch.ones(3, 3), torch.ones(2, 3, dtype=torch.float64), torch.ones(2, 4)):
        with pytest.raises(RuntimeError, match=r"rays.viewdirs must be float32 \[Q, 3\] with Q = 2"):
            sh.shade_samples(sm, f28, svox.Rays(rays.origins, rays.dirs, bad), rotations=rot)
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="rotations must be on the device of the features"):
            sh.shade_samples(sm, f28, rays, rotations=rot.cuda())
    # the old keyword keeps raising, with the same words, and names the new one
    with pytest.raises(RuntimeError, match="transformation_matrices are not served.*rotations="):
        sh.shade_samples(sm, f28, rays, transformation_matrices=rot)
    with pytest.raises(RuntimeError, match="transformation_matrices are not served"):
        sh.view_basis(rays, transformation_matrices=rot)
    with pytest.raises(TypeError):                                     # view_basis has no such keyword: a per-ray basis has no row
        sh.view_basis(rays, rotations=rot)
    # CPU tensors: only the GPU path exists
    with pytest.raises(RuntimeError, match="only the GPU"):
        sh.shade_samples(sm, f28, rays, rotations=rot)
    with pytest.raises(RuntimeError, match="only the GPU"):
        sh.shade_samples(sm, f28, rays, rotations=torch.eye(4).repeat(3, 1, 1))
    with pytest.raises(RuntimeError, match="only the GPU"):
        rgba.shade_samples(sm, f4, rotations=rot)                      # RGBA ignores them: the plain call's refusal
    with pytest.raises(RuntimeError, match="only the GPU"):
        svox.shade_samples(sh, sm, f28, rays, rotations=rot)
    # the operator layer's own checks, for callers that go below the renderer
    X = _C._extras
    o9, o4 = sh._get_options(), rgba._get_options()
    v = rays.viewdirs
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        X.shade_rot_fwd(f28, sm.row, sm.ray, rot, v, None, 2, o9, True)
    with pytest.raises(RuntimeError, match="RGBA has no basis to rotate"):
        X.shade_rot_fwd(f4, sm.row, sm.ray, rot, v, None, 2, o4, True)
    with pytest.raises(RuntimeError, match="plan must be a row plan"):
        X.shade_rot_bwd((3, 28), sm.row, sm.ray, rot, v, None, 2, o9, True, torch.zeros(6, 3), None, None, None)
    with pytest.raises(RuntimeError, match="plan must be a row plan"):
        X.shade_rot_bwd_rotations(torch.zeros(6, 3), v, sm.ray, (3, 3, 3), None)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        X.shade_rot_bwd_viewdirs(torch.zeros(6, 3), rot, sm.offsets, sm.row, sm.ray)


# the restatement against the yardstick -----------------------------------------------------------------------------------
def check_against_float64(name, activate, got=None, d=3, label=""):
    """The three float32 gradients (`got`, or the restatement's) against grads64 within bounds; returns them."""
    s, L, rot, v, gv, gs = host_lists(name)
    rot = rotations(s.ot.M, d)
    ex = extra_of(s)
    feats = s.features.numpy()
    values, _ = VR.forward32(feats, L.row, L.ray, s.opt, rot, v, ex, activate)
    if got is None:
        gu = VR.gu32(feats, L.row, L.ray, s.opt, rot, v, ex, values, gv, activate)
        got = (VR.features_grad32(feats, L.row, L.ray, s.opt, rot, v, ex, values, gv, gs, activate),
               VR.rotations_grad32(gu, L.row, L.ray, v, rot.shape), VR.viewdirs_grad32(gu, L.offsets, L.row, L.ray, rot, s.Q))
    want = VR.grads64(feats, L.row, L.ray, s.opt, rot, v, ex, gv, gs, activate)
    bound = VR.bounds(feats, L.offsets, L.row, L.ray, s.opt, rot, v, ex, values, gv, gs, activate)
    for what, a, w, b in zip(("features", "rotations", "viewdirs"), got, want, bound):
        r = worst(a, w, b)
        nz = w != 0
        rel = float(np.median(b[nz] / np.abs(w[nz])))
        print(f"{name} activate={activate}{label} {what}.grad: worst |err| / bound = {r:.3f}; median bound / |grad| = {rel:.2e}")
        assert a.dtype == np.float32 and a.shape == w.shape and r <= 1
        assert np.count_nonzero(w) > 20 and rel <= 1e-2                # the comparison says something: the typical entry to 2 digits
    return got


@pytest.mark.parametrize("activate", [True, False])
@pytest.mark.parametrize("name", ["sh9", "sh4_sub", "sh16", "sh25", "sg6", "asg6", "n3_sh4"])
def test_sequences_within_the_bounds_of_float64(name, activate):
    gf, gr, gvd = check_against_float64(name, activate)
    s, L, rot, _, _, _ = host_lists(name)
    outside = [c * s.opt.basis_dim + i for c in range(s.C) for i in range(s.opt.basis_dim) if not s.opt.min_comp <= i <= s.opt.max_comp]
    assert not gf[:, outside].any()
    never = np.bincount(L.row, minlength=s.ot.M) == 0
    assert never.any() and not gf[never].any() and not gr[never].any()
    assert not gvd[np.diff(L.offsets) == 0].any()


def test_sequences_4x4_and_long_rows():
    a = check_against_float64(LONG, True)
    b = check_against_float64(LONG, True, d=4, label=" [M, 4, 4]")
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1][:, :3, :3])
    np.testing.assert_array_equal(a[2], b[2])
    assert not b[1][:, 3].any() and not b[1][:, :, 3].any()
