"""The gradient in the view direction on the GPU: view_basis in viewdirs and shade_samples in basis, bit for bit against the
restatement (tests/viewgrad_restate.py) and within its derived bounds of float64; both gradients of one call, the edges,
determinism, the refusals, and the colour chain from c2w to a loss and back.

Every test that asks autograd for a gradient in viewdirs, basis or c2w through these two operators fails without the
feature (autograd raises: the tensor was never used); the forward-bit tests pass either way, on purpose."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd.renderer import _make_camera_spec, pinhole_rays
from tests import raygeom_restate as G
from tests import samples_restate as R
from tests import shade_restate as SR
from tests import test_gpu_shade as TS
from tests import viewgrad_restate as V
from tests.test_viewgrad_host import extra_of, view_batch, worst

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tg(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


# 1. view_basis in viewdirs -----------------------------------------------------------------------------------------------
def view_grad(L, v, g, gpu):
    """(basis, viewdirs.grad) as numpy for the 66 directions v and the upstream gradient g."""
    vt = tg(v, gpu).requires_grad_(True)
    o = torch.zeros_like(vt)
    basis = L.r.view_basis(svox.Rays(o, vt.detach(), vt))
    assert basis.requires_grad
    basis.backward(tg(g, gpu))
    return basis.detach().cpu().numpy(), vt.grad.cpu().numpy()


@pytest.mark.parametrize("name", ["n3_sh4", "sh9", "sh16", "sh25", "sg6", "asg6"])
def test_grad_viewdirs_bits(gpu, name):
    L = TS.lists(name, gpu)
    s = L.s
    v, ex = view_batch(s), extra_of(s)
    assert v.shape[0] % 64 and (v == 0).any()
    want_basis = O.basis(s.opt.format, s.opt.basis_dim, v, ex)
    g = np.random.default_rng(3).standard_normal(want_basis.shape).astype(np.float32)
    basis, got = view_grad(L, v, g, gpu)
    np.testing.assert_array_equal(bits(basis), bits(want_basis))                    # the forward keeps its bits
    with torch.no_grad():
        plain = L.r.view_basis(svox.Rays(tg(v, gpu), tg(v, gpu), tg(v, gpu)))
    assert not plain.requires_grad
    np.testing.assert_array_equal(bits(plain.cpu().numpy()), bits(want_basis))
    want = V.view_backward32(s.opt, v, ex, want_basis, g)
    assert got.dtype == np.float32 and got.shape == (66, 3) and np.count_nonzero(want) >= 3 * 60
    np.testing.assert_array_equal(bits(got), bits(want))
    r = worst(got, V.view_grad64(s.opt, v, ex, g), V.view_bound(s.opt, v, ex, g))
    print(f"{name}: worst |err| / bound = {r:.3f}")
    assert r <= 1
    np.testing.assert_array_equal(bits(view_grad(L, v, g, gpu)[1]), bits(got))      # twice the same bits


def test_view_basis_without_grad_keeps_its_route(gpu):
    L = TS.lists("sh9", gpu)
    v = tg(view_batch(L.s), gpu)
    rays = svox.Rays(v, v, v.clone().requires_grad_(True))
    with torch.no_grad():
        assert not L.r.view_basis(rays).requires_grad
    assert not L.r.view_basis(svox.Rays(v, v, v)).requires_grad
    R4 = TS.lists("rgba4", gpu)                                                     # RGBA: no basis, no gradient, no kernel
    got = R4.r.view_basis(rays)
    assert tuple(got.shape) == (66, 0) and not got.requires_grad
    assert tuple(_C._extras.view_basis_backward(R4.r.tree._spec(R4.r.tree.features), svox.renderer._rays_spec_from_rays(svox.Rays(v, v, v)),
                                        R4.r._get_options(), None, None).shape) == (66, 3)


# 2. shade_samples in basis -----------------------------------------------------------------------------------------------
def basis_grad(L, gpu, samples=None, features=None, basis=None, gv=None, activate=True, gs=None, want_features=False):
    """(values, basis.grad[, features.grad]) as numpy from one backward."""
    f = (L.f if features is None else features).clone().requires_grad_(want_features)
    b = tg(L.basis if basis is None else basis, gpu).requires_grad_(True)
    samples = L.samples if samples is None else samples
    values, sigma = L.r.shade_samples(samples, f, basis=b, activate=activate)
    outs, gos = [], []
    if gv is not None:
        outs.append(values), gos.append(tg(gv, gpu))
    if gs is not None:
        outs.append(sigma), gos.append(tg(gs, gpu))
    grads = torch.autograd.grad(outs, [b, f] if want_features else [b], gos, allow_unused=True)
    return (values.detach().cpu().numpy(),) + tuple(None if x is None else x.cpu().numpy() for x in grads)


@pytest.mark.parametrize("activate", [True, False])
@pytest.mark.parametrize("name", ["sh9", "sh4_sub", "sh4_gap", "sh4_c2", "sg6", "asg6", "n3_sh4", "d5_sh9"])
def test_grad_basis_bits(gpu, name, activate):
    L = TS.lists(name, gpu)
    s = L.s
    off = L.samples.offsets.cpu().numpy()
    values, got = basis_grad(L, gpu, gv=L.gv, activate=activate)
    want_v = L.restated(activate)[0]
    np.testing.assert_array_equal(bits(values), bits(want_v))                       # the forward keeps its bits
    args = (L.feats, off, L.row, L.ray, s.opt, want_v, L.gv, activate)
    want = V.basis_backward32(*args)
    assert got.dtype == np.float32 and got.shape == (s.Q, s.opt.basis_dim) and np.count_nonzero(want) > 100
    np.testing.assert_array_equal(bits(got), bits(want))
    outside = [i for i in range(s.opt.basis_dim) if not s.opt.min_comp <= i <= s.opt.max_comp]
    assert not got[:, outside].any() and not np.signbit(got[:, outside]).any()
    empty = np.diff(off) == 0
    assert empty.any() and not got[empty].any()
    r = worst(got, V.basis_grad64(*args), V.basis_bound(*args))
    print(f"{name} activate={activate}: worst |err| / bound = {r:.3f}")
    assert r <= 1
    if activate:
        np.testing.assert_array_equal(bits(basis_grad(L, gpu, gv=L.gv)[1]), bits(got))      # twice the same bits


def test_lane_groups_do_not_straddle_rays(gpu):
    """bd = 4, 6, 9, 16, 25 lanes a ray: 256 is a multiple of 4 and 16 only, and Q = 1024 rays fill more than one block."""
    for name in ("sh16", "sh25"):
        L = TS.lists(name, gpu)
        off = L.samples.offsets.cpu().numpy()
        _, got = basis_grad(L, gpu, gv=L.gv)
        want = V.basis_backward32(L.feats, off, L.row, L.ray, L.s.opt, L.restated()[0], L.gv, True)
        np.testing.assert_array_equal(bits(got), bits(want))
        assert L.s.Q * L.s.opt.basis_dim > 4 * 256


def test_grad_basis_edges(gpu):
    L = TS.lists("sh9", gpu)
    counts = L.samples.counts.cpu().numpy()
    off = L.samples.offsets.cpu().numpy()
    hit, miss = np.flatnonzero(counts > 3), np.flatnonzero(counts == 0)
    want_all = V.basis_backward32(L.feats, off, L.row, L.ray, L.s.opt, L.restated()[0], L.gv, True)
    # a ray without samples between rays with samples; the one-ray list
    for idx in ([int(hit[0]), int(miss[0]), int(hit[-1])], [int(counts.argmax())]):
        rays, sm = TS._subset(L, idx, gpu)
        pick = np.concatenate([np.arange(off[q], off[q + 1]) for q in idx])
        _, got = basis_grad(L, gpu, samples=sm, basis=L.basis[idx], gv=L.gv[pick])
        np.testing.assert_array_equal(bits(got), bits(want_all[idx]))
        assert got.shape == (len(idx), 9)
    # the empty list: zeros for every ray
    o = torch.full((70, 3), 5.0, device=gpu)
    d = torch.nn.functional.normalize(torch.rand(70, 3, device=gpu) + 0.1, dim=1).contiguous()
    rays = svox.Rays(o, d, d)
    sm = L.r.ray_samples(rays, features=L.f, min_sigma=0.0)
    assert len(sm) == 0
    b = L.r.view_basis(rays).requires_grad_(True)
    values, _ = L.r.shade_samples(sm, L.f, basis=b)
    values.sum().backward()
    assert tuple(b.grad.shape) == (70, 9) and not b.grad.any()


def test_grad_basis_rows_outside_and_a_selected_list(gpu):
    L = TS.lists("sh9", gpu)
    off = L.samples.offsets.cpu().numpy()
    M = L.M + 40
    feats = torch.cat([L.s.features, torch.randn(40, L.K, generator=torch.Generator().manual_seed(11))])
    row = L.row.astype(np.int64).copy()
    row[::5], row[1::7], row[2::11], row[3::13] = -1, M, 2 ** 31 - 1, -2 ** 31
    sm = L.samples
    made = svox.RaySamples(sm.offsets, sm.ray, tg(row.astype(np.int32), gpu), sm.depth, sm.length)
    values, got = basis_grad(L, gpu, samples=made, features=feats.to(gpu), gv=L.gv)
    want_v = SR.forward(feats.numpy(), row, L.ray, L.s.opt, L.basis)[0]
    np.testing.assert_array_equal(bits(values), bits(want_v))
    np.testing.assert_array_equal(bits(got), bits(V.basis_backward32(feats.numpy(), off, row, L.ray, L.s.opt, want_v, L.gv, True)))
    # a list from select
    keep = np.random.default_rng(9).uniform(size=L.T) < 0.6
    sub, index = L.samples.select(tg(keep, gpu))
    index = index.cpu().numpy()
    _, got = basis_grad(L, gpu, samples=sub, gv=L.gv[index])
    want = V.basis_backward32(L.feats, sub.offsets.cpu().numpy(), L.row[index], L.ray[index], L.s.opt, L.restated()[0][index], L.gv[index], True)
    np.testing.assert_array_equal(bits(got), bits(want))
    assert 0 < len(sub) < L.T


# 3. both gradients of one call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sh9", "sg6"])
def test_both_gradients_of_one_call(gpu, name):
    L = TS.lists(name, gpu)
    off = L.samples.offsets.cpu().numpy()
    want_f = SR.grad(L.feats, L.row, L.ray, L.s.opt, L.basis, L.restated()[0], L.gv, L.gs)
    want_b = V.basis_backward32(L.feats, off, L.row, L.ray, L.s.opt, L.restated()[0], L.gv, True)
    _, gb, gf = basis_grad(L, gpu, gv=L.gv, gs=L.gs, want_features=True)
    np.testing.assert_array_equal(bits(gf), bits(want_f))                          # the bits tests/test_gpu_shade.py pins
    np.testing.assert_array_equal(bits(gb), bits(want_b))
    np.testing.assert_array_equal(bits(basis_grad(L, gpu, gv=L.gv, gs=L.gs)[1]), bits(want_b))       # basis alone
    np.testing.assert_array_equal(bits(TS.run(L, gv=L.gv, gs=L.gs)[2]), bits(want_f))                # features alone
    # only sigma is used: grad_values is absent, basis.grad is zeros
    _, gb0 = basis_grad(L, gpu, gs=L.gs)
    assert gb0.shape == want_b.shape and not gb0.any()
    # RGBA: no basis, no gradient
    R4 = TS.lists("rgba4", gpu)
    f = R4.f.clone().requires_grad_(True)
    values, _ = R4.r.shade_samples(R4.samples, f, R4.rays)
    values.backward(tg(R4.gv, gpu))
    np.testing.assert_array_equal(bits(f.grad.cpu().numpy()), bits(SR.grad(R4.feats, R4.row, R4.ray, R4.s.opt, R4.basis, R4.restated()[0], R4.gv, None)))
    assert tuple(_C._extras.shade_samples_bwd_basis(R4.f, R4.samples.offsets, R4.samples.row, R4.samples.ray, R4.s.Q, R4.r._get_options(), True,
                                            values.detach(), None).shape) == (R4.s.Q, 0)


# 4. determinism, rays= against basis= ------------------------------------------------------------------------------------
def test_same_bits_with_rays_as_with_basis(gpu):
    L = TS.lists("sh9", gpu)

    def run(through_rays):
        v = L.rays.viewdirs.clone().requires_grad_(True)
        rays = svox.Rays(L.rays.origins, L.rays.dirs, v)
        if through_rays:
            values, _ = L.r.shade_samples(L.samples, L.f, rays)
        else:
            values, _ = L.r.shade_samples(L.samples, L.f, basis=L.r.view_basis(rays))
        values.backward(tg(L.gv, gpu))
        return values.detach().cpu().numpy(), v.grad.cpu().numpy()

    a, b, c = run(True), run(False), run(True)
    np.testing.assert_array_equal(bits(a[0]), bits(L.restated()[0]))
    for x in (b, c):
        np.testing.assert_array_equal(bits(x[0]), bits(a[0]))
        np.testing.assert_array_equal(bits(x[1]), bits(a[1]))
    gb = V.basis_backward32(L.feats, L.samples.offsets.cpu().numpy(), L.row, L.ray, L.s.opt, L.restated()[0], L.gv, True)
    np.testing.assert_array_equal(bits(a[1]), bits(V.view_backward32(L.s.opt, L.s.rays[2], None, L.basis, gb)))
    assert np.count_nonzero(a[1]) > 500


# 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_what_is_refused(gpu):
    L = TS.lists("sh9", gpu)
    s = L.s
    c2w = tg(np.eye(4, dtype=np.float32)[:3], gpu)
    cam = _make_camera_spec(c2w, s.W, s.H, 30.0, 30.0)
    spec = L.r.tree._spec(L.r.tree.features.detach())
    b = tg(L.basis, gpu)
    with pytest.raises(RuntimeError, match="camera mode has no viewdirs tensor"):
        _C._extras.view_basis_backward(spec, cam, L.r._get_options(), b, torch.ones_like(b))
    # a second backward: the graph is gone; and no double backward
    bb = b.clone().requires_grad_(True)
    values, _ = L.r.shade_samples(L.samples, L.f, basis=bb)
    values.sum().backward()
    with pytest.raises(RuntimeError, match="second time"):
        values.sum().backward()
    bb = b.clone().requires_grad_(True)
    values, _ = L.r.shade_samples(L.samples, L.f, basis=bb)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(values.sum(), bb, create_graph=True)
    v = L.rays.viewdirs.clone().requires_grad_(True)
    basis = L.r.view_basis(svox.Rays(L.rays.origins, L.rays.dirs, v))
    (gv,) = torch.autograd.grad(basis.sum(), v, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        gv.sum().backward()
    with pytest.raises(RuntimeError, match="transformation_matrices are not served"):
        L.r.view_basis(svox.Rays(L.rays.origins, L.rays.dirs, v), transformation_matrices=torch.eye(3, device=gpu).repeat(L.M, 1, 1))


# 6. the chain --------------------------------------------------------------------------------------------------------------
def test_colour_chain_from_c2w(gpu):
    """pinhole_rays(c2w) -> ray_samples(faces=True) -> sample_geometry, view_basis -> shade_samples -> sample_weights(length=)
    -> accumulate(colour) -> loss.backward(): c2w.grad against the same chain in float64 over the SAME lists.

    The bound, propagated (u = 2^-24; every "tight" function is the abs-linear response of a gradient that is linear in its
    upstream gradient, so an upstream error of that size moves it by at most that much):
      values   the forward against float64: tmp sums 9 products of a float32 basis value (within 3 u of its abs-evaluation,
               viewgrad_restate.sh_abs64) and a coefficient: d_tmp = 1.001 (4 + 9) u sum_i B_i |f_i|; the sigmoid's slope is at
               most 1/4, pexpf is priced at 4 u of e, the rounded division at u: d_sig = d_tmp / 4 + 6 u sig
      w        the forward tolerance of sample_weights: d_w = 1e-5 w + 1e-6 (what tests/test_gpu_raygeom.py uses)
      g_values = G_q,c w_k: d_gv = |G| (d_w + u w);  the bracket t = g_values d(sig): d_t = d_gv / 4 + |g_values| d_sig
      g_basis  basis_bound at the magnitudes |g_values| + d_gv, plus basis_tight(d_t)
      g_view   view_bound at |g_basis| + d_gb, plus view_tight(d_gb)
      g_w = sum_c G values: d_gw = sum_c |G| (d_sig + (C + 1) u |values|);  g_length: 1e-5 of its tight scale
               (sample_weights' tolerance) plus the scale of d_gw
      g_dirs   geometry_bound for the float64 chain's g_length, plus geometry_tight(d_gl); the two halves meet in one float32
               add on the way into pinhole_rays (viewdirs IS dirs there)
      c2w      as tests/test_gpu_raygeom.py: origins are c2w's last column (the bounds add up over the rays), dirs = R (X, Y,
               Z) (they add up times |X|, |Y|, |Z|), the float32 sums over Q rays priced at (Q + 2) u of their terms' magnitudes."""
    from svox_t_amd import synth
    L = TS.lists("sh9", gpu)
    s = L.s
    W, H, Q, C, bd = s.W, s.H, s.Q, s.C, 9
    pose = np.asarray(synth.camera_pose(), dtype=np.float32)
    fx = fy = 1.0 * W
    Gq = np.random.default_rng(31).standard_normal((Q, C)).astype(np.float32)

    def chain(geometry=True):
        c2w = tg(pose, gpu).requires_grad_(True)
        o, d, v = pinhole_rays(c2w, W, H, fx, fy)
        rays = svox.Rays(o, d, v)
        sm = L.r.ray_samples(rays, features=L.f, min_sigma=0.0, faces=True)
        values, sigma = L.r.shade_samples(sm, L.f, rays)
        if geometry:
            _, length = svox.sample_geometry(sm, rays)
            w, _ = svox.sample_weights(sm, sigma, length=length)
        else:
            w, _ = svox.sample_weights(sm, sigma)
        out = svox.accumulate(sm, w, values)
        (out * tg(Gq, gpu)).sum().backward()
        return c2w, (o, d, v), sm, values

    c2w, (o, d, v), sm, values = chain()
    assert torch.equal(chain()[0].grad, c2w.grad)                                  # twice the same bits
    got = c2w.grad.cpu().numpy()
    view_only = chain(geometry=False)[0].grad.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(view_only[:, :3]).min() > 0 and not view_only[:, 3].any() and len(sm) > 1000

    # the yardstick: the same rays (their float32 numbers) through the restated march, then float64 all the way
    rays_np = tuple(x.detach().cpu().numpy() for x in (o, d, v))
    F = G.lists_with_faces(s.ot, rays_np, s.opt, 0.0)
    Ls = F.lists
    for name, a in zip(R.Lists._fields, (sm.offsets, sm.row, sm.ray, sm.depth, sm.length)):
        np.testing.assert_array_equal(a.cpu().numpy(), getattr(Ls, name), err_msg=name)
    np.testing.assert_array_equal(sm.face.cpu().numpy(), F.face)
    np.testing.assert_array_equal(bits(values.detach().cpu().numpy()),
                                  bits(SR.forward(L.feats, Ls.row, Ls.ray, s.opt, SR.basis(s.opt, rays_np[2]))[0]))
    ray = torch.from_numpy(Ls.ray.astype(np.int64))
    row = Ls.row.astype(np.int64)
    c64 = torch.from_numpy(pose).double().requires_grad_(True)
    # pinhole_rays in double: its (X, Y, Z) are float32 numbers that do not depend on c2w (an identity pose returns them);
    # dirs = R (X, Y, Z), anchored at the float32 rays the lists were marched from, so both chains stand at the same point
    with torch.no_grad():
        XYZ = pinhole_rays(torch.eye(4), W, H, fx, fy)[1].double()
    d_lin = XYZ @ c64[:3, :3].T
    d64 = d_lin + (torch.from_numpy(rays_np[1]).double() - d_lin).detach()
    o64 = c64[:3, 3].expand(Q, 3) * 1.0
    v64 = d64 * 1.0
    for x in (o64, d64, v64):
        x.retain_grad()
    _, length64 = G.geometry64(F, o64, d64, anchored=True)
    basis64 = V.basis64(s.opt, v64)
    f64 = torch.from_numpy(L.feats[row]).double()
    values64 = torch.sigmoid(torch.einsum("ki,kci->kc", basis64[ray], f64[:, :C * bd].reshape(-1, C, bd)))
    w64, _ = G.weights64(length64, f64[:, -1], Ls.offsets)
    for x in (length64, basis64, values64, w64):
        x.retain_grad()
    out64 = torch.zeros(Q, C, dtype=torch.float64).index_add(0, ray, w64[:, None] * values64)
    (out64 * torch.from_numpy(Gq).double()).sum().backward()
    want = c64.grad.numpy()

    U = V.U
    rq = Ls.ray.astype(np.int64)
    absG = np.abs(Gq.astype(np.float64))[rq]                                       # [T, C]
    wv, sig = w64.detach().numpy(), values64.detach().numpy()
    fabs = np.abs(L.feats[row].astype(np.float64))[:, :C * bd].reshape(-1, C, bd)
    d_tmp = V.SLACK * (4 + bd) * U * np.einsum("ki,kci->kc", V.sh_abs64(bd, rays_np[2])[rq], fabs)
    d_sig = 0.25 * d_tmp + 6 * U * sig
    d_w = 1e-5 * wv + 1e-6
    gv64 = np.abs(values64.grad.numpy())
    d_gv = absG * (d_w + U * wv)[:, None]
    d_t = 0.25 * d_gv + gv64 * d_sig
    feats, off = L.feats, Ls.offsets
    d_gb = V.basis_bound(feats, off, Ls.row, Ls.ray, s.opt, sig.astype(np.float32), gv64 + d_gv, True) \
        + V.basis_tight(feats, off, Ls.row, Ls.ray, s.opt, d_t)
    gb64 = np.abs(basis64.grad.numpy())
    b_view = V.view_bound(s.opt, rays_np[2], None, gb64 + d_gb) + V.view_tight(s.opt, rays_np[2], None, d_gb)
    d_gw = (absG * (d_sig + (C + 1) * U * sig)).sum(1)
    sigma_np = L.feats[row, -1]
    d_gl = 1e-5 * G.grad_length_scale(Ls.length, sigma_np, off, np.abs(w64.grad.numpy()), None) \
        + G.grad_length_scale(Ls.length, sigma_np, off, d_gw, None)
    bo, bdirs = G.geometry_bound(F, rays_np[1], None, length64.grad.numpy(), float(s.opt.step_size), s.ot.offset)
    lo, ld = G.geometry_tight(F, rays_np[1], d_gl, d_gl)
    bo, bdirs = bo + lo, bdirs + ld + b_view
    xyz = np.abs(XYZ.numpy())                                                      # |X|, |Y|, |Z| per ray
    go_abs = np.abs(o64.grad.numpy())
    gd_abs = np.abs(d64.grad.numpy() - v64.grad.numpy()) + np.abs(v64.grad.numpy())
    bound = np.zeros_like(want)
    bound[:, 3] = bo.sum(0) + (Q + 2) * U * go_abs.sum(0)
    bound[:, :3] = np.einsum("qi,qj->ij", bdirs, xyz) + (Q + 2) * U * np.einsum("qi,qj->ij", gd_abs, xyz)
    ratio = np.abs(got - want) / bound
    print("c2w.grad:\n", got, "\nfloat64:\n", want, "\n|err| / bound:\n", ratio)
    assert np.all(ratio <= 1) and np.all(np.abs(want) > 0)
    # the view-dependent part alone (the geometry detached: w has the same numbers): dirs = R (X, Y, Z), so its gradient
    # in R is sum_q g_view[q, i] (X, Y, Z)[q, j] -- a much smaller bound, without the geometry's step term
    gview = v64.grad.numpy()
    want_view = np.einsum("qi,qj->ij", gview, XYZ.numpy())
    bound_view = np.einsum("qi,qj->ij", b_view, xyz) + (Q + 2) * U * np.einsum("qi,qj->ij", np.abs(gview), xyz)
    ratio_view = np.abs(view_only[:, :3] - want_view) / bound_view
    print("the view term alone:\n", view_only[:, :3], "\nfloat64:\n", want_view, "\n|err| / bound:\n", ratio_view,
          "\nbound / |want|:\n", bound_view / np.abs(want_view))
    assert np.all(ratio_view <= 1) and np.all(bound_view <= 1e-3 * np.einsum("qi,qj->ij", np.abs(gview), xyz))
    tight = np.zeros_like(want)
    tight[:, 3] = go_abs.sum(0)
    tight[:, :3] = np.einsum("qi,qj->ij", gd_abs, xyz)
    print("bound / tight:\n", bound / tight)
    assert np.all(bound <= 2e-2 * tight)                                           # the comparison says something
