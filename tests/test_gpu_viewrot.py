"""shade_samples(rotations=) on the GPU: the forward's bits against the restatement (tests/viewrot_restate.py), [M, 4, 4]
against its 3 x 3 block, identity rotations against the unrotated call, RGBA; the three gradients -- features, rotations,
viewdirs -- bit for bit against the restatement and within their derived bounds of float64, alone and from one call; the
edges, determinism, the composed renderer against forward(transformation_matrices=) and the oracle, and the pose chain
from joint matrices to a loss and back.

Every test here that passes `rotations=` fails without the feature (TypeError: an unexpected keyword argument)."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
from oracle import oracle as O
from tests import shade_restate as SR
from tests import test_gpu_shade as TS
from tests import test_viewrot_host as H
from tests import viewrot_restate as VR
from tests.test_viewgrad_host import extra_of
from tests.util import assert_grads_close

pytestmark = pytest.mark.gpu
NAMES = ["sh9", "sh4_sub", "sh4_gap", "sh4_c2", "sh16", "sh25", "sg6", "asg6", "n3_sh4", "d5_sh9", H.LONG]
_WANT = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tg(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def lists(name, gpu):
    H.scene(name)                                                      # (registers the scenes the siblings' tables do not hold)
    return TS.lists(name, gpu)


def run(L, gpu, rot, v, samples=None, features=None, gv=None, gs=None, activate=True, wrt="frv"):
    """(values, sigma, {"f": features.grad, "r": rotations.grad, "v": viewdirs.grad}) as numpy; only the gradients named in
    `wrt` are asked for; gv / gs: numpy upstream gradients or None (not given)."""
    f = (L.f if features is None else features).clone().requires_grad_("f" in wrt)
    R = tg(rot, gpu).requires_grad_("r" in wrt)
    vt = tg(v, gpu).requires_grad_("v" in wrt)
    rays = svox.Rays(L.rays.origins, L.rays.dirs, vt)
    values, sigma = L.r.shade_samples(L.samples if samples is None else samples, f, rays, rotations=R, activate=activate)
    outs, gos = [], []
    if gv is not None:
        outs.append(values), gos.append(tg(gv, gpu))
    if gs is not None:
        outs.append(sigma), gos.append(tg(gs, gpu))
    grads = {}
    if outs and wrt:
        got = torch.autograd.grad(outs, [dict(f=f, r=R, v=vt)[w] for w in wrt], gos, allow_unused=True)
        grads = {w: (None if x is None else x.cpu().numpy()) for w, x in zip(wrt, got)}
    return values.detach().cpu().numpy(), sigma.detach().cpu().numpy(), grads


def restated(L, rot, v, activate=True, gv=None, gs=None, row=None, ray=None, feats=None, offsets=None):
    """(values, sigma, features.grad, rotations.grad, viewdirs.grad) of the restatement."""
    s = L.s
    feats = L.feats if feats is None else feats
    row = L.row if row is None else row
    ray = L.ray if ray is None else ray
    offsets = L.samples.offsets.cpu().numpy() if offsets is None else offsets
    ex = extra_of(s)
    values, sigma = VR.forward32(feats, row, ray, s.opt, rot, v, ex, activate)
    gu = VR.gu32(feats, row, ray, s.opt, rot, v, ex, values, gv, activate)
    return (values, sigma, VR.features_grad32(feats, row, ray, s.opt, rot, v, ex, values, gv, gs, activate),
            VR.rotations_grad32(gu, row, ray, v, rot.shape), VR.viewdirs_grad32(gu, offsets, row, ray, rot, s.Q))


def wanted(name, L, activate, d=3):
    """The restatement of the scene's standard case, once."""
    key = (name, activate, d)
    if key not in _WANT:
        _WANT[key] = restated(L, H.rotations(L.M, d), H.viewdirs(L.s), activate, L.gv, L.gs)
    return _WANT[key]


# 1. forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activate", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_forward_bits(gpu, name, activate):
    L = lists(name, gpu)
    rot, v = H.rotations(L.M), H.viewdirs(L.s)
    values, sigma, _ = run(L, gpu, rot, v, activate=activate, wrt="")
    want_v, want_s = wanted(name, L, activate)[:2]
    assert values.dtype == np.float32 and values.shape == (L.T, L.C) and sigma.shape == (L.T,) and L.T > 1000
    np.testing.assert_array_equal(bits(values), bits(want_v))
    np.testing.assert_array_equal(bits(sigma), bits(want_s))
    assert np.abs(values - L.restated(activate)[0]).max() > 1e-3      # the rotations do something
    v4, s4, _ = run(L, gpu, H.rotations(L.M, 4), v, activate=activate, wrt="")       # [M, 4, 4]: its 3 x 3 block
    np.testing.assert_array_equal(bits(v4), bits(values))
    np.testing.assert_array_equal(bits(s4), bits(sigma))


@pytest.mark.parametrize("name", ["sh9", "sh4_sub", "sh25", "sg6", "asg6"])
def test_identity_rotations_give_the_unrotated_bits(gpu, name):
    L = lists(name, gpu)
    v = H.viewdirs(L.s)                                                # (no negative zero: 1 * v + 0 * w + 0 * x keeps every bit)
    eye = np.tile(np.eye(3, dtype=np.float32), (L.M, 1, 1))
    for activate in (True, False):
        values, sigma, _ = run(L, gpu, eye, v, activate=activate, wrt="")
        with torch.no_grad():
            pv, ps = L.r.shade_samples(L.samples, L.f, svox.Rays(L.rays.origins, L.rays.dirs, tg(v, gpu)), activate=activate)
        np.testing.assert_array_equal(bits(values), bits(pv.cpu().numpy()))
        np.testing.assert_array_equal(bits(sigma), bits(ps.cpu().numpy()))
    # the package-level function takes the keyword too
    values, _ = svox.shade_samples(L.r, L.samples, L.f, svox.Rays(L.rays.origins, L.rays.dirs, tg(v, gpu)), rotations=tg(eye, gpu),
                                   activate=False)
    np.testing.assert_array_equal(bits(values.cpu().numpy()), bits(pv.cpu().numpy()))


@pytest.mark.parametrize("name", ["rgba4", "rgba6"])
def test_rgba_ignores_rotations(gpu, name):
    L = lists(name, gpu)
    rot = tg(H.rotations(L.M), gpu).requires_grad_(True)
    f = L.f.clone().requires_grad_(True)
    values, sigma = L.r.shade_samples(L.samples, f, rotations=rot)     # (no rays needed: nothing is rotated)
    np.testing.assert_array_equal(bits(values.detach().cpu().numpy()), bits(L.restated()[0]))
    np.testing.assert_array_equal(bits(sigma.detach().cpu().numpy()), bits(L.restated()[1]))
    gf, gr = torch.autograd.grad([values, sigma], [f, rot], [tg(L.gv, gpu), tg(L.gs, gpu)], allow_unused=True)
    assert gr is None                                                  # no gradient reaches the rotations
    np.testing.assert_array_equal(bits(gf.cpu().numpy()), bits(SR.grad(L.feats, L.row, L.ray, L.s.opt, L.basis, L.restated()[0], L.gv, L.gs)))
    v2, _ = L.r.shade_samples(L.samples, L.f, L.rays, rotations=tg(H.rotations(L.M, 4), gpu))
    np.testing.assert_array_equal(bits(v2.cpu().numpy()), bits(L.restated()[0]))


# 2. the gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activate", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_gradients_bits_and_bounds(gpu, name, activate):
    L = lists(name, gpu)
    rot, v = H.rotations(L.M), H.viewdirs(L.s)
    _, _, want_f, want_r, want_v = wanted(name, L, activate)
    _, _, g = run(L, gpu, rot, v, gv=L.gv, gs=L.gs, activate=activate)               # all three from one call
    assert g["f"].shape == (L.M, L.K) and g["r"].shape == (L.M, 3, 3) and g["v"].shape == (L.s.Q, 3)
    assert min(np.count_nonzero(want_f), np.count_nonzero(want_r), np.count_nonzero(want_v)) > 40
    for key, want in (("f", want_f), ("r", want_r), ("v", want_v)):
        np.testing.assert_array_equal(bits(g[key]), bits(want), err_msg=key)
        alone = run(L, gpu, rot, v, gv=L.gv, gs=L.gs, activate=activate, wrt=key)[2][key]      # each alone: the same bits
        np.testing.assert_array_equal(bits(alone), bits(want), err_msg=key + " alone")
    never = np.ones(L.M, bool)
    never[L.row] = False
    assert not g["f"][never].any() and not g["r"][never].any()
    assert not g["v"][np.diff(L.samples.offsets.cpu().numpy()) == 0].any()
    # within the derived bounds of the float64 yardstick (the host test holds the restatement to the same bounds); the
    # lists the GPU marched are the restated ones
    # lists and upstream gradients are the restated ones
    s, Lh, _, _, gvh, gsh = H.host_lists(name)
    for a, b in ((Lh.row, L.row), (Lh.ray, L.ray), (gvh, L.gv), (gsh, L.gs)):
        np.testing.assert_array_equal(a, b)
    H.check_against_float64(name, activate, got=(g["f"], g["r"], g["v"]), label=" GPU")


@pytest.mark.parametrize("name", ["sh9", "sg6", H.LONG])
def test_gradients_of_4x4_rotations(gpu, name):
    L = lists(name, gpu)
    v = H.viewdirs(L.s)
    r4 = H.rotations(L.M, 4)
    _, _, want_f, want_r, want_v = wanted(name, L, True)
    _, _, g = run(L, gpu, r4, v, gv=L.gv, gs=L.gs)
    assert g["r"].shape == (L.M, 4, 4)
    np.testing.assert_array_equal(bits(g["f"]), bits(want_f))
    np.testing.assert_array_equal(bits(g["v"]), bits(want_v))
    np.testing.assert_array_equal(bits(g["r"][:, :3, :3]), bits(want_r))
    outside = g["r"].copy()
    outside[:, :3, :3] = 1
    assert np.all((outside == 1) | (bits(outside) == 0))              # exact +0 outside the 3 x 3 block, every element written


def test_long_rows_run_the_chunk_and_join_kernels(gpu):
    L = lists(H.LONG, gpu)
    plan = L.samples.row_plan(L.M)
    assert plan.longest > 512 and plan.long_rows.shape[0] >= 1 and plan.chunk_long.shape[0] >= 3
    _, _, want_f, want_r, _ = wanted(H.LONG, L, True)
    hit = [0, 2, 3, 4, 5]                                              # (row 1's matrix is all zero: its basis is the constant alone)
    assert np.all(want_f[hit, :-1] != 0) and np.all(want_r[hit] != 0) and np.all(want_f[:6, -1] != 0)


# 3. edges --------------------------------------------------------------------------------------------------------------
def test_rows_and_rays_outside_their_ranges(gpu):
    """A hand-edited list: rows outside [0, M) and rays outside [0, Q) get zeros and take part in no gradient; a table with
    40 rows more than the tree names."""
    L = lists("sh9", gpu)
    M = L.M + 40
    feats = torch.cat([L.s.features, torch.randn(40, L.K, generator=torch.Generator().manual_seed(11))])
    row, ray = L.row.astype(np.int64).copy(), L.ray.astype(np.int64).copy()
    row[::5], row[1::7], row[2::11], row[3::13] = -1, M, 2 ** 31 - 1, -2 ** 31
    ray[4::9], ray[6::17], ray[8::19] = -1, L.s.Q, 2 ** 31 - 1
    sm = L.samples
    made = svox.RaySamples(sm.offsets, tg(ray.astype(np.int32), gpu), tg(row.astype(np.int32), gpu), sm.depth, sm.length)
    rot, v = H.rotations(M), H.viewdirs(L.s)
    values, sigma, g = run(L, gpu, rot, v, samples=made, features=feats.to(gpu), gv=L.gv, gs=L.gs)
    want = restated(L, rot, v, True, L.gv, L.gs, row=row, ray=ray, feats=feats.numpy())
    bad_row = (row < 0) | (row >= M)
    bad = bad_row | (ray < 0) | (ray >= L.s.Q)
    assert bad.sum() > L.T // 3 and not values[bad].any() and not sigma[bad_row].any()
    for got, w, what in zip((values, sigma, g["f"], g["r"], g["v"]), want, ("values", "sigma", "f", "r", "v")):
        np.testing.assert_array_equal(bits(got), bits(w), err_msg=what)
    assert not g["f"][L.M:].any() and not g["r"][L.M:].any()
    # the upstream gradient of the samples outside does not matter
    gv2 = L.gv.copy()
    gv2[bad] = 1e30
    g2 = run(L, gpu, rot, v, samples=made, features=feats.to(gpu), gv=gv2, gs=L.gs)[2]
    for key in "frv":
        np.testing.assert_array_equal(bits(g2[key]), bits(g[key]), err_msg=key)


def test_a_selected_sublist(gpu):
    L = lists("sh9", gpu)
    keep = np.random.default_rng(9).uniform(size=L.T) < 0.6
    sub, index = L.samples.select(tg(keep, gpu))
    index = index.cpu().numpy()
    assert 0 < len(sub) < L.T
    rot, v = H.rotations(L.M), H.viewdirs(L.s)
    values, sigma, g = run(L, gpu, rot, v, samples=sub, gv=L.gv[index], gs=L.gs[index])
    want = restated(L, rot, v, True, L.gv[index], L.gs[index], row=L.row[index], ray=L.ray[index], offsets=sub.offsets.cpu().numpy())
    for got, w, what in zip((values, sigma, g["f"], g["r"], g["v"]), want, ("values", "sigma", "f", "r", "v")):
        np.testing.assert_array_equal(bits(got), bits(w), err_msg=what)


@pytest.mark.parametrize("name", ["sh9", "sg6"])
def test_a_none_upstream_gradient(gpu, name):
    L = lists(name, gpu)
    rot, v = H.rotations(L.M), H.viewdirs(L.s)
    # only sigma is used: zeros for the rotations and the directions, the sigma column alone in the table
    g = run(L, gpu, rot, v, gs=L.gs)[2]
    want = restated(L, rot, v, True, None, L.gs)
    np.testing.assert_array_equal(bits(g["f"]), bits(want[2]))
    assert not g["f"][:, :-1].any() and g["f"][:, -1].any()
    assert g["r"].shape == (L.M, 3, 3) and not g["r"].any() and g["v"].shape == (L.s.Q, 3) and not g["v"].any()
    # only values is used
    g = run(L, gpu, rot, v, gv=L.gv)[2]
    want = restated(L, rot, v, True, L.gv, None)
    for key, w in zip("frv", want[2:]):
        np.testing.assert_array_equal(bits(g[key]), bits(w), err_msg=key)
    assert not g["f"][:, -1].any()


@pytest.mark.parametrize("name", ["sh4_sub", "sh4_gap"])
def test_components_outside_the_range_contribute_exact_zeros(gpu, name):
    L = lists(name, gpu)
    s = L.s
    rot, v = H.rotations(L.M), H.viewdirs(s)
    bd = s.opt.basis_dim
    outside = [c * bd + i for c in range(L.C) for i in range(bd) if not s.opt.min_comp <= i <= s.opt.max_comp]
    outside += list(range(L.C * bd, L.K - 1))                          # (a column that is no channel's)
    assert outside
    _, _, g = run(L, gpu, rot, v, gv=L.gv, gs=L.gs)
    assert not g["f"][:, outside].any() and not np.signbit(g["f"][:, outside]).any()
    # ... and whatever the table holds there reaches neither the values nor the other two gradients
    f2 = L.f.clone()
    f2[:, outside] = 1e3 * torch.randn(L.M, len(outside), generator=torch.Generator().manual_seed(2)).to(gpu)
    values, _, g2 = run(L, gpu, rot, v, features=f2, gv=L.gv, gs=L.gs)
    np.testing.assert_array_equal(bits(values), bits(wanted(name, L, True)[0]))
    for key in "frv":
        np.testing.assert_array_equal(bits(g2[key]), bits(g[key]), err_msg=key)


def test_no_samples_and_twice_the_same_bits(gpu):
    L = lists("d5_sh9", gpu)
    rot, v = H.rotations(L.M), H.viewdirs(L.s)
    a = run(L, gpu, rot, v, gv=L.gv, gs=L.gs)
    b = run(L, gpu, rot, v, gv=L.gv, gs=L.gs)
    np.testing.assert_array_equal(bits(a[0]), bits(b[0]))
    for key in "frv":
        np.testing.assert_array_equal(bits(a[2][key]), bits(b[2][key]), err_msg=key)
    # the empty list: every gradient is zeros of its shape
    o = torch.full((70, 3), 5.0, device=gpu)
    d = torch.nn.functional.normalize(torch.rand(70, 3, device=gpu) + 0.1, dim=1).contiguous()
    sm = L.r.ray_samples(svox.Rays(o, d, d), features=L.f, min_sigma=0.0)
    assert len(sm) == 0
    f, R, vt = L.f.clone().requires_grad_(True), tg(rot, gpu).requires_grad_(True), d.clone().requires_grad_(True)
    values, sigma = L.r.shade_samples(sm, f, svox.Rays(o, d, vt), rotations=R)
    assert tuple(values.shape) == (0, L.C) and tuple(sigma.shape) == (0,)
    (values.sum() + sigma.sum()).backward()
    for x, shape in ((f, (L.M, L.K)), (R, (L.M, 3, 3)), (vt, (70, 3))):
        assert tuple(x.grad.shape) == shape and not x.grad.any()


def test_what_is_refused(gpu):
    L = lists("sh9", gpu)
    rot = tg(H.rotations(L.M), gpu)
    with pytest.raises(RuntimeError, match="transformation_matrices are not served"):
        L.r.shade_samples(L.samples, L.f, L.rays, transformation_matrices=rot)
    with pytest.raises(RuntimeError, match="exclude each other"):
        L.r.shade_samples(L.samples, L.f, L.rays, basis=L.r.view_basis(L.rays), rotations=rot)
    with pytest.raises(RuntimeError, match="`rotations` needs `rays`"):
        L.r.shade_samples(L.samples, L.f, rotations=rot)
    with pytest.raises(RuntimeError, match="rotations holds"):
        L.r.shade_samples(L.samples, L.f, L.rays, rotations=rot[:-1])
    with pytest.raises(RuntimeError, match="device of the features"):
        L.r.shade_samples(L.samples, L.f, L.rays, rotations=rot.cpu())
    with pytest.raises(RuntimeError, match=r"rays.viewdirs must be float32 \[Q, 3\]"):
        L.r.shade_samples(L.samples, L.f, svox.Rays(L.rays.origins, L.rays.dirs, L.rays.viewdirs[:-1]), rotations=rot)
    # once differentiable: a double backward raises
    R = rot.clone().requires_grad_(True)
    values, _ = L.r.shade_samples(L.samples, L.f, L.rays, rotations=R)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(values.sum(), R, create_graph=True)
    f = L.f.clone().requires_grad_(True)
    values, _ = L.r.shade_samples(L.samples, f, L.rays, rotations=rot)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(values.sum(), f, create_graph=True)


# 4. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_matrix", "a_matrix_a_row"])
def test_composed_chain_against_the_renderer_and_the_oracle(gpu, case):
    """ray_samples(min_sigma=0) -> shade_samples(rotations=) -> composite, plus (1 - alpha) background_brightness, against
    renderer(features, rays, transformation_matrices=) at thresholds 0, on the SH9 tree.  Alpha: the same bits.  Colours:
    both sum the same n non-negative terms of a ray, each within an ulp: |a - b| <= (n + 4) 2^-23 |b| + 1e-7.
    Gradient: the oracle's backward under O.transformation_matrices, at the project's tolerance (assert_grads_close).

    The oracle is the reference's backward, and with matrices that differ from row to row the reference's second pass
    shades every sample with the basis its first pass left behind: its sigma column is then not
    the gradient of the forward, and no chain that differentiates the forward can meet it (measured here: 636 of 704 sigma
    entries off, the worst 5.1e4 bounds, with every colour column inside).  So the comparison of the WHOLE table with the
    oracle is made with one general matrix shared by all rows, where both passes see the same basis and the reference's
    backward is the gradient; with a matrix a row the colour columns are held to the oracle at the same tolerance, and the
    sigma column is sample_weights' and accumulate's own gradient (tests/test_gpu_samples.py) of the colours checked above."""
    L = lists("sh9", gpu)
    s, C = L.s, L.C
    rot = H.rotations(L.M)
    if case == "one_matrix":
        rot = np.ascontiguousarray(np.broadcast_to(rot[0], rot.shape))
    Rt = tg(rot, gpu)
    f = L.f.clone().requires_grad_(True)
    samples = L.r.ray_samples(L.rays, features=f, min_sigma=0.0)
    values, sigma = L.r.shade_samples(samples, f, L.rays, rotations=Rt)
    out, alpha, _w = svox.composite(samples, sigma, values)
    full = torch.cat([out + (1.0 - alpha)[:, None] * L.r.background_brightness, alpha[:, None]], dim=1)
    with torch.no_grad():
        want = L.r(L.f, L.rays, transformation_matrices=Rt)
        plain = L.r(L.f, L.rays)
    assert tuple(full.shape) == tuple(want.shape) == (s.Q, C + 1)
    assert torch.equal(full[:, C].detach(), want[:, C])
    assert (want[:, :C] - plain[:, :C]).abs().max() > 1e-2             # the matrices change the picture
    a, b = full[:, :C].detach().cpu().numpy().astype(np.float64), want[:, :C].cpu().numpy().astype(np.float64)
    n = samples.counts.cpu().numpy().astype(np.float64)[:, None]
    excess = np.abs(a - b) - ((n + 4) * 2.0 ** -23 * np.abs(b) + 1e-7)
    print(f"{case}: worst |a - b| - bound = {excess.max():.3e}; worst |a - b| = {np.abs(a - b).max():.3e}")
    assert np.all(excess <= 0), (int((excess > 0).sum()), float(excess.max()))
    (full * tg(s.g, gpu)).sum().backward()
    got = f.grad.cpu().numpy()
    with O.transformation_matrices(rot):
        grad_want, absum, _tight = O.volume_render_backward(s.ot, *s.rays, s.opt, s.g, want_abs="both")
    assert np.count_nonzero(grad_want[:, -1]) > 100
    if case == "one_matrix":
        assert_grads_close(got, grad_want, absum)
    else:
        assert_grads_close(got[:, :-1], grad_want[:, :-1], absum[:, :-1], what="colour columns")
    f4 = L.f.clone().requires_grad_(True)                              # [M, 4, 4] through the whole chain: the same bits
    r4 = H.rotations(L.M, 4)
    r4[:, :3, :3] = rot
    v4, s4 = L.r.shade_samples(samples, f4, L.rays, rotations=tg(r4, gpu))
    o4, a4, _ = svox.composite(samples, s4, v4)
    assert torch.equal(o4, out) and torch.equal(a4, alpha)
    (torch.cat([o4 + (1.0 - a4)[:, None] * L.r.background_brightness, a4[:, None]], dim=1) * tg(s.g, gpu)).sum().backward()
    assert torch.equal(f4.grad, f.grad)


def test_pose_chain_from_joint_matrices(gpu):
    """joints -> warp_vertices -> shade_samples(rotations=) -> sample_weights -> accumulate -> loss -> joints.grad, on the
    long-row scene (8 feature rows).  warp_vertices' backward sums a joint's rows with float atomics, so the skinning keeps
    to two rows a joint: a sum of two addends (and zeros: the warped points are not used) has the same bits in either
    order, and the comparison bit for bit is one of THIS operator's gradient, not of the atomics' order."""
    L = lists(H.LONG, gpu)
    M, J = L.M, 8
    g = torch.Generator().manual_seed(21)
    joints0 = (torch.eye(4)[None] + 0.3 * torch.randn(J, 4, 4, generator=g)).to(gpu)
    w = torch.rand(M, 2, generator=g)
    weights = (w / w.sum(1, keepdim=True)).to(gpu)
    joint_index = torch.stack([torch.arange(M), (torch.arange(M) + 1) % J], dim=1).to(torch.int32).to(gpu)
    assert all(int((joint_index == j).sum()) <= 2 for j in range(J))
    zeros = torch.zeros(M, 3, device=gpu)
    Gq = tg(np.random.default_rng(31).standard_normal((L.s.Q, L.C)).astype(np.float32), gpu)

    def loss_of(mats):
        values, sigma = L.r.shade_samples(L.samples, L.f, L.rays, rotations=mats)
        wts, _ = svox.sample_weights(L.samples, sigma)
        return (svox.accumulate(L.samples, wts, values) * Gq).sum()

    joints = joints0.clone().requires_grad_(True)
    _, mats = svox.warp_vertices(joints, zeros, weights, joint_index)
    assert tuple(mats.shape) == (M, 4, 4) and mats.requires_grad
    loss_of(mats).backward()
    got = joints.grad
    assert torch.isfinite(got).all() and int((got[:, :3, :3] != 0).sum()) >= 9 * 5      # (the joints of the rows that are hit)
    # the same gradient in two steps: rotations.grad of a detached run, handed to warp_vertices' own backward
    m2 = mats.detach().clone().requires_grad_(True)
    loss_of(m2).backward()
    assert tuple(m2.grad.shape) == (M, 4, 4) and not m2.grad[:, 3].any() and not m2.grad[:, :, 3].any()
    j2 = joints0.clone().requires_grad_(True)
    _, mats2 = svox.warp_vertices(j2, zeros, weights, joint_index)
    (want,) = torch.autograd.grad(mats2, j2, m2.grad)
    assert torch.equal(got, want)
