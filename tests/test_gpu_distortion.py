"""render_distortion on the GPU against its restatement (tests/distortion_restate.py) and the C++ oracle."""
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from svox_t_amd.renderer import _make_camera_spec
from tests import depth_restate as DR
from tests import distortion_restate as R
from tests.util import Case, assert_grads_close, assert_outputs_close

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")

CASES = {
    "d5_rgba4": dict(depth=5, K=4, data_format="RGBA", width=64, height=64),
    "d5_sh9": dict(depth=5, K=28, data_format="SH9", width=64, height=64),
    "d5_sh4_world": dict(depth=5, K=13, data_format="SH4", width=64, height=64,
                         radius=[1.0, 1.2, 0.8], center=[0.1, -0.2, 0.3]),           # delta_scale != 1
}
OTHER = {"d6_sh9": dict(depth=6, K=28, data_format="SH9", width=96, height=96)}
_BUILT = {}


def built(name):
    """(case, oracle tree, rays): one object each per case, so that the restatement's march is computed once."""
    if name not in _BUILT:
        c = Case(**(CASES.get(name) or OTHER[name]))
        _BUILT[name] = (c, c.oracle_tree(), c.rays_np())
    return _BUILT[name]


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    return built(request.param)


def grad_outputs(Q, kind, seed=11):
    g = synth.grad_output(Q, 2, seed=seed).numpy()
    if kind == "gd":
        g[:, 1:] = 0
    elif kind == "ga":
        g[:, :1] = 0
    else:
        assert kind == "all"
    return g


def hip_grad(r, tree, rays, g, gpu, **kw):
    tree.features.grad = None
    out = r.render_distortion(tree.features, rays, **kw)
    out.backward(torch.from_numpy(g).to(gpu))
    got = tree.features.grad.cpu().numpy()
    assert np.all(got[:, :-1] == 0)                  # only the sigma column receives gradient
    return out.detach().cpu().numpy(), got


# forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True])
def test_forward_parity(case, gpu, fast):
    c, ot, rays = case
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    with torch.no_grad():
        got = r.render_distortion(tree.features, c.rays_gpu(gpu), fast=fast).cpu().numpy()
    opt = c.oracle_opts(fast=fast)
    want = R.distortion(ot, rays, opt, torch.float64).numpy()
    err = np.abs(got - want)
    print("max |err| per column", err.max(0), "max |want|", np.abs(want).max(0))
    assert got.dtype == np.float32 and got.shape == (c.Q, 2)
    assert_outputs_close(got, want)
    # alpha: the same product sequence as opacity_render, on both sides
    np.testing.assert_array_equal(got[:, 1:2], O.opacity_render(ot, *rays, opt))
    assert (got[:, 0] != 0).sum() > 500 and np.all(got[got[:, 1] == 0] == 0)


# backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all", "gd", "ga"])
def test_backward_parity(case, gpu, kind):
    c, ot, rays = case
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    g = grad_outputs(c.Q, kind)
    opt = c.oracle_opts()
    _, got = hip_grad(r, tree, c.rays_gpu(gpu), g, gpu)
    want = R.distortion_grad(ot, rays, opt, g)
    scale = R.distortion_grad_scale(ot, rays, opt, g)
    ratio = np.abs(got - want)[scale > 0] / (1e-5 * scale[scale > 0])
    print(kind, "worst |err| / bound", ratio.max(), "entries", ratio.size)
    assert_grads_close(got, want, scale)
    assert np.all(got[scale == 0] == 0) and (got != 0).sum() > 500
    if kind == "ga":                                 # alpha alone: the C++ oracle's opacity backward
        want, _, tight = O.volume_render_backward(ot, *rays, opt, g[:, 1:2].copy(), want_abs="both")
        assert_grads_close(got, want, tight)


def test_fast_gives_the_gradient_at_thresholds_zero(case, gpu):
    c, ot, rays = case
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    g = grad_outputs(c.Q, "all", seed=12)
    _, got = hip_grad(r, tree, c.rays_gpu(gpu), g, gpu, fast=True)
    opt = c.oracle_opts()
    scale = R.distortion_grad_scale(ot, rays, opt, g)
    assert_grads_close(got, R.distortion_grad(ot, rays, opt, g), scale)
    _, exact = hip_grad(r, tree, c.rays_gpu(gpu), g, gpu, fast=False)
    assert_grads_close(got, exact, scale)


# shapes and degenerate inputs ---------------------------------------------------------------------------------------
def check_case(c, gpu, seed=13, ot=None, tree=None, **kw):
    ot = c.oracle_tree() if ot is None else ot
    tree = c.tree(gpu) if tree is None else tree
    rays, opt = c.rays_np(), c.oracle_opts()
    r = svox.VolumeRenderer(tree)
    g = grad_outputs(c.Q, "all", seed=seed)
    out, got = hip_grad(r, tree, c.rays_gpu(gpu), g, gpu, **kw)
    assert_outputs_close(out, R.distortion(ot, rays, opt, torch.float64).numpy())
    np.testing.assert_array_equal(out[:, 1:2], O.opacity_render(ot, *rays, opt))
    assert_grads_close(got, R.distortion_grad(ot, rays, opt, g), R.distortion_grad_scale(ot, rays, opt, g))
    return out, got


@pytest.mark.parametrize("tiled", [False, True])
def test_image_sides_that_are_no_multiple_of_eight(gpu, tiled):
    c = Case(depth=5, K=4, data_format="RGBA", width=50, height=34)
    out, got = check_case(c, gpu, image_shape=(34, 50) if tiled else None)
    assert (out[:, 1] > 0).sum() > 300 and (got != 0).any()


@pytest.mark.parametrize("Q", [1, 65])
def test_tiny_batches(gpu, Q):
    c, ot, rays = built("d5_rgba4")
    pick = (np.arange(Q) * 37 + 64 * 30 + 20) % 4096   # from the middle rows on: most of them meet the shell
    sub = tuple(np.ascontiguousarray(a[pick]) for a in rays)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    g = grad_outputs(Q, "all", seed=14)
    rg = svox.Rays(*(torch.from_numpy(a).to(gpu) for a in sub))
    out, got = hip_grad(r, tree, rg, g, gpu)
    opt = c.oracle_opts()
    assert out.shape == (Q, 2) and (out[:, 1] > 0).any()
    assert_outputs_close(out, R.distortion(ot, sub, opt, torch.float64).numpy())
    assert_grads_close(got, R.distortion_grad(ot, sub, opt, g), R.distortion_grad_scale(ot, sub, opt, g))


def test_rays_that_all_miss(gpu):
    c, _, _ = built("d5_rgba4")
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    Q = 200
    o = torch.full((Q, 3), 5.0, device=gpu)
    d = torch.nn.functional.normalize(torch.rand(Q, 3, device=gpu) + 0.1, dim=1).contiguous()     # away from the cube
    out, got = hip_grad(r, tree, svox.Rays(o, d, d), np.ones((Q, 2), np.float32), gpu)
    assert np.all(out == 0) and np.all(got == 0)


def test_branching_factor_three(gpu):
    """N = 3: the generic descent.  Every leaf of the fixture's topology gets a feature row of its own."""
    t = np.load(os.path.join(G, "topology_full_n3_l2.npz"))
    n = int(t["n_internal"])
    child, pd = t["child"][:n], t["parent_depth"][:n]
    leaves = child.reshape(-1) == 0
    M = int(leaves.sum())
    data = np.full(child.size, -1, np.int32)
    data[leaves] = np.arange(M, dtype=np.int32)
    data = data.reshape(child.shape + (1,))
    feats = synth.shell_features(M, 7, seed=4)
    with torch.no_grad():
        feats[:, -1] *= 0.02                          # a full tree: keep it translucent
    tree = svox.N3Tree.from_arrays(child, data, pd, feats, data_format="RGBA", device=gpu)
    assert tree.N == 3
    ot = O.Tree(feats.numpy(), data, child, offset=tree.offset.cpu().numpy(), scaling=tree.invradius.cpu().numpy())
    o, d, v = synth.pinhole_rays(40, 40, c2w=synth.camera_pose(radius=1.6))
    rays = (o.numpy(), d.numpy(), v.numpy())
    opt = O.make_options(format=O.FORMAT_RGBA, basis_dim=-1)
    r = svox.VolumeRenderer(tree)
    g = grad_outputs(1600, "all", seed=15)
    out, got = hip_grad(r, tree, svox.Rays(o.to(gpu), d.to(gpu), v.to(gpu)), g, gpu)
    assert_outputs_close(out, R.distortion(ot, rays, opt, torch.float64).numpy())
    np.testing.assert_array_equal(out[:, 1:2], O.opacity_render(ot, *rays, opt))
    assert_grads_close(got, R.distortion_grad(ot, rays, opt, g), R.distortion_grad_scale(ot, rays, opt, g))
    assert (out[:, 1] > 0).sum() > 300 and (got != 0).sum() > 100


def test_rows_of_32_floats(gpu):
    check_case(Case(depth=4, K=32, data_format="RGBA", width=40, height=40), gpu)


@pytest.mark.parametrize("samples", [0, 2, 8, 64])
@pytest.mark.parametrize("tiled", [False, True])
def test_any_list_capacity_gives_the_same_gradient(gpu, samples, tiled, monkeypatch):
    """The forward records up to `samples` (row, delta_t, s) a ray when a backward will follow (rounded up to 4); the
    backward reads them and marches behind the end of an over-long ray's records -- all of the ray with 0 -- carrying T,
    A, D, E, the previous s and the suffix sum across the seam.  At depth 6 / 96 x 96 many rays that meet the shell have
    more than 8 samples, and a tile more than one pass of the LDS table."""
    monkeypatch.setattr(_C._extras, "DISTORTION_SAMPLES", samples)
    c, ot, rays = built("d6_sh9")
    opt = c.oracle_opts()
    lengths = np.array([len(s[0]) for s in ray_samples("d6_sh9")])
    assert (lengths > 8).sum() > 500                  # a seam inside the ray at capacities 4 (from 2) and 8
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    g = grad_outputs(c.Q, "all", seed=16)
    want, scale = R.distortion_grad(ot, rays, opt, g), R.distortion_grad_scale(ot, rays, opt, g)
    out, got = hip_grad(r, tree, c.rays_gpu(gpu), g, gpu, image_shape=(96, 96) if tiled else None)
    np.testing.assert_array_equal(out[:, 1:2], O.opacity_render(ot, *rays, opt))
    assert_outputs_close(out, R.distortion(ot, rays, opt, torch.float64).numpy())
    assert_grads_close(got, want, scale)


_SAMPLES = {}


def ray_samples(name):
    if name not in _SAMPLES:
        c, ot, rays = built(name)
        _SAMPLES[name] = R.ray_samples(ot, rays, c.oracle_opts())
    return _SAMPLES[name]


# ray order ----------------------------------------------------------------------------------------------------------
def test_ray_order_does_not_change_results(gpu):
    c, ot, rays = built("d5_sh9")
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    g = grad_outputs(c.Q, "all", seed=17)
    perm = torch.randperm(c.Q, generator=torch.Generator().manual_seed(5))
    sub = tuple(np.ascontiguousarray(a[perm.numpy()]) for a in rays)
    rg = svox.Rays(*(torch.from_numpy(a).to(gpu) for a in sub))
    o0, g0 = hip_grad(r, tree, rg, g, gpu, sort_rays=False)
    o1, g1 = hip_grad(r, tree, rg, g, gpu, sort_rays=True)
    np.testing.assert_array_equal(o0, o1)
    opt = c.oracle_opts()
    assert_outputs_close(o0, R.distortion(ot, sub, opt, torch.float64).numpy())      # every row at its own index
    want, scale = R.distortion_grad(ot, sub, opt, g), R.distortion_grad_scale(ot, sub, opt, g)
    assert_grads_close(g0, want, scale)
    assert_grads_close(g1, want, scale)


# replay, changed features -------------------------------------------------------------------------------------------
def test_two_backwards_over_one_graph(gpu):
    c, ot, rays = built("d5_rgba4")
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    g = grad_outputs(c.Q, "all", seed=18)
    out = r.render_distortion(tree.features, c.rays_gpu(gpu))
    opt = c.oracle_opts()
    want, scale = R.distortion_grad(ot, rays, opt, g), R.distortion_grad_scale(ot, rays, opt, g)
    grads = []
    for _ in range(2):
        tree.features.grad = None
        out.backward(torch.from_numpy(g).to(gpu), retain_graph=True)
        grads.append(tree.features.grad.cpu().numpy())
        assert_grads_close(grads[-1], want, scale)
    assert_grads_close(grads[0], grads[1], scale)


def test_backward_after_the_features_changed_marches(gpu, monkeypatch):
    """The plan the forward left is keyed by the feature table's version: after an in-place change no plan matches and
    the backward marches -- the gradient at the table's new values, as with no records at all."""
    c, _, _ = built("d5_rgba4")
    tree = c.tree(gpu)
    spec, opt = tree._spec(tree.features), svox.VolumeRenderer(tree)._get_options()
    rg = c.rays_gpu(gpu)
    g = torch.from_numpy(grad_outputs(c.Q, "all", seed=19)).to(gpu)

    def rspec():
        s = svox.renderer._rays_spec_from_rays(rg, None, None)
        s.need_grad = True
        return s

    rs = rspec()
    _C.distortion(spec, rs, opt)
    assert rs._svoxt_distortion_plan is not None and rs._svoxt_distortion_plan[3] > 0
    with torch.no_grad():
        tree.features[:, -1] *= 1.5
    stale = _C.distortion_backward(spec, rs, opt, g).cpu().numpy()
    monkeypatch.setattr(_C._extras, "DISTORTION_SAMPLES", 0)
    rs0 = rspec()
    _C.distortion(spec, rs0, opt)
    assert rs0._svoxt_distortion_plan is None
    marched = _C.distortion_backward(spec, rs0, opt, g).cpu().numpy()
    ot = O.Tree(tree.features.detach().cpu().numpy(), c.st.data, c.st.child, offset=tree.offset.cpu().numpy(),
                scaling=tree.invradius.cpu().numpy())
    oopt = c.oracle_opts()
    scale = R.distortion_grad_scale(ot, c.rays_np(), oopt, g.cpu().numpy())
    assert_grads_close(stale, marched, scale)
    assert_grads_close(stale, R.distortion_grad(ot, c.rays_np(), oopt, g.cpu().numpy()), scale)
    assert (stale != 0).sum() > 500


def test_both_operators_recorded_on_one_spec(gpu):
    """render_depth_moments(at="mid") and render_distortion share their forward, backward and plan code: recorded one
    after the other on ONE rays spec, each keeps a plan of its own, and the backwards -- taken in the opposite order --
    give what each operator gives on a fresh spec.  Through csrc, not the renderer: VolumeRenderer builds a fresh spec for
    every call, so only this level can put two plans on one spec.  The plan assertions are what catches a collision (a
    backward whose plan does not match marches, and still agrees); one Rays object through the renderer follows, for the
    autograd Function both operators share."""
    c, ot, rays = built("d5_rgba4")
    tree = c.tree(gpu)
    spec, opt = tree._spec(tree.features), svox.VolumeRenderer(tree)._get_options()
    rg = c.rays_gpu(gpu)
    g3 = synth.grad_output(c.Q, 3, seed=20).to(gpu)
    g2 = torch.from_numpy(grad_outputs(c.Q, "all", seed=21)).to(gpu)

    def rspec():
        s = svox.renderer._rays_spec_from_rays(rg, None, None)
        s.need_grad = True
        return s

    rs = rspec()
    _C.depth_moments(spec, rs, opt, "mid")
    _C.distortion(spec, rs, opt)
    for plan in (rs._svoxt_depth_plan, rs._svoxt_distortion_plan):
        assert plan is not None and plan[2] is not None and plan[3] > 0
    assert rs._svoxt_depth_plan[2].data_ptr() != rs._svoxt_distortion_plan[2].data_ptr()
    ds = _C.distortion_backward(spec, rs, opt, g2).cpu().numpy()
    dm = _C.depth_moments_backward(spec, rs, opt, g3, "mid").cpu().numpy()
    own = rspec()
    _C.distortion(spec, own, opt)
    ds_own = _C.distortion_backward(spec, own, opt, g2).cpu().numpy()
    own = rspec()
    _C.depth_moments(spec, own, opt, "mid")
    dm_own = _C.depth_moments_backward(spec, own, opt, g3, "mid").cpu().numpy()
    oopt = c.oracle_opts()
    assert_grads_close(ds, ds_own, R.distortion_grad_scale(ot, rays, oopt, g2.cpu().numpy()))
    assert_grads_close(dm, dm_own, DR.moments_grad_scale(ot, rays, oopt, "mid", g3.cpu().numpy()))
    assert (ds != 0).sum() > 500 and (dm != 0).sum() > 500
    r = svox.VolumeRenderer(tree)
    out_dm = r.render_depth_moments(tree.features, rg, at="mid")
    out_ds = r.render_distortion(tree.features, rg)
    tree.features.grad = None
    out_ds.backward(g2)
    ds_r = tree.features.grad.cpu().numpy()
    tree.features.grad = None
    out_dm.backward(g3)
    dm_r = tree.features.grad.cpu().numpy()
    assert_grads_close(ds_r, ds_own, R.distortion_grad_scale(ot, rays, oopt, g2.cpu().numpy()))
    assert_grads_close(dm_r, dm_own, DR.moments_grad_scale(ot, rays, oopt, "mid", g3.cpu().numpy()))


# the loss, the camera form ------------------------------------------------------------------------------------------
def test_distortion_loss_reductions(gpu):
    c, ot, rays = built("d5_sh4_world")
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    rg = c.rays_gpu(gpu)
    with torch.no_grad():
        d = r.render_distortion(tree.features, rg)[:, 0]
        torch.testing.assert_close(r.distortion_loss(tree.features, rg, reduction="none"), d, rtol=0, atol=0)
        torch.testing.assert_close(r.distortion_loss(tree.features, rg, reduction="sum"), d.sum(), rtol=0, atol=0)
        torch.testing.assert_close(r.distortion_loss(tree.features, rg), d.mean(), rtol=0, atol=0)
    with pytest.raises(ValueError, match="reduction must be"):
        r.distortion_loss(tree.features, rg, reduction="max")
    tree.features.grad = None
    loss = r.distortion_loss(tree.features, rg, reduction="mean")
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    got = tree.features.grad.cpu().numpy()
    g = np.zeros((c.Q, 2), dtype=np.float32)
    g[:, 0] = np.float32(1.0) / np.float32(c.Q)      # what torch hands the operator for a mean
    opt = c.oracle_opts()
    assert_grads_close(got, R.distortion_grad(ot, rays, opt, g), R.distortion_grad_scale(ot, rays, opt, g))
    assert (got[:, -1] != 0).sum() > 500 and np.all(got[:, :-1] == 0)


def test_camera_form(gpu):
    c, _, _ = built("d5_sh4_world")
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    pose = torch.from_numpy(synth.camera_pose(radius=3.0, center=(0.1, -0.2, 0.3))).float().to(gpu).contiguous()
    cam = _make_camera_spec(pose, 72, 40, 90.0, 90.0)
    spec, opt = tree._spec(tree.features), r._get_options()
    with torch.no_grad():
        out = _C.distortion(spec, cam, opt)
    assert out.shape == (72 * 40, 2) and torch.isfinite(out).all()
    assert (out[:, 0] > 0).sum() > 300 and (out[:, 0] >= 0).all() and (out[out[:, 1] == 0] == 0).all()
    g = torch.ones(72 * 40, 2, device=gpu)
    grad = _C.distortion_backward(spec, cam, opt, g)
    assert grad.shape == tree.features.shape and torch.isfinite(grad).all() and (grad[:, :-1] == 0).all()
    assert (grad[:, -1] != 0).sum() > 100
