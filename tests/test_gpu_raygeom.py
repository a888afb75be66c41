"""Sample faces, sample_geometry and sample_weights(length=) on the GPU against the restatement (tests/raygeom_restate.py):
the face bytes and the two float32 backward sequences bit for bit, the gradients against the float64 yardstick within
the derived bounds, and the pose-refinement chain from c2w to a loss and back."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
from svox_t_amd.renderer import pinhole_rays
from tests import raygeom_restate as G
from tests import samples_restate as R
from tests.test_raygeom_host import CASES, built, random_upstream, worst

pytestmark = pytest.mark.gpu


def gpu_lists(s):
    return R.Lists(*(x.cpu().numpy() for x in (s.offsets, s.row, s.ray, s.depth, s.length)))


def assert_same_lists(got: R.Lists, want: R.Lists):
    for name in R.Lists._fields:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)


def on_gpu(F: G.FaceLists, gpu, face=True):
    L = F.lists
    t = [torch.from_numpy(x).to(gpu) for x in (L.offsets, L.ray, L.row, L.depth, L.length)]
    return svox.RaySamples(*t, torch.from_numpy(F.face).to(gpu) if face else None)


def geometry_grads(s, rays_np, gpu, gD, gL):
    """grad_origins / grad_dirs of sum(gD * depth) + sum(gL * length) through svox.sample_geometry (None: that output is
    left out of the loss, the kernel's null pointer)."""
    o = torch.from_numpy(rays_np[0]).to(gpu).requires_grad_(True)
    d = torch.from_numpy(rays_np[1]).to(gpu).requires_grad_(True)
    depth, length = svox.sample_geometry(s, svox.Rays(o, d, d))
    assert torch.equal(depth, s.depth) and torch.equal(length, s.length) and depth.requires_grad and length.requires_grad
    outs, grads = [], []
    if gD is not None:
        outs.append(depth)
        grads.append(torch.from_numpy(gD).to(gpu))
    if gL is not None:
        outs.append(length)
        grads.append(torch.from_numpy(gL).to(gpu))
    torch.autograd.backward(outs, grads)
    return o.grad.cpu().numpy(), d.grad.cpu().numpy()


def check_backward(b, F, s, gpu, seed, levels=0):
    """The backward of `s` (the lists F on the GPU): the restatement's float32 sequence bit for bit, the float64 yardstick
    within the derived bound, twice the same bits -- with both upstream gradients and with each alone."""
    T = len(F.face)
    gD, gL = random_upstream(T, seed)
    n = np.diff(F.lists.offsets)
    for gd_, gl_ in ((gD, gL), (gD, None), (None, gL)):
        go, gd = geometry_grads(s, b.rays, gpu, gd_, gl_)
        go32, gd32 = G.geometry_backward32(F, b.rays[1], gd_, gl_)
        assert go.dtype == np.float32 and go.shape == (b.Q, 3) == gd.shape
        np.testing.assert_array_equal(go.view(np.uint32), go32.view(np.uint32))
        np.testing.assert_array_equal(gd.view(np.uint32), gd32.view(np.uint32))
        assert not go[n == 0].any() and not gd[n == 0].any()
        go64, gd64 = G.geometry_grad64(F, b.rays[0], b.rays[1], gd_, gl_)
        bo, bd = G.geometry_bound(F, b.rays[1], gd_, gl_, float(b.opt.step_size), b.ot.offset, N=b.ot.N, levels=levels)
        ro, rd = worst(go, go64, bo), worst(gd, gd64, bd)
        print(f"worst |err| / bound: origins {ro:.3f}, dirs {rd:.3f}")
        assert ro <= 1 and rd <= 1
        again = geometry_grads(s, b.rays, gpu, gd_, gl_)
        np.testing.assert_array_equal(again[0].view(np.uint32), go.view(np.uint32))
        np.testing.assert_array_equal(again[1].view(np.uint32), gd.view(np.uint32))
    assert (go != 0).sum() > 20


# faces parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_sigma", [None, 0.0])
@pytest.mark.parametrize("name", ["d5_rgba4", "d5_sh4_world", "n3", "mixed", "hostile"])
def test_faces_parity(gpu, name, min_sigma):
    """face against the restatement byte for byte; the other five arrays are those of faces=False, array for array.
    n3: the generic descent; mixed: 65 + 1 rays with origins inside the cube (entry 3), two zero direction components and
    rays that miss; hostile: random_tree / random_rays of tests/test_adversarial_host.py."""
    b = built(name)
    r = b.renderer(gpu)
    rg = b.rays_on(gpu)
    s = r.ray_samples(rg, min_sigma=min_sigma, faces=True)
    plain = r.ray_samples(rg, min_sigma=min_sigma)
    F = b.faces(min_sigma)
    assert plain.face is None and s.face.dtype == torch.uint8 and s.face.shape == (len(s),) and s.face.device == s.ray.device
    assert_same_lists(gpu_lists(s), gpu_lists(plain))
    assert_same_lists(gpu_lists(s), F.lists)
    np.testing.assert_array_equal(s.face.cpu().numpy(), F.face)
    assert len(s) > 50
    if name in ("mixed", "hostile"):
        assert ((F.face & 3) == 3).sum() >= 5 and (np.diff(F.lists.offsets) == 0).sum() >= 8
    # the backward of these very lists
    if min_sigma == 0.0:
        check_backward(b, F, s, gpu, seed=5, levels=3 if name == "n3" else 0)


@pytest.mark.parametrize("name", ["d5_rgba4_48x40", "d5_rgba4_50x34"])
def test_lane_assignment_changes_nothing(gpu, name):
    b = built(name)
    r = b.renderer(gpu)
    rg = b.rays_on(gpu)
    H, W = CASES[name]["height"], CASES[name]["width"]
    F = b.faces(0.0)
    for kw in (dict(image_shape=(H, W)), dict(), dict(sort_rays=True), dict(sort_rays=False)):
        s = r.ray_samples(rg, min_sigma=0.0, faces=True, **kw)
        assert_same_lists(gpu_lists(s), F.lists)
        np.testing.assert_array_equal(s.face.cpu().numpy(), F.face)
    assert len(F.face) > 1000


def test_no_rays_and_rays_that_all_miss(gpu):
    b = built("d5_rgba4")
    r = b.renderer(gpu)
    Q = 70
    o = torch.full((Q, 3), 5.0, device=gpu, requires_grad=True)
    d = (torch.rand(Q, 3, device=gpu) + 0.1).requires_grad_(True)           # away from the cube
    s = r.ray_samples(svox.Rays(o, d, d), faces=True)
    assert len(s) == 0 and s.face.shape == (0,) and s.face.dtype == torch.uint8
    depth, length = svox.sample_geometry(s, svox.Rays(o, d, d))
    w, alpha = svox.sample_weights(s, torch.zeros(0, device=gpu), length=length)
    (depth.sum() + length.sum() + alpha.sum() + w.sum()).backward()
    assert o.grad.shape == (Q, 3) and not o.grad.any() and not d.grad.any()
    s0 = r.ray_samples(svox.Rays(o[:0].detach(), d[:0].detach(), d[:0].detach()), faces=True)
    assert s0.Q == 0 and len(s0) == 0 and s0.face.shape == (0,)


# select, split, merge ------------------------------------------------------------------------------------------------
def test_select_carries_face_and_split_and_merge_drop_it(gpu):
    b = built("d5_sh4_world")
    F = b.faces(0.0)
    s = on_gpu(F, gpu)
    keep = torch.from_numpy(np.random.default_rng(9).uniform(size=len(s)) < 0.6).to(gpu)
    sub, index = s.select(keep)
    assert torch.equal(sub.face, s.face[index]) and 0 < len(sub) < len(s)
    Fs = G.subset(F, index.cpu().numpy())
    assert_same_lists(gpu_lists(sub), Fs.lists)
    check_backward(b, Fs, sub, gpu, seed=6)
    plain_sub, _ = on_gpu(F, gpu, face=False).select(keep)
    assert plain_sub.face is None
    rays = b.rays_on(gpu)
    fine, _ = s.split(max_length=0.01)
    merged, _, _ = svox.merge_samples(s, s)
    for lists in (fine, merged, plain_sub):
        assert lists.face is None
        with pytest.raises(RuntimeError, match="carry no `face`.*not leaf faces"):
            svox.sample_geometry(lists, rays)


# sample_weights(length=) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("holes", [False, True])
def test_sample_weights_with_length(gpu, holes):
    """length = samples.length: the bits of the call without it, forward and grad_sigma.  Any other length: the forward
    is the restatement's float32 sequence, grad_length its second output bit for bit and within 1e-5 of the tight scale of
    float64 autograd (grad_sigma's tolerance); grad_sigma keeps the bits of the plain backward; twice the same bits."""
    F = built("d5_rgba4").faces()
    L = F.lists
    T, Q = L.row.shape[0], len(L.offsets) - 1
    s = on_gpu(F, gpu)
    rng = np.random.default_rng(21)
    sigma = rng.exponential(20.0, T).astype(np.float32) + np.float32(1e-3)
    if holes:
        sigma[::5] = 0
        sigma[2::11] = -1.5
    gw, ga = rng.standard_normal(T).astype(np.float32), rng.standard_normal(Q).astype(np.float32)
    tg = lambda x: torch.from_numpy(x).to(gpu)                                   # noqa: E731

    def run(length, w_, a_, plain=False):
        sg = tg(sigma).requires_grad_(True)
        ln = None if plain else tg(length).requires_grad_(True)
        w, alpha = svox.sample_weights(s, sg) if plain else svox.sample_weights(s, sg, length=ln)
        outs = [x for x, g in ((w, w_), (alpha, a_)) if g is not None]
        torch.autograd.backward(outs, [tg(g) for g in (w_, a_) if g is not None])
        return (w.detach().cpu().numpy(), alpha.detach().cpu().numpy(), sg.grad.cpu().numpy(), None if plain else ln.grad.cpu().numpy())

    other = (L.length * rng.uniform(0.5, 1.5, T)).astype(np.float32)
    for w_, a_ in ((gw, ga), (gw, None), (None, ga)):
        w0, a0, gs0, _ = run(None, w_, a_, plain=True)
        w1, a1, gs1, gl1 = run(L.length, w_, a_)
        for x, y in ((w0, w1), (a0, a1), (gs0, gs1)):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
        for length in (L.length, other):
            w, alpha, gs, gl = run(length, w_, a_)
            w32, a32 = R.weights(length, sigma, L.offsets, torch.float32)
            np.testing.assert_array_equal(w, w32.numpy())
            np.testing.assert_array_equal(alpha, a32.numpy())
            gs32, gl32 = G.weights_backward32(length, sigma, L.offsets, w_, a_)
            np.testing.assert_array_equal(gl.view(np.uint32), gl32.view(np.uint32))
            np.testing.assert_array_equal(gs.view(np.uint32), gs32.view(np.uint32))
            l64 = torch.from_numpy(length).double().requires_grad_(True)
            s64 = torch.from_numpy(sigma).double().requires_grad_(True)
            w64, a64 = G.weights64(l64, s64, L.offsets)
            loss = 0.0 * l64.sum()
            if w_ is not None:
                loss = loss + (w64 * torch.from_numpy(w_).double()).sum()
            if a_ is not None:
                loss = loss + (a64 * torch.from_numpy(a_).double()).sum()
            loss.backward()
            rl = worst(gl, l64.grad.numpy(), 1e-5 * G.grad_length_scale(length, sigma, L.offsets, w_, a_))
            rs = worst(gs, s64.grad.numpy(), 1e-5 * R.grad_sigma_scale(length, sigma, L.offsets, w_, a_))
            print(f"worst |err| / bound: grad_length {rl:.3f}, grad_sigma {rs:.3f}")
            assert rl <= 1 and rs <= 1 and (gl != 0).sum() > 1000 and np.all((sigma > 0) | (gl == 0))
            again = run(length, w_, a_)
            np.testing.assert_array_equal(again[2].view(np.uint32), gs.view(np.uint32))
            np.testing.assert_array_equal(again[3].view(np.uint32), gl.view(np.uint32))
    # length alone needs a gradient
    ln = tg(other).requires_grad_(True)
    w, alpha = svox.sample_weights(s, tg(sigma), length=ln)
    torch.autograd.backward([w, alpha], [tg(gw), tg(ga)])
    np.testing.assert_array_equal(ln.grad.cpu().numpy().view(np.uint32), G.weights_backward32(other, sigma, L.offsets, gw, ga)[1].view(np.uint32))


# the chain -----------------------------------------------------------------------------------------------------------
def test_pose_refinement_chain(gpu):
    """pinhole_rays(c2w) -> ray_samples(faces=True) -> sample_geometry -> sample_weights(sigma, length=) ->
    accumulate(w, depth) -> loss.backward(): c2w.grad against the float64 yardstick chained through the same torch code.

    The bound, propagated: per ray the derived bound of the geometry gradient for the float64 chain's own upstream
    gradients (raygeom_restate.geometry_bound), plus what the float32 upstream gradients may be off by, through the
    gradient's linearity (geometry_tight) -- g_length by 1e-5 of its tight scale (sample_weights' tolerance), g_depth =
    g_q w_k by |g_q| (1e-5 w_k + 1e-6) (the forward tolerance of w) --, then through pinhole_rays: origins are c2w's last
    column (the bounds add up over the rays), dirs = R (X, Y, Z) (they add up times |X|, |Y|, |Z|), and the float32 sums
    over the Q rays are priced at Q 2^-24 of the sums of the absolute values of their terms, whatever their order."""
    from svox_t_amd import synth
    name = "d5_rgba4_48x40"
    b = built(name)
    H, W = CASES[name]["height"], CASES[name]["width"]
    pose = synth.camera_pose(azimuth_deg=30.0, radius=1.6)
    fx = fy = 0.5 * W / np.tan(0.5 * 0.6911)
    r = b.renderer(gpu)
    rng = np.random.default_rng(31)
    g, ga = rng.standard_normal(W * H).astype(np.float32), rng.standard_normal(W * H).astype(np.float32)

    def chain():
        c2w = torch.from_numpy(pose.astype(np.float32)).to(gpu).requires_grad_(True)
        o, d, v = pinhole_rays(c2w, W, H, fx, fy)
        rays = svox.Rays(o, d, v)
        s = r.ray_samples(rays, min_sigma=0.0, faces=True)
        depth, length = svox.sample_geometry(s, rays)
        sigma = r.tree.features.detach()[s.row.long(), -1]
        w, alpha = svox.sample_weights(s, sigma, length=length)
        out = svox.accumulate(s, w, depth[:, None])
        ((out[:, 0] * torch.from_numpy(g).to(gpu)).sum() + (alpha * torch.from_numpy(ga).to(gpu)).sum()).backward()
        return c2w, (o, d, v), s

    c2w, (o, d, v), s = chain()
    assert torch.equal(chain()[0].grad, c2w.grad)                 # twice the same bits
    got = c2w.grad.cpu().numpy()
    assert got.shape == pose.shape and np.isfinite(got).all() and len(s) > 1000

    # the yardstick: the same rays (their float32 numbers) through the restated march, then float64 all the way
    rays_np = (o.detach().cpu().numpy(), d.detach().cpu().numpy(), v.detach().cpu().numpy())
    F = G.lists_with_faces(b.ot, rays_np, b.opt, 0.0)
    assert_same_lists(gpu_lists(s), F.lists)
    np.testing.assert_array_equal(s.face.cpu().numpy(), F.face)
    L = F.lists
    c64 = torch.from_numpy(pose.astype(np.float32)).double().requires_grad_(True)
    o64, d64, _ = pinhole_rays(c64, W, H, fx, fy)
    o64.retain_grad()
    d64.retain_grad()
    depth64, length64 = G.geometry64(F, o64, d64, anchored=True)
    depth64.retain_grad()
    length64.retain_grad()
    sig64 = torch.from_numpy(b.ot.features[L.row, -1]).double()
    w64, a64 = G.weights64(length64, sig64, L.offsets)
    out64 = R.accumulate(w64 * depth64, None, L.offsets, torch.float64)
    ((out64 * torch.from_numpy(g).double()).sum() + (a64 * torch.from_numpy(ga).double()).sum()).backward()
    want = c64.grad.numpy()

    gD, gL = depth64.grad.numpy(), length64.grad.numpy()
    bo, bd = G.geometry_bound(F, rays_np[1], gD, gL, float(b.opt.step_size), b.ot.offset)
    gq = np.abs(g.astype(np.float64))[L.ray]
    dD = gq * (1e-5 * w64.detach().numpy() + 1e-6)
    # g_length comes from sample_weights (grad_w = g_q depth_k, grad_alpha = ga) and g_depth's error enters gz_in too
    dL = 1e-5 * G.grad_length_scale(L.length, b.ot.features[L.row, -1], L.offsets, gq * L.depth.astype(np.float64), ga)
    lo, ld = G.geometry_tight(F, rays_np[1], dD + dL, dL)
    bo, bd = bo + lo, bd + ld
    Q = W * H
    xyz = np.abs(np.linalg.solve(pose[:3, :3].astype(np.float64), rays_np[1].astype(np.float64).T).T)      # |X|, |Y|, |Z| per ray
    go_abs, gd_abs = np.abs(o64.grad.numpy()), np.abs(d64.grad.numpy())
    bound = np.zeros_like(want)
    bound[:, 3] = bo.sum(0) + Q * G.U * go_abs.sum(0)
    bound[:, :3] = np.einsum("qi,qj->ij", bd, xyz) + Q * G.U * np.einsum("qi,qj->ij", gd_abs, xyz)
    ratio = np.abs(got - want) / bound
    print("c2w.grad:\n", got, "\nfloat64:\n", want, "\n|err| / bound:\n", ratio)
    assert np.all(ratio <= 1) and np.all(np.abs(want) > 0)
    # the bound is a small part of the gradient's own addends, so the comparison says something
    tight = np.zeros_like(want)
    tight[:, 3] = go_abs.sum(0)
    tight[:, :3] = np.einsum("qi,qj->ij", gd_abs, xyz)
    assert np.all(bound <= 2e-2 * tight)

    # points(geometry=) on the same graph: differentiable down to c2w, plain torch
    c2 = torch.from_numpy(pose.astype(np.float32)).to(gpu).requires_grad_(True)
    o2, d2, v2 = pinhole_rays(c2, W, H, fx, fy)
    rays2 = svox.Rays(o2, d2, v2)
    pts = s.points(rays2, "mid", geometry=svox.sample_geometry(s, rays2))
    assert torch.equal(pts.detach(), s.points(rays2, "mid")) and pts.requires_grad
    pts.sum().backward()
    assert c2.grad is not None and torch.isfinite(c2.grad).all() and c2.grad.abs().sum() > 0
