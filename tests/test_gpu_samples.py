"""The per-sample interface on the GPU: ray_samples against the restatement's lists (tests/samples_restate.py), and
sample_weights / accumulate against its float32 sequence, its float64 autograd, and the operators they are tied to."""
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
from oracle import oracle as O
from svox_t_amd import synth
from tests import depth_restate as D
from tests import samples_restate as R
from tests.util import Case, assert_grads_close, assert_outputs_close

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")

CASES = {
    "d5_rgba4": dict(depth=5, K=4, data_format="RGBA", width=64, height=64),
    "d5_sh4_world": dict(depth=5, K=13, data_format="SH4", width=64, height=64,
                         radius=[1.0, 1.2, 0.8], center=[0.1, -0.2, 0.3]),           # delta_scale != 1
    "d5_rgba4_50x34": dict(depth=5, K=4, data_format="RGBA", width=50, height=34),
    "d5_rgba4_48x40": dict(depth=5, K=4, data_format="RGBA", width=48, height=40),
    "d6_sh9": dict(depth=6, K=28, data_format="SH9", width=96, height=96),
    "d8_rgba4": dict(depth=8, K=4, data_format="RGBA", width=64, height=64),
}
_BUILT = {}


def built(name):
    """(case, oracle tree, rays, options): one object each per case, so that the restatement's march is computed once."""
    if name not in _BUILT:
        c = Case(**CASES[name])
        _BUILT[name] = (c, c.oracle_tree(), c.rays_np(), c.oracle_opts())
    return _BUILT[name]


def lists_of(name, min_sigma=None):
    key = (name, min_sigma)
    if key not in _BUILT:
        c, ot, rays, opt = built(name)
        _BUILT[key] = R.lists(ot, rays, opt, min_sigma)
    return _BUILT[key]


def as_lists(s):
    return R.Lists(*(x.cpu().numpy() for x in (s.offsets, s.row, s.ray, s.depth, s.length)))


def on_gpu(L, gpu):
    return svox.RaySamples(*(torch.from_numpy(x).to(gpu) for x in (L.offsets, L.ray, L.row, L.depth, L.length)))


def assert_lists_equal(got, want):
    assert got.offsets.dtype == np.int64 and got.row.dtype == np.int32 and got.ray.dtype == np.int32
    assert got.depth.dtype == np.float32 and got.length.dtype == np.float32
    for name in R.Lists._fields:                       # (the floats too: the march is bit-exact)
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=name)


# parity of the lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_sigma", [None, 0.0])
@pytest.mark.parametrize("name", ["d5_rgba4", "d5_sh4_world"])
def test_lists_parity(gpu, name, min_sigma):
    c, ot, rays, opt = built(name)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    s = r.ray_samples(c.rays_gpu(gpu), min_sigma=min_sigma)
    want = lists_of(name, min_sigma)
    assert s.Q == c.Q and len(s) == want.row.shape[0] > 1000 and int(s.offsets[-1]) == len(s)
    assert_lists_equal(as_lists(s), want)
    np.testing.assert_array_equal(s.counts.cpu().numpy(), np.diff(want.offsets))
    if min_sigma is not None:
        assert len(s) < lists_of(name, None).row.shape[0]          # the filter drops something


def test_features_argument_feeds_the_filter(gpu):
    c, ot, rays, opt = built("d5_rgba4")
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    other = tree.features.detach().clone()
    other[::2, -1] = -1.0
    s = r.ray_samples(c.rays_gpu(gpu), features=other, min_sigma=0.0)
    ot2 = O.Tree(other.cpu().numpy(), c.st.data, c.st.child, offset=ot.offset, scaling=ot.scaling)
    assert_lists_equal(as_lists(s), R.lists(ot2, rays, opt, 0.0))
    # without min_sigma the table is not read
    assert_lists_equal(as_lists(r.ray_samples(c.rays_gpu(gpu), features=other)), lists_of("d5_rgba4"))


# lane assignment changes nothing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5_rgba4_50x34", "d5_rgba4_48x40"])
def test_lane_assignment_changes_nothing(gpu, name):
    """Declared an image (48 x 40: walked in 8 x 8 tiles; 50 x 34: its sides are no multiples of 8), undeclared, and in
    svoxt_ray_order's order: the same lists."""
    c, ot, rays, opt = built(name)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    rg = c.rays_gpu(gpu)
    H, W = CASES[name]["height"], CASES[name]["width"]
    want = lists_of(name, 0.0)
    for kw in (dict(image_shape=(H, W)), dict(), dict(sort_rays=True), dict(sort_rays=False)):
        assert_lists_equal(as_lists(r.ray_samples(rg, min_sigma=0.0, **kw)), want)
    assert want.row.shape[0] > 1000


# edge cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 65])
def test_tiny_batches(gpu, Q):
    c, ot, rays, opt = built("d5_rgba4")
    pick = (np.arange(Q) * 37 + 64 * 30 + 20) % 4096   # from the middle rows on: most of them meet the shell
    sub = tuple(np.ascontiguousarray(a[pick]) for a in rays)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    s = r.ray_samples(svox.Rays(*(torch.from_numpy(a).to(gpu) for a in sub)), min_sigma=0.0)
    want = R.lists(ot, sub, opt, 0.0)
    assert s.Q == Q and len(s) > 0
    assert_lists_equal(as_lists(s), want)
    sigma = tree.features.detach()[s.row.long(), -1]
    w, alpha = svox.sample_weights(s, sigma)
    w32, a32 = R.weights(want.length, ot.features[want.row, -1], want.offsets, torch.float32)
    np.testing.assert_array_equal(w.cpu().numpy(), w32.numpy())
    np.testing.assert_array_equal(alpha.cpu().numpy(), a32.numpy())


def test_rays_that_all_miss(gpu):
    c, _, _, _ = built("d5_rgba4")
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    Q = 200
    o = torch.full((Q, 3), 5.0, device=gpu)
    d = torch.nn.functional.normalize(torch.rand(Q, 3, device=gpu) + 0.1, dim=1).contiguous()     # away from the cube
    s = r.ray_samples(svox.Rays(o, d, d))
    assert s.Q == Q and len(s) == 0 and s.offsets.shape == (Q + 1,) and not s.offsets.any()
    assert s.row.shape == s.ray.shape == s.depth.shape == s.length.shape == (0,)
    sigma = torch.zeros(0, device=gpu, requires_grad=True)
    values = torch.zeros(0, 3, device=gpu, requires_grad=True)
    w, alpha = svox.sample_weights(s, sigma)
    out = svox.accumulate(s, w, values)
    assert w.shape == (0,) and alpha.shape == (Q,) and out.shape == (Q, 3) and svox.accumulate(s, w).shape == (Q,)
    assert not alpha.any() and not out.any()
    (out.sum() + alpha.sum()).backward()
    assert sigma.grad.shape == (0,) and values.grad.shape == (0, 3)
    s0 = r.ray_samples(svox.Rays(o[:0], d[:0], d[:0]))
    assert s0.Q == 0 and len(s0) == 0 and s0.offsets.tolist() == [0]


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
    rg = svox.Rays(o.to(gpu), d.to(gpu), v.to(gpu))
    for ms in (None, 0.0):
        want = R.lists(ot, rays, opt, ms)
        assert_lists_equal(as_lists(r.ray_samples(rg, min_sigma=ms)), want)
        assert want.row.shape[0] > 3000
    s = r.ray_samples(rg)
    with torch.no_grad():
        _, alpha = svox.sample_weights(s, tree.features[s.row.long(), -1])
    np.testing.assert_array_equal(alpha.cpu().numpy()[:, None], O.opacity_render(ot, *rays, opt))


@pytest.mark.parametrize("name,side,longest", [("d6_sh9", 96, 34), ("d8_rgba4", 64, 89)])
def test_long_rays(gpu, name, side, longest):
    """Lists longer than a wavefront's 64 lanes.  Depth 6 / SH9 at 96 x 96 was meant to have them and has not: its
    longest list holds 34 samples (the restatement's count, 33 with sigma > 0), so the case is kept for parity and the
    longer-than-64 condition is held on depth 8 at 64 x 64, whose longest list holds 89."""
    c, ot, rays, opt = built(name)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    s = r.ray_samples(c.rays_gpu(gpu), image_shape=(side, side))
    want = lists_of(name)
    assert int(s.counts.max()) == int(np.diff(want.offsets).max()) == longest
    if name == "d8_rgba4":
        assert longest > 64
    assert_lists_equal(as_lists(s), want)
    with torch.no_grad():
        w, alpha = svox.sample_weights(s, tree.features[s.row.long(), -1])
        m = svox.accumulate(s, w, torch.stack([s.depth, s.depth * s.depth], dim=1))
    w32, a32 = R.weights(want.length, ot.features[want.row, -1], want.offsets, torch.float32)
    np.testing.assert_array_equal(w.cpu().numpy(), w32.numpy())
    np.testing.assert_array_equal(alpha.cpu().numpy()[:, None], O.opacity_render(ot, *rays, opt))
    np.testing.assert_array_equal(m.cpu().numpy(), D.moments(ot, rays, opt, "entry", torch.float32).numpy()[:, :2])


# bit anchors on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_sigma", [None, 0.0])
@pytest.mark.parametrize("name", ["d5_rgba4", "d5_sh4_world"])
def test_bit_anchors_on_the_device(gpu, name, min_sigma):
    c, _, _, _ = built(name)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    rg = c.rays_gpu(gpu)
    with torch.no_grad():
        s = r.ray_samples(rg, min_sigma=min_sigma)
        w, alpha = svox.sample_weights(s, tree.features[s.row.long(), -1])
        m = svox.accumulate(s, w, torch.stack([s.depth, s.depth * s.depth], dim=1))
        opacity = r.opacity_render(tree.features, rg)
        moments = r.render_depth_moments(tree.features, rg, at="entry")
    np.testing.assert_array_equal(alpha.cpu().numpy()[:, None], opacity.cpu().numpy())
    np.testing.assert_array_equal(m.cpu().numpy(), moments.cpu().numpy()[:, :2])
    np.testing.assert_array_equal(alpha.cpu().numpy(), moments.cpu().numpy()[:, 2])
    assert (alpha > 0).sum() > 500 and (m[:, 0] > 0).sum() > 500


# operators against the restatement -------------------------------------------------------------------------------------
def random_sigma(T, seed, holes=False):
    rng = np.random.default_rng(seed)
    sigma = rng.exponential(20.0, T).astype(np.float32) + np.float32(1e-3)     # lengths are ~ 1 / 32: length * sigma ~ 0.6
    if holes:
        sigma[::5] = 0
        sigma[2::11] = -rng.exponential(3.0, sigma[2::11].shape[0]).astype(np.float32)
    return sigma


@pytest.mark.parametrize("holes", [False, True])
def test_sample_weights_against_the_restatement(gpu, holes):
    """Forward: the float32 sequence, bit for bit.  grad_sigma: the float64 autograd to 1e-5 of the tight scale (the sum of
    the absolute values of its addends).  holes: every fifth sigma is 0, some are negative -- w = 0, no gradient."""
    L = lists_of("d5_rgba4")
    T, Q = L.row.shape[0], len(L.offsets) - 1
    s = on_gpu(L, gpu)
    sigma = random_sigma(T, 21, holes)
    rng = np.random.default_rng(22)
    gw = rng.standard_normal(T).astype(np.float32)
    ga = rng.standard_normal(Q).astype(np.float32)
    sg = torch.from_numpy(sigma).to(gpu).requires_grad_(True)
    w, alpha = svox.sample_weights(s, sg)
    w32, a32 = R.weights(L.length, sigma, L.offsets, torch.float32)
    np.testing.assert_array_equal(w.detach().cpu().numpy(), w32.numpy())
    np.testing.assert_array_equal(alpha.detach().cpu().numpy(), a32.numpy())
    torch.autograd.backward([w, alpha], [torch.from_numpy(gw).to(gpu), torch.from_numpy(ga).to(gpu)])
    got = sg.grad.cpu().numpy()
    s64 = torch.from_numpy(sigma).double().requires_grad_(True)
    w64, a64 = R.weights(L.length, s64, L.offsets, torch.float64)
    ((w64 * torch.from_numpy(gw).double()).sum() + (a64 * torch.from_numpy(ga).double()).sum()).backward()
    want = s64.grad.numpy()
    tight = R.grad_sigma_scale(L.length, sigma, L.offsets, gw, ga)
    ratio = np.abs(got - want)[tight > 0] / (1e-5 * tight[tight > 0])
    print("grad_sigma: worst |err| / bound", ratio.max(), "entries", ratio.size)
    assert_grads_close(got, want, tight)
    assert (got != 0).sum() > 1000 and np.all((sigma > 0) == (tight > 0))
    # a gradient through one output alone
    for only in (0, 1):
        sg.grad = None
        w, alpha = svox.sample_weights(s, sg)
        (w * torch.from_numpy(gw).to(gpu)).sum().backward() if only == 0 else (alpha * torch.from_numpy(ga).to(gpu)).sum().backward()
        part = R.grad_sigma_scale(L.length, sigma, L.offsets, gw if only == 0 else None, ga if only == 1 else None)
        s64.grad = None
        w64, a64 = R.weights(L.length, s64, L.offsets, torch.float64)
        ((w64 * torch.from_numpy(gw).double()).sum() if only == 0 else (a64 * torch.from_numpy(ga).double()).sum()).backward()
        assert_grads_close(sg.grad.cpu().numpy(), s64.grad.numpy(), part)


@pytest.mark.parametrize("C", [1, 3, 7])
def test_accumulate_against_the_restatement(gpu, C):
    """Forward: acc += w * v in list order, bit for bit.  grad_w (a sum of C products of numbers in [-1, 1]: rounding
    below C * 2^-24 * C, far inside assert_outputs_close's 1e-6) and grad_values (one product) against float64."""
    L = lists_of("d5_rgba4")
    T, Q = L.row.shape[0], len(L.offsets) - 1
    s = on_gpu(L, gpu)
    w32, _ = R.weights(L.length, random_sigma(T, 23), L.offsets, torch.float32)
    rng = np.random.default_rng(24 + C)
    values = rng.uniform(-1, 1, (T, C)).astype(np.float32)
    g = rng.uniform(-1, 1, (Q, C)).astype(np.float32)
    wg = w32.to(gpu).requires_grad_(True)
    vg = torch.from_numpy(values).to(gpu).requires_grad_(True)
    out = svox.accumulate(s, wg, vg)
    assert out.shape == (Q, C)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), R.accumulate(w32, values, L.offsets, torch.float32).numpy())
    out.backward(torch.from_numpy(g).to(gpu))
    w64 = w32.double().requires_grad_(True)
    v64 = torch.from_numpy(values).double().requires_grad_(True)
    (R.accumulate(w64, v64, L.offsets, torch.float64) * torch.from_numpy(g).double()).sum().backward()
    assert_outputs_close(wg.grad.cpu().numpy(), w64.grad.numpy(), what="grad_w")
    assert_outputs_close(vg.grad.cpu().numpy(), v64.grad.numpy(), what="grad_values")
    assert (wg.grad != 0).sum() > 1000 and (vg.grad != 0).sum() > 1000
    if C == 1:                                         # without values: the plain sum of w, and its gradient
        wg.grad = None
        plain = svox.accumulate(s, wg)
        assert plain.shape == (Q,)
        np.testing.assert_array_equal(plain.detach().cpu().numpy(), R.accumulate(w32, None, L.offsets, torch.float32).numpy())
        plain.backward(torch.from_numpy(g[:, 0].copy()).to(gpu))
        np.testing.assert_array_equal(wg.grad.cpu().numpy(), g[L.ray, 0])


# end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5_rgba4", "d5_sh4_world"])
def test_end_to_end_gradient_is_the_depth_moments(gpu, name):
    c, ot, rays, opt = built(name)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    g = synth.grad_output(c.Q, 3, seed=31).numpy()
    gt = torch.from_numpy(g).to(gpu)
    s = r.ray_samples(c.rays_gpu(gpu), min_sigma=0.0)
    tree.features.grad = None
    sigma = tree.features[s.row.long(), -1]
    out, alpha, w = svox.composite(s, sigma, torch.stack([s.depth, s.depth * s.depth], dim=1))
    assert out.shape == (c.Q, 2) and alpha.shape == (c.Q,) and w.shape == (len(s),)
    ((out * gt[:, :2]).sum() + (alpha * gt[:, 2]).sum()).backward()
    got = tree.features.grad.cpu().numpy()
    want, scale = D.moments_grad(ot, rays, opt, "entry", g), D.moments_grad_scale(ot, rays, opt, "entry", g)
    ratio = np.abs(got - want)[scale > 0] / (1e-5 * scale[scale > 0])
    print(name, "worst |err| / bound", ratio.max(), "entries", ratio.size)
    assert_grads_close(got, want, scale)
    assert np.all(got[:, :-1] == 0) and (got[:, -1] != 0).sum() > 500


# determinism -----------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(gpu):
    c, _, _, _ = built("d5_sh4_world")
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    rg = c.rays_gpu(gpu)
    runs = []
    for _ in range(2):
        s = r.ray_samples(rg, min_sigma=0.0)
        sigma = torch.from_numpy(random_sigma(len(s), 41)).to(gpu).requires_grad_(True)
        values = torch.from_numpy(np.random.default_rng(42).uniform(-1, 1, (len(s), 3)).astype(np.float32)).to(gpu)
        out, alpha, w = svox.composite(s, sigma, values)
        g = torch.from_numpy(np.random.default_rng(43).uniform(-1, 1, (c.Q, 4)).astype(np.float32)).to(gpu)
        ((out * g[:, :3]).sum() + (alpha * g[:, 3]).sum()).backward()
        runs.append([x.detach().cpu().numpy() for x in (s.offsets, s.row, s.ray, s.depth, s.length, w, out, alpha, sigma.grad)])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    assert (runs[0][-1] != 0).sum() > 1000


# a derived per-row statistic -------------------------------------------------------------------------------------------
def test_per_row_maximum_weight(gpu):
    """What prune(weights=) and subdivide(weights=) want: the largest compositing weight every feature row received."""
    name = "d5_rgba4"
    c, ot, rays, opt = built(name)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    with torch.no_grad():
        s = r.ray_samples(c.rays_gpu(gpu), min_sigma=0.0)
        w, _ = svox.sample_weights(s, tree.features[s.row.long(), -1])
        got = torch.zeros(tree.features.shape[0], device=gpu).index_reduce_(0, s.row.long(), w, "amax", include_self=True)
    L = lists_of(name, 0.0)
    w32, _ = R.weights(L.length, ot.features[L.row, -1], L.offsets, torch.float32)
    want = np.zeros(ot.M, dtype=np.float32)
    np.maximum.at(want, L.row, w32.numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert (want > 0).sum() > 500
