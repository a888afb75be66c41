"""The deterministic render backward on the GPU (VolumeRenderer.forward / opacity_render with deterministic=True): its
bits against the restatement (tests/rowgrad_restate.py), the oracle's tolerance, the same bits on every route, the long
rows' kernels, "every element written", the opacity backward, the edges and the public surface."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from tests import depth_restate as D
from tests import rowgrad_restate as RG
from tests.util import assert_grads_close

pytestmark = pytest.mark.gpu
_BUILT = {}


class Scene:
    """A tree, its oracle twin, W x H rays from outside the cube (wide enough that the corner rays miss it) and an
    upstream gradient; everything is built once per name."""

    def __init__(self, fmt, K, depth=4, W=32, H=32, n3=False, lobes=None, comp=None, fx=None, seed=0):
        df = svox.DataFormat(fmt)
        self.fmt, self.K, self.W, self.H, self.Q = fmt, K, W, H, W * H
        self.comp = comp
        self.lobes = lobes
        if n3:
            self.cpu_tree, self.features = full_tree(3, 2, K, occupied=0.35, seed=seed, fmt=fmt)
        else:
            st = synth.shell_tree(depth)
            self.features = synth.shell_features(st.n_features, K, seed=seed)
            self.cpu_tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, self.features, data_format=fmt,
                                                    extra_data=lobes)
        t = self.cpu_tree
        n = t.n_internal
        self.ot = O.Tree(self.features.numpy(), t.data[:n].numpy(), t.child[:n].numpy(), offset=t.offset.numpy(),
                         scaling=t.invradius.numpy(), extra=None if lobes is None else lobes.numpy())
        kw = {} if comp is None else dict(min_comp=comp[0], max_comp=comp[1])
        self.opt = O.make_options(format=df.format, basis_dim=df.basis_dim, **kw)
        o, d, v = synth.pinhole_rays(W, H, c2w=synth.camera_pose(), fx=(1.0 * W if fx is None else fx))
        self.rays = (o.numpy(), d.numpy(), v.numpy())
        self.C = O.out_data_dim(self.opt, K) - 1
        self.g = synth.grad_output(self.Q, self.C + 1).numpy()
        self._want = {}

    def renderer(self, gpu):
        tree = self.cpu_tree.to(gpu)
        kw = {} if self.comp is None else dict(min_comp=self.comp[0], max_comp=self.comp[1])
        return svox.VolumeRenderer(tree, **kw)

    def rays_gpu(self, gpu):
        return svox.Rays(*(torch.from_numpy(a).to(gpu) for a in self.rays))

    def restated(self, opacity=False):
        if opacity not in self._want:
            self._want[opacity] = RG.grad(self.ot, self.rays, self.opt, self.g[:, -1:] if opacity else self.g)
        return self._want[opacity]

    def grad(self, gpu, features=None, opacity=False, **kw):
        """The deterministic gradient of sum(out * g) on the GPU, float32 [M, K] torch."""
        r = self.renderer(gpu)
        f = (self.features if features is None else features).to(gpu).requires_grad_(True)
        rays = self.rays_gpu(gpu)
        if opacity:
            out = r.opacity_render(f, rays, deterministic=True, **kw)
            out.backward(torch.from_numpy(self.g[:, -1:].copy()).to(gpu))
        else:
            out = r(f, rays, deterministic=True, **kw)
            out.backward(torch.from_numpy(self.g).to(gpu))
        return f.grad


def full_tree(N, levels, K, occupied=1.0, rows=None, seed=0, fmt="RGBA"):
    """A full tree of `levels` refinements; a leaf is occupied with probability `occupied` and names a row of its own, or
    leaf index % rows."""
    t = svox.N3Tree(N=N, data_dim=K, init_reserve=8, data_format=fmt)
    for _ in range(levels):
        t.refine(1)
    leaves = t._all_leaves()
    g = torch.Generator().manual_seed(seed)
    occ = torch.rand(len(leaves), generator=g) < occupied
    idx = torch.full((len(leaves),), synth.EMPTY_SENTINEL, dtype=torch.int32)
    n = int(occ.sum())
    idx[occ] = torch.arange(n, dtype=torch.int32) if rows is None else torch.arange(n, dtype=torch.int32) % rows
    t.data[tuple(leaves.T)] = idx[:, None]
    return t, synth.shell_features(n if rows is None else rows, K, seed=seed)


def _lobes(kind, B):
    g = torch.Generator().manual_seed(4)
    if kind == "SG":
        return torch.cat([torch.rand(B, 1, generator=g) * 4 + 0.5, torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)], -1)
    raise ValueError(kind)


CONFIG1_FX = 1111.111 * 64 / 800.0          # the pinhole of tests.util.Case at 64 pixels
SCENES = {
    "rgba4": lambda: Scene("RGBA", 4),
    "sh9": lambda: Scene("SH9", 28),
    "sh4_sub": lambda: Scene("SH4", 13, comp=(1, 2)),
    "rgba32": lambda: Scene("RGBA", 32),
    "sg6": lambda: Scene("SG6", 19, lobes=_lobes("SG", 6)),
    "n3_rgba4": lambda: Scene("RGBA", 4, n3=True),
    "n3_sh4": lambda: Scene("SH4", 13, n3=True),
    # the oracle's shapes: the D = 5 shell tree, 64 x 64 rays
    "d5_sh9": lambda: Scene("SH9", 28, depth=5, W=64, H=64, fx=CONFIG1_FX),
    "d5_rgba4": lambda: Scene("RGBA", 4, depth=5, W=64, H=64, fx=CONFIG1_FX),
    # a row of 13 floats for three channels of four: column 12 belongs to no channel
    "sh4_gap": lambda: Scene("SH4", 14, comp=(1, 2)),
}


def scene(name):
    if name not in _BUILT:
        _BUILT[name] = SCENES[name]()
    return _BUILT[name]


def tight(s, g):
    key = ("tight", s, g.shape[1])
    if key not in _BUILT:
        _BUILT[key] = O.volume_render_backward(s.ot, *s.rays, s.opt, g, want_abs="both")
    return _BUILT[key]


# 1. bits against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rgba4", "sh9", "sh4_sub", "rgba32", "sg6", "n3_rgba4", "n3_sh4"])
def test_bits_against_the_restatement(gpu, name):
    s = scene(name)
    m = D.march(s.ot, s.rays, s.opt)
    assert (~m.hit).any() and m.hit.any()                              # some rays miss the cube
    assert (s.features[:, -1] < 0).any()                               # and some rows are empty space
    got = s.grad(gpu).cpu().numpy()
    want = s.restated()
    assert got.dtype == np.float32 and got.shape == want.shape == (s.ot.M, s.K)
    assert np.count_nonzero(want) > 100
    np.testing.assert_array_equal(got, want)


# 2. the oracle's tolerance ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5_sh9", "d5_rgba4"])
def test_oracle_tolerance(gpu, name):
    s = scene(name)
    assert s.ot.M == 3344 and s.Q == 4096
    want, _absum, tg = tight(s, s.g)
    got = s.grad(gpu).cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print(f"{name}: worst |got - want| / (1e-5 tight) = {(err / (1e-5 * tg + 1e-300)).max():.3f}")
    assert np.all(err <= 1e-5 * tg)
    assert np.count_nonzero(want) > 1000


# 3. the same bits in every run and on every route ----------------------------------------------------------------------
def test_same_bits_in_every_run_and_on_every_route(gpu):
    s = scene("d5_sh9")
    first = s.grad(gpu)
    assert torch.equal(s.grad(gpu), first)
    for kw in (dict(sort_rays=True), dict(sort_rays=False), dict(image_shape=(s.H, s.W)), dict(fast=True), dict(fast=False)):
        assert torch.equal(s.grad(gpu, **kw), first), kw
    saved = _C.LIST_POOL, _C.FWD_LIST_SAMPLES
    try:
        _C.LIST_POOL, _C.FWD_LIST_SAMPLES = (not saved[0]), 8
        assert torch.equal(s.grad(gpu), first)
        assert torch.equal(s.grad(gpu, image_shape=(s.H, s.W)), first)
        _C.FWD_LIST_SAMPLES = 0
        assert torch.equal(s.grad(gpu), first)
    finally:
        _C.LIST_POOL, _C.FWD_LIST_SAMPLES = saved
    # and after the default, atomic route has run on the same tensors
    r = s.renderer(gpu)
    f = s.features.to(gpu).requires_grad_(True)
    r(f, s.rays_gpu(gpu)).backward(torch.from_numpy(s.g).to(gpu))
    assert torch.equal(s.grad(gpu), first)


# 4. the long rows ------------------------------------------------------------------------------------------------------
def test_long_rows_run_the_chunk_and_join_kernels(gpu):
    """A depth-2 full tree (64 leaves) whose data names 4 feature rows, 48 x 48 rays: thousands of samples a row."""
    if "long" not in _BUILT:
        t, feats = full_tree(2, 2, 4, rows=4, seed=3)
        feats[:, -1] = torch.tensor([0.5, 1.5, 0.25, 2.0])
        s = Scene.__new__(Scene)
        s.fmt, s.K, s.W, s.H, s.Q, s.comp, s.lobes = "RGBA", 4, 48, 48, 48 * 48, None, None
        s.cpu_tree, s.features = t, feats
        n = t.n_internal
        s.ot = O.Tree(feats.numpy(), t.data[:n].numpy(), t.child[:n].numpy(), offset=t.offset.numpy(), scaling=t.invradius.numpy())
        s.opt = O.make_options()
        s.rays = tuple(a.numpy() for a in synth.pinhole_rays(48, 48))
        s.C, s.g, s._want = 3, synth.grad_output(48 * 48, 4).numpy(), {}
        _BUILT["long"] = s
    s = _BUILT["long"]
    assert s.ot.M == 4
    got = s.grad(gpu).cpu().numpy()
    last = dict(_C._extras.ROWGRAD_LAST)
    assert last["longest"] > 512 and last["n_long"] == 4 and last["n_chunks"] >= 3 * 4, last    # chunk and join kernels ran
    np.testing.assert_array_equal(got, s.restated())
    assert np.all(got != 0)


# 5. every element written ----------------------------------------------------------------------------------------------
def test_every_element_written(gpu):
    s = scene("sh4_gap")
    K, M, stride = s.K, s.ot.M, s.K + 5
    r = s.renderer(gpu)
    f = s.features.to(gpu)
    spec = r.tree._spec(f)
    rspec = svox.renderer._rays_spec_from_rays(s.rays_gpu(gpu))
    buf = torch.full((M, stride), float("nan"), device=gpu)
    out = _C.volume_render_backward_rows(spec, rspec, r._get_options(), torch.from_numpy(s.g).to(gpu), grad=buf)
    assert out is buf
    got = buf.cpu().numpy()
    assert np.all(np.isfinite(got[:, :K])) and np.all(np.isnan(got[:, K:]))
    np.testing.assert_array_equal(got[:, :K], s.restated())
    con = RG.contributions(s.ot, s.rays, s.opt, s.g)
    untouched = np.ones(M, bool)
    untouched[con.row] = False
    assert untouched.sum() > M // 10 and not got[untouched, :K].any()               # (the sigma = -1 rows among them)
    outside = [c * 4 + i for c in range(3) for i in (0, 3)] + [12]                  # outside [min_comp, max_comp]; no channel's
    assert not got[:, outside].any() and np.all(np.signbit(got[:, outside]) == 0)
    inside = [c * 4 + i for c in range(3) for i in (1, 2)] + [K - 1]
    assert np.count_nonzero(got[~untouched][:, inside]) > 0.9 * (~untouched).sum() * len(inside)


# 6. C = 0 --------------------------------------------------------------------------------------------------------------
def test_opacity_backward(gpu):
    s = scene("d5_rgba4")
    got = s.grad(gpu, opacity=True).cpu().numpy()
    assert not got[:, :-1].any() and np.count_nonzero(got[:, -1]) > 1000
    np.testing.assert_array_equal(got, s.restated(opacity=True))
    want, _absum, tg = tight(s, np.ascontiguousarray(s.g[:, -1:]))
    err = np.abs(got.astype(np.float64) - want)
    print(f"opacity: worst |got - want| / (1e-5 tight) = {(err / (1e-5 * tg + 1e-300)).max():.3f}")
    assert np.all(err <= 1e-5 * tg)
    # the same bits whatever the walk
    assert np.array_equal(s.grad(gpu, opacity=True, image_shape=(s.H, s.W)).cpu().numpy(), got)


# 7. edges --------------------------------------------------------------------------------------------------------------
def test_no_rays(gpu):
    s = scene("rgba4")
    r = s.renderer(gpu)
    f = s.features.to(gpu).requires_grad_(True)
    e = torch.zeros(0, 3, device=gpu)
    spec = r.tree._spec(f)
    rspec = svox.renderer._rays_spec_from_rays(svox.Rays(e, e, e))
    grad = _C.volume_render_backward_rows(spec, rspec, r._get_options(), torch.zeros(0, 4, device=gpu))
    assert grad.shape == f.shape and not grad.any() and _C._extras.ROWGRAD_LAST["T"] == 0


def test_rays_that_all_miss(gpu):
    s = scene("sh9")
    r = s.renderer(gpu)
    f = s.features.to(gpu).requires_grad_(True)
    Q = 200
    o = torch.full((Q, 3), 5.0, device=gpu)
    d = torch.nn.functional.normalize(torch.rand(Q, 3, device=gpu) + 0.1, dim=1).contiguous()     # away from the cube
    out = r(f, svox.Rays(o, d, d), deterministic=True)
    out.backward(torch.ones_like(out))
    last = _C._extras.ROWGRAD_LAST
    assert last["Q"] == Q and last["T"] == 0 and last["bytes"] == 0          # nothing allocated, nothing launched over T
    assert f.grad.shape == f.shape and not f.grad.any()


def test_a_tree_without_density(gpu):
    s = scene("rgba4")
    feats = s.features.clone()
    feats[:, -1] = -feats[:, -1].abs()
    feats[::3, -1] = 0.0
    grad = s.grad(gpu, features=feats)
    assert _C._extras.ROWGRAD_LAST["T"] == 0 and not grad.any()


def test_one_ray_one_sample(gpu):
    """A root whose eight leaves hold one occupied leaf: the ray through it has one sample, and the entries of its row are
    the oracle's single float32 contributions exactly."""
    t = svox.N3Tree(N=2, data_dim=4, init_reserve=4)
    idx = torch.full((8,), synth.EMPTY_SENTINEL, dtype=torch.int32)
    idx[5] = 0
    t.data[0].view(-1)[:] = idx
    feats = torch.tensor([[0.4, -1.1, 0.2, 3.0]])
    n = t.n_internal
    ot = O.Tree(feats.numpy(), t.data[:n].numpy(), t.child[:n].numpy(), offset=t.offset.numpy(), scaling=t.invradius.numpy())
    # leaf 5 = (1, 0, 1): x in [.5, 1), y in [0, .5), z in [.5, 1); a ray along +x through it meets leaf (0, 0, 1) first (empty)
    o = np.array([[-1.0, 0.25, 0.75]], np.float32)
    d = np.array([[1.0, 0.0, 0.0]], np.float32)
    g = np.array([[0.5, -2.0, 1.5, 0.75]], np.float32)
    opt = O.make_options()
    want = O.volume_render_backward(ot, o, d, d, opt, g)
    assert np.all(want != 0)
    tg = t.to(gpu)
    r = svox.VolumeRenderer(tg)
    f = feats.to(gpu).requires_grad_(True)
    out = r(f, svox.Rays(*(torch.from_numpy(a).to(gpu) for a in (o, d, d))), deterministic=True)
    out.backward(torch.from_numpy(g).to(gpu))
    assert _C._extras.ROWGRAD_LAST["T"] == 1
    got = f.grad.cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.float64), want)
    np.testing.assert_array_equal(got, RG.grad(ot, (o, d, d), opt, g))


# 8. the surface --------------------------------------------------------------------------------------------------------
def test_surface(gpu):
    s = scene("d5_sh9")
    r = s.renderer(gpu)
    rays = s.rays_gpu(gpu)
    f = s.features.to(gpu).requires_grad_(True)
    out_det = r(f, rays, deterministic=True)
    out = r(f, rays)
    assert torch.equal(out_det, out)
    np.testing.assert_array_equal(out_det.detach().cpu().numpy(), O.volume_render(s.ot, *s.rays, s.opt))
    a_det = r.opacity_render(f, rays, deterministic=True)
    assert torch.equal(a_det, r.opacity_render(f, rays))
    with torch.no_grad():
        assert torch.equal(r(f, rays, deterministic=True), out)
    xf = torch.eye(3, device=gpu).repeat(f.shape[0], 1, 1)
    with pytest.raises(RuntimeError, match="transformation_matrices"):
        r(f, rays, transformation_matrices=xf, deterministic=True)
    c2w = torch.from_numpy(synth.camera_pose()).float()
    with pytest.raises(RuntimeError, match="deterministic=True is not served"):
        r.render_persp(f, c2w, width=16, height=16, fx=20.0, deterministic=True)
    with pytest.raises(RuntimeError, match="deterministic=True is not served"):
        r.motion_render(f, rays, deterministic=True)
    with pytest.raises(RuntimeError, match="deterministic=True is not served"):
        r.motion_feature_render(f, None, None, None, rays, deterministic=True)
    # nothing existing moved: the default route's gradient, the project's tolerance on the same inputs
    out.backward(torch.from_numpy(s.g).to(gpu))
    want, absum, _tg = tight(s, s.g)
    assert_grads_close(f.grad.cpu().numpy(), want, absum)
