"""The oracle and the restatements against a host build of the reference's own device code (oracle/ref.py: the text of
rt_kernel.cu and svox_kernel.cu in front of their host entry points, compiled by g++ with stand-in headers, every kernel
run for thread ids 0 .. Q-1 in ascending order on one thread).  No GPU.

Both sides run with the C library's expf (O.use_libm_exp) -- the reference's code calls `expf`, which here is glibc's --
and, for the float64 instantiation, with O.double_as_reference: the reference calls expf and sqrtf in double too.

  forward, bit for bit, float32 and float64, thresholds 0 and 1e-2:
      volume_render (SH1/4/16/25, RGBA, SG, ASG, a component sub-range, view rotations, _weight_accum),
      volume_render_image (with and without the NDC warp), opacity_render, render_depth, motion_render,
      motion_feature_render, grid_weight_render, query_vertical, warp_vertices, calc_corners;
  gradient of one ray (pixel, point) per call, float32: every entry bit for bit --
      volume_render_backward, the image backward, opacity_render_backward, warp_vertices_backward;
  gradient of the whole batch: the reference's float32 sequential sum within tests.util.assert_grads_close of the
      oracle's float64 sum on the `tight` scale; the double instantiation against the double oracle on one thread bit for
      bit (the oracle then adds in ray order, sample order, as the reference's thread loop does).

Left out by construction, not by tolerance: motion_feature_render_backward, which adds into an
uninitialised local in the reference (A17); query_vertical_backward on points in occupied leaves, where the reference
writes through a null pointer (A14) -- it is compared on points in empty leaves alone; data words below 0, which the
reference indexes with; rows that two leaves share (a ray would add twice to an entry and "one contribution" would not
hold) -- test_the_inputs_are_defined asserts
that the inputs have neither.
"""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
from oracle import oracle as O
from oracle import ref as R
from oracle import skinning as S
from svox_t_amd import synth
from tests import grid_weight_restate as GW
from tests.test_adversarial_host import IDS, adversarial
from tests.test_gpu_random_stress import random_rays, random_tree
from tests.util import assert_grads_close

pytestmark = pytest.mark.skipif(not R.available(), reason="neither oracle/_ref/libsvoxt_ref.so nor the reference tree")

DTYPES = (np.float32, np.float64)
STEP, BACKGROUND = 2e-3, 0.5
N_SINGLE = 200                       # rays (pixels, points) whose gradient is compared one per call


@pytest.fixture(autouse=True)
def reference_arithmetic():
    """glibc's expf on both sides, the reference's float calls in double; every other test relies on the defaults."""
    threads = O.num_threads()
    O.use_libm_exp(True)
    O.double_as_reference(True)
    try:
        yield
    finally:
        O.use_libm_exp(False)
        O.double_as_reference(False)
        O.set_num_threads(threads)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} values differ from the reference"


def assert_single_grad(ref32, want64, what):
    """A float32 gradient of the reference against the oracle's float64 array holding float32 values: every entry."""
    assert ref32.dtype == np.float32 and want64.dtype == np.float64
    w32 = want64.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want64, equal_nan=True), f"{what}: the oracle's entries are not float32 values"
    assert_same_bits(ref32, w32, what)


def ratio(got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    return float((err / (np.asarray(bound, np.float64) + 1e-30)).max())


def opts(scene, fast=False, **kw):
    th = 1e-2 if fast else 0.0
    kw = dict(dict(step_size=STEP, background_brightness=BACKGROUND, format=scene.format, basis_dim=scene.basis_dim,
                   sigma_thresh=th, stop_thresh=th), **kw)
    return O.make_options(**kw)


# ---- the small additions to the adversarial inputs ---------------------------------------------------------------------------
class Small:
    """random_tree of depth <= 4 (a few hundred rows), 300 random_rays over it; fmt is the tree's layout, `format` /
    `basis_dim` / `extra` what the options and the oracle tree say (the lobe formats share SH4's 13 columns)."""

    def __init__(self, fmt, K, seed, format=None, extra=None, N=2):
        t, feats = random_tree(seed, N=N, max_depth=4, data_format=fmt, K=K)
        n = t.n_internal
        self.t = t
        self.child, self.data = t.child[:n].numpy().copy(), t.data[:n].numpy().copy()
        self.parent_depth = t.parent_depth[:n].numpy().copy()
        self.features = feats.numpy()
        self.M, self.K = self.features.shape
        df = svox.DataFormat(fmt)
        self.format, self.basis_dim = (df.format if format is None else format), df.basis_dim
        self.ot = O.Tree(self.features, self.data, self.child, offset=t.offset.numpy().copy(), scaling=t.invradius.numpy().copy(),
                         extra=extra)
        self.rays = tuple(np.ascontiguousarray(a.numpy()) for a in random_rays(200 + seed, 300, t))
        self.Q = 300


def lobes(kind, n=4, seed=5):
    """SG: n rows of (sharpness, unit axis); ASG: n rows of (two bandwidths, three orthonormal axes x, y, z)."""
    rng = np.random.default_rng(seed)
    if kind == "SG":
        ax = rng.standard_normal((n, 3))
        return np.concatenate([rng.uniform(0.5, 8.0, (n, 1)), ax / np.linalg.norm(ax, axis=1, keepdims=True)], 1).astype(np.float32)
    q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    return np.concatenate([rng.uniform(0.5, 8.0, (n, 2)), q[:, :, 0], q[:, :, 1], q[:, :, 2]], 1).astype(np.float32)


_SMALL = {}


def small(name):
    if name not in _SMALL:
        _SMALL[name] = {
            "sh16": lambda: Small("SH16", 49, 3),
            "sh25": lambda: Small("SH25", 76, 4),
            "sh4": lambda: Small("SH4", 13, 5),
            "rgba": lambda: Small("RGBA", 4, 6),
            "sg": lambda: Small("SH4", 13, 7, format=O.FORMAT_SG, extra=lobes("SG")),
            "asg": lambda: Small("SH4", 13, 8, format=O.FORMAT_ASG, extra=lobes("ASG")),
            "n3": lambda: Small("SH1", 4, 9, N=3),
        }[name]()
    return _SMALL[name]


SMALL = ("sh16", "sh25", "sh4", "rgba", "sg", "asg", "n3")


def single_rays(scene, opt, n=N_SINGLE):
    """n ray indices with samples: first rays from inside the cube and rays with one or two zero direction components,
    then the rest in order."""
    o, d, _ = scene.rays
    steps, active = O.ray_steps(scene.ot, *scene.rays, O.make_options(step_size=opt.step_size, format=opt.format,
                                                                       basis_dim=opt.basis_dim))
    tree_o = scene.ot.offset + scene.ot.scaling * o
    inside = np.all((tree_o > 0) & (tree_o < 1), axis=1) & (active > 0)
    zeros = ((d == 0).sum(1) > 0) & (active > 0)
    first = np.concatenate([np.nonzero(inside)[0][:n // 4], np.nonzero(zeros & ~inside)[0][:n // 4]])
    rest = np.setdiff1d(np.nonzero(active > 0)[0], first)
    pick = np.concatenate([first, rest])[:n]
    return pick, int(inside[pick].sum()), int(zeros[pick].sum())


# ---- the inputs are ones on which the reference is defined -----------------------------------------------------------------------
def test_the_inputs_are_defined():
    scenes = [adversarial(*i) for i in IDS] + [small(n) for n in SMALL]
    for s in scenes:
        rows = s.data[s.data < s.M]
        assert s.data.min() >= 0, "a negative data word: the reference would index features with it"
        assert rows.size == s.M and np.unique(rows).size == s.M, "two leaves share a row"
        assert np.isfinite(s.ot.features).all()
    for i in IDS:
        a = adversarial(*i)
        pick, inside, zeros = single_rays(a, a.opt)
        assert pick.size == N_SINGLE and inside >= 40 and zeros >= 40, (i, pick.size, inside, zeros)
    for n in SMALL:                                          # 300 rays each: fewer of every kind, still 200 with samples
        pick, inside, zeros = single_rays(small(n), opts(small(n)))
        assert pick.size == N_SINGLE and inside >= 20 and zeros >= 20, (n, pick.size, inside, zeros)


# ---- forward, per-ray kernels ----------------------------------------------------------------------------------------------------
def _forward_rays(scene, what, **kw):
    for dtype in DTYPES:
        t = scene.ot.astype(dtype)
        for fast in (False, True):
            opt = opts(scene, fast, **kw)
            tag = f"{what} {np.dtype(dtype).name} fast={fast}"
            assert_same_bits(O.volume_render(t, *scene.rays, opt), R.volume_render(t, *scene.rays, opt), tag + " volume_render")
            assert_same_bits(O.opacity_render(t, *scene.rays, opt), R.opacity_render(t, *scene.rays, opt), tag + " opacity_render")
            assert_same_bits(O.render_depth(t, *scene.rays, opt), R.render_depth(t, *scene.rays, opt), tag + " render_depth")


@pytest.mark.parametrize("name,seed", IDS)
def test_forward_adversarial(name, seed):
    a = adversarial(name, seed)
    _forward_rays(a, f"{name}/{seed}")
    out = R.volume_render(a.ot, *a.rays, a.opt)
    assert np.isfinite(out).all() and np.count_nonzero(out[:, -1]) > 500          # (it rendered something)


@pytest.mark.parametrize("name", SMALL)
def test_forward_formats(name):
    _forward_rays(small(name), name)


def test_forward_component_subrange():
    for name, lo, hi in (("sh4", 1, 2), ("sh16", 4, 8), ("sh25", 0, 15), ("sg", 2, 3), ("asg", 0, 0)):
        _forward_rays(small(name), f"{name}[{lo}:{hi}]", min_comp=lo, max_comp=hi)


def rotations(M, dim, seed=12):
    q = np.linalg.qr(np.random.default_rng(seed).standard_normal((M, 3, 3)))[0].astype(np.float32)
    if dim == 3:
        return q
    x = np.zeros((M, 4, 4), np.float32)
    x[:, :3, :3], x[:, 3, 3] = q, 1
    return x


@pytest.mark.parametrize("name", ("sh4", "sh16", "sg", "asg", "rgba"))
def test_forward_and_gradient_with_view_rotations(name):
    """transformation_matrices [M, 3, 3] and [M, 4, 4]: the forward in float32 and float64, the gradient of one ray per
    call in float32."""
    s = small(name)
    for dtype in DTYPES[::-1]:
        t = s.ot.astype(dtype)
        for dim in (3, 4):
            x = rotations(s.M, dim)
            for fast in (False, True):
                opt = opts(s, fast)
                with O.transformation_matrices(x, dtype):
                    want = O.volume_render(t, *s.rays, opt)
                assert_same_bits(want, R.volume_render(t, *s.rays, opt, xform=x), f"{name} {np.dtype(dtype).name} xform {dim} fast={fast}")
            assert (want != O.volume_render(t, *s.rays, opt)).any() or name == "rgba"
    opt = opts(s)
    g = synth.grad_output(s.Q, want.shape[1], seed=3).numpy()
    pick, _, _ = single_rays(s, opt)
    assert pick.size == N_SINGLE
    for q in pick:
        one = tuple(a[q:q + 1] for a in s.rays)
        with O.transformation_matrices(x):
            w = O.volume_render_backward(s.ot, *one, opt, g[q:q + 1])
        assert_single_grad(R.volume_render_backward(s.ot, *one, opt, g[q:q + 1], xform=x), w, f"{name} xform ray {q}")


@pytest.mark.parametrize("name", ("sh4", "rgba", "n3"))
def test_weight_accum(name):
    """_weight_accum: the output is unchanged; one ray per call gives every slot its weight bit for bit; the batch is
    the reference's float32 sequential sum, within (n - 1) 2^-24 of the float64 sum of n <= Q non-negative weights."""
    s = small(name)
    for fast in (False, True):
        opt = opts(s, fast)
        want, wsum = O.volume_render_weights(s.ot, *s.rays, opt)
        acc = np.zeros(s.child.shape, np.float32)
        assert_same_bits(want, R.volume_render(s.ot, *s.rays, opt, weight_accum=acc), f"{name} fast={fast}: out with _weight_accum")
        assert np.count_nonzero(acc) > 20 and np.array_equal(acc != 0, wsum != 0)
        assert np.all(np.abs(acc.astype(np.float64) - wsum) <= (s.Q - 1) * 2.0 ** -24 * wsum)
    pick, _, _ = single_rays(s, opt, 100)
    for q in pick:
        one = tuple(a[q:q + 1] for a in s.rays)
        _, w1 = O.volume_render_weights(s.ot, *one, opt)
        acc = np.zeros(s.child.shape, np.float32)
        R.volume_render(s.ot, *one, opt, weight_accum=acc)
        assert_single_grad(acc, w1, f"{name}: weights of ray {q}")


# ---- the image kernels -----------------------------------------------------------------------------------------------------------
W, H = 40, 24


def camera(scene, ndc):
    """A camera outside the cube looking at its centre (world coordinates); with the NDC warp a forward-facing one."""
    t = scene.t
    lo, hi = t.tree2world(torch.zeros(1, 3))[0].numpy(), t.tree2world(torch.ones(1, 3))[0].numpy()
    mid, ext = (lo + hi) / 2, hi - lo
    if ndc:
        return GW.look_at(mid + np.array([0.1, 0.2, 2.5]) * ext, mid, up=(0.0, 1.0, 0.0)), 30.0
    return GW.look_at(mid + np.array([1.3, -1.1, 0.9]) * ext, mid), 28.0


@pytest.mark.parametrize("ndc", (False, True), ids=("plain", "ndc"))
@pytest.mark.parametrize("name", ("sh4", "rgba", "sg"))
def test_image_forward_and_gradient(name, ndc):
    """render_image_kernel / render_image_backward_kernel (cam2world_ray, maybe_world2ndc) against O.camera_rays +
    the per-ray oracle: the forward in float64 and float32, the gradient in float32."""
    s = small(name)
    c2w, f = camera(s, ndc)
    warp = (W, H, f) if ndc else None
    for dtype in DTYPES[::-1]:
        t = s.ot.astype(dtype)
        rays = O.camera_rays(c2w, f, f * 1.1, W, H, ndc=warp, dtype=dtype)
        for fast in (False, True):
            opt = opts(s, fast)
            if ndc:
                opt.ndc_width, opt.ndc_height, opt.ndc_focal = W, H, f
            want = O.volume_render(t, *rays, opt)
            got = R.volume_render_image(t, c2w, f, f * 1.1, W, H, opt)
            assert_same_bits(want.reshape(H, W, -1), got, f"{name} ndc={ndc} fast={fast} {np.dtype(dtype).name} image")
    hit = np.nonzero(want[:, -1] > 0)[0]
    assert hit.size > 100, "the camera does not see the tree"
    # one pixel per call: the upstream gradient is zero at every other pixel, whose contributions are then exact zeros
    g = synth.grad_output(W * H, want.shape[1], seed=4).numpy()
    assert hit.size >= N_SINGLE
    for q in hit[:: hit.size // N_SINGLE][:N_SINGLE]:
        g1 = np.zeros_like(g)
        g1[q] = g[q]
        w = O.volume_render_backward(s.ot, *(a[q:q + 1] for a in rays), opt, g[q:q + 1])
        got = R.volume_render_image_backward(s.ot, c2w, f, f * 1.1, W, H, opt, g1.reshape(H, W, -1))
        assert_single_grad(got, w, f"{name} ndc={ndc} pixel {q}")
    want, _, tight = O.volume_render_backward(s.ot, *rays, opt, g, want_abs="both")
    got = R.volume_render_image_backward(s.ot, c2w, f, f * 1.1, W, H, opt, g.reshape(H, W, -1))
    print(f"{name} ndc={ndc}: image batch gradient, worst err / (1e-5 tight) {ratio(got, want, 1e-5 * tight):.4f}")
    assert_grads_close(got, want, tight, what="image batch gradient")


# ---- the gradients of the ray batch ------------------------------------------------------------------------------------------------
def _single_ray_gradients(scene, what):
    opt = opts(scene)
    cols = O.out_data_dim(opt, scene.K)
    g = synth.grad_output(scene.Q, cols, seed=11).numpy()
    pick, _, _ = single_rays(scene, opt)
    assert pick.size == N_SINGLE
    entries = 0
    for q in pick:
        one = tuple(a[q:q + 1] for a in scene.rays)
        w = O.volume_render_backward(scene.ot, *one, opt, g[q:q + 1])
        got = R.volume_render_backward(scene.ot, *one, opt, g[q:q + 1])
        assert_single_grad(got, w, f"{what}: volume_render_backward of ray {q}")
        entries += np.count_nonzero(got)
        ga = np.ascontiguousarray(g[q:q + 1, -1:])
        assert_single_grad(R.opacity_render_backward(scene.ot, *one, opt, ga), O.volume_render_backward(scene.ot, *one, opt, ga),
                           f"{what}: opacity_render_backward of ray {q}")
    assert entries > 5 * pick.size
    return pick.size, entries


def _batch_gradients(scene, what):
    opt = opts(scene)
    cols = O.out_data_dim(opt, scene.K)
    worst = {}
    for c in (cols, 1):
        g = synth.grad_output(scene.Q, c, seed=11).numpy()
        want, _, tight = O.volume_render_backward(scene.ot, *scene.rays, opt, g, want_abs="both")
        got = R.volume_render_backward(scene.ot, *scene.rays, opt, g)
        worst[c] = ratio(got, want, 1e-5 * tight)
        assert_grads_close(got, want, tight, what=f"{what}: float32 batch gradient, grad_output [Q, {c}]")
        # double against double: one oracle thread adds in ray order, sample order, as the reference's thread loop does
        O.set_num_threads(1)
        t64 = scene.ot.astype(np.float64)
        assert_same_bits(O.volume_render_backward(t64, *scene.rays, opt, g), R.volume_render_backward(t64, *scene.rays, opt, g),
                         f"{what}: float64 batch gradient, grad_output [Q, {c}]")
    print(f"{what}: float32 batch gradient, worst err / (1e-5 tight): colours+alpha {worst[cols]:.4f}, alpha alone {worst[1]:.4f}; "
          f"float64 batch gradient bit for bit")
    return worst


@pytest.mark.parametrize("name,seed", IDS)
def test_gradient_adversarial(name, seed):
    a = adversarial(name, seed)
    n, entries = _single_ray_gradients(a, f"{name}/{seed}")
    print(f"{name}/{seed}: {n} rays one per call, {entries} non-zero entries, all bit-identical")
    _batch_gradients(a, f"{name}/{seed}")


@pytest.mark.parametrize("name", SMALL)
def test_gradient_formats(name):
    s = small(name)
    _single_ray_gradients(s, name)
    _batch_gradients(s, name)


# ---- motion ------------------------------------------------------------------------------------------------------------------------
def test_motion_render():
    """First hit: joint distances, depth, hit point, feature row; tree.extra = joint positions [J, 3]."""
    for name in ("rgba", "n3", "sh4"):
        s = small(name)
        joints = np.random.default_rng(2).uniform(-1, 1, (5, 3)).astype(np.float32)
        for dtype in DTYPES:
            t = O.Tree(s.features, s.data, s.child, s.ot.offset, s.ot.scaling, extra=joints, dtype=dtype)
            for fast in (False, True):
                opt = opts(s, fast)
                want, got = O.motion_render(t, *s.rays, opt), R.motion_render(t, *s.rays, opt)
                for w, g, nm in zip(want, got, ("distances", "depth", "hit_point", "data_idx")):
                    assert_same_bits(w, g, f"{name} {np.dtype(dtype).name} fast={fast} motion_render {nm}")
                assert np.count_nonzero(got[1]) > 50


def test_motion_feature_render():
    for name in ("rgba", "n3", "sh4"):
        s = small(name)
        rng = np.random.default_rng(3)
        J, F, B = 6, 7, 3
        jf = rng.standard_normal((J, F)).astype(np.float32) * 2
        sw = rng.random((s.M, B)).astype(np.float32)
        sw[rng.random((s.M, B)) < 0.3] = 0
        sw[rng.random((s.M, B)) < 0.05] = -0.25
        ji = rng.integers(0, J, (s.M, B))
        for dtype in DTYPES:
            t, mo = s.ot.astype(dtype), O.Motion(jf, sw, ji, dtype)
            for fast in (False, True):
                opt = opts(s, fast)
                want = O.motion_feature_render(t, mo, *s.rays, opt)
                assert_same_bits(want, R.motion_feature_render(t, mo, *s.rays, opt), f"{name} {np.dtype(dtype).name} fast={fast}")
                assert np.count_nonzero(want) > 300


# ---- the dense-grid weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndc", (False, True), ids=("plain", "ndc"))
def test_grid_weight_render(ndc):
    """grid_weight_render_kernel over three views against tests/grid_weight_restate.py without its advance guard (the
    reference's bare `t += delta_t`), float32 and float64: the maxima bit for bit, the hit counts as integers.  A
    seventh of the shell's cells holds 1e-3 and another seventh exactly 1e-2, so the two thresholds give different grids
    (`sigma > sigma_thresh` is the kernel's only use of either threshold)."""
    R_ = 12                                                            # not a power of two: the scaled position rounds
    sigma = GW.shell_sigma(R_, seed=1)
    flat = sigma.reshape(-1)                                           # (a view: boolean indexing would assign to a copy)
    nz = np.nonzero(flat > 0)[0]
    flat[nz[::7]], flat[nz[3::7]] = 1e-3, 1e-2
    assert (sigma == np.float32(1e-3)).sum() >= 40 and (sigma == np.float32(1e-2)).sum() >= 40 and (sigma > 1).sum() > 200
    offset, scaling = np.float32([0.1, -0.05, 0.02]), np.float32([0.8, 1.1, 0.9])
    eyes = ((2.0, 1.5, 1.2), (-1.2, 2.2, 0.4), (0.3, -1.8, 2.1))
    if ndc:
        cams = np.stack([GW.look_at((0.5 + 0.1 * i, 0.45, 3.0 + 0.2 * i), (0.5, 0.5, 0.0), up=(0.0, 1.0, 0.0)) for i in range(3)])
    else:
        cams = np.stack([GW.look_at(e) for e in eyes])
    f = 30.0
    for dtype in DTYPES:
        grids = []
        for thresh in (0.0, 1e-2):
            opt = O.make_options(step_size=STEP, sigma_thresh=thresh)
            if ndc:
                opt.ndc_width, opt.ndc_height, opt.ndc_focal = W, H, f
            want = GW.march_cameras(sigma, cams, f, f, W, H, offset, scaling, ndc=(W, H, f) if ndc else None, step_size=STEP,
                                    sigma_thresh=thresh, advance_guard=False, max_steps=10000, dtype=dtype)
            gw, gh = R.grid_weight_render(sigma, cams, f, f, W, H, opt, offset, scaling, dtype=dtype)
            assert_same_bits(want.weight, gw, f"grid weights ndc={ndc} thresh={thresh} {np.dtype(dtype).name}")
            np.testing.assert_array_equal(want.hits, gh.astype(np.int64))
            assert gh.max() < 2 ** 24 and np.count_nonzero(gw) > 100
            grids.append((gw, gh))
        # the threshold matters: cells at or below 1e-2 are hit under 0 and not under 1e-2, and the cells behind them
        # then see more light
        assert ((grids[0][1] > 0) & (grids[1][1] == 0)).sum() > 20 and (grids[0][0] != grids[1][0]).sum() > 100


# ---- svox_kernel.cu ------------------------------------------------------------------------------------------------------------------
def query_points(scene, n, seed=6):
    """Points inside, on the faces of and outside the cube, in world coordinates."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.15, 1.15, (n, 3))
    p[: n // 10] = rng.integers(0, 2, (n // 10, 3))                     # the corners: clamp_coord's two ends
    p[n // 10: n // 5, 0] = 1.0
    return ((p - scene.ot.offset.astype(np.float64)) / scene.ot.scaling.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("name,seed", IDS)
def test_query_vertical(name, seed):
    a = adversarial(name, seed)
    p = query_points(a, 2000)
    for dtype in DTYPES:
        t = a.ot.astype(dtype)
        wv, wn, wd = O.query(t, p)
        gv, gn, gd, leaf = R.query(t, p)
        tag = f"{name}/{seed} {np.dtype(dtype).name} query_vertical"
        assert_same_bits(wv, gv, tag + " values")
        np.testing.assert_array_equal(wn, gn)
        np.testing.assert_array_equal(wd, gd)
        # leaf_node: the distinct slots in ascending order, unpacked to (node, u, v, w)
        slots = np.unique(wn)
        N = a.ot.N
        np.testing.assert_array_equal(leaf, np.stack([slots // N ** 3, slots // N ** 2 % N, slots // N % N, slots % N], 1))
    assert (wd < 0).sum() > 100 and (wd >= 0).sum() > 500
    # query_vertical_backward: the reference writes through a null pointer for every point whose leaf names a row
    # (the host build faults there as a GPU would), so it is defined on points in empty leaves alone, where
    # it returns before the write: no contribution, on either side
    empty = p[wd < 0]
    g = synth.grad_output(empty.shape[0], a.K, seed=8).numpy()
    assert not R.query_backward(a.ot, empty, g).any() and not O.query_backward(a.ot, empty, g).any()


def skinning_case(Q=400, J=7, B=4, seed=0):
    rng = np.random.default_rng(seed)
    mats = rng.normal(size=(J, 4, 4)).astype(np.float32)
    mats[:, 3] = [0, 0, 0, 1]
    p = rng.normal(size=(Q, 3)).astype(np.float32)
    sw = rng.random((Q, B)).astype(np.float32)
    sw[rng.random((Q, B)) < 0.3] = 0
    sw[rng.random((Q, B)) < 0.05] = -0.25
    ji = rng.integers(0, J, size=(Q, B))
    ji[::9, 1] = ji[::9, 0]                                             # a joint bound twice to one point
    return mats, p, sw, ji


def test_warp_vertices():
    mats, p, sw, ji = skinning_case()
    rng = np.random.default_rng(1)
    dv = rng.normal(size=p.shape).astype(np.float32)
    dm = rng.normal(size=(len(p), 4, 4)).astype(np.float32)
    for dtype in DTYPES:
        tag = f"{np.dtype(dtype).name} warp_vertices"
        wv, wm = S.warp_vertices(mats, p, sw, ji, dtype=dtype)
        gv, gm = R.warp_vertices(mats, p, sw, ji, dtype=dtype)
        assert_same_bits(wv, gv, tag + " vertices")
        assert_same_bits(wm, gm, tag + " matrix_out")
        wp, wmat, wabs, wsw = S.warp_vertices_backward(mats, p, sw, ji, dv, dm, dtype=dtype)
        gp, gmat, gsw = R.warp_vertices_backward(mats, p, sw, ji, dv, dm, dtype=dtype)
        assert_same_bits(wp, gp, tag + "_backward points")                         # per point: no sum across points
        assert_same_bits(wsw, gsw, tag + "_backward skinning weights")
        print(f"{tag} batch gradient in the matrices, worst err / (1e-5 sum|c|) {ratio(gmat, wmat, 1e-5 * wabs):.4f}")
        assert_grads_close(gmat, wmat, wabs, what=tag + " batch gradient in the matrices")
    # one point per call: a joint's entry takes two addends per binding (matrix and vertex term), so it is a float32
    # value only where the point binds the joint once and one of the two terms is zero -- take dm = 0
    zero = np.zeros_like(dm)
    once = np.nonzero([(np.unique(ji[q][sw[q] > 0]).size == (sw[q] > 0).sum()) for q in range(len(p))])[0][:N_SINGLE]
    assert once.size == N_SINGLE
    for q in once:
        one = (mats, p[q:q + 1], sw[q:q + 1], ji[q:q + 1], dv[q:q + 1], zero[q:q + 1])
        w = S.warp_vertices_backward(*one)
        got = R.warp_vertices_backward(*one)
        assert_single_grad(got[1], w[1], f"warp_vertices_backward matrices of point {q}")


def corner_walk(parent_depth, N, leaves, dtype):
    """N3Tree._calc_corners' walk up the parent chain (corner = (corner + slot) / N per level, leaf first) in numpy and
    in `dtype`: in float32 it is that walk, which test_calc_corners asserts."""
    curr = np.asarray(leaves, np.int64).copy()
    corner = np.zeros((curr.shape[0], 3), dtype)
    live = np.arange(curr.shape[0])
    while True:
        corner[live] = ((corner[live] + curr[:, 1:].astype(dtype)) / dtype(N)).astype(dtype)
        up = curr[:, 0] != 0
        if not up.any():
            return corner
        live = live[up]
        packed = parent_depth[curr[up, 0], 0].astype(np.int64)
        curr = np.stack([packed // N ** 3, packed // N ** 2 % N, packed // N % N, packed % N], 1)


@pytest.mark.parametrize("name,seed", IDS)
def test_calc_corners(name, seed):
    """calc_corner_kernel against N3Tree._calc_corners' walk up the parent chain on the CPU (float32) and against the
    same walk in numpy, float32 and float64."""
    a = adversarial(name, seed)
    t = a.tree("cpu")
    leaves = t._all_leaves()
    assert leaves.shape[0] > 5000 and int(t.parent_depth[leaves[:, 0].long(), 1].max()) >= 2
    want = t._calc_corners(leaves).numpy()
    got = R.calc_corners(a.ot, a.parent_depth, leaves.numpy())
    assert_same_bits(want, got, f"{name}/{seed} calc_corners")
    for dtype in DTYPES:
        walk = corner_walk(a.parent_depth, a.ot.N, leaves.numpy(), dtype)
        if dtype == np.float32:
            assert_same_bits(want, walk, f"{name}/{seed}: the numpy walk is N3Tree._calc_corners'")
        assert_same_bits(walk, R.calc_corners(a.ot.astype(dtype), a.parent_depth, leaves.numpy()),
                         f"{name}/{seed} calc_corners {np.dtype(dtype).name}")
