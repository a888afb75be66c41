"""Tensors that start anywhere in a buffer (include/svoxt.h, "Alignment"): every operator here is run on fresh
allocations and then with one argument at a time moved 1, 2 and 3 elements into a larger buffer -- 4, 8 and 12 bytes off a
16-byte boundary, what `flat[1:].view(M, K)`, `rays.origins[i * B:]` or `grad[1:]` hand over.  The shifted call has to
give what the operator's own test asks of the aligned one (the oracle bit for bit, assert_grads_close on the oracle's
scale for float atomics, the restatement's bits), the aligned run's bits where the operator is deterministic, and take the
same route (csrc.LAST_ROUTE).  Operators that write a caller's table leave the sentinel words around it alone.

Shapes: the depth-5 shell tree and a 40 x 24 image -- 960 rays, 15 tiles of 8 x 8, no multiple of 256 -- rendered as a
declared image and as a shuffled batch.  The C half (what libsvoxt refuses) is tests/test_placement_host.py."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from oracle import skinning as S
from svox_t_amd import synth
from tests import assign_restate as AR
from tests import depth_restate as DR
from tests import distortion_restate as XR
from tests import grid_weight_restate as GR
from tests import merge_restate as MR
from tests import neighbors_restate as NR
from tests import p2v_restate as PV
from tests import prune_restate as PRUNE
from tests import quantize_restate as QUANT
from tests import rowgrad_restate as RG
from tests import rows_restate as RR
from tests import samples_restate as SR
from tests import subdivide_restate as SUBD
from tests.test_gpu_motion import binding, skeleton
from tests.test_skinning_oracle import case as warp_case
from tests.util import Case, assert_grads_close, assert_outputs_close

pytestmark = pytest.mark.gpu

W, H, DEPTH = 40, 24, 5
Q = W * H
SHIFTS = (1, 2, 3)
SENTINEL = 0x7FA5C3D1                 # a NaN as float32, 2141570001 as int32: nothing computes it


# ------------------------------------------------------------------------------------------------------------ the helper
def shifted(t, s):
    """(view, buffer): the values of t, s elements into a buffer of s + numel + 4 elements whose other words hold SENTINEL;
    the view is contiguous, has t's shape and dtype and starts 4 s bytes (8 s for int64) behind the buffer's start."""
    n = t.numel()
    buf = torch.empty(s + n + 4, dtype=t.dtype, device=t.device)
    buf.view(torch.int32).fill_(SENTINEL)
    buf[s:s + n].copy_(t.detach().reshape(-1))
    view = buf[s:s + n].view(t.shape)
    assert view.is_contiguous() and buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + s * t.element_size()
    return view, buf


def assert_guards(buf, s, what=""):
    """The s elements in front of the view and the four behind it still hold SENTINEL, compared as int32."""
    w = buf.element_size() // 4
    words = buf.view(torch.int32)
    assert bool((words[:s * w] == SENTINEL).all()), f"{what}: the {s} elements in front of the table were written"
    assert bool((words[-4 * w:] == SENTINEL).all()), f"{what}: the elements behind the table were written"


def bits(x):
    """The float32 bit patterns of a tensor or an array (a float64 array of float32 values is taken as those values)."""
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float32).view(np.int32)


def test_the_helper(gpu):
    for dtype in (torch.float32, torch.int32, torch.int64):
        t = torch.arange(24, device=gpu).to(dtype).view(6, 4)
        for s in SHIFTS:
            v, buf = shifted(t, s)
            assert torch.equal(v, t) and v.dtype == dtype and v.shape == t.shape and buf.numel() == s + 24 + 4
            assert v.data_ptr() % 16 == (s * t.element_size()) % 16
            assert_guards(buf, s)
            buf[s - 1] = 0
            with pytest.raises(AssertionError, match="in front"):
                assert_guards(buf, s)
            buf.view(torch.int32).fill_(SENTINEL)
            buf[-1] = 0
            with pytest.raises(AssertionError, match="behind"):
                assert_guards(buf, s)


# ------------------------------------------------------------------------------------------------------------ the scenes
PAYLOADS = {"rgba4": ("RGBA", 4), "sh9": ("SH9", 28), "rgba8": ("RGBA", 8), "rgba16": ("RGBA", 16), "rgba32": ("RGBA", 32),
            "sh4": ("SH4", 13), "sg9": ("SG9", 28)}
_BUILT = {}


class Scene:
    """A payload on the depth-5 shell tree, its oracle twin, the 40 x 24 rays in image order and shuffled, an upstream
    gradient; the references are computed once and kept."""

    def __init__(self, name):
        fmt, K = PAYLOADS[name]
        self.c = c = Case(depth=DEPTH, K=K, data_format=fmt, width=W, height=H)
        self.fmt, self.K = fmt, K
        self.lobes = None
        if fmt.startswith("SG"):
            g = torch.Generator().manual_seed(4)
            self.lobes = torch.cat([torch.rand(c.basis_dim, 1, generator=g) * 4 + 0.5,
                                    torch.nn.functional.normalize(torch.randn(c.basis_dim, 3, generator=g), dim=-1)], -1).contiguous()
        t = c.tree()
        self.ot = O.Tree(c.features.numpy(), c.st.data, c.st.child, offset=t.offset.numpy(), scaling=t.invradius.numpy(),
                         extra=None if self.lobes is None else self.lobes.numpy())
        self.M = c.st.n_features
        self.perm = np.random.default_rng(5).permutation(Q)
        self.cols = O.out_data_dim(c.oracle_opts(), K)
        self.g = synth.grad_output(Q, self.cols).numpy()
        self._ref = {}

    def rays_np(self, order="image"):
        r = self.c.rays_np()
        return r if order == "image" else tuple(np.ascontiguousarray(a[self.perm]) for a in r)

    def g_np(self, order="image"):
        return self.g if order == "image" else np.ascontiguousarray(self.g[self.perm])

    def rays_gpu(self, gpu, order="image"):
        return svox.Rays(*(torch.from_numpy(a).to(gpu) for a in self.rays_np(order)))

    def tree(self, gpu, features=None, child=None, data=None):
        """The tree on the GPU; features / child / data: GPU tensors to adopt AS THEY ARE (shifted views)."""
        c = self.c
        dev_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
        tree = svox.N3Tree.from_arrays(dev_t(c.st.child) if child is None else child, dev_t(c.st.data) if data is None else data,
                                       c.st.parent_depth, c.features.to(gpu) if features is None else features,
                                       data_format=self.fmt, radius=c.radius, center=c.center, device=gpu)
        if self.lobes is not None:
            tree.extra_data = self.lobes.to(gpu)
        for mine, theirs in ((features, tree.features), (child, tree.child), (data, tree.data)):
            assert mine is None or theirs.data_ptr() == mine.data_ptr()          # adopted, not copied
        return tree

    def forward_ref(self, fast, order="image"):
        key = ("fwd", fast, order)
        if key not in self._ref:
            self._ref[key] = O.volume_render(self.ot, *self.rays_np(order), self.c.oracle_opts(fast=fast))
        return self._ref[key]

    def backward_ref(self, fast, order="image"):
        """(grad, sum |contribution|) of the oracle: the scale assert_grads_close takes with rtol 1e-5."""
        key = ("bwd", fast, order)
        if key not in self._ref:
            self._ref[key] = O.volume_render_backward(self.ot, *self.rays_np(order), self.c.oracle_opts(fast=fast), self.g_np(order),
                                                      want_abs=True)
        return self._ref[key]

    def deterministic_ref(self):
        if "rows" not in self._ref:
            self._ref["rows"] = RG.grad(self.ot, self.rays_np(), self.c.oracle_opts(), self.g)
        return self._ref["rows"]


def scene(name):
    if name not in _BUILT:
        _BUILT[name] = Scene(name)
    return _BUILT[name]


def placements(t):
    """[(shift, tensor, buffer)]: t as it is, then 1, 2 and 3 elements into a buffer."""
    return [(0, t, None)] + [(s,) + shifted(t, s) for s in SHIFTS]


def route():
    return dict(_C.LAST_ROUTE)


def render_step(tree, feats, rays, g, *, fast=False, image_shape=None, deterministic=False, xf=None):
    """Forward and backward of VolumeRenderer.forward on `feats` (used as it stands: a view stays a view)."""
    f = feats.detach().requires_grad_(True)
    assert f.data_ptr() == feats.data_ptr()
    r = svox.VolumeRenderer(tree)
    kw = {} if xf is None else dict(transformation_matrices=xf)
    out = r(f, rays, fast=fast, image_shape=image_shape, deterministic=deterministic, **kw)
    fwd = route()
    out.backward(g)
    return out.detach(), f.grad, (fwd["forward"], fwd["forward_terms"], route()["backward"])


# ======================================================================================================================
# 1. Colour render, feature table shifted
# ======================================================================================================================
ROUTES = [  # (name, ray order, image_shape, BWD_GATHER, deterministic)
    ("image", "image", (H, W), 1, False),
    ("shuffled", "shuffled", None, 1, False),
    ("shuffled, per tile", "shuffled", None, 2, False),
    ("image, deterministic", "image", (H, W), 1, True),
]


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name", list(PAYLOADS))
def test_colour_render_with_the_feature_table_shifted(gpu, name, fast, monkeypatch):
    sc = scene(name)
    tree = sc.tree(gpu)
    feats = sc.c.features.to(gpu)
    for what, order, shape, gather, det in ROUTES:
        monkeypatch.setattr(_C, "BWD_GATHER", gather)
        rays = sc.rays_gpu(gpu, order)
        g = torch.from_numpy(sc.g_np(order)).to(gpu)
        want = sc.forward_ref(fast, order)
        gw, gabs = sc.backward_ref(fast, order)
        first = None
        for s, f, buf in placements(feats):
            out, grad, rt = render_step(tree, f, rays, g, fast=fast, image_shape=shape, deterministic=det)
            tag = f"{name} fast={fast} {what} shift {s}"
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=tag)
            if det:
                # (the deterministic gradient is the one at thresholds 0, whatever the forward's: tests/test_gpu_rowgrad.py)
                assert np.array_equal(bits(grad), bits(sc.deterministic_ref())), tag
            else:
                assert_grads_close(grad.cpu().numpy(), gw, gabs, what=tag)
            if s == 0:
                first = (out, grad, rt)
                continue
            assert f.data_ptr() % 16 == 4 * s and rt == first[2], (tag, rt, first[2])
            assert torch.equal(out, first[0]), tag
            if det:
                assert torch.equal(grad, first[1]), tag
            assert_guards(buf, s, tag)
    if name in ("rgba8", "rgba16", "rgba32"):           # rows of 8 / 16 / 32 floats: the exponentials table's route
        assert "shade_chan_kernel" in first[2][0], first[2]


@pytest.mark.parametrize("name", ["rgba4", "sh9", "rgba32", "sh4"])
def test_sigma_only_operators_and_the_camera_with_the_feature_table_shifted(gpu, name):
    """opacity_render and its backward, render_depth (single floats of the table, 4-byte aligned for the library too), and
    render_persp: the colour render with rays made in the kernel, forward and backward."""
    sc = scene(name)
    tree = sc.tree(gpu)
    r = svox.VolumeRenderer(tree)
    feats = sc.c.features.to(gpu)
    rays = sc.rays_gpu(gpu)
    opt = sc.c.oracle_opts()
    g1 = synth.grad_output(Q, 1, seed=3)
    want_a = O.opacity_render(sc.ot, *sc.rays_np(), opt)
    want_d = O.render_depth(sc.ot, *sc.rays_np(), opt)
    ga, gabs = O.volume_render_backward(sc.ot, *sc.rays_np(), opt, g1.numpy(), want_abs=True)
    pose = synth.camera_pose(azimuth_deg=70.0, elevation_deg=-15.0).astype(np.float32)
    fx = 1111.111 * W / 800.0
    po, pd, pv = O.camera_rays(pose, fx, fx, W, H)
    want_p = O.volume_render(sc.ot, po, pd, pv, opt)
    assert (want_p[:, -1] > 0.05).mean() > 0.05
    gp = torch.randn(H, W, sc.cols, generator=torch.Generator().manual_seed(4))
    gpw, gpabs = O.volume_render_backward(sc.ot, po, pd, pv, opt, gp.reshape(Q, -1).numpy(), want_abs=True)
    c2w = torch.from_numpy(pose).to(gpu)
    for s, f, buf in placements(feats):
        for shape in ((H, W), None):
            fa = f.detach().requires_grad_(True)
            alpha = r.opacity_render(fa, rays, image_shape=shape)
            np.testing.assert_array_equal(alpha.detach().cpu().numpy(), want_a)
            alpha.backward(g1.to(gpu))
            assert_grads_close(fa.grad.cpu().numpy(), ga, gabs, what=f"opacity backward, shift {s}")
            assert bool((fa.grad[:, :-1] == 0).all())
            with torch.no_grad():
                np.testing.assert_array_equal(r.render_depth(f, rays, image_shape=shape).cpu().numpy(), want_d)
        fp = f.detach().requires_grad_(True)
        img = r.render_persp(fp, c2w, width=W, height=H, fx=fx)
        np.testing.assert_array_equal(img.detach().reshape(Q, -1).cpu().numpy(), want_p)
        img.backward(gp.to(gpu))
        assert_grads_close(fp.grad.cpu().numpy(), gpw, gpabs, what=f"render_persp backward, shift {s}")
        if buf is not None:
            assert f.data_ptr() % 16 == 4 * s
            assert_guards(buf, s)


def rotations(M, dim, seed=9):
    A = torch.randn(M, 3, 3, generator=torch.Generator().manual_seed(seed))
    Qm, _ = torch.linalg.qr(A)
    if dim == 3:
        return Qm.contiguous()
    X = torch.zeros(M, 4, 4)
    X[:, :3, :3] = Qm
    X[:, :3, 3] = torch.randn(M, 3, generator=torch.Generator().manual_seed(seed + 1))
    X[:, 3, 3] = 1
    return X.contiguous()


@pytest.mark.parametrize("name,dim", [("sh9", 4), ("sh4", 4), ("sh9", 3)])
def test_view_rotations_with_the_table_and_the_matrices_shifted(gpu, name, dim):
    """transformation_matrices [M, 4, 4] (and [M, 3, 3]): the feature table shifted under aligned matrices, then the
    matrices shifted under an aligned table."""
    sc = scene(name)
    tree = sc.tree(gpu)
    feats = sc.c.features.to(gpu)
    xf = rotations(sc.M, dim)
    rays = sc.rays_gpu(gpu)
    g = torch.from_numpy(sc.g).to(gpu)
    with O.transformation_matrices(xf.numpy()):
        want = O.volume_render(sc.ot, *sc.rays_np(), sc.c.oracle_opts())
        gw, gabs = O.volume_render_backward(sc.ot, *sc.rays_np(), sc.c.oracle_opts(), sc.g, want_abs=True)
    assert np.abs(want - sc.forward_ref(False)).max() > 1e-3            # the rotations do change the image
    xg = xf.to(gpu)
    first = None
    for which in ("features", "transformation_matrices"):
        for s, t, buf in placements(feats if which == "features" else xg):
            f, x = (t, xg) if which == "features" else (feats, t)
            out, grad, rt = render_step(tree, f, rays, g, image_shape=(H, W), xf=x)
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{which} shift {s}")
            assert_grads_close(grad.cpu().numpy(), gw, gabs, what=f"{which} shift {s}")
            if first is None:
                first = (out, rt)
            assert rt == first[1] and torch.equal(out, first[0]), (which, s, rt, first[1])
            if buf is not None:
                assert t.data_ptr() % 16 == 4 * s
                assert_guards(buf, s)


# ======================================================================================================================
# 2. Every other tensor argument of the render family shifted, one at a time
# ======================================================================================================================
RENDER_ARGS = ["origins", "dirs", "vdirs", "grad_output", "child", "data", "offset", "scaling"]


@pytest.mark.parametrize("order", ["image", "shuffled"])
@pytest.mark.parametrize("which", RENDER_ARGS)
def test_colour_render_with_one_other_argument_shifted(gpu, which, order):
    """SH9: origins / dirs / vdirs / grad_output 4, 8 and 12 bytes on (12: rows 1.. of a [Q + 1, 3] buffer), the int32
    child / data tables adopted by N3Tree.from_arrays as views one to three ints on, offset and scaling."""
    sc = scene("sh9")
    feats = sc.c.features.to(gpu)
    want = sc.forward_ref(False, order)
    gw, gabs = sc.backward_ref(False, order)
    shape = (H, W) if order == "image" else None
    o, d, v = sc.rays_gpu(gpu, order)
    g = torch.from_numpy(sc.g_np(order)).to(gpu)
    base_tree = sc.tree(gpu)
    source = {"origins": o, "dirs": d, "vdirs": v, "grad_output": g, "child": base_tree.child, "data": base_tree.data,
              "offset": base_tree.offset, "scaling": base_tree.invradius}[which]
    first = None
    for s, t, buf in placements(source):
        tree = base_tree
        if which in ("child", "data"):
            tree = sc.tree(gpu, **{which: t})
        elif which in ("offset", "scaling"):
            tree = sc.tree(gpu)
            setattr(tree, "offset" if which == "offset" else "invradius", t)
        rays = svox.Rays(t if which == "origins" else o, t if which == "dirs" else d, t if which == "vdirs" else v)
        out, grad, rt = render_step(tree, feats, rays, t if which == "grad_output" else g, image_shape=shape)
        tag = f"{which} {order} shift {s}"
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=tag)
        assert_grads_close(grad.cpu().numpy(), gw, gabs, what=tag)
        if first is None:
            first = (out, rt)
        assert rt == first[1] and torch.equal(out, first[0]), (tag, rt, first[1])
        if buf is not None:
            assert t.data_ptr() % 16 == 4 * s
            assert_guards(buf, s, tag)


def test_colour_render_with_extra_data_and_the_camera_matrix_shifted(gpu):
    """SG9's lobes (extra_data, with the table aligned and with both shifted) and render_persp's c2w."""
    sc = scene("sg9")
    feats = sc.c.features.to(gpu)
    rays = sc.rays_gpu(gpu)
    g = torch.from_numpy(sc.g).to(gpu)
    want = sc.forward_ref(False)
    gw, gabs = sc.backward_ref(False)
    first = None
    for s, lobes, buf in placements(sc.lobes.to(gpu)):
        for f, fbuf in ((feats, None),) + ((shifted(feats, s),) if s else ()):
            tree = sc.tree(gpu)
            tree.extra_data = lobes
            out, grad, rt = render_step(tree, f, rays, g, image_shape=(H, W))
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"extra_data shift {s}")
            assert_grads_close(grad.cpu().numpy(), gw, gabs, what=f"extra_data shift {s}")
            if first is None:
                first = (out, rt)
            assert rt == first[1] and torch.equal(out, first[0]), (s, rt, first[1])
        if buf is not None:
            assert lobes.data_ptr() % 16 == 4 * s
            assert_guards(buf, s)
    # the camera matrix
    sc = scene("sh9")
    tree = sc.tree(gpu)
    r = svox.VolumeRenderer(tree)
    pose = synth.camera_pose(azimuth_deg=70.0, elevation_deg=-15.0).astype(np.float32)
    fx = 1111.111 * W / 800.0
    po, pd, pv = O.camera_rays(pose, fx, fx, W, H)
    want = O.volume_render(sc.ot, po, pd, pv, sc.c.oracle_opts())
    gp = torch.randn(H, W, 4, generator=torch.Generator().manual_seed(4))
    gpw, gpabs = O.volume_render_backward(sc.ot, po, pd, pv, sc.c.oracle_opts(), gp.reshape(Q, 4).numpy(), want_abs=True)
    for s, c2w, buf in placements(torch.from_numpy(pose).to(gpu)):
        f = sc.c.features.to(gpu).requires_grad_(True)
        img = r.render_persp(f, c2w, width=W, height=H, fx=fx)
        np.testing.assert_array_equal(img.detach().reshape(Q, 4).cpu().numpy(), want, err_msg=f"c2w shift {s}")
        img.backward(gp.to(gpu))
        assert_grads_close(f.grad.cpu().numpy(), gpw, gpabs, what=f"c2w shift {s}")
        if buf is not None:
            assert c2w.data_ptr() % 16 == 4 * s
            assert_guards(buf, s)


# ======================================================================================================================
# 3. Per-ray and per-sample operators
# ======================================================================================================================
@pytest.mark.parametrize("which", ["features", "origins", "dirs", "grad_output"])
@pytest.mark.parametrize("op", ["depth_moments", "distortion"])
def test_per_ray_sigma_operators(gpu, op, which):
    sc = scene("rgba4")
    tree = sc.tree(gpu)
    r = svox.VolumeRenderer(tree)
    rays_np, opt = sc.rays_np(), sc.c.oracle_opts()
    cols = 3 if op == "depth_moments" else 2
    g = synth.grad_output(Q, cols, seed=11).numpy()
    key = ("ray", op)
    if key not in sc._ref:
        if op == "depth_moments":
            sc._ref[key] = (DR.moments(sc.ot, rays_np, opt, "mid", torch.float64).numpy(), DR.moments_grad(sc.ot, rays_np, opt, "mid", g),
                            DR.moments_grad_scale(sc.ot, rays_np, opt, "mid", g))
        else:
            sc._ref[key] = (XR.distortion(sc.ot, rays_np, opt, torch.float64).numpy(), XR.distortion_grad(sc.ot, rays_np, opt, g),
                            XR.distortion_grad_scale(sc.ot, rays_np, opt, g))
    want, gw, scale = sc._ref[key]
    feats = sc.c.features.to(gpu)
    o, d, v = sc.rays_gpu(gpu)
    gg = torch.from_numpy(g).to(gpu)
    source = {"features": feats, "origins": o, "dirs": d, "grad_output": gg}[which]
    first = None
    for s, t, buf in placements(source):
        f = (t if which == "features" else feats).detach().requires_grad_(True)
        rays = svox.Rays(t if which == "origins" else o, t if which == "dirs" else d, v)
        for shape in ((H, W), None):
            f.grad = None
            out = r.render_depth_moments(f, rays, at="mid", image_shape=shape) if op == "depth_moments" else \
                r.render_distortion(f, rays, image_shape=shape)
            out.backward(t if which == "grad_output" else gg)
            assert_outputs_close(out.detach().cpu().numpy(), want, what=f"{op} {which} shift {s}")
            assert_grads_close(f.grad.cpu().numpy(), gw, scale, what=f"{op} {which} shift {s}")
            if first is None:
                first = out.detach()
            assert torch.equal(out.detach(), first), (op, which, s)           # the forward is a fixed sequence per ray
        if buf is not None:
            assert t.data_ptr() % 16 == 4 * s
            assert_guards(buf, s)


def test_ray_samples_and_view_basis(gpu):
    """ray_samples with the table (read for min_sigma) and the rays shifted: the restatement's lists; view_basis with the
    view directions shifted: the oracle's basis."""
    sc = scene("sh9")
    tree = sc.tree(gpu)
    r = svox.VolumeRenderer(tree)
    key = ("lists", 0.0)
    if key not in sc._ref:
        sc._ref[key] = SR.lists(sc.ot, sc.rays_np(), sc.c.oracle_opts(), 0.0)
    want = sc._ref[key]
    assert want.row.shape[0] > 1000
    feats = sc.c.features.to(gpu)
    o, d, v = sc.rays_gpu(gpu)
    basis_want = O.basis(sc.c.format, sc.c.basis_dim, sc.rays_np()[2], None)
    for which, source in (("features", feats), ("origins", o), ("dirs", d), ("vdirs", v)):
        for s, t, buf in placements(source):
            rays = svox.Rays(t if which == "origins" else o, t if which == "dirs" else d, t if which == "vdirs" else v)
            for shape in ((H, W), None):
                got = r.ray_samples(rays, features=t if which == "features" else feats, min_sigma=0.0, image_shape=shape)
                for field in SR.Lists._fields:
                    np.testing.assert_array_equal(getattr(got, field).cpu().numpy(), getattr(want, field), err_msg=f"{field}, {which} shift {s}")
            if which == "vdirs":
                np.testing.assert_array_equal(r.view_basis(rays).cpu().numpy(), basis_want)
            if buf is not None:
                assert_guards(buf, s)


def test_sample_weights_accumulate_and_reduce_rows(gpu):
    """The per-sample operators with every float and int input shifted in turn: offsets (int64: 8, 16 and 24 bytes on), row,
    ray, length, sigma, w, values and the upstream gradients."""
    sc = scene("rgba4")
    key = ("lists", 0.0)
    if key not in sc._ref:
        sc._ref[key] = SR.lists(sc.ot, sc.rays_np(), sc.c.oracle_opts(), 0.0)
    L = sc._ref[key]
    T = L.row.shape[0]
    assert T > 1000
    rng = np.random.default_rng(21)
    sigma = (rng.exponential(20.0, T) + 1e-3).astype(np.float32)
    sigma[::5] = 0
    values = rng.uniform(-1, 1, (T, 3)).astype(np.float32)
    gw, ga = rng.standard_normal(T).astype(np.float32), rng.standard_normal(Q).astype(np.float32)
    gout = rng.uniform(-1, 1, (Q, 3)).astype(np.float32)
    w32, a32 = SR.weights(L.length, sigma, L.offsets, torch.float32)
    acc32 = SR.accumulate(w32, values, L.offsets, torch.float32).numpy()
    s64 = torch.from_numpy(sigma).double().requires_grad_(True)
    w64, a64 = SR.weights(L.length, s64, L.offsets, torch.float64)
    ((w64 * torch.from_numpy(gw).double()).sum() + (a64 * torch.from_numpy(ga).double()).sum()).backward()
    tight = SR.grad_sigma_scale(L.length, sigma, L.offsets, gw, ga)
    wd = w32.double().requires_grad_(True)
    vd = torch.from_numpy(values).double().requires_grad_(True)
    (SR.accumulate(wd, vd, L.offsets, torch.float64) * torch.from_numpy(gout).double()).sum().backward()
    M = sc.M
    red_want = {op: RR.reduce(values, L.row, M, op, empty=-1.0) for op in ("sum", "mean", "max", "min")}
    base = {k: torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for k, a in dict(
        offsets=L.offsets, ray=L.ray, row=L.row, depth=L.depth, length=L.length, sigma=sigma, w=w32.numpy(), values=values,
        grad_w=gw, grad_alpha=ga, grad_out=gout).items()}
    for which in base:
        for s, t, buf in placements(base[which]):
            a = dict(base)
            a[which] = t
            smp = svox.RaySamples(a["offsets"], a["ray"], a["row"], a["depth"], a["length"])
            sg = a["sigma"].detach().requires_grad_(True)
            w, alpha = svox.sample_weights(smp, sg)
            np.testing.assert_array_equal(w.detach().cpu().numpy(), w32.numpy(), err_msg=f"w, {which} shift {s}")
            np.testing.assert_array_equal(alpha.detach().cpu().numpy(), a32.numpy(), err_msg=f"alpha, {which} shift {s}")
            torch.autograd.backward([w, alpha], [a["grad_w"], a["grad_alpha"]])
            assert_grads_close(sg.grad.cpu().numpy(), s64.grad.numpy(), tight, what=f"grad_sigma, {which} shift {s}")
            wg = a["w"].detach().requires_grad_(True)
            vg = a["values"].detach().requires_grad_(True)
            out = svox.accumulate(smp, wg, vg)
            np.testing.assert_array_equal(out.detach().cpu().numpy(), acc32, err_msg=f"accumulate, {which} shift {s}")
            out.backward(a["grad_out"])
            assert_outputs_close(wg.grad.cpu().numpy(), wd.grad.numpy(), what=f"grad_w, {which} shift {s}")
            assert_outputs_close(vg.grad.cpu().numpy(), vd.grad.numpy(), what=f"grad_values, {which} shift {s}")
            if which in ("row", "values", "offsets"):
                for op, want in red_want.items():
                    got = svox.reduce_rows(smp, a["values"], M, op, empty=-1.0)
                    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"reduce_rows {op}, {which} shift {s}")
            if buf is not None:
                assert_guards(buf, s, which)


# ======================================================================================================================
# 4. Motion and query
# ======================================================================================================================
def test_motion_render(gpu):
    sc = scene("rgba4")
    c = sc.c
    joints = skeleton(7, 1, np.atleast_1d(c.radius) * np.ones(3), c.center)
    ot = O.Tree(sc.ot.features, sc.ot.data, sc.ot.child, sc.ot.offset, sc.ot.scaling, extra=joints)
    want = O.motion_render(ot, *sc.rays_np(), c.oracle_opts())
    assert (want[3] > 0).mean() > 0.2
    feats = c.features.to(gpu)
    jg = torch.from_numpy(joints).to(gpu)
    o, d, v = sc.rays_gpu(gpu)
    for which, source in (("features", feats), ("extra_data", jg), ("origins", o), ("dirs", d)):
        for s, t, buf in placements(source):
            tree = sc.tree(gpu)
            tree.extra_data = t if which == "extra_data" else jg
            r = svox.VolumeRenderer(tree)
            rays = svox.Rays(t if which == "origins" else o, t if which == "dirs" else d, v)
            got = r.motion_render(t if which == "features" else feats, rays, image_shape=(H, W))
            for a, b, what in zip(got, want, ("joint distances", "depth", "hit_point", "data_idx")):
                np.testing.assert_array_equal(a.cpu().numpy(), b, err_msg=f"{what}, {which} shift {s}")
            if buf is not None:
                assert_guards(buf, s, which)


@pytest.mark.parametrize("F,B", [(8, 4), (13, 3), (32, 2)])
def test_motion_feature_render(gpu, F, B):
    """Joint features (rows of 8 / 13 / 32 floats), skinning weights, int32 joint indices, the tree's table and the upstream
    gradient, each shifted in turn."""
    sc = scene("rgba4")
    c = sc.c
    J = 11
    rng = np.random.default_rng(F)
    jf = rng.normal(size=(J, F)).astype(np.float32)
    sw, ji = binding(sc.M, J, B, F)
    mo = O.Motion(jf, sw, ji)
    opt = c.oracle_opts(background_brightness=0.5)
    want = O.motion_feature_render(sc.ot, mo, *sc.rays_np(), opt)
    gout = torch.randn(Q, F, generator=torch.Generator().manual_seed(3))
    wg, wabs = O.motion_feature_render_backward(sc.ot, mo, *sc.rays_np(), opt, gout.numpy(), want_abs=True)
    tree = sc.tree(gpu)
    r = svox.VolumeRenderer(tree, background_brightness=0.5)
    base = dict(features=c.features.to(gpu), joint_features=torch.from_numpy(jf).to(gpu), skinning_weights=torch.from_numpy(sw).to(gpu),
                joint_index=torch.from_numpy(ji).to(gpu), grad_output=gout.to(gpu))
    rays = sc.rays_gpu(gpu)
    first = None
    for which in base:
        for s, t, buf in placements(base[which]):
            a = dict(base)
            a[which] = t
            jft = a["joint_features"].detach().requires_grad_(True)
            out = r.motion_feature_render(a["features"], jft, a["skinning_weights"], a["joint_index"], rays, image_shape=(H, W))
            np.testing.assert_array_equal(out.detach().cpu().numpy(), want, err_msg=f"{which} shift {s}")
            out.backward(a["grad_output"])
            assert_grads_close(jft.grad.cpu().numpy(), wg, wabs, what=f"{which} shift {s}")
            if first is None:
                first = out.detach()
            assert torch.equal(out.detach(), first)
            if buf is not None:
                assert t.data_ptr() % 16 == 4 * s
                assert_guards(buf, s, which)


def test_query_vertical_and_its_backward(gpu):
    sc = scene("sh4")
    gen = torch.Generator().manual_seed(11)
    pts = torch.rand(3000, 3, generator=gen)
    pts[:200] = torch.rand(200, 3, generator=gen) * 3 - 1
    wv, wn, wd = O.query(sc.ot, pts.numpy())
    gout = torch.randn(wv.shape, generator=gen)
    want = O.query_backward(sc.ot, pts.numpy(), gout.numpy())
    absum = O.query_backward(sc.ot, pts.numpy(), gout.abs().numpy())
    for name in ("sh4", "sh9"):                                  # rows of 13 and of 28 floats
        if name == "sh9":
            sc = scene("sh9")
            wv, wn, wd = O.query(sc.ot, pts.numpy())
            gout = torch.randn(wv.shape, generator=gen)
            want = O.query_backward(sc.ot, pts.numpy(), gout.numpy())
            absum = O.query_backward(sc.ot, pts.numpy(), gout.abs().numpy())
        tree = sc.tree(gpu)
        base = dict(features=sc.c.features.to(gpu), points=pts.to(gpu), grad_output=gout.to(gpu))
        for which in base:
            for s, t, buf in placements(base[which]):
                a = dict(base)
                a[which] = t
                f = a["features"].detach().requires_grad_(True)
                vals, node_ids, data_ids = tree(f, a["points"], want_node_ids=True, want_data_ids=True)
                np.testing.assert_array_equal(vals.detach().cpu().numpy(), wv, err_msg=f"{which} shift {s}")
                np.testing.assert_array_equal(node_ids.cpu().numpy(), wn)
                np.testing.assert_array_equal(data_ids.cpu().numpy(), wd)
                vals.backward(a["grad_output"])
                assert_grads_close(f.grad.cpu().numpy(), want, absum, what=f"{which} shift {s}")
                if buf is not None:
                    assert_guards(buf, s, which)


def test_counters_frontier_and_neighbours_with_the_int_tables_shifted(gpu):
    """The readers of the int32 tables alone: count_forward (the oracle's step / level / sample counts) with the feature table,
    child and data shifted; frontier_nodes and leaf_neighbors (their restatements, byte for byte) with child and
    parent_depth shifted."""
    from svox_t_amd.renderer import _rays_spec_from_rays
    sc = scene("rgba4")
    _, want_cnt = O.volume_render(sc.ot, *sc.rays_np(), sc.c.oracle_opts(), count=True)
    base_tree = sc.tree(gpu)
    rspec = lambda: _rays_spec_from_rays(sc.rays_gpu(gpu))              # noqa: E731
    for which, source in (("features", sc.c.features.to(gpu)), ("child", base_tree.child), ("data", base_tree.data)):
        for s, t, buf in placements(source):
            tree = sc.tree(gpu, **{which: t})
            cnt = _C.count_forward(tree._spec(tree.features), rspec(), svox.VolumeRenderer(tree)._get_options())
            assert tuple(cnt.cpu().tolist()) == tuple(want_cnt), (which, s)
            if buf is not None:
                assert_guards(buf, s, which)
    st = sc.c.st
    n, N = st.n_internal, 2
    want_fr = MR.frontier(st.child, n)
    want_nb = NR.leaf_neighbors(st.child, st.parent_depth, n, N)
    child, pd = torch.from_numpy(st.child).to(gpu), torch.from_numpy(st.parent_depth).to(gpu)
    for which in ("child", "parent_depth"):
        for s, t, buf in placements(child if which == "child" else pd):
            c_, p_ = (t, pd) if which == "child" else (child, t)
            np.testing.assert_array_equal(_C.frontier_nodes(c_, n).cpu().numpy(), want_fr)
            got = _C.leaf_neighbors(c_, p_, n, want_nb.shape[0], int(st.parent_depth[:n, 1].max()))
            assert got.dtype == torch.int32 and got.cpu().numpy().tobytes() == want_nb.tobytes(), (which, s)
            if buf is not None:
                assert_guards(buf, s, which)


def test_warp_vertices(gpu):
    mats, p, sw, ji = warp_case(Q=777, J=6, B=3, seed=777)
    wv, wm = S.warp_vertices(mats, p, sw, ji)
    gen = torch.Generator().manual_seed(1)
    gv, gm = torch.randn(777, 3, generator=gen), torch.randn(777, 4, 4, generator=gen)
    gp, gmat, gabs, gsw = S.warp_vertices_backward(mats, p, sw, ji, gv.numpy(), gm.numpy())
    base = dict(matrices=torch.from_numpy(mats).to(gpu), points=torch.from_numpy(p).to(gpu), skinning_weights=torch.from_numpy(sw).to(gpu),
                joint_index=torch.from_numpy(ji.astype(np.int32)).to(gpu), grad_vertices=gv.to(gpu), grad_matrices=gm.to(gpu))
    for which in base:
        for s, t, buf in placements(base[which]):
            a = dict(base)
            a[which] = t
            m_, p_, w_ = (a[k].detach().requires_grad_(True) for k in ("matrices", "points", "skinning_weights"))
            v, m = svox.warp_vertices(m_, p_, w_, a["joint_index"])
            np.testing.assert_array_equal(v.detach().cpu().numpy(), wv, err_msg=f"{which} shift {s}")
            np.testing.assert_array_equal(m.detach().cpu().numpy(), wm, err_msg=f"{which} shift {s}")
            torch.autograd.backward([v, m], [a["grad_vertices"], a["grad_matrices"]])
            np.testing.assert_array_equal(p_.grad.cpu().numpy(), gp)
            np.testing.assert_array_equal(w_.grad.cpu().numpy(), gsw)
            assert_grads_close(m_.grad.cpu().numpy(), gmat, gabs, what=f"{which} shift {s}")
            if buf is not None:
                assert_guards(buf, s, which)


# ======================================================================================================================
# 5. Operators that write a caller's table, with guard words
# ======================================================================================================================
def _set_inputs(gpu, K):
    """A depth-4 shell tree with K columns, points inside its leaves (several per row) and outside, values."""
    key = ("set", K)
    if key not in _BUILT:
        st = synth.shell_tree(4)
        rng = np.random.default_rng(11 + K)
        table0 = rng.standard_normal((st.n_features, K)).astype(np.float32)
        tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, table0, device=gpu)
        lb = tree.leaf_boxes()
        occ = (lb.rows >= 0).nonzero().squeeze(1)
        idx = occ.repeat(3)
        gen = torch.Generator().manual_seed(5)
        u = torch.rand((idx.shape[0], 3), generator=gen).to(gpu)
        inside = lb.corners[idx] + u * lb.lengths[idx]
        outside = tree.tree2world((torch.rand((64, 3), generator=gen) * 3.0 - 1.0).to(gpu))
        pts = torch.cat([inside, outside])
        pts = pts[torch.randperm(pts.shape[0], generator=gen).to(gpu)].contiguous()
        vals = (rng.standard_normal((pts.shape[0], K)) * 100.0).astype(np.float32)
        rows = AR.point_rows(st.child, st.data, st.n_features, pts.cpu().numpy(), tree.offset.cpu().numpy(), tree.invradius.cpu().numpy())
        assert (rows >= 0).mean() > 0.25
        _BUILT[key] = (tree, pts, vals, table0, rows)
    return _BUILT[key]


@pytest.mark.parametrize("mode", AR.MODES)
@pytest.mark.parametrize("K", [4, 8, 13])
def test_set_into_shifted_tables_and_from_shifted_values(gpu, K, mode):
    """N3Tree.set: values shifted, the table shifted, both, the points shifted.  K = 4 and 8 take the 16-byte route on
    aligned pointers and the 4-byte one otherwise; the table's neighbours keep their bits either way."""
    tree, pts, vals, table0, rows = _set_inputs(gpu, K)
    want = AR.assign(table0, rows, vals, mode)
    vals_d, table_d = torch.from_numpy(vals).to(gpu), torch.from_numpy(table0).to(gpu)
    for what in ("values", "table", "both", "points"):
        for s in (0,) + SHIFTS:
            if s == 0 and what != "values":
                continue
            v, vbuf = shifted(vals_d, s) if (s and what in ("values", "both")) else (vals_d, None)
            t, tbuf = shifted(table_d, s) if (s and what in ("table", "both")) else (table_d.clone(), None)
            p, pbuf = shifted(pts, s) if (s and what == "points") else (pts, None)
            ver = t._version
            assert tree.set(p, v, reduce=mode, features=t) is None
            assert t._version > ver
            assert np.array_equal(bits(t), bits(want)), (K, mode, what, s, int((bits(t) != bits(want)).any(1).sum()))
            for buf in (vbuf, tbuf, pbuf):
                if buf is not None:
                    assert_guards(buf, s, f"set {mode} K={K} {what}")
            if vbuf is not None:
                assert torch.equal(v, vals_d)                       # the values were only read


@pytest.mark.parametrize("K", [4, 13, 28])
def test_tv_and_tv_add_grad(gpu, K):
    """tv over a shifted table; tv_add_grad into a shifted `out` (accumulate mode: rows without an edge and the guard
    words keep their bits), from a shifted table."""
    st = synth.shell_tree(4)
    feats = synth.shell_features(st.n_features, K, seed=2)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, device=gpu)
    n, N, M = tree.filled, 2, st.n_features
    child, data, pd = tree.child.cpu().numpy(), tree.data.cpu().numpy(), tree.parent_depth.cpu().numpy()
    _, depths, _ = NR.cells(child, pd, n, N)
    pl = NR.plan(NR.leaf_neighbors(child, pd, n, N), depths, NR.leaf_rows(child, data, n, M), M)
    assert pl["E"] > 100
    cols = None
    for p, weight in ((2, "uniform"), (1, "area")):
        loss_want, G = NR.tv(feats.numpy(), pl, cols, p, weight, N)
        out0 = np.random.default_rng(3).standard_normal((M, K)).astype(np.float32)
        add_want = NR.add_grad(out0, 0.25, G, pl, cols)
        fg = feats.to(gpu)
        for s, f, buf in placements(fg):
            fr = f.detach().requires_grad_(True)
            loss = tree.tv(fr, p=p, weight=weight)
            assert np.array_equal(bits(loss.detach().reshape(1)), bits(np.asarray(loss_want).reshape(1))), (p, weight, s)
            loss.backward()
            assert np.array_equal(bits(fr.grad), bits(G)), (p, weight, s)
            if buf is not None:
                assert_guards(buf, s, "tv")
            for so, out, obuf in placements(torch.from_numpy(out0).to(gpu)):
                ver = out._version
                tree.tv_add_grad(out, 0.25, features=f, p=p, weight=weight)
                assert out._version > ver
                assert np.array_equal(bits(out), bits(add_want)), (p, weight, s, so)
                if obuf is not None:
                    assert_guards(obuf, so, "tv_add_grad out")


def test_frontier_reductions_with_a_shifted_table_and_out(gpu):
    """reduce_frontier / max_frontier / diam_frontier over a shifted table, and csrc.frontier_reduce into a shifted out=."""
    st = synth.shell_tree(4)
    for K in (4, 8, 13, 32):
        feats = synth.shell_features(st.n_features, K, seed=K)
        tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, device=gpu)
        n = tree.filled
        nodes = MR.frontier(st.child, n)
        assert nodes.size > 50
        np.testing.assert_array_equal(tree.frontier().cpu().numpy(), nodes)
        fg = feats.to(gpu)
        wants = {(op, empty): MR.reduce(feats.numpy(), st.data, n, nodes, op, None, empty)[0]
                 for op in ("mean", "sum", "max", "min") for empty in ("zero", "skip")}
        want_diam = MR.diam(feats.numpy(), st.data, n, nodes, None, "zero", 1.0)
        for s, f, buf in placements(fg):
            for (op, empty), want in wants.items():
                got = tree.reduce_frontier(op, features=f, empty=empty)
                assert np.array_equal(bits(got), bits(want)), (K, op, empty, s)
                for so in SHIFTS:
                    out, obuf = shifted(torch.zeros_like(got), so)
                    ret = _C.frontier_reduce(f, tree.data, n, 2, tree.frontier(), None, op, empty, out=out)
                    assert ret.data_ptr() == out.data_ptr() and np.array_equal(bits(out), bits(want)), (K, op, empty, s, so)
                    assert_guards(obuf, so, "frontier_reduce out")
            diam = tree.diam_frontier(features=f)
            err = np.abs(diam.cpu().numpy().astype(np.float64) - want_diam)         # (the bound of tests/test_gpu_merge.py)
            assert (err <= (K + 4) * 2.0 ** -23 * want_diam).all(), (K, s)
            if s == 0:
                first_diam = diam
            assert torch.equal(diam, first_diam), (K, s)
            if buf is not None:
                assert_guards(buf, s, "frontier")
        for s in SHIFTS:                                        # the data words: their address chooses the library's route too
            dview, dbuf = shifted(tree.data, s)
            assert torch.equal(_C.frontier_diam(fg, dview, n, 2, tree.frontier()), first_diam), (K, s)
            for (op, empty), want in wants.items():
                assert np.array_equal(bits(_C.frontier_reduce(fg, dview, n, 2, tree.frontier(), None, op, empty)), bits(want)), (K, op, s)
            assert_guards(dbuf, s, "frontier data")


@pytest.mark.parametrize("K", [4, 13, 32])
@pytest.mark.parametrize("op", ["prune", "subdivide", "merge", "quantize"])
def test_tree_surgery_on_a_shifted_feature_table(gpu, op, K):
    """prune / subdivide / merge / quantize read the old table (its rows are gathered, reduced or clustered) and install a
    new one.  On a tree whose table is a shifted view: the restatement's tables, row map and feature bits (quantize: its
    ids, colours within one ulp, as tests/test_gpu_quantize.py asks), the aligned run's bits, and the old table and its
    guard words as they were."""
    st = synth.shell_tree(4)
    child, data, pd, n, M = st.child, st.data, st.parent_depth, st.n_internal, st.n_features
    feats = synth.shell_features(M, K, seed=K + 1)
    fnp = feats.numpy()
    rng = np.random.default_rng(K)
    keep, sel = rng.random(child.shape) < 0.6, rng.random(child.shape) < 0.3
    if op == "prune":
        want = PRUNE.prune(child, data, pd, n, M, keep=keep)
        want_tables, want_n, want_map, want_feats = want[:3], want[3], want[4], fnp[want[4]]
    elif op == "subdivide":
        want = SUBD.subdivide(child, data, pd, n, M, sel=sel, own_rows=True)
        want_tables, want_n, want_map, want_feats = want[:3], n + want[3], want[5], fnp[want[5]]
        assert want[3] > 0 and want[4] > 0
    elif op == "merge":
        want = MR.merge(child, data, pd, n, fnp, MR.frontier(child, n), op="mean")
        want_tables, want_n, want_map, want_feats = want[:3], want[3], want[5], want[4]
        assert want[3] < n
    else:
        want_colors, want_ids, *_ = QUANT.quantize(fnp, None, 4)
    first = None
    dg = torch.from_numpy(data).to(gpu)                     # (the int32 words: read, remapped or rewritten in place)
    cases = [("features", s_, t_, dg.clone(), b_) for s_, t_, b_ in placements(feats.to(gpu))] + \
            [("data", s_, feats.to(gpu)) + shifted(dg, s_) for s_ in SHIFTS]
    for which, s, table, dwords, buf in cases:
        before = table.clone()
        tree = svox.N3Tree.from_arrays(torch.from_numpy(child).to(gpu), dwords, pd, table, device=gpu)
        assert tree.features.data_ptr() == table.data_ptr() and (which == "data" or table.data_ptr() % 16 == 4 * s)
        assert tree.data.data_ptr() == dwords.data_ptr() and (which == "features" or dwords.data_ptr() % 16 == 4 * s)
        if op == "quantize":
            res = tree.quantize(4)
            np.testing.assert_array_equal(res.color_id_map.cpu().numpy(), want_ids)
            err = np.abs(res.colors.cpu().numpy().astype(np.float64) - want_colors.astype(np.float64))
            assert (err <= np.spacing(np.abs(want_colors)).astype(np.float64)).all(), (K, s)
            got = (tree.features.detach().clone(), tree.data.clone(), res.color_id_map)
        else:
            res = tree.prune(torch.from_numpy(keep).to(gpu)) if op == "prune" else \
                tree.subdivide(torch.from_numpy(sel).to(gpu)) if op == "subdivide" else tree.merge(op="mean")
            m = tree.filled
            assert m == want_n
            for g_, w_, what in zip((tree.child, tree.data, tree.parent_depth), want_tables, ("child", "data", "parent_depth")):
                np.testing.assert_array_equal(g_[:m].cpu().numpy().reshape(w_[:m].shape), w_[:m], err_msg=f"{op} {what} shift {s}")
            np.testing.assert_array_equal(res.row_map.cpu().numpy(), want_map)
            assert np.array_equal(bits(tree.features), bits(want_feats)), (op, K, s)
            got = (tree.features.detach().clone(), tree.child[:m].clone(), tree.data[:m].clone(), res.row_map)
        if first is None:
            first = got
        assert all(torch.equal(x, y) for x, y in zip(got, first)), (op, K, s)
        assert tree.features.data_ptr() != table.data_ptr() and torch.equal(table, before)      # a new table; the old one was only read
        if buf is not None:
            assert_guards(buf, s, op)


def test_unshare_rewrites_a_shifted_data_table_in_place(gpu):
    """unshare_rows writes the int32 data words in place: the restatement's words and row map on a table (and under a
    child table) 4, 8 and 12 bytes on, the guard words untouched.  leaf_boxes (leaf_corners) reads child and parent_depth:
    the bits of the CPU walk, as in tests/test_gpu_assign.py."""
    st = synth.shell_tree(4)
    child, data, n, M = st.child, st.data, st.n_internal, st.n_features
    words = data.astype(np.int64) & 0xFFFFFFFF
    shared = np.where(words < M, words // 3, words).astype(np.uint32).view(np.int32).reshape(data.shape)
    want_data, want_rows, want_map = SUBD.unshare(child, shared, n, M)
    assert want_rows > 0
    cg, dg = torch.from_numpy(child).to(gpu), torch.from_numpy(shared).to(gpu)
    for which in ("data", "child"):
        for s in (0,) + SHIFTS:
            c_, cbuf = shifted(cg, s) if (s and which == "child") else (cg, None)
            d_, dbuf = shifted(dg, s) if (s and which == "data") else (dg.clone(), None)
            rows_added, row_map = _C.unshare_rows(c_, d_, n, M)
            assert rows_added == want_rows, (which, s)
            np.testing.assert_array_equal(row_map.cpu().numpy(), want_map)
            np.testing.assert_array_equal(d_.cpu().numpy().reshape(want_data.shape), want_data, err_msg=f"{which} shift {s}")
            for buf in (cbuf, dbuf):
                if buf is not None:
                    assert_guards(buf, s, f"unshare {which}")
    tree, _, _, _, _ = _set_inputs(gpu, 4)
    leaves = tree._all_leaves()
    want = tree.clone(device="cpu")._calc_corners(leaves)              # the CPU walk of parent_depth to the root
    for which in ("child", "parent_depth"):
        for s, t, buf in placements(tree.child if which == "child" else tree.parent_depth):
            t2 = svox.N3Tree.from_arrays(t if which == "child" else tree.child, tree.data, t if which == "parent_depth" else tree.parent_depth,
                                         tree.features.detach(), device=gpu)
            assert (t2.child if which == "child" else t2.parent_depth).data_ptr() == t.data_ptr()
            lb = t2.leaf_boxes(world=False)
            assert torch.equal(lb.leaf_node.cpu(), leaves) and np.array_equal(bits(lb.corners), bits(want)), (which, s)
            if buf is not None:
                assert_guards(buf, s, f"leaf_boxes {which}")


def test_accumulate_weights_into_a_shifted_table(gpu):
    sc = scene("rgba4")
    tree = sc.tree(gpu)
    r = svox.VolumeRenderer(tree)
    rays = sc.rays_gpu(gpu)
    want_out, want = O.volume_render_weights(sc.ot, *sc.rays_np(), sc.c.oracle_opts())
    assert want.sum() > 0
    for s in (0,) + SHIFTS:
        with torch.no_grad(), tree.accumulate_weights() as acc:
            buf = None
            if s:
                view, buf = shifted(torch.zeros(tree.child.shape, device=gpu), s)
                tree._weight_accum = acc.weight_accum = view
            out = r(tree.features, rays)
            got = acc.value.double().cpu().numpy()
        np.testing.assert_array_equal(out.cpu().numpy(), want_out)
        assert (got[want[:got.shape[0]] == 0] == 0).all()
        np.testing.assert_allclose(got, want[:got.shape[0]], rtol=1e-6, atol=0)
        if buf is not None:
            assert_guards(buf, s, "_weight_accum")


# ======================================================================================================================
# 6. voxelize and grid_weights
# ======================================================================================================================
def test_voxelize_with_points_and_features_shifted(gpu):
    n, P, F = 17, 1000, 4
    rng = np.random.default_rng(7)
    dirs = rng.normal(size=(P, 3))
    pts = (0.5 + 0.35 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    feats = (rng.random(size=(P, F)) + 0.5).astype(np.float32)
    corner, size = (0, 0, 0), (1, 1, 1)
    vs = 1.0 / (n - 1)
    cr, kr = 2.0 * vs, vs
    go = rng.normal(size=(n, n, n, 1)).astype(np.float32)
    pr = PV.pairs(pts, corner, size, n, cr)
    vol, scale, pg_w, pabs, fg_w, fabs = PV.forward_backward(pts, feats, pr, corner, size, n, kr, go)
    base = dict(points=torch.from_numpy(pts).to(gpu), features=torch.from_numpy(feats).to(gpu), grad_output=torch.from_numpy(go).to(gpu))
    first = None
    for which in base:
        for s, t, buf in placements(base[which]):
            a = dict(base)
            a[which] = t
            got = _C.p2v(a["points"], a["features"], corner, size, n, kr, cr)
            assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - vol) <= 1e-5 * scale)
            pg, fg = _C.p2v_backward(a["grad_output"], a["points"], a["features"], corner, size, n, kr, cr)
            assert np.all(np.abs(pg.cpu().numpy().astype(np.float64) - pg_w) <= 1e-6 * pabs)
            assert np.all(np.abs(fg.cpu().numpy().astype(np.float64)[:, F - 1] - fg_w) <= 1e-6 * fabs)
            if first is None:
                first = (got, pg, fg)
            assert all(torch.equal(x, y) for x, y in zip((got, pg, fg), first)), (which, s)       # deterministic, both ways
            pr_, fr_ = a["points"].detach().requires_grad_(True), a["features"].detach().requires_grad_(True)
            svox.voxelize(pr_, fr_, corner, size, n, kr, cr).backward(a["grad_output"])
            assert torch.equal(pr_.grad, first[1]) and torch.equal(fr_.grad, first[2])
            if buf is not None:
                assert_guards(buf, s, which)


def test_grid_weights_with_volume_cameras_and_out_shifted(gpu):
    R, Wg, Hg, f = 16, 24, 24, 1.2 * 24
    geom = ((0.5, 0.52, 0.47), (0.5, 0.4, 0.45))
    sigma = GR.shell_sigma(R, seed=R + Wg, scale=0.6 * R)
    off, sc_ = (np.asarray(v, np.float64) for v in geom)
    centre = (0.5 - off) / sc_
    cams = []
    for direction in ((1.0, 0.4, 0.3), (-0.5, 0.7, 0.6)):
        dvec = np.asarray(direction, np.float64)
        cams.append(GR.look_at(centre + 1.5 * dvec / np.linalg.norm(dvec) / sc_, centre))
    c2w = np.ascontiguousarray(np.stack([np.asarray(c, np.float32) for c in cams]))
    want = GR.march_cameras(sigma, c2w, f, f, Wg, Hg, geom[0], geom[1])            # max / sum over both views
    assert want.hits.sum() > 0
    base = dict(sigma=torch.from_numpy(sigma).to(gpu), cameras=torch.from_numpy(c2w).to(gpu))
    kw = dict(fx=f, fy=f, width=Wg, height=Hg, offset=list(geom[0]), scaling=list(geom[1]))
    for which in ("sigma", "cameras", "out"):
        for s in (0,) + SHIFTS:
            a = dict(base)
            bufs = []
            if s and which != "out":
                a[which], b = shifted(base[which], s)
                bufs.append(b)
            out = None
            if which == "out":
                zw, zh = torch.zeros(sigma.shape, device=gpu), torch.zeros(sigma.shape, device=gpu)
                if s:
                    (zw, b1), (zh, b2) = shifted(zw, s), shifted(zh, s)
                    bufs += [b1, b2]
                out = (zw, zh)
            res = svox.grid_weights(a["sigma"], cameras=a["cameras"], out=out, **kw)
            assert np.array_equal(res.hits.cpu().numpy().astype(np.int64), want.hits), (which, s)
            assert np.array_equal(bits(res.weight), bits(want.weight.astype(np.float32))), (which, s)
            if out is not None:
                assert res.weight.data_ptr() == out[0].data_ptr()
            for b in bufs:
                assert_guards(b, s, f"grid_weights {which}")


# ======================================================================================================================
# 7. The cache does not go stale
# ======================================================================================================================
@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("name", ["rgba32", "rgba8", "sh9"])
def test_caches_on_a_shifted_table_do_not_go_stale(gpu, name, held):
    """static_features on a shifted table (and inside features_held()): the second render is served from the cache exactly
    where the aligned table's is; after features.mul_(0.5) the render is the oracle's for the new values."""
    sc = scene(name)
    rays = sc.rays_gpu(gpu)
    opt = sc.c.oracle_opts()
    want0 = sc.forward_ref(False)
    halved = O.Tree((sc.c.features * 0.5).numpy(), sc.ot.data, sc.ot.child, offset=sc.ot.offset, scaling=sc.ot.scaling,
                    extra=sc.ot.extra)
    want1 = O.volume_render(halved, *sc.rays_np(), opt)
    assert not np.array_equal(want0, want1)

    def builds(f):
        """How many (mask / table) builds a second render of the same table costs: 0 when served from the cache."""
        ent = _C._SIGMA_CACHE.get(id(f))
        return None if ent is None else (ent[3].data_ptr(), None if ent[4] is None else ent[4].data_ptr())

    served = {}
    for s in (0,) + SHIFTS:
        _C.invalidate_caches()
        f, buf = shifted(sc.c.features.to(gpu), s) if s else (sc.c.features.to(gpu), None)
        tree = sc.tree(gpu, features=f)
        f = tree.features                                       # (the Parameter from_arrays made of the view: the same storage)
        assert f.data_ptr() % 16 == 4 * s
        tree.static_features = not held
        r = svox.VolumeRenderer(tree)
        ctx = _C.features_held() if held else torch.no_grad()
        with torch.no_grad(), ctx:
            a = r(f, rays, image_shape=(H, W))
            first = builds(f)
            b = r(f, rays, image_shape=(H, W))
            second = builds(f)
            np.testing.assert_array_equal(a.cpu().numpy(), want0)
            assert torch.equal(a, b)
            served[s] = (first is not None, first == second)
            assert served[s] == served[0], (name, held, s, served)
            if first is not None:
                # the cache knows the CALLER's tensor, not the aligned copy handed to the kernels
                ent = _C._SIGMA_CACHE[id(f)]
                assert ent[0]() is f and ent[1] == (f._version, f.data_ptr())
            if not held:
                f.mul_(0.5)
                c2 = r(f, rays, image_shape=(H, W))
                np.testing.assert_array_equal(c2.cpu().numpy(), want1, err_msg=f"{name} shift {s}: a stale copy was served")
        if held:
            assert id(f) not in _C._SIGMA_CACHE                 # dropped when the block ended
            with torch.no_grad():
                f.mul_(0.5)
                with _C.features_held():
                    c2 = r(f, rays, image_shape=(H, W))
                    np.testing.assert_array_equal(c2.cpu().numpy(), want1, err_msg=f"{name} shift {s}: a stale copy was served")
                    assert torch.equal(r(f, rays, image_shape=(H, W)), c2)
        if buf is not None:
            assert_guards(buf, s)
    if name != "sh9":
        assert served[0] == (True, True), served                # rows of 8 / 32 floats: mask and exponentials table, cached
    _C.invalidate_caches()


def test_a_flat_view_of_rows_of_32_floats_renders_by_the_exponentials_table_route(gpu):
    """VolumeRenderer.forward(flat[1:].view(M, 32), rays): the oracle's bits, by the exponentials table's route."""
    sc = scene("rgba32")
    tree = sc.tree(gpu)
    flat = torch.cat([torch.zeros(1), sc.c.features.reshape(-1)]).to(gpu)
    f = flat[1:].view(sc.M, 32)
    assert f.is_contiguous() and f.data_ptr() % 16 == 4
    with torch.no_grad():
        out = svox.VolumeRenderer(tree)(f, sc.rays_gpu(gpu))
    np.testing.assert_array_equal(out.cpu().numpy(), sc.forward_ref(False))
    assert "shade_chan_kernel" in _C.LAST_ROUTE["forward"], _C.LAST_ROUTE


# ======================================================================================================================
# 8. The builders, the plans and the remaining readers; coverage cannot shrink silently
# ======================================================================================================================
def test_build_octree_and_construct_tree(gpu):
    """build_octree from shifted points (offset, scaling): the oracle builder's three tables.  construct_tree writes the
    data words in place: the builder's words in a shifted table, from shifted points, the guard words untouched."""
    from oracle import builder as ob
    from tests.test_gpu_builder import cloud
    depth, P = 5, 3000
    pts = cloud(P, seed=depth * 1000 + P)
    tree0 = svox.N3Tree(N=2, data_dim=4, map_location=gpu)
    off, sc = tree0.offset, tree0.invradius
    want_child, want_data, want_pd = ob.build_from_points(pts, off.cpu().numpy(), sc.cpu().numpy(), depth)
    n = want_child.shape[0]
    pg = torch.from_numpy(pts).to(gpu)
    for which, source in (("points", pg), ("offset", off), ("scaling", sc)):
        for s, t, buf in placements(source):
            child, data, pd, cnt = _C.build_octree(t if which == "points" else pg, t if which == "offset" else off,
                                                   t if which == "scaling" else sc, depth, svox.svox.EMPTY_INDEX, 0)
            assert cnt == n, (which, s)
            np.testing.assert_array_equal(child[:n].cpu().numpy(), want_child)
            np.testing.assert_array_equal(pd[:n].cpu().numpy(), want_pd)
            np.testing.assert_array_equal(data[:n].cpu().numpy().reshape(want_data.shape), want_data)
            if buf is not None:
                assert_guards(buf, s, f"build_octree {which}")
    empty = torch.full((n, 2, 2, 2, 1), svox.svox.EMPTY_INDEX, dtype=torch.int32, device=gpu)
    for which in ("data", "points", "child"):
        for s in (0,) + SHIFTS:
            d_, dbuf = shifted(empty, s) if (s and which == "data") else (empty.clone(), None)
            p_, pbuf = shifted(pg, s) if (s and which == "points") else (pg, None)
            c_, cbuf = shifted(torch.from_numpy(want_child).to(gpu), s) if (s and which == "child") else (torch.from_numpy(want_child).to(gpu), None)
            tree = svox.N3Tree.from_arrays(c_, d_, want_pd, torch.zeros(P, 4, device=gpu), device=gpu)
            assert tree.data.data_ptr() == d_.data_ptr() and tree.child.data_ptr() == c_.data_ptr()
            tree.construct_tree(p_)
            np.testing.assert_array_equal(tree.data[:n].cpu().numpy().reshape(want_data.shape), want_data, err_msg=f"{which} shift {s}")
            for buf in (dbuf, pbuf, cbuf):
                if buf is not None:
                    assert_guards(buf, s, f"construct_tree {which}")


def test_refine_leaves_writes_shifted_tables_in_place(gpu):
    """refine_leaves: the tables N3Tree.refine writes with tensor ops on the CPU, bit for bit, with each of child, data,
    parent_depth (written in place) and leaf_node (int64) shifted in turn."""
    st = synth.shell_tree(3)
    cpu = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, torch.zeros(st.n_features, 4))
    leaves = cpu._all_leaves()[::5].long().contiguous()
    cpu._resize_add_cap(leaves.shape[0])
    n = cpu.filled
    assert cpu.capacity >= n + leaves.shape[0]
    before = {"child": cpu.child.clone(), "data": cpu.data.clone(), "parent_depth": cpu.parent_depth.clone(), "leaf_node": leaves}
    cpu.refine(sel=tuple(leaves.T), leaf_node=leaves)
    want = {"child": cpu.child, "data": cpu.data, "parent_depth": cpu.parent_depth}
    assert cpu.filled == n + leaves.shape[0] and not torch.equal(want["child"], before["child"])
    for which in before:
        for s in (0,) + SHIFTS:
            a = {k: v.to(gpu).clone() for k, v in before.items()}
            buf = None
            if s:
                a[which], buf = shifted(a[which], s)
            _C.refine_leaves(a["child"], a["data"], a["parent_depth"], n, a["leaf_node"])
            for k in want:
                assert torch.equal(a[k].cpu(), want[k]), (which, s, k)
            if buf is not None:
                assert_guards(buf, s, f"refine_leaves {which}")


def test_snap_points_and_count_touched(gpu):
    """snap_points with the points, child, data and parent_depth shifted: the corner of the oracle's leaf by the CPU walk.
    count_touched with the feature table and the rays shifted: the distinct rows of the restatement's sample lists."""
    from svox_t_amd.renderer import _rays_spec_from_rays
    sc = scene("rgba4")
    gen = torch.Generator().manual_seed(11)
    pts = torch.rand(2000, 3, generator=gen)
    pts[:100] = torch.rand(100, 3, generator=gen) * 3 - 1                  # some outside the cube: clamped
    _, wn, _ = O.query(sc.ot, pts.numpy())
    cpu = sc.c.tree()
    want = cpu._calc_corners(cpu._unpack_index(torch.from_numpy(np.asarray(wn)).long()))      # (offset 0, scaling 1: world = tree)
    base = sc.tree(gpu)
    sources = {"points": pts.to(gpu), "child": base.child, "data": base.data, "parent_depth": base.parent_depth}
    for which, source in sources.items():
        for s, t, buf in placements(source):
            tree = sc.tree(gpu, **({which: t} if which in ("child", "data") else {}))
            if which == "parent_depth":
                tree.parent_depth = t
            got = tree.snap(t if which == "points" else sources["points"])
            assert np.array_equal(bits(got), bits(want)), (which, s)
            if buf is not None:
                assert_guards(buf, s, f"snap {which}")
    rows_valid = np.unique(SR.lists(sc.ot, sc.rays_np(), sc.c.oracle_opts(), None).row).size
    rows_composited = np.unique(SR.lists(sc.ot, sc.rays_np(), sc.c.oracle_opts(), 0.0).row).size
    o, d, v = sc.rays_gpu(gpu)
    first = None
    for which, source in (("features", sc.c.features.to(gpu)), ("origins", o), ("dirs", d)):
        for s, t, buf in placements(source):
            tree = sc.tree(gpu, **({"features": t} if which == "features" else {}))
            rays = svox.Rays(t if which == "origins" else o, t if which == "dirs" else d, v)
            got = _C.count_touched(tree._spec(tree.features), _rays_spec_from_rays(rays), svox.VolumeRenderer(tree)._get_options())
            assert (got["rows_valid"], got["rows_composited"]) == (rows_valid, rows_composited), (which, s, got)
            first = first or got
            assert got == first, (which, s)
            if buf is not None:
                assert_guards(buf, s, f"count_touched {which}")


def test_tv_plan_and_frontier_reduce_backward(gpu):
    """tv_plan from shifted neighbours, depths (int32) and rows (int64): the restatement's plan, byte for byte.
    frontier_reduce_backward with the table, the data words and the upstream gradient shifted, on a tree whose leaves each
    own a row: torch autograd over the gathered rows, bit for bit (tests/test_gpu_merge.py)."""
    from tests.test_gpu_merge import gathered, torch_reduce
    st = synth.shell_tree(4)
    n, N, M = st.n_internal, 2, st.n_features
    _, depths, _ = NR.cells(st.child, st.parent_depth, n, N)
    nb, rows = NR.leaf_neighbors(st.child, st.parent_depth, n, N), NR.leaf_rows(st.child, st.data, n, M)
    pl = NR.plan(nb, depths, rows, M)
    base = dict(neighbors=torch.from_numpy(np.ascontiguousarray(nb, np.int32)).to(gpu),
                depths=torch.from_numpy(np.ascontiguousarray(depths, np.int32)).to(gpu),
                rows=torch.from_numpy(np.ascontiguousarray(rows, np.int64)).to(gpu))
    for which in base:
        for s, t, buf in placements(base[which]):
            a = dict(base)
            a[which] = t
            mine = _C.tv_plan(a["neighbors"], a["depths"], a["rows"], M, N)
            assert mine.E == pl["E"] > 100
            for nm in ("row_ptr", "other", "meta"):
                assert getattr(mine, nm).cpu().numpy().tobytes() == pl[nm].tobytes(), (which, s, nm)
            if buf is not None:
                assert_guards(buf, s, f"tv_plan {which}")
    for K in (4, 13):
        feats = synth.shell_features(M, K, seed=K)
        tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, device=gpu)
        nodes = tree.frontier()
        for op in ("mean", "sum", "max", "min"):
            for empty in ("zero", "skip"):
                f2 = feats.to(gpu).requires_grad_(True)
                rws, has, _ = gathered(tree, f2, None)
                res = torch_reduce(rws, has, op, empty, tensor_count=True)
                gout = torch.randn(res.shape, generator=torch.Generator().manual_seed(1)).to(gpu)
                res.backward(gout)
                assert int((f2.grad != 0).sum()) > 100
                srcs = dict(features=feats.to(gpu), data=tree.data, grad_out=gout)
                for which in srcs:
                    for s, t, buf in placements(srcs[which]):
                        a = dict(srcs)
                        a[which] = t
                        got = _C.frontier_reduce_backward(a["features"], a["data"], n, N, nodes, None, op, empty, a["grad_out"])
                        assert torch.equal(got, f2.grad), (K, op, empty, which, s)
                        if buf is not None:
                            assert_guards(buf, s, f"frontier_reduce_backward {which}")


def test_ray_order_of_shifted_rays(gpu):
    """ray_order with origins and dirs shifted: a permutation with the rays that miss the cube last (its own test's
    properties); the batch rendered in that order gives the oracle's bits at every ray's own row."""
    from svox_t_amd.renderer import _rays_spec_from_rays
    sc = scene("sh9")
    tree = sc.tree(gpu)
    r = svox.VolumeRenderer(tree)
    o, d, v = (a.copy() for a in sc.rays_np("shuffled"))
    o[:50] += 10.0
    want = O.volume_render(sc.ot, o, d, v, sc.c.oracle_opts())
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    inv = 1.0 / (dn.astype(np.float64) + 1e-9)
    t1, t2 = -o * inv, (1.0 - o) * inv
    miss = np.maximum(t1, t2).min(axis=1) < np.maximum(np.minimum(t1, t2).max(axis=1), 0.0)
    assert miss[:50].all() and 50 <= miss.sum() < Q
    og, dg, vg = (torch.from_numpy(x).to(gpu) for x in (o, d, v))
    for which, source in (("origins", og), ("dirs", dg)):
        for s, t, buf in placements(source):
            rays = svox.Rays(t if which == "origins" else og, t if which == "dirs" else dg, vg)
            perm = _C.ray_order(tree._spec(tree.features), _rays_spec_from_rays(rays), r._get_options()).cpu().numpy()
            assert sorted(perm.tolist()) == list(range(Q)), (which, s)
            assert set(perm[Q - miss.sum():].tolist()) == set(np.nonzero(miss)[0].tolist()), (which, s)
            with torch.no_grad():
                np.testing.assert_array_equal(r(tree.features, rays, sort_rays=True).cpu().numpy(), want)
            if buf is not None:
                assert_guards(buf, s, f"ray_order {which}")


# operator of svox_t_amd.csrc -> (the tests here that run it on shifted input, the arguments they shift)
RENDER_TESTS = ("test_colour_render_with_the_feature_table_shifted test_colour_render_with_one_other_argument_shifted "
                "test_colour_render_with_extra_data_and_the_camera_matrix_shifted test_view_rotations_with_the_table_and_the_matrices_shifted "
                "test_accumulate_weights_into_a_shifted_table")
COVERED = {
    "volume_render": (RENDER_TESTS, "features origins dirs vdirs child data offset scaling extra_data "
                      "transformation_matrices _weight_accum"),
    "volume_render_backward": (RENDER_TESTS, "features origins dirs vdirs grad_output child data offset "
                               "scaling extra_data transformation_matrices"),
    "volume_render_backward_rows": ("test_colour_render_with_the_feature_table_shifted", "features"),
    "volume_render_image": ("test_colour_render_with_extra_data_and_the_camera_matrix_shifted", "features c2w"),
    "volume_render_image_backward": ("test_colour_render_with_extra_data_and_the_camera_matrix_shifted", "features c2w"),
    "opacity_render": ("test_sigma_only_operators_and_the_camera_with_the_feature_table_shifted", "features"),
    "opacity_render_backward": ("test_sigma_only_operators_and_the_camera_with_the_feature_table_shifted", "features"),
    "render_depth": ("test_sigma_only_operators_and_the_camera_with_the_feature_table_shifted", "features"),
    "depth_moments": ("test_per_ray_sigma_operators", "features origins dirs"),
    "depth_moments_backward": ("test_per_ray_sigma_operators", "features origins dirs grad_output"),
    "distortion": ("test_per_ray_sigma_operators", "features origins dirs"),
    "distortion_backward": ("test_per_ray_sigma_operators", "features origins dirs grad_output"),
    "ray_samples": ("test_ray_samples_and_view_basis", "features origins dirs vdirs"),
    "view_basis": ("test_ray_samples_and_view_basis", "vdirs"),
    "sample_weights": ("test_sample_weights_accumulate_and_reduce_rows", "offsets length sigma"),
    "sample_weights_backward": ("test_sample_weights_accumulate_and_reduce_rows", "offsets length sigma grad_w grad_alpha"),
    "sample_accumulate": ("test_sample_weights_accumulate_and_reduce_rows", "offsets w values"),
    "sample_accumulate_backward": ("test_sample_weights_accumulate_and_reduce_rows", "ray w values grad_out"),
    "sample_reduce_rows": ("test_sample_weights_accumulate_and_reduce_rows", "row values"),
    "row_plan": ("test_sample_weights_accumulate_and_reduce_rows", "row"),
    "motion_render": ("test_motion_render", "features extra_data origins dirs"),
    "motion_feature_render": ("test_motion_feature_render", "features joint_features skinning_weights joint_index"),
    "motion_feature_render_backward": ("test_motion_feature_render", "features joint_features skinning_weights joint_index grad_output"),
    "query_vertical": ("test_query_vertical_and_its_backward", "features indices"),
    "query_vertical_backward": ("test_query_vertical_and_its_backward", "features indices grad_output"),
    "warp_vertices": ("test_warp_vertices", "matrices indices skinning_weights joint_index"),
    "warp_vertices_backward": ("test_warp_vertices", "matrices indices skinning_weights joint_index grad_vertices grad_matrices"),
    "count_forward": ("test_counters_frontier_and_neighbours_with_the_int_tables_shifted", "features child data"),
    "count_touched": ("test_snap_points_and_count_touched", "features origins dirs"),
    "frontier_nodes": ("test_counters_frontier_and_neighbours_with_the_int_tables_shifted", "child"),
    "leaf_neighbors": ("test_counters_frontier_and_neighbours_with_the_int_tables_shifted", "child parent_depth"),
    "assign_leaves": ("test_set_into_shifted_tables_and_from_shifted_values", "values features indices"),
    "tv_rows": ("test_tv_and_tv_add_grad", "features out"),
    "tv_plan": ("test_tv_plan_and_frontier_reduce_backward", "neighbors depths rows"),
    "frontier_reduce": ("test_frontier_reductions_with_a_shifted_table_and_out", "features data out"),
    "frontier_diam": ("test_frontier_reductions_with_a_shifted_table_and_out", "features data"),
    "frontier_reduce_backward": ("test_tv_plan_and_frontier_reduce_backward", "features data grad_out"),
    "prune_tree": ("test_tree_surgery_on_a_shifted_feature_table", "data"),
    "gather_rows": ("test_tree_surgery_on_a_shifted_feature_table", "src"),
    "subdivide_tree": ("test_tree_surgery_on_a_shifted_feature_table", "data"),
    "merge_tree": ("test_tree_surgery_on_a_shifted_feature_table", "features data"),
    "quantize_median_cut": ("test_tree_surgery_on_a_shifted_feature_table", "data"),
    "remap_index": ("test_tree_surgery_on_a_shifted_feature_table", "data"),
    "unshare_rows": ("test_unshare_rewrites_a_shifted_data_table_in_place", "child data"),
    "leaf_corners": ("test_unshare_rewrites_a_shifted_data_table_in_place", "child parent_depth"),
    "snap_points": ("test_snap_points_and_count_touched", "indices child data parent_depth"),
    "refine_leaves": ("test_refine_leaves_writes_shifted_tables_in_place", "child data parent_depth leaf_node"),
    "build_octree": ("test_build_octree_and_construct_tree", "points offset scaling"),
    "construct_tree": ("test_build_octree_and_construct_tree", "data indices child"),
    "ray_order": ("test_ray_order_of_shifted_rays", "origins dirs"),
    "grid_weights": ("test_grid_weights_with_volume_cameras_and_out_shifted", "sigma cameras out"),
    "p2v": ("test_voxelize_with_points_and_features_shifted", "points point_features"),
    "p2v_order": ("test_voxelize_with_points_and_features_shifted", "points point_features"),
    "p2v_backward": ("test_voxelize_with_points_and_features_shifted", "grad_output points point_features"),
}
# operators without a caller-supplied device tensor that reaches a kernel, or covered by name in another file
EXEMPT = {
    "can_record": "a host predicate over the packed structs: nothing is launched",
    "get_out_data_dim": "takes options and an int",
    "freeze_pools": "takes a bool",
    "invalidate_caches": "drops host-side cache entries and bumps version counters: no kernel",
    "slot_decision": "host-side checks of the decision arguments of prune / subdivide: no kernel",
    "assign_vertical": "out of scope: raises (N3Tree.set / assign_leaves is the operator)",
    "calc_corners": "out of scope: raises (leaf_corners is the operator)",
    "grid_weight_render": "out of scope: raises (grid_weights is the operator)",
    "optim_step": "tests/test_gpu_optim.py::test_tables_that_are_not_16_byte_aligned_take_the_scalar_path",
    "sample_gather_rows": "tests/test_gpu_rows.py::test_gather (a table whose storage is not 16-byte aligned)",
    "shade_samples_fwd": "tests/test_gpu_shade.py::test_forward_of_a_table_that_is_not_16_byte_aligned",
    "shade_samples_bwd": "tests/test_gpu_shade.py::test_forward_of_a_table_that_is_not_16_byte_aligned (its backward reads no table: "
                         "the forward's output and the row plan)",
}


def test_every_public_operator_is_run_shifted_or_exempt():
    """Every public function of svox_t_amd.csrc is in COVERED -- with a test of this file and the arguments it shifts -- or
    in EXEMPT with a one-line reason: a new operator cannot stay out of this file unnoticed."""
    import types
    public = sorted(n for n in dir(_C) if not n.startswith("_") and isinstance(getattr(_C, n), types.FunctionType))
    assert len(public) >= 60
    assert not set(COVERED) & set(EXEMPT)
    missing = [n for n in public if n not in COVERED and n not in EXEMPT]
    assert not missing, f"run these operators on shifted input here (or exempt them with a reason): {missing}"
    stale = [n for n in list(COVERED) + list(EXEMPT) if n not in public]
    assert not stale, f"no such public operator any more: {stale}"
    for name, (tests, args) in COVERED.items():
        assert tests.split() and all(callable(globals().get(t)) and t.startswith("test_") for t in tests.split()), (name, tests)
        assert args.split(), name
    for name, reason in EXEMPT.items():
        assert reason and "\n" not in reason, name
