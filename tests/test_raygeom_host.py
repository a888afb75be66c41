"""Sample faces and sample_geometry without a GPU: the restatement (tests/raygeom_restate.py) against its own float64
yardstick within the derived bound and against central differences of the float32 march, the refusals of the Python
layer and the argument checks of the new C entry points.  The cases are built once and shared with
tests/test_gpu_raygeom.py."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import raygeom_restate as G
from tests import samples_restate as R
from tests.test_adversarial_host import adversarial
from tests.test_gpu_random_stress import random_tree
from tests.util import Case

NAMES = ("svoxt_ray_samples_emit_faces", "svoxt_sample_geometry_bwd", "svoxt_sample_weights_bwd_length")
CASES = {
    "d5_rgba4": dict(depth=5, K=4, data_format="RGBA", width=64, height=64),
    "d5_sh4_world": dict(depth=5, K=13, data_format="SH4", width=64, height=64,
                         radius=[1.0, 1.2, 0.8], center=[0.1, -0.2, 0.3]),           # delta_scale != 1
    "d5_rgba4_50x34": dict(depth=5, K=4, data_format="RGBA", width=50, height=34),
    "d5_rgba4_48x40": dict(depth=5, K=4, data_format="RGBA", width=48, height=40),
}
_BUILT = {}


class Built:
    """A case as (oracle tree, rays, options) objects that stay -- the restated march is computed once per case -- and
    a way onto the GPU."""

    def __init__(self, ot, rays, opt, make_tree, step_size=None):
        self.ot, self.rays, self.opt, self.make_tree, self.step_size = ot, rays, opt, make_tree, step_size
        self.Q = rays[0].shape[0]
        self._faces = {}

    def faces(self, min_sigma=None) -> G.FaceLists:
        if min_sigma not in self._faces:
            self._faces[min_sigma] = G.lists_with_faces(self.ot, self.rays, self.opt, min_sigma)
        return self._faces[min_sigma]

    def renderer(self, device):
        kw = {} if self.step_size is None else dict(step_size=self.step_size)
        return svox.VolumeRenderer(self.make_tree(device), **kw)

    def rays_on(self, device):
        return svox.Rays(*(torch.from_numpy(a).to(device) for a in self.rays))


def built(name) -> Built:
    if name in _BUILT:
        return _BUILT[name]
    if name in CASES:
        c = Case(**CASES[name])
        b = Built(c.oracle_tree(), c.rays_np(), c.oracle_opts(), c.tree)
    elif name == "hostile":
        a = adversarial("n2_sh4", 0)
        b = Built(a.ot, a.rays, a.opt, a.tree, step_size=float(a.opt.step_size))
    elif name == "n3":
        b = _n3()
    else:
        assert name == "mixed", name
        b = _mixed()
    _BUILT[name] = b
    return b


def _n3() -> Built:
    """random_tree with N = 3 (the generic descent), depth 3, under its own scaled and shifted cube; 40 x 40 pinhole rays."""
    from svox_t_amd import synth
    t, feats = random_tree(2, N=3, max_depth=3, data_format="RGBA", K=4)
    n = t.n_internal
    child, data, pd = t.child[:n].numpy().copy(), t.data[:n].numpy().copy(), t.parent_depth[:n].numpy().copy()
    radius, center = (0.7, 1.3, 0.9), (0.2, -0.1, 0.4)
    ot = O.Tree(feats.numpy(), data, child, offset=t.offset.numpy().copy(), scaling=t.invradius.numpy().copy())
    pose = synth.camera_pose(azimuth_deg=40.0, radius=1.6 * 2 * 1.3, center=np.asarray(center, dtype=np.float64))
    o, d, v = synth.pinhole_rays(40, 40, c2w=pose)
    opt = O.make_options(format=O.FORMAT_RGBA, basis_dim=-1)
    make = lambda device: svox.N3Tree.from_arrays(child, data, pd, feats, data_format="RGBA", radius=list(radius),      # noqa: E731
                                                  center=list(center), device=device)
    return Built(ot, (o.numpy(), d.numpy(), v.numpy()), opt, make)


def _mixed() -> Built:
    """65 + 1 rays over d5_sh4_world's tree: rays from the image, 12 origins inside the cube (entry 3), a ray along +x (two
    zero direction components), one with one zero component, 8 rays that miss, non-unit directions; the 66th ray sits in
    a second wavefront of its own."""
    c = Case(**CASES["d5_sh4_world"])
    o, d, v = (a.copy() for a in c.rays_np())
    pick = (np.arange(66) * 61 + 64 * 20 + 7) % o.shape[0]
    o, d, v = o[pick], d[pick], v[pick]
    rng = np.random.default_rng(7)
    cen, rad = np.asarray(CASES["d5_sh4_world"]["center"]), np.asarray(CASES["d5_sh4_world"]["radius"])
    o[:12] = (cen + rad * rng.uniform(-0.6, 0.6, (12, 3))).astype(np.float32)
    u = rng.standard_normal((8, 3))
    o[:8] = (cen + rad * 0.70 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)     # in the shell: the first crossing is a sample
    d[:12] = rng.standard_normal((12, 3)).astype(np.float32)
    o[12], d[12] = (cen + rad * np.array([-2.0, 0.11, -0.07])).astype(np.float32), np.array([1.0, 0.0, 0.0], np.float32)
    o[13], d[13] = (cen + rad * np.array([0.13, -2.0, 0.21])).astype(np.float32), np.array([0.0, 1.5, 0.2], np.float32)
    o[14:22] = (cen + 5.0 * rad).astype(np.float32)
    d[14:22] = np.abs(rng.standard_normal((8, 3))).astype(np.float32) + 0.1       # away from the cube
    d[22:] *= rng.uniform(0.5, 2.0, (44, 1)).astype(np.float32)
    rays = tuple(np.ascontiguousarray(a) for a in (o, d, v))
    return Built(c.oracle_tree(), rays, c.oracle_opts(), c.tree)


def random_upstream(T, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(T).astype(np.float32), rng.standard_normal(T).astype(np.float32)


def worst(got, want, bound):
    """max |got - want| / bound over the entries with a bound; entries without one must be exactly 0 on both sides."""
    got, want, bound = (np.asarray(x, dtype=np.float64) for x in (got, want, bound))
    zero = bound == 0
    assert np.all(got[zero] == 0) and np.all(want[zero] == 0)
    return float((np.abs(got - want)[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# ---------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    assert {"sample_geometry"} <= set(svox.__all__)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    err = lib.svoxt_last_error
    buf = (ctypes.c_float * 96)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd4 = ctypes.c_void_p(p.value + 4)                # 4-byte aligned, not 8
    odd1 = ctypes.c_void_p(p.value + 1)
    t = _C._CTree(features=p, M=1, K=4, N=2, data=p, child=p, n_internal=1, offset=p, scaling=p)
    o = _C._COptions(format=0, basis_dim=-1)
    r = _C._CRays(Q=64, origins=p, dirs=p, vdirs=p)
    T, Rr, Op = ctypes.byref(t), ctypes.byref(r), ctypes.byref(o)
    nan = ctypes.byref(ctypes.c_float(float("nan")))

    emit = lib.svoxt_ray_samples_emit_faces
    for a in ((None, Rr, Op), (T, None, Op), (T, Rr, None)):
        assert emit(*a, None, p, p, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit_faces" in err() and b"NULL" in err()
    assert emit(T, Rr, Op, nan, p, p, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit_faces: min_sigma is NaN" in err()
    assert emit(T, Rr, Op, None, None, p, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit_faces: offsets is NULL" in err()
    assert emit(T, Rr, Op, None, odd4, p, p, p, p, p, None) == 1 and b"offsets is not 8-byte aligned" in err()
    many = _C._CRays(Q=1 << 31, origins=p, dirs=p, vdirs=p)
    assert emit(T, ctypes.byref(many), Op, None, p, p, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit_faces: too many rays" in err()
    for i in range(5):
        outs = [p] * 5
        outs[i] = None
        assert emit(T, Rr, Op, None, p, *outs, None) == 1 and b"svoxt_ray_samples_emit_faces: row / ray / depth / length / face is NULL" in err()
    for i in range(4):
        outs = [p] * 5
        outs[i] = odd1
        assert emit(T, Rr, Op, None, p, *outs, None) == 1 and b"svoxt_ray_samples_emit_faces: row / ray / depth / length is not 4-byte" in err()

    gb, wl = lib.svoxt_sample_geometry_bwd, lib.svoxt_sample_weights_bwd_length
    for Q, Tn in ((-1, 4), (1 << 31, 4), (4, -1), (4, 1 << 31)):
        assert gb(p, Q, Tn, p, p, p, p, p, p, p, p, None) == 1 and b"svoxt_sample_geometry_bwd: " in err() and b"must be in [0, 2^31)" in err()
        assert wl(p, Q, Tn, p, p, p, p, p, p, None) == 1 and b"svoxt_sample_weights_bwd_length: " in err() and b"must be in [0, 2^31)" in err()
    for i in (0, 6, 9, 10):                            # offsets, dirs, grad_origins, grad_dirs
        a = [p] * 11
        a[i] = None
        assert gb(a[0], 4, 4, *a[3:], None) == 1 and b"svoxt_sample_geometry_bwd: offsets / dirs / grad_origins / grad_dirs is NULL" in err()
    for i in (3, 4, 5):
        a = [p] * 11
        a[i] = None
        assert gb(a[0], 4, 4, *a[3:], None) == 1 and b"svoxt_sample_geometry_bwd: face / depth / length is NULL" in err()
    for i in (0, 4, 5, 6, 7, 8, 9, 10):
        a = [p] * 11
        a[i] = odd4 if i == 0 else odd1
        assert gb(a[0], 4, 4, *a[3:], None) == 1 and b"svoxt_sample_geometry_bwd: a misaligned argument" in err()
    assert wl(None, 4, 4, p, p, p, p, p, p, None) == 1 and b"svoxt_sample_weights_bwd_length: offsets is NULL" in err()
    for i in (0, 1, 4, 5):
        a = [p] * 6
        a[i] = None
        assert wl(p, 4, 4, *a, None) == 1 and b"svoxt_sample_weights_bwd_length: length / sigma / grad_sigma / grad_length is NULL" in err()
    for i in range(7):
        a = [p] * 7
        a[i] = odd4 if i == 0 else odd1
        assert wl(a[0], 4, 4, *a[1:], None) == 1 and b"svoxt_sample_weights_bwd_length: a misaligned argument" in err()

    # an empty batch is a valid no-op
    r0 = _C._CRays(Q=0)
    assert emit(T, ctypes.byref(r0), Op, None, None, None, None, None, None, None, None) == 0
    assert gb(None, 0, 0, None, None, None, None, None, None, None, None, None) == 0
    assert wl(None, 0, 0, None, None, None, None, None, None, None) == 0
    assert wl(None, 4, 0, None, None, None, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------------- the Python layer
def cpu_samples(T=6, face=True):
    off = torch.tensor([0, 2, 2, T], dtype=torch.int64)
    ray = torch.tensor([0, 0, 2, 2, 2, 2], dtype=torch.int32)[:T]
    f = torch.full((T,), 1 | 2 << 2, dtype=torch.uint8) if face else None
    return svox.RaySamples(off, ray, torch.zeros(T, dtype=torch.int32), torch.zeros(T), torch.ones(T), f)


def test_python_layer_refusals():
    s = cpu_samples()
    assert s.face.dtype == torch.uint8 and cpu_samples(face=False).face is None
    for bad in (torch.zeros(6, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8), torch.zeros(6, 1, dtype=torch.uint8), [0] * 6):
        with pytest.raises(RuntimeError, match=r"face must be uint8 \[T\]"):
            svox.RaySamples(s.offsets, s.ray, s.row, s.depth, s.length, bad)
    rays = svox.Rays(torch.zeros(3, 3), torch.ones(3, 3), torch.ones(3, 3))
    with pytest.raises(RuntimeError, match="carry no `face`.*faces=True"):
        svox.sample_geometry(cpu_samples(face=False), rays)
    with pytest.raises(RuntimeError, match="samples must be a RaySamples"):
        svox.sample_geometry((s.offsets,), rays)
    with pytest.raises(RuntimeError, match="camera-mode and NDC rays are not served"):
        svox.sample_geometry(s, None)
    with pytest.raises(RuntimeError, match="camera-mode and NDC rays are not served"):
        svox.sample_geometry(s, (rays.origins, rays.dirs))
    for o, d in ((torch.zeros(4, 3), torch.ones(4, 3)), (torch.zeros(3, 3), torch.ones(2, 3)), (torch.zeros(3, 3, dtype=torch.float64), torch.ones(3, 3)),
                 (torch.zeros(3, 3), torch.ones(3, 4)), (torch.zeros(9), torch.ones(3, 3))):
        with pytest.raises(RuntimeError, match=r"must be float32 \[Q, 3\] with Q = 3"):
            svox.sample_geometry(s, svox.Rays(o, d, d))
    with pytest.raises(RuntimeError, match="GPU"):
        svox.sample_geometry(s, rays)
    # sample_weights(length=)
    for bad in (torch.ones(5), torch.ones(6, 1), torch.ones(6, dtype=torch.float64), [1.0] * 6):
        with pytest.raises(RuntimeError, match=r"length must be float32 \[T\]"):
            svox.sample_weights(s, torch.ones(6), length=bad)
    with pytest.raises(RuntimeError, match="GPU"):
        svox.sample_weights(s, torch.ones(6), length=torch.ones(6))
    # points(geometry=): plain torch, works on any device
    o = torch.arange(9, dtype=torch.float32).reshape(3, 3).requires_grad_(True)
    d = (torch.ones(3, 3) * torch.tensor([1.0, 2.0, 3.0])).requires_grad_(True)
    depth = torch.linspace(0.5, 1.0, 6).requires_grad_(True)
    length = torch.full((6,), 0.25).requires_grad_(True)
    r2 = svox.Rays(o, d, d)
    pts = s.points(r2, "mid", geometry=(depth, length))
    idx = s.ray.long()
    want = o[idx] + d[idx] * (depth + 0.5 * length)[:, None]
    assert torch.equal(pts, want) and pts.requires_grad
    pts.sum().backward()
    assert torch.equal(o.grad, torch.tensor([[2.0] * 3, [0.0] * 3, [4.0] * 3])) and torch.equal(length.grad, torch.full((6,), 3.0))
    assert torch.equal(s.points(r2, "entry", geometry=(depth, length)), o[idx] + d[idx] * depth[:, None])
    assert not s.points(r2).requires_grad and torch.equal(s.points(r2), (o[idx] + d[idx] * 0.5).detach())      # as before
    for bad in ((depth,), (depth, length[:5]), (depth.double(), length), depth):
        with pytest.raises(RuntimeError, match="points: geometry"):
            s.points(r2, geometry=bad)


# ------------------------------------------------------------------------------------------ the restatement's anchors
@pytest.mark.parametrize("name", ["d5_rgba4", "mixed", "hostile", "n3"])
def test_the_lists_are_samples_restates_and_the_faces_well_formed(name):
    b = built(name)
    for ms in (None, 0.0):
        F, want = b.faces(ms), R.lists(b.ot, b.rays, b.opt, ms)
        for field in R.Lists._fields:
            np.testing.assert_array_equal(getattr(F.lists, field), getattr(want, field), err_msg=field)
        L = F.lists
        en, ex = F.face & 3, (F.face >> 2) & 3
        assert F.face.dtype == np.uint8 and np.all(F.face < 16) and np.all(ex < 3) and len(F.face) > 50
        starts = np.zeros(len(F.face), bool)
        starts[L.offsets[:-1][np.diff(L.offsets) > 0]] = True
        assert np.all(starts[en == 3]) and np.all(F.first[en == 3])          # "no plane" only on a ray's first crossing
        o_t = b.ot.offset + b.ot.scaling * b.rays[0]
        inside = np.all((o_t > 0) & (o_t < 1), axis=1)
        assert np.all((en == 3) == (F.first & inside[L.ray]))
        # an axis with a zero direction component is never a face: the ray runs parallel to those planes
        assert np.all(b.rays[1][L.ray, np.minimum(en, 2)][en < 3] != 0) and np.all(b.rays[1][L.ray, ex] != 0)
        # the planes lie where the samples are: depth is its plane's parameter plus at most one step (and rounding)
        d, o = b.rays[1].astype(np.float64), b.rays[0].astype(np.float64)
        z_out = (F.p_out - o[L.ray, ex]) / d[L.ray, ex]
        step = float(b.opt.step_size) * F.delta_scale[L.ray]
        got = (L.depth + L.length).astype(np.float64)
        assert np.all(np.abs(got - z_out - step) <= 1e-4 * np.maximum(1.0, np.abs(got)) / np.abs(F.d_t[L.ray, ex]))
    if name in ("mixed", "hostile"):
        assert (en == 3).sum() >= 5 and ((b.rays[1] == 0).sum(1) == 2)[L.ray].any()
        assert (np.diff(L.offsets) == 0).sum() >= 8
    assert len(set(en.tolist())) >= 3 and len(set(ex.tolist())) == 3


@pytest.mark.parametrize("name", ["d5_sh4_world", "hostile", "n3", "mixed"])
def test_definition_against_the_float64_yardstick(name):
    """The float32 sequence against autograd through z = (P_a - o_a) / d_a, within the bound derived in
    tests/raygeom_restate.py -- each upstream gradient alone and both."""
    b = built(name)
    F = b.faces(0.0)
    T = len(F.face)
    gD, gL = random_upstream(T, 3)
    levels = 3 if name == "n3" else 0
    for gd_, gl_ in ((gD, gL), (gD, None), (None, gL)):
        go32, gd32 = G.geometry_backward32(F, b.rays[1], gd_, gl_)
        go64, gd64 = G.geometry_grad64(F, b.rays[0], b.rays[1], gd_, gl_)
        bo, bd = G.geometry_bound(F, b.rays[1], gd_, gl_, float(b.opt.step_size), b.ot.offset, N=b.ot.N, levels=levels)
        ro, rd = worst(go32, go64, bo), worst(gd32, gd64, bd)
        print(f"{name}: worst |err| / bound: origins {ro:.3f}, dirs {rd:.3f}; addends {int((bo > 0).sum())} / {int((bd > 0).sum())}")
        assert ro <= 1 and rd <= 1
        assert np.isfinite(go32).all() and np.isfinite(gd32).all() and (go32 != 0).sum() > 20
        n = np.diff(F.lists.offsets)
        assert not go32[n == 0].any() and not gd32[n == 0].any()
    # the step term is most of the bound: the definition's distance from the planes' gradient is the term it leaves out
    assert np.median((np.abs(gd32 - gd64) / np.maximum(bd, 1e-300))[bd > 0]) > 1e-3


# --------------------------------------------------------------------------------------------------- finite differences
def _fd_case():
    """random_tree(3): N = 2, depth 5, under random_tree's scaled and shifted cube; 400 rays towards points in the cube, 40
    of them from inside it, direction lengths 0.5 .. 2."""
    if "fd" in _BUILT:
        return _BUILT["fd"]
    t, feats = random_tree(3, N=2, max_depth=5, data_format="RGBA", K=4)
    n = t.n_internal
    ot = O.Tree(feats.numpy(), t.data[:n].numpy().copy(), t.child[:n].numpy().copy(), offset=t.offset.numpy().copy(),
                scaling=t.invradius.numpy().copy())
    rng = np.random.default_rng(12)
    lo, hi = t.tree2world(torch.zeros(1, 3))[0].numpy().astype(np.float64), t.tree2world(torch.ones(1, 3))[0].numpy().astype(np.float64)
    Q = 400
    cen, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    u = rng.standard_normal((Q, 3))
    o = cen + 2.5 * half * u / np.linalg.norm(u, axis=1, keepdims=True)
    o[:40] = lo + rng.uniform(0.1, 0.9, (40, 3)) * (hi - lo)
    target = lo + rng.uniform(0.15, 0.85, (Q, 3)) * (hi - lo)
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (Q, 1))
    _BUILT["fd"] = (ot, o.astype(np.float32), d.astype(np.float32), O.make_options(format=O.FORMAT_RGBA, basis_dim=-1))
    return _BUILT["fd"]


def _ray_loss(ot, o, d, opt):
    """(per-ray loss sum w depth + sum w in float64 over the float32 lists, FaceLists, d loss / d depth, d loss / d length)."""
    F = G.lists_with_faces(ot, (o, d, d), opt)
    L = F.lists
    depth = torch.from_numpy(L.depth).double().requires_grad_(True)
    length = torch.from_numpy(L.length).double().requires_grad_(True)
    sigma = torch.from_numpy(ot.features[L.row, -1]).double()
    w, _ = G.weights64(length, sigma, L.offsets)
    per = torch.zeros(len(L.offsets) - 1, dtype=torch.float64).index_add(0, torch.from_numpy(L.ray.astype(np.int64)), w * depth + w)
    per.sum().backward()
    return per.detach().numpy(), F, depth.grad.numpy(), length.grad.numpy()


@pytest.mark.parametrize("wrt", ["origins", "dirs"])
def test_definition_against_finite_differences(wrt):
    """Central differences of the float32 march at eps = 1e-4 along a random unit direction per ray.  Rays whose crossing
    set changes under the perturbation disagree by construction (the lists are piecewise constant in the rays); the
    conditions are the issue's: over rays with |analytic| > 1e-3 the median relative difference (denominator clamped at
    1e-2) <= 2e-2 and at least 80 % within 5 %."""
    ot, o, d, opt = _fd_case()
    base, F, gD, gL = _ray_loss(ot, o, d, opt)
    go, gd = G.geometry_backward32(F, d, gD, gL)
    rng = np.random.default_rng(13 if wrt == "origins" else 14)
    v = rng.standard_normal(o.shape)
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    eps = np.float32(1e-4)
    if wrt == "origins":
        plus, minus = _ray_loss(ot, o + eps * v, d, opt)[0], _ray_loss(ot, o - eps * v, d, opt)[0]
        analytic = (go.astype(np.float64) * v).sum(1)
        h = ((o + eps * v).astype(np.float64) - (o - eps * v).astype(np.float64))
    else:
        plus, minus = _ray_loss(ot, o, d + eps * v, opt)[0], _ray_loss(ot, o, d - eps * v, opt)[0]
        analytic = (gd.astype(np.float64) * v).sum(1)
        h = ((d + eps * v).astype(np.float64) - (d - eps * v).astype(np.float64))
    # the step actually taken, in float32 numbers: its length along v
    step = (h * v).sum(1)
    fd = (plus - minus) / step
    pick = np.abs(analytic) > 1e-3
    rel = np.abs(fd - analytic)[pick] / np.maximum(np.abs(analytic)[pick], 1e-2)
    med, within = float(np.median(rel)), float((rel <= 0.05).mean())
    print(f"{wrt}: rays {int(pick.sum())} of {len(pick)}, median relative difference {med:.2e}, within 5 %: {100 * within:.1f} %")
    assert pick.sum() >= 150
    assert med <= 2e-2 and within >= 0.80


# -------------------------------------------------------------------------------------------- sample_weights in length
@pytest.mark.parametrize("holes", [False, True])
def test_grad_length_restated_against_float64_autograd(holes):
    """The float32 two-sweep sequence with its second output against autograd through length, to 1e-5 of the tight scale
    (the existing grad_sigma tolerance); grad_sigma from the same pass holds its own."""
    L = built("d5_rgba4").faces().lists
    T, Q = L.row.shape[0], len(L.offsets) - 1
    rng = np.random.default_rng(21)
    sigma = rng.exponential(20.0, T).astype(np.float32) + np.float32(1e-3)
    if holes:
        sigma[::5] = 0
        sigma[2::11] = -1.5
    length = (L.length * rng.uniform(0.5, 1.5, T)).astype(np.float32)            # not the lists' own
    gw, ga = rng.standard_normal(T).astype(np.float32), rng.standard_normal(Q).astype(np.float32)
    for w_, a_ in ((gw, ga), (gw, None), (None, ga)):
        gs32, gl32 = G.weights_backward32(length, sigma, L.offsets, w_, a_)
        l64 = torch.from_numpy(length).double().requires_grad_(True)
        s64 = torch.from_numpy(sigma).double().requires_grad_(True)
        w64, a64 = G.weights64(l64, s64, L.offsets)
        loss = 0.0 * l64.sum()
        if w_ is not None:
            loss = loss + (w64 * torch.from_numpy(w_).double()).sum()
        if a_ is not None:
            loss = loss + (a64 * torch.from_numpy(a_).double()).sum()
        loss.backward()
        tl = G.grad_length_scale(length, sigma, L.offsets, w_, a_)
        ts = R.grad_sigma_scale(length, sigma, L.offsets, w_, a_)
        rl, rs = worst(gl32, l64.grad.numpy(), 1e-5 * tl), worst(gs32, s64.grad.numpy(), 1e-5 * ts)
        print(f"holes {holes}: worst |err| / bound: grad_length {rl:.3f}, grad_sigma {rs:.3f}")
        assert rl <= 1 and rs <= 1 and (gl32 != 0).sum() > 1000
        assert np.all((sigma > 0) | (gl32 == 0))
    # the forward with the lists' own length is samples_restate's
    w_a, al_a = R.weights(L.length, sigma, L.offsets, torch.float32)
    w_b, al_b = G.weights64(torch.from_numpy(L.length).double(), torch.from_numpy(sigma).double(), L.offsets)
    assert np.abs(w_a.numpy() - w_b.numpy()).max() < 1e-5 and np.abs(al_a.numpy() - al_b.numpy()).max() < 1e-5
