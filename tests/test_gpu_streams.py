"""Every operator on a held-back side stream, and the caches across streams.

Late inputs (tests/stream_hold.py): each case runs its operator ONCE inside torch.cuda.stream(s) while s is held by a
sleep and every device input still holds a poison -- a valid input that gives another answer -- and receives its true
content by a copy enqueued on s behind the sleep.  The result must be the default-stream result of the true inputs: bit
for bit where the project states "the same bits in every run", within the project's own gradient tolerance (tests.util
assert_grads_close on the oracle's scale) for the backwards that sum with float atomics.  A launch, memset or copy that
goes to the null stream, or a host read that waits for the wrong stream, sees the poison.  Independently of any race
showing, every C entry of the case is checked ON THE CALL: the stream handle it receives is s's, before it launches.

Caches across streams: what outlives the call that built it (acceleration grids, sigma bitmask and exponentials table, the
padded table, row / stencil / tv plans, the neighbour table, the frontier) is built on one stream and consumed on another.
These tests never read unfinished data: the ordering is asserted on the calls -- the consumer's wait on the producer's
event before its first launch, record_stream for the allocator -- and the values only after both streams were synchronised.
"""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from svox_t_amd.csrc import _abi, _extras, _marshal
from svox_t_amd.renderer import _rays_spec_from_rays
from tests import depth_restate as DR
from tests import distortion_restate as XR
from tests.stream_hold import assert_held, hold, late
from tests.test_gpu_random_stress import random_rays, random_tree
from tests.util import Case, assert_grads_close

pytestmark = pytest.mark.gpu

EMPTY = int(synth.EMPTY_SENTINEL)
Q = 2000                                           # 31 full tiles of 64 rays and one of 16


# ----------------------------------------------------------------------------------------------------------- the scenes
class Scene:
    """Host tables of a tree and a ray batch; nothing on the GPU."""

    def __init__(self, child, data, pd, feats, fmt, radius, center, rays):
        self.child = torch.as_tensor(np.ascontiguousarray(child), dtype=torch.int32)
        self.data = torch.as_tensor(np.ascontiguousarray(data), dtype=torch.int32).reshape(tuple(self.child.shape) + (1,))
        self.pd = torch.as_tensor(np.ascontiguousarray(pd), dtype=torch.int32)
        self.feats, self.fmt, self.radius, self.center = feats.contiguous(), fmt, list(radius), list(center)
        self.o, self.d, self.v = rays
        self.M, self.K = feats.shape
        self.n = self.child.shape[0]
        df = svox.DataFormat(fmt)
        self.format, self.basis_dim = df.format, df.basis_dim

    def oracle_tree(self):
        t = svox.N3Tree.from_arrays(self.child, self.data, self.pd, self.feats, data_format=self.fmt, radius=self.radius,
                                    center=self.center)
        return O.Tree(self.feats.numpy(), self.data.numpy(), self.child.numpy(), offset=t.offset.numpy().copy(),
                      scaling=t.invradius.numpy().copy())

    def rays_np(self):
        return self.o.numpy(), self.d.numpy(), self.v.numpy()


_SCENES: dict = {}


def scene(name) -> Scene:
    """"random": random_tree(0, max_depth=5), SH4 / K = 13, with random_rays(0, 2000): rays inside, outside and missing.
    "shell": the depth-5 shell tree, SH4 / K = 13, with a 64 x 64 pinhole image."""
    if name not in _SCENES:
        if name == "random":
            t, feats = random_tree(0, max_depth=5)
            n = t.n_internal
            _SCENES[name] = Scene(t.child[:n].numpy().copy(), t.data[:n].numpy().copy(), t.parent_depth[:n].numpy().copy(),
                                  feats, "SH4", (0.7, 1.3, 0.9), (0.2, -0.1, 0.4), random_rays(0, Q, t))
        else:
            c = Case(depth=5, K=13, data_format="SH4", width=64, height=64)
            _SCENES[name] = Scene(c.st.child, c.st.data, c.st.parent_depth, c.features, "SH4", [0.5] * 3, [0.5] * 3,
                                  (c.origins, c.dirs, c.vdirs))
    return _SCENES[name]


def oracle_scale(name, cols, seed):
    """(grad_output, gradient, sum of |contributions|) of the oracle's colour backward: the scale assert_grads_close takes."""
    key = ("scale", name, cols, seed)
    if key not in _SCENES:
        S = scene(name)
        g = synth.grad_output(S.o.shape[0], cols, seed=seed)
        opt = O.make_options(step_size=1e-3, background_brightness=1.0, format=S.format, basis_dim=S.basis_dim)
        gw, ab = O.volume_render_backward(S.oracle_tree(), *S.rays_np(), opt, g.numpy(), want_abs=True)
        _SCENES[key] = (g, gw, ab)
    return _SCENES[key]


# ------------------------------------------------------------------------------------------------ inputs in three modes
class Inputs:
    """Where a case's device inputs come from: "true" (the content, on the default stream), "poison" (the poison, on the
    default stream) or "late" (the poison now, the content behind the hold of `stream`)."""

    def __init__(self, mode, gpu, stream=None):
        self.mode, self.gpu, self.stream = mode, gpu, stream

    def t(self, src, poison=None):
        src = torch.as_tensor(src)
        poison = torch.zeros_like(src) if poison is None else torch.as_tensor(poison).to(src.dtype).expand_as(src).contiguous()
        if self.mode == "late":
            return late(self.stream, src, poison)
        return (src if self.mode == "true" else poison).contiguous().to(self.gpu)

    def grad(self, src, poison=None):
        return self.t(src, poison).requires_grad_(True)

    def tree(self, S: Scene, feats=None):
        """The scene's tree: child <- zeros (a root of leaves), data <- the empty sentinel, parent_depth and features <- zeros."""
        t = svox.N3Tree.from_arrays(S.child, S.data, S.pd, S.feats, data_format=S.fmt, radius=S.radius, center=S.center,
                                    device=self.gpu)
        t.child = self.t(S.child)
        t.data = self.t(S.data, torch.full_like(S.data, EMPTY))
        t.parent_depth = self.t(S.pd)
        t.features = torch.nn.Parameter(self.t(S.feats if feats is None else feats))
        t._invalidate()
        return t

    def rays(self, S: Scene, grad=False):
        """The scene's rays; the poison starts outside the cube and points away from it."""
        away = torch.tensor([1.0, 1.0, 1.0]) / 3.0 ** 0.5
        far = torch.tensor(S.center) + 10.0 * torch.tensor(S.radius)
        mk = self.grad if grad else self.t
        return svox.Rays(mk(S.o, far), mk(S.d, away), mk(S.v, away))

    def samples(self, L, row=None):
        """A RaySamples of the host lists L: offsets <- zeros (empty lists), ray / row <- 0, depth / length <- zeros."""
        return svox.RaySamples(self.t(L["offsets"]), self.t(L["ray"]), self.t(L["row"] if row is None else row),
                               self.t(L["depth"]), self.t(L["length"]), None if L.get("face") is None else self.t(L["face"]))


def true_lists(gpu, name="random"):
    """The scene's leaf crossings (faces=True) as host tensors, marched once on the default stream; the rest of the suite
    pins them to the restatement."""
    key = ("lists", name)
    if key not in _SCENES:
        S = scene(name)
        inp = Inputs("true", gpu)
        s = svox.VolumeRenderer(inp.tree(S)).ray_samples(inp.rays(S), faces=True)
        _SCENES[key] = {k: getattr(s, k).cpu() for k in ("offsets", "ray", "row", "depth", "length", "face")}
        assert len(s) > 2000
    return _SCENES[key]


def folded_rows(L):
    """row with every third sample folded onto rows 0 .. 7: rows of far more than 256 samples, which reduce_rows and
    the row plan sum in chunks."""
    row = L["row"].clone()
    row[::3] %= 8
    assert int(torch.bincount(row.long()).max()) > 256
    return row


def csr_filter(L, keep):
    """The host lists L without the samples where keep is False."""
    keep = keep.bool()
    counts = torch.zeros(L["offsets"].shape[0] - 1, dtype=torch.int64).index_add_(0, L["ray"].long(), keep.long())
    out = {k: L[k][keep].contiguous() for k in ("ray", "row", "depth", "length")}
    out["offsets"] = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    out["face"] = None
    return out


# ------------------------------------------------------------------------------------------- the stream of every C entry
def _handle_of(name, args):
    """The stream handle a C entry receives (0: the null stream), or None for an entry that takes no stream (sizes, plans
    made on the host): the last parameter of every launching entry is the stream (svox_t_amd/csrc/_abi.py, EXPORTS)."""
    argtypes = _abi.EXPORTS[name][1]
    if not argtypes or argtypes[-1] is not ctypes.c_void_p:
        return None
    a = args[-1]
    return (a.value or 0) if isinstance(a, ctypes.c_void_p) else int(a or 0)


class Recorder:
    """_call wrapped wherever it is bound.  `expect`: the handle every launching entry must receive -- asserted on the call,
    BEFORE the entry runs; None: only record."""

    def __init__(self, monkeypatch, expect=None):
        self.calls, self.expect, self.log = [], expect, []
        real = _marshal._call

        def recording_call(name, *args):
            h = self.handle(name, args)
            if h is not None:
                self.calls.append((name, h))
                self.log.append(("call", name, h))
                if self.expect is not None:
                    assert h != 0, f"{name} received the null stream"
                    assert h == self.expect, f"{name} received stream {h:#x}, not the current stream {self.expect:#x}"
            return real(name, *args)

        for mod in (_marshal, _C, _extras):
            monkeypatch.setattr(mod, "_call", recording_call)

    def handle(self, name, args):
        return _handle_of(name, args)


def outputs(xs):
    return [None if x is None else x.detach().cpu().numpy().copy() for x in xs]


def _bits(x):
    return x.view(f"u{x.itemsize}") if x.dtype.kind == "f" else x


def differ(a, b):
    return len(a) != len(b) or any((x is None) != (y is None) or (x is not None and (
        x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(_bits(x), _bits(y)))) for x, y in zip(a, b))


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def run_late(gpu, monkeypatch, prep, run, close=None):
    """prep(inputs) -> state: builds the inputs, launches nothing of the library's and reads nothing back; run(state) ->
    tensors.  close: {output index: abs_sum} for the outputs summed with float atomics (assert_grads_close against the
    default-stream result); every other output bit for bit."""
    want = outputs(run(prep(Inputs("true", gpu))))
    try:
        bad = outputs(run(prep(Inputs("poison", gpu))))
    except RuntimeError:
        bad = None                                   # (the operator refuses the poison: that is a different result too)
    assert bad is None or differ(want, bad), "the poisoned inputs give the right answer: the case proves nothing"
    torch.cuda.synchronize()
    _C.invalidate_caches()
    s = torch.cuda.Stream(device=gpu)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.default_stream(gpu).cuda_stream
    state = prep(Inputs("late", gpu, s))               # every input holds its poison; nothing is enqueued on s yet
    torch.cuda.synchronize()
    ev = hold(s)                                       # the sleep, and behind it the copies of the true contents
    rec = Recorder(monkeypatch, expect=s.cuda_stream)
    with torch.cuda.stream(s):
        assert_held(ev)
        got = run(state)
    s.synchronize()
    got = outputs(got)
    assert rec.calls, "the case ran no C entry"
    assert all(h == s.cuda_stream for _, h in rec.calls)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if close is not None and i in close:
            assert_grads_close(g, w, close[i], what=f"output {i}")
        else:
            same_bits(g, w, f"output {i}")
    return rec


# ------------------------------------------------------------------------------------------------------- the render family
def _render_case(gpu, monkeypatch, method="forward", cols=4, tol=True, switches=(), **kw):
    S = scene("random")
    g, _, ab = oracle_scale("random", cols, 3)
    for k, v in switches:
        monkeypatch.setattr(_C, k, v)

    def prep(inp):
        tree = inp.tree(S)
        return tree, svox.VolumeRenderer(tree), inp.rays(S), inp.t(g)

    def run(st):
        tree, r, rays, gout = st
        out = (r if method == "forward" else getattr(r, method))(tree.features, rays, **kw)
        out.backward(gout)
        return out, tree.features.grad

    return run_late(gpu, monkeypatch, prep, run, close={1: ab} if tol else None)


def test_forward_backward_default_route(gpu, monkeypatch):
    _render_case(gpu, monkeypatch)


def test_forward_backward_deterministic(gpu, monkeypatch):
    """deterministic=True: the gradient is summed over the row plan, the same bits in every run -- and on every stream."""
    _render_case(gpu, monkeypatch, deterministic=True, tol=False)


def test_forward_backward_fast(gpu, monkeypatch):
    _render_case(gpu, monkeypatch, fast=True)


def test_forward_backward_sorted_rays(gpu, monkeypatch):
    rec = _render_case(gpu, monkeypatch, sort_rays=True)
    assert any(n == "svoxt_ray_order" for n, _ in rec.calls)


def test_forward_backward_with_dry_list_pools(gpu, monkeypatch):
    """A pool of one block per part: nearly every ray finds none, stops recording and marches the rest."""
    monkeypatch.setattr(_C, "_pool_blocks_for", lambda tiles, S, kind="record": 1)
    _render_case(gpu, monkeypatch, sort_rays=True)


def test_opacity_render_backward(gpu, monkeypatch):
    _render_case(gpu, monkeypatch, method="opacity_render", cols=1)


def test_render_persp_backward(gpu, monkeypatch):
    S = scene("shell")
    g = synth.grad_output(64 * 64, 4, seed=5)
    opt = O.make_options(step_size=1e-3, background_brightness=1.0, format=S.format, basis_dim=S.basis_dim)
    pose = torch.from_numpy(np.asarray(synth.camera_pose(), dtype=np.float32))
    away = torch.eye(4)[:3].clone()
    away[2, 3] = -10.0                                  # behind the cube, looking down -z: away from it

    def prep(inp):
        tree = inp.tree(S)
        return tree, svox.VolumeRenderer(tree), inp.t(pose, away), inp.t(g.reshape(64, 64, 4))

    def run(st):
        tree, r, c2w, gout = st
        out = r.render_persp(tree.features, c2w, width=64, height=64, fx=70.0)
        out.backward(gout)
        return out, tree.features.grad

    # the scale: the oracle's backward over the same pinhole rays (synth.pinhole_rays follows the kernels' cam2world_ray)
    o, d, v = synth.pinhole_rays(64, 64, c2w=pose.numpy().astype(np.float64), fx=70.0, fy=70.0)
    _, ab = O.volume_render_backward(S.oracle_tree(), o.numpy(), d.numpy(), v.numpy(), opt, g.numpy(), want_abs=True)
    run_late(gpu, monkeypatch, prep, run, close={1: ab})


def test_render_depth(gpu, monkeypatch):
    S = scene("random")

    def prep(inp):
        tree = inp.tree(S)
        return tree, svox.VolumeRenderer(tree), inp.rays(S)

    def run(st):
        tree, r, rays = st
        with torch.no_grad():
            return (r.render_depth(tree.features, rays),)

    run_late(gpu, monkeypatch, prep, run)


def test_query_vertical_backward(gpu, monkeypatch):
    S = scene("random")
    pts = torch.rand(3000, 3, generator=torch.Generator().manual_seed(1)) * 1.2 - 0.1
    g = synth.grad_output(3000, S.K, seed=2)

    def prep(inp):
        return inp.tree(S), inp.t(pts, torch.full_like(pts, 0.5)), inp.t(g)

    def run(st):
        tree, p, gout = st
        out = tree(tree.features, p, world=False)
        out.backward(gout)
        return out, tree.features.grad

    # (sum of |contributions| per entry: the |upstream rows| scattered to the rows the points fall in, from the default-stream run)
    inp = Inputs("true", gpu)
    tree, p, gout = prep(inp)
    f = tree.features.detach().clone().requires_grad_(True)
    tree(f, p, world=False).backward(gout.abs())
    run_late(gpu, monkeypatch, prep, run, close={1: f.grad.cpu().numpy()})


def test_step_api(gpu, monkeypatch):
    """svoxt_step_plan / _forward / _backward through csrc's step API, with the acceleration grid built inside the case."""
    S = scene("shell")
    g, _, ab = oracle_scale("shell", 4, 11)

    def prep(inp):
        tree = inp.tree(S)
        return tree, svox.VolumeRenderer(tree), inp.rays(S), inp.t(g)

    def run(st):
        tree, r, rays, gout = st
        opt = r._get_options()
        ct = _C._pack_tree_accel(tree._spec(tree.features.detach()), True)
        cr, co = _C._pack_rays(_rays_spec_from_rays(rays, (64, 64))), _C._pack_opts(opt)
        step = _abi._CStep()
        _C._call("svoxt_step_plan", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), 0, ctypes.byref(step))
        ws = torch.empty((step.workspace_bytes + 256,), dtype=torch.uint8, device=gpu)
        base = (ws.data_ptr() + 255) // 256 * 256
        out = torch.empty((64 * 64, 4), dtype=torch.float32, device=gpu)
        grad = torch.full((S.M, S.K), float("nan"), dtype=torch.float32, device=gpu)
        st_ = _C._stream(gout.device)
        _C._call("svoxt_step_forward", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), out.data_ptr(), ctypes.byref(step), base, st_)
        _C._call("svoxt_step_backward", ctypes.byref(ct), ctypes.byref(cr), ctypes.byref(co), gout.data_ptr(), grad.data_ptr(),
                 ctypes.byref(step), base, st_)
        run.keep = (ws, ct)
        return out, grad

    run_late(gpu, monkeypatch, prep, run, close={1: ab})


def _sweep_case(gpu, monkeypatch, method, cols, scale_of, **kw):
    S = scene("random")
    g = synth.grad_output(Q, cols, seed=7)
    opt = O.make_options(step_size=1e-3, background_brightness=1.0, format=S.format, basis_dim=S.basis_dim)
    scale = scale_of(S.oracle_tree(), S.rays_np(), opt, g.numpy())

    def prep(inp):
        tree = inp.tree(S)
        return tree, svox.VolumeRenderer(tree), inp.rays(S), inp.t(g)

    def run(st):
        tree, r, rays, gout = st
        out = getattr(r, method)(tree.features, rays, **kw)
        out.backward(gout)
        return out, tree.features.grad

    run_late(gpu, monkeypatch, prep, run, close={1: scale})


def test_render_depth_moments_backward(gpu, monkeypatch):
    _sweep_case(gpu, monkeypatch, "render_depth_moments", 3, lambda ot, rays, opt, g: DR.moments_grad_scale(ot, rays, opt, "entry", g))


def test_render_distortion_backward(gpu, monkeypatch):
    _sweep_case(gpu, monkeypatch, "render_distortion", 2, XR.distortion_grad_scale)


# ----------------------------------------------------------------------------------------------------- the sample family
@pytest.mark.parametrize("faces", [False, True], ids=["plain", "faces"])
def test_ray_samples(gpu, monkeypatch, faces):
    S = scene("random")

    def prep(inp):
        tree = inp.tree(S)
        return svox.VolumeRenderer(tree), inp.rays(S)

    def run(st):
        r, rays = st
        s = r.ray_samples(rays, faces=faces)
        return [s.offsets, s.ray, s.row, s.depth, s.length] + ([s.face] if faces else [])

    run_late(gpu, monkeypatch, prep, run)


def test_sample_geometry_backward(gpu, monkeypatch):
    S, L = scene("random"), true_lists(gpu)
    T = L["ray"].shape[0]
    gd, gl = synth.grad_output(T, 1, seed=3)[:, 0], synth.grad_output(T, 1, seed=4)[:, 0]

    def prep(inp):
        return inp.samples(L), inp.rays(S, grad=True), inp.t(gd), inp.t(gl)

    def run(st):
        s, rays, a, b = st
        depth, length = svox.sample_geometry(s, rays)
        torch.autograd.backward([depth, length], [a, b])
        return depth, length, rays.origins.grad, rays.dirs.grad

    run_late(gpu, monkeypatch, prep, run)


def test_sample_weights_accumulate_backward(gpu, monkeypatch):
    S, L = scene("random"), true_lists(gpu)
    T = L["ray"].shape[0]
    sigma = S.feats[L["row"].long(), -1].clamp(min=0.0).contiguous()
    vals = synth.grad_output(T, 3, seed=5)
    g = synth.grad_output(Q, 3, seed=6)

    def prep(inp):
        return inp.samples(L), inp.grad(sigma), inp.t(L["length"]), inp.grad(vals), inp.t(g)

    def run(st):
        s, sg, length, v, gout = st
        w, alpha = svox.sample_weights(s, sg, length=length)
        out = svox.accumulate(s, w, v)
        torch.autograd.backward([out, alpha], [gout, gout[:, 0].contiguous()])
        return w, alpha, out, sg.grad, v.grad

    run_late(gpu, monkeypatch, prep, run)


def test_gather_reduce_rows_and_row_plan(gpu, monkeypatch):
    S, L = scene("random"), true_lists(gpu)
    row = folded_rows(L)
    T = row.shape[0]
    g = synth.grad_output(T, S.K, seed=8)
    vals = synth.grad_output(T, 2, seed=9)
    assert S.M >= 300

    def prep(inp):
        return inp.samples(L, row), inp.grad(S.feats), inp.t(g), inp.t(vals)

    def run(st):
        s, table, gout, v = st
        f = svox.gather_rows(s, table)
        f.backward(gout)
        plan = s.row_plan(S.M)
        assert plan.longest > 256
        return (f, table.grad, svox.reduce_rows(s, v, S.M, "sum"), svox.reduce_rows(s, v, S.M, "max"), plan.row_ptr, plan.perm,
                plan.long_rows, plan.long_chunk_ptr, plan.chunk_long)

    run_late(gpu, monkeypatch, prep, run)


def test_view_basis_backward(gpu, monkeypatch):
    S = scene("random")
    g = synth.grad_output(Q, 4, seed=10)

    def prep(inp):
        tree = inp.tree(S)
        return svox.VolumeRenderer(tree), inp.rays(S, grad=True), inp.t(g)

    def run(st):
        r, rays, gout = st
        basis = r.view_basis(rays)
        basis.backward(gout)
        return basis, rays.viewdirs.grad

    run_late(gpu, monkeypatch, prep, run)


@pytest.mark.parametrize("wrt", ["features", "basis"])
def test_shade_samples(gpu, monkeypatch, wrt):
    S, L = scene("random"), true_lists(gpu)
    T = L["ray"].shape[0]
    gv, gs = synth.grad_output(T, 3, seed=11), synth.grad_output(T, 1, seed=12)[:, 0]
    basis = synth.grad_output(Q, 4, seed=13)

    def prep(inp):
        tree = inp.tree(S)
        b = inp.grad(basis) if wrt == "basis" else None
        return tree, svox.VolumeRenderer(tree), inp.samples(L), inp.rays(S), b, inp.t(gv), inp.t(gs)

    def run(st):
        tree, r, s, rays, b, a, c = st
        rgb, sigma = r.shade_samples(s, tree.features, rays if b is None else None, basis=b)
        torch.autograd.backward([rgb, sigma], [a, c.contiguous()])
        return [rgb, sigma, tree.features.grad] + ([] if b is None else [b.grad])

    run_late(gpu, monkeypatch, prep, run)


def test_shade_samples_rotations_all_three_gradients(gpu, monkeypatch):
    S, L = scene("random"), true_lists(gpu)
    T = L["ray"].shape[0]
    gv, gs = synth.grad_output(T, 3, seed=14), synth.grad_output(T, 1, seed=15)[:, 0]
    mats = torch.randn(S.M, 3, 3, generator=torch.Generator().manual_seed(16))

    def prep(inp):
        tree = inp.tree(S)
        return tree, svox.VolumeRenderer(tree), inp.samples(L), inp.rays(S, grad=True), inp.grad(mats), inp.t(gv), inp.t(gs)

    def run(st):
        tree, r, s, rays, m, a, c = st
        rgb, sigma = r.shade_samples(s, tree.features, rays, rotations=m)
        torch.autograd.backward([rgb, sigma], [a, c.contiguous()])
        return rgb, sigma, tree.features.grad, m.grad, rays.viewdirs.grad

    run_late(gpu, monkeypatch, prep, run)


@pytest.mark.parametrize("op", ["sum", "max"])
def test_ray_scan_backward(gpu, monkeypatch, op):
    L = true_lists(gpu)
    T = L["ray"].shape[0]
    vals, g = synth.grad_output(T, 2, seed=17), synth.grad_output(T, 2, seed=18)

    def prep(inp):
        return inp.samples(L), inp.grad(vals), inp.t(g)

    def run(st):
        s, v, gout = st
        out = svox.ray_scan(s, v, op)
        out.backward(gout)
        return out, v.grad

    run_late(gpu, monkeypatch, prep, run)


def test_ray_quantile(gpu, monkeypatch):
    L = true_lists(gpu)
    w = synth.grad_output(L["ray"].shape[0], 1, seed=19)[:, 0].abs().contiguous()

    def prep(inp):
        return inp.samples(L), inp.t(w)

    run_late(gpu, monkeypatch, prep, lambda st: svox.ray_quantile(st[0], st[1], [0.25, 0.5]))


def _lists_out(s, *index):
    return [s.offsets, s.ray, s.row, s.depth, s.length] + list(index)


def test_select(gpu, monkeypatch):
    L = true_lists(gpu)
    keep = torch.rand(L["ray"].shape[0], generator=torch.Generator().manual_seed(20)) < 0.6

    def prep(inp):
        return inp.samples(L), inp.t(keep)

    run_late(gpu, monkeypatch, prep, lambda st: _lists_out(*st[0].select(st[1])))


def test_split(gpu, monkeypatch):
    L = true_lists(gpu)
    cut = float(L["length"].median())

    run_late(gpu, monkeypatch, lambda inp: inp.samples(L), lambda s: _lists_out(*s.split(max_length=cut)))


def test_merge_samples(gpu, monkeypatch):
    L = true_lists(gpu)
    B = csr_filter(L, L["row"] % 2 == 0)
    A = dict(L, face=None)

    def prep(inp):
        return inp.samples(A), inp.samples(B)

    def run(st):
        m, ia, ib = svox.merge_samples(*st)
        return _lists_out(m, ia, ib)

    run_late(gpu, monkeypatch, prep, run)


# -------------------------------------------------------------------------------------------------------- the tree family
def _tables(tree):
    n = tree.filled
    return [tree.child[:n], tree.data[:n], tree.parent_depth[:n], tree.features]


def test_interp_both_gradients(gpu, monkeypatch):
    S = scene("shell")
    pts = torch.rand(3000, 3, generator=torch.Generator().manual_seed(21)) * 0.9 + 0.05
    g = synth.grad_output(3000, S.K, seed=22)

    def prep(inp):
        return inp.tree(S), inp.grad(pts, torch.full_like(pts, 0.5)), inp.t(g)

    def run(st):
        tree, p, gout = st
        out = tree.interp(p)
        out.backward(gout)
        return out, tree.features.grad, p.grad

    run_late(gpu, monkeypatch, prep, run)


def _edit_case(gpu, monkeypatch, edit, mask_seed=None, scene_name="shell"):
    S = scene(scene_name)
    mask = None if mask_seed is None else (torch.rand(tuple(S.child.shape), generator=torch.Generator().manual_seed(mask_seed)) < 0.5)

    def prep(inp):
        return inp.tree(S), (None if mask is None else inp.t(mask))

    def run(st):
        tree, m = st
        extra = edit(tree, m)
        return _tables(tree) + list(extra or [])

    run_late(gpu, monkeypatch, prep, run)


def test_prune(gpu, monkeypatch):
    _edit_case(gpu, monkeypatch, lambda tree, m: [tree.prune(m).row_map], mask_seed=23)


def test_merge(gpu, monkeypatch):
    _edit_case(gpu, monkeypatch, lambda tree, m: tree.merge() and None)


def test_reduce_frontier_grad(gpu, monkeypatch):
    S = scene("shell")
    fr = svox.N3Tree.from_arrays(S.child, S.data, S.pd, S.feats, data_format=S.fmt, device=gpu).frontier().shape[0]
    g = synth.grad_output(fr, S.K, seed=24)

    def prep(inp):
        return inp.tree(S), inp.t(g)

    def run(st):
        tree, gout = st
        out = tree.reduce_frontier("mean", grad=True)
        out.backward(gout)
        return out, tree.features.grad, tree.frontier()

    run_late(gpu, monkeypatch, prep, run)


def test_subdivide(gpu, monkeypatch):
    _edit_case(gpu, monkeypatch, lambda tree, m: [tree.subdivide(m).row_map], mask_seed=25)


def test_unshare(gpu, monkeypatch):
    def edit(tree, m):
        tree.subdivide(m, own_rows=False)          # leaves that share rows, made on the same stream
        tree.unshare()

    _edit_case(gpu, monkeypatch, edit, mask_seed=26)


@pytest.mark.parametrize("reduce", ["sum", "last"])
def test_set(gpu, monkeypatch, reduce):
    S = scene("shell")
    pts = torch.rand(3000, 3, generator=torch.Generator().manual_seed(27))
    vals = synth.grad_output(3000, S.K, seed=28)

    def prep(inp):
        return inp.tree(S), inp.t(pts, torch.full_like(pts, 0.5)), inp.t(vals)

    def run(st):
        tree, p, v = st
        tree.set(p, v, reduce=reduce)
        return (tree.features,)

    run_late(gpu, monkeypatch, prep, run)


def test_leaf_boxes(gpu, monkeypatch):
    run_late(gpu, monkeypatch, lambda inp: inp.tree(scene("shell")), lambda tree: list(tree.leaf_boxes()))


def test_leaf_neighbors(gpu, monkeypatch):
    run_late(gpu, monkeypatch, lambda inp: inp.tree(scene("random")), lambda tree: list(tree.leaf_neighbors()))


def test_tv_backward_and_add_grad(gpu, monkeypatch):
    S = scene("random")
    acc = synth.grad_output(S.M, S.K, seed=29)

    def prep(inp):
        return inp.tree(S), inp.t(acc)

    def run(st):
        tree, out = st
        loss = tree.tv()
        loss.backward()
        tree.tv_add_grad(out, 0.5, dim=-1)
        return loss, tree.features.grad, out

    run_late(gpu, monkeypatch, prep, run)


def test_quantize_median_cut(gpu, monkeypatch):
    S = scene("random")
    w = torch.rand(S.M, generator=torch.Generator().manual_seed(30)) + 0.1

    def prep(inp):
        return inp.t(S.feats), inp.t(w)

    run_late(gpu, monkeypatch, prep, lambda st: svox.quantize_median_cut(st[0], 5, st[1]))


def _cloud():
    g = torch.Generator().manual_seed(31)
    return torch.rand(3000, 3, generator=g), torch.randn(3000, 4, generator=g)


def test_voxelize_backward(gpu, monkeypatch):
    pts, feats = _cloud()
    gout = synth.grad_output(24 ** 3, 1, seed=32).reshape(24, 24, 24, 1)

    def prep(inp):
        return inp.grad(pts, torch.full_like(pts, 0.5)), inp.grad(feats), inp.t(gout)

    def run(st):
        p, f, g = st
        vol = svox.voxelize(p, f, (0, 0, 0), (1, 1, 1), 24, 1.0 / 23, 2.0 / 23)
        vol.backward(g.reshape(vol.shape))
        return vol, p.grad, f.grad

    run_late(gpu, monkeypatch, prep, run)


def test_grid_weights(gpu, monkeypatch):
    S = scene("random")
    sigma = torch.rand(24, 24, 24, generator=torch.Generator().manual_seed(33)) * 20.0

    def prep(inp):
        return inp.t(sigma), inp.rays(S)

    def run(st):
        vol, rays = st
        return list(svox.grid_weights(vol, rays=(rays.origins, rays.dirs), radius=S.radius, center=S.center))

    run_late(gpu, monkeypatch, prep, run)


def test_build_from_points(gpu, monkeypatch):
    pts, _ = _cloud()

    def prep(inp):
        tree = svox.N3Tree(N=2, data_dim=4, data_format="RGBA").to(gpu)
        return tree, inp.t(pts, torch.full_like(pts, 0.5))

    def run(st):
        tree, p = st
        tree.build_from_points(p, 5)
        return _tables(tree)[:3]

    run_late(gpu, monkeypatch, prep, run)


def test_adam_step_on_late_gradients(gpu, monkeypatch):
    """(the three optimizers' handles are pinned in tests/test_gpu_optim.py; this is the held / late form of Adam)"""
    S = scene("random")
    grad = synth.grad_output(S.M, S.K, seed=34)
    grad[::3] = 0.0                                     # untouched rows: the lazy step skips them

    def prep(inp):
        p = torch.nn.Parameter(inp.t(S.feats))
        p.grad = inp.t(grad)
        return p, svox.FeatureAdam([p], lr=1e-2)

    def run(st):
        p, opt = st
        opt.step()
        return p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]

    run_late(gpu, monkeypatch, prep, run)


# ------------------------------------------------------------------------------------------------ caches across streams
# entries that take the tree WITHOUT its grid and mask (svoxt_ray_order and svoxt_image_probe run in front of the packer
# that attaches them) or build such a product: they read no cache product
NOT_READERS = {"svoxt_ray_order", "svoxt_image_probe", "svoxt_accel_build", "svoxt_sigma_mask_build", "svoxt_sigma_mask_build_fill",
               "svoxt_exp_table_build"}
# ... and which entries read a product that is not attached to the tree struct (the others: every entry outside NOT_READERS)
READERS = {"row_plan": lambda n: "rows" in n or "shade" in n, "stencil_plan": lambda n: n == "svoxt_interp_rows_bwd",
           "tv_plan": lambda n: n.startswith("svoxt_tv_rows"), "leaf_neighbors": lambda n: n.startswith("svoxt_tv_plan"),
           "frontier": lambda n: "frontier" in n}


class Ordering(Recorder):
    """... and, besides the entries, every cache product built (_marshal._Produced), every wait a consumer issues on a
    producer's event, every record_stream.  On a tree without the helper nothing is ever waited for."""

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        self.built, self.waits, self.recorded = [], [], []
        P = getattr(_marshal, "_Produced", None)
        if P is None:
            return
        init, cross = P.__init__, P._cross
        rec = self

        def new_init(p, what, value, tensors, device):
            init(p, what, value, tensors, device)
            rec.built.append(p)
            rec.log.append(("built", p.what, p.handle))

        crossing = []                                    # the product whose slow path is running
        real_wait, real_rs = torch.cuda.Stream.wait_event, torch.Tensor.record_stream

        def wait_event(stream, event):
            if crossing and event is crossing[-1].event:
                rec.waits.append((crossing[-1], stream.cuda_stream))
                rec.log.append(("wait", crossing[-1].what, stream.cuda_stream))
            return real_wait(stream, event)

        def record_stream(tensor, stream):
            rec.recorded.append((tensor.data_ptr(), stream.cuda_stream))
            return real_rs(tensor, stream)

        def new_cross(p, handle):
            crossing.append(p)
            try:
                cross(p, handle)
            finally:
                crossing.pop()

        monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)
        monkeypatch.setattr(torch.Tensor, "record_stream", record_stream)
        monkeypatch.setattr(P, "__init__", new_init)
        monkeypatch.setattr(P, "_cross", new_cross)

    def waited_before_first_launch(self, what, handle, since):
        """The wait for product `what` on stream `handle` comes before that stream's first C entry after log position
        `since` that may read it."""
        tail = self.log[since:]
        wait = next((i for i, e in enumerate(tail) if e == ("wait", what, handle)), None)
        reads = READERS.get(what, lambda n: n not in NOT_READERS)
        launch = next((i for i, e in enumerate(tail) if e[0] == "call" and e[2] == handle and reads(e[1])), len(tail))
        return wait is not None and wait < launch


def _cache_scenarios(gpu):
    """name -> (make() -> state, use(state) -> tensors, the products the use builds): each use is read-only and builds what
    it caches on its first call."""
    S = scene("random")

    def tree_static(K_feats=None):
        tree = Inputs("true", gpu).tree(S, K_feats)
        tree.static_features = True
        return tree

    def render(record):
        def make():
            tree = tree_static()
            return tree, svox.VolumeRenderer(tree), Inputs("true", gpu).rays(S)

        def use(st):
            tree, r, rays = st
            if record:
                f = tree.features.detach().requires_grad_(True)
                out = r(f, rays, sort_rays=True)
                out.backward(torch.ones_like(out))
                return out.detach(), f.grad
            with torch.no_grad():
                return (r(tree.features, rays, sort_rays=True),)
        return make, use

    def rgba8():
        def make():
            feats = S.feats[:, :8].contiguous()
            t = svox.N3Tree.from_arrays(S.child, S.data, S.pd, feats, data_format="RGBA", radius=S.radius, center=S.center, device=gpu)
            t.static_features = True
            return t, svox.VolumeRenderer(t), Inputs("true", gpu).rays(S)

        def use(st):
            with torch.no_grad():
                return (st[1](st[0].features, st[2], sort_rays=True),)
        return make, use

    def padded():
        def make():
            feats = S.feats[:, :6].contiguous()
            t = svox.N3Tree.from_arrays(S.child, S.data, S.pd, feats, data_format="RGBA", radius=S.radius, center=S.center, device=gpu)
            spec_rays = _rays_spec_from_rays(Inputs("true", gpu).rays(S), None, None)
            # (the padded table is kept on the rays spec under the identity of the table it was padded from: ONE tensor object)
            return t, svox.VolumeRenderer(t), spec_rays, t.features.detach()

        def use(st):
            t, r, rspec, f = st
            with torch.no_grad():
                return (_C.volume_render(t._spec(f), rspec, r._get_options()),)
        return make, use

    def rows():
        def make():
            Ls = true_lists(gpu)
            inp = Inputs("true", gpu)
            return inp.samples(Ls, folded_rows(Ls)), inp.t(synth.grad_output(Ls["ray"].shape[0], 2, seed=40))

        return make, lambda st: (svox.reduce_rows(st[0], st[1], S.M, "sum"),)

    def stencil():
        def make():
            tree = Inputs("true", gpu).tree(S)
            pts = torch.rand(3000, 3, generator=torch.Generator().manual_seed(41)).to(gpu)
            with torch.no_grad():
                return tree, tree.interp_stencil(pts, world=False), Inputs("true", gpu).t(synth.grad_output(3000, S.K, seed=42))

        def use(st):
            tree, sten, g = st
            f = tree.features.detach().requires_grad_(True)
            svox.interp_rows(sten, f).backward(g)
            return (f.grad,)
        return make, use

    def tv():
        def use(tree):
            with torch.no_grad():
                return (tree.tv(), tree.leaf_neighbors().neighbors)
        return (lambda: Inputs("true", gpu).tree(S)), use

    def frontier():
        def use(tree):
            with torch.no_grad():
                return (tree.reduce_frontier("sum"), tree.frontier())
        return (lambda: Inputs("true", gpu).tree(scene("shell"))), use

    return {
        "render_scratch": render(False) + ({"accel"},),                                   # the one-kernel forward: the row-major grid
        "render_split": render(False) + ({"accel", "sigma_mask"},),                       # (FWD_SPLIT "1": march + shade, a bit per row)
        "render_record": render(True) + ({"accel_bricks"},),                              # the recording forward: the grid in bricks
        "render_rgba8": rgba8() + ({"accel_bricks", "sigma_mask+exp_table"},),            # rows of 8 floats: mask and exponentials
        "padded_table": padded() + ({"pad_table"},),
        "row_plan": rows() + ({"row_plan"},),
        "stencil_plan": stencil() + ({"stencil_plan"},),
        "tv_plan": tv() + ({"leaf_neighbors", "tv_plan"},),
        "frontier": frontier() + ({"frontier"},),
    }


SCENARIOS = ["render_scratch", "render_split", "render_record", "render_rgba8", "padded_table", "row_plan", "stencil_plan", "tv_plan", "frontier"]


@pytest.mark.parametrize("name", SCENARIOS)
def test_a_cache_built_on_one_stream_is_waited_for_on_another(gpu, monkeypatch, name):
    """Build on A, consume on B without synchronising in between, then on B again and on A again.  Every product is waited
    for by B before B's first launch, exactly once; a reuse on the stream that built it, or on a stream that has waited,
    issues no wait and creates no event; both results are the default-stream bits."""
    make, use, must_build = _cache_scenarios(gpu)[name]
    if name == "render_split":
        monkeypatch.setattr(_C, "FWD_SPLIT", "1")
    want = outputs(use(make()))
    torch.cuda.synchronize()
    _C.invalidate_caches()
    st = make()
    torch.cuda.synchronize()
    A, B = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    rec = Ordering(monkeypatch)
    with torch.cuda.stream(A):
        got_a = use(st)
    built = list(rec.built)
    kinds = {p.what for p in built}
    assert all(p.handle == A.cuda_stream for p in built), [(p.what, p.handle) for p in built]
    assert not rec.waits, "a product consumed on the stream that built it was waited for"
    since = len(rec.log)
    with torch.cuda.stream(B):                        # no synchronisation in between: B must order itself behind A
        got_b = use(st)
    cached = built                                    # (a product is made through the helper only where it is cached)
    missing = [p.what for p in cached if (p, B.cuda_stream) not in rec.waits]
    assert must_build <= kinds and not missing, f"no wait recorded for {sorted(must_build - kinds) + missing} (built: {sorted(kinds)})"
    for p in cached:
        assert rec.waited_before_first_launch(p.what, B.cuda_stream, since), f"{p.what}: B launched before it waited"
        assert rec.waits.count((p, B.cuda_stream)) == 1
    assert not rec.built[len(built):], "the consumer rebuilt a cached product"
    n_built, n_waits = len(rec.built), len(rec.waits)
    with torch.cuda.stream(B):
        use(st)
    with torch.cuda.stream(A):
        use(st)
    assert len(rec.built) == n_built, f"a reuse created a product (and an event): {[p.what for p in rec.built[n_built:]]}"
    assert len(rec.waits) == n_waits, "a reuse on a stream that is already ordered waited again"
    A.synchronize()
    B.synchronize()
    for got in (outputs(got_a), outputs(got_b)):
        for i, (g, w) in enumerate(zip(got, want)):
            if name == "render_record" and i == 1:
                continue                              # (the atomic backward: its values are pinned by the late-input cases)
            same_bits(g, w, f"{name} output {i}")


@pytest.mark.parametrize("drop", ["invalidate_caches", "tree_dies", "edit_replaces_tables"])
def test_a_cache_consumed_on_another_stream_is_named_to_the_allocator(gpu, monkeypatch, drop):
    """A grid built on A and marched on B is dropped while B may still be reading it: record_stream(B) was called on it when
    B first consumed it, so the allocator does not hand the memory back to A's pool under B's kernel."""
    S = scene("random")
    inp = Inputs("true", gpu)
    tree, rays = inp.tree(S), inp.rays(S)
    tree.static_features = True
    r = svox.VolumeRenderer(tree)
    monkeypatch.setattr(_C, "FWD_SPLIT", "1")           # march + shade: the forward that reads the cached sigma bitmask
    torch.cuda.synchronize()
    _C.invalidate_caches()
    A, B = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    rec = Ordering(monkeypatch)
    with torch.no_grad():
        with torch.cuda.stream(A):
            r(tree.features, rays, sort_rays=True)
        with torch.cuda.stream(B):
            r(tree.features, rays, sort_rays=True)
    assert rec.built, "no wait recorded: nothing was built through the helper"
    for p in rec.built:
        for t in p.tensors:
            assert (t.data_ptr(), B.cuda_stream) in rec.recorded, f"{p.what}: record_stream(B) was not called"
    assert {"accel", "sigma_mask"} <= {p.what for p in rec.built}, sorted(p.what for p in rec.built)
    if drop == "invalidate_caches":
        _C.invalidate_caches()
    elif drop == "tree_dies":
        del r, tree
    else:
        tree.prune(torch.ones(tuple(tree.child.shape), dtype=torch.bool, device=gpu))
    assert not [k for k in _C._ACCEL_CACHE], "the grid outlived what it was built from"
    A.synchronize()
    B.synchronize()


def test_grad_scratch_is_per_stream(gpu, monkeypatch):
    """Two backwards of one shape on two streams get different padded gradient buffers; both gradients are within the
    project's tolerance of the default-stream one."""
    S = scene("random")
    g, _, ab = oracle_scale("random", 4, 3)
    inp = Inputs("true", gpu)
    tree, rays, gout = inp.tree(S), inp.rays(S), inp.t(g)
    r = svox.VolumeRenderer(tree)
    given, real = [], _C._grad_scratch

    def recording(dev, M, stride):
        ent = real(dev, M, stride)
        given.append((torch.cuda.current_stream(dev).cuda_stream, ent[0].data_ptr()))
        return ent

    monkeypatch.setattr(_C, "_grad_scratch", recording)

    def step():
        f = tree.features.detach().clone().requires_grad_(True)
        out = r(f, rays, sort_rays=True)
        out.backward(gout)
        return f.grad

    want = step().cpu().numpy()
    torch.cuda.synchronize()
    given.clear()
    A, B = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    grads = []
    for s in (A, B):
        with torch.cuda.stream(s):
            grads.append(step())
    assert [h for h, _ in given] == [A.cuda_stream, B.cuda_stream], given
    assert given[0][1] != given[1][1], "two streams share one gradient scratch buffer"
    A.synchronize()
    B.synchronize()
    for gr in grads:
        assert_grads_close(gr.cpu().numpy(), want, ab)


def test_what_holds_a_cached_product_is_still_copied_and_pickled(gpu):
    """An event is neither copyable nor picklable: a copy of a tree with its tv plan, or of the plan itself, is a product of
    its own on the stream that made the copy, with tensors of its own and the same values."""
    tree = Inputs("true", gpu).tree(scene("random"))
    with torch.no_grad():
        want = outputs([tree.tv()])[0]
    made = tree._last_tv_plan[1]
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        twin = copy.deepcopy(tree)
        back = pickle.loads(pickle.dumps(made))
        with torch.no_grad():
            got = twin.tv()
    s.synchronize()
    assert twin._last_tv_plan[1] is not made and twin._last_tv_plan[1].handle == back.handle == s.cuda_stream
    assert back.value.row_ptr.data_ptr() != made.value.row_ptr.data_ptr() and torch.equal(back.value.other, made.value.other)
    same_bits(outputs([got])[0], want, "tv of the copy")
