"""The per-ray and per-sample operators on adversarial trees and rays: render_depth_moments, render_distortion,
ray_samples / sample_weights / accumulate, gather_rows / reduce_rows and the row plan, view_basis / shade_samples, and
the deterministic backwards, on the inputs of tests/test_gpu_random_stress.py -- selective refinement, N = 3, anisotropic
radius and centre, feature rows in a random permutation; sigma of 0, -5 and 1e-2 ... 1e4 mixed within a ray, rows whose
coefficients are all 40; origins inside the cube, axis- and plane-parallel directions, rays that miss, directions that
are not unit length -- and on a hand-made tile whose 64 rays fill the LDS table of the sigma-only backwards to the 768
entries it ever holds.  The inputs, their references and what the references alone guarantee are those of
tests/test_adversarial_host.py; every bound is one the operator's own test file already states.

Every gradient test prints its worst |got - want| / (1e-5 scale); DESIGN.md 5 keeps the table."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import rows_restate as RR
from tests import shade_restate as SH
from tests import test_adversarial_host as H
from tests.test_gpu_samples import as_lists, assert_lists_equal
from tests.util import assert_grads_close, assert_outputs_close

pytestmark = pytest.mark.gpu
_ON = {}
KINDS = ("all", "first", "alpha")
OPS = ("entry", "mid", "distortion")
SAMPLES_ATTR = {"entry": "DEPTHMOM_SAMPLES", "mid": "DEPTHMOM_SAMPLES", "distortion": "DISTORTION_SAMPLES"}


class OnGpu:
    """A case of the host file on the GPU: its renderer, rays, feature table and the lists of ray_samples, built once."""

    def __init__(self, a, gpu):
        self.a = a
        self.r = a.renderer(gpu)
        self.rays = a.rays_on(gpu)
        self.f = a.features.to(gpu)
        self._samples = {}

    def samples(self, min_sigma=None):
        if min_sigma not in self._samples:
            self._samples[min_sigma] = self.r.ray_samples(self.rays, features=self.f, min_sigma=min_sigma)
        return self._samples[min_sigma]

    def sweep(self, op, fast=False, features=None, **kw):
        f = self.f if features is None else features
        if op == "distortion":
            return self.r.render_distortion(f, self.rays, fast=fast, **kw)
        return self.r.render_depth_moments(f, self.rays, at=op, fast=fast, **kw)

    def sweep_grad(self, op, g, **kw):
        f = self.f.clone().requires_grad_(True)
        out = self.sweep(op, features=f, **kw)
        out.backward(torch.from_numpy(g).to(f.device))
        return out.detach().cpu().numpy(), f.grad.cpu().numpy()

    def render_grad(self, cols, **kw):
        """The deterministic gradient for a.grad_out(cols): cols 1 is opacity_render's, C + 1 forward's."""
        f = self.f.clone().requires_grad_(True)
        if cols == 1:
            out = self.r.opacity_render(f, self.rays, deterministic=True, **kw)
        else:
            out = self.r(f, self.rays, deterministic=True, **kw)
        out.backward(torch.from_numpy(self.a.grad_out(cols)).to(f.device))
        return f.grad.cpu().numpy()


def on_gpu(key, gpu) -> OnGpu:
    if key not in _ON:
        _ON[key] = OnGpu(H.full_tile(key[1]) if key[0] == "tile" else H.adversarial(*key), gpu)
    return _ON[key]


def ratio_line(what, got, want, scale):
    print(f"{what}: worst |got - want| / (1e-5 scale) = {H.worst_ratio(got, want, 1e-5 * scale):.3f}")


# 1. ray_samples -----------------------------------------------------------------------------------------------------------
def check_lists(g):
    a = g.a
    for min_sigma in (None, 0.0):
        s = g.samples(min_sigma)
        want = a.lists(min_sigma)
        assert s.Q == a.Q and len(s) == want.row.shape[0] and int(s.offsets[-1]) == len(s)
        assert_lists_equal(as_lists(s), want)
        np.testing.assert_array_equal(s.counts.cpu().numpy(), np.diff(want.offsets))


@pytest.mark.parametrize("name,seed", H.IDS)
def test_ray_samples(gpu, name, seed):
    g = on_gpu((name, seed), gpu)
    n = np.diff(g.a.lists().offsets)
    assert (n == 0).sum() > 200 and (g.a.starts_inside() & (n > 0)).sum() > 50       # rays with no sample, rays from inside
    assert len(g.samples(0.0)) < len(g.samples())                                    # and the filter drops something
    check_lists(g)


# 2. sample_weights, accumulate --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", H.IDS)
def test_sample_weights(gpu, name, seed):
    """Over the unfiltered lists: sigma of 0, -5 and 1e4 within one ray."""
    g = on_gpu((name, seed), gpu)
    a, s = g.a, g.samples()
    sigma = g.f[s.row.long(), -1].clone().requires_grad_(True)
    dead = (sigma <= 0).detach()
    assert int(dead.sum()) > 1000 and int((~dead).sum()) > 10000
    w, alpha = svox.sample_weights(s, sigma)
    np.testing.assert_array_equal(alpha.detach().cpu().numpy()[:, None], a.opacity())
    assert not w.detach()[dead].any() and not torch.signbit(w.detach()[dead]).any()
    with torch.no_grad():
        m = svox.accumulate(s, w.detach(), torch.stack([s.depth, s.depth * s.depth], dim=1))
        moments = g.r.render_depth_moments(g.f, g.rays, at="entry")
    np.testing.assert_array_equal(m.cpu().numpy(), moments.cpu().numpy()[:, :2])
    np.testing.assert_array_equal(alpha.detach().cpu().numpy(), moments.cpu().numpy()[:, 2])
    gw, ga, want, scale = a.weights_grad()
    torch.autograd.backward([w, alpha], [torch.from_numpy(gw).to(gpu), torch.from_numpy(ga).to(gpu)])
    got = sigma.grad.cpu().numpy()
    ratio_line(f"sample_weights {name}/{seed}", got, want, scale)
    assert_grads_close(got, want, scale)
    assert not got[dead.cpu().numpy()].any() and (got != 0).sum() > 5000


# 3. the sigma-only operators, forward ---------------------------------------------------------------------------------------
def check_sweep_forward(g, fasts=(False, True)):
    a = g.a
    for op in OPS:
        for fast in fasts:
            with torch.no_grad():
                got = g.sweep(op, fast).cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (a.Q, 2 if op == "distortion" else 3)
            assert_outputs_close(got, a.forward64(op, fast), what=f"{op} fast={fast}")
            np.testing.assert_array_equal(got[:, -1:], a.opacity(fast))
            assert np.all(got[got[:, -1] == 0] == 0)


@pytest.mark.parametrize("name,seed", H.IDS)
def test_sweep_forward(gpu, name, seed):
    g = on_gpu((name, seed), gpu)
    check_sweep_forward(g)
    assert (g.a.opacity()[:, 0] > 0).sum() > 1000 and (g.a.opacity()[:, 0] == 0).sum() > 200


# 4. the sigma-only operators, backward --------------------------------------------------------------------------------------
def check_sweep_backward(g, op, kind, label, monkeypatch):
    """The default route, sort_rays=True, and lists of 4 and 12 records a ray (a longer ray overflows and the backward
    resumes the march): each to the same bound against the same reference."""
    a = g.a
    cols = 2 if op == "distortion" else 3
    grad_out = a.grad_out(cols, kind)
    want, scale = a.sweep_grad(op, kind)
    routes = [("default", {}, None), ("sort_rays", dict(sort_rays=True), None), ("capacity 4", {}, 4), ("capacity 12", {}, 12)]
    for route, kw, capacity in routes:
        with monkeypatch.context() as mp:
            if capacity is not None:
                mp.setattr(_C._extras, SAMPLES_ATTR[op], capacity)
            out, got = g.sweep_grad(op, grad_out, **kw)
        ratio_line(f"{label} {op} {kind} {route}", got, want, scale)
        np.testing.assert_array_equal(out[:, -1:], a.opacity())
        assert_grads_close(got, want, scale, what=f"{op} {kind} {route}")
        assert not got[:, :-1].any() and not got[scale == 0].any()
        if kind == "alpha":                              # alpha alone: the C++ oracle's opacity backward
            ow, _, tight = a.oracle_alpha_grad(cols)
            assert_grads_close(got, ow, tight, what=f"{op} alpha {route} against the oracle")
    return got


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name,seed", H.IDS)
def test_sweep_backward(gpu, name, seed, op, monkeypatch):
    g = on_gpu((name, seed), gpu)
    assert (np.diff(g.a.lists(0.0).offsets) > 12).sum() > 300             # rays that overflow lists of 4 and of 12 records
    for kind in KINDS:
        got = check_sweep_backward(g, op, kind, f"{name}/{seed}", monkeypatch)
        assert (got != 0).sum() > 1000


# 5. samples to feature rows and back ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", H.IDS)
def test_rows(gpu, name, seed):
    """The plan, gather_rows (and its gradient) and reduce_rows over lists whose rows are a random permutation."""
    g = on_gpu((name, seed), gpu)
    a, s = g.a, g.samples()
    row = a.lists().row
    T, M = row.shape[0], a.M
    want = RR.plan(row, M)
    plan = s.row_plan(M)
    np.testing.assert_array_equal(plan.row_ptr.cpu().numpy(), want.row_ptr)
    np.testing.assert_array_equal(plan.perm.cpu().numpy(), want.perm)
    assert plan.n_outside == want.n_outside == 0 and plan.longest == want.longest and plan.T == T
    assert np.any(np.diff(row[:200]) < 0) and (np.diff(want.row_ptr) == 0).sum() > 100    # no order in the rows; rows nobody names
    rng = np.random.default_rng(60 + seed)
    for K in (4, 13):
        table = rng.standard_normal((M, K)).astype(np.float32)
        v = (rng.standard_normal((T, K)) * np.exp(rng.uniform(-2, 2, (T, K)))).astype(np.float32)
        tg = torch.from_numpy(table).to(gpu).requires_grad_(True)
        vg = torch.from_numpy(v).to(gpu)
        out = svox.gather_rows(s, tg)
        np.testing.assert_array_equal(out.detach().cpu().numpy(), RR.gather(table, row))
        out.backward(vg)
        np.testing.assert_array_equal(tg.grad.cpu().numpy(), RR.gather_grad(v, row, M, K))
        for op in ("sum", "max", "mean"):
            got = svox.reduce_rows(s, vg, M, op, empty=-1.0).cpu().numpy()
            np.testing.assert_array_equal(got, RR.reduce(v, row, M, op, empty=-1.0), err_msg=f"{op} K={K}")


# 6. view_basis, shade_samples -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", H.IDS)
def test_view_basis_and_shade_samples(gpu, name, seed):
    g = on_gpu((name, seed), gpu)
    a, s = g.a, g.samples()
    L = a.lists()
    basis = g.r.view_basis(g.rays)
    if a.fmt == "RGBA":
        assert tuple(basis.shape) == (a.Q, 0)
    else:
        np.testing.assert_array_equal(basis.cpu().numpy(), O.basis(a.format, a.basis_dim, a.rays[2]))
    saturated = a.ot.features[L.row, 0] == 40
    assert saturated.sum() > 100 and (a.ot.features[L.row, -1] <= 0).sum() > 1000
    rng = np.random.default_rng(70 + seed)
    gv = rng.standard_normal((L.row.shape[0], a.C)).astype(np.float32)
    gs = rng.standard_normal(L.row.shape[0]).astype(np.float32)
    for activate in (True, False):
        f = g.f.clone().requires_grad_(True)
        values, sigma = g.r.shade_samples(s, f, g.rays, activate=activate)
        want_v, want_s = a.shaded(None, activate)
        np.testing.assert_array_equal(values.detach().cpu().numpy(), want_v)
        np.testing.assert_array_equal(sigma.detach().cpu().numpy(), want_s)
        got = torch.autograd.grad([values, sigma], [f], [torch.from_numpy(gv).to(gpu), torch.from_numpy(gs).to(gpu)])[0]
        want = SH.grad(a.ot.features, L.row, L.ray, a.opt, a.basis(), want_v, gv, gs, activate)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert np.count_nonzero(want) > 10000
        if activate and a.fmt == "RGBA":             # a saturated sigmoid is 1, its derivative an exact 0 through double
            assert np.all(want_v[saturated] == 1)


# 7. the deterministic backwards -----------------------------------------------------------------------------------------------
def check_deterministic(g, label):
    a = g.a
    for cols in (a.C + 1, 1):
        got = g.render_grad(cols)
        np.testing.assert_array_equal(got, a.rowgrad(cols))
        want, _, tight = a.oracle_grad(cols)
        ratio_line(f"{label} deterministic grad_out [Q, {cols}]", got, want, tight)
        assert np.all(np.abs(got.astype(np.float64) - want) <= 1e-5 * tight)
        for kw in (dict(sort_rays=True), dict(fast=True)):
            assert np.array_equal(g.render_grad(cols, **kw), got), kw
        if cols == 1:
            assert not got[:, :-1].any()
    return got


@pytest.mark.parametrize("name,seed", H.IDS)
def test_deterministic_backwards(gpu, name, seed):
    g = on_gpu((name, seed), gpu)
    got = check_deterministic(g, f"{name}/{seed}")
    assert np.count_nonzero(got[:, -1]) > 1000


# 8. the composed renderer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_sigma", [0.0, None])
@pytest.mark.parametrize("name,seed", H.IDS)
def test_composed_renderer(gpu, name, seed, min_sigma):
    """ray_samples -> shade_samples -> sample_weights -> accumulate, plus (1 - alpha) background_brightness, against
    forward: the bound of tests/test_gpu_shade.py's composed chain, n the ray's samples with sigma > 0 (with min_sigma
    None the lists keep the others: their weight is an exact 0 and adds nothing)."""
    g = on_gpu((name, seed), gpu)
    a, s = g.a, g.samples(min_sigma)
    with torch.no_grad():
        values, sigma = g.r.shade_samples(s, g.f, g.rays)
        w, alpha = svox.sample_weights(s, sigma)
        out = svox.accumulate(s, w, values)
        full = torch.cat([out + (1.0 - alpha)[:, None] * g.r.background_brightness, alpha[:, None]], dim=1)
        want = g.r(g.f, g.rays)
    np.testing.assert_array_equal(want.cpu().numpy(), a.render())
    assert torch.equal(full[:, a.C], want[:, a.C])
    x, b = full[:, :a.C].cpu().numpy().astype(np.float64), want[:, :a.C].cpu().numpy().astype(np.float64)
    n = g.samples(0.0).counts.cpu().numpy().astype(np.float64)[:, None]
    excess = np.abs(x - b) - ((n + 4) * 2.0 ** -23 * np.abs(b) + 1e-7)
    print(f"{name}/{seed} min_sigma={min_sigma}: worst |a - b| - bound = {excess.max():.3e}; worst |a - b| = {np.abs(x - b).max():.3e}")
    assert np.all(excess <= 0), (int((excess > 0).sum()), float(excess.max()))


# the full-table tile ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("behind_misses", [False, True])
def test_full_table_tile(gpu, behind_misses, monkeypatch):
    """64 rays whose first 12 samples name 768 distinct feature rows -- everything the LDS table of the sigma-only
    backwards takes between two flushes -- and 1 024 in all; alone, and as the last tile of a batch behind 64 rays that
    miss.  Items 1, 3, 4 and 7 of the cases above."""
    g = on_gpu(("tile", behind_misses), gpu)
    n, first, total = g.a.counts()
    assert np.all(n == 16) and first == 768 and total == 1024                # from samples_restate.lists
    label = "tile behind misses" if behind_misses else "tile"
    check_lists(g)
    check_sweep_forward(g)
    for op in OPS:
        for kind in KINDS:
            got = check_sweep_backward(g, op, kind, label, monkeypatch)
            assert np.count_nonzero(got[:, -1]) == 1024, (op, kind)
    got = check_deterministic(g, label)
    assert np.count_nonzero(got[:, -1]) == 1024
