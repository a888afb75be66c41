"""The adversarial inputs of tests/test_gpu_adversarial.py without a GPU: the irregular trees and incoherent rays of
tests/test_gpu_random_stress.py (random_tree / random_rays) and a hand-made tile that fills the LDS table of the
sigma-only backwards, built once and shared with the GPU file, and what the references alone say about them -- so that
a failure on the GPU points at a kernel and not at the inputs:

    the float32 restatements stay within half of the forward bound of the float64 ones;
    rowgrad_restate.grad stays within half of 1e-5 * tight of the C++ oracle;
    every float64 reference and every scale is finite, and no reference gradient is non-zero where its scale is 0;
    the restatements composed into a renderer give the oracle's alpha and its colours within the composed chain's bound;
    the full-table tile has 16 samples a ray, 768 distinct rows in a lane's first 12 samples and 1 024 in all.

The 0.5 is a cap on the references, not a kernel tolerance: it keeps a later change of the inputs from quietly eating
the room the kernels need."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
from oracle import oracle as O
from svox_t_amd import synth
from tests import depth_restate as D
from tests import distortion_restate as DS
from tests import rowgrad_restate as RG
from tests import samples_restate as SR
from tests import shade_restate as SH
from tests.test_gpu_random_stress import random_rays, random_tree
from tests.test_gpu_rowgrad import full_tree

CASES = {
    "n2_sh4": dict(N=2, fmt="SH4", K=13, max_depth=6),
    "n2_rgba4": dict(N=2, fmt="RGBA", K=4, max_depth=6),
    "n3_sh1": dict(N=3, fmt="SH1", K=4, max_depth=3),
}
SEEDS = (0, 1)
IDS = [(name, seed) for name in CASES for seed in SEEDS]
Q = 2000                                   # 31 tiles of 64 rays and one of 16
STEP, BACKGROUND = 2e-3, 0.5
RADIUS, CENTER = (0.7, 1.3, 0.9), (0.2, -0.1, 0.4)          # random_tree's own defaults
_BUILT = {}


class Inputs:
    """A tree as numpy tables with its oracle twin, a ray batch and the options, and every reference a test asks for,
    computed once.  The objects are kept: tests.depth_restate.march recognises a case by them."""

    def _adopt(self, t, feats, fmt, rays):
        n = t.n_internal
        self.fmt, self.K, self.M = fmt, int(feats.shape[1]), int(feats.shape[0])
        self.features = feats
        self.child, self.data = t.child[:n].numpy().copy(), t.data[:n].numpy().copy()
        self.parent_depth = t.parent_depth[:n].numpy().copy()
        self.ot = O.Tree(feats.numpy(), self.data, self.child, offset=t.offset.numpy().copy(), scaling=t.invradius.numpy().copy())
        self.rays = tuple(np.ascontiguousarray(a) for a in rays)
        self.Q = self.rays[0].shape[0]
        df = svox.DataFormat(fmt)
        self.format, self.basis_dim = df.format, df.basis_dim
        self.opt = self.opts()
        self.C = O.out_data_dim(self.opt, self.K) - 1
        self._ref = {}

    def opts(self, fast=False):
        th = 1e-2 if fast else 0.0
        return O.make_options(step_size=STEP, background_brightness=BACKGROUND, format=self.format, basis_dim=self.basis_dim,
                              sigma_thresh=th, stop_thresh=th)

    def tree(self, device):
        return svox.N3Tree.from_arrays(self.child, self.data, self.parent_depth, self.features, data_format=self.fmt,
                                       radius=list(self.radius), center=list(self.center), device=device)

    def renderer(self, device):
        return svox.VolumeRenderer(self.tree(device), step_size=STEP, background_brightness=BACKGROUND)

    def rays_on(self, device):
        return svox.Rays(*(torch.from_numpy(a).to(device) for a in self.rays))

    def ref(self, key, make):
        if key not in self._ref:
            self._ref[key] = make()
        return self._ref[key]

    # the lists ---------------------------------------------------------------------------------------------------------
    def lists(self, min_sigma=None):
        return self.ref(("lists", min_sigma), lambda: SR.lists(self.ot, self.rays, self.opt, min_sigma))

    def starts_inside(self):
        """The rays whose origin lies strictly inside the tree's cube."""
        o = self.ot.offset + self.ot.scaling * self.rays[0]
        return np.all((o > 0) & (o < 1), axis=1)

    # upstream gradients ------------------------------------------------------------------------------------------------
    def grad_out(self, cols, kind="all", seed=11):
        """synth.grad_output [Q, cols]; kind "first": the first column alone, "alpha": the last column alone."""
        g = synth.grad_output(self.Q, cols, seed=seed).numpy()
        if kind == "first":
            g[:, 1:] = 0
        elif kind == "alpha":
            g[:, :-1] = 0
        else:
            assert kind == "all", kind
        return g

    # the sigma-only operators: (float64 autograd, scale) per operator and kind, the forward's graph built once ----------
    def _graph(self, op):
        def make():
            feats = torch.from_numpy(self.ot.features).double().requires_grad_(True)
            zero = D._zero_thresholds(self.opt)
            if op == "distortion":
                out = DS.distortion(self.ot, self.rays, zero, torch.float64, features=feats, early_stop=False)
            else:
                out = D.moments(self.ot, self.rays, zero, op, torch.float64, features=feats, early_stop=False)
            return feats, out
        return self.ref(("graph", op), make)

    def sweep_grad(self, op, kind):
        """(want, scale) float64 [M, K] of op "entry" | "mid" (render_depth_moments) | "distortion" for grad_out(kind): what
        depth_restate.moments_grad / distortion_restate.distortion_grad compute, over one forward per operator."""
        def make():
            feats, out = self._graph(op)
            g = self.grad_out(2 if op == "distortion" else 3, kind)
            want = torch.autograd.grad((out * torch.from_numpy(g).double()).sum(), feats, retain_graph=True)[0].numpy()
            if op == "distortion":
                scale = DS.distortion_grad_scale(self.ot, self.rays, self.opt, g)
            else:
                scale = D.moments_grad_scale(self.ot, self.rays, self.opt, op, g)
            return want, scale
        return self.ref(("sweep_grad", op, kind), make)

    def forward64(self, op, fast=False):
        def make():
            if op == "distortion":
                return DS.distortion(self.ot, self.rays, self.opts(fast), torch.float64).numpy()
            return D.moments(self.ot, self.rays, self.opts(fast), op, torch.float64).numpy()
        return self.ref(("forward64", op, fast), make)

    def opacity(self, fast=False):
        return self.ref(("opacity", fast), lambda: O.opacity_render(self.ot, *self.rays, self.opts(fast)))

    def oracle_grad(self, cols, kind="all"):
        """(grad, abs_sum, tight) of O.volume_render_backward for grad_out(cols, kind); cols 1: the opacity backward."""
        def make():
            g = self.grad_out(cols, kind)
            return O.volume_render_backward(self.ot, *self.rays, self.opt, g, want_abs="both")
        return self.ref(("oracle_grad", cols, kind), make)

    def oracle_alpha_grad(self, cols):
        """(grad, abs_sum, tight) of the oracle's opacity backward for the alpha column of grad_out(cols, "alpha")."""
        def make():
            g = np.ascontiguousarray(self.grad_out(cols, "alpha")[:, -1:])
            return O.volume_render_backward(self.ot, *self.rays, self.opt, g, want_abs="both")
        return self.ref(("oracle_alpha_grad", cols), make)

    def rowgrad(self, cols):
        return self.ref(("rowgrad", cols), lambda: RG.grad(self.ot, self.rays, self.opt, self.grad_out(cols)))

    def render(self, fast=False):
        return self.ref(("render", fast), lambda: O.volume_render(self.ot, *self.rays, self.opts(fast)))

    # shade_samples -------------------------------------------------------------------------------------------------------
    def basis(self):
        return self.ref("basis", lambda: SH.basis(self.opt, self.rays[2]))

    def shaded(self, min_sigma=None, activate=True):
        """(values [T, C], sigma [T]) of shade_restate.forward over lists(min_sigma)."""
        L = self.lists(min_sigma)
        return self.ref(("shaded", min_sigma, activate),
                        lambda: SH.forward(self.ot.features, L.row, L.ray, self.opt, self.basis(), activate))

    # sample_weights: upstream gradients, the float64 autograd and its scale ------------------------------------------------
    def weights_grad(self):
        """(gw [T], ga [Q], want [T], scale [T]) over lists(None) with sigma = features[row, -1]."""
        def make():
            L = self.lists()
            sigma = self.ot.features[L.row, -1]
            rng = np.random.default_rng(22)
            gw = rng.standard_normal(L.row.shape[0]).astype(np.float32)
            ga = rng.standard_normal(self.Q).astype(np.float32)
            s64 = torch.from_numpy(sigma).double().requires_grad_(True)
            w64, a64 = SR.weights(L.length, s64, L.offsets, torch.float64)
            ((w64 * torch.from_numpy(gw).double()).sum() + (a64 * torch.from_numpy(ga).double()).sum()).backward()
            return gw, ga, s64.grad.numpy(), SR.grad_sigma_scale(L.length, sigma, L.offsets, gw, ga)
        return self.ref("weights_grad", make)


class Adversarial(Inputs):
    """random_tree(seed) of a case and random_rays(100 + seed, 2 000 rays) over it."""

    def __init__(self, name, seed):
        cfg = CASES[name]
        t, feats = random_tree(seed, N=cfg["N"], max_depth=cfg["max_depth"], data_format=cfg["fmt"], K=cfg["K"])
        self.radius, self.center = RADIUS, CENTER
        self._adopt(t, feats, cfg["fmt"], (a.numpy() for a in random_rays(100 + seed, Q, t)))


class FullTile(Inputs):
    """A full N = 2 tree of 16^3 leaves, one feature row each with sigma > 0, and the 64 rays along +x through the centres
    of every other leaf in y and z: 16 samples a ray, no row twice.  A lane's first 12 samples -- one pass of the
    sigma-only backward between two flushes of its LDS table -- name 64 x 12 = 768 distinct rows, the most the table
    ever holds (csrc/svoxt_raylists.h).  behind_misses: the same 64 rays as the second tile, behind 64 rays that miss."""

    def __init__(self, behind_misses=False):
        t, feats = full_tree(2, 3, K=4, occupied=1.0)
        feats = feats.clone()
        feats[:, -1] = feats[:, -1].abs() + 0.5
        self.radius, self.center = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
        j, k = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
        o = np.stack([np.full(64, -0.5), (2 * j.reshape(-1) + 0.5) / 16, (2 * k.reshape(-1) + 0.5) / 16], axis=1).astype(np.float32)
        d = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (64, 1))
        if behind_misses:
            o = np.concatenate([np.full((64, 3), 5.0, np.float32), o])
            d = np.concatenate([np.tile(np.array([[0.6, 0.0, 0.8]], np.float32), (64, 1)), d])     # away from the cube
        self._adopt(t, feats, "RGBA", (o, d, d.copy()))

    def counts(self):
        """(samples a ray of the 64 rays, distinct rows among their first 12 samples, distinct rows among all)."""
        L = self.lists()
        n = np.diff(L.offsets)[-64:]
        first = np.concatenate([L.row[a:a + 12] for a in L.offsets[-65:-1]])
        return n, np.unique(first).shape[0], np.unique(L.row).shape[0]


def adversarial(name, seed) -> Adversarial:
    if (name, seed) not in _BUILT:
        _BUILT[name, seed] = Adversarial(name, seed)
    return _BUILT[name, seed]


def full_tile(behind_misses=False) -> FullTile:
    if ("tile", behind_misses) not in _BUILT:
        _BUILT["tile", behind_misses] = FullTile(behind_misses)
    return _BUILT["tile", behind_misses]


def worst_ratio(got, want, bound):
    """max |got - want| / (bound + 1e-30), the denormal-sized floor of tests.util.assert_grads_close."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    return float((err / (np.asarray(bound, np.float64) + 1e-30)).max()) if err.size else 0.0


# the inputs are what the GPU file says they are ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", IDS)
def test_the_inputs_are_hostile(name, seed):
    a = adversarial(name, seed)
    L, L0 = a.lists(), a.lists(0.0)
    n = np.diff(L.offsets)
    inside = a.starts_inside()
    sigma = a.ot.features[L.row, -1]
    print(f"{name}/{seed}: M {a.M}, samples {L.row.shape[0]} ({L0.row.shape[0]} with sigma > 0), longest {n.max()}, "
          f"rays without a sample {(n == 0).sum()}, rays from inside {inside.sum()} ({(inside & (n > 0)).sum()} with samples)")
    assert 5000 <= a.M <= 16500 and 10000 < L0.row.shape[0] < 25000 and np.diff(L0.offsets).max() < 64       # small on purpose
    assert (n == 0).sum() > 200 and (inside & (n > 0)).sum() > 50
    # zero direction components, on rays that have samples
    assert ((a.rays[1] == 0).sum(1) == 2)[n > 0].sum() > 20 and ((a.rays[1] == 0).sum(1) == 1)[n > 0].sum() > 20
    # every kind of sigma, mixed within rays; rows whose coefficients are all 40
    assert (sigma == 0).sum() > 500 and (sigma < 0).sum() > 500 and (sigma > 1e3).sum() > 500
    per_ray = lambda mask: np.add.reduceat(np.append(mask, False).astype(np.int64), L.offsets[:-1])[n > 0] > 0     # noqa: E731
    assert (per_ray(sigma <= 0) & per_ray(sigma > 1e3) & per_ray((sigma > 0) & (sigma < 1))).sum() > 100
    assert (a.ot.features[L0.row, 0] == 40).sum() > 100
    # random_tree's rows are a permutation: a tile of 64 rays names hundreds of distinct rows in one pass of the table
    first = [np.unique(np.concatenate([L0.row[b:b + 12] for b in L0.offsets[t:t + 64]])).shape[0] for t in range(0, Q - 63, 64)]
    assert max(first) > 400 and np.any(np.diff(L0.row[:200]) < 0)


def test_the_full_table_tile():
    for behind in (False, True):
        t = full_tile(behind)
        n, first, total = t.counts()
        assert t.M == 4096 and t.Q == (128 if behind else 64)
        assert np.all(n == 16) and first == 768 and total == 1024
        assert np.all(t.ot.features[:, -1] >= 0.5)
        if behind:
            assert not np.diff(t.lists().offsets)[:64].any()


# the references hold the bounds with room to spare ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", IDS)
def test_float32_restatements_stay_within_the_forward_bound(name, seed):
    a = adversarial(name, seed)
    for op in ("entry", "mid", "distortion"):
        for fast in (False, True):
            want = a.forward64(op, fast)
            if op == "distortion":
                got = DS.distortion(a.ot, a.rays, a.opts(fast), torch.float32).numpy()
            else:
                got = D.moments(a.ot, a.rays, a.opts(fast), op, torch.float32).numpy()
            ratio = worst_ratio(got, want, 1e-5 * np.abs(want) + 1e-6)
            print(f"{name}/{seed} {op} fast={fast}: worst err / bound {ratio:.3f}")
            assert np.isfinite(want).all() and ratio < 0.5
            np.testing.assert_array_equal(got[:, -1:], a.opacity(fast))


@pytest.mark.parametrize("name,seed", IDS)
def test_rowgrad_restatement_stays_within_the_oracles_tolerance(name, seed):
    a = adversarial(name, seed)
    for cols in (a.C + 1, 1):
        want, absum, tight = a.oracle_grad(cols)
        got = a.rowgrad(cols)
        ratio = worst_ratio(got, want, 1e-5 * tight)
        print(f"{name}/{seed} grad_out [Q, {cols}]: worst err / (1e-5 tight) {ratio:.3f}")
        assert np.isfinite(want).all() and np.isfinite(tight).all() and np.isfinite(got).all()
        assert ratio < 0.5 and not got[tight == 0].any() and not want[tight == 0].any()
        assert np.count_nonzero(want[:, -1]) > 1000


@pytest.mark.parametrize("name,seed", IDS)
def test_references_and_scales_are_finite(name, seed):
    a = adversarial(name, seed)
    for op in ("entry", "mid", "distortion"):
        for kind in ("all", "first", "alpha"):
            want, scale = a.sweep_grad(op, kind)
            assert np.isfinite(want).all() and np.isfinite(scale).all() and np.all(scale >= 0), (op, kind)
            assert not want[scale == 0].any() and not scale[:, :-1].any() and np.count_nonzero(want) > 1000, (op, kind)
            if kind == "alpha":                      # alpha alone: the C++ oracle's opacity backward, under both scales
                ow, _, tight = a.oracle_alpha_grad(2 if op == "distortion" else 3)
                assert worst_ratio(want, ow, 1e-5 * tight) < 0.5 and worst_ratio(want, ow, 1e-5 * scale) < 0.5
    gw, ga, want, scale = a.weights_grad()
    sigma = a.ot.features[a.lists().row, -1]
    assert np.isfinite(want).all() and np.isfinite(scale).all()
    assert not want[scale == 0].any() and np.all((scale > 0) == (sigma > 0))


def test_full_table_tile_references():
    for behind in (False, True):
        t = full_tile(behind)
        for op in ("entry", "mid", "distortion"):
            for kind in ("all", "first", "alpha"):
                want, scale = t.sweep_grad(op, kind)
                assert np.isfinite(want).all() and np.isfinite(scale).all() and not want[scale == 0].any()
                assert np.count_nonzero(want[:, -1].astype(np.float32)) == np.count_nonzero(scale[:, -1]) == 1024
        want, _, tight = t.oracle_grad(4)
        assert worst_ratio(t.rowgrad(4), want, 1e-5 * tight) < 0.5 and np.count_nonzero(want[:, -1]) == 1024


@pytest.mark.parametrize("name,seed", IDS)
def test_composed_restatements_against_the_oracles_renderer(name, seed):
    """lists -> shade_restate.forward -> samples_restate.weights -> accumulate in float32, plus (1 - alpha) background:
    alpha has the bits of O.volume_render's, the colours are within (n + 4) 2^-23 |b| + 1e-7 of it, n the ray's samples
    with sigma > 0 (tests/test_gpu_shade.py states the bound) -- whether or not the lists keep the samples with
    sigma <= 0, whose weight is an exact 0."""
    a = adversarial(name, seed)
    want = a.render()
    n = np.diff(a.lists(0.0).offsets).astype(np.float64)[:, None]
    for min_sigma in (0.0, None):
        L = a.lists(min_sigma)
        values, sigma = a.shaded(min_sigma)
        w, alpha = SR.weights(L.length, sigma, L.offsets, torch.float32)
        assert not w.numpy()[sigma <= 0].any()
        out = SR.accumulate(w, values, L.offsets, torch.float32)
        full = (out + (1.0 - alpha)[:, None] * np.float32(BACKGROUND)).numpy()
        np.testing.assert_array_equal(alpha.numpy(), want[:, a.C])
        b = want[:, :a.C].astype(np.float64)
        excess = np.abs(full.astype(np.float64) - b) - ((n + 4) * 2.0 ** -23 * np.abs(b) + 1e-7)
        print(f"{name}/{seed} min_sigma={min_sigma}: worst |a - b| - bound = {excess.max():.3e}")
        assert np.all(excess <= 0)
    assert (a.ot.features[a.lists(0.0).row, 0] == 40).sum() > 100
