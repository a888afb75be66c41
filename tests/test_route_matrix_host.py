"""The inputs of tests/test_gpu_route_matrix.py without a GPU: the irregular trees of tests/test_gpu_random_stress.py
(random_tree: selective refinement, rows in a random permutation, empty leaves, sigma of 0, -5 and 1e-2 ... 1e4 within a
ray, saturated coefficients, anisotropic world scaling) with ONE PAYLOAD PER KERNEL FAMILY of the colour render step, and
three ray batches a tree -- random_rays as they come, an image whose camera sits inside the cube, an image most of whose
tiles miss -- built once and shared with the GPU file, every reference computed once per (tree, batch), and what the
inputs and references alone guarantee, so that a failure on the GPU points at a kernel and not at the inputs:

    ragged   many rays without a sample, rays longer than 36 samples (depth-6 trees) and than 24 with sigma > 0, none
             longer than the default list capacity of 96,
             origins inside the cube, sigma = 0, < 0 and >= 1e3 among the rows of one ray's list;
    inside   every origin strictly inside the cube, no ray without a sample;
    far      most rays miss, many 8 x 8 tiles without a sample, tiles that mix hits with misses;
    all      some ray with more than 12 samples of sigma > 0 (lists of 4 and 12 records overflow);
    every reference is finite, no reference gradient is non-zero where its scale is 0.

Also here: oracle.Tree without the lobes an SG / ASG format needs is a ValueError, not a null pointer in the C++ oracle."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
from oracle import oracle as O
from svox_t_amd import synth
from tests import test_adversarial_host as H
from tests.test_gpu_random_stress import random_rays, random_tree

# name -> N, depth, format, K, what it is there for (the family of kernels its default route must reach)
PAYLOADS = {
    "sh9": dict(N=2, max_depth=6, fmt="SH9", K=28),                   # fwd_roles_kernel, grad_fused_kernel<EXACT>: the headline pair
    "rgba4": dict(N=2, max_depth=6, fmt="RGBA", K=4),                 # the same pair, RGBA
    "rgba8": dict(N=2, max_depth=6, fmt="RGBA", K=8, extreme=True),   # march_rec + shade_chan, grad_wide_kernel, <ONEPASS>, the table
    "rgba32": dict(N=2, max_depth=6, fmt="RGBA", K=32, extreme=True),
    "sh16": dict(N=2, max_depth=5, fmt="SH16", K=49),                 # the wide-SH per-tile backward over the forward's hand-over
    "sg9": dict(N=2, max_depth=6, fmt="SG9", K=28, lobes=9),          # SG lists serve the exact per-tile backward only
    "sh4_two": dict(N=2, max_depth=6, fmt="SH4", K=9),                # PAD_PAYLOADS: two channels rendered as three
    "rgba6": dict(N=2, max_depth=6, fmt="RGBA", K=6),                 # PAD_PAYLOADS: a row of 8
    "sh4_four": dict(N=2, max_depth=5, fmt="SH4", K=17),              # GROUP_PAYLOADS: four channels in two groups
    "sh4_xf": dict(N=2, max_depth=6, fmt="SH4", K=13, xf=True),       # transformation_matrices: the <XF> kernels
    "n3_sh1": dict(N=3, max_depth=3, fmt="SH1", K=4),                 # N = 3: the per-ray kernels
}
SEEDS = (0, 1)
BATCHES = ("ragged", "inside", "far")
IDS = [(p, s, b) for p in PAYLOADS for s in SEEDS for b in BATCHES]
Q = 2048
INSIDE = dict(width=48, height=40, radius=0.45, fx=1111.111 * 48 / 800.0)
FAR = dict(width=64, height=32, radius=4.0, fx=40.0)
# the extreme feature values of tests/test_gpu_exp_table.py: exponentials that overflow to +inf or underflow to 0
EXTREME = (-200.0, -89.0, -88.72, -87.5, -1e-30, 0.0, 1e-30, 86.9, 87.1, 103.0, 1e30, -1e30)
_TREES, _BUILT = {}, {}


def _tree(payload, seed):
    """(N3Tree on the CPU, features, lobes or None, view rotations or None) of a payload and seed, built once."""
    if (payload, seed) not in _TREES:
        cfg = PAYLOADS[payload]
        t, feats = random_tree(seed, N=cfg["N"], max_depth=cfg["max_depth"], data_format=cfg["fmt"], K=cfg["K"])
        g = torch.Generator().manual_seed(1000 + seed)
        if cfg.get("extreme"):
            sel = torch.rand(feats[:, :-1].shape, generator=g)
            vals = torch.tensor(EXTREME)
            pick = vals[torch.randint(0, len(vals), feats[:, :-1].shape, generator=g)]
            feats[:, :-1] = torch.where(sel < 0.5, pick, feats[:, :-1])
        lobes = xf = None
        if cfg.get("lobes"):        # as tests/test_gpu_render_parity.py::test_random_views_through_the_image_routes makes them
            lobes = torch.cat([torch.rand(cfg["lobes"], 1, generator=g) * 4 + 0.5,
                               torch.nn.functional.normalize(torch.randn(cfg["lobes"], 3, generator=g), dim=-1)], -1).contiguous()
        if cfg.get("xf"):
            xf = torch.randn(feats.shape[0], 4, 4, generator=g)
        _TREES[payload, seed] = (t, feats, lobes, xf)
    return _TREES[payload, seed]


class RouteInputs(H.Inputs):
    """A payload's tree of one seed with one of its three ray batches, and every reference the GPU file asks for."""

    def __init__(self, payload, seed, batch):
        cfg = PAYLOADS[payload]
        t, feats, lobes, xf = _tree(payload, seed)
        self.payload, self.seed, self.batch = payload, seed, batch
        self.radius, self.center = H.RADIUS, H.CENTER
        self.lobes, self.xf = lobes, xf
        self.image = self.pose = self.fx = None
        if batch == "ragged":
            rays = tuple(a.numpy() for a in random_rays(100 + seed, Q, t))
        else:
            cam = INSIDE if batch == "inside" else FAR
            self.pose = synth.camera_pose(azimuth_deg=30 + 50 * seed, elevation_deg=20, radius=cam["radius"],
                                          center=H.CENTER).astype(np.float32)
            self.fx, self.image = cam["fx"], (cam["height"], cam["width"])
            # the rays the kernels of render_persp form themselves (cam2world_ray): one reference serves both ways in
            rays = O.camera_rays(self.pose, self.fx, self.fx, cam["width"], cam["height"])
        self._adopt(t, feats, cfg["fmt"], rays)
        if lobes is not None:
            self.ot = O.Tree(self.ot.features, self.data, self.child, offset=self.ot.offset, scaling=self.ot.scaling,
                             extra=lobes.numpy())

    def tree(self, device):
        return svox.N3Tree.from_arrays(self.child, self.data, self.parent_depth, self.features, data_format=self.fmt,
                                       radius=list(self.radius), center=list(self.center), extra_data=self.lobes, device=device)

    rays_gpu = H.Inputs.rays_on          # (the name tests/test_gpu_step_api.py::_run asks a case for)

    def ref(self, key, make):
        """Every reference of a tree with view rotations is the oracle's under O.transformation_matrices."""
        if self.xf is None or key in self._ref:
            return super().ref(key, make)
        with O.transformation_matrices(self.xf.numpy()):
            return super().ref(key, make)

    def depth(self, fast=False):
        return self.ref(("depth", fast), lambda: O.render_depth(self.ot, *self.rays, self.opts(fast)))

    def step_api(self, fast=False):
        """(out, grad, abs_sum, tight) for the options of tests/test_gpu_step_api.py::_run: the renderer's defaults
        (step 1e-3, white background) and grad_out(C + 1) -- its synth.grad_output(Q, C + 1, seed=11)."""
        def make():
            th = 1e-2 if fast else 0.0
            oo = O.make_options(format=self.format, basis_dim=self.basis_dim, sigma_thresh=th, stop_thresh=th)
            out = O.volume_render(self.ot, *self.rays, oo)
            return (out,) + tuple(O.volume_render_backward(self.ot, *self.rays, oo, self.grad_out(self.C + 1), want_abs="both"))
        return self.ref(("step_api", fast), make)

    def tiles(self):
        """Samples per 8 x 8 pixel tile of an image batch, [tiles, 64]: the order the kernels walk a declared image in."""
        h, w = self.image
        n = np.diff(self.lists().offsets).reshape(h // 8, 8, w // 8, 8)
        return n.transpose(0, 2, 1, 3).reshape(-1, 64)


def inputs(payload, seed, batch) -> RouteInputs:
    if (payload, seed, batch) not in _BUILT:
        _BUILT[payload, seed, batch] = RouteInputs(payload, seed, batch)
    return _BUILT[payload, seed, batch]


# the inputs are what the GPU file says they are ------------------------------------------------------------------------------
@pytest.mark.parametrize("payload,seed", [(p, s) for p in PAYLOADS for s in SEEDS])
def test_the_trees_are_irregular(payload, seed):
    cfg = PAYLOADS[payload]
    a = inputs(payload, seed, "ragged")
    depth = a.parent_depth[:, 1]
    leaf = a.child == 0
    occupied = leaf & (a.data[..., 0] >= 0) & (a.data[..., 0] < a.M)
    rows = a.data[..., 0][occupied]
    print(f"{payload}/{seed}: {a.child.shape[0]} internal nodes, M {a.M}, depths {depth.min()}..{depth.max()}")
    assert a.ot.N == cfg["N"] and a.K == cfg["K"] and a.features.shape == (a.M, a.K)
    assert np.unique(depth).shape[0] >= cfg["max_depth"] - 1                 # leaves at every level: the depth changes from cell to cell
    assert (leaf & ~occupied).sum() > 0.2 * leaf.sum()                      # empty leaves
    assert np.array_equal(np.sort(rows), np.arange(a.M)) and np.any(np.diff(rows) < 0)       # the rows are a permutation, not in leaf order
    sigma = a.ot.features[:, -1]
    assert (sigma == 0).sum() > 0.05 * a.M and (sigma == -5).sum() > 0.05 * a.M and (sigma >= 1e3).sum() > 0.05 * a.M
    if not cfg.get("extreme"):
        assert np.all(a.ot.features[:, :-1] == 40, axis=1).sum() > 0.02 * a.M                 # saturated sigmoids
    else:
        colour = a.ot.features[:, :-1]
        for v in EXTREME:
            assert (colour == np.float32(v)).sum() > 0.02 * colour.size, v
        assert 0.4 < np.isin(colour, np.asarray(EXTREME, np.float32)).mean() < 0.6
    if cfg["max_depth"] == 6:
        assert 3000 <= a.child.shape[0] <= 4500 and 12000 <= a.M <= 20000
    if a.lobes is not None:
        assert a.ot.extra.shape == (cfg["lobes"], 4)
    if a.xf is not None:
        assert tuple(a.xf.shape) == (a.M, 4, 4)


@pytest.mark.parametrize("payload,seed,batch", IDS)
def test_the_batches_are_what_they_claim(payload, seed, batch):
    a = inputs(payload, seed, batch)
    L, L0 = a.lists(), a.lists(0.0)
    n, n0 = np.diff(L.offsets), np.diff(L0.offsets)
    inside = a.starts_inside()
    print(f"{payload}/{seed}/{batch}: Q {a.Q}, rays without a sample {(n == 0).sum()}, longest {n.max()} ({n0.max()} with sigma > 0), "
          f"rays from inside {inside.sum()}")
    assert a.Q == (Q if a.image is None else a.image[0] * a.image[1]) and n0.max() > 12 and n.max() <= 96
    if batch == "ragged":
        assert a.image is None and (n == 0).sum() >= 400 and n0.max() > 24
        # (a depth-5 tree is 32 leaves across and the N = 3 tree 27: their longest rays have 29 ... 42 samples, and of twelve
        # ray seeds tried on the depth-5 tree of seed 1 none gave more than 33 -- "more than 36" is held where a tree can give it)
        assert n.max() > (36 if PAYLOADS[payload]["max_depth"] == 6 else 28)
        assert 0 < inside.sum() < Q and (inside & (n > 0)).sum() > 50
        sigma = a.ot.features[L.row, -1]
        per_ray = lambda mask: np.add.reduceat(np.append(mask, False).astype(np.int64), L.offsets[:-1])[n > 0] > 0     # noqa: E731
        assert (per_ray(sigma == 0) & per_ray(sigma < 0) & per_ray(sigma >= 1e3)).sum() >= 100
        # ... alternating within the ray: a sample with sigma <= 0 between two with sigma > 0, and lists that END on one
        live = sigma > 0
        assert (live[:-2] & ~live[1:-1] & live[2:] & (L.ray[:-2] == L.ray[2:])).sum() > 1000
        assert (~live[L.offsets[1:][n > 0] - 1]).sum() > 100
    elif batch == "inside":
        assert a.image == (40, 48) and inside.all() and (n == 0).sum() == 0
        assert np.all(a.rays[0] == a.rays[0][0])                                 # one origin: the march of every ray starts inside a leaf
    else:
        assert a.image == (32, 64) and not inside.any() and (n == 0).sum() >= 1400
        t = a.tiles()
        empty, mixed = ~t.any(axis=1), t.any(axis=1) & ~t.all(axis=1)
        print(f"    tiles without a sample {empty.sum()}, tiles that mix hits and misses {mixed.sum()}, of {t.shape[0]}")
        assert t.shape[0] == 32 and empty.sum() >= 10 and mixed.sum() >= 4


@pytest.mark.parametrize("payload,seed,batch", IDS)
def test_references_are_finite_and_zero_where_their_scale_is(payload, seed, batch):
    a = inputs(payload, seed, batch)
    extreme = PAYLOADS[payload].get("extreme", False)
    for fast in (False, True):
        out = a.render(fast)
        assert out.shape == (a.Q, a.C + 1) and np.isfinite(out).all()
        assert np.isfinite(a.depth(fast)).all()
        np.testing.assert_array_equal(out[:, -1:], a.opacity(fast))
        s = a.step_api(fast)
        assert all(np.isfinite(x).all() for x in s) and not s[1][s[3] == 0].any()
    for cols in (a.C + 1, 1):
        want, absum, tight = a.oracle_grad(cols)
        assert np.isfinite(want).all() and np.isfinite(absum).all() and np.isfinite(tight).all()
        assert np.all(absum >= 0) and np.all(tight >= 0) and np.array_equal(tight == 0, absum == 0)
        assert not want[tight == 0].any()
        # a sum is no larger than the sum of its terms' sizes (with view rotations the reference's second pass takes off
        # `accum` what its first never put on: the oracle prices that too, or three entries of sh4_xf / 0 / far are up to
        # 30 000 times their scale); the colour step's scales: the opacity backward prices its one term its own way
        assert cols == 1 or (np.all(np.abs(want) <= tight * (1 + 1e-6)) and np.all(tight <= absum * (1 + 1e-6)))
        if cols == 1:
            # (from inside the cube a ray's transmittance can underflow within a few samples: few entries, or none, move alpha)
            assert not want[:, :-1].any() and np.count_nonzero(want) > {"ragged": 1000, "far": 400, "inside": -1}[batch]
        else:
            assert np.count_nonzero(want) > (300 if batch == "inside" else 1000)
    want, absum, _ = a.oracle_grad(a.C + 1)
    if batch == "far":
        assert (absum == 0).all(axis=1).sum() > 0.3 * a.M                       # rows nobody saw
    if extreme:                                                             # saturated either way: sigmoid' an exact 0
        L0 = a.lists(0.0)
        seen = np.unique(L0.row)
        assert (want[seen, :-1] == 0).sum() > 0.2 * seen.shape[0] * (a.K - 1)


# oracle.Tree without lobes ------------------------------------------------------------------------------------------------------
def test_oracle_refuses_sg_and_asg_without_lobes():
    """An SG / ASG format reads tree.extra [basis_dim, 4] (ASG: [basis_dim, 11]) in the C++ oracle: a Tree without it,
    or with another number of lobes, used to hand over a null pointer (a segmentation fault in the test process)."""
    a = inputs("sg9", 0, "far")
    bare = O.Tree(a.ot.features, a.data, a.child, offset=a.ot.offset, scaling=a.ot.scaling)
    short = O.Tree(a.ot.features, a.data, a.child, offset=a.ot.offset, scaling=a.ot.scaling, extra=a.lobes.numpy()[:5])
    g = a.grad_out(4)
    for fmt in (O.FORMAT_SG, O.FORMAT_ASG):
        opt = O.make_options(step_size=H.STEP, format=fmt, basis_dim=9)
        for t in (bare, short):
            with pytest.raises(ValueError, match="lobes"):
                O.volume_render(t, *a.rays, opt)
            with pytest.raises(ValueError, match="lobes"):
                O.volume_render_backward(t, *a.rays, opt, g, want_abs="both")
            with pytest.raises(ValueError, match="lobes"):
                O.volume_render_weights(t, *a.rays, opt)
        with pytest.raises(ValueError, match="lobes"):
            O.basis(fmt, 9, a.rays[2])
    # the operators that read no colour take such a tree, and a tree with its lobes renders
    assert O.opacity_render(bare, *a.rays, a.opt).shape == (a.Q, 1)
    assert np.isfinite(O.volume_render(a.ot, *a.rays, a.opt)).all()
    assert O.basis(O.FORMAT_SH, 9, a.rays[2]).shape == (a.Q, 9)
