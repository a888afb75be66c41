"""The per-ray operators agree on what a ray's crossings and samples are.  They all take the shared walk of
csrc/svoxt_device.h (next_crossing / is_sample / walk_crossings / walk_samples), so the agreement is structural; this
file pins it from outside, against the lists of tests/samples_restate.py:

    T_all   the crossings whose data word names a feature row             lists(min_sigma=None)
    T_pos   those of them whose sigma > 0 (a NaN sigma is not)            lists(min_sigma=0)

    ray_samples(min_sigma=None)                                 finds T_all  (the crossing layer: sigma is not read)
    ray_samples(min_sigma=0.0)                                  finds T_pos
    count_forward, sigma_thresh = 1e30: counters[3], valid leaves     T_all  (nothing is composited, no ray stops)
    count_forward, both thresholds 0:   counters[4], composited       T_pos  (given that no ray's transmittance reaches 0)
    volume_render_backward_rows:        ROWGRAD_LAST["T"]             T_pos  (count by svoxt_ray_samples_count, then
                                                                              rowgrad_record_kernel writes as many)

Inputs: the smallest trees of tests/test_adversarial_host.py with N = 2 and with N = 3 (selective refinement, empty
leaves, rows in a random permutation, sigma of 0, -5 and 1e-2 ... 1e4), every 13th row's sigma replaced by NaN, and the
positive sigmas scaled until no ray is opaque; a 16 x 16 image declared as one (walked in 8 x 8 tiles) and 100 rays of the
host file's incoherent batch, undeclared (one full wavefront and a partial one).

The precondition of the composited count -- T > 0 along every ray, or count_fwd_kernel stops the ray at T <= 0 and
counts fewer -- is asserted from the restatement's float32 weights, which have the kernels' bits: alpha = 1 - T_end
stays below 0.99, and T only falls along a ray.  The scale is chosen for exp(-4) at the most opaque ray, 0.018."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from svox_t_amd.renderer import _rays_spec_from_rays
from tests import samples_restate as SR
from tests import test_adversarial_host as H

TREES = [("n2_rgba4", 1), ("n3_sh1", 1)]            # M = 14 875 and 5 073: the smallest of H.IDS for either N
BATCHES = {"image16": (16, 16), "batch100": None}
_BUILT = {}


class Walk:
    """One tree and one ray batch: the oracle's twin, the restatement's two lists and what the GPU side needs."""

    def __init__(self, name, seed, batch):
        a = H.adversarial(name, seed)
        self.a, self.shape = a, BATCHES[batch]
        if self.shape is not None:
            h, w = self.shape
            rays = synth.pinhole_rays(w, h, c2w=synth.camera_pose(radius=3.0, center=H.CENTER))
            self.rays = tuple(np.ascontiguousarray(x.numpy()) for x in rays)
        else:
            self.rays = tuple(np.ascontiguousarray(x[::20]) for x in a.rays)
        self.Q = self.rays[0].shape[0]
        feats = a.features.numpy().copy()
        feats[::13, -1] = np.nan
        unit = O.Tree(feats, a.data, a.child, offset=a.ot.offset, scaling=a.ot.scaling)
        L = SR.lists(unit, self.rays, a.opt, 0.0)
        tau = np.zeros(self.Q)
        np.add.at(tau, L.ray, L.length.astype(np.float64) * feats[L.row, -1])
        pos = feats[:, -1] > 0
        feats[pos, -1] *= np.float32(4.0 / tau.max())
        self.features = feats
        self.ot = O.Tree(feats, a.data, a.child, offset=a.ot.offset, scaling=a.ot.scaling)
        self.all = SR.lists(self.ot, self.rays, a.opt, None)
        self.pos = SR.lists(self.ot, self.rays, a.opt, 0.0)
        self.T_all, self.T_pos = int(self.all.row.shape[0]), int(self.pos.row.shape[0])


def walk(name, seed, batch) -> Walk:
    if (name, seed, batch) not in _BUILT:
        _BUILT[name, seed, batch] = Walk(name, seed, batch)
    return _BUILT[name, seed, batch]


CASES = [(name, seed, batch) for name, seed in TREES for batch in BATCHES]


@pytest.mark.parametrize("name,seed,batch", CASES)
def test_the_inputs_hold_the_precondition(name, seed, batch):
    """No GPU: every kind of sigma is met, the filter drops something, and no ray's transmittance reaches 0."""
    k = walk(name, seed, batch)
    assert k.Q == (256 if batch == "image16" else 100)
    sigma = k.features[k.all.row, -1]
    kinds = [(sigma > 0).sum(), (sigma == 0).sum(), (sigma < 0).sum(), np.isnan(sigma).sum()]
    print(f"{name}/{seed} {batch}: T_all {k.T_all}, T_pos {k.T_pos}, sigma > 0 / == 0 / < 0 / NaN among the crossings {kinds}")
    assert min(kinds) > 10 and k.T_pos == kinds[0] < k.T_all
    assert (k.a.data.reshape(-1)[k.a.child.reshape(-1) == 0] == synth.EMPTY_SENTINEL).sum() > 100      # empty leaves
    w, alpha = SR.weights(k.pos.length, k.features[k.pos.row, -1], k.pos.offsets, torch.float32)
    assert np.isfinite(w.numpy()).all() and 0.5 < float(alpha.max()) < 0.99                         # T_end > 0.01 on every ray


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,batch", CASES)
def test_every_operator_walks_the_same_samples(gpu, name, seed, batch):
    k = walk(name, seed, batch)
    a = k.a
    tree = svox.N3Tree.from_arrays(a.child, a.data, a.parent_depth, torch.from_numpy(k.features), data_format=a.fmt,
                                   radius=list(a.radius), center=list(a.center), device=gpu)
    r = svox.VolumeRenderer(tree, step_size=H.STEP, background_brightness=H.BACKGROUND)
    rays = svox.Rays(*(torch.from_numpy(x).to(gpu) for x in k.rays))
    kw = {} if k.shape is None else dict(image_shape=k.shape)
    # ray_samples: the lists themselves, bit for bit
    for min_sigma, want in ((None, k.all), (0.0, k.pos)):
        s = r.ray_samples(rays, min_sigma=min_sigma, **kw)
        assert len(s) == want.row.shape[0] == int(s.offsets[-1])
        for field in SR.Lists._fields:
            np.testing.assert_array_equal(getattr(s, field).cpu().numpy(), getattr(want, field), err_msg=field)
    # the counters
    spec, rspec = tree._spec(tree.features), _rays_spec_from_rays(rays, k.shape)
    opt = r._get_options()
    assert opt.sigma_thresh == 0 and opt.stop_thresh == 0
    zero = _C.count_forward(spec, rspec, opt).cpu().tolist()
    opt.sigma_thresh = 1e30
    none = _C.count_forward(spec, rspec, opt).cpu().tolist()
    print(f"{name}/{seed} {batch}: counters at thresholds 0 {zero}, at sigma_thresh 1e30 {none}; T_all {k.T_all}, T_pos {k.T_pos}")
    assert none[3] == k.T_all and none[4] == 0
    assert zero[4] == k.T_pos and zero[3] == k.T_all and zero[:3] == none[:3]
    # the deterministic backward's record
    g = synth.grad_output(k.Q, a.C + 1, seed=5).to(gpu)
    grad = _C.volume_render_backward_rows(spec, rspec, r._get_options(), g)
    assert _C._extras.ROWGRAD_LAST["T"] == k.T_pos
    assert torch.isfinite(grad).all() and int((grad[:, -1] != 0).sum()) > 10
