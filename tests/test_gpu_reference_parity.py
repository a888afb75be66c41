"""The HIP kernels against outputs recorded from a host build of the reference's own ray kernels
(tests/golden/reference_*.npz, written by tests/golden/make_reference_golden.py; read here as data only).

Per scene -- SH4, RGBA, SG4; a depth-4 tree of a few hundred rows with zero, negative and huge sigma, 300 rays from inside
and outside the cube -- and per threshold set:
    forward, opacity_render and render_depth have the bits of the oracle with its portable expf (the kernels' pexpf);
    |HIP - reference| <= the fixture's `portable_gap`, with no margin: the gap was measured on the CPU, oracle against
    reference, and the HIP outputs are the oracle's bits;
    the gradient is within tests.util.assert_grads_close of the reference's recorded float32 gradient, on the oracle's
    `tight` scale.
"""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
from tests.test_reference_golden import OUTPUTS, SCENES, scene
from tests.util import assert_grads_close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", SCENES)
def test_kernels_against_the_recorded_reference(gpu, name):
    s = scene(name)
    g = s.g
    extra = None if s.extra is None else torch.from_numpy(s.extra)
    tree = svox.N3Tree.from_arrays(g["child"], g["data"], g["parent_depth"], torch.from_numpy(g["features"]), data_format=s.data_format,
                                   radius=[float(v) for v in g["radius"]], center=[float(v) for v in g["center"]], extra_data=extra,
                                   device=gpu)
    np.testing.assert_array_equal(tree.offset.cpu().numpy(), g["offset"])               # the transform the reference was given
    np.testing.assert_array_equal(tree.invradius.cpu().numpy(), g["scaling"])
    r = svox.VolumeRenderer(tree, step_size=float(g["step_size"]), background_brightness=float(g["background_brightness"]))
    rays = svox.Rays(*(torch.from_numpy(a).to(gpu) for a in s.rays))
    feats = torch.from_numpy(g["features"]).to(gpu)
    for fast in (0, 1):
        want = s.oracle(fast)
        f = feats.clone().requires_grad_(True)
        out = r(f, rays, fast=bool(fast))
        with torch.no_grad():
            got = dict(render=out.detach().cpu().numpy(), opacity=r.opacity_render(f, rays, fast=bool(fast)).cpu().numpy(),
                       depth=r.render_depth(f, rays, fast=bool(fast)).cpu().numpy())
        for k in OUTPUTS:
            np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=f"{name} {k} fast={fast}: oracle bits")
            gap = np.abs(got[k].astype(np.float64) - g[f"{k}_{fast}"].astype(np.float64)).max()
            print(f"{name} {k} fast={fast}: worst |HIP - reference| {gap:.3e}, portable_gap {float(g[f'portable_gap_{k}_{fast}']):.3e}")
            assert gap <= float(g[f"portable_gap_{k}_{fast}"]), (name, k, fast, gap)
        if not fast:
            out.backward(torch.from_numpy(g["grad_output"]).to(gpu))
            _, _, tight = s.oracle_grad()
            grad = f.grad.cpu().numpy()
            err = np.abs(grad.astype(np.float64) - g["grad"].astype(np.float64))
            print(f"{name}: gradient against the reference's, worst err / (1e-5 tight) {(err / (1e-5 * tight + 1e-30)).max():.4f}")
            assert_grads_close(grad, g["grad"], tight, what=f"{name}: gradient against the reference's")
