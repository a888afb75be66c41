"""tests/golden/reference_*.npz -- outputs and gradients recorded from a host build of the reference's own ray kernels
(tests/golden/make_reference_golden.py) -- against the oracle.  Needs neither the reference nor oracle/_ref nor a GPU:
it keeps the chain reference -> oracle -> HIP kernels checkable everywhere.

    the oracle with the C library's expf (which is what the recorded build's `expf` was) returns the recorded
    volume_render, opacity_render and render_depth bit for bit, under both threshold sets;
    with its own portable expf it is off by exactly the recorded `portable_gap` (one float32 ulp below 1, 2^-24, for the
    colours and the opacity; 0 for the depth, which takes no exponential);
    its float64 gradient sum is within tests.util.assert_grads_close of the recorded float32 sequential sum on the
    `tight` scale with the C library's expf, and within the same bound with the portable one.

The bit-for-bit half holds wherever the C library's expf returns what the recording machine's did (glibc's expf is one
table-driven sequence since 2.27); where another library rounds an argument differently, regenerate the fixtures.
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.util import assert_grads_close

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ("sh4", "rgba", "sg4")
OUTPUTS = ("render", "opacity", "depth")
_LOADED = {}


class Scene:
    def __init__(self, name):
        g = np.load(os.path.join(GOLDEN, f"reference_{name}.npz"))
        self.g = {k: g[k] for k in g.files}
        self.name = name
        self.extra = self.g.get("extra")
        self.ot = O.Tree(self.g["features"], self.g["data"], self.g["child"], offset=self.g["offset"], scaling=self.g["scaling"],
                         extra=self.extra)
        self.rays = (self.g["origins"], self.g["dirs"], self.g["vdirs"])
        self.data_format = str(self.g["data_format"])

    def opt(self, fast):
        th = float(self.g["thresholds"][fast])
        return O.make_options(step_size=float(self.g["step_size"]), background_brightness=float(self.g["background_brightness"]),
                              format=int(self.g["format"]), basis_dim=int(self.g["basis_dim"]), sigma_thresh=th, stop_thresh=th)

    def oracle(self, fast):
        """{render, opacity, depth} of the oracle under its current expf."""
        opt = self.opt(fast)
        return dict(render=O.volume_render(self.ot, *self.rays, opt), opacity=O.opacity_render(self.ot, *self.rays, opt),
                    depth=O.render_depth(self.ot, *self.rays, opt))

    def oracle_grad(self):
        """(grad, abs_sum, tight) float64 of the oracle for the recorded upstream gradient."""
        return O.volume_render_backward(self.ot, *self.rays, self.opt(0), self.g["grad_output"], want_abs="both")


def scene(name) -> Scene:
    if name not in _LOADED:
        _LOADED[name] = Scene(name)
    return _LOADED[name]


@pytest.mark.parametrize("name", SCENES)
def test_the_fixtures_are_small_scenes_that_render(name):
    s = scene(name)
    g = s.g
    assert os.path.getsize(os.path.join(GOLDEN, f"reference_{name}.npz")) <= 177295          # the largest fixture before these
    assert 200 <= g["origins"].shape[0] <= 400 and 300 <= g["features"].shape[0] <= 2000 and g["parent_depth"][:, 1].max() >= 3
    assert np.count_nonzero(g["opacity_0"]) > 150 and (g["opacity_0"] == 0).sum() > 20 and np.count_nonzero(g["grad"]) > 1000
    sigma = g["features"][:, -1]
    assert (sigma == 0).any() and (sigma < 0).any() and (sigma > 1e3).any()
    assert (g["extra"].shape == (4, 4)) if name == "sg4" else ("extra" not in g)


@pytest.mark.parametrize("name", SCENES)
def test_oracle_with_libm_expf_is_the_recorded_reference(name):
    s = scene(name)
    O.use_libm_exp(True)
    try:
        got = {fast: s.oracle(fast) for fast in (0, 1)}
    finally:
        O.use_libm_exp(False)
    for fast in (0, 1):
        for k in OUTPUTS:
            want = s.g[f"{k}_{fast}"]
            assert got[fast][k].dtype == want.dtype == np.float32
            np.testing.assert_array_equal(got[fast][k].view(np.uint32), want.view(np.uint32), err_msg=f"{name} {k} fast={fast}")


@pytest.mark.parametrize("name", SCENES)
def test_oracle_with_portable_expf_reproduces_the_gap(name):
    s = scene(name)
    for fast in (0, 1):
        got = s.oracle(fast)
        for k in OUTPUTS:
            gap = np.abs(got[k].astype(np.float64) - s.g[f"{k}_{fast}"].astype(np.float64)).max()
            assert gap == float(s.g[f"portable_gap_{k}_{fast}"]), (name, k, fast, gap)
            assert gap <= 2.0 ** -24                   # outputs in [0, 1] up to the background: one ulp below 1
    assert float(s.g["portable_gap_depth_0"]) == 0.0


@pytest.mark.parametrize("name", SCENES)
def test_oracle_gradient_against_the_recorded_gradient(name):
    """With the C library's expf the oracle's float64 sum and the recorded float32 sequential sum differ by the order and
    width of the additions alone.  With the portable expf -- the comparison tests/test_gpu_reference_parity.py makes for
    the kernels -- single contributions move by an ulp of the exponential, and where a ray's transmittance has reached
    the denormals the portable expf returns 0 (below -87) while the recorded build went on adding values below 1e-40:
    those entries are inside the 1e-30 floor, but non-zero where the oracle has no contribution, so the bound alone is
    asserted there."""
    s = scene(name)
    got = s.g["grad"]
    O.use_libm_exp(True)
    try:
        want, _, tight = s.oracle_grad()
    finally:
        O.use_libm_exp(False)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name}: recorded gradient against the oracle (libm expf), worst err / (1e-5 tight) {(err / (1e-5 * tight + 1e-30)).max():.4f}")
    assert_grads_close(got, want, tight, what=f"{name}: recorded gradient, libm expf")
    want, _, tight = s.oracle_grad()
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name}: recorded gradient against the oracle (portable expf), worst err / (1e-5 tight) {(err / (1e-5 * tight + 1e-30)).max():.4f}")
    assert np.all(err <= 1e-5 * tight + 1e-30)
    assert np.abs(got[tight == 0]).max(initial=0.0) < 1e-40
