"""Hostile trees, rays and cameras through every route of the colour render step (VolumeRenderer.forward / render_persp /
opacity_render / render_depth, their backwards, and the svoxt_step_* entry points): the irregular trees of
tests/test_gpu_random_stress.py with one payload per kernel family, and three batches a tree -- incoherent rays as they
come, an image from inside the cube, an image most of whose tiles miss.  The inputs, their references and what those
guarantee are tests/test_route_matrix_host.py's.  One test is one (payload, seed, batch): it uploads the tree once and
walks the payload's routes over the same device tensors, each route at thresholds 0 and `fast`, held to the contract
every route of this project has:

    forward, render_depth, opacity_render    the oracle's bits;
    gradient                                 |got - want| <= 1e-5 tight, exactly 0 where the oracle's abs_sum is 0, finite;
    the route taken                          _C.LAST_ROUTE names the kernels the switches were meant to select (KERNELS
                                             below restates the intent per family); for N = 3 no per-tile kernel.

A test gathers what its routes got wrong and fails once, with all of it; a launch error ends it at once and every later
test of the file fails without touching the GPU.  Every route prints its worst |got - want| / (1e-5 tight) with the
backward's kernel; DESIGN.md 5 keeps the worst per family.

On the ragged batch -- no image, too small to be sorted by itself: the per-ray backwards are what its default takes --
the forced routes run once more on top of BWD_GATHER = 2, which sends tiles of 64 incoherent rays through the per-tile
kernels, and the list capacities also on top of BWD_GATHER = 0 (tails of the per-ray list walk).

Pairs the routing does not admit, and why:
    sort_rays on inside / far            a declared image is walked in tiles as it stands (_wants_sort);
    EXP_TABLE on other than rgba8 / rgba32 / rgba6     the table exists for RGBA-style rows of 8 / 16 / 32 floats (rgba6: as 8);
    PAD_PAYLOADS, GROUP_PAYLOADS, BWD_XF_FUSED     on their own payloads (sh4_two and rgba6; sh4_four; sh4_xf);
    render_persp on sh4_xf               camera batches take no transformation_matrices;
    render_persp on ragged               not an image;
    opacity_render, render_depth         under the switches their routes read (SIGMA_ONLY below); not on sh4_xf, whose
                                         sigma-only operators take no transformation_matrices and are sh9's;
    the step API                         sh9, rgba32, rgba6 and n3_sh1, as rays and (image batches) as a declared image;
    the forward's label under FWD_SPLIT on sg9     a recording SG forward has one form (march + tile shade) whatever the
                                         switch says, and LAST_ROUTE does not tell: its backward's label is asserted;
    ACCEL_BRICKS with ACCEL_LOG2 = 0     no grid, no layout: run once; on n3_sh1 no grid exists at any setting (N = 3);
    BWD_LIST_SAMPLES 4 and 12            give lists of 8 and 16 slots (whole lines of 8 records): both overflow on every
                                         batch but sh16 / inside, whose longest ray has 14 samples with sigma > 0."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import test_route_matrix_host as H
from tests.test_adversarial_host import BACKGROUND, STEP, worst_ratio
from tests.test_gpu_step_api import _run as step_api_run
from tests.util import assert_grads_close

pytestmark = pytest.mark.gpu

FAMILY = {"sh9": "three", "rgba4": "three", "sh4_two": "three", "sh4_four": "three", "rgba8": "wide", "rgba32": "wide",
          "rgba6": "wide", "sh16": "wide_sh", "sg9": "sg", "sh4_xf": "xf", "n3_sh1": "n3"}
ROLES, XF_ROLES = "fwd_roles_kernel (march + shade_tile in one launch)", "fwd_roles_kernel<XF>"
TILE2, CHAN, ONE = "march_rec_kernel + shade_tile_kernel", "march_rec_kernel + shade_chan_kernel", "render_fwd_kernel"
FUSED, FUSED_XF, WIDE = "grad_fused_kernel<EXACT>", "grad_fused_kernel<EXACT, XF>", "grad_wide_kernel"
MERGE, ONEPASS = "render_bwd_kernel<GATHER> + grad_merge_kernel", "render_bwd_kernel<ONEPASS>"
REPLAY, MARCH = "render_bwd_kernel<REPLAY>", "render_bwd_kernel (marches"
PER_TILE = ("fwd_roles_kernel", "grad_fused_kernel", "grad_wide_kernel", "grad_merge_kernel")
STEP_API = ("sh9", "rgba32", "rgba6", "n3_sh1")
# switches under which opacity_render (+ backward) and render_depth are run too: the ones their routes read
SIGMA_ONLY = {"AUTO_PLAN", "BWD_LIST_SAMPLES", "LIST_POOL", "_dry", "ACCEL_LOG2", "ACCEL_BRICKS", "BWD_GATHER"}
_FAULT = []


def KERNELS(fam, coherent, sw, grad=True):
    """(forward, backward) LAST_ROUTE must start with -- what each switch is MEANT to select, per payload family; None: not
    asserted.  coherent: a declared image or sort_rays."""
    gather, fused, terms = sw.get("BWD_GATHER", 1), sw.get("BWD_FUSED", True), sw.get("BWD_TERMS", True)
    split = sw.get("FWD_SPLIT", "")
    lists = grad and sw.get("AUTO_PLAN", True) and sw.get("BWD_LIST_SAMPLES", 96) > 0
    one_launch = sw.get("FWD_OVERLAP", True) and sw.get("LIST_POOL", True) and sw.get("SIGMA_MASK", True)
    tile = fam != "n3" and (gather == 2 or (gather == 1 and coherent))
    handover = lists and fused and terms and gather > 0          # the forward leaves the exact per-tile backward its terms
    if fam == "wide":
        fwd = ONE if split == "0" else CHAN
        bwd = (WIDE if tile and terms and fused else ONEPASS if terms else REPLAY) if lists else MARCH
    elif fam == "sg":
        rec = handover and tile                                   # SG lists serve the exact per-tile backward only
        fwd = None if split else (ROLES if one_launch and sw.get("ACCEL_LOG2") != 0 else TILE2) if rec else ONE
        bwd = FUSED if rec else MARCH
    elif fam == "xf":
        if lists and split == "" and sw.get("FWD_OVERLAP", True) and sw.get("LIST_POOL", True) and sw.get("BWD_XF_FUSED", True):
            fwd = XF_ROLES
        else:
            fwd = TILE2 if split == "1" else ONE
        bwd = ((FUSED_XF if fused and sw.get("BWD_XF_FUSED", True) else MERGE) if tile else REPLAY) if lists else MARCH
    else:
        two = TILE2 if fam == "n3" or not one_launch else ROLES
        fwd = two if (split == "1" or (handover and split == "")) else ONE
        if fam == "wide_sh":
            bwd = (FUSED if tile and handover else REPLAY) if lists else MARCH
        else:
            bwd = ((FUSED if fused else MERGE) if tile else REPLAY) if lists else MARCH
    return fwd, bwd


class OnGpu:
    """An input of the host file on the GPU: tree, renderer, rays, feature table and upstream gradients, uploaded once."""

    def __init__(self, a, gpu):
        self.a, self.gpu = a, gpu
        self.r = svox.VolumeRenderer(a.tree(gpu), step_size=STEP, background_brightness=BACKGROUND)
        self.rays = a.rays_on(gpu)
        self.f = a.features.to(gpu)
        self.xf = None if a.xf is None else a.xf.to(gpu)
        self.g = torch.from_numpy(a.grad_out(a.C + 1)).to(gpu)
        self.g1 = torch.from_numpy(a.grad_out(1)).to(gpu)
        self.pose = None if a.pose is None else torch.from_numpy(a.pose).to(gpu)

    def forward(self, f, fast, persp=False, **kw):
        a = self.a
        if persp:
            return self.r.render_persp(f, self.pose, width=a.image[1], height=a.image[0], fx=a.fx, fast=fast).view(a.Q, -1)
        return self.r(f, self.rays, transformation_matrices=self.xf, fast=fast, image_shape=a.image, **kw)

    def step(self, fast, backwards=1, persp=False, **kw):
        """(out, [gradient of each backward], forward's label, [backward's label])."""
        f = self.f.detach().clone().requires_grad_(True)
        out = self.forward(f, fast, persp, **kw)
        fwd = _C.LAST_ROUTE["forward"]
        grads, bwds = [], []
        for i in range(backwards):
            grads.append(torch.autograd.grad(out, f, self.g, retain_graph=i + 1 < backwards)[0].cpu().numpy())
            bwds.append(_C.LAST_ROUTE["backward"])
        return out.detach().cpu().numpy(), grads, fwd, bwds

    def sigma_only(self, fast, **kw):
        """(opacity, its gradient, depth)."""
        f = self.f.detach().clone().requires_grad_(True)
        out = self.r.opacity_render(f, self.rays, fast=fast, image_shape=self.a.image, **kw)
        grad = torch.autograd.grad(out, f, self.g1)[0].cpu().numpy()
        with torch.no_grad():
            depth = self.r.render_depth(self.f, self.rays, fast=fast, image_shape=self.a.image)
        return out.detach().cpu().numpy(), grad, depth.cpu().numpy()


def routes(a):
    """[(name, switches, keywords of forward)] of a payload and batch.  "_dry": a pool of 32 blocks, as
    tests/test_gpu_render_parity.py::test_sample_list_pool_runs_dry_or_is_dense forces it."""
    fam, image = FAMILY[a.payload], a.image is not None
    forced = [{"BWD_FUSED": False}, {"BWD_TERMS": False}, {"AUTO_PLAN": False}, {"BWD_LIST_SAMPLES": 0}, {"BWD_LIST_SAMPLES": 4},
              {"BWD_LIST_SAMPLES": 12}, {"LIST_POOL": False}, {"_dry": True}, {"FWD_SPLIT": "0"}, {"FWD_SPLIT": "1"},
              {"FWD_OVERLAP": False}, {"SIGMA_MASK": False}]
    if fam == "wide":
        forced.append({"EXP_TABLE": False})
    forced += [{"GRAD_SCRATCH": False}, {"GRAD_SCRATCH": True}, {"GRAD_SCRATCH": True, "_again": True}]
    if a.payload in ("sh4_two", "rgba6"):
        forced.append({"PAD_PAYLOADS": False})
    if a.payload == "sh4_four":
        forced.append({"GROUP_PAYLOADS": False})
    if fam == "xf":
        forced.append({"BWD_XF_FUSED": False})
    forced += [{"ACCEL_LOG2": 0}] + [{"ACCEL_LOG2": g, "ACCEL_BRICKS": b} for g in (2, 5, 7) for b in (True, False)]
    name = lambda sw: " ".join("pool of 32 blocks" if k == "_dry" else f"{k}={v}" for k, v in sw.items() if k != "_again") \
        + (" again" if "_again" in sw else "")                                                                         # noqa: E731
    out = [("default", {}, {}), ("BWD_GATHER=0", {"BWD_GATHER": 0}, {}), ("BWD_GATHER=2", {"BWD_GATHER": 2}, {})]
    if not image:
        out.append(("sort_rays", {}, {"sort_rays": True}))
    out += [(name(sw), sw, {}) for sw in forced]
    if not image:
        out += [("BWD_GATHER=2 " + name(sw), dict(sw, BWD_GATHER=2), {}) for sw in forced if "AUTO_PLAN" not in sw]
        out += [("BWD_GATHER=0 " + name(sw), dict(sw, BWD_GATHER=0), {}) for sw in ({"BWD_LIST_SAMPLES": 4}, {"BWD_LIST_SAMPLES": 12})]
    return out


class Walk:
    """The checks of one test: what a route got wrong is noted, not raised; a launch error is raised and remembered."""

    def __init__(self, g, monkeypatch):
        self.g, self.a, self.mp = g, g.a, monkeypatch
        self.problems = []
        self.label = f"{g.a.payload}/{g.a.seed}/{g.a.batch}"

    def note(self, route, fn):
        try:
            fn()
        except AssertionError as e:
            self.problems.append(f"{self.label} {route}: {str(e).strip().splitlines()[0][:300] if str(e).strip() else 'assertion failed'}")

    def equal(self, route, what, got, want):
        self.note(f"{route} {what}", lambda: np.testing.assert_array_equal(got, want))

    def grad(self, route, kernel, got, cols=None):
        a = self.a
        want, absum, tight = a.oracle_grad(a.C + 1 if cols is None else cols)
        ratio = worst_ratio(got, want, 1e-5 * tight)
        print(f"{self.label} {route} [{kernel.split(' (')[0]}]: worst |got - want| / (1e-5 scale) = {ratio:.3f}")

        def check():
            assert got.shape == (a.M, a.K) and np.isfinite(got).all(), "gradient not finite"
            assert_grads_close(got, want, tight, what="gradient")
            assert np.all(got[absum == 0] == 0), "non-zero gradient where the oracle's abs_sum is 0"
        self.note(route, check)

    def names(self, route, fwd, bwd, want):
        def check():
            for got, w, side in ((fwd, want[0], "forward"), (bwd, want[1], "backward")):
                if got is not None and w is not None:
                    assert got.startswith(w), f"{side} took {got!r}, meant {w!r}"
                if got is not None and FAMILY[self.a.payload] == "n3":
                    assert not any(k in got for k in PER_TILE), f"{side} of an N = 3 tree named a per-tile kernel: {got!r}"
        self.note(route, check)

    def switches(self, mp, sw):
        for k, v in sw.items():
            if k == "_dry":
                mp.setattr(_C, "_pool_blocks_for", lambda tiles, S, kind="record": 32)
            elif k != "_again":
                mp.setattr(_C, k, v)

    def route(self, name, sw, kw):
        a, g = self.a, self.g
        fam = FAMILY[a.payload]
        coherent = a.image is not None or bool(kw.get("sort_rays"))
        with self.mp.context() as mp:
            self.switches(mp, sw)
            for fast in (False, True):
                tag = name + (" fast" if fast else "")
                second = name == "default"                     # a second backward over the same forward: the lists were consumed
                out, grads, fwd, bwds = g.step(fast, backwards=2 if second else 1, **kw)
                self.equal(tag, "forward", out, a.render(fast))
                self.grad(tag, bwds[0], grads[0])
                if second:
                    self.grad(tag + ", second backward", bwds[1], grads[1])
                with torch.no_grad():
                    self.equal(tag, "forward under no_grad", g.forward(g.f, fast, **kw).cpu().numpy(), a.render(fast))
                if not fast:                                   # (the labels of the forward depend on the stop threshold: asserted at 0)
                    generic = sw.get("PAD_PAYLOADS") is False or sw.get("GROUP_PAYLOADS") is False
                    if generic:
                        self.note(tag, lambda: self._generic(fwd, bwds[0]))
                    else:
                        self.names(tag, fwd, bwds[0], KERNELS(fam, coherent, sw))
                        self.names(tag + ", no_grad", _C.LAST_ROUTE["forward"], None, KERNELS(fam, coherent, sw, grad=False))
                        self.note(tag, lambda: self._not_generic(fwd))
                    if second:
                        self.names(tag + ", second backward", None, bwds[1], (None, MARCH))
                    if bwds[0].startswith(WIDE):
                        table = sw.get("EXP_TABLE", True) and sw.get("SIGMA_MASK", True) and sw.get("FWD_SPLIT", "") != "0"
                        self.note(tag, lambda: self._table(bwds[0], table))
                if set(sw) <= SIGMA_ONLY and self.a.xf is None:
                    skw = {k: v for k, v in kw.items() if k == "sort_rays"}
                    op, og, depth = g.sigma_only(fast, **skw)
                    self.equal(tag, "opacity_render", op, a.opacity(fast))
                    self.equal(tag, "render_depth", depth, a.depth(fast))
                    self.grad(tag + ", opacity_render", "opacity_render_backward", og, cols=1)

    @staticmethod
    def _generic(fwd, bwd):
        assert "generic" in fwd or "marches" in bwd, f"no generic kernel with the payload's own switch off: {fwd!r}, {bwd!r}"

    @staticmethod
    def _not_generic(fwd):
        assert "generic" not in fwd, f"the forward fell back to the generic kernel: {fwd!r}"

    @staticmethod
    def _table(bwd, table):
        assert ("forward's table" in bwd) == bool(table), f"exponentials table {'not ' if table else ''}used: {bwd!r}"

    def no_grad_lists(self):
        """Scratch lists of 4 (8) records for a forward nobody differentiates."""
        a, g = self.a, self.g
        with self.mp.context() as mp:
            mp.setattr(_C, "FWD_LIST_SAMPLES", 4)
            for fast in (False, True):
                with torch.no_grad():
                    out = g.forward(g.f, fast).cpu().numpy()
                self.equal(f"FWD_LIST_SAMPLES=4 no_grad{' fast' if fast else ''}", "forward", out, a.render(fast))
                if not fast:
                    self.names("FWD_LIST_SAMPLES=4 no_grad", _C.LAST_ROUTE["forward"], None,
                               KERNELS(FAMILY[a.payload], a.image is not None, {}, grad=False))

    def persp(self):
        """The same image with the rays formed in the kernels (render_persp: _C.volume_render_image)."""
        a, g = self.a, self.g
        for fast in (False, True):
            tag = "render_persp" + (" fast" if fast else "")
            out, grads, fwd, bwds = g.step(fast, persp=True)
            self.equal(tag, "forward", out, a.render(fast))
            self.grad(tag, bwds[0], grads[0])
            if not fast:
                self.names(tag, fwd, bwds[0], KERNELS(FAMILY[a.payload], True, {}))

    def step_api(self):
        a, g = self.a, self.g
        for image in ((False, True) if a.image is not None else (False,)):
            for fast in (False, True):
                for pool in ((0, 32) if not fast else (0,)):
                    tag = f"step API image={image}{' fast' if fast else ''}{' pool of 32 blocks' if pool else ''}"
                    th = 1e-2 if fast else 0.0
                    out, grad, _, _, step = step_api_run(a, g.gpu, image, (th, th), pool)
                    want_out, want, absum, tight = a.step_api(fast)
                    self.equal(tag, "forward", out, want_out)
                    ratio = worst_ratio(grad, want, 1e-5 * tight)
                    print(f"{self.label} {tag} [svoxt_step_backward]: worst |got - want| / (1e-5 scale) = {ratio:.3f}")
                    self.note(tag, lambda: (assert_grads_close(grad, want, tight), _zero(grad, absum)))
                    self.note(tag, lambda: _records(step, a.payload))


def _zero(grad, absum):
    assert np.isfinite(grad).all() and np.all(grad[absum == 0] == 0), "non-zero gradient where the oracle's abs_sum is 0"


def _records(step, payload):
    assert bool(step.records), "the step recorded no lists"
    assert (step.pad_K > 0) == (payload == "rgba6"), f"pad_K {step.pad_K}"


@pytest.mark.parametrize("payload,seed,batch", H.IDS)
def test_every_route(gpu, payload, seed, batch, monkeypatch):
    if _FAULT:
        pytest.fail(f"not run: {_FAULT[0]} raised a launch error earlier in this file")
    a = H.inputs(payload, seed, batch)
    try:
        w = Walk(OnGpu(a, gpu), monkeypatch)
        for name, sw, kw in routes(a):           # the default first: a fault then points at one switch
            w.route(name, sw, kw)
        w.no_grad_lists()
        if a.image is not None and a.xf is None:
            w.persp()
        if payload in STEP_API:
            w.step_api()
        torch.cuda.synchronize()
    except RuntimeError:
        _FAULT.append(f"{payload}/{seed}/{batch}")
        raise
    assert not w.problems, f"{len(w.problems)} problems:\n" + "\n".join(w.problems)

