"""The per-sample interface without a GPU: the C ABI's argument checks, the Python layer's, and the anchors that tie the
restatement (tests/samples_restate.py) to the C++ oracle and to the depth moments' restatement."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import depth_restate as D
from tests import samples_restate as R
from tests.util import Case

NAMES = ("svoxt_ray_samples_workspace_bytes", "svoxt_ray_samples_count", "svoxt_ray_samples_emit", "svoxt_sample_weights_fwd",
         "svoxt_sample_weights_bwd", "svoxt_sample_accumulate_fwd", "svoxt_sample_accumulate_bwd")


@pytest.fixture(scope="module")
def case():
    return Case(depth=5, K=4, data_format="RGBA", width=48, height=48)


def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    wb = _C._lib.svoxt_ray_samples_workspace_bytes
    assert wb(0) == 0 and wb(-1) == -1 and wb(1 << 31) == -1
    assert wb(1) > 0 and wb(1) % 256 == 0 and wb(100000) >= 2 * 4 * 100000 + 8


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

    # ray_samples: the tree / rays / options, min_sigma, offsets, the workspace, the outputs
    count = lambda *a: lib.svoxt_ray_samples_count(*a)
    emit = lambda *a: lib.svoxt_ray_samples_emit(*a)
    for a in ((None, Rr, Op), (T, None, Op), (T, Rr, None)):
        assert count(*a, None, p, p, 1 << 20, None) == 1 and b"svoxt_ray_samples_count" in err() and b"NULL" in err()
        assert emit(*a, None, p, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit" in err() and b"NULL" in err()
    assert count(T, Rr, Op, nan, p, p, 1 << 20, None) == 1 and b"svoxt_ray_samples_count: min_sigma is NaN" in err()
    assert emit(T, Rr, Op, nan, p, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit: min_sigma is NaN" in err()
    assert count(T, Rr, Op, None, None, p, 1 << 20, None) == 1 and b"svoxt_ray_samples_count: offsets is NULL" in err()
    assert emit(T, Rr, Op, None, None, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit: offsets is NULL" in err()
    assert count(T, Rr, Op, None, odd4, p, 1 << 20, None) == 1 and b"svoxt_ray_samples_count: offsets is not 8-byte aligned" in err()
    assert emit(T, Rr, Op, None, odd4, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit: offsets is not 8-byte aligned" in err()
    many = _C._CRays(Q=1 << 31, origins=p, dirs=p, vdirs=p)
    assert count(T, ctypes.byref(many), Op, None, p, p, 1 << 40, None) == 1 and b"svoxt_ray_samples_count: too many rays" in err()
    assert emit(T, ctypes.byref(many), Op, None, p, p, p, p, p, None) == 1 and b"svoxt_ray_samples_emit: too many rays" in err()
    need = lib.svoxt_ray_samples_workspace_bytes(64)
    assert count(T, Rr, Op, None, p, None, need, None) == 1 and b"svoxt_ray_samples_count: workspace is NULL" in err()
    assert count(T, Rr, Op, None, p, odd4, need, None) == 1 and b"svoxt_ray_samples_count: workspace is not 8-byte aligned" in err()
    assert count(T, Rr, Op, None, p, p, need - 1, None) == 1 and b"svoxt_ray_samples_count: workspace smaller" in err()
    for outs in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert emit(T, Rr, Op, None, p, *outs, None) == 1 and b"svoxt_ray_samples_emit: row / ray / depth / length is NULL" in err()
    for outs in ((odd1, p, p, p), (p, p, p, odd1)):
        assert emit(T, Rr, Op, None, p, *outs, None) == 1 and b"svoxt_ray_samples_emit: row / ray / depth / length is not 4-byte" in err()

    # the per-sample primitives: extents, NULLs, alignment
    wf, wbk = lib.svoxt_sample_weights_fwd, lib.svoxt_sample_weights_bwd
    af, ab = lib.svoxt_sample_accumulate_fwd, lib.svoxt_sample_accumulate_bwd
    for Q, Tn in ((-1, 4), (1 << 31, 4), (4, -1), (4, 1 << 31)):
        assert wf(p, Q, Tn, p, p, p, p, None) == 1 and b"svoxt_sample_weights_fwd: " in err() and b"must be in [0, 2^31)" in err()
        assert wbk(p, Q, Tn, p, p, p, p, p, None) == 1 and b"svoxt_sample_weights_bwd: " in err()
        assert af(p, Q, Tn, p, p, 1, p, None) == 1 and b"svoxt_sample_accumulate_fwd: " in err()
        assert ab(p, Q, Tn, p, p, 1, p, p, p, None) == 1 and b"svoxt_sample_accumulate_bwd: " in err()
    assert wf(None, 4, 4, p, p, p, p, None) == 1 and b"svoxt_sample_weights_fwd: offsets / alpha is NULL" in err()
    assert wf(p, 4, 4, p, p, p, None, None) == 1 and b"svoxt_sample_weights_fwd: offsets / alpha is NULL" in err()
    for a in ((None, p, p), (p, None, p), (p, p, None)):
        assert wf(p, 4, 4, *a, p, None) == 1 and b"svoxt_sample_weights_fwd: length / sigma / w is NULL" in err()
    for a in ((odd4, p, p, p, p), (p, odd1, p, p, p), (p, p, odd1, p, p), (p, p, p, odd1, p), (p, p, p, p, odd1)):
        assert wf(a[0], 4, 4, *a[1:], None) == 1 and b"svoxt_sample_weights_fwd: a misaligned argument" in err()
    assert wbk(None, 4, 4, p, p, p, p, p, None) == 1 and b"svoxt_sample_weights_bwd: offsets is NULL" in err()
    for a in ((None, p, p), (p, None, p), (p, p, None)):
        assert wbk(p, 4, 4, a[0], a[1], p, p, a[2], None) == 1 and b"svoxt_sample_weights_bwd: length / sigma / grad_sigma is NULL" in err()
    for a in ((odd4, p, p, p, p, p), (p, odd1, p, p, p, p), (p, p, p, odd1, p, p), (p, p, p, p, odd1, p), (p, p, p, p, p, odd1)):
        assert wbk(a[0], 4, 4, *a[1:], None) == 1 and b"svoxt_sample_weights_bwd: a misaligned argument" in err()
    for C in (0, -3):
        assert af(p, 4, 4, p, p, C, p, None) == 1 and b"svoxt_sample_accumulate_fwd: C must be >= 1" in err()
        assert ab(p, 4, 4, p, p, C, p, p, p, None) == 1 and b"svoxt_sample_accumulate_bwd: C must be >= 1" in err()
    assert af(p, 4, 4, p, None, 3, p, None) == 1 and b"svoxt_sample_accumulate_fwd: values is NULL" in err()
    assert ab(p, 4, 4, p, None, 3, p, p, None, None) == 1 and b"svoxt_sample_accumulate_bwd: values is NULL" in err()
    assert ab(p, 4, 4, p, None, 1, p, p, p, None) == 1 and b"svoxt_sample_accumulate_bwd: values is NULL" in err()
    assert af(None, 4, 4, p, p, 1, p, None) == 1 and b"svoxt_sample_accumulate_fwd: offsets / out is NULL" in err()
    assert af(p, 4, 4, p, p, 1, None, None) == 1 and b"svoxt_sample_accumulate_fwd: offsets / out is NULL" in err()
    assert af(p, 4, 4, None, p, 1, p, None) == 1 and b"svoxt_sample_accumulate_fwd: w is NULL" in err()
    for a in ((odd4, p, p, p), (p, odd1, p, p), (p, p, odd1, p), (p, p, p, odd1)):
        assert af(a[0], 4, 4, a[1], a[2], 1, a[3], None) == 1 and b"svoxt_sample_accumulate_fwd: a misaligned argument" in err()
    assert ab(None, 4, 4, p, p, 1, p, p, p, None) == 1 and b"svoxt_sample_accumulate_bwd: ray / grad_out is NULL" in err()
    assert ab(p, 4, 4, p, p, 1, None, p, p, None) == 1 and b"svoxt_sample_accumulate_bwd: ray / grad_out is NULL" in err()
    assert ab(p, 4, 4, None, p, 1, p, p, p, None) == 1 and b"svoxt_sample_accumulate_bwd: w is NULL" in err()
    for a in ((odd1, p, p, p, p, p), (p, odd1, p, p, p, p), (p, p, odd1, p, p, p), (p, p, p, odd1, p, p), (p, p, p, p, odd1, p),
              (p, p, p, p, p, odd1)):
        assert ab(a[0], 4, 4, a[1], a[2], 1, a[3], a[4], a[5], None) == 1 and b"svoxt_sample_accumulate_bwd: a misaligned argument" in err()

    # an empty batch is a valid no-op
    r0 = _C._CRays(Q=0)
    assert count(T, ctypes.byref(r0), Op, None, None, None, 0, None) == 0
    assert emit(T, ctypes.byref(r0), Op, None, None, None, None, None, None, None) == 0
    assert wf(None, 0, 0, None, None, None, None, None) == 0
    assert wbk(None, 0, 0, None, None, None, None, None, None) == 0
    assert af(None, 0, 0, None, None, 1, None, None) == 0
    assert ab(None, 0, 0, None, None, 1, None, None, None, None) == 0


def cpu_samples(T=6, Q=3):
    off = torch.tensor([0, 2, 2, T], dtype=torch.int64)[:Q + 1]
    return svox.RaySamples(off, torch.zeros(T, dtype=torch.int32), torch.zeros(T, dtype=torch.int32), torch.zeros(T), torch.ones(T))


def test_python_layer_checks_device_shapes_and_dtypes():
    tree = svox.N3Tree(N=2, data_dim=4, init_reserve=4)
    r = svox.VolumeRenderer(tree)
    rays = svox.Rays(torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        r.ray_samples(rays)
    with pytest.raises(RuntimeError, match="GPU"):
        r.ray_samples(rays, min_sigma=0.0)
    s = cpu_samples()
    assert s.Q == 3 and len(s) == 6 and s.counts.tolist() == [2, 0, 4]
    with pytest.raises(RuntimeError, match="GPU"):
        svox.sample_weights(s, torch.ones(6))
    with pytest.raises(RuntimeError, match="GPU"):
        svox.accumulate(s, torch.ones(6), torch.ones(6, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        svox.accumulate(s, torch.ones(6))
    with pytest.raises(RuntimeError, match="GPU"):
        svox.composite(s, torch.ones(6), torch.ones(6, 2))
    for sigma in (torch.ones(5), torch.ones(6, 1), torch.ones(6, dtype=torch.float64), torch.ones(6, dtype=torch.int32), None):
        with pytest.raises(RuntimeError, match=r"sigma must be float32 \[T\]"):
            svox.sample_weights(s, sigma)
    for w in (torch.ones(7), torch.ones(6, 1), torch.ones(6, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match=r"w must be float32 \[T\]"):
            svox.accumulate(s, w)
    for v in (torch.ones(6), torch.ones(5, 3), torch.ones(6, 3, 1), torch.ones(6, 0), torch.ones(6, 3, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match=r"values must be float32 \[T, C\]"):
            svox.accumulate(s, torch.ones(6), v)
    with pytest.raises(RuntimeError, match="samples must be a RaySamples|one entry per sample"):
        svox.sample_weights((s.offsets,), torch.ones(6))
    with pytest.raises(RuntimeError, match=r"row must be int32 \[T\]"):
        svox.RaySamples(s.offsets, s.ray, s.row.long(), s.depth, s.length)
    with pytest.raises(RuntimeError, match=r"offsets must be int64"):
        svox.RaySamples(s.offsets.int(), s.ray, s.row, s.depth, s.length)
    spec, rspec, opt = tree._spec(tree.features), svox.renderer._rays_spec_from_rays(rays), r._get_options()
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.ray_samples(spec, rspec, opt)
    with pytest.raises(RuntimeError, match="min_sigma is NaN"):
        _C.ray_samples(spec, rspec, opt, float("nan"))


# ------------------------------------------------------------------------------------------ anchors of the restatement
@pytest.fixture(scope="module")
def built(case):
    ot, rays, opt = case.oracle_tree(), case.rays_np(), case.oracle_opts()
    return ot, rays, opt, R.lists(ot, rays, opt), R.lists(ot, rays, opt, min_sigma=0.0)


def test_lists_are_well_formed(case, built):
    ot, rays, opt, every, pos = built
    for L in (every, pos):
        T = L.row.shape[0]
        assert L.offsets[0] == 0 and L.offsets[-1] == T and np.all(np.diff(L.offsets) >= 0) and L.offsets.shape == (case.Q + 1,)
        assert np.array_equal(L.ray, np.repeat(np.arange(case.Q), np.diff(L.offsets)).astype(np.int32))
        assert L.row.min() >= 0 and L.row.max() < ot.M and np.all(L.length > 0)
        inside = L.ray[1:] == L.ray[:-1]
        assert np.all(L.depth[1:][inside] > L.depth[:-1][inside])                     # march order within a ray
    assert np.all(ot.features[pos.row, -1] > 0) and 1000 < pos.row.shape[0] <= every.row.shape[0]


@pytest.mark.parametrize("which", ["every", "positive"])
def test_alpha_is_the_oracles_opacity(built, which):
    """sigma = features[row, -1]: the float32 sequence T *= expf(-(length * sigma)) over the oracle's samples, bit for bit
    -- with the unfiltered lists (samples with sigma <= 0 are passed over) and with those of min_sigma = 0."""
    ot, rays, opt, every, pos = built
    L = every if which == "every" else pos
    w, alpha = R.weights(L.length, ot.features[L.row, -1], L.offsets, torch.float32)
    want = O.opacity_render(ot, *rays, opt)
    np.testing.assert_array_equal(alpha.numpy()[:, None], want)
    assert (want > 0).sum() > 100 and w.dtype == torch.float32 and np.all(w.numpy()[ot.features[L.row, -1] <= 0] == 0)


def test_accumulating_depth_gives_the_depth_moments(built):
    ot, rays, opt, every, pos = built
    want = D.moments(ot, rays, opt, "entry", torch.float32).numpy()
    for L in (every, pos):
        w, alpha = R.weights(L.length, ot.features[L.row, -1], L.offsets, torch.float32)
        vals = np.stack([L.depth, L.depth * L.depth], axis=1)
        got = R.accumulate(w, vals, L.offsets, torch.float32).numpy()
        np.testing.assert_array_equal(got, want[:, :2])
        np.testing.assert_array_equal(alpha.numpy(), want[:, 2])
        np.testing.assert_array_equal(R.accumulate(w, None, L.offsets, torch.float32).numpy(),
                                      R.accumulate(w, np.ones((w.shape[0], 1), np.float32), L.offsets, torch.float32).numpy()[:, 0])
    assert (want[:, 0] > 0).sum() > 100


def loss64(L, sigma, g):
    w, alpha = R.weights(L.length, sigma, L.offsets, torch.float64)
    d = torch.from_numpy(L.depth).double()
    m = R.accumulate(w, torch.stack([d, d * d], dim=1), L.offsets, torch.float64)
    return (m * g[:, :2]).sum() + (alpha * g[:, 2]).sum(), w, m


def test_gradient_is_the_depth_moments_and_agrees_with_finite_differences(case, built):
    ot, rays, opt, every, pos = built
    rng = np.random.default_rng(5)
    g = rng.standard_normal((case.Q, 3))
    gt = torch.from_numpy(g)
    L = pos
    sigma = torch.from_numpy(ot.features[L.row, -1]).double().requires_grad_(True)
    loss, w, _ = loss64(L, sigma, gt)
    loss.backward()
    gs = sigma.grad.numpy()
    by_row = np.zeros(ot.M)
    np.add.at(by_row, L.row, gs)
    want = D.moments_grad(ot, rays, opt, "entry", g)
    # two float64 autograd passes over the same function, summed in different orders: 1e-12 of the addends
    scale = D.moments_grad_scale(ot, rays, opt, "entry", g)[:, -1]
    assert np.all(np.abs(by_row - want[:, -1]) <= 1e-12 * scale + 1e-300) and (want[:, -1] != 0).sum() > 100
    # the tight scale prices what grad_sigma is made of
    d = L.depth.astype(np.float64)
    grad_w = g[L.ray, 0] * d + g[L.ray, 1] * d * d
    tight = R.grad_sigma_scale(L.length, ot.features[L.row, -1], L.offsets, grad_w, g[:, 2])
    assert np.all(np.abs(gs) <= tight * (1 + 1e-9)) and np.all(tight > 0)
    # central differences in float64 on 10 samples: truncation ~ h^2 f''' and cancellation ~ 1e-16 |loss| / h, both far
    # below 1e-5 of the gradient's own addends
    cand = np.nonzero(ot.features[L.row, -1] > 1.0)[0]
    base = sigma.detach()
    for k in rng.choice(cand, size=10, replace=False):
        h = 1e-4 * float(base[k])
        sp, sm = base.clone(), base.clone()
        sp[k] += h
        sm[k] -= h
        fd = (float(loss64(L, sp, gt)[0]) - float(loss64(L, sm, gt)[0])) / (2 * h)
        assert abs(fd - gs[k]) <= 1e-5 * tight[k], (k, fd, gs[k], tight[k])


def test_samples_with_no_density_take_no_part(built):
    """sigma <= 0: w = 0, T unchanged, no gradient -- in both precisions."""
    ot, rays, opt, every, pos = built
    L = every
    sig = ot.features[L.row, -1].copy()
    sig[::3] = 0
    sig[1::7] = -2.0
    w32, a32 = R.weights(L.length, sig, L.offsets, torch.float32)
    s64 = torch.from_numpy(sig).double().requires_grad_(True)
    w64, a64 = R.weights(L.length, s64, L.offsets, torch.float64)
    (w64.sum() + a64.sum()).backward()
    off = sig <= 0
    assert np.all(w32.numpy()[off] == 0) and np.all(w64.detach().numpy()[off] == 0) and np.all(s64.grad.numpy()[off] == 0)
    keep = ~off
    counts = np.bincount(L.ray[keep], minlength=len(L.offsets) - 1)
    off2 = np.concatenate([[0], np.cumsum(counts)])
    w32b, a32b = R.weights(L.length[keep], sig[keep], off2, torch.float32)
    np.testing.assert_array_equal(w32.numpy()[keep], w32b.numpy())
    np.testing.assert_array_equal(a32.numpy(), a32b.numpy())
