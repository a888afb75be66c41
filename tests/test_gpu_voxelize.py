"""voxelize / p2v / p2v_backward on the GPU against restatements of the reference (tests/p2v_restate.py): the exact
(point, voxel) pair set, values and gradients, run-to-run determinism, the autograd surface and the edge cases."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import p2v_restate as R

pytestmark = pytest.mark.gpu

HUGE_KR = 1e30          # 2*kr*kr overflows to inf in float32: every weight is exactly 1


def shell(P, seed, cluster=0, center=(0.5, 0.5, 0.5), spread=0.05):
    """noisy sphere shell in the unit cube, the first `cluster` points (after a shuffle) inside one small box"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True) + 1e-12
    pts = np.asarray(center) + 0.35 * (1.0 + spread * rng.normal(size=(P, 1))) * d
    if cluster:
        sel = rng.choice(P, cluster, replace=False)
        pts[sel] = 0.3 + 0.004 * rng.random(size=(cluster, 3))
    return pts.astype(np.float32)


def lattice_case():
    """points on the lattice and half-way, anisotropic voxels (0.125, 0.0625, 0.25), cr = 0.25 exactly: r == cr ties;
    points outside the volume within and beyond cr"""
    corner, size, n = (-1.0, 0.5, -2.0), (2.0, 1.0, 4.0), 17
    vs = np.array([0.125, 0.0625, 0.25], np.float32)
    rng = np.random.default_rng(3)
    ijk = rng.integers(0, n, size=(300, 3)).astype(np.float32)
    on = ijk * vs + np.array(corner, np.float32)
    half = on + 0.5 * vs
    out_near = np.array([[corner[0] - 0.2, corner[1] + 0.5, corner[2] + 1.0],
                         [corner[0] + 1.0, corner[1] + size[1] + 0.25, corner[2] + 2.0],
                         [corner[0] + 2.1, corner[1] + 0.3, corner[2] - 0.25]], np.float32)
    out_far = np.array([[corner[0] - 0.26, 0.7, 0.0], [5.0, 5.0, 5.0], [-1e6, 0.7, 0.0], [0.0, 0.7, 1e30]], np.float32)
    pts = np.concatenate([on, half, out_near, out_far]).astype(np.float32)
    return pts, corner, size, n, 0.25


def run(pts, F, corner, size, n, kr, cr, gpu, seed=0):
    rng = np.random.default_rng(seed)
    feats = rng.random(size=(len(pts), F)).astype(np.float32) + 0.5
    p = torch.from_numpy(pts).to(gpu)
    f = torch.from_numpy(feats).to(gpu)
    return feats, p, f


CASES = [  # (name, P, n, F, corner, size, conv_radius in voxels of axis 0)
    ("n2_P1", 1, 2, 1, (0, 0, 0), (1, 1, 1), 0.3),
    ("n2_P7", 7, 2, 4, (0.1, -0.2, 0.0), (1, 2, 1), 1.5),
    ("n3_P7", 7, 3, 1, (0, 0, 0), (1, 1, 1), 12.0),
    ("n17_P1000", 1000, 17, 4, (0, 0, 0), (1, 1, 1), 2.0),
    ("n17_P1000_r12", 1000, 17, 1, (0.05, 0, -0.1), (1, 1.5, 0.8), 12.0),
    ("n64_P1000_r6", 1000, 64, 4, (0, 0, 0), (1, 1, 1), 6.0),
    ("n64_P50000", 50000, 64, 1, (0, 0, 0), (1, 1, 1), 2.0),
    ("n64_P50000_cluster", 50000, 64, 4, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1.0),
    ("n64_P1000_r0.3", 1000, 64, 1, (-0.5, -0.5, -0.5), (2, 1, 1), 0.3),
]


@pytest.mark.parametrize("case", CASES + [("lattice", None, None, 4, None, None, None)], ids=lambda c: c[0])
def test_exact_pair_set(gpu, case):
    name, P, n, F, corner, size, crv = case
    if name == "lattice":
        pts, corner, size, n, cr = lattice_case()
        P = len(pts)
    else:
        pts = shell(P, seed=P + n, cluster=20000 if "cluster" in name else 0)
        cr = crv * float(size[0]) / (n - 1)
    feats, p, f = run(pts, F, corner, size, n, HUGE_KR, cr, gpu)
    f[:, F - 1] = 1.0
    pr = R.pairs(pts, corner, size, n, cr)
    want_vox, want_pt = R.pair_counts(pr, P, n)
    got = svox.voxelize(p, f, corner, size, n, HUGE_KR, cr)
    assert got.shape == (n, n, n, 1) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want_vox.astype(np.float32)), name
    pg, fg = _C.p2v_backward(torch.ones(n, n, n, 1, device=gpu), p, f, corner, size, n, HUGE_KR, cr)
    fg = fg.cpu().numpy()
    assert np.array_equal(fg[:, F - 1], want_pt.astype(np.float32))
    assert not fg[:, :F - 1].any()
    assert not pg.cpu().numpy().any()


def test_no_points(gpu):
    for corner, size in (((0, 0, 0), (1, 1, 1)), (torch.zeros(3, device=gpu), torch.ones(3, device=gpu))):
        v = svox.voxelize(torch.zeros(0, 3, device=gpu), torch.zeros(0, 2, device=gpu), corner, size, 5, 1.0, 0.5)
        assert v.shape == (5, 5, 5, 1) and not v.any()


@pytest.mark.parametrize("P,n,F,crv,krv,corner,size", [
    (1000, 17, 4, 2.0, 1.0, (0, 0, 0), (1, 1, 1)),
    (20000, 64, 1, 3.0, 1.5, (-0.1, 0.0, 0.05), (1.2, 1.0, 0.9)),
    (2000, 64, 2, 6.0, 2.0, (0, 0, 0), (1, 1, 1)),
    (200000, 256, 1, 2.0, 1.0, (0, 0, 0), (1, 1, 1)),
])
def test_values_and_gradients(gpu, P, n, F, crv, krv, corner, size):
    pts = shell(P, seed=7 + P)
    vs = float(size[0]) / (n - 1)
    cr, kr = crv * vs, krv * vs
    feats, p, f = run(pts, F, corner, size, n, kr, cr, gpu, seed=P)
    go = np.random.default_rng(1).normal(size=(n, n, n, 1)).astype(np.float32)
    pr = R.pairs(pts, corner, size, n, cr)
    vol, scale, pg_w, pabs, fg_w, fabs = R.forward_backward(pts, feats, pr, corner, size, n, kr, go)
    got = _C.p2v(p, f, corner, size, n, kr, cr).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - vol) <= 1e-5 * scale)
    pg, fg = _C.p2v_backward(torch.from_numpy(go).to(gpu), p, f, corner, size, n, kr, cr)
    pg, fg = pg.cpu().numpy().astype(np.float64), fg.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(pg - pg_w) <= 1e-6 * pabs)
    assert np.all(np.abs(fg[:, F - 1] - fg_w) <= 1e-6 * fabs)
    assert not fg[:, :F - 1].any()


def test_deterministic_with_a_split_tile(gpu):
    P, n = 2_000_000, 256
    pts = shell(P, seed=11, cluster=500_000)            # the cluster: one 4x4x4 tile, hundreds of chunks
    vs = 1.0 / (n - 1)
    feats, p, f = run(pts, 1, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs, gpu)
    a = _C.p2v(p, f, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    b = _C.p2v(p, f, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    assert torch.equal(a, b)
    assert a.sum().item() > 0
    go = torch.randn(n, n, n, 1, device=gpu)
    g1 = _C.p2v_backward(go, p, f, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    g2 = _C.p2v_backward(go, p, f, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


def test_autograd(gpu):
    n, P, F = 32, 3000, 3
    vs = 1.0 / (n - 1)
    pts = shell(P, seed=5)
    feats, p, f = run(pts, F, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs, gpu)
    pr_, fr_ = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
    v = svox.voxelize(pr_, fr_, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    assert v.grad_fn is not None
    v.sum().backward()                                   # an expanded, stride-0 gradient
    pg, fg = _C.p2v_backward(torch.ones(n, n, n, 1, device=gpu), p, f, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    assert torch.equal(pr_.grad, pg) and torch.equal(fr_.grad, fg)
    assert fr_.grad[:, F - 1].abs().sum() > 0 and pr_.grad.abs().sum() > 0
    # only the features require a gradient: they get one (the reference returns None unless points require one)
    f2 = f.clone().requires_grad_(True)
    svox.voxelize(p, f2, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs).sum().backward()
    assert f2.grad is not None and torch.equal(f2.grad, fg)
    # only the points
    p3 = p.clone().requires_grad_(True)
    svox.voxelize(p3, f, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs).sum().backward()
    assert torch.equal(p3.grad, pg)
    # nothing to record: no graph, nothing saved
    assert svox.voxelize(p, f, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs).grad_fn is None
    with torch.no_grad():
        assert svox.voxelize(pr_, fr_, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs).grad_fn is None
    # F = 1: column F-1 is column 0, where the reference writes the feature gradient (p2v_kernel.cu:203): its value,
    # sum over the point's pairs of grad_output * w, against the float64 restatement
    f1 = f[:, :1].clone().requires_grad_(True)
    svox.voxelize(p, f1, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs).sum().backward()
    pr = R.pairs(pts, (0, 0, 0), (1, 1, 1), n, 2 * vs)
    *_, col0, col0_abs = R.forward_backward(pts, feats[:, :1], pr, (0, 0, 0), (1, 1, 1), n, vs, np.ones((n, n, n, 1)))
    got = f1.grad[:, 0].cpu().numpy().astype(np.float64)
    assert f1.grad.shape == (P, 1) and col0_abs.sum() > 0
    assert np.all(np.abs(got - col0) <= 1e-6 * col0_abs)


def test_far_corner(gpu):
    """A corner far from the origin widens the apron's rounding bound: the workspace the Python layer asks for must
    be what the forward plans with, and the pair set is still the reference's."""
    for corner, crv in (((100.0, 100.0, 100.0), 3.49), ((1000.0, -1000.0, 1000.0), 3.3)):
        n, P = 256, 20000
        vs = 1.0 / (n - 1)
        cr = crv * vs
        pts = (shell(P, seed=21) + np.asarray(corner, np.float32)).astype(np.float32)
        feats, p, f = run(pts, 1, corner, (1, 1, 1), n, HUGE_KR, cr, gpu)
        f.fill_(1.0)
        want, _ = R.pair_counts(R.pairs(pts, corner, (1, 1, 1), n, cr), P, n)
        got = svox.voxelize(p, f, corner, (1, 1, 1), n, HUGE_KR, cr)
        assert np.array_equal(got.cpu().numpy(), want.astype(np.float32)), corner


def test_edge_cases(gpu):
    n = 16
    vs = 1.0 / (n - 1)
    pts = shell(5000, seed=9)
    feats, p, f = run(pts, 2, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs, gpu)
    far = torch.full((100, 3), 7.0, device=gpu)
    v = svox.voxelize(far, torch.ones(100, 1, device=gpu), (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    assert v.shape == (n, n, n, 1) and not v.any()
    base = svox.voxelize(p, f, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    assert base.is_contiguous() and base.dtype == torch.float32 and base.device == p.device
    # a NaN / inf point contributes nothing (the other points keep their order: bit-identical) and gets zero gradient
    bad = torch.tensor([[float("nan"), 0.5, 0.5], [0.5, float("inf"), 0.5]], device=gpu)
    p2 = torch.cat([p[:100], bad, p[100:]])
    f2 = torch.cat([f[:100], torch.ones(2, 2, device=gpu), f[100:]])
    assert torch.equal(svox.voxelize(p2, f2, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs), base)
    pg, fg = _C.p2v_backward(torch.ones(n, n, n, 1, device=gpu), p2, f2, (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    assert not pg[100:102].any() and not fg[100:102].any()
    # float32 only, on the device
    with pytest.raises(RuntimeError):
        svox.voxelize(p.double(), f.double(), (0, 0, 0), (1, 1, 1), n, vs, 2 * vs)
    with pytest.raises(RuntimeError):
        svox.voxelize(p, f, (0, 0, 0), (1, 1, 1), 1, vs, 2 * vs)
    with pytest.raises(RuntimeError):
        svox.voxelize(p, f, (0, 0, 0), (1, 1, 1), n, 0.0, 2 * vs)
