"""grid_weights on the GPU against the numpy restatement of the reference's grid_weight_render
(tests/grid_weight_restate.py, itself pinned to the C++ oracle by tests/test_grid_weights_host.py): hits equal and
weight bit-identical over ALL cells, many views against single views and against streaming through out=, run-to-run
determinism, the marching kernels' own counter on the equivalent octree,
and the voxelize -> grid_weights -> build_from_points pipeline."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import grid_weight_restate as G

pytestmark = pytest.mark.gpu

CUBIC = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))                 # (offset, scaling): world cube [-1, 1]^3
SKEW = ((0.5, 0.52, 0.47), (0.5, 0.4, 0.45))               # non-cubic scaling, off-centre: world box around the origin


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def eye_for(geom, direction, dist):
    """a camera position `dist` unit-cube lengths from the cube's centre, in world coordinates"""
    off, sc = (np.asarray(v, np.float64) for v in geom)
    d = np.asarray(direction, np.float64)
    centre = (0.5 - off) / sc
    return centre + dist * d / np.linalg.norm(d) / sc, centre


def gpu_run(gpu, sigma, c2w, f, W, H, geom, **kw):
    res = svox.grid_weights(torch.from_numpy(sigma).to(gpu), cameras=torch.from_numpy(np.asarray(c2w, np.float32)).to(gpu),
                            fx=f, fy=f, width=W, height=H, offset=list(geom[0]), scaling=list(geom[1]), **kw)
    assert isinstance(res, svox.GridWeights) and res.weight.shape == sigma.shape and res.hits.shape == sigma.shape
    return res.weight.cpu().numpy(), res.hits.cpu().numpy()


def check(gpu, sigma, c2w, f, W, H, geom, ndc=None, expect_hits=True, **kw):
    want = G.march_cameras(sigma, c2w, f, f, W, H, geom[0], geom[1], ndc=ndc, **kw)
    assert want.hits.max() < 1 << 24                        # where the reference's float count is exact too
    assert (want.hits.sum() > 0) == expect_hits
    weight, hits = gpu_run(gpu, sigma, c2w, f, W, H, geom, ndc=None if ndc is None else svox.NDCConfig(*ndc), **kw)
    print(f"R={sigma.shape[0]} {W}x{H}: hits {int(want.hits.sum())} in {int((want.hits > 0).sum())} cells, "
          f"hits differ in {int((hits.astype(np.int64) != want.hits).sum())}, weight bits differ in "
          f"{int((bits(weight) != bits(want.weight)).sum())} of {want.hits.size}")
    assert np.array_equal(hits.astype(np.int64), want.hits)
    assert np.array_equal(bits(weight), bits(want.weight))
    return weight, hits


# (R, W, H, geometry, view direction, distance, sigma_thresh, step_size): cameras outside (distance > 0.87) and inside
CASES = [
    (1, 16, 16, CUBIC, (1.0, 0.4, 0.3), 1.6, 0.0, 1e-3),
    (5, 20, 12, SKEW, (0.3, -1.0, 0.5), 1.4, 0.0, 1e-3),
    (5, 8, 8, CUBIC, (0.2, 0.1, 1.0), 0.2, 0.01, 1e-2),
    (16, 24, 24, CUBIC, (1.0, 0.2, -0.3), 0.1, 0.01, 1e-3),
    (16, 31, 17, SKEW, (-0.5, 0.7, 0.6), 1.5, 0.0, 1e-2),
    (64, 64, 48, SKEW, (0.9, 0.5, 0.35), 1.5, 0.0, 1e-2),
    (64, 40, 40, CUBIC, (0.1, -0.9, 0.2), 0.3, 0.01, 1e-3),
    (100, 37, 29, SKEW, (0.6, 0.6, -0.5), 1.3, 0.01, 1e-3),
    (100, 32, 32, CUBIC, (-1.0, 0.1, 0.1), 1.2, 0.0, 1e-3),
]


@pytest.mark.parametrize("R,W,H,geom,direction,dist,thr,step", CASES,
                         ids=[f"R{c[0]}-{c[1]}x{c[2]}-{'cubic' if c[3] is CUBIC else 'skew'}-d{c[5]}-t{c[6]}-s{c[7]}" for c in CASES])
def test_matches_the_restatement_bit_for_bit(gpu, R, W, H, geom, direction, dist, thr, step):
    sigma = G.shell_sigma(R, seed=R + W, scale=0.6 * R)
    eye, centre = eye_for(geom, direction, dist)
    check(gpu, sigma, G.look_at(eye, centre), 1.2 * W, W, H, geom, sigma_thresh=thr, step_size=step)


def test_camera_looking_away_leaves_zeros(gpu):
    sigma = G.shell_sigma(16, seed=1)
    eye, centre = eye_for(CUBIC, (1.0, 0.3, 0.2), 2.0)
    weight, hits = check(gpu, sigma, G.look_at(eye, 2 * eye - centre), 30.0, 24, 16, CUBIC, expect_hits=False)
    assert not weight.any() and not hits.any()


def test_zero_inf_and_nan_cells(gpu):
    R = 16
    sigma = G.shell_sigma(R, seed=2, inner=0.0, outer=1.0, scale=3.0)          # dense: every ray samples many cells
    sigma[::3] = 0.0
    sigma[8] = np.inf                                       # an opaque wall across the cube; the camera is on its +x side
    sigma[10, 8, 8] = np.nan
    sigma[11, 7, 9] = np.nan
    eye, centre = eye_for(CUBIC, (1.0, 0.25, 0.15), 1.5)    # (y and z inside the cube's extent: every ray enters through +x)
    weight, hits = check(gpu, sigma, G.look_at(eye, centre), 60.0, 48, 48, CUBIC)
    assert hits[8].sum() > 0 and hits[10, 8, 8] == 0 and hits[11, 7, 9] == 0 and hits[10, 8, 7] > 0 and not hits[::3].any()
    assert np.isfinite(weight).all() and weight[9:].max() > 0
    # the rays go on behind the wall: what lies there is sampled with T == 0 and still counted, with weight 0
    assert hits[:8].sum() > 0 and not weight[:8].any()


def test_ndc(gpu):
    """forward-facing camera, NDC warp on: the volume is the NDC cube [-1, 1]^3"""
    R, W, H, f = 16, 24, 16, 20.0
    sigma = G.shell_sigma(R, seed=4, inner=0.0, outer=1.0, scale=2.0)
    geom = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = (0.1, -0.05, 0.3)
    check(gpu, sigma, c2w, f, W, H, geom, ndc=(W, H, f))


def test_trailing_unit_dimension_and_ray_batch_mode(gpu):
    R, W, H, f = 16, 20, 20, 25.0
    sigma = G.shell_sigma(R, seed=6)
    eye, centre = eye_for(SKEW, (0.7, 0.6, 0.4), 1.5)
    c2w = G.look_at(eye, centre)
    weight, hits = check(gpu, sigma, c2w, f, W, H, SKEW)
    w4, h4 = gpu_run(gpu, sigma[..., None], c2w, f, W, H, SKEW)
    assert w4.shape == (R, R, R, 1) and np.array_equal(bits(w4[..., 0]), bits(weight)) and np.array_equal(h4[..., 0], hits)
    # [3, 4] matrices and a single matrix without the view dimension are the same camera
    w3, h3 = gpu_run(gpu, sigma, c2w[None, :3], f, W, H, SKEW)
    w2, h2 = gpu_run(gpu, sigma, c2w, f, W, H, SKEW)
    assert np.array_equal(bits(w3), bits(weight)) and np.array_equal(h3, hits)
    assert np.array_equal(bits(w2), bits(weight)) and np.array_equal(h2, hits)
    o, d, v = O.camera_rays(c2w, f, f, W, H)
    res = svox.grid_weights(torch.from_numpy(sigma).to(gpu), rays=svox.Rays(*(torch.from_numpy(x).to(gpu) for x in (o, d, v))),
                            offset=list(SKEW[0]), scaling=list(SKEW[1]))
    assert np.array_equal(bits(res.weight.cpu().numpy()), bits(weight)) and np.array_equal(res.hits.cpu().numpy(), hits)
    empty = svox.grid_weights(torch.from_numpy(sigma).to(gpu), rays=(torch.zeros(0, 3, device=gpu), torch.zeros(0, 3, device=gpu)))
    assert not empty.weight.any() and not empty.hits.any()


def _seven_views(geom):
    dirs = [(1, 0.2, 0.1), (-1, 0.3, 0.2), (0.2, 1, -0.3), (0.1, -1, 0.4), (0.3, 0.2, 1), (-0.2, 0.4, -1), (0.7, 0.7, 0.7)]
    return np.stack([G.look_at(*eye_for(geom, d, 1.3 + 0.05 * i)) for i, d in enumerate(dirs)])


def test_many_views_equal_single_views_and_streaming(gpu):
    R, W, H, f = 16, 28, 20, 30.0
    sigma = G.shell_sigma(R, seed=7)
    c2w = _seven_views(SKEW)
    weight, hits = check(gpu, sigma, c2w, f, W, H, SKEW, sigma_thresh=0.01)
    singles = [gpu_run(gpu, sigma, c2w[i:i + 1], f, W, H, SKEW, sigma_thresh=0.01) for i in range(7)]
    assert np.array_equal(bits(np.max([s[0] for s in singles], axis=0)), bits(weight))
    assert np.array_equal(np.sum([s[1].astype(np.int64) for s in singles], axis=0), hits.astype(np.int64))
    out = None
    for part in (c2w[:3], c2w[3:4], c2w[4:]):               # streamed: max and count compose across calls
        res = svox.grid_weights(torch.from_numpy(sigma).to(gpu), cameras=torch.from_numpy(part).to(gpu), fx=f, width=W, height=H,
                                offset=list(SKEW[0]), scaling=list(SKEW[1]), sigma_thresh=0.01, out=out)
        if out is not None:
            assert res.weight is out[0] and res.hits is out[1]
        out = (res.weight, res.hits)
    assert np.array_equal(bits(out[0].cpu().numpy()), bits(weight)) and np.array_equal(out[1].cpu().numpy(), hits)


def test_same_bits_twice_and_through_the_operator_module(gpu):
    R, W, H, f = 64, 96, 72, 90.0
    sigma = torch.from_numpy(G.shell_sigma(R, seed=8)).to(gpu)
    cams = torch.from_numpy(_seven_views(CUBIC)).to(gpu)
    kw = dict(cameras=cams, fx=f, width=W, height=H, offset=list(CUBIC[0]), scaling=list(CUBIC[1]))
    a, b = svox.grid_weights(sigma, **kw), svox.grid_weights(sigma, **kw)
    assert a.hits.sum() > 0
    assert torch.equal(a.weight.view(torch.int32), b.weight.view(torch.int32)) and torch.equal(a.hits, b.hits)
    spec, opt = _C.CameraSpec(), _C.RenderOptions()
    spec.c2w, spec.fx, spec.fy, spec.width, spec.height = cams, f, f, W, H
    opt.step_size, opt.ndc_width = 1e-3, -1
    half = torch.full((3,), 0.5, device=gpu)
    w, h = _C.grid_weights(sigma, spec, opt, half, half)     # the reference's argument order, its (weight, hits)
    assert torch.equal(w.view(torch.int32), a.weight.view(torch.int32)) and torch.equal(h, a.hits)


def test_hits_equal_the_tree_march_counter_on_the_equivalent_octree(gpu):
    """no CPU in it: the dense grid of R = 64 as a full depth-6 octree, marched by count_fwd_kernel"""
    R, W, H, f = 64, 120, 88, 110.0
    sig = G.shell_sigma(R, seed=9)
    feat, data, child = G.full_octree(sig)
    eye, centre = eye_for(SKEW, (0.8, -0.5, 0.4), 1.4)
    o, d, v = (torch.from_numpy(x).to(gpu) for x in O.camera_rays(G.look_at(eye, centre), f, f, W, H))
    offset, scaling = (torch.tensor(x, dtype=torch.float32, device=gpu) for x in SKEW)
    for thr, step in ((0.0, 1e-3), (0.01, 1e-2)):
        tree = _C.TreeSpec()
        tree.features, tree.data, tree.child = (torch.from_numpy(x).to(gpu) for x in (feat, data, child))
        tree.offset, tree.scaling = offset, scaling
        rays = _C.RaysSpec()
        rays.origins, rays.dirs, rays.vdirs = o, d, v
        opt = _C.RenderOptions()
        opt.step_size, opt.sigma_thresh, opt.stop_thresh, opt.ndc_width = step, thr, -1.0, -1       # never stops early
        counters = _C.count_forward(tree, rays, opt).cpu().tolist()
        res = svox.grid_weights(torch.from_numpy(sig).to(gpu), rays=(o, d), offset=offset, scaling=scaling, sigma_thresh=thr,
                                step_size=step)
        assert counters[4] > 0 and int(res.hits.double().sum().item()) == counters[4]


def _leaves(child, data):
    """(data word, integer corner at the leaf's own depth, depth) of every leaf of an N = 2 tree"""
    out, todo = [], [(0, np.zeros(3, np.int64), 0)]
    while todo:
        node, corner, depth = todo.pop()
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    c = corner * 2 + (i, j, k)
                    if child[node, i, j, k] != 0:
                        todo.append((node + int(child[node, i, j, k]), c, depth + 1))
                    else:
                        out.append((int(data[node, i, j, k]), c, depth + 1))
    return out


def test_pipeline_voxelize_grid_weights_build(gpu):
    n, depth = 32, 5
    rng = np.random.default_rng(11)
    d = rng.normal(size=(4000, 3))
    pts = (0.5 + 0.3 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    vol = svox.voxelize(torch.from_numpy(pts).to(gpu), torch.full((len(pts), 1), 4.0, device=gpu), [0.0, 0.0, 0.0],
                        [1.0, 1.0, 1.0], n, 0.02, 0.06)
    assert vol.shape == (n, n, n, 1)
    # voxel i sits at i / (n - 1): the world box whose cell centres are the voxels
    radius, center = 0.5 * n / (n - 1), 0.5
    cams = torch.from_numpy(np.stack([G.look_at((0.5 + 1.4 * np.cos(a), 0.5 + 1.4 * np.sin(a), 0.5 + 0.4 * np.sin(2 * a)))
                                      for a in np.linspace(0, 2 * np.pi, 6, endpoint=False)])).to(gpu)
    gw = svox.grid_weights(vol, cameras=cams, fx=140.0, width=128, height=128, radius=radius, center=center, sigma_thresh=0.01)
    thr = 0.05
    cells = (gw.weight[..., 0] > thr).nonzero()
    assert 100 < len(cells) < n ** 3 // 4
    centres = cells.to(torch.float32) / (n - 1)
    tree = svox.N3Tree(N=2, data_dim=4, radius=radius, center=[center] * 3, map_location=gpu)
    n_internal = tree.build_from_points(centres, depth)
    child, data = tree.child[:n_internal].cpu().numpy(), tree.data[:n_internal].cpu().numpy().reshape(n_internal, 2, 2, 2)
    passed = {tuple(c) for c in cells.cpu().tolist()}
    built = [(idx, c, dep) for idx, c, dep in _leaves(child, data) if 0 <= idx < len(cells)]
    assert len(built) == len(cells)                          # one leaf per passed cell ...
    weight = gw.weight[..., 0].cpu().numpy()
    for idx, c, dep in built:                                # ... at the cells' depth, in a cell whose weight passed
        assert dep == depth and tuple(c) in passed and weight[tuple(c)] > thr
        assert tuple(c) == tuple(cells[idx].tolist())
