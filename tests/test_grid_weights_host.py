"""grid_weights without a GPU: the restatement the GPU tests compare against is itself pinned to the C++ oracle (a
dense grid of R <= 16 IS a one-node N3Tree with N = R; for R = 2^L a full octree of depth L takes bit-identical
steps), the new names exist, and every argument check fires before any GPU work."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import grid_weight_restate as G

INVALID = 1


def _case(R, W, H, seed, sigma_thresh=0.0):
    sigma = G.shell_sigma(R, seed=seed, scale=6.0 * R / 8)
    scaling = np.array([0.5, 0.4, 0.45], np.float32)                   # non-cubic
    offset = np.array([0.5, 0.52, 0.48], np.float32)
    c2w = G.look_at((1.9, 1.3, 0.9), target=(0.0, 0.0, 0.0))
    o, d, v = O.camera_rays(c2w, 1.1 * W, 1.1 * W, W, H)
    return sigma, o, d, v, offset, scaling, sigma_thresh


def _check_against_oracle(tree_arrays, sigma, o, d, v, offset, scaling, sigma_thresh):
    feat, data, child = tree_arrays
    tree = O.Tree(feat, data, child, offset=offset, scaling=scaling)
    # stop_thresh = -1: the oracle never stops early, like grid_trace_ray
    opt = O.make_options(step_size=1e-3, sigma_thresh=sigma_thresh, stop_thresh=-1.0)
    out, cnt = O.volume_render(tree, o, d, v, opt, count=True)
    _, wacc = O.volume_render_weights(tree, o, d, v, opt)
    res = G.march(sigma, o, d, offset, scaling, step_size=1e-3, sigma_thresh=sigma_thresh)
    assert cnt.rays_hit == int(res.hit_cube.sum()) and cnt.rays_hit > 0
    assert cnt.steps == int(res.steps.sum())
    assert cnt.active == int(res.active.sum()) == int(res.hits.sum()) and cnt.active > 0
    alpha = (np.float32(1) - res.T).astype(np.float32)
    alpha[~res.hit_cube] = 0
    assert np.array_equal(alpha.view(np.int32), np.ascontiguousarray(out[:, -1]).view(np.int32)), "1 - T is not the oracle's alpha"
    # per-cell sums of the weights: the oracle adds in ray order, the restatement in step order (both in double)
    R = sigma.shape[0]
    if child.shape[1] == R:                                            # one node: slot = cell
        wsum = wacc.reshape(R, R, R)
    else:                                                              # full octree: the last level's slots, by data word
        leaf = child.reshape(-1) == 0
        wsum = np.zeros(R ** 3)
        wsum[data.reshape(-1)[leaf]] = wacc.reshape(-1)[leaf]
        wsum = wsum.reshape(R, R, R)
    np.testing.assert_allclose(res.weight_sum, wsum, rtol=0, atol=1e-12)
    assert (res.weight <= res.weight_sum.astype(np.float32) * np.float32(1 + 1e-6)).all()
    assert ((res.weight > 0) <= (res.hits > 0)).all()
    assert res.hits.max() < 1 << 24
    return res


@pytest.mark.parametrize("R", [8, 16])
def test_restatement_is_the_oracle_on_a_one_node_tree(R):
    sigma, o, d, v, offset, scaling, thr = _case(R, 64, 64, seed=R)
    _check_against_oracle(G.one_node_tree(sigma), sigma, o, d, v, offset, scaling, thr)


def test_restatement_is_the_oracle_on_a_full_octree():
    sigma, o, d, v, offset, scaling, thr = _case(64, 128, 128, seed=3, sigma_thresh=0.01)
    res = _check_against_oracle(G.full_octree(sigma), sigma, o, d, v, offset, scaling, thr)
    assert int(res.steps.sum()) > 500_000


def test_full_octree_equals_one_node_tree():
    """the two embeddings of the same grid (R = 16 is both) give the oracle the same steps"""
    sigma, o, d, v, offset, scaling, _ = _case(16, 32, 32, seed=5)
    opt = O.make_options(step_size=1e-3, stop_thresh=-1.0)
    outs = []
    for feat, data, child in (G.one_node_tree(sigma), G.full_octree(sigma)):
        out, cnt = O.volume_render(O.Tree(feat, data, child, offset=offset, scaling=scaling), o, d, v, opt, count=True)
        outs.append((out, cnt.steps, cnt.active))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:]


def test_march_ends_when_the_step_cannot_move_t():
    """An axis-aligned ray through cell corners with step_size = 1e-9, from far enough away that t is in the thousands:
    it enters at x = 1, crosses the first cell and lands exactly on the corner x = 0.875 going down -- the cell-local
    coordinate is 0, the chord is 0, delta_t = 1e-9 and t + 1e-9 == t in float.  The reference's bare `t += delta_t`
    never ends there; with march_advance the march ends (and the kernel advances t through march_advance only)."""
    R = 8
    sigma = np.ones((R, R, R), np.float32)
    o = np.array([[1024.5, 0.25, 0.5]], np.float32)
    d = np.array([[-1.0, 0.0, 0.0]], np.float32)
    unit = dict(offset=np.zeros(3, np.float32), scaling=np.ones(3, np.float32))
    res = G.march(sigma, o, d, step_size=1e-9, max_steps=100_000, **unit)
    assert res.hit_cube[0] and res.iterations == 2 and res.hits.sum() == 2
    with pytest.raises(AssertionError, match="did not end"):           # the same ray without the guard stalls
        G.march(sigma, o, d, step_size=1e-9, advance_guard=False, max_steps=2_000, **unit)
    assert G.march(sigma, o, d, step_size=1e-3, max_steps=2_000, **unit).iterations >= 8   # a step that moves t: all 8 cells


# ---- the new names --------------------------------------------------------------------------------------------------

def test_library_exports_grid_weights():
    assert "svoxt_grid_weights" in _C.EXPORTS
    assert hasattr(_C._lib, "svoxt_grid_weights")
    assert _C._lib.svoxt_abi_version() == 22                           # exports were added, nothing changed


def test_public_name():
    assert callable(svox.grid_weights) and callable(_C.grid_weights)
    assert "grid_weights" in svox.__all__ and "GridWeights" in svox.__all__
    assert svox.GridWeights._fields == ("weight", "hits")


def test_reference_name_stays_a_stub_that_names_the_new_one():
    with pytest.raises(NotImplementedError, match="grid_weights"):
        _C.grid_weight_render(None, None, None)


# ---- argument checks: the C ABI (pointers are never dereferenced: every case is refused before any HIP call) --------

def _abi_call(**kw):
    a = dict(sigma=1, R=8, c2w=1, Q=64, w=8, h=8, fx=10.0, fy=10.0, origins=None, dirs=None, V=1, stride=16, step=1e-3,
             offset=1, scaling=1, flags=0, weight=2, hits=3, opt=True, rays=True)
    a.update(kw)
    r = _C._CRays()
    r.c2w, r.Q, r.image_width, r.image_height, r.fx, r.fy = a["c2w"], a["Q"], a["w"], a["h"], a["fx"], a["fy"]
    r.origins, r.dirs = a["origins"], a["dirs"]
    o = _C._COptions()
    o.step_size, o.ndc_width = a["step"], -1
    rc = _C._lib.svoxt_grid_weights(a["sigma"], a["R"], ctypes.byref(r) if a["rays"] else None, a["V"], a["stride"],
                                    ctypes.byref(o) if a["opt"] else None, a["offset"], a["scaling"], a["flags"], a["weight"],
                                    a["hits"], None)
    return rc, _C._lib.svoxt_last_error()


ABI_BAD = [dict(R=0), dict(R=-4), dict(R=1291), dict(sigma=None), dict(weight=None), dict(hits=None), dict(hits=2),
           dict(offset=None), dict(scaling=None), dict(opt=False), dict(rays=False), dict(step=0.0), dict(step=-1e-3),
           dict(step=float("inf")), dict(step=float("nan")), dict(flags=2), dict(V=0), dict(V=-1), dict(stride=9),
           dict(Q=63), dict(w=0, Q=0), dict(fx=0.0), dict(fy=float("nan")), dict(w=1 << 17, h=1 << 17, Q=1 << 34, V=64),
           dict(c2w=None, V=2, origins=1, dirs=1), dict(c2w=None, origins=None, dirs=1), dict(c2w=None, origins=1, dirs=None),
           dict(c2w=None, Q=-1, origins=1, dirs=1)]


@pytest.mark.parametrize("bad", ABI_BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in ABI_BAD])
def test_abi_rejects_before_any_hip_call(bad):
    rc, err = _abi_call(**bad)
    assert rc == INVALID, err
    assert b"svoxt_grid_weights" in err


def test_abi_accepts_the_largest_volume_up_to_the_checks_behind_it():
    rc, err = _abi_call(R=1290, rays=False)                            # 1290^3 < 2^31 <= 1291^3
    assert rc == INVALID and b"rays is NULL" in err


# ---- argument checks: the Python layers (CPU or meta tensors: nothing can reach the GPU) ------------------------------

CAM = dict(cameras=torch.eye(4)[None], fx=10.0, width=8, height=8)
RAYS = dict(rays=(torch.zeros(4, 3), torch.ones(4, 3)))
S8 = torch.zeros(8, 8, 8)
PY_BAD = [
    ("CUDA tensor", dict(sigma=S8, **CAM)),                                                   # CPU tensors
    ("CUDA tensor", dict(sigma=S8, **RAYS)),
    ("float32", dict(sigma=S8.double(), **CAM)),
    ("cubic", dict(sigma=torch.zeros(8, 8, 4), **CAM)),
    ("cubic", dict(sigma=torch.zeros(8, 8), **CAM)),
    ("cubic", dict(sigma=torch.zeros(8, 8, 8, 2), **CAM)),
    ("cubic", dict(sigma=torch.zeros(0, 0, 0), **CAM)),
    ("2\\^31", dict(sigma=torch.empty(1291, 1291, 1291, device="meta"), **CAM)),
    ("exactly one", dict(sigma=S8, **CAM, **RAYS)),
    ("exactly one", dict(sigma=S8)),
    ("no view", dict(sigma=S8, **dict(CAM, cameras=torch.zeros(0, 4, 4)))),
    ("cameras must be", dict(sigma=S8, **dict(CAM, cameras=torch.zeros(2, 4, 3)))),
    ("cameras must be", dict(sigma=S8, **dict(CAM, cameras=torch.eye(4, dtype=torch.float64)[None]))),
    ("fx, width and height", dict(sigma=S8, cameras=torch.eye(4)[None])),
    ("positive", dict(sigma=S8, **dict(CAM, width=0))),
    (r"\[Q, 3\]", dict(sigma=S8, rays=(torch.zeros(4, 2), torch.ones(4, 2)))),
    ("same number", dict(sigma=S8, rays=(torch.zeros(4, 3), torch.ones(5, 3)))),
    ("ndc", dict(sigma=S8, ndc=svox.NDCConfig(8, 8, 10.0), **RAYS)),
    ("shape of sigma", dict(sigma=S8, out=(torch.zeros(8, 8, 8), torch.zeros(8, 8, 8, 1)), **CAM)),
    ("shape of sigma", dict(sigma=S8, out=(torch.zeros(4, 4, 4), torch.zeros(4, 4, 4)), **CAM)),
    ("shape of sigma", dict(sigma=S8, out=(torch.zeros(8, 8, 8), torch.zeros(8, 8, 8, dtype=torch.int32)), **CAM)),
    (r"\(weight, hits\)", dict(sigma=S8, out=torch.zeros(8, 8, 8), **CAM)),
    ("two tensors", dict(sigma=S8, out=(S8, S8), **CAM)),
    ("step_size", dict(sigma=S8, step_size=0.0, **CAM)),
    ("step_size", dict(sigma=S8, step_size=-1.0, **CAM)),
    ("step_size", dict(sigma=S8, step_size=float("inf"), **CAM)),
    ("step_size", dict(sigma=S8, step_size=float("nan"), **CAM)),
    ("not both", dict(sigma=S8, radius=1.0, offset=[0, 0, 0], scaling=[1, 1, 1], **CAM)),
    ("go together", dict(sigma=S8, offset=[0, 0, 0], **CAM)),
    ("1 or 3", dict(sigma=S8, radius=[1.0, 2.0], **CAM)),
]


@pytest.mark.parametrize("match,kw", PY_BAD, ids=[f"{i}-{m}" for i, (m, _) in enumerate(PY_BAD)])
def test_python_layer_refuses(match, kw):
    kw = dict(kw)
    sigma = kw.pop("sigma")
    with pytest.raises(RuntimeError, match=match) as e:
        svox.grid_weights(sigma, **kw)
    assert not isinstance(e.value, NotImplementedError)


def test_radius_and_center_map_like_n3tree():
    """offset = 0.5 (1 - center / radius), scaling = 0.5 / radius: seen through the operator module's arguments"""
    seen = {}
    real = _C.grid_weights

    def spy(sigma, spec, opt, offset, scaling, out=None):
        seen.update(offset=offset, scaling=scaling, opt=opt, spec=spec)
        return real(sigma, spec, opt, offset, scaling, out=out)

    import svox_t_amd.gridw as gridw
    gridw._C.grid_weights, keep = spy, gridw._C.grid_weights
    try:
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            svox.grid_weights(S8, radius=[1.0, 2.0, 4.0], center=[0.5, 1.0, -1.0], sigma_thresh=0.25, step_size=0.01,
                              ndc=svox.NDCConfig(8, 6, 10.0), **CAM)
    finally:
        gridw._C.grid_weights = keep
    tree = svox.N3Tree(radius=[1.0, 2.0, 4.0], center=[0.5, 1.0, -1.0])
    assert torch.equal(seen["offset"], tree.offset) and torch.equal(seen["scaling"], tree.invradius)
    o = seen["opt"]
    assert (o.step_size, o.sigma_thresh, o.ndc_width, o.ndc_height, o.ndc_focal) == (0.01, 0.25, 8, 6, 10.0)
    assert seen["spec"].fy == 10.0                                     # fy defaults to fx
