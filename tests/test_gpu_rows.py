"""Samples to feature rows and back on the GPU: the row plan, gather_rows, reduce_rows and spread_rows against the numpy
restatement (tests/rows_restate.py), bit for bit, and against torch indexing.

Inputs: (a) the real lists of d5_rgba4 and d6_sh9; (b) the same lists with row % 13 (segments of more than a thousand
samples: several chunks and a ragged tail); (c) the hand-made rows of rows_restate.hand_made (segments of exactly 0, 1,
255, 256, 257, 512, 513 and 1500 samples, rows outside the table)."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from svox_t_amd import synth
from tests import depth_restate as D
from tests import rows_restate as R
from tests.util import Case, assert_grads_close

pytestmark = pytest.mark.gpu

CASES = {
    "d5_rgba4": dict(depth=5, K=4, data_format="RGBA", width=64, height=64),
    "d6_sh9": dict(depth=6, K=28, data_format="SH9", width=96, height=96),
}
_BUILT = {}


def real(name, gpu):
    """(case, tree on the GPU, renderer, the RaySamples of the case's rays with min_sigma = 0) -- marched once."""
    if name not in _BUILT:
        c = Case(**CASES[name])
        tree = c.tree(gpu)
        r = svox.VolumeRenderer(tree)
        _BUILT[name] = (c, tree, r, r.ray_samples(c.rays_gpu(gpu), min_sigma=0.0))
    return _BUILT[name]


def samples_of(row, gpu):
    """A RaySamples around a bare row array: one ray that owns every sample."""
    row = torch.as_tensor(row, dtype=torch.int32).to(gpu)
    T = row.shape[0]
    z = torch.zeros(T, device=gpu)
    return svox.RaySamples(torch.tensor([0, T], dtype=torch.int64, device=gpu), torch.zeros(T, dtype=torch.int32, device=gpu), row, z, z + 1)


def rows_input(which, gpu):
    """(row int32 numpy [T], M, K of the natural table) of the inputs a5, a6, b5, b6, c."""
    if which == "c":
        row, M, _ = R.hand_made()
        return row, M, 33
    name = "d5_rgba4" if which[1] == "5" else "d6_sh9"
    c, tree, _, s = real(name, gpu)
    row = s.row.cpu().numpy()
    if which[0] == "b":
        return (row % 13).astype(np.int32), 16, c.K                 # rows 13 .. 15 have no sample
    return row, tree.features.shape[0], c.K


INPUTS = ["a5", "a6", "b5", "b6", "c"]


# 1. the plan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", INPUTS)
def test_plan(gpu, which):
    row, M, _ = rows_input(which, gpu)
    s = samples_of(row, gpu)
    before = _C._extras.ROW_PLAN_BUILDS
    plan = s.row_plan(M)
    assert isinstance(plan, svox.RowPlan) and s.row_plan(M) is plan and _C._extras.ROW_PLAN_BUILDS == before + 1
    want = R.plan(row, M)
    row_ptr, perm = plan.row_ptr.cpu().numpy(), plan.perm.cpu().numpy()
    assert row_ptr.dtype == np.int32 and perm.dtype == np.int32 and row_ptr.shape == (M + 1,) and perm.shape == row.shape
    np.testing.assert_array_equal(row_ptr, want.row_ptr)
    np.testing.assert_array_equal(perm[:row_ptr[M]], want.perm[:want.row_ptr[M]])
    np.testing.assert_array_equal(np.sort(perm), np.arange(row.shape[0]))                   # the outside samples are behind, each once
    np.testing.assert_array_equal(plan.counts.cpu().numpy(), np.diff(want.row_ptr))
    assert plan.n_outside == want.n_outside and plan.longest == want.longest and plan.M == M and plan.T == row.shape[0]
    # the long rows: ascending, each with its chunks, every chunk naming its row
    counts = np.diff(want.row_ptr)
    long_rows = np.nonzero(counts > 256)[0]
    np.testing.assert_array_equal(plan.long_rows.cpu().numpy(), long_rows)
    chunks = -(-counts[long_rows] // 256)
    np.testing.assert_array_equal(plan.long_chunk_ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(chunks)]))
    np.testing.assert_array_equal(plan.chunk_long.cpu().numpy(), np.repeat(np.arange(long_rows.shape[0]), chunks))
    if which == "c":
        assert plan.n_outside == 13 and plan.longest == 1500 and long_rows.tolist() == [4, 5, 6, 7, 36]
    elif which[0] == "b":
        assert plan.longest > 1000 and long_rows.shape[0] == 13 and plan.n_outside == 0
    else:
        assert 1 <= plan.longest <= 256 and long_rows.shape[0] == 0 and plan.n_outside == 0 and row.shape[0] > 10000
    # another table height is another plan
    assert s.row_plan(M + 3) is not plan and s.row_plan(M + 3).M == M + 3 and s.row_plan(M) is plan


# 2. gather -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 28, 33])
def test_gather(gpu, K):
    rng = np.random.default_rng(10 + K)
    dims = [None, -1, slice(0, None, 2), [K - 1, 0] if K > 1 else [0], torch.tensor([K // 2])]
    for which in ("a5", "c"):
        row, M, _ = rows_input(which, gpu)
        s = samples_of(row, gpu)
        table = rng.standard_normal((M, K)).astype(np.float32)
        tg = torch.from_numpy(table).to(gpu)
        inside = (row >= 0) & (row < M)
        for dim in dims:
            out = svox.gather_rows(s, tg, dim=dim)
            cols = None if dim is None else np.arange(K)[dim.numpy() if isinstance(dim, torch.Tensor) else dim].reshape(-1)
            assert out.dtype == torch.float32 and out.shape == (row.shape[0], K if cols is None else cols.shape[0]) and not out.requires_grad
            got = out.cpu().numpy()
            np.testing.assert_array_equal(got, R.gather(table, row, cols))
            ref = tg[s.row.long()[torch.from_numpy(inside).to(gpu)]]             # torch indexing, on the rows it accepts
            np.testing.assert_array_equal(got[inside], ref.cpu().numpy() if cols is None else ref.cpu().numpy()[:, cols])
            if which == "c":
                assert (~inside).sum() == 13 and not got[~inside].any()
    # a table whose storage is not 16-byte aligned takes the other kernel: the same values
    row, M, _ = rows_input("c", gpu)
    s = samples_of(row, gpu)
    flat = torch.from_numpy(rng.standard_normal(M * 4 + 1).astype(np.float32)).to(gpu)
    off = flat[1:].view(M, 4)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    np.testing.assert_array_equal(svox.gather_rows(s, off).cpu().numpy(), R.gather(off.cpu().numpy(), row))


# 3. gather backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", INPUTS)
def test_gather_backward(gpu, which):
    row, M, K = rows_input(which, gpu)
    s = samples_of(row, gpu)
    T = row.shape[0]
    rng = np.random.default_rng(20)
    inside = (row >= 0) & (row < M)
    n = np.bincount(row[inside], minlength=M)[:, None]
    for dim in (None, [K - 1, 1] if K > 2 else [0]):
        cols = None if dim is None else np.asarray(dim)
        C = K if cols is None else cols.shape[0]
        g = (rng.standard_normal((T, C)) * np.exp(rng.uniform(-2, 2, (T, C)))).astype(np.float32)
        gg = torch.from_numpy(g).to(gpu)
        runs = []
        for _ in range(2):
            table = torch.zeros(M, K, device=gpu, requires_grad=True)
            svox.gather_rows(s, table, dim=dim).backward(gg)
            runs.append(table.grad.cpu().numpy())
        got = runs[0]
        assert got.tobytes() == runs[1].tobytes()
        np.testing.assert_array_equal(got, R.gather_grad(g, row, M, K, cols))
        want, mag = np.zeros((M, C)), np.zeros((M, C))
        np.add.at(want, row[inside], g[inside].astype(np.float64))
        np.add.at(mag, row[inside], np.abs(g[inside]).astype(np.float64))
        sel = got if cols is None else got[:, cols]
        assert np.all(np.abs(sel - want) <= R.gamma(n) * mag)
        assert not sel[n[:, 0] == 0].any() and (sel[n[:, 0] > 0] != 0).all()
        if cols is not None:
            assert not np.delete(got, cols, axis=1).any()
    assert (n == 0).sum() > 0 or which == "a5" or which == "a6"


def test_gather_backward_is_two_level(gpu):
    """The 2^24 row of tests/test_rows_host.py on the device: 16 777 260, not the sequential 16 777 216."""
    v = np.ones((300, 1), np.float32)
    v[0] = 2.0 ** 24
    s = samples_of(np.zeros(300, np.int32), gpu)
    table = torch.zeros(1, 1, device=gpu, requires_grad=True)
    svox.gather_rows(s, table).backward(torch.from_numpy(v).to(gpu))
    assert table.grad.item() == 16777260.0
    assert svox.reduce_rows(s, torch.from_numpy(v).to(gpu), 1).item() == 16777260.0
    # 256 of them are one chunk: sequential
    s = samples_of(np.zeros(256, np.int32), gpu)
    assert svox.reduce_rows(s, torch.from_numpy(v[:256, 0].copy()).to(gpu), 1).item() == 16777216.0


# 4. reductions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 28, 33])
@pytest.mark.parametrize("which", ["b5", "b6", "c"])
def test_reductions(gpu, which, C):
    row, M, _ = rows_input(which, gpu)
    s = samples_of(row, gpu)
    T = row.shape[0]
    rng = np.random.default_rng(30 + C)
    v = rng.standard_normal((T, C)).astype(np.float32)
    if C == 1:
        v = v[:, 0].copy()                                          # 1-D values: a 1-D result
    vg = torch.from_numpy(v).to(gpu)
    inside = (row >= 0) & (row < M)
    has = np.bincount(row[inside], minlength=M) > 0
    idx = torch.from_numpy(row[inside].astype(np.int64)).to(gpu)
    for op in ("sum", "mean", "max", "min"):
        out = svox.reduce_rows(s, vg, M, op, empty=-1.0)
        assert out.shape == ((M,) if C == 1 else (M, C)) and out.dtype == torch.float32 and not out.requires_grad
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got, R.reduce(v, row, M, op, empty=-1.0), err_msg=op)
        assert np.all(got[~has] == -1.0) and (~has).sum() in (2, 3) and not np.any(got[has] == -1.0)
        if op in ("max", "min"):
            ref = torch.zeros_like(out).index_reduce_(0, idx, vg[torch.from_numpy(inside).to(gpu)], "a" + op, include_self=False)
            np.testing.assert_array_equal(got[has], ref.cpu().numpy()[has])
    # the default `empty` is 0
    assert not svox.reduce_rows(s, vg, M, "max").cpu().numpy()[~has].any()


def test_a_nan_stays_in_its_row(gpu):
    row, M, sizes = R.hand_made()
    s = samples_of(row, gpu)
    rng = np.random.default_rng(40)
    v = rng.standard_normal((row.shape[0], 3)).astype(np.float32)
    long_k = int(np.nonzero(row == 7)[0][700])                      # the third chunk of the 1500-sample row
    short_k = int(np.nonzero(row == 2)[0][100])                     # a row of 255
    v[long_k, 1] = np.nan
    v[short_k, 2] = np.nan
    for op in ("sum", "mean", "max", "min"):
        got = svox.reduce_rows(s, torch.from_numpy(v).to(gpu), M, op).cpu().numpy()
        assert np.isnan(got[7, 1]) and np.isnan(got[2, 2]) and np.isnan(got).sum() == 2, op
        np.testing.assert_array_equal(got, R.reduce(v, row, M, op))


@pytest.mark.parametrize("which", ["b5", "c"])
def test_reduction_backward_is_the_gather(gpu, which):
    row, M, _ = rows_input(which, gpu)
    s = samples_of(row, gpu)
    T = row.shape[0]
    rng = np.random.default_rng(50)
    g = torch.from_numpy(rng.standard_normal((M, 3)).astype(np.float32)).to(gpu)
    counts = s.row_plan(M).counts
    for op in ("sum", "mean"):
        v = torch.from_numpy(rng.standard_normal((T, 3)).astype(np.float32)).to(gpu).requires_grad_(True)
        out = svox.reduce_rows(s, v, M, op)
        assert out.requires_grad
        out.backward(g)
        up = g if op == "sum" else g / counts.clamp(min=1).float()[:, None]
        np.testing.assert_array_equal(v.grad.cpu().numpy(), svox.gather_rows(s, up).cpu().numpy())
        np.testing.assert_array_equal(v.grad.cpu().numpy(), R.gather(up.cpu().numpy(), row))
        # 1-D values: a 1-D gradient
        v1 = torch.from_numpy(rng.standard_normal(T).astype(np.float32)).to(gpu).requires_grad_(True)
        svox.reduce_rows(s, v1, M, op).backward(g[:, 0].contiguous())
        np.testing.assert_array_equal(v1.grad.cpu().numpy(), R.gather(up.cpu().numpy()[:, :1], row)[:, 0])
    for op in ("max", "min"):
        v = torch.ones(T, 3, device=gpu, requires_grad=True)
        assert not svox.reduce_rows(s, v, M, op).requires_grad


# 5. end to end ---------------------------------------------------------------------------------------------------------
def test_end_to_end_gradient_is_the_depth_moments(gpu):
    """test_gpu_samples' end-to-end test with gather_rows in the place of torch indexing: the forward keeps its bits, the
    gradient reaches the table within the project's standing 1e-5 of the tight scale, and has the same bytes twice."""
    name = "d5_rgba4"
    c, tree, r, s = real(name, gpu)
    ot, rays, opt = c.oracle_tree(), c.rays_np(), c.oracle_opts()
    g = synth.grad_output(c.Q, 3, seed=31).numpy()
    gt = torch.from_numpy(g).to(gpu)
    runs = []
    for _ in range(2):
        tree.features.grad = None
        sigma = svox.gather_rows(s, tree.features, dim=-1)[:, 0]
        out, alpha, w = svox.composite(s, sigma, torch.stack([s.depth, s.depth * s.depth], dim=1))
        ((out * gt[:, :2]).sum() + (alpha * gt[:, 2]).sum()).backward()
        runs.append(tree.features.grad.cpu().numpy().copy())
    with torch.no_grad():
        np.testing.assert_array_equal(sigma.detach().cpu().numpy(), tree.features[s.row.long(), -1].cpu().numpy())
        np.testing.assert_array_equal(alpha.detach().cpu().numpy()[:, None], r.opacity_render(tree.features, c.rays_gpu(gpu)).cpu().numpy())
    got = runs[0]
    assert got.tobytes() == runs[1].tobytes()
    want, scale = D.moments_grad(ot, rays, opt, "entry", g), D.moments_grad_scale(ot, rays, opt, "entry", g)
    ratio = np.abs(got - want)[scale > 0] / (1e-5 * scale[scale > 0])
    print(name, "worst |err| / bound", ratio.max(), "entries", ratio.size)
    assert_grads_close(got, want, scale)
    assert np.all(got[:, :-1] == 0) and (got[:, -1] != 0).sum() > 500
    tree.features.grad = None


# 6. the weight map -----------------------------------------------------------------------------------------------------
def test_the_weight_map(gpu):
    c, tree, r, s = real("d5_rgba4", gpu)
    M = tree.features.shape[0]
    with torch.no_grad():
        w, _ = svox.sample_weights(s, svox.gather_rows(s, tree.features, dim=-1)[:, 0])
        wmax = svox.reduce_rows(s, w, M, "max")
        ref = torch.zeros(M, device=gpu).index_reduce_(0, s.row.long(), w, "amax", include_self=True)
    np.testing.assert_array_equal(wmax.cpu().numpy(), ref.cpu().numpy())
    assert wmax.shape == (M,) and (wmax > 0).sum() > 500
    # per slot
    spread = tree.spread_rows(wmax, empty=-1.0)
    assert spread.shape == tree.child.shape and spread.dtype == torch.float32
    words = tree.data[..., 0].long()
    leaf = (tree.child == 0) & (words >= 0) & (words < M)
    np.testing.assert_array_equal(spread[leaf].cpu().numpy(), wmax[words[leaf]].cpu().numpy())
    assert torch.all(spread[~leaf] == -1.0) and int(leaf.sum()) > 0 and int((~leaf).sum()) > 0
    # a shorter per-row array: the rows it does not cover are `empty`
    half = tree.spread_rows(wmax[:M // 2].contiguous(), empty=-2.0)
    low = leaf & (words < M // 2)
    np.testing.assert_array_equal(half[low].cpu().numpy(), wmax[words[low]].cpu().numpy())
    assert torch.all(half[~low] == -2.0)
    # what subdivide takes
    threshold = float(wmax[wmax > 0].median())
    grown = c.tree(gpu)
    before = grown.filled
    sel = (tree.spread_rows(wmax) >= threshold) & leaf
    res = grown.subdivide(weights=grown.spread_rows(wmax), threshold=threshold)
    assert res.nodes_added > 0 and grown.filled == before + res.nodes_added
    split = (tree.child[:before] == 0) & (grown.child[:before] != 0)           # leaves then, nodes now
    assert int(split.sum()) == res.nodes_added and torch.all(sel[:before][split])
    assert torch.all(wmax[words[:before][split]] >= threshold)


# 7. tiny ---------------------------------------------------------------------------------------------------------------
def test_tiny(gpu):
    table = torch.arange(12, dtype=torch.float32, device=gpu).reshape(3, 4).requires_grad_(True)
    # T = 0 (and Q = 0): empty outputs, `empty` in every row, a zero gradient
    s0 = svox.RaySamples(torch.zeros(1, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu),
                         torch.zeros(0, dtype=torch.int32, device=gpu), torch.zeros(0, device=gpu), torch.zeros(0, device=gpu))
    assert s0.Q == 0 and len(s0) == 0
    plan = s0.row_plan(3)
    assert plan.row_ptr.tolist() == [0, 0, 0, 0] and plan.perm.shape == (0,) and plan.n_outside == 0 and plan.longest == 0
    out = svox.gather_rows(s0, table)
    assert out.shape == (0, 4)
    out.sum().backward()
    assert table.grad.shape == (3, 4) and not table.grad.any()
    for op in ("sum", "mean", "max", "min"):
        assert svox.reduce_rows(s0, torch.zeros(0, 2, device=gpu), 3, op, empty=7.0).tolist() == [[7.0, 7.0]] * 3
        assert svox.reduce_rows(s0, torch.zeros(0, device=gpu), 3, op).tolist() == [0.0] * 3
    assert svox.reduce_rows(s0, torch.zeros(0, 2, device=gpu), 0).shape == (0, 2)
    # M = 1
    s = samples_of([0, 0, 5, 0], gpu)
    p1 = s.row_plan(1)
    assert p1.row_ptr.tolist() == [0, 3] and p1.perm.tolist()[:3] == [0, 1, 3] and p1.n_outside == 1 and p1.longest == 3
    v = torch.tensor([1.0, 2.0, 100.0, 4.0], device=gpu)
    assert svox.reduce_rows(s, v, 1).tolist() == [7.0] and svox.reduce_rows(s, v, 1, "max").tolist() == [4.0]
    assert svox.reduce_rows(s, v, 1, "mean").item() == np.float32(7.0) / np.float32(3.0)
    # M = 0: everything is outside
    p0 = s.row_plan(0)
    assert p0.row_ptr.tolist() == [0] and p0.n_outside == 4 and p0.longest == 0
    assert svox.reduce_rows(s, v, 0).shape == (0,)
    assert not svox.gather_rows(s, torch.zeros(0, 2, device=gpu)).any()
    # T = 1
    s1 = samples_of([2], gpu)
    assert svox.gather_rows(s1, table).tolist() == [[8.0, 9.0, 10.0, 11.0]]
    assert svox.reduce_rows(s1, torch.tensor([[3.0, -0.0]], device=gpu), 3, "sum", empty=-1.0).tolist() == [[-1.0, -1.0], [-1.0, -1.0], [3.0, 0.0]]
    # a table taller than any row named
    tall = s.row_plan(1000)
    assert tall.row_ptr.shape == (1001,) and tall.n_outside == 0 and tall.counts.sum().item() == 4 and tall.counts[5].item() == 1
    out = svox.reduce_rows(s, v, 1000, "min", empty=-3.0)
    assert out[0].item() == 1.0 and out[5].item() == 100.0 and torch.all(out[6:] == -3.0) and torch.all(out[1:5] == -3.0)
