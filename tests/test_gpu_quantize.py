"""quantize_median_cut on the GPU (csrc/svoxt_quant.hip): against the reference's own recorded outputs
(tests/golden/quantize_*.npz, the criteria of tests/test_quantize_host.py), against the numpy restatement at sizes the
fixtures do not reach, under heavy ties, for determinism, and through N3Tree.quantize."""
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from svox_t_amd import synth
from tests import quantize_restate as R
from tests.test_quantize_host import FIXTURES, G, check_against_fixture
from tests.util import Case, assert_grads_close

pytestmark = pytest.mark.gpu


def run(gpu, data, weights, order):
    w = torch.from_numpy(weights).to(gpu) if weights is not None else torch.empty(0, device=gpu)
    colors, ids = _C.quantize_median_cut(torch.from_numpy(data).to(gpu), w, order)
    assert colors.dtype == torch.float32 and ids.dtype == torch.int32
    return colors.cpu().numpy(), ids.cpu().numpy()


def check_against_restatement(gpu, data, weights, order):
    """Ids exactly the restatement's; colours within 1 ulp of the float32 rounding of its float64 mean."""
    want, want_ids, *_ = R.quantize(data, weights, order)
    got, ids = run(gpu, data, weights, order)
    np.testing.assert_array_equal(ids, want_ids)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    print(f"max err in ulp = {(err / ulp).max():.2f}")
    assert got.shape == want.shape and (err <= ulp).all()


def table(M, K, seed):
    return np.random.default_rng(seed).standard_normal((M, K)).astype(np.float32)


def dyadic_weights(M, seed):
    """k / 1024, k an integer in [0, 4096]: every float64 sum of them is exact, whatever its shape."""
    return (np.random.default_rng(seed).integers(0, 4097, M) / 1024.0).astype(np.float32)


@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_equals_the_reference(gpu, name):
    g = np.load(os.path.join(G, name))
    colors, ids = run(gpu, g["data"], g["weights"] if len(g["weights"]) else None, int(g["order"]))
    check_against_fixture(g, colors, ids)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("order", [0, 1, 12, 16])
@pytest.mark.parametrize("K", [4, 28, 32])
def test_gpu_equals_the_restatement(gpu, K, order, weighted):
    M = 200_000
    check_against_restatement(gpu, table(M, K, K + order), dyadic_weights(M, order) if weighted else None, order)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("K,order", [(4, 12), (28, 10), (1, 16)])
def test_as_many_colours_as_rows(gpu, K, order, weighted):
    M = 1 << order
    check_against_restatement(gpu, table(M, K, order), dyadic_weights(M, K) if weighted else None, order)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_heavy_ties(gpu, weighted):
    """8 levels a column and some -0.0 / +0.0: nearly every cut falls inside a run of equal values, so the ids are
    right only if the order within a segment is (value, row index) with the two zeros equal."""
    M, K = 100_000, 6
    rng = np.random.default_rng(11)
    data = (rng.integers(-4, 4, (M, K)) / 4.0).astype(np.float32)
    data[(data == 0) & (rng.random((M, K)) < 0.5)] = -0.0
    assert np.signbit(data[data == 0]).any() and not np.signbit(data[data == 0]).all()
    check_against_restatement(gpu, data, dyadic_weights(M, 3) if weighted else None, 14)


def test_two_calls_give_identical_bits(gpu):
    data = torch.from_numpy(table(150_000, 28, 5)).to(gpu)
    w = torch.from_numpy(dyadic_weights(150_000, 6) * np.float32(1.1)).to(gpu)          # inexact sums too
    for weights in (None, w):
        a = svox.quantize_median_cut(data, 13, weights=weights)
        b = svox.quantize_median_cut(data, 13, weights=weights)
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_tree_quantize(gpu):
    """Shell tree of depth 5, SH9.  The quantised tree with its palette renders, bit for bit, what the original tree
    renders from the expanded table colors[color_id_map]; the palette's gradient is the expanded table's, added up by
    colour."""
    c = Case(depth=5, K=28, data_format="SH9", width=64, height=64)
    orig, tree = c.tree(gpu), c.tree(gpu)
    M = orig.features.shape[0]
    order = 8
    child, pd, data = tree.child.clone(), tree.parent_depth.clone(), tree.data.clone()
    res = tree.quantize(order)
    assert isinstance(res, svox.svox.QuantizeResult)
    assert res.colors.shape == (1 << order, 28) and res.color_id_map.shape == (M,)
    assert isinstance(tree.features, torch.nn.Parameter) and torch.equal(tree.features.detach(), res.colors)
    assert torch.equal(tree.child, child) and torch.equal(tree.parent_depth, pd)
    named = (data.view(-1).long() & 0xFFFFFFFF) < M
    assert bool(named.any()) and not bool(named.all())                   # the shell tree has empty leaves
    assert bool((tree.data.view(-1)[~named] == svox.svox.EMPTY_INDEX).all()) and torch.equal(tree.data.view(-1)[~named], data.view(-1)[~named])
    assert torch.equal(tree.data.view(-1)[named].long(), res.color_id_map.long()[data.view(-1)[named].long()])
    want_colors, want_ids, *_ = R.quantize(c.features.numpy(), None, order)
    np.testing.assert_array_equal(res.color_id_map.cpu().numpy(), want_ids)

    expanded = torch.nn.Parameter(res.colors[res.color_id_map.long()].contiguous())
    rays = c.rays_gpu(gpu)
    r_q, r_o = svox.VolumeRenderer(tree), svox.VolumeRenderer(orig)
    out_q, out_o = r_q(tree.features, rays), r_o(expanded, rays)
    assert torch.equal(out_q.view(torch.int32), out_o.view(torch.int32)) and float(out_q.detach()[:, -1].max()) > 0.5
    with torch.no_grad():
        for call in ("render_depth", "opacity_render"):
            a, b = getattr(r_q, call)(tree.features, rays), getattr(r_o, call)(expanded, rays)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), call
    go = synth.grad_output(c.Q, out_q.shape[1], seed=3).to(gpu)
    out_q.backward(go)
    out_o.backward(go)
    ids = res.color_id_map.long()
    want = torch.zeros_like(res.colors, dtype=torch.float64).index_add_(0, ids, expanded.grad.double())
    abs_sum = torch.zeros_like(res.colors, dtype=torch.float64).index_add_(0, ids, expanded.grad.double().abs())
    assert float(abs_sum.max()) > 0
    assert_grads_close(tree.features.grad.cpu().numpy(), want.cpu().numpy(), abs_sum.cpu().numpy(), what="palette grad")

    with tree.accumulate_weights():
        with pytest.raises(RuntimeError, match="Tree locked"):
            tree.quantize(4)
    # weighted, with the per-row weights of a render
    tree2 = c.tree(gpu)
    r2 = svox.VolumeRenderer(tree2)
    with tree2.accumulate_weights() as accum:
        with torch.no_grad():
            r2(tree2.features, rays)
    n = tree2.n_internal
    words = tree2.data[:n, ..., 0]
    leaf = (tree2.child[:n] == 0) & (words >= 0) & (words < M)
    w = torch.zeros(M, device=gpu)
    w[words[leaf].long()] = accum.value[:n][leaf]
    res2 = tree2.quantize(order, weights=w)
    ids2 = res2.color_id_map
    assert int(ids2.min()) >= 0 and int(ids2.max()) < 1 << order and bool(torch.isfinite(res2.colors).all())
    assert float(w.max()) > 0 and not torch.equal(ids2, res.color_id_map)           # the weights moved the cuts
