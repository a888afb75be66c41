"""ray_scan, ray_quantile and RaySamples.select on the GPU, bit for bit against the restatement (tests/scan_restate.py)
and against the operators they are tied to (accumulate, sample_weights, ray_samples(min_sigma=0))."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import samples_restate as R
from tests import scan_restate as S
from tests.test_gpu_samples import as_lists, assert_lists_equal, built, lists_of     # (their cache: one march per case and session)

pytestmark = pytest.mark.gpu

# Hand-made lists: 131 rays (no multiple of 64) whose lengths cycle through the sizes at which a lane-per-(ray, channel)
# walk can go wrong -- empty rays at the start, inside and at the end, one and two samples, a wavefront's 64 and its
# neighbours, lists longer than a workgroup's 256 lanes and than 1024.  T = 19 760.
LENGTHS = (0, 1, 2, 63, 64, 65, 0, 0, 300, 1025)
Q_HAND = 131
_HAND = {}


def hand():
    if not _HAND:
        counts = np.array([LENGTHS[q % len(LENGTHS)] for q in range(Q_HAND)])
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        T = int(offsets[-1])
        rng = np.random.default_rng(7)
        ray = np.repeat(np.arange(Q_HAND), counts).astype(np.int32)
        length = rng.uniform(0.01, 0.05, T).astype(np.float32)
        depth = (np.cumsum(length) - length).astype(np.float32)
        _HAND["L"] = R.Lists(offsets, rng.integers(0, 500, T).astype(np.int32), ray, depth, length)
        assert counts[0] == 0 and counts[-1] == 0 and counts.max() == 1025 and T == 19760
    return _HAND["L"]


def on_gpu(L, gpu):
    return svox.RaySamples(*(torch.from_numpy(np.ascontiguousarray(x)).to(gpu) for x in (L.offsets, L.ray, L.row, L.depth, L.length)))


def hostile_values(op, C, seed):
    T = hand().row.shape[0]
    rng = np.random.default_rng(seed)
    if op == "prod":
        v = rng.uniform(0.5, 1.5, (T, C)).astype(np.float32)         # (the product of 1025 of them stays a normal float32)
        v[rng.choice(T, 40, replace=False), rng.integers(0, C, 40)] = 0.0
        v[hand().offsets[9] + 500, 0] = 0.0                           # ... one inside a ray of 1025
    else:
        v = rng.standard_normal((T, C)).astype(np.float32)
    if op in ("max", "min"):
        v[::9] = v[3::9][: v[::9].shape[0]]                           # ties
        v[5::31] = np.nan
        v[11::53] = np.inf
        v[17::59] = -np.inf
        o = hand().offsets
        v[o[8]:o[8] + 3] = np.nan                                     # a ray of 300 that starts with NaNs
        v[o[3]:o[4]] = np.nan                                         # a ray of 63 that takes nothing at all
    return v, rng.standard_normal((T, C)).astype(np.float32)


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def assert_same_bits(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, what
    np.testing.assert_array_equal(g, w, err_msg=what)


# ray_scan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("op", S.OPS)
def test_scan_bits_on_hand_made_lists(gpu, op, C):
    """Every exclusive / reverse combination, forward and backward: the float32 restatement's bits."""
    L = hand()
    s = on_gpu(L, gpu)
    v, g = hostile_values(op, C, 100 + C)
    gt = torch.from_numpy(g).to(gpu)
    for exclusive in (False, True):
        for reverse in (False, True):
            what = f"{op} C={C} exclusive={exclusive} reverse={reverse}"
            vt = torch.from_numpy(v).to(gpu).requires_grad_(True)
            out = svox.ray_scan(s, vt, op, exclusive=exclusive, reverse=reverse)
            want = S.scan(v, L.offsets, op, exclusive, reverse)
            assert out.shape == (v.shape[0], C) and out.dtype == torch.float32
            assert_same_bits(out, want, what)
            out.backward(gt)
            got = vt.grad.cpu().numpy()
            assert_same_bits(got, S.scan_backward(v, L.offsets, op, exclusive, reverse, g), what + " backward")
            if op == "prod":
                assert np.all(np.isfinite(got)) and (v == 0).sum() >= 30 and (got != 0).sum() > 1000
            if op in ("max", "min"):
                # mass: the g of every position that took a value arrives somewhere, nothing else does; sums of at most
                # 1025 float32 terms: n 2^-24 sum|g|
                took = want != np.float32(S.IDENTITY[op])
                assert not np.isnan(want).any() and 0 < (~took).sum() < took.sum()
                live = np.where(took, g, 0).astype(np.float64)
                assert np.all(np.abs(got.astype(np.float64).sum(0) - live.sum(0)) <= 1025 * 2.0 ** -24 * np.abs(live).sum(0))
                assert np.all(got[np.isnan(v)] == 0)
    if C == 1:                                          # a flat [T] tensor is its [T, 1] form
        flat = svox.ray_scan(s, torch.from_numpy(v[:, 0].copy()).to(gpu), op, exclusive=True, reverse=True)
        assert flat.shape == (v.shape[0],)
        assert_same_bits(flat, want[:, 0])


def d5(gpu):
    c, ot, rays, opt = built("d5_rgba4")
    tree = c.tree(gpu)
    return c, ot, tree, svox.VolumeRenderer(tree), c.rays_gpu(gpu)


def test_scan_anchors(gpu):
    """On the 64 x 64 case: a ray's last inclusive sum of w is accumulate(samples, w); the exclusive product of the
    restatement's attenuations, stepped once more, is 1 - alpha, and times (1 - att) it is w -- all bit for bit."""
    c, ot, tree, r, rg = d5(gpu)
    with torch.no_grad():
        s = r.ray_samples(rg)
        sigma = tree.features[s.row.long(), -1].contiguous()
        w, alpha = svox.sample_weights(s, sigma)
        total = svox.accumulate(s, w)
        run = svox.ray_scan(s, w)
    counts = s.counts.cpu().numpy()
    last = (s.offsets[1:] - 1).cpu().numpy()
    have = counts > 0
    want = np.where(have, run.cpu().numpy()[np.where(have, last, 0)], np.float32(0))
    assert_same_bits(total, want.astype(np.float32))
    assert have.sum() > 1000 and counts.max() > 10
    L = lists_of("d5_rgba4")
    sg = ot.features[L.row, -1]
    att = np.where(sg > 0, O.expf(-(L.length * sg)), np.float32(1)).astype(np.float32)
    at = torch.from_numpy(att).to(gpu)
    with torch.no_grad():
        before = svox.ray_scan(s, at, "prod", exclusive=True)
        after = svox.ray_scan(s, at, "prod")
    assert_same_bits(before * at, after)                                              # the step
    end = np.where(have, after.cpu().numpy()[np.where(have, last, 0)], np.float32(1)).astype(np.float32)
    assert_same_bits(np.float32(1) - end, alpha)
    assert_same_bits(torch.where(sigma > 0, before * (1 - at), torch.zeros_like(at)), w)
    assert (alpha > 0).sum() > 500


# ray_quantile -----------------------------------------------------------------------------------------------------------
def hostile_weights(seed=9):
    T = hand().row.shape[0]
    rng = np.random.default_rng(seed)
    w = rng.uniform(0, 0.02, T).astype(np.float32)                   # (a ray of 63 sums to ~ 0.6, one of 300 passes 1)
    w[::4] = 0
    w[1::7] = -1.0
    w[2::13] = np.nan
    o = hand().offsets
    w[o[13]:o[14]] = 0                                                # a ray of 63 without a positive weight
    return w


@pytest.mark.parametrize("normalize", [True, False])
def test_quantile_is_the_restatements(gpu, normalize):
    L = hand()
    s = on_gpu(L, gpu)
    w = hostile_weights()
    q = [0.0, 0.25, 0.5, 1.0]
    wt = torch.from_numpy(w).to(gpu)
    index, frac = svox.ray_quantile(s, wt, q, normalize=normalize)
    want_i, want_f = S.quantile(w, L.offsets, q, normalize)
    assert index.dtype == torch.int64 and frac.dtype == torch.float32 and index.shape == frac.shape == (Q_HAND, 4)
    np.testing.assert_array_equal(index.cpu().numpy(), want_i)
    assert_same_bits(frac, want_f)
    hit = want_i >= 0
    assert 50 < hit.sum() < hit.size and (want_f > 0).sum() > 50 and not hit[13].any() and np.all(w[want_i[hit]] > 0)
    if not normalize:
        assert hit[:, 0].sum() > hit[:, 3].sum() > 0                                   # short rays never reach 1
    # q as a tensor, and a single quantile
    i2, f2 = svox.ray_quantile(s, wt, torch.tensor(q, device=gpu), normalize=normalize)
    assert torch.equal(i2, index) and torch.equal(f2, frac)
    i1, f1 = svox.ray_quantile(s, wt, 0.5, normalize=normalize)
    assert torch.equal(i1[:, 0], index[:, 2]) and torch.equal(f1[:, 0], frac[:, 2])
    # the depth: inside its sample
    z = svox.quantile_depth(s, wt, q, normalize=normalize)
    at = index.clamp(min=0)
    inside = (z >= s.depth[at]) & (z <= s.depth[at] + s.length[at])
    assert z.shape == (Q_HAND, 4) and bool((inside | (index < 0)).all()) and bool(torch.isnan(z[index < 0]).all())
    assert bool((svox.quantile_depth(s, wt, q, normalize=normalize, empty=-7.0)[index < 0] == -7.0).all())


def test_quantile_of_rays_that_all_miss(gpu):
    Q = 200
    s = svox.RaySamples(torch.zeros(Q + 1, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu),
                        torch.zeros(0, dtype=torch.int32, device=gpu), torch.zeros(0, device=gpu), torch.zeros(0, device=gpu))
    index, frac = svox.ray_quantile(s, torch.zeros(0, device=gpu), [0.0, 0.5, 1.0])
    assert index.shape == frac.shape == (Q, 3) and bool((index == -1).all()) and not frac.any()
    assert bool(torch.isnan(svox.quantile_depth(s, torch.zeros(0, device=gpu), 0.5)).all())
    v = torch.zeros(0, 2, device=gpu, requires_grad=True)
    out = svox.ray_scan(s, v, "prod", exclusive=True)
    out.sum().backward()
    assert out.shape == (0, 2) and v.grad.shape == (0, 2)
    # weights that are all zero, negative or NaN on real lists
    sh = on_gpu(hand(), gpu)
    w = torch.from_numpy(np.where(hostile_weights() > 0, np.float32(0), hostile_weights())).to(gpu)
    index, frac = svox.ray_quantile(sh, w, [0.0, 1.0])
    assert bool((index == -1).all()) and not frac.any()


# select -----------------------------------------------------------------------------------------------------------------
def test_select_positive_sigma_is_the_filtered_march(gpu):
    """select(sigma > 0) of the unfiltered lists: ray_samples(min_sigma=0.0) array for array, floats included; and
    sample_weights / accumulate on the subset with sigma[index] have the bits they have on the filtered lists."""
    c, ot, tree, r, rg = d5(gpu)
    f = tree.features.detach()
    with torch.no_grad():
        every, pos = r.ray_samples(rg), r.ray_samples(rg, min_sigma=0.0)
        sigma = f[every.row.long(), -1].contiguous()
        sel, index = every.select(sigma > 0)
        assert isinstance(sel, svox.RaySamples) and index.dtype == torch.int64 and 1000 < len(sel) < len(every)
        assert_lists_equal(as_lists(sel), as_lists(pos))
        assert_lists_equal(as_lists(sel), lists_of("d5_rgba4", 0.0))
        assert torch.equal(index, torch.nonzero(sigma > 0)[:, 0])
        values = torch.stack([every.depth, every.depth * every.depth, every.length], dim=1)
        w_sel, a_sel = svox.sample_weights(sel, sigma[index])
        w_pos, a_pos = svox.sample_weights(pos, f[pos.row.long(), -1].contiguous())
        assert_same_bits(w_sel, w_pos)
        assert_same_bits(a_sel, a_pos)
        assert_same_bits(svox.accumulate(sel, w_sel, values[index]), svox.accumulate(pos, w_pos, torch.stack([pos.depth, pos.depth * pos.depth, pos.length], dim=1)))
    # gradients flow through torch's indexing
    sg = sigma.clone().requires_grad_(True)
    w, alpha = svox.sample_weights(sel, sg[index])
    (w.sum() + alpha.sum()).backward()
    assert bool((sg.grad[sigma <= 0] == 0).all()) and int((sg.grad != 0).sum()) > 1000


def test_select_edge_cases(gpu):
    L = hand()
    s = on_gpu(L, gpu)
    T = len(s)
    builds = _C._extras.ROW_PLAN_BUILDS
    s.row_plan(500)
    full, index = s.select(torch.ones(T, dtype=torch.bool, device=gpu))
    assert_lists_equal(as_lists(full), L)
    assert torch.equal(index, torch.arange(T, device=gpu)) and "_row_plans" not in full.__dict__
    plan = full.row_plan(500)                                         # built for the new lists, not carried over
    assert _C._extras.ROW_PLAN_BUILDS == builds + 2 and plan.T == T
    # a hostile mask on the hand-made lists
    keep = np.random.default_rng(3).random(T) < 0.4
    keep[L.offsets[9]:L.offsets[10]] = False                          # a ray of 1025 becomes empty
    keep[L.offsets[8]:L.offsets[9]] = True
    sub, index = s.select(torch.from_numpy(keep).to(gpu))
    want = S.select(keep, L.offsets, L.ray, L.row, L.depth, L.length)
    assert_lists_equal(as_lists(sub), R.Lists(want[0], want[2], want[1], want[3], want[4]))
    np.testing.assert_array_equal(index.cpu().numpy(), want[5])
    assert sub.Q == Q_HAND and int(sub.counts[9]) == 0 and int(sub.counts[8]) == 300 and sub.row_plan(500).T == len(sub)
    # nothing kept: valid empty lists that every operator of the family accepts
    none, index = s.select(torch.zeros(T, dtype=torch.bool, device=gpu))
    assert len(none) == 0 and none.Q == Q_HAND and none.offsets.shape == (Q_HAND + 1,) and not none.offsets.any() and index.shape == (0,)
    assert none.row.shape == none.ray.shape == none.depth.shape == none.length.shape == (0,)
    e1, e2 = torch.zeros(0, device=gpu, requires_grad=True), torch.zeros(0, 3, device=gpu, requires_grad=True)
    w, alpha = svox.sample_weights(none, e1)
    out = svox.accumulate(none, w, e2)
    run = svox.ray_scan(none, e2, "max", reverse=True)
    (out.sum() + alpha.sum() + run.sum()).backward()
    assert alpha.shape == (Q_HAND,) and out.shape == (Q_HAND, 3) and run.shape == (0, 3) and not alpha.any() and not out.any()
    assert bool((svox.ray_quantile(none, e1.detach(), [0.5])[0] == -1).all())
    table = torch.ones(7, 4, device=gpu, requires_grad=True)
    rows = svox.gather_rows(none, table)
    assert rows.shape == (0, 4) and svox.reduce_rows(none, rows, 7).shape == (7, 4) and not svox.reduce_rows(none, rows, 7).any()
    again, idx = none.select(torch.zeros(0, dtype=torch.bool, device=gpu))
    assert len(again) == 0 and again.Q == Q_HAND and idx.shape == (0,) and none.row_plan(7).T == 0
    c, ot, tree, r, rg = d5(gpu)
    rgb, sig = r.shade_samples(none, tree.features)
    assert rgb.shape[0] == 0 and sig.shape == (0,)


@pytest.mark.parametrize("Q", [1, 65])
def test_select_on_tiny_batches(gpu, Q):
    c, ot, tree, r, _ = d5(gpu)
    rays = built("d5_rgba4")[2]
    pick = (np.arange(Q) * 37 + 64 * 30 + 20) % 4096                  # the batches of test_tiny_batches
    rg = svox.Rays(*(torch.from_numpy(np.ascontiguousarray(a[pick])).to(gpu) for a in rays))
    every, pos = r.ray_samples(rg), r.ray_samples(rg, min_sigma=0.0)
    sel, index = every.select(tree.features.detach()[every.row.long(), -1] > 0)
    assert sel.Q == Q and 0 < len(sel) <= len(every) and sel.offsets.shape == (Q + 1,)
    assert_lists_equal(as_lists(sel), as_lists(pos))
    assert torch.equal(every.row[index], sel.row)


# placement and determinism ----------------------------------------------------------------------------------------------
def shifted(t, gpu):
    """The values of t as a contiguous view that starts 4 bytes (int64: 8; bool: 1) behind a 16-byte boundary."""
    t = torch.as_tensor(t).to(gpu)
    n = t.numel()
    buf = torch.zeros(n + 8, dtype=t.dtype, device=gpu)
    view = buf[1:1 + n].view(t.shape)
    view.copy_(t)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == t.element_size() % 16 and view.is_contiguous()
    return view


def test_placement_changes_nothing(gpu):
    L = hand()
    s = on_gpu(L, gpu)
    s2 = svox.RaySamples(*(shifted(torch.from_numpy(np.ascontiguousarray(x)), gpu) for x in (L.offsets, L.ray, L.row, L.depth, L.length)))
    for op in S.OPS:
        v, g = hostile_values(op, 3, 200)
        a = torch.from_numpy(v).to(gpu).requires_grad_(True)
        b = shifted(torch.from_numpy(v), gpu).requires_grad_(True)
        oa = svox.ray_scan(s, a, op, exclusive=True, reverse=True)
        ob = svox.ray_scan(s2, b, op, exclusive=True, reverse=True)
        assert_same_bits(oa, ob, op)
        oa.backward(torch.from_numpy(g).to(gpu))
        ob.backward(shifted(torch.from_numpy(g), gpu))
        assert_same_bits(a.grad, b.grad, op + " backward")
    w = hostile_weights()
    q = [0.0, 0.25, 0.5, 1.0]
    ia, fa = svox.ray_quantile(s, torch.from_numpy(w).to(gpu), q)
    ib, fb = svox.ray_quantile(s2, shifted(torch.from_numpy(w), gpu), shifted(torch.tensor(q), gpu))
    assert torch.equal(ia, ib)
    assert_same_bits(fa, fb)
    keep = torch.from_numpy(np.random.default_rng(4).random(len(s)) < 0.5)
    k2 = shifted(keep, gpu)
    assert k2.data_ptr() % 2 == 1
    (sa, xa), (sb, xb) = s.select(keep.to(gpu)), s2.select(k2)
    assert_lists_equal(as_lists(sa), as_lists(sb))
    assert torch.equal(xa, xb) and 0 < len(sa) < len(s)


def test_two_runs_give_the_same_bits(gpu):
    L = hand()
    s = on_gpu(L, gpu)
    runs = []
    for _ in range(2):
        got = []
        for op in S.OPS:
            v, g = hostile_values(op, 5, 300)
            vt = torch.from_numpy(v).to(gpu).requires_grad_(True)
            for exclusive, reverse in ((False, False), (True, True)):
                vt.grad = None
                out = svox.ray_scan(s, vt, op, exclusive=exclusive, reverse=reverse)
                out.backward(torch.from_numpy(g).to(gpu))
                got += [bits(out), bits(vt.grad)]
        wt = torch.from_numpy(hostile_weights()).to(gpu)
        for normalize in (True, False):
            index, frac = svox.ray_quantile(s, wt, [0.0, 0.25, 0.5, 1.0], normalize=normalize)
            got += [index.cpu().numpy(), bits(frac)]
        sub, index = s.select(wt > 0.01)
        got += [bits(x) for x in (sub.offsets, sub.ray, sub.row, sub.depth, sub.length, index)]
        runs.append(got)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert len(runs[0]) == 26
