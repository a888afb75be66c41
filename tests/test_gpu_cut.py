"""RaySamples.split and merge_samples on the GPU, bit for bit against the restatement (tests/cut_restate.py), and the
composite of two trees along shared rays against the operators it is built from."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
from tests import cut_restate as X
from tests import samples_restate as R
from tests.test_gpu_samples import as_lists, built, lists_of                     # (their cache: one march per case and session)
from tests.test_gpu_scan import LENGTHS, Q_HAND, assert_same_bits, hand, on_gpu

pytestmark = pytest.mark.gpu
F = np.float32
NAN = F(np.nan)
_MADE = {}


def ends(L):
    return (L.depth + L.length).astype(F)


def hand_a():
    """The hand-made lists of tests/test_gpu_scan.py (131 rays, T = 19 760) with a few samples made degenerate in rays
    of 300 and 65: length 0, negative and NaN, and a NaN depth."""
    if "a" not in _MADE:
        L = hand()
        depth, length = L.depth.copy(), L.length.copy()
        for q, at in ((8, 0), (28, 296), (68, 150), (58, 10), (45, 30), (5, 30)):
            k = int(L.offsets[q]) + at
            length[k:k + 3] = (0.0, -0.02, NAN)
            depth[k + 3], length[k + 3] = NAN, NAN
        _MADE["a"] = L._replace(depth=depth, length=length)
    return _MADE["a"]


def hand_b():
    """(lists, witnesses): a second list over the same 131 rays.  Rays without a sample in A: B empty (q % 10 in {0, 7}) or
    full (6).  The others, by decade d = q // 10:
        d % 7 == 0  B empty                         4  equal starts, different ends (longer, then shorter), degenerate samples
                 1  B identical to A                5  one B sample spanning the whole ray
                 2  one B sample nested in A's first, and degenerate samples (length 0, negative, NaN; NaN depth)
                 3  B abuts A exactly: from the end of A's first sample, and from the end of its last
                 6  B = A moved on by 0.4 of each sample's length: the general case
    witnesses[kind] = [(ray, sample of A, sample of B)] (a sample is -1 where the kind has none)."""
    if "b" in _MADE:
        return _MADE["b"]
    A = hand_a()
    ea = ends(A)
    depth, length, counts = [], [], []
    wit = {k: [] for k in ("empty_empty", "empty_full", "full_empty", "identical", "nested", "abut", "equal_start", "span", "shifted",
                           "degenerate")}

    def put(z, d):
        depth.append(F(z))
        length.append(F(d))
        return len(depth) - 1

    for q in range(Q_HAND):
        lo, hi = int(A.offsets[q]), int(A.offsets[q + 1])
        before = len(depth)
        mode = (q // 10) % 7
        if lo == hi:
            if q % 10 == 6:
                for j in range(5):
                    put(0.5 + 0.25 * j, 0.125)
                wit["empty_full"].append((q, -1, before))
            else:
                wit["empty_empty"].append((q, -1, -1))
        elif mode == 0:
            wit["full_empty"].append((q, lo, -1))
        elif mode == 1:
            for k in range(lo, hi):
                put(A.depth[k], A.length[k])
            wit["identical"].append((q, lo, before))
        elif mode == 2:
            wit["degenerate"].append((q, lo, put(A.depth[lo] - F(1.0), 0.0)))
            put(A.depth[lo] - F(1.0), -0.5)
            wit["nested"].append((q, lo, put(A.depth[lo] + F(0.25) * A.length[lo], F(0.5) * A.length[lo])))
            put(A.depth[lo] + F(0.5) * A.length[lo], NAN)
            put(NAN, 0.01)
        elif mode == 3:
            wit["abut"].append((q, lo, put(ea[lo], F(0.4) * A.length[lo])))
            if hi - lo > 1:
                wit["abut"].append((q, hi - 1, put(ea[hi - 1], 0.03)))
        elif mode == 4:
            wit["equal_start"].append((q, lo, put(A.depth[lo], F(1.5) * A.length[lo])))
            put(ea[lo] + A.length[lo], 0.0)
            if hi - lo > 3:
                wit["equal_start"].append((q, lo + 3, put(A.depth[lo + 3], F(0.5) * A.length[lo + 3])))
        elif mode == 5:
            first = next(k for k in range(lo, hi) if A.length[k] > 0)
            wit["span"].append((q, lo, put(A.depth[first] - F(0.01), (np.nanmax(ea[lo:hi]) - A.depth[first]) + F(0.02))))
        else:
            for k in range(lo, hi):
                if A.length[k] > 0:
                    put(A.depth[k] + F(0.4) * A.length[k], F(0.9) * A.length[k])
            wit["shifted"].append((q, lo, before))
        counts.append(len(depth) - before)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    T = int(offsets[-1])
    rng = np.random.default_rng(8)
    B = R.Lists(offsets, rng.integers(0, 500, T).astype(np.int32), np.repeat(np.arange(Q_HAND), counts).astype(np.int32),
                np.array(depth, dtype=F), np.array(length, dtype=F))
    _MADE["b"] = (B, wit)
    return _MADE["b"]


def hand_merge():
    if "m" not in _MADE:
        _MADE["m"] = X.merge(hand_a(), hand_b()[0])
    return _MADE["m"]


def empty_like(L):
    Q = len(L.offsets) - 1
    return R.Lists(np.zeros(Q + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=F), np.zeros(0, dtype=F))


def assert_merge_bits(got, want, what=""):
    (m, ia, ib), (wm, wia, wib) = got, want
    assert m.offsets.dtype == torch.int64 and ia.dtype == torch.int64 and ib.dtype == torch.int64
    for g, w, name in zip(as_lists(m), wm, R.Lists._fields):
        assert_same_bits(g, w, f"{what} {name}")
    assert_same_bits(ia, wia, what + " index_a")
    assert_same_bits(ib, wib, what + " index_b")
    assert not hasattr(m, "_row_plans")


def test_every_pairing_is_present():
    A, (B, wit) = hand_a(), hand_b()
    ea, eb = ends(A), ends(B)
    na, nb = np.diff(A.offsets), np.diff(B.offsets)
    assert all(len(v) >= 1 for v in wit.values()), {k: len(v) for k, v in wit.items()}
    assert all(na[q] == 0 and nb[q] == 0 for q, _, _ in wit["empty_empty"])
    assert all(na[q] == 0 and nb[q] == 5 for q, _, _ in wit["empty_full"])
    assert all(na[q] > 0 and nb[q] == 0 for q, _, _ in wit["full_empty"]) and {na[q] for q, _, _ in wit["full_empty"]} >= {1, 64, 1025}
    for q, ka, kb in wit["identical"]:
        assert nb[q] == na[q] and np.array_equal(A.depth[ka:ka + na[q]], B.depth[kb:kb + nb[q]], equal_nan=True)
    assert all(A.depth[ka] < B.depth[kb] and eb[kb] < ea[ka] for _, ka, kb in wit["nested"])
    assert all(ea[ka] == B.depth[kb] and eb[kb] > B.depth[kb] for _, ka, kb in wit["abut"])
    assert all(A.depth[ka] == B.depth[kb] and eb[kb] != ea[ka] for _, ka, kb in wit["equal_start"])
    assert {bool(eb[kb] > ea[ka]) for _, ka, kb in wit["equal_start"]} == {True, False}
    assert any(na[q] == 1025 and nb[q] == 1 and B.depth[kb] < A.depth[ka] and eb[kb] > np.nanmax(ea[ka:ka + 1025]) for q, ka, kb in wit["span"])
    for L in (A, B):                                   # degenerate samples in both lists: length 0, negative, NaN; NaN depth
        assert (L.length == 0).any() and (L.length < 0).any() and np.isnan(L.length).any() and np.isnan(L.depth).any()
    assert (np.isnan(B.depth) & (B.length > 0)).any()
    assert len(A.depth) == 19760 and na[0] == 0 and na[-1] == 0 and tuple(na[:10]) == LENGTHS


# merge ------------------------------------------------------------------------------------------------------------------
def test_merge_bits_on_hand_made_lists(gpu):
    A, (B, _) = hand_a(), hand_b()
    a, b = on_gpu(A, gpu), on_gpu(B, gpu)
    want = hand_merge()
    got = svox.merge_samples(a, b)
    assert_merge_bits(got, want, "merge")
    assert_merge_bits(svox.merge_samples(a, b), want, "the second run")
    m, ia, ib = got
    assert bool((m.row == -1).all()) and len(m) == int(m.offsets[-1]) > len(a)
    assert bool((m.counts <= 2 * (a.counts + b.counts)).all())
    both = int(((ia >= 0) & (ib >= 0)).sum())
    assert both > 1000 and int((ib < 0).sum()) > 1000 and int((ia < 0).sum()) > 100
    assert_merge_bits(svox.merge_samples(b, a), X.merge(B, A), "sides swapped")


def test_merge_identities_as_bit_equality(gpu):
    A = hand()                                          # (no degenerate sample: merge(a, a) emits those once per side)
    a, none = on_gpu(A, gpu), on_gpu(empty_like(A), gpu)
    arange = torch.arange(len(a), device=gpu)
    for first in (True, False):
        m, ia, ib = svox.merge_samples(a, none) if first else svox.merge_samples(none, a)
        for g, w, name in zip(as_lists(m), A._replace(row=np.full(len(a), -1, dtype=np.int32)), R.Lists._fields):
            assert_same_bits(g, w, name)
        mine, other = (ia, ib) if first else (ib, ia)
        assert torch.equal(mine, arange) and bool((other == -1).all())
    m, ia, ib = svox.merge_samples(a, a)
    for g, w, name in zip(as_lists(m), A._replace(row=np.full(len(a), -1, dtype=np.int32)), R.Lists._fields):
        assert_same_bits(g, w, name)
    assert torch.equal(ia, arange) and torch.equal(ib, arange)
    # with degenerate samples: still the list itself against an empty one
    D = hand_a()
    m, ia, ib = svox.merge_samples(on_gpu(D, gpu), none)
    for g, w, name in zip(as_lists(m), D._replace(row=np.full(len(a), -1, dtype=np.int32)), R.Lists._fields):
        assert_same_bits(g, w, name)
    assert torch.equal(ia, arange) and bool((ib == -1).all())


def sub_lists(L, q0, Q):
    lo, hi = int(L.offsets[q0]), int(L.offsets[q0 + Q])
    return R.Lists(L.offsets[q0:q0 + Q + 1] - lo, L.row[lo:hi], (L.ray[lo:hi] - q0).astype(np.int32), L.depth[lo:hi], L.length[lo:hi])


@pytest.mark.parametrize("Q,q0", [(1, 29), (1, 0), (65, 20)])
def test_small_batches(gpu, Q, q0):
    A, B = sub_lists(hand_a(), q0, Q), sub_lists(hand_b()[0], q0, Q)
    none = empty_like(A)
    for x, y in ((A, B), (A, none), (none, B), (none, none)):
        got = svox.merge_samples(on_gpu(x, gpu), on_gpu(y, gpu))
        assert_merge_bits(got, X.merge(x, y), f"Q={Q}")
        assert got[0].Q == Q and got[0].offsets.shape == (Q + 1,)
    for L in (A, none):
        s = on_gpu(L, gpu)
        fine, index = s.split(0.02)
        want = X.split(L.offsets, L.ray, L.row, L.depth, L.length, max_length=0.02)
        for g, w in zip((fine.offsets, fine.ray, fine.row, fine.depth, fine.length, index), want):
            assert_same_bits(g, w, f"split Q={Q}")
        assert fine.Q == Q and index.dtype == torch.int64


# split ------------------------------------------------------------------------------------------------------------------
def hand_pieces():
    T = len(hand_a().depth)
    pieces = np.array([0, -5, 1, 3, 2, 1, -(1 << 31), 7], dtype=np.int64)[np.arange(T) % 8].astype(np.int32)
    pieces[::997] = 1000
    return pieces


@pytest.mark.parametrize("how", ["inf", "half", "max_pieces", "pieces", "ones"])
def test_split_bits_on_hand_made_lists(gpu, how):
    L = hand_a()
    T = len(L.depth)
    s = on_gpu(L, gpu)
    half = float(np.nanmedian(L.length))
    kw = dict(inf=dict(max_length=float("inf")), half=dict(max_length=half), max_pieces=dict(max_length=1e-4, max_pieces=16),
              pieces=dict(pieces=hand_pieces()), ones=dict(pieces=np.ones(T, dtype=np.int32)))[how]
    want = X.split(L.offsets, L.ray, L.row, L.depth, L.length, **kw)
    if "pieces" in kw:
        kw = dict(kw, pieces=torch.from_numpy(kw["pieces"]).to(gpu))
    fine, index = s.split(**kw)
    for g, w, name in zip((fine.offsets, fine.ray, fine.row, fine.depth, fine.length, index), want, ("offsets", "ray", "row", "depth", "length", "index")):
        assert_same_bits(g, w, f"{how} {name}")
    assert index.dtype == torch.int64 and not hasattr(fine, "_row_plans")
    m = np.bincount(want[5], minlength=T)
    good = L.length > 0
    if how in ("inf", "ones"):                          # the old lists array for array
        for g, w, name in zip(as_lists(fine), L, R.Lists._fields):
            assert_same_bits(g, w, name)
        assert torch.equal(index, torch.arange(T, device=gpu))
    elif how == "half":
        assert 0.4 * T < (m > 1).sum() < 0.6 * T and m.max() == 2
    elif how == "max_pieces":
        assert (m[good] == 16).all() and (m[~good] == 1).all() and len(fine) == 16 * good.sum() + (~good).sum()
    else:
        assert set(np.unique(m)) == {1, 2, 3, 7, 1000}
    # offsets' by the select rule: empty rays at the start, inside and at the end stay empty, the last entry is T'
    off = fine.offsets.cpu().numpy()
    assert off[0] == 0 and off[-1] == len(fine) and off[1] == 0 and off[-2] == off[-1]
    np.testing.assert_array_equal(np.diff(off) == 0, np.diff(L.offsets) == 0)
    assert_same_bits(s.split(**kw)[0].depth, want[3], "the second run")


def test_overflow_is_refused_after_the_count(gpu):
    """Three samples of 2^30 pieces each: the 64-bit total 3 * 2^30 >= 2^31 is read back and refused; nothing is emitted."""
    s = svox.RaySamples(torch.tensor([0, 3], device=gpu), torch.zeros(3, dtype=torch.int32, device=gpu), torch.zeros(3, dtype=torch.int32, device=gpu),
                        torch.zeros(3, device=gpu), torch.ones(3, device=gpu))
    before = torch.cuda.memory_allocated(gpu)
    with pytest.raises(RuntimeError, match=r"would hold 3221225472 samples; a list holds fewer than 2\^31"):
        s.split(pieces=torch.full((3,), 1 << 30, dtype=torch.int32, device=gpu), max_pieces=1 << 30)
    assert torch.cuda.memory_allocated(gpu) - before < (1 << 20)
    fine, index = s.split(pieces=torch.full((3,), 1 << 30, dtype=torch.int32, device=gpu), max_pieces=1 << 9)
    assert len(fine) == 3 << 9 and index.tolist() == sorted([0, 1, 2] * (1 << 9))


# placement --------------------------------------------------------------------------------------------------------------
def shifted(t):
    """The values of t one element into a 16-byte aligned buffer: 4 bytes off the boundary, 8 for int64."""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()]
    view.copy_(t)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view


def shifted_samples(L, gpu):
    s = on_gpu(L, gpu)
    return svox.RaySamples(*(shifted(x) for x in (s.offsets, s.ray, s.row, s.depth, s.length)))


def test_inputs_that_start_anywhere(gpu):
    A, (B, _) = hand_a(), hand_b()
    assert_merge_bits(svox.merge_samples(shifted_samples(A, gpu), shifted_samples(B, gpu)), hand_merge(), "merge, shifted")
    pieces = hand_pieces()
    for kw in (dict(max_length=0.02), dict(pieces=pieces)):
        want = X.split(A.offsets, A.ray, A.row, A.depth, A.length, **kw)
        if "pieces" in kw:
            kw = dict(pieces=shifted(torch.from_numpy(pieces).to(gpu)))
        fine, index = shifted_samples(A, gpu).split(**kw)
        for g, w in zip((fine.offsets, fine.ray, fine.row, fine.depth, fine.length, index), want):
            assert_same_bits(g, w, "split, shifted")


# real lists -------------------------------------------------------------------------------------------------------------
def two_trees(gpu):
    """The 64 x 64 rays of case d5_rgba4 through its own tree (A) and through the tree of d5_sh4_world (B: another radius
    and centre, delta_scale != 1): (rays, tree A, tree B, lists A, lists B), the lists with min_sigma = 0."""
    ca, _, rays, _ = built("d5_rgba4")
    cb, otb, _, optb = built("d5_sh4_world")
    if "world" not in _MADE:
        _MADE["world"] = R.lists(otb, rays, optb, 0.0)
    return ca.rays_gpu(gpu), ca.tree(gpu), cb.tree(gpu), lists_of("d5_rgba4", 0.0), _MADE["world"]


def real_merge():
    if "real" not in _MADE:
        _MADE["real"] = X.merge(lists_of("d5_rgba4", 0.0), _MADE["world"])
    return _MADE["real"]


def test_real_lists_merge_bits(gpu):
    rays, ta, tb, LA, LB = two_trees(gpu)
    sa = svox.VolumeRenderer(ta).ray_samples(rays, min_sigma=0.0)
    sb = svox.VolumeRenderer(tb).ray_samples(rays, min_sigma=0.0)
    for g, w in zip(as_lists(sb), LB):
        assert_same_bits(g, w, "the rays of one case through the tree of the other")
    assert len(sa) > 1000 and len(sb) > 1000
    got = svox.merge_samples(sa, sb)
    assert_merge_bits(got, real_merge(), "real lists")
    assert int(((got[1] >= 0) & (got[2] >= 0)).sum()) > 1000                    # the two media overlap


def test_an_empty_second_tree_leaves_opacity_render(gpu):
    rays, ta, tb, _, _ = two_trees(gpu)
    ra, rb = svox.VolumeRenderer(ta), svox.VolumeRenderer(tb)
    dead = tb.features.detach().clone()
    dead[:, -1] = -1.0
    with torch.no_grad():
        sa = ra.ray_samples(rays, min_sigma=0.0)
        sb = rb.ray_samples(rays, features=dead, min_sigma=0.0)
        assert len(sb) == 0
        m, ia, ib = svox.merge_samples(sa, sb)
        sigma = svox.take_samples(ta.features[sa.row.long(), -1], ia) + svox.take_samples(dead[sb.row.long(), -1], ib)
        _, alpha = svox.sample_weights(m, sigma)
        opacity = ra.opacity_render(ta.features, rays)
    assert_same_bits(alpha[:, None], opacity)
    assert int((alpha > 0).sum()) > 500


def test_two_live_trees_against_the_float64_product(gpu):
    """alpha of the merged lists with sigma_a + sigma_b against 1 - (1 - alpha_a)(1 - alpha_b) in float64 from the two lists
    apart: within cut_restate's bound (the host test holds the restatement to half of it)."""
    rays, ta, tb, LA, LB = two_trees(gpu)
    with torch.no_grad():
        sa = svox.VolumeRenderer(ta).ray_samples(rays, min_sigma=0.0)
        sb = svox.VolumeRenderer(tb).ray_samples(rays, min_sigma=0.0)
        siga, sigb = ta.features[sa.row.long(), -1], tb.features[sb.row.long(), -1]
        m, ia, ib = svox.merge_samples(sa, sb)
        sigma = svox.take_samples(siga, ia) + svox.take_samples(sigb, ib)
        _, alpha = svox.sample_weights(m, sigma)
    na, nb = siga.cpu().numpy(), sigb.cpu().numpy()
    t_a = 1.0 - R.weights(LA.length, na.astype(np.float64), LA.offsets, torch.float64)[1].numpy()
    t_b = 1.0 - R.weights(LB.length, nb.astype(np.float64), LB.offsets, torch.float64)[1].numpy()
    want = 1.0 - t_a * t_b
    bound = X.alpha_bound(as_lists(m), sigma.cpu().numpy(), LA, na, LB, nb)
    ratio = np.abs(alpha.cpu().numpy().astype(np.float64) - want) / bound
    print(f"two live trees: worst |alpha - alpha64| / bound = {float(ratio.max()):.3f}")
    assert (ratio <= 1.0).all(), float(ratio.max())
    assert ((t_a < 1) & (t_b < 1)).sum() > 500 and (want > 0.5).sum() > 100


def test_split_alpha_against_the_lists_it_came_from(gpu):
    """Not bit-equal: exp(-(length * sigma)) is one rounded exponential, the product of m rounded exponentials of
    -(step * sigma) another number.  Within cut_restate's bound for the pair."""
    rays, ta, _, LA, _ = two_trees(gpu)
    with torch.no_grad():
        s = svox.VolumeRenderer(ta).ray_samples(rays, min_sigma=0.0)
        sig = ta.features[s.row.long(), -1]
        fine, index = s.split(float(np.median(LA.length)))
        _, coarse = svox.sample_weights(s, sig)
        _, alpha = svox.sample_weights(fine, sig[index])
    assert 1.3 * len(s) < len(fine) < 2.5 * len(s)
    bound = X.split_alpha_bound(LA, sig.cpu().numpy(), fine.offsets.cpu().numpy(), sig[index].cpu().numpy())
    diff = np.abs(alpha.cpu().numpy().astype(np.float64) - coarse.cpu().numpy().astype(np.float64))
    print(f"split alpha: worst |alpha(split) - alpha| / bound = {float((diff / bound).max()):.3f}")
    assert (diff <= bound).all() and (diff > 0).any()


def test_composed_example_end_to_end(gpu):
    """Two media along shared rays: sigma = sigma_a + sigma_b, colour weighted by density, through shade_samples,
    sample_weights and accumulate.  Gradients reach both feature tables, finite, and a second run gives the same bits."""
    rays, ta, tb, _, _ = two_trees(gpu)
    ra, rb = svox.VolumeRenderer(ta), svox.VolumeRenderer(tb)
    g = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, (rays.origins.shape[0], 3)).astype(F)).to(gpu)
    tiny = 1e-20

    def run():
        fa = ta.features.detach().clone().requires_grad_(True)
        fb = tb.features.detach().clone().requires_grad_(True)
        sa, sb = ra.ray_samples(rays, min_sigma=0.0), rb.ray_samples(rays, min_sigma=0.0)
        rgb_a, sig_a = ra.shade_samples(sa, fa, rays)
        rgb_b, sig_b = rb.shade_samples(sb, fb, rays)
        m, ia, ib = svox.merge_samples(sa, sb)
        s_a, s_b = svox.take_samples(sig_a, ia), svox.take_samples(sig_b, ib)
        sigma = s_a + s_b
        rgb = (s_a[:, None] * svox.take_samples(rgb_a, ia) + s_b[:, None] * svox.take_samples(rgb_b, ib)) / sigma.clamp_min(tiny)[:, None]
        w, alpha = svox.sample_weights(m, sigma)
        out = svox.accumulate(m, w, rgb)
        ((out * g).sum() + alpha.sum()).backward()
        return out.detach(), alpha.detach(), fa.grad, fb.grad

    first, second = run(), run()
    for x, y, name in zip(first, second, ("out", "alpha", "grad A", "grad B")):
        assert bool(torch.isfinite(x).all()), name
        assert_same_bits(x, y, name)
    out, alpha, ga, gb = first
    assert out.shape == (rays.origins.shape[0], 3) and int((alpha > 0).sum()) > 500
    assert int((ga != 0).sum()) > 500 and int((gb != 0).sum()) > 500
    assert int((ga[:, -1] != 0).sum()) > 100 and int((gb[:, -1] != 0).sum()) > 100
